"""Time the fused MIND routing against the layered path it replaces, on the GPU (fails
without one), with the fused SASRec pair at the same shape as a second yardstick.

Shape: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded),
D = 64, K = 4 interests, R = 3 routing iterations, a 63,002-row fp32 item table,
route_weight at its initial scale N(0, 1/sqrt(D)).

Paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions:
  fused    dense.mind_route -> mrec_mind_fwd (+ mrec_mind_bwd + mrec_sasrec_wgrad);
  layered  the same arithmetic as stock torch ops (cpu_path.mind_route with the kernel's
           bf16 rounding points): a GEMM, then per iteration a softmax, a mask, two
           batched matmuls over [B, K, L] and the squash;
  sasrec   dense.sasrec_encode -> mrec_sasrec_fwd / _bwd, one layer (routing measurements
           only).
Measurements:
  route_fwd      the routing alone on gathered rows, no autograd;
  route_fwd_bwd  routing forward + backward (the rows' gradient and d route_weight);
  train_step     MIND.train_step with ``softmax_shared`` over 4096 shared negatives, SGD;
  launch_fwd / launch_bwd  mrec_mind_fwd and mrec_mind_bwd alone on preallocated buffers,
           with each launch's algorithmic bytes and their time at the stream-copy rate of
           profiles/ceilings.json.

Writes <out>/bench_mind.json (default profiles/mind).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import _mrec, dense  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity  # noqa: E402
from pytorchrec_amd.loss import SharedNegativeLoss  # noqa: E402
from pytorchrec_amd.model import MIND, SASRec  # noqa: E402
from pytorchrec_amd.sampling import NegativeSampler  # noqa: E402

B, L, D, K, R, ITEMS, SHARED = 4096, 50, 64, 4, 3, 63002, 4096
WARMUP, REPS = 5, 30


def build(cls, dev, **kw):
    m = cls(CategoricalColumnWithIdentity(ITEMS, "iid"), CategoricalColumnWithIdentity(L + 1, "his_len"),
            CategoricalColumnWithIdentity(ITEMS, "his"), CategoricalColumnWithIdentity(2, "label"),
            emb_size=D, max_his_len=L, device=dev, random_seed=1, **kw)
    if cls is SASRec:
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for name in ("Q", "K", "W1", "W2"):
                w = getattr(m, name).weight
                w.copy_((D ** -0.5 * torch.randn(w.shape, generator=g)).to(dev))
    m.i_embeddings.check_ids = False
    return m


def draw(gen, dev):
    lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev)
    his = torch.randint(1, ITEMS, (B, L), generator=gen, device=dev)
    his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
    return {"his": his, "his_len": lens, "iid": torch.randint(1, ITEMS, (B,), generator=gen, device=dev),
            "uid": torch.arange(B, device=dev)}


def launch_args(m, rows, batch, dev):
    """A mrec_mind_args block on preallocated buffers (kept alive by the second value)."""
    his, lens = batch["his"].to(torch.int32).contiguous(), batch["his_len"].to(torch.int32).contiguous()
    rows2 = rows.reshape(B * L, D).contiguous()
    parts = int(_mrec.lib().mrec_mind_parts(B))
    bufs = {"u": torch.empty(B, K, D, device=dev), "w": torch.empty(B, K, L, dtype=torch.bfloat16, device=dev),
            "z": torch.empty(B, K, D, device=dev), "du": torch.randn(B, K, D, device=dev),
            "dx": torch.empty(B * L, D, dtype=torch.bfloat16, device=dev),
            "part": torch.empty(parts, D * D, device=dev)}
    s, init = m.route_weight.detach().contiguous(), m.route_init.contiguous()
    a = _mrec.MindArgs(rows2.data_ptr(), D, his.data_ptr(), L, lens.data_ptr(), s.data_ptr(), D,
                       init.data_ptr(), init.stride(0), B, L, D, K, R, 0, bufs["u"].data_ptr(),
                       bufs["w"].data_ptr(), bufs["z"].data_ptr(), bufs["du"].data_ptr(),
                       bufs["dx"].data_ptr(), D, bufs["part"].data_ptr(), parts)
    return a, (his, lens, rows2, bufs, s, init), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mind"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mind.py needs a GPU")
    dev = torch.device("cuda")
    mind = build(MIND, dev, num_interests=K, routing_iters=R)
    sas = build(SASRec, dev, num_layers=1)
    gen = torch.Generator(device=dev).manual_seed(3)
    first = draw(gen, dev)
    sampler = NegativeSampler(first["uid"], first["iid"], 1, ITEMS, seed=5, device=dev)
    mind.compile(torch.optim.SGD(mind.get_parameters(), lr=0.01), SharedNegativeLoss("softmax"), [], dev)
    mind.set_shared_negatives(sampler, SHARED)
    du = torch.randn(B, K, D, generator=gen, device=dev)
    dv = torch.randn(B, D, generator=gen, device=dev)
    encoders = {"fused": (mind, dense.mind_route, du), "layered": (mind, dense.mind_route, du),
                "sasrec": (sas, dense.sasrec_encode, dv)}
    times, live, parts = {}, [], 0
    order_rng = np.random.default_rng(4)
    st = _mrec.stream_handle()

    def timed(key, rep, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.setdefault(key, []).append(e0.elapsed_time(e1) * 1e3)

    for rep in range(WARMUP + REPS):
        batch = draw(gen, dev)
        live.append(int(batch["his_len"].sum()))
        rows = (0.3 * torch.randn(B, L, D, generator=gen, device=dev)).to(torch.bfloat16)

        def route_fwd(m, fn, g):
            with torch.no_grad():
                fn(rows, batch["his"], batch["his_len"], m.eval())

        def route_fwd_bwd(m, fn, g):
            x = rows.detach().requires_grad_()
            fn(x, batch["his"], batch["his_len"], m.eval()).backward(g)

        def train_step(m, fn, g):
            m.train_step(batch)

        for name, step in (("route_fwd", route_fwd), ("route_fwd_bwd", route_fwd_bwd),
                           ("train_step", train_step)):
            for path in order_rng.permutation(list(encoders)):
                if name == "train_step" and path == "sasrec":
                    continue
                dense.MIND_FUSED = path != "layered"
                m, fn, g = encoders[path]
                for p in m.parameters():
                    p.grad = None
                timed((name, path), rep, lambda: step(m, fn, g))
        a, keep, parts = launch_args(mind, rows, batch, dev)
        timed(("launch_fwd", "fused"), rep, lambda: _mrec.call("mrec_mind_fwd", ctypes.byref(a), st))
        timed(("launch_bwd", "fused"), rep, lambda: _mrec.call("mrec_mind_bwd", ctypes.byref(a), st))
    dense.MIND_FUSED = True
    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy_gbs = json.load(f)["stream_copy"]["GB/s"]
    live_mean = float(np.mean(live))
    small = B * L * 4 + B * K * L * 2  # his, w
    fwd_bytes = int(live_mean * D * 2 + small + 2 * B * K * D * 4)
    bwd_bytes = int(live_mean * D * 2 + B * L * D * 2 + small + 2 * B * K * D * 4 + parts * D * D * 4)
    res = {"B": B, "L": L, "D": D, "K": K, "iters": R, "items": ITEMS, "shared_negatives": SHARED,
           "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "live_positions_mean": live_mean,
           "workgroups": parts, "stream_copy_GB/s": copy_gbs, "measurements": {}}

    def stats(key):
        t = np.array(times[key])
        return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
                "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90))}

    for name in ("route_fwd", "route_fwd_bwd", "train_step"):
        row = {path: stats((name, path)) for path in encoders if (name, path) in times}
        row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
        if "sasrec" in row:
            row["fused_over_sasrec_median"] = row["fused"]["median_us"] / row["sasrec"]["median_us"]
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(f"{p} {row[p]['median_us']:.1f} us" for p in encoders if p in row))
    for name, nbytes in (("launch_fwd", fwd_bytes), ("launch_bwd", bwd_bytes)):
        row = stats((name, "fused"))
        row["algorithmic_bytes"] = nbytes
        row["bytes_at_stream_copy_us"] = nbytes / (copy_gbs * 1e3)
        row["share_of_stream_copy_ceiling"] = row["bytes_at_stream_copy_us"] / row["median_us"]
        res["measurements"][name] = row
        print(f"{name}: {row['median_us']:.1f} us, {row['share_of_stream_copy_ceiling']:.2f} of the copy ceiling")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_mind.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
