"""Time the fused Caser encoder against the layered path it replaces, on the GPU (fails without
one), with the fused GRU4Rec pair at the same shape as a second yardstick.

Shape: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded), D = 64,
ids from a 63,002-row table; two configurations: heights 1..4, n_h 16, n_v 4 and heights
(3, 5), n_h 32, n_v 8 (the element budget's edge).

Paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions with p10 - p90:
  fused    dense.caser_encode -> mrec_caser_fwd / _bwd (+ the partial sum and the dW1 GEMM);
  layered  the same arithmetic as stock torch ops (cpu_path.caser_encode with the kernel's
           bf16 rounding points);
  gru      dense.gru_encode -> mrec_gru_fwd / _bwd, E = H = 64.
Measurements:
  encode_fwd      the encoder alone on gathered rows, no autograd;
  encode_fwd_bwd  the same with autograd: forward + backward;
  train_step      Caser.train_step with ``softmax_shared`` over 4096 shared negatives, SGD;
  launch_fwd / launch_bwd  mrec_caser_fwd / _bwd alone on preallocated buffers.

Writes <out>/bench_caser.json (default profiles/caser).
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
from pytorchrec_amd.model import Caser, GRU4Rec  # noqa: E402
from pytorchrec_amd.sampling import NegativeSampler  # noqa: E402

B, L, D, ITEMS = 4096, 50, 64, 63002
CONFIGS = {"h1234_nh16_nv4": dict(conv_heights="1,2,3,4", n_h=16, n_v=4),
           "h35_nh32_nv8": dict(conv_heights="3,5", n_h=32, n_v=8)}
WARMUP, REPS = 5, 30


def build(cls, dev, **kw):
    return cls(CategoricalColumnWithIdentity(ITEMS, "iid"), CategoricalColumnWithIdentity(L + 1, "his_len"),
               CategoricalColumnWithIdentity(ITEMS, "his"), CategoricalColumnWithIdentity(2, "label"),
               emb_size=D, device=dev, random_seed=1, **kw).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caser"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_caser.py needs a GPU")
    dev = torch.device("cuda")
    models = {k: build(Caser, dev, max_his_len=L, **kw) for k, kw in CONFIGS.items()}
    gru = build(GRU4Rec, dev, hidden_size=D)
    uid = torch.arange(B, device=dev)
    sampler = NegativeSampler(uid, torch.randint(1, ITEMS, (B,), device=dev), 1, ITEMS, seed=5, device=dev)
    for m in models.values():
        m.i_embeddings.check_ids = False
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), SharedNegativeLoss("softmax"), [], dev)
        m.set_shared_negatives(sampler, 4096)
    dv = torch.randn(B, D, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    rng = np.random.default_rng(4)
    st = _mrec.stream_handle()
    times = {}

    def timed(key, rep, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.setdefault(key, []).append(e0.elapsed_time(e1) * 1e3)

    for rep in range(WARMUP + REPS):
        rows = (0.3 * torch.randn(B, L, D, generator=gen, device=dev)).to(torch.bfloat16)
        lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev)
        his = torch.randint(1, ITEMS, (B, L), generator=gen, device=dev)
        his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
        for cfg, m in models.items():
            for path in rng.permutation(["fused", "layered", "gru"]):
                dense.CASER_FUSED = path != "layered"
                with torch.no_grad():
                    if path == "gru":
                        fn = lambda: dense.gru_encode(rows, lens, gru)  # noqa: E731
                    else:
                        fn = lambda: dense.caser_encode(rows, his, lens, m)  # noqa: E731
                    timed(("encode_fwd", cfg, path), rep, fn)
                x = rows.detach().requires_grad_()
                if path == "gru":
                    fb = lambda: dense.gru_encode(x, lens, gru).backward(dv)  # noqa: E731
                else:
                    fb = lambda: dense.caser_encode(x, his, lens, m).backward(dv)  # noqa: E731
                for q in list(m.parameters()) + list(gru.parameters()):
                    q.grad = None
                timed(("encode_fwd_bwd", cfg, path), rep, fb)
            batch = {"his": his, "his_len": lens, "uid": uid,
                     "iid": torch.randint(1, ITEMS, (B,), generator=gen, device=dev)}
            for path in rng.permutation(["fused", "layered"]):
                dense.CASER_FUSED = path != "layered"
                timed(("train_step", cfg, path), rep, lambda: m.train_step(batch))
            dense.CASER_FUSED = True
            # the launches alone: the argument block of one recorded forward, run again
            x = rows.detach().requires_grad_()
            v = dense.caser_encode(x, his, lens, m)
            a, keep = v.grad_fn.args, v.grad_fn.keep
            nH, parts = int(a.n_heights), int(_mrec.lib().mrec_caser_parts(B))
            P = int(_mrec.lib().mrec_caser_param_count(D, L, nH, a.heights, int(a.n_h), int(a.n_v)))
            dpre = torch.empty(B, D, dtype=torch.bfloat16, device=dev)
            dx = torch.empty(B * L, D, dtype=torch.bfloat16, device=dev)
            part = torch.empty(parts, P, device=dev)
            a.dv, a.dpre, a.d_rows, a.ld_drows = dv.data_ptr(), dpre.data_ptr(), dx.data_ptr(), D
            a.part, a.parts = part.data_ptr(), parts
            timed(("launch_fwd", cfg, "fused"), rep, lambda: _mrec.call("mrec_caser_fwd", ctypes.byref(a), st))
            timed(("launch_bwd", cfg, "fused"), rep, lambda: _mrec.call("mrec_caser_bwd", ctypes.byref(a), st))
            del v, keep

    def stats(key):
        t = np.array(times[key])
        return {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                "p90_us": float(np.percentile(t, 90))}

    res = {"B": B, "L": L, "D": D, "items": ITEMS, "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "measurements": []}
    for cfg in models:
        row = {"config": cfg, **CONFIGS[cfg]}
        for what in ("encode_fwd", "encode_fwd_bwd"):
            row[what] = {path: stats((what, cfg, path)) for path in ("fused", "layered", "gru")}
            row[what]["speedup_median"] = row[what]["layered"]["median_us"] / row[what]["fused"]["median_us"]
        row["train_step"] = {path: stats(("train_step", cfg, path)) for path in ("fused", "layered")}
        row["launch_fwd"], row["launch_bwd"] = stats(("launch_fwd", cfg, "fused")), stats(("launch_bwd", cfg, "fused"))
        res["measurements"].append(row)
        print(cfg, json.dumps({k: ({p: round(s["median_us"], 1) for p, s in r.items() if isinstance(s, dict)}
                                   if "median_us" not in r else round(r["median_us"], 1))
                               for k, r in row.items() if isinstance(r, dict)}))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_caser.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
