"""Time the fused SR-GNN encoder forward against the layered path it replaces, on the GPU
(fails without one), with the fused GRU4Rec forward at the same shape as a second yardstick.

Shape: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded), D = 64,
gnn_steps 1 and 2, ids from a 63,002-row table (hardly a repeat) and from a 200-id vocabulary
(repeats in most sessions).

Paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions with p10 - p90:
  fused    dense.srgnn_encode without autograd -> mrec_srgnn_fwd;
  layered  the same arithmetic as stock torch ops (cpu_path.srgnn_encode with the kernel's
           bf16 rounding points), graph construction in tensor ops included;
  gru      dense.gru_encode -> mrec_gru_fwd, E = H = 64.
Measurements:
  encode_fwd     the encoder alone on gathered rows, no autograd;
  launch_fwd     mrec_srgnn_fwd alone on preallocated buffers, with its algorithmic bytes
                 (the rows at representative positions, his, v) and their time at the
                 stream-copy rate of profiles/ceilings.json.
  encode_fwd_bwd the same with autograd: forward + backward (SR-GNN fused and layered, GRU4Rec);
  train_step     SRGNN.train_step with ``softmax_shared`` over 4096 shared negatives, SGD
                 (the large vocabulary only);
  launch_bwd     mrec_srgnn_bwd alone, with its algorithmic bytes.

Writes <out>/bench_srgnn.json (default profiles/srgnn).
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
from pytorchrec_amd import _mrec, cpu_path, dense  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity  # noqa: E402
from pytorchrec_amd.loss import SharedNegativeLoss  # noqa: E402
from pytorchrec_amd.model import GRU4Rec, SRGNN  # noqa: E402
from pytorchrec_amd.sampling import NegativeSampler  # noqa: E402

B, L, D, ITEMS = 4096, 50, 64, 63002
WARMUP, REPS = 5, 30


def build(cls, dev, **kw):
    return cls(CategoricalColumnWithIdentity(ITEMS, "iid"), CategoricalColumnWithIdentity(L + 1, "his_len"),
               CategoricalColumnWithIdentity(ITEMS, "his"), CategoricalColumnWithIdentity(2, "label"),
               emb_size=D, device=dev, random_seed=1, **kw).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srgnn"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_srgnn.py needs a GPU")
    dev = torch.device("cuda")
    models = {1: build(SRGNN, dev, max_his_len=L, gnn_steps=1), 2: build(SRGNN, dev, max_his_len=L, gnn_steps=2)}
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
    times, nodes = {}, {}

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
        for vocab in (ITEMS - 1, 200):
            his = torch.randint(1, vocab + 1, (B, L), generator=gen, device=dev)
            his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
            nodes.setdefault(vocab, []).append(int(cpu_path.srgnn_graph(his)[2].sum()))
            for steps, m in models.items():
                for path in rng.permutation(["fused", "layered", "gru"]):
                    dense.SRGNN_FUSED = path != "layered"
                    with torch.no_grad():
                        if path == "gru":
                            fn = lambda: dense.gru_encode(rows, lens, gru)  # noqa: E731
                        else:
                            fn = lambda: dense.srgnn_encode(rows, his, lens, m)  # noqa: E731
                        timed(("encode_fwd", vocab, steps, path), rep, fn)
                    x = rows.detach().requires_grad_()
                    if path == "gru":
                        fb = lambda: dense.gru_encode(x, lens, gru).backward(dv)  # noqa: E731
                    else:
                        fb = lambda: dense.srgnn_encode(x, his, lens, m).backward(dv)  # noqa: E731
                    for q in list(m.parameters()) + list(gru.parameters()):
                        q.grad = None
                    timed(("encode_fwd_bwd", vocab, steps, path), rep, fb)
                batch = {"his": his, "his_len": lens, "uid": uid,
                         "iid": torch.randint(1, ITEMS, (B,), generator=gen, device=dev)}
                for path in rng.permutation(["fused", "layered"] if vocab != 200 else []):
                    dense.SRGNN_FUSED = path != "layered"
                    timed(("train_step", vocab, steps, path), rep, lambda: m.train_step(batch))
                dense.SRGNN_FUSED = True
                his32 = his.to(torch.int32).contiguous()
                rows2 = rows.reshape(B * L, D)
                ps = [p.detach().contiguous() for p in
                      (m.W_ein, m.W_eout, m.W_ih, m.W_hh, m.W1, m.W2, m.Wt, m.b_ein, m.b_eout, m.b_iah,
                       m.b_oah, m.b_ih, m.b_hh, m.c1, m.q, m.bt)]
                v = torch.empty(B, D, device=dev)
                a = _mrec.SrgnnArgs(rows2.data_ptr(), D, his32.data_ptr(), L, *(p.data_ptr() for p in ps),
                                    B, L, D, steps, v.data_ptr(), None, None, None, 0, None, 0)
                parts = int(_mrec.lib().mrec_srgnn_parts(B))
                hs = torch.empty(steps, B, L, D, dtype=torch.bfloat16, device=dev)
                dx = torch.empty(B * L, D, dtype=torch.bfloat16, device=dev)
                part = torch.empty(parts, 15 * D * D + 13 * D, device=dev)
                a.hs, a.dv, a.d_rows, a.ld_drows = hs.data_ptr(), dv.data_ptr(), dx.data_ptr(), D
                a.part, a.parts = part.data_ptr(), parts
                timed(("launch_fwd", vocab, steps, "fused"), rep,
                      lambda: _mrec.call("mrec_srgnn_fwd", ctypes.byref(a), st))
                timed(("launch_bwd", vocab, steps, "fused"), rep,
                      lambda: _mrec.call("mrec_srgnn_bwd", ctypes.byref(a), st))
    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy_gbs = json.load(f)["stream_copy"]["GB/s"]

    def stats(key):
        t = np.array(times[key])
        return {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                "p90_us": float(np.percentile(t, 90))}

    res = {"B": B, "L": L, "D": D, "items": ITEMS, "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "stream_copy_GB/s": copy_gbs,
           "measurements": []}
    for vocab in (ITEMS - 1, 200):
        for steps in models:
            row = {"vocabulary": vocab, "gnn_steps": steps, "nodes_per_batch_mean": float(np.mean(nodes[vocab]))}
            for path in ("fused", "layered", "gru"):
                row[path] = stats(("encode_fwd", vocab, steps, path))
            row["fwd_bwd"] = {path: stats(("encode_fwd_bwd", vocab, steps, path)) for path in ("fused", "layered", "gru")}
            row["fwd_bwd"]["speedup_median"] = row["fwd_bwd"]["layered"]["median_us"] / row["fwd_bwd"]["fused"]["median_us"]
            if ("train_step", vocab, steps, "fused") in times:
                row["train_step"] = {path: stats(("train_step", vocab, steps, path)) for path in ("fused", "layered")}
            lb = stats(("launch_bwd", vocab, steps, "fused"))
            lb["algorithmic_bytes"] = int(row["nodes_per_batch_mean"] * D * 2 + B * L * 4 + B * D * 4 + B * L * D * 2 * (steps + 1)
                                          + int(_mrec.lib().mrec_srgnn_parts(B)) * (15 * D * D + 13 * D) * 4)
            lb["bytes_at_stream_copy_us"] = lb["algorithmic_bytes"] / (copy_gbs * 1e3)
            row["launch_bwd"] = lb
            row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
            row["fused_over_gru_median"] = row["fused"]["median_us"] / row["gru"]["median_us"]
            launch = stats(("launch_fwd", vocab, steps, "fused"))
            launch["algorithmic_bytes"] = int(row["nodes_per_batch_mean"] * D * 2 + B * L * D * 2 * steps + B * L * 4 + B * D * 4)
            launch["bytes_at_stream_copy_us"] = launch["algorithmic_bytes"] / (copy_gbs * 1e3)
            launch["share_of_stream_copy_ceiling"] = launch["bytes_at_stream_copy_us"] / launch["median_us"]
            row["launch_fwd"] = launch
            res["measurements"].append(row)
            print(f"vocab {vocab} steps {steps}: fused {row['fused']['median_us']:.1f} us, layered "
                  f"{row['layered']['median_us']:.1f} us, gru {row['gru']['median_us']:.1f} us, launch "
                  f"{launch['median_us']:.1f} us, bwd launch {lb['median_us']:.1f} us; fwd+bwd fused "
                  f"{row['fwd_bwd']['fused']['median_us']:.1f} layered {row['fwd_bwd']['layered']['median_us']:.1f} gru "
                  f"{row['fwd_bwd']['gru']['median_us']:.1f}; train " + str({k: round(v['median_us'], 1) for k, v in row.get('train_step', {}).items()}))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_srgnn.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
