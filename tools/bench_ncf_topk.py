"""Time NCF's fused full-catalogue top-K (mrec_ncf_topk behind ``NCF.recommend``) against
``IModel.recommend_by_forward``, the path it replaces, on the GPU (fails without one).

Shape: emb_size 64, layers [128, 64, 32], k = 100, B = 4096 users, catalogues of 10^5
items (``--items`` for others), fp32 and bf16 banks; table rows 0.5 N(0, 1), dense
tensors 0.3 N(0, 1).

Paths, in one process on the same model and users, alternating in a fresh random order,
by device events after warm-up, the median over the repetitions:
  fused          NCF.recommend -> retrieval.ncf_topk -> mrec_ncf_topk (scan + merge launches;
                 neither a gathered row nor a [B, items] score reaches memory);
  forward@C      recommend_by_forward at chunk C in {1024 (its default), 4096, 16384}: per
                 chunk one bank gather of [B, C] rows of 4 E bf16, one mrec_ncf_fwd over
                 them, one sort-merge with the running list.
Before timing, ``recommend`` of the first 64 users is compared with ``recommend_by_forward``:
scores within 3e-2 of the largest score, ids equal wherever the neighbouring forward scores
are further apart than twice that.

Writes <out>/bench_ncf_topk.json (default profiles/ncf_topk) with, per shape, every median,
the ratio forward@default / fused and forward@best / fused, the split count, and the
algorithmic work of both paths: MACs (the MLP per pair, the MF term, and for the fused path
the item half of layer 0 once per item and user tile) and bytes (the item tables once per
user tile against the gathered rows written and read once per pair).  The fused path's share
of the bf16 MFMA peak is its MFMA MACs over its median time over 1.25e15 MAC/s (the 2.5 PF
dense figure).  ``--rehearse`` runs the torch restatement against the model's forward at a
toy size on the CPU to check the script itself; it times nothing and writes nothing.
``--trace-run`` is the program of a kernel-trace run (``rocprofv3 --kernel-trace --stats --
python tools/bench_ncf_topk.py --trace-run``), whose per-kernel statistics are kept as
profiles/ncf_topk/kernel_stats.csv.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import retrieval  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C  # noqa: E402
from pytorchrec_amd.model import NCF  # noqa: E402
from pytorchrec_amd.model.IModel import IModel  # noqa: E402

B, E, LAYERS, K = 4096, 64, (128, 64, 32), 100
USERS = 8192
DTYPES = (torch.bfloat16, torch.float32)
CHUNKS = (1024, 4096, 16384)
WARMUP, REPS = 1, 5
PEAK_MACS = 1.25e15  # bf16 MFMA, dense (2.5 PFLOP/s)


def build(users, items, emb, layers, dtype, dev, seed=5):
    m = NCF(C(users, "uid"), C(items, "iid"), C(2, "label"), emb_size=emb, layers=list(layers),
            dropout=0.0, emb_dtype=dtype, device=dev, random_seed=seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p is not m.embeddings.weight:
                p.copy_((0.3 * torch.randn(p.shape, generator=g)).to(p.device))
        for f in range(4):
            t = m.embeddings.table(f)
            for c0 in range(0, t.shape[0], 1 << 18):
                c1 = min(t.shape[0], c0 + (1 << 18))
                t[c0:c1] = (0.5 * torch.randn(c1 - c0, emb, generator=g)).to(device=t.device, dtype=t.dtype)
    return m.eval()


def check(m, uid, k):
    """recommend against recommend_by_forward on the first 64 users -> share of equal ids."""
    n = 64
    ids, sc = m.recommend({"uid": uid[:n]}, k)
    want_i, want_s = IModel.recommend_by_forward(m, {"uid": uid[:n]}, k, chunk=4096)
    bar = 3e-2 * float(want_s.abs().max())
    assert float((sc - want_s).abs().max()) <= bar, "fused scores off the forward path"
    gap = (want_s[:, :-1] - want_s[:, 1:]).abs()
    clear = torch.ones_like(want_i, dtype=torch.bool)
    clear[:, :-1] &= gap > 2 * bar
    clear[:, 1:] &= gap > 2 * bar
    assert torch.equal(ids[clear], want_i[clear]), "fused ids off the forward path"
    return float((ids == want_i).float().mean())


def work(batch, items, emb, layers, elem, tile_users):
    """Algorithmic MACs and bytes of one call, per path."""
    widths = [2 * emb] + list(layers)
    mlp = sum(a * b for a, b in zip(widths[:-1], widths[1:]))
    upper = mlp - 2 * emb * layers[0]
    pairs = batch * items
    user_tiles = -(-batch // tile_users)
    return {
        "pairs": pairs,
        "forward": {"mfma_macs": pairs * mlp, "valu_macs": pairs * (emb + layers[-1]),
                    "bytes": pairs * (4 * emb * 2 * 2 + 4 * 2) + pairs * 4 * emb * elem},
        "fused": {"mfma_macs": pairs * upper + user_tiles * items * emb * layers[0],
                  "valu_macs": pairs * (emb + layers[-1] + layers[0]) + batch * emb * layers[0],
                  "bytes": user_tiles * items * 2 * emb * elem + batch * 2 * emb * elem},
    }


def rehearse():
    from pytorchrec_amd import cpu_path
    m = build(23, 61, 8, (16, 8), torch.float32, None)
    uid = torch.randint(0, 23, (9,), generator=torch.Generator().manual_seed(1))
    ids, sc = retrieval.ncf_topk(m, uid, 7)
    want_i, want_s = IModel.recommend_by_forward(m, {"uid": uid}, 7, chunk=16)
    assert torch.allclose(sc, want_s, rtol=1e-4, atol=1e-6)
    assert float((ids == want_i).float().mean()) > 0.9
    w = work(B, 100_000, E, LAYERS, 2, 16)
    assert w["forward"]["mfma_macs"] // w["pairs"] == 26624 and w["fused"]["mfma_macs"] // w["pairs"] == 10240 + 64 * 128 // 16
    assert cpu_path.ncf_topk is not None
    print("rehearsal ok (torch paths at a toy size on the CPU; nothing timed)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncf_topk"))
    ap.add_argument("--items", type=int, nargs="+", default=[100_000])
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--trace-run", action="store_true",
                    help="two calls of the fused path and of forward@4096 (bf16 bank, the first --items), "
                         "nothing timed or written: the program of a kernel-trace run")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ncf_topk.py needs a GPU")
    dev = torch.device("cuda")
    if args.trace_run:
        m = build(USERS, args.items[0], E, LAYERS, torch.bfloat16, dev)
        uid = torch.randint(0, USERS, (B,), generator=torch.Generator().manual_seed(9)).to(dev)
        for _ in range(2):
            m.recommend({"uid": uid}, K)
            IModel.recommend_by_forward(m, {"uid": uid}, K, chunk=4096)
        torch.cuda.synchronize()
        return
    order_rng = np.random.default_rng(4)
    tu, ti = retrieval.ncf_tile_users(), retrieval.ncf_tile_items()
    paths = ["fused"] + [f"forward@{c}" for c in CHUNKS]
    res = {"B": B, "E": E, "layers": list(LAYERS), "k": K, "warmup": WARMUP, "reps": args.reps,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "tile_users": tu, "tile_items": ti,
           "peak_mfma_macs_per_s": PEAK_MACS, "measurements": []}
    for items in args.items:
        for dtype in DTYPES:
            m = build(USERS, items, E, LAYERS, dtype, dev)
            uid = torch.randint(0, USERS, (B,), generator=torch.Generator().manual_seed(9)).to(dev)
            data = {"uid": uid}
            same = check(m, uid, K)
            fns = {"fused": lambda: m.recommend(data, K)}
            for c in CHUNKS:
                fns[f"forward@{c}"] = (lambda c=c: IModel.recommend_by_forward(m, data, K, chunk=c))
            live, dropped = list(paths), {}
            for p in paths[1:]:  # a chunk whose gathered rows do not fit is left out, and said so
                try:
                    fns[p]()
                    torch.cuda.synchronize()
                except (RuntimeError, ValueError) as e:
                    live.remove(p)
                    dropped[p] = str(e).splitlines()[0][:200]
                    torch.cuda.empty_cache()
            times = {p: [] for p in live}
            for rep in range(WARMUP + args.reps):
                for path in order_rng.permutation(live):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[path]()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= WARMUP:
                        times[path].append(e0.elapsed_time(e1) * 1e3)
            row = {"items": items, "bank_dtype": str(dtype).replace("torch.", ""),
                   "splits": retrieval.ncf_default_splits(B, items), "ids_equal_to_forward": same,
                   "paths_left_out": dropped,
                   "work": work(B, items, E, LAYERS, m.embeddings.weight.element_size(), tu)}
            for p in live:
                t = np.array(times[p])
                row[p] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}
            best = min((p for p in live[1:]), key=lambda p: row[p]["median_us"])
            fused = row["fused"]["median_us"]
            row["best_forward"] = best
            row["forward_default_over_fused"] = row[f"forward@{CHUNKS[0]}"]["median_us"] / fused
            row["forward_best_over_fused"] = row[best]["median_us"] / fused
            row["fused_share_of_mfma_peak"] = row["work"]["fused"]["mfma_macs"] / (fused * 1e-6) / PEAK_MACS
            res["measurements"].append(row)
            print(f"items {items} {row['bank_dtype']}: " + ", ".join(
                f"{p} {row[p]['median_us'] / 1e3:.1f} ms" for p in live) +
                f"; default / fused {row['forward_default_over_fused']:.2f}x, best ({best}) / fused "
                f"{row['forward_best_over_fused']:.2f}x, splits {row['splits']}, "
                f"{100 * row['fused_share_of_mfma_peak']:.1f} % of the MFMA peak", flush=True)
            del m, uid, data, fns
            torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_ncf_topk.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
