"""Time the fused full-catalogue top-K (mrec_topk behind ``retrieval.topk``) against the
torch-ops way of answering the same question, on the GPU (fails without one).

Shapes: B = 4096 queries, D = 64, k = 100, catalogues of 10^5 and 10^6 items, fp32 and
bf16 banks; N(0, 1) queries and rows.

Two paths, in one process on the same inputs, alternating in a fresh random order, by
device events after warm-up, the median over the repetitions:
  fused  retrieval.topk -> mrec_topk (scan + merge launches; the [B, items] scores never
         reach memory);
  torch  what a torch user writes when [B, items] does not fit: per chunk of 65,536 items
         ``q @ T[chunk].T`` in the bank's dtype (bf16 banks: a bf16 GEMM), ``torch.topk``
         of the chunk, and a ``torch.topk`` merge with the running list.  It applies no
         exclusion and no tie rule, so it does less than the fused path.
Before timing, the fused result of the first 64 queries is compared with
``cpu_path.topk`` (the contract in torch ops) on the same device: the ids must agree
wherever neighbouring scores are not within rounding of each other.

Writes <out>/bench_topk.json (default profiles/topk) with, per shape, both medians, their
ratio, the split count, and the algorithmic work: 2 B items D flop, and the table bytes
read once per query tile.  ``--rehearse`` runs the torch path at a toy size on the CPU to
check the script itself; it times nothing and writes nothing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import cpu_path, retrieval  # noqa: E402
from pytorchrec_amd.embedding import EmbeddingBank  # noqa: E402

B, D, K = 4096, 64, 100
ITEMS = (100_000, 1_000_000)
DTYPES = (torch.float32, torch.bfloat16)
CHUNK = 65536
WARMUP, REPS = 3, 12
PATHS = ("fused", "torch")


def build(items, dtype, dev, gen):
    bank = EmbeddingBank([items], D, dtype=dtype, device=dev)
    with torch.no_grad():
        for c0 in range(0, items, 1 << 18):
            c1 = min(items, c0 + (1 << 18))
            bank.weight[c0:c1, :D] = torch.randn(c1 - c0, D, generator=gen, device=dev).to(dtype)
    return bank


def torch_topk(table, q, k, chunk=CHUNK):
    """Chunked ``q @ T.T`` + ``torch.topk`` + a running merge -> (ids int64, scores fp32)."""
    qd = q.to(table.dtype)
    best_s = best_i = None
    for c0 in range(0, table.shape[0], chunk):
        s = (qd @ table[c0:c0 + chunk].t()).float()
        cs, ci = torch.topk(s, min(k, s.shape[1]), dim=1)
        ci = ci + c0
        if best_s is not None:
            cs, ci = torch.cat([best_s, cs], 1), torch.cat([best_i, ci], 1)
            cs, sel = torch.topk(cs, min(k, cs.shape[1]), dim=1)
            ci = torch.gather(ci, 1, sel)
        best_s, best_i = cs, ci
    return best_i, best_s


def check(bank, q, k):
    """The fused result of the first 64 queries against cpu_path.topk -> share of equal ids."""
    n = 64
    ids, sc = retrieval.topk(bank, 0, q[:n], k)
    want_i, want_s = cpu_path.topk(bank.weight.detach(), D, q[:n].float(), k, 0, bank.category_nums[0],
                                   False, None, chunk=CHUNK)
    tol = (D + 2) * 2.0 ** -24 * float(q[:n].abs().max()) * float(bank.table(0).detach().abs().max()) * D
    assert float((sc - want_s).abs().max()) <= tol, "fused scores off the torch-ops restatement"
    gap = (want_s[:, :-1] - want_s[:, 1:]).abs()
    clear = torch.ones_like(want_i, dtype=torch.bool)
    clear[:, :-1] &= gap > 2 * tol
    clear[:, 1:] &= gap > 2 * tol
    assert torch.equal(ids[clear], want_i[clear]), "fused ids off the torch-ops restatement"
    return float((ids == want_i).float().mean())


def rehearse():
    gen = torch.Generator().manual_seed(1)
    table = torch.randn(1000, D, generator=gen)
    q = torch.randn(8, D, generator=gen)
    ids, sc = torch_topk(table, q, 10, chunk=300)
    want = torch.topk(q @ table.t(), 10, dim=1)
    assert torch.equal(ids, want.indices) and torch.allclose(sc, want.values)
    print("rehearsal ok (torch path at a toy size on the CPU; nothing timed)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py needs a GPU")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    res = {"B": B, "D": D, "k": K, "chunk_torch": CHUNK, "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "tile_queries": retrieval.tile_queries(),
           "tile_items": retrieval.tile_items(), "measurements": []}
    for items in ITEMS:
        for dtype in DTYPES:
            bank = build(items, dtype, dev, gen)
            table = bank.table(0)
            q = torch.randn(B, D, generator=gen, device=dev)
            same = check(bank, q, K)
            fns = {"fused": lambda: retrieval.topk(bank, 0, q, K),
                   "torch": lambda: torch_topk(table, q, K)}
            times = {p: [] for p in PATHS}
            for rep in range(WARMUP + REPS):
                for path in order_rng.permutation(PATHS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[path]()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= WARMUP:
                        times[path].append(e0.elapsed_time(e1) * 1e3)
            row = {"items": items, "bank_dtype": str(dtype).replace("torch.", ""),
                   "splits": retrieval.default_splits(B, items), "ids_equal_to_restatement": same,
                   "flop": 2 * B * items * D,
                   "table_bytes_per_query_tile": items * D * bank.weight.element_size(),
                   "query_tiles": -(-B // retrieval.tile_queries())}
            for p in PATHS:
                t = np.array(times[p])
                row[p] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                          "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                          "p90_us": float(np.percentile(t, 90))}
            row["torch_over_fused_median"] = row["torch"]["median_us"] / row["fused"]["median_us"]
            res["measurements"].append(row)
            print(f"items {items} {row['bank_dtype']}: " + ", ".join(
                f"{p} {row[p]['median_us']:.0f} us [{row[p]['min_us']:.0f}, {row[p]['max_us']:.0f}]"
                for p in PATHS) + f", torch / fused {row['torch_over_fused_median']:.2f}x, "
                f"splits {row['splits']}", flush=True)
            del bank, table, q
            torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_topk.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
