"""Time forward + backward of the pooled lookup against the composed path it replaces,
on the GPU (fails without one).

Shapes: B = 4096 bags of L = 50 ids, D = 16 bf16 + first-order column (64-B rows),
fused SGD, two tables: 63,002 rows (C4's item table, cache-resident) and 2^23 rows
(512 MB, beyond the 256 MB Infinity Cache).  Ids are uniform over [1, rows) with lengths uniform in
1..50 and redrawn for every repetition, so most of the large table is touched from
step to step.

Two paths, in one process, alternating, by device events after warm-up:
  pooled    pooled_gather(mode="sqrtn", pad="zero") + backward;
  composed  gather(flat ids, pad_negative=True) + torch masked sum + scale + backward
            (a [B*L, D] activation forward, a [B*L, D] gradient backward).

Writes profiles/pool/bench_pool.json: per table the median, min and max time of each
path over the repetitions, and the byte-model rate of the pooled path:
  forward  bytes per bag  = L * (id bytes + row bytes) + output row
  backward bytes per bag  = L * (4 + 2 * row bytes) + gradient row
(L counted as the valid length: padding positions cost their id bytes only.)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd.embedding import EmbeddingBank, gather, pooled_gather  # noqa: E402

B, L, D = 4096, 50, 16
WARMUP, REPS = 5, 30


def draw_ids(rows, gen, dev):
    ids = torch.randint(1, rows, (B, L), generator=gen, device=dev, dtype=torch.int32)
    lens = torch.randint(1, L + 1, (B, 1), generator=gen, device=dev)
    return ids * (torch.arange(L, device=dev)[None, :] < lens), lens


def pooled_step(bank, ids, dout):
    pooled_gather(bank, [ids], mode="sqrtn", pad="zero", out_dtype=torch.float32).backward(dout)


def composed_step(bank, ids, dout):
    flat = torch.where(ids > 0, ids, torch.full_like(ids, -1)).reshape(-1)
    rows = gather(bank, [flat], out_dtype=torch.float32, pad_negative=True).reshape(B, L, D)
    n = (ids > 0).sum(1, keepdim=True).float()
    (rows.sum(1) * n.rsqrt()).backward(dout)


def bench_table(rows, dev):
    bank = EmbeddingBank([rows], D, with_first_order=True, dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        bank.weight.normal_(0, 0.01)
    bank.use_fused_sgd(0.01)
    bank.check_ids = False
    gen = torch.Generator(device=dev).manual_seed(rows)
    dout = torch.randn(B, D, generator=gen, device=dev)
    steps = {"pooled": pooled_step, "composed": composed_step}
    times = {k: [] for k in steps}
    valid = []
    for rep in range(WARMUP + REPS):
        ids, lens = draw_ids(rows, gen, dev)
        for name, fn in steps.items():  # alternating, on the same ids
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(bank, ids, dout)
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(e0.elapsed_time(e1) * 1e3)
        if rep >= WARMUP:
            valid.append(float(lens.sum()))
    row_bytes = bank.row_stride * bank.weight.element_size()
    nv = float(np.mean(valid))
    fwd = B * L * 4 + nv * row_bytes + B * D * 4
    bwd = nv * (4 + 2 * row_bytes) + (B * L - nv) * 4 + B * D * 4
    out = {"rows": rows, "table_bytes": rows * row_bytes, "mean_valid_lookups": nv,
           "model_bytes_fwd": fwd, "model_bytes_bwd": bwd}
    for name, t in times.items():
        t = np.array(t)
        out[name] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                     "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                     "p90_us": float(np.percentile(t, 90))}
    out["pooled"]["model_GBps"] = (fwd + bwd) / (out["pooled"]["median_us"] * 1e-6) / 1e9
    out["speedup_median"] = out["composed"]["median_us"] / out["pooled"]["median_us"]
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool.py needs a GPU")
    dev = torch.device("cuda")
    res = {"B": B, "L": L, "D": D, "dtype": "bf16", "update": "fused sgd", "warmup": WARMUP,
           "reps": REPS, "timing": "device events around forward + backward, host-launched",
           "device": torch.cuda.get_device_name(0), "tables": []}
    for rows in (63002, 1 << 23):
        r = bench_table(rows, dev)
        res["tables"].append(r)
        print(f"rows {rows}: pooled {r['pooled']['median_us']:.1f} us "
              f"[{r['pooled']['min_us']:.1f}, {r['pooled']['max_us']:.1f}], composed "
              f"{r['composed']['median_us']:.1f} us [{r['composed']['min_us']:.1f}, "
              f"{r['composed']['max_us']:.1f}], byte model {r['pooled']['model_GBps']:.0f} GB/s")
    out_dir = os.path.join(ROOT, "profiles", "pool")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_pool.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
