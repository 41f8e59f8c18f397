"""Time the fused Compressed Interaction Network against the torch ops it replaces, on the GPU
(fails without one).

Two measurements, each with two paths in one process, alternating in a fresh random order,
by device events after warm-up, the median over the repetitions:

  cin          forward + backward of the CIN alone on bf16 operands, B = 4096, m = 26, D = 16,
               at H = [200, 200, 200] and at H = [128, 128]: ``dense.cin`` -> mrec_cin_fwd +
               mrec_cin_bwd per layer, against ``cpu_path.cin(round_bf16=True)`` on the GPU (the
               same contract in torch ops, Z formed for 256 samples at a time);
  train_step   a whole ``XDeepFM.train_step`` at the Criteo shape (26 x 38,462 rows, 13 dense,
               D = 16, cin 200-200-200, MLP 400-400, bf16 bank, B = 4096, BCE, SGD) with
               ``dense.CIN_FUSED`` on and off.

A timed window is INNER calls between two events; the figure is the window over INNER.  The
repetitions are cut into GROUPS consecutive groups and the spread of a path is the range of
its group medians: the fused path counts as faster when its median is below the torch-ops
median by more than its own spread.

Writes <out>/bench_xdeepfm.json (default profiles/xdeepfm) with ms per call, samples/s and
the fraction of the 2.5 PFLOP/s bf16 MFMA peak by the algorithmic flop count: a layer's
forward is 2 B D H_prev m H, its backward twice that (the data and the weight gradient).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import dense  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn  # noqa: E402
from pytorchrec_amd.loss import BCEWithLogitsLoss  # noqa: E402
from pytorchrec_amd.model import XDeepFM  # noqa: E402

B, M, D, ROWS, N_DENSE = 4096, 26, 16, 38462, 13
CIN_SHAPES = ([200, 200, 200], [128, 128])
LAYERS = [400, 400]
WARMUP, REPS, GROUPS = 3, 20, 5
INNER = {"cin": 2, "train_step": 2}
PATHS = ("fused", "torch_ops")
PEAK_FLOPS = 2.5e15
BF = torch.bfloat16


def build(dev):
    sparse = [CategoricalColumnWithIdentity(ROWS, f"c{f}") for f in range(M)]
    dcols = [NumericColumn(f"d{j}") for j in range(N_DENSE)]
    m = XDeepFM(sparse, dcols, CategoricalColumnWithIdentity(2, "label"), emb_size=D, layers=LAYERS,
                cin_layers=CIN_SHAPES[0], emb_dtype=BF, device=dev, random_seed=1)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BCEWithLogitsLoss(), [], dev)
    m.embeddings.check_ids = False
    return m


def draw(m, gen, dev):
    data = {c.feature_name: torch.randint(0, ROWS, (B,), generator=gen, device=dev, dtype=torch.int32)
            for c in m.sparse_columns}
    data["__dense__"] = torch.rand(B, N_DENSE, generator=gen, device=dev)
    data["label"] = (torch.rand(B, generator=gen, device=dev) < 0.25).long()
    return data


def cin_flops(widths):
    """Algorithmic flops of forward + backward (no field-pitch or tile padding counted)."""
    fwd = sum(2 * B * D * hp * M * h for hp, h in zip([M, *widths[:-1]], widths))
    return {"fwd": fwd, "fwd_bwd": 3 * fwd}


def summarise(t):
    t = np.asarray(t)
    groups = [float(np.median(g)) for g in np.array_split(t, GROUPS)]
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "group_medians_us": groups, "spread_us": max(groups) - min(groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xdeepfm"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xdeepfm.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev)
    for widths in CIN_SHAPES:
        assert dense.cin_supported(M, D, widths, BF)
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    weights = {tuple(w): [(torch.randn(h, hp, M, generator=gen, device=dev) * (hp * M) ** -0.5).requires_grad_()
                          for hp, h in zip([M, *w[:-1]], w)] for w in CIN_SHAPES}
    times = {}

    def timed(name, kind, fn):
        for path in order_rng.permutation(PATHS):
            dense.CIN_FUSED = path == "fused"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER[kind]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            yield (name, path), e0.elapsed_time(e1) * 1e3 / INNER[kind]

    for rep in range(WARMUP + REPS):
        data = draw(m, gen, dev)
        x0 = torch.randn(B, M * D, generator=gen, device=dev).to(BF)
        jobs = []
        for widths in CIN_SHAPES:
            ws = weights[tuple(widths)]
            dp = torch.randn(B, sum(widths), generator=gen, device=dev)

            def cin(ws=ws, dp=dp):
                x = x0.detach().requires_grad_()
                dense.cin(x, M, ws, x_dtype=BF).backward(dp)
                for w in ws:
                    w.grad = None

            jobs.append(("cin_" + "_".join(map(str, widths)), "cin", cin))
        jobs.append(("train_step", "train_step", lambda: m.train_step(data)))
        for name, kind, fn in jobs:
            for key, us in timed(name, kind, fn):
                if rep >= WARMUP:
                    times.setdefault(key, []).append(us)
    dense.CIN_FUSED = True

    res = {"B": B, "m": M, "D": D, "rows_per_table": ROWS, "n_dense": N_DENSE, "mlp": LAYERS,
           "dtype": "bf16", "warmup": WARMUP, "reps": REPS, "groups": GROUPS, "inner": INNER,
           "timing": "device events around INNER host-launched calls, alternating, random order",
           "device": torch.cuda.get_device_name(0), "peak_bf16_flops": PEAK_FLOPS, "measurements": {}}
    for name in ["cin_" + "_".join(map(str, w)) for w in CIN_SHAPES] + ["train_step"]:
        row = {p: summarise(times[(name, p)]) for p in PATHS}
        fu, to = row["fused"], row["torch_ops"]
        for p in PATHS:
            row[p]["ms_per_call"] = row[p]["median_us"] * 1e-3
            row[p]["samples_per_s"] = B / (row[p]["median_us"] * 1e-6)
        row["speedup_median"] = to["median_us"] / fu["median_us"]
        row["fused_is_faster"] = bool(to["median_us"] - fu["median_us"] > fu["spread_us"])
        if name.startswith("cin_"):
            fl = cin_flops([int(v) for v in name.split("_")[1:]])
            row["flops"] = fl
            for p in PATHS:
                row[p]["fraction_of_mfma_peak"] = fl["fwd_bwd"] / (row[p]["median_us"] * 1e-6) / PEAK_FLOPS
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}] "
            f"spread {row[p]['spread_us']:.1f}" for p in PATHS)
            + f", speedup {row['speedup_median']:.2f}x, faster: {row['fused_is_faster']}"
            + (f", fused at {fu['fraction_of_mfma_peak']:.3f} of the MFMA peak" if "flops" in row else ""),
            flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_xdeepfm.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
