"""Time the fused DLRM dot interaction against the torch ops it replaces, on the GPU (fails
without one).

Two measurements, each with two paths in one process, alternating in a fresh random order,
by device events after warm-up, the median over the repetitions:

  interaction   forward + backward of the interaction alone on bf16 operands, B = 4096,
                F = 26 (n = 27 vectors), at D = 16 and D = 128: ``dense.dot_interact`` ->
                mrec_dot_interact_fwd + mrec_dot_interact_bwd, against
                ``cpu_path.dot_interact(round_bf16=True)`` on the GPU (cat, bmm, index
                gather, cat, and autograd's backward of each);
  train_step    a whole ``DLRM.train_step`` at the Criteo shape (26 x 38,462 rows, 13 dense,
                D = 16, bottom 512-256-64-16, top 512-256, bf16 bank, B = 4096, BCE, SGD)
                with ``dense.DOT_INTERACT`` on and off.

The interaction's two launches are also timed alone (``kernels``: the library calls on
preallocated buffers, no autograd and no allocation in the window), which is what the
fraction of the stream-copy ceiling is taken from; the ``fused`` figure above includes the
host work of ``torch.autograd.Function`` around them.

A timed window is INNER calls between two events; the figure is the window over INNER.  The
repetitions are cut into GROUPS consecutive groups and the spread of a path is the range of
its group medians: the fused path counts as faster when its median is below the torch-ops
median by more than its own spread.

Writes <out>/bench_dlrm.json (default profiles/dlrm) with the algorithmic bytes of the fused
interaction -- forward reads (F + 1) D elements and writes x_cols per sample; backward reads
both again as operands and dx, and writes (F + 1) D -- and the fraction of the measured
stream-copy ceiling (profiles/ceilings.json) they amount to at the median of the kernels alone.
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
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn  # noqa: E402
from pytorchrec_amd.loss import BCEWithLogitsLoss  # noqa: E402
from pytorchrec_amd.model import DLRM  # noqa: E402

B, F, ROWS, N_DENSE = 4096, 26, 38462, 13
DIMS = (16, 128)
BOTTOM, TOP = [512, 256, 64, 16], [512, 256]
WARMUP, REPS, GROUPS = 5, 40, 5
INNER = {"interaction": 10, "kernels": 20, "train_step": 2}
PATHS = ("fused", "torch_ops")
BF = torch.bfloat16


def build(dev):
    sparse = [CategoricalColumnWithIdentity(ROWS, f"c{f}") for f in range(F)]
    dcols = [NumericColumn(f"d{j}") for j in range(N_DENSE)]
    m = DLRM(sparse, dcols, CategoricalColumnWithIdentity(2, "label"), emb_size=16,
             bottom_layers=BOTTOM, top_layers=TOP, emb_dtype=BF, device=dev, random_seed=1)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BCEWithLogitsLoss(), [], dev)
    m.embeddings.check_ids = False
    return m


def draw(m, gen, dev):
    data = {c.feature_name: torch.randint(0, ROWS, (B,), generator=gen, device=dev, dtype=torch.int32)
            for c in m.sparse_columns}
    data["__dense__"] = torch.rand(B, N_DENSE, generator=gen, device=dev)
    data["label"] = (torch.rand(B, generator=gen, device=dev) < 0.25).long()
    return data


def x_cols_of(D):
    n = F + 1
    return (D + n * (n - 1) // 2 + 7) // 8 * 8


def interaction_bytes(D):
    """Algorithmic bytes of the fused pair on bf16 tensors: the forward reads the operands and
    writes x; the backward reads the operands and dx and writes the operands' gradients."""
    ops, xc = (F + 1) * D, x_cols_of(D)
    return {"fwd": B * 2 * (ops + xc), "bwd": B * 2 * (ops + xc + ops)}


def kernel_pair(bot, rows, dx, D):
    """-> a callable issuing mrec_dot_interact_fwd + _bwd on preallocated buffers."""
    x = torch.empty(B, x_cols_of(D), dtype=BF, device=rows.device)
    dbot, drows = torch.empty_like(bot), torch.empty_like(rows)
    a = _mrec.DotInteractArgs()
    a.bot, a.bot_dtype, a.ld_bot = bot.data_ptr(), _mrec.BF16, bot.stride(0)
    a.rows, a.rows_dtype, a.ld_rows = rows.data_ptr(), _mrec.BF16, rows.stride(0)
    a.batch, a.n_fields, a.D = B, F, D
    a.x, a.x_dtype, a.ld_x, a.x_cols = x.data_ptr(), _mrec.BF16, x.stride(0), x.shape[1]
    a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), _mrec.BF16, dx.stride(0)
    a.dbot, a.ld_dbot = dbot.data_ptr(), dbot.stride(0)
    a.drows, a.ld_drows = drows.data_ptr(), drows.stride(0)
    st = _mrec.stream_handle()

    def run(keep=(x, dbot, drows)):
        _mrec.call("mrec_dot_interact_fwd", ctypes.byref(a), st)
        _mrec.call("mrec_dot_interact_bwd", ctypes.byref(a), st)

    return run


def summarise(t):
    t = np.asarray(t)
    groups = [float(np.median(g)) for g in np.array_split(t, GROUPS)]
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "group_medians_us": groups, "spread_us": max(groups) - min(groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlrm"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dlrm.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev)
    for D in DIMS:
        assert dense.dot_interact_supported(D, F, BF, BF, BF, BF)
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    times = {}

    def timed(name, kind, fn, paths=PATHS):
        for path in order_rng.permutation(paths):
            dense.DOT_INTERACT = path == "fused"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER[kind]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            yield (name, path), e0.elapsed_time(e1) * 1e3 / INNER[kind]

    for rep in range(WARMUP + REPS):
        data = draw(m, gen, dev)
        jobs = []
        for D in DIMS:
            rows = torch.randn(B, F * D, generator=gen, device=dev).to(BF)
            bot = torch.randn(B, D, generator=gen, device=dev).to(BF)
            dx = torch.randn(B, x_cols_of(D), generator=gen, device=dev).to(BF)

            def interaction(rows=rows, bot=bot, dx=dx, D=D):
                b, r = bot.detach().requires_grad_(), rows.detach().requires_grad_()
                dense.dot_interact(b, r, F, x_cols=x_cols_of(D), x_dtype=BF).backward(dx)

            jobs.append((f"interaction_D{D}", "interaction", interaction))
            jobs.append((f"interaction_D{D}", "kernels", kernel_pair(bot, rows, dx, D)))
        jobs.append(("train_step", "train_step", lambda: m.train_step(data)))
        for name, kind, fn in jobs:
            if kind == "kernels":  # one path: the launches themselves
                for _, us in timed(name, kind, fn, paths=("fused",)):
                    if rep >= WARMUP:
                        times.setdefault((name, "kernels"), []).append(us)
                continue
            for key, us in timed(name, kind, fn):
                if rep >= WARMUP:
                    times.setdefault(key, []).append(us)
    dense.DOT_INTERACT = True

    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy_gbs = float(json.load(f)["stream_copy"]["GB/s"])
    res = {"B": B, "F": F, "rows_per_table": ROWS, "n_dense": N_DENSE, "bottom": BOTTOM, "top": TOP,
           "dtype": "bf16", "warmup": WARMUP, "reps": REPS, "groups": GROUPS, "inner": INNER,
           "timing": "device events around INNER host-launched calls, alternating, random order",
           "device": torch.cuda.get_device_name(0), "stream_copy_GBps": copy_gbs, "measurements": {}}
    for name in [f"interaction_D{D}" for D in DIMS] + ["train_step"]:
        row = {p: summarise(times[(name, p)]) for p in PATHS}
        fu, to = row["fused"], row["torch_ops"]
        row["speedup_median"] = to["median_us"] / fu["median_us"]
        row["fused_is_faster"] = bool(to["median_us"] - fu["median_us"] > fu["spread_us"])
        if name.startswith("interaction"):
            by = interaction_bytes(int(name.split("_D")[1]))
            row["x_cols"] = x_cols_of(int(name.split("_D")[1]))
            row["fused_model_bytes"] = by
            total = by["fwd"] + by["bwd"]
            row["kernels"] = summarise(times[(name, "kernels")])
            row["kernels_GBps_of_model_bytes"] = total / row["kernels"]["median_us"] * 1e-3
            row["kernels_fraction_of_stream_copy"] = row["kernels_GBps_of_model_bytes"] / copy_gbs
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}] "
            f"spread {row[p]['spread_us']:.1f}" for p in PATHS)
            + f", speedup {row['speedup_median']:.2f}x, faster: {row['fused_is_faster']}"
            + (f", kernels alone {row['kernels']['median_us']:.1f} us = "
               f"{row['kernels_fraction_of_stream_copy']:.3f} of stream copy" if "kernels" in row else ""))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_dlrm.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
