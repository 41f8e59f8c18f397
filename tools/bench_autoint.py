"""Time the fused AutoInt interacting layers against the torch ops they replace, on the GPU
(fails without one).

Two measurements, each with two paths in one process, alternating in a fresh random order,
by device events after warm-up, the median over the repetitions:

  stack        forward + backward of the interacting stack alone on bf16 operands, B = 4096,
               m = 26, D = 16, three layers of 2 heads x 32 (the paper's) and three of 2 x 8:
               ``dense.autoint`` -> mrec_autoint_fwd + mrec_autoint_bwd per layer, against
               ``cpu_path.autoint(round_bf16=True)`` on the GPU (the same contract in torch ops,
               the scores formed for 256 samples at a time);
  train_step   a whole ``AutoInt.train_step`` at the Criteo shape (26 x 38,462 rows, 13 dense,
               D = 16, three layers of 2 x 32, MLP 400-400, bf16 bank, B = 4096, BCE, SGD) with
               ``dense.AUTOINT_FUSED`` on and off.

The library calls of one middle layer (d_in = A) are also timed alone (``kernels``: forward,
then backward, on fixed buffers): the figure the fraction of the stream-copy ceiling
(profiles/ceilings.json) is taken from, for the algorithmic bytes -- x read and y written in the
forward; x, y, dy read and dx written in the backward.

A timed window is INNER calls between two events; the figure is the window over INNER.  The
repetitions are cut into GROUPS consecutive groups and the spread of a path is the range of
its group medians: the fused path counts as faster when its median is below the torch-ops
median by more than its own spread.

Writes <out>/bench_autoint.json (default profiles/autoint).
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
from pytorchrec_amd.model import AutoInt  # noqa: E402

B, M, D, ROWS, N_DENSE = 4096, 26, 16, 38462, 13
STACKS = ((3, 2, 32), (3, 2, 8))  # layers, heads, head_dim
LAYERS = [400, 400]
WARMUP, REPS, GROUPS = 3, 20, 5
INNER = {"stack": 2, "train_step": 2, "kernels": 8}
PATHS = ("fused", "torch_ops")
BF = torch.bfloat16


def build(dev):
    sparse = [CategoricalColumnWithIdentity(ROWS, f"c{f}") for f in range(M)]
    dcols = [NumericColumn(f"d{j}") for j in range(N_DENSE)]
    nl, heads, hd = STACKS[0]
    m = AutoInt(sparse, dcols, CategoricalColumnWithIdentity(2, "label"), emb_size=D, layers=LAYERS,
                att_layers=nl, att_heads=heads, att_head_dim=hd, emb_dtype=BF, device=dev, random_seed=1)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BCEWithLogitsLoss(), [], dev)
    m.embeddings.check_ids = False
    return m


def draw(m, gen, dev):
    data = {c.feature_name: torch.randint(0, ROWS, (B,), generator=gen, device=dev, dtype=torch.int32)
            for c in m.sparse_columns}
    data["__dense__"] = torch.rand(B, N_DENSE, generator=gen, device=dev)
    data["label"] = (torch.rand(B, generator=gen, device=dev) < 0.25).long()
    return data


def stack_weights(nl, heads, hd, gen, dev):
    A, d, out = heads * hd, D, []
    for _ in range(nl):
        out.append(tuple((torch.randn(A, d, generator=gen, device=dev) * d ** -0.5).requires_grad_()
                         for _ in range(4)))
        d = A
    return out


def layer_calls(layer, heads, gen, dev):
    """The two library calls of one layer on fixed bf16 buffers -> (callable, algorithmic bytes)."""
    A, d = layer[0].shape
    x = torch.randn(B, M * d, generator=gen, device=dev).to(BF)
    dy = torch.randn(B, M * A, generator=gen, device=dev).to(BF)
    y, dx = torch.empty(B, M * A, dtype=BF, device=dev), torch.empty(B, M * d, dtype=BF, device=dev)
    dw = torch.empty(4, A, d, device=dev)
    nws = int(_mrec.lib().mrec_autoint_bwd_workspace_size(B, d, A))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    wf, wb = dense.autoint_images(*layer)
    a = _mrec.AutoIntArgs()
    code = _mrec.dtype_code(BF)
    a.x, a.x_dtype, a.ld_x = x.data_ptr(), code, x.stride(0)
    a.w_fwd, a.ld_w_fwd, a.w_bwd, a.ld_w_bwd = wf.data_ptr(), wf.stride(0), wb.data_ptr(), wb.stride(0)
    a.has_res, a.batch, a.n_fields, a.d_in, a.heads, a.head_dim, a.A, a.scale = 1, B, M, d, heads, A // heads, A, 1.0
    a.y, a.y_dtype, a.ld_y = y.data_ptr(), code, y.stride(0)
    a.dy, a.dy_dtype, a.ld_dy = dy.data_ptr(), code, dy.stride(0)
    a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), code, dx.stride(0)
    a.dw, a.workspace, a.workspace_bytes = dw.data_ptr(), ws.data_ptr(), nws
    keep = (x, dy, y, dx, dw, ws, wf, wb)

    def run():
        st = _mrec.stream_handle()
        _mrec.call("mrec_autoint_fwd", ctypes.byref(a), st)
        _mrec.call("mrec_autoint_bwd", ctypes.byref(a), st)
        return keep

    nbytes = 2 * B * M * ((d + A) + (d + A + A + d))
    return run, nbytes


def summarise(t):
    t = np.asarray(t)
    groups = [float(np.median(g)) for g in np.array_split(t, GROUPS)]
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "group_medians_us": groups, "spread_us": max(groups) - min(groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoint"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoint.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev)
    for nl, heads, hd in STACKS:
        assert dense.autoint_supported(M, D, [heads * hd] * nl, heads, BF)
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    weights = {s: stack_weights(*s, gen, dev) for s in STACKS}
    kernels = {s: layer_calls(weights[s][1], s[1], gen, dev) for s in STACKS}
    times = {}

    def timed(name, kind, fn):
        for path in (("kernels",) if kind == "kernels" else order_rng.permutation(PATHS)):
            dense.AUTOINT_FUSED = path != "torch_ops"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER[kind]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            yield (name, path), e0.elapsed_time(e1) * 1e3 / INNER[kind]

    names = {s: "stack_%dx%dx%d" % s for s in STACKS}
    for rep in range(WARMUP + REPS):
        data = draw(m, gen, dev)
        x0 = torch.randn(B, M * D, generator=gen, device=dev).to(BF)
        jobs = []
        for s in STACKS:
            ws = weights[s]
            dy = torch.randn(B, M * s[1] * s[2], generator=gen, device=dev).to(BF)

            def stack(ws=ws, dy=dy, heads=s[1]):
                x = x0.detach().requires_grad_()
                dense.autoint(x, M, ws, heads, 1.0, x_dtype=BF).backward(dy)
                for l in ws:
                    for w in l:
                        w.grad = None

            jobs.append((names[s], "stack", stack))
            jobs.append((names[s], "kernels", kernels[s][0]))
        jobs.append(("train_step", "train_step", lambda: m.train_step(data)))
        for name, kind, fn in jobs:
            for key, us in timed(name, kind, fn):
                if rep >= WARMUP:
                    times.setdefault(key, []).append(us)
    dense.AUTOINT_FUSED = True

    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy = json.load(f)["stream_copy"]
    copy_bps = copy["bytes_moved"] / (copy["us"] * 1e-6)
    res = {"B": B, "m": M, "D": D, "rows_per_table": ROWS, "n_dense": N_DENSE, "mlp": LAYERS,
           "dtype": "bf16", "warmup": WARMUP, "reps": REPS, "groups": GROUPS, "inner": INNER,
           "timing": "device events around INNER host-launched calls, alternating, random order",
           "device": torch.cuda.get_device_name(0), "stream_copy_bytes_per_s": copy_bps, "measurements": {}}
    for name in [names[s] for s in STACKS] + ["train_step"]:
        row = {p: summarise(times[(name, p)]) for p in PATHS}
        fu, to = row["fused"], row["torch_ops"]
        for p in PATHS:
            row[p]["ms_per_call"] = row[p]["median_us"] * 1e-3
            row[p]["samples_per_s"] = B / (row[p]["median_us"] * 1e-6)
        row["speedup_median"] = to["median_us"] / fu["median_us"]
        row["fused_is_faster"] = bool(to["median_us"] - fu["median_us"] > fu["spread_us"])
        extra = ""
        if (name, "kernels") in times:
            s = [k for k in STACKS if names[k] == name][0]
            row["kernels"] = summarise(times[(name, "kernels")])
            row["kernels"]["what"] = "mrec_autoint_fwd + mrec_autoint_bwd of one layer with d_in = A, bf16"
            row["kernels"]["algorithmic_bytes"] = kernels[s][1]
            row["kernels"]["stream_copy_us"] = kernels[s][1] / copy_bps * 1e6
            row["kernels"]["fraction_of_stream_copy"] = row["kernels"]["stream_copy_us"] / row["kernels"]["median_us"]
            extra = (f", one layer's two calls alone {row['kernels']['median_us']:.1f} us = "
                     f"{row['kernels']['fraction_of_stream_copy']:.3f} of stream copy")
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}] "
            f"spread {row[p]['spread_us']:.1f}" for p in PATHS)
            + f", speedup {row['speedup_median']:.2f}x, faster: {row['fused_is_faster']}" + extra, flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_autoint.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
