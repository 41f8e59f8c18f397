"""Time the fused DCN-Mix cross stack against the torch ops it replaces, on the GPU (fails
without one).

Each measurement has two paths in one process, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions:

  stack        forward + backward of the cross stack alone, B = 4096, d = 429, three layers,
               bf16 x0, (K, r) = (4, 64) and (1, 64): ``dense.cross_mix`` -> mrec_cross_mix_fwd
               + mrec_cross_mix_bwd + the weight-gradient GEMMs, against
               ``cpu_path.cross_mix(round_bf16=True)`` on the GPU (the same contract in torch ops);
  train_step   a whole ``DCNMix.train_step`` at the Criteo shape (26 x 38,462 rows, 13 dense,
               D = 16, three layers of 4 x 64, MLP 400-400, bf16 bank, B = 4096, BCE, SGD) with
               ``dense.CROSS_MIX_FUSED`` on and off; the ``dcnv2`` step at the same shape is
               timed beside it for context (``dcnv2_train_step``, one path).

The training forward launch is also timed alone (``forward``) on fixed buffers: the figure the
fraction of the stream-copy ceiling (profiles/ceilings.json) is taken from, for its algorithmic
bytes -- x0 read, the saved stack and x_L written; so is the backward launch (``backward``).  The first stack's forward is also timed at
B = 2048, 4096 and 8192 (``forward_by_batch``): half a 16-row tile, one tile and two tiles per
CU, which is what the tile height costs.

A timed window is INNER calls between two events; the figure is the window over INNER.  The
repetitions are cut into GROUPS consecutive groups and the spread of a path is the range of
its group medians: the fused path counts as faster when its median is below the torch-ops
median by more than its own spread.

Writes <out>/bench_dcnmix.json (default profiles/dcnmix).
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
from pytorchrec_amd.model import DCNMix, DCNv2  # noqa: E402

B, M, D, ROWS, N_DENSE, NL = 4096, 26, 16, 38462, 13, 3
DIN = M * D + N_DENSE  # 429
STACKS = ((4, 64), (1, 64))  # K, r
TILE_BATCHES = (2048, 4096, 8192)  # 128, 256, 512 tiles of 16 rows on 256 CUs
LAYERS = [400, 400]
WARMUP, REPS, GROUPS = 3, 20, 5
INNER = {"stack": 2, "train_step": 2, "forward": 8}
PATHS = ("fused", "torch_ops")
BF = torch.bfloat16


def build(cls, dev, **kw):
    sparse = [CategoricalColumnWithIdentity(ROWS, f"c{f}") for f in range(M)]
    dcols = [NumericColumn(f"d{j}") for j in range(N_DENSE)]
    m = cls(sparse, dcols, CategoricalColumnWithIdentity(2, "label"), emb_size=D, layers=LAYERS,
            cross_layers=NL, emb_dtype=BF, device=dev, random_seed=1, **kw)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BCEWithLogitsLoss(), [], dev)
    m.embeddings.check_ids = False
    return m


def draw(m, gen, dev):
    data = {c.feature_name: torch.randint(0, ROWS, (B,), generator=gen, device=dev, dtype=torch.int32)
            for c in m.sparse_columns}
    data["__dense__"] = torch.rand(B, N_DENSE, generator=gen, device=dev)
    data["label"] = (torch.rand(B, generator=gen, device=dev) < 0.25).long()
    return data


def stack_weights(K, r, gen, dev):
    n = lambda *s, std: (torch.randn(*s, generator=gen, device=dev) * std).requires_grad_()  # noqa: E731
    return [(n(K * r, DIN, std=DIN ** -0.5), n(K, r, r, std=r ** -0.5), n(DIN, K * r, std=(K * r) ** -0.5),
             n(DIN, std=0.1), n(K, DIN, std=DIN ** -0.5) if K > 1 else None) for _ in range(NL)]


def forward_call(layers, K, r, gen, dev, B=B):
    """The training forward launch on fixed bf16 buffers -> (callable, algorithmic bytes)."""
    dp = (DIN + 7) // 8 * 8
    x0 = torch.randn(B, dp, generator=gen, device=dev).to(BF)
    y = torch.empty(B, dp, dtype=BF, device=dev)
    saved = torch.empty(NL, B, dp, dtype=BF, device=dev)
    a = _mrec.CrossMixArgs()
    keep = [x0, y, saved]
    for l, (V, C, U, b, gate) in enumerate(layers):
        keep.append(dense.cross_mix_images(V, C, U, gate)[0])
        a.w_img[l], a.bias[l] = keep[-1].data_ptr(), b.data_ptr()
    a.x0, a.x0_dtype, a.ld_x0 = x0.data_ptr(), _mrec.dtype_code(BF), dp
    a.batch, a.d, a.K, a.r, a.layers, a.train = B, DIN, K, r, NL, 1
    a.y, a.ld_y = y.data_ptr(), dp
    a.saved, a.ld_saved, a.saved_layer_stride = saved.data_ptr(), dp, B * dp

    dy, dx0 = torch.randn(B, dp, generator=gen, device=dev).to(BF), torch.empty(B, dp, device=dev)
    nws = int(_mrec.lib().mrec_cross_mix_bwd_workspace_size(B, DIN, K, r, NL))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    a.dy, a.dy_dtype, a.ld_dy = dy.data_ptr(), _mrec.dtype_code(BF), dp
    a.dx0, a.ld_dx0, a.workspace, a.workspace_bytes = dx0.data_ptr(), dp, ws.data_ptr(), nws
    keep += [dy, dx0, ws]

    def run():
        _mrec.call("mrec_cross_mix_fwd", ctypes.byref(a), _mrec.stream_handle())
        return keep

    def run_bwd():  # (reads the stack a forward call saved)
        _mrec.call("mrec_cross_mix_bwd", ctypes.byref(a), _mrec.stream_handle())

    return run, 2 * B * (DIN + NL * dp + DIN), run_bwd


def summarise(t):
    t = np.asarray(t)
    groups = [float(np.median(g)) for g in np.array_split(t, GROUPS)]
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "group_medians_us": groups, "spread_us": max(groups) - min(groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcnmix"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcnmix.py needs a GPU")
    dev = torch.device("cuda")
    m = build(DCNMix, dev, cross_experts=STACKS[0][0], cross_rank=STACKS[0][1])
    v2 = build(DCNv2, dev)
    for K, r in STACKS:
        assert dense.cross_mix_supported(DIN, K, r, NL, BF)
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    weights = {s: stack_weights(*s, gen, dev) for s in STACKS}
    forwards = {s: forward_call(weights[s], *s, gen, dev) for s in STACKS}
    by_batch = {b: forward_call(weights[STACKS[0]], *STACKS[0], gen, dev, B=b)[0] for b in TILE_BATCHES}
    times = {}

    def timed(name, kind, fn, single):
        for path in ((single,) if single else order_rng.permutation(PATHS)):
            dense.CROSS_MIX_FUSED = path != "torch_ops"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER[kind]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            yield (name, path), e0.elapsed_time(e1) * 1e3 / INNER[kind]

    names = {s: "stack_K%d_r%d" % s for s in STACKS}
    for rep in range(WARMUP + REPS):
        data = draw(m, gen, dev)
        x0 = torch.randn(B, DIN + 3, generator=gen, device=dev).to(BF)[:, :DIN]
        dy = torch.randn(B, DIN + 3, generator=gen, device=dev).to(BF)[:, :DIN]
        jobs = []
        for s in STACKS:
            def stack(ws=weights[s]):
                x = x0.detach().requires_grad_()
                dense.cross_mix(x, ws).backward(dy)
                for l in ws:
                    for w in l:
                        if w is not None:
                            w.grad = None

            jobs.append((names[s], "stack", stack, None))
            jobs.append((names[s], "forward", forwards[s][0], "forward"))
            jobs.append((names[s], "forward", forwards[s][2], "backward"))
        jobs += [("forward_B%d" % b, "forward", fn, "forward") for b, fn in by_batch.items()]
        jobs.append(("train_step", "train_step", lambda: m.train_step(data), None))
        jobs.append(("dcnv2_train_step", "train_step", lambda: v2.train_step(data), "fused"))
        for name, kind, fn, single in jobs:
            for key, us in timed(name, kind, fn, single):
                if rep >= WARMUP:
                    times.setdefault(key, []).append(us)
    dense.CROSS_MIX_FUSED = True

    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy = json.load(f)["stream_copy"]
    copy_bps = copy["bytes_moved"] / (copy["us"] * 1e-6)
    res = {"B": B, "d": DIN, "layers": NL, "rows_per_table": ROWS, "n_dense": N_DENSE, "mlp": LAYERS,
           "dtype": "bf16", "tile_rows": 16, "warmup": WARMUP, "reps": REPS, "groups": GROUPS, "inner": INNER,
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
        if (name, "forward") in times:
            s = [k for k in STACKS if names[k] == name][0]
            fw = row["forward"] = summarise(times[(name, "forward")])
            fw["what"] = "mrec_cross_mix_fwd (training: saved stack and x_L written), bf16 x0"
            fw["algorithmic_bytes"] = forwards[s][1]
            fw["stream_copy_us"] = forwards[s][1] / copy_bps * 1e6
            fw["fraction_of_stream_copy"] = fw["stream_copy_us"] / fw["median_us"]
            row["backward"] = summarise(times[(name, "backward")])
            row["backward"]["what"] = "mrec_cross_mix_bwd alone (dx0 and the weight gradients' operands)"
            extra = (f", forward alone {fw['median_us']:.1f} us = {fw['fraction_of_stream_copy']:.3f} of stream copy"
                     f", backward launch alone {row['backward']['median_us']:.1f} us")
        if name == "train_step":
            row["dcnv2_train_step"] = summarise(times[("dcnv2_train_step", "fused")])
            extra = f", dcnv2 step {row['dcnv2_train_step']['median_us']:.1f} us"
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}] "
            f"spread {row[p]['spread_us']:.1f}" for p in PATHS)
            + f", speedup {row['speedup_median']:.2f}x, faster: {row['fused_is_faster']}" + extra, flush=True)
    # what the 16-row tile costs: the forward launch of the first stack at half a tile, one tile
    # and two tiles per CU (the weight images are read once per tile)
    res["forward_by_batch"] = {str(b): summarise(times[("forward_B%d" % b, "forward")]) for b in TILE_BATCHES}
    print("forward alone by batch: " + ", ".join(
        f"B = {b}: {v['median_us']:.1f} us" for b, v in res["forward_by_batch"].items()), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_dcnmix.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
