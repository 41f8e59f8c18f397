"""Time the fused NCF pair scorer against the layered path it replaces, on the GPU (fails
without one).

Shapes: the NeuMF tower E = 64, layers [128, 64, 32]; 200,000 users and 63,002 items in one
fp32 four-table bank; the dense weights at lively scale (N(0, 0.3)).
  eval    B = 4096 samples of N = 100 candidates (leave-one-out evaluation): 409,600 pairs,
          forward only;
  train   B = 4096 samples of N = 2 (pair-wise training: the positive and one negative):
          8,192 pairs, forward + backward.

Two paths, in one process, alternating in a fresh random order, by device events after
warm-up, the median over the repetitions:
  fused    dense.ncf_score -> mrec_ncf_fwd (+ mrec_ncf_bwd + mrec_sasrec_wgrad);
  layered  the same arithmetic as stock torch ops (cpu_path.ncf_score with the kernel's
           bf16 rounding points): one GEMM per layer and pointwise kernels in between.
Two measurements per shape: the scorer alone on gathered rows, and the whole model
(``NCF.forward`` in eval mode: gather + scorer; ``NCF.train_step`` with BPR and SGD:
forward, backward, every update).

Writes <out>/bench_ncf.json (default profiles/ncf) with the algorithmic bytes of the fused
scorer: forward reads the [4E] bf16 row and writes one fp32 per pair; backward reads the
row and dpred and writes the [4E] bf16 gradient per pair, plus one fp32 partial of the
dense gradients per workgroup.
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
from pytorchrec_amd.loss import BPRLoss  # noqa: E402
from pytorchrec_amd.model import NCF  # noqa: E402

B, E, LAYERS, USERS, ITEMS = 4096, 64, [128, 64, 32], 200000, 63002
N_EVAL, N_TRAIN = 100, 2
WARMUP, REPS = 5, 30
PATHS = ("fused", "layered")


def build(dev):
    m = NCF(CategoricalColumnWithIdentity(USERS, "uid"), CategoricalColumnWithIdentity(ITEMS, "iid"),
            CategoricalColumnWithIdentity(2, "label"), emb_size=E, layers=LAYERS, dropout=0.0,
            device=dev, random_seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g).to(dev))
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BPRLoss(), [], dev)
    m.embeddings.check_ids = False
    return m


def draw(gen, dev, n):
    return {"uid": torch.randint(0, USERS, (B,), generator=gen, device=dev),
            "iid": torch.randint(0, ITEMS, (B, n), generator=gen, device=dev)}


def steps(m, ev, tr, rows_ev, rows_tr, dpred):
    def eval_score_fwd():
        with torch.no_grad():
            dense.ncf_score(rows_ev, m.eval())

    def eval_model_fwd():
        with torch.no_grad():
            m.eval()(ev)

    def train_score_fwd_bwd():
        x = rows_tr.detach().requires_grad_()
        dense.ncf_score(x, m.eval()).backward(dpred)

    def train_step():
        m.train_step(tr)

    return {"eval_score_fwd": eval_score_fwd, "eval_model_fwd": eval_model_fwd,
            "train_score_fwd_bwd": train_score_fwd_bwd, "train_step": train_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncf"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ncf.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev)
    assert dense.ncf_supported(E, LAYERS)
    gen = torch.Generator(device=dev).manual_seed(3)
    dpred = torch.randn(B * N_TRAIN, generator=gen, device=dev)
    times = {}
    order_rng = np.random.default_rng(4)
    for rep in range(WARMUP + REPS):
        ev, tr = draw(gen, dev, N_EVAL), draw(gen, dev, N_TRAIN)
        rows_ev = (0.3 * torch.randn(B * N_EVAL, 4 * E, generator=gen, device=dev)).to(torch.bfloat16)
        rows_tr = (0.3 * torch.randn(B * N_TRAIN, 4 * E, generator=gen, device=dev)).to(torch.bfloat16)
        for name, fn in steps(m, ev, tr, rows_ev, rows_tr, dpred).items():
            for path in order_rng.permutation(PATHS):
                dense.NCF_FUSED = path == "fused"
                for p in m.parameters():
                    p.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times.setdefault((name, path), []).append(e0.elapsed_time(e1) * 1e3)
    dense.NCF_FUSED = True
    lib = _mrec.lib()
    P = int(lib.mrec_ncf_param_count(E, len(LAYERS), (ctypes.c_int32 * len(LAYERS))(*LAYERS)))
    pe, pt = B * N_EVAL, B * N_TRAIN
    res = {"B": B, "E": E, "layers": LAYERS, "N_eval": N_EVAL, "N_train": N_TRAIN, "users": USERS,
           "items": ITEMS, "pairs_eval": pe, "pairs_train": pt, "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "tile": int(lib.mrec_ncf_tile()),
           "fused_model_bytes_eval_fwd": pe * (4 * E * 2 + 4),
           "fused_model_bytes_train_fwd_bwd": (pt * (4 * E * 2 + 4) + pt * (2 * 4 * E * 2 + 4)
                                               + int(lib.mrec_ncf_parts(pt)) * P * 4),
           "measurements": {}}
    for name in ("eval_score_fwd", "eval_model_fwd", "train_score_fwd_bwd", "train_step"):
        row = {}
        for path in PATHS:
            t = np.array(times[(name, path)])
            row[path] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                         "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                         "p90_us": float(np.percentile(t, 90))}
        row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}]"
            for p in PATHS) + f", speedup {row['speedup_median']:.2f}x")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_ncf.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
