"""Time the fused DIEN interest evolution against the same contract in torch ops, and
against two plain GRU launches, on the GPU (fails without one).

Shapes: B = 4096 histories of L = 50 positions (lengths uniform in 1..50), at E = H = 32
(config C4's row width: item | category at emb_size 16) and E = H = 64; the eight
recurrent tensors at lively scale (N(0, 0.3)).

Per shape, in one process, alternating in a fresh random order on the same inputs, by
device events around each host-launched call after warm-up, the median over 40 repetitions
(12 of the layered path).  A call of 0.2 - 0.8 ms timed this way spreads by tens of percent
from call to call (launch and allocator time are inside it), so the ratios against ``gru``
hold to one digit; min, max, p10 and p90 are written beside each median:
  fused    dense.interest_evolution -> mrec_interest_fwd (+ mrec_interest_bwd +
           mrec_sasrec_wgrad);
  layered  cpu_path.interest_evolution on the GPU with the kernel's bf16 rounding points:
           2 L dependent steps of small GEMMs and pointwise kernels;
  gru      dense.gru_encode (mrec_gru_fwd / _bwd) at the same (B, L, E, H): one of the two
           recurrences, without attention, h_last only.  Two of these are the yardstick.
Two measurements per path: ``fwd`` (no autograd) and ``fwd_bwd`` (dv and d_hs1 random; every
gradient).  ``bwd`` is reported as their difference.
Then the DIEN train step (C4-shaped tables, emb_size 16, negative history, BCE + auxiliary
loss, SGD) with ``dense.DIEN_FUSED`` on and off.

Writes <out>/bench_dien.json (default profiles/dien).
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import dense  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as Col  # noqa: E402
from pytorchrec_amd.loss import BCEWithLogitsLoss  # noqa: E402
from pytorchrec_amd.model import DIEN  # noqa: E402

B, L, ITEMS, CATES = 4096, 50, 63002, 802
SHAPES = ((32, 32), (64, 64))
WARMUP, REPS, LAYERED_REPS = 3, 40, 12  # the layered path takes 40 ms a call: fewer of them
PATHS = ("fused", "layered", "gru")


def op_steps(E, H, gen, dev):
    shapes = [(3 * H, E), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,)]
    ws = [(0.3 * torch.randn(s, generator=gen, device=dev)).requires_grad_() for s in shapes]
    rnn = types.SimpleNamespace(weight_ih_l0=ws[0], weight_hh_l0=ws[1], bias_ih_l0=ws[2], bias_hh_l0=ws[3])
    gru_model = types.SimpleNamespace(rnn=rnn, i_embeddings=types.SimpleNamespace(check_ids=False))
    x = (0.3 * torch.randn(B, L, E, generator=gen, device=dev)).to(torch.bfloat16)
    lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev).to(torch.int32)
    p = 0.5 * torch.randn(B, H, generator=gen, device=dev)
    dv = torch.randn(B, H, generator=gen, device=dev)
    dh1 = torch.randn(B, L, H, generator=gen, device=dev)

    def fwd(path):
        with torch.no_grad():
            if path == "gru":
                dense.gru_encode(x, lens, gru_model)
            else:
                dense.interest_evolution(x, lens, p, ws, check=False)

    def fwd_bwd(path):
        for w in ws:
            w.grad = None
        xg = x.detach().requires_grad_()
        if path == "gru":
            dense.gru_encode(xg, lens, gru_model).backward(dv)
        else:
            v, hs1 = dense.interest_evolution(xg, lens, p.detach().requires_grad_(), ws, check=False)
            torch.autograd.backward([v, hs1], [dv, dh1])

    return {"fwd": fwd, "fwd_bwd": fwd_bwd}


def build_model(dev):
    m = DIEN(Col(ITEMS, "iid"), Col(CATES, "cid"), Col(ITEMS, "pos_his"), Col(CATES, "pos_his_cate"),
             Col(2, "label"), emb_size=16, layers=(200, 80), emb_dtype=torch.bfloat16, device=dev,
             neg_his_column=Col(ITEMS, "neg_his"), neg_his_cate_column=Col(CATES, "neg_his_cate"),
             random_seed=2020)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.05), BCEWithLogitsLoss(), [], dev)
    return m


def model_batch(gen, dev):
    lens = torch.randint(1, L + 1, (B, 1), generator=gen, device=dev)
    live = torch.arange(L, device=dev)[None] < lens
    d = {"iid": torch.randint(1, ITEMS, (B,), generator=gen, device=dev, dtype=torch.int32),
         "cid": torch.randint(1, CATES, (B,), generator=gen, device=dev, dtype=torch.int32)}
    for k, n in (("pos_his", ITEMS), ("pos_his_cate", CATES), ("neg_his", ITEMS), ("neg_his_cate", CATES)):
        d[k] = torch.randint(1, n, (B, L), generator=gen, device=dev, dtype=torch.int32) * live
    d["label"] = (torch.rand(B, generator=gen, device=dev) < 0.25).float()
    return d


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(t):
    t = np.array(t)
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dien"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dien.py needs a GPU")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(3)
    rng = np.random.default_rng(4)
    res = {"B": B, "L": L, "warmup": WARMUP, "reps": REPS, "layered_reps": LAYERED_REPS, "device": torch.cuda.get_device_name(0),
           "timing": "device events around each call, host-launched, alternating, random order",
           "op": {}, "train_step": {}}
    for E, H in SHAPES:
        times = {}
        fns = op_steps(E, H, gen, dev)
        for rep in range(WARMUP + REPS):
            for name, fn in fns.items():
                for path in rng.permutation(PATHS):
                    if path == "layered" and rep >= WARMUP + LAYERED_REPS:
                        continue
                    dense.DIEN_FUSED = path != "layered"
                    t = timed(fn, path)
                    if rep >= WARMUP:
                        times.setdefault((name, path), []).append(t)
        dense.DIEN_FUSED = True
        row = {name: {path: stats(times[(name, path)]) for path in PATHS} for name in fns}
        row["bwd_median_us"] = {path: row["fwd_bwd"][path]["median_us"] - row["fwd"][path]["median_us"]
                                for path in PATHS}
        row["speedup_fwd_bwd_median"] = (row["fwd_bwd"]["layered"]["median_us"]
                                         / row["fwd_bwd"]["fused"]["median_us"])
        row["fused_over_two_gru_fwd_bwd"] = (row["fwd_bwd"]["fused"]["median_us"]
                                             / (2 * row["fwd_bwd"]["gru"]["median_us"]))
        res["op"][f"E{E}_H{H}"] = row
        for name in fns:
            print(f"E={E} H={H} {name}: " + ", ".join(
                f"{path} {row[name][path]['median_us']:.1f} us" for path in PATHS))
    m = build_model(dev)
    times = {}
    for rep in range(WARMUP + REPS):
        batch = model_batch(gen, dev)
        for path in rng.permutation(("fused", "layered")):
            if path == "layered" and rep >= WARMUP + LAYERED_REPS:
                continue
            dense.DIEN_FUSED = path == "fused"
            t = timed(m.train_step, batch)
            if rep >= WARMUP:
                times.setdefault(path, []).append(t)
    dense.DIEN_FUSED = True
    res["train_step"] = {path: stats(t) for path, t in times.items()}
    res["train_step"]["speedup_median"] = (res["train_step"]["layered"]["median_us"]
                                           / res["train_step"]["fused"]["median_us"])
    print("train_step: " + ", ".join(f"{p} {res['train_step'][p]['median_us']:.1f} us"
                                     for p in ("fused", "layered")))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_dien.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
