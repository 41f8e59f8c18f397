"""Time the fused shared-negative losses (mrec_shneg_loss_fwd / _bwd behind
``loss.SharedNegativeLoss``) against the same contract in torch ops, on the GPU (fails
without one), and a GRU4Rec train step with a shared pool against its pair-wise step.

Loss alone.  B = 4096 queries, D = 64, fp32 queries, bf16 rows, S in {1024, 4096, 65,536}
negatives, N(0, 0.35^2) operands (scores of a few units), all three kinds, no ids.  Two
paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions:
  fused  SharedNegativeLoss -> the kernels of csrc/shneg.hip (the [B, S] scores never
         reach memory);
  torch  SharedNegativeLoss with ``fused = False`` -> ``cpu_path.shared_negative_loss`` on
         the device: the [B, S] fp32 matrix written and re-read by each op.
``fwd`` is the loss under ``no_grad``, ``fwd_bwd`` the loss and its backward to q, pos, neg.
Before timing, the two paths' losses and gradients are compared at every shape.

Train step.  GRU4Rec at B = 4096, L = 50, E = H = 64 on 63,002 items, plain SGD:
``set_shared_negatives(sampler, 4096)`` with ``softmax_shared`` against the same model's
pair-wise step, ``set_negative_sampler(sampler, 1)`` with BPR -- what 4096 negatives cost
over one.

Writes <out>/bench_shneg.json (default profiles/shneg) with every median, the ratios, the
split count and the algorithmic work (2 B S D flop per product: one forward, four
backward; operand bytes (B + S) D).  ``--probe`` measures the device functions the losses
call against fp64 (``mrec_shneg_math_probe``: the tests' EPS_F) and writes
<out>/math_probe.json.  ``--rehearse`` runs the script's own logic at a toy size on the
CPU; it times nothing and writes nothing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import _mrec  # noqa: E402
from pytorchrec_amd.loss import BPRLoss, SharedNegativeLoss, shneg_default_splits  # noqa: E402

B, D = 4096, 64
POOLS = (1024, 4096, 65536)
KINDS = ("softmax", "bpr", "top1")
WARMUP, REPS = 3, 10
PATHS = ("fused", "torch")
L, E, H, ITEMS, S_STEP = 50, 64, 64, 63002, 4096


def operands(S, dev, gen, batch=B, dim=D):
    q = torch.randn(batch, dim, generator=gen, device=dev) * 0.35
    pos = (torch.randn(batch, dim, generator=gen, device=dev) * 0.35).to(torch.bfloat16)
    neg = (torch.randn(S, dim, generator=gen, device=dev) * 0.35).to(torch.bfloat16)
    return q, pos, neg


def make(kind, fused):
    loss = SharedNegativeLoss(kind)
    loss.fused = fused
    return loss


def fwd(loss, q, pos, neg):
    with torch.no_grad():
        return loss(q, pos, neg)


def fwd_bwd(loss, q, pos, neg):
    q, pos, neg = (t.detach().requires_grad_() for t in (q, pos, neg))
    out = loss(q, pos, neg)
    out.backward()
    return out.detach(), q.grad, pos.grad, neg.grad


def compare(kind, q, pos, neg):
    """Both paths on the same inputs -> the largest difference of each result over the
    result's largest magnitude (the fused coefficients and the bf16 outputs are rounded to
    bf16: 2^-9 relative each)."""
    a, b = fwd_bwd(make(kind, True), q, pos, neg), fwd_bwd(make(kind, False), q, pos, neg)
    out = {}
    for name, x, y in zip(("loss", "dq", "dpos", "dneg"), a, b):
        out[name] = float((x.double() - y.double()).abs().max() / y.double().abs().max().clamp(min=1e-30))
    assert out["loss"] < 1e-4 and max(out["dq"], out["dpos"], out["dneg"]) < 2e-2, out
    return out


def timed(fns, order_rng, warmup=WARMUP, reps=REPS):
    times = {p: [] for p in fns}
    for rep in range(warmup + reps):
        for path in order_rng.permutation(list(fns)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[path]()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[path].append(e0.elapsed_time(e1) * 1e3)
    out = {}
    for p, t in times.items():
        t = np.array(t)
        out[p] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
                  "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90))}
    return out


def build_gru(dev):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import GRU4Rec
    m = GRU4Rec(CategoricalColumnWithIdentity(ITEMS, "iid"), CategoricalColumnWithIdentity(L + 1, "his_len"),
                CategoricalColumnWithIdentity(ITEMS, "his"), CategoricalColumnWithIdentity(2, "label"),
                emb_size=E, hidden_size=H, device=dev, random_seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g).to(dev))
    m.i_embeddings.check_ids = False
    return m


def draw_sessions(gen, dev, batch=B, items=ITEMS, length=L):
    lens = torch.randint(1, length + 1, (batch,), generator=gen, device=dev)
    his = torch.randint(1, items, (batch, length), generator=gen, device=dev)
    his = his * (torch.arange(length, device=dev)[None, :] < lens[:, None])
    return {"his": his, "his_len": lens, "iid": torch.randint(1, items, (batch,), generator=gen, device=dev),
            "uid": torch.arange(batch, device=dev)}


def train_steps(dev, gen, order_rng):
    from pytorchrec_amd.sampling import NegativeSampler
    data = draw_sessions(gen, dev)
    sampler = NegativeSampler(data["uid"], data["iid"], 1, ITEMS, seed=5, device=dev)
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    ucol = CategoricalColumnWithIdentity(B, "uid")
    shared, pair = build_gru(dev), build_gru(dev)
    shared.compile(torch.optim.SGD(shared.get_parameters(), lr=0.01), SharedNegativeLoss("softmax"), [], dev)
    shared.set_shared_negatives(sampler, S_STEP)
    pair.compile(torch.optim.SGD(pair.get_parameters(), lr=0.01), BPRLoss(), [], dev)
    pair.set_negative_sampler(sampler, n_neg=1, uid_column=ucol)
    t = timed({"shared_4096": lambda: shared.train_step(data), "pairwise_1": lambda: pair.train_step(data)},
              order_rng)
    t["shared_over_pairwise_median"] = t["shared_4096"]["median_us"] / t["pairwise_1"]["median_us"]
    return t


def probe(out_dir):
    dev = torch.device("cuda")
    names = ["expf", "logf", "softplus", "sigmoid", "dsigmoid"]
    res = {"device": torch.cuda.get_device_name(0), "n": 1 << 22, "unit": "2^-24", "functions": {}}
    for fn, name in enumerate(names):
        lo, hi = (-170.0, 20.0) if fn == 0 else (1e-3, 1e6) if fn == 1 else (-170.0, 170.0)
        g = torch.Generator().manual_seed(fn)
        u = torch.rand(res["n"], dtype=torch.float64, generator=g)
        x = (torch.exp(u * (np.log(hi) - np.log(lo)) + np.log(lo)) if fn == 1 else u * (hi - lo) + lo).float()
        xd = x.to(dev)
        y = torch.empty_like(xd)
        _mrec.call("mrec_shneg_math_probe", fn, xd.data_ptr(), xd.numel(), y.data_ptr(), _mrec.stream_handle(dev))
        x64 = x.double()
        want = [torch.exp(x64), torch.log(x64), torch.nn.functional.softplus(x64, threshold=1e9),
                torch.sigmoid(x64), torch.sigmoid(x64) * torch.sigmoid(-x64)][fn]
        ok = want.abs() > 2.0 ** -126  # results in fp32's normal range
        rel = ((y.cpu().double() - want).abs() / want.abs())[ok]
        res["functions"][name] = {"range": [lo, hi], "max_rel_err": float(rel.max()),
                                  "max_rel_err_units": float(rel.max()) * 2.0 ** 24}
        print(f"{name}: worst relative error {res['functions'][name]['max_rel_err_units']:.2f} x 2^-24", flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "math_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def rehearse():
    gen = torch.Generator().manual_seed(1)
    q, pos, neg = operands(50, torch.device("cpu"), gen, batch=20, dim=8)
    for kind in KINDS:
        out = fwd_bwd(make(kind, True), q, pos, neg)  # (a CPU tensor takes the torch path)
        assert all(bool(torch.isfinite(t.float()).all()) for t in out)
        assert torch.equal(fwd(make(kind, False), q, pos, neg), out[0])
    print("rehearsal ok (torch path at a toy size on the CPU; nothing timed)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shneg"))
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--probe", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shneg.py needs a GPU")
    if args.probe:
        return probe(args.out)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(3)
    order_rng = np.random.default_rng(4)
    lib = _mrec.lib()
    res = {"B": B, "D": D, "q_dtype": "float32", "row_dtype": "bfloat16", "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "tile_queries": int(lib.mrec_shneg_tile_queries()),
           "tile_candidates": int(lib.mrec_shneg_tile_candidates()), "loss": []}
    for S in POOLS:
        q, pos, neg = operands(S, dev, gen)
        for kind in KINDS:
            row = {"S": S, "kind": kind, "splits": shneg_default_splits(B, S), "flop_per_product": 2 * B * S * D,
                   "operand_bytes": B * D * 4 + (B + S) * D * 2, "score_matrix_bytes_fp32": B * S * 4,
                   "max_rel_diff_fused_vs_torch": compare(kind, q, pos, neg)}
            f, t = make(kind, True), make(kind, False)
            row["fwd"] = timed({"fused": lambda: fwd(f, q, pos, neg), "torch": lambda: fwd(t, q, pos, neg)}, order_rng)
            row["fwd_bwd"] = timed({"fused": lambda: fwd_bwd(f, q, pos, neg),
                                    "torch": lambda: fwd_bwd(t, q, pos, neg)}, order_rng)
            for mode in ("fwd", "fwd_bwd"):
                row[mode]["torch_over_fused_median"] = row[mode]["torch"]["median_us"] / row[mode]["fused"]["median_us"]
            row["fused_fwd_bwd_faster"] = row["fwd_bwd"]["torch_over_fused_median"] > 1.0
            res["loss"].append(row)
            print(f"S {S} {kind}: " + ", ".join(
                f"{mode} fused {row[mode]['fused']['median_us']:.0f} us torch {row[mode]['torch']['median_us']:.0f} us "
                f"({row[mode]['torch_over_fused_median']:.2f}x)" for mode in ("fwd", "fwd_bwd")), flush=True)
            torch.cuda.empty_cache()
        del q, pos, neg
    res["gru4rec_train_step"] = dict(train_steps(dev, gen, order_rng), B=B, L=L, E=E, H=H, items=ITEMS,
                                     shared_negatives=S_STEP, shared_loss="softmax_shared", pairwise_loss="bpr")
    ts = res["gru4rec_train_step"]
    print(f"gru4rec step: shared {ts['shared_4096']['median_us']:.0f} us, pair-wise {ts['pairwise_1']['median_us']:.0f} us "
          f"({ts['shared_over_pairwise_median']:.2f}x)", flush=True)
    res["fused_fwd_bwd_faster_at_4096_and_65536"] = all(r["fused_fwd_bwd_faster"] for r in res["loss"] if r["S"] >= 4096)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_shneg.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
