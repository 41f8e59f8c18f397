"""Time the fused HSTU encoder against the layered path it replaces, on the GPU (fails
without one), with the fused SASRec pair at the same shape as a second yardstick.

Shape: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded),
D = 64, H = 2 heads, 2 layers, a 63,002-row fp32 item table, lively weights (projections
N(0, 1/sqrt(D)), LayerNorm gains 1 + 0.2 N, biases and rab 0.2 N).

Paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median over the repetitions:
  fused    dense.hstu_encode -> mrec_hstu_fwd (+ mrec_hstu_bwd + mrec_sasrec_wgrad);
  layered  the same arithmetic as stock torch ops (cpu_path.hstu_encode with the kernel's
           bf16 rounding points): per layer a LayerNorm, a GEMM, a SiLU, two batched
           matmuls over the [B, H, L, L] scores, a mask, a LayerNorm, a product, a GEMM, an add;
  sasrec   dense.sasrec_encode -> mrec_sasrec_fwd / _bwd, 2 layers of the shared block
           (encoder measurements only).
Measurements:
  encode_fwd      the encoder alone on gathered rows, no autograd;
  encode_fwd_bwd  encoder forward + backward (the rows' gradient and every dense one);
  train_step      HSTU.train_step with ``softmax_shared`` over 4096 shared negatives, SGD.

Writes <out>/bench_hstu.json (default profiles/hstu) with the forward launch's algorithmic
bytes (the live rows read once, every layer's [B, L, D] bf16 output written once and read
once by the next layer, v written) and their time at the stream-copy rate of
profiles/ceilings.json.
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
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity  # noqa: E402
from pytorchrec_amd.loss import SharedNegativeLoss  # noqa: E402
from pytorchrec_amd.model import HSTU, SASRec  # noqa: E402
from pytorchrec_amd.sampling import NegativeSampler  # noqa: E402

B, L, D, H, LAYERS, ITEMS, SHARED = 4096, 50, 64, 2, 2, 63002, 4096
WARMUP, REPS = 5, 30


def build(cls, dev, **kw):
    m = cls(CategoricalColumnWithIdentity(ITEMS, "iid"), CategoricalColumnWithIdentity(L + 1, "his_len"),
            CategoricalColumnWithIdentity(ITEMS, "his"), CategoricalColumnWithIdentity(2, "label"),
            emb_size=D, max_his_len=L, num_layers=LAYERS, device=dev, random_seed=1, **kw)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("i_embeddings"):
                continue
            n = torch.randn(p.shape, generator=g)
            if "norm" in name and name.endswith("weight"):
                n = 1.0 + 0.2 * n
            elif name in ("uvqk_weight", "out_weight", "Q.weight", "K.weight", "W1.weight", "W2.weight"):
                n = D ** -0.5 * n
            else:
                n = 0.2 * n
            p.copy_(n.to(dev))
    m.i_embeddings.check_ids = False
    return m


def draw(gen, dev):
    lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev)
    his = torch.randint(1, ITEMS, (B, L), generator=gen, device=dev)
    his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
    return {"his": his, "his_len": lens, "iid": torch.randint(1, ITEMS, (B,), generator=gen, device=dev),
            "uid": torch.arange(B, device=dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hstu"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hstu.py needs a GPU")
    dev = torch.device("cuda")
    hstu, sas = build(HSTU, dev, num_heads=H), build(SASRec, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    first = draw(gen, dev)
    sampler = NegativeSampler(first["uid"], first["iid"], 1, ITEMS, seed=5, device=dev)
    hstu.compile(torch.optim.SGD(hstu.get_parameters(), lr=0.01), SharedNegativeLoss("softmax"), [], dev)
    hstu.set_shared_negatives(sampler, SHARED)
    dv = torch.randn(B, D, generator=gen, device=dev)
    encoders = {"fused": (hstu, dense.hstu_encode), "layered": (hstu, dense.hstu_encode),
                "sasrec": (sas, dense.sasrec_encode)}
    times, live = {}, []
    order_rng = np.random.default_rng(4)
    for rep in range(WARMUP + REPS):
        batch = draw(gen, dev)
        live.append(int(batch["his_len"].sum()))
        rows = (0.3 * torch.randn(B, L, D, generator=gen, device=dev)).to(torch.bfloat16)

        def encode_fwd(m, fn):
            with torch.no_grad():
                fn(rows, batch["his"], batch["his_len"], m.eval())

        def encode_fwd_bwd(m, fn):
            x = rows.detach().requires_grad_()
            fn(x, batch["his"], batch["his_len"], m.eval()).backward(dv)

        def train_step(m, fn):
            m.train_step(batch)

        for name, step in (("encode_fwd", encode_fwd), ("encode_fwd_bwd", encode_fwd_bwd),
                           ("train_step", train_step)):
            for path in order_rng.permutation(list(encoders)):
                if name == "train_step" and path == "sasrec":
                    continue
                dense.HSTU_FUSED = path != "layered"
                m, fn = encoders[path]
                for p in m.parameters():
                    p.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(m, fn)
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times.setdefault((name, path), []).append(e0.elapsed_time(e1) * 1e3)
    dense.HSTU_FUSED = True
    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy_gbs = json.load(f)["stream_copy"]["GB/s"]
    live_mean = float(np.mean(live))
    fwd_bytes = int(live_mean * D * 2 + (2 * LAYERS - 1) * B * L * D * 2 + B * D * 4)
    res = {"B": B, "L": L, "D": D, "H": H, "layers": LAYERS, "items": ITEMS, "shared_negatives": SHARED,
           "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "live_positions_mean": live_mean,
           "fused_model_bytes_fwd": fwd_bytes, "stream_copy_GB/s": copy_gbs,
           "fwd_bytes_at_stream_copy_us": fwd_bytes / (copy_gbs * 1e3), "measurements": {}}
    for name in ("encode_fwd", "encode_fwd_bwd", "train_step"):
        row = {}
        for path in encoders:
            if (name, path) in times:
                t = np.array(times[(name, path)])
                row[path] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                             "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                             "p90_us": float(np.percentile(t, 90))}
        row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
        if "sasrec" in row:
            row["fused_over_sasrec_median"] = row["fused"]["median_us"] / row["sasrec"]["median_us"]
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(f"{p} {row[p]['median_us']:.1f} us" for p in encoders if p in row))
    res["fwd_share_of_stream_copy_ceiling"] = (res["fwd_bytes_at_stream_copy_us"]
                                               / res["measurements"]["encode_fwd"]["fused"]["median_us"])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_hstu.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
