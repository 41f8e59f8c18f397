"""Time the fused SASRec encoder against the layered path it replaces, on the GPU (fails
without one).

Shapes: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded),
D = 64, 2 layers, N = 100 candidates per sample, a 63,002-row fp32 item table, weights at
lively scale (N(0, 0.3)).

Two paths, in one process, alternating, by device events after warm-up, the median over
the repetitions:
  fused    dense.sasrec_encode -> mrec_sasrec_fwd (+ mrec_sasrec_bwd + mrec_sasrec_wgrad);
  layered  the same arithmetic as stock torch ops (cpu_path.sasrec_encode with the
           kernel's bf16 rounding points): what the reference's forward runs on this GPU.
Four measurements per path:
  encode_fwd       the encoder alone on gathered rows, no autograd;
  encode_fwd_bwd   encoder forward + backward (rows' gradient and the nine dense ones);
  model_fwd        SASRec.forward in eval mode: gather + encoder + the N candidate dots;
  model_fwd_bwd    SASRec.forward + backward of a scalar loss, fused-SGD item table.

Writes <out>/bench_sasrec.json (default profiles/sasrec) with the algorithmic bytes of
the fused encoder: forward reads the [L, D] bf16 rows and writes layers x [L, D] bf16
outputs + [D] fp32 per sample; backward reads the rows and (layers - 1) saved outputs
and writes the [L, D] bf16 gradient.
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
from pytorchrec_amd.model import SASRec  # noqa: E402

B, L, D, LAYERS, N, ITEMS = 4096, 50, 64, 2, 100, 63002
WARMUP, REPS = 5, 30


def build(dev):
    m = SASRec(CategoricalColumnWithIdentity(ITEMS, "iid"),
               CategoricalColumnWithIdentity(L + 1, "his_len"),
               CategoricalColumnWithIdentity(ITEMS, "his"), None, emb_size=D, max_his_len=L,
               num_layers=LAYERS, dropout=0.0, device=dev, random_seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in m.parameters():
            n = torch.randn(p.shape, generator=g).to(dev)
            p.copy_(0.3 * n)
        m.layer_norm.weight.add_(1.0)
    m.i_embeddings.use_fused_sgd(0.01)
    m.i_embeddings.check_ids = False
    return m


def draw(gen, dev):
    lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev)
    his = torch.randint(1, ITEMS, (B, L), generator=gen, device=dev)
    his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
    iid = torch.randint(1, ITEMS, (B, N), generator=gen, device=dev)
    return {"his": his, "his_len": lens, "iid": iid}


def steps(m, batch, rows, dv):
    def encode_fwd():
        with torch.no_grad():
            dense.sasrec_encode(rows, batch["his"], batch["his_len"], m)

    def encode_fwd_bwd():
        x = rows.detach().requires_grad_()
        dense.sasrec_encode(x, batch["his"], batch["his_len"], m).backward(dv)

    def model_fwd():
        with torch.no_grad():
            m(batch)

    def model_fwd_bwd():
        m(batch)[0].square().mean().backward()

    return {"encode_fwd": encode_fwd, "encode_fwd_bwd": encode_fwd_bwd, "model_fwd": model_fwd,
            "model_fwd_bwd": model_fwd_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sasrec"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sasrec.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(3)
    dv = torch.randn(B, D, generator=gen, device=dev)
    times = {}
    for rep in range(WARMUP + REPS):
        batch = draw(gen, dev)
        rows = (0.3 * torch.randn(B, L, D, generator=gen, device=dev)).to(torch.bfloat16)
        for name, fn in steps(m, batch, rows, dv).items():
            for path in ("fused", "layered"):  # alternating, on the same inputs
                dense.SASREC_FUSED = path == "fused"
                for p in m.parameters():
                    p.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times.setdefault((name, path), []).append(e0.elapsed_time(e1) * 1e3)
    dense.SASREC_FUSED = True
    fwd_bytes = B * (L * D * 2 * (1 + LAYERS) + L * 4 + D * 4)
    bwd_bytes = B * (L * D * 2 * (1 + LAYERS - 1) + L * D * 2 + L * 4 + D * 4)
    res = {"B": B, "L": L, "D": D, "layers": LAYERS, "N": N, "items": ITEMS, "warmup": WARMUP,
           "reps": REPS, "timing": "device events around each call, host-launched, alternating",
           "device": torch.cuda.get_device_name(0), "fused_model_bytes_fwd": fwd_bytes,
           "fused_model_bytes_bwd": bwd_bytes, "measurements": {}}
    for name in ("encode_fwd", "encode_fwd_bwd", "model_fwd", "model_fwd_bwd"):
        row = {}
        for path in ("fused", "layered"):
            t = np.array(times[(name, path)])
            row[path] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                         "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                         "p90_us": float(np.percentile(t, 90))}
        row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
        res["measurements"][name] = row
        print(f"{name}: fused {row['fused']['median_us']:.1f} us [{row['fused']['min_us']:.1f}, "
              f"{row['fused']['max_us']:.1f}], layered {row['layered']['median_us']:.1f} us "
              f"[{row['layered']['min_us']:.1f}, {row['layered']['max_us']:.1f}], "
              f"x{row['speedup_median']:.2f}")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_sasrec.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
