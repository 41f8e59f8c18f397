"""Time the fused GRU4Rec encoder against the layered path it replaces, on the GPU (fails
without one).

Shapes: B = 4096 histories of L = 50 positions (lengths uniform in 1..50, tail-padded),
E = H = 64, N = 100 candidates per sample, a 63,002-row fp32 item table, the GRU weights
at lively scale (N(0, 0.3)).

Four paths, in one process, alternating, by device events after warm-up, the median over
the repetitions:
  fused          dense.gru_encode -> mrec_gru_fwd (+ mrec_gru_bwd + mrec_sasrec_wgrad) with
                 the default tile order ("auto": sorted by length only when the batch has
                 more tiles than workgroups; at B = 4096 that is the batch order);
  fused_sorted   the same kernels, the tiles filled with the samples sorted by length
                 (order = argsort(his_len, descending), the sort included in the time);
  fused_unsorted the same kernels with the tiles in batch order (order = NULL);
  layered        the same arithmetic as stock torch ops (cpu_path.gru_encode with the
                 kernel's bf16 rounding points): L dependent steps of small GEMMs and
                 pointwise kernels.
Four measurements per path:
  encode_fwd       the recurrence alone on gathered rows, no autograd;
  encode_fwd_bwd   recurrence forward + backward (rows' gradient and the four dense ones);
  model_fwd        GRU4Rec.forward in eval mode: gather + recurrence + out + the N dots;
  train_step       GRU4Rec.train_step (MSE, SGD): forward, backward, every update.
The encoder's forward + backward is also timed at B = 16384 (1024 tiles, four per
workgroup on 256 CUs), fused paths only: the shape at which the tile order matters.

Writes <out>/bench_gru4rec.json (default profiles/gru4rec) with the algorithmic bytes of
the fused encoder over the live positions: forward reads the [E] bf16 row and writes the
[H] fp32 hidden state per live position, plus [H] fp32 per sample; backward reads the row
and the saved state, and writes the [E] bf16 gradient, per live position (the gradient
also at dead positions, as zeros).
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
from pytorchrec_amd.model import GRU4Rec  # noqa: E402

B, L, E, H, N, ITEMS = 4096, 50, 64, 64, 100, 63002
WARMUP, REPS = 5, 30
PATHS = ("fused", "fused_sorted", "fused_unsorted", "layered")
ORDER = {"fused": "auto", "fused_sorted": "sorted", "fused_unsorted": None, "layered": "auto"}
B_LARGE = 4 * B


def build(dev):
    m = GRU4Rec(CategoricalColumnWithIdentity(ITEMS, "iid"),
                CategoricalColumnWithIdentity(L + 1, "his_len"),
                CategoricalColumnWithIdentity(ITEMS, "his"),
                CategoricalColumnWithIdentity(2, "label"), emb_size=E, hidden_size=H, device=dev,
                random_seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g).to(dev))
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), torch.nn.MSELoss(), [], dev)
    m.i_embeddings.check_ids = False
    return m


def draw(gen, dev, B=B):
    lens = torch.randint(1, L + 1, (B,), generator=gen, device=dev)
    his = torch.randint(1, ITEMS, (B, L), generator=gen, device=dev)
    his = his * (torch.arange(L, device=dev)[None, :] < lens[:, None])
    iid = torch.randint(1, ITEMS, (B, N), generator=gen, device=dev)
    label = torch.zeros(B, N, dtype=torch.int64, device=dev)
    label[:, 0] = 1
    return {"his": his, "his_len": lens, "iid": iid, "label": label}


def steps(m, batch, rows, dh, big):
    def encode_fwd():
        with torch.no_grad():
            dense.gru_encode(rows, batch["his_len"], m, order=m.tile_order)

    def encode_fwd_bwd():
        x = rows.detach().requires_grad_()
        dense.gru_encode(x, batch["his_len"], m, order=m.tile_order).backward(dh)

    def encode_fwd_bwd_large():
        x = big[0].detach().requires_grad_()
        dense.gru_encode(x, big[1], m, order=m.tile_order).backward(big[2])

    def model_fwd():
        with torch.no_grad():
            m.eval()(batch)

    def train_step():
        m.train_step(batch)

    return {"encode_fwd": encode_fwd, "encode_fwd_bwd": encode_fwd_bwd, "model_fwd": model_fwd,
            "train_step": train_step, "encode_fwd_bwd_large": encode_fwd_bwd_large}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru4rec"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru4rec.py needs a GPU")
    dev = torch.device("cuda")
    m = build(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    dh = torch.randn(B, H, generator=gen, device=dev)
    times, live = {}, []
    order_rng = np.random.default_rng(4)
    for rep in range(WARMUP + REPS):
        batch = draw(gen, dev)
        live.append(int(batch["his_len"].sum()))
        rows = (0.3 * torch.randn(B, L, E, generator=gen, device=dev)).to(torch.bfloat16)
        big = ((0.3 * torch.randn(B_LARGE, L, E, generator=gen, device=dev)).to(torch.bfloat16),
               draw(gen, dev, B_LARGE)["his_len"],
               torch.randn(B_LARGE, H, generator=gen, device=dev))
        for name, fn in steps(m, batch, rows, dh, big).items():
            # alternating, on the same inputs, in a fresh random order each time: the path
            # that runs first after fresh inputs, or right after the 18 ms of small layered
            # kernels, measured up to 2x slower than the same code elsewhere in the order
            for path in order_rng.permutation(PATHS):
                if name == "encode_fwd_bwd_large" and path == "layered":
                    continue
                dense.GRU_FUSED = path != "layered"
                m.tile_order = ORDER[path]
                for p in m.parameters():
                    p.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times.setdefault((name, path), []).append(e0.elapsed_time(e1) * 1e3)
    dense.GRU_FUSED, m.tile_order = True, "auto"
    live_mean = float(np.mean(live))
    fwd_bytes = int(live_mean * (E * 2 + H * 4) + B * (H * 4 + 4))
    bwd_bytes = int(live_mean * (E * 2 + 2 * H * 4) + B * L * E * 2 + B * (H * 4 + 4))
    res = {"B": B, "B_large": B_LARGE, "L": L, "E": E, "H": H, "N": N, "items": ITEMS,
           "warmup": WARMUP, "reps": REPS,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "live_positions_mean": live_mean,
           "fused_model_bytes_fwd": fwd_bytes, "fused_model_bytes_bwd": bwd_bytes,
           "measurements": {}}
    for name in ("encode_fwd", "encode_fwd_bwd", "model_fwd", "train_step", "encode_fwd_bwd_large"):
        row = {}
        for path in PATHS:
            if (name, path) not in times:
                continue
            t = np.array(times[(name, path)])
            row[path] = {"median_us": float(np.median(t)), "min_us": float(t.min()),
                         "max_us": float(t.max()), "p10_us": float(np.percentile(t, 10)),
                         "p90_us": float(np.percentile(t, 90))}
        if "layered" in row:
            row["speedup_median"] = row["layered"]["median_us"] / row["fused"]["median_us"]
        row["unsorted_over_sorted"] = (row["fused_unsorted"]["median_us"]
                                       / row["fused_sorted"]["median_us"])
        res["measurements"][name] = row
        print(f"{name}: " + ", ".join(
            f"{p} {row[p]['median_us']:.1f} us [{row[p]['min_us']:.1f}, {row[p]['max_us']:.1f}]"
            for p in PATHS if p in row))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_gru4rec.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
