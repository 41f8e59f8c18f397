"""Time LightGCN's fused propagation (mrec_graph_prop) against the torch-op path it
replaces, on the GPU (fails without one; there is no CPU fallback).

Graphs, seeded and synthetic (power-law user activity and item popularity, duplicates
removed), both at D = 64, K = 3:
  ml1m   6,040 users x 3,706 items, about 10^6 interactions: the node table fits in L2;
  large  10^5 users x 5 10^4 items, about 10^7 interactions: it does not.
Paths, in one process on the same inputs, alternating in a fresh random order, by device
events after warm-up, the median and the p10-p90 spread over the repetitions:
  fused       graph.propagate -> K launches of mrec_graph_prop, fp32 layers;
  fused_bf16  the same with the layers between the launches stored in bf16;
  sparse      graph.PROP_FUSED = False: per layer a torch.sparse.mm with A^ as a CSR tensor
              and an add, then a scale (values materialised once, outside the timing).
Measurements:
  prop_fwd      the propagation alone, no autograd;
  prop_fwd_bwd  propagation forward + backward;
  train_step    LightGCN.train_step, BPR with one negative per row at B = 4096, SGD.

Writes <out>/bench_lightgcn.json (default profiles/lightgcn) with the algorithmic bytes of
an average layer (per CSR entry a column id, a dinv and a source row; per node a dinv, the
running sum read and written, the next layer written) and their time at the stream-copy
rate of profiles/ceilings.json.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd import graph  # noqa: E402
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity  # noqa: E402
from pytorchrec_amd.loss import BPRLoss  # noqa: E402
from pytorchrec_amd.model import LightGCN  # noqa: E402

D, K, B = 64, 3, 4096
WARMUP, REPS = 5, 40
GRAPHS = {"ml1m": (6040, 3706, 1_000_000, 1.5), "large": (100_000, 50_000, 10_000_000, 1.18)}
PATHS = {"fused": (True, None), "fused_bf16": (True, torch.bfloat16), "sparse": (False, None)}


def power_law_interactions(n_users, n_items, n, spare, seed):
    """About ``n`` distinct pairs: users ~ rank^-0.5, items ~ rank^-0.9 (``spare`` times as
    many draws, for the duplicates the graph builder removes)."""
    gen = torch.Generator().manual_seed(seed)
    draws = int(n * spare)
    pu = (torch.arange(n_users, dtype=torch.float64) + 1).pow(-0.5)
    pi = (torch.arange(n_items, dtype=torch.float64) + 1).pow(-0.9)
    u = torch.multinomial(pu, draws, replacement=True, generator=gen)
    i = torch.multinomial(pi, draws, replacement=True, generator=gen)
    return u, i


def layer_bytes(g, bf16):
    """Algorithmic bytes of the K layers, averaged: the first gathers fp32 whatever the layer
    dtype, the last stores no next layer."""
    nnz, N = 2 * g.n_edges, g.n_nodes
    es = 2 if bf16 else 4
    total = 0
    for k in range(K):
        src = 4 if k == 0 else es
        total += nnz * (4 + 4 + D * src) + N * (4 + 2 * D * 4) + (N * D * es if k < K - 1 else 0)
    return total / K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightgcn"))
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lightgcn.py needs a GPU")
    dev = torch.device("cuda")
    with open(os.path.join(ROOT, "profiles", "ceilings.json")) as f:
        copy_gbs = json.load(f)["stream_copy"]["GB/s"]
    res = {"D": D, "K": K, "B": B, "warmup": WARMUP, "reps": REPS, "long_row": graph.LONG_ROW,
           "timing": "device events around each call, host-launched, alternating, random order",
           "device": torch.cuda.get_device_name(0), "stream_copy_GB/s": copy_gbs, "graphs": {}}
    order_rng = np.random.default_rng(4)
    for gi, name in enumerate(args.graphs.split(",")):
        n_users, n_items, n, spare = GRAPHS[name]
        u, i = power_law_interactions(n_users, n_items, n, spare, seed=10 + gi)
        m = LightGCN(CategoricalColumnWithIdentity(n_users, "uid"),
                     CategoricalColumnWithIdentity(n_items, "iid"), None, D, n_layers=K,
                     device=dev, random_seed=1)
        m.set_graph(u, i)
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.01), BPRLoss(), [], dev)
        m.embeddings.check_ids = m._propagated.check_ids = False
        g = m.graph.to(dev)
        g.csr_tensor(torch.float32)  # the sparse path's operand, built outside the timing
        deg = (g.row_ptr[1:] - g.row_ptr[:-1]).cpu()
        gen = torch.Generator(device=dev).manual_seed(3)
        x = 0.1 * torch.randn(g.n_nodes, D, generator=gen, device=dev)
        dy = torch.randn(g.n_nodes, D, generator=gen, device=dev)
        times = {}
        for rep in range(WARMUP + REPS):
            batch = {"uid": torch.randint(0, n_users, (B,), generator=gen, device=dev),
                     "iid": torch.randint(0, n_items, (B, 2), generator=gen, device=dev)}

            def prop_fwd(layer):
                with torch.no_grad():
                    graph.propagate(g, x, K, layer)

            def prop_fwd_bwd(layer):
                xg = x.detach().requires_grad_()
                graph.propagate(g, xg, K, layer).backward(dy)

            def train_step(layer):
                m.layer_dtype = layer
                m.train_step(batch)

            for meas, step in (("prop_fwd", prop_fwd), ("prop_fwd_bwd", prop_fwd_bwd),
                               ("train_step", train_step)):
                for path in order_rng.permutation(list(PATHS)):
                    graph.PROP_FUSED, layer = PATHS[path]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(layer)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= WARMUP:
                        times.setdefault((meas, path), []).append(e0.elapsed_time(e1) * 1e3)
        graph.PROP_FUSED = True
        row = {"n_users": n_users, "n_items": n_items, "interactions": g.n_edges,
               "csr_entries": 2 * g.n_edges, "max_degree": int(deg.max()),
               "median_degree": float(deg.double().median()), "long_rows": int(g.long_row.numel()),
               "work_entries": int(g.work.shape[0]),
               "table_bytes": g.n_nodes * D * 4, "measurements": {}}
        for meas in ("prop_fwd", "prop_fwd_bwd", "train_step"):
            r = {}
            for path in PATHS:
                t = np.array(times[(meas, path)])
                r[path] = {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                           "p90_us": float(np.percentile(t, 90)), "min_us": float(t.min()),
                           "max_us": float(t.max())}
            for path in ("fused", "fused_bf16"):
                r[f"sparse_over_{path}_median"] = r["sparse"]["median_us"] / r[path]["median_us"]
            row["measurements"][meas] = r
            print(f"{name} {meas}: " + ", ".join(f"{p} {r[p]['median_us']:.1f} us "
                                                 f"[{r[p]['p10_us']:.1f}, {r[p]['p90_us']:.1f}]" for p in PATHS))
        for path, bf16 in (("fused", False), ("fused_bf16", True)):
            nb = layer_bytes(g, bf16)
            per_layer_us = row["measurements"]["prop_fwd"][path]["median_us"] / K
            row[f"{path}_layer"] = {"algorithmic_bytes": nb, "median_us": per_layer_us,
                                    "GB/s": nb / per_layer_us / 1e3,
                                    "bytes_at_stream_copy_us": nb / (copy_gbs * 1e3),
                                    "share_of_stream_copy_ceiling": nb / (copy_gbs * 1e3) / per_layer_us}
        res["graphs"][name] = row
        del m, g, x, dy
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_lightgcn.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
