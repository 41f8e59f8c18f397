"""Time ranking evaluation through its two paths, and one negative-sampling call, on
the GPU (fails without one).

Shapes: FunkSVD (D = 64, fp32 tables) over 4096 users x 99 candidates (a leave-one-out
dev set: the positive plus 98 sampled items of 50,000), served in batches of 1024 by
the columnar loader; metrics ndcg@10 and hit@10.

Two paths of ``IModel.evaluate``, in one process, alternating, by a host clock around
the call (it ends in a device-to-host copy, hence a synchronise) after warm-up:
  device  every metric a ranking metric: mrec_rank_pos per batch, one copy of the
          4096 int32 ranks at the end;
  host    the same metrics wrapped so that ``evaluate`` does not recognise them: every
          [1024, 99] prediction batch is copied to the host and ranked in numpy.
Both return the same values (checked).

``NegativeSampler.sample`` of 4096 x 1 (users with 20 positives each of 50,000 items)
by device events around the call, host-launched.

Writes bench_rank.json into profiles/rank (or the directory given as the first
argument): the median, min, max, p10 and p90 of each.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity  # noqa: E402
from pytorchrec_amd.loader import ColumnarDataset  # noqa: E402
from pytorchrec_amd.loss import BPRLoss  # noqa: E402
from pytorchrec_amd.metrics import get_metric  # noqa: E402
from pytorchrec_amd.model import FunkSVD  # noqa: E402
from pytorchrec_amd.sampling import NegativeSampler  # noqa: E402

U, N, ITEMS, D, BATCH = 4096, 99, 50000, 64, 1024
WARMUP, REPS = 5, 30


class Unrecognised:
    """A ranking metric behind a plain callable: ``evaluate`` takes its host path."""

    def __init__(self, metric):
        self.metric, self.name = metric, metric.name

    def __call__(self, prediction, target):
        return self.metric(prediction, target)


def stats(t):
    t = np.array(t)
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
            "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90))}


def bench_evaluate(dev):
    rng = np.random.default_rng(0)
    data = ColumnarDataset({"uid": np.arange(U), "iid": rng.integers(0, ITEMS, (U, N))})
    model = FunkSVD(CategoricalColumnWithIdentity(U, "uid"), CategoricalColumnWithIdentity(ITEMS, "iid"),
                    None, emb_size=D, random_seed=1)
    opt = torch.optim.SGD(model.get_parameters(), lr=0.1)
    ranking = [get_metric("ndcg@10"), get_metric("hit@10")]
    paths = {"device": ranking, "host": [Unrecognised(m) for m in ranking]}
    times = {k: [] for k in paths}
    values = {}
    for rep in range(WARMUP + REPS):
        for name, metrics in paths.items():  # alternating
            model.compile(opt, BPRLoss(), metrics, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[name] = model.evaluate(data, BATCH, verbose=0)
            dt = time.perf_counter() - t0
            if rep >= WARMUP:
                times[name].append(dt * 1e6)
    assert values["device"] == values["host"], values
    out = {name: stats(t) for name, t in times.items()}
    out["values"] = values["device"]
    out["speedup_median"] = out["host"]["median_us"] / out["device"]["median_us"]
    return out


def bench_sample(dev):
    rng = np.random.default_rng(1)
    uu = np.repeat(np.arange(U), 20)
    sampler = NegativeSampler(uu, rng.integers(0, ITEMS, uu.size), 0, ITEMS, seed=0, n_users=U,
                              device=dev)
    uids = torch.from_numpy(rng.permutation(U)).int().to(dev)
    times = []
    for rep in range(WARMUP + 100):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sampler.sample(uids, 1, step=rep)
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append(e0.elapsed_time(e1) * 1e3)
    out = stats(times)
    out["unresolved"] = sampler.unresolved()
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank.py needs a GPU")
    dev = torch.device("cuda:0")
    res = {"users": U, "candidates": N, "items": ITEMS, "D": D, "eval_batch": BATCH,
           "warmup": WARMUP, "reps": REPS, "device": torch.cuda.get_device_name(0),
           "timing": {"evaluate": "host clock around evaluate() (ends in a D2H copy), loader included",
                      "sample": "device events around one sample() of 4096 x 1, host-launched"},
           "evaluate": bench_evaluate(dev), "sample_4096x1": bench_sample(dev)}
    e, s = res["evaluate"], res["sample_4096x1"]
    print(f"evaluate 4096 x 99: device ranks {e['device']['median_us']:.0f} us "
          f"[{e['device']['min_us']:.0f}, {e['device']['max_us']:.0f}], host ranks "
          f"{e['host']['median_us']:.0f} us [{e['host']['min_us']:.0f}, {e['host']['max_us']:.0f}]; "
          f"sample 4096 x 1: {s['median_us']:.1f} us [{s['min_us']:.1f}, {s['max_us']:.1f}]")
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rank")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_rank.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
