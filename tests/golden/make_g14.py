"""Generate golden fixture G14: the reference's ranking pieces.

Run where the reference is importable only (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_g14.py

The fixture is data only and records the torch version that produced it:

  * ``x`` fp32 [1000, 2] = 4 N(0, 1) (seed 1414) whose first rows are (-30, 30),
    (30, -30), (0, 0), (-60, 45) -- the softplus threshold and the saturated
    sigmoids -- with the reference ``BPRLoss`` / ``Top1Loss`` outputs
    (``<loss>_<reduction>``) and input gradients (``<loss>_<reduction>_grad``; the
    ``none`` output is summed before ``backward``) for the three reductions;
  * ``pred`` fp32 [257, 99], tie-free per row, with ``ranks`` =
    ``IMetric.get_pos_rank`` of the flattened prediction and ``ndcg@k`` / ``hit@k`` for
    k in {1, 5, 10, 99};
  * one reference ``FunkSVD.train_step`` with ``BPRLoss`` and ``SGD(lr=0.5)``: seed
    2020, G11's ``uid`` and the first two columns of G11's ``iid`` (the G10 model: 50
    users, 37 items, D = 8); the tables before and after the step and the loss.
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    try:
        from torchrec.feature_column import CategoricalColumnWithIdentity
        from torchrec.loss.BPRLoss import BPRLoss
        from torchrec.loss.Top1Loss import Top1Loss
        from torchrec.metric.metrics import get_metric
        from torchrec.model.FunkSVD import FunkSVD
    except ImportError:
        raise SystemExit("run with PYTHONPATH=<reference checkout>")
    torch.set_num_threads(1)
    arrays = {}

    rng = np.random.default_rng(1414)
    x = (4.0 * rng.standard_normal((1000, 2))).astype(np.float32)
    x[:4] = [(-30, 30), (30, -30), (0, 0), (-60, 45)]
    arrays["x"] = x
    for name, cls in (("bpr", BPRLoss), ("top1", Top1Loss)):
        for reduction in ("none", "mean", "sum"):
            t = torch.from_numpy(x.copy()).requires_grad_()
            out = cls(reduction=reduction)(t, None)
            out.sum().backward()
            arrays[f"{name}_{reduction}"] = out.detach().numpy()
            arrays[f"{name}_{reduction}_grad"] = t.grad.numpy()

    pred = rng.standard_normal((257, 99)).astype(np.float32)
    assert all(len(np.unique(r)) == 99 for r in pred), "a tied row: change the seed"
    arrays["pred"] = pred
    flat = pred.reshape(-1)
    arrays["ranks"] = get_metric("ndcg@10").get_pos_rank(flat).astype(np.int64)
    for k in (1, 5, 10, 99):
        for m in ("ndcg", "hit"):
            arrays[f"{m}@{k}"] = np.array(float(get_metric(f"{m}@{k}")(flat, None)), np.float64)

    g11 = np.load(os.path.join(OUT, "g11_funksvd_sampled.npz"))
    rows_u, D = g11["u_table"].shape
    rows_i = g11["i_table"].shape[0]
    ucol = CategoricalColumnWithIdentity(rows_u, "uid")
    icol = CategoricalColumnWithIdentity(rows_i, "iid")
    lcol = CategoricalColumnWithIdentity(2, "label")
    model = FunkSVD(uid_column=ucol, iid_column=icol, label_column=lcol, emb_size=D,
                    random_seed=2020)
    arrays["u_before"] = model.u_embeddings.weight.detach().clone().numpy()
    arrays["i_before"] = model.i_embeddings.weight.detach().clone().numpy()
    lr = 0.5
    model.compile(optimizer=torch.optim.SGD(model.get_parameters(), lr=lr), loss=BPRLoss(),
                  metrics=[get_metric("ndcg@10")], device=torch.device("cpu"))
    uid, iid = g11["uid"], np.ascontiguousarray(g11["iid"][:, :2])
    logs = model.train_step({"uid": torch.from_numpy(uid).int(), "iid": torch.from_numpy(iid).int()})
    arrays.update(u_after=model.u_embeddings.weight.detach().numpy(),
                  i_after=model.i_embeddings.weight.detach().numpy(), uid=uid, iid=iid,
                  lr=np.array(lr), loss=np.array(float(logs["loss"].detach())),
                  torch_version=np.array(torch.__version__))
    np.savez_compressed(os.path.join(OUT, "g14_ranking.npz"), **arrays)
    print("wrote g14_ranking.npz", {k: getattr(v, "shape", None) for k, v in arrays.items()})


if __name__ == "__main__":
    main()
