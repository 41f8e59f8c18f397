"""Generate golden fixture G13: one ``IModel.train_step`` of the reference SVD++
(torchrec/model/SVDPP.py) with dense-gradient SGD, the SVD++ counterpart of G10.

Run where the reference is importable only (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_g13.py

Shapes and id draws are G4's (U = 50, I = 37, D = 8, B = 64, L = 9, history lengths
in 1..L; uid / iid / his are read back from g4_svdpp.npz and the label from
g3_funksvd.npz, the same batch), seed 2020, ``MSELoss``, ``SGD(lr=0.5)``.  The
fixture is data only: the five tables and global_bias before and after the step,
the batch, lr, the loss and the torch version that produced it.
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    try:
        from torchrec.feature_column import CategoricalColumnWithIdentity
        from torchrec.metric.metrics import get_metric
        from torchrec.model.SVDPP import SVDPP
    except ImportError:
        raise SystemExit("run with PYTHONPATH=<reference checkout>")
    torch.set_num_threads(1)
    g4 = np.load(os.path.join(OUT, "g4_svdpp.npz"))
    g3 = np.load(os.path.join(OUT, "g3_funksvd.npz"))
    assert np.array_equal(g3["uid"], g4["uid"]) and np.array_equal(g3["iid"], g4["iid"])
    rows_u, D = g4["u_table"].shape
    rows_i = g4["i_table"].shape[0]
    ucol = CategoricalColumnWithIdentity(rows_u, "uid")
    icol = CategoricalColumnWithIdentity(rows_i, "iid")
    hcol = CategoricalColumnWithIdentity(rows_i, "iids")
    lcol = CategoricalColumnWithIdentity(2, "label")
    model = SVDPP(random_seed=2020, uid_column=ucol, iid_column=icol, iids_column=hcol,
                  label_column=lcol, emb_size=D)
    tables = {"u": model.u_embeddings, "i": model.i_embeddings,
              "imp": model.implicit_i_embeddings, "ub": model.u_bias, "ib": model.i_bias}
    arrays = {f"{k}_before": m.weight.detach().clone().numpy() for k, m in tables.items()}
    arrays["gb_before"] = np.array(float(model.global_bias.detach()), dtype=np.float32)
    lr = 0.5
    model.compile(optimizer=torch.optim.SGD(model.get_parameters(), lr=lr),
                  loss=torch.nn.MSELoss(), metrics=[get_metric("ndcg@10")],
                  device=torch.device("cpu"))
    batch = {"uid": torch.from_numpy(g4["uid"]).int(), "iid": torch.from_numpy(g4["iid"]).int(),
             "iids": torch.from_numpy(g4["his"]).int(), "label": torch.from_numpy(g3["label"]).int()}
    logs = model.train_step(dict(batch))
    arrays.update({f"{k}_after": m.weight.detach().numpy() for k, m in tables.items()})
    arrays["gb_after"] = np.array(float(model.global_bias.detach()), dtype=np.float32)
    arrays.update(uid=g4["uid"], iid=g4["iid"], iids=g4["his"], label=g3["label"],
                  lr=np.array(lr), loss=np.array(float(logs["loss"])),
                  torch_version=np.array(torch.__version__))
    np.savez_compressed(os.path.join(OUT, "g13_svdpp_sgd_step.npz"), **arrays)
    print("wrote g13_svdpp_sgd_step.npz", {k: getattr(v, "shape", None) for k, v in arrays.items()})


if __name__ == "__main__":
    main()
