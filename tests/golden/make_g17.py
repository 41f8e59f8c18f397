"""Generate golden fixture G17: the reference NCF (torchrec/model/NCF.py) in two weight
states, on the CPU.

Run where the reference is importable only (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_g17.py

Shapes: U = 50 users, I = 37 items, E = 8, layers [16, 8], N = 5 candidates, B = 24,
seed 2020, dropout 0.  Users and items repeat across the batch (samples 1 and 2 share
sample 0's user; every sample's last candidate is sample 0's first).

  State A  the seed-2020 initial ``state_dict`` (pins the RNG order): its eval forward,
           and one ``train_step`` with ``MSELoss`` and ``SGD(lr=0.5)``: all nine tensors
           after the step, and the loss.  Everything is N(0, 0.01) here, so the MLP's
           gradients are tiny: this state pins the RNG order and the plumbing only.
  State B  all nine tensors 0.3 N(0, 1) from ``torch.Generator().manual_seed(17)`` in
           ``state_dict`` order: the forward [B, N], all nine parameter gradients of
           ``prediction.square().mean()``, and all nine tensors after one SGD step of
           lr 0.05 on them.  This state pins the update.

The fixture is data only: the batch, the tensors above, the learning rates and the torch
version.
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
U, I, E, LAYERS, N, B, SEED, LR, LR_B = 50, 37, 8, [16, 8], 5, 24, 2020, 0.5, 0.05


def make_batch():
    rng = np.random.default_rng(17)
    uid = rng.integers(0, U, size=B)
    uid[1] = uid[2] = uid[0]
    iid = rng.integers(0, I, size=(B, N))
    iid[:, N - 1] = iid[0, 0]
    label = np.zeros((B, N), np.int64)
    label[:, 0] = 1
    return uid.astype(np.int64), iid.astype(np.int64), label


def main():
    try:
        from torchrec.feature_column import CategoricalColumnWithIdentity
        from torchrec.metric.metrics import get_metric
        from torchrec.model.NCF import NCF
    except ImportError:
        raise SystemExit("run with PYTHONPATH=<reference checkout>")
    torch.set_num_threads(1)
    uid, iid, label = make_batch()
    cols = dict(uid_column=CategoricalColumnWithIdentity(U, "uid"),
                iid_column=CategoricalColumnWithIdentity(I, "iid"),
                label_column=CategoricalColumnWithIdentity(2, "label"))
    model = NCF(random_seed=SEED, emb_size=E, layers=list(LAYERS), dropout=0.0, **cols)
    keys = list(model.state_dict().keys())
    arrays = {"keys": np.array(keys), "uid": uid, "iid": iid, "label": label,
              "layers": np.array(LAYERS), "lr": np.array(LR), "lr_b": np.array(LR_B),
              "torch_version": np.array(torch.__version__)}
    arrays.update({f"A::{k}": v.detach().clone().numpy() for k, v in model.state_dict().items()})
    model.compile(optimizer=torch.optim.SGD(model.get_parameters(), lr=LR),
                  loss=torch.nn.MSELoss(), metrics=[get_metric("ndcg@10")],
                  device=torch.device("cpu"))
    batch = {"uid": torch.from_numpy(uid), "iid": torch.from_numpy(iid),
             "label": torch.from_numpy(label)}
    with torch.no_grad():
        pred, target = model.test_step(dict(batch))
    arrays["A_pred"] = pred.numpy().copy()
    arrays["A_target"] = target.numpy().copy()
    logs = model.train_step(dict(batch))
    arrays["A_loss"] = np.array(float(logs["loss"].detach()))
    arrays.update({f"A_after::{k}": v.detach().clone().numpy()
                   for k, v in model.state_dict().items()})

    gen = torch.Generator().manual_seed(17)
    state = {k: 0.3 * torch.randn(v.shape, generator=gen) for k, v in model.state_dict().items()}
    model.load_state_dict(state)
    model.eval()
    model.zero_grad()
    pred, _ = model(dict(batch))
    pred.square().mean().backward()
    named = dict(model.named_parameters())
    assert list(named) == keys
    arrays.update({f"B::{k}": v.numpy() for k, v in state.items()})
    arrays["B_pred"] = pred.detach().numpy().copy()
    arrays.update({f"B_grad::{k}": named[k].grad.detach().numpy().copy() for k in keys})
    with torch.no_grad():
        for k in keys:
            named[k].add_(named[k].grad, alpha=-LR_B)
    arrays.update({f"B_after::{k}": v.detach().clone().numpy()
                   for k, v in model.state_dict().items()})
    for k, v in arrays.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(OUT, "g17_ncf.npz"), **arrays)
    print("wrote g17_ncf.npz", {k: getattr(v, "shape", None) for k, v in arrays.items()})
    print("grad maxima:", {k: float(np.abs(arrays[f"B_grad::{k}"]).max()) for k in keys})


if __name__ == "__main__":
    main()
