"""Generate golden fixture G16: the reference GRU4Rec (torchrec/model/GRU4Rec.py) in two
weight states, on the CPU.

Run where the reference is importable only (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_g16.py

Shapes: I = 41 items, E = 16, H = 32, L = 12, N = 5 candidates, B = 24, seed 2020.
History lengths lie in 1..L and the rows are tail-padded with 0; sample 0 has length 1,
sample 1 length L.

  State A  the seed-2020 initial ``state_dict`` (pins the RNG order): its eval forward,
           and one ``train_step`` with ``MSELoss`` and ``SGD(lr=0.5)``: all six tensors
           after the step, and the loss.  The embedding and ``out`` are N(0, 0.01) here, so
           the GRU weight gradients are 1e-8 .. 1e-10: this state pins the RNG order and
           the plumbing only.
  State B  all six tensors 0.3 N(0, 1) from ``torch.Generator().manual_seed(16)`` in
           ``state_dict`` order: the forward [B, N], all six parameter gradients of
           ``prediction.square().mean()``, and all six tensors after one SGD step of
           lr 0.05 on them.  This state pins the update.

The fixture is data only: the batch, the tensors above, the learning rates and the torch
version.
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
I, E, H, L, N, B, SEED, LR, LR_B = 41, 16, 32, 12, 5, 24, 2020, 0.5, 0.05


def make_batch():
    rng = np.random.default_rng(16)
    his_len = rng.integers(1, L + 1, size=B)
    his_len[0], his_len[1] = 1, L
    his = np.zeros((B, L), np.int64)
    for b in range(B):
        his[b, :his_len[b]] = rng.integers(1, I, size=his_len[b])
    iid = rng.integers(1, I, size=(B, N))
    label = np.zeros((B, N), np.int64)
    label[:, 0] = 1
    return his, his_len.astype(np.int64), iid.astype(np.int64), label


def main():
    try:
        from torchrec.feature_column import CategoricalColumnWithIdentity
        from torchrec.metric.metrics import get_metric
        from torchrec.model.GRU4Rec import GRU4Rec
    except ImportError:
        raise SystemExit("run with PYTHONPATH=<reference checkout>")
    torch.set_num_threads(1)
    his, his_len, iid, label = make_batch()
    cols = dict(iid_column=CategoricalColumnWithIdentity(I, "iid"),
                his_len_column=CategoricalColumnWithIdentity(L + 1, "his_len"),
                his_column=CategoricalColumnWithIdentity(I, "his"),
                label_column=CategoricalColumnWithIdentity(2, "label"))
    model = GRU4Rec(random_seed=SEED, emb_size=E, hidden_size=H, **cols)
    keys = list(model.state_dict().keys())
    arrays = {"keys": np.array(keys), "his": his, "his_len": his_len, "iid": iid, "label": label,
              "lr": np.array(LR), "lr_b": np.array(LR_B),
              "torch_version": np.array(torch.__version__)}
    arrays.update({f"A::{k}": v.detach().clone().numpy() for k, v in model.state_dict().items()})
    model.compile(optimizer=torch.optim.SGD(model.get_parameters(), lr=LR),
                  loss=torch.nn.MSELoss(), metrics=[get_metric("ndcg@10")],
                  device=torch.device("cpu"))
    batch = {"iid": torch.from_numpy(iid), "his": torch.from_numpy(his),
             "his_len": torch.from_numpy(his_len), "label": torch.from_numpy(label)}
    with torch.no_grad():
        pred, target = model.test_step(dict(batch))
    arrays["A_pred"] = pred.numpy().copy()
    arrays["A_target"] = target.numpy().copy()
    logs = model.train_step(dict(batch))
    arrays["A_loss"] = np.array(float(logs["loss"].detach()))
    arrays.update({f"A_after::{k}": v.detach().clone().numpy()
                   for k, v in model.state_dict().items()})

    gen = torch.Generator().manual_seed(16)
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
    np.savez_compressed(os.path.join(OUT, "g16_gru4rec.npz"), **arrays)
    print("wrote g16_gru4rec.npz", {k: getattr(v, "shape", None) for k, v in arrays.items()})
    print("grad maxima:", {k: float(np.abs(arrays[f"B_grad::{k}"]).max()) for k in keys})


if __name__ == "__main__":
    main()
