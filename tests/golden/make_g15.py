"""Generate golden fixture G15: the reference SASRec (torchrec/model/SASRec.py) in two
weight states, on the CPU.

Run where the reference is importable only (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_g15.py

Shapes: I = 41 items, D = 16, L = max_his_len = 12, N = 5 candidates, B = 24, 2 layers,
dropout 0, seed 2020.  History lengths lie in 1..L and the rows are tail-padded with 0;
sample 0 has length 1, sample 1 length L, and sample 2 is the forced-valid PAD row
(``his[2, 0] == 0``, length 1).

  State A  the seed-2020 initial ``state_dict`` (pins the RNG order): its eval forward,
           and one ``train_step`` with ``MSELoss`` and ``SGD(lr=0.5)``: all ten tensors
           after the step, and the loss.
  State B  "lively" weights (at the 0.01 initialisation the Q / K gradients are ~1e-10):
           embeddings and Linears N(0, 0.3), LayerNorm weight 1 + 0.2 N and bias 0.2 N,
           from ``torch.Generator().manual_seed(15)`` in ``state_dict`` order; the forward
           [B, N] and all ten parameter gradients of ``prediction.square().mean()``.

The fixture is data only: the batch, the tensors above, lr and the torch version.
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
I, D, L, N, B, LAYERS, SEED, LR = 41, 16, 12, 5, 24, 2, 2020, 0.5


def make_batch():
    rng = np.random.default_rng(15)
    his_len = rng.integers(1, L + 1, size=B)
    his_len[0], his_len[1], his_len[2] = 1, L, 1
    his = np.zeros((B, L), np.int64)
    for b in range(B):
        his[b, :his_len[b]] = rng.integers(1, I, size=his_len[b])
    his[2] = 0
    iid = rng.integers(1, I, size=(B, N))
    label = np.zeros((B, N), np.int64)
    label[:, 0] = 1
    return his, his_len.astype(np.int64), iid.astype(np.int64), label


def main():
    try:
        from torchrec.feature_column import CategoricalColumnWithIdentity
        from torchrec.metric.metrics import get_metric
        from torchrec.model.SASRec import SASRec
    except ImportError:
        raise SystemExit("run with PYTHONPATH=<reference checkout>")
    torch.set_num_threads(1)
    his, his_len, iid, label = make_batch()
    cols = dict(iid_column=CategoricalColumnWithIdentity(I, "iid"),
                his_len_column=CategoricalColumnWithIdentity(L + 1, "his_len"),
                his_column=CategoricalColumnWithIdentity(I, "his"),
                label_column=CategoricalColumnWithIdentity(2, "label"))
    model = SASRec(random_seed=SEED, emb_size=D, hidden_size=D, max_his_len=L, num_layers=LAYERS,
                   dropout=0.0, **cols)
    keys = list(model.state_dict().keys())
    arrays = {"keys": np.array(keys), "his": his, "his_len": his_len, "iid": iid, "label": label,
              "lr": np.array(LR), "torch_version": np.array(torch.__version__)}
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

    gen = torch.Generator().manual_seed(15)
    state = {}
    for k, v in model.state_dict().items():
        n = torch.randn(v.shape, generator=gen)
        if k == "layer_norm.weight":
            state[k] = 1.0 + 0.2 * n
        elif k == "layer_norm.bias":
            state[k] = 0.2 * n
        else:
            state[k] = 0.3 * n
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
    for k, v in arrays.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(OUT, "g15_sasrec.npz"), **arrays)
    print("wrote g15_sasrec.npz", {k: getattr(v, "shape", None) for k, v in arrays.items()})
    print("grad maxima:", {k: float(np.abs(arrays[f"B_grad::{k}"]).max()) for k in keys})


if __name__ == "__main__":
    main()
