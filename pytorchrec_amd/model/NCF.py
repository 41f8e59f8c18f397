"""NCF (NeuMF) on the hot path — the reference's neural collaborative filtering model
(torchrec/model/NCF.py:13-79).

For pair (b, n), with u = uid[b] and i = iid[b, n]:

    g          = mf_u[u] * mf_i[i]                              [E]
    h_0        = [mlp_u[u] | mlp_i[i]]                          [2E]
    h_{l+1}    = dropout(relu(W_l h_l + b_l))                   the reference's Dense stack
    prediction = Wp . [g | h_k]                                 Linear(E + width_k, 1), no bias
    target     = zeros [B, N] float32, column 0 = 1

The four tables live in ONE ``EmbeddingBank([users, items, users, items], E)``: one gather
launch over the ids ``[uu, ii, uu, ii]`` (the uid of sample b repeated for its N
candidates, as FunkSVD does) returns the row ``[mf_u | mf_i | mlp_u | mlp_i]`` of every
pair, and there is one backward plan under any of the bank's update modes.  On a GPU the
whole scorer is one launch each way (``dense.ncf_score``: mrec_ncf_fwd / _bwd,
csrc/ncf.hip) for emb_size in {8, 16, 32, 64} and 1-3 hidden layers of widths that are
multiples of 8 up to 128; any other shape, and training with dropout > 0, runs the same
arithmetic as torch ops (``cpu_path.ncf_score``, also the CPU path).

Differences from the reference, documented in DESIGN.md:
  * a 1-D ``iid`` raises ValueError (the reference fails on ``i_ids.shape[1]`` with an
    IndexError that names no cause);
  * ``get_argument_descriptions`` is real (the reference returns None);
  * ``layers`` also accepts the CLI string form ("64,32,16");
  * the device is the tensors' own.

Checkpoint compatibility: ``state_dict`` / ``load_state_dict`` speak the reference's keys
(``mf_u_embeddings.weight``, ``mf_i_embeddings.weight``, ``mlp_u_embeddings.weight``,
``mlp_i_embeddings.weight``, ``mlp.mlp.dense_{l}.linear.{weight,bias}``,
``prediction.weight``).  Initialisation consumes the CPU RNG in the reference's order
(the four Embedding constructors, the MLP's Linears, ``prediction``; then
``IModel._reset_weights_fn`` in registration order), so the same ``random_seed`` gives
bit-identical parameters (golden G17).

``recommend`` (full-catalogue top-k): the scorer is an MLP over the pair, not a dot
product with an item row, so there is no ``_retrieval_query``.  On a GPU, for the shapes
``retrieval.ncf_supported`` names, it is ``retrieval.ncf_topk`` -- one ``mrec_ncf_topk``
launch (csrc/ncf_topk.hip) that forms the (user, item) pairs on chip, with layer 0 split
into a per-user and a per-item half, and selects the k best without a gathered row or a
``[B, items]`` score reaching memory.  The kernel's LDS plan holds every layer's weight
image and the per-user key buffers at once, so wide towers -- (64, [128, 128, 128]), most
three-layer towers of widths near 100 at emb_size 64 -- are outside it.  On a CPU, for any
other shape, and with
``retrieval.NCF_TOPK_FUSED = False`` it is ``IModel.recommend_by_forward``: the item
range goes through ``forward`` in chunks of candidates.
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Linear

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank, gather
from pytorchrec_amd.model.DeepFM import _parse_layers
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.model.layer.MLP import MLP
from pytorchrec_amd.utils.argument import ArgumentDescription
from pytorchrec_amd.utils.data_structure import tensor_to_device

_BANK_KEY = "embeddings.weight"
_TABLE_KEYS = ("mf_u_embeddings.weight", "mf_i_embeddings.weight", "mlp_u_embeddings.weight",
               "mlp_i_embeddings.weight")


def _table_slices(module):
    bank = module.embeddings
    return [slice(o, o + n) for o, n in zip(bank.row_offset, bank.category_nums)]


def _state_dict_hook(module, state_dict, prefix, local_metadata):
    """embeddings.weight -> the reference's four table keys, ahead of the dense keys."""
    w = state_dict.pop(prefix + _BANK_KEY, None)
    if w is None:
        return state_dict
    D = module.emb_size
    rest = [(k, state_dict.pop(k)) for k in list(state_dict.keys()) if k.startswith(prefix)]
    for key, sl in zip(_TABLE_KEYS, _table_slices(module)):
        state_dict[prefix + key] = w[sl, :D].clone()
    for k, v in rest:
        state_dict[k] = v
    return state_dict


def _load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys,
                   unexpected_keys, error_msgs):
    """The reference keys (or the packed bank key) -> the packed bank weight."""
    if not any(prefix + k in state_dict for k in _TABLE_KEYS):
        return
    bank, D = module.embeddings, module.emb_size
    w = bank.weight.detach().clone()
    for key, sl in zip(_TABLE_KEYS, _table_slices(module)):
        t = state_dict.pop(prefix + key, None)
        if t is None:
            if strict:
                missing_keys.append(prefix + key)
            continue
        want = (sl.stop - sl.start, D)
        if tuple(t.shape) != want:
            error_msgs.append(f"size mismatch for {prefix + key}: copying a param with shape "
                              f"{tuple(t.shape)}, the shape in current model is {want}.")
            continue
        w[sl, :D] = t.to(device=w.device, dtype=w.dtype)
    state_dict[prefix + _BANK_KEY] = w


class NCF(IModel):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="layers", type_=str, help_info="MLP widths, e.g. 128,64,32",
                                default_value="128,64,32"),
            ArgumentDescription(name="dropout", type_=float, help_info="MLP dropout",
                                default_value=0.0, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, uid_column, iid_column, label_column, emb_size: int, layers,
                 dropout: float = 0.0, emb_dtype: torch.dtype = torch.float32, device=None,
                 **kwargs):
        self.uid_column = uid_column
        self.iid_column = iid_column
        self.label_column = label_column
        self.emb_size = int(emb_size)
        self.layers = _parse_layers(layers)
        self.dropout = float(dropout)
        self.emb_dtype = emb_dtype
        self.build_device = torch.device(device) if device is not None else None
        if not self.layers:
            raise ValueError("layers must name at least one hidden width")
        super().__init__(**kwargs)
        self._register_state_dict_hook(_state_dict_hook)
        self._register_load_state_dict_pre_hook(_load_pre_hook, with_module=True)

    def _init_weights(self):
        nu, ni = self.uid_column.category_num, self.iid_column.category_num
        self.embeddings = EmbeddingBank([nu, ni, nu, ni], self.emb_size, dtype=self.emb_dtype,
                                        device=self.build_device)
        # the module constructors draw in the reference's order (NCF.py:39-51): four
        # Embeddings N(0, 1), the MLP's Linears, the prediction Linear
        self._init_tables(1.0)
        self.mlp = MLP(input_units=2 * self.emb_size, hidden_units_list=self.layers,
                       activation="relu", dropout=self.dropout)
        self.prediction = Linear(self.emb_size + self.layers[-1], 1, bias=False)

    def _init_tables(self, std: float):
        """normal(0, std) per table in the reference's order (mf_u, mf_i, mlp_u, mlp_i),
        drawn on the CPU default generator like the reference's CPU-built model."""
        bank = self.embeddings
        with torch.no_grad():
            if bank.row_stride != self.emb_size:
                bank.weight.zero_()  # row padding stays zero
            for f, n in enumerate(bank.category_nums):
                t = torch.empty(n, self.emb_size)
                torch.nn.init.normal_(t, mean=0.0, std=std)
                bank.table(f).copy_(t.to(bank.weight.dtype))

    def _reset_weights(self):
        # IModel._reset_weights_fn in registration order (IModel.py:61-68): the four
        # tables, every Dense's Linear (weight, then bias), the prediction Linear
        self._init_tables(0.01)
        self.mlp.apply(self._reset_weights_fn)
        self._reset_weights_fn(self.prediction)
        if self.build_device is not None:
            self.mlp.to(self.build_device)
            self.prediction.to(self.build_device)

    candidate_lists = True  # (recommend_by_forward applies; see the module docstring)

    def set_shared_negatives(self, source, n_shared=None, iid_column=None):
        """Not available: NCF scores a (user, item) pair with an MLP, not with a dot product
        of a query vector and an item row, which is what the shared-negative losses take.
        Train NCF pair-wise (``set_negative_sampler``)."""
        if source is None:
            return super().set_shared_negatives(None)
        raise NotImplementedError("NCF scores pairs with an MLP: there is no query vector to "
                                  "rank a shared pool of item rows against")

    def forward(self, data: Dict[str, Tensor]):
        u_ids = self.uid_column.get_feature_ids(data)
        i_ids = self.iid_column.get_feature_ids(data)
        if i_ids.dim() != 2:
            raise ValueError(f"NCF scores candidate lists: iid must be [B, N], got "
                             f"{tuple(i_ids.shape)}")
        B, N = i_ids.shape
        bank = self.embeddings
        uu = u_ids.reshape(B, 1).expand(B, N).reshape(-1).contiguous()
        ii = i_ids.reshape(-1).to(uu.dtype).contiguous()
        act_dtype = torch.bfloat16 if bank.weight.is_cuda else torch.float32
        # [mf_u | mf_i | mlp_u | mlp_i] of every pair in ONE lookup
        rows = gather(bank, [uu, ii, uu, ii], out_dtype=act_dtype)
        prediction = dense_ops.ncf_score(rows, self).reshape(B, N)
        target = torch.zeros_like(prediction, dtype=torch.float32)
        target[:, 0] = 1
        return prediction, target

    def recommend(self, data: Dict[str, Tensor], k: int, *, exclude=None, low=None, high=None):
        """``IModel.recommend``'s contract.  The fused kernel on a GPU when it covers the
        shape (``retrieval.ncf_topk``), else ``recommend_by_forward``.  Runs in eval mode
        (no dropout) under ``no_grad`` and restores the training flag."""
        from pytorchrec_amd import retrieval
        bank = self.embeddings
        dense = [p for p in self.parameters() if p is not bank.weight]
        if not (retrieval.NCF_TOPK_FUSED and bank.weight.is_cuda and isinstance(k, int)
                and all(p.is_cuda and p.dtype == torch.float32 for p in dense)
                and retrieval.ncf_supported(self.emb_size, self.layers, k, bank.weight.dtype)):
            return self.recommend_by_forward(data, k, exclude=exclude, low=low, high=high)
        low, high = self._retrieval_range(low, high)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                data = tensor_to_device(data, self._model_device())
                uid = self.uid_column.get_feature_ids(data).reshape(-1)
                return retrieval.ncf_topk(self, uid, k, low=low, high=high, exclude=exclude)
        finally:
            self.train(was_training)
