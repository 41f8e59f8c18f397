"""SASRec on the hot path — the reference's sequential recommender
(torchrec/model/SASRec.py:34-118).

    X          = i_emb[his] + p_emb[(his_len - j) valid_j]
    num_layers x (ONE shared block):
        Q, K   = X Wq^T, X Wk^T
        A      = softmax_k(D^-0.5 Q K^T) over valid keys (no causal mask)
        X      = LayerNorm(X + dropout(relu(A K W1^T + b1) W2^T + b2))
    v          = sum_{valid j} X_j / his_len
    prediction = v . i_emb[iid[b, n]]                                    [B, N]

valid_j = his_j > 0 with position 0 forced valid (utils.py:5-10).  On a GPU the whole
encoder is one launch each way (``dense.sasrec_encode``: mrec_sasrec_fwd / _bwd /
_wgrad, csrc/sasrec.hip) for emb_size in {16, 32, 64} and histories of up to 64
positions; any other shape, and training with dropout > 0, runs the same arithmetic
as torch ops (``cpu_path.sasrec_encode``, also the CPU path).

Differences from the reference, all documented in DESIGN.md:
  * the softmax shift is each row's own maximum over its valid keys, not the global
    ``attention.max()`` (the same softmax on paper; the reference turns to NaN when
    the global maximum sits far above a row, this build does not);
  * a 1-D ``iid`` raises ValueError (the reference broadcasts it to [B, B]);
  * the device is the tensors' own (the reference needs ``compiled_device``).

Checkpoint compatibility: ``state_dict`` / ``load_state_dict`` speak the reference's
ten keys; the item table is a single-table ``EmbeddingBank`` named ``i_embeddings``
whose history and candidate rows come from ONE gather (one update per row and step).
On a GPU the masked history positions are padding slots of that gather (``pad_skip``).
Initialisation consumes the CPU RNG in the reference's order (the module
constructors, then ``IModel._reset_weights``), so the same ``random_seed`` gives
bit-identical parameters (pinned by golden G15).
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import LayerNorm, Linear, Module, Parameter

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank, gather
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.utils.argument import ArgumentDescription

_I_KEY = "i_embeddings.weight"


class PositionEmbedding(Module):
    """The position table [max_his_len + 1, D] as a plain fp32 dense parameter (at
    most 65 rows: the fused kernel reads it directly, its gradient is dense)."""

    def __init__(self, rows: int, dim: int):
        super().__init__()
        self.weight = Parameter(torch.empty(rows, dim))
        torch.nn.init.normal_(self.weight)  # nn.Embedding's own draw: N(0, 1)


def _state_dict_hook(module, state_dict, prefix, local_metadata):
    """The bank's pitched rows -> the reference's i_embeddings.weight [I, D]."""
    w = state_dict.get(prefix + _I_KEY)
    if w is not None and w.shape[1] != module.emb_size:
        state_dict[prefix + _I_KEY] = w[:, :module.emb_size].clone()
    return state_dict


def _load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys,
                   unexpected_keys, error_msgs):
    """The reference's [I, D] table -> the bank's pitched rows (a pitched one passes)."""
    bank, D = module.i_embeddings, module.emb_size
    t = state_dict.get(prefix + _I_KEY)
    if t is None or bank.row_stride == D or t.dim() != 2 or t.shape[1] != D:
        return
    if t.shape[0] != bank.total_rows:
        return  # torch reports the size mismatch itself
    w = bank.weight.detach().clone()
    w[:, :D] = t.to(device=w.device, dtype=w.dtype)
    state_dict[prefix + _I_KEY] = w


def draw_items(bank, emb_size: int, std: float):
    """normal(0, std) for a single-table item bank, drawn on the CPU default generator in
    the reference's shape like its CPU-built model, then copied."""
    t = torch.empty(bank.total_rows, emb_size)
    torch.nn.init.normal_(t, mean=0.0, std=std)
    with torch.no_grad():
        if bank.row_stride != emb_size:
            bank.weight.zero_()  # row padding stays zero
        bank.table(0).copy_(t.to(bank.weight.dtype))


class SASRec(IModel):
    # GPU: masked history positions are padding slots of the lookup (see forward);
    # False keeps the plain history ids (A/B, parity tests)
    pad_skip = True

    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="max_his_len", type_=int, help_info="history positions",
                                default_value=50, lower_closed_bound=1),
            ArgumentDescription(name="num_layers", type_=int, help_info="attention blocks",
                                default_value=1, lower_closed_bound=1),
            ArgumentDescription(name="dropout", type_=float, help_info="dropout",
                                default_value=0.2, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, iid_column, his_len_column, his_column, label_column, emb_size: int,
                 max_his_len: int, num_layers: int, dropout: float = 0.0, hidden_size: int = 0,
                 emb_dtype: torch.dtype = torch.float32, device=None, **kwargs):
        self.iid_column = iid_column
        self.his_len_column = his_len_column
        self.his_column = his_column
        self.label_column = label_column
        self.emb_size = int(emb_size)
        self.hidden_size = hidden_size  # accepted and unused, as in the reference
        self.max_his_len = int(max_his_len)
        self.num_layers = int(num_layers)
        self.dropout = float(dropout)
        self.emb_dtype = emb_dtype
        self.build_device = torch.device(device) if device is not None else None
        if self.num_layers < 1:
            raise ValueError(f"num_layers must be >= 1, got {num_layers}")
        super().__init__(**kwargs)
        self._register_state_dict_hook(_state_dict_hook)
        self._register_load_state_dict_pre_hook(_load_pre_hook, with_module=True)

    def _init_weights(self):
        D, dev = self.emb_size, self.build_device
        self.i_embeddings = EmbeddingBank([self.iid_column.category_num], D, dtype=self.emb_dtype,
                                          device=dev)
        # the module constructors draw in the reference's order (SASRec.py:66-76):
        # Embedding N(0, 1) twice, then the four Linears' own initialisations
        self._draw_items(1.0)
        self.p_embeddings = PositionEmbedding(self.max_his_len + 1, D)
        self.Q = Linear(D, D, bias=False)
        self.K = Linear(D, D, bias=False)
        self.W1 = Linear(D, D)
        self.W2 = Linear(D, D)
        self.layer_norm = LayerNorm(D)

    def _draw_items(self, std: float):
        draw_items(self.i_embeddings, self.emb_size, std)

    def _reset_weights(self):
        # IModel._reset_weights_fn in registration order (IModel.py:61-68): the two
        # Embeddings, then Q, K, W1, W2 (weight, then bias); LayerNorm stays 1 / 0
        # (drawn on the CPU generator like the reference's CPU-built model, then moved)
        self._draw_items(0.01)
        for m in (self.p_embeddings, self.Q, self.K, self.W1, self.W2):
            self._reset_weights_fn(m)
        if self.build_device is not None:
            for m in (self.p_embeddings, self.Q, self.K, self.W1, self.W2, self.layer_norm):
                m.to(self.build_device)

    candidate_lists = True
    retrieval_low = 1  # id 0 is the padding item

    def _history_lookup_ids(self, his: Tensor):
        """The history's lookup ids, flat ``[B L]``, and whether negative ones are padding
        slots of the gather."""
        bank = self.i_embeddings
        if not (bank.weight.is_cuda and self.pad_skip):
            return his.reshape(-1), False
        # masked history positions (never a key, dropped from v: an exactly zero
        # gradient) become padding slots (-1): zero rows forward, skipped by the
        # backward, so the PAD row is not a ~B L / 2-lookup hot row of every step's
        # update.  A negative id anywhere else stays out of range (IndexError).
        past = torch.full_like(his, bank.category_nums[0])
        pad = torch.where(his < 0, past, torch.full_like(his, -1))
        pad[:, 0] += his[:, 0] == 0  # position 0 is forced valid: the PAD row itself
        return torch.where(his > 0, his, pad).reshape(-1), True

    def _encode_history(self, data: Dict[str, Tensor]) -> Tensor:
        """v [B, D] from a history-only lookup (``recommend``: no candidates to gather)."""
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if his.dim() != 2:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        B, L = his.shape
        bank = self.i_embeddings
        act_dtype = torch.bfloat16 if bank.weight.is_cuda else torch.float32
        hist_ids, padded = self._history_lookup_ids(his)
        rows = gather(bank, [hist_ids], out_dtype=act_dtype, pad_negative=padded)
        return dense_ops.sasrec_encode(rows.reshape(B, L, self.emb_size), his, his_len, self)

    def _retrieval_query(self, data: Dict[str, Tensor]):
        """``recommend``: the score is v . i, the query the encoder's output."""
        return self._encode_history(data).float(), self.i_embeddings, 0, False, None

    def _lookup_rows(self, his: Tensor, cand: Tensor) -> Tensor:
        """History and candidate rows in ONE lookup (one sorted-segment backward, one update
        per row, as a single nn.Embedding would do): ``[B L + len(cand), D]``, the history
        first."""
        bank = self.i_embeddings
        act_dtype = torch.bfloat16 if bank.weight.is_cuda else torch.float32
        hist_ids, padded = self._history_lookup_ids(his)
        cand = cand.to(his.dtype)
        if padded:
            past = torch.full_like(his.reshape(-1)[:1], bank.category_nums[0])
            cand = torch.where(cand < 0, past, cand)
        return gather(bank, [torch.cat([hist_ids, cand])], out_dtype=act_dtype, pad_negative=padded)

    def _shared_negative_inputs(self, data: Dict[str, Tensor], neg_ids):
        """History, positives and the pool in the single lookup ``forward`` builds; q is the
        encoder's output of ``_retrieval_query``, with gradients and dropout."""
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if his.dim() != 2:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        pos_ids = self._shared_positive_ids(data)
        B, L = his.shape
        cand = pos_ids if neg_ids is None else torch.cat([pos_ids, neg_ids.to(pos_ids.dtype)])
        rows = self._lookup_rows(his, cand)
        v = dense_ops.sasrec_encode(rows[:B * L].reshape(B, L, self.emb_size), his, his_len, self)
        pos_rows = rows[B * L:B * L + B]
        neg_rows = rows[B * L + B:] if neg_ids is not None else pos_rows
        return v.float(), pos_rows, neg_rows, pos_ids

    def forward(self, data: Dict[str, Tensor]):
        i_ids = self.iid_column.get_feature_ids(data)
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if i_ids.dim() != 2:
            raise ValueError(f"SASRec scores candidate lists: iid must be [B, N], got "
                             f"{tuple(i_ids.shape)}")
        if his.dim() != 2 or his.shape[0] != i_ids.shape[0]:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        B, N = i_ids.shape
        L, D = his.shape[1], self.emb_size
        rows = self._lookup_rows(his, i_ids.reshape(-1))
        v = dense_ops.sasrec_encode(rows[:B * L].reshape(B, L, D), his, his_len, self)
        prediction = (v.unsqueeze(1) * rows[B * L:].reshape(B, N, D).float()).sum(-1)
        target = None
        if self.label_column is not None and self.label_column.feature_name in data:
            target = data[self.label_column.feature_name].float()
        return prediction, target
