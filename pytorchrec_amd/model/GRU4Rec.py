"""GRU4Rec on the hot path — the reference's recurrent session recommender
(torchrec/model/GRU4Rec.py:38-70).

    x_t        = i_emb[his[b, t]]                              t = 0 .. his_len[b] - 1
    r_t, z_t   = sigmoid(W_i{r,z} x_t + b_i{r,z} + W_h{r,z} h_{t-1} + b_h{r,z})    h_-1 = 0
    n_t        = tanh(W_in x_t + b_in + r_t (W_hn h_{t-1} + b_hn))
    h_t        = (1 - z_t) n_t + z_t h_{t-1}
    v          = out.weight @ h_{his_len - 1}                  Linear(H -> E, no bias)
    prediction = v . i_emb[iid[b, n]]                          [B, N]

The reference sorts by length, packs, runs nn.GRU and unsorts; all that does is run
sample b for exactly his_len[b] steps.  A position is live iff t < his_len[b]: the ids
past the length never matter, and (unlike SASRec) id 0 inside the length is an ordinary
row.  On a GPU the whole recurrence is one launch each way (``dense.gru_encode``:
mrec_gru_fwd / _bwd, csrc/gru.hip) for emb_size and hidden_size in {16, 32, 64} and up
to 64 positions; any other shape runs the same arithmetic as torch ops
(``cpu_path.gru_encode``, also the CPU path).  ``out`` goes through ``dense.linear``.

Differences from the reference, documented in DESIGN.md:
  * a 1-D ``iid`` raises ValueError (the reference broadcasts it to [B, B]);
  * ``his_len`` outside 1..L raises IndexError (the reference fails inside
    pack_padded_sequence with a RuntimeError);
  * the device is the tensors' own (the reference needs ``compiled_device``).

Checkpoint compatibility: ``state_dict`` / ``load_state_dict`` speak the reference's six
keys (``i_embeddings.weight``, the four ``rnn.*_l0``, ``out.weight``); the item table is a
single-table ``EmbeddingBank`` whose history and candidate rows come from ONE gather.
``rnn`` holds the four parameters under nn.GRU's names but is no nn.GRU (moving one to a
device hands its weights to MIOpen).  Initialisation consumes the CPU RNG in the
reference's order, so the same ``random_seed`` gives bit-identical parameters (golden G16).
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Linear, Module, Parameter

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank, gather
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.model.SASRec import _load_pre_hook, _state_dict_hook, draw_items
from pytorchrec_amd.utils.argument import ArgumentDescription


class GruCell(Module):
    """One GRU layer's parameters under nn.GRU's names and in its layout (gate order
    r, z, n), drawn as ``nn.GRU.reset_parameters`` draws them: U(-1/sqrt(H), 1/sqrt(H))
    over weight_ih, weight_hh, bias_ih, bias_hh, in that order."""

    def __init__(self, input_size: int, hidden_size: int):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.weight_ih_l0 = Parameter(torch.empty(3 * hidden_size, input_size))
        self.weight_hh_l0 = Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.bias_ih_l0 = Parameter(torch.empty(3 * hidden_size))
        self.bias_hh_l0 = Parameter(torch.empty(3 * hidden_size))
        stdv = 1.0 / hidden_size ** 0.5 if hidden_size > 0 else 0
        for w in self.parameters():
            torch.nn.init.uniform_(w, -stdv, stdv)


class GRU4Rec(IModel):
    # GPU: history positions past the length are padding slots of the lookup (see
    # forward); False keeps the plain history ids (A/B, parity tests)
    pad_skip = True
    # GPU: how the fused kernel's 16-sample tiles are filled (speed only, A/B): "auto"
    # (sorted by length when the batch has more tiles than workgroups), "sorted", or None
    # for the batch order (``dense.gru_encode``)
    tile_order = "auto"

    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="hidden_size", type_=int, help_info="GRU hidden units",
                                default_value=64, lower_closed_bound=1),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, iid_column, his_len_column, his_column, label_column, emb_size: int,
                 hidden_size: int, emb_dtype: torch.dtype = torch.float32, device=None, **kwargs):
        self.iid_column = iid_column
        self.his_len_column = his_len_column
        self.his_column = his_column
        self.label_column = label_column
        self.emb_size = int(emb_size)
        self.hidden_size = int(hidden_size)
        self.emb_dtype = emb_dtype
        self.build_device = torch.device(device) if device is not None else None
        super().__init__(**kwargs)
        self._register_state_dict_hook(_state_dict_hook)
        self._register_load_state_dict_pre_hook(_load_pre_hook, with_module=True)

    def _init_weights(self):
        E, dev = self.emb_size, self.build_device
        self.i_embeddings = EmbeddingBank([self.iid_column.category_num], E, dtype=self.emb_dtype,
                                          device=dev)
        # the module constructors draw in the reference's order (GRU4Rec.py:39-41):
        # Embedding N(0, 1), nn.GRU's uniform draws, then the Linear's own initialisation
        draw_items(self.i_embeddings, E, 1.0)
        self.rnn = GruCell(E, self.hidden_size)
        self.out = Linear(self.hidden_size, E, bias=False)

    def _reset_weights(self):
        # IModel._reset_weights_fn in registration order (IModel.py:61-68): the Embedding
        # and ``out``; nn.GRU matches neither 'Linear' nor 'Embedding' and keeps its draw
        # (drawn on the CPU generator like the reference's CPU-built model, then moved)
        draw_items(self.i_embeddings, self.emb_size, 0.01)
        self._reset_weights_fn(self.out)
        if self.build_device is not None:
            self.rnn.to(self.build_device)
            self.out.to(self.build_device)

    candidate_lists = True

    def _history_lookup_ids(self, his: Tensor, his_len: Tensor):
        """The history's lookup ids, flat ``[B L]``, and whether negative ones are padding
        slots of the gather."""
        bank = self.i_embeddings
        live = torch.arange(his.shape[1], device=his.device).unsqueeze(0) < his_len.reshape(-1, 1)
        if bank.weight.is_cuda and self.pad_skip:
            # positions past the length (never read by the recurrence: an exactly zero
            # gradient) become padding slots (-1): zero rows forward, skipped by the
            # backward.  A negative id anywhere else stays out of range (IndexError).
            past = torch.full_like(his, bank.category_nums[0])
            return torch.where(live, torch.where(his < 0, past, his),
                               torch.full_like(his, -1)).reshape(-1), True
        # the ids past the length never matter: row 0 stands in for them
        return torch.where(live, his, torch.zeros_like(his)).reshape(-1), False

    def _session_vector(self, rows: Tensor, his_len: Tensor) -> Tensor:
        """v = out(h_last) [B, E] fp32 from the history rows [B, L, E]."""
        h = dense_ops.gru_encode(rows, his_len, self, order=self.tile_order)
        return dense_ops.linear(h, self.out.weight, None, out_dtype=torch.float32)

    def _retrieval_query(self, data: Dict[str, Tensor]):
        """``recommend``: the score is v . i with v = out(h), from a history-only lookup."""
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if his.dim() != 2:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        B, L = his.shape
        bank = self.i_embeddings
        act_dtype = torch.bfloat16 if bank.weight.is_cuda else torch.float32
        hist_ids, padded = self._history_lookup_ids(his, his_len)
        rows = gather(bank, [hist_ids], out_dtype=act_dtype, pad_negative=padded)
        v = self._session_vector(rows.reshape(B, L, self.emb_size), his_len)
        return v.float(), bank, 0, False, None

    def _lookup_rows(self, his: Tensor, his_len: Tensor, cand: Tensor) -> Tensor:
        """History and candidate rows in ONE lookup (one sorted-segment backward, one update
        per row, as a single nn.Embedding would do): ``[B L + len(cand), E]``, the history
        first."""
        bank = self.i_embeddings
        act_dtype = torch.bfloat16 if bank.weight.is_cuda else torch.float32
        hist_ids, padded = self._history_lookup_ids(his, his_len)
        cand = cand.to(his.dtype)
        if padded:
            past = torch.full_like(his.reshape(-1)[:1], bank.category_nums[0])
            cand = torch.where(cand < 0, past, cand)
        return gather(bank, [torch.cat([hist_ids, cand])], out_dtype=act_dtype, pad_negative=padded)

    def _shared_negative_inputs(self, data: Dict[str, Tensor], neg_ids):
        """History, positives and the pool in the single lookup ``forward`` builds; q is the
        session vector of ``_retrieval_query``, with gradients."""
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if his.dim() != 2:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        pos_ids = self._shared_positive_ids(data)
        B, L = his.shape
        cand = pos_ids if neg_ids is None else torch.cat([pos_ids, neg_ids.to(pos_ids.dtype)])
        rows = self._lookup_rows(his, his_len, cand)
        v = self._session_vector(rows[:B * L].reshape(B, L, self.emb_size), his_len)
        pos_rows = rows[B * L:B * L + B]
        neg_rows = rows[B * L + B:] if neg_ids is not None else pos_rows
        return v.float(), pos_rows, neg_rows, pos_ids

    def forward(self, data: Dict[str, Tensor]):
        i_ids = self.iid_column.get_feature_ids(data)
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if i_ids.dim() != 2:
            raise ValueError(f"GRU4Rec scores candidate lists: iid must be [B, N], got "
                             f"{tuple(i_ids.shape)}")
        if his.dim() != 2 or his.shape[0] != i_ids.shape[0]:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        B, N = i_ids.shape
        L, E = his.shape[1], self.emb_size
        rows = self._lookup_rows(his, his_len, i_ids.reshape(-1))
        v = self._session_vector(rows[:B * L].reshape(B, L, E), his_len)
        prediction = (v.float().unsqueeze(1) * rows[B * L:].reshape(B, N, E).float()).sum(-1)
        target = None
        if self.label_column is not None and self.label_column.feature_name in data:
            target = data[self.label_column.feature_name].float()
        return prediction, target
