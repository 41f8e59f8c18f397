"""DIEN — Deep Interest Evolution Network (Zhou et al., AAAI 2019), DIN's successor.

Absent from the reference; built from DIN's idioms (model/DIN.py) with DIN's attention-
weighted sum replaced by two recurrent layers over the behaviour history:

    e_t   = [item row | category row] of history position t          E = 2 emb_size
    h1_t  = GRU1(e_t, h1_{t-1})                     the interest extractor
    a     = softmax_t(h1_t . p),  p = att_query(q)  q the target's row, bilinear score
    h2_t  = AUGRU(h1_t, h2_{t-1}; a_t)              u_t = a_t (1 - z_t)
    logit = prediction(MLP([q | h2_last | sum_t e_t]))

``his_len`` is the count of valid positions (id > 0, position 0 forced valid; histories
are tail-padded, as in DIN).  On a GPU the three stages are one launch each way
(``dense.interest_evolution``: mrec_interest_fwd / _bwd, csrc/augru.hip) for E and
``hidden_size`` in {16, 32, 64} and up to 64 positions; any other shape, the CPU, and
``dense.DIEN_FUSED = False`` run the same arithmetic as torch ops
(``cpu_path.interest_evolution``).

Auxiliary loss (given ``neg_his_column`` / ``neg_his_cate_column``): for t < his_len - 1
    -log sigmoid(h1_t . W_aux e_{t+1}) - log(1 - sigmoid(h1_t . W_aux ne_{t+1}))
averaged over those positions and weighted by ``aux_weight``, in torch ops on the
returned h1 sequence; its gradient enters the kernel as d_hs1.  It is part of
``fused_bce_loss`` (the training loss under BCEWithLogitsLoss).

Differences from the paper, documented in DESIGN.md: the score is the paper's bilinear
form (not DIN's MLP unit); the auxiliary discriminator is bilinear, not an MLP; no
dropout inside the recurrence.
"""
from __future__ import annotations

from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Linear

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import gather
from pytorchrec_amd.sharding import make_bank
from pytorchrec_amd.feature_column import CategoricalColumn
from pytorchrec_amd.model.DeepFM import _parse_layers
from pytorchrec_amd.model.DIN import din_id_buffers, din_lookup_ids, din_sources
from pytorchrec_amd.model.GRU4Rec import GruCell
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.model.layer.MLP import MLP
from pytorchrec_amd.utils.argument import ArgumentDescription


class DIEN(IModel):
    # GPU: masked history positions are padding slots of the lookup (as DIN); False
    # keeps the plain [target | history] ids (A/B, parity tests)
    pad_skip = True
    # how the fused kernel's 16-sample tiles are filled (``dense.gru_encode``): speed only
    tile_order = "auto"
    # samples per call of the layered path (bounds its [chunk, L, 3H] intermediates)
    layered_chunk = 8192

    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="embedding dim",
                                default_value=16, lower_closed_bound=1),
            ArgumentDescription(name="hidden_size", type_=int,
                                help_info="GRU hidden units (0: 2 * emb_size)",
                                default_value=0, lower_closed_bound=0),
            ArgumentDescription(name="layers", type_=str, help_info="top MLP widths",
                                default_value="200,80"),
            ArgumentDescription(name="aux_weight", type_=float,
                                help_info="weight of the auxiliary loss", default_value=1.0,
                                lower_closed_bound=0.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, iid_column: CategoricalColumn, cid_column: CategoricalColumn,
                 his_column: CategoricalColumn, his_cate_column: CategoricalColumn,
                 label_column=None, emb_size: int = 16, layers=(200, 80), dropout: float = 0.0,
                 emb_dtype: torch.dtype = torch.float32, device=None, hidden_size: int = 0,
                 neg_his_column: CategoricalColumn = None,
                 neg_his_cate_column: CategoricalColumn = None, aux_weight: float = 1.0,
                 **kwargs):
        if (neg_his_column is None) != (neg_his_cate_column is None):
            raise ValueError("neg_his_column and neg_his_cate_column go together")
        self.iid_column = iid_column
        self.cid_column = cid_column
        self.his_column = his_column
        self.his_cate_column = his_cate_column
        self.neg_his_column = neg_his_column
        self.neg_his_cate_column = neg_his_cate_column
        self.label_column = label_column
        self.emb_size = int(emb_size)
        self.hidden_size = int(hidden_size) if hidden_size else 2 * self.emb_size
        self.layers = _parse_layers(layers)
        self.dropout = float(dropout)
        self.aux_weight = float(aux_weight)
        self.emb_dtype = emb_dtype
        self.build_device = torch.device(device) if device is not None else None
        super().__init__(**kwargs)

    def _init_weights(self):
        dev = self.build_device
        D, H = self.emb_size, self.hidden_size
        self.embeddings = make_bank([self.iid_column.category_num,
                                     self.cid_column.category_num], D,
                                    with_first_order=False, dtype=self.emb_dtype, device=dev)
        E = 2 * D
        self.extractor = GruCell(E, H)   # layer 1
        self.evolution = GruCell(H, H)   # layer 2 (AUGRU)
        self.att_query = Linear(E, H, bias=False)
        self.aux = Linear(E, H, bias=False) if self.neg_his_column is not None else None
        self.mlp = MLP(2 * E + H, self.layers, "relu", self.dropout)
        self.prediction = Linear(self.layers[-1], 1)
        if dev is not None:
            for m in (self.extractor, self.evolution, self.att_query, self.aux, self.mlp,
                      self.prediction):
                if m is not None:
                    m.to(dev)

    def _recurrent_params(self):
        c1, c2 = self.extractor, self.evolution
        return (c1.weight_ih_l0, c1.weight_hh_l0, c1.bias_ih_l0, c1.bias_hh_l0,
                c2.weight_ih_l0, c2.weight_hh_l0, c2.bias_ih_l0, c2.bias_hh_l0)

    def _evolve(self, k: Tensor, his_len: Tensor, p: Tensor):
        """(v [B, H], hs1 [B, L, H]) of ``dense.interest_evolution``; the layered path runs
        in chunks of the batch."""
        params = self._recurrent_params()
        B, L, E = k.shape
        fused = (k.is_cuda and dense_ops.DIEN_FUSED
                 and dense_ops.interest_supported(E, self.hidden_size, L))
        if fused or B <= self.layered_chunk:
            return dense_ops.interest_evolution(k, his_len, p, params, order=self.tile_order,
                                                check=False)
        parts = [dense_ops.interest_evolution(k[i:i + self.layered_chunk],
                                              his_len[i:i + self.layered_chunk],
                                              p[i:i + self.layered_chunk], params, check=False)
                 for i in range(0, B, self.layered_chunk)]
        return torch.cat([v for v, _ in parts]), torch.cat([h for _, h in parts])

    def _history_rows(self, his: Tensor, hcat: Tensor, valid: Tensor, act_dtype):
        """Rows [B, L, E] of a (negative) history; invalid positions are padding slots on a
        GPU and are masked by the caller everywhere."""
        bank = self.embeddings
        B, L = his.shape
        if bank.weight.is_cuda and self.pad_skip:
            pad = torch.full_like(his, -1)
            ids = [torch.where(valid, his, pad).reshape(-1), torch.where(valid, hcat.to(his.dtype), pad).reshape(-1)]
            rows = gather(bank, ids, out_dtype=act_dtype, pad_negative=True)
        else:
            rows = gather(bank, [his.reshape(-1), hcat.reshape(-1).to(his.dtype)], out_dtype=act_dtype)
        return rows.reshape(B, L, -1)

    def _top(self, data: Dict[str, Tensor], want_aux: bool = False):
        """-> (top [B, 2E + H] fp32, auxiliary loss or None; the negative history is looked
        up only with ``want_aux``)."""
        bank = self.embeddings
        on_gpu = bank.weight.is_cuda
        act_dtype = torch.bfloat16 if on_gpu else torch.float32
        iid = self.iid_column.get_feature_ids(data)
        cid = self.cid_column.get_feature_ids(data)
        his = self.his_column.get_feature_ids(data)
        hcat = self.his_cate_column.get_feature_ids(data)
        B, L = his.shape
        # target and history rows in ONE lookup per table, as DIN
        if on_gpu and self.pad_skip:
            if bank.update == "adam":
                ids_i, ids_c = din_lookup_ids(iid, cid, his, hcat, bank.category_nums)
                rows = gather(bank, [ids_i, ids_c], out_dtype=act_dtype, pad_negative=True)
            else:
                rows = gather(bank, din_id_buffers(his), out_dtype=act_dtype, pad_negative=True,
                              din_src=din_sources(iid, cid, his, hcat, bank.category_nums))
        else:
            rows = gather(bank, [torch.cat([iid.reshape(-1), his.reshape(-1).to(iid.dtype)]),
                                 torch.cat([cid.reshape(-1), hcat.reshape(-1).to(cid.dtype)])],
                          out_dtype=act_dtype)
        q, k = rows[:B], rows[B:].reshape(B, L, -1)
        valid = his > 0
        valid[:, 0] = True
        his_len = valid.sum(1).to(torch.int32)
        vmask = valid.unsqueeze(-1)
        qf = q.float()
        p = dense_ops.linear(q, self.att_query.weight, None, out_dtype=torch.float32)
        v, hs1 = self._evolve(k, his_len, p)
        pooled = (k.float() * vmask).sum(1)
        aux = None
        if (want_aux and self.aux is not None and self.aux_weight != 0.0
                and self.neg_his_column.feature_name in data and L > 1):
            nhis = self.neg_his_column.get_feature_ids(data)
            ncat = self.neg_his_cate_column.get_feature_ids(data)
            kn = self._history_rows(nhis, ncat, valid, act_dtype)
            w = self.aux.weight.float()
            nxt = valid[:, 1:]  # t + 1 < his_len
            g = hs1[:, :-1] @ w  # [B, L - 1, E]: h1_t W_aux
            pos = (g * k[:, 1:].float()).sum(-1)
            neg = (g * kn[:, 1:].float()).sum(-1)
            both = torch.nn.functional.softplus(-pos) + torch.nn.functional.softplus(neg)
            aux = (both * nxt).sum() / nxt.sum().clamp(min=1)
        return torch.cat([qf, v.float(), pooled], dim=-1), aux

    def forward(self, data: Dict[str, Tensor]):
        top, _ = self._top(data)
        h = self.mlp(top)
        logit = dense_ops.head(h, self.prediction.weight, self.prediction.bias)
        target = None
        if self.label_column is not None and self.label_column.feature_name in data:
            target = data[self.label_column.feature_name].float()
        return logit.reshape(-1).float(), target

    def fused_bce_loss(self, data: Dict[str, Tensor]):
        """Training loss: BCE with logits (mean) with the output layer fused into it, plus
        ``aux_weight`` times the auxiliary loss when the negative history is given."""
        top, aux = self._top(data, want_aux=True)
        y = data[self.label_column.feature_name].float()
        if dense_ops.tower_supported(top, self.mlp, self.prediction):
            loss = dense_ops.tower_bce(top, self.mlp, self.prediction, None, y)
        else:
            h = self.mlp(top)
            loss, _ = dense_ops.ctr_head_bce(h, self.prediction.weight, self.prediction.bias, None, y)
        if aux is not None:
            loss = loss + self.aux_weight * aux
        return loss
