"""MIND on the hot path — the multi-interest retriever (Li et al., "Multi-Interest Network
with Dynamic Routing", CIKM 2019; the same routing is ComiRec-DR, Cen et al., KDD 2020): a
history is routed into K interest capsules instead of one query vector, and an item's score
is its best interest's.

    X          = i_emb[his]                                 (invalid rows are zero rows)
    H^_j       = X_j route_weight^T                         (one map shared by all capsules)
    b_kj       = route_init[k, j]                           (a buffer, never trained)
    routing_iters times:
        w_kj   = softmax over the active k of b_kj at valid j, exactly 0 elsewhere
        z_k    = sum_j w_kj H^_j;   u_k = squash(z_k);   b_kj += u_k . H^_j
    U          = the last u                                              [B, K, D]
    prediction = max over the active k of U_bk . i_emb[iid[b, n]]        [B, N]

Active interests: all K, or with ``dynamic_k`` MIND's adaptive count max(1, min(K,
floor(log2(his_len)))).  The routing logits carry no gradient (MIND 4.2): training flows
through the squash and the last z only.  There are no position embeddings, as in MIND.

Training readout (``_shared_negative_inputs``: the query trained against the positive and
the shared pool): ``interest_pow = 0`` is ComiRec's hard readout, the interest that scores
the positive highest; ``interest_pow = p > 0`` is q = sum_k softmax_k(p U_k . e) U_k over
the active interests.  MIND's label-aware attention writes pow(score, p), which is
undefined for negative scores; this is the temperature form of it (p -> infinity is the
hard readout in both).  ``forward`` scores with the maximum in training and evaluation
alike: it is the serving rule, so no label enters an evaluation score.

Everything around the extractor is SASRec's (model/SASRec.py): the single-table item bank
``i_embeddings`` with ``pad_skip`` and its state-dict hooks, the one-gather lookup,
shared-negative training.  ``recommend`` serves all B K interest vectors in ONE
``retrieval.topk`` call and merges each user's K k candidates.  On a GPU the routing is one
launch each way (``dense.mind_route``: mrec_mind_fwd / _bwd, csrc/mind.hip, one wave per
sample) for emb_size in {16, 32, 64}, up to 8 interests, histories of up to 64 positions
and up to 4 iterations; any other shape runs the same arithmetic as torch ops
(``cpu_path.mind_route``, also the CPU path).
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Parameter

from pytorchrec_amd import cpu_path
from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank
from pytorchrec_amd.model.SASRec import SASRec
from pytorchrec_amd.utils.argument import ArgumentDescription
from pytorchrec_amd.utils.data_structure import tensor_to_device


class MIND(SASRec):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="max_his_len", type_=int, help_info="history positions",
                                default_value=50, lower_closed_bound=1),
            ArgumentDescription(name="num_interests", type_=int, help_info="interest capsules",
                                default_value=4, lower_closed_bound=1),
            ArgumentDescription(name="routing_iters", type_=int, help_info="routing iterations",
                                default_value=3, lower_closed_bound=1),
            ArgumentDescription(name="dynamic_k", type_=int,
                                help_info="1: min(K, log2(his_len)) active interests",
                                default_value=0, lower_closed_bound=0),
            ArgumentDescription(name="interest_pow", type_=float,
                                help_info="readout temperature (0: hard readout)",
                                default_value=0.0, lower_closed_bound=0.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, iid_column, his_len_column, his_column, label_column, emb_size: int,
                 max_his_len: int, num_interests: int = 4, routing_iters: int = 3,
                 dynamic_k: bool = False, interest_pow: float = 0.0, **kwargs):
        self.num_interests = int(num_interests)
        self.routing_iters = int(routing_iters)
        self.dynamic_k = bool(dynamic_k)
        self.interest_pow = float(interest_pow)
        if self.num_interests < 1 or self.routing_iters < 1:
            raise ValueError(f"num_interests ({num_interests}) and routing_iters ({routing_iters}) "
                             f"must be >= 1")
        if self.interest_pow < 0:
            raise ValueError(f"interest_pow must be >= 0, got {interest_pow}")
        kwargs.pop("num_layers", None)
        super().__init__(iid_column, his_len_column, his_column, label_column, emb_size,
                         max_his_len, 1, **kwargs)

    def _init_weights(self):
        D = self.emb_size
        self.i_embeddings = EmbeddingBank([self.iid_column.category_num], D, dtype=self.emb_dtype,
                                          device=self.build_device)
        self.route_weight = Parameter(torch.empty(D, D))
        # the routing logits' start, N(0, 1) as in MIND: drawn once, saved, never trained
        self.register_buffer("route_init", torch.randn(self.num_interests, self.max_his_len))

    def _reset_weights(self):
        # drawn on the CPU generator (so a seed gives the same parameters on any device),
        # then moved: the items N(0, 0.01) like SASRec's, the routing map N(0, D^-1/2)
        self._draw_items(0.01)
        with torch.no_grad():
            torch.nn.init.normal_(self.route_weight, mean=0.0, std=self.emb_size ** -0.5)
        if self.build_device is not None:
            self.route_weight.data = self.route_weight.data.to(self.build_device)
            self.route_init = self.route_init.to(self.build_device)

    def _encode(self, rows: Tensor, his: Tensor, his_len: Tensor) -> Tensor:
        """U [B, K, D], the interest capsules of the gathered history rows [B, L, D]."""
        return dense_ops.mind_route(rows, his, his_len, self)

    def _active(self, his_len: Tensor) -> Tensor:
        """[B, K] bool: the interests each sample uses."""
        K = self.num_interests
        kp = cpu_path.mind_active(his_len, K, self.dynamic_k)
        return torch.arange(K, device=his_len.device)[None, :] < kp[:, None]

    def _readout(self, U: Tensor, e: Tensor, act: Tensor) -> Tensor:
        """q [B, D]: the interests read out against the item rows e [B, D]."""
        s = (U * e.unsqueeze(1)).sum(-1).masked_fill(~act, float("-inf"))
        if self.interest_pow == 0:
            return U[torch.arange(U.shape[0], device=U.device), s.argmax(dim=1)]
        return (torch.softmax(self.interest_pow * s, dim=1).unsqueeze(-1) * U).sum(1)

    def _retrieval_query(self, data: Dict[str, Tensor]):
        raise NotImplementedError("MIND serves K queries per user: see recommend")

    def _shared_negative_inputs(self, data: Dict[str, Tensor], neg_ids):
        """As SASRec's, with the readout against the positive's row as q."""
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if his.dim() != 2:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        pos_ids = self._shared_positive_ids(data)
        B, L = his.shape
        cand = pos_ids if neg_ids is None else torch.cat([pos_ids, neg_ids.to(pos_ids.dtype)])
        rows = self._lookup_rows(his, cand)
        U = self._encode(rows[:B * L].reshape(B, L, self.emb_size), his, his_len)
        pos_rows = rows[B * L:B * L + B]
        neg_rows = rows[B * L + B:] if neg_ids is not None else pos_rows
        q = self._readout(U, pos_rows.float(), self._active(his_len.reshape(-1)))
        return q.float(), pos_rows, neg_rows, pos_ids

    def forward(self, data: Dict[str, Tensor]):
        i_ids = self.iid_column.get_feature_ids(data)
        his = self.his_column.get_feature_ids(data)
        his_len = self.his_len_column.get_feature_ids(data)
        if i_ids.dim() != 2:
            raise ValueError(f"MIND scores candidate lists: iid must be [B, N], got "
                             f"{tuple(i_ids.shape)}")
        if his.dim() != 2 or his.shape[0] != i_ids.shape[0]:
            raise ValueError(f"his must be [B, L], got {tuple(his.shape)}")
        B, N = i_ids.shape
        L, D = his.shape[1], self.emb_size
        rows = self._lookup_rows(his, i_ids.reshape(-1))
        U = self._encode(rows[:B * L].reshape(B, L, D), his, his_len)
        s = torch.bmm(U, rows[B * L:].reshape(B, N, D).float().transpose(1, 2))  # [B, K, N]
        act = self._active(his_len.reshape(-1))
        prediction = s.masked_fill(~act.unsqueeze(-1), float("-inf")).max(dim=1).values
        target = None
        if self.label_column is not None and self.label_column.feature_name in data:
            target = data[self.label_column.feature_name].float()
        return prediction, target

    def recommend(self, data: Dict, k: int, *, exclude=None, low=None, high=None):
        """As ``IModel.recommend``, the score of an item being its best active interest's:
        one ``retrieval.topk`` call over the B K interest vectors (a user's exclusion row
        reaches each of the user's queries through ``Exclusion.rows``), then per user the
        K k candidates merged in torch ops: an item several interests found keeps its
        highest score; by score descending, then id ascending."""
        from pytorchrec_amd import retrieval
        k = int(k)
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")
        low, high = self._retrieval_range(low, high)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                self.flush_embedding_optimizers()
                dev = self._model_device()
                data = tensor_to_device(data, dev)
                U = self._encode_history(data).float()
                B, K, D = U.shape
                act = self._active(self.his_len_column.get_feature_ids(data).reshape(-1))
                ex = None
                if exclude is not None:
                    ex = exclude.to(dev)
                    base = ex.rows if ex.rows is not None else torch.arange(B, device=dev)
                    ex = retrieval.Exclusion(ex.offsets, ex.items, base.repeat_interleave(K))
                ids, scores = retrieval.topk(self.i_embeddings, 0, U.reshape(B * K, D), k, low=low,
                                             high=high, exclude=ex)
                off = ~act.unsqueeze(-1)
                scores = scores.reshape(B, K, k).masked_fill(off, float("-inf")).reshape(B, K * k)
                ids = ids.reshape(B, K, k).long().masked_fill(off, -1).reshape(B, K * k)
                # group by id with the best score first, drop the repeats, then the total order
                ids, scores = _sorted_by(ids, scores, by_id_first=True)
                dup = torch.zeros_like(ids, dtype=torch.bool)
                dup[:, 1:] = ids[:, 1:] == ids[:, :-1]
                scores = scores.masked_fill(dup, float("-inf"))
                ids = ids.masked_fill(dup | (scores == float("-inf")), -1)
                ids, scores = _sorted_by(ids, scores, by_id_first=False)
                return ids[:, :k].to(torch.int32).contiguous(), scores[:, :k].contiguous()
        finally:
            self.train(was_training)


def _sorted_by(ids: Tensor, scores: Tensor, by_id_first: bool):
    """Rows of (ids, scores) sorted by (id ascending, score descending) or by (score
    descending, id ascending): two stable sorts, the minor key first."""
    for by_id in ((False, True) if by_id_first else (True, False)):
        order = torch.sort(ids if by_id else scores, dim=1, descending=not by_id, stable=True).indices
        ids, scores = ids.gather(1, order), scores.gather(1, order)
    return ids, scores
