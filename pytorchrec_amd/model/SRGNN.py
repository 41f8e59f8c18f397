"""SR-GNN on the hot path — the session-graph recommender (Wu et al., "Session-based
Recommendation with Graph Neural Networks", AAAI 2019): each history becomes its own small
directed graph, a gated GNN runs on it, and an attention readout gives the query vector.

    valid_j    = his_j > 0 or j == 0; positions ascend in time
    nodes      = the distinct ids of the valid positions; alias(t) the first valid position
                 with the id of t; edge a -> b when some consecutive valid positions have
                 these aliases (binary; an item following itself is a self-loop)
    H_a        = i_emb[his_a] at the representative positions (no position embeddings)
    gnn_steps times:
        M_in   = A_in (H W_ein^T + b_ein) + b_iah,  M_out = A_out (H W_eout^T + b_eout) + b_oah
        gi, gh = [M_in | M_out] W_ih^T + b_ih,  H W_hh^T + b_hh
        r, z   = sigmoid(gi_r + gh_r), sigmoid(gi_z + gh_z);  c = tanh(gi_c + r gh_c)
        H      = c + z (H - c)
    h_last     = H[alias(last valid position)]
    alpha_k    = q . sigmoid(W1 h_last + W2 H[alias(t_k)] + c1)      over the valid positions
    v          = Wt [sum_k alpha_k H[alias(t_k)] | h_last] + bt
    prediction = v . i_emb[iid[b, n]]                                [B, N]

A_in / A_out average over the distinct in- / out-edges (a degree of 0 divides as 1).

Everything around the encoder is SASRec's (model/SASRec.py): the single-table item bank
``i_embeddings`` with ``pad_skip`` and its state-dict hooks, the one-gather lookup,
``recommend`` / ``evaluate_full``, shared-negative and pair-wise training.  On a GPU the
whole encoder, the graph construction included, is one launch each way
(``dense.srgnn_encode``: mrec_srgnn_fwd / _bwd, csrc/srgnn.hip, one workgroup per sample) for
emb_size in {16, 32, 64}, histories of up to 64 positions and up to 4 steps; any other shape
and the CPU run the same arithmetic as torch ops (``cpu_path.srgnn_encode``).
"""
from typing import List

import torch
from torch import Tensor
from torch.nn import Parameter

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank
from pytorchrec_amd.model.SASRec import SASRec
from pytorchrec_amd.utils.argument import ArgumentDescription

# state-dict name -> shape in units of D
_SHAPES = {"W_ein": (1, 1), "W_eout": (1, 1), "W1": (1, 1), "W2": (1, 1), "b_ein": (1,),
           "b_eout": (1,), "b_iah": (1,), "b_oah": (1,), "c1": (1,), "q": (1,), "bt": (1,),
           "W_ih": (3, 2), "W_hh": (3, 1), "b_ih": (3,), "b_hh": (3,), "Wt": (1, 2)}


class SRGNN(SASRec):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="max_his_len", type_=int, help_info="history positions",
                                default_value=50, lower_closed_bound=1),
            ArgumentDescription(name="gnn_steps", type_=int, help_info="gated-GNN steps",
                                default_value=1, lower_closed_bound=1),
        ]

    def __init__(self, iid_column, his_len_column, his_column, label_column, emb_size: int,
                 max_his_len: int, gnn_steps: int = 1, **kwargs):
        self.gnn_steps = int(gnn_steps)
        if self.gnn_steps < 1:
            raise ValueError(f"gnn_steps must be >= 1, got {gnn_steps}")
        kwargs.pop("num_layers", None)
        kwargs.pop("dropout", None)
        super().__init__(iid_column, his_len_column, his_column, label_column, emb_size,
                         max_his_len, 1, **kwargs)

    def _init_weights(self):
        D = self.emb_size
        self.i_embeddings = EmbeddingBank([self.iid_column.category_num], D, dtype=self.emb_dtype,
                                          device=self.build_device)
        for name, shape in _SHAPES.items():
            setattr(self, name, Parameter(torch.empty(*(n * D for n in shape))))

    def _reset_weights(self):
        # drawn on the CPU generator (so a seed gives the same parameters on any device), then
        # moved: every parameter, the items too, U(-D^-1/2, D^-1/2) as the paper's code does
        bound = self.emb_size ** -0.5
        bank = self.i_embeddings
        t = torch.empty(bank.total_rows, self.emb_size).uniform_(-bound, bound)
        with torch.no_grad():
            if bank.row_stride != self.emb_size:
                bank.weight.zero_()  # row padding stays zero
            bank.table(0).copy_(t.to(bank.weight.dtype))
            for name in _SHAPES:
                getattr(self, name).uniform_(-bound, bound)
        if self.build_device is not None:
            for name in _SHAPES:
                p = getattr(self, name)
                p.data = p.data.to(self.build_device)

    def _encode(self, rows: Tensor, his: Tensor, his_len: Tensor) -> Tensor:
        """v [B, D] of the gathered history rows [B, L, D]."""
        return dense_ops.srgnn_encode(rows, his, his_len, self)
