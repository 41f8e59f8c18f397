"""HSTU on the hot path — the causal, multi-head sequential encoder with its own weights
per layer (Zhai et al., "Actions Speak Louder than Words", ICML 2024): pointwise SiLU
attention in place of softmax, a learned relative-position bias and a gating branch U; a
pre-norm block with one fused U|V|Q|K projection replaces the FFN.

    X          = i_emb[his] + p_emb[(his_len - j) valid_j]      (invalid rows are zero rows)
    per layer l (own weights):
        N         = LayerNorm(X; norm1[l])
        [U|V|Q|K] = SiLU(N uvqk_weight[l]^T + uvqk_bias[l])
        per head: A = SiLU(Q_h K_h^T + rab[l, h, i - j]) / max_his_len
                      for j <= i and valid_j, exactly 0 elsewhere;  C_h = A V_h
        X         = X + dropout((LayerNorm(concat C_h; norm2[l]) U) out_weight[l]^T + out_bias[l])
    v          = X[t], t the last valid position
    prediction = v . i_emb[iid[b, n]]                                    [B, N]

Left out of the paper's block: the time-bucket half of the relative bias (the data
pipeline carries no timestamps) and a final output normalisation.

Everything around the encoder is SASRec's (model/SASRec.py): the single-table item bank
``i_embeddings`` with ``pad_skip`` and its state-dict hooks, the one-gather lookup,
``recommend`` / shared-negative training.  On a GPU the whole encoder is one launch each
way (``dense.hstu_encode``: mrec_hstu_fwd / _bwd, csrc/hstu.hip) for emb_size in
{16, 32, 64}, heads of width 16, 32 or 64, histories of up to 64 positions and up to 4
layers; any other shape, and training with dropout > 0, runs the same arithmetic as torch
ops (``cpu_path.hstu_encode``, also the CPU path).

The parameters are stacked per kind, [num_layers, ...], so that the kernel gets one
pointer and a layer stride.
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Parameter

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd.embedding import EmbeddingBank
from pytorchrec_amd.model.SASRec import PositionEmbedding, SASRec
from pytorchrec_amd.utils.argument import ArgumentDescription

_STACKED = ("norm1_weight", "norm1_bias", "uvqk_weight", "uvqk_bias", "rab", "norm2_weight",
            "norm2_bias", "out_weight", "out_bias")


class HSTU(SASRec):
    eps = 1e-5  # both LayerNorms

    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                default_value=64, lower_closed_bound=1),
            ArgumentDescription(name="max_his_len", type_=int, help_info="history positions",
                                default_value=50, lower_closed_bound=1),
            ArgumentDescription(name="num_layers", type_=int, help_info="HSTU blocks",
                                default_value=2, lower_closed_bound=1),
            ArgumentDescription(name="num_heads", type_=int, help_info="attention heads",
                                default_value=2, lower_closed_bound=1),
            ArgumentDescription(name="dropout", type_=float, help_info="dropout",
                                default_value=0.2, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, iid_column, his_len_column, his_column, label_column, emb_size: int,
                 max_his_len: int, num_layers: int = 2, dropout: float = 0.0, num_heads: int = 2,
                 **kwargs):
        self.num_heads = int(num_heads)
        if self.num_heads < 1 or int(emb_size) % self.num_heads:
            raise ValueError(f"emb_size ({emb_size}) must be a multiple of num_heads ({num_heads})")
        super().__init__(iid_column, his_len_column, his_column, label_column, emb_size,
                         max_his_len, num_layers, dropout=dropout, **kwargs)

    def _init_weights(self):
        D, n, H = self.emb_size, self.num_layers, self.num_heads
        self.i_embeddings = EmbeddingBank([self.iid_column.category_num], D, dtype=self.emb_dtype,
                                          device=self.build_device)
        self.p_embeddings = PositionEmbedding(self.max_his_len + 1, D)
        self.norm1_weight = Parameter(torch.ones(n, D))
        self.norm1_bias = Parameter(torch.zeros(n, D))
        self.uvqk_weight = Parameter(torch.empty(n, 4 * D, D))
        self.uvqk_bias = Parameter(torch.zeros(n, 4 * D))
        self.rab = Parameter(torch.zeros(n, H, self.max_his_len))
        self.norm2_weight = Parameter(torch.ones(n, D))
        self.norm2_bias = Parameter(torch.zeros(n, D))
        self.out_weight = Parameter(torch.empty(n, D, D))
        self.out_bias = Parameter(torch.zeros(n, D))

    def _reset_weights(self):
        # drawn on the CPU generator (so a seed gives the same parameters on any device),
        # then moved: the two tables N(0, 0.01) like SASRec's, the projections N(0, 0.02);
        # biases and the relative bias zero, the LayerNorms 1 / 0
        self._draw_items(0.01)
        with torch.no_grad():
            torch.nn.init.normal_(self.p_embeddings.weight, mean=0.0, std=0.01)
            torch.nn.init.normal_(self.uvqk_weight, mean=0.0, std=0.02)
            torch.nn.init.normal_(self.out_weight, mean=0.0, std=0.02)
        if self.build_device is not None:
            self.p_embeddings.to(self.build_device)
            for name in _STACKED:
                p = getattr(self, name)
                p.data = p.data.to(self.build_device)

    def _encode(self, rows: Tensor, his: Tensor, his_len: Tensor) -> Tensor:
        return dense_ops.hstu_encode(rows, his, his_len, self)
