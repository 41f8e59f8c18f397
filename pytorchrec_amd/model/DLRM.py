"""DLRM: bottom MLP, pairwise dot interaction, top MLP (Naumov et al., 2019).

Absent from the reference; built from its primitives like ``DCNv2``: one ``EmbeddingBank``
for the sparse fields (``nn.Embedding`` semantics, no first-order column), the reference
``MLP`` (Linear -> ReLU -> Dropout per layer, so the reference initialisation applies) for
both towers, then ``Linear(last, 1)``.

    bot        = bottom_mlp(dense)                          [B, emb_size]
    t          = [bot, v_0 .. v_{F-1}]                      n = F + 1 vectors
    x          = [bot | t_i . t_j for j < i | 0 pad]        emb_size + n (n - 1) / 2 columns
    prediction = Linear(top_mlp(x))

The last bottom width must equal ``emb_size``.  With no dense columns there is no bottom MLP
and the interaction runs over the F embedding rows alone.  On a GPU the interaction is one
launch each way (``dense.dot_interact``: mrec_dot_interact_fwd / _bwd,
csrc/dot_interact.hip) for emb_size in {8, 16, 32, 64, 128} and up to 31 fields; any other
shape runs the same arithmetic as torch ops (``cpu_path.dot_interact``, also the CPU path).
Row-sharded banks (``sharded_tables``) are not supported.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import Tensor
from torch.nn import Linear

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd import sharding
from pytorchrec_amd.embedding import EmbeddingBank, gather
from pytorchrec_amd.feature_column import CategoricalColumn, NumericColumn
from pytorchrec_amd.model.DeepFM import _CTRBase, _parse_layers, _round_up
from pytorchrec_amd.model.layer.MLP import MLP
from pytorchrec_amd.utils.argument import ArgumentDescription


class DLRM(_CTRBase):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="embedding dim",
                                default_value=16, lower_closed_bound=1),
            ArgumentDescription(name="bottom_layers", type_=str,
                                help_info="bottom MLP widths; the last equals emb_size",
                                default_value="512,256,64,16"),
            ArgumentDescription(name="top_layers", type_=str, help_info="top MLP widths",
                                default_value="512,256"),
            ArgumentDescription(name="dropout", type_=float, help_info="MLP dropout",
                                default_value=0.0, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, sparse_columns: Sequence[CategoricalColumn],
                 dense_columns: Optional[Sequence[NumericColumn]] = None, label_column=None,
                 emb_size: int = 16, bottom_layers="512,256,64,16", top_layers="512,256",
                 dropout: float = 0.0, emb_dtype: torch.dtype = torch.float32, device=None,
                 **kwargs):
        self._setup_columns(sparse_columns, dense_columns, label_column, emb_size, emb_dtype,
                            device)
        self.bottom_layers = _parse_layers(bottom_layers)
        self.top_layers = _parse_layers(top_layers)
        self.dropout = float(dropout)
        if not self.sparse_columns:
            raise ValueError("DLRM needs at least one sparse column")
        if not self.top_layers:
            raise ValueError("top_layers must name at least one hidden width")
        if self.dense_columns and (not self.bottom_layers
                                   or self.bottom_layers[-1] != self.emb_size):
            raise ValueError(f"the last bottom_layers width must equal emb_size = {self.emb_size}, "
                             f"got {self.bottom_layers}")
        super().__init__(**kwargs)

    def _init_weights(self):
        if sharding._ACTIVE:
            raise NotImplementedError("DLRM does not support row-sharded banks "
                                      "(sharded_tables): the dot interaction reads whole rows "
                                      "of every field on the sample's own rank")
        dev = self.build_device
        F, D, nd = len(self.sparse_columns), self.emb_size, len(self.dense_columns)
        self.embeddings = EmbeddingBank([c.category_num for c in self.sparse_columns], D,
                                        with_first_order=False, dtype=self.emb_dtype, device=dev)
        self.bottom_mlp = MLP(nd, self.bottom_layers, "relu", self.dropout) if nd else None
        n = F + (1 if nd else 0)
        self.top_in = (D if nd else 0) + n * (n - 1) // 2
        self.x_cols = _round_up(self.top_in, 8)  # 16-byte aligned rows; the pad is zero
        self.top_mlp = MLP(self.top_in, self.top_layers, "relu", self.dropout)
        self.prediction = Linear(self.top_layers[-1], 1)
        if dev is not None:
            for m in (self.bottom_mlp, self.top_mlp, self.prediction):
                if m is not None:
                    m.to(dev)

    def _x(self, data: Dict[str, Tensor]):
        """The top MLP's input [B, x_cols]."""
        act = self._x0_dtype()
        rows = gather(self.embeddings, self._ids(data), out_dtype=act)
        bot = self.bottom_mlp(self._dense(data)) if self.bottom_mlp is not None else None
        return dense_ops.dot_interact(bot, rows, len(self.sparse_columns), x_cols=self.x_cols,
                                      x_dtype=act)

    def forward(self, data: Dict[str, Tensor]):
        h = self.top_mlp(self._x(data))
        return dense_ops.head(h, self.prediction.weight, self.prediction.bias), self._target(data)

    def fused_bce_loss(self, data: Dict[str, Tensor]):
        """Training loss (BCE with logits, mean): the top MLP, the output layer and the loss
        as one fused tower launch when the tower covers the shape, else the output layer
        fused into the loss."""
        x = self._x(data)
        if dense_ops.tower_supported(x, self.top_mlp, self.prediction):
            return dense_ops.tower_bce(x, self.top_mlp, self.prediction, None, self._target(data))
        loss, _ = dense_ops.ctr_head_bce(self.top_mlp(x), self.prediction.weight,
                                         self.prediction.bias, None, self._target(data))
        return loss
