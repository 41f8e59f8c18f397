"""xDeepFM: a Compressed Interaction Network beside DeepFM's linear part and MLP (Lian et
al., KDD 2018).

Absent from the reference; built from its primitives like ``DeepFM``: one ``EmbeddingBank``
with the first-order weight as an extra column, the reference ``MLP`` over the embedding
concat and the dense columns, ``Linear(last, 1)``, and the CIN over the m sparse fields:

    X^0        = the embedding rows                          [B, m, D]
    X^k[h]     = sum_{i, j} W^k[h, i, j] X^{k-1}[i] * X^0[j]   (element-wise over D), k = 1 .. L
    p          = [sum_d X^1 | .. | sum_d X^L]                [B, sum_k H_k]
    logit      = global_bias + dense . w_dense + sum_f w_f[id_f] + cin_out(p) + prediction(mlp(x0))

Identity activation, no bias, every map feeds both the output and the next layer (the
paper's "direct" connection, no split_half).  Dense columns feed the MLP and the linear term
only.  x0 and the first-order term come from the one ``interact`` launch (fm2=False); the CIN
reads the first m * D columns of its rows.  On a GPU the CIN is ``dense.cin``: mrec_cin_fwd /
mrec_cin_bwd (csrc/cin.hip), one call per layer each way, for 2 <= m <= 32 fields, emb_size in
{8, 16, 32, 64}, layer widths that are multiples of 8 up to 256 and at most 4 layers; any other
shape runs the same arithmetic as torch ops chunked over the batch (``cpu_path.cin``, also the
CPU path).  Row-sharded banks (``sharded_tables``) are not supported.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import Tensor
from torch.nn import Linear, Parameter, ParameterList

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd import sharding
from pytorchrec_amd.embedding import EmbeddingBank, interact
from pytorchrec_amd.feature_column import CategoricalColumn, NumericColumn
from pytorchrec_amd.model.DeepFM import _CTRBase, _parse_layers, _round_up
from pytorchrec_amd.model.layer.MLP import MLP
from pytorchrec_amd.utils.argument import ArgumentDescription


class XDeepFM(_CTRBase):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="embedding dim",
                                default_value=16, lower_closed_bound=1),
            ArgumentDescription(name="layers", type_=str, help_info="MLP widths, e.g. 400,400",
                                default_value="400,400"),
            ArgumentDescription(name="cin_layers", type_=str,
                                help_info="CIN feature maps per layer, e.g. 200,200,200",
                                default_value="200,200,200"),
            ArgumentDescription(name="dropout", type_=float, help_info="MLP dropout",
                                default_value=0.0, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, sparse_columns: Sequence[CategoricalColumn],
                 dense_columns: Optional[Sequence[NumericColumn]] = None, label_column=None,
                 emb_size: int = 16, layers=(400, 400), cin_layers="200,200,200",
                 dropout: float = 0.0, emb_dtype: torch.dtype = torch.float32, device=None,
                 **kwargs):
        self._setup_columns(sparse_columns, dense_columns, label_column, emb_size, emb_dtype,
                            device)
        self.layers = _parse_layers(layers)
        self.cin_layers = _parse_layers(cin_layers)
        self.dropout = float(dropout)
        if not self.sparse_columns:
            raise ValueError("XDeepFM needs at least one sparse column")
        if not self.cin_layers or any(h < 1 for h in self.cin_layers):
            raise ValueError("cin_layers must name at least one positive width")
        if not self.layers:
            raise ValueError("layers must name at least one hidden width")
        super().__init__(**kwargs)

    def _init_weights(self):
        if sharding._ACTIVE:
            raise NotImplementedError("XDeepFM does not support row-sharded banks "
                                      "(sharded_tables): the CIN reads whole rows "
                                      "of every field on the sample's own rank")
        dev = self.build_device
        m, D, n = len(self.sparse_columns), self.emb_size, len(self.dense_columns)
        self.embeddings = EmbeddingBank([c.category_num for c in self.sparse_columns], D,
                                        with_first_order=True, dtype=self.emb_dtype, device=dev)
        self.dense_weight = Parameter(torch.randn(n, device=dev) * 0.01) if n else None
        self.global_bias = Parameter(torch.zeros(1, device=dev))
        self.deep_in = m * D + n
        self.x0_cols = _round_up(self.deep_in, 8)  # 16-byte aligned rows; pad is zero
        widths = [m] + self.cin_layers
        self.cin_weights = ParameterList(
            [Parameter(torch.empty(widths[k + 1], widths[k], m)) for k in range(len(self.cin_layers))])
        self.cin_out = Linear(sum(self.cin_layers), 1, bias=False)
        self.mlp = MLP(self.deep_in, self.layers, "relu", self.dropout)
        self.prediction = Linear(self.layers[-1], 1)

    def _reset_weights(self):
        # IModel._reset_weights_fn over the modules, then the CIN maps the same way:
        # normal(0, 0.01), drawn on the CPU generator and moved
        super()._reset_weights()
        for w in self.cin_weights:
            torch.nn.init.normal_(w, mean=0.0, std=0.01)
        if self.build_device is not None:
            for mod in (self.cin_weights, self.cin_out, self.mlp, self.prediction):
                mod.to(self.build_device)

    def _parts(self, data: Dict[str, Tensor], dense, with_linear: bool):
        """x0 [B, x0_cols] and the base logit: first order (+ the dense linear term and the
        global bias when ``with_linear``) + the CIN's."""
        lin = (self.dense_weight, self.global_bias) if with_linear else (None, None)
        x0, logit = interact(self.embeddings, self._ids(data), dense, *lin, fm2=False,
                             first_order=True, x0_cols=self.x0_cols, x0_dtype=self._x0_dtype())
        m = len(self.sparse_columns)
        p = dense_ops.cin(x0[:, :m * self.emb_size], m, list(self.cin_weights))
        return x0, dense_ops.head(p, self.cin_out.weight, None, base=logit)

    def forward(self, data: Dict[str, Tensor]):
        x0, base = self._parts(data, self._dense(data), True)
        prediction = dense_ops.head(self.mlp(x0), self.prediction.weight, self.prediction.bias,
                                    base=base)
        return prediction, self._target(data)

    def fused_bce_loss(self, data: Dict[str, Tensor]):
        """Training loss (BCE with logits, mean): the MLP, the output layer, the dense
        first-order term + global bias and the loss in one fused tower launch, with the
        first-order and CIN logits as its base, as in ``DeepFM``."""
        dense = self._dense(data)
        x0, base = self._parts(data, dense, False)
        if dense_ops.tower_supported(x0, self.mlp, self.prediction, dense):
            return dense_ops.tower_bce(x0, self.mlp, self.prediction, base, self._target(data),
                                       xs=dense, ws=self.dense_weight, b2=self.global_bias)
        loss, _ = dense_ops.ctr_head_bce(self.mlp(x0), self.prediction.weight, self.prediction.bias,
                                         base, self._target(data), xs=dense, ws=self.dense_weight,
                                         b2=self.global_bias)
        return loss
