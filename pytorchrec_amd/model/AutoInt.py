"""AutoInt+: multi-head self-attention over the feature fields beside an MLP (Song et al.,
CIKM 2019).

Absent from the reference; built from its primitives like ``XDeepFM``: one ``EmbeddingBank``
with the first-order weight as an extra column, the reference ``MLP`` over the embedding
concat and the dense columns, ``Linear(last, 1)``, and the interacting stack over the m sparse
fields:

    X^0     = the embedding rows                                       [B, m, D]
    Q, K, V = X^(k-1) Wq^T, X^(k-1) Wk^T, X^(k-1) Wv^T                   heads of att_head_dim
    P_h     = softmax over the keys of scale * Q_h K_h^T               [B, m, m] per head
    X^k     = relu([P_1 V_1 | .. | P_H V_H] + X^(k-1) Wres^T)          [B, m, A], k = 1 .. L
    logit   = global_bias + dense . w_dense + sum_f w_f[id_f] + att_out(X^L) + prediction(mlp(x0))

No mask, bias, dropout or LayerNorm inside a layer, as in the paper; ``att_scaling`` adds the
transformer's ``head_dim ** -0.5`` (the paper has none).  Dense columns feed the MLP and the
linear term only.  x0 and the first-order term come from the one ``interact`` launch
(fm2=False); the stack reads the first m * D columns of its rows.  On a GPU the stack is
``dense.autoint``: mrec_autoint_fwd / mrec_autoint_bwd (csrc/autoint.hip), one call per layer
each way, for 2 <= m <= 32 fields, emb_size in {8, 16, 32, 64}, A = att_heads * att_head_dim in
{16, 32, 64}, att_head_dim in {8, 16, 32} and at most 4 layers; any other shape (more than 32
sparse fields among them) runs the same arithmetic as torch ops chunked over the batch
(``cpu_path.autoint``, also the CPU path).  Row-sharded banks (``sharded_tables``) are not
supported.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import Tensor
from torch.nn import Linear, Module, ModuleList, Parameter

from pytorchrec_amd import dense as dense_ops
from pytorchrec_amd import sharding
from pytorchrec_amd.embedding import EmbeddingBank, interact
from pytorchrec_amd.feature_column import CategoricalColumn, NumericColumn
from pytorchrec_amd.model.DeepFM import _CTRBase, _parse_layers, _round_up
from pytorchrec_amd.model.layer.MLP import MLP
from pytorchrec_amd.utils.argument import ArgumentDescription


class _InteractingLayer(Module):
    """The four projections of one layer (``res`` only with ``att_res``); ``dense.autoint``
    does the arithmetic."""

    def __init__(self, d_in: int, A: int, res: bool):
        super().__init__()
        self.query = Linear(d_in, A, bias=False)
        self.key = Linear(d_in, A, bias=False)
        self.value = Linear(d_in, A, bias=False)
        if res:
            self.res = Linear(d_in, A, bias=False)

    def weights(self):
        return (self.query.weight, self.key.weight, self.value.weight,
                self.res.weight if hasattr(self, "res") else None)


class AutoInt(_CTRBase):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [
            ArgumentDescription(name="emb_size", type_=int, help_info="embedding dim",
                                default_value=16, lower_closed_bound=1),
            ArgumentDescription(name="layers", type_=str, help_info="MLP widths, e.g. 400,400",
                                default_value="400,400"),
            ArgumentDescription(name="att_layers", type_=int, help_info="interacting layers",
                                default_value=3, lower_closed_bound=1),
            ArgumentDescription(name="att_heads", type_=int, help_info="attention heads per layer",
                                default_value=2, lower_closed_bound=1),
            ArgumentDescription(name="att_head_dim", type_=int, help_info="columns per head",
                                default_value=32, lower_closed_bound=1),
            ArgumentDescription(name="att_res", type_=bool,
                                help_info="residual projection in every interacting layer",
                                default_value=True),
            ArgumentDescription(name="att_scaling", type_=bool,
                                help_info="scale the scores by head_dim ** -0.5 (the paper: no)",
                                default_value=False),
            ArgumentDescription(name="dropout", type_=float, help_info="MLP dropout",
                                default_value=0.0, lower_closed_bound=0.0, upper_open_bound=1.0),
        ]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, sparse_columns: Sequence[CategoricalColumn],
                 dense_columns: Optional[Sequence[NumericColumn]] = None, label_column=None,
                 emb_size: int = 16, layers=(400, 400), att_layers: int = 3, att_heads: int = 2,
                 att_head_dim: int = 32, att_res: bool = True, att_scaling: bool = False,
                 att_size: Optional[int] = None, dropout: float = 0.0,
                 emb_dtype: torch.dtype = torch.float32, device=None, **kwargs):
        self._setup_columns(sparse_columns, dense_columns, label_column, emb_size, emb_dtype,
                            device)
        self.layers = _parse_layers(layers)
        self.att_layers, self.att_heads = int(att_layers), int(att_heads)
        self.att_head_dim = int(att_head_dim)
        self.att_res, self.att_scaling = bool(att_res), bool(att_scaling)
        self.dropout = float(dropout)
        if not self.sparse_columns:
            raise ValueError("AutoInt needs at least one sparse column")
        if self.att_layers < 1 or self.att_heads < 1 or self.att_head_dim < 1:
            raise ValueError("att_layers, att_heads and att_head_dim must be positive")
        if att_size is not None and int(att_size) != self.att_heads * self.att_head_dim:
            raise ValueError(f"att_size {att_size} is not att_heads * att_head_dim = "
                             f"{self.att_heads} * {self.att_head_dim}")
        if not self.layers:
            raise ValueError("layers must name at least one hidden width")
        super().__init__(**kwargs)

    def _init_weights(self):
        if sharding._ACTIVE:
            raise NotImplementedError("AutoInt does not support row-sharded banks "
                                      "(sharded_tables): the interacting layers read whole rows "
                                      "of every field on the sample's own rank")
        dev = self.build_device
        m, D, n = len(self.sparse_columns), self.emb_size, len(self.dense_columns)
        self.embeddings = EmbeddingBank([c.category_num for c in self.sparse_columns], D,
                                        with_first_order=True, dtype=self.emb_dtype, device=dev)
        self.dense_weight = Parameter(torch.randn(n, device=dev) * 0.01) if n else None
        self.global_bias = Parameter(torch.zeros(1, device=dev))
        self.deep_in = m * D + n
        self.x0_cols = _round_up(self.deep_in, 8)  # 16-byte aligned rows; pad is zero
        A = self.att_heads * self.att_head_dim
        self.att_size = A
        self.att = ModuleList([_InteractingLayer(D if k == 0 else A, A, self.att_res)
                               for k in range(self.att_layers)])
        self.att_out = Linear(m * A, 1, bias=False)
        self.mlp = MLP(self.deep_in, self.layers, "relu", self.dropout)
        self.prediction = Linear(self.layers[-1], 1)

    def _reset_weights(self):
        # IModel._reset_weights_fn over the modules: every Linear, the attention projections
        # among them, is normal(0, 0.01), drawn on the CPU generator and moved
        super()._reset_weights()
        if self.build_device is not None:
            for mod in (self.att, self.att_out, self.mlp, self.prediction):
                mod.to(self.build_device)

    def _parts(self, data: Dict[str, Tensor], dense, with_linear: bool):
        """x0 [B, x0_cols] and the base logit: first order (+ the dense linear term and the
        global bias when ``with_linear``) + the interacting stack's."""
        lin = (self.dense_weight, self.global_bias) if with_linear else (None, None)
        x0, logit = interact(self.embeddings, self._ids(data), dense, *lin, fm2=False,
                             first_order=True, x0_cols=self.x0_cols, x0_dtype=self._x0_dtype())
        m = len(self.sparse_columns)
        scale = self.att_head_dim ** -0.5 if self.att_scaling else 1.0
        y = dense_ops.autoint(x0[:, :m * self.emb_size], m, [l.weights() for l in self.att],
                              self.att_heads, scale)
        return x0, dense_ops.head(y, self.att_out.weight, None, base=logit)

    def forward(self, data: Dict[str, Tensor]):
        x0, base = self._parts(data, self._dense(data), True)
        prediction = dense_ops.head(self.mlp(x0), self.prediction.weight, self.prediction.bias,
                                    base=base)
        return prediction, self._target(data)

    def fused_bce_loss(self, data: Dict[str, Tensor]):
        """Training loss (BCE with logits, mean): the MLP, the output layer, the dense
        first-order term + global bias and the loss in one fused tower launch, with the
        first-order and attention logits as its base, as in ``XDeepFM``."""
        dense = self._dense(data)
        x0, base = self._parts(data, dense, False)
        if dense_ops.tower_supported(x0, self.mlp, self.prediction, dense):
            return dense_ops.tower_bce(x0, self.mlp, self.prediction, base, self._target(data),
                                       xs=dense, ws=self.dense_weight, b2=self.global_bias)
        loss, _ = dense_ops.ctr_head_bce(self.mlp(x0), self.prediction.weight, self.prediction.bias,
                                         base, self._target(data), xs=dense, ws=self.dense_weight,
                                         b2=self.global_bias)
        return loss
