"""LightGCN on the hot path (He et al., "LightGCN: Simplifying and Powering Graph
Convolution Network for Recommendation", SIGIR 2020):

    E        = graph.propagate(G, E0, n_layers)  =  1/(K+1) sum_{k<=K} A^^k E0
    score    = E[u] . E[n_users + i]

E0 is FunkSVD's two-table bank (users, then items: exactly the node table), with
FunkSVD's state-dict keys and initialisation, so a FunkSVD checkpoint loads as E0.  The
propagation is K launches of ``mrec_graph_prop`` each way on a GPU (pytorchrec_amd/graph.py).

Everything else is FunkSVD's, reading a *propagated bank* through ``_bank()``: a
two-table ``EmbeddingBank`` whose ``weight`` is this step's ``E``, a plain tensor in the
autograd graph and not a parameter.  The fused ``interact`` / ``gather`` launches read it,
their deterministic dense-gradient backward delivers ``dE``, and autograd carries that
through the propagation into ``embeddings.weight.grad``.  The propagated bank is no
sub-module: it does not appear in ``parameters()``, ``state_dict()`` or
``embedding_banks()``.

E0 trains by its dense gradient and the torch optimizer (the gradient reaches every node
within K hops of the batch; use the optimizer's ``weight_decay`` for the L2 term).  In
eval mode ``E`` is computed once and kept until the weights or the graph change.
"""
from typing import Any, Dict, List

import torch

from pytorchrec_amd import graph as graph_ops
from pytorchrec_amd.embedding import EmbeddingBank
from pytorchrec_amd.model.FunkSVD import FunkSVD
from pytorchrec_amd.utils.argument import ArgumentDescription


class PropagatedBank(EmbeddingBank):
    """A bank-shaped view of a computed table: ``weight`` is set per step and is no parameter."""

    def __init__(self, category_nums, dim: int):
        super().__init__(category_nums, dim, dtype=torch.float32, update="dense", device="meta")
        del self._parameters["weight"]
        self.weight = None


class LightGCN(FunkSVD):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return super().get_argument_descriptions() + [
            ArgumentDescription(name="n_layers", type_=int, help_info="propagation layers",
                                default_value=3, lower_closed_bound=0)]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, uid_column, iid_column, label_column, emb_size: int, n_layers: int = 3,
                 layer_dtype=None, emb_dtype: torch.dtype = torch.float32, **kwargs):
        if emb_dtype != torch.float32:
            raise ValueError(f"LightGCN's node table is fp32, got emb_dtype={emb_dtype} "
                             "(layer_dtype=torch.bfloat16 stores the propagated layers in bf16)")
        if int(n_layers) < 0:
            raise ValueError(f"n_layers must be >= 0, got {n_layers}")
        if layer_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"layer_dtype must be None, float32 or bfloat16, got {layer_dtype}")
        self.n_layers = int(n_layers)
        self.layer_dtype = layer_dtype
        super().__init__(uid_column, iid_column, label_column, emb_size, emb_dtype=emb_dtype,
                         **kwargs)
        # (kept out of _modules: not a sub-module, see the module docstring)
        self.__dict__["_propagated"] = PropagatedBank(self.embeddings.category_nums, emb_size)
        self.__dict__["_graph"] = None
        self.__dict__["_eval_table"] = None  # (table, the E0 version it was computed from)

    # -- the graph --------------------------------------------------------------------
    def set_graph(self, u_ids, i_ids):
        """The training interactions (user ids, item ids); duplicates are removed."""
        self.__dict__["_graph"] = graph_ops.BipartiteGraph.from_interactions(
            u_ids, i_ids, self.uid_column.category_num, self.iid_column.category_num)
        self.__dict__["_eval_table"] = None
        return self

    @property
    def graph(self):
        return self._graph

    # -- the propagated table ---------------------------------------------------------
    def propagated_table(self) -> torch.Tensor:
        """``E [N, row_stride]``: in training mode this step's, in the autograd graph; in
        eval mode computed once without one and reused until ``train()``,
        ``load_state_dict``, ``set_graph`` or any in-place change of E0."""
        if self._graph is None:
            raise RuntimeError("LightGCN has no graph: call set_graph(u_ids, i_ids) with the "
                               "training interactions first")
        w = self.embeddings.weight
        if self._graph.device != w.device:
            self.__dict__["_graph"] = self._graph.to(w.device)
        if self.training:
            return graph_ops.propagate(self._graph, w, self.n_layers, self.layer_dtype,
                                       dim=self.emb_size)
        key = (w._version, w.data_ptr())
        if self._eval_table is None or self._eval_table[1] != key:
            with torch.no_grad():
                t = graph_ops.propagate(self._graph, w.detach(), self.n_layers, self.layer_dtype,
                                        dim=self.emb_size)
            self.__dict__["_eval_table"] = (t, key)
        return self._eval_table[0]

    def _bank(self) -> EmbeddingBank:
        bank = self._propagated
        bank.weight = self.propagated_table()
        return bank

    def train(self, mode: bool = True):
        if mode:
            self.__dict__["_eval_table"] = None
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.__dict__["_eval_table"] = None
        return super().load_state_dict(*args, **kwargs)

    # -- the update ---------------------------------------------------------------------
    def _configure_embedding_update(self, optimizer):
        # the gradient of a step touches every node within K hops of its batch: a
        # row-sparse fused update does not apply, the torch optimizer takes the dense one
        self.embeddings.use_dense_grad()
