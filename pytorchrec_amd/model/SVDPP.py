"""SVD++ on the hot path — the reference's implicit-feedback model
(torchrec/model/SVDPP.py:12-91).

    prediction = (u + imp) . i + u_bias + i_bias + global_bias
    imp        = sum_{valid j} implicit_i[iids_j] / sqrt(valid count)      (SVDPP.py:49-55)

The explicit part ``u . i + u_bias + i_bias + global_bias`` is one fused interaction
launch: the 2-field FM over {uid, iid} is ``u . i`` and the two bias
tables are the bank's packed first-order column.  The same launch returns the
gathered ``i`` rows in ``x0``.  The history term is one pooled lookup
(``pooled_gather``, mode "sqrtn", id 0 = padding), and the last ``[B, D]`` row dot
``imp . i`` is ordinary torch, whose autograd feeds ``dx0`` to the interaction's
backward and ``dimp`` to the pooled backward.  An empty history contributes a zero
vector (the reference: NaN).

Both branches of the reference ``forward``:
  * single item, ``iid`` [B]: prediction [B], target = label.float();
  * sampled, ``iid`` [B, N] (SVDPP.py:72-89): the history is pooled once per sample
    and repeated for its N candidates, like the user row; prediction [B, N], target
    [B, N] float32 with column 0 = 1.

Checkpoint compatibility: ``state_dict`` / ``load_state_dict`` speak the reference's
keys (``u_embeddings.weight``, ``i_embeddings.weight``, ``implicit_i_embeddings.weight``,
``u_bias.weight`` [U, 1], ``i_bias.weight`` [I, 1], ``global_bias``).  Initialisation
consumes the CPU RNG in the reference's order (the five ``nn.Embedding``
constructions, then ``IModel._reset_weights`` over them in the same order), so the
same ``random_seed`` gives bit-identical tables (pinned by golden G13).
"""
from typing import Any, Dict, List

import torch
from torch import Tensor
from torch.nn import Parameter

from pytorchrec_amd.embedding import EmbeddingBank, gather, interact, pooled_gather
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.utils.argument import ArgumentDescription

_BANK_KEY, _IMP_BANK_KEY = "embeddings.weight", "implicit_i_embeddings.weight"
_U_KEY, _I_KEY = "u_embeddings.weight", "i_embeddings.weight"
_UB_KEY, _IB_KEY, _GB_KEY = "u_bias.weight", "i_bias.weight", "global_bias"


def _state_dict_hook(module, state_dict, prefix, local_metadata):
    """The packed banks -> the reference's five tables; global_bias as its 0-d scalar."""
    w = state_dict.pop(prefix + _BANK_KEY, None)
    nu, D = module.uid_column.category_num, module.emb_size
    if w is not None:
        state_dict[prefix + _U_KEY] = w[:nu, :D].clone()
        state_dict[prefix + _I_KEY] = w[nu:, :D].clone()
        state_dict[prefix + _UB_KEY] = w[:nu, D:D + 1].clone()
        state_dict[prefix + _IB_KEY] = w[nu:, D:D + 1].clone()
    imp = state_dict.get(prefix + _IMP_BANK_KEY)
    if imp is not None:
        state_dict[prefix + _IMP_BANK_KEY] = imp[:, :D].clone()
    gb = state_dict.get(prefix + _GB_KEY)
    if gb is not None:
        state_dict[prefix + _GB_KEY] = gb.reshape(()).clone()
    return state_dict


def _load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys,
                   unexpected_keys, error_msgs):
    """The reference keys -> the packed bank weights (a packed key passes through)."""
    nu, D = module.uid_column.category_num, module.emb_size
    bank, imp_bank = module.embeddings, module.implicit_i_embeddings
    ref_keys = (_U_KEY, _I_KEY, _UB_KEY, _IB_KEY)
    if any(prefix + k in state_dict for k in ref_keys):
        w = bank.weight.detach().clone()
        rows = {_U_KEY: slice(0, nu), _UB_KEY: slice(0, nu),
                _I_KEY: slice(nu, bank.total_rows), _IB_KEY: slice(nu, bank.total_rows)}
        for k in ref_keys:
            t = state_dict.pop(prefix + k, None)
            if t is None:
                if strict:
                    missing_keys.append(prefix + k)
                continue
            sl = rows[k]
            cols = slice(0, D) if k in (_U_KEY, _I_KEY) else slice(D, D + 1)
            want = (sl.stop - sl.start, cols.stop - cols.start)
            if tuple(t.shape) != want:
                error_msgs.append(f"size mismatch for {prefix + k}: copying a param with shape "
                                  f"{tuple(t.shape)}, the shape in current model is {want}.")
                continue
            w[sl, cols] = t.to(device=w.device, dtype=w.dtype)
        state_dict[prefix + _BANK_KEY] = w
    t = state_dict.get(prefix + _IMP_BANK_KEY)
    if t is not None and t.dim() == 2 and t.shape[1] == D and imp_bank.row_stride != D:
        w = imp_bank.weight.detach().clone()
        if t.shape[0] == w.shape[0]:
            w[:, :D] = t.to(device=w.device, dtype=w.dtype)
            state_dict[prefix + _IMP_BANK_KEY] = w
    gb = state_dict.get(prefix + _GB_KEY)
    if gb is not None and gb.dim() == 0:
        state_dict[prefix + _GB_KEY] = gb.reshape(1)


class SVDPP(IModel):
    @classmethod
    def get_argument_descriptions(cls) -> List[ArgumentDescription]:
        return [ArgumentDescription(name="emb_size", type_=int, help_info="Embedding层维度",
                                    default_value=64, lower_closed_bound=1)]

    @classmethod
    def check_argument_values(cls, arguments: Dict[str, Any]) -> None:
        super().check_argument_values(arguments)

    def __init__(self, uid_column, iid_column, iids_column, label_column, emb_size: int,
                 emb_dtype: torch.dtype = torch.float32, device=None, **kwargs):
        self.uid_column = uid_column
        self.iid_column = iid_column
        self.iids_column = iids_column
        self.label_column = label_column
        self.emb_size = emb_size
        self.emb_dtype = emb_dtype
        self.build_device = device
        super().__init__(**kwargs)
        self._register_state_dict_hook(_state_dict_hook)
        self._register_load_state_dict_pre_hook(_load_pre_hook, with_module=True)

    def _init_weights(self):
        nu, ni = self.uid_column.category_num, self.iid_column.category_num
        # tables u and i with their biases as the packed first-order column
        self.embeddings = EmbeddingBank([nu, ni], self.emb_size, with_first_order=True,
                                        dtype=self.emb_dtype, device=self.build_device)
        self.implicit_i_embeddings = EmbeddingBank([ni], self.emb_size, dtype=self.emb_dtype,
                                                   device=self.build_device)
        self.global_bias = Parameter(torch.zeros(1, device=self.build_device))
        # the nn.Embedding constructors draw N(0, 1) per table: keep the RNG stream
        # where the reference has it
        self._init_tables(1.0)

    def _init_tables(self, std: float):
        """normal(0, std) per table in the reference's order (u, i, implicit, u_bias,
        i_bias: SVDPP.py:37-41), drawn on the CPU default generator in the reference's
        shapes like its CPU-built model, then copied."""
        nu, ni, D = self.uid_column.category_num, self.iid_column.category_num, self.emb_size
        bank, imp = self.embeddings, self.implicit_i_embeddings

        def draw(rows, cols):
            t = torch.empty(rows, cols)
            torch.nn.init.normal_(t, mean=0.0, std=std)
            return t

        with torch.no_grad():
            bank.weight.zero_()  # row padding stays zero
            imp.weight.zero_()
            bank.table(0).copy_(draw(nu, D).to(bank.weight.dtype))
            bank.table(1).copy_(draw(ni, D).to(bank.weight.dtype))
            imp.table(0).copy_(draw(ni, D).to(imp.weight.dtype))
            bank.first_order(0).copy_(draw(nu, 1)[:, 0].to(bank.weight.dtype))
            bank.first_order(1).copy_(draw(ni, 1)[:, 0].to(bank.weight.dtype))

    def _reset_weights(self):
        # IModel._reset_weights_fn visits the five Embedding modules in registration
        # order (IModel.py:61-68): normal(0, 0.01) each; global_bias stays 0
        self._init_tables(0.01)

    def _pooled_history(self, data: Dict[str, Tensor]) -> Tensor:
        iids = self.iids_column.get_feature_ids(data)
        return pooled_gather(self.implicit_i_embeddings, [iids], mode="sqrtn", pad="zero",
                             out_dtype=torch.float32)

    candidate_lists = True

    def set_shared_negatives(self, source, n_shared=None, iid_column=None):
        """Not available: SVD++'s score carries a LEARNED item bias, b_i, while the shared-
        negative losses add only constant biases to ``q . row`` (they get no gradient), so
        b_i would not train.  Train SVD++ pair-wise (``set_negative_sampler``)."""
        if source is None:
            return super().set_shared_negatives(None)
        raise NotImplementedError("SVDPP scores with a learned item bias, which the shared-"
                                  "negative losses (constant biases only) cannot train")

    def _retrieval_query(self, data: Dict[str, Tensor]):
        """``recommend``: score = (u + imp) . i + b_i, plus b_u + global_bias per sample;
        b_i is the item table's packed first-order column."""
        u_ids = self.uid_column.get_feature_ids(data)
        rows, w = gather(self.embeddings, [u_ids, torch.zeros_like(u_ids)],
                         out_dtype=torch.float32, with_w=True)
        q = rows[:, :self.emb_size] + self._pooled_history(data)
        return q, self.embeddings, 1, True, w[:, 0] + self.global_bias

    def forward(self, data: Dict[str, Tensor]):
        u_ids = self.uid_column.get_feature_ids(data)
        i_ids = self.iid_column.get_feature_ids(data)
        D = self.emb_size
        imp = self._pooled_history(data)  # [B, D]
        sampled = i_ids.dim() != 1
        if sampled:
            # (SVDPP.py:72-89) every (sample, candidate) pair is one interaction row
            B, N = i_ids.shape
            u_ids = u_ids.reshape(B, 1).expand(B, N).reshape(-1).contiguous()
            i_ids = i_ids.reshape(-1).contiguous()
            imp = imp.unsqueeze(1).expand(B, N, D).reshape(B * N, D)
        x0, logit = interact(self.embeddings, [u_ids, i_ids], bias=self.global_bias, fm2=True,
                             first_order=True, x0_cols=2 * D, x0_dtype=self.embeddings.weight.dtype)
        prediction = logit + (imp * x0[:, D:2 * D].float()).sum(dim=-1)
        if sampled:
            prediction = prediction.reshape(B, N)
            target = torch.zeros_like(prediction, dtype=torch.float32)
            target[:, 0] = 1
            return prediction, target
        target = None
        if self.label_column is not None and self.label_column.feature_name in data:
            target = data[self.label_column.feature_name].float()
        return prediction, target
