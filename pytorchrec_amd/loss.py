"""Losses — the reference registry's names (torchrec/loss/losses.py:8-21 registers
BPR / Top1 / MSE) plus the CTR loss it lacks.

``BCEWithLogitsLoss`` is a ``torch.nn.modules.loss._Loss`` (so it passes
``IModel.compile``'s type check, IModel.py:103-104) with exactly
``torch.nn.BCEWithLogitsLoss(reduction="mean")`` semantics; on a GPU its forward
and backward are single libmrec kernels (fixed-order reduction).

``BPRLoss`` / ``Top1Loss`` are the reference's pairwise ranking losses
(torchrec/loss/BPRLoss.py:15-23, Top1Loss.py:14-22): the input is ``[B, 2]`` with the
positive's score in column 0 and the negative's in column 1 (anything else raises
``AssertionError``, as the reference's ``assert`` does), ``target`` is ignored and
may be ``None``, ``reduction`` is ``none`` / ``mean`` / ``sum``.  On the CPU they are
the reference's formulas in torch; on a GPU forward and backward are one libmrec
kernel each (``mrec_pair_loss_fwd`` / ``_bwd``: fp32 arithmetic, a fixed-order
reduction so two runs give the same bits, the upstream gradient read on the
device).

``SharedNegativeLoss`` ranks every query against its own positive and ONE pool of S
negatives shared by the whole batch (sampled softmax, or BPR / Top1 averaged over the
pool; in-batch negatives when the pool is the positives themselves): ``forward(q, pos,
neg, pos_id, neg_id, pos_bias, neg_bias)`` takes the query vectors and the gathered item
rows, not scores.  The contract stands once, in include/mrec.h "Shared negatives".  On a
GPU, for the compiled shapes (``mrec_shneg_supported``), loss and gradients are the fused
kernels of csrc/shneg.hip -- the ``[B, S]`` scores never reach memory -- and everywhere
else ``cpu_path.shared_negative_loss``, the same contract in torch ops.  Registry names:
``softmax_shared``, ``bpr_shared``, ``top1_shared``.
"""
import ctypes
from typing import Dict, Optional, Type

import torch
import torch.nn.functional as F  # noqa
from torch.nn.modules.loss import _Loss, MSELoss  # noqa

from pytorchrec_amd import _mrec, cpu_path


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y):
        z = z.contiguous().float()
        y = y.contiguous().float()
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        _mrec.call("mrec_bce_fwd", z.data_ptr(), y.data_ptr(), z.numel(), loss.data_ptr(),
                   _mrec.stream_handle())
        ctx.save_for_backward(z, y)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        z, y = ctx.saved_tensors
        g = g.contiguous().float().reshape(1)
        dz = torch.empty_like(z)
        _mrec.call("mrec_bce_bwd", z.data_ptr(), y.data_ptr(), z.numel(), g.data_ptr(),
                   dz.data_ptr(), _mrec.stream_handle())
        return dz, None


class BCEWithLogitsLoss(_Loss):
    """Mean binary cross entropy on logits."""

    def __init__(self):
        super().__init__(reduction="mean")

    def forward(self, prediction, target):
        if prediction.is_cuda:
            return _BCEFn.apply(prediction.reshape(-1), target.reshape(-1))
        return torch.nn.functional.binary_cross_entropy_with_logits(prediction.float(),
                                                                    target.float())


_REDUCTIONS = {"none": _mrec.REDUCE_NONE, "mean": _mrec.REDUCE_MEAN, "sum": _mrec.REDUCE_SUM}


class _PairLossFn(torch.autograd.Function):
    """x [B, 2] fp32 on a GPU -> the loss ([B] for ``none``, else a scalar).  The rows
    are read in place through their stride (a ``[B, 2]`` slice of a wider tensor is
    not copied)."""

    @staticmethod
    def forward(ctx, x, kind, reduction):
        B = x.shape[0]
        if x.stride(1) != 1 or (B > 1 and x.stride(0) < 2):
            x = x.contiguous()
        ld = max(int(x.stride(0)), 2)
        out = (torch.empty if B else torch.zeros)(
            B if reduction == _mrec.REDUCE_NONE else 1, dtype=torch.float32, device=x.device)
        if B:  # (an empty batch has no storage to point at: the loss is 0, as the kernel's)
            _mrec.call("mrec_pair_loss_fwd", x.data_ptr(), ld, B, kind, reduction,
                       out.data_ptr(), _mrec.stream_handle())
        ctx.save_for_backward(x)
        ctx.pair = (kind, reduction, ld)
        return out if reduction == _mrec.REDUCE_NONE else out.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        kind, reduction, ld = ctx.pair
        B = x.shape[0]
        g = g.contiguous().float().reshape(-1)
        if reduction == _mrec.REDUCE_NONE and g.numel() != B:
            g = g.expand(B).contiguous()
        dx = torch.empty(B, 2, dtype=torch.float32, device=x.device)
        if B:
            _mrec.call("mrec_pair_loss_bwd", x.data_ptr(), ld, B, kind, reduction, g.data_ptr(),
                       dx.data_ptr(), _mrec.stream_handle())
        return dx, None, None


class _PairLoss(_Loss):
    _kind = None

    def __init__(self, reduction="mean"):
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction参数不合法: {reduction}")
        super().__init__(None, None, reduction)

    def _cpu(self, pos, neg):
        raise NotImplementedError

    def forward(self, input: torch.Tensor, target: torch.Tensor = None):  # noqa
        """input: [B, 2], positive first; target is ignored."""
        assert len(input.shape) == 2 and input.shape[1] == 2, input.shape
        if input.is_cuda:
            return _PairLossFn.apply(input.float(), self._kind, _REDUCTIONS[self.reduction])
        ret = self._cpu(input[:, 0], input[:, 1])
        if self.reduction != "none":
            ret = torch.mean(ret) if self.reduction == "mean" else torch.sum(ret)
        return ret


class BPRLoss(_PairLoss):
    """softplus(neg - pos), torch's softplus (x for x > 20, else log1p(exp(x)))."""
    _kind = _mrec.PAIR_BPR

    def _cpu(self, pos, neg):
        return F.softplus(-(pos - neg))


class Top1Loss(_PairLoss):
    """sigmoid(neg - pos) + sigmoid(neg^2)."""
    _kind = _mrec.PAIR_TOP1

    def _cpu(self, pos, neg):
        return torch.sigmoid(neg - pos) + torch.sigmoid(neg * neg)


# ---------------------------------------------------------------------------
# shared negatives
# ---------------------------------------------------------------------------
_SHNEG_KINDS = {"softmax": _mrec.SHNEG_SOFTMAX, "bpr": _mrec.SHNEG_BPR, "top1": _mrec.SHNEG_TOP1}


def shneg_tile_queries() -> int:
    return int(_mrec.lib().mrec_shneg_tile_queries())


def shneg_tile_candidates() -> int:
    return int(_mrec.lib().mrec_shneg_tile_candidates())


def shneg_default_splits(batch: int, n_neg: int) -> int:
    return int(_mrec.lib().mrec_shneg_splits(int(batch), int(n_neg)))


def shneg_supported(dim: int, q_dtype: torch.dtype, row_dtype: torch.dtype) -> bool:
    """True when the fused kernels cover (embedding size, q dtype, rows dtype).  Decided
    from the shape alone; never an error."""
    floats = (torch.float32, torch.bfloat16)
    if q_dtype not in floats or row_dtype not in floats or not 0 <= int(dim) < 2 ** 31:
        return False
    return bool(_mrec.lib().mrec_shneg_supported(int(dim), _mrec.dtype_code(q_dtype),
                                                 _mrec.dtype_code(row_dtype)))


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def shneg_call(fn: str, q, pos, neg, kind: int, reduction: int, *, stats, loss=None, g=None,
               dq=None, dpos=None, dneg=None, pos_id=None, neg_id=None, pos_bias=None,
               neg_bias=None, splits: int = 0, workspace: Optional[torch.Tensor] = None,
               dim: Optional[int] = None):
    """One ``mrec_shneg_loss_fwd`` / ``mrec_shneg_loss_bwd`` call, arguments as given
    (nothing is checked or repaired here: a bad argument comes back from the library as
    ``ValueError`` and launches nothing).  Every operand may be a window of a larger
    allocation, addressed through its row stride."""
    a = _mrec.ShnegArgs()
    a.q, a.q_dtype, a.ldq = q.data_ptr(), _mrec.dtype_code(q.dtype), _ld(q)
    a.pos, a.ld_pos = pos.data_ptr(), _ld(pos)
    a.neg, a.ld_neg = neg.data_ptr(), _ld(neg)
    a.row_dtype = _mrec.dtype_code(pos.dtype)
    a.batch, a.n_neg = int(q.shape[0]), int(neg.shape[0])
    a.D = int(q.shape[1]) if dim is None else int(dim)
    a.pos_id, a.neg_id = _mrec.ptr(pos_id), _mrec.ptr(neg_id)
    ids = pos_id if pos_id is not None else neg_id
    a.id_dtype = _mrec.dtype_code(ids.dtype) if ids is not None else _mrec.I32
    a.pos_bias, a.neg_bias = _mrec.ptr(pos_bias), _mrec.ptr(neg_bias)
    a.kind, a.reduction = int(kind), int(reduction)
    a.loss, a.stats, a.g = _mrec.ptr(loss), _mrec.ptr(stats), _mrec.ptr(g)
    for name, t in (("dq", dq), ("dpos", dpos), ("dneg", dneg)):
        if t is not None:
            setattr(a, name, t.data_ptr())
            setattr(a, "ld_" + name, _ld(t))
    a.splits = int(splits)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), int(workspace.numel())
    try:
        _mrec.call(fn, ctypes.byref(a), _mrec.stream_handle(q.device))
    except _mrec.MrecError as e:
        if e.status == _mrec.EINVAL:
            raise ValueError(str(e)) from e
        raise


def _shneg_rows(t: torch.Tensor) -> torch.Tensor:
    """``t [n, D]`` as the ABI can address it: unit column stride, 16-byte aligned rows.  A
    window that already is stays where it is."""
    eb = t.element_size()
    if (t.stride(1) == 1 and t.data_ptr() % 16 == 0
            and (t.shape[0] <= 1 or (t.stride(0) >= t.shape[1] and t.stride(0) * eb % 16 == 0))):
        return t
    return t.contiguous()


class _ShnegFn(torch.autograd.Function):
    """The fused forward and backward (csrc/shneg.hip).  Saves the operands and 4 floats per
    query; the backward recomputes the scores."""

    @staticmethod
    def forward(ctx, q, pos, neg, pos_id, neg_id, pos_bias, neg_bias, kind, reduction, splits):
        dev = q.device
        B, D = q.shape
        S = neg.shape[0]
        alias = neg is pos
        q, pos = _shneg_rows(q), _shneg_rows(pos)
        neg = pos if alias else _shneg_rows(neg)
        if pos_id is not None:
            pos_id = pos_id.contiguous()
            neg_id = pos_id if alias and neg_id is pos_id else neg_id.to(pos_id.dtype).contiguous()
        pos_bias = pos_bias.detach().float().contiguous() if pos_bias is not None else None
        neg_bias = neg_bias.detach().float().contiguous() if neg_bias is not None else None
        none = reduction == _mrec.REDUCE_NONE
        stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
        out = (torch.empty if B else torch.zeros)(B if none else 1, dtype=torch.float32, device=dev)
        if B:  # (an empty batch launches nothing: the loss is empty, or 0)
            ws = None if none else torch.empty(4 * B + 16, dtype=torch.uint8, device=dev)
            shneg_call("mrec_shneg_loss_fwd", q, pos, neg, kind, reduction, stats=stats, loss=out,
                       pos_id=pos_id, neg_id=neg_id, pos_bias=pos_bias, neg_bias=neg_bias,
                       splits=splits, workspace=ws)
        ctx.save_for_backward(q, pos, neg, pos_id, neg_id, pos_bias, neg_bias, stats)
        ctx.shneg = (kind, reduction, splits)
        return out if none else out.reshape(())

    @staticmethod
    def backward(ctx, g):
        q, pos, neg, pos_id, neg_id, pos_bias, neg_bias, stats = ctx.saved_tensors
        kind, reduction, splits = ctx.shneg
        lib = _mrec.lib()
        dev = q.device
        B, D = q.shape
        S = neg.shape[0]
        g = g.contiguous().float().reshape(-1)
        if reduction == _mrec.REDUCE_NONE and g.numel() != B:
            g = g.expand(B).contiguous()
        make = torch.empty if B else torch.zeros  # (no query: no launch, dneg is zero)
        dq = torch.empty(B, D, dtype=q.dtype, device=dev)
        dpos = torch.empty(B, D, dtype=pos.dtype, device=dev)
        dneg = make(S, D, dtype=neg.dtype, device=dev)
        if B:
            n = splits or shneg_default_splits(B, S)
            ws = None
            if n > 1 and S > 0:
                ws = torch.empty(int(lib.mrec_shneg_workspace_size(B, S, D, n)) + 16,
                                 dtype=torch.uint8, device=dev)
            shneg_call("mrec_shneg_loss_bwd", q, pos, neg, kind, reduction, stats=stats, g=g,
                       dq=dq, dpos=dpos, dneg=dneg, pos_id=pos_id, neg_id=neg_id,
                       pos_bias=pos_bias, neg_bias=neg_bias, splits=splits, workspace=ws)
        return dq, dpos, dneg, None, None, None, None, None, None, None


class SharedNegativeLoss(_Loss):
    """List-wise loss over a pool of negatives shared by the batch: ``kind`` is ``softmax``
    (sampled softmax), ``bpr`` or ``top1`` (the pairwise loss of every (positive, negative)
    pair, averaged over the pool).

    ``forward(q [B, D], pos [B, D], neg [S, D], pos_id=None, neg_id=None, pos_bias=None,
    neg_bias=None)``: ``pos`` / ``neg`` are the gathered item rows (``neg`` may be ``pos``
    itself: in-batch negatives); candidate j is masked for query b iff ``neg_id[j] ==
    pos_id[b]``; the biases are fp32 constants added to the scores (the log-Q correction)
    and get no gradient.  ``[B]`` for ``reduction="none"``, else a scalar.  ``fused = False``
    (class or instance) forces the torch-ops path on a GPU too; ``splits`` is the number of
    parts the batch is cut into for the pool's gradient (0: chosen from the shape; the result
    never depends on it)."""
    fused = True

    def __init__(self, kind: str, reduction: str = "mean", splits: int = 0):
        if kind not in _SHNEG_KINDS:
            raise ValueError(f"kind参数不合法: {kind}")
        if reduction not in _REDUCTIONS:
            raise ValueError(f"reduction参数不合法: {reduction}")
        if not 0 <= int(splits) <= 64:
            raise ValueError(f"splits must be in 0 .. 64, got {splits}")
        super().__init__(None, None, reduction)
        self.kind = kind
        self.splits = int(splits)

    def uses_fused(self, q, pos, neg) -> bool:
        return (self.fused and q.is_cuda and pos.is_cuda and neg.is_cuda
                and pos.dtype == neg.dtype and shneg_supported(q.shape[1], q.dtype, pos.dtype))

    def forward(self, q, pos, neg, pos_id=None, neg_id=None, pos_bias=None, neg_bias=None):  # noqa
        if q.dim() != 2 or pos.shape != q.shape or neg.dim() != 2 or neg.shape[1] != q.shape[1]:
            raise ValueError(f"need q [B, D], pos [B, D], neg [S, D]; got {tuple(q.shape)}, "
                             f"{tuple(pos.shape)}, {tuple(neg.shape)}")
        if (pos_id is None) != (neg_id is None):
            raise ValueError("pos_id and neg_id go together")
        if pos_id is not None and (pos_id.shape != (q.shape[0],) or neg_id.shape != (neg.shape[0],)):
            raise ValueError("need pos_id [B] and neg_id [S]")
        if self.uses_fused(q, pos, neg):
            return _ShnegFn.apply(q, pos, neg, pos_id, neg_id, pos_bias, neg_bias,
                                  _SHNEG_KINDS[self.kind], _REDUCTIONS[self.reduction], self.splits)
        return cpu_path.shared_negative_loss(q, pos, neg, self.kind, self.reduction, pos_id, neg_id,
                                             pos_bias, neg_bias, round_bf16=q.is_cuda)


class SoftmaxSharedLoss(SharedNegativeLoss):
    def __init__(self, reduction: str = "mean"):
        super().__init__("softmax", reduction)


class BPRSharedLoss(SharedNegativeLoss):
    def __init__(self, reduction: str = "mean"):
        super().__init__("bpr", reduction)


class Top1SharedLoss(SharedNegativeLoss):
    def __init__(self, reduction: str = "mean"):
        super().__init__("top1", reduction)


_loss_classes: Dict[str, Type[_Loss]] = {
    "bpr": BPRLoss,
    "top1": Top1Loss,
    "bce": BCEWithLogitsLoss,
    "mse": MSELoss,
    "softmax_shared": SoftmaxSharedLoss,
    "bpr_shared": BPRSharedLoss,
    "top1_shared": Top1SharedLoss,
}

loss_name_list = _loss_classes.keys()


def get_loss(loss_name: str) -> Type[_Loss]:
    """Mirror of torchrec/loss/losses.py:get_loss."""
    if (not isinstance(loss_name, str)) or (loss_name not in _loss_classes):
        raise ValueError(f"loss_name参数不合法: {loss_name}")
    return _loss_classes[loss_name]
