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
"""
from typing import Dict, Type

import torch
import torch.nn.functional as F  # noqa
from torch.nn.modules.loss import _Loss, MSELoss  # noqa

from pytorchrec_amd import _mrec


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


_loss_classes: Dict[str, Type[_Loss]] = {
    "bpr": BPRLoss,
    "top1": Top1Loss,
    "bce": BCEWithLogitsLoss,
    "mse": MSELoss,
}

loss_name_list = _loss_classes.keys()


def get_loss(loss_name: str) -> Type[_Loss]:
    """Mirror of torchrec/loss/losses.py:get_loss."""
    if (not isinstance(loss_name, str)) or (loss_name not in _loss_classes):
        raise ValueError(f"loss_name参数不合法: {loss_name}")
    return _loss_classes[loss_name]
