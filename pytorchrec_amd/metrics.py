"""Metrics: the reference's leave-one-out ranking metrics (NDCG@k, Hit@k;
torchrec/metric/{IMetric,NDCG,Hit}.py, metrics.py:6-17) and the CTR metrics it lacks
(AUC, log-loss).  Each metric is a callable
``m(prediction, target) -> float`` with a ``name`` (what ``IModel.evaluate``
records), computed on the host in float64.

The rank rule (a contract: the numpy form here, ``mrec_rank_pos`` on the device
and every test use it)

  * A 2-D prediction ``[U, N]`` is ranked per row, for any ``N >= 1``.  A 1-D
    prediction is reshaped to ``(-1, user_sample_n)`` as the reference does
    (IMetric.py:19); a size that does not divide raises ``ValueError``.  Column 0
    of a row is the positive, the others are its sampled negatives.
  * ``rank = 1 + #{j >= 1 : p[j] > p[0]}``.  Ties therefore resolve in the
    positive's favour, which is what a stable descending sort gives.  The
    reference's ``(-p).argsort()`` is unstable: for tied rows its answer is
    arbitrary, anywhere between this rule and the pessimistic one (and rank 1 for
    an all-equal row).  Consequence: constant predictions score perfectly, so a
    collapsed model shows as a *perfect* metric, not a poor one.
  * A NaN in column 0 gives rank ``N``; a NaN in any other column never counts.

On a tie-free, NaN-free input the rule reproduces the reference's ranks exactly
(golden G14)."""
from __future__ import annotations

import numpy as np


class AUC:
    name = "auc"

    def __call__(self, prediction, target) -> float:
        p = np.asarray(prediction, np.float64).reshape(-1)
        y = np.asarray(target, np.float64).reshape(-1) > 0.5
        n_pos, n_neg = int(y.sum()), int((~y).sum())
        if n_pos == 0 or n_neg == 0:
            return float("nan")
        order = np.argsort(p, kind="mergesort")
        ranks = np.empty(len(p), np.float64)
        sp = p[order]
        i = 0
        while i < len(sp):  # average ranks over ties
            j = i
            while j + 1 < len(sp) and sp[j + 1] == sp[i]:
                j += 1
            ranks[order[i:j + 1]] = (i + j) / 2.0 + 1.0
            i = j + 1
        return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


class LogLoss:
    name = "logloss"

    def __call__(self, prediction, target) -> float:
        z = np.asarray(prediction, np.float64).reshape(-1)
        y = np.asarray(target, np.float64).reshape(-1)
        if z.size == 0:
            return float("nan")
        return float(np.mean(np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))))


def pos_rank(prediction, user_sample_n: int) -> np.ndarray:
    """The positive's rank per user by the module's rank rule -> int64 ``[U]``."""
    p = np.asarray(prediction)
    if p.ndim != 2:
        if user_sample_n < 1 or p.size % user_sample_n:
            raise ValueError(f"{p.size} predictions do not divide into users of "
                             f"{user_sample_n} candidates")
        p = p.reshape((-1, user_sample_n))
    n = p.shape[1]
    if n < 1:
        raise ValueError("a prediction row needs at least the positive's column")
    ranks = 1 + (p[:, 1:] > p[:, :1]).sum(axis=1).astype(np.int64)
    ranks[np.isnan(p[:, 0])] = n
    return ranks


def rank_pos_device(prediction):
    """``pos_rank`` of a 2-D GPU tensor ``[U, N]`` through ``mrec_rank_pos`` -> int32
    ``[U]`` on the same device (rows read in place through their stride; no copy to
    the host)."""
    import torch
    from pytorchrec_amd import _mrec
    if prediction.dim() != 2 or not prediction.is_cuda or prediction.shape[1] < 1:
        raise ValueError("rank_pos_device needs a [U, N >= 1] GPU tensor")
    p = prediction.detach().float()
    U, N = p.shape
    if p.stride(1) != 1 or (U > 1 and p.stride(0) < N):
        p = p.contiguous()
    out = torch.empty(U, dtype=torch.int32, device=p.device)
    _mrec.call("mrec_rank_pos", p.data_ptr(), U, N, max(int(p.stride(0)), N), out.data_ptr(),
               _mrec.stream_handle(p.device))
    return out


def topk_pos_rank(ids, pos):
    """The 1-based place of ``pos[b]`` in the retrieved list ``ids[b]`` (``[B, K]``), or
    ``K + 1`` when it is absent: the positive's rank among ALL items wherever it is at most
    K, so ``NDCG(., k).fast_calc`` / ``Hit(., k).fast_calc`` of it are the full-catalogue
    NDCG@k / Hit@k for k <= K.  Torch tensors give an int64 tensor on their device, anything
    else an int64 numpy array."""
    import torch
    as_numpy = not torch.is_tensor(ids)
    t = torch.as_tensor(np.asarray(ids)) if as_numpy else ids
    p = torch.as_tensor(np.asarray(pos)) if not torch.is_tensor(pos) else pos
    if t.dim() != 2 or p.reshape(-1).shape[0] != t.shape[0]:
        raise ValueError("topk_pos_rank needs ids [B, K] and pos [B]")
    K = t.shape[1]
    hit = t.to(torch.int64) == p.reshape(-1, 1).to(device=t.device, dtype=torch.int64)
    place = torch.arange(1, K + 1, device=t.device).unsqueeze(0).expand_as(hit)
    rank = torch.where(hit, place, torch.full_like(place, K + 1)).amin(dim=1) if K else \
        torch.ones(t.shape[0], dtype=torch.int64, device=t.device)
    return rank.numpy() if as_numpy else rank


class RankingMetric:
    """Base of the leave-one-out metrics (torchrec/metric/IMetric.py): a metric of the
    positives' ranks alone, so ``IModel.evaluate`` may feed it ranks computed on the
    device (``fast_calc``) instead of the predictions."""

    def __init__(self, user_sample_n: int):
        self.name = "IMetric"
        self.user_sample_n = user_sample_n

    def get_pos_rank(self, prediction) -> np.ndarray:
        return pos_rank(prediction, self.user_sample_n)

    def __call__(self, prediction, target=None, *args, **kwargs):
        return self.fast_calc(self.get_pos_rank(prediction))

    def fast_calc(self, pos_ranks: np.ndarray):
        raise NotImplementedError


class NDCG(RankingMetric):
    def __init__(self, user_sample_n: int, k: int):
        self.k = k
        super().__init__(user_sample_n)
        self.name = f"ndcg@{self.k}"

    def fast_calc(self, pos_ranks: np.ndarray):
        hit_pos_ranks = pos_ranks[pos_ranks <= self.k]
        return np.sum(1 / np.log2(hit_pos_ranks + 1)) / len(pos_ranks)


class Hit(RankingMetric):
    def __init__(self, user_sample_n: int, k: int):
        self.k = k
        super().__init__(user_sample_n)
        self.name = f"hit@{self.k}"

    def fast_calc(self, pos_ranks: np.ndarray):
        hit_pos_ranks = pos_ranks[pos_ranks <= self.k]
        return len(hit_pos_ranks) / len(pos_ranks)


_metric_classes = {"auc": AUC, "logloss": LogLoss}
_ranking_classes = {"ndcg": NDCG, "hit": Hit}


def get_metric(name: str):
    """``auc`` / ``logloss``, or the reference's ``"<ndcg|hit>@<k>"`` with k >= 1 and
    99 sampled candidates per user (torchrec/metric/metrics.py:6-17)."""
    if not isinstance(name, str):
        raise ValueError(f"metric_name参数不合法: {name}")
    n = name.strip().lower()
    if n in _metric_classes:
        return _metric_classes[n]()
    cls_name, sep, k = n.partition("@")
    if sep and cls_name in _ranking_classes and k.isdigit() and int(k) >= 1:
        return _ranking_classes[cls_name](99, int(k))
    raise ValueError(f"unknown metric {name!r}; choose from {sorted(_metric_classes)} or "
                     f"'<ndcg|hit>@<k>' with k >= 1")
