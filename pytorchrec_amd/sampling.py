"""Negative sampling for pair-wise training — the device counterpart of
``SimpleDataReader.train_neg_sample`` (torchrec/data/SimpleDataReader.py:280-300: one
``rng.integers(low, high)`` per training row, redrawn while the user has interacted
with it).

``NegativeSampler`` keeps the training positives as a per-user CSR (``offsets`` int64
``[n_users + 1]``, ``items`` int32, each user's items sorted and de-duplicated) on its
device.  ``sample(uids, n_neg, step)`` draws ``int32 [B, n_neg]`` items of
``[low, high)``: output ``(b, j)`` is a counter hash of ``(seed, step, b * n_neg + j,
attempt)`` (splitmix64 finalisers, written down in include/mrec.h) mapped to the range
by multiply-shift and rejected, by binary search, while the user's list contains it —
``_mrec.NEG_MAX_ATTEMPTS`` (32) attempts at the most; then the last draw is kept and
counted in ``unresolved()``.  A uid outside ``[0, n_users)`` has an empty list.  The
result depends on ``(seed, step, B, n_neg, ids)`` only: on a GPU it is one
``mrec_neg_sample`` launch, on the CPU ``cpu_path.neg_sample`` restates the hash in
numpy, and the two give the same bits.  numpy's own random stream is not reproduced.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from pytorchrec_amd import _mrec, cpu_path


class NegativeSampler:
    def __init__(self, uids, iids, low: int, high: int, seed: int = 0,
                 n_users: Optional[int] = None, device=None):
        u = np.asarray(uids.cpu() if torch.is_tensor(uids) else uids).astype(np.int64).reshape(-1)
        i = np.asarray(iids.cpu() if torch.is_tensor(iids) else iids).astype(np.int64).reshape(-1)
        if u.shape != i.shape:
            raise ValueError("uids and iids must pair up: one item per training row")
        low, high = int(low), int(high)
        if not (-(1 << 31) <= low < high <= (1 << 31) - 1):
            raise ValueError(f"need int32 low < high, got [{low}, {high})")
        if n_users is None:
            n_users = int(u.max()) + 1 if u.size else 0
        n_users = int(n_users)
        if u.size and (int(u.min()) < 0 or int(u.max()) >= n_users):
            raise ValueError(f"training uids must lie in [0, n_users = {n_users})")
        if i.size and (int(i.min()) < -(1 << 31) or int(i.max()) >= (1 << 31)):
            raise ValueError("item ids must fit int32")
        pairs = np.unique(np.stack([u, i], axis=1), axis=0) if u.size else np.zeros((0, 2), np.int64)
        offsets = np.zeros(n_users + 1, np.int64)
        np.cumsum(np.bincount(pairs[:, 0], minlength=n_users), out=offsets[1:])
        self.low, self.high, self.seed, self.n_users = low, high, int(seed), n_users
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.offsets = torch.from_numpy(offsets).to(self.device)
        # (at least one element: the library takes no NULL pointer)
        items = pairs[:, 1].astype(np.int32) if pairs.size else np.zeros(1, np.int32)
        self.items = torch.from_numpy(items).to(self.device)
        self.n_items = int(pairs.shape[0])
        self._unresolved = torch.zeros(1, dtype=torch.int32, device=self.device)
        # the CPU path's membership keys: uid << 32 | the item's 32 bits, sorted
        self._keys = (np.sort((pairs[:, 0] << 32) | (pairs[:, 1] & 0xFFFFFFFF))
                      if self.device.type == "cpu" else None)

    def sample(self, uids: torch.Tensor, n_neg: int = 1, step: int = 0) -> torch.Tensor:
        n_neg, step = int(n_neg), int(step)
        if n_neg < 1:
            raise ValueError(f"n_neg must be >= 1, got {n_neg}")
        if uids.dim() != 1 or uids.dtype not in (torch.int32, torch.int64):
            raise ValueError("uids must be a 1-D int32 or int64 tensor")
        if self.device.type != "cuda":
            out, left = cpu_path.neg_sample(uids.cpu().numpy(), n_neg, self._keys, self.n_users,
                                            self.low, self.high, self.seed, step,
                                            _mrec.NEG_MAX_ATTEMPTS)
            self._unresolved += left
            return torch.from_numpy(out)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("negative sampling inside a HIP-graph capture is not supported: "
                               "draw the negatives before the captured region")
        u = uids.to(self.device).contiguous()
        B = u.shape[0]
        out = torch.empty(B, n_neg, dtype=torch.int32, device=self.device)
        mask = (1 << 64) - 1
        _mrec.call("mrec_neg_sample", u.data_ptr(), _mrec.dtype_code(u.dtype), B, n_neg,
                   self.offsets.data_ptr(), self.items.data_ptr(), self.n_users, self.low,
                   self.high, self.seed & mask, step & mask, out.data_ptr(),
                   self._unresolved.data_ptr(), _mrec.stream_handle(self.device))
        return out

    def unresolved(self) -> int:
        """Outputs, since construction, whose every attempt hit the user's own items
        (the last draw was kept).  Reads the device counter: one sync."""
        return int(self._unresolved.item())
