"""The user-item interaction graph and its normalised propagation (LightGCN, He et al.,
SIGIR 2020).

``BipartiteGraph.from_interactions`` builds, once, everything a propagation needs: the
symmetric adjacency over ``N = n_users + n_items`` nodes (user ``u`` is node ``u``, item
``i`` node ``n_users + i``) in CSR form with every row's columns ascending, so that the
order of a row's sum belongs to the graph and not to the order the interactions arrived
in; ``dinv = deg^-1/2`` (0 for an isolated node), computed in fp64 on the host and rounded
once; and the work list of ``mrec_graph_prop`` (include/mrec.h): one entry per row of up to
``LONG_ROW`` neighbours, and a row longer than that cut into entries of ``LONG_ROW``
neighbours with a slot each in a partial buffer.  No per-edge value is stored: the weight
of edge (r, c) is ``dinv[r] * dinv[c]``.

``propagate(g, x, n_layers)`` is ``1/(K+1) sum_k A^^k x``.  On a GPU, for an fp32 ``x`` of
8, 16, 32 or 64 live columns and 1 <= K <= 4, it is K launches of ``mrec_graph_prop`` each
way (csrc/graph_prop.hip; the operator is symmetric, so the backward is the same launches
on the gradient and nothing is saved); anything else, and ``PROP_FUSED = False``, runs the
same contract as torch ops (``cpu_path.graph_propagate``).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from pytorchrec_amd import _mrec, cpu_path

LONG_ROW = 256  # MREC_GRAPH_LONG_ROW: rows with more neighbours are cut into segments
PROP_FUSED = True  # False: the contract in torch ops on a GPU too (the parity tests set it)
MAX_FUSED_LAYERS = 4


class BipartiteGraph:
    """CSR adjacency, ``dinv`` and the kernel's work list; immutable once built."""

    def __init__(self, n_users: int, n_items: int, row_ptr, col, dinv, work, work_beg, long_row,
                 long_ptr, n_slots: int, max_deg: int):
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.n_nodes = self.n_users + self.n_items
        self.row_ptr, self.col, self.dinv = row_ptr, col, dinv
        self.work, self.work_beg = work, work_beg
        self.long_row, self.long_ptr = long_row, long_ptr
        self.n_slots, self.max_deg = int(n_slots), int(max_deg)
        self._edge_rows, self._csr = None, {}

    @property
    def n_edges(self) -> int:
        """Distinct interactions (the CSR holds each twice)."""
        return int(self.col.shape[0]) // 2

    @property
    def device(self):
        return self.col.device

    @classmethod
    def from_interactions(cls, u_ids, i_ids, n_users: int, n_items: int, device=None):
        u = torch.as_tensor(u_ids).reshape(-1).to("cpu", torch.int64)
        i = torch.as_tensor(i_ids).reshape(-1).to("cpu", torch.int64)
        n_users, n_items = int(n_users), int(n_items)
        N = n_users + n_items
        if u.shape != i.shape:
            raise ValueError("u_ids and i_ids must have one length")
        if n_users < 0 or n_items < 0 or N >= 2 ** 31:
            raise ValueError(f"need 0 <= n_users + n_items < 2^31, got {n_users} + {n_items}")
        if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n_users
                          or int(i.min()) < 0 or int(i.max()) >= n_items):
            raise IndexError("index out of range in self")
        key = torch.unique(u * max(n_items, 1) + i)  # de-duplicated, sorted by (u, i)
        uu, ii = key // max(n_items, 1), key % max(n_items, 1)
        by_item = torch.sort(ii * max(n_users, 1) + uu).values % max(n_users, 1)
        deg = torch.cat([torch.bincount(uu, minlength=n_users), torch.bincount(ii, minlength=n_items)])
        row_ptr = torch.zeros(N + 1, dtype=torch.int64)
        row_ptr[1:] = torch.cumsum(deg, 0)
        col = torch.cat([ii + n_users, by_item]).to(torch.int32)
        dinv = torch.where(deg > 0, deg.double().rsqrt(), torch.zeros((), dtype=torch.float64)).float()
        # the work list: the segments of the long rows first (slot = position), then every
        # other row in node order (slot -1; an isolated row has len 0)
        long_row = torch.nonzero(deg > LONG_ROW).reshape(-1)
        n_seg = (deg[long_row] + LONG_ROW - 1) // LONG_ROW
        long_ptr = torch.zeros(long_row.numel() + 1, dtype=torch.int64)
        long_ptr[1:] = torch.cumsum(n_seg, 0)
        n_slots = int(long_ptr[-1])
        seg_row = torch.repeat_interleave(long_row, n_seg)
        seg = torch.arange(n_slots) - torch.repeat_interleave(long_ptr[:-1], n_seg)
        seg_len = torch.clamp(deg[seg_row] - seg * LONG_ROW, max=LONG_ROW)
        short = torch.nonzero(deg <= LONG_ROW).reshape(-1)
        w_row = torch.cat([seg_row, short])
        work = torch.zeros(w_row.numel(), 4, dtype=torch.int32)
        work[:, 0] = w_row
        work[:, 1] = torch.cat([seg_len, deg[short]])
        work[:, 2] = torch.cat([torch.arange(n_slots), torch.full_like(short, -1)])
        work_beg = torch.cat([row_ptr[seg_row] + seg * LONG_ROW, row_ptr[short]])
        g = cls(n_users, n_items, row_ptr, col, dinv, work, work_beg, long_row.to(torch.int32),
                long_ptr.to(torch.int32), n_slots, int(deg.max()) if N else 0)
        return g.to(device) if device is not None else g

    def to(self, device) -> "BipartiteGraph":
        device = torch.device(device)
        if device == self.device:
            return self
        mv = (lambda t: t.to(device))
        return BipartiteGraph(self.n_users, self.n_items, mv(self.row_ptr), mv(self.col),
                              mv(self.dinv), mv(self.work), mv(self.work_beg), mv(self.long_row),
                              mv(self.long_ptr), self.n_slots, self.max_deg)

    def edge_rows(self) -> torch.Tensor:
        """The row of every CSR entry, int64 [2E] (the torch-op path's index)."""
        if self._edge_rows is None:
            deg = self.row_ptr[1:] - self.row_ptr[:-1]
            self._edge_rows = torch.repeat_interleave(
                torch.arange(self.n_nodes, device=self.device), deg)
        return self._edge_rows

    def csr_tensor(self, dtype=torch.float32) -> torch.Tensor:
        """A^ as a torch sparse CSR tensor with its values materialised (the torch-op path
        on a GPU); built once per dtype."""
        if dtype not in self._csr:
            rows, col = self.edge_rows(), self.col.long()
            vals = (self.dinv[rows] * self.dinv[col]).to(dtype)
            self._csr[dtype] = torch.sparse_csr_tensor(self.row_ptr, col, vals,
                                                       size=(self.n_nodes, self.n_nodes))
        return self._csr[dtype]


def fused_supported(x: torch.Tensor, dim: int, n_layers: int) -> bool:
    return (PROP_FUSED and x.is_cuda and x.dtype == torch.float32
            and dim in (8, 16, 32, 64) and 1 <= int(n_layers) <= MAX_FUSED_LAYERS
            and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def _propagate_fused(g: BipartiteGraph, x: torch.Tensor, dim: int, K: int, bf16: bool):
    """K launches of mrec_graph_prop on ``x [N, ld]`` -> ``[N, ld]``, pad columns zero."""
    N, ld = x.shape
    out = torch.empty_like(x)
    if N == 0:
        return out
    if int(_mrec.lib().mrec_graph_long_row()) != LONG_ROW:
        raise _mrec.MrecUnavailable("libmrec was built with another MREC_GRAPH_LONG_ROW; rebuild it")
    dev = x.device
    ldt = torch.bfloat16 if bf16 else torch.float32
    layers = [torch.empty(N, dim, dtype=ldt, device=dev) for _ in range(min(K - 1, 2))]
    total = torch.empty(N, dim, dtype=torch.float32, device=dev) if K > 1 else None
    partial = (torch.empty(g.n_slots, dim, dtype=torch.float32, device=dev) if g.n_slots else None)
    a = _mrec.GraphPropArgs(
        n_rows=N, dim=dim, col=g.col.data_ptr(), dinv=g.dinv.data_ptr(),
        n_work=g.work.shape[0], work=g.work.data_ptr(), work_beg=g.work_beg.data_ptr(),
        n_long=g.long_row.shape[0], long_row=_mrec.ptr(g.long_row) if g.n_slots else None,
        long_ptr=_mrec.ptr(g.long_ptr) if g.n_slots else None, partial=_mrec.ptr(partial),
        next_dtype=_mrec.dtype_code(ldt))
    src, stream = x, _mrec.stream_handle(dev)
    for k in range(K):
        last = k == K - 1
        nxt = None if last else layers[k % 2]
        acc_in = x if k == 0 else total
        acc_out = out if last else total
        a.src, a.src_dtype, a.ld_src = src.data_ptr(), _mrec.dtype_code(src.dtype), src.stride(0)
        a.next = _mrec.ptr(nxt)
        a.acc_in, a.ld_acc_in = acc_in.data_ptr(), acc_in.stride(0)
        a.acc_out, a.ld_acc_out = acc_out.data_ptr(), acc_out.stride(0)
        a.divide, a.zero_pad = (float(K + 1), 1) if last else (0.0, 0)
        _mrec.call("mrec_graph_prop", ctypes.byref(a), stream)
        src = nxt
    return out


def _propagate_torch(g: BipartiteGraph, x: torch.Tensor, K: int, layer_dtype):
    """The contract in torch ops: ``cpu_path.graph_propagate`` on the CPU; on a GPU the same
    layers as ``torch.sparse.mm`` with A^ as a CSR tensor (its values the fp32 products
    dinv[r] dinv[c]), which is what a user without the kernel would write."""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
        return cpu_path.graph_propagate(g, x, K, layer_dtype)
    A = g.csr_tensor(x.dtype)
    total = y = x.contiguous()
    for k in range(K):
        src = y.to(torch.bfloat16).to(x.dtype) if layer_dtype == torch.bfloat16 and k else y
        y = torch.sparse.mm(A, src)
        total = total + y
    return total / (K + 1)


def _propagate_any(g: BipartiteGraph, x: torch.Tensor, dim: int, K: int, layer_dtype):
    if x.shape[0] != g.n_nodes:
        raise ValueError(f"x must have {g.n_nodes} rows, got {x.shape[0]}")
    if g.device != x.device:
        raise ValueError(f"the graph is on {g.device}, x on {x.device}: move the graph (graph.to)")
    x = x.contiguous()
    if fused_supported(x, dim, K):
        return _propagate_fused(g, x, dim, K, layer_dtype == torch.bfloat16)
    y = _propagate_torch(g, x[:, :dim], K, layer_dtype)
    if dim == x.shape[1]:
        return y
    return torch.cat([y, y.new_zeros(x.shape[0], x.shape[1] - dim)], dim=1)


class _PropagateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, dim, K, layer_dtype):
        ctx.g, ctx.dim, ctx.K, ctx.layer_dtype = g, dim, K, layer_dtype
        return _propagate_any(g, x.detach(), dim, K, layer_dtype)

    @staticmethod
    def backward(ctx, dy):
        # A^ is symmetric: the gradient goes through the same operator
        dy = dy.contiguous()
        return _propagate_any(ctx.g, dy, ctx.dim, ctx.K, ctx.layer_dtype), None, None, None, None


def propagate(g: BipartiteGraph, x: torch.Tensor, n_layers: int, layer_dtype=None,
              dim: Optional[int] = None) -> torch.Tensor:
    """``1/(K+1) sum_{k<=K} A^^k x`` over the graph ``g`` for ``x [N, ld]`` -> ``[N, ld]``.

    ``dim`` (default ``ld``): the live columns of a bank-like ``x``; the columns past it come
    out zero and get no gradient.  ``layer_dtype`` bfloat16 stores the layers between the
    launches in bf16 (half the gathered bytes; sums stay fp32)."""
    if x.dim() != 2:
        raise ValueError(f"x must be [N, ld], got {tuple(x.shape)}")
    dim = x.shape[1] if dim is None else int(dim)
    K = int(n_layers)
    if K < 0 or not 1 <= dim <= x.shape[1]:
        raise ValueError(f"need n_layers >= 0 and 1 <= dim <= {x.shape[1]}, got {K}, {dim}")
    if layer_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"layer_dtype must be None, float32 or bfloat16, got {layer_dtype}")
    return _PropagateFn.apply(x, g, dim, K, layer_dtype)


__all__ = ["BipartiteGraph", "propagate", "fused_supported", "LONG_ROW", "PROP_FUSED"]
