"""Full-catalogue top-K retrieval: which k items of a table score highest per query.

    score[b, i] = bf16(q[b]) . bf16(T[i]) (+ w[i])          i in [low, high)
    topk(...)   = the k best eligible items per query, by score descending, then id
                  ascending -> (ids int32 [B, k], scores float32 [B, k])

The ``[B, items]`` score matrix never exists.  On a GPU, for the compiled shapes
(``mrec_topk_supported``: dim in {8, 16, 32, 64}, k <= 128) it is ``mrec_topk``
(csrc/topk.hip): a skinny MFMA GEMM whose accumulators feed a threshold-and-buffer
selection in LDS.  Everywhere else -- a CPU bank, another dim or k, a row-sharded bank --
it is ``cpu_path.topk``, the same contract in torch ops, chunked over the items (with
the kernel's bf16 operands on a GPU; on a CPU the operands stay fp32, which is what the
models' CPU forward computes).  The
contract (eligibility, exclusion, padding with id -1 / score -inf, determinism) is
written down once, in include/mrec.h above ``mrec_topk``.

``ncf_topk`` is the same for NCF, whose score is an MLP over the (user, item) pair and
not a dot product with an item row: ``mrec_ncf_topk`` (csrc/ncf_topk.hip) runs the NeuMF
scorer on (user, item) pairs formed on chip and feeds the same selection; its contract
stands above ``mrec_ncf_topk`` in include/mrec.h, and ``cpu_path.ncf_topk`` restates it.

``Exclusion`` is a per-query set of items that must not be returned (a user's training
positives, a session's own history): a CSR of sorted, de-duplicated table-local ids,
the layout ``sampling.NegativeSampler`` keeps.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from pytorchrec_amd import _mrec, cpu_path


class Exclusion:
    """``items[offsets[r] : offsets[r + 1]]`` (int32, ascending, distinct, table-local)
    are excluded for CSR row r; query b uses row ``rows[b]``, or row b when ``rows`` is
    None.  A row index outside the CSR excludes nothing."""

    def __init__(self, offsets: torch.Tensor, items: torch.Tensor, rows: Optional[torch.Tensor] = None):
        if offsets.dim() != 1 or offsets.numel() < 1 or items.dim() != 1:
            raise ValueError("Exclusion needs 1-D offsets [n_rows + 1] and items")
        if rows is not None and (rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64)):
            raise ValueError("Exclusion rows must be a 1-D int32 or int64 tensor")
        self.offsets = offsets.to(torch.int64).contiguous()
        self.items = items.to(torch.int32).contiguous()
        self.rows = rows.contiguous() if rows is not None else None

    @property
    def n_rows(self) -> int:
        return self.offsets.numel() - 1

    def to(self, device) -> "Exclusion":
        return Exclusion(self.offsets.to(device), self.items.to(device),
                         self.rows.to(device) if self.rows is not None else None)

    @classmethod
    def from_sampler(cls, sampler, uids: torch.Tensor) -> "Exclusion":
        """The training positives a ``NegativeSampler`` holds, addressed by ``uids``: its
        CSR is used in place; its items are re-based by ``sampler.low`` when the table's
        id 0 is not the sampler's id 0."""
        items = sampler.items if sampler.low == 0 else sampler.items - sampler.low
        return cls(sampler.offsets, items, uids.to(sampler.offsets.device))

    @classmethod
    def from_lists(cls, lists: torch.Tensor, pad=None) -> "Exclusion":
        """One row of ``lists [B, L]`` per query (a session's own history): sorted and
        de-duplicated on its device; ``pad`` and negative ids are dropped."""
        if lists.dim() != 2:
            raise ValueError(f"lists must be [B, L], got {tuple(lists.shape)}")
        x = lists.to(torch.int64)
        big = torch.iinfo(torch.int64).max
        drop = x < 0
        if pad is not None:
            drop = drop | (x == int(pad))
        x, _ = torch.sort(torch.where(drop, torch.full_like(x, big), x), dim=1)
        keep = x != big
        if x.shape[1] > 1:
            keep[:, 1:] &= x[:, 1:] != x[:, :-1]
        offsets = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=x.device)
        torch.cumsum(keep.sum(1), 0, out=offsets[1:])
        items = x[keep].to(torch.int32)
        if items.numel() == 0:  # (at least one element: the library takes no NULL pointer)
            items = torch.zeros(1, dtype=torch.int32, device=x.device)
        return cls(offsets, items)


def tile_queries() -> int:
    return int(_mrec.lib().mrec_topk_tile_queries())


def tile_items() -> int:
    return int(_mrec.lib().mrec_topk_tile_items())


def default_splits(batch: int, n_items: int) -> int:
    return int(_mrec.lib().mrec_topk_splits(int(batch), int(n_items)))


def supported(dim: int, k: int, dtype: torch.dtype) -> bool:
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(_mrec.lib().mrec_topk_supported(int(dim), int(k), _mrec.dtype_code(dtype)))


def topk_fused(bank, table: int, q: torch.Tensor, k: int, low: int, high: int, use_w: bool = False,
               exclude: Optional[Exclusion] = None, splits: int = 0, out_ids=None, out_scores=None,
               workspace: Optional[torch.Tensor] = None):
    """One ``mrec_topk`` call, arguments as given (nothing is checked or repaired here: a
    bad argument comes back from the library as ``ValueError`` and launches nothing).
    ``out_ids`` / ``out_scores`` may be ``[>= B, >= k]`` windows with one common row stride;
    ``workspace`` a uint8 tensor (default: sized by ``mrec_topk_workspace_size``)."""
    lib = _mrec.lib()
    dev = q.device
    B = int(q.shape[0])
    if out_ids is None:
        out_ids = torch.empty(B, max(int(k), 0), dtype=torch.int32, device=dev)
    if out_scores is None:
        out_scores = torch.empty(B, max(int(k), 0), dtype=torch.float32, device=dev)
    if out_ids.stride(0) != out_scores.stride(0) and B > 1:
        raise ValueError("out_ids and out_scores need one common row stride")
    ld_out = max(int(out_ids.stride(0)), int(k))
    if workspace is None:
        n = int(splits) if splits else default_splits(B, int(high) - int(low))
        nbytes = int(lib.mrec_topk_workspace_size(B, int(k), n)) if 0 < n <= 64 else 0
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    args = _mrec.TopkArgs()
    desc = bank.desc()
    desc.ref()  # (refreshes the data pointer)
    args.bank = ctypes.pointer(desc.struct)
    args.table, args.low, args.high = int(table), int(low), int(high)
    args.q, args.q_dtype = q.data_ptr(), _mrec.dtype_code(q.dtype)
    args.ldq = int(q.stride(0)) if B > 1 else max(int(q.stride(0)), int(q.shape[1]))
    args.batch, args.k, args.use_w = B, int(k), int(bool(use_w))
    if exclude is not None:
        args.excl_offsets, args.excl_items = exclude.offsets.data_ptr(), exclude.items.data_ptr()
        args.excl_n_rows = exclude.n_rows
        if exclude.rows is not None:
            args.excl_row, args.excl_row_dtype = exclude.rows.data_ptr(), _mrec.dtype_code(exclude.rows.dtype)
    args.splits = int(splits)
    args.workspace, args.workspace_bytes = workspace.data_ptr(), int(workspace.numel())
    args.out_ids, args.out_scores, args.ld_out = out_ids.data_ptr(), out_scores.data_ptr(), ld_out
    try:
        _mrec.call("mrec_topk", ctypes.byref(args), _mrec.stream_handle(dev))
    except _mrec.MrecError as e:
        if e.status == _mrec.EINVAL:
            raise ValueError(str(e)) from e
        raise
    return out_ids, out_scores


@torch.no_grad()
def topk(bank, table: int, q: torch.Tensor, k: int, *, low: int = 0, high: Optional[int] = None,
         use_w: bool = False, exclude: Optional[Exclusion] = None, item_splits: Optional[int] = None):
    """The k best items of table ``table`` of ``bank`` in ``[low, high)`` for each row of
    ``q [B, dim]`` -> ``(ids int32 [B, k], scores float32 [B, k])``, sorted by score
    descending, then id ascending; slots past the eligible items hold (-1, -inf).
    ``use_w`` adds the bank's first-order column to the score.  ``item_splits`` is the
    number of parts the item range is scanned in on a GPU (default: chosen from the
    shape); the result never depends on it."""
    from pytorchrec_amd.sharding import ShardedEmbeddingBank
    table, k = int(table), int(k)
    if not 0 <= table < bank.n_tables:
        raise ValueError(f"table {table} out of range: the bank has {bank.n_tables}")
    sharded = isinstance(bank, ShardedEmbeddingBank)
    n_rows = int(bank.global_rows[table]) if sharded else bank.category_nums[table]
    low = int(low)
    high = n_rows if high is None else int(high)
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if not 0 <= low <= high <= n_rows:
        raise ValueError(f"need 0 <= low <= high <= {n_rows}, got [{low}, {high})")
    if q.dim() != 2 or q.shape[1] != bank.dim:
        raise ValueError(f"q must be [B, {bank.dim}], got {tuple(q.shape)}")
    if use_w and not bank.has_w:
        raise ValueError("use_w needs a bank with a first-order column")
    if item_splits is not None and not 1 <= int(item_splits) <= 64:
        raise ValueError(f"item_splits must be in 1 .. 64, got {item_splits}")
    q = q.detach()
    if exclude is not None and exclude.offsets.device != q.device:
        exclude = exclude.to(q.device)
    fused = (q.is_cuda and not sharded and bank.weight.is_cuda
             and q.dtype in (torch.float32, torch.bfloat16)
             and supported(bank.dim, k, bank.weight.dtype))
    if fused:
        if q.stride(1) != 1:
            q = q.contiguous()
        bank.flush_optimizer()  # the kernel reads the rows as stored
        return topk_fused(bank, table, q, k, low, high, use_w, exclude, int(item_splits or 0))
    if sharded:
        full = bank.gather_global()
        o = sum(int(n) for n in bank.global_rows[:table])
        rows = full[o:o + n_rows]
    else:
        o = bank.row_offset[table]
        rows = bank.weight.detach()[o:o + n_rows]
    ex = (exclude.offsets, exclude.items, exclude.rows) if exclude is not None else None
    # a GPU query keeps the kernel's bf16 operands; a CPU bank is scored as the models' CPU
    # forward scores it, in fp32
    return cpu_path.topk(rows, bank.dim, q.float(), k, low, high, use_w, ex, round_bf16=q.is_cuda)


# ---------------------------------------------------------------------------
# NCF: the NeuMF scorer over every (user, item) pair, fused with the selection
# ---------------------------------------------------------------------------

# the fused kernel is the default for the compiled shapes on a GPU; False sends
# ``NCF.recommend`` through ``recommend_by_forward`` (the parity tests and the benchmark)
NCF_TOPK_FUSED = True

# the bank's tables in NCF's order
NCF_TABLES = (0, 1, 2, 3)  # mf_u, mf_i, mlp_u, mlp_i


def ncf_tile_users() -> int:
    return int(_mrec.lib().mrec_ncf_topk_tile_users())


def ncf_tile_items() -> int:
    return int(_mrec.lib().mrec_ncf_topk_tile_items())


def ncf_default_splits(batch: int, n_items: int) -> int:
    return int(_mrec.lib().mrec_ncf_topk_splits(int(batch), int(n_items)))


def ncf_supported(E: int, widths, k: int, dtype: torch.dtype) -> bool:
    """True when ``mrec_ncf_topk`` covers (emb_size, hidden widths, k, bank dtype).  Decided
    from the shape alone; never an error."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    ws = [int(w) for w in widths]
    if not 1 <= len(ws) <= 3 or not -2 ** 31 <= int(k) < 2 ** 31:
        return False
    arr = (ctypes.c_int32 * 3)(*ws)
    return bool(_mrec.lib().mrec_ncf_topk_supported(int(E), len(ws), arr, int(k), _mrec.dtype_code(dtype)))


def _ncf_params(model_or_params):
    """-> (bank, weights, biases, wp): from an NCF model, or the tuple itself."""
    if isinstance(model_or_params, (tuple, list)):
        bank, ws, bs, wp = model_or_params
        return bank, list(ws), list(bs), wp
    from pytorchrec_amd.dense import _ncf_params as dense_params
    ws, bs, wp = dense_params(model_or_params)
    return model_or_params.embeddings, ws, bs, wp


def ncf_topk_fused(bank, uid: torch.Tensor, weights, biases, wp, k: int, low: int, high: int,
                   exclude: Optional[Exclusion] = None, splits: int = 0, out_ids=None, out_scores=None,
                   workspace: Optional[torch.Tensor] = None, oob_flag: Optional[torch.Tensor] = None,
                   tables=NCF_TABLES):
    """One ``mrec_ncf_topk`` call, arguments as given (nothing is checked or repaired here:
    a bad argument comes back from the library as ``ValueError`` and launches nothing).
    ``weights`` / ``biases`` / ``wp`` are contiguous fp32 tensors on the bank's device;
    ``out_ids`` / ``out_scores`` may be ``[>= B, >= k]`` windows with one common row stride;
    ``workspace`` a uint8 tensor (default: sized by ``mrec_ncf_topk_workspace_size``);
    ``oob_flag`` an int32 word the kernel sets for a uid outside the user tables."""
    lib = _mrec.lib()
    dev = uid.device
    B = int(uid.shape[0])
    if out_ids is None:
        out_ids = torch.empty(B, max(int(k), 0), dtype=torch.int32, device=dev)
    if out_scores is None:
        out_scores = torch.empty(B, max(int(k), 0), dtype=torch.float32, device=dev)
    if out_ids.stride(0) != out_scores.stride(0) and B > 1:
        raise ValueError("out_ids and out_scores need one common row stride")
    ld_out = max(int(out_ids.stride(0)), int(k))
    if workspace is None:
        n = int(splits) if splits else ncf_default_splits(B, int(high) - int(low))
        nbytes = int(lib.mrec_ncf_topk_workspace_size(B, int(k), n)) if 0 < n <= 64 else 0
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    args = _mrec.NcfTopkArgs()
    desc = bank.desc()
    desc.ref()  # (refreshes the data pointer)
    args.bank = ctypes.pointer(desc.struct)
    args.table_mf_u, args.table_mf_i, args.table_mlp_u, args.table_mlp_i = (int(t) for t in tables)
    args.low, args.high = int(low), int(high)
    args.uid, args.uid_dtype, args.batch = uid.data_ptr(), _mrec.dtype_code(uid.dtype), B
    args.n_layers = min(len(weights), 3)
    for l in range(args.n_layers):
        args.widths[l] = int(weights[l].shape[0])
        args.w[l], args.ld_w[l] = weights[l].data_ptr(), int(weights[l].stride(0))
        args.b[l] = biases[l].data_ptr()
    args.wp, args.k, args.splits = wp.data_ptr(), int(k), int(splits)
    if exclude is not None:
        args.excl_offsets, args.excl_items = exclude.offsets.data_ptr(), exclude.items.data_ptr()
        args.excl_n_rows = exclude.n_rows
        if exclude.rows is not None:
            args.excl_row, args.excl_row_dtype = exclude.rows.data_ptr(), _mrec.dtype_code(exclude.rows.dtype)
    args.d_oob_flag = _mrec.ptr(oob_flag)
    args.workspace, args.workspace_bytes = workspace.data_ptr(), int(workspace.numel())
    args.out_ids, args.out_scores, args.ld_out = out_ids.data_ptr(), out_scores.data_ptr(), ld_out
    try:
        _mrec.call("mrec_ncf_topk", ctypes.byref(args), _mrec.stream_handle(dev))
    except _mrec.MrecError as e:
        if e.status == _mrec.EINVAL:
            raise ValueError(str(e)) from e
        raise
    return out_ids, out_scores


@torch.no_grad()
def ncf_topk(model_or_params, uid: torch.Tensor, k: int, *, low: int = 0, high: Optional[int] = None,
             exclude: Optional[Exclusion] = None, item_splits: Optional[int] = None):
    """The k best items of ``[low, high)`` for each user of ``uid [B]`` (int32 or int64)
    under the NeuMF scorer of an NCF model -- or of ``(bank, weights, biases, wp)``, the
    bank holding the tables ``[mf_u, mf_i, mlp_u, mlp_i]`` -- ``(ids int32 [B, k], scores
    float32 [B, k])`` by score descending, then id ascending; slots past the eligible items
    hold (-1, -inf).  The model's dropout is not applied (evaluation).  A uid outside the
    user tables is an ``IndexError`` before anything is scored (``bank.check_ids``, as the
    gather rejects it; with the check off such a user's list is all padding).
    ``item_splits``: as for ``topk``."""
    from pytorchrec_amd.sharding import ShardedEmbeddingBank
    bank, ws, bs, wp = _ncf_params(model_or_params)
    k = int(k)
    sharded = isinstance(bank, ShardedEmbeddingBank)
    rows_of = [int(n) for n in (bank.global_rows if sharded else bank.category_nums)]
    if bank.n_tables != 4 or rows_of[0] != rows_of[2] or rows_of[1] != rows_of[3]:
        raise ValueError("ncf_topk needs a bank of the four tables [mf_u, mf_i, mlp_u, mlp_i]")
    n_users, n_rows = rows_of[0], rows_of[1]
    low = int(low)
    high = n_rows if high is None else int(high)
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if not 0 <= low <= high <= n_rows:
        raise ValueError(f"need 0 <= low <= high <= {n_rows}, got [{low}, {high})")
    if uid.dim() != 1 or uid.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"uid must be a 1-D int32 or int64 tensor, got {tuple(uid.shape)} {uid.dtype}")
    if item_splits is not None and not 1 <= int(item_splits) <= 64:
        raise ValueError(f"item_splits must be in 1 .. 64, got {item_splits}")
    E = bank.dim
    if (not ws or len(ws) != len(bs) or ws[0].shape[1] != 2 * E
            or wp.numel() != E + ws[-1].shape[0]):
        raise ValueError("the dense parameters do not fit the bank's embedding size")
    uid = uid.detach().contiguous()
    B = int(uid.shape[0])
    if B and (bank.check_ids or not uid.is_cuda):
        if bool(((uid < 0) | (uid >= n_users)).any()):
            raise IndexError("index out of range in self")
    if exclude is not None and exclude.offsets.device != uid.device:
        exclude = exclude.to(uid.device)
    fused = (uid.is_cuda and not sharded and bank.weight.is_cuda
             and all(p.is_cuda and p.dtype == torch.float32 for p in (*ws, *bs, wp))
             and ncf_supported(E, [w.shape[0] for w in ws], k, bank.weight.dtype))
    bank.flush_optimizer()  # both paths read the rows as stored
    if fused:
        if B == 0:
            return (torch.empty(0, k, dtype=torch.int32, device=uid.device),
                    torch.empty(0, k, dtype=torch.float32, device=uid.device))
        ws = [w.detach() if w.stride(1) == 1 else w.detach().contiguous() for w in ws]
        bs = [b.detach().contiguous() for b in bs]
        return ncf_topk_fused(bank, uid, ws, bs, wp.detach().contiguous().reshape(-1), k, low, high,
                              exclude, int(item_splits or 0))
    if sharded:
        full = bank.gather_global()
        offs = [sum(rows_of[:t]) for t in range(4)]
    else:
        full, offs = bank.weight.detach(), bank.row_offset
    tables = [full[o:o + n] for o, n in zip(offs, rows_of)]
    ex = (exclude.offsets, exclude.items, exclude.rows) if exclude is not None else None
    # a GPU bank keeps the kernel's rounding points; a CPU bank is scored as the model's CPU
    # forward scores it, in fp32
    return cpu_path.ncf_topk(tables, E, uid, ws, bs, wp, k, low, high, ex, round_bf16=uid.is_cuda)
