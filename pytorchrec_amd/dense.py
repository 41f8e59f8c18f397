"""Dense-tower ops: Linear(+bias)(+ReLU), DCN-v2 cross, DIN attention pooling, the
SASRec / GRU4Rec encoders, the NCF scorer, DLRM's pairwise dot interaction, xDeepFM's
Compressed Interaction Network, AutoInt's interacting (field self-attention) layers.

One seam for the model code.  On a GPU they run on libmrec's MFMA bf16 GEMM
(``mrec_gemm``: fp32 accumulation, bias / ReLU / DCN epilogues fused, the fp32
master weights converted to bf16 by one small prep kernel, the bias gradient
carried as an extra ones column of the weight-gradient GEMM).

ReLU' is applied by the *consumer* of a ReLU output: the backward GEMM (or head
kernel) that produces d(relu output) masks it in its epilogue and stamps the
gradient tensor (``_MASK_TAG`` = (mask data_ptr, version)); the producing layer
skips its own masking only when the stamp on the incoming gradient is intact.
Autograd accumulation of several consumers' gradients bumps the version, so the
producer then masks itself (masking is idempotent) — correct in every graph,
free in the MLP chain.  On a CPU device (config C1) they are the
reference's fp32 torch ops.

Activation tensors are [M, N] views of [M, round8(N)] bf16 buffers so every
row starts 16-byte aligned.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch
import torch.nn.functional as F

from pytorchrec_amd import _mrec

_BF16 = torch.bfloat16


def _r8(n: int) -> int:
    return (n + 7) // 8 * 8


def _alloc(M: int, N: int, dtype, device) -> torch.Tensor:
    return torch.empty(M, _r8(N), dtype=dtype, device=device)[:, :N]


def _op(t: torch.Tensor, layout: int) -> _mrec.Operand:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("GEMM operands must be 2-D with unit inner stride")
    return _mrec.Operand(t.data_ptr(), _mrec.dtype_code(t.dtype), layout, t.stride(0))


def _split_for(M: int, N: int, K: int) -> int:
    """K slices per output tile: more while a small-output long-K GEMM (weight
    gradients) would leave most of the 256 CUs (3 workgroups each) idle."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = 1
    while tiles * s < 384 and K // (s + 1) >= 256 and s < 64:
        s += 1
    return s


def _split_beside(M: int, N: int, K: int, budget: int = 256) -> int:
    """K slices of a weight-gradient GEMM that shares its launch with a dx GEMM
    (448 workgroups at C2): at most ``budget`` workgroups, so the launch fits one
    residency wave (768 slots).  C2 (49 tiles, K 4096): 5 slices 138.3 us/step,
    7 slices 143.4, 4 slices +1.3 %."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = 1
    while tiles * (s + 1) <= budget and K // (s + 1) >= 256 and s < 64:
        s += 1
    return s


_MASK_TAG = "_mrec_relu_masked"
_RELU_OUT = "_mrec_relu_out"


def _stamp(grad: torch.Tensor, mask_src: torch.Tensor) -> torch.Tensor:
    setattr(grad, _MASK_TAG, (mask_src.data_ptr(), grad._version))
    return grad


def _premasked(grad: torch.Tensor, y_ptr: int) -> bool:
    t = getattr(grad, _MASK_TAG, None)
    return t is not None and t[0] == y_ptr and t[1] == grad._version


def _is_relu_out(x: torch.Tensor) -> bool:
    return getattr(x, _RELU_OUT, False) and x.is_cuda


# the tensors of an mrec_epilogue -> the field that takes a matrix's row stride
_EPI_LD = {"bias": None, "ones_out": None, "mul": "ld_mul", "add": "ld_add", "aux": "ld_aux",
           "mask": "ld_mask", "img_row": "ld_img_row", "img_tr": "ld_img_tr"}


def _epilogue(act=0, sgd_lr=None, img_kind=0, **tensors) -> _mrec.Epilogue:
    """mrec_epilogue by field name; ``tensors``: any of _EPI_LD, each may be None."""
    e = _mrec.Epilogue(act=act, update=int(sgd_lr is not None),
                       lr=float(sgd_lr) if sgd_lr is not None else 0.0, img_kind=img_kind)
    for name, t in tensors.items():
        ld = _EPI_LD[name]
        if t is not None:
            setattr(e, name, t.data_ptr())
            if ld:
                setattr(e, ld, t.stride(0))
    return e


def gemm(A, a_layout, B, b_layout, M, N, K, *, ones_out=None, b_cols=None, bias=None, act=0,
         mul=None, add=None, aux=None, mask=None, out=None, out_dtype=_BF16, split_k=None,
         sgd_lr=None, img_row=None, img_tr=None, img_kind=0):
    """C[M, N] = epi(A[M, K] @ B[K, N]) on libmrec (see include/mrec.h mrec_gemm).
    ``ones_out`` (fp32 [M]) receives sum_k A(m, k) through an appended ones column;
    ``mask`` ([M, N] bf16) zeroes outputs where mask <= 0 (ReLU')."""
    dev = A.device
    if out is None:
        out = _alloc(M, N, out_dtype, dev)
    if split_k is None:
        split_k = _split_for(M, N + (ones_out is not None), K)
    ws_bytes = _mrec.lib().mrec_gemm_workspace_size(M, N, K, split_k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    epi = _epilogue(act, sgd_lr, img_kind, bias=bias, mul=mul, add=add, aux=aux, mask=mask,
                    ones_out=ones_out, img_row=img_row, img_tr=img_tr)
    a_op, b_op = _op(A, a_layout), _op(B, b_layout)
    _mrec.call("mrec_gemm", M, N, K, ctypes.byref(a_op), ctypes.byref(b_op),
               N if ones_out is not None else -1, N if b_cols is None else b_cols,
               ctypes.byref(epi), out.data_ptr(), _mrec.dtype_code(out.dtype), out.stride(0),
               split_k, _mrec.ptr(ws), ws_bytes, _mrec.stream_handle())
    return out


class _Call:
    """One GEMM of an mrec_gemm_multi launch (the ctypes structs + every tensor they
    point at, kept alive until the launch that runs it)."""

    def __init__(self, A, a_layout, B, b_layout, M, N, K, phase, *, ones_out=None, b_cols=None,
                 mask=None, out=None, out_dtype=_BF16, split_k=1, sgd_lr=None, img_row=None,
                 img_tr=None, ws=None, add=None, img_kind=0):
        dev = A.device
        if out is None:
            out = _alloc(M, N, out_dtype, dev)
        ws_bytes = _mrec.lib().mrec_gemm_workspace_size(M, N, K, split_k)
        if ws_bytes and ws is None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        self.out, self.ws = out, ws
        self.keep = [A, B, ones_out, mask, img_row, img_tr, out, ws, add]
        self.epi = _epilogue(_mrec.ACT_NONE, sgd_lr, img_kind, add=add, mask=mask,
                             ones_out=ones_out, img_row=img_row, img_tr=img_tr)
        self.a, self.b = _op(A, a_layout), _op(B, b_layout)
        self.args = (M, N, K, N if ones_out is not None else -1, N if b_cols is None else b_cols,
                     out.data_ptr(), _mrec.dtype_code(out.dtype), out.stride(0), split_k,
                     _mrec.ptr(ws), ws_bytes)
        self.phase, self.split_k = phase, split_k
        self.writes = {p for p in (out.data_ptr(), _mrec.ptr(ones_out), _mrec.ptr(img_row),
                                   _mrec.ptr(img_tr)) if p}
        self.reads = {A.data_ptr(), B.data_ptr()} | ({add.data_ptr()} if add is not None else set())

    def with_phase(self, phase):
        c = object.__new__(_Call)
        c.__dict__.update(self.__dict__)
        c.phase = phase
        return c

    def struct(self) -> _mrec.GemmCall:
        M, N, K, ones, bcols, C, cdt, ldc, sk, ws, wsb = self.args
        return _mrec.GemmCall(M, N, K, ctypes.pointer(self.a), ctypes.pointer(self.b), ones, bcols,
                              ctypes.pointer(self.epi), C, cdt, ldc, sk, ws, wsb, self.phase)


# ----------------------------------------------------------------------------
# deferred work: three module-level lists, only ever mutated in place
# ----------------------------------------------------------------------------
# _PENDING: split-K REDUCE jobs (a layer's dW reduction with its fused SGD or flat DP
#   write) that wait for a later launch to take them along: launch_multi, the
#   tower's dW launch, the embedding update (co_reduce_args); flush_pending at the
#   end of the backward runs whatever is left.
# _FINISH: at most one deferred CTR head finish, taken by the next GEMM launch.
# _FEED_JOB: the batch feed's copy of a later batch (an mrec_feed_job,
#   loader.capture_steps), taken by the next mrec_tower_dw launch: its PCIe reads
#   then run in extra workgroups beside the L2-bound weight-gradient tiles instead
#   of on the step's critical path.
_PENDING = []
_FINISH = []
_FEED_JOB = []
CO_REDUCE_MAX = 6  # reductions one embedding-update launch takes along (gemm_common.h kMaxCoReduce)


def set_feed_job(job):
    _FEED_JOB[:] = [job]


def take_feed_job():
    job = _FEED_JOB[0] if _FEED_JOB else None
    _FEED_JOB.clear()
    return job


def take_pending(n: int):
    """Remove and return up to ``n`` deferred reductions, for a launch that runs
    them beside its own work (``mrec_emb_bwd_apply_ex``)."""
    jobs = _PENDING[:n]
    del _PENDING[:n]
    return jobs


def co_reduce_args():
    """Up to CO_REDUCE_MAX deferred reductions as the ``n_reduce, reduce`` arguments of a
    launch that runs them beside its own work -> (n, GemmCall array or None, keep-alive).
    The array points into the keep-alive: hold it until ``_mrec.call`` has returned."""
    jobs = take_pending(CO_REDUCE_MAX)
    arr = (_mrec.GemmCall * len(jobs))(*[j.struct() for j in jobs]) if jobs else None
    return len(jobs), arr, jobs


def _take_finish():
    """The deferred head finish for the launch about to be made, or None."""
    return _FINISH.pop(0) if _FINISH else None


def _run(jobs):
    if not jobs:
        return
    arr = (_mrec.GemmCall * len(jobs))(*[j.struct() for j in jobs])
    fin = _take_finish()
    if fin is None:
        _mrec.call("mrec_gemm_multi", len(jobs), arr, _mrec.stream_handle())
        return
    _mrec.call("mrec_gemm_multi_ex", len(jobs), arr, None, ctypes.byref(fin.struct),
               _mrec.stream_handle())


def _run_all(jobs):
    """``jobs`` in launches of at most four problems (mrec_gemm_multi's limit)."""
    for i in range(0, len(jobs), 4):
        _run(jobs[i:i + 4])


def _flush_writers(reads):
    """A launch is about to read the addresses ``reads``: if a pending job writes one
    of them, every pending job runs first, in launches of their own."""
    if any(p.writes & reads for p in _PENDING):
        _run_all(take_pending(len(_PENDING)))


def launch_multi(calls):
    """Run ``calls`` plus the pending deferred reductions in as few launches as
    possible (a pending job that writes what a call reads is flushed first)."""
    _flush_writers(set().union(*[c.reads for c in calls]))
    _run_all(list(calls) + take_pending(len(_PENDING)))


class _HeadFinish:
    """One mrec_ctr_head_finish over the head's (w, b, ws, b2): the SGD update in place
    (``lr``, ``params``) or the gradients into ``grads``.  Deferred
    (``defer_head_finish``) it is run by spare workgroups of the next GEMM launch, or
    on its own at the end of the backward."""

    def __init__(self, part, B, H, ns, g, lr=None, params=None, grads=None):
        update = grads is None
        self.keep = [part, g, params, grads]
        ptrs = [_mrec.ptr(t) for t in (params if update else grads)]
        none = [None] * 4
        self.struct = _mrec.HeadFinishJob(part.data_ptr(), part.stride(0), B, H, ns, _mrec.ptr(g),
                                          int(update), float(lr) if update else 0.0,
                                          *(ptrs + none if update else none + ptrs))

    def run(self):
        j = self.struct
        _mrec.call("mrec_ctr_head_finish", j.part, j.ldp, j.batch, j.H, j.ns, j.g, j.update, j.lr,
                   j.w, j.bias, j.ws, j.b2, j.dw_out, j.db_out, j.dws_out, j.db2_out,
                   _mrec.stream_handle())


def defer_head_finish(fin: _HeadFinish):
    _flush_finish()
    _FINISH.append(fin)
    torch.autograd.Variable._execution_engine.queue_callback(flush_pending)


def _flush_finish():
    while _FINISH:
        _FINISH.pop(0).run()


def flush_pending():
    """Apply every deferred reduction now (queued as an autograd end-of-backward
    callback whenever one is deferred, so a backward pass never ends with work
    pending)."""
    _run_all(take_pending(len(_PENDING)))
    _flush_finish()


def _defer(call: "_Call"):
    _PENDING.append(call.with_phase(_mrec.GEMM_REDUCE))
    torch.autograd.Variable._execution_engine.queue_callback(flush_pending)


def weight_prep(W: torch.Tensor, row: bool = True, tr: bool = True):
    """bf16 images of an fp32 [N, K] weight: row [N, r8(K)] and W^T [K, r8(N)]."""
    W = _weight_f32(W)
    N, K = W.shape
    wr = torch.empty(N, _r8(K), dtype=_BF16, device=W.device) if row else None
    wt = torch.empty(K, _r8(N), dtype=_BF16, device=W.device) if tr else None
    _mrec.call("mrec_weight_prep", W.data_ptr(), N, K, W.stride(0), _mrec.ptr(wr),
               wr.stride(0) if wr is not None else 0, _mrec.ptr(wt),
               wt.stride(0) if wt is not None else 0, _mrec.stream_handle())
    return wr, wt


# bf16 images of an fp32 master weight, cached on the Parameter per kind:
#   "rowtr": row-major W and W^T (operands of mrec_gemm);
#   "tower": the MFMA-fragment images of the fused tower (mrec_tower_fwd_bwd);
#   "cin":   the forward and transposed images of a CIN layer (mrec_cin_fwd / _bwd);
#   "autoint": the [Wres | Wq | Wk | Wv] image of an AutoInt layer and its transpose, kept on
#            Wq (mrec_autoint_fwd / _bwd).
# An entry is valid while (weight._version, weight._mrec_gen) is unchanged: torch
# modifying the weight bumps the version; a kernel updating it in place (fused
# SGD) re-emits the images it was handed and ``images_updated`` bumps the
# generation and re-stamps that kind, so only the other kind goes stale.
_IMG_ATTR = {"rowtr": "_mrec_img", "tower": "_mrec_timg", "cin": "_mrec_cimg",
             "autoint": "_mrec_aimg"}


def _img_state(weight):
    return weight._version, getattr(weight, "_mrec_gen", 0)


def cached_images(weight: torch.Tensor, kind: str):
    """The valid cached ``kind`` images of ``weight`` (a pair) or None."""
    c = getattr(weight, _IMG_ATTR[kind], None)
    if (c is not None and (c[0], c[1]) == _img_state(weight) and c[2].device == weight.device):
        return c[2], c[3]
    return None


def images_updated(weight: torch.Tensor, kind: str):
    """An in-place update of ``weight`` (fused SGD) has been enqueued that also
    rewrites its ``kind`` images: they stay valid, every other kind is stale."""
    gen = getattr(weight, "_mrec_gen", 0) + 1
    weight._mrec_gen = gen
    attr = _IMG_ATTR[kind]
    c = getattr(weight, attr, None)
    if c is not None:
        setattr(weight, attr, (weight._version, gen) + tuple(c[2:]))


def weight_images(weight: torch.Tensor):
    """(row, transposed) bf16 images of a Parameter, cached on it and rebuilt only
    when the weight changed since (see ``_IMG_ATTR``)."""
    c = cached_images(weight, "rowtr")
    if c is not None and c[0].shape[0] == weight.shape[0]:
        return c
    wr, wt = weight_prep(weight)
    weight._mrec_img = _img_state(weight) + (wr, wt)
    return wr, wt


def tower_images(weight: torch.Tensor):
    """(fwd, bwd) MFMA-fragment images of a Linear weight [N, K] for the fused
    tower (csrc/tower_common.h), cached like ``weight_images``.  Zero-initialised:
    the prep writes only real elements, the pad entries stay zero."""
    c = cached_images(weight, "tower")
    if c is not None:
        return c
    W = _weight_f32(weight)
    N, K = W.shape
    lib = _mrec.lib()
    pf = torch.zeros(int(lib.mrec_tower_image_elems(N, K, 0)), dtype=_BF16, device=W.device)
    pb = torch.zeros(int(lib.mrec_tower_image_elems(N, K, 1)), dtype=_BF16, device=W.device)
    _mrec.call("mrec_tower_weight_prep", W.data_ptr(), N, K, W.stride(0), pf.data_ptr(),
               pb.data_ptr(), _mrec.stream_handle())
    weight._mrec_timg = _img_state(weight) + (pf, pb)
    return pf, pb


def sgd_lr(*params) -> Optional[float]:
    """The learning rate when every given parameter (None entries ignored) is
    trained by plain SGD fused into its backward (IModel.compile marks them), with
    one common lr; else None (the gradient is returned to the optimizer)."""
    lr = None
    for p in params:
        if p is None:
            continue
        g = getattr(p, "_mrec_sgd_group", None)
        if g is None:
            return None
        if lr is None:
            lr = float(g["lr"])
        elif float(g["lr"]) != lr:
            return None
    return lr


def dp_grads(*params):
    """Data-parallel flat-gradient views of ``params`` (None entries ignored), or
    None unless every given parameter has one (``IModel.distribute`` assigns them:
    the backward kernels write the gradients there, IModel all-reduces the flat
    buffer once and applies SGD with one mrec_sgd_multi launch)."""
    out = []
    for p in params:
        if p is None:
            out.append(None)
            continue
        g = getattr(p, "_mrec_dp_grad", None)
        if g is None:
            return None
        out.append(g)
    return out


# A parameter's gradient goes to exactly one of three places:
#   "sgd": plain SGD fused into the kernel that finishes the gradient (``sgd_lr``):
#          the parameter is updated in place, the bf16 images it was handed are
#          rewritten (``images_updated``) and autograd gets None;
#   "dp":  the parameter's view of the data-parallel flat buffer (``dp_grads``), which
#          IModel all-reduces once and applies with one mrec_sgd_multi; autograd
#          gets None;
#   "ret": a fresh fp32 tensor returned to autograd.
# The parameters decided together share one destination: SGD when all of them have
# one common lr, else DP when all of them have a view, else returned.
_IMG_KIND = {"rowtr": _mrec.IMG_ROW_TR, "tower": _mrec.IMG_TOWER}


def _decide(params, dp: bool = True):
    """(lr, views) of ``params`` decided together: at most one is not None."""
    lr = sgd_lr(*params)
    return lr, (dp_grads(*params) if dp and lr is None else None)


class _GradDest(NamedTuple):
    """The destination of one (W, b) pair's gradients (see above): ``kw`` are the
    destination's keyword arguments of the dW = dY^T [X | 1] GEMM (``_Call`` or
    ``gemm``), ``dW`` / ``db`` what the backward returns to autograd."""
    where: str
    kw: dict
    dW: Optional[torch.Tensor]
    db: Optional[torch.Tensor]


def _grad_dest(W, b, imgs, kind: str, decided=None) -> _GradDest:
    """Where the gradients of W [N, K] and b [N] (or None) go.  ``imgs``: W's cached
    ``kind`` images, which a fused update rewrites; ``decided``: (lr, (W's view, b's
    view) or None) when the pair was decided with others, else ``_decide((W, b))``.
    Call it when the GEMM is built: a fused update is announced here."""
    lr, views = _decide((W, b)) if decided is None else decided
    if lr is not None:
        images_updated(W, kind)
        kw = dict(out=W.detach(), ones_out=None if b is None else b.detach(),
                  out_dtype=torch.float32, sgd_lr=lr, img_row=imgs[0], img_tr=imgs[1],
                  img_kind=_IMG_KIND[kind])
        return _GradDest("sgd", kw, None, None)
    if views is not None:
        kw = dict(out=views[0], ones_out=views[1], out_dtype=torch.float32)
        return _GradDest("dp", kw, None, None)
    dW = torch.empty(W.shape[0], W.shape[1], dtype=torch.float32, device=W.device)
    db = None if b is None else torch.empty(W.shape[0], dtype=torch.float32, device=W.device)
    return _GradDest("ret", dict(out=dW, ones_out=db, out_dtype=torch.float32), dW, db)


_NO_GRAD = _GradDest("ret", {}, None, None)  # no weight gradient is wanted


def _dx_dw(dy, x, wt, N: int, K: int, dest: _GradDest, want_dx: bool = True, **dx_epi):
    """One layer's backward GEMMs over the M rows of dY [M, N] and x [M, K (+ pad)]:
    dx = epi(dY W), shaped like x (B = the W^T image ``wt``; ``dx_epi``: its mask or
    addend), when wanted, and dW, db = dY^T [x | 1] into ``dest``.  -> dx or None.

      dx[m, k] = sum_n dY[m, n] W[n, k]: B(k'=n, col=k) = W^T[k*ld + n] -> ROW
      dW[n, k] = sum_m dY[m, n] x[m, k]: A(i=n, red=m) = dY[m*ld + n] -> COL,
      B(red=m, col=k) = x[m*ld + k] -> COL; ones column -> db

    Returned gradients: plain mrec_gemm calls.  Else one mrec_gemm_multi launch that
    also takes the pending reductions along: with split-K the dW GEMM leaves partial
    slabs there and its reduction (with the update) is deferred to a later launch;
    without it the whole dW GEMM runs beside the dx GEMM -- unless it updates in
    place (fused SGD): its epilogue rewrites ``wt``, which the dx GEMM reads, so it
    gets a launch of its own after it."""
    M, K_x = x.shape
    if dest.where == "ret":
        dx = None
        if want_dx:
            flush_pending()
            dx = gemm(dy, _mrec.LAYOUT_ROW, wt, _mrec.LAYOUT_ROW, M, K_x, N, b_cols=K, **dx_epi)
        if dest is not _NO_GRAD:
            gemm(dy, _mrec.LAYOUT_COL, x, _mrec.LAYOUT_COL, N, K, M, **dest.kw)
        return dx
    cdx = [_Call(dy, _mrec.LAYOUT_ROW, wt, _mrec.LAYOUT_ROW, M, K_x, N, _mrec.GEMM_FULL, b_cols=K,
                 **dx_epi)] if want_dx else []
    sk = _split_beside(N, K + 1, M)
    cdw = _Call(dy, _mrec.LAYOUT_COL, x, _mrec.LAYOUT_COL, N, K, M,
                _mrec.GEMM_PARTIAL if sk > 1 else _mrec.GEMM_FULL, split_k=sk, **dest.kw)
    if sk > 1:
        launch_multi(cdx + [cdw])
        _defer(cdw)
    elif dest.where == "dp":
        launch_multi(cdx + [cdw])
    else:
        launch_multi(cdx)
        launch_multi([cdw])
    return cdx[0].out if cdx else None


def _bf16_rows(t: torch.Tensor) -> torch.Tensor:
    """bf16 [M, N] with 16-byte aligned rows (what mrec_gemm requires); copies into
    an r8-padded buffer only when the input is not already laid out that way."""
    if (t.dtype == _BF16 and t.stride(-1) == 1 and t.stride(0) % 8 == 0
            and t.data_ptr() % 16 == 0):
        return t
    M, N = t.shape
    if N % 8:  # the pad columns are read by 16-B staging: they must be zero
        out = torch.zeros(M, _r8(N), dtype=_BF16, device=t.device)[:, :N]
    else:
        out = _alloc(M, N, _BF16, t.device)
    out.copy_(t)
    return out


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().float().contiguous()


def _weight_f32(w: torch.Tensor) -> torch.Tensor:
    w = w.detach()
    if w.dtype != torch.float32:
        w = w.float()
    return w if w.stride(1) == 1 else w.contiguous()


class _LinearFn(torch.autograd.Function):
    """y = act(x[:, :K] W^T + b) with W [N, K] fp32 (nn.Linear layout).
    x_relu: x is a ReLU output, so dx is masked by x in the dx GEMM's epilogue.
    dW and db go where ``_grad_dest`` says."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool, out_dtype, x_relu: bool):
        x = _bf16_rows(x)
        M, K_x = x.shape
        N, K = weight.shape
        flush_pending()
        wr, wt = weight_images(weight)
        y = gemm(x, _mrec.LAYOUT_ROW, wr[:, :K], _mrec.LAYOUT_ROW, M, N, K, bias=_f32c(bias),
                 act=_mrec.ACT_RELU if relu else _mrec.ACT_NONE, out_dtype=out_dtype)
        ctx.save_for_backward(x, y if relu else None)
        ctx.relu, ctx.NK, ctx.x_relu = relu, (N, K), x_relu
        ctx.y_ptr = y.data_ptr()
        ctx.weight, ctx.bias, ctx.wr, ctx.wt = weight, bias, wr, wt
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        N, K = ctx.NK
        if ctx.relu and not _premasked(dy, ctx.y_ptr):
            dy = torch.where(y > 0, dy.to(y.dtype), torch.zeros((), dtype=y.dtype, device=y.device))
        dy = _bf16_rows(dy)
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dest = _grad_dest(ctx.weight, ctx.bias, (ctx.wr, ctx.wt), "rowtr") if need_w else _NO_GRAD
        dx = _dx_dw(dy, x, ctx.wt, N, K, dest, ctx.needs_input_grad[0],
                    mask=x if ctx.x_relu else None)
        if ctx.x_relu and dx is not None:
            _stamp(dx, x)
        return dx, dest.dW, dest.db, None, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
           act: Optional[str] = None, out_dtype=_BF16) -> torch.Tensor:
    """y = act(x W^T + b), W stored [out, in] like nn.Linear (Dense.py:12).  x may
    carry zero pad columns beyond in_features; they are ignored (and get a zero
    gradient)."""
    if not x.is_cuda:
        k = weight.shape[1]
        xx = x[:, :k] if x.shape[1] > k else x
        y = F.linear(xx.float(), weight.float(), None if bias is None else bias.float())
        return torch.relu(y) if act == "relu" else y
    y = _LinearFn.apply(x, weight, bias, act == "relu", out_dtype, _is_relu_out(x))
    if act == "relu":
        setattr(y, _RELU_OUT, True)
    return y


def _cross_fwd(x0, xl, W, b):
    """x0 * (x_l W^T + b) + x_l as one GEMM -> (it, z = x_l W^T + b, W's row and
    transposed images)."""
    M, d = xl.shape[0], W.shape[0]
    wr, wt = weight_images(W)
    z = _alloc(M, d, _BF16, xl.device)
    out = gemm(xl, _mrec.LAYOUT_ROW, wr[:, :d], _mrec.LAYOUT_ROW, M, d, d, bias=_f32c(b), mul=x0,
               add=xl, aux=z)
    return out, z, wr, wt


class _CrossFn(torch.autograd.Function):
    """DCN-v2 layer x_{l+1} = x0 * (x_l W^T + b) + x_l (one GEMM, epilogue fused;
    z = x_l W^T + b kept for the backward)."""

    @staticmethod
    def forward(ctx, x0, xl, weight, bias):
        x0, xl = _bf16_rows(x0), _bf16_rows(xl)
        out, z, wr, wt = _cross_fwd(x0, xl, weight, bias)
        ctx.save_for_backward(x0, xl, z)
        ctx.weight, ctx.bias, ctx.wr, ctx.wt = weight, bias, wr, wt
        return out

    @staticmethod
    def backward(ctx, g):
        x0, xl, z = ctx.saved_tensors
        wt = ctx.wt
        g = _bf16_rows(g)
        M = g.shape[0]
        d = z.shape[1]
        # dz = g * x0; dx_l = dz W + g; dW = dz^T x_l; db = sum dz
        dz = _alloc(M, d, _BF16, g.device)
        torch.mul(g[:, :d], x0[:, :d], out=dz)
        if dz.stride(0) > d:
            dz.as_strided((M, dz.stride(0) - d), (dz.stride(0), 1), d).zero_()
        dxl = gemm(dz, _mrec.LAYOUT_ROW, wt, _mrec.LAYOUT_ROW, M, xl.shape[1], d, b_cols=d,
                   add=_pad_cols(g, xl.shape[1]))
        # fused SGD or returned: this single-layer op has no data-parallel destination
        dest = _grad_dest(ctx.weight, ctx.bias, (ctx.wr, wt), "rowtr",
                          _decide((ctx.weight, ctx.bias), dp=False))
        gemm(dz, _mrec.LAYOUT_COL, xl, _mrec.LAYOUT_COL, d, d, M, **dest.kw)
        dx0 = (g.float() * z.float()).to(_BF16)
        if x0.shape[1] > d:
            dx0 = F.pad(dx0, (0, x0.shape[1] - d))
        return dx0, dxl, dest.dW, dest.db


class _CrossNetFn(torch.autograd.Function):
    """The whole DCN-v2 cross network x_{l+1} = x0 * (x_l W_l^T + b_l) + x_l,
    l = 0..L-1, as one autograd node: forward = one fused GEMM per layer; backward
    per layer = ONE elementwise kernel (mrec_dcn_cross_bwd_prep: dz = g*x0 and the
    fp32 sum over layers of g*z, i.e. x0's multiplier gradient) + the dx_l GEMM
    (layer 0 adds that sum, so its output is dx0) + the dW GEMM (``_grad_dest`` per
    layer)."""

    @staticmethod
    def forward(ctx, x0, n, *params):
        weights, biases = params[:n], params[n:]
        x0 = _bf16_rows(x0)
        xl = x0
        saved = []
        for W, b in zip(weights, biases):
            out, z, wr, wt = _cross_fwd(x0, xl, W, b)
            saved.append((xl, z, wr, wt))
            xl = out
        ctx.x0, ctx.saved, ctx.weights, ctx.biases = x0, saved, weights, biases
        return xl

    @staticmethod
    def backward(ctx, g):
        x0, saved = ctx.x0, ctx.saved
        L = len(saved)
        g = _bf16_rows(g)
        M = g.shape[0]
        d = saved[0][1].shape[1]
        acc = torch.empty(M, _r8(d), dtype=torch.float32, device=g.device)
        dWs, dbs = [None] * L, [None] * L
        for l in reversed(range(L)):
            xl, z, wr, wt = saved[l]
            W, b = ctx.weights[l], ctx.biases[l]
            dz = _alloc(M, d, _BF16, g.device)
            addend = _alloc(M, xl.shape[1], _BF16, g.device) if l == 0 else None
            _mrec.call("mrec_dcn_cross_bwd_prep", M, d, g.data_ptr(), g.stride(0),
                       x0.data_ptr(), x0.stride(0), z.data_ptr(), z.stride(0), dz.data_ptr(),
                       dz.stride(0), acc.data_ptr(), acc.stride(0), int(l == L - 1),
                       _mrec.ptr(addend), addend.stride(0) if addend is not None else 0,
                       _mrec.stream_handle())
            # dx_l = dz W (+ g: x_l feeds the residual; layer 0: + sum_l g_l*z_l too)
            add = addend if l == 0 else _pad_cols(g, xl.shape[1])
            dest = _grad_dest(W, b, (wr, wt), "rowtr")
            dWs[l], dbs[l] = dest.dW, dest.db
            g = _dx_dw(dz, xl, wt, d, d, dest, add=add)
        ctx.saved = None
        return (g, None, *dWs, *dbs)


def cross_net(x0: torch.Tensor, weights: Sequence[torch.Tensor],
              biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """A stack of DCN-v2 cross layers over x0 (one autograd node on the GPU)."""
    if not x0.is_cuda or any(b is None for b in biases):
        x = x0
        for W, b in zip(weights, biases):
            x = cross(x0, x, W, b)
        return x
    return _CrossNetFn.apply(x0, len(weights), *weights, *biases)


def _pad_cols(t: torch.Tensor, n: int) -> torch.Tensor:
    if t.shape[1] == n:
        return t
    out = torch.zeros(t.shape[0], _r8(n), dtype=t.dtype, device=t.device)[:, :n]
    out[:, :t.shape[1]] = t
    return out


def cross(x0: torch.Tensor, xl: torch.Tensor, weight: torch.Tensor,
          bias: Optional[torch.Tensor]) -> torch.Tensor:
    """DCN-v2 cross layer x_{l+1} = x0 * (W x_l + b) + x_l."""
    d = weight.shape[1]
    if not xl.is_cuda:
        x0c = x0[:, :d].float()
        xlc = xl[:, :d].float()
        return x0c * F.linear(xlc, weight.float(), None if bias is None else bias.float()) + xlc
    return _CrossFn.apply(x0, xl, weight, bias)


def din_attention(q: torch.Tensor, k: torch.Tensor, valid: torch.Tensor, att_mlp,
                  att_out: torch.nn.Linear):
    """DIN target attention (torch ops; the CPU path and the reference restatement):
    s_j = att_out(att_mlp([q, k_j, q-k_j, q*k_j])); a = softmax over valid j
    (invalid -> -inf, SASRec.py:26-29); u = sum_j a_j k_j.
    q [B, E], k [B, L, E], valid [B, L] bool -> u [B, E] (fp32)."""
    B, L, E = k.shape
    qb = q.unsqueeze(1).expand(B, L, E).to(k.dtype)
    feat = torch.cat([qb, k, qb - k, qb * k], dim=-1).reshape(B * L, 4 * E)
    h = att_mlp(feat)
    s = linear(h, att_out.weight, att_out.bias, out_dtype=torch.float32).float().reshape(B, L)
    s = s.masked_fill(~valid, float("-inf"))
    a = torch.softmax(s, dim=-1)
    return (a.unsqueeze(-1) * k.float()).sum(1)


class _DinState:
    """Carries the pooling backward's dk / dq pieces to the feature backward (the
    pooling backward always runs first: its ds feeds the attention MLP backward)."""


class _DinFeatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, st: _DinState, L: int):
        B, E = q.shape
        feat = _alloc(B * L, 4 * E, _BF16, q.device)
        _mrec.call("mrec_din_feat_fwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), B, L,
                   E, feat.data_ptr(), feat.stride(0), _mrec.stream_handle())
        ctx.save_for_backward(q, k)
        ctx.st, ctx.L = st, L
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        q, k = ctx.saved_tensors
        st = ctx.st
        B, E = q.shape
        dfeat = _bf16_rows(dfeat)
        dq = torch.empty(B, E, dtype=torch.float32, device=q.device)
        _mrec.call("mrec_din_feat_bwd", dfeat.data_ptr(), dfeat.stride(0), st.dtop.data_ptr(),
                   st.dtop.stride(0), q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), B,
                   ctx.L, E, st.dk.data_ptr(), st.dk.stride(0), dq.data_ptr(), dq.stride(0),
                   _mrec.stream_handle())
        dk = st.dk
        del st.dk, st.dtop
        return dq, dk, None, None


class _DinPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, q, k, his, st: _DinState, L: int):
        B, E = q.shape
        a = torch.empty(B, L, dtype=torch.float32, device=q.device)
        top = _alloc(B, 2 * E, _BF16, q.device)
        his = his.to(torch.int32)
        _mrec.call("mrec_din_pool_fwd", s.data_ptr(), s.stride(0), his.data_ptr(), his.stride(0),
                   q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), B, L, E, a.data_ptr(),
                   top.data_ptr(), top.stride(0), _mrec.stream_handle())
        ctx.save_for_backward(a, k)
        ctx.st, ctx.L, ctx.E, ctx.s_shape = st, L, E, s.shape
        return top

    @staticmethod
    def backward(ctx, dtop):
        a, k = ctx.saved_tensors
        st = ctx.st
        B, L, E = a.shape[0], ctx.L, ctx.E
        dtop = _bf16_rows(dtop)
        ds = torch.empty(B * L, 1, dtype=torch.float32, device=a.device)
        dk = torch.empty(B * L, E, dtype=torch.float32, device=a.device)
        _mrec.call("mrec_din_pool_bwd", dtop.data_ptr(), dtop.stride(0), a.data_ptr(), k.data_ptr(),
                   k.stride(0), B, L, E, ds.data_ptr(), dk.data_ptr(), dk.stride(0),
                   _mrec.stream_handle())
        st.dk, st.dtop = dk, dtop
        return ds, None, None, None, None, None


class _DinRowsFeatFn(torch.autograd.Function):
    """_DinFeatFn over the gathered rows [q (B) | k (B L)] as ONE input: the backward
    returns the rows' bf16 gradient from one kernel (mrec_din_feat_bwd_rows), so
    autograd adds no slice-backward zero fills, copies or dtype casts."""

    @staticmethod
    def forward(ctx, rows, B: int, st: _DinState, L: int):
        q, k = rows[:B], rows[B:]
        E = rows.shape[1]
        feat = _alloc(B * L, 4 * E, _BF16, rows.device)
        _mrec.call("mrec_din_feat_fwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), B, L,
                   E, feat.data_ptr(), feat.stride(0), _mrec.stream_handle())
        ctx.save_for_backward(rows)
        ctx.st, ctx.L, ctx.B = st, L, B
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        rows, = ctx.saved_tensors
        st, B, L = ctx.st, ctx.B, ctx.L
        q, k = rows[:B], rows[B:]
        E = rows.shape[1]
        dfeat = _bf16_rows(dfeat)
        d_rows = torch.empty_like(rows)
        _mrec.call("mrec_din_feat_bwd_rows", dfeat.data_ptr(), dfeat.stride(0), st.dtop.data_ptr(),
                   st.dtop.stride(0), q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), B, L, E,
                   st.dk.data_ptr(), st.dk.stride(0), d_rows.data_ptr(), d_rows.stride(0),
                   _mrec.stream_handle())
        del st.dk, st.dtop
        return d_rows, None, None, None


def _din_scores(feat: torch.Tensor, att_mlp, att_out: torch.nn.Linear) -> torch.Tensor:
    """Attention-unit scores [B L, 1] fp32: the attention MLP's GEMMs + Linear(h, 1).
    Not the score tower (score_tower): measured at C4 it is slower than the GEMMs
    (fwd 279, bwd 527, weight gradients 213 us vs ~360 us for the GEMM path in all):
    12,800 16-row workgroups at 2 per CU run 25 residency rounds of the tower's
    latency chain, and the k-fragment images of 204,800 rows go through HBM."""
    h = att_mlp(feat)
    return linear(h, att_out.weight, att_out.bias, out_dtype=torch.float32)


# the fused attention unit (mrec_din_att_*, din_att.hip) is the default for the
# compiled shapes; False selects the layered kernels (the parity tests set it)
DIN_FUSED = True


def _din_att_linears(att_mlp, att_out):
    lins = [m for m in att_mlp.modules() if isinstance(m, torch.nn.Linear)]
    return lins + [att_out]


def din_att_supported(E: int, att_mlp, att_out: torch.nn.Linear) -> bool:
    """True when the fused attention unit covers this block: two ReLU Dense layers
    + Linear(H2, 1), all with bias, no active dropout, a compiled (E, H1, H2)."""
    lins = _din_att_linears(att_mlp, att_out)
    if len(lins) != 3 or any(m.bias is None for m in lins) or lins[2].out_features != 1:
        return False
    if att_mlp.training and any(isinstance(m, torch.nn.Dropout) and m.p > 0
                                for m in att_mlp.modules()):
        return False
    H1, H2 = lins[0].out_features, lins[1].out_features
    if (lins[0].in_features != 4 * E or lins[1].in_features != H1
            or lins[2].in_features != H2):
        return False
    return bool(_mrec.lib().mrec_din_att_supported(E, H1, H2))


def _weights_changed(*params):
    """An in-place kernel update of these fp32 masters that re-emitted no image:
    every cached bf16 image kind goes stale."""
    for p in params:
        p._mrec_gen = getattr(p, "_mrec_gen", 0) + 1


class _DinAttFn(torch.autograd.Function):
    """The whole DIN attention unit over the gathered rows [q (B) | k (B L)]: one
    forward launch (features, MLP, scores, masked softmax, pooling -> top) and one
    backward launch (the rows' bf16 gradient + weight-gradient partials) plus the
    partials' fixed-order sum, which applies the fused SGD when the optimizer is
    plain SGD (sgd_lr) or hands the gradients to it."""

    @staticmethod
    def forward(ctx, rows, his, B: int, L: int, w1, b1, w2, b2, w3, b3):
        E = rows.shape[1]
        H1, H2 = w1.shape[0], w2.shape[0]
        ws = [_weight_f32(w1), b1.detach().float().contiguous(), _weight_f32(w2),
              b2.detach().float().contiguous(), w3.detach().float().reshape(-1).contiguous(),
              b3.detach().float().contiguous()]
        his = his.to(torch.int32)
        if his.stride(1) != 1:
            his = his.contiguous()
        a = torch.empty(B, L, dtype=torch.float32, device=rows.device)
        top = _alloc(B, 2 * E, _BF16, rows.device)
        _mrec.call("mrec_din_att_fwd", rows.data_ptr(), rows.stride(0), his.data_ptr(),
                   his.stride(0), B, L, E, ws[0].data_ptr(), ws[0].stride(0), ws[1].data_ptr(),
                   H1, ws[2].data_ptr(), ws[2].stride(0), ws[3].data_ptr(), H2, ws[4].data_ptr(),
                   ws[5].data_ptr(), a.data_ptr(), top.data_ptr(), top.stride(0),
                   _mrec.stream_handle())
        ctx.save_for_backward(rows, a)
        ctx.ws, ctx.params, ctx.B, ctx.L = ws, (w1, b1, w2, b2, w3, b3), B, L
        return top

    @staticmethod
    def backward(ctx, dtop):
        rows, a = ctx.saved_tensors
        ws, params, B, L = ctx.ws, ctx.params, ctx.B, ctx.L
        E = rows.shape[1]
        H1, H2 = params[0].shape[0], params[2].shape[0]
        dtop = _bf16_rows(dtop)
        d_rows = _alloc(rows.shape[0], E, _BF16, rows.device)
        lib = _mrec.lib()
        parts = int(lib.mrec_din_att_parts(B))
        P = int(lib.mrec_din_att_param_count(E, H1, H2))
        part = torch.empty(parts, P, dtype=torch.float32, device=rows.device)
        st = _mrec.stream_handle()
        _mrec.call("mrec_din_att_bwd", rows.data_ptr(), rows.stride(0), B, L, E,
                   ws[0].data_ptr(), ws[0].stride(0), ws[1].data_ptr(), H1, ws[2].data_ptr(),
                   ws[2].stride(0), ws[3].data_ptr(), H2, ws[4].data_ptr(), ws[5].data_ptr(),
                   a.data_ptr(), dtop.data_ptr(), dtop.stride(0), d_rows.data_ptr(),
                   d_rows.stride(0), part.data_ptr(), parts, st)
        ctx.ws = None
        w1, b1, w2, b2, w3, b3 = params
        lr = sgd_lr(*params)
        inplace = (lr is not None and all(p.dtype == torch.float32 and p.is_contiguous()
                                          for p in params))
        if inplace:
            _mrec.call("mrec_din_att_wgrad", part.data_ptr(), parts, E, H1, H2, None, lr,
                       w1.data_ptr(), w1.stride(0), b1.data_ptr(), w2.data_ptr(), w2.stride(0),
                       b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), st)
            _weights_changed(*params)
            return d_rows, None, None, None, None, None, None, None, None, None
        g = torch.empty(P, dtype=torch.float32, device=rows.device)
        _mrec.call("mrec_din_att_wgrad", part.data_ptr(), parts, E, H1, H2, g.data_ptr(), 0.0,
                   None, 0, None, None, 0, None, None, None, st)
        gw1, gw2, gb1, gb2, gw3, gb3 = torch.split(g, [H1 * 4 * E, H2 * H1, H1, H2, H2, 1])
        grads = [t.view_as(p) for t, p in zip((gw1, gb1, gw2, gb2, gw3, gb3), params)]
        dpg = dp_grads(*params)
        if dpg is not None:  # data parallel: into the flat buffer IModel all-reduces
            for dst, src in zip(dpg, grads):
                dst.copy_(src.view_as(dst))
            return d_rows, None, None, None, None, None, None, None, None, None
        return (d_rows, None, None, None, *grads)


def din_attention_top_rows(rows: torch.Tensor, B: int, his: torch.Tensor, att_mlp,
                           att_out: torch.nn.Linear) -> torch.Tensor:
    """din_attention_top over the gather output rows [q (B) | k (B L)] (bf16, 16-B
    aligned rows): the rows' gradient comes back as one bf16 tensor.  The fused
    attention unit (one launch each way) when it covers the block."""
    L = his.shape[1]
    rows = _bf16_rows(rows)
    if DIN_FUSED and din_att_supported(rows.shape[1], att_mlp, att_out):
        w1, w2, w3 = (m.weight for m in _din_att_linears(att_mlp, att_out))
        b1, b2, b3 = (m.bias for m in _din_att_linears(att_mlp, att_out))
        return _DinAttFn.apply(rows, his, B, L, w1, b1, w2, b2, w3, b3)
    st = _DinState()
    feat = _DinRowsFeatFn.apply(rows, B, st, L)
    s = _din_scores(feat, att_mlp, att_out)
    r = rows.detach()
    return _DinPoolFn.apply(s, r[:B], r[B:], his, st, L)


def din_attention_top(q: torch.Tensor, k: torch.Tensor, his: torch.Tensor, att_mlp,
                      att_out: torch.nn.Linear) -> torch.Tensor:
    """The DIN top-MLP input [q | u] (bf16 [B, 2E]) on libmrec kernels: attention-unit
    input builder, MFMA attention MLP + Linear(h, 1), masked-softmax pooling; the
    backward is the pooling / builder kernels.  q [B, E], k [B*L, E] (bf16, the
    gathered target and history rows), his [B, L] ids (validity)."""
    B, E = q.shape
    L = his.shape[1]
    q, k = _bf16_rows(q), _bf16_rows(k)
    st = _DinState()
    feat = _DinFeatFn.apply(q, k, st, L)
    s = _din_scores(feat, att_mlp, att_out)
    return _DinPoolFn.apply(s, q, k, his, st, L)


# the fused SASRec encoder (mrec_sasrec_*, sasrec.hip) is the default for the compiled
# shapes; False selects the layered path (the parity tests set it)
SASREC_FUSED = True


def sasrec_supported(D: int, L: int, num_layers: int = 1, dropout: float = 0.0,
                     training: bool = False) -> bool:
    """True when the fused encoder covers this block: a compiled (D, L), at least one
    layer and no active dropout.  Decided from the shape alone; never an error."""
    if num_layers < 1 or (training and dropout > 0):
        return False
    return bool(_mrec.lib().mrec_sasrec_supported(int(D), int(L)))


def _sasrec_params(model):
    ln = model.layer_norm
    return (model.p_embeddings.weight, model.Q.weight, model.K.weight, model.W1.weight,
            model.W1.bias, model.W2.weight, model.W2.bias, ln.weight, ln.bias)


def _sum_partials(bwd_name, a, rows, parts, P, sizes, params, dev, order=None):
    """The tail the fused encoders' backwards share.  ``bwd_name`` (argument block ``a``,
    launched when there are ``rows``) leaves per-workgroup partials [parts, P] of the dense
    gradients; mrec_sasrec_wgrad, which is shape-agnostic, sums them in workgroup order.
    The sum is split by ``sizes`` and piece ``order[i]`` (piece i without ``order``) is
    parameter i's gradient.  -> the gradients of ``params``; under data parallelism they
    go into the flat buffer IModel all-reduces instead and every entry is None."""
    part = torch.empty(parts, P, dtype=torch.float32, device=dev)
    g = torch.zeros(P, dtype=torch.float32, device=dev)
    a.part, a.parts = part.data_ptr(), parts
    st = _mrec.stream_handle()
    if rows:
        _mrec.call(bwd_name, ctypes.byref(a), st)
        _mrec.call("mrec_sasrec_wgrad", part.data_ptr(), parts, P, g.data_ptr(), st)
    pieces = torch.split(g, sizes)
    if order is not None:
        pieces = [pieces[i] for i in order]
    grads = [t.view_as(p) for t, p in zip(pieces, params)]
    dpg = dp_grads(*params)
    if dpg is None:
        return tuple(grads)
    for dst, src in zip(dpg, grads):
        dst.copy_(src.view_as(dst))
    return (None,) * len(params)


class _SasrecFn(torch.autograd.Function):
    """The whole SASRec encoder over the gathered history rows [B, L, D]: one forward
    launch (every layer -> v [B, D], the layer outputs saved), one backward launch
    (the rows' bf16 gradient + per-workgroup partials of the nine dense gradients) and
    the partials' fixed-order sum."""

    @staticmethod
    def forward(ctx, rows, his, his_len, check: bool, eps: float, num_layers: int, pos, wq, wk,
                w1, b1, w2, b2, gamma, beta):
        B, L, D = rows.shape
        dev = rows.device
        rows2 = _bf16_rows(rows.reshape(B * L, D))
        his = his.to(torch.int32)
        if his.stride(1) != 1:
            his = his.contiguous()
        his_len = his_len.reshape(-1).to(torch.int32).contiguous()
        ws = [_weight_f32(pos), _weight_f32(wq), _weight_f32(wk), _weight_f32(w1), _f32c(b1),
              _weight_f32(w2), _f32c(b2), _f32c(gamma), _f32c(beta)]
        hs = torch.empty(num_layers, B, L, D, dtype=_BF16, device=dev)
        v = torch.empty(B, D, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
        a = _mrec.SasrecArgs(
            rows2.data_ptr(), rows2.stride(0), his.data_ptr(), his.stride(0), his_len.data_ptr(),
            ws[0].data_ptr(), ws[0].stride(0), ws[0].shape[0], ws[1].data_ptr(), ws[1].stride(0),
            ws[2].data_ptr(), ws[2].stride(0), ws[3].data_ptr(), ws[3].stride(0),
            ws[4].data_ptr(), ws[5].data_ptr(), ws[5].stride(0), ws[6].data_ptr(),
            ws[7].data_ptr(), ws[8].data_ptr(), float(eps), int(num_layers), B, L, D,
            hs.data_ptr(), v.data_ptr(), _mrec.ptr(flag), None, None, 0, None, 0)
        if B:
            _mrec.call("mrec_sasrec_fwd", ctypes.byref(a), _mrec.stream_handle())
        if flag is not None and int(flag.item()) != 0:
            raise IndexError("index out of range in self")
        a.d_oob_flag = None
        ctx.args, ctx.keep = a, (rows2, his, his_len, ws, hs)
        ctx.params = (pos, wq, wk, w1, b1, w2, b2, gamma, beta)
        return v

    @staticmethod
    def backward(ctx, dv):
        a, (rows2, his, his_len, ws, hs) = ctx.args, ctx.keep
        params = ctx.params
        B, L, D = int(a.batch), int(a.L), int(a.D)
        dev = rows2.device
        dv = dv.detach().float().contiguous()
        d_rows = torch.empty(B * L, D, dtype=_BF16, device=dev)
        a.dv, a.d_rows, a.ld_drows = dv.data_ptr(), d_rows.data_ptr(), d_rows.stride(0)
        lib = _mrec.lib()
        # the kernel's partial: [wq, wk, w1, w2, b1, b2, gamma, beta, pos]
        sizes = [D * D] * 4 + [D] * 4 + [ws[0].shape[0] * D]
        grads = _sum_partials("mrec_sasrec_bwd", a, B, int(lib.mrec_sasrec_parts(B)),
                              int(lib.mrec_sasrec_param_count(D, ws[0].shape[0])), sizes,
                              params, dev, order=(8, 0, 1, 2, 4, 3, 5, 6, 7))
        ctx.args = ctx.keep = None
        return (d_rows.reshape(B, L, D), None, None, None, None, None) + grads


def sasrec_encode(rows: torch.Tensor, his: torch.Tensor, his_len: torch.Tensor,
                  model) -> torch.Tensor:
    """v [B, D] (fp32) of the SASRec encoder over the gathered history rows [B, L, D]
    with ``model``'s shared block (p_embeddings, Q, K, W1, W2, layer_norm, num_layers,
    dropout).  On a GPU the fused kernels when they cover the shape; else, on the CPU
    and when dropout is active, the layered path: the same arithmetic as torch ops
    (``cpu_path.sasrec_encode``), rounding to bf16 on a GPU where the kernel does."""
    from pytorchrec_amd import cpu_path
    B, L, D = rows.shape
    params = _sasrec_params(model)
    eps, nl = model.layer_norm.eps, model.num_layers
    if (rows.is_cuda and SASREC_FUSED
            and sasrec_supported(D, L, nl, model.dropout, model.training)
            and all(p.dtype == torch.float32 for p in params)):
        check = bool(getattr(model.i_embeddings, "check_ids", True))
        return _SasrecFn.apply(rows, his, his_len, check, eps, nl, *params)
    return cpu_path.sasrec_encode(rows, his, his_len, *params, eps, nl, dropout=model.dropout,
                                  training=model.training,
                                  rnd=cpu_path.bf16_round if rows.is_cuda else None)


# the fused GRU4Rec encoder (mrec_gru_*, gru.hip) is the default for the compiled shapes;
# False selects the layered path (the parity tests set it)
GRU_FUSED = True


def gru_supported(E: int, H: int, L: int) -> bool:
    """True when the fused recurrence covers (E, H, L).  Decided from the shape alone;
    never an error."""
    return bool(_mrec.lib().mrec_gru_supported(int(E), int(H), int(L)))


def _gru_params(model):
    rnn = model.rnn
    return (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)


class _GruFn(torch.autograd.Function):
    """The whole GRU recurrence over the gathered history rows [B, L, E]: one forward
    launch (-> h_last [B, H], the fp32 hidden sequence saved), one backward launch (the
    rows' bf16 gradient + per-workgroup partials of the four dense gradients) and the
    partials' fixed-order sum (mrec_sasrec_wgrad, which is shape-agnostic)."""

    @staticmethod
    def forward(ctx, rows, his_len, order, check: bool, w_ih, w_hh, b_ih, b_hh):
        B, L, E = rows.shape
        H = w_hh.shape[1]
        dev = rows.device
        rows2 = _bf16_rows(rows.reshape(B * L, E))
        his_len = his_len.reshape(-1).to(torch.int32).contiguous()
        if order is not None:
            order = order.reshape(-1).to(torch.int32).contiguous()
        ws = [_weight_f32(w_ih), _weight_f32(w_hh), _f32c(b_ih), _f32c(b_hh)]
        hs = torch.empty(B, L, H, dtype=torch.float32, device=dev)
        h_last = torch.empty(B, H, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
        a = _mrec.GruArgs(
            rows2.data_ptr(), rows2.stride(0), his_len.data_ptr(), _mrec.ptr(order),
            ws[0].data_ptr(), ws[0].stride(0), ws[1].data_ptr(), ws[1].stride(0),
            ws[2].data_ptr(), ws[3].data_ptr(), E, H, L, B, hs.data_ptr(), h_last.data_ptr(),
            _mrec.ptr(flag), None, None, 0, None, 0)
        if B:
            _mrec.call("mrec_gru_fwd", ctypes.byref(a), _mrec.stream_handle())
        if flag is not None and int(flag.item()) != 0:
            raise IndexError("index out of range in self")
        a.d_oob_flag = None
        ctx.args, ctx.keep = a, (rows2, his_len, order, ws, hs)
        ctx.params = (w_ih, w_hh, b_ih, b_hh)
        return h_last

    @staticmethod
    def backward(ctx, dh):
        a, (rows2, his_len, order, ws, hs) = ctx.args, ctx.keep
        params = ctx.params
        B, L, E, H = int(a.batch), int(a.L), int(a.E), int(a.H)
        dev = rows2.device
        dh = dh.detach().float().contiguous()
        d_rows = torch.empty(B * L, E, dtype=_BF16, device=dev)
        a.dh_last, a.d_rows, a.ld_drows = dh.data_ptr(), d_rows.data_ptr(), d_rows.stride(0)
        lib = _mrec.lib()
        grads = _sum_partials("mrec_gru_bwd", a, B, int(lib.mrec_gru_parts(B)),
                              int(lib.mrec_gru_param_count(E, H)),
                              [3 * H * E, 3 * H * H, 3 * H, 3 * H], params, dev)
        ctx.args = ctx.keep = None
        return (d_rows.reshape(B, L, E), None, None, None) + grads


def gru_encode(rows: torch.Tensor, his_len: torch.Tensor, model, order="auto") -> torch.Tensor:
    """h_{his_len - 1} [B, H] (fp32) of ``model.rnn`` (weight_ih_l0, weight_hh_l0,
    bias_ih_l0, bias_hh_l0) over the gathered history rows [B, L, E].  On a GPU the fused
    kernels when they cover the shape; else, and on the CPU, the layered path: the same
    arithmetic as torch ops (``cpu_path.gru_encode``), rounding to bf16 on a GPU where the
    kernel does.  ``order`` places samples in the kernel's tiles: "sorted" (by length,
    descending, as the reference's own topk), None (batch order), an int permutation, or
    "auto": sorted when the batch has more tiles than the launch has workgroups (each
    workgroup then runs several tiles back to back, and tiles of equal lengths shorten
    their sum), batch order otherwise (every tile has a workgroup of its own, the launch
    lasts as long as its longest sample either way, and the sort is pure overhead:
    DESIGN.md §3.14).  It changes speed only."""
    from pytorchrec_amd import cpu_path
    B, L, E = rows.shape
    params = _gru_params(model)
    check = bool(getattr(getattr(model, "i_embeddings", None), "check_ids", True))
    if (rows.is_cuda and GRU_FUSED and gru_supported(E, params[1].shape[1], L)
            and all(p.dtype == torch.float32 for p in params)):
        if isinstance(order, str):
            if order not in ("auto", "sorted"):
                raise ValueError(f"order must be 'auto', 'sorted', None or a permutation: {order}")
            lib = _mrec.lib()
            if order == "sorted" or B > int(lib.mrec_gru_parts(B)) * int(lib.mrec_gru_tile()):
                order = torch.argsort(his_len.reshape(-1), descending=True, stable=True)
            else:
                order = None
        return _GruFn.apply(rows, his_len, order, check, *params)
    return cpu_path.gru_encode(rows, his_len, *params,
                               rnd=cpu_path.bf16_round if rows.is_cuda else None, check=check)


# the fused NCF pair scorer (mrec_ncf_*, ncf.hip) is the default for the compiled shapes;
# False selects the layered path (the parity tests and the benchmark set it)
NCF_FUSED = True


def _ncf_widths(widths):
    ws = [int(w) for w in widths]
    return len(ws), (ctypes.c_int32 * max(len(ws), 1))(*ws)


def ncf_supported(E: int, widths) -> bool:
    """True when the fused scorer covers (emb_size, hidden widths).  Decided from the
    shape alone; never an error."""
    nl, arr = _ncf_widths(widths)
    return bool(_mrec.lib().mrec_ncf_supported(int(E), nl, arr))


def _ncf_params(model):
    lin = [d.linear for d in model.mlp.mlp]
    return [m.weight for m in lin], [m.bias for m in lin], model.prediction.weight


class _NcfFn(torch.autograd.Function):
    """The whole NCF scorer over the gathered rows [pairs, 4E]: one forward launch
    (-> pred [pairs], nothing saved but the rows), one backward launch (the rows' bf16
    gradient + per-workgroup partials of the dense gradients, the forward recomputed)
    and the partials' fixed-order sum (mrec_sasrec_wgrad, which is shape-agnostic)."""

    @staticmethod
    def forward(ctx, rows, E: int, nl: int, *params):
        # params = w_0 .. w_{k-1}, b_0 .. b_{k-1}, wp
        pairs = rows.shape[0]
        dev = rows.device
        rows2 = _bf16_rows(rows)
        ws = [_weight_f32(w) for w in params[:nl]]
        bs = [_f32c(b) for b in params[nl:2 * nl]]
        wp = _f32c(params[2 * nl]).reshape(-1)
        pred = torch.empty(pairs, dtype=torch.float32, device=dev)
        a = _mrec.NcfArgs()
        a.rows, a.ld_rows, a.pairs = rows2.data_ptr(), rows2.stride(0), pairs
        a.E, a.n_layers = int(E), int(nl)
        for l in range(nl):
            a.widths[l] = ws[l].shape[0]
            a.w[l], a.ld_w[l], a.b[l] = ws[l].data_ptr(), ws[l].stride(0), bs[l].data_ptr()
        a.wp, a.pred = wp.data_ptr(), pred.data_ptr()
        if pairs:
            _mrec.call("mrec_ncf_fwd", ctypes.byref(a), _mrec.stream_handle())
        ctx.args, ctx.keep = a, (rows2, ws, bs, wp)
        ctx.params = params
        return pred

    @staticmethod
    def backward(ctx, dpred):
        a, (rows2, ws, bs, wp) = ctx.args, ctx.keep
        params = ctx.params
        pairs, E, nl = int(a.pairs), int(a.E), int(a.n_layers)
        dev = rows2.device
        dpred = dpred.detach().float().contiguous()
        d_rows = torch.empty(pairs, 4 * E, dtype=_BF16, device=dev)
        a.dpred, a.d_rows, a.ld_drows = dpred.data_ptr(), d_rows.data_ptr(), d_rows.stride(0)
        lib = _mrec.lib()
        sizes = [w.numel() for w in ws] + [b.numel() for b in bs] + [wp.numel()]
        grads = _sum_partials("mrec_ncf_bwd", a, pairs, int(lib.mrec_ncf_parts(pairs)),
                              int(lib.mrec_ncf_param_count(E, nl, a.widths)), sizes,
                              params, dev)
        ctx.args = ctx.keep = None
        return (d_rows, None, None) + grads


def ncf_score(rows: torch.Tensor, model) -> torch.Tensor:
    """pred [pairs] (fp32) of ``model``'s NCF scorer (mlp, prediction, emb_size, dropout)
    over the gathered rows [pairs, 4E] = [mf_u | mf_i | mlp_u | mlp_i].  On a GPU the
    fused kernels when they cover the shape, the parameters are fp32 and no dropout is
    active; else, and on the CPU, the layered path: the same arithmetic as torch ops
    (``cpu_path.ncf_score``), rounding to bf16 on a GPU where the kernel does."""
    from pytorchrec_amd import cpu_path
    E = int(model.emb_size)
    ws, bs, wp = _ncf_params(model)
    drop = float(model.dropout)
    if (rows.is_cuda and NCF_FUSED and not (model.training and drop > 0)
            and ncf_supported(E, [w.shape[0] for w in ws])
            and all(p.dtype == torch.float32 for p in (*ws, *bs, wp))):
        return _NcfFn.apply(rows, E, len(ws), *ws, *bs, wp)
    return cpu_path.ncf_score(rows, E, ws, bs, wp,
                              rnd=cpu_path.bf16_round if rows.is_cuda else None,
                              dropout=drop, training=model.training)


# the fused DLRM dot interaction (mrec_dot_interact_*, dot_interact.hip) is the default for
# the compiled shapes; False selects the torch-ops path (the parity tests and the benchmark
# set it)
DOT_INTERACT = True

_DI_DTYPES = (torch.float32, _BF16)


def dot_interact_supported(D: int, n_fields: int, bot_dtype=torch.float32,
                           rows_dtype=torch.float32, x_dtype=torch.float32,
                           dx_dtype=torch.float32) -> bool:
    """True when the fused interaction covers (D, n_fields) and the four dtypes.  Decided
    from the shape alone; never an error."""
    dts = (bot_dtype, rows_dtype, x_dtype, dx_dtype)
    if any(t not in _DI_DTYPES for t in dts):
        return False
    return bool(_mrec.lib().mrec_dot_interact_supported(int(D), int(n_fields),
                                                        *[_mrec.dtype_code(t) for t in dts]))


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """[M, N] with unit inner stride and 16-byte aligned rows; copies only when it must."""
    es = t.element_size()
    if (t.stride(1) == 1 and t.stride(0) >= t.shape[1] and (t.stride(0) * es) % 16 == 0
            and t.data_ptr() % 16 == 0):
        return t
    out = _alloc(t.shape[0], t.shape[1], t.dtype, t.device)
    out.copy_(t)
    return out


class _DotInteractFn(torch.autograd.Function):
    """x = [bot | pairwise dots | 0 pad] of the gathered rows and the bottom vector: one
    forward launch, one backward launch (dbot in bot's dtype, drows in the rows'), nothing
    saved but the two inputs."""

    @staticmethod
    def forward(ctx, bot, rows, F_: int, D: int, x_cols: int, x_dtype):
        B, dev = rows.shape[0], rows.device
        rows2 = _rows16(rows.detach())
        bot2 = _rows16(bot.detach()) if bot is not None else None
        x = _alloc(B, x_cols, x_dtype, dev)
        a = _mrec.DotInteractArgs()
        if bot2 is not None:
            a.bot, a.bot_dtype, a.ld_bot = bot2.data_ptr(), _mrec.dtype_code(bot2.dtype), bot2.stride(0)
        a.rows, a.rows_dtype, a.ld_rows = rows2.data_ptr(), _mrec.dtype_code(rows2.dtype), rows2.stride(0)
        a.batch, a.n_fields, a.D = B, int(F_), int(D)
        a.x, a.x_dtype, a.ld_x, a.x_cols = x.data_ptr(), _mrec.dtype_code(x_dtype), x.stride(0), int(x_cols)
        if B:
            _mrec.call("mrec_dot_interact_fwd", ctypes.byref(a), _mrec.stream_handle())
        ctx.args, ctx.keep = a, (bot2, rows2)
        return x

    @staticmethod
    def backward(ctx, dx):
        a, (bot2, rows2) = ctx.args, ctx.keep
        B, F_, D = int(a.batch), int(a.n_fields), int(a.D)
        dev = rows2.device
        dx = dx.detach()
        if dx.dtype not in _DI_DTYPES:
            dx = dx.float()
        dx = _rows16(dx)
        dbot = _alloc(B, D, bot2.dtype, dev) if bot2 is not None else None
        drows = _alloc(B, F_ * D, rows2.dtype, dev)
        a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), _mrec.dtype_code(dx.dtype), dx.stride(0)
        if dbot is not None:
            a.dbot, a.ld_dbot = dbot.data_ptr(), dbot.stride(0)
        a.drows, a.ld_drows = drows.data_ptr(), drows.stride(0)
        if B:
            _mrec.call("mrec_dot_interact_bwd", ctypes.byref(a), _mrec.stream_handle())
        ctx.args = ctx.keep = None
        return dbot, drows, None, None, None, None


def dot_interact(bot: Optional[torch.Tensor], rows: torch.Tensor, n_fields: int,
                 x_cols: Optional[int] = None, x_dtype=None) -> torch.Tensor:
    """DLRM's pairwise dot interaction (include/mrec.h "DLRM dot interaction"): with t_0 =
    ``bot [B, D]`` (None: no bottom vector) and t_i the fields of ``rows [B, n_fields * D]``
    (``embedding.gather``'s layout), x ``[B, x_cols] = [t_0 | t_i . t_j, j < i | 0 pad]`` in
    ``x_dtype`` (default: the rows'), the pairs in ``torch.tril_indices`` order.  ``x_cols``
    defaults to D + P rounded up to 8, the row pitch ``tower_supported`` asks of x0.  On a GPU
    the fused kernels for the compiled shapes; else, and on the CPU, the same contract as
    torch ops (``cpu_path.dot_interact``), rounding the operands to bf16 on a GPU where the
    kernel does."""
    from pytorchrec_amd import cpu_path
    F_ = int(n_fields)
    if F_ < 1 or rows.dim() != 2 or rows.shape[1] % F_:
        raise ValueError(f"rows must be [B, n_fields * D], got {tuple(rows.shape)} for {F_} fields")
    D = rows.shape[1] // F_
    if bot is not None and (bot.dim() != 2 or bot.shape[0] != rows.shape[0] or bot.shape[1] != D):
        raise ValueError(f"bot must be [B, {D}], got {tuple(bot.shape)}")
    n = F_ + (bot is not None)
    width = (D if bot is not None else 0) + n * (n - 1) // 2
    if x_cols is None:
        x_cols = _r8(width)
    if x_cols < width:
        raise ValueError(f"x_cols = {x_cols} is smaller than D + P = {width}")
    x_dtype = x_dtype or rows.dtype
    if (rows.is_cuda and DOT_INTERACT
            and dot_interact_supported(D, F_, bot.dtype if bot is not None else torch.float32,
                                       rows.dtype, x_dtype)):
        return _DotInteractFn.apply(bot, rows, F_, D, int(x_cols), x_dtype)
    return cpu_path.dot_interact(bot, rows, F_, D, int(x_cols), round_bf16=rows.is_cuda,
                                 x_dtype=x_dtype)


# the fused CIN (mrec_cin_fwd / _bwd, cin.hip) is the default for the compiled shapes; False
# selects the torch-ops path (the parity tests and the benchmark set it)
CIN_FUSED = True


def cin_supported(m: int, D: int, widths: Sequence[int], x_dtype=torch.float32,
                  x0_dtype=None) -> bool:
    """True when the fused CIN covers m fields of D elements, the layer widths (at most 4
    layers) and the activation dtype.  Decided from the shape alone; never an error."""
    widths = [int(w) for w in widths]
    x0_dtype = x0_dtype or x_dtype
    if not 1 <= len(widths) <= 4 or x_dtype not in _DI_DTYPES or x0_dtype not in _DI_DTYPES:
        return False
    lib, hp = _mrec.lib(), int(m)
    for h in widths:
        if not lib.mrec_cin_supported(int(m), int(D), hp, h, _mrec.dtype_code(x0_dtype),
                                      _mrec.dtype_code(x_dtype)):
            return False
        hp = h
    return True


def cin_images(weight: torch.Tensor):
    """(forward, transposed) bf16 images of a CIN weight [H, H_prev, m] (include/mrec.h
    "CIN": the field pitch and the tile pads are zeros), cached like ``weight_images``."""
    c = cached_images(weight, "cin")
    if c is not None:
        return c
    W = weight.detach().float()
    H, Hp, m = W.shape
    lib = _mrec.lib()
    MP = int(lib.mrec_cin_field_pitch(m))
    wf = torch.zeros(int(lib.mrec_cin_fwd_rows(H)), Hp, MP, dtype=_BF16, device=W.device)
    wf[:H, :, :m] = W
    wb = torch.zeros((Hp * MP + 31) // 32 * 32, int(lib.mrec_cin_bwd_cols(H)), dtype=_BF16,
                     device=W.device)
    wb[:Hp * MP].view(Hp, MP, -1)[:, :m, :H] = W.permute(1, 2, 0)
    wf = wf.view(wf.shape[0], Hp * MP)
    weight._mrec_cimg = _img_state(weight) + (wf, wb)
    return wf, wb


class _CinFn(torch.autograd.Function):
    """p = the CIN's pooled maps of x0: one forward launch per layer, which writes X^k (kept
    for the backward) and its slice of p; one backward call per layer, top down, each a data
    gradient launch (dX^{k-1} and the fp32 dX^0 accumulator) and a weight gradient launch."""

    @staticmethod
    def forward(ctx, x0, m: int, D: int, x_dtype, *weights):
        B, dev = x0.shape[0], x0.device
        x0r = _rows16(x0.detach())
        widths = [w.shape[0] for w in weights]
        p = torch.empty(B, sum(widths), dtype=torch.float32, device=dev)
        st = _mrec.stream_handle()
        args, xs, keep = [], [], []
        xp, hp, off = x0r, m, 0
        for w in weights:
            H = w.shape[0]
            wf, wb = cin_images(w)
            xk = _alloc(B, H * D, x_dtype, dev)
            a = _mrec.CinArgs()
            a.x0, a.x0_dtype, a.ld_x0 = x0r.data_ptr(), _mrec.dtype_code(x0r.dtype), x0r.stride(0)
            a.xp, a.xp_dtype, a.ld_xp = xp.data_ptr(), _mrec.dtype_code(xp.dtype), xp.stride(0)
            a.w_fwd, a.ld_w_fwd, a.w_bwd, a.ld_w_bwd = wf.data_ptr(), wf.stride(0), wb.data_ptr(), wb.stride(0)
            a.batch, a.n_fields, a.D, a.H_prev, a.H = B, int(m), int(D), int(hp), int(H)
            a.x_dtype = _mrec.dtype_code(x_dtype)
            a.xk, a.ld_xk = xk.data_ptr(), xk.stride(0)
            a.p, a.ld_p = p.data_ptr() + 4 * off, p.stride(0)
            if B:
                _mrec.call("mrec_cin_fwd", ctypes.byref(a), st)
            args.append(a)
            xs.append(xk)
            keep.append((wf, wb))
            xp, hp, off = xk, H, off + H
        ctx.args, ctx.keep, ctx.weights = args, (x0r, xs, keep), weights
        ctx.x0_dtype = x0.dtype
        return p

    @staticmethod
    def backward(ctx, dp):
        args, (x0r, xs, keep), weights = ctx.args, ctx.keep, ctx.weights
        B, dev = x0r.shape[0], x0r.device
        m, D = int(args[0].n_fields), int(args[0].D)
        dp = dp.detach().float().contiguous()
        dx0 = torch.zeros(B, m * D, dtype=torch.float32, device=dev)
        st = _mrec.stream_handle()
        offs = [0]
        for w in weights:
            offs.append(offs[-1] + w.shape[0])
        dws, dxk = [None] * len(weights), None
        for k in range(len(weights) - 1, -1, -1):
            a = args[k]
            H, Hp = int(a.H), int(a.H_prev)
            if dxk is not None:
                a.dxk, a.ld_dxk = dxk.data_ptr(), dxk.stride(0)
            a.dp, a.ld_dp = dp.data_ptr() + 4 * offs[k], dp.stride(0)
            if k > 0:
                a.dp_prev, a.ld_dp_prev = dp.data_ptr() + 4 * offs[k - 1], dp.stride(0)
            dxp = _alloc(B, Hp * D, xs[k - 1].dtype if k > 0 else torch.float32, dev)
            a.dxp, a.dxp_dtype, a.ld_dxp = dxp.data_ptr(), _mrec.dtype_code(dxp.dtype), dxp.stride(0)
            a.dx0, a.ld_dx0 = dx0.data_ptr(), dx0.stride(0)
            dw = torch.empty(H, Hp, m, dtype=torch.float32, device=dev)
            a.dw = dw.data_ptr()
            if B:
                _mrec.call("mrec_cin_bwd", ctypes.byref(a), st)
            else:
                dw.zero_()
            dws[k], dxk = dw, dxp
        if B:
            dx0 += dxk  # layer 1: X^0 is also the X^{k-1} operand
        ctx.args = ctx.keep = ctx.weights = None
        return (dx0.to(ctx.x0_dtype), None, None, None,
                *[g.to(w.dtype) for g, w in zip(dws, weights)])


def cin(x0: torch.Tensor, n_fields: int, weights, x_dtype=None) -> torch.Tensor:
    """xDeepFM's Compressed Interaction Network (include/mrec.h "CIN"): ``x0 [B, n_fields * D]``
    read as [B, m, D] (a column slice of the interact launch's x0 rows is fine),
    ``weights[k - 1]`` = W^k [H_k, H_{k-1}, m] with H_0 = m ->  p ``[B, sum_k H_k]`` fp32, the
    maps X^k summed over d.  X^k is kept in ``x_dtype`` (default: x0's).  On a GPU the fused
    kernels for the compiled shapes; else, and on the CPU, the same contract as torch ops
    chunked over the batch (``cpu_path.cin``), rounding on a GPU where the kernels round."""
    from pytorchrec_amd import cpu_path
    weights = list(weights)
    m = int(n_fields)
    if m < 1 or x0.dim() != 2 or x0.shape[1] % m:
        raise ValueError(f"x0 must be [B, n_fields * D], got {tuple(x0.shape)} for {m} fields")
    if not weights or weights[0].shape[2] != m:
        raise ValueError(f"CIN weights must be [H_k, H_(k-1), {m}], one per layer")
    D = x0.shape[1] // m
    x_dtype = x_dtype or x0.dtype
    if (x0.is_cuda and CIN_FUSED and all(w.dim() == 3 for w in weights)
            and cin_supported(m, D, [w.shape[0] for w in weights], x_dtype, x0.dtype)
            and all(w.shape[1] == h and w.shape[2] == m
                    for w, h in zip(weights, [m] + [w.shape[0] for w in weights[:-1]]))):
        return _CinFn.apply(x0, m, D, x_dtype, *weights)
    return cpu_path.cin(x0, weights, round_bf16=x0.is_cuda, x_dtype=x_dtype)


# the fused AutoInt interacting layers (mrec_autoint_fwd / _bwd, autoint.hip) are the default
# for the compiled shapes; False selects the torch-ops path (the parity tests and the
# benchmark set it)
AUTOINT_FUSED = True


def _autoint_dims(m: int, d_in: int, layers, heads: int):
    """[(d_in_k, A_k, head_dim_k)] of well-formed layers, else None."""
    dims, d = [], int(d_in)
    for l in layers:
        if len(l) != 4 or any(w is not None and (w.dim() != 2 or tuple(w.shape) != (l[0].shape[0], d))
                              for w in l) or any(w is None for w in l[:3]):
            return None
        A = l[0].shape[0]
        if heads < 1 or A % heads:
            return None
        dims.append((d, A, A // heads))
        d = A
    return dims


def autoint_supported(m: int, d_in: int, widths: Sequence[int], heads: int,
                      x_dtype=torch.float32, x0_dtype=None) -> bool:
    """True when the fused interacting layers cover m fields of d_in elements, the layer widths
    A_k = heads * head_dim_k (at most 4 layers) and the activation dtypes.  Decided from the
    shape alone; never an error."""
    widths = [int(w) for w in widths]
    x0_dtype = x0_dtype or x_dtype
    heads = int(heads)
    if (not 1 <= len(widths) <= 4 or heads < 1 or x_dtype not in _DI_DTYPES
            or x0_dtype not in _DI_DTYPES or any(w < 1 or w % heads for w in widths)):
        return False
    lib, d, xd = _mrec.lib(), int(d_in), x0_dtype
    for A in widths:
        if not lib.mrec_autoint_supported(int(m), d, heads, A // heads, _mrec.dtype_code(xd),
                                          _mrec.dtype_code(x_dtype)):
            return False
        d, xd = A, x_dtype
    return True


def autoint_images(Wq, Wk, Wv, Wres):
    """(forward, transposed) bf16 images of one interacting layer (include/mrec.h "AutoInt":
    rows [Wres | Wq | Wk | Wv], zeros without Wres), cached on Wq like ``weight_images`` and
    valid while none of the four weights changed."""
    others = tuple((id(w), _img_state(w)) for w in (Wk, Wv, Wres) if w is not None)
    c = cached_images(Wq, "autoint")
    if c is not None and Wq._mrec_aimg[4] == others:
        return c
    A, d = Wq.shape
    rows = int(_mrec.lib().mrec_autoint_image_rows(A))
    wf = torch.zeros(rows, d, dtype=_BF16, device=Wq.device)
    for k, w in ((1, Wq), (2, Wk), (3, Wv), (0, Wres)):
        if w is not None:
            wf[k * A:(k + 1) * A] = w.detach()
    wb = wf.t().contiguous()
    Wq._mrec_aimg = _img_state(Wq) + (wf, wb, others)
    return wf, wb


class _AutoIntFn(torch.autograd.Function):
    """The interacting stack: one forward launch per layer bottom up, each writing the
    layer's Y (kept: it is the next layer's input and the backward's ReLU mask); one backward
    call per layer top down (dx, then dw through the caller's workspace)."""

    @staticmethod
    def forward(ctx, x0, m: int, heads: int, scale: float, x_dtype, has_res, *flat):
        B, dev = x0.shape[0], x0.device
        xs = [_rows16(x0.detach())]
        st = _mrec.stream_handle()
        args, keep, it = [], [], iter(flat)
        for res in has_res:
            Wq, Wk, Wv = next(it), next(it), next(it)
            Wres = next(it) if res else None
            A, d = Wq.shape
            wf, wb = autoint_images(Wq, Wk, Wv, Wres)
            x = xs[-1]
            y = _alloc(B, m * A, x_dtype, dev)
            a = _mrec.AutoIntArgs()
            a.x, a.x_dtype, a.ld_x = x.data_ptr(), _mrec.dtype_code(x.dtype), x.stride(0)
            a.w_fwd, a.ld_w_fwd, a.w_bwd, a.ld_w_bwd = wf.data_ptr(), wf.stride(0), wb.data_ptr(), wb.stride(0)
            a.has_res, a.batch, a.n_fields, a.d_in = int(res), B, int(m), int(d)
            a.heads, a.head_dim, a.A, a.scale = int(heads), int(A // heads), int(A), float(scale)
            a.y, a.y_dtype, a.ld_y = y.data_ptr(), _mrec.dtype_code(y.dtype), y.stride(0)
            if B:
                _mrec.call("mrec_autoint_fwd", ctypes.byref(a), st)
            args.append(a)
            keep.append((wf, wb))
            xs.append(y)
        ctx.args, ctx.keep, ctx.flat, ctx.has_res = args, (xs, keep), flat, has_res
        ctx.x0_dtype = x0.dtype
        return xs[-1]

    @staticmethod
    def backward(ctx, dy):
        args, (xs, keep), flat, has_res = ctx.args, ctx.keep, ctx.flat, ctx.has_res
        B, dev = xs[0].shape[0], xs[0].device
        lib, st = _mrec.lib(), _mrec.stream_handle()
        dy = dy.detach()
        if dy.dtype not in _DI_DTYPES:
            dy = dy.float()
        dy = _rows16(dy)
        ws_bytes = max([int(lib.mrec_autoint_bwd_workspace_size(B, int(a.d_in), int(a.A))) for a in args] + [16])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        dws = [None] * len(args)
        for k in range(len(args) - 1, -1, -1):
            a = args[k]
            dx = _alloc(B, int(a.n_fields) * int(a.d_in), xs[k].dtype, dev)
            dw = torch.empty(4 if has_res[k] else 3, int(a.A), int(a.d_in), dtype=torch.float32, device=dev)
            a.dy, a.dy_dtype, a.ld_dy = dy.data_ptr(), _mrec.dtype_code(dy.dtype), dy.stride(0)
            a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), _mrec.dtype_code(dx.dtype), dx.stride(0)
            a.dw, a.workspace, a.workspace_bytes = dw.data_ptr(), ws.data_ptr(), ws_bytes
            if B:
                _mrec.call("mrec_autoint_bwd", ctypes.byref(a), st)
            else:
                dw.zero_()
            dws[k], dy = dw, dx
        grads = []
        it = iter(flat)
        for k, res in enumerate(has_res):
            for j in range(4 if res else 3):
                grads.append(dws[k][j].to(next(it).dtype))
        ctx.args = ctx.keep = ctx.flat = None
        return (dy.to(ctx.x0_dtype), None, None, None, None, None, *grads)


def autoint(x0: torch.Tensor, n_fields: int, layers, heads: int, scale: float = 1.0,
            x_dtype=None) -> torch.Tensor:
    """AutoInt's interacting stack (include/mrec.h "AutoInt"): ``x0 [B, n_fields * d_in]`` read
    as [B, m, d_in] (a column slice of the interact launch's x0 rows is fine), ``layers`` a
    sequence of ``(Wq, Wk, Wv, Wres or None)`` in nn.Linear layout -> ``[B, m * A_last]``, every
    layer multi-head self-attention over the fields, a residual projection and a ReLU.  The
    layers' outputs are kept in ``x_dtype`` (default: x0's).  On a GPU the fused kernels for the
    compiled shapes; else, and on the CPU, the same contract as torch ops chunked over the batch
    (``cpu_path.autoint``), rounding on a GPU where the kernels round."""
    from pytorchrec_amd import cpu_path
    layers = [tuple(l) for l in layers]
    m, heads = int(n_fields), int(heads)
    if m < 1 or x0.dim() != 2 or x0.shape[1] % m:
        raise ValueError(f"x0 must be [B, n_fields * d_in], got {tuple(x0.shape)} for {m} fields")
    if not layers:
        raise ValueError("autoint needs at least one layer (Wq, Wk, Wv, Wres or None)")
    d_in = x0.shape[1] // m
    x_dtype = x_dtype or x0.dtype
    if x0.is_cuda and AUTOINT_FUSED:
        dims = _autoint_dims(m, d_in, layers, heads)
        if dims is not None and autoint_supported(m, d_in, [A for _, A, _ in dims], heads, x_dtype,
                                                  x0.dtype):
            has_res = tuple(l[3] is not None for l in layers)
            flat = [w for l in layers for w in l if w is not None]
            return _AutoIntFn.apply(x0, m, heads, float(scale), x_dtype, has_res, *flat)
    return cpu_path.autoint(x0, layers, heads, scale, round_bf16=x0.is_cuda, x_dtype=x_dtype)


def colsum(s: torch.Tensor, X: Optional[torch.Tensor], want_total: bool = True, *,
           out: Optional[torch.Tensor] = None, total: Optional[torch.Tensor] = None,
           sgd_lr: Optional[float] = None):
    """(sum_b s[b] X[b, :], sum_b s[b]) with libmrec's deterministic column sum.
    With ``sgd_lr`` the sums are applied in place as SGD to ``out`` / ``total``
    (parameters) instead: p -= lr * sum."""
    s = s.contiguous().float()
    C = 0 if X is None else X.shape[1]
    dev = s.device
    if out is None and C:
        out = torch.empty(C, dtype=torch.float32, device=dev)
    if total is None and want_total:
        total = torch.empty(1, dtype=torch.float32, device=dev)
    if X is not None and X.stride(1) != 1:
        X = X.contiguous()
    _mrec.call("mrec_colsum", s.data_ptr(), _mrec.ptr(X),
               _mrec.dtype_code(X.dtype) if X is not None else _mrec.F32,
               X.stride(0) if X is not None else 0, s.shape[0], C, _mrec.ptr(out),
               _mrec.ptr(total) if want_total else None, int(sgd_lr is not None),
               float(sgd_lr or 0.0), _mrec.stream_handle())
    return out, (total if want_total else None)


class _HeadFn(torch.autograd.Function):
    """z = base + h W^T + b for a Linear(H, 1) output layer (fp32 z [B])."""

    @staticmethod
    def forward(ctx, h, weight, bias, base, h_relu: bool):
        h = _bf16_rows(h)
        B, H = h.shape
        w = _weight_f32(weight).reshape(-1)
        b = bias.detach().float() if bias is not None else None
        base_c = base.detach().float().contiguous() if base is not None else None
        z = torch.empty(B, dtype=torch.float32, device=h.device)
        _mrec.call("mrec_head_fwd", h.data_ptr(), h.stride(0), B, H, w.data_ptr(), _mrec.ptr(b),
                   _mrec.ptr(base_c), z.data_ptr(), _mrec.stream_handle())
        ctx.save_for_backward(h, w)
        ctx.has_bias, ctx.has_base, ctx.h_relu = bias is not None, base is not None, h_relu
        ctx.weight, ctx.bias = weight, bias
        return z

    @staticmethod
    def backward(ctx, dz):
        h, w = ctx.saved_tensors
        B, H = h.shape
        dz = dz.contiguous().float()
        dh = None
        if ctx.needs_input_grad[0]:
            dh = _alloc(B, H, _BF16, dz.device)
            _mrec.call("mrec_head_bwd", dz.data_ptr(), w.data_ptr(), B, H,
                       h.data_ptr() if ctx.h_relu else None, h.stride(0), dh.data_ptr(),
                       dh.stride(0), _mrec.stream_handle())
            if ctx.h_relu:
                _stamp(dh, h)
        lr = sgd_lr(ctx.weight, ctx.bias)
        if lr is not None and ctx.weight.is_contiguous():
            colsum(dz, h, want_total=ctx.has_bias, out=ctx.weight.detach().view(-1),
                   total=ctx.bias.detach() if ctx.has_bias else None, sgd_lr=lr)
            dW = db = None
        else:
            dW, db = colsum(dz, h, want_total=ctx.has_bias)
            dW = dW.reshape(1, H)
        return dh, dW, db, (dz if ctx.has_base else None), None


def head(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
         base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Logit of a Linear(H, 1) output layer plus an optional per-sample base logit
    (the FM / wide part): z = base + h W^T + b, fp32 [B]."""
    if not h.is_cuda:
        z = F.linear(h.float(), weight.float(), None if bias is None else bias.float()).reshape(-1)
        return z if base is None else z + base.float()
    return _HeadFn.apply(h, weight, bias, base, _is_relu_out(h))


# ----------------------------------------------------------------------------
# fused CTR head + BCE loss (the train step's last layer and its loss)
# ----------------------------------------------------------------------------

_TICKETS = {}
_ONES = {}


def _ticket(dev) -> torch.Tensor:
    t = _TICKETS.get(dev)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=dev)  # zero once; kernels leave it zero
        _TICKETS[dev] = t
    return t


def grad_one(dev) -> torch.Tensor:
    """Persistent scalar 1.0 used as the loss gradient (no fill kernel per step, and
    lets the fused head skip scaling its stashed gradients)."""
    t = _ONES.get(dev)
    if t is None:
        t = torch.ones((), dtype=torch.float32, device=dev)
        _ONES[dev] = t
    return t


def _head_param_grads(part, B: int, H: int, ns: int, g, one: bool, head):
    """The gradients of a CTR head's (w, b, ws, b2) from the partials ``part`` of the
    kernel that ran its forward (fixed-order sums), scaled by the loss gradient ``g``
    (``one``: g is ``grad_one``, no scaling) -> (dW, db, dws, db2) for autograd.
    Fused SGD and the data-parallel flat buffer defer the finish: it is independent
    of the backward GEMMs and rides along the next launch (all None is returned);
    returned gradients are finished now."""
    w, b, ws, b2 = head
    lr, views = _decide(head)
    gs = None if one else g
    if lr is not None and w.is_contiguous():
        defer_head_finish(_HeadFinish(part, B, H, ns, gs, lr=lr, params=[
            None if t is None else t.detach() for t in head]))
        return None, None, None, None
    if views is not None:
        defer_head_finish(_HeadFinish(part, B, H, ns, gs, grads=views))
        return None, None, None, None
    f32 = dict(dtype=torch.float32, device=part.device)
    dW = torch.empty(1, H, **f32)
    db = torch.empty(1, **f32) if b is not None else None
    dws = torch.empty(ns, **f32) if ws is not None else None
    db2 = torch.empty(1, **f32) if b2 is not None else None
    _HeadFinish(part, B, H, ns, g, grads=[dW, db, dws, db2]).run()
    return dW, db, dws, db2


class _CTRHeadBCEFn(torch.autograd.Function):
    """loss = BCEWithLogits(base + h W^T + b [+ xs ws + b2], y) (mean) for a
    Linear(H, 1) head (+ an optional side linear term: DeepFM's dense first-order
    weight and global bias).  The forward kernel also produces dh, dz and the
    parameter-gradient partials; the backward only reduces the partials
    (``_head_param_grads``)."""

    @staticmethod
    def forward(ctx, h, weight, bias, base, ws, b2, y, xs, h_relu: bool):
        h = _bf16_rows(h)
        B, H = h.shape
        dev = h.device
        w = _weight_f32(weight).reshape(-1)
        b = bias.detach().float() if bias is not None else None
        base_c = base.detach().float().contiguous() if base is not None else None
        y = y.detach().float().contiguous()
        ns = 0
        if xs is not None:
            xs = xs.detach().float()
            if xs.stride(1) != 1:
                xs = xs.contiguous()
            ns = xs.shape[1]
        wsd = ws.detach().float().contiguous() if ws is not None else None
        b2d = b2.detach().float() if b2 is not None else None
        z = torch.empty(B, dtype=torch.float32, device=dev)
        dz = torch.empty(B, dtype=torch.float32, device=dev)
        dh = _alloc(B, H, _BF16, dev)
        nparts = int(_mrec.lib().mrec_ctr_head_parts(B))
        ldp = _r8(H + 1 + ns)
        part = torch.empty(nparts, ldp, dtype=torch.float32, device=dev)
        loss_part = torch.empty(nparts, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _mrec.call("mrec_ctr_head_fwd", h.data_ptr(), h.stride(0), B, H, w.data_ptr(),
                   _mrec.ptr(b), _mrec.ptr(base_c), y.data_ptr(), _mrec.ptr(xs),
                   xs.stride(0) if xs is not None else 0, ns, _mrec.ptr(wsd), _mrec.ptr(b2d),
                   int(bool(h_relu)), z.data_ptr(), dz.data_ptr(), dh.data_ptr(), dh.stride(0),
                   part.data_ptr(), ldp, loss_part.data_ptr(), _ticket(dev).data_ptr(),
                   loss.data_ptr(), _mrec.stream_handle())
        if h_relu:
            _stamp(dh, h)
        ctx.save_for_backward(part, dz, dh)
        ctx.weight, ctx.bias, ctx.ws, ctx.b2 = weight, bias, ws, b2
        ctx.H, ctx.B, ctx.ns, ctx.has_base = H, B, ns, base is not None
        ctx.mark_non_differentiable(z)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for z
        return loss.reshape(()), z

    @staticmethod
    def backward(ctx, gloss, gz=None):
        part, dz, dh = ctx.saved_tensors
        dev = part.device
        g = gloss.detach().float().reshape(1).contiguous()
        one = g.data_ptr() == grad_one(dev).data_ptr()
        dW, db, dws, db2 = _head_param_grads(part, ctx.B, ctx.H, ctx.ns, g, one,
                                             (ctx.weight, ctx.bias, ctx.ws, ctx.b2))
        if not one:
            dh = (dh.float() * g).to(_BF16)
            dz = dz * g
        return dh, dW, db, (dz if ctx.has_base else None), dws, db2, None, None, None


def ctr_head_bce(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                 base: Optional[torch.Tensor], y: torch.Tensor, xs: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None):
    """(loss, z): mean BCE-with-logits of z = base + h W^T + b (+ xs ws + b2) against
    y — the CTR models' output layer and loss in one kernel (GPU, training) — else
    the plain ``head`` + torch loss."""
    ns = 0 if xs is None else xs.shape[1]
    if h.is_cuda and torch.is_grad_enabled() and h.shape[1] <= 1024 and ns <= 64:
        return _CTRHeadBCEFn.apply(h, weight, bias, base, ws, b2, y, xs, _is_relu_out(h))
    z = head(h, weight, bias, base)
    if xs is not None:
        z = z + xs.float() @ ws.float()
    if b2 is not None:
        z = z + b2.float()
    return F.binary_cross_entropy_with_logits(z.float(), y.float()), z


# ----------------------------------------------------------------------------
# fused MLP tower + CTR head + BCE (mrec_tower_fwd_bwd)
# ----------------------------------------------------------------------------

TOWER = True  # False: the layered kernels (the parity tests set it)
TOWER_MAXL, TOWER_MAXW = 4, 512
# DCN-v2 cross layers inside the tower launch (more: the layered cross network of
# _CrossNetFn ahead of the tower)
TOWER_MAXC = 3


def _mlp_linears(mlp) -> list:
    return [m.linear for m in mlp.mlp] if hasattr(mlp, "mlp") else list(mlp)


def tower_supported(x0: torch.Tensor, mlp, head: torch.nn.Linear, xs=None, cross=None) -> bool:
    """The fused tower covers the reference MLP (Linear -> ReLU per layer,
    Dense.py:4-24) with dropout 0 (or eval) + Linear(N_L, 1) + BCE on the GPU, and
    up to 3 DCN-v2 cross layers (``nn.Linear(d, d)``, d = the MLP's input width)
    ahead of it when the batch takes mrec_tower_dw."""
    dense_layers = list(mlp.mlp) if hasattr(mlp, "mlp") else []
    lins = [d.linear for d in dense_layers]
    widths = [lins[0].in_features] + [l.out_features for l in lins] if lins else []
    if cross:
        if not lins or len(cross) > TOWER_MAXC:
            return False
        d = widths[0]
        if any(c.in_features != d or c.out_features != d or c.weight.dtype != torch.float32
               or not c.weight.is_contiguous() for c in cross):
            return False
        if not _tdw_splits(x0.shape[0], [d] * len(cross) + widths):
            return False
    if not (TOWER and x0.is_cuda and torch.is_grad_enabled() and x0.dtype == _BF16):
        return False
    if not dense_layers or len(dense_layers) > TOWER_MAXL:
        return False
    if any(d.dropout.p > 0 and d.training for d in dense_layers):
        return False
    if any(w > TOWER_MAXW for w in widths) or head.out_features != 1:
        return False
    if any(l.weight.dtype != torch.float32 or not l.weight.is_contiguous() for l in lins):
        return False
    if xs is not None and xs.shape[1] > 64:
        return False
    return (x0.shape[1] >= widths[0] and x0.stride(1) == 1 and x0.stride(0) % 8 == 0
            and x0.data_ptr() % 16 == 0)


def _eff_split(K: int, s: int) -> int:
    """mrec_gemm's split-K count for K and a requested s (plan_split in gemm.hip)."""
    k = max(((K + s - 1) // s + 63) // 64 * 64, 64)
    return (K + k - 1) // k if K > 0 else 1


def _tdw_tiles(widths) -> int:
    """64 x 64 output tiles of the tower's dW_l = dY_l^T [X_l | 1]."""
    return sum(((widths[l + 1] + 63) // 64) * ((widths[l] + 1 + 63) // 64)
               for l in range(len(widths) - 1))


def _tdw_splits(B: int, widths=None) -> int:
    """K slices of mrec_tower_dw (0: not used): about 640 one-wave workgroups (2.5
    per CU) over the tiles, slices of >= 256 rows, at most 64 and at most B / 1024
    (but 4 allowed): the REDUCE that follows reads every slice's slab, and for a small
    tower it is the longer part.  4 for the C2 tower (147 tiles; 8 slices ran no
    faster and double the slabs the reduction reads) and for DIN's top tower (16
    tiles: 16 slices 0.2256-0.2258 ms/step, 8: 0.2245-0.2252, 4: 0.2233-0.2240), 64
    for DIN's layered attention unit (8 tiles over 204,800 rows)."""
    if B < 256:
        return 0
    # at least 4 (C3's 245 tiles: 2 slices 0.1243 ms/step, 4: 0.1194; 3 and 5 slower)
    want = (4 if widths is None else
            max(4, min(64, 640 // _tdw_tiles(widths), max(4, B // 1024))))
    for s in range(want, 1, -1):
        if B // s >= 256 and _eff_split(B, s) == s:
            return s
    return 0


def _split_tower(widths, K: int) -> int:
    """K slices of the tower's weight-gradient GEMMs (generic mrec_gemm_multi path,
    dW_l [N_l, K_l + 1] over the batch), which share one launch: about two residency
    waves of 256-thread workgroups (3 per CU), slices of >= 256 rows."""
    tiles = _tdw_tiles(widths)
    s = 1
    while tiles * (s + 1) <= 640 and K // (s + 1) >= 256 and s < 64:
        s += 1
    return s


class _TowerBufs(NamedTuple):
    """What a tower launch with a backward half writes: the activations h_l (all but
    the last), the pre-activation gradients dh_l, the cross layers' x_c / dz_c and
    x0's image (k-fragment images only), and dx0 (None when not needed)."""
    hs: list
    dhs: list
    x0_img: Optional[torch.Tensor]
    cx_imgs: list
    cdz_imgs: list
    dx0: Optional[torch.Tensor]


def _tower_buffers(x0, widths, tdw: int, need_dx0: bool, C: int = 0) -> _TowerBufs:
    """The weight gradients' operands are k-fragment images for mrec_tower_dw
    (``tdw``: the tower writes them, x0's and the C cross layers' too), else
    row-major ``_alloc`` rows for the generic GEMM."""
    B, dev = x0.shape[0], x0.device
    L = len(widths) - 1
    if tdw:
        def buf(n):
            return torch.empty(int(_mrec.lib().mrec_kfrag_elems(B, n)), dtype=_BF16, device=dev)
    else:
        def buf(n):
            return _alloc(B, n, _BF16, dev)
    hs = [buf(widths[l + 1]) for l in range(L - 1)]
    dhs = [buf(widths[l + 1]) for l in range(L)]
    x0_img = buf(widths[0]) if tdw else None
    cx_imgs = [buf(widths[0]) for _ in range(C if tdw else 0)]
    cdz_imgs = [buf(widths[0]) for _ in range(C if tdw else 0)]
    dx0 = None
    if need_dx0:  # x0's shape: it may carry pad columns past K0, which get a zero gradient
        Kx = x0.shape[1]
        dx0 = (_alloc(B, Kx, _BF16, dev) if _r8(Kx) == _r8(widths[0]) else
               torch.zeros(B, _r8(Kx), dtype=_BF16, device=dev)[:, :Kx])
    return _TowerBufs(hs, dhs, x0_img, cx_imgs, cdz_imgs, dx0)


def _tower_args(x0, widths, imgs, bsd, hw, hb, bufs: Optional[_TowerBufs] = None, part=None):
    """mrec_tower_args: the MLP and its head, plus (``bufs``, ``part``) the outputs of a
    launch with a backward half.  The mode and what only one mode takes (labels,
    side term, loss, cross layers; scores; dz_in) are the caller's to fill."""
    a = _mrec.TowerArgs()
    L = len(widths) - 1
    a.batch, a.n_layers = x0.shape[0], L
    for l in range(L + 1):
        a.width[l] = widths[l]
    a.x0, a.ld_x0 = x0.data_ptr(), x0.stride(0)
    for l in range(L):
        a.w_fwd[l], a.w_bwd[l] = imgs[l][0].data_ptr(), imgs[l][1].data_ptr()
        a.bias[l] = _mrec.ptr(bsd[l])
    a.head_w, a.head_b = hw.data_ptr(), _mrec.ptr(hb)
    if bufs is not None:
        for l in range(L):
            a.dh_out[l], a.ld_dh[l] = bufs.dhs[l].data_ptr(), bufs.dhs[l].stride(0)
            if l < L - 1:
                a.h_out[l], a.ld_h[l] = bufs.hs[l].data_ptr(), bufs.hs[l].stride(0)
        a.kfrag, a.x0_img = int(bufs.x0_img is not None), _mrec.ptr(bufs.x0_img)
        a.dx0 = _mrec.ptr(bufs.dx0)
        a.ld_dx0 = bufs.dx0.stride(0) if bufs.dx0 is not None else 0
        a.part, a.ldp = part.data_ptr(), part.stride(0)
    return a


class _TowerBCEFn(torch.autograd.Function):
    """loss = BCEWithLogits(MLP(x0) . w + b + base [+ xs . ws + b2], y) (mean).
    Forward = ONE mrec_tower_fwd_bwd launch, which also produces every input /
    pre-activation gradient (dx0, dz, dh_l); backward = the weight-gradient GEMMs
    (``_tower_param_grads``: one launch with the head finish)."""

    @staticmethod
    def forward(ctx, x0, base, xs, y, n_layers, n_cross, *params):
        L, C = n_layers, n_cross
        Ws, bs = params[:L], params[L:2 * L]
        head_w, head_b, ws, b2 = params[2 * L:2 * L + 4]
        cWs, cbs = params[2 * L + 4:2 * L + 4 + C], params[2 * L + 4 + C:2 * L + 4 + 2 * C]
        B = x0.shape[0]
        dev = x0.device
        widths = [Ws[0].shape[1]] + [W.shape[0] for W in Ws]
        imgs = [tower_images(W) for W in Ws]
        cimgs = [tower_images(W) for W in cWs]
        need_w = any(ctx.needs_input_grad[6:6 + 2 * L]) or any(
            ctx.needs_input_grad[6 + 2 * L + 4:6 + 2 * L + 4 + 2 * C])
        tdw = _tdw_splits(B, [widths[0]] * C + widths) if need_w else 0
        if C and need_w and not tdw:
            raise ValueError("cross layers in the tower need mrec_tower_dw (tower_supported)")
        bufs = _tower_buffers(x0, widths, tdw, ctx.needs_input_grad[0], C)
        dz = torch.empty(B, dtype=torch.float32, device=dev)
        ns = 0 if xs is None else xs.shape[1]
        if xs is not None:
            xs = xs.detach().float()
            if xs.stride(1) != 1:
                xs = xs.contiguous()
        H = widths[L]
        nparts = int(_mrec.lib().mrec_ctr_head_parts(B))
        ldp = _r8(H + 1 + ns)
        part = torch.empty(nparts, ldp, dtype=torch.float32, device=dev)
        loss_part = torch.empty(nparts, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        hw, hb, wsd, b2d = _f32c(head_w).reshape(-1), _f32c(head_b), _f32c(ws), _f32c(b2)
        bsd, cbsd = [_f32c(b) for b in bs], [_f32c(b) for b in cbs]
        base_c, yc = _f32c(base), _f32c(y)
        a = _tower_args(x0, widths, imgs, bsd, hw, hb, bufs, part)
        a.n_cross = C
        for c in range(C):
            a.cross_w_fwd[c], a.cross_w_bwd[c] = cimgs[c][0].data_ptr(), cimgs[c][1].data_ptr()
            a.cross_bias[c] = _mrec.ptr(cbsd[c])
            if tdw:
                a.cross_x_img[c] = bufs.cx_imgs[c].data_ptr()
                a.cross_dz_img[c] = bufs.cdz_imgs[c].data_ptr()
        a.base = _mrec.ptr(base_c)
        a.xs, a.ld_xs, a.ns = _mrec.ptr(xs), xs.stride(0) if xs is not None else 0, ns
        a.ws, a.b2, a.y = _mrec.ptr(wsd), _mrec.ptr(b2d), yc.data_ptr()
        a.z, a.dz = None, dz.data_ptr()
        a.loss_part, a.ticket, a.loss = loss_part.data_ptr(), _ticket(dev).data_ptr(), loss.data_ptr()
        _mrec.call("mrec_tower_fwd_bwd", ctypes.byref(a), _mrec.stream_handle())
        ctx.save_for_backward(x0 if bufs.x0_img is None else bufs.x0_img, dz, part, bufs.dx0,
                              *bufs.hs, *bufs.dhs, *bufs.cx_imgs, *bufs.cdz_imgs)
        ctx.L, ctx.C, ctx.B, ctx.ns, ctx.widths = L, C, B, ns, widths
        ctx.tdw, ctx.need_w = tdw, need_w
        ctx.Ws, ctx.bs, ctx.imgs = Ws, bs, imgs
        ctx.cWs, ctx.cbs, ctx.cimgs = cWs, cbs, cimgs
        ctx.head = (head_w, head_b, ws, b2)
        ctx.has_base = base is not None
        ctx.mark_non_differentiable(dz)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        L, C, B = ctx.L, ctx.C, ctx.B
        saved = ctx.saved_tensors
        x0, dz, part, dx0 = saved[:4]
        hs, dhs = list(saved[4:4 + L - 1]), list(saved[4 + L - 1:4 + 2 * L - 1])
        cx_imgs = list(saved[4 + 2 * L - 1:4 + 2 * L - 1 + C]) if ctx.tdw else []
        cdz_imgs = list(saved[4 + 2 * L - 1 + C:]) if ctx.tdw else []
        dev = part.device
        g = gloss.detach().float().reshape(1).contiguous()
        one = g.data_ptr() == grad_one(dev).data_ptr()
        tdw = ctx.tdw
        if not one:  # a scaled loss: every stashed gradient scales with it
            dz = dz * g
            dx0 = (dx0.float() * g).to(_BF16) if dx0 is not None else None
            dhs = [(d.float() * g).to(_BF16) if tdw else _bf16_rows((d.float() * g).to(_BF16))
                   for d in dhs]
            cdz_imgs = [(d.float() * g).to(_BF16) for d in cdz_imgs]
        # cross layer c: dW = dz_c^T [x_c | 1] from the images x_0 .. x_{C-1} (tdw only);
        # the MLP's first X is x_C
        xc = [x0] + cx_imgs
        lay = [(ctx.cWs[c], ctx.cbs[c], ctx.cimgs[c], cdz_imgs[c] if tdw else None,
                xc[c] if tdw else None) for c in range(C)]
        xin = [xc[C] if tdw else x0[:, :ctx.widths[0]]] + hs
        lay += list(zip(ctx.Ws, ctx.bs, ctx.imgs, dhs, xin))
        dWs, dbs, head_grads = _tower_param_grads(lay, ctx.head, part, B, ctx.ns, g, one, tdw,
                                                  ctx.need_w)
        return (dx0, dz if ctx.has_base else None, None, None, None, None, *dWs[C:], *dbs[C:],
                *head_grads, *dWs[:C], *dbs[:C])


def _tower_param_grads(lay, head, part, B: int, ns: int, g, one: bool, tdw: int, need_w: bool):
    """The weight-gradient tail of a fused tower (BCE and given-dz modes).  ``lay``:
    every layer of the launch as (W [N, K], b, tower images, dY, X), cross layers
    ahead of the MLP's; their dW = dY^T [X | 1] by mrec_tower_dw from the k-fragment
    images dY, X (``tdw`` slices), else by the generic split-K GEMMs from the rows
    dY [B, N], X [B, K]; one destination for all of them (``_decide``).  Then the head
    parameters from the tower's partials (``_head_param_grads``).  ->
    (dWs, dbs, (dW_h, db_h, dws, db2)), None where not returned."""
    # --- weight gradients of the layers: one launch, one destination for all ---
    n = len(lay)
    lr, views = _decide([t[0] for t in lay] + [t[1] for t in lay])
    returned = lr is None and views is None
    dWs, dbs = [None] * n, [None] * n
    calls = []
    if need_w:
        sk = tdw or _split_tower([lay[0][0].shape[1]] + [t[0].shape[0] for t in lay], B)
        ph = _mrec.GEMM_PARTIAL if sk > 1 else _mrec.GEMM_FULL
        # with mrec_tower_dw the calls below only carry the REDUCE phase's
        # arguments (its operands are never read: k-fragment images as stand-ins)
        opnd = (lambda t: t.view(-1, 8)) if tdw else (lambda t: t)  # noqa: E731
        for i, (W, bias_l, img, dy, xx) in enumerate(lay):
            dest = _grad_dest(W, bias_l, img, "tower",
                              (lr, None if views is None else (views[i], views[n + i])))
            dWs[i], dbs[i] = dest.dW, dest.db
            calls.append(_Call(opnd(dy), _mrec.LAYOUT_COL, opnd(xx), _mrec.LAYOUT_COL, *W.shape, B,
                               ph, split_k=sk, **dest.kw))
    # --- the head's parameters: deferred, so that the launch below takes it along ---
    head_grads = _head_param_grads(part, B, lay[-1][0].shape[0], ns, g, one, head)
    if not calls:
        _flush_finish()
    else:
        # the partial slabs (or, without split-K, the whole GEMMs) ...
        if tdw:
            _tower_dw(calls, [t[3] for t in lay], [t[4] for t in lay],
                      [tuple(t[0].shape) for t in lay], B, tdw)
        else:
            launch_multi(calls)
        # ... then the reductions of the slabs: mrec_tower_dw always leaves slabs
        if tdw or calls[0].split_k > 1:
            if returned:  # autograd may copy the gradients on return: complete them now
                _run_all([c.with_phase(_mrec.GEMM_REDUCE) for c in calls])
            else:  # in-place SGD / flat DP buffer: ride in the next launches
                for c in calls:
                    _defer(c)
    return dWs, dbs, head_grads


def _tower_dw(calls, dys, xins, dims, B: int, splits: int):
    """The tower's weight-gradient partial slabs by mrec_tower_dw from the
    k-fragment images (+ the deferred CTR head finish in the same launch); the
    split-K REDUCE of each call (fused SGD / flat DP buffer / returned gradient)
    follows as usual.  Pending reductions that write what this reads run first,
    the others right after it."""
    _flush_writers({t.data_ptr() for t in list(dys) + list(xins)})
    a = _mrec.TowerDwArgs()
    a.n_layers, a.batch, a.splits = len(calls), B, splits
    for l, c in enumerate(calls):
        a.n_out[l], a.n_in[l] = dims[l]
        a.dy_img[l], a.x_img[l] = dys[l].data_ptr(), xins[l].data_ptr()
        a.ws[l], a.ldws[l] = c.ws.data_ptr(), (dims[l][1] + 1 + 7) // 8 * 8
    fin = _take_finish()
    feed = take_feed_job()
    _mrec.call("mrec_tower_dw_ex", ctypes.byref(a), ctypes.byref(fin.struct) if fin else None,
               ctypes.byref(feed) if feed is not None else None, _mrec.stream_handle())
    _run_all(take_pending(len(_PENDING)))


def tower_bce(x0: torch.Tensor, mlp, head: torch.nn.Linear, base: Optional[torch.Tensor],
              y: torch.Tensor, xs: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
              b2: Optional[torch.Tensor] = None, cross=None) -> torch.Tensor:
    """Training loss of a CTR model's deep part: mean BCE-with-logits of
    MLP(x0) . head.weight + head.bias + base (+ xs . ws + b2) — the reference MLP
    (MLP.py:8-23) and Linear(N_L, 1) — as one fused tower launch (caller checks
    ``tower_supported``).  ``cross``: DCN-v2 cross layers (``nn.Linear(d, d)``)
    applied to x0 ahead of the MLP in the same launch (mrec_tower_args.n_cross)."""
    lins = _mlp_linears(mlp)
    cross = list(cross or [])
    params = ([l.weight for l in lins] + [l.bias for l in lins] +
              [head.weight, head.bias, ws, b2] + [c.weight for c in cross] + [c.bias for c in cross])
    return _TowerBCEFn.apply(x0, base, xs, y, len(lins), len(cross), *params)


class _ScoreTowerFn(torch.autograd.Function):
    """s = MLP(x0) . w + b per row (fp32 [B]): DIN's attention unit (att_mlp +
    att_out over the [q, k, q-k, q*k] rows) on the fused tower.  Forward = one
    MREC_TOWER_FORWARD launch (the scores only, nothing else leaves LDS); backward =
    one MREC_TOWER_GIVEN_DZ launch with dz = ds (the forward recomputed in LDS:
    dx0 and every pre-activation gradient, the k-fragment images) + mrec_tower_dw +
    the head finish, as the BCE tower's backward."""

    @staticmethod
    def forward(ctx, x0, n_layers, *params):
        L = n_layers
        Ws, bs = params[:L], params[L:2 * L]
        head_w, head_b = params[2 * L:2 * L + 2]
        B = x0.shape[0]
        widths = [Ws[0].shape[1]] + [W.shape[0] for W in Ws]
        imgs = [tower_images(W) for W in Ws]
        bsd, hw, hb = [_f32c(b) for b in bs], _f32c(head_w).reshape(-1), _f32c(head_b)
        z = torch.empty(B, dtype=torch.float32, device=x0.device)
        a = _tower_args(x0, widths, imgs, bsd, hw, hb)
        a.mode, a.z, a.ldp = _mrec.TOWER_FORWARD, z.data_ptr(), _r8(widths[L] + 1)
        _mrec.call("mrec_tower_fwd_bwd", ctypes.byref(a), _mrec.stream_handle())
        ctx.save_for_backward(x0)
        ctx.L, ctx.widths, ctx.Ws, ctx.bs, ctx.imgs = L, widths, Ws, bs, imgs
        ctx.head = (head_w, head_b, None, None)
        ctx.keep = (bsd, hw, hb)
        return z

    @staticmethod
    def backward(ctx, ds):
        x0, = ctx.saved_tensors
        L, widths = ctx.L, ctx.widths
        B = x0.shape[0]
        dev = x0.device
        ds = ds.detach().float().reshape(B).contiguous()
        need_w = any(ctx.needs_input_grad[2:2 + 2 * L])
        tdw = _tdw_splits(B, widths) if need_w else 0
        bufs = _tower_buffers(x0, widths, tdw, ctx.needs_input_grad[0])
        H = widths[L]
        part = torch.empty(int(_mrec.lib().mrec_ctr_head_parts(B)), _r8(H + 1), dtype=torch.float32,
                           device=dev)
        bsd, hw, hb = ctx.keep
        a = _tower_args(x0, widths, ctx.imgs, bsd, hw, hb, bufs, part)
        a.mode, a.dz_in = _mrec.TOWER_GIVEN_DZ, ds.data_ptr()
        _mrec.call("mrec_tower_fwd_bwd", ctypes.byref(a), _mrec.stream_handle())
        g = grad_one(dev)
        xin = [bufs.x0_img if tdw else x0[:, :widths[0]]] + bufs.hs
        dWs, dbs, (dW_h, db_h, _, _) = _tower_param_grads(
            list(zip(ctx.Ws, ctx.bs, ctx.imgs, bufs.dhs, xin)), ctx.head, part, B, 0, g, True, tdw,
            need_w)
        return (bufs.dx0, None, *dWs, *dbs, dW_h, db_h)


def score_tower(x0: torch.Tensor, mlp, head: torch.nn.Linear) -> torch.Tensor:
    """MLP(x0) . head.weight + head.bias per row (fp32 [B]) on the fused tower
    (caller checks ``tower_supported``): DIN's attention-unit scores."""
    lins = _mlp_linears(mlp)
    params = [l.weight for l in lins] + [l.bias for l in lins] + [head.weight, head.bias]
    return _ScoreTowerFn.apply(x0, len(lins), *params)
