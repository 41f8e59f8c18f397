"""The bf16 GEMM (csrc/gemm.hip, csrc/gemm_common.h) over its layouts, edges,
epilogues, split-K plans, fused-SGD epilogues, multi-job launches, co-launched
reductions and weight-image writers, each against a plain fp64 restatement.

Exact-integer method.  A, B, ``mul`` and ``add`` hold integers in [-3, 3] (exact in
bf16), ``bias`` multiples of 0.25, master weights multiples of 0.5, lr = 0.5 and
K <= 1152, so every partial sum is a multiple of 0.125 far below 2^24: the fp32
result is exact for any summation order, split and tile order.  The expected value
is computed in fp64 on the CPU and cast to fp32 (a bf16 output: that fp32 value
rounded once with RNE) and every comparison is ``torch.equal`` -- no tolerance, one
dropped, doubled or misplaced term fails.

Guards.  Every operand and output is a window of a larger allocation of the test's
own (``_Guarded``: one guard row in front, one behind, 64 more elements).  Operand
pads the contract wants zero are zero; everything the kernel must not read is NaN
(rows past the valid ones, k rows >= K of a COL operand, columns past round8(valid)
up to ld = round8(valid) + 8, the pads of ``mul`` / ``add`` / ``mask``, the whole
split-K workspace before the call).  Outputs start as 7.0: after the call columns
[N, pad_to) of C are 0 and every guard element still holds 7.0.  Nothing is read
or written out of bounds and no case provokes a fault.

The last section (random-normal operands) keeps test_gpu_dense.py's derived bound,
|got - ref| <= 2^-8 |ref| + 1e-5 sum|a b| (1e-6 |ref| for an fp32 output).

Fused SGD, "slices 1, 3 and 9" at reduction length 200: plan_split rounds a slice
to whole 64-wide k groups, so requests 1 / 3 / 9 resolve to 1 / 2 / 4 slabs there;
one more case (reduction length 576, request 9) really has 9 slabs and runs the
8-deep loop of the reduction with the update epilogue.
"""
import ctypes

import numpy as np
import pytest
import torch

gpu_test = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT = 7.0
NAN = float("nan")
LR = 0.5
LAYOUTS = {"RR": (False, False), "RC": (False, True), "CR": (True, False), "CC": (True, True)}
FULL, PARTIAL, REDUCE = 0, 1, 2
KG = 64  # k per staging group (gemm.hip)


def _r8(n):
    return (n + 7) // 8 * 8


def _ceil(a, b):
    return -(-a // b)


def _plan(K, req):
    """gemm.hip plan_split restated: (k per slice, slices)."""
    kps = max(KG, _ceil(_ceil(K, max(req, 1)), KG) * KG)
    return kps, (_ceil(K, kps) if K > 0 else 1)


def _ws_bytes(M, N, K, req):
    s = _plan(K, req)[1]
    return s * M * _r8(N + 1) * 4 if s > 1 else 0


# ---------------------------------------------------------------------------
# numpy restatements of the weight images
# ---------------------------------------------------------------------------

def _tower_idx_fwd(n, k, K):
    ks = (K + 31) >> 5
    return ((((n >> 4) * ks + (k >> 5)) * 64 + (n & 15) + 16 * ((k & 31) >> 3)) * 8) + (k & 7)


def _tower_idx_bwd(n, k, N):
    ns = (N + 31) >> 5
    return ((((k >> 4) * ns + (n >> 5)) * 64 + (k & 15) + 16 * ((n & 31) >> 3)) * 8) + (n & 7)


def _tower_elems(N, K, bwd):
    return _ceil(K, 16) * _ceil(N, 32) * 512 if bwd else _ceil(N, 16) * _ceil(K, 32) * 512


def _tower_image(w_bf16, bwd):
    """bf16 [N, K] (CPU) -> its fwd / bwd MFMA-fragment image, pads zero."""
    N, K = w_bf16.shape
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    idx = _tower_idx_bwd(n, k, N) if bwd else _tower_idx_fwd(n, k, K)
    img = np.zeros(_tower_elems(N, K, bwd), np.int16)
    img[idx.reshape(-1)] = w_bf16.contiguous().view(torch.int16).numpy().reshape(-1)
    return torch.from_numpy(img).view(BF16)


IMG_SHAPES = [(1, 1), (33, 45), (32, 32), (70, 129), (64, 64), (4, 4), (3, 5), (70, 48), (129, 66)]


@pytest.mark.parametrize("N,K", IMG_SHAPES)
def test_tower_index_restatements_are_injective_and_in_range(N, K):
    """The numpy restatements of tower_idx_fwd / tower_idx_bwd map [0, N) x [0, K)
    one-to-one into [0, elems), elems the restated tower_img_elems_* and the
    library's mrec_tower_image_elems.  Runs without a GPU."""
    from pytorchrec_amd import _mrec
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    for bwd in (0, 1):
        idx = (_tower_idx_bwd(n, k, N) if bwd else _tower_idx_fwd(n, k, K)).reshape(-1)
        elems = _tower_elems(N, K, bwd)
        assert elems == int(_mrec.lib().mrec_tower_image_elems(N, K, bwd))
        assert idx.min() >= 0 and idx.max() < elems
        assert np.unique(idx).size == N * K
    # four consecutive k of a row (fwd) / n of a column (bwd) stay adjacent: what
    # the 4 x 4 block update stores as 8 bytes
    for j in range(1, 4):
        if K > j:
            assert _tower_idx_fwd(0, j, K) == _tower_idx_fwd(0, 0, K) + j
        if N > j:
            assert _tower_idx_bwd(j, 0, N) == _tower_idx_bwd(0, 0, N) + j


# ---------------------------------------------------------------------------
# guarded buffers, operands, the raw call
# ---------------------------------------------------------------------------

class _Guarded:
    """A [rows, ld] window of a flat allocation filled with ``fill``: a guard row in
    front (rounded to 8 elements so the window keeps the allocation's 16-byte
    alignment, plus ``offset`` elements), a guard row and 64 elements behind.
    ``host`` is the CPU image (inputs: what is uploaded; outputs: edited into the
    expected image), ``dev`` the device copy made by ``up``."""

    def __init__(self, rows, ld, dtype, fill, offset=0):
        self.rows, self.ld = rows, ld
        self.front = _r8(max(ld, 1)) + offset
        self.host = torch.full((self.front + (rows + 1) * ld + 64,), fill, dtype=dtype)
        self.dev = None

    def win(self, flat=None):
        flat = self.host if flat is None else flat
        return flat[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)

    def up(self, dev):
        self.dev = self.host.to(dev)
        return self

    @property
    def t(self):
        return self.win(self.dev)

    def check(self, what):
        """device contents == host (expected) image, guards included"""
        got = self.dev.cpu()
        if torch.equal(got, self.host):
            return
        bad = torch.nonzero(~(got == self.host)).reshape(-1)
        i = int(bad[0])
        r, c = divmod(i - self.front, self.ld) if self.ld else (0, 0)
        raise AssertionError(f"{what}: {bad.numel()} elements differ; first at flat {i} "
                             f"(window row {r}, col {c}): got {got[i].item()}, "
                             f"want {self.host[i].item()}")


def _ints(rng, *shape, lo=-3, hi=3):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def _operand(vals, col, dev, span=None, pad=0.0):
    """``vals`` fp64 [I, K] (element (i, k); values exact in bf16) as a guarded ROW
    ([i][k]) or COL ([k][i]) bf16 operand.  ``span``: the extent the kernel is told
    for i (N for a B whose b_cols = I < N).  The NaN behind the valid k reaches the
    end of the last 64-wide k group (COL: rows, ROW: the guard behind the window),
    so a kernel that staged a whole group would read NaN, still inside the
    allocation.  ``pad``: the value of the pad up to round8 (zero by contract)."""
    I, K = vals.shape
    span = I if span is None else span
    if not col:
        g = _Guarded(span + 2, _r8(K) + 8, BF16, NAN)
        w = g.win()
        w[:I, :K] = vals.to(BF16)
        w[:I, K:_r8(K)] = pad
    else:
        g = _Guarded(max(K + 2, _ceil(K, KG) * KG), _r8(span) + 8, BF16, NAN)
        w = g.win()
        w[:K, :I] = vals.T.to(BF16)
        w[:K, I:_r8(I)] = pad
    return g.up(dev)


def _vec1(vals, dev, fill=NAN):
    """fp32 vector inside a guarded allocation"""
    g = _Guarded(1, vals.numel(), F32, fill)
    g.win()[0] = vals.float()
    return g.up(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return 0 if t is None else t.stride(0)


class _Job:
    """One mrec_gemm call over device tensors (2-D windows; 1-D for bias / ones_out):
    ``run`` through mrec_gemm, ``call`` as an mrec_gemm_call of mrec_gemm_multi."""

    def __init__(self, M, N, K, A, a_col, B, b_col, C, *, ones_out=None, b_cols=None, split=1,
                 ws=None, ws_bytes=None, bias=None, act=0, mul=None, add=None, aux=None,
                 mask=None, lr=None, img_row=None, img_tr=None, img_kind=0, ld_img_row=0,
                 ld_img_tr=0, a_off=0, lda=None, ldb=None, ldc=None, ones_col=None):
        from pytorchrec_amd import _mrec
        self.keep = [A, B, C, ones_out, ws, bias, mul, add, aux, mask, img_row, img_tr]
        self.a = _mrec.Operand(A.data_ptr() + a_off, _mrec.BF16,
                               _mrec.LAYOUT_COL if a_col else _mrec.LAYOUT_ROW,
                               A.stride(0) if lda is None else lda)
        self.b = _mrec.Operand(B.data_ptr(), _mrec.BF16,
                               _mrec.LAYOUT_COL if b_col else _mrec.LAYOUT_ROW,
                               B.stride(0) if ldb is None else ldb)
        self.epi = _mrec.Epilogue(_ptr(bias), act, _ptr(mul), _ld(mul), _ptr(add), _ld(add),
                                  _ptr(aux), _ld(aux), _ptr(mask), _ld(mask), _ptr(ones_out),
                                  int(lr is not None), float(lr or 0.0), _ptr(img_row),
                                  ld_img_row, _ptr(img_tr), ld_img_tr, img_kind)
        if ones_col is None:
            ones_col = N if ones_out is not None else -1
        if ws_bytes is None:
            ws_bytes = ws.numel() * ws.element_size() if ws is not None else 0
        self.args = (M, N, K, ones_col, N if b_cols is None else b_cols, C.data_ptr(),
                     _mrec.dtype_code(C.dtype), C.stride(0) if ldc is None else ldc, split,
                     _ptr(ws), ws_bytes)

    def status(self):
        from pytorchrec_amd import _mrec
        M, N, K, ones, bcols, C, cdt, ldc, sk, ws, wsb = self.args
        return _mrec.lib().mrec_gemm(M, N, K, ctypes.byref(self.a), ctypes.byref(self.b), ones,
                                     bcols, ctypes.byref(self.epi), C, cdt, ldc, sk, ws, wsb,
                                     _mrec.stream_handle())

    def run(self):
        from pytorchrec_amd import _mrec
        _mrec.check("mrec_gemm", self.status())

    def call(self, phase):
        from pytorchrec_amd import _mrec
        M, N, K, ones, bcols, C, cdt, ldc, sk, ws, wsb = self.args
        return _mrec.GemmCall(M, N, K, ctypes.pointer(self.a), ctypes.pointer(self.b), ones, bcols,
                              ctypes.pointer(self.epi), C, cdt, ldc, sk, ws, wsb, phase)


def _multi_status(calls):
    from pytorchrec_amd import _mrec
    arr = (_mrec.GemmCall * max(1, len(calls)))(*calls)
    return _mrec.lib().mrec_gemm_multi(len(calls), arr, _mrec.stream_handle())


def _multi(calls):
    from pytorchrec_amd import _mrec
    _mrec.check("mrec_gemm_multi", _multi_status(calls))


def _workspace(M, N, K, req, dev, ones):
    """The split-K workspace of exactly mrec_gemm_workspace_size bytes (checked
    against the restated formula), NaN-filled, with 16 guard floats behind.
    Returns (allocation, workspace, floats the slabs take: slices x M x
    round8(N + ones), the slab stride the reduction reads)."""
    from pytorchrec_amd import _mrec
    nbytes = int(_mrec.lib().mrec_gemm_workspace_size(M, N, K, req))
    assert nbytes == _ws_bytes(M, N, K, req), (nbytes, _ws_bytes(M, N, K, req))
    if nbytes == 0:
        return None, None, 0
    buf = torch.full((nbytes // 4 + 16,), NAN, dtype=F32)
    buf[nbytes // 4:] = SENT
    buf = buf.to(dev)
    return buf, buf[:nbytes // 4], _plan(K, req)[1] * M * _r8(N + int(ones))


def _check_ws(buf, ws, used):
    """every slab element was written (no NaN left), nothing behind the slabs"""
    if buf is None:
        return
    h = buf.cpu()
    n = ws.numel()
    assert not torch.isnan(h[:used]).any(), "a slab element the reduction reads was never written"
    assert torch.isnan(h[used:n]).all(), "write behind the slabs"
    assert torch.all(h[n:] == SENT), "write behind the workspace"


# bf16 bit patterns of the mask: +1, 2, -1, +0, -0, smallest subnormal, its negative
_MASK_BITS = np.array([0x3f80, 0x4000, 0xbf80, 0x0000, 0x8000, 0x0001, 0x8001], np.uint16)
_MASK_HAND = [0x0000, 0x8000, 0xbf80, 0x3f80, 0x0001]  # +0, -0, negative, positive, subnormal


def _mask_bits(rng, M, N):
    """mask bits [M, N]: the hand-chosen values at the start of row 0 and at the end
    of the last row (as far as N allows), random picks of _MASK_BITS elsewhere"""
    bits = _MASK_BITS[rng.integers(0, len(_MASK_BITS), (M, N))]
    n = min(N, len(_MASK_HAND))
    bits[0, :n] = _MASK_HAND[:n]
    bits[M - 1, N - n:] = _MASK_HAND[:n]
    return bits


def _mask_keep(bits):
    """the documented rule "mask > 0 keeps", on the bits: nonzero and sign clear"""
    return torch.from_numpy((bits != 0) & ((bits & 0x8000) == 0))


class _Product:
    """A plain (non-update) GEMM case: guarded operands, outputs and fp64 expectation."""

    def __init__(self, dev, lay, M, N, K, c_f32, *, ones=False, b_cols=None, req=1, terms=(),
                 path="vec", seed=0, a_pad=0.0):
        a_col, b_col = LAYOUTS[lay]
        rng = np.random.default_rng([seed, M, N, K])
        bc = N if b_cols is None else b_cols
        Av, Bv = _ints(rng, M, K), _ints(rng, bc, K)
        self.A = _operand(Av, a_col, dev, pad=a_pad)
        self.B = _operand(Bv, b_col, dev, span=N)
        v = torch.zeros(M, N, dtype=torch.float64)
        v[:, :bc] = Av @ Bv.T
        ldx = _r8(N) + 8
        kw = {}
        self.extra = []

        def side(vals):  # bf16 [M, N] epilogue operand, its pads NaN
            g = _Guarded(M, ldx, BF16, NAN)
            g.win()[:, :N] = vals
            self.extra.append(g.up(dev))
            return g.t[:, :N]

        self.aux = None
        if "bias" in terms:
            bias = _ints(rng, N, lo=-8, hi=8) * 0.25
            g = _vec1(bias, dev)
            self.extra.append(g)
            kw["bias"] = g.t[0]
            v = v + bias
        if "aux" in terms:
            self.aux = _Guarded(M, ldx, BF16, SENT)
            self.aux.win()[:, :N] = v.float().to(BF16)
            if path == "vec" and _plan(K, req)[1] == 1:  # whole 16-byte chunks: pads zero
                self.aux.win()[:, N:_r8(N)] = 0
        if "act" in terms:
            kw["act"] = 1
            v = v.clamp_min(0.0)
        if "mul" in terms:
            mul = _ints(rng, M, N)
            kw["mul"] = side(mul.to(BF16))
            v = v * mul
        if "add" in terms:
            add = _ints(rng, M, N)
            kw["add"] = side(add.to(BF16))
            v = v + add
        if "mask" in terms:
            bits = _mask_bits(rng, M, N)
            kw["mask"] = side(torch.from_numpy(bits.view(np.int16)).view(BF16))
            v = torch.where(_mask_keep(bits), v, torch.zeros_like(v))
        self.want = v.float()
        dt = F32 if c_f32 else BF16
        ldc, off = {"vec": (ldx, 0), "ldN": (N, 0), "off1": (ldx, 1)}[path]
        pad_to = min(ldc, _r8(N))
        self.C = _Guarded(M, ldc, dt, SENT, offset=off)
        w = self.C.win()
        w[:, :N] = self.want.to(dt)
        w[:, N:pad_to] = 0
        self.ones = None
        if ones:
            self.ones = _Guarded(1, M, F32, SENT)
            self.ones.win()[0] = Av.sum(1).float()
        self.wsbuf, self.ws, self.ws_used = _workspace(M, N, K, req, dev, ones)
        self.slabs = _plan(K, req)[1]
        self.scalar = path != "vec" or self.slabs > 1  # which epilogue writes C and aux
        self.dims, self.lay, self.kw, self.req, self.b_cols, self.N = (M, N, K), lay, kw, req, b_cols, N
        self.outputs(dev)

    def outputs(self, dev):
        """fresh sentinel-filled outputs and the job writing them"""
        a_col, b_col = LAYOUTS[self.lay]
        M, N, K = self.dims
        outs = [g for g in (self.C, self.aux, self.ones) if g is not None]
        for g in outs:
            g.dev = torch.full_like(g.host, SENT).to(dev)
        self.job = _Job(M, N, K, self.A.t, a_col, self.B.t, b_col, self.C.t,
                        ones_out=self.ones.t[0] if self.ones else None, b_cols=self.b_cols,
                        split=self.req, ws=self.ws, aux=self.aux.t[:, :N] if self.aux else None,
                        **self.kw)
        return outs

    def check(self, what=""):
        self.C.check(what + " C")
        if self.aux is not None:
            if self.scalar:
                # the scalar epilogue leaves aux's pad columns alone (or zero)
                N, got = self.N, self.aux.win(self.aux.dev.cpu())
                pad = got[:, N:_r8(N)]
                self.aux.win()[:, N:_r8(N)] = torch.where((pad == 0) | (pad == SENT), pad,
                                                          torch.full_like(pad, SENT))
            self.aux.check(what + " aux")
        if self.ones is not None:
            self.ones.check(what + " ones_out")
        _check_ws(self.wsbuf, self.ws, self.ws_used)

    def run_check(self, what=""):
        self.job.run()
        self.check(what)
        return self


# ---------------------------------------------------------------------------
# 1. layout x shape x output dtype
# ---------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (63, 7, 63), (64, 64, 64), (65, 65, 65), (130, 72, 129), (5, 127, 200),
          (70, 8, 264), (33, 129, 8), (64, 128, 192)]


@gpu_test
@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_layout_shape_dtype(gpu, lay, shape, c_f32):
    """Every layout pair at the tile and k-group edges (one, two, three and four k
    groups, k tails of 1 and 8, M / N at 63 / 64 / 65): the product is exact, the
    pad columns are zero, NaN rows / columns / k outside the operands are never
    read (the zero page replaces them) and no guard element changes."""
    _Product(gpu, lay, *shape, c_f32).run_check()


@gpu_test
@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_k_zero_gives_activated_bias(gpu, lay):
    """K = 0: no k group is staged (the operands are all NaN); C = relu(bias)."""
    p = _Product(gpu, lay, 5, 12, 0, False, terms=("bias", "act")).run_check()
    assert torch.equal(p.want[0], p.want[4]) and (p.want > 0).any() and (p.want == 0).any()


@gpu_test
@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_b_cols_below_n_is_zero_operand(gpu, lay, c_f32):
    """b_cols = 67 < N = 72: rows [67, 72) of a ROW B are NaN, a COL B is zero up to
    round8(67) and NaN behind; those columns of the product are exactly epi(0)."""
    p = _Product(gpu, lay, 70, 72, 72, c_f32, b_cols=67, terms=("bias", "act")).run_check()
    assert torch.equal(p.want[:, 67:], p.want[:1, 67:].expand(70, 5))


# ---------------------------------------------------------------------------
# 2. ones column
# ---------------------------------------------------------------------------

def _ones_params():
    out = []
    for lay in ("CC", "RR"):
        for N in (45, 48, 63, 64, 128):
            for K, reqs in ((1, (1,)), (65, (1, 2)), (200, (1, 4))):
                out += [pytest.param(lay, N, K, r, id=f"{lay}-N{N}-K{K}-s{r}") for r in reqs]
    return out


@gpu_test
@pytest.mark.parametrize("lay,N,K,req", _ones_params())
def test_ones_column(gpu, lay, N, K, req):
    """b_ones_col = N under a COL and a ROW B: on a chunk boundary (48), the last
    column of a tile (63), a tile of its own (64, 128), inside a chunk (45), over
    one, two and four k groups with a tail, plain and split.  ones_out is the exact
    row sum of A; the pad column the ones column occupies is 0 when < pad_to."""
    p = _Product(gpu, lay, 70, N, K, True, ones=True, req=req).run_check()
    assert p.slabs == {1: 1, 2: 2, 4: 4}[req] or K == 1


@gpu_test
@pytest.mark.parametrize("K,req", [(1, 1), (65, 1), (65, 2)])
@pytest.mark.parametrize("N", [45, 64])
def test_ones_column_is_zero_past_k(gpu, N, K, req):
    """The ones column is a B column like any other: zero for k >= K.  Under the
    operand contract that zero cannot be seen (A is zero there too: its zero pad,
    then the zero page), so this one case steps outside the contract on purpose: a
    ROW A whose pad [K, round8(K)) holds 2.0, B's pad zero.  The product stays exact
    (B's zero pad) and so must ones_out (the ones column's own zero past K)."""
    _Product(gpu, "RR", 70, N, K, True, ones=True, req=req, a_pad=2.0).run_check()


# ---------------------------------------------------------------------------
# 3. epilogue
# ---------------------------------------------------------------------------

TERMS = {"bias": ("bias",), "act": ("act",), "aux": ("aux",), "mul": ("mul",), "add": ("add",),
         "mask": ("mask",), "all": ("bias", "act", "aux", "mul", "add", "mask")}


def _epi_params():
    out = []
    for N, paths in ((45, ("vec", "ldN", "off1")), (64, ("vec", "off1"))):
        for path in paths:
            for name in TERMS:
                for c_f32 in (False, True):
                    out.append(pytest.param(N, path, name, c_f32, 1,
                                            id=f"N{N}-{path}-{name}-{'f32' if c_f32 else 'bf16'}"))
    for N in (45, 64):  # the split-K reduce runs the scalar epilogue on aligned buffers
        for c_f32 in (False, True):
            out.append(pytest.param(N, "vec", "all", c_f32, 2,
                                    id=f"N{N}-reduce-all-{'f32' if c_f32 else 'bf16'}"))
    return out


@gpu_test
@pytest.mark.parametrize("N,path,name,c_f32,req", _epi_params())
def test_epilogue_terms(gpu, N, path, name, c_f32, req):
    """bias, act, aux, mul, add, mask alone and together on the 16-byte path (vec),
    and on the scalar path: ldc == N = 45 (ldN), a C one element off alignment
    (off1), the split-K reduce.  aux = bf16(acc + bias) before the activation; the
    mask holds +0, -0, a negative, a positive and the smallest subnormal in known
    places and keeps exactly the nonzero, sign-clear ones (mask > 0)."""
    _Product(gpu, "RR", 70, N, 72, c_f32, terms=TERMS[name], path=path, req=req).run_check()


@gpu_test
@pytest.mark.parametrize("N", [45, 64])
def test_mask_vector_and_scalar_paths_agree(gpu, N):
    """The two mask predicates (a float compare on the 16-byte path, a bit test on
    the scalar path) give bitwise the same C, the subnormal kept by both."""
    v = _Product(gpu, "RR", 70, N, 72, True, terms=("mask",), path="vec", seed=3).run_check()
    s = _Product(gpu, "RR", 70, N, 72, True, terms=("mask",), path="off1", seed=3).run_check()
    assert torch.equal(v.C.t[:, :N].cpu(), s.C.t[:, :N].cpu())
    # the rule on the hand-placed values: +0, -0 and the negative drop, the positive
    # and the subnormal keep
    hand = np.array(_MASK_HAND, np.uint16)
    assert _mask_keep(hand).tolist() == [False, False, False, True, True]


# ---------------------------------------------------------------------------
# 4. split-K
# ---------------------------------------------------------------------------

SPLITS = [(70, 45, 130, 3, 3, 2), (64, 64, 65, 2, 2, 1), (10, 20, 576, 9, 9, 64),
          (10, 20, 1093, 64, 18, 5), (70, 45, 64, 4, 1, 64)]


@gpu_test
@pytest.mark.parametrize("M,N,K,req,slabs,last", SPLITS,
                         ids=[f"{m}x{n}x{k}-s{r}" for m, n, k, r, _, _ in SPLITS])
@pytest.mark.parametrize("lay", ["CC", "RR"])
def test_split_k(gpu, lay, M, N, K, req, slabs, last):
    """A last slice of 2 and of 1 k, 9 slabs (one 8-deep batch of the reduction), 18
    (two batches and a tail), a request that resolves to one slice (workspace size
    0).  The workspace is NaN before the call: every slab element the reduction
    reads was written.  Two runs agree bitwise."""
    kps, s = _plan(K, req)
    assert s == slabs and K - (s - 1) * kps == last
    p = _Product(gpu, lay, M, N, K, True, ones=True, req=req)
    assert (p.ws is None) == (slabs == 1)
    p.run_check("first run")
    first = [g.dev.clone() for g in (p.C, p.ones)]
    if p.ws is not None:
        p.ws.fill_(NAN)
    p.outputs(gpu)
    p.run_check("second run")
    assert all(torch.equal(a, g.dev) for a, g in zip(first, (p.C, p.ones)))


# ---------------------------------------------------------------------------
# 5. fused-SGD epilogue
# ---------------------------------------------------------------------------

class _Update:
    """update = 1, COL / COL, b_ones_col = N: the weight-gradient GEMM of a Linear
    [n_out, n_in] over a batch of K as its SGD step.  ``r8``: the master is a view
    of an [n_out, round8(n_in)] buffer, else contiguous [n_out, n_in]."""

    def __init__(self, dev, n_out, n_in, K, req, kind, r8, seed=0, normal=False):
        from pytorchrec_amd import _mrec
        self.dev, self.kind, self.dims, self.req = dev, kind, (n_out, n_in, K), req
        rng = np.random.default_rng([seed, n_out, n_in, K])
        if normal:
            dY = torch.from_numpy(rng.standard_normal((K, n_out))).to(BF16).double()
            X = torch.from_numpy(rng.standard_normal((K, n_in))).to(BF16).double()
            self.W0 = torch.from_numpy(rng.standard_normal((n_out, n_in))).float().double()
            self.b0 = torch.from_numpy(rng.standard_normal(n_out)).float().double()
        else:
            dY, X = _ints(rng, K, n_out), _ints(rng, K, n_in)
            self.W0 = _ints(rng, n_out, n_in, lo=-4, hi=4) * 0.5
            self.b0 = _ints(rng, n_out, lo=-4, hi=4) * 0.5
        self.A = _operand(dY.T.contiguous(), True, dev)
        self.B = _operand(X.T.contiguous(), True, dev)
        self.dW, self.db = dY.T @ X, dY.sum(0)
        self.mag_w, self.mag_b = dY.abs().T @ X.abs(), dY.abs().sum(0)
        self.ldc = _r8(n_in) if r8 else n_in
        self.wsbuf, self.ws, self.ws_used = _workspace(n_out, n_in, K, req, dev, True)
        self.slabs = _plan(K, req)[1]
        self.tower = kind == _mrec.IMG_TOWER

    def outputs(self):
        """fresh master / bias / images (prepped from the old W by the library) + job"""
        from pytorchrec_amd import _mrec
        n_out, n_in, K = self.dims
        dev = self.dev
        W = _Guarded(n_out, self.ldc, F32, SENT)
        W.win()[:, :n_in] = self.W0.float()
        b = _Guarded(1, n_out, F32, SENT)
        b.win()[0] = self.b0.float()
        if self.tower:
            imgs = [_Guarded(1, _tower_elems(n_out, n_in, bwd), BF16, SENT) for bwd in (0, 1)]
            ld_row = ld_tr = 0
        else:
            ld_row, ld_tr = _r8(n_in), _r8(n_out)
            imgs = [_Guarded(n_out, ld_row, BF16, SENT), _Guarded(n_in, ld_tr, BF16, SENT)]
        for g in imgs:
            g.win().zero_()
        for g in [W, b] + imgs:
            g.up(dev)
        if self.tower:
            _mrec.call("mrec_tower_weight_prep", W.t.data_ptr(), n_out, n_in, self.ldc,
                       imgs[0].t.data_ptr(), imgs[1].t.data_ptr(), _mrec.stream_handle())
        else:
            _mrec.call("mrec_weight_prep", W.t.data_ptr(), n_out, n_in, self.ldc,
                       imgs[0].t.data_ptr(), ld_row, imgs[1].t.data_ptr(), ld_tr,
                       _mrec.stream_handle())
        job = _Job(n_out, n_in, K, self.A.t, True, self.B.t, True, W.t[:, :n_in],
                   ones_out=b.t[0], split=self.req, ws=self.ws, lr=LR, img_row=imgs[0].t,
                   img_tr=imgs[1].t, img_kind=self.kind, ld_img_row=ld_row, ld_img_tr=ld_tr)
        return dict(W=W, b=b, imgs=imgs, job=job)

    def expect(self, o):
        """edit the host images of ``o`` into the exact-integer expectation"""
        n_out, n_in, _ = self.dims
        newW = (self.W0 - LR * self.dW).float()
        o["W"].win()[:, :n_in] = newW
        o["b"].win()[0] = (self.b0 - LR * self.db).float()
        self.expect_images(o, newW.to(BF16))

    def expect_images(self, o, w_bf16):
        n_out, n_in, _ = self.dims
        if self.tower:
            for bwd in (0, 1):
                o["imgs"][bwd].win()[0] = _tower_image(w_bf16, bwd)
        else:
            o["imgs"][0].win()[:, :n_in] = w_bf16
            o["imgs"][1].win()[:, :n_out] = w_bf16.T

    def check(self, o, what=""):
        for name in ("W", "b"):
            o[name].check(f"{what} {name}")
        o["imgs"][0].check(what + " img_row / fwd")
        o["imgs"][1].check(what + " img_tr / bwd")
        _check_ws(self.wsbuf, self.ws, self.ws_used)


def _update_params():
    out = []
    for n_out, n_in in [(4, 4), (3, 5), (33, 45), (64, 64), (70, 48), (129, 66)]:
        for r8 in ((False, True) if n_in % 4 else (False,)):
            for kind in (0, 1):
                for K, req in ((200, 1), (200, 3)):
                    out.append((n_out, n_in, K, req, kind, r8))
    for kind in (0, 1):
        out += [(33, 45, 200, 9, kind, True), (33, 45, 576, 9, kind, True)]
    return [pytest.param(*p, id=f"{p[0]}x{p[1]}-K{p[2]}-s{p[3]}-{'tower' if p[4] else 'rowtr'}-"
                                f"{'r8view' if p[5] else 'contig'}") for p in out]


@gpu_test
@pytest.mark.parametrize("n_out,n_in,K,req,kind,r8", _update_params())
def test_fused_sgd_epilogue(gpu, n_out, n_in, K, req, kind, r8):
    """Master and bias bitwise w - lr dW and b - lr db; the row / transposed images
    equal the image of the new master with zero pads, the tower images the numpy
    fragment image with every pad entry still zero.  One slice runs the update in
    the GEMM's own epilogue, more run the reduction: with tower images and
    ldc % 4 == 0 in 4 x 4 blocks with remainder rows (n_out % 4) and columns
    (n_in % 4) on the element path, with a contiguous [n_out, n_in] master of
    n_in % 4 != 0 on the element path alone."""
    u = _Update(gpu, n_out, n_in, K, req, kind, r8)
    assert u.slabs == {(200, 1): 1, (200, 3): 2, (200, 9): 4, (576, 9): 9}[(K, req)]
    o = u.outputs()
    o["job"].run()
    u.expect(o)
    u.check(o)


# ---------------------------------------------------------------------------
# 6. multi-job launch
# ---------------------------------------------------------------------------

def _tiles(M, N, ones):
    return _ceil(M, 64) * _ceil(N + ones, 64)


@gpu_test
def test_multi_job_launch_mixes_kinds_and_phases(gpu):
    """One launch: a FULL RR job with a mask, a PARTIAL CC job, the REDUCE of an
    earlier, different PARTIAL and a FULL CR job; no job's tile or reduce workgroup
    count is a multiple of 8, so padding workgroups sit between the jobs.  Every
    result is bitwise that of the same call through mrec_gemm (and the fp64 value);
    the REDUCE of the launch's own PARTIAL, run alone afterwards, equals mrec_gemm's
    split result."""
    full_rr = _Product(gpu, "RR", 70, 130, 72, False, terms=("mask",), seed=1)
    part_cc = _Product(gpu, "CC", 70, 45, 130, True, ones=True, req=3, seed=2)
    red = _Product(gpu, "CC", 33, 70, 200, True, ones=True, req=4, seed=3)
    full_cr = _Product(gpu, "CR", 65, 65, 65, True, seed=4)
    assert [_tiles(70, 130, 0), _tiles(70, 45, 1), _tiles(65, 65, 0)] == [6, 2, 4]
    assert _ceil(33 * (_r8(71) // 4), 256) == 3 and red.slabs == 4 and part_cc.slabs == 3
    # the same calls through mrec_gemm alone
    alone = {}
    for name, p in (("rr", full_rr), ("cc", part_cc), ("red", red), ("cr", full_cr)):
        p.run_check(name + " alone")
        alone[name] = [g.dev.clone() for g in (p.C, p.ones) if g is not None]
        if p.ws is not None:
            p.ws.fill_(NAN)
        p.outputs(gpu)
    _multi([red.job.call(PARTIAL)])
    _multi([full_rr.job.call(FULL), part_cc.job.call(PARTIAL), red.job.call(REDUCE),
            full_cr.job.call(FULL)])
    for name, p in (("rr", full_rr), ("red", red), ("cr", full_cr)):
        p.check(name + " in the launch")
        got = [g.dev for g in (p.C, p.ones) if g is not None]
        assert all(torch.equal(a, b) for a, b in zip(alone[name], got)), name
    assert torch.all(part_cc.C.dev == SENT) and torch.all(part_cc.ones.dev == SENT)
    _multi([part_cc.job.call(REDUCE)])
    part_cc.check("REDUCE alone")
    assert all(torch.equal(a, g.dev) for a, g in zip(alone["cc"], (part_cc.C, part_cc.ones)))


@gpu_test
def test_multi_job_launch_drops_empty_jobs(gpu):
    """n = 0 is OK and launches nothing; a job with M = 0 is dropped, its output
    untouched, the job beside it computed."""
    from pytorchrec_amd import _mrec
    assert _multi_status([]) == _mrec.OK
    p = _Product(gpu, "RC", 65, 7, 63, False, seed=5)
    e = _Product(gpu, "RR", 3, 9, 16, False, seed=6)
    M, N, K = e.dims
    empty = _Job(0, N, K, e.A.t, False, e.B.t, False, e.C.t)
    _multi([empty.call(FULL), p.job.call(FULL)])
    p.check()
    assert torch.all(e.C.dev == SENT)
    _multi([empty.call(FULL)])
    assert torch.all(e.C.dev == SENT)


# ---------------------------------------------------------------------------
# 7. a reduce co-launched with an embedding update
# ---------------------------------------------------------------------------

class _Pending:
    """what dense._PENDING holds: an object whose struct() is the REDUCE call"""

    def __init__(self, job):
        self.job = job

    def struct(self):
        return self.job.call(REDUCE)


def _emb_backward(gpu, B):
    """one small fused-SGD embedding backward; returns the bank's bits"""
    from pytorchrec_amd import embedding as E
    from test_gpu_embedding import _bank, _bits, _fill
    rng = np.random.default_rng(B)
    nums, D = [50, 7], 16
    bank = _bank(nums, D, False, F32, update="sgd")
    bank.use_fused_sgd(LR)
    bank.stochastic_rounding = False
    _fill(bank, [(rng.standard_normal((n, D)) * 0.5).astype(np.float32) for n in nums])
    ids = [torch.from_numpy(rng.integers(0, n, B).astype(np.int32)).to(gpu) for n in nums]
    dy = torch.from_numpy((rng.standard_normal((B, 2 * D)) * 0.05).astype(np.float32)).to(gpu)
    E.gather(bank, ids, out_dtype=F32).backward(dy)
    torch.cuda.synchronize()
    return _bits(bank.weight)


@gpu_test
@pytest.mark.parametrize("slabs", [4, 9])
@pytest.mark.parametrize("path,B", [("hash", 300), ("sorted", 4100), ("large", 8200)])
def test_reduce_co_launched_with_embedding_update(gpu, path, B, slabs, monkeypatch):
    """A fused-SGD REDUCE (tower images, the 4 x 4 block path with remainders) queued
    on dense._PENDING after its PARTIAL launch is taken by the embedding update's
    launch: the hash and the sorted apply kernel and the large-batch bucket kernel
    (splitk_reduce_body<false> through co_reduce).  The queue is drained, the GEMM
    result is bitwise that of the same REDUCE through mrec_gemm_multi on a copy (and
    the exact value), the embedding result bitwise that of the same backward with
    nothing pending."""
    from pytorchrec_amd import _mrec, dense as D, embedding as E
    monkeypatch.setattr(E, "LARGE_FUSED", True)
    assert (B > _mrec.BWD_MAX_BATCH) == (path == "large")
    assert (B > _mrec.BWD_HASH_MAX_BATCH) == (path != "hash")
    K, req = {4: (200, 4), 9: (576, 9)}[slabs]
    u = _Update(gpu, 33, 45, K, req, _mrec.IMG_TOWER, True, seed=7)
    assert u.slabs == slabs
    o, ref = u.outputs(), u.outputs()
    _multi([o["job"].call(PARTIAL)])
    _multi([ref["job"].call(REDUCE)])
    u.expect(ref)
    u.check(ref, "mrec_gemm_multi REDUCE")
    assert not D._PENDING
    plain = _emb_backward(gpu, B)
    D._PENDING.append(_Pending(o["job"]))
    try:
        beside = _emb_backward(gpu, B)
        assert not D._PENDING, "the embedding launch did not take the pending reduction"
    finally:
        D._PENDING.clear()
    u.expect(o)
    u.check(o, "co-launched REDUCE")
    for name in ("W", "b"):
        assert torch.equal(o[name].dev, ref[name].dev), name
    assert all(torch.equal(a.dev, b.dev) for a, b in zip(o["imgs"], ref["imgs"]))
    assert np.array_equal(plain, beside)


# ---------------------------------------------------------------------------
# 8. image writers
# ---------------------------------------------------------------------------

def _weight_source(N, K, dev, seed):
    """fp32 [N, K] in a strided (ldw = K + 5), NaN-surrounded source; values with
    bf16 rounding ties both ways"""
    rng = np.random.default_rng([seed, N, K])
    W = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0e-39, -0.0])
    W.reshape(-1)[:min(5, N * K)] = ties[:min(5, N * K)]
    g = _Guarded(N, K + 5, F32, NAN)
    g.win()[:, :K] = W
    return W, g.up(dev)


PREP_SHAPES = [(1, 1), (33, 45), (32, 32), (70, 129)]


@gpu_test
@pytest.mark.parametrize("N,K", PREP_SHAPES)
def test_weight_prep_images(gpu, N, K):
    """mrec_weight_prep from a strided source: the row image [N, ldr] and W^T
    [K, ldt] are the RNE bf16 of W with every pad column up to ld zero."""
    from pytorchrec_amd import _mrec
    W, src = _weight_source(N, K, gpu, 1)
    row = _Guarded(N, _r8(K) + 8, BF16, SENT).up(gpu)
    tr = _Guarded(K, _r8(N) + 8, BF16, SENT).up(gpu)
    _mrec.call("mrec_weight_prep", src.t.data_ptr(), N, K, src.ld, row.t.data_ptr(), row.ld,
               tr.t.data_ptr(), tr.ld, _mrec.stream_handle())
    row.win().zero_()
    row.win()[:, :K] = W.to(BF16)
    tr.win().zero_()
    tr.win()[:, :N] = W.to(BF16).T
    row.check("row image")
    tr.check("transposed image")


@gpu_test
@pytest.mark.parametrize("N,K", PREP_SHAPES)
def test_tower_weight_prep_images(gpu, N, K):
    """mrec_tower_weight_prep from a strided source against the numpy restatement
    of tower_idx_fwd / tower_idx_bwd; pad entries stay zero."""
    from pytorchrec_amd import _mrec
    W, src = _weight_source(N, K, gpu, 2)
    imgs = [_Guarded(1, _tower_elems(N, K, bwd), BF16, SENT) for bwd in (0, 1)]
    for g in imgs:
        g.win().zero_()
        g.up(gpu)
    _mrec.call("mrec_tower_weight_prep", src.t.data_ptr(), N, K, src.ld, imgs[0].t.data_ptr(),
               imgs[1].t.data_ptr(), _mrec.stream_handle())
    for bwd in (0, 1):
        imgs[bwd].win()[0] = _tower_image(W.to(BF16), bwd)
        imgs[bwd].check("bwd image" if bwd else "fwd image")


@gpu_test
@pytest.mark.parametrize("N,K", [(33, 45), (64, 64)])
def test_sgd_multi_tower_images(gpu, N, K):
    """mrec_sgd_multi with MREC_IMG_TOWER: w -= lr g exactly (multiples of 0.5) and
    the fragment images of the new w, pads zero; a row / transposed job rides in
    the same launch."""
    from pytorchrec_amd import _mrec
    rng = np.random.default_rng([8, N, K])
    jobs, checks, keep = [], [], []
    for kind in (_mrec.IMG_TOWER, _mrec.IMG_ROW_TR):
        W0 = _ints(rng, N, K, lo=-9, hi=9) * 0.5
        G = _ints(rng, N, K, lo=-40, hi=40) * 0.25
        w = _Guarded(N, K + 3, F32, SENT)
        w.win()[:, :K] = W0.float()
        g = _Guarded(N, K + 1, F32, NAN)
        g.win()[:, :K] = G.float()
        if kind == _mrec.IMG_TOWER:
            imgs = [_Guarded(1, _tower_elems(N, K, bwd), BF16, SENT) for bwd in (0, 1)]
            ld_row = ld_tr = 0
        else:
            ld_row, ld_tr = _r8(K), _r8(N)
            imgs = [_Guarded(N, ld_row, BF16, SENT), _Guarded(K, ld_tr, BF16, SENT)]
        for x in imgs:
            x.win().zero_()
        for x in [w, g] + imgs:
            x.up(gpu)
        jobs.append(_mrec.SgdJob(w.t.data_ptr(), g.t.data_ptr(), N, K, w.ld, g.ld, LR,
                                 imgs[0].t.data_ptr(), ld_row, imgs[1].t.data_ptr(), ld_tr, kind))
        new = (W0 - LR * G).float()
        w.win()[:, :K] = new
        if kind == _mrec.IMG_TOWER:
            for bwd in (0, 1):
                imgs[bwd].win()[0] = _tower_image(new.to(BF16), bwd)
        else:
            imgs[0].win()[:, :K] = new.to(BF16)
            imgs[1].win()[:, :N] = new.to(BF16).T
        checks += [(w, "master"), (imgs[0], "img_row / fwd"), (imgs[1], "img_tr / bwd")]
        keep.append(g)  # the gradient stays allocated until the launch has run
    arr = (_mrec.SgdJob * len(jobs))(*jobs)
    _mrec.call("mrec_sgd_multi", len(jobs), arr, _mrec.stream_handle())
    for x, what in checks:
        x.check(what)
    del keep


# ---------------------------------------------------------------------------
# 9. argument rejection (every call returns before any launch)
# ---------------------------------------------------------------------------

@gpu_test
def test_bad_arguments_are_rejected_before_any_launch(gpu):
    from pytorchrec_amd import _mrec
    p = _Product(gpu, "RR", 70, 45, 130, True, ones=True, req=3, seed=9)
    M, N, K = p.dims
    A, B, C, ones = p.A.t, p.B.t, p.C.t, p.ones.t[0]
    bias = torch.zeros(N, device=gpu)

    def job(**kw):
        kw.setdefault("ones_out", ones)
        return _Job(M, N, K, A, False, B, False, C, **kw)

    bad = {
        "A misaligned by 2 bytes": job(a_off=2),
        "lda % 8 != 0": job(lda=A.stride(0) + 4),
        "ldb % 8 != 0": job(ldb=B.stride(0) + 4),
        "b_ones_col not -1 or N": job(ones_col=N - 1),
        "b_ones_col beyond N": job(ones_col=N + 1),
        "b_cols > N": job(b_cols=N + 1),
        "split_k = 65": job(split=65, ws=p.ws),
        "ldc < N": job(ldc=N - 1),
        "update with a bias": job(lr=LR, bias=bias),
    }
    for what, j in bad.items():
        assert j.status() == _mrec.EINVAL, what
    short = job(split=3, ws=p.ws, ws_bytes=_ws_bytes(M, N, K, 3) - 4)
    assert short.status() == _mrec.ENOSPC
    good = job(split=3, ws=p.ws)
    full = job()
    multi_bad = {
        "n = 5": [full.call(FULL)] * 5,
        "FULL with a splitting split_k": [good.call(FULL)],
        "PARTIAL with one slice": [full.call(PARTIAL)],
        "REDUCE with one slice": [full.call(REDUCE)],
        "a bad job behind a good one": [full.call(FULL), bad["ldc < N"].call(FULL)],
    }
    for what, calls in multi_bad.items():
        assert _multi_status(calls) == _mrec.EINVAL, what
    torch.cuda.synchronize()
    for g in (p.C, p.ones):
        assert torch.all(g.dev == SENT), "a rejected call wrote an output"
    assert torch.isnan(p.ws).all(), "a rejected call wrote the workspace"
    p.run_check("the same arguments, valid")


# ---------------------------------------------------------------------------
# 10. random-normal numerics
# ---------------------------------------------------------------------------

def _close(got, want, mag, out_bf16):
    """test_gpu_dense.py's derived bound"""
    got, want, mag = got.double().cpu(), want.double(), mag.double()
    tol = (2.0 ** -8 if out_bf16 else 1e-6) * want.abs() + 1e-5 * mag + 1e-30
    return ((got - want).abs() / tol).max().item()


@gpu_test
@pytest.mark.parametrize("c_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,K,req", [(130, 72, 129, 1), (65, 65, 1093, 5)])
@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_random_normal_product(gpu, lay, M, N, K, req, c_f32):
    """Standard-normal bf16 operands against fp64 on the same operands, one shape
    in one slice, one split."""
    a_col, b_col = LAYOUTS[lay]
    rng = np.random.default_rng([10, M, N, K])
    Av = torch.from_numpy(rng.standard_normal((M, K))).to(BF16).double()
    Bv = torch.from_numpy(rng.standard_normal((N, K))).to(BF16).double()
    A, B = _operand(Av, a_col, gpu), _operand(Bv, b_col, gpu)
    C = _Guarded(M, _r8(N) + 8, F32 if c_f32 else BF16, SENT).up(gpu)
    wsbuf, ws, used = _workspace(M, N, K, req, gpu, False)
    assert (_plan(K, req)[1] > 1) == (req > 1)
    _Job(M, N, K, A.t, a_col, B.t, b_col, C.t[:, :N], split=req, ws=ws).run()
    worst = _close(C.t[:, :N], Av @ Bv.T, Av.abs() @ Bv.abs().T, not c_f32)
    assert worst <= 1.0, worst
    got = C.dev.cpu()
    C.host.copy_(got)
    C.win()[:, :N] = SENT
    C.win()[:, N:_r8(N)] = SENT
    assert torch.all(C.win(got)[:, N:_r8(N)] == 0) and torch.all(C.host == SENT)
    _check_ws(wsbuf, ws, used)


@gpu_test
@pytest.mark.parametrize("kind", [0, 1], ids=["rowtr", "tower"])
def test_random_normal_fused_sgd(gpu, kind):
    """One fused-SGD update on standard-normal operands: the master within
    lr * 1e-5 * sum|a b| + 2^-23 |w| of fp64, the images bitwise the RNE of the
    GPU's master."""
    n_out, n_in = 33, 45
    u = _Update(gpu, n_out, n_in, 200, 3, kind, True, seed=11, normal=True)
    o = u.outputs()
    o["job"].run()
    W = o["W"].t[:, :n_in].cpu()
    b = o["b"].t[0].cpu()
    for got, old, grad, mag in ((W, u.W0, u.dW, u.mag_w), (b, u.b0, u.db, u.mag_b)):
        want = old - LR * grad
        tol = LR * 1e-5 * mag + 2.0 ** -23 * want.abs() + 1e-30
        assert ((got.double() - want).abs() <= tol).all(), ((got.double() - want).abs() / tol).max()
    o["W"].win()[:, :n_in] = W
    o["b"].win()[0] = b
    u.expect_images(o, W.to(BF16))
    u.check(o)
