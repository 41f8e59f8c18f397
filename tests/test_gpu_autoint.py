"""The fused AutoInt interacting layers on the GPU (mrec_autoint_fwd / _bwd, csrc/autoint.hip).

Shapes.  The kernels give one wave a sample and one 32-row tile to its m fields, walk the
batch W = 4, 3 or 2 samples per workgroup (by the LDS the shape needs), take d_in in 16-wide k
steps (d_in = 8 is half a step), project onto 4 A image rows in 32-column tiles (A = 16 shares
a tile between res | q and k | v), run the scores in head_dim-wide k steps (8 is half a step,
32 two steps) and give a 32-column output tile to 32 / head_dim heads.  Hence m in {2, 16, 17,
26, 32} (the tile's edge, odd, full), B in {1, 3, 5, 70} (less than one workgroup, a ragged
last one, many), every d_in, and (A, head_dim) in {(16, 8), (32, 32), (64, 32), (64, 8)}: a
shared projection tile, one head per tile, two tiles, and four heads per tile in two tiles.
The weight gradient gives a workgroup ceil(B / parts) samples: B = 70 has parts of 4 and 2.

1. exact: integer and dyadic operands for which every rounding point of the contract holds
   its value exactly, so the expected values are plain fp64 arithmetic and the comparison is
   ``torch.equal``;
2. Gaussian operands against fp64 on the bf16-rounded inputs, by the project's yardstick;
3. memory discipline; 4. determinism; 5. dispatch; 6. the empty batch; 7. the model.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from test_autoint_cpu import (RefAutoInt, autoint, autoint_linears, copy_into_ref, named_pairs, stack_case)
from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
F64 = torch.float64
KERNELS = {"mrec_autoint_fwd", "mrec_autoint_bwd"}
SHAPES = [(16, 8), (32, 32), (64, 32), (64, 8)]  # (A, head_dim)


def _r8(v):
    return (v + 7) // 8 * 8


def padded(t, dtype, gpu, extra_rows=0, extra_cols=0, fill=float("nan")):
    """t [B, C] as a [B, C] view of a [B + extra_rows, r8(C) + extra_cols] device buffer whose
    other elements hold ``fill`` (rows 16-byte aligned) -> (buffer, view)."""
    B, C = t.shape
    buf = torch.full((B + extra_rows, _r8(C) + extra_cols), fill, dtype=dtype, device=gpu)
    buf[:B, :C] = t.to(gpu).to(dtype)
    return buf, buf[:B, :C]


def raw_layer(x, layer, heads, scale, dy, y_dtype, dx_dtype, wide=False, sent=7.0, batch=None, y=None):
    """One layer through the library calls on test-owned buffers.  x [B, m * d_in] and dy
    [B, m * A] are device views (any strides the contract allows); ``wide`` puts every output,
    dw and the workspace inside a larger buffer filled with ``sent``.  -> dict of views (y, dx,
    dw) and of whole buffers (bufs)."""
    from pytorchrec_amd import _mrec, dense
    gpu = x.device
    A, d_in = layer[0].shape
    m = x.shape[1] // d_in
    B = x.shape[0]
    nb = B if batch is None else batch
    er, ec = (3, 8) if wide else (0, 0)
    lib, st = _mrec.lib(), _mrec.stream_handle()
    bufs = {}

    def out(name, rows, cols, dtype):
        buf, view = padded(torch.full((rows, cols), sent), dtype, gpu, er, ec, fill=sent)
        bufs[name] = (buf, rows, cols)
        return view

    wf, wb = dense.autoint_images(*layer)
    if y is None:
        y = out("y", B, m * A, y_dtype)
    a = _mrec.AutoIntArgs()
    a.x, a.x_dtype, a.ld_x = x.data_ptr(), _mrec.dtype_code(x.dtype), x.stride(0)
    a.w_fwd, a.ld_w_fwd, a.w_bwd, a.ld_w_bwd = wf.data_ptr(), wf.stride(0), wb.data_ptr(), wb.stride(0)
    a.has_res, a.batch, a.n_fields, a.d_in = int(layer[3] is not None), nb, m, d_in
    a.heads, a.head_dim, a.A, a.scale = heads, A // heads, A, float(scale)
    a.y, a.y_dtype, a.ld_y = y.data_ptr(), _mrec.dtype_code(y.dtype), y.stride(0)
    _mrec.call("mrec_autoint_fwd", ctypes.byref(a), st)
    res = {"y": y, "bufs": bufs, "keep": (wf, wb)}
    if dy is None:
        return res
    dx = out("dx", B, m * d_in, dx_dtype)
    n = (4 if layer[3] is not None else 3) * A * d_in
    flat = torch.full((n + 64,), sent, dtype=F32, device=gpu)  # dw with 32 guard floats each side
    bufs["dw"] = (flat, n)
    nws = int(lib.mrec_autoint_bwd_workspace_size(nb, d_in, A))
    ws = torch.full((nws + 256,), 0x5a, dtype=torch.uint8, device=gpu)  # 128 guard bytes each side
    bufs["ws"] = (ws, nws)
    a.dy, a.dy_dtype, a.ld_dy = dy.data_ptr(), _mrec.dtype_code(dy.dtype), dy.stride(0)
    a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), _mrec.dtype_code(dx.dtype), dx.stride(0)
    a.dw, a.workspace, a.workspace_bytes = flat.data_ptr() + 4 * 32, ws.data_ptr() + 128, nws
    _mrec.call("mrec_autoint_bwd", ctypes.byref(a), st)
    res.update(dx=dx, dw=flat[32:32 + n].view(-1, A, d_in))
    return res


def fused(x0, layers, heads, scale, dy, x_dtype=None):
    """dense.autoint forward + backward on device tensors -> (y, dx0, [dW per weight])."""
    from pytorchrec_amd import dense
    d_in = layers[0][0].shape[1]
    x = x0.detach().requires_grad_()
    L = [tuple(None if w is None else w.detach().clone().requires_grad_() for w in l) for l in layers]
    y = dense.autoint(x, x0.shape[1] // d_in, L, heads, scale, x_dtype=x_dtype)
    y.backward(dy)
    return y.detach(), x.grad, [w.grad for l in L for w in l if w is not None]


def _spy(monkeypatch):
    """Every libmrec call by name."""
    from pytorchrec_amd import _mrec
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def to_gpu(layers, gpu):
    return [tuple(None if w is None else w.to(gpu) for w in l) for l in layers]


# ---------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------

def holds_bf16(t):
    return torch.equal(t.float().bfloat16().double(), t)


def exact_reference(X, layer, heads, scale, dY):
    """The contract in fp64 for operands the exact families build: a softmax row is its ties'
    indicator over their count (asserted: every other key lies >= 128 below the maximum, where
    fp32's exp is 0).  Asserts that every rounding point holds its value exactly.
    -> (Y, dX, dW [4 or 3, A, d_in], tie counts)."""
    Wq, Wk, Wv, Wres = layer
    B, m, _ = X.shape
    A = Wq.shape[0]
    hd = A // heads
    Q, K, V = X @ Wq.T, X @ Wk.T, X @ Wv.T
    O = torch.zeros(B, m, A, dtype=F64)
    Ps, ties = [], []
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        S = scale * Q[:, :, c] @ K[:, :, c].transpose(1, 2)
        top = S.max(-1, keepdim=True).values
        hit = S == top
        assert bool(((S <= top - 128) | hit).all()), "a key lies within 128 of the maximum"
        P = hit.double() / hit.sum(-1, keepdim=True)
        ties.append(hit.sum(-1))
        Ps.append(P)
        O[:, :, c] = P @ V[:, :, c]
    Y = torch.relu(O + (X @ Wres.T if Wres is not None else 0))
    dZ = dY * (Y > 0)
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    dSs = []
    for h, P in enumerate(Ps):
        c = slice(h * hd, (h + 1) * hd)
        dV[:, :, c] = P.transpose(1, 2) @ dZ[:, :, c]
        dP = dZ[:, :, c] @ V[:, :, c].transpose(1, 2)
        dS = scale * (P * (dP - (dP * P).sum(-1, keepdim=True)))
        dSs.append(dS)
        dQ[:, :, c] = dS @ K[:, :, c]
        dK[:, :, c] = dS.transpose(1, 2) @ Q[:, :, c]
    dX = dQ @ Wq + dK @ Wk + dV @ Wv + (dZ @ Wres if Wres is not None else 0)
    gs = [dQ, dK, dV] + ([dZ] if Wres is not None else [])
    dW = torch.stack([torch.einsum("bia,bid->ad", g, X) for g in gs])
    for name, t in (("X", X), ("Q", Q), ("K", K), ("V", V), ("P", torch.stack(Ps)), ("Y", Y), ("dY", dY),
                    ("dS", torch.stack(dSs)), ("dQ", dQ), ("dK", dK), ("dV", dV), ("dX", dX),
                    *[(f"W{k}", w) for k, w in enumerate(layer) if w is not None]):
        assert holds_bf16(t), f"{name} is not exact in bf16"
    for name, t in (("O", O), ("dW", dW)):  # fp32 sums of dyadics far below 2^24 units
        assert torch.equal(t.float().double(), t) and float(t.abs().max()) < 2 ** 12, name
    return Y, dX, dW, torch.stack(ties)


def _sparse_rows(g, rows, cols, allowed, nnz, values=(-1, 1)):
    """[rows, cols] with ``nnz`` entries from ``values`` per row, in the ``allowed`` columns."""
    W = torch.zeros(rows, cols, dtype=F64)
    allowed = torch.as_tensor(allowed)
    for r in range(rows):
        pick = allowed[torch.randperm(len(allowed), generator=g)[:nnz]]
        W[r, pick] = torch.tensor(values, dtype=F64)[torch.randint(len(values), (len(pick),), generator=g)]
    return W


def _sparse_dy(g, B, m, A, heads, must=None):
    """dY with at most three non-zero fields per sample (one when more than two heads share the
    key columns; field ``must[b]`` among them) and one +-1 per head in them, so that the sums
    over the queries and the heads stay short."""
    hd = A // heads
    dY = torch.zeros(B, m, A, dtype=F64)
    for b in range(B):
        rows = torch.randperm(m, generator=g)[:3 if heads <= 2 else 1].tolist()
        if must is not None:
            rows[0] = int(must[b])
        for i in rows:
            for h in range(heads):
                c = h * hd + int(torch.randint(hd, (1,), generator=g))
                dY[b, i, c] = 1.0 if int(torch.randint(2, (1,), generator=g)) else -1.0
    return dY


def uniform_case(B, m, d_in, A, hd, seed, zero):
    """Wq = 0 (``zero`` = "q") or Wk = 0 ("k"): every score is 0 and every probability exactly
    1 / m (m a power of two).  The other of the two reads ONE field's columns only (every other
    field's are 0 there), so that dQ (resp. dK) is one product per element."""
    g = torch.Generator().manual_seed(seed)
    heads = A // hd
    half = d_in // 2
    X = torch.randint(-1, 2, (B, m, d_in), generator=g).double()
    X[:, :, :half] = 0
    one = torch.randint(m, (B,), generator=g)
    X[torch.arange(B), one, :half] = torch.randint(0, 2, (B, half), generator=g).double() * 2 - 1
    Wa = _sparse_rows(g, A, d_in, range(half), 1, values=(-2, -1, 1, 2))
    Wv = _sparse_rows(g, A, d_in, range(half, d_in), min(2, d_in - half))
    Wres = _sparse_rows(g, A, d_in, range(d_in), 2)
    Z = torch.zeros(A, d_in, dtype=F64)
    layer = (Z, Wa, Wv, Wres) if zero == "q" else (Wa, Z, Wv, Wres)
    return X, layer, heads, 1.0, _sparse_dy(g, B, m, A, heads, must=one)


def selecting_case(B, m, d_in, A, hd, seed, res=True):
    """scale = 128 and integer operands: a query's maximum is reached by exactly 1, 2 or 4 keys
    and every other key has probability exactly 0.  Column 0 of X is the query column (+-1,
    +-2), columns 1 and 2 are key columns whose largest value (3) and smallest (-3) are each
    taken by 1, 2 or 4 fields per sample; head h reads key column 1 + h % 2 and the query column
    with a sign that changes with h // 2, so a head selects the top or the bottom group.  Wv
    reads the other columns only: tied keys agree in K and differ in V."""
    g = torch.Generator().manual_seed(seed)
    heads = A // hd
    X = torch.randint(-1, 2, (B, m, d_in), generator=g).double()
    X[:, :, 0] = (torch.randint(0, 2, (B, m), generator=g) * 2 - 1) * torch.randint(1, 3, (B, m), generator=g)
    for b in range(B):
        for kc in (1, 2):
            col = torch.randint(-2, 3, (m,), generator=g).double()
            if m == 2:
                t1 = t2 = 1
            else:
                t1 = (1, 2, 4)[int(torch.randint(3, (1,), generator=g))]
                t2 = (1, 2, 4)[int(torch.randint(3, (1,), generator=g))]
                while t1 + t2 > m:
                    t1, t2 = max(1, t1 // 2), max(1, t2 // 2)
            order = torch.randperm(m, generator=g)
            col[order[:t1]] = 3.0
            col[order[t1:t1 + t2]] = -3.0
            X[b, :, kc] = col
    Wq, Wk = torch.zeros(A, d_in, dtype=F64), torch.zeros(A, d_in, dtype=F64)
    for h in range(heads):
        Wq[h * hd, 0] = (1.0, -1.0)[(h // 2) % 2]
        Wk[h * hd, 1 + h % 2] = 1.0
    Wv = _sparse_rows(g, A, d_in, range(3, d_in), 2)
    Wres = _sparse_rows(g, A, d_in, range(d_in), 2) if res else None
    return X, (Wq, Wk, Wv, Wres), heads, 128.0, _sparse_dy(g, B, m, A, heads)


NONZERO = {}


def check_exact(gpu, case, combos, wide=False):
    X, layer, heads, scale, dY = case
    B, m, d_in = X.shape
    A = layer[0].shape[0]
    Y, dX, dW, ties = exact_reference(X, layer, heads, scale, dY)
    assert set(ties.unique().tolist()) <= ({1, 2, 4} if scale == 128.0 else {m})
    dev = tuple(None if w is None else w.float().to(gpu) for w in layer)
    for name, t in (("dX", dX), *zip(("dWq", "dWk", "dWv", "dWres"), dW)):
        NONZERO[name] = NONZERO.get(name, False) or bool((t != 0).any())
    for xd, yd, dyd, dxd in combos:
        _, x = padded(X.reshape(B, -1), xd, gpu, 1, 8)
        _, dy = padded(dY.reshape(B, -1), dyd, gpu, 1, 8)
        r = raw_layer(x, dev, heads, scale, dy, yd, dxd, wide=wide)
        tag = f"x {xd} y {yd} dy {dyd} dx {dxd}"
        assert torch.equal(r["y"].double().cpu(), Y.reshape(B, -1)), "y, " + tag
        assert torch.equal(r["dx"].double().cpu(), dX.reshape(B, -1)), "dx, " + tag
        assert torch.equal(r["dw"].double().cpu(), dW), "dw, " + tag
    return ties


ALL_COMBOS = list(itertools.product((F32, BF), repeat=4))  # x, y, dy, dx
TWO_COMBOS = [(F32, BF, F32, BF), (BF, F32, BF, F32)]


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("m", [2, 16, 32])
def test_exact_uniform_attention(gpu, m, zero):
    """P = 1 / m exactly; Wq = 0 leaves dQ (and dWq) as the softmax's only gradient, Wk = 0 dK."""
    for k, (d_in, (A, hd)) in enumerate(zip((8, 16, 32, 64), SHAPES)):
        case = uniform_case(5, m, d_in, A, hd, 100 * m + k, zero)
        check_exact(gpu, case, ALL_COMBOS if k == 1 else TWO_COMBOS)
    dX, dW = exact_reference(*case)[1:3]
    assert bool((dW[0 if zero == "q" else 1] != 0).any()) and not bool((dW[1 if zero == "q" else 0] != 0).any())


@pytest.mark.parametrize("d_in,A,hd", [(8, 16, 8), (16, 32, 32), (16, 64, 32), (32, 64, 8), (64, 64, 32)])
@pytest.mark.parametrize("m", [2, 17, 26])
def test_exact_selecting_attention(gpu, m, d_in, A, hd):
    """Ties of 1, 2 and 4 keys with different values: the gradient through the softmax is not
    zero, and a probability is 0, 1/4, 1/2 or 1."""
    seen = set()
    for B in (1, 3, 5, 70):
        case = selecting_case(B, m, d_in, A, hd, 7 * m + B, res=B != 3)
        ties = check_exact(gpu, case, ALL_COMBOS if (B == 5 and d_in == 16) else TWO_COMBOS[B % 2:][:1])
        seen |= set(ties.unique().tolist())
    assert seen == ({1} if m == 2 else {1, 2, 4})


def test_exact_cases_reach_every_gradient(gpu):
    """Across the families each of dX, dWq, dWk, dWv and dWres has non-zero entries."""
    check_exact(gpu, uniform_case(5, 16, 16, 32, 32, 1, "q"), TWO_COMBOS[:1])
    check_exact(gpu, uniform_case(5, 16, 16, 32, 32, 2, "k"), TWO_COMBOS[:1])
    check_exact(gpu, selecting_case(5, 17, 16, 32, 32, 3), TWO_COMBOS[:1])
    assert all(NONZERO.get(k) for k in ("dX", "dWq", "dWk", "dWv", "dWres")), NONZERO


# ---------------------------------------------------------------------------
# 2. Gaussian operands, per layer on the kernels' own inputs
# ---------------------------------------------------------------------------

def rb64(t):
    return t.float().bfloat16().double()


def yardstick(got, cmp, want, what, worst):
    """The kernels' distance to fp64 is at most 1.5x the comparator's plus 1 % of the quantity,
    in L2 and in max norm."""
    got, cmp, want = got.double().cpu(), cmp.double().cpu(), want.double().cpu()
    for kind, norm in (("L2", lambda t: float(t.norm())), ("max", lambda t: float(t.abs().max()))):
        eg, ec, n = norm(got - want), norm(cmp - want), norm(want)
        bound = 1.5 * ec + 0.01 * n
        worst.append(eg / bound if bound else 0.0)
        print(f"{what} {kind}: kernels {eg / n:.3e}, comparator {ec / n:.3e} of the quantity; "
              f"{eg / bound if bound else 0.0:.3f} of the bound")
        assert eg <= bound, (what, kind, eg / n, ec / n)


GAUSS_CASES = [(1, 2, 8, 16, 8, 1), (3, 17, 16, 32, 32, 2), (70, 26, 16, 64, 32, 3), (5, 32, 64, 64, 8, 2),
               (5, 16, 32, 64, 32, 1), (70, 26, 8, 16, 8, 2)]


@pytest.mark.parametrize("act", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,m,d_in,A,hd,nl", GAUSS_CASES)
def test_gaussian_against_fp64_by_the_comparator_yardstick(gpu, B, m, d_in, A, hd, nl, act):
    """A bound through the softmax that is tight needs the scores' spread per row, which the
    rounding contract does not give; so the project's yardstick: per layer, on the kernel's
    own input x (and its own y for the ReLU mask), fp64 on the bf16-rounded x, weights and dy
    is the truth, ``cpu_path.autoint(round_bf16=True)`` on the GPU the comparator."""
    from pytorchrec_amd import cpu_path
    heads = A // hd
    x0, layers, dy = stack_case(B, m, d_in, [A] * nl, 50 + B + m, res=nl != 2, dtype=F32, w_scale=1.5)
    layers = to_gpu(layers, gpu)
    worst = []
    x = padded(x0, act, gpu)[1]
    for k, layer in enumerate(layers):
        g = padded(torch.randn(B, m * A, generator=torch.Generator().manual_seed(k)), act, gpu)[1]
        r = raw_layer(x, layer, heads, 0.5, g, act, act)
        ins = lambda dt, rnd: (rnd(x).to(dt).requires_grad_(),  # noqa: E731
                               [tuple(None if w is None else rnd(w).to(dt).requires_grad_() for w in layer)])
        xt, Lt = ins(F64, lambda t: t.detach().bfloat16())
        yt = cpu_path.autoint(xt, Lt, heads, 0.5)
        yt.backward(rb64(g))
        xc, Lc = ins(F32, lambda t: t.detach())
        yc = cpu_path.autoint(xc, Lc, heads, 0.5, round_bf16=True, x_dtype=act)
        yc.backward(g.to(yc.dtype))
        tag = f"layer {k + 1}"
        yardstick(r["y"], yc.detach(), yt.detach(), tag + " y", worst)
        yardstick(r["dx"], xc.grad, xt.grad, tag + " dx", worst)
        flat = lambda L: [w for w in L[0] if w is not None]  # noqa: E731
        for j, (wc, wt) in enumerate(zip(flat(Lc), flat(Lt))):
            yardstick(r["dw"][j], wc.grad, wt.grad, tag + " dW" + "qkvr"[j], worst)
        x = r["y"]
    print(f"worst observed fraction of the bound: {max(worst):.3f}")


# ---------------------------------------------------------------------------
# 3. memory discipline
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,d_in,A,hd", [(2, 8, 16, 8), (26, 16, 64, 32), (17, 64, 64, 8), (31, 32, 32, 32)])
def test_strides_nan_pads_and_sentinels(gpu, m, d_in, A, hd, dtype):
    """x, dy and y live in wider buffers with NaN in every pad column and spare row; every
    output, dw and the workspace sit between sentinels.  m < 32: a pad key leaking into a
    softmax, or a NaN read past a row, shows in the values."""
    B, heads = 7, A // hd
    x0, layers, dy = stack_case(B, m, d_in, [A], 9, dtype=F32)
    layer = to_gpu(layers, gpu)[0]
    xbuf, x = padded(x0, dtype, gpu, 2, 24)
    dbuf, g = padded(dy, dtype, gpu, 2, 16)
    r = raw_layer(x, layer, heads, 0.5, g, dtype, dtype, wide=True, sent=7.0)
    tight = raw_layer(padded(x0, dtype, gpu)[1], layer, heads, 0.5, padded(dy, dtype, gpu)[1], dtype, dtype)
    for name in ("y", "dx", "dw"):
        assert bool(torch.isfinite(r[name].float()).all()), name
        assert torch.equal(r[name], tight[name]), name
    for name in ("y", "dx"):
        buf, rows, cols = r["bufs"][name]
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:rows, :cols] = False
        assert bool((buf[mask] == 7.0).all()), f"{name}: wrote outside its rows"
    flat, n = r["bufs"]["dw"]
    assert bool((flat[:32] == 7.0).all()) and bool((flat[32 + n:] == 7.0).all()), "dw guards"
    ws, nws = r["bufs"]["ws"]
    assert bool((ws[:128] == 0x5a).all()) and bool((ws[128 + nws:] == 0x5a).all()), "workspace guards"
    assert bool(torch.isnan(xbuf[:, m * d_in:].float()).all()) and bool(torch.isnan(dbuf[B:].float()).all())
    # batch smaller than the buffers: rows >= batch are untouched
    part = raw_layer(x, layer, heads, 0.5, g, dtype, dtype, wide=True, sent=7.0, batch=4)
    for name in ("y", "dx"):
        assert torch.equal(part[name][:4], r[name][:4]) and bool((part[name][4:] == 7.0).all()), name


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,d_in,A,hd", [(26, 16, 64, 32), (9, 64, 64, 8), (32, 8, 16, 8)])
def test_bits_do_not_depend_on_run_or_position(gpu, m, d_in, A, hd, dtype):
    B, heads = 70, A // hd
    x0, layers, dy = stack_case(B, m, d_in, [A], 12, dtype=F32)
    layer = to_gpu(layers, gpu)[0]
    x, g = padded(x0, dtype, gpu)[1], padded(dy, dtype, gpu)[1]
    a = raw_layer(x, layer, heads, 0.5, g, dtype, dtype)
    b = raw_layer(x, layer, heads, 0.5, g, dtype, dtype)
    for name in ("y", "dx", "dw"):
        assert torch.equal(a[name], b[name]), name + " differs from run to run"
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
    big_x = torch.cat([x0[perm], x0[:9]])
    big_g = torch.cat([dy[perm], dy[:9]])
    c = raw_layer(padded(big_x, dtype, gpu)[1], layer, heads, 0.5, padded(big_g, dtype, gpu)[1], dtype, dtype)
    for name in ("y", "dx"):
        assert torch.equal(c[name][:B], a[name][perm.to(gpu)]), name + " depends on the position"
        assert torch.equal(c[name][B:], a[name][:9]), name + " depends on the batch"


# ---------------------------------------------------------------------------
# 5. dispatch, 6. the empty batch
# ---------------------------------------------------------------------------

def test_compiled_shape_runs_both_kernels_once_per_layer(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    x0, layers, dy = stack_case(9, 26, 16, [64, 64, 64], 1, dtype=F32)
    fused(x0.to(gpu).to(BF), to_gpu(layers, gpu), 2, 1.0, dy.to(gpu).to(BF))
    assert [c for c in calls if c in KERNELS] == ["mrec_autoint_fwd"] * 3 + ["mrec_autoint_bwd"] * 3


@pytest.mark.parametrize("how", ["switch", "m33", "A24"])
def test_the_switch_and_unsupported_shapes_take_the_torch_ops(gpu, monkeypatch, how):
    from pytorchrec_amd import cpu_path, dense
    m, d_in, A = {"switch": (26, 16, 64), "m33": (33, 8, 16), "A24": (5, 8, 24)}[how]
    if how == "switch":
        monkeypatch.setattr(dense, "AUTOINT_FUSED", False)
    else:
        assert dense.AUTOINT_FUSED and not dense.autoint_supported(m, d_in, [A], 2)
    x0, layers, dy = stack_case(9, m, d_in, [A], 2, dtype=F32)
    layers = to_gpu(layers, gpu)
    calls = _spy(monkeypatch)
    y, dx, dws = fused(x0.to(gpu), layers, 2, 0.5, dy.to(gpu))
    assert not KERNELS & set(calls)
    x = x0.to(gpu).requires_grad_()
    L = [tuple(w.detach().clone().requires_grad_() for w in layers[0])]
    want = cpu_path.autoint(x, L, 2, 0.5, round_bf16=True)
    want.backward(dy.to(gpu))
    assert torch.equal(y, want.detach()) and torch.equal(dx, x.grad)
    for a, b in zip(dws, L[0]):
        assert torch.equal(a, b.grad)


def test_empty_batch(gpu, monkeypatch):
    from pytorchrec_amd import dense
    _, layers, _ = stack_case(1, 26, 16, [64, 64], 3, dtype=F32)
    layers = to_gpu(layers, gpu)
    assert dense.autoint_supported(26, 16, [64, 64], 2, BF)
    calls = _spy(monkeypatch)
    y, dx, dws = fused(torch.zeros(0, 26 * 16, dtype=BF, device=gpu), layers, 2, 1.0,
                       torch.zeros(0, 26 * 64, dtype=BF, device=gpu))
    assert tuple(y.shape) == (0, 26 * 64) and tuple(dx.shape) == (0, 26 * 16) and y.dtype == BF
    assert len(dws) == 8 and all(tuple(g.shape) == tuple(w.shape) and not bool(g.any())
                                 for g, w in zip(dws, [w for l in layers for w in l]))
    assert not KERNELS & set(calls)
    # the library itself: batch = 0 launches nothing and touches no buffer
    x = torch.zeros(4, 26 * 16, dtype=BF, device=gpu)
    r = raw_layer(x, layers[0], 2, 1.0, torch.zeros(4, 26 * 64, dtype=BF, device=gpu), BF, BF, wide=True,
                  sent=7.0, batch=0)
    assert bool((r["bufs"]["y"][0] == 7.0).all()) and bool((r["bufs"]["dx"][0] == 7.0).all())
    assert bool((r["bufs"]["dw"][0] == 7.0).all())


# ---------------------------------------------------------------------------
# 7. the model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("emb_dtype", [F32, BF], ids=["fp32", "bf16"])
def test_autoint_train_step_matches_the_fp64_model(gpu, monkeypatch, emb_dtype):
    """One AutoInt train step (B = 256, 6 fields of 50 rows, 3 dense, D = 16, two layers of
    2 x 8, layers [64, 32], BCEWithLogitsLoss, plain SGD) against RefAutoInt in fp64 from
    identical weights: the loss within 2e-3 and every parameter's UPDATE, the attention
    projections and att_out included.  The yardstick is
    test_xdeepfm_train_step_matches_the_fp64_model's: the same model in torch fp32 with bf16
    rounding at the build's storage points (RefAutoInt(bf16_points=True), run here on the GPU)
    says what bf16 storage alone costs, and the kernels' distance to fp64 may not exceed 1.5x
    that plus 1 % of the update, in L2 and in max norm.  Tables fp32 and bf16 (RNE, lr 1e4 so
    that the table updates are many bf16 ulps and the emulation's tables are rounded the same
    way)."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    bf16 = emb_dtype == BF
    B, lr = 256, (1e4 if bf16 else 1.0)
    nums, nd, D, layers = [50] * 6, 3, 16, (64, 32)
    m = autoint(rows=50, F=6, n_dense=nd, D=D, att_layers=2, heads=2, head_dim=8, layers=layers, device=gpu,
                emb_dtype=emb_dtype, random_seed=2020)
    m.embeddings.stochastic_rounding = False
    with torch.no_grad():  # weights large enough that every part matters
        for lin in autoint_linears(m):
            lin.weight.mul_(10.0)
            lin.bias.mul_(10.0)
        for l in m.att:
            for w in l.weights():
                w.mul_(30.0)
        m.att_out.weight.mul_(30.0)
        m.embeddings.weight.mul_(30.0)
    assert m.embeddings.weight.dtype == emb_dtype
    r = RefAutoInt(nums, nd, D, 2, 2, 8, layers)
    copy_into_ref(m, r)
    data, ids, dense, label = ctr_batch(m, B)
    data = {k: v.to(gpu) for k, v in data.items()}
    before_state = [v.clone() for v in r.state_dict().values()]
    before = [b.detach().clone() for _, _, b in named_pairs(m, r)]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], gpu)
    assert m.embeddings.update == "sgd"
    calls = _spy(monkeypatch)
    loss = float(m.train_step(data)["loss"].detach())
    for name in ("mrec_interact_fwd_ex", "mrec_autoint_fwd", "mrec_autoint_bwd", "mrec_tower_fwd_bwd"):
        assert name in calls, (name, calls)
    assert calls.count("mrec_autoint_fwd") == 2 == calls.count("mrec_autoint_bwd")
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    print(f"loss {loss:.6f} against {rloss:.6f}")
    assert abs(loss - rloss) <= 2e-3 * max(1.0, abs(rloss)), (loss, rloss)
    e = RefAutoInt(nums, nd, D, 2, 2, 8, layers, dtype=torch.float32, bf16_points=True)
    e.load_state_dict(dict(zip(e.state_dict(), before_state)))
    e = e.to(gpu)
    ref_train_step(e, lr, ids.to(gpu), dense.to(gpu), label.to(gpu))

    def upd_close(got_after, emu_after, want_after, before, name):
        dg = got_after.double().cpu() - before
        de = emu_after.double().cpu() - before
        dw = want_after.double() - before
        assert float(dw.abs().max()) > 0, name
        for kind, norm in (("L2", lambda t: float(t.norm())), ("max", lambda t: float(t.abs().max()))):
            eg, ee = norm(dg - dw), norm(de - dw)
            print(f"{name} {kind}: kernels {eg / norm(dw):.3e}, emulation {ee / norm(dw):.3e} of the update")
            assert eg <= 1.5 * ee + 0.01 * norm(dw), (name, kind, eg / norm(dw), ee / norm(dw))

    in_bank = lambda name: name.startswith("table") or (name[0] == "w" and name[1:].isdigit())  # noqa: E731
    for (name, got, want), (_, _, emu), old in zip(named_pairs(m, r), named_pairs(m, e), before):
        emu = emu.detach().to(BF) if (bf16 and in_bank(name)) else emu.detach()
        upd_close(got.detach(), emu, want.detach(), old, name)
