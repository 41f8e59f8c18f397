"""GPU checks of the fused Compressed Interaction Network (mrec_cin_fwd / mrec_cin_bwd,
csrc/cin.hip) and of ``XDeepFM`` on cuda:0.

Shapes are the smallest at which the kernels can go wrong: B in {1, 3, 5, 70} (a wave carries
64 / D samples, a workgroup four waves), m in {2, 8, 9, 26, 32} fields (the fewest; either side
of the 8 fields a half-wave holds, at the field pitch 16; Criteo, at the pitch 32; the full
pitch), H from {8, 24, 200, 256}
(one column tile with a pad; 7 tiles and the 13-step backward; 8 tiles, which are two forward
launches), D in {8, 16, 32, 64} (8, 4, 2, 1 samples per wave), 1 to 3 layers.  The fp64
oracle's Z stays under 50 MB per case.

1. exact: operands, W and dp from {-1, 0, 1}, W sparse; every intermediate is an integer its
   dtype holds, so X^k, p, dX^0 and dW equal the int64 computation bit for bit;
2. Gaussian operands against fp64 on the bf16-rounded operands, layer by layer on the kernels'
   own inputs, with a bound derived from the rounding contract;
3. memory discipline: strides, NaN pads, sentinels;
4. determinism: run to run (dW included), and under a move of the samples inside a larger batch;
5. dispatch: the kernels run for compiled shapes only, and the switch turns them off;
6. the empty batch;
7. one ``XDeepFM.train_step`` against the same model in torch fp64, by the yardstick of
   ``test_dlrm_train_step_matches_the_fp64_model``.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step
from test_xdeepfm_cpu import RefXDeepFM, copy_into_ref, named_pairs, xdeepfm, xdeepfm_linears

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
U24, U8 = 2.0 ** -24, 2.0 ** -8
DTYPE_COMBOS = list(itertools.product((F32, BF), repeat=2))  # x0, X^k


def _r8(v):
    return (v + 7) // 8 * 8


def padded(t, dtype, gpu, extra_rows=0, extra_cols=0, fill=float("nan")):
    """t [B, C] as a [B, C] view of a [B + extra_rows, r8(C) + extra_cols] device buffer whose
    other elements hold ``fill`` (rows 16-byte aligned) -> (buffer, view)."""
    B, C = t.shape
    buf = torch.full((B + extra_rows, _r8(C) + extra_cols), fill, dtype=dtype, device=gpu)
    buf[:B, :C] = t.to(gpu).to(dtype)
    return buf, buf[:B, :C]


def widths_of(m, widths):
    return [m, *widths]


def raw_cin(x0, ws, dp, x_dtype, wide=False, sent=7.0, batch=None, fresh_dx0=False):
    """The library calls of all layers on test-owned buffers: forward bottom up, backward top
    down, as ``dense._CinFn`` issues them.  x0 [B, m * D] and dp [B, sum H] are device views
    (any strides the contract allows); ``wide`` puts every output inside a larger buffer filled
    with ``sent``.  ``fresh_dx0`` gives every layer's backward its own zeroed dX^0 accumulator.
    -> dict of views (xs, p, dxps, dx0 or dx0s, dws) and of whole buffers (bufs)."""
    from pytorchrec_amd import _mrec, dense
    gpu = x0.device
    m = ws[0].shape[2]
    B, D = x0.shape[0], x0.shape[1] // m
    nb = B if batch is None else batch
    er, ec = (3, 8) if wide else (0, 0)
    hs = widths_of(m, [w.shape[0] for w in ws])
    offs = np.concatenate([[0], np.cumsum(hs[1:])]).astype(int)
    st = _mrec.stream_handle()
    bufs = {}

    def out(name, rows, cols, dtype, zero=False):
        buf, view = padded(torch.full((rows, cols), 0.0 if zero else sent), dtype, gpu, er, ec, fill=sent)
        bufs[name] = (buf, rows, cols)
        return view

    p = out("p", B, int(offs[-1]), F32)
    xs, args, xp = [], [], x0
    for k, W in enumerate(ws):
        wf, wb = dense.cin_images(W)
        xk = out(f"x{k + 1}", B, hs[k + 1] * D, x_dtype)
        a = _mrec.CinArgs()
        a.x0, a.x0_dtype, a.ld_x0 = x0.data_ptr(), _mrec.dtype_code(x0.dtype), x0.stride(0)
        a.xp, a.xp_dtype, a.ld_xp = xp.data_ptr(), _mrec.dtype_code(xp.dtype), xp.stride(0)
        a.w_fwd, a.ld_w_fwd, a.w_bwd, a.ld_w_bwd = wf.data_ptr(), wf.stride(0), wb.data_ptr(), wb.stride(0)
        a.batch, a.n_fields, a.D, a.H_prev, a.H = nb, m, D, hs[k], hs[k + 1]
        a.x_dtype = _mrec.dtype_code(x_dtype)
        a.xk, a.ld_xk = xk.data_ptr(), xk.stride(0)
        a.p, a.ld_p = p.data_ptr() + 4 * int(offs[k]), p.stride(0)
        _mrec.call("mrec_cin_fwd", ctypes.byref(a), st)
        args.append((a, wf, wb))
        xs.append(xk)
        xp = xk
    res = {"xs": xs, "p": p, "bufs": bufs}
    if dp is None:
        return res
    dx0s = [out(f"dx0_{k}", B, m * D, F32, zero=True) for k in range(len(ws) if fresh_dx0 else 1)]
    dxps, dws, dxk = [None] * len(ws), [None] * len(ws), None
    for k in range(len(ws) - 1, -1, -1):
        a = args[k][0]
        if dxk is not None:
            a.dxk, a.ld_dxk = dxk.data_ptr(), dxk.stride(0)
        a.dp, a.ld_dp = dp.data_ptr() + 4 * int(offs[k]), dp.stride(0)
        if k > 0:
            a.dp_prev, a.ld_dp_prev = dp.data_ptr() + 4 * int(offs[k - 1]), dp.stride(0)
        dxp = out(f"dxp{k}", B, hs[k] * D, x_dtype if k > 0 else F32)
        a.dxp, a.dxp_dtype, a.ld_dxp = dxp.data_ptr(), _mrec.dtype_code(dxp.dtype), dxp.stride(0)
        dx0 = dx0s[k if fresh_dx0 else 0]
        a.dx0, a.ld_dx0 = dx0.data_ptr(), dx0.stride(0)
        n = hs[k + 1] * hs[k] * m
        flat = torch.full((n + 64,), sent, dtype=F32, device=gpu)  # dw with 32 guard floats each side
        bufs[f"dw{k}"] = (flat, n)
        a.dw = flat.data_ptr() + 4 * 32
        _mrec.call("mrec_cin_bwd", ctypes.byref(a), st)
        dxps[k], dws[k], dxk = dxp, flat[32:32 + n].view(hs[k + 1], hs[k], m), dxp
    res.update(dxps=dxps, dws=dws, dx0s=dx0s, dx0=dx0s[0])
    return res


def fused(x0, ws, dp, x_dtype):
    """dense.cin forward + backward on device tensors -> (p, dx0, [dW])."""
    from pytorchrec_amd import dense
    m = ws[0].shape[2]
    x = x0.detach().requires_grad_()
    w = [t.detach().clone().requires_grad_() for t in ws]
    p = dense.cin(x, m, w, x_dtype=x_dtype)
    p.backward(dp)
    return p.detach(), x.grad, [t.grad for t in w]


def _spy(monkeypatch):
    """Every libmrec call by name."""
    from pytorchrec_amd import _mrec
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


KERNELS = {"mrec_cin_fwd", "mrec_cin_bwd"}


# ---------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------

def ternary_case(B, m, D, widths, seed, nnz=2):
    """x0, dp from {-1, 0, 1}; each W^k has up to ``nnz`` entries of +-1 per output map and at
    most 32 (top layer) or 6 per input map i, so that the gradients stay small; and the int64
    results.
    -> (x0, ws, dp, xs, p, dxs, dx0, dws) with dxs[k] = dX^k as layer k + 1's backward reads it."""
    g = torch.Generator().manual_seed(seed)
    hs = widths_of(m, widths)
    x0 = torch.randint(-1, 2, (B, m * D), generator=g)
    dp = torch.randint(-1, 2, (B, sum(widths)), generator=g)
    ws = []
    for k, (hp, h) in enumerate(zip(hs[:-1], hs[1:])):
        W = torch.zeros(h, hp, m, dtype=torch.int64)
        used, cap = [0] * hp, (32 if k == len(widths) - 1 else 6)
        for r in torch.randperm(h, generator=g).tolist():
            for _ in range(nnz):
                i = int(torch.randint(0, hp, (1,), generator=g))
                if used[i] >= cap:
                    i = used.index(min(used))
                if used[i] >= cap:
                    continue
                used[i] += 1
                j = int(torch.randint(0, m, (1,), generator=g))
                W[r, i, j] = int(torch.randint(0, 2, (1,), generator=g)) * 2 - 1
        ws.append(W)
    X0 = x0.reshape(B, m, D).double()
    xs, xp = [], X0
    for W in ws:
        xp = torch.einsum("hij,bid,bjd->bhd", W.double(), xp, X0)
        xs.append(xp)
    p = torch.cat([x.sum(2) for x in xs], 1)
    offs = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    dx0 = torch.zeros_like(X0)
    dxs, dws, dxk = [None] * len(ws), [None] * len(ws), None
    for k in range(len(ws) - 1, -1, -1):
        gk = dp[:, offs[k]:offs[k + 1]].double().unsqueeze(2).expand(B, widths[k], D)
        gk = gk if dxk is None else dxk + gk
        dxs[k] = gk
        xpk = X0 if k == 0 else xs[k - 1]
        Wd = ws[k].double()
        dws[k] = torch.einsum("bhd,bid,bjd->hij", gk, xpk, X0)
        dx0 += torch.einsum("bhd,hij,bid->bjd", gk, Wd, xpk)
        dxk = torch.einsum("bhd,hij,bjd->bid", gk, Wd, X0)
    dx0 += dxk
    # every intermediate is an integer bf16 holds (|v| <= 256); sums stay exact in fp32
    for t in (*xs, *dxs, dxk, dx0):
        assert float(t.abs().max()) <= 256, float(t.abs().max())
    for t in (p, *dws):
        assert float(t.abs().max()) < 2 ** 24
    lng = lambda t: t.long()  # noqa: E731
    return x0, ws, dp, [lng(x) for x in xs], lng(p), dxs, lng(dx0.reshape(B, m * D)), [lng(w) for w in dws]


EXACT_CASES = [  # m, D, widths
    (2, 8, [8]), (8, 16, [24, 8]), (9, 32, [8, 24, 8]), (26, 16, [200]), (26, 16, [24, 200]),
    (32, 8, [256]), (32, 64, [8, 24]), (9, 64, [24]), (8, 32, [8, 256]), (26, 8, [8, 8, 8]),
]


def check_exact(gpu, B, m, D, widths, combos, runs=("raw", "fused")):
    x0, ws, dp, xs, p, dxs, dx0, dws = ternary_case(B, m, D, widths, 1000 * m + D + B + len(widths))
    wg = [w.float().to(gpu) for w in ws]
    for xd0, xd in combos:
        what = (B, m, D, widths, xd0, xd)
        if "raw" in runs:
            r = raw_cin(padded(x0, xd0, gpu)[1], wg, dp.float().to(gpu), xd)
            for k, x in enumerate(xs):
                assert r["xs"][k].dtype == xd
                assert torch.equal(r["xs"][k].cpu().double().long().reshape(x.shape), x), ("X", k, what)
            assert torch.equal(r["p"].cpu().double().long(), p), ("p", what)
            full = r["dx0"].cpu().double() + r["dxps"][0].cpu().double()
            assert torch.equal(full.long(), dx0), ("dx0", what)
            for k, w in enumerate(dws):
                assert torch.equal(r["dws"][k].cpu().double().long(), w), ("dW", k, what)
        if "fused" in runs:
            gp, gx, gw = fused(x0.to(gpu).to(xd0), wg, dp.float().to(gpu), xd)
            assert gp.dtype == F32 and gx.dtype == xd0
            assert torch.equal(gp.cpu().double().long(), p), ("p", what)
            assert torch.equal(gx.cpu().double().long(), dx0), ("dx0", what)
            for k, w in enumerate(dws):
                assert torch.equal(gw[k].cpu().double().long(), w), ("dW", k, what)


@pytest.mark.parametrize("m,D,widths", EXACT_CASES)
def test_exact_every_dtype_combination(gpu, monkeypatch, m, D, widths):
    calls = _spy(monkeypatch)
    check_exact(gpu, 70, m, D, widths, DTYPE_COMBOS)
    n = 2 * len(DTYPE_COMBOS) * len(widths)
    assert calls.count("mrec_cin_fwd") == n == calls.count("mrec_cin_bwd")


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("m,D,widths", [(2, 8, [8]), (26, 16, [24, 200]), (9, 64, [24]), (32, 32, [8, 24, 8])])
def test_exact_small_batches(gpu, B, m, D, widths):
    check_exact(gpu, B, m, D, widths, [(F32, F32), (BF, BF)])


def test_empty_batch(gpu):
    x0 = torch.zeros(0, 5 * 16, device=gpu, dtype=BF)
    ws = [torch.randn(8, 5, 5, device=gpu), torch.randn(16, 8, 5, device=gpu)]
    p, dx0, dws = fused(x0, ws, torch.zeros(0, 24, device=gpu), BF)
    assert tuple(p.shape) == (0, 24) and tuple(dx0.shape) == (0, 80)
    assert all(tuple(g.shape) == tuple(w.shape) and not bool(g.any()) for g, w in zip(dws, ws))


# ---------------------------------------------------------------------------
# 2. Gaussian operands against fp64 on the bf16-rounded operands
# ---------------------------------------------------------------------------

def gaussian_case(B, m, D, widths, seed, x0_dtype):
    g = torch.Generator().manual_seed(seed)
    hs = widths_of(m, widths)
    x0 = torch.randn(B, m * D, generator=g).to(x0_dtype)
    ws = [torch.randn(h, hp, m, generator=g) * (hp * m) ** -0.5 for hp, h in zip(hs[:-1], hs[1:])]
    dp = torch.randn(B, sum(widths), generator=g)
    return x0, ws, dp


def rb64(t):
    """The bf16 value a product reads, as fp64 numpy."""
    return t.detach().float().cpu().bfloat16().double().numpy()


def layer_bounds(x0, xp, W, g_in, dp_prev, D, x_dtype, dxp_dtype):
    """One layer in fp64 on the bf16-rounded operands, with the derived error bounds.

    x0 [B, m D], xp [B, Hp D], g_in [B, H D] (dX^k as stored) or [B, H] (dp, the top layer),
    dp_prev [B, Hp] or None.  Rounding contract: x0, xp, W, dX^k enter as bf16 (exact here: the
    oracle rounds them too); Z is rounded once (2^-8 per term, forward and dW); products of
    bf16 values are exact in fp32; an fp32 accumulation of K terms errs by at most K 2^-24 of
    the sum of the terms' magnitudes.
      X^k   (2^-8 + Hp MP 2^-24) sum |W xp x0|  (+ 2^-8 |X^k| stored in bf16), MP <= 32
      p     the sum over d of the first part, + D 2^-24 sum_d |X^k|
      dxp   no bf16 rounding: dZ is K = r16(H) terms, then one fp32 product and m (<= 32) more
            additions: (H + 15 + 32 + 2) 2^-24 sum |g W x0|, + 2^-24 |dxp| for dp_prev, (+
            2^-8 |dxp| in bf16)
      dx0   likewise, Hp additions per register: (H + 15 + Hp + 2) 2^-24 sum |g W xp|, +
            2^-24 |dx0| for the add into the accumulator
      dW    (2^-8 + r16(B D) 2^-24) sum |g xp x0|
    -> dict name -> (want, bound)"""
    B = x0.shape[0]
    X0 = rb64(x0).reshape(B, -1, D)
    XP = rb64(xp).reshape(B, -1, D)
    m, Hp = X0.shape[1], XP.shape[1]
    Wb = rb64(W)
    H = Wb.shape[0]
    G = rb64(g_in)
    G = G.reshape(B, H, D) if G.shape[1] == H * D else np.broadcast_to(G[:, :, None], (B, H, D))
    Z = (XP[:, :, None, :] * X0[:, None, :, :]).reshape(B, Hp * m, D)
    W2 = Wb.reshape(H, Hp * m)
    xk = np.einsum("hn,bnd->bhd", W2, Z)
    xa = np.einsum("hn,bnd->bhd", np.abs(W2), np.abs(Z))
    xb = (U8 + Hp * 32 * U24) * xa
    out = {"p": (xk.sum(2), xb.sum(2) + D * U24 * np.abs(xk).sum(2))}
    out["xk"] = (xk.reshape(B, H * D), (xb + (U8 * np.abs(xk) if x_dtype == BF else 0.0)).reshape(B, H * D))
    dZ = np.einsum("hn,bhd->bnd", W2, G).reshape(B, Hp, m, D)
    dZa = np.einsum("hn,bhd->bnd", np.abs(W2), np.abs(G)).reshape(B, Hp, m, D)
    dxp = (dZ * X0[:, None]).sum(2)
    dxpa = (dZa * np.abs(X0[:, None])).sum(2)
    if dp_prev is not None:
        dxp = dxp + dp_prev.detach().double().cpu().numpy()[:, :, None]
    db = (H + 15 + 32 + 2) * U24 * dxpa + U24 * np.abs(dxp) + (U8 * np.abs(dxp) if dxp_dtype == BF else 0.0)
    out["dxp"] = (dxp.reshape(B, Hp * D), db.reshape(B, Hp * D))
    dx0 = (dZ * XP[:, :, None]).sum(1)
    dx0a = (dZa * np.abs(XP[:, :, None])).sum(1)
    out["dx0"] = (dx0.reshape(B, m * D), ((H + 15 + Hp + 2) * U24 * dx0a + U24 * np.abs(dx0)).reshape(B, m * D))
    dw = np.einsum("bhd,bnd->hn", G, Z)
    dwa = np.einsum("bhd,bnd->hn", np.abs(G), np.abs(Z))
    out["dw"] = (dw.reshape(H, Hp, m), ((U8 + (B * D + 15) * U24) * dwa).reshape(H, Hp, m))
    return out


def assert_within(got, want_bound, what):
    want, bound = want_bound
    err = np.abs(got.detach().double().cpu().numpy().reshape(want.shape) - want)
    worst = float(np.max(err / (bound + 1e-300) * (err > 0)))
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


GAUSS_CASES = [  # B, m, D, widths   (Z of the fp64 oracle: B Hp m D 8 bytes, under 50 MB)
    (70, 2, 8, [8, 24]), (70, 8, 16, [24, 8, 24]), (70, 9, 32, [24, 8]), (70, 26, 16, [200]),
    (5, 26, 16, [24, 200, 8]), (70, 32, 8, [256, 8]), (5, 32, 64, [8, 24]), (3, 9, 64, [24, 24]),
    (1, 26, 16, [200, 200]),
]


def check_layers(r, x0, ws, dp, D, x_dtype, tag):
    """Every layer of a raw_cin(fresh_dx0=True) result against the oracle on that layer's own
    inputs as the kernels stored them."""
    offs = np.concatenate([[0], np.cumsum([w.shape[0] for w in ws])]).astype(int)
    L = len(ws)
    for k in range(L):
        xp = x0 if k == 0 else r["xs"][k - 1]
        g_in = r["dxps"][k + 1] if k + 1 < L else dp[:, offs[k]:offs[k + 1]]
        dpp = dp[:, offs[k - 1]:offs[k]] if k > 0 else None
        b = layer_bounds(x0, xp, ws[k], g_in, dpp, D, x_dtype, x_dtype if k > 0 else F32)
        t = f"{tag} layer {k + 1}"
        assert_within(r["xs"][k], b["xk"], "X^k " + t)
        assert_within(r["p"][:, offs[k]:offs[k + 1]], b["p"], "p " + t)
        assert_within(r["dxps"][k], b["dxp"], "dxp " + t)
        assert_within(r["dx0s"][k], b["dx0"], "dx0 " + t)
        assert_within(r["dws"][k], b["dw"], "dW " + t)


@pytest.mark.parametrize("B,m,D,widths", GAUSS_CASES)
def test_gaussian_within_the_derived_bound(gpu, B, m, D, widths):
    for xd0, xd in ((F32, F32), (BF, BF), (F32, BF)):
        x0, ws, dp = gaussian_case(B, m, D, widths, 7 * m + D, xd0)
        r = raw_cin(padded(x0, xd0, gpu)[1], [w.to(gpu) for w in ws], dp.to(gpu), xd, fresh_dx0=True)
        check_layers(r, x0, ws, dp, D, xd, f"B={B} m={m} D={D} {widths} {xd0} {xd}")


# ---------------------------------------------------------------------------
# 3. memory discipline
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,D,widths", [(2, 8, [8, 24]), (26, 16, [200, 8]), (9, 64, [24]), (32, 32, [256])])
def test_strides_nan_pads_and_sentinels(gpu, m, D, widths, dtype):
    B, SENT = 5, 7.0
    x0, ws, dp = gaussian_case(B, m, D, widths, 31 * m + D, dtype)
    wg = [w.to(gpu) for w in ws]
    tight = raw_cin(padded(x0, dtype, gpu)[1], wg, dp.to(gpu), dtype)
    # wide: x0 as a column slice of wider rows (the model's x0 with its dense and pad columns),
    # NaN in every pad column and in the rows past the batch of the inputs, a sentinel all over
    # the outputs
    wx0 = padded(x0, dtype, gpu, 2, 16)[1]
    wdp = padded(dp, F32, gpu, 2, 8)[1]
    wide = raw_cin(wx0, wg, wdp, dtype, wide=True, sent=SENT)
    torch.cuda.synchronize()
    names = [f"x{k + 1}" for k in range(len(ws))] + ["p", "dx0_0"] + [f"dxp{k}" for k in range(len(ws))]
    views = {**{f"x{k + 1}": (tight["xs"][k], wide["xs"][k]) for k in range(len(ws))},
             "p": (tight["p"], wide["p"]), "dx0_0": (tight["dx0"], wide["dx0"]),
             **{f"dxp{k}": (tight["dxps"][k], wide["dxps"][k]) for k in range(len(ws))}}
    for name in names:
        t, w = views[name]
        buf, rows, cols = wide["bufs"][name]
        assert bool(torch.isfinite(w.float()).all()), name
        assert torch.equal(w, t), name
        assert bool((buf[:rows, cols:] == SENT).all()), name + ": columns past the width"
        assert bool((buf[rows:] == SENT).all()), name + ": rows past the batch"
    for k in range(len(ws)):
        flat, n = wide["bufs"][f"dw{k}"]
        assert torch.equal(wide["dws"][k], tight["dws"][k]) and bool(torch.isfinite(flat).all())
        assert bool((flat[:32] == SENT).all()) and bool((flat[32 + n:] == SENT).all()), f"dw{k}"
    # a batch smaller than the buffers: the rows past it keep the sentinel (dx0: its zero)
    small = raw_cin(wx0, wg, wdp, dtype, wide=True, sent=SENT, batch=B - 2)
    torch.cuda.synchronize()
    for name in names:
        t, w = views[name][0], small["bufs"][name][0]
        rows, cols = small["bufs"][name][1:]
        keep = 0.0 if name == "dx0_0" else SENT
        assert torch.equal(w[:B - 2, :cols], t[:B - 2]), name
        assert bool((w[B - 2:B, :cols] == keep).all()) and bool((w[B:] == SENT).all()), name


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,D,widths", [(26, 16, [200, 24]), (9, 64, [24, 8]), (32, 8, [8, 256])])
def test_bits_do_not_depend_on_run_or_position(gpu, m, D, widths, dtype):
    x0, ws, dp = gaussian_case(70, m, D, widths, 3 * m + D, dtype)
    x0, dp, wg = x0.to(gpu), dp.to(gpu), [w.to(gpu) for w in ws]

    def run(x, d):
        r = raw_cin(padded(x, dtype, gpu)[1], wg, d, dtype)
        return [*r["xs"], r["p"], r["dx0"], *r["dxps"]], r["dws"]

    a, aw = run(x0, dp)
    b, bw = run(x0, dp)
    for u, v in zip(a + aw, b + bw):
        assert torch.equal(u, v)
    f1, f2 = fused(x0, wg, dp, dtype), fused(x0, wg, dp, dtype)
    assert torch.equal(f1[0], f2[0]) and torch.equal(f1[1], f2[1])
    assert all(torch.equal(u, v) for u, v in zip(f1[2], f2[2]))
    pos = torch.tensor([69, 3, 34, 0, 17], device=gpu)  # the small batch's samples, in its order
    s, _ = run(x0[pos], dp[pos])
    for u, v in zip(a, s):
        assert torch.equal(u[pos], v)


# ---------------------------------------------------------------------------
# 5. dispatch
# ---------------------------------------------------------------------------

def test_compiled_shape_runs_both_kernels(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    x0, ws, dp = gaussian_case(9, 26, 16, [200, 200, 200], 1, BF)
    fused(x0.to(gpu), [w.to(gpu) for w in ws], dp.to(gpu), BF)
    assert [c for c in calls if c in KERNELS] == ["mrec_cin_fwd"] * 3 + ["mrec_cin_bwd"] * 3


@pytest.mark.parametrize("how", ["switch", "m33", "H12", "D12"])
def test_the_switch_and_unsupported_shapes_take_the_torch_ops(gpu, monkeypatch, how):
    from pytorchrec_amd import dense
    m, D, H = {"switch": (26, 16, 24), "m33": (33, 8, 8), "H12": (5, 8, 12), "D12": (5, 12, 8)}[how]
    if how == "switch":
        monkeypatch.setattr(dense, "CIN_FUSED", False)
    else:
        assert dense.CIN_FUSED and not dense.cin_supported(m, D, [H])
    B = 9
    x0, ws, dp = gaussian_case(B, m, D, [H], 2, F32)
    calls = _spy(monkeypatch)
    p, dx0, dws = fused(x0.to(gpu), [w.to(gpu) for w in ws], dp.to(gpu), F32)
    assert not KERNELS & set(calls)
    b = layer_bounds(x0, x0, ws[0], dp, None, D, F32, F32)
    assert_within(p, b["p"], f"{how} p")
    # (layer 1: X^0 plays both roles; the two parts of dx0 err independently)
    want = b["dx0"][0] + b["dxp"][0]
    assert_within(dx0, (want, b["dx0"][1] + b["dxp"][1] + U24 * np.abs(want)), f"{how} dx0")
    assert_within(dws[0], b["dw"], f"{how} dW")


# ---------------------------------------------------------------------------
# 7. the model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("emb_dtype", [F32, BF], ids=["fp32", "bf16"])
def test_xdeepfm_train_step_matches_the_fp64_model(gpu, monkeypatch, emb_dtype):
    """One XDeepFM train step (B = 256, 6 fields of 50 rows, 3 dense, D = 16, cin [16, 8],
    layers [64, 32], BCEWithLogitsLoss, plain SGD) against RefXDeepFM in fp64 from identical
    weights: the loss within 2e-3 and every parameter's UPDATE, the CIN maps and cin_out
    included.  The yardstick is test_dlrm_train_step_matches_the_fp64_model's: the same model in
    torch fp32 with bf16 rounding at the build's storage points (RefXDeepFM(bf16_points=True),
    run here on the GPU) says what bf16 storage alone costs, and the kernels' distance to fp64
    may not exceed 1.5x that plus 1 % of the update, in L2 and in max norm.  Tables fp32 and
    bf16 (RNE, lr 1e4 so that the table updates are many bf16 ulps and the emulation's tables
    are rounded the same way)."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    bf16 = emb_dtype == BF
    B, lr = 256, (1e4 if bf16 else 1.0)
    nums, nd, D, cin, layers = [50] * 6, 3, 16, (16, 8), (64, 32)
    m = xdeepfm(rows=50, F=6, n_dense=nd, D=D, cin=cin, layers=layers, device=gpu, emb_dtype=emb_dtype,
                random_seed=2020)
    m.embeddings.stochastic_rounding = False
    with torch.no_grad():  # weights large enough that every layer matters
        for lin in xdeepfm_linears(m):
            lin.weight.mul_(10.0)
            lin.bias.mul_(10.0)
        for w in m.cin_weights:
            w.mul_(30.0)
        m.cin_out.weight.mul_(30.0)
        m.embeddings.weight.mul_(30.0)
    assert m.embeddings.weight.dtype == emb_dtype
    r = RefXDeepFM(nums, nd, D, cin, layers)
    copy_into_ref(m, r)
    data, ids, dense, label = ctr_batch(m, B)
    data = {k: v.to(gpu) for k, v in data.items()}
    before_state = [v.clone() for v in r.state_dict().values()]
    before = [b.detach().clone() for _, _, b in named_pairs(m, r)]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], gpu)
    assert m.embeddings.update == "sgd"
    calls = _spy(monkeypatch)
    loss = float(m.train_step(data)["loss"].detach())
    for name in ("mrec_interact_fwd_ex", "mrec_cin_fwd", "mrec_cin_bwd", "mrec_tower_fwd_bwd"):
        assert name in calls, (name, calls)
    assert calls.count("mrec_cin_fwd") == 2 == calls.count("mrec_cin_bwd")
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    print(f"loss {loss:.6f} against {rloss:.6f}")
    assert abs(loss - rloss) <= 2e-3 * max(1.0, abs(rloss)), (loss, rloss)
    e = RefXDeepFM(nums, nd, D, cin, layers, dtype=torch.float32, bf16_points=True)
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
