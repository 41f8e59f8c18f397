"""Every bank row geometry of the embedding kernels against the fp64 oracle.

The embedding kernels (emb_fwd.hip, emb_bwd.hip, emb_apply.h, emb_bwd_large.hip,
the forward Adam catch-up) are compiled once per row geometry: a bank row is
16..256 bytes, read by LPR = row_bytes / 16 lanes (1, 2, 4, 8 or 16), times two
dtypes.  LPR decides which lane holds the first-order weight, which lanes are dead
padding, the field iterations per wave, the DPP reduction (LPR 4 only), the
cross-lane reduce of row-wise Adagrad and the workers per block of the hot-segment
tree.  The sibling files pin D = 16 (and fp32 D = 8): this file sweeps the rest
through the public wrappers (EmbeddingBank, gather, interact, use_fused_sgd,
use_fused_optimizer).

Bars.  Gathers and the x0 embedding columns are bit copies (RNE bits when
narrowing).  The interaction logit keeps the project's bar (test_interact_deepfm_stage):
|got - want| <= 1e-5 (|want| + ref.fm2_magnitude(v)).  Dense gradients: a row hit
<= 16 times is bitwise the sequential fp32 sum of its lookups' gradients in
ascending sample order (emb_bwd.hip), for a bf16 bank its one RNE rounding
(apply_row_raw_g adds the fp32 sum to the zeroed gradient row and rounds once);
hotter rows are within 1e-6 sum |g| of the fp64 sum (plus that one bf16 rounding).
Fused SGD: fp32 within 2e-6 scale of ref.sgd_rows, bf16 within one bf16 ulp.

The per-lookup gradient of the interaction backward is dx0 + dlogit (fm_sum - v),
formed in fp32 by the kernel from ITS fm_sum: the bitwise checks restate that fma
in numpy from the kernel's fm_sum (read from the autograd node, and itself checked
against v.sum(1)), and the restated gradient is tied to the fp64 oracle
(dx0 + ref.fm2_bwd) within 1e-6 of its magnitude |dx0| + |dlogit| (sum_f |v| + |v|)
(fm_sum carries < F roundings of sum_f |v|, the subtraction and the fma one each:
< 7 * 2^-24 for F = 5).

The generator and the expected values take a device: the tests at the bottom (not
marked gpu) run forward, dense gradient and fp32 fused SGD on the CPU path
(cpu_path.py), which proves the generator, the oracle calls and the oracle-side
tolerances without a GPU.  The CPU path sums in another order (autograd) and, for
a bf16 bank, in bf16: the bitwise checks are the GPU's only, and a bf16 bank's CPU
dense gradient gets the bound of its bf16 accumulation, (n + 1) 2^-8 of the
magnitude for a row hit n times.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref
from test_gpu_embedding import (_as_f32, _bank, _bits, _fill, _fm_tol_ok, _ids_with_edges,
                                _rand_tables, _wbits)
from test_gpu_optim import _run

gpu_test = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
CPU = torch.device("cpu")
SENT = 776.0  # pad-column sentinel (exact in bf16 too)
NUMS = [1, 7, 300, 5000]
B_FWD, B_HASH, B_SORTED, B_LARGE = 257, 2500, 4100, 8200
LR = 0.1

# (dtype, dim, has_w): every (dtype, LPR) with and without a w lane where one fits,
# plus the lane-mask edges (w lane with one live element, dead lanes behind it, w in
# the last lane, a dim that is no power of two, full rows)
GEOMS = [
    (F32, 4, False), (F32, 4, True), (F32, 8, True), (F32, 12, True), (F32, 24, True),
    (F32, 32, True), (F32, 60, True), (F32, 64, False),
    (BF16, 8, False), (BF16, 8, True), (BF16, 24, True), (BF16, 32, False), (BF16, 32, True),
    (BF16, 56, True), (BF16, 64, True), (BF16, 128, False),
]


def _es(dtype):
    return 4 if dtype == F32 else 2


def _lpr(dtype, dim, has_w):
    need, b = (dim + int(has_w)) * _es(dtype), 16
    while b < need:
        b *= 2
    return b // 16


def _gid(gi):
    dtype, dim, has_w = GEOMS[gi]
    return "%s-d%d-%s-lpr%d" % ("f32" if dtype == F32 else "bf16", dim, "w" if has_w else "nw",
                                _lpr(dtype, dim, has_w))


def _fwd_params():
    """F = 1, F = WPW + 1 (a second, nearly empty field iteration) where <= 64, and
    F = 64 = MREC_MAX_TABLES for the LPR 1 geometries and the two full 256-B rows."""
    out = []
    for gi, (dtype, dim, has_w) in enumerate(GEOMS):
        lpr = _lpr(dtype, dim, has_w)
        fs = [1]
        if 64 // lpr + 1 <= 64:
            fs.append(64 // lpr + 1)
        if lpr == 1 or (lpr == 16 and not has_w):
            fs.append(64)
        out += [pytest.param(gi, F, id="%s-F%d" % (_gid(gi), F)) for F in fs]
    return out


ALL = [pytest.param(gi, id=_gid(gi)) for gi in range(len(GEOMS))]
# the sorted layout and the large-batch path: LPR 1 and LPR 16 of both dtypes (the
# LPR 16 rows with a w lane and dead lanes behind it), and fp32 dim 8 + w
EDGE = [pytest.param(GEOMS.index(g), id=_gid(GEOMS.index(g)))
        for g in [(F32, 4, False), (F32, 32, True), (BF16, 8, False), (BF16, 64, True), (F32, 8, True)]]


def _sgd_params(geoms):
    """Fused SGD: RNE everywhere, stochastic rounding where it exists (bf16 rows)."""
    return [pytest.param(p.values[0], sr, id="%s-%s" % (p.id, "sr" if sr else "rne"))
            for p in geoms for sr in (False, True) if not sr or GEOMS[p.values[0]][0] == BF16]


def test_sweep_covers_every_instantiation():
    """Every (dtype, LPR) pair is in the forward / hash sweep, LPR 1 and 16 of both
    dtypes in the sorted and large-batch ones."""
    assert {(g[0], _lpr(*g)) for g in GEOMS} == {(d, l) for d in (F32, BF16) for l in (1, 2, 4, 8, 16)}
    edge = {(GEOMS[p.values[0]][0], _lpr(*GEOMS[p.values[0]])) for p in EDGE}
    assert edge == {(d, l) for d in (F32, BF16) for l in (1, 16)} | {(F32, 4)}
    assert (F32, 8, True) in [GEOMS[p.values[0]] for p in EDGE]


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

def _tables(rng, nums, dim, has_w, dtype):
    tabs = _rand_tables(rng, nums, dim, dtype)
    wts = None
    if has_w:
        wts = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in nums]
        if dtype == BF16:
            wts = [ref.bf16_round(x) for x in wts]
    return tabs, wts


def _filled_bank(c, device, update="dense", sentinel=True):
    """The case's bank; ``sentinel``: SENT in every pad column (past [v | w])."""
    dtype, dim, has_w = c["geom"]
    if device.type == "cuda":
        bank = _bank(c["nums"], dim, has_w, dtype, update=update, device=device)
    else:
        from pytorchrec_amd.embedding import EmbeddingBank
        bank = EmbeddingBank(c["nums"], dim, with_first_order=has_w, dtype=dtype, update=update,
                             device=device)
    assert bank.row_stride * _es(dtype) == 16 * _lpr(dtype, dim, has_w)
    _fill(bank, c["tabs"], c["wts"])
    used = dim + int(has_w)
    if sentinel and used < bank.row_stride:
        with torch.no_grad():
            bank.weight[:, used:] = SENT
    return bank


def _ids_t(c, device, id_dtype):
    return [torch.from_numpy(np.ascontiguousarray(c["ids"][:, f])).to(device, id_dtype)
            for f in range(len(c["nums"]))]


@functools.lru_cache(maxsize=None)
def _fwd_case(gi, F):
    dtype, dim, has_w = GEOMS[gi]
    rng = np.random.default_rng(1000 + 100 * gi + F)
    nums = [NUMS[f % 4] for f in range(F)]
    tabs, wts = _tables(rng, nums, dim, has_w, dtype)
    ids = np.stack([_ids_with_edges(rng, n, B_FWD) for n in nums], 1)
    v_raw = ref.multi_table_gather(tabs, ids)  # [B, F, D], the bank's dtype (bf16: bits)
    w_g = np.stack([wts[f][ids[:, f]] for f in range(F)], 1) if has_w else None
    return dict(geom=GEOMS[gi], nums=nums, tabs=tabs, wts=wts, ids=ids, v_raw=v_raw,
                v=_as_f32(v_raw), w_g=w_g)


def _mixed_ids(rng, n, B, huge=0):
    """B lookups of a table of n >= 300 rows: rows hit once, 2..16 times, 17..200
    times, one row hit ``huge`` times if given; the other rows untouched."""
    counts = ([huge] if huge else []) + [17, 33, 64, 120, 180] + list(range(2, 17)) + [2, 16]
    left = B - sum(counts)
    assert left >= 0
    singles = min(left, (n - len(counts)) // 2)
    left -= singles
    if left:
        k = -(-left // 150)
        assert left // k >= 17
        counts += [left // k + (i < left % k) for i in range(k)]
    counts += [1] * singles
    assert len(counts) < n and sum(counts) == B
    ids = np.repeat(rng.permutation(n)[:len(counts)], counts)
    rng.shuffle(ids)
    return ids


@functools.lru_cache(maxsize=None)
def _bwd_case(gi, B, nums, huge):
    """Tables and ids of a backward case; the table of the most rows holds the row
    hit ``huge`` (> 1024) times.  Tables below 300 rows: uniform ids, last row untouched."""
    dtype, dim, has_w = GEOMS[gi]
    rng = np.random.default_rng(2000 + 100 * gi + B)
    nums = list(nums)
    tabs, wts = _tables(rng, nums, dim, has_w, dtype)
    big = int(np.argmax(nums))
    cols = []
    for f, n in enumerate(nums):
        if n >= 300:
            cols.append(_mixed_ids(rng, n, B, huge if f == big else 0))
        else:
            cols.append(rng.integers(0, max(1, n - 1), B))
    ids = np.stack(cols, 1)
    for f, n in enumerate(nums):  # no class may silently be empty
        if n >= 300:
            cnt = np.bincount(ids[:, f], minlength=n)
            assert (cnt == 0).any() and (cnt == 1).any()
            assert ((cnt >= 2) & (cnt <= 16)).any() and ((cnt >= 17) & (cnt <= 200)).any()
            assert (cnt > 1024).any() == (f == big)
    return dict(geom=GEOMS[gi], nums=nums, tabs=tabs, wts=wts, ids=ids)


# ---------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------

def _check_gather(device, gi, F):
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.embedding import gather
    c = _fwd_case(gi, F)
    dtype, dim, has_w = c["geom"]
    bank = _filled_bank(c, device)
    want = c["v_raw"].reshape(B_FWD, -1)
    with torch.no_grad():
        for id_dtype in (torch.int32, torch.int64):
            ids = _ids_t(c, device, id_dtype)
            res = gather(bank, ids, with_w=has_w)
            out = res[0] if has_w else res
            assert out.dtype == dtype and out.shape == (B_FWD, F * dim)
            assert np.array_equal(_bits(out), _wbits(want))
            assert not np.any(out.float().cpu().numpy() == SENT)
            if has_w:
                assert np.array_equal(res[1].cpu().numpy(), c["w_g"])
        if dtype == BF16:  # widened: exact
            out32 = gather(bank, ids, out_dtype=F32)
            assert out32.dtype == F32
            assert np.array_equal(out32.cpu().numpy(), _as_f32(want))
        elif dim % 8 == 0 or device.type == "cpu":  # narrowed: RNE
            out16 = gather(bank, ids, out_dtype=BF16)
            assert out16.dtype == BF16
            assert np.array_equal(_bits(out16), ref.f32_to_bf16_bits(want))
        else:  # a bf16 field of dim * 2 bytes is no multiple of 16 bytes (mrec.h)
            with pytest.raises(_mrec.MrecError, match="16B") as e:
                gather(bank, ids, out_dtype=BF16)
            assert e.value.status == _mrec.EINVAL


def _check_interact(device, gi, F):
    from pytorchrec_amd.embedding import interact
    c = _fwd_case(gi, F)
    dtype, dim, has_w = c["geom"]
    B, v = B_FWD, c["v"]
    banks = [_filled_bank(c, device, sentinel=False), _filled_bank(c, device, sentinel=True)]
    rng = np.random.default_rng(7)
    bias = np.array([0.25], np.float32)
    w_g = c["w_g"] if has_w else np.zeros((B, 1), np.float32)
    x0_dtypes = [F32] + ([BF16] if dim * 2 % 16 == 0 else [])  # the x0 alignment rule
    runs = [(nd, xd, True) for nd in (0, 13, 70) for xd in x0_dtypes] + [(13, F32, False)]
    for k, (nd, x0_dtype, use_dw) in enumerate(runs):  # (False: DCN-v2, no dense first order)
        dense = rng.random((B, nd)).astype(np.float32) if nd else None
        dense_w = (rng.standard_normal(nd) * 0.1).astype(np.float32) if nd and use_dw else None
        x0_cols = (F * dim + nd + 7) // 8 * 8 + 8
        ids = _ids_t(c, device, torch.int32 if k % 2 == 0 else torch.int64)
        outs = []
        for bank in banks:
            x0, logit = interact(bank, ids, None if dense is None else torch.from_numpy(dense).to(device),
                                 None if dense_w is None else torch.from_numpy(dense_w).to(device),
                                 torch.from_numpy(bias).to(device), fm2=True, first_order=has_w,
                                 x0_cols=x0_cols, x0_dtype=x0_dtype)
            fm_sum = None
            if device.type == "cuda":  # internal: the autograd node's saved tensor
                fm_sum = logit.grad_fn.saved_tensors[1].detach().cpu().numpy()
            outs.append((_bits(x0), logit.detach().cpu().numpy(), fm_sum))
        # the pad columns of the bank reach nothing
        assert np.array_equal(outs[0][0], outs[1][0]), (nd, x0_dtype)
        assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32)), (nd, x0_dtype)
        x0n, got, fm_sum = outs[1]
        assert x0n.shape == (B, x0_cols)
        want = ref.fm2(v) + ref.first_order(w_g, dense if dense_w is not None else None, dense_w,
                                            bias[0])
        ok, worst = _fm_tol_ok(got.astype(np.float64), v, want)
        assert ok, (nd, x0_dtype, use_dw, worst)
        # x0 = [v | dense | 0]
        if x0_dtype == BF16:
            want_v = c["v_raw"] if dtype == BF16 else ref.f32_to_bf16_bits(v)
            want_d = ref.f32_to_bf16_bits(dense) if nd else None
        else:
            want_v = v.view(np.uint32)
            want_d = dense.view(np.uint32) if nd else None
        assert np.array_equal(x0n[:, :F * dim], want_v.reshape(B, -1)), (nd, x0_dtype)
        if nd:
            assert np.array_equal(x0n[:, F * dim:F * dim + nd], want_d), (nd, x0_dtype)
        assert np.all(x0n[:, F * dim + nd:] == 0), (nd, x0_dtype)
        if fm_sum is not None:
            assert np.array_equal(outs[0][2].view(np.uint32), fm_sum.view(np.uint32))
            err = np.abs(fm_sum - v.astype(np.float64).sum(1))
            assert np.all(err <= 1e-6 * np.abs(v).astype(np.float64).sum(1)), (nd, err.max())


@gpu_test
@pytest.mark.parametrize("gi,F", _fwd_params())
def test_gather_geometry(gpu, gi, F):
    _check_gather(gpu, gi, F)


@gpu_test
@pytest.mark.parametrize("gi,F", _fwd_params())
def test_interact_geometry(gpu, gi, F):
    _check_interact(gpu, gi, F)


# ---------------------------------------------------------------------------
# 2. backward
# ---------------------------------------------------------------------------

def _half_ulp(dtype, x):
    """The one RNE rounding of a bf16 bank's dense-gradient row."""
    return 0.5 * ref.bf16_ulp(x) * 1.0001 if dtype == BF16 else 0.0


def _hash_hot_tol(want, mag):
    return 1e-6 * mag


def _large_hot_tol(want, mag):  # fixed point: one fp32 rounding of the exact sum
    return 2.0 ** -24 * np.abs(want) + 1e-12 * mag + 1e-30


def _check_dense_grad(c, bank, grad, g64, mag, gw, g32=None, hot_tol=_hash_hot_tol):
    """grad: the bank-shaped dense gradient.  g64 [B, F, D]: the oracle's per-lookup
    gradients, mag their magnitudes (error scale), gw [B] the first-order gradient or
    None.  g32 (GPU): the per-lookup gradients in the kernel's fp32 bits -> the
    bitwise / hot-row checks of the summation itself."""
    dtype, dim, has_w = c["geom"]
    on_cpu = not grad.is_cuda
    gb = _bits(grad)
    gf = _as_f32(gb) if dtype == BF16 else gb.view(np.float32)
    used = dim + int(has_w)
    assert np.all(gb[:, used:] == 0)  # pad columns
    for f, n in enumerate(c["nums"]):
        o, ids = bank.row_offset[f], c["ids"][:, f]
        cnt = np.bincount(ids, minlength=n)
        assert np.all(gb[o:o + n][cnt == 0] == 0), f  # untouched rows: exactly zero
        cols = [(slice(0, dim), g64[:, f], mag[:, f], None if g32 is None else g32[:, f])]
        if gw is not None:
            gw2 = gw.astype(np.float64)[:, None]
            cols.append((slice(dim, dim + 1), gw2, np.abs(gw2), None if g32 is None else gw[:, None]))
        elif has_w:
            assert np.all(gb[o:o + n, dim] == 0), f
        for sl, a64, amag, a32 in cols:
            got = gf[o:o + n, sl].astype(np.float64)
            want = ref.dense_grad(n, ids, a64)
            m = ref.dense_grad(n, ids, amag)
            if on_cpu and dtype == BF16:  # the CPU path rounds and accumulates in bf16
                tol = (cnt[:, None] + 1) * 2.0 ** -8 * m
            else:
                tol = 1e-6 * m + _half_ulp(dtype, np.abs(want) + 1e-6 * m)
            assert np.all(np.abs(got - want) <= tol + 1e-30), (f, sl)
            if a32 is None:
                continue
            seq = np.zeros((n, a32.shape[1]), np.float32)
            np.add.at(seq, ids, a32)  # sequential fp32, ascending sample order
            short = cnt <= 16
            seqb = ref.f32_to_bf16_bits(seq) if dtype == BF16 else seq.view(np.uint32)
            assert np.array_equal(gb[o:o + n, sl][short], seqb[short]), (f, sl)
            hot = ~short
            w32 = ref.dense_grad(n, ids, a32.astype(np.float64))[hot]
            m32 = ref.dense_grad(n, ids, np.abs(a32).astype(np.float64))[hot]
            tol = hot_tol(w32, m32)
            assert np.all(np.abs(got[hot] - w32) <= tol + _half_ulp(dtype, np.abs(w32) + tol)), (f, sl)


def _check_sgd(c, bank, before, g64, gw, lr):
    """The bank after one fused SGD step against ref.sgd_rows: fp32 within 2e-6 scale
    (scale as in test_fused_sgd_f32_matches_oracle), bf16 within one bf16 ulp; the w
    column on its own; untouched rows and every pad column bit-identical."""
    dtype, dim, has_w = c["geom"]
    after = _bits(bank.weight)
    af = _as_f32(after) if dtype == BF16 else after.view(np.float32)
    used = dim + int(has_w)
    assert np.array_equal(after[:, used:], before[:, used:])  # pad columns
    for f, n in enumerate(c["nums"]):
        o, ids = bank.row_offset[f], c["ids"][:, f]
        touched = np.bincount(ids, minlength=n) > 0
        assert np.array_equal(after[o:o + n][~touched], before[o:o + n][~touched]), f
        tab = _as_f32(c["tabs"][f])
        want = ref.sgd_rows(tab, ids, g64[:, f], lr)
        got = af[o:o + n, :dim].astype(np.float64)
        if dtype == BF16:
            assert np.all(np.abs(got - want)[touched] <= ref.bf16_ulp(want[touched]) * 1.0001), f
        else:
            scale = np.abs(tab).max() + lr * np.abs(ref.dense_grad(n, ids, np.abs(g64[:, f]))).max()
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * scale)
        if not has_w:
            continue
        if gw is None:
            assert np.array_equal(after[o:o + n, dim], before[o:o + n, dim]), f
            continue
        want_w = ref.sgd_rows(c["wts"][f][:, None], ids, gw[:, None], lr)[:, 0]
        got_w = af[o:o + n, dim].astype(np.float64)
        if dtype == BF16:
            assert np.all(np.abs(got_w - want_w)[touched] <=
                          ref.bf16_ulp(want_w[touched]) * 1.0001), f
        else:
            np.testing.assert_allclose(got_w, want_w, rtol=0, atol=2e-6 * (1 + np.abs(want_w).max()))


def _interact_backward(device, c, update, sr=False):
    """One interaction forward + backward (dx0 from the "tower", dlogit feeding FM2
    and the first order).  -> bank, weight bits before, and the gradients' oracle."""
    from pytorchrec_amd.embedding import interact
    dtype, dim, has_w = c["geom"]
    F, B = len(c["nums"]), c["ids"].shape[0]
    rng = np.random.default_rng(B + dim)
    bank = _filled_bank(c, device, update=update)
    if update == "sgd":
        bank.use_fused_sgd(lr=LR)
        bank.stochastic_rounding = sr
    before = _bits(bank.weight)
    ids = _ids_t(c, device, torch.int32 if dim % 8 else torch.int64)
    x0, logit = interact(bank, ids, fm2=True, first_order=has_w, x0_cols=F * dim, x0_dtype=dtype)
    fm_sum = None
    if device.type == "cuda":
        fm_sum = logit.grad_fn.saved_tensors[1].detach().cpu().numpy()
    dx0 = (rng.standard_normal((B, F * dim)) * 0.05).astype(np.float32)
    if dtype == BF16:  # a bf16 tower hands back a bf16 dx0
        dx0 = ref.bf16_round(dx0)
    dlogit = (rng.standard_normal(B) * 0.05).astype(np.float32)
    torch.autograd.backward([x0, logit], [torch.from_numpy(dx0).to(device, dtype),
                                          torch.from_numpy(dlogit).to(device)])
    v32 = _as_f32(ref.multi_table_gather(c["tabs"], c["ids"]))
    v = v32.astype(np.float64)
    dx = dx0.reshape(B, F, dim)
    g64 = dx + ref.fm2_bwd(v, dlogit)
    a = np.abs(v)
    mag = np.abs(dx) + np.abs(dlogit)[:, None, None] * (a.sum(1, keepdims=True) + a)
    g32 = None
    if fm_sum is not None:
        err = np.abs(fm_sum - v.sum(1))
        assert np.all(err <= 1e-6 * a.sum(1)), err.max()
        # fmaf(dlogit, fm_sum - v, dx0) of lookup_grad_v: the fp32 subtraction, then the
        # product exact in fp64 and one rounding
        d = fm_sum[:, None, :] - v32
        assert d.dtype == np.float32
        g32 = (dlogit.astype(np.float64)[:, None, None] * d.astype(np.float64) + dx).astype(np.float32)
        assert np.all(np.abs(g32 - g64) <= 1e-6 * mag)
    return bank, before, g64, mag, (dlogit if has_w else None), g32


def _hash_dense_grad(device, gi):
    c = _bwd_case(gi, B_HASH, tuple(NUMS[f % 4] for f in range(5)), 1100)
    bank, before, g64, mag, gw, g32 = _interact_backward(device, c, "dense")
    assert np.array_equal(_bits(bank.weight), before)
    _check_dense_grad(c, bank, bank.weight.grad, g64, mag, gw, g32)
    bank2 = _interact_backward(device, c, "dense")[0]  # bitwise reproducible
    assert np.array_equal(_bits(bank.weight.grad), _bits(bank2.weight.grad))


def _hash_fused_sgd(device, gi, sr):
    c = _bwd_case(gi, B_HASH, tuple(NUMS[f % 4] for f in range(5)), 1100)
    bank, before, g64, mag, gw, g32 = _interact_backward(device, c, "sgd", sr)
    _check_sgd(c, bank, before, g64, gw, LR)


@gpu_test
@pytest.mark.parametrize("gi", ALL)
def test_hash_layout_dense_grad(gpu, gi):
    """B = 2500 through the interaction's in-launch hash plan, F = 5 tables of
    1, 7, 300, 5000, 1 rows (a 1100-lookup row: two kHotChunk passes of HotSeg)."""
    _hash_dense_grad(gpu, gi)


@gpu_test
@pytest.mark.parametrize("gi,sr", _sgd_params(ALL))
def test_hash_layout_fused_sgd(gpu, gi, sr):
    _hash_fused_sgd(gpu, gi, sr)


def _gather_backward(device, c, update, sr=False):
    from pytorchrec_amd.embedding import gather
    dtype, dim, has_w = c["geom"]
    F, B = len(c["nums"]), c["ids"].shape[0]
    rng = np.random.default_rng(B + dim + 1)
    bank = _filled_bank(c, device, update=update)
    if update == "sgd":
        bank.use_fused_sgd(lr=LR)
        bank.stochastic_rounding = sr
    before = _bits(bank.weight)
    dy = (rng.standard_normal((B, F * dim)) * 0.05).astype(np.float32)
    out = gather(bank, _ids_t(c, device, torch.int32), out_dtype=F32)
    out.backward(torch.from_numpy(dy).to(device))
    g32 = dy.reshape(B, F, dim)
    return bank, before, g32.astype(np.float64), np.abs(g32).astype(np.float64), g32


def _sorted_case(gi):
    return _bwd_case(gi, B_SORTED, tuple(NUMS[f % 4] for f in range(5)), 1100)


@gpu_test
@pytest.mark.parametrize("gi", EDGE)
def test_sorted_layout_dense_grad(gpu, gi):
    """B = 4100 (> MREC_BWD_HASH_MAX_BATCH: the radix-sort plan and apply_kernel) via
    gather(...).backward; the first-order column gets no gradient here (gather hands
    one back for single-table banks only): it stays zero."""
    c = _sorted_case(gi)
    bank, before, g64, mag, g32 = _gather_backward(gpu, c, "dense")
    _check_dense_grad(c, bank, bank.weight.grad, g64, mag, None, g32)
    bank2 = _gather_backward(gpu, c, "dense")[0]  # bitwise reproducible
    assert np.array_equal(_bits(bank.weight.grad), _bits(bank2.weight.grad))


@gpu_test
@pytest.mark.parametrize("gi,sr", _sgd_params(EDGE))
def test_sorted_layout_fused_sgd(gpu, gi, sr):
    """The same batch with the fused SGD update; the first-order column keeps its bits."""
    c = _sorted_case(gi)
    bank, before, g64, mag, g32 = _gather_backward(gpu, c, "sgd", sr)
    _check_sgd(c, bank, before, g64, None, LR)


@gpu_test
@pytest.mark.parametrize("update", ["dense", "sgd"])
@pytest.mark.parametrize("gi", EDGE)
def test_large_batch_backward(gpu, gi, update, monkeypatch):
    """B = 8200 lookups per table (> MREC_BWD_MAX_BATCH: emb_bwd_large.hip), tables of
    3000 and 40 rows, a row hit 2100 times (> 2048: the chunked fixed-point kernels).
    The fused launch and the plan / apply pair agree bitwise; bars as in
    test_backward_large_batch_dense_grad / _sgd_one_update_per_row (bf16: RNE)."""
    from pytorchrec_amd import embedding as E
    c = _bwd_case(gi, B_LARGE, (3000, 40), 2100)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(E, "LARGE_FUSED", fused)
        res[fused] = _gather_backward(gpu, c, update)
    bank, before, g64, mag, g32 = res[True]
    what = (lambda b: b.weight.grad) if update == "dense" else (lambda b: b.weight)
    assert np.array_equal(_bits(what(bank)), _bits(what(res[False][0])))
    if update == "dense":
        _check_dense_grad(c, bank, bank.weight.grad, g64, mag, None, g32, hot_tol=_large_hot_tol)
    else:
        _check_sgd(c, bank, before, g64, None, LR)


# ---------------------------------------------------------------------------
# 3. fused optimizers at other geometries
# ---------------------------------------------------------------------------

OPT_GEOMS = [(F32, 4, False, 3), (F32, 4, True, 1), (F32, 8, True, 1), (F32, 32, True, 1),
             (F32, 64, False, 3), (BF16, 8, False, 2), (BF16, 24, True, 1), (BF16, 64, True, 1)]
OPT_BARS = {F32: dict(rtol=1e-5, atol=1e-6), BF16: dict(rtol=2e-2, atol=2e-3)}  # test_gpu_optim's


def _check_optimizer(name, dtype, D, has_w, F, **kw):
    got, want, bank, S = _run(name, dtype, has_w=has_w, F=F, D=D, with_state=True, **kw)
    for f in range(F):
        np.testing.assert_allclose(got[f], want[f], **OPT_BARS[dtype])
    assert not bank.weight[:, D + int(has_w):].any()  # pad columns stay zero
    if name == "rowwise_adagrad":
        # both accumulators (fp32 sums of fp32 gradients whatever the bank's dtype):
        # the vector's is mean_d g^2 over dim, not over the row pitch
        rows = bank.category_nums[0]
        s0 = bank.optim_state["s0"].cpu().numpy().astype(np.float64)
        for f in range(F):
            o = bank.row_offset[f]
            np.testing.assert_allclose(s0[o:o + rows, 0], S[f][0], **OPT_BARS[F32])
            np.testing.assert_allclose(s0[o:o + rows, 1], S[f][1][:, 0] if has_w else 0.0,
                                       **OPT_BARS[F32])


@gpu_test
@pytest.mark.parametrize("name", ["rowwise_adagrad", "adagrad", "adam_l2", "adamw_ref"])
@pytest.mark.parametrize("dtype,D,has_w,F", OPT_GEOMS,
                         ids=["%s-F%d" % (_gid(GEOMS.index(g[:3])), g[3]) for g in OPT_GEOMS])
def test_fused_optimizer_geometry(gpu, name, dtype, D, has_w, F):
    """_run of test_gpu_optim.py (rows left stale for several steps: the forward
    catch-up adam_current with live_elems, and flush_optimizer) at other row
    geometries, its bars unchanged."""
    _check_optimizer(name, dtype, D, has_w, F, rows=61, B=96, steps=5, seed=D + F)


@gpu_test
@pytest.mark.parametrize("name", ["adagrad", "adam_l2"])
def test_fused_optimizer_geometry_large_batch(gpu, name):
    """The large-batch path with a fused optimizer and a first-order column at
    fp32 dim 32 + w (LPR 16, 7 dead lanes)."""
    _check_optimizer(name, F32, 32, True, 1, rows=3001, B=10000, steps=3, seed=7, lr=0.01)


# ---------------------------------------------------------------------------
# 4. CPU twin (no GPU): the generator, the oracle calls and the tolerances
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("gi", ALL)
def test_cpu_twin_forward(gi):
    _check_gather(CPU, gi, 5)
    _check_interact(CPU, gi, 5)


@pytest.mark.parametrize("gi", ALL)
def test_cpu_twin_dense_grad(gi):
    _hash_dense_grad(CPU, gi)


@pytest.mark.parametrize("gi", [p for p in ALL if GEOMS[p.values[0]][0] == F32])
def test_cpu_twin_fused_sgd_f32(gi):
    _hash_fused_sgd(CPU, gi, False)
