"""GPU checks of the fused DLRM dot interaction (mrec_dot_interact_fwd / _bwd,
csrc/dot_interact.hip) and of ``DLRM`` on cuda:0.

Shapes are the smallest at which the kernels can go wrong: B in {1, 3, 5, 70} (a workgroup
carries four samples), n in {2, 16, 17, 27, 32} vectors (one pair; either side of the
backward's K-step boundary; Criteo; the full tile), D in {8, 16, 32, 64, 128} (every
instantiation).  Without a bottom vector n = F <= 31, so the full tile becomes n = 31.

1. exact: operands and dx from {-1, 0, 1}; every output is a small integer that bf16 holds,
   so x, dbot, drows equal the int64 computation bit for bit, for every dtype combination;
2. Gaussian operands against fp64 on the bf16-rounded operands, with a derived bound;
3. memory discipline: strides, NaN pads, sentinels;
4. determinism: run to run, and under a move of the samples inside a larger batch;
5. dispatch: the kernels run for compiled shapes only, and the switch turns them off;
6. one ``DLRM.train_step`` against the same model in torch fp64, by the yardstick of
   ``test_c3_dcnv2_train_step_matches_oracle_model``.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from test_dlrm_cpu import (RefDLRM, copy_into_ref, dlrm, dlrm_batch, dlrm_linears, gram_of,
                           pair_count, ref_train_step, vectors)

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
NS = (2, 16, 17, 27, 32)
DS = (8, 16, 32, 64, 128)
DTYPE_COMBOS = list(itertools.product((F32, BF), repeat=4))  # bot, rows, x, dx
U24, U16, U8 = 2.0 ** -24, 2.0 ** -16, 2.0 ** -8


def fields_of(n, with_bot):
    return n - 1 if with_bot else min(n, 31)


def _r8(v):
    return (v + 7) // 8 * 8


def padded(t, dtype, gpu, extra_rows=0, extra_cols=0, fill=float("nan")):
    """t [B, C] as a [B, C] view of a [B + extra_rows, r8(C) + extra_cols] device buffer
    whose other elements hold ``fill`` (rows 16-byte aligned)."""
    B, C = t.shape
    buf = torch.full((B + extra_rows, _r8(C) + extra_cols), fill, dtype=dtype, device=gpu)
    buf[:B, :C] = t.to(gpu).to(dtype)
    return buf, buf[:B, :C]


def raw_args(bot, rows, F, D):
    from pytorchrec_amd import _mrec
    a = _mrec.DotInteractArgs()
    if bot is not None:
        a.bot, a.bot_dtype, a.ld_bot = bot.data_ptr(), _mrec.dtype_code(bot.dtype), bot.stride(0)
    a.rows, a.rows_dtype, a.ld_rows = rows.data_ptr(), _mrec.dtype_code(rows.dtype), rows.stride(0)
    a.batch, a.n_fields, a.D = rows.shape[0], F, D
    return a


def raw_fwd(bot, rows, F, D, x_buf, x_cols, batch=None):
    """mrec_dot_interact_fwd straight on the given views: x_buf is written in place."""
    from pytorchrec_amd import _mrec
    a = raw_args(bot, rows, F, D)
    if batch is not None:
        a.batch = batch
    a.x, a.x_dtype, a.ld_x, a.x_cols = x_buf.data_ptr(), _mrec.dtype_code(x_buf.dtype), x_buf.stride(0), x_cols
    _mrec.call("mrec_dot_interact_fwd", ctypes.byref(a), _mrec.stream_handle())


def raw_bwd(bot, rows, F, D, dx, dbot_buf, drows_buf, batch=None):
    from pytorchrec_amd import _mrec
    a = raw_args(bot, rows, F, D)
    if batch is not None:
        a.batch = batch
    a.dx, a.dx_dtype, a.ld_dx = dx.data_ptr(), _mrec.dtype_code(dx.dtype), dx.stride(0)
    if dbot_buf is not None:
        a.dbot, a.ld_dbot = dbot_buf.data_ptr(), dbot_buf.stride(0)
    a.drows, a.ld_drows = drows_buf.data_ptr(), drows_buf.stride(0)
    _mrec.call("mrec_dot_interact_bwd", ctypes.byref(a), _mrec.stream_handle())


def raw(bot, rows, F, x_cols, x_dtype, dx):
    """The two library calls on device tensors of any dtype combination (autograd hands a
    backward the gradient in x's dtype, so only this reaches dx_dtype != x_dtype)
    -> (x, dbot or None, drows)."""
    gpu, B, D = rows.device, rows.shape[0], rows.shape[1] // F
    b = padded(bot, bot.dtype, gpu)[1] if bot is not None else None
    r = padded(rows, rows.dtype, gpu)[1]
    d = padded(dx, dx.dtype, gpu)[1]
    x = padded(torch.zeros(B, x_cols), x_dtype, gpu)[1]
    dbot = padded(torch.zeros(B, D), bot.dtype, gpu)[1] if bot is not None else None
    drows = padded(torch.zeros(B, F * D), rows.dtype, gpu)[1]
    raw_fwd(b, r, F, D, x, x_cols)
    raw_bwd(b, r, F, D, d, dbot, drows)
    return x, dbot, drows


def fused(bot, rows, F, x_cols, x_dtype, dx):
    """dense.dot_interact forward + backward on device tensors -> (x, dbot or None, drows).
    ``dx`` reaches the backward in x's dtype, whatever its own."""
    from pytorchrec_amd import dense
    b = bot.detach().requires_grad_() if bot is not None else None
    r = rows.detach().requires_grad_()
    x = dense.dot_interact(b, r, F, x_cols=x_cols, x_dtype=x_dtype)
    x.backward(dx)
    return x.detach(), (b.grad if b is not None else None), r.grad


# ---------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------

def ternary_case(B, n, D, with_bot, seed):
    """Operands and dx from {-1, 0, 1} and the int64 results: (bot, rows, dx, x, dbot, drows),
    x_cols = D + P + 3 (a scalar tail behind the last whole vector)."""
    g = torch.Generator().manual_seed(seed)
    F = fields_of(n, with_bot)
    nv = F + with_bot
    Dh = D if with_bot else 0
    P = pair_count(nv)
    x_cols = Dh + P + 3
    rows = torch.randint(-1, 2, (B, F * D), generator=g)
    bot = torch.randint(-1, 2, (B, D), generator=g) if with_bot else None
    dx = torch.randint(-1, 2, (B, x_cols), generator=g)
    t = rows.reshape(B, F, D)
    if with_bot:
        t = torch.cat([bot.unsqueeze(1), t], 1)
    z = torch.bmm(t.double(), t.double().transpose(1, 2)).long()  # (exact: |z| <= 128)
    li, lj = torch.tril_indices(nv, nv, -1)
    x = torch.zeros(B, x_cols, dtype=torch.int64)
    if with_bot:
        x[:, :D] = bot
    x[:, Dh:Dh + P] = z[:, li, lj]
    G = torch.zeros(B, nv, nv, dtype=torch.int64)
    G[:, li, lj] = dx[:, Dh:Dh + P]
    G = G + G.transpose(1, 2)
    dt = torch.bmm(G.double(), t.double()).long()
    dbot = dt[:, 0] + dx[:, :D] if with_bot else None
    drows = dt[:, with_bot:].reshape(B, F * D)
    assert int(x.abs().max()) <= 128 and int(dt.abs().max()) <= 32
    return F, x_cols, bot, rows, dx, x, dbot, drows


def check_exact(gpu, B, n, D, with_bot, combos):
    F, x_cols, bot, rows, dx, x, dbot, drows = ternary_case(B, n, D, with_bot, 1000 * n + D + B)
    for bd, rd, xd, dd in combos:
        # the library calls for every combination; through autograd too where it can be
        for run in (raw, fused) if xd == dd else (raw,):
            got = run(bot.to(gpu).to(bd) if with_bot else None, rows.to(gpu).to(rd), F, x_cols, xd,
                      dx.to(gpu).to(dd))
            what = (run.__name__, B, n, D, with_bot, bd, rd, xd, dd)
            assert got[0].dtype == xd and got[2].dtype == rd, what
            assert torch.equal(got[0].cpu().double().long(), x), what
            assert torch.equal(got[2].cpu().double().long(), drows), what
            if with_bot:
                assert got[1].dtype == bd and torch.equal(got[1].cpu().double().long(), dbot), what


@pytest.mark.parametrize("with_bot", [True, False], ids=["bot", "nobot"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_exact_every_dtype_combination(gpu, monkeypatch, n, D, with_bot):
    from pytorchrec_amd import _mrec
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    # (without bot its dtype does not matter: half the combinations)
    combos = DTYPE_COMBOS if with_bot else [c for c in DTYPE_COMBOS if c[0] == F32]
    check_exact(gpu, 70, n, D, with_bot, combos)
    runs = len(combos) + sum(c[2] == c[3] for c in combos)
    assert calls.count("mrec_dot_interact_fwd") == runs == calls.count("mrec_dot_interact_bwd")


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("n,D", [(2, 8), (27, 16), (17, 32), (32, 128)])
def test_exact_small_batches(gpu, B, n, D):
    for with_bot in (True, False):
        check_exact(gpu, B, n, D, with_bot, [(F32, F32, F32, F32), (BF, BF, BF, BF), (F32, BF, F32, BF)])


def test_empty_batch(gpu):
    bot, rows = torch.zeros(0, 16, device=gpu), torch.zeros(0, 5 * 16, device=gpu)
    x, dbot, drows = fused(bot, rows, 5, 32, BF, torch.zeros(0, 32, dtype=BF, device=gpu))
    assert tuple(x.shape) == (0, 32) and tuple(dbot.shape) == (0, 16) and tuple(drows.shape) == (0, 80)


# ---------------------------------------------------------------------------
# 2. Gaussian operands against fp64 on the bf16-rounded operands
# ---------------------------------------------------------------------------

def gaussian_case(B, n, D, with_bot, seed, bot_dtype, rows_dtype, dx_dtype):
    """N(0, 1) operands as the given dtypes hold them, and dx."""
    g = torch.Generator().manual_seed(seed)
    F = fields_of(n, with_bot)
    Dh = D if with_bot else 0
    x_cols = _r8(Dh + pair_count(F + with_bot))
    rows = torch.randn(B, F * D, generator=g).to(rows_dtype)
    bot = torch.randn(B, D, generator=g).to(bot_dtype) if with_bot else None
    dx = torch.randn(B, x_cols, generator=g).to(dx_dtype)
    return F, x_cols, bot, rows, dx


def bounds(bot, rows, F, D, x_cols, dx, x_dtype):
    """fp64 results on the bf16-rounded operands and the derived error bounds.

    Forward: products of bf16 values are exact in fp32, and any order of the D fp32 additions
    errs by at most D 2^-24 sum_d |t_i[d] t_j[d]|; a bf16 x adds half an ulp, 2^-8 |z| (and
    2^-8 |t_0| where an fp32 t_0 is copied into a bf16 x).  Backward: n terms per output, each
    coefficient exact (bf16 dx) or hi + lo with 2^-16 (fp32 dx): (n 2^-24 + c) sum_j |G[i, j]
    t_j[d]|; dbot takes one more fp32 addition, 2^-24 |dbot|; a bf16 output adds 2^-8 of it.
    -> ((x, bound), (dbot, bound) or None, (drows, bound))"""
    with_bot = bot is not None
    B = rows.shape[0]
    r64 = rows.bfloat16().double().numpy()
    b64 = bot.bfloat16().double().numpy() if with_bot else None
    t = vectors(b64, r64, F, D)
    n = t.shape[1]
    Dh = D if with_bot else 0
    P = pair_count(n)
    li, lj = np.tril_indices(n, -1)
    z = np.einsum("bid,bjd->bij", t, t)[:, li, lj]
    za = np.einsum("bid,bjd->bij", np.abs(t), np.abs(t))[:, li, lj]
    x = np.zeros((B, x_cols))
    xb = np.zeros((B, x_cols))
    x[:, Dh:Dh + P] = z
    xb[:, Dh:Dh + P] = D * U24 * za + (U8 * np.abs(z) if x_dtype == BF else 0.0)
    if with_bot:
        x[:, :D] = bot.double().numpy()  # the copy is not rounded to bf16 first
        xb[:, :D] = U8 * np.abs(x[:, :D]) if (x_dtype == BF and bot.dtype == F32) else 0.0
    dx64 = dx.double().numpy()
    G = gram_of(dx64, n, Dh)
    dt = np.einsum("bij,bjd->bid", G, t)
    da = np.einsum("bij,bjd->bid", np.abs(G), np.abs(t))
    c = 0.0 if dx.dtype == BF else U16
    db = (n * U24 + c) * da
    drows = dt[:, with_bot:].reshape(B, F * D)
    drows_b = db[:, with_bot:].reshape(B, F * D) + (U8 * np.abs(drows) if rows.dtype == BF else 0.0)
    if not with_bot:
        return (x, xb), None, (drows, drows_b)
    dbot = dt[:, 0] + dx64[:, :D]
    dbot_b = db[:, 0] + U24 * np.abs(dbot) + (U8 * np.abs(dbot) if bot.dtype == BF else 0.0)
    return (x, xb), (dbot, dbot_b), (drows, drows_b)


def assert_within(got, want_bound, what):
    want, bound = want_bound
    err = np.abs(got.detach().double().cpu().numpy() - want)
    tiny = 1e-300
    worst = float(np.max(err / (bound + tiny) * (err > 0)))
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


GAUSS_COMBOS = [(F32, F32, F32, F32), (BF, BF, BF, BF), (F32, BF, BF, F32), (BF, F32, F32, BF)]


@pytest.mark.parametrize("with_bot", [True, False], ids=["bot", "nobot"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_gaussian_within_the_derived_bound(gpu, n, D, with_bot):
    for bd, rd, xd, dd in GAUSS_COMBOS:
        F, x_cols, bot, rows, dx = gaussian_case(70, n, D, with_bot, 7 * n + D, bd, rd, dd)
        got = raw(bot.to(gpu) if with_bot else None, rows.to(gpu), F, x_cols, xd, dx.to(gpu))
        wx, wbot, wrows = bounds(bot, rows, F, D, x_cols, dx, xd)
        tag = f"n={n} D={D} bot={with_bot} {bd} {rd} {xd} {dd}"
        assert_within(got[0], wx, "x " + tag)
        assert_within(got[2], wrows, "drows " + tag)
        if with_bot:
            assert_within(got[1], wbot, "dbot " + tag)


# ---------------------------------------------------------------------------
# 3. memory discipline
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_bot", [True, False], ids=["bot", "nobot"])
@pytest.mark.parametrize("n,D", [(2, 8), (27, 16), (17, 32), (32, 128)])
def test_strides_nan_pads_and_sentinels(gpu, n, D, with_bot, dtype):
    B, SENT = 5, 7.0
    F, _, bot, rows, dx = gaussian_case(B, n, D, with_bot, 31 * n + D, dtype, dtype, dtype)
    Dh = D if with_bot else 0
    P = pair_count(F + with_bot)
    x_cols = Dh + P + 11  # zeros behind the pairs, ending inside a 16-byte vector
    dx = torch.randn(B, x_cols, generator=torch.Generator().manual_seed(5)).to(dtype)
    # tight call: exact widths, r8 pitches
    tb = padded(bot, dtype, gpu)[1] if with_bot else None
    tr = padded(rows, dtype, gpu)[1]
    tdx = padded(dx, dtype, gpu)[1]
    tx = padded(torch.zeros(B, x_cols), dtype, gpu)[1]
    tdb = padded(torch.zeros(B, D), dtype, gpu)[1] if with_bot else None
    tdr = padded(torch.zeros(B, F * D), dtype, gpu)[1]
    raw_fwd(tb, tr, F, D, tx, x_cols)
    raw_bwd(tb, tr, F, D, tdx, tdb, tdr)
    # wide call: larger strides, NaN in every pad column and in the rows past the batch of
    # the inputs (dx's columns >= D + P included), a sentinel all over the outputs
    wb = padded(bot, dtype, gpu, 2, 8)[1] if with_bot else None
    wr = padded(rows, dtype, gpu, 2, 16)[1]
    dxn = dx.clone()
    dxn[:, Dh + P:] = float("nan")
    wdx = padded(dxn, dtype, gpu, 2, 8)[1]
    xbuf, wx = padded(torch.full((B, x_cols), SENT), dtype, gpu, 3, 8, fill=SENT)
    dbbuf, wdb = padded(torch.full((B, D), SENT), dtype, gpu, 3, 8, fill=SENT) if with_bot else (None, None)
    drbuf, wdr = padded(torch.full((B, F * D), SENT), dtype, gpu, 3, 8, fill=SENT)
    raw_fwd(wb, wr, F, D, wx, x_cols)
    raw_bwd(wb, wr, F, D, wdx, wdb, wdr)
    torch.cuda.synchronize()
    for name, tight, wide, buf, cols in (("x", tx, wx, xbuf, x_cols), ("dbot", tdb, wdb, dbbuf, D),
                                         ("drows", tdr, wdr, drbuf, F * D)):
        if tight is None:
            continue
        assert bool(torch.isfinite(wide.float()).all()), name
        assert torch.equal(wide, tight), name
        assert bool((buf[:B, cols:] == SENT).all()), name + ": columns past the width"
        assert bool((buf[B:] == SENT).all()), name + ": rows past the batch"
    assert bool((wx[:, Dh + P:] == 0).all()) and not bool((wx[:, Dh:Dh + P] == 0).all())
    # a batch smaller than the buffers: the rows past it keep the sentinel too
    xbuf.fill_(SENT)
    raw_fwd(wb, wr, F, D, wx, x_cols, batch=B - 2)
    torch.cuda.synchronize()
    assert torch.equal(wx[:B - 2], tx[:B - 2]) and bool((xbuf[B - 2:] == SENT).all())


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,D", [(27, 16), (17, 64), (32, 128)])
def test_bits_do_not_depend_on_run_or_position(gpu, n, D, dtype):
    F, x_cols, bot, rows, dx = gaussian_case(70, n, D, True, 3 * n + D, dtype, dtype, dtype)
    bot, rows, dx = bot.to(gpu), rows.to(gpu), dx.to(gpu)
    a = fused(bot, rows, F, x_cols, dtype, dx)
    b = fused(bot, rows, F, x_cols, dtype, dx)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    pos = torch.tensor([69, 3, 34, 0, 17], device=gpu)  # the small batch's samples, in its order
    s = fused(bot[pos], rows[pos], F, x_cols, dtype, dx[pos])
    for u, v in zip(a, s):
        assert torch.equal(u[pos], v)


# ---------------------------------------------------------------------------
# 5. dispatch
# ---------------------------------------------------------------------------

def _spy(monkeypatch):
    """Every libmrec call by name."""
    from pytorchrec_amd import _mrec
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


KERNELS = {"mrec_dot_interact_fwd", "mrec_dot_interact_bwd"}


def test_compiled_shape_runs_both_kernels(gpu, monkeypatch):
    calls = _spy(monkeypatch)
    F, x_cols, bot, rows, dx = gaussian_case(9, 27, 16, True, 1, BF, BF, BF)
    fused(bot.to(gpu), rows.to(gpu), F, x_cols, BF, dx.to(gpu))
    assert calls == ["mrec_dot_interact_fwd", "mrec_dot_interact_bwd"]


@pytest.mark.parametrize("how", ["switch", "D24", "F32"])
def test_the_switch_and_unsupported_shapes_take_the_torch_ops(gpu, monkeypatch, how):
    from pytorchrec_amd import cpu_path, dense
    F, D = {"switch": (26, 16), "D24": (5, 24), "F32": (32, 16)}[how]
    if how == "switch":
        monkeypatch.setattr(dense, "DOT_INTERACT", False)
    else:
        assert dense.DOT_INTERACT and not dense.dot_interact_supported(D, F)
    B = 9
    g = torch.Generator().manual_seed(2)
    rows, bot = torch.randn(B, F * D, generator=g), torch.randn(B, D, generator=g)
    x_cols = _r8(D + pair_count(F + 1))
    dx = torch.randn(B, x_cols, generator=g)
    calls = _spy(monkeypatch)
    got = fused(bot.to(gpu), rows.to(gpu), F, x_cols, F32, dx.to(gpu))
    assert not KERNELS & set(calls)
    b, r = bot.to(gpu).requires_grad_(), rows.to(gpu).requires_grad_()
    want = cpu_path.dot_interact(b, r, F, D, x_cols, round_bf16=True)
    want.backward(dx.to(gpu))
    # (the same torch ops on both sides: within the bound of test 2, in fact equal)
    wx, wbot, wrows = bounds(bot, rows, F, D, x_cols, dx, F32)
    for name, g_, w_, (_, bound) in (("x", got[0], want, wx), ("dbot", got[1], b.grad, wbot),
                                     ("drows", got[2], r.grad, wrows)):
        err = (g_.double() - w_.detach().double()).abs().cpu().numpy()
        print(f"{how} {name}: max |diff| {err.max():.3e}")
        assert np.all(err <= bound), (how, name, float(err.max()))


# ---------------------------------------------------------------------------
# 6. the model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("emb_dtype", [F32, BF], ids=["fp32", "bf16"])
def test_dlrm_train_step_matches_the_fp64_model(gpu, monkeypatch, emb_dtype):
    """One DLRM train step (B = 256, 6 fields of 50 rows, 3 dense, D = 16, bottom [32, 16],
    top [64, 32], BCEWithLogitsLoss, plain SGD fused into the backward kernels) against
    RefDLRM in fp64 from identical weights: the loss within 2e-3 and every parameter's
    UPDATE.  The yardstick is test_c3_dcnv2_train_step_matches_oracle_model's: the same model
    in torch fp32 with bf16 rounding at the build's storage points (RefDLRM(bf16_points=True),
    run here on the GPU) says what bf16 storage alone costs, and the kernels' distance to
    fp64 may not exceed 1.5x that plus 1 % of the update, in L2 and in max norm.  Tables fp32
    and bf16 (RNE, lr 1e4 so that the table updates are many bf16 ulps and the emulation's
    tables are rounded the same way)."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    bf16 = emb_dtype == BF
    B, lr = 256, (1e4 if bf16 else 1.0)
    nums, nd, D, bottom, top = [50] * 6, 3, 16, (32, 16), (64, 32)
    m = dlrm(rows=50, F=6, n_dense=nd, D=D, bottom=bottom, top=top, device=gpu, emb_dtype=emb_dtype,
             random_seed=2020)
    m.embeddings.stochastic_rounding = False
    with torch.no_grad():  # weights large enough that every layer matters
        for lin in dlrm_linears(m):
            lin.weight.mul_(10.0)
            lin.bias.mul_(10.0)
        m.embeddings.weight.mul_(30.0)
    assert m.embeddings.weight.dtype == emb_dtype
    r = RefDLRM(nums, nd, D, bottom, top)
    copy_into_ref(m, r)
    data, ids, dense, label = dlrm_batch(m, B)
    data = {k: v.to(gpu) for k, v in data.items()}
    before_state = [v.clone() for v in r.state_dict().values()]
    before_t = [e.weight.detach().clone() for e in r.emb]
    before_l = [(x.weight.detach().clone(), x.bias.detach().clone()) for x in r.linears()]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], gpu)
    assert m.embeddings.update == "sgd"
    calls = _spy(monkeypatch)
    loss = float(m.train_step(data)["loss"].detach())
    for name in ("mrec_emb_gather_fwd", "mrec_dot_interact_fwd", "mrec_dot_interact_bwd",
                 "mrec_tower_fwd_bwd"):
        assert name in calls, (name, calls)
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    print(f"loss {loss:.6f} against {rloss:.6f}")
    assert abs(loss - rloss) <= 2e-3 * max(1.0, abs(rloss)), (loss, rloss)
    e = RefDLRM(nums, nd, D, bottom, top, dtype=torch.float32, bf16_points=True)
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

    rnd = (lambda t: t.detach().to(BF)) if bf16 else (lambda t: t.detach())  # noqa: E731
    for f in range(len(nums)):
        upd_close(m.embeddings.table(f).detach(), rnd(e.emb[f].weight), r.emb[f].weight.detach(),
                  before_t[f], f"table{f}")
    for i, (a, b_, c_) in enumerate(zip(dlrm_linears(m), r.linears(), e.linears())):
        upd_close(a.weight.detach(), c_.weight.detach(), b_.weight.detach(), before_l[i][0], f"W{i}")
        upd_close(a.bias.detach(), c_.bias.detach(), b_.bias.detach(), before_l[i][1], f"b{i}")
