"""The fused NCF pair scorer (mrec_ncf_fwd / _bwd + mrec_sasrec_wgrad, ncf.hip) on the GPU.

1. Parity with an fp64 restatement on every pair with the layered GPU path as the
   yardstick.  Bars (those of test_gpu_sasrec.py / test_gpu_gru4rec.py, whose helpers this
   file uses): per quantity, max error <= max(tol, 1.5 x the layered path's max error)
   with tol 3e-2 forward / 5e-2 gradients, relative to the quantity's magnitude, and mean
   error <= max(3e-3, 1.5 x the layered path's mean error).  Both GPU paths round the
   weight matrices and every MLP operand to bf16; the fp64 restatement rounds nothing.

2. Exact-integer edges, by the method of test_gpu_tower_exact.py.  Rows hold -1 / 0 / 1,
   the MLP weights are sparse with entries +-1, biases and wp are small integers and
   dpred is +-2^-10 or twice that.  Then every activation is a small integer and every
   gradient a small multiple of 2^-10: each value the kernel rounds to bf16 is unchanged
   by it and each fp32 sum is exact in any order.  The expected value is computed in fp64
   on the CPU and every comparison is ``torch.equal``.  The conditions on the inputs are
   asserted by the generator and checked on the CPU by ``test_exact_case_conditions``
   (no GPU): representable (every h_l, dz_l, dh_0 and d mf survive a bf16 round trip),
   order independent (sum |terms| < 2^24 quanta for every fp32 accumulation), sensitive
   (every ReLU active on 25-75 % of its elements, every 16 x 16 -- hence every 16 x 32 --
   block of every weight, edge blocks included, holds a non-zero, every live pair has
   dpred != 0).  Operands and outputs are windows of larger allocations: what must not be
   read is NaN, outputs start as 7.0 and rows >= pairs, columns >= 4E and the guards are
   still 7.0 afterwards.  No case provokes a fault.

3. Run-to-run bit equality, placement independence, the fallbacks to the layered path,
   and goldens G7 / G17 through the whole model on cuda:0.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_gru4rec import _errs, _meets_bars
from test_ncf_cpu import KEYS, g7_state, g17_batch, g17_state, ncf, widths_arr

gpu_test = pytest.mark.gpu
BF16 = torch.bfloat16


def _tile():
    from pytorchrec_amd import _mrec
    return int(_mrec.lib().mrec_ncf_tile())


def _second_tile_pairs():
    """More tiles than workgroups: some workgroup takes a second tile."""
    from pytorchrec_amd import _mrec
    return (int(_mrec.lib().mrec_ncf_parts(1 << 20)) + 1) * _tile() + 3


def _params(m):
    from pytorchrec_amd import dense as D
    ws, bs, wp = D._ncf_params(m)
    return [*ws, *bs, wp]


def _names(nl):
    return [f"dW{l}" for l in range(nl)] + [f"db{l}" for l in range(nl)] + ["dWp"]


def lively_(m, seed, scale=0.3):
    """State-B scale: every dense tensor ``scale`` N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in _params(m):
            p.copy_((scale * torch.randn(p.shape, generator=g)).to(p.device))
    return m


# ---------------------------------------------------------------------------
# 1. parity with fp64
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(pairs, E, layers, dropout=0.0):
    """(model, rows bf16 [pairs, 4E], dpred) on cuda:0."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + pairs % 997 + E)
    m = lively_(ncf(emb_size=E, layers=list(layers), dropout=dropout, device=dev), 7 + E + len(layers))
    rows = (0.5 * torch.randn(pairs, 4 * E, generator=g)).to(BF16).to(dev)
    dpred = torch.randn(pairs, generator=g).to(dev)
    return m, rows, dpred


def _score64(x, E, ws, bs, wp):
    g = x[:, :E] * x[:, E:2 * E]
    h = x[:, 2 * E:]
    for w, b in zip(ws, bs):
        h = torch.relu(h @ w.T + b)
    return torch.cat([g, h], 1) @ wp.reshape(-1)


@functools.lru_cache(maxsize=None)
def _ref64(pairs, E, layers):
    """fp64 torch restatement of the scorer and its gradients (computed once)."""
    m, rows, dpred = _case(pairs, E, layers)
    nl = len(layers)
    x = rows.detach().double().cpu().requires_grad_()
    ps = [p.detach().double().cpu().requires_grad_() for p in _params(m)]
    pred = _score64(x, E, ps[:nl], ps[nl:2 * nl], ps[2 * nl])
    pred.backward(dpred.double().cpu())
    ref = {"prediction": pred.detach(), "dX": x.grad}
    ref.update({n: p.grad for n, p in zip(_names(nl), ps)})
    return ref


def _run(case, fused, monkeypatch, rows=None, dpred=None, train=False):
    """One forward + backward of dense.ncf_score -> {prediction, dX, d<param>}."""
    from pytorchrec_amd import dense as D
    m, rows0, dpred0 = case
    monkeypatch.setattr(D, "NCF_FUSED", fused)
    for p in _params(m):
        p.grad = None
    x = (rows0 if rows is None else rows).detach().clone().requires_grad_()
    pred = D.ncf_score(x, m.train() if train else m.eval())
    assert ("Ncf" in type(pred.grad_fn).__name__) == fused
    pred.backward(dpred0 if dpred is None else dpred)
    got = {"prediction": pred.detach(), "dX": x.grad}
    got.update({n: p.grad.clone() for n, p in zip(_names(len(m.layers)), _params(m))})
    return got


def _shapes():
    return [(1, 8, (16, 8)), ("T-1", 16, (32, 16, 8)), ("T", 16, (32, 16, 8)),
            ("T+1", 16, (32, 16, 8)), (96, 8, (16, 8)), (300, 32, (64, 32, 16)),
            (200, 64, (128, 64, 32)), (130, 64, (64,)), ("second", 8, (16, 8))]


def _pairs(spec):
    if isinstance(spec, int):
        return spec
    return {"T-1": _tile() - 1, "T": _tile(), "T+1": _tile() + 1}.get(spec) or _second_tile_pairs()


@gpu_test
@pytest.mark.parametrize("pairs,E,layers", _shapes())
def test_fused_scorer_matches_fp64_reference(gpu, monkeypatch, pairs, E, layers):
    """pred, the rows' gradient and every dense gradient on every pair: one pair, the tile
    edges, G7's batch, every required tower, and more tiles than workgroups (a workgroup's
    accumulators carry over into its second tile)."""
    pairs = _pairs(pairs)
    case, ref = _case(pairs, E, layers), _ref64(pairs, E, layers)
    errs = {}
    for fused in (True, False):
        got = _run(case, fused, monkeypatch)
        assert set(got) == set(ref)
        for name, t in got.items():
            assert t.shape == ref[name].shape, name
            assert torch.isfinite(t.float()).all(), (fused, name)
            errs[(fused, name)] = _errs(t, ref[name])
        if fused:
            assert got["dX"].dtype == BF16 and got["prediction"].dtype == torch.float32
    _meets_bars(errs, list(ref))


@gpu_test
def test_two_runs_are_bitwise_equal(gpu, monkeypatch):
    from pytorchrec_amd import dense as D
    case = _case(300, 32, (64, 32, 16))
    a, b = _run(case, True, monkeypatch), _run(case, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    with torch.no_grad():  # a forward on its own gives the same bits
        again = D.ncf_score(case[1], case[0].eval())
    assert torch.equal(again, a["prediction"])
    big = _case(_second_tile_pairs(), 8, (16, 8))
    a, b = _run(big, True, monkeypatch), _run(big, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name


@gpu_test
@pytest.mark.parametrize("pairs,E,layers", [(300, 32, (64, 32, 16)), ("second", 8, (16, 8))])
def test_a_pairs_bits_do_not_depend_on_its_place(gpu, monkeypatch, pairs, E, layers):
    """The same pairs in a permuted order: pred and d_rows are bitwise equal per pair; the
    dense gradients agree to 1e-5 of their magnitude (only their summation order moved)."""
    pairs = _pairs(pairs)
    case = _case(pairs, E, layers)
    m, rows, dpred = case
    perm = torch.randperm(pairs, generator=torch.Generator().manual_seed(4)).to(rows.device)
    base = _run(case, True, monkeypatch)
    got = _run(case, True, monkeypatch, rows=rows[perm].contiguous(), dpred=dpred[perm].contiguous())
    assert torch.equal(got["prediction"], base["prediction"][perm])
    assert torch.equal(got["dX"], base["dX"][perm])
    for name in _names(len(layers)):
        fmax, _ = _errs(got[name], base[name].double().cpu())
        assert fmax <= 1e-5, (name, fmax)


# ---------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------

def _direct(case, train=False):
    """cpu_path.ncf_score with the kernel's rounding points, called directly."""
    from pytorchrec_amd import cpu_path, dense as D
    m, rows, dpred = case
    for p in _params(m):
        p.grad = None
    x = rows.clone().requires_grad_()
    ws, bs, wp = D._ncf_params(m)
    pred = cpu_path.ncf_score(x, m.emb_size, ws, bs, wp, rnd=cpu_path.bf16_round,
                              dropout=m.dropout, training=train)
    pred.backward(dpred)
    return [pred.detach(), x.grad] + [p.grad.clone() for p in _params(m)]


@gpu_test
def test_the_switch_selects_the_layered_path_bit_for_bit(gpu, monkeypatch):
    """NCF_FUSED = False is cpu_path.ncf_score with bf16 rounding, bit for bit (its
    agreement with the fused path within the bars is the parity test above)."""
    case = _case(96, 8, (16, 8))
    got = _run(case, False, monkeypatch)
    for a, b in zip(got.values(), _direct(case)):
        assert torch.equal(a, b)


@gpu_test
@pytest.mark.parametrize("E,layers", [(24, (16, 8)), (8, (20, 8)), (8, (16, 8, 8, 8)), (8, (136,))])
def test_unsupported_shapes_take_the_layered_path(gpu, monkeypatch, E, layers):
    """With the switch on, a shape outside mrec_ncf_supported runs cpu_path.ncf_score with
    bf16 rounding, bit for bit (there is no fused result to compare with); its forward
    meets the forward bar against fp64 on its own."""
    from pytorchrec_amd import dense
    assert dense.NCF_FUSED and not dense.ncf_supported(E, layers)
    case = _case(70, E, layers)
    m, rows, dpred = case
    for p in _params(m):
        p.grad = None
    x = rows.clone().requires_grad_()
    pred = dense.ncf_score(x, m.eval())
    assert "Ncf" not in type(pred.grad_fn).__name__
    pred.backward(dpred)
    got = [pred.detach(), x.grad] + [p.grad.clone() for p in _params(m)]
    for i, (a, b) in enumerate(zip(got, _direct(case))):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), i
    fmax, fmean = _errs(got[0], _ref64(70, E, layers)["prediction"])
    assert fmax <= 3e-2 and fmean <= 3e-3, (fmax, fmean)


@gpu_test
def test_active_dropout_takes_the_layered_path(gpu, monkeypatch):
    """dropout > 0: training runs the layered path with torch dropout (the same bits as
    cpu_path.ncf_score called directly under the same seed, and not the eval bits); eval
    runs the fused kernels and equals the dropout-free model bit for bit."""
    case = _case(96, 8, (16, 8), 0.5)
    plain = _case(96, 8, (16, 8))
    assert case[0].dropout == 0.5 and all(torch.equal(a, b) for a, b in
                                          zip(_params(case[0]), _params(plain[0])))
    torch.manual_seed(3)
    got = _run(case, False, monkeypatch, train=True)  # NCF_FUSED False: certainly layered
    from pytorchrec_amd import dense
    monkeypatch.setattr(dense, "NCF_FUSED", True)
    m, rows, dpred = case
    torch.manual_seed(3)
    pred = dense.ncf_score(rows.clone().requires_grad_(), m.train())
    assert "Ncf" not in type(pred.grad_fn).__name__
    assert torch.equal(pred.detach(), got["prediction"])
    torch.manual_seed(3)
    for a, b in zip(got.values(), _direct(case, train=True)):
        assert torch.equal(a, b)
    fused_eval = _run(case, True, monkeypatch)
    want = _run(plain, True, monkeypatch)
    for name in want:
        assert torch.equal(fused_eval[name], want[name]), name
    assert not torch.equal(got["prediction"], want["prediction"])
    m.eval()


# ---------------------------------------------------------------------------
# 2. exact-integer edges
# ---------------------------------------------------------------------------

Q = 2.0 ** -10  # the backward's quantum: the smallest |dpred|
SENT = 7.0
NAN = float("nan")


class Exact:
    """One exact-integer case; ``pairs`` may be given relative to the tile T."""

    def __init__(self, name, pairs, E, layers, seed, nnz=4):
        self.name, self.pairs_spec, self.E, self.layers, self.seed, self.nnz = (
            name, pairs, E, tuple(layers), seed, nnz)

    def __repr__(self):
        return self.name

    def pairs(self, T):
        a, b = self.pairs_spec
        return a * T + b


# pairs = a T + b
EXACT = [
    Exact("p1_e8_w8", (0, 1), 8, (8,), 0),                  # one pair, one layer, width 8
    Exact("Tm1_e8_16_8", (1, -1), 8, (16, 8), 0),           # K = 16: half a k step
    Exact("Tp1_e16_32_24_8", (1, 1), 16, (32, 24, 8), 0),   # three layers, width 24
    Exact("2Tp5_e8_24_16", (2, 5), 8, (24, 16), 0),         # three tiles, width 24 first
    Exact("Tp1_e64_128_64_32", (1, 1), 64, (128, 64, 32), 0, nnz=3),  # the NeuMF tower
]


def _bf16_exact(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()
    return bool(torch.equal(t.to(BF16).float(), t))


def _exact_inputs(case, T=64):
    """Integer inputs and the fp64 restatement of the contract, with the conditions
    asserted.  Deterministic in (case, T)."""
    rng = np.random.default_rng(1234 + case.seed)
    pairs, E, nl = case.pairs(T), case.E, len(case.layers)
    rows = rng.integers(-1, 2, size=(pairs, 4 * E)).astype(np.float64)
    ws, bs = [], []
    K = 2 * E
    for N in case.layers:
        w = np.zeros((N, K))
        for n in range(N):
            cols = rng.choice(K, size=min(case.nnz, K), replace=False)
            w[n, cols] = rng.choice([-1.0, 1.0], size=cols.size)
        for n0 in range(0, N, 16):  # every 16 x 16 block (edge blocks too) holds a non-zero
            for k0 in range(0, K, 16):
                blk = w[n0:n0 + 16, k0:k0 + 16]
                if not blk.any():
                    blk[rng.integers(blk.shape[0]), rng.integers(blk.shape[1])] = rng.choice([-1.0, 1.0])
        ws.append(w)
        bs.append(rng.integers(0, 3, size=N).astype(np.float64))
        K = N
    wp = rng.choice([-2.0, -1.0, 1.0, 2.0], size=E + K)
    dpred = rng.choice([-2 * Q, -Q, Q, 2 * Q], size=pairs)
    # the contract in fp64
    g = rows[:, :E] * rows[:, E:2 * E]
    hs = [rows[:, 2 * E:]]
    for w, b in zip(ws, bs):
        hs.append(np.maximum(hs[-1] @ w.T + b, 0.0))
    pred = g @ wp[:E] + hs[-1] @ wp[E:]
    d_rows = np.zeros_like(rows)
    d_rows[:, :E] = dpred[:, None] * wp[None, :E] * rows[:, E:2 * E]
    d_rows[:, E:2 * E] = dpred[:, None] * wp[None, :E] * rows[:, :E]
    dwp = np.concatenate([dpred @ g, dpred @ hs[-1]])
    dh = dpred[:, None] * wp[None, E:]
    dws, dbs, dzs = [None] * nl, [None] * nl, [None] * nl
    for l in range(nl - 1, -1, -1):
        dz = dh * (hs[l + 1] > 0)
        dzs[l], dws[l], dbs[l] = dz, dz.T @ hs[l], dz.sum(0)
        dh = dz @ ws[l]
    d_rows[:, 2 * E:] = dh
    out = dict(rows=rows, ws=ws, bs=bs, wp=wp, dpred=dpred, hs=hs, dzs=dzs, pred=pred, d_rows=d_rows,
               dws=dws, dbs=dbs, dwp=dwp, g=g)
    _assert_conditions(case, out)
    return out


def _assert_conditions(case, c):
    E, nl = case.E, len(case.layers)
    # representable
    for l, h in enumerate(c["hs"]):
        assert _bf16_exact(h) and np.abs(h).max() <= 256, (case, "h", l, np.abs(h).max())
    for l, dz in enumerate(c["dzs"]):
        assert _bf16_exact(dz) and np.abs(dz).max() <= 256 * Q, (case, "dz", l, np.abs(dz).max() / Q)
    assert _bf16_exact(c["d_rows"]) and np.abs(c["d_rows"]).max() <= 256 * Q, (
        case, "d_rows", np.abs(c["d_rows"]).max() / Q)
    # order independent: sum |terms| < 2^24 quanta (1 forward, Q backward)
    lim = float(2 ** 24)
    for l, w in enumerate(c["ws"]):
        assert (np.abs(c["hs"][l]) @ np.abs(w).T + np.abs(c["bs"][l])).max() < lim
        assert (np.abs(c["dzs"][l]) @ np.abs(w)).max() / Q < lim
        assert (np.abs(c["dzs"][l]).T @ np.abs(c["hs"][l])).max() / Q < lim
        assert np.abs(c["dzs"][l]).sum(0).max() / Q < lim
    assert (np.abs(c["g"]) @ np.abs(c["wp"][:E]) + np.abs(c["hs"][-1]) @ np.abs(c["wp"][E:])).max() < lim
    assert max((np.abs(c["dpred"]) @ np.abs(c["g"])).max(),
               (np.abs(c["dpred"]) @ np.abs(c["hs"][-1])).max()) / Q < lim
    # sensitive
    for l, w in enumerate(c["ws"]):
        active = float((c["hs"][l + 1] > 0).mean())
        assert 0.25 <= active <= 0.75, (case, "relu", l, active)
        for n0 in range(0, w.shape[0], 16):
            for k0 in range(0, w.shape[1], 16):
                assert w[n0:n0 + 16, k0:k0 + 16].any(), (case, "block", l, n0, k0)
    assert (c["dpred"] != 0).all() and (c["wp"] != 0).all()
    for name in ("dws", "dbs"):
        for l in range(nl):
            assert np.any(c[name][l] != 0), (case, name, l)


@pytest.mark.parametrize("case", EXACT, ids=repr)
def test_exact_case_conditions(case):
    """The generator's conditions, on the CPU, for every case of the matrix (the tile is
    64 pairs; the GPU test asserts that too)."""
    c = _exact_inputs(case)
    assert c["pred"].shape == (case.pairs(64),)
    assert c["d_rows"].shape == (case.pairs(64), 4 * case.E)


def _window(alloc_rows, alloc_cols, rows, cols, values, dtype, fill, dev, r0=1, c0=0):
    """A [rows, cols] window at (r0, c0) of a [alloc_rows, alloc_cols] allocation filled
    with ``fill``; the window holds ``values`` (None: left as ``fill``).  c0 keeps the
    window's alignment; -> (allocation, window)."""
    buf = torch.full((alloc_rows, alloc_cols), fill, dtype=dtype, device=dev)
    win = buf[r0:r0 + rows, c0:c0 + cols]
    if values is not None:
        win.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return buf, win


@gpu_test
@pytest.mark.parametrize("case", EXACT, ids=repr)
def test_exact_integer_edges(gpu, case):
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    T = int(lib.mrec_ncf_tile())
    assert T == 64
    c = _exact_inputs(case, T)
    pairs, E, nl = case.pairs(T), case.E, len(case.layers)
    ld = 4 * E + 8
    f32 = torch.float32
    rows_buf, rows = _window(pairs + 3, ld, pairs, 4 * E, c["rows"], BF16, NAN, gpu)
    Ks = [2 * E] + list(case.layers[:-1])
    wbufs = [_window(N + 2, K + 5, N, K, w, f32, NAN, gpu, c0=2) for N, K, w in zip(case.layers, Ks, c["ws"])]
    bbufs = [_window(1, N + 4, 1, N, b[None, :], f32, NAN, gpu, r0=0, c0=3) for N, b in zip(case.layers, c["bs"])]
    wp_buf, wp = _window(1, E + case.layers[-1] + 4, 1, E + case.layers[-1], c["wp"][None, :], f32, NAN,
                         gpu, r0=0, c0=1)
    dp_buf, dp = _window(1, pairs + 8, 1, pairs, c["dpred"][None, :], f32, NAN, gpu, r0=0, c0=4)
    pred_buf, pred = _window(1, pairs + 8, 1, pairs, None, f32, SENT, gpu, r0=0, c0=4)
    dr_buf, dr = _window(pairs + 3, ld, pairs, 4 * E, None, BF16, SENT, gpu)
    parts = int(lib.mrec_ncf_parts(pairs))
    P = int(lib.mrec_ncf_param_count(E, nl, widths_arr(case.layers)))
    part_buf, part = _window(parts + 2, P, parts, P, None, f32, SENT, gpu)
    grads = torch.full((P + 8,), SENT, dtype=f32, device=gpu)
    a = _mrec.NcfArgs()
    a.rows, a.ld_rows, a.pairs, a.E, a.n_layers = rows.data_ptr(), ld, pairs, E, nl
    for l in range(nl):
        a.widths[l] = case.layers[l]
        a.w[l], a.ld_w[l], a.b[l] = wbufs[l][1].data_ptr(), wbufs[l][1].stride(0), bbufs[l][1].data_ptr()
    a.wp, a.pred = wp.data_ptr(), pred.data_ptr()
    a.dpred, a.d_rows, a.ld_drows = dp.data_ptr(), dr.data_ptr(), ld
    a.part, a.parts = part.data_ptr(), parts
    st = _mrec.stream_handle()
    _mrec.call("mrec_ncf_fwd", ctypes.byref(a), st)
    _mrec.call("mrec_ncf_bwd", ctypes.byref(a), st)
    _mrec.call("mrec_sasrec_wgrad", part.data_ptr(), parts, P, grads.data_ptr(), st)
    torch.cuda.synchronize()

    def t32(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).float()

    # pred: live exact, the guards untouched
    want = torch.full((1, pairs + 8), SENT)
    want[0, 4:4 + pairs] = t32(c["pred"])
    assert torch.equal(pred_buf.cpu(), want)
    # the whole d_rows image: live exact, rows >= pairs, columns >= 4E and the guards 7.0
    want = torch.full((pairs + 3, ld), SENT)
    want[1:1 + pairs, :4 * E] = t32(c["d_rows"])
    assert torch.equal(dr_buf.float().cpu(), want)
    # every dense gradient, summed in workgroup order
    flat = np.concatenate([w.reshape(-1) for w in c["dws"]] + list(c["dbs"]) + [c["dwp"]])
    assert flat.size == P
    assert torch.equal(grads[:P].cpu(), t32(flat))
    assert (grads[P:] == SENT).all()
    assert (part_buf[0] == SENT).all() and (part_buf[parts + 1:] == SENT).all()
    assert torch.isfinite(part).all()
    # the inputs are as they were
    assert torch.isnan(rows_buf[0].float()).all() and torch.isnan(rows_buf[1 + pairs:].float()).all()
    assert torch.equal(rows.float().cpu(), t32(c["rows"]))


# ---------------------------------------------------------------------------
# 3. through the model on cuda:0
# ---------------------------------------------------------------------------

def _model(gpu, state=None, **kw):
    m = ncf(device=gpu, **kw)
    assert m.embeddings.weight.is_cuda and all(p.is_cuda for p in m.parameters())
    if state is not None:
        m.load_state_dict(state)
    return m


@gpu_test
@pytest.mark.parametrize("emb_dtype", [torch.float32, torch.bfloat16])
def test_g7_prediction_through_the_model(gpu, monkeypatch, emb_dtype):
    from pytorchrec_amd import dense as D
    g = golden("g7_ncf.npz")
    batch = {"uid": torch.from_numpy(g["uid"]).to(gpu), "iid": torch.from_numpy(g["iid"]).to(gpu)}
    errs = {}
    for fused in (True, False):
        monkeypatch.setattr(D, "NCF_FUSED", fused)
        m = _model(gpu, g7_state(g), emb_dtype=emb_dtype).eval()
        with torch.no_grad():
            pred, target = m(batch)
        assert pred.shape == (32, 3) and pred.dtype == torch.float32
        assert torch.equal(target.cpu(), torch.tensor([1.0, 0.0, 0.0]).expand(32, 3))
        errs[(fused, "prediction")] = _errs(pred, torch.from_numpy(g["prediction"]))
    _meets_bars(errs, ["prediction"])


@gpu_test
def test_g17_state_a_init_is_bit_identical_on_the_device(gpu):
    g = golden("g17_ncf.npz")
    sd = _model(gpu).state_dict()
    assert tuple(sd) == KEYS
    for k in KEYS:
        assert np.array_equal(sd[k].cpu().numpy().view(np.uint32), g[f"A::{k}"].view(np.uint32)), k


@gpu_test
@pytest.mark.parametrize("emb_dtype", [torch.float32, torch.bfloat16])
def test_g17_state_b_forward_through_the_model(gpu, monkeypatch, emb_dtype):
    from pytorchrec_amd import dense as D
    g = golden("g17_ncf.npz")
    errs = {}
    for fused in (True, False):
        monkeypatch.setattr(D, "NCF_FUSED", fused)
        m = _model(gpu, g17_state(g, "B"), emb_dtype=emb_dtype).eval()
        with torch.no_grad():
            pred, target = m(g17_batch(g, gpu))
        assert np.array_equal(target.cpu().numpy(), g["A_target"])
        errs[(fused, "prediction")] = _errs(pred, torch.from_numpy(g["B_pred"]))
    _meets_bars(errs, ["prediction"])


@gpu_test
def test_g17_state_b_gradients_and_sgd_step_through_the_model(gpu, monkeypatch):
    """All nine gradients of prediction.square().mean() and all nine tensors after one SGD
    step of lr 0.05 against the reference's, fused and layered (fp32 bank, dense grads)."""
    from pytorchrec_amd import dense as D
    from test_ncf_cpu import named_grads
    g = golden("g17_ncf.npz")
    errs, calls = {}, []
    real = D._NcfFn.apply
    monkeypatch.setattr(D._NcfFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    for fused in (True, False):
        monkeypatch.setattr(D, "NCF_FUSED", fused)
        m = _model(gpu, g17_state(g, "B")).eval()
        opt = torch.optim.SGD(m.parameters(), lr=float(g["lr_b"]))
        pred, _ = m(g17_batch(g, gpu))
        pred.square().mean().backward()
        grads = named_grads(m)
        for k in KEYS:
            errs[(fused, "grad " + k)] = _errs(grads[k], torch.from_numpy(g[f"B_grad::{k}"]))
        opt.step()
        sd = m.state_dict()
        for k in KEYS:
            errs[(fused, k)] = _errs(sd[k], torch.from_numpy(g[f"B_after::{k}"]))
    assert len(calls) == 1  # the fused step went through the kernels, exactly once
    _meets_bars(errs, ["grad " + k for k in KEYS] + list(KEYS))


@gpu_test
def test_duplicate_ids_fused_sgd_against_dense_grad(gpu):
    """G17's batch repeats users and items.  One train_step (MSE, SGD lr 0.05) with the
    bank's fused-SGD update lands where the dense-grad update does: every table to 1e-6
    of its magnitude (their segment sums may run in another order), and both moved."""
    g = golden("g17_ncf.npz")
    assert len(np.unique(g["uid"])) < 24 and len(np.unique(g["iid"])) < g["iid"].size
    out = {}
    for mode in ("sgd", "dense"):
        m = _model(gpu, g17_state(g, "B"))
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.05), torch.nn.MSELoss(), [], gpu)
        assert m.embeddings.update == "sgd"
        if mode == "dense":
            m.embeddings.use_dense_grad()
        loss = float(m.train_step(g17_batch(g, gpu))["loss"].detach())
        assert np.isfinite(loss)
        out[mode] = m.state_dict()
    for k in KEYS:
        a, b = out["sgd"][k], out["dense"][k]
        assert not torch.equal(a.cpu(), torch.from_numpy(g[f"B::{k}"])), k
        torch.testing.assert_close(a, b, rtol=0, atol=1e-6 * b.abs().max().item())


@gpu_test
def test_empty_batch(gpu):
    m = _model(gpu).eval()
    batch = {"uid": torch.zeros(0, dtype=torch.int64, device=gpu),
             "iid": torch.zeros(0, 5, dtype=torch.int64, device=gpu)}
    pred, target = m(batch)
    assert pred.shape == (0, 5) and target.shape == (0, 5) and pred.dtype == torch.float32


@gpu_test
@pytest.mark.parametrize("column,bad", [("uid", 50), ("iid", 37), ("iid", -1)])
def test_an_id_outside_its_table_is_an_index_error(gpu, column, bad):
    g = golden("g17_ncf.npz")
    batch = g17_batch(g, gpu)
    batch[column] = batch[column].clone()
    batch[column].reshape(-1)[3] = bad
    with pytest.raises(IndexError):
        _model(gpu).eval()(batch)


@gpu_test
def test_fit_pair_wise_and_evaluate(gpu):
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.metrics import get_metric
    from pytorchrec_amd.sampling import NegativeSampler
    from test_ranking_cpu import planted_set
    tu, ti, du, dev = planted_set()
    train = ColumnarDataset({"uid": tu, "iid": ti})
    devset = ColumnarDataset({"uid": du, "iid": dev})
    m = ncf(users=200, items=120, emb_size=8, layers=[16, 8], seed=11, device=gpu)
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), BPRLoss(), [get_metric("ndcg@10")], gpu)
    m.set_negative_sampler(NegativeSampler(tu, ti, 0, 120, seed=3, n_users=200))
    hist = m.fit(train, 256, 6, dev_dataset=devset, train_mode="pair_wise", verbose=0)
    print("loss per epoch:", [round(r["loss"], 4) for r in hist],
          "ndcg@10:", [round(r["ndcg@10"], 4) for r in hist])
    assert len(hist) == 6 and set(hist[0]) == {"loss", "ndcg@10"}
    assert hist[-1]["loss"] < 0.9 * hist[0]["loss"], (hist[0]["loss"], hist[-1]["loss"])
    got = m.evaluate(devset, 128, verbose=0)
    assert got["ndcg@10"] == hist[-1]["ndcg@10"]
