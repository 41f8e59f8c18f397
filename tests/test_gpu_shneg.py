"""The fused shared-negative kernels (csrc/shneg.hip) on an MI355X: exact expectations at the
tile edges, masking, independence from the split count / run / placement, Gaussian inputs
against the fp64 oracle inside the derived tolerance, aliasing, argument errors, and the
model layer (funksvd / sasrec / gru4rec) against the same step through the torch-ops path.

The oracle and the tolerance are test_shneg_cpu.py's (its docstring derives every term; the
device functions' error, EPS_F, was measured alone on this GPU and is recorded there).

Exact cases.  With all-zero queries every score is 0, so top1's loss is exactly 1.0, bpr's
is log 2 and softmax's log(n_b + 1); the coefficients are g_b / n_b times 1/2 (bpr), 1/4
(top1), or g_b / (n_b + 1) (softmax).  The ids are laid out so that every n_b (softmax: n_b
+ 1) is a power of two and every g_b is one too: the coefficients are then exact in bf16
and, with integer rows in [-2, 2] and S <= 600, every partial sum is exact in fp32, so the
gradients must EQUAL the closed form (rounded once to the output dtype).  The transposed
case (integer queries, all-zero rows) does the same for dpos and dneg.
"""
import copy
import math

import pytest
import torch

from test_shneg_cpu import BF, EPS_F, KINDS, MODELS, U, _sampler, _train_data, assert_within, gaussian_case, oracle

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DIMS = (8, 16, 32, 64)
DTYPES = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]  # (q, rows)
REDUCE = {"none": 0, "mean": 1, "sum": 2}
KIND = {"softmax": 0, "bpr": 1, "top1": 2}


def tiles():
    from pytorchrec_amd.loss import shneg_tile_candidates, shneg_tile_queries
    return shneg_tile_queries(), shneg_tile_candidates()


def window(t, fill, dev):
    """``t [n, D]`` as a window of a larger allocation filled with ``fill`` (16-byte aligned
    rows: 2 rows above, 8 columns to the left, 8 to the right, 2 rows below)."""
    n, D = t.shape
    big = torch.full((n + 4, D + 16), fill, dtype=t.dtype, device=dev)
    big[2:2 + n, 8:8 + D] = t.to(dev)
    return big, big[2:2 + n, 8:8 + D]


def guard_ok(big, n, D, fill):
    ref = torch.full_like(big, fill)
    ref[2:2 + n, 8:8 + D] = big[2:2 + n, 8:8 + D]
    return torch.equal(big.view(torch.int16 if big.dtype == BF16 else torch.int32),
                       ref.view(torch.int16 if big.dtype == BF16 else torch.int32))


def fused(q, pos, neg, kind, reduction, g, ids=None, bias=None, splits=0, outs=None):
    """forward + backward through the raw calls -> (loss, dq, dpos, dneg)."""
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.loss import shneg_call, shneg_default_splits
    dev = q.device
    B, D = q.shape
    S = neg.shape[0]
    lib = _mrec.lib()
    stats = torch.empty(B, 4, dtype=F32, device=dev)
    loss = torch.empty(B if reduction == "none" else 1, dtype=F32, device=dev)
    n = splits or shneg_default_splits(B, S)
    ws = torch.empty(int(lib.mrec_shneg_workspace_size(B, S, D, n)) + 16, dtype=torch.uint8, device=dev)
    kw = dict(pos_id=ids[0] if ids else None, neg_id=ids[1] if ids else None,
              pos_bias=bias[0] if bias else None, neg_bias=bias[1] if bias else None, splits=splits, workspace=ws)
    shneg_call("mrec_shneg_loss_fwd", q, pos, neg, KIND[kind], REDUCE[reduction], stats=stats, loss=loss, **kw)
    if outs is None:
        outs = (torch.empty(B, D, dtype=q.dtype, device=dev), torch.empty(B, D, dtype=pos.dtype, device=dev),
                torch.empty(S, D, dtype=neg.dtype, device=dev))
    gt = torch.as_tensor(g, dtype=F32, device=dev).reshape(-1).contiguous()
    shneg_call("mrec_shneg_loss_bwd", q, pos, neg, KIND[kind], REDUCE[reduction], stats=stats, g=gt,
               dq=outs[0], dpos=outs[1], dneg=outs[2], **kw)
    return (loss, *outs)


# ---------------------------------------------------------------------------
# exact expectations
# ---------------------------------------------------------------------------

def exact_ids(B, S, softmax):
    """pos_id / neg_id such that every n_b (softmax: n_b + 1) is a power of two: the first k1
    candidates share id 1000, the next k2 id 2000, the others are distinct; a query's
    positive is 1000 or 2000 (k1 or k2 of its candidates are masked)."""
    off = 1 if softmax else 0
    t1 = 2 ** int(math.floor(math.log2(S + off))) - off
    t2 = (t1 + off) // 2 - off if t1 + off >= 2 else t1
    k1, k2 = S - t1, S - t2
    if k1 + k2 > S:
        k2 = 0
    nid = torch.arange(S, dtype=torch.int64) + 10
    nid[:k1] = 1000
    nid[k1:k1 + k2] = 2000
    two = k2 > 0
    pid = torch.tensor([2000 if (two and b % 3 == 1) else 1000 for b in range(B)], dtype=torch.int64)
    return pid, nid


def closed_form(kind, q, pos, neg, pid, nid, g):
    """All scores zero: loss and gradients in fp64 from the counts alone."""
    Q, P, N = q.double(), pos.double(), neg.double()
    live = (nid.reshape(1, -1) != pid.reshape(-1, 1)).double()
    n = live.sum(1)
    g = g.double()
    if kind == "softmax":
        a = live * (g / (n + 1)).unsqueeze(1)
        ap = g * (1 / (n + 1) - 1)
        loss = torch.log(n + 1)
    else:
        f = 0.5 if kind == "bpr" else 0.25
        a = live * (g / n * f).unsqueeze(1)
        ap = -g * f
        loss = torch.full_like(n, math.log(2.0) if kind == "bpr" else 1.0)
    return loss, a @ N + ap.unsqueeze(1) * P, ap.unsqueeze(1) * Q, a.t() @ Q, n


def run_exact(gpu, kind, B, S, D, qdt, rdt, transposed, reduction="none"):
    gen = torch.Generator().manual_seed(B * 1009 + S * 17 + D)
    ints = lambda n: torch.randint(-2, 3, (n, D), generator=gen).float()  # noqa: E731
    if transposed:
        q, pos, neg = ints(B), torch.zeros(B, D), torch.zeros(S, D)
    else:
        q, pos, neg = torch.zeros(B, D), ints(B), ints(S)
    pid, nid = exact_ids(B, S, kind == "softmax")
    if reduction == "none":
        g = torch.tensor([[1.0, 2.0, 0.5, -1.0, 4.0][b % 5] for b in range(B)])
        gb = g
    else:
        g = torch.tensor(2.0)
        gb = g.expand(B)
    want = closed_form(kind, q, pos, neg, pid, nid, gb)
    n = want[4]
    assert bool((torch.log2(n + (kind == "softmax")) % 1 == 0).all()), n
    # operands and outputs as windows of larger allocations with hostile surroundings
    bq, wq = window(q.to(qdt), float("nan"), gpu)
    bp, wp = window(pos.to(rdt), 1e30, gpu)
    bn, wn = window(neg.to(rdt), float("nan"), gpu)
    bdq, wdq = window(torch.zeros(B, D, dtype=qdt), -7.0, gpu)
    bdp, wdp = window(torch.zeros(B, D, dtype=rdt), -7.0, gpu)
    bdn, wdn = window(torch.zeros(S, D, dtype=rdt), -7.0, gpu)
    ids = (pid.to(gpu), nid.to(gpu)) if (B + S) % 2 else (pid.to(gpu).int(), nid.to(gpu).int())
    loss, dq, dpos, dneg = fused(wq, wp, wn, kind, reduction, g, ids=ids, outs=(wdq, wdp, wdn))
    assert guard_ok(bdq, B, D, -7.0) and guard_ok(bdp, B, D, -7.0) and guard_ok(bdn, S, D, -7.0)
    per = want[0]
    if reduction == "none":
        got = loss.cpu().double()
        if kind == "top1":
            assert torch.equal(got, per)
        else:  # log 2, log(n + 1): the device log and a sum of n + 1 equal terms
            assert bool(((got - per).abs() <= (EPS_F + (n + 2) * U) * per.abs()).all()), (got, per)
    else:
        assert abs(float(loss) - float(per.sum())) <= (EPS_F + (n.max() + B + 2) * U) * float(per.sum())
    for name, got, w, dt in (("dq", dq, want[1], qdt), ("dpos", dpos, want[2], rdt), ("dneg", dneg, want[3], rdt)):
        assert torch.equal(got.cpu(), w.float().to(dt)), (name, kind, B, S, D, qdt, rdt, transposed)


def edge_sizes():
    TQ, TC = tiles()
    return [1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3], [1, TC - 1, TC, TC + 1, 3 * TC + 5]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("si", range(5))
@pytest.mark.parametrize("bi", range(5))
def test_exact_at_the_tile_edges(gpu, kind, bi, si):
    """Every (B, S) edge pair, both orientations; the embedding size and the dtypes cycle
    through all their combinations over the grid."""
    Bs, Ss = edge_sizes()
    c = bi * 5 + si + 7 * KINDS.index(kind)
    D = DIMS[c % 4]
    qdt, rdt = DTYPES[(c // 4) % 4]
    for transposed in (False, True):
        run_exact(gpu, kind, Bs[bi], Ss[si], D, qdt, rdt, transposed)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qdt,rdt", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_exact_every_dim_and_dtype(gpu, kind, D, qdt, rdt):
    Bs, Ss = edge_sizes()
    run_exact(gpu, kind, Bs[3], Ss[4], D, qdt, rdt, False)
    run_exact(gpu, kind, Bs[4], Ss[3], D, qdt, rdt, True, reduction="sum")


@pytest.mark.parametrize("kind", KINDS)
def test_exact_many_chunks_and_splits(gpu, kind):
    """S = 600 pool rows against B = 2100 queries: three chunks of the batch, split."""
    for splits in (1, 3):
        gen = torch.Generator().manual_seed(5)
        B, S, D = 2100, 600 if kind != "softmax" else 575, 32
        q = torch.randint(-2, 3, (B, D), generator=gen).float()
        pid, nid = exact_ids(B, S, kind == "softmax")
        g = torch.tensor([[1.0, 2.0, 0.5, -1.0, 4.0][b % 5] for b in range(B)])
        want = closed_form(kind, q, torch.zeros(B, D), torch.zeros(S, D), pid, nid, g)
        # (dneg sums up to 2100 terms of |a q| <= 2^-6: exact in fp32)
        out = fused(q.to(gpu), torch.zeros(B, D, dtype=BF16, device=gpu), torch.zeros(S, D, dtype=BF16, device=gpu),
                    kind, "none", g, ids=(pid.to(gpu), nid.to(gpu)), splits=splits)
        assert torch.equal(out[3].cpu(), want[3].float().to(BF16))
        assert torch.equal(out[2].cpu(), want[2].float().to(BF16))


# ---------------------------------------------------------------------------
# masking
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_masking(gpu, kind):
    TQ, TC = tiles()
    B, S, D = 2 * TQ + 3, 3 * TC + 5, 32
    q, pos, neg, _ = gaussian_case(B, S, D, seed=11, row_dtype=BF16, device=gpu)
    gen = torch.Generator().manual_seed(12)
    pid = torch.randint(0, 5, (B,), generator=gen).to(gpu)        # positives 0 .. 4
    nid = torch.randint(0, 40, (S,), generator=gen).to(gpu) + 3   # candidates 3 .. 42
    nid[[0, TC - 1, TC, S - 1]] = 777                              # masked for EVERY query below
    pid[1], pid[TQ] = 555, 555                                    # ... and n_b = 0 for these two
    nid_all = nid.clone()
    dead = torch.zeros(S, dtype=torch.bool, device=gpu)
    dead[[0, TC - 1, TC, S - 1]] = True
    g = torch.linspace(0.5, 2.0, B)
    # (a) rows masked for every query: NaN or zero, the same bits; their dneg is zero
    everyone = torch.full_like(pid, 777)
    zero = torch.where(dead.unsqueeze(1), torch.zeros_like(neg), neg)
    nan = torch.where(dead.unsqueeze(1), torch.full_like(neg, float("nan")), neg)
    a = fused(q, pos, zero, kind, "none", g, ids=(everyone, nid_all))
    b = fused(q, pos, nan, kind, "none", g, ids=(everyone, nid_all))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(b[3][dead], torch.zeros(4, D, dtype=BF16, device=gpu))
    assert bool(torch.isfinite(b[0]).all()) and bool((b[3][~dead].float().abs().sum(1) > 0).all())
    # (b) n_b = 0: all candidates carry the query's positive
    same = torch.full_like(nid, 555)
    pid2 = pid.clone()
    out = fused(q, pos, neg, kind, "none", g, ids=(pid2, same))
    for b0 in (1, TQ):
        assert float(out[0][b0]) == 0.0
        assert torch.equal(out[1][b0], torch.zeros(D, device=gpu)) and not out[2][b0].float().abs().any()
    assert bool((out[0][[0, 2, TQ + 1]] > 0).all())
    o = oracle(q, pos, neg, kind, "none", g.double().to(gpu), pos_id=pid2, neg_id=same)
    assert_within(out[0], o["loss"], o["tol_loss"], "loss")
    assert_within(out[1], o["dq"], o["tol_dq"], "dq")


# ---------------------------------------------------------------------------
# independence from the split count, the run and the placement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_split_run_and_placement_independence(gpu, kind):
    from pytorchrec_amd.loss import shneg_default_splits
    B, S, D = 3100, 70, 64  # four chunks of the batch
    q, pos, neg, kw = gaussian_case(B, S, D, seed=13, row_dtype=BF16, ids=True, bias=True, device=gpu)
    ids, bias = (kw["pos_id"], kw["neg_id"]), (kw["pos_bias"], kw["neg_bias"])
    assert shneg_default_splits(B, S) > 1
    ref = fused(q, pos, neg, kind, "mean", 1.3, ids=ids, bias=bias, splits=1)
    for splits in (1, 2, 3, 0):
        got = fused(q, pos, neg, kind, "mean", 1.3, ids=ids, bias=bias, splits=splits)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), splits
    # other places: the operands as windows of larger allocations
    _, wq = window(q, float("nan"), gpu)
    _, wp = window(pos, 1e30, gpu)
    _, wn = window(neg, float("nan"), gpu)
    got = fused(wq, wp, wn, kind, "mean", 1.3, ids=ids, bias=bias)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------
# Gaussian inputs against the fp64 oracle
# ---------------------------------------------------------------------------

def check_case(gpu, kind, reduction, B, S, D, qdt, rdt, extras, scale, seed):
    q, pos, neg, kw = gaussian_case(B, S, D, seed=seed, q_dtype=qdt, row_dtype=rdt, ids=extras, bias=extras,
                                    scale=scale, device=gpu)
    g = torch.linspace(0.5, 2.0, B) if reduction == "none" else torch.tensor(1.7)
    ids = (kw["pos_id"], kw["neg_id"]) if extras else None
    bias = (kw["pos_bias"], kw["neg_bias"]) if extras else None
    loss, dq, dpos, dneg = fused(q, pos, neg, kind, reduction, g, ids=ids, bias=bias)
    o = oracle(q, pos, neg, kind, reduction, g.double().to(gpu), **kw)
    assert bool(torch.isfinite(loss).all())
    assert_within(loss.reshape(o["loss"].shape), o["loss"], o["tol_loss"], f"{kind} {reduction} loss")
    assert_within(dq, o["dq"], o["tol_dq"], "dq")
    assert_within(dpos, o["dpos"], o["tol_dpos"], "dpos")
    assert_within(dneg, o["dneg"], o["tol_dneg"], "dneg")


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_inside_the_tolerance(gpu, kind, reduction, extras):
    TQ, TC = tiles()
    c = KINDS.index(kind) + 3 * ["none", "mean", "sum"].index(reduction) + extras
    qdt, rdt = DTYPES[c % 4]
    check_case(gpu, kind, reduction, 2 * TQ + 3, 3 * TC + 5, DIMS[c % 4], qdt, rdt, extras, 0.35, seed=20 + c)
    # more than one chunk each way, the common training dtypes
    check_case(gpu, kind, reduction, 1100, 1300, 64, F32, BF16, extras, 0.35, seed=40 + c)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_of_plus_minus_80(gpu, kind):
    """Scores scaled to +-80 (Gaussian operands at scale 3.2, D = 64): softmax neither
    overflows nor loses the tolerance."""
    q, pos, neg, _ = gaussian_case(70, 300, 64, seed=30, row_dtype=BF16, scale=3.2, device=gpu)
    s = q.to(BF16).float() @ neg.float().t()
    assert float(s.max()) > 60 and float(s.min()) < -60
    check_case(gpu, kind, "mean", 70, 300, 64, F32, BF16, True, 3.2, seed=30)
    check_case(gpu, kind, "none", 70, 300, 64, F32, BF16, False, 3.2, seed=31)


# ---------------------------------------------------------------------------
# aliasing, the loss class, argument errors
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_in_batch_aliasing_equals_a_copy(gpu, kind):
    from pytorchrec_amd.loss import SharedNegativeLoss
    q, pos, _, _ = gaussian_case(100, 1, 32, seed=14, row_dtype=BF16, device=gpu)
    pid = torch.randint(0, 60, (100,), generator=torch.Generator().manual_seed(1)).to(gpu)
    loss = SharedNegativeLoss(kind)
    q1, p1 = q.clone().requires_grad_(), pos.clone().requires_grad_()
    l1 = loss(q1, p1, p1, pid, pid)
    l1.backward()
    q2, p2, n2 = q.clone().requires_grad_(), pos.clone().requires_grad_(), pos.clone().requires_grad_()
    l2 = loss(q2, p2, n2, pid, pid.clone())
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(q1.grad, q2.grad)
    assert torch.equal(p1.grad, p2.grad + n2.grad)


@pytest.mark.parametrize("kind", KINDS)
def test_loss_class_runs_the_kernels_and_matches_the_torch_path(gpu, kind, monkeypatch):
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.loss import SharedNegativeLoss
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda fn, *a: (calls.append(fn), real(fn, *a))[1])
    q, pos, neg, kw = gaussian_case(67, 133, 64, seed=15, row_dtype=BF16, ids=True, bias=True, device=gpu)
    outs = []
    for use in (True, False):
        loss = SharedNegativeLoss(kind, "mean")
        loss.fused = use
        a, b, c = (t.clone().requires_grad_() for t in (q, pos, neg))
        # strided windows are read in place: a [B, 2 D] gather result's halves
        wide = torch.cat([a, a], 1)
        out = loss(wide[:, 64:], b, c, **kw)
        out.backward()
        outs.append((out.detach(), a.grad, b.grad, c.grad))
        assert (calls.count("mrec_shneg_loss_fwd"), calls.count("mrec_shneg_loss_bwd")) == (1, 1)
    o = oracle(q, pos, neg, kind, "mean", 1.0, **kw)
    for i, name in enumerate(("loss", "dq", "dpos", "dneg")):
        for got in (outs[0][i], outs[1][i]):
            assert_within(got.reshape(o[name].shape), o[name], o["tol_" + name], name)
    # empty shapes: nothing is launched
    n = len(calls)
    loss = SharedNegativeLoss(kind, "none")
    e = loss(q[:0].requires_grad_(), pos[:0], neg)
    assert e.shape == (0,) and len(calls) == n
    z = loss(q, pos, neg[:0])
    assert torch.equal(z, torch.zeros(67, device=gpu))


def test_argument_errors(gpu):
    """ValueError before any launch: the outputs keep their guard values."""
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.loss import shneg_call
    q, pos, neg, kw = gaussian_case(2100, 40, 64, seed=16, row_dtype=BF16, ids=True, device=gpu)
    stats = torch.full((2100, 4), -7.0, device=gpu)
    loss = torch.full((1,), -7.0, device=gpu)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    base = dict(stats=stats, loss=loss, workspace=ws)
    with pytest.raises(ValueError, match="unsupported"):
        shneg_call("mrec_shneg_loss_fwd", q, pos, neg, 0, 1, dim=48, **base)
    with pytest.raises(ValueError, match="go together"):
        shneg_call("mrec_shneg_loss_fwd", q, pos, neg, 0, 1, pos_id=kw["pos_id"], **base)
    with pytest.raises(ValueError, match="go together"):
        shneg_call("mrec_shneg_loss_fwd", q, pos, neg, 0, 1, neg_id=kw["neg_id"], **base)
    with pytest.raises(ValueError, match="workspace"):
        shneg_call("mrec_shneg_loss_fwd", q, pos, neg, 0, 1, stats=stats, loss=loss, workspace=ws[:64])
    with pytest.raises(ValueError, match="aligned"):
        shneg_call("mrec_shneg_loss_fwd", q[:, 1:], pos, neg, 0, 1, dim=32, **base)
    # the backward's chunk partials: three chunks x 40 x 64 floats are needed with 3 splits
    dq, dpos, dneg = torch.full_like(q, -7.0), torch.full_like(pos, -7.0), torch.full_like(neg, -7.0)
    g = torch.ones(1, device=gpu)
    with pytest.raises(ValueError, match="workspace"):
        shneg_call("mrec_shneg_loss_bwd", q, pos, neg, 0, 1, stats=stats, g=g, dq=dq, dpos=dpos, dneg=dneg,
                   splits=3, workspace=ws[:3 * 40 * 64 * 4 - 16])
    torch.cuda.synchronize()
    for t in (stats, loss, dq, dpos, dneg):
        assert bool((t.float() == -7.0).all())


# ---------------------------------------------------------------------------
# the model layer on cuda:0
# ---------------------------------------------------------------------------

def _gpu_model(name, gpu):
    from test_gru4rec_cpu import gru4rec
    from test_ranking_cpu import funk
    from test_sasrec_cpu import sasrec
    if name == "funksvd":
        m = funk(users=160, items=61)
    elif name == "sasrec":
        m = sasrec(items=61, max_his_len=8)
    else:
        m = gru4rec(items=61, max_his_len=8)
    with torch.no_grad():  # lively weights: scores of order 1, not 1e-4
        for b in m.embedding_banks():
            b.weight.mul_(30.0)
    return m


@pytest.mark.parametrize("source", ["sampler", "in_batch"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_model_train_step_runs_fused_and_matches_the_torch_path(gpu, model, source, monkeypatch):
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.loss import SharedNegativeLoss
    data, pairs = _train_data()
    calls = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda fn, *a: (calls.append(fn), real(fn, *a))[1])
    results = []
    base = _gpu_model(model, gpu)
    for use in (True, False):
        m = copy.deepcopy(base)
        loss = SharedNegativeLoss("softmax")
        loss.fused = use
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.5), loss, [], gpu)
        if source == "sampler":
            m.set_shared_negatives(_sampler(pairs), 48)
        else:
            m.set_shared_negatives("in_batch")
        if use:  # the oracle's loss and its tolerance from the step's own inputs
            m.train()
            with torch.no_grad():
                dev_data = {k: v.to(gpu) for k, v in data.items()}
                pool = m.shared_negative_pool(0)
                pool = pool.to(gpu) if pool is not None else None
                q, pr, nr, pid = m._shared_negative_inputs(dev_data, pool)
                nid = pid if pool is None else pool.to(pid.dtype)
                o = oracle(q, pr, nr if pool is not None else pr, "softmax", "mean", 1.0, pos_id=pid, neg_id=nid)
        before = [b.weight.detach().clone() for b in m.embedding_banks()]
        n0 = len(calls)
        out = float(m.train_step(data)["loss"].detach())
        ran = calls[n0:]
        assert (("mrec_shneg_loss_fwd" in ran) and ("mrec_shneg_loss_bwd" in ran)) == use
        results.append((out, [b.weight.detach() - w0 for b, w0 in zip(m.embedding_banks(), before)]))
    (lf, df), (lt, dt) = results
    tol = float(o["tol_loss"])
    print(f"{model} {source}: fused {lf:.7f} torch {lt:.7f} oracle {float(o['loss']):.7f} tol {tol:.2e}")
    assert abs(lf - float(o["loss"])) <= tol and abs(lt - float(o["loss"])) <= tol
    # the updated rows under plain SGD: each path rounds the loss's row gradients to bf16 once
    # (2^-8 relative), and the encoder's bf16 row gradients, whose inputs differ in the last
    # fp32 bits, may round the other way (2^-8 each side): 4 x 2^-8 of the largest update
    for a, b in zip(df, dt):
        mag = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"  rows: max |update| {mag:.3e}, max |diff| {err:.3e}")
        assert mag > 0 and err <= 4 * BF * mag
        assert torch.equal(a.abs().sum(1) > 0, b.abs().sum(1) > 0)  # the same rows moved
