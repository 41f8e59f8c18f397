"""Ranking training and evaluation on the CPU path (no GPU): the loss / metric
registries, BPR / Top1 and NDCG / Hit against golden G14 (the reference's own outputs),
the rank rule's ties and NaNs, one pairwise FunkSVD step against G14, the negative
sampler's contract, ``fit(train_mode="pair_wise")`` on a small planted set, and the
argument validation of the four new libmrec exports.

Tolerances: loss values rtol 1e-5 / atol 1e-6 and gradients rtol 1e-4 / atol 1e-6
against the fp64 evaluation of the reference formula (the project's own, from
test_ctr_head_bce_fused_matches_torch); the FunkSVD step uses G10's (loss rtol 1e-5,
tables rtol 1e-5 / atol 1e-8, untouched user rows bit-equal).
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.nn.modules.loss import _Loss  # noqa

from conftest import golden

REDUCTIONS = ("none", "mean", "sum")
KINDS = ("bpr", "top1")


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def pair_loss_f64(kind, x, reduction="none", g=None):
    """The reference formulas in fp64 -> (loss, d loss / d x scaled by the upstream g).
    BPR: softplus(neg - pos) with torch's threshold (x for x > 20, else log1p(exp x));
    Top1: sigmoid(neg - pos) + sigmoid(neg^2)."""
    x = np.asarray(x, np.float64)
    pos, neg = x[:, 0], x[:, 1]
    d = neg - pos

    def sig(z):
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1.0, e) / (1.0 + e)

    def dsig(z):
        e = np.exp(-np.abs(z))
        return e / (1.0 + e) ** 2

    if kind == "bpr":
        with np.errstate(over="ignore"):
            l = np.where(d > 20, d, np.log1p(np.exp(np.minimum(d, 50.0))))
        s = np.where(d > 20, 1.0, sig(d))
        dpos, dneg = -s, s
    else:
        l = sig(d) + sig(neg * neg)
        dpos, dneg = -dsig(d), dsig(d) + 2.0 * neg * dsig(neg * neg)
    B = len(x)
    if g is None:
        g = np.ones(B if reduction == "none" else 1)
    g = np.asarray(g, np.float64).reshape(-1)
    scale = g if reduction == "none" else np.full(B, g[0] / (B if reduction == "mean" else 1.0))
    grad = np.stack([dpos * scale, dneg * scale], axis=1)
    if reduction == "mean":
        l = l.mean() if B else 0.0
    elif reduction == "sum":
        l = l.sum()
    return l, grad


def rank_rule(p):
    """rank = 1 + #{j >= 1 : p[j] > p[0]}; NaN in column 0 -> N; written out per row."""
    p = np.asarray(p)
    out = np.empty(p.shape[0], np.int64)
    for r, row in enumerate(p):
        out[r] = p.shape[1] if np.isnan(row[0]) else 1 + sum(1 for v in row[1:] if v > row[0])
    return out


def funk(emb_size=8, users=50, items=37, seed=2020):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import FunkSVD
    return FunkSVD(CategoricalColumnWithIdentity(users, "uid"),
                   CategoricalColumnWithIdentity(items, "iid"),
                   CategoricalColumnWithIdentity(2, "label"), emb_size=emb_size, random_seed=seed)


def check_funksvd_bpr_step_g14(m, device):
    """One pairwise BPR train_step of the seed-2020 FunkSVD lands on G14's tables."""
    from pytorchrec_amd.loss import BPRLoss
    g = golden("g14_ranking.npz")
    sd = m.state_dict()
    assert np.array_equal(sd["u_embeddings.weight"].cpu().numpy().view(np.uint32),
                          g["u_before"].view(np.uint32))
    assert np.array_equal(sd["i_embeddings.weight"].cpu().numpy().view(np.uint32),
                          g["i_before"].view(np.uint32))
    m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), BPRLoss(), [], device)
    loss = float(m.train_step({"uid": torch.from_numpy(g["uid"]),
                               "iid": torch.from_numpy(g["iid"])})["loss"].detach())
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(float(g["loss"])), (loss, float(g["loss"]))
    sd = m.state_dict()
    for key, want in (("u_embeddings.weight", g["u_after"]), ("i_embeddings.weight", g["i_after"])):
        np.testing.assert_allclose(sd[key].cpu().numpy(), want, rtol=1e-5, atol=1e-8, err_msg=key)
    untouched = np.setdiff1d(np.arange(50), g["uid"])
    assert np.array_equal(sd["u_embeddings.weight"].cpu().numpy()[untouched].view(np.uint32),
                          g["u_after"][untouched].view(np.uint32))
    assert not np.array_equal(g["u_before"], g["u_after"])  # (the step moved something)


# ---------------------------------------------------------------------------
# registries
# ---------------------------------------------------------------------------

def test_registries_answer_the_reference_names():
    from pytorchrec_amd.loss import get_loss
    from pytorchrec_amd.metrics import get_metric
    for name in ("bpr", "top1", "bce", "mse"):
        cls = get_loss(name)
        assert isinstance(cls, type) and issubclass(cls, _Loss), name
    assert isinstance(get_loss("bpr")(), _Loss) and isinstance(get_loss("top1")("sum"), _Loss)
    with pytest.raises(ValueError):
        get_loss("hinge")
    m = get_metric("ndcg@10")
    assert (m.name, m.k, m.user_sample_n) == ("ndcg@10", 10, 99)
    m = get_metric("hit@5")
    assert (m.name, m.k, m.user_sample_n) == ("hit@5", 5, 99)
    for bad in ("ndcg", "ndcg@0", "map@5", 5):
        with pytest.raises(ValueError):
            get_metric(bad)
    assert get_metric("auc").name == "auc" and get_metric("logloss").name == "logloss"


# ---------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_pair_losses_match_g14_and_fp64(kind, reduction):
    from pytorchrec_amd.loss import get_loss
    g = golden("g14_ranking.npz")
    x = g["x"]
    assert x.shape == (1000, 2) and np.array_equal(x[:4], np.array(
        [(-30, 30), (30, -30), (0, 0), (-60, 45)], np.float32))
    t = torch.from_numpy(x.copy()).requires_grad_()
    out = get_loss(kind)(reduction=reduction)(t, None)
    out.sum().backward()
    want, want_grad = pair_loss_f64(kind, x, reduction)
    for ref_out, ref_grad in ((g[f"{kind}_{reduction}"], g[f"{kind}_{reduction}_grad"]),
                              (want, want_grad)):
        np.testing.assert_allclose(out.detach().numpy(), ref_out, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t.grad.numpy(), ref_grad, rtol=1e-4, atol=1e-6)


def test_pair_losses_refuse_other_shapes():
    from pytorchrec_amd.loss import BPRLoss, Top1Loss
    for cls in (BPRLoss, Top1Loss):
        with pytest.raises(AssertionError):
            cls()(torch.zeros(5, 3), None)
        with pytest.raises(AssertionError):
            cls()(torch.zeros(6), None)
        assert cls()(torch.zeros(5, 2)).shape == ()  # target may be left out altogether


# ---------------------------------------------------------------------------
# ranks and metrics
# ---------------------------------------------------------------------------

def test_ranks_and_metrics_match_g14():
    from pytorchrec_amd.metrics import get_metric, pos_rank
    g = golden("g14_ranking.npz")
    pred = g["pred"]
    assert pred.shape == (257, 99) and pred.dtype == np.float32
    m = get_metric("ndcg@10")
    ranks = m.get_pos_rank(pred.reshape(-1))
    assert np.array_equal(ranks, g["ranks"])
    assert np.array_equal(m.get_pos_rank(pred), g["ranks"])  # 2-D and flattened agree
    assert np.array_equal(pos_rank(pred, 99), rank_rule(pred))
    for k in (1, 5, 10, 99):
        for name in ("ndcg", "hit"):
            mk = get_metric(f"{name}@{k}")
            want = float(g[f"{name}@{k}"])
            for got in (mk(pred.reshape(-1), None), mk(pred, None), mk.fast_calc(g["ranks"])):
                assert abs(float(got) - want) <= 1e-12 * abs(want), (name, k, got, want)
    with pytest.raises(ValueError):
        m.get_pos_rank(pred.reshape(-1)[:-1])


def test_rank_rule_ties_and_nans():
    from pytorchrec_amd.metrics import NDCG, Hit
    nan, inf = float("nan"), float("inf")
    rows = np.array([[1.0, 1.0, 1.0, 1.0],     # all equal: rank 1
                     [0.5, 0.5, 0.7, 0.2],     # a tie and one above: rank 2
                     [nan, 0.1, 0.2, 0.3],     # NaN positive: rank N
                     [0.0, nan, nan, 1.0],     # NaN elsewhere never counts: rank 2
                     [-inf, -inf, 0.0, inf],   # rank 3
                     [inf, inf, inf, nan]],    # rank 1
                    np.float32)
    want = np.array([1, 2, 4, 2, 3, 1])
    m = NDCG(4, 2)
    assert np.array_equal(m.get_pos_rank(rows), want)
    assert np.array_equal(m.get_pos_rank(rows.reshape(-1)), want)
    assert np.array_equal(rank_rule(rows), want)
    assert abs(m(rows, None) - (1 + 1 / np.log2(3) + 1 / np.log2(3) + 1) / 6) < 1e-15
    assert Hit(4, 1)(rows, None) == 2 / 6
    # any N >= 1 for a 2-D input, whatever user_sample_n says
    assert np.array_equal(NDCG(99, 10).get_pos_rank(np.zeros((3, 1), np.float32)), [1, 1, 1])
    assert np.array_equal(NDCG(99, 10).get_pos_rank(rows), want)


# ---------------------------------------------------------------------------
# one pairwise train step
# ---------------------------------------------------------------------------

def test_funksvd_pairwise_bpr_step_matches_reference_g14_cpu():
    check_funksvd_bpr_step_g14(funk(), torch.device("cpu"))


# ---------------------------------------------------------------------------
# the negative sampler (CPU path)
# ---------------------------------------------------------------------------

def sampler_case(device=None, seed=0):
    """50 users over items [5, 69): user 0 holds every even item (half the range free),
    user 1 the whole range, user 2 nothing, the others random sets."""
    from pytorchrec_amd.sampling import NegativeSampler
    rng = np.random.default_rng(7)
    low, high = 5, 69
    sets = {0: np.arange(low + 1, high, 2), 1: np.arange(low, high), 2: np.zeros(0, np.int64)}
    assert len(sets[0]) * 2 == high - low
    for u in range(3, 50):
        sets[u] = rng.choice(np.arange(low, high), size=int(rng.integers(1, 40)), replace=False)
    uu = np.concatenate([np.full(len(v), u) for u, v in sets.items()])
    ii = np.concatenate([v for v in sets.values()])
    uu, ii = np.concatenate([uu, uu[:20]]), np.concatenate([ii, ii[:20]])  # duplicates
    return NegativeSampler(uu, ii, low, high, seed=seed, n_users=50, device=device), sets, low, high


def test_sampler_csr_and_draws():
    s, sets, low, high = sampler_case()
    off, items = s.offsets.numpy(), s.items.numpy()
    assert off.dtype == np.int64 and items.dtype == np.int32 and off.shape == (51,)
    for u, v in sets.items():
        assert np.array_equal(items[off[u]:off[u + 1]], np.unique(v)), u
    uids = torch.tensor([u for u in range(2, 50)] * 6 + [0] * 40 + [77, -3], dtype=torch.int64)
    out = s.sample(uids, n_neg=4, step=3)
    assert out.dtype == torch.int32 and out.shape == (len(uids), 4)
    o = out.numpy()
    assert o.min() >= low and o.max() < high
    for b, u in enumerate(uids.tolist()):
        assert not np.isin(o[b], sets.get(u, [])).any(), (b, u)
    assert s.unresolved() == 0  # user 0 has half the range free: 2^-32 per output
    # unknown uids draw freely over the whole range
    free = s.sample(torch.full((4096,), 1000, dtype=torch.int32), 1, step=0).numpy()
    assert set(free.reshape(-1).tolist()) == set(range(low, high))
    far = s.sample(torch.tensor([1 << 40, -(1 << 40)]), 2, step=0).numpy()  # past int32
    assert far.min() >= low and far.max() < high
    # same (seed, step) -> same bits; another step or seed -> another tensor
    assert torch.equal(out, s.sample(uids, n_neg=4, step=3))
    assert not torch.equal(out, s.sample(uids, n_neg=4, step=4))
    assert not torch.equal(out, sampler_case(seed=1)[0].sample(uids, n_neg=4, step=3))
    assert torch.equal(out, s.sample(uids.int(), n_neg=4, step=3))  # int32 uids
    # output (b, j) is flat output b * n_neg + j
    flat = s.sample(uids.repeat_interleave(4), n_neg=1, step=3)
    assert torch.equal(out.reshape(-1), flat.reshape(-1))
    assert s.unresolved() == 0


def test_sampler_counts_what_it_could_not_resolve():
    s, sets, low, high = sampler_case()
    out = s.sample(torch.tensor([1, 2, 1], dtype=torch.int32), n_neg=5, step=0).numpy()
    assert s.unresolved() == 10  # user 1's set covers the range: every output of its rows
    assert out.min() >= low and out.max() < high
    s2 = sampler_case()[0]
    s2.sample(torch.tensor([1], dtype=torch.int32), n_neg=3, step=9)
    assert s2.unresolved() == 3


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sampler_draws_are_uniform(seed):
    """64 items, empty sets, 65,536 draws: chi^2 under 103.4, the 0.999 quantile of
    chi^2 with 63 degrees of freedom -- a bad hash or a biased map fails it."""
    from pytorchrec_amd.sampling import NegativeSampler
    s = NegativeSampler([], [], 0, 64, seed=seed, n_users=0)
    draws = s.sample(torch.zeros(65536, dtype=torch.int32), 1, step=0).numpy().reshape(-1)
    counts = np.bincount(draws, minlength=64)
    assert counts.shape == (64,)
    chi2 = float(((counts - 1024.0) ** 2 / 1024.0).sum())
    print(f"seed {seed}: chi2 = {chi2:.2f}")
    assert chi2 < 103.4, chi2


# ---------------------------------------------------------------------------
# fit(train_mode="pair_wise")
# ---------------------------------------------------------------------------

def planted_set(users=200, items=120, groups=4, per_user=9, seed=5):
    """Users and items in `groups` groups; a user's positives come from its own group:
    `per_user` for training and one held out, first of its 99 dev candidates."""
    rng = np.random.default_rng(seed)
    per_group = items // groups
    tu, ti, dev = [], [], np.empty((users, 99), np.int64)
    for u in range(users):
        own = (u % groups) * per_group + rng.choice(per_group, per_user + 1, replace=False)
        tu += [u] * per_user
        ti += own[:per_user].tolist()
        others = np.setdiff1d(np.arange(items), own)
        dev[u] = np.concatenate([own[per_user:], rng.choice(others, 98, replace=False)])
    return np.array(tu), np.array(ti), np.arange(users), dev


def test_fit_pair_wise_with_the_sampler():
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.metrics import get_metric, pos_rank
    from pytorchrec_amd.sampling import NegativeSampler
    tu, ti, du, dev = planted_set()
    train = ColumnarDataset({"uid": tu, "iid": ti})
    devset = ColumnarDataset({"uid": du, "iid": dev})
    m = funk(emb_size=16, users=200, items=120, seed=11)
    metrics = [get_metric("ndcg@10"), get_metric("hit@10")]
    cpu = torch.device("cpu")
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), BPRLoss(), metrics, cpu)
    with pytest.raises(ValueError, match="train_neg_sample.*set_negative_sampler"):
        m.fit(train, 256, 1, train_mode="pair_wise", verbose=0)
    m.set_negative_sampler(NegativeSampler(tu, ti, 0, 120, seed=3, n_users=200))
    hist = m.fit(train, 256, 10, dev_dataset=devset, train_mode="pair_wise", verbose=0)
    assert len(hist) == 10
    for row in hist:
        assert set(row) == {"loss", "ndcg@10", "hit@10"}
    print("loss per epoch:", [round(r["loss"], 4) for r in hist],
          "ndcg@10:", [round(r["ndcg@10"], 4) for r in hist])
    assert hist[-1]["loss"] < 0.5 * hist[0]["loss"], (hist[0]["loss"], hist[-1]["loss"])
    assert m._neg_step == 10 * 8  # one draw per train_step (1800 rows in batches of 256)
    got = m.evaluate(devset, 128, verbose=0)
    pred = m.predict(devset, 77)
    assert pred.shape == (200, 99)
    ranks = pos_rank(pred, 99)
    for mk in metrics:
        assert got[mk.name] == float(mk.fast_calc(ranks)) == hist[-1][mk.name]


# ---------------------------------------------------------------------------
# ABI: argument validation before any device work (no GPU present)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorchrec_amd import _mrec
    return _mrec.lib()


P = 4096  # a non-NULL address that is never dereferenced: validation comes first


def _einval(lib, st, word):
    from pytorchrec_amd import _mrec
    assert st == _mrec.EINVAL, st
    assert word.encode() in lib.mrec_last_error(), lib.mrec_last_error()


def test_pair_loss_exports_validate_their_arguments(lib):
    fwd, bwd = lib.mrec_pair_loss_fwd, lib.mrec_pair_loss_bwd
    _einval(lib, fwd(None, 2, 8, 0, 1, P, None), "NULL")
    _einval(lib, fwd(P, 2, 8, 0, 1, None, None), "NULL")
    _einval(lib, fwd(P, 2, -1, 0, 1, P, None), "shape")
    _einval(lib, fwd(P, 1, 8, 0, 1, P, None), "shape")
    _einval(lib, fwd(P, 2, 8, 2, 1, P, None), "unknown")
    _einval(lib, fwd(P, 2, 8, -1, 1, P, None), "unknown")
    _einval(lib, fwd(P, 2, 8, 1, 3, P, None), "unknown")
    _einval(lib, bwd(None, 2, 8, 0, 1, P, P, None), "NULL")
    _einval(lib, bwd(P, 2, 8, 0, 1, None, P, None), "NULL")
    _einval(lib, bwd(P, 2, 8, 0, 1, P, None, None), "NULL")
    _einval(lib, bwd(P, 2, -1, 0, 1, P, P, None), "shape")
    _einval(lib, bwd(P, 0, 8, 0, 1, P, P, None), "shape")
    _einval(lib, bwd(P, 2, 8, 7, 1, P, P, None), "unknown")
    _einval(lib, bwd(P, 2, 8, 0, -2, P, P, None), "unknown")


def test_rank_pos_validates_its_arguments(lib):
    f = lib.mrec_rank_pos
    _einval(lib, f(None, 4, 99, 99, P, None), "NULL")
    _einval(lib, f(P, 4, 99, 99, None, None), "NULL")
    _einval(lib, f(P, -1, 99, 99, P, None), "row count")
    _einval(lib, f(P, 4, 0, 99, P, None), "n < 1")
    _einval(lib, f(P, 4, 99, 98, P, None), "ld < n")


def test_neg_sample_validates_its_arguments(lib):
    from pytorchrec_amd import _mrec
    f = lib.mrec_neg_sample
    ok = [P, _mrec.I32, 8, 1, P, P, 10, 0, 64, 0, 0, P, P, None]

    def call(**kw):
        names = ["uids", "dt", "batch", "n_neg", "offsets", "items", "n_users", "low", "high",
                 "seed", "step", "out", "unres", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return f(*a)

    for k in ("uids", "offsets", "items", "out", "unres"):
        _einval(lib, call(**{k: None}), "NULL")
    _einval(lib, call(dt=_mrec.F32), "int32 or int64")
    _einval(lib, call(batch=-1), "negative")
    _einval(lib, call(n_users=-1), "negative")
    _einval(lib, call(n_neg=0), "n_neg < 1")
    _einval(lib, call(high=0), "high <= low")
    _einval(lib, call(low=5, high=4), "high <= low")
    # the attempt bound lives in the header; the binding restates it
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "mrec.h")) as fh:
        bound = int(re.search(r"#define MREC_NEG_MAX_ATTEMPTS (\d+)", fh.read()).group(1))
    assert bound == _mrec.NEG_MAX_ATTEMPTS == 32
