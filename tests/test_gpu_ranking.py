"""Ranking training and evaluation on the GPU: the pair-loss kernels, mrec_rank_pos,
the device-side ``evaluate``, one pairwise FunkSVD step against golden G14, the
sampler kernel against its numpy restatement, and training end to end with sampled
negatives.

Tolerances are those of tests/test_ranking_cpu.py: loss values rtol 1e-5 / atol 1e-6
and gradients rtol 1e-4 / atol 1e-6 against the fp64 evaluation of the reference
formula; the FunkSVD steps use G10's (loss rtol 1e-5, tables rtol 1e-5 / atol 1e-8,
untouched rows bit-equal).  Ranks and sampled items are compared exactly.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from test_ranking_cpu import (KINDS, REDUCTIONS, check_funksvd_bpr_step_g14, funk, pair_loss_f64,
                              rank_rule, sampler_case)

pytestmark = pytest.mark.gpu


@pytest.fixture
def calls(monkeypatch):
    """Names of the libmrec entry points called while the fixture is live."""
    from pytorchrec_amd import _mrec
    names = []
    real = _mrec.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_mrec, "call", spy)
    return names


# ---------------------------------------------------------------------------
# pair-loss kernels
# ---------------------------------------------------------------------------

def _pair_input(B):
    """G14's x (its first rows are the extreme ones) repeated up to B rows, with the
    repeats scaled so they are new values."""
    x = golden("g14_ranking.npz")["x"]
    reps = -(-max(B, 1) // len(x))
    x = np.concatenate([x * np.float32(1.0 - 0.13 * r) for r in range(reps)])[:B]
    return np.ascontiguousarray(x, np.float32)


def _run_pair(gpu, kind, reduction, x, g):
    """Forward + backward through a [B, 2] slice of a [B, 4] tensor with upstream g."""
    from pytorchrec_amd.loss import get_loss
    B = len(x)
    x4 = torch.full((B, 4), 7.0, device=gpu)
    x4[:, 1:3] = torch.from_numpy(x).to(gpu)
    x4.requires_grad_()
    view = x4[:, 1:3]
    assert B < 2 or not view.is_contiguous()
    loss = get_loss(kind)(reduction=reduction)(view, None)
    gt = torch.from_numpy(np.asarray(g, np.float32)).to(gpu)
    if reduction == "none":
        loss.backward(gt)
    else:
        (loss * gt.reshape(())).backward()  # the upstream gradient is a device scalar
    grad = x4.grad
    assert torch.count_nonzero(grad[:, 0]) == 0 and torch.count_nonzero(grad[:, 3]) == 0
    return loss.detach(), grad[:, 1:3].detach().clone()


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099])
@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_pair_loss_kernels_match_fp64(gpu, calls, kind, reduction, B):
    x = _pair_input(B)
    rng = np.random.default_rng(B)
    g = (rng.uniform(0.5, 2.0, B) * rng.choice([-1.0, 1.0], B)).astype(np.float32) \
        if reduction == "none" else np.array([-1.75], np.float32)
    loss, grad = _run_pair(gpu, kind, reduction, x, g)
    assert calls.count("mrec_pair_loss_fwd") == 1 and calls.count("mrec_pair_loss_bwd") == 1
    want, want_grad = pair_loss_f64(kind, x, reduction, g.astype(np.float64))
    np.testing.assert_allclose(loss.cpu().numpy(), want, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), want_grad, rtol=1e-4, atol=1e-6)
    if reduction == "none":  # the fixture's own rows against the reference's outputs
        n = min(B, 1000)
        np.testing.assert_allclose(loss.cpu().numpy()[:n],
                                   golden("g14_ranking.npz")[f"{kind}_none"][:n],
                                   rtol=1e-5, atol=1e-6)
    loss2, grad2 = _run_pair(gpu, kind, reduction, x, g)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), "two runs differ in bits"


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_pair_loss_kernels_match_reference_g14(gpu, kind, reduction):
    g = golden("g14_ranking.npz")
    ones = np.ones(1000 if reduction == "none" else 1, np.float32)
    loss, grad = _run_pair(gpu, kind, reduction, g["x"], ones)
    np.testing.assert_allclose(loss.cpu().numpy(), g[f"{kind}_{reduction}"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), g[f"{kind}_{reduction}_grad"], rtol=1e-4,
                               atol=1e-6)


@pytest.mark.parametrize("kind", KINDS)
def test_pair_loss_of_an_empty_batch(gpu, kind):
    from pytorchrec_amd.loss import get_loss
    for reduction in REDUCTIONS:
        x = torch.zeros(0, 2, device=gpu, requires_grad=True)
        loss = get_loss(kind)(reduction=reduction)(x, None)
        if reduction == "none":
            assert loss.shape == (0,)
        else:
            assert float(loss.detach()) == 0.0
        loss.sum().backward()
        assert x.grad.shape == (0, 2)
    with pytest.raises(AssertionError):
        get_loss(kind)()(torch.zeros(4, 3, device=gpu), None)
    # the kernel's own batch 0: the reduced loss is written as 0
    from pytorchrec_amd import _mrec
    some = torch.ones(2, device=gpu)
    for reduction in (_mrec.REDUCE_MEAN, _mrec.REDUCE_SUM):
        out = torch.full((1,), 5.0, device=gpu)
        _mrec.call("mrec_pair_loss_fwd", some.data_ptr(), 2, 0, KINDS.index(kind), reduction,
                   out.data_ptr(), _mrec.stream_handle())
        assert float(out) == 0.0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# mrec_rank_pos
# ---------------------------------------------------------------------------

def _rank_rows(rows, N, seed):
    """Scores with ties (a coarse grid), +-inf and NaNs, in column 0 and elsewhere."""
    rng = np.random.default_rng(seed)
    p = np.round(rng.standard_normal((rows, N)) * 4).astype(np.float32) / 4
    fine = rng.standard_normal((rows, N)).astype(np.float32)
    p[2::3] = fine[2::3]  # tie-free rows too
    for r in range(rows):
        kind = r % 8
        if kind == 1:
            p[r, 0] = np.nan
        elif kind == 2 and N > 1:
            p[r, rng.integers(1, N, max(1, N // 5))] = np.nan
        elif kind == 3:
            p[r] = p[r, 0]  # all equal
        elif kind == 4:
            p[r, rng.integers(0, N, 3)] = np.inf
        elif kind == 5:
            p[r, 0] = -np.inf
            p[r, N // 2:] = -np.inf
        elif kind == 6:
            p[r, 0] = np.inf
    return p


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 99, 100, 129, 1000])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_rank_pos_matches_the_rule(gpu, calls, rows, N):
    from pytorchrec_amd.metrics import pos_rank, rank_pos_device
    for variant in range(2 if rows > 1 else 8):
        p = _rank_rows(max(rows, 8), N, seed=rows * 1009 + N + variant)
        # (a single row takes each of the 8 kinds of row in turn)
        p = np.ascontiguousarray(p[variant:variant + 1] if rows == 1 else p[:rows])
        want = rank_rule(p)
        assert np.array_equal(want, pos_rank(p, 99))
        dense = torch.from_numpy(p).to(gpu)
        wide = torch.full((rows, N + 3), float("inf"), device=gpu)  # pad columns must not count
        wide[:, :N] = dense
        for t, ld in ((dense, N), (wide[:, :N], N + 3)):
            assert t.stride(0) == ld or rows == 1
            got = rank_pos_device(t)
            assert got.dtype == torch.int32 and got.shape == (rows,)
            assert np.array_equal(got.cpu().numpy(), want), (rows, N, ld)
    assert set(calls) == {"mrec_rank_pos"}


def test_rank_pos_matches_reference_g14(gpu):
    from pytorchrec_amd.metrics import rank_pos_device
    g = golden("g14_ranking.npz")
    got = rank_pos_device(torch.from_numpy(g["pred"]).to(gpu))
    assert np.array_equal(got.cpu().numpy(), g["ranks"])


# ---------------------------------------------------------------------------
# evaluate
# ---------------------------------------------------------------------------

def test_evaluate_ranks_on_the_device(gpu, calls):
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.metrics import get_metric, pos_rank
    U, items = 300, 500
    rng = np.random.default_rng(42)
    dev = ColumnarDataset({"uid": np.arange(U), "iid": rng.integers(0, items, (U, 99))})
    m = funk(emb_size=8, users=U, items=items, seed=3)
    ranking = [get_metric("ndcg@10"), get_metric("hit@10"), get_metric("ndcg@1")]
    opt = torch.optim.SGD(m.get_parameters(), lr=0.1)
    m.compile(opt, BPRLoss(), ranking, gpu)
    del calls[:]
    got = m.evaluate(dev, 128, verbose=0)
    assert calls.count("mrec_rank_pos") == 3, calls  # once per batch of 128, 128, 44
    pred = m.predict(dev, 128)
    assert pred.shape == (U, 99)
    ranks = pos_rank(pred, 99)
    assert len(set(ranks.tolist())) > 10  # (not a degenerate ranking)
    assert set(got) == {"ndcg@10", "hit@10", "ndcg@1"}
    for mk in ranking:
        want = float(mk.fast_calc(ranks))
        assert abs(got[mk.name] - want) <= 1e-12 * abs(want), (mk.name, got[mk.name], want)
    # a CTR metric in the list: the host path, the same ranking values
    m.compile(opt, BPRLoss(), ranking + [get_metric("auc")], gpu)
    del calls[:]
    mixed = m.evaluate(dev, 128, verbose=0)
    assert "mrec_rank_pos" not in calls
    assert 0.0 <= mixed["auc"] <= 1.0
    for mk in ranking:
        assert abs(mixed[mk.name] - got[mk.name]) <= 1e-12 * abs(got[mk.name])


# ---------------------------------------------------------------------------
# one pairwise train step against the reference
# ---------------------------------------------------------------------------

def test_funksvd_pairwise_bpr_step_matches_reference_g14(gpu, calls):
    """The fused-SGD bank plus the pair-loss kernels against the reference's own step."""
    m = funk()
    check_funksvd_bpr_step_g14(m, gpu)
    assert m.embeddings.update == "sgd" and m.embeddings.weight.is_cuda
    assert calls.count("mrec_pair_loss_fwd") == 1 and calls.count("mrec_pair_loss_bwd") == 1


# ---------------------------------------------------------------------------
# the sampler kernel against its numpy restatement
# ---------------------------------------------------------------------------

def _big_sampler(device):
    """Negative ids, a 150,000-item set (a deep binary search), an empty and a small set."""
    from pytorchrec_amd.sampling import NegativeSampler
    rng = np.random.default_rng(99)
    low, high = -1000, 200000
    big = rng.choice(np.arange(low, high), 150000, replace=False)
    small = np.array([-1000, -1, 0, 1, 199999, 5, 77, 4096, 65536, 131072])
    uu = np.concatenate([np.zeros(len(big), np.int64), np.full(len(small), 2)])
    return NegativeSampler(uu, np.concatenate([big, small]), low, high, seed=5, n_users=3,
                           device=device)


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_sampler_kernel_equals_the_cpu_path(gpu, calls, B):
    cases = [(sampler_case(gpu)[0], sampler_case()[0], 50), (_big_sampler(gpu), _big_sampler(None), 3)]
    for on_gpu, on_cpu, users in cases:
        assert on_gpu.items.is_cuda and on_gpu.offsets.dtype == torch.int64
        rng = np.random.default_rng(B)
        uids = rng.integers(-2, users + 3, B)  # unknown uids on both sides
        uids[0] = 1 if users == 50 else 0      # the full set / the large set
        for n_neg in (1, 4):
            for dt in (torch.int32, torch.int64):
                u = torch.from_numpy(uids).to(dt)
                step = 10 * n_neg + (dt == torch.int64)
                got = on_gpu.sample(u.to(gpu), n_neg, step=step)
                want = on_cpu.sample(u, n_neg, step=step)
                assert got.is_cuda and got.dtype == torch.int32 and got.shape == (B, n_neg)
                assert torch.equal(got.cpu(), want), (B, n_neg, dt)
        assert on_gpu.unresolved() == on_cpu.unresolved()
        if users == 50:
            assert on_cpu.unresolved() >= 2 * (1 + 4)  # user 1's rows, every call
    assert set(calls) == {"mrec_neg_sample"}


def test_sampling_refuses_graph_capture(gpu, calls, monkeypatch):
    """Sampling inside a HIP-graph capture is out of scope: a clear error, no launch."""
    s = sampler_case(gpu)[0]
    u = torch.zeros(8, dtype=torch.int32, device=gpu)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        s.sample(u, 1)
    assert "mrec_neg_sample" not in calls


# ---------------------------------------------------------------------------
# training end to end with sampled negatives
# ---------------------------------------------------------------------------

def test_train_steps_with_sampled_negatives_match_the_cpu_model(gpu):
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.sampling import NegativeSampler
    rng = np.random.default_rng(8)
    B, lr = 64, 0.5
    uid = rng.integers(0, 40, B)  # users 40..49 stay untouched
    iid = rng.integers(0, 30, B)  # and items 30..36: the sampler draws from [0, 30) too
    mg, mc = funk(), funk()
    mg.compile(torch.optim.SGD(mg.get_parameters(), lr=lr), BPRLoss(), [], gpu)
    mc.compile(torch.optim.SGD(mc.get_parameters(), lr=lr), BPRLoss(), [], torch.device("cpu"))
    assert mg.embeddings.update == "sgd"
    mg.set_negative_sampler(NegativeSampler(uid, iid, 0, 30, seed=1, n_users=50, device=gpu), n_neg=1)
    seen = []
    mg.register_forward_pre_hook(lambda mod, args: seen.append(args[0]["iid"].detach().cpu()))
    before = {k: v.cpu().numpy().copy() for k, v in mg.state_dict().items()}
    batch = {"uid": torch.from_numpy(uid).int(), "iid": torch.from_numpy(iid).int()}
    for step in range(3):
        lg = float(mg.train_step(dict(batch))["loss"].detach())
        cand = seen[-1]
        assert cand.shape == (B, 2) and np.array_equal(cand[:, 0].numpy(), iid)
        neg = cand[:, 1].numpy()
        assert neg.min() >= 0 and neg.max() < 30
        for b in range(B):
            assert neg[b] not in iid[uid == uid[b]]
        lc = float(mc.train_step({"uid": batch["uid"], "iid": cand})["loss"].detach())
        assert abs(lg - lc) <= 1e-5 * abs(lc), (step, lg, lc)
    assert len(seen) == 3 and not torch.equal(seen[0], seen[1])  # a fresh draw per step
    assert mg._neg_sampler.unresolved() == 0
    sg, sc = mg.state_dict(), mc.state_dict()
    touched_i = np.unique(torch.cat(seen).numpy())
    for key, touched in (("u_embeddings.weight", np.unique(uid)), ("i_embeddings.weight", touched_i)):
        got = sg[key].cpu().numpy()
        np.testing.assert_allclose(got, sc[key].numpy(), rtol=1e-5, atol=1e-8, err_msg=key)
        rest = np.setdiff1d(np.arange(got.shape[0]), touched)
        assert len(rest) and np.array_equal(got[rest].view(np.uint32), before[key][rest].view(np.uint32))
        assert not np.array_equal(got[touched], before[key][touched])
