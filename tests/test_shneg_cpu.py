"""Shared-negative list-wise losses on the CPU path (no GPU): ``cpu_path.shared_negative_loss``
against the pairwise losses and ``cross_entropy``, its gradients (gradcheck), the masking
rules, the model layer (``set_shared_negatives`` for funksvd / sasrec / gru4rec), the
argument validation of the new libmrec exports -- and the fp64 oracle with the derived
tolerance that the GPU suite (test_gpu_shneg.py) imports.

The oracle and its tolerance
----------------------------
``oracle`` restates include/mrec.h "Shared negatives" in fp64 on the bf16-rounded operands
(the products' operands are exact in both, so what is left is the kernel's own arithmetic)
and returns, next to every result, a bound on |kernel - oracle| that is derived, term by
term, from the number formats (u = 2^-24, the unit roundoff of fp32):

* Scores.  s[b, j] is a sum of D exact products accumulated in fp32 plus an fp32 bias:
  |ds| <= (D + 2) u mag, mag = sum_d |q| |neg| + |bias|; the same for s+.  Ds_b is the
  largest of these over query b's unmasked candidates and its positive.
* A sum of n_b + 1 non-negative fp32 terms, in any order: relative (n_b + 1) u.
* The arguments of exp / sigmoid are differences of two fp32 scores: one more rounding,
  u R_b with R_b the largest |argument| of the query; an argument perturbed by e changes
  exp, sigmoid, sigmoid' (|f'| <= f) by the relative amount exp(e) - 1 at the most.
* The device functions (expf, logf, log1pf(expf), the sigmoid and sigmoid' built from expf
  and one division).  The HIP documentation installed with the toolchain states no error
  bound for them, so each was measured ALONE against fp64 on an MI355X (the probe
  ``mrec_shneg_math_probe``, tools/bench_shneg.py --probe; 2^22 arguments each, uniform over
  [-170, 170] ([-170, 20] for expf), log-uniform over [1e-3, 1e6] for logf -- wider than any
  argument of these tests; profiles/shneg/math_probe.json): worst relative error expf
  1.39 u, logf 3.12 u, softplus 2.20 u, sigmoid 2.91 u, sigmoid' 4.69 u (another draw of the
  same ranges gave 2.97 u and 4.80 u).  EPS_F = 10 u is twice the worst of them, rounded up;
  a coefficient passes through at most three such calls (C_F = 3).
* The coefficients a[b, j] enter the MFMA as hi + lo, two bf16 values (the header says so):
  hi = bf16(a), lo = bf16(a - hi), and a - hi is exact in fp32.  Round-to-nearest to bf16's
  8 significant bits is 2^-8 relative at the worst (2^-9 only at the top of a binade), so
  what is lost is 2^-8 |lo| <= 2^-16 |a|: COEF = 2^-16 relative each.  a[b, +] is not rounded.
* A coefficient below fp32's normal range (2^-126 g_b: exp of a score far under the
  maximum) is kept with less than full precision, or flushed: 2^-126 |g_b| absolute each.
* The two gradient sums accumulate in fp32: (terms + 3) u of the sum of magnitudes.  The
  output rounding: u in fp32, 2^-8 in bf16 (8 significant bits), of the result's magnitude.

So per query rho_b = C_F EPS_F + (n_b + 2) u + 8 u is the relative error of a coefficient
besides the perturbed scores, E[b, j] = A[b, j] (rho_b + (exp(e_b) - 1) + COEF) bounds the
error of one coefficient of magnitude A[b, j] (top1 adds the term of s sigmoid'(s^2), whose
argument s^2 moves by 2 |s| ds), and the gradients' bounds are E propagated through the
fp64 sums of magnitudes: tol(dq) = E |neg| + E+ |pos| + (S + 3) u (A |neg| + |a+| |pos|) +
rounding, and likewise for dneg and dpos.  The loss bound is 2 Ds_b (|dL/ds| sums to at
most 2) plus the relative terms above on the summed quantity, plus EPS_F |log| for softmax.
``test_fp32_restatement_is_inside_the_bound`` shows that the bound (without the bf16 term,
which the torch path does not have) holds for a plain fp32 evaluation and is small: it is
neither vacuous nor broken by the oracle alone.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

from test_gru4rec_cpu import gru4rec
from test_ranking_cpu import funk
from test_sasrec_cpu import planted_sequences, sasrec

U = 2.0 ** -24
EPS_F = 10 * U   # twice the worst measured relative error of the device functions (docstring)
C_F = 3
BF = 2.0 ** -8    # round-to-nearest to bf16, relative, at the worst
COEF = 2.0 ** -16  # a coefficient as hi + lo
UNDER = 2.0 ** -126
KINDS = ("softmax", "bpr", "top1")


def bf16(t):
    return t.detach().to(torch.bfloat16).to(torch.float64)


def _sig(x):
    return torch.sigmoid(x)


def _dsig(x):
    return torch.sigmoid(x) * torch.sigmoid(-x)


def oracle(q, pos, neg, kind, reduction, g, pos_id=None, neg_id=None, pos_bias=None, neg_bias=None,
           coef_bf16=True):
    """fp64 restatement of the contract on the bf16-rounded operands -> dict with ``loss``,
    ``dq``, ``dpos``, ``dneg`` and a bound ``tol_*`` on each (module docstring).  ``g`` is the
    upstream gradient ([B] for ``none``, else a scalar).  The gradients' output rounding is
    derived from the operands' dtypes."""
    dev = q.device
    Q, P, N = bf16(q), bf16(pos), bf16(neg)
    B, D = Q.shape
    S = N.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    if pos_id is not None:
        mask = neg_id.reshape(1, S).to(torch.int64) == pos_id.reshape(B, 1).to(torch.int64)
        if B:
            N = torch.where(mask.all(0).unsqueeze(1), torch.zeros_like(N), N)
    else:
        mask = torch.zeros(B, S, dtype=torch.bool, device=dev)
    live = ~mask
    nb = neg_bias.double().reshape(1, S) if neg_bias is not None else torch.zeros(1, S, **f64)
    pb = pos_bias.double().reshape(B) if pos_bias is not None else torch.zeros(B, **f64)
    s = torch.where(live, Q @ N.t() + nb, torch.zeros(1, **f64))
    sp = (Q * P).sum(1) + pb
    ds = (D + 2) * U * (Q.abs() @ N.abs().t() + nb.abs()) * live
    dsp = (D + 2) * U * ((Q.abs() * P.abs()).sum(1) + pb.abs())
    Ds = torch.maximum(dsp, ds.max(1).values if S else torch.zeros(B, **f64))
    n = live.sum(1).double()
    gv = torch.as_tensor(g, **f64)
    gb = gv.reshape(B) if reduction == "none" else (gv / max(B, 1) if reduction == "mean" else gv).expand(B)
    rho = C_F * EPS_F + (n + 2) * U + 8 * U
    ninf = torch.full((1,), float("-inf"), **f64)
    if kind == "softmax":
        M = torch.maximum(sp, torch.where(live, s, ninf).max(1).values if S else sp)
        e = torch.where(live, torch.exp(s - M.unsqueeze(1)), torch.zeros(1, **f64))
        ep = torch.exp(sp - M)
        T = ep + e.sum(1)
        L = torch.log(T) + M - sp
        R = torch.maximum((sp - M).abs(), torch.where(live, (s - M.unsqueeze(1)).abs(), torch.zeros(1, **f64)).max(1).values
                          if S else torch.zeros(B, **f64))
        pert = torch.expm1(2 * Ds + U * R)
        tol_L = (2 * Ds + U * R) + rho + EPS_F * torch.log(T).abs() + 4 * U * (torch.log(T).abs() + (M - sp).abs() + L.abs())
        a = gb.unsqueeze(1) * e / T.unsqueeze(1)
        A = a.abs()
        E = A * (rho + pert).unsqueeze(1)
        ap = gb * (ep / T - 1)
        Ep = gb.abs() * (ep / T) * (rho + pert) + 2 * U * gb.abs()
    else:
        x = torch.where(live, s - sp.unsqueeze(1), torch.zeros(1, **f64))
        R = x.abs().max(1).values if S else torch.zeros(B, **f64)
        Dx = 2 * Ds + U * R
        pert = torch.expm1(Dx)
        c = torch.where(n > 0, gb / n.clamp(min=1), torch.zeros(1, **f64))
        if kind == "bpr":
            t = torch.where(live, torch.nn.functional.softplus(x, threshold=1e9), torch.zeros(1, **f64))
            first = _sig(x) * live
            a = c.unsqueeze(1) * first
            E = a.abs() * (rho + pert).unsqueeze(1)
            dL = Dx  # |softplus'| <= 1
        else:
            sq = s * s
            dsq = 2 * s.abs() * (ds + U * s.abs()) + U * sq
            t = torch.where(live, _sig(x) + _sig(sq), torch.zeros(1, **f64))
            first = _dsig(x) * live
            second = 2 * s * _dsig(sq) * live
            a = c.unsqueeze(1) * (first + second)
            E = c.abs().unsqueeze(1) * (first * (rho + pert).unsqueeze(1)
                                        + second.abs() * (rho.unsqueeze(1) + torch.expm1(dsq))
                                        + 2 * ds * _dsig(sq) * live)
            dL = ((first * Dx.unsqueeze(1) + _dsig(sq) * live * dsq).sum(1) / n.clamp(min=1))
        L = t.sum(1) / n.clamp(min=1)
        tol_L = dL + ((n + 1) * U + EPS_F + 8 * U) * L.abs()
        A = c.abs().unsqueeze(1) * (first + (second.abs() if kind == "top1" else 0))
        ap = -(c.unsqueeze(1) * first).sum(1)
        Ep = (c.abs().unsqueeze(1) * first * (rho + pert).unsqueeze(1)).sum(1) + (n + 1) * U * ap.abs()
    E = E + UNDER * gb.abs().unsqueeze(1) * live
    Ep = Ep + UNDER * gb.abs() * (n + 1)
    if coef_bf16:
        E = E + COEF * A
    rq = BF if q.dtype == torch.bfloat16 else U
    rr = BF if pos.dtype == torch.bfloat16 else U
    dq = a @ N + ap.unsqueeze(1) * P
    dpos = ap.unsqueeze(1) * Q
    dneg = a.t() @ Q
    out = {
        "dq": dq, "dpos": dpos, "dneg": dneg, "per_query": L, "n": n,
        "tol_dq": E @ N.abs() + Ep.unsqueeze(1) * P.abs()
                  + (S + 3) * U * (A @ N.abs() + ap.abs().unsqueeze(1) * P.abs()) + rq * dq.abs(),
        "tol_dpos": Ep.unsqueeze(1) * Q.abs() + (2 * U + rr) * dpos.abs(),
        "tol_dneg": E.t() @ Q.abs() + (B + 3) * U * (A.t() @ Q.abs()) + rr * dneg.abs(),
    }
    if reduction == "none":
        out["loss"], out["tol_loss"] = L, tol_L
    else:
        k = 1.0 / max(B, 1) if reduction == "mean" else 1.0
        out["loss"] = L.sum() * k
        out["tol_loss"] = (tol_L.sum() + (B + 2) * U * L.abs().sum()) * k
    return out


def gaussian_case(B, S, D, seed, q_dtype=torch.float32, row_dtype=torch.float32, ids=False, bias=False,
                  scale=0.35, device="cpu"):
    """Gaussian operands (scores of a few units at scale 0.35), optional ids with collisions
    and biases."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, D, generator=g) * scale).to(q_dtype).to(device)
    pos = (torch.randn(B, D, generator=g) * scale).to(row_dtype).to(device)
    neg = (torch.randn(S, D, generator=g) * scale).to(row_dtype).to(device)
    kw = {}
    if ids:
        kw["pos_id"] = torch.randint(0, max(S // 2, 2), (B,), generator=g).to(device)
        kw["neg_id"] = torch.randint(0, max(S // 2, 2), (S,), generator=g).to(device)
    if bias:
        kw["pos_bias"] = torch.randn(B, generator=g).to(device)
        kw["neg_bias"] = torch.randn(S, generator=g).to(device)
    return q, pos, neg, kw


def assert_within(got, want, tol, what):
    got, want, tol = got.detach().double().cpu(), want.cpu(), tol.cpu()
    err = (got - want).abs()
    worst = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |diff| {float(err.max()) if err.numel() else 0.0:.3e}, "
          f"max tol {float(tol.max()) if tol.numel() else 0.0:.3e}, worst diff/tol {worst:.3f}")
    assert bool((err <= tol).all()), (what, worst)


def shared_loss(q, pos, neg, kind, reduction="mean", **kw):
    from pytorchrec_amd import cpu_path
    return cpu_path.shared_negative_loss(q, pos, neg, kind, reduction, kw.get("pos_id"), kw.get("neg_id"),
                                         kw.get("pos_bias"), kw.get("neg_bias"))


# ---------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bpr", "top1"])
@pytest.mark.parametrize("S", [1, 7])
def test_pairwise_kinds_are_the_pairwise_losses_averaged(kind, S):
    from pytorchrec_amd.loss import BPRLoss, Top1Loss
    q, pos, neg, kw = gaussian_case(9, S, 8, seed=1, ids=S > 1)
    got = shared_loss(q, pos, neg, kind, "none", **kw)
    pair = (BPRLoss if kind == "bpr" else Top1Loss)(reduction="none")
    sp, s = (q * pos).sum(1), q @ neg.t()
    per = torch.stack([pair(torch.stack([sp, s[:, j]], 1), None) for j in range(S)], 1)
    if S == 1:
        assert torch.allclose(got, per[:, 0], rtol=1e-6, atol=1e-7)
        return
    live = kw["neg_id"].reshape(1, S) != kw["pos_id"].reshape(-1, 1)
    assert 0 < int((~live).sum()) < live.numel()
    want = (per * live).sum(1) / live.sum(1).clamp(min=1)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_softmax_is_cross_entropy_over_the_unmasked(reduction):
    q, pos, neg, kw = gaussian_case(11, 13, 16, seed=2, ids=True, bias=True)
    got = shared_loss(q, pos, neg, "softmax", reduction, **kw)
    sp = (q * pos).sum(1) + kw["pos_bias"]
    s = q @ neg.t() + kw["neg_bias"]
    mask = kw["neg_id"].reshape(1, -1) == kw["pos_id"].reshape(-1, 1)
    assert bool(mask.any())
    logits = torch.cat([sp.unsqueeze(1), s.masked_fill(mask, float("-inf"))], 1)
    want = torch.nn.functional.cross_entropy(logits, torch.zeros(11, dtype=torch.int64), reduction=reduction)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("kind", KINDS)
def test_gradcheck_fp64(kind):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(3, 4, generator=g, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(3, 4, generator=g, dtype=torch.float64, requires_grad=True)
    neg = torch.randn(5, 4, generator=g, dtype=torch.float64, requires_grad=True)
    pid, nid = torch.tensor([0, 1, 2]), torch.tensor([2, 5, 0, 6, 7])
    pb, nb = torch.randn(3, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    from pytorchrec_amd import cpu_path
    for red in ("none", "mean", "sum"):
        assert torch.autograd.gradcheck(
            lambda a, b, c: cpu_path.shared_negative_loss(a, b, c, kind, red, pid, nid, pb, nb), (q, pos, neg))
    # in-batch: the same tensor on both sides
    assert torch.autograd.gradcheck(
        lambda a, b: cpu_path.shared_negative_loss(a, b, b, kind, "mean", pid, pid), (q, pos))


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_agrees_with_autograd(kind):
    """The oracle's hand-written gradients are the autograd gradients of the fp64 loss."""
    q, pos, neg, kw = gaussian_case(7, 9, 8, seed=4, ids=True, bias=True)
    Q, P, N = (bf16(t).requires_grad_() for t in (q, pos, neg))
    up = torch.linspace(0.5, 2.0, 7, dtype=torch.float64)
    shared_loss(Q, P, N, kind, "none", **kw).backward(up)
    o = oracle(q, pos, neg, kind, "none", up, **kw)
    for got, want in ((Q.grad, o["dq"]), (P.grad, o["dpos"]), (N.grad, o["dneg"])):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12)
    assert torch.allclose(shared_loss(Q, P, N, kind, "none", **kw), o["loss"], rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------
# masking and the empty shapes
# ---------------------------------------------------------------------------

def _loss_and_grads(q, pos, neg, kind, reduction="sum", **kw):
    q, pos, neg = (t.detach().clone().requires_grad_() for t in (q, pos, neg))
    loss = shared_loss(q, pos, neg, kind, reduction, **kw)
    loss.sum().backward()
    return loss.detach(), q.grad, pos.grad, neg.grad


@pytest.mark.parametrize("kind", KINDS)
def test_masked_candidate_row_of_nan_changes_nothing(kind):
    q, pos, neg, _ = gaussian_case(6, 5, 8, seed=5)
    pid = torch.tensor([3, 3, 3, 3, 3, 3])
    nid = torch.tensor([0, 3, 1, 2, 3])  # candidates 1 and 4 are masked for every query
    ref = _loss_and_grads(q, pos, torch.where(nid.unsqueeze(1) == 3, torch.zeros(1), neg), kind, pos_id=pid, neg_id=nid)
    bad = neg.clone()
    bad[nid == 3] = float("nan")
    got = _loss_and_grads(q, pos, bad, kind, pos_id=pid, neg_id=nid)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert torch.equal(got[3][nid == 3], torch.zeros(2, 8))


@pytest.mark.parametrize("kind", KINDS)
def test_no_unmasked_candidate_and_empty_shapes(kind):
    q, pos, neg, _ = gaussian_case(4, 3, 8, seed=6)
    pid, nid = torch.tensor([1, 9, 9, 2]), torch.tensor([9, 9, 9])  # n_b = 0 for queries 1, 2
    loss, dq, dpos, dneg = _loss_and_grads(q, pos, neg, kind, "none", pos_id=pid, neg_id=nid)
    assert torch.equal(loss[1:3], torch.zeros(2)) and bool((loss[[0, 3]] > 0).all())
    assert torch.equal(dq[1:3], torch.zeros(2, 8)) and torch.equal(dpos[1:3], torch.zeros(2, 8))
    # S = 0: every n_b is 0
    loss, dq, dpos, dneg = _loss_and_grads(q, pos, neg[:0], kind, "none")
    assert torch.equal(loss, torch.zeros(4)) and torch.equal(dq, torch.zeros(4, 8)) and dneg.shape == (0, 8)
    # B = 0: empty, or 0
    assert shared_loss(q[:0], pos[:0], neg, kind, "none").shape == (0,)
    for red in ("mean", "sum"):
        loss, dq, dpos, dneg = _loss_and_grads(q[:0], pos[:0], neg, kind, red)
        assert float(loss) == 0.0 and torch.equal(dneg, torch.zeros(3, 8))


@pytest.mark.parametrize("kind", KINDS)
def test_biases_shift_the_scores_and_get_no_gradient(kind):
    q, pos, neg, kw = gaussian_case(5, 6, 8, seed=7, bias=True)
    pb, nb = kw["pos_bias"].clone().requires_grad_(), kw["neg_bias"].clone().requires_grad_()
    got = shared_loss(q.requires_grad_(), pos, neg, kind, "none", pos_bias=pb, neg_bias=nb)
    got.sum().backward()
    assert pb.grad is None and nb.grad is None and q.grad is not None
    # the same scores from an extra column: q' = [q, 1], pos' = [pos, pos_bias], neg' = [neg, neg_bias]
    one = torch.ones(5, 1)
    want = shared_loss(torch.cat([q.detach(), one], 1), torch.cat([pos, pb.detach().unsqueeze(1)], 1),
                       torch.cat([neg, nb.detach().unsqueeze(1)], 1), kind, "none")
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    assert not torch.allclose(got, shared_loss(q.detach(), pos, neg, kind, "none"), rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("kind,scale", [(k, 0.35) for k in KINDS] + [("softmax", 3.2), ("bpr", 3.2)])
def test_fp32_restatement_is_inside_the_bound(kind, scale):
    """The torch-ops path in fp32 on the bf16-rounded Gaussian operands (scores of a few
    units; for softmax and bpr also of +-80, at scale 3.2) lies inside the derived bound
    without its bf16 term, and that bound is small.  (top1 at +-80 is left to the GPU suite,
    where the kernel is held to the bound: torch's sigmoid backward forms s (1 - s) in fp32,
    which cancels to 0 for x > 17 where the true sigmoid' is 4e-8 -- the restatement, not the
    bound, is off there; the kernel evaluates e / (1 + e)^2.)"""
    from pytorchrec_amd import cpu_path
    q, pos, neg, kw = gaussian_case(40, 150, 64, seed=8, ids=True, bias=True, scale=scale)
    up = torch.linspace(0.25, 1.5, 40)
    a, b, c = (t.detach().clone().requires_grad_() for t in (q, pos, neg))
    loss = cpu_path.shared_negative_loss(a, b, c, kind, "none", kw["pos_id"], kw["neg_id"], kw["pos_bias"],
                                         kw["neg_bias"], round_bf16=True)
    loss.backward(up)
    o = oracle(q, pos, neg, kind, "none", up.double(), coef_bf16=False, **kw)
    assert_within(loss, o["loss"], o["tol_loss"], f"{kind} loss")
    assert_within(a.grad, o["dq"], o["tol_dq"], f"{kind} dq")
    assert_within(b.grad, o["dpos"], o["tol_dpos"], f"{kind} dpos")
    assert_within(c.grad, o["dneg"], o["tol_dneg"], f"{kind} dneg")
    if scale < 1:  # not vacuous: worst-case fp32 terms only, below one bf16 rounding of the values
        assert float(o["tol_loss"].max()) < 1e-3 * (1 + float(o["loss"].abs().max()))
        assert float(o["tol_dq"].max()) < BF * float(o["dq"].abs().max())
        assert float(o["tol_dneg"].max()) < BF * float(o["dneg"].abs().max())


# ---------------------------------------------------------------------------
# the loss class, the registry, the library's argument checks
# ---------------------------------------------------------------------------

def test_loss_class_and_registry():
    from torch.nn.modules.loss import _Loss
    from pytorchrec_amd.loss import BPRLoss, SharedNegativeLoss, Top1Loss, get_loss
    for name, kind in (("softmax_shared", "softmax"), ("bpr_shared", "bpr"), ("top1_shared", "top1")):
        loss = get_loss(name)()
        assert isinstance(loss, SharedNegativeLoss) and isinstance(loss, _Loss)
        assert loss.kind == kind and loss.reduction == "mean"
        assert get_loss(name)(reduction="sum").reduction == "sum"
    assert get_loss("bpr") is BPRLoss and get_loss("top1") is Top1Loss  # unchanged
    with pytest.raises(ValueError):
        SharedNegativeLoss("hinge")
    with pytest.raises(ValueError):
        SharedNegativeLoss("bpr", reduction="max")
    q, pos, neg, kw = gaussian_case(5, 6, 8, seed=9, ids=True)
    loss = SharedNegativeLoss("softmax", "none")
    assert torch.equal(loss(q, pos, neg, **kw), shared_loss(q, pos, neg, "softmax", "none", **kw))
    with pytest.raises(ValueError, match="go together"):
        loss(q, pos, neg, pos_id=kw["pos_id"])
    with pytest.raises(ValueError):
        loss(q, pos[:4], neg)


def test_library_rejects_bad_arguments_before_any_device_work():
    """D outside the compiled set, ids on one side, a NULL operand: MREC_EINVAL from the host
    checks (no GPU is touched).  The accessors answer."""
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    assert lib.mrec_shneg_tile_queries() >= 1 and lib.mrec_shneg_tile_candidates() >= 1
    assert all(lib.mrec_shneg_supported(d, _mrec.F32, _mrec.BF16) for d in (8, 16, 32, 64))
    assert not any(lib.mrec_shneg_supported(d, _mrec.F32, _mrec.BF16) for d in (0, 4, 12, 24, 48, 128))
    assert not lib.mrec_shneg_supported(64, _mrec.I32, _mrec.BF16)
    assert lib.mrec_shneg_splits(0, 100) == 1 and 1 <= lib.mrec_shneg_splits(4096, 64) <= 64
    assert lib.mrec_shneg_workspace_size(100, 50, 64, 1) >= 400
    buf = (ctypes.c_float * 4096)()
    addr = (ctypes.addressof(buf) + 15) // 16 * 16

    def args(**kw):
        a = _mrec.ShnegArgs()
        a.q = a.pos = a.neg = addr
        a.q_dtype = a.row_dtype = _mrec.F32
        a.ldq = a.ld_pos = a.ld_neg = 64
        a.batch, a.n_neg, a.D = 4, 4, 64
        a.loss = a.stats = addr
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for a, word in ((args(D=48), b"unsupported"), (args(pos_id=addr), b"go together"),
                    (args(q=None), b"aligned"), (args(kind=7), b"kind"), (args(splits=65), b"splits"),
                    (args(ldq=63), b"aligned"), (args(reduction=_mrec.REDUCE_MEAN), b"workspace")):
        assert lib.mrec_shneg_loss_fwd(ctypes.byref(a), None) == _mrec.EINVAL
        assert word in lib.mrec_last_error(), lib.mrec_last_error()
    assert lib.mrec_shneg_loss_bwd(ctypes.byref(args()), None) == _mrec.EINVAL  # (no g)
    assert lib.mrec_shneg_loss_fwd(ctypes.byref(args(batch=0)), None) == _mrec.OK   # nothing to do


# ---------------------------------------------------------------------------
# the model layer
# ---------------------------------------------------------------------------

MODELS = {"funksvd": lambda: funk(users=160, items=61),
          "sasrec": lambda: sasrec(items=61, max_his_len=8),
          "gru4rec": lambda: gru4rec(items=61, max_his_len=8)}


def _train_data():
    train, _, pairs = planted_sequences()
    return {k: torch.from_numpy(v) for k, v in train.items()}, pairs


def _sampler(pairs, seed=3):
    from pytorchrec_amd.sampling import NegativeSampler
    return NegativeSampler(pairs[0], pairs[1], 1, 61, seed=seed)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("source", ["sampler", "in_batch"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_train_steps_reduce_the_loss(model, source, kind):
    from pytorchrec_amd.loss import SharedNegativeLoss
    data, pairs = _train_data()
    m = MODELS[model]()
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), SharedNegativeLoss(kind), [], torch.device("cpu"))
    if source == "sampler":
        m.set_shared_negatives(_sampler(pairs), 16)
    else:
        m.set_shared_negatives("in_batch")
    losses = [float(m.train_step(data)["loss"].detach()) for _ in range(12)]
    assert np.isfinite(losses).all() and min(losses[-3:]) < losses[0], losses


def test_pool_is_reproducible_from_seed_and_step():
    data, pairs = _train_data()
    a, b, c = MODELS["funksvd"](), MODELS["funksvd"](), MODELS["funksvd"]()
    a.set_shared_negatives(_sampler(pairs, 3), 32)
    b.set_shared_negatives(_sampler(pairs, 3), 32)
    c.set_shared_negatives(_sampler(pairs, 4), 32)
    p0, p1 = a.shared_negative_pool(0), a.shared_negative_pool(1)
    assert p0.shape == (32,) and int(p0.min()) >= 1 and int(p0.max()) < 61
    assert torch.equal(p0, b.shared_negative_pool(0)) and torch.equal(p1, b.shared_negative_pool(1))
    assert not torch.equal(p0, p1) and not torch.equal(p0, c.shared_negative_pool(0))
    a.set_shared_negatives("in_batch")
    assert a.shared_negative_pool(0) is None


@pytest.mark.parametrize("source", ["sampler", "in_batch"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_one_gather_per_bank_per_step(model, source, monkeypatch):
    from pytorchrec_amd import embedding
    from pytorchrec_amd.loss import SharedNegativeLoss
    data, pairs = _train_data()
    m = MODELS[model]()
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.1), SharedNegativeLoss("softmax"), [], torch.device("cpu"))
    m.set_shared_negatives(_sampler(pairs), 16) if source == "sampler" else m.set_shared_negatives("in_batch")
    calls = []
    mod = sys.modules[type(m).__module__]

    def spy(bank, ids, *a, **kw):
        calls.append((bank, [int(t.shape[0]) for t in ids]))
        return embedding.gather(bank, ids, *a, **kw)

    monkeypatch.setattr(mod, "gather", spy)
    m.train_step(data)
    B, S = 160, 16 if source == "sampler" else 0
    assert len(calls) == len(m.embedding_banks()) == 1, calls
    want = B + S if model == "funksvd" else B * 8 + B + S
    assert all(n == want for n in calls[0][1]), (calls, want)
    m.train_step(data)
    assert len(calls) == 2


def test_models_without_a_dot_product_score_raise():
    from test_ncf_cpu import ncf
    from test_pool_cpu import svdpp
    for m in (svdpp(), ncf()):
        with pytest.raises(NotImplementedError):
            m.set_shared_negatives("in_batch")
        m.set_shared_negatives(None)  # turning it off is always fine
        assert type(m).set_shared_negatives.__doc__ and "Not available" in type(m).set_shared_negatives.__doc__


def test_shared_negatives_exclude_the_row_sampler_and_need_a_shared_loss():
    from pytorchrec_amd.loss import BPRLoss, SharedNegativeLoss
    data, pairs = _train_data()
    m = MODELS["funksvd"]()
    m.set_negative_sampler(_sampler(pairs), n_neg=2)
    with pytest.raises(ValueError, match="exclude each other"):
        m.set_shared_negatives("in_batch")
    m.set_negative_sampler(None)
    m.set_shared_negatives("in_batch")
    with pytest.raises(ValueError, match="exclude each other"):
        m.set_negative_sampler(_sampler(pairs), n_neg=2)
    for bad in ({"source": "everything"}, {"source": _sampler(pairs)}, {"source": _sampler(pairs), "n_shared": 0},
                {"source": "in_batch", "n_shared": 4}):
        with pytest.raises(ValueError):
            m.set_shared_negatives(**bad)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.1), BPRLoss(), [], torch.device("cpu"))
    with pytest.raises(ValueError, match="SharedNegativeLoss"):
        m.train_step(data)
    m.set_shared_negatives(None)  # off: the compiled pairwise loss trains as before
    m.set_negative_sampler(_sampler(pairs), n_neg=1)
    assert np.isfinite(float(m.train_step(data)["loss"].detach()))
    m.set_negative_sampler(None)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.1), SharedNegativeLoss("bpr"), [], torch.device("cpu"))
    m.set_shared_negatives(_sampler(pairs), 8)
    assert np.isfinite(float(m.train_step(data)["loss"].detach()))


def test_fit_pair_wise_accepts_shared_negatives():
    from pytorchrec_amd.loss import SharedNegativeLoss

    class Rows(torch.utils.data.Dataset):
        def __init__(self, cols):
            self.cols = cols

        def __len__(self):
            return 160

        def __getitem__(self, i):
            return {k: v[i] for k, v in self.cols.items()}

    data, pairs = _train_data()
    m = MODELS["gru4rec"]()
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), SharedNegativeLoss("softmax"), [], torch.device("cpu"))
    with pytest.raises(ValueError, match="needs negatives"):
        m.fit(Rows(data), 80, 1, train_mode="pair_wise", verbose=0)
    m.set_shared_negatives(_sampler(pairs), 16)
    hist = m.fit(Rows(data), 80, 3, train_mode="pair_wise", verbose=0, shuffle=False)
    assert len(hist) == 3 and all(np.isfinite(h["loss"]) for h in hist)
