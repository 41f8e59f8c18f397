"""mrec_graph_prop (csrc/graph_prop.hip) and LightGCN on the GPU, against exact integer
expectations and against a dense fp64 reference under a derived element-wise bound."""
import pytest
import torch

from pytorchrec_amd import graph
from pytorchrec_amd.loss import BPRLoss
from test_lightgcn_cpu import (bound, bpr_step_fp64, dense_ahat, dense_propagate, interactions,
                               make_model, skew_graph)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
N_USERS, N_ITEMS = 24, 24
USERS_WITHOUT_TIES = (10, 11, 14, 15)  # of the model fixture's seeds: asserted where it is used


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("D", [8, 16, 32, 64])
@pytest.mark.parametrize("a, b", [(16, 4), (64, 16), (4 * graph.LONG_ROW, 4)])
def test_complete_bipartite_is_exact(gpu, a, b, D, K):
    """K(a, b) with square degrees: every edge weight 1/sqrt(a b) is a power of two and the
    inputs are small integers, so every partial sum is exact in any order.  Odd layers are
    S_other / sqrt(a b), even ones S_own / own count, S the integer column sums of a side."""
    r = int(round((a * b) ** 0.5))
    assert r * r == a * b and r & (r - 1) == 0
    u, i = torch.arange(a).repeat_interleave(b), torch.arange(b).repeat(a)
    g = graph.BipartiteGraph.from_interactions(u, i, a, b, device=gpu)
    gen = torch.Generator().manual_seed(a + D + K)
    x = torch.full((a + b, D + 8), 7.0)  # a bank-like table: 8 pad columns of junk
    x[:, :D] = torch.randint(-4, 5, (a + b, D), generator=gen).float()
    Su, Si = x[:a, :D].double().sum(0), x[a:, :D].double().sum(0)
    total = x[:, :D].double().clone()
    for k in range(1, K + 1):
        total[:a] += (Si / r) if k % 2 else (Su / a)
        total[a:] += (Su / r) if k % 2 else (Si / b)
    want = total.float() / (K + 1)
    y = graph.propagate(g, x.to(gpu), K, dim=D).cpu()
    assert torch.equal(y[:, :D], want)
    assert y.shape == x.shape and not y[:, D:].any()


@pytest.fixture(scope="module")
def skew(gpu):
    u, i, nu, ni = skew_graph()
    g = graph.BipartiteGraph.from_interactions(u, i, nu, ni, device=gpu)
    gen = torch.Generator().manual_seed(3)
    x, dy = torch.randn(nu + ni, 64, generator=gen), torch.randn(nu + ni, 64, generator=gen)
    return g, dense_ahat(u, i, nu, ni), x, dy


@pytest.mark.parametrize("layer", [None, BF16])
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("D", [8, 16, 32, 64])
def test_forward_and_gradient_against_fp64(gpu, skew, D, K, layer):
    g, Ah, x, dy = skew
    x, dy = x[:, :D].contiguous(), dy[:, :D].contiguous()
    xg = x.to(gpu).requires_grad_()
    y = graph.propagate(g, xg, K, layer)
    y.backward(dy.to(gpu))
    for got, src in ((y.detach(), x), (xg.grad, dy)):
        err = (got.cpu().double() - dense_propagate(Ah, src.double(), K)).abs()
        tol = bound(Ah, src, K, g.max_deg, layer is BF16)
        print(f"D={D} K={K} {layer}: max err/bound {float((err / tol).max()):.3g}")
        assert (err <= tol).all()
    # equal inputs, equal bits; and the torch-op path meets the same bound
    x2 = x.to(gpu).requires_grad_()
    y2 = graph.propagate(g, x2, K, layer)
    y2.backward(dy.to(gpu))
    assert torch.equal(y2, y) and torch.equal(x2.grad, xg.grad)


def test_unfused_path_meets_the_same_bound(gpu, skew, monkeypatch):
    g, Ah, x, _ = skew
    monkeypatch.setattr(graph, "PROP_FUSED", False)
    y = graph.propagate(g, x.to(gpu), 3)
    err = (y.cpu().double() - dense_propagate(Ah, x.double(), 3)).abs()
    assert (err <= bound(Ah, x, 3, g.max_deg)).all()


def test_unsupported_shapes_and_empty_graph(gpu, skew):
    from pytorchrec_amd import _mrec
    g, Ah, x, _ = skew
    assert not graph.fused_supported(x[:, :24].contiguous().to(gpu), 24, 3)
    assert not graph.fused_supported(x.to(gpu), 64, 5)
    y = graph.propagate(g, x[:, :24].contiguous().to(gpu), 2)  # the contract in torch ops
    err = (y.cpu().double() - dense_propagate(Ah, x[:, :24].double(), 2)).abs()
    assert (err <= bound(Ah, x[:, :24], 2, g.max_deg)).all()
    a = _mrec.GraphPropArgs(n_rows=4, dim=24)
    assert _mrec.lib().mrec_graph_prop(a, None) == _mrec.EINVAL
    a = _mrec.GraphPropArgs(n_rows=0, dim=64)
    assert _mrec.lib().mrec_graph_prop(a, None) == _mrec.OK
    e = graph.BipartiteGraph.from_interactions([], [], 0, 0, device=gpu)
    assert graph.propagate(e, torch.zeros(0, 8, device=gpu), 2).shape == (0, 8)


@pytest.fixture()
def model(gpu):
    m = make_model(N_USERS, N_ITEMS, D=8, K=3)
    with torch.no_grad():
        m.embeddings.weight.mul_(40)  # scores of order 1
    u, i = interactions(N_USERS, N_ITEMS, 80, seed=19)
    m.set_graph(u, i)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.5), BPRLoss(), [], gpu)
    return m, dense_ahat(u, i, N_USERS, N_ITEMS)


@pytest.mark.parametrize("fused", [True, False])
def test_bpr_sgd_step_against_fp64(gpu, model, fused, monkeypatch):
    """new E0 = E0 - lr P(dE), P the propagation and dE = c E[other] / B per pair, c =
    sigmoid(neg - pos) <= 1.  With eps = 2^-23 (max_deg + 8) (K + 1), Pabs = P(|E0|) >= |E|
    and dEabs the same dE built from Pabs with c = 1 (so |dE| <= dEabs):
      * the backward launches err by at most eps P(|dE|) <= eps P(dEabs);
      * the forward leaves |dE| off by eps dEabs through E[other] (|err E| <= eps Pabs), and by
        at most eps smax dEabs through c: a score is off by 2 eps sum_d Pabs_u Pabs_i <= 2 eps
        smax, c has slope <= 1/4 in each of its two scores; doubled for the fp32 dot products.
    In all lr eps (2 + 2 smax) P(dEabs), plus one rounding of the weights."""
    m, Ah = model
    monkeypatch.setattr(graph, "PROP_FUSED", fused)
    gen = torch.Generator().manual_seed(4)
    B, lr, K = 16, 0.5, 3
    uid = torch.randint(0, N_USERS, (B,), generator=gen)
    iid = torch.randint(0, N_ITEMS, (B, 2), generator=gen)
    before = m.embeddings.weight.detach().cpu().clone()
    loss = float(m.train_step({"uid": uid, "iid": iid})["loss"].detach())
    want, want_loss = bpr_step_fp64(before, Ah, K, uid, iid, lr, N_USERS)
    Pabs = dense_propagate(Ah, before.abs().double(), K)
    pu, pi = Pabs[uid][:, None].expand(B, 2, 8), Pabs[N_USERS + iid]
    smax = float((pu * pi).sum(-1).max())
    dEabs = torch.zeros_like(Pabs).index_add_(0, uid, pi.sum(1) / B)
    dEabs.index_add_(0, (N_USERS + iid).reshape(-1), pu.reshape(-1, 8) / B)
    eps = 2.0 ** -23 * (m.graph.max_deg + 8) * (K + 1)
    tol = lr * eps * (2 + 2 * smax) * dense_propagate(Ah, dEabs, K) + 2.0 ** -23 * before.abs()
    err = (m.embeddings.weight.detach().cpu().double() - want).abs()
    print(f"fused={fused}: loss {loss:.6f} / {want_loss:.6f}, max err/tol {float((err / tol).max()):.3g}")
    assert abs(loss - want_loss) <= 2 * eps * smax + 1e-6 and (want - before).abs().max() > 1e-3
    assert (err <= tol).all()


def test_forward_branches_and_recommend(gpu, model):
    m, Ah = model
    E = dense_propagate(Ah, m.embeddings.weight.detach().cpu().double(), 3)
    S = E[:N_USERS] @ E[N_USERS:].t()  # the contract's scores
    gen = torch.Generator().manual_seed(6)
    uid = torch.randint(0, N_USERS, (12,), generator=gen)
    cand = torch.randint(0, N_ITEMS, (12, 5), generator=gen)
    tolE = bound(Ah, m.embeddings.weight.detach().cpu(), 3, m.graph.max_deg)
    Eu, Ei, tu, ti = E[uid][:, None], E[N_USERS + cand], tolE[uid][:, None], tolE[N_USERS + cand]
    # (the fused score is the 2-field FM, ((u + i)^2 - u^2 - i^2) / 2 summed in fp32)
    tol = (Eu.abs() * ti + Ei.abs() * tu + 2.0 ** -23 * 16 * (Eu.abs() + Ei.abs()) ** 2).sum(-1)
    m.eval()
    with torch.no_grad():
        p5, _ = m({"uid": uid.to(gpu), "iid": cand.to(gpu)})
        p1, _ = m({"uid": uid.to(gpu), "iid": cand[:, 0].contiguous().to(gpu)})
    assert ((p5.cpu().double() - S[uid[:, None], cand]).abs() <= tol).all()
    assert ((p1.cpu().double() - S[uid, cand[:, 0]]).abs() <= tol[:, 0]).all()
    # recommend scores bf16 operands (mrec_topk): two roundings of 2^-8 per product; two
    # scores keep their order when they differ by more than twice that
    users = torch.tensor(USERS_WITHOUT_TIES)
    top = torch.sort(S[users], dim=1, descending=True)
    absS = E[users].abs() @ E[N_USERS:].abs().t()
    gap_tol = 2 * (2 * 2.0 ** -8 + 2.0 ** -16) * absS.max(1).values
    gaps = top.values[:, :10] - top.values[:, 1:11]
    assert (gaps > gap_tol[:, None]).all(), "precondition: no ties within the tolerance"
    ids, _ = m.recommend({"uid": users.to(gpu)}, 10)
    assert torch.equal(ids.cpu().long(), top.indices[:, :10])

