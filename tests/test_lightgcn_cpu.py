"""LightGCN without a GPU: the graph builder, the propagation contract
(``cpu_path.graph_propagate``) and the model, each against a deliberately naive reference:
a dense N x N normalised adjacency in fp64 and K matmuls."""
import pytest
import torch

from pytorchrec_amd import cpu_path, graph
from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
from pytorchrec_amd.loss import BPRLoss
from pytorchrec_amd.model import FunkSVD, LightGCN


def dense_ahat(u, i, n_users, n_items):
    N = n_users + n_items
    A = torch.zeros(N, N, dtype=torch.float64)
    A[u, n_users + i] = 1
    A[n_users + i, u] = 1
    deg = A.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    return dinv[:, None] * A * dinv[None, :]


def dense_propagate(Ah, x, K):
    total, y = x.clone(), x
    for _ in range(K):
        y = Ah @ y
        total = total + y
    return total / (K + 1)


def bound(Ah, x, K, max_deg, bf16=False):
    """|y - y64| <= 2^-23 (max_deg + 8) (K + 1) P, P the same propagation of |x| (A^ is
    non-negative, so P bounds every partial sum); bf16 layers add K 2^-8 P."""
    P = dense_propagate(Ah, x.abs().double(), K)
    return (2.0 ** -23 * (max_deg + 8) * (K + 1) + (K * 2.0 ** -8 if bf16 else 0.0)) * P


def skew_graph():
    """A seeded graph of forced row lengths at every gather-step and segment edge, plus
    random users: -> (u, i, n_users, n_items)."""
    L = graph.LONG_ROW
    forced = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, L - 1, L, L + 1, 2 * L + 3]
    gen = torch.Generator().manual_seed(11)
    n_items, n_users = 2 * L + 40, len(forced) + 40
    us, its = [], []
    for u, d in enumerate(forced + [8] * 40):
        it = torch.randperm(n_items, generator=gen)[:d]
        us.append(torch.full((d,), u, dtype=torch.int64))
        its.append(it)
    return torch.cat(us), torch.cat(its), n_users, n_items


def test_from_interactions():
    u = torch.tensor([0, 0, 1, 2, 0, 2])
    i = torch.tensor([1, 1, 0, 1, 2, 0])  # (0, 1) twice; user 3 and item 3 isolated
    g = graph.BipartiteGraph.from_interactions(u, i, 4, 4)
    assert g.n_edges == 5 and g.n_nodes == 8
    assert g.row_ptr.dtype == torch.int64 and g.col.dtype == torch.int32 and g.dinv.dtype == torch.float32
    deg = g.row_ptr[1:] - g.row_ptr[:-1]
    assert deg.tolist() == [2, 1, 2, 0, 2, 2, 1, 0]
    A = torch.zeros(8, 8)
    A[g.edge_rows(), g.col.long()] = 1
    assert torch.equal(A, A.t()) and torch.equal(A.double(), (dense_ahat(u, i, 4, 4) > 0).double())
    for r in range(8):
        row = g.col[g.row_ptr[r]:g.row_ptr[r + 1]].tolist()
        assert row == sorted(row)
    want = torch.where(deg > 0, deg.double().rsqrt(), torch.zeros(8, dtype=torch.float64)).float()
    assert torch.equal(g.dinv, want) and g.dinv[3] == 0 and g.dinv[7] == 0
    # every row is covered once by the work list; an isolated row has length 0
    assert sorted(g.work[:, 0].tolist()) == list(range(8)) and g.n_slots == 0


@pytest.mark.parametrize("u, i", [([4], [0]), ([-1], [0]), ([0], [4]), ([0], [-1])])
def test_out_of_range_ids_raise(u, i):
    with pytest.raises(IndexError):
        graph.BipartiteGraph.from_interactions(torch.tensor(u), torch.tensor(i), 4, 4)


def test_long_rows_are_cut_into_segments():
    u, i, nu, ni = skew_graph()
    g = graph.BipartiteGraph.from_interactions(u, i, nu, ni)
    L = graph.LONG_ROW
    assert g.max_deg == 2 * L + 3 and g.n_slots == 2 + 3 and g.long_ptr.tolist() == [0, 2, 5]
    seg = g.work[:g.n_slots]
    assert seg[:, 1].tolist() == [L, 1, L, L, 3] and seg[:, 2].tolist() == list(range(5))
    assert torch.equal(g.work_beg[:g.n_slots] - g.row_ptr[seg[:, 0].long()],
                       torch.tensor([0, L, 0, L, 2 * L]))
    assert int(g.work[:, 1].sum()) == 2 * g.n_edges and (g.work[g.n_slots:, 2] == -1).all()


@pytest.mark.parametrize("K", [0, 1, 3])
def test_contract_and_gradient_equal_dense_fp64(K):
    u, i, nu, ni = skew_graph()
    g = graph.BipartiteGraph.from_interactions(u, i, nu, ni)
    Ah = dense_ahat(u, i, nu, ni)
    gen = torch.Generator().manual_seed(K)
    x = torch.randn(nu + ni, 12, dtype=torch.float64, generator=gen).requires_grad_()
    dy = torch.randn(nu + ni, 12, dtype=torch.float64, generator=gen)
    y = cpu_path.graph_propagate(g, x, K)
    # fp64 sums, but dinv is the graph's fp32 one: two roundings per edge weight and layer,
    # inside the "+ 8" of the bound with no degree term at all
    assert ((y - dense_propagate(Ah, x.detach(), K)).abs() <= bound(Ah, x.detach(), K, 0)).all()
    z = graph.propagate(g, x, K, dim=8)  # 8 live columns: the rest come out zero
    torch.testing.assert_close(z[:, :8], y[:, :8].detach(), rtol=0, atol=0)
    assert not z[:, 8:].any()
    z.backward(dy)
    want = dense_propagate(Ah, dy[:, :8], K)  # A^ is symmetric
    assert ((x.grad[:, :8] - want).abs() <= bound(Ah, dy[:, :8], K, 0)).all()
    assert not x.grad[:, 8:].any()


@pytest.mark.parametrize("bf16", [False, True])
def test_fp32_contract_stays_inside_the_derived_bound(bf16):
    """The bound the GPU tests hold the kernel to, checked on the torch-op contract first."""
    u, i, nu, ni = skew_graph()
    g = graph.BipartiteGraph.from_interactions(u, i, nu, ni)
    Ah = dense_ahat(u, i, nu, ni)
    x = torch.randn(nu + ni, 64, generator=torch.Generator().manual_seed(3))
    for K in (1, 3, 4):
        y = cpu_path.graph_propagate(g, x, K, torch.bfloat16 if bf16 else None).double()
        err = (y - dense_propagate(Ah, x.double(), K)).abs()
        assert (err <= bound(Ah, x, K, g.max_deg, bf16)).all()


def make_model(n_users=9, n_items=14, D=8, K=2, cls=LightGCN, **kw):
    cols = [CategoricalColumnWithIdentity(n_users, "uid"), CategoricalColumnWithIdentity(n_items, "iid")]
    if cls is LightGCN:
        kw.setdefault("n_layers", K)
    return cls(cols[0], cols[1], None, D, random_seed=5, **kw)


def interactions(n_users, n_items, n, seed=2):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(0, n_users, (n,), generator=gen), torch.randint(0, n_items, (n,), generator=gen))


def bpr_step_fp64(E0, Ah, K, uid, iid, lr, n_users):
    """One BPR + SGD step written with dense fp64 ops -> the updated E0."""
    E0 = E0.double().requires_grad_()
    E = dense_propagate(Ah, E0, K)
    s = (E[uid][:, None, :] * E[n_users + iid]).sum(-1)
    loss = torch.nn.functional.softplus(s[:, 1] - s[:, 0]).mean()
    loss.backward()
    return (E0 - lr * E0.grad).detach(), float(loss.detach())


def test_model_state_dict_graph_and_step():
    m = make_model()
    f = make_model(cls=FunkSVD)
    assert sorted(m.state_dict()) == sorted(f.state_dict()) == ["i_embeddings.weight", "u_embeddings.weight"]
    assert [n for n, _ in m.named_parameters()] == ["embeddings.weight"] and len(m.embedding_banks()) == 1
    with torch.no_grad():
        f.embeddings.weight.mul_(30)  # scores of order 1
    m.load_state_dict(f.state_dict())
    assert torch.equal(m.embeddings.weight, f.embeddings.weight)
    data = {"uid": torch.tensor([0, 3, 8, 3]), "iid": torch.tensor([[1, 2], [0, 13], [5, 1], [7, 7]])}
    with pytest.raises(RuntimeError):
        m(data)
    u, i = interactions(9, 14, 40)
    m.set_graph(u, i)
    m.compile(torch.optim.SGD(m.get_parameters(), lr=0.5), BPRLoss(), [], torch.device("cpu"))
    before = m.embeddings.weight.detach().clone()
    loss = float(m.train_step(data)["loss"].detach())
    want, want_loss = bpr_step_fp64(before, dense_ahat(u, i, 9, 14), 2, data["uid"], data["iid"], 0.5, 9)
    assert abs(loss - want_loss) < 1e-6
    assert (want - before.double()).abs().max() > 1e-3  # the step moved the table
    torch.testing.assert_close(m.embeddings.weight.detach().double(), want, rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        make_model(emb_dtype=torch.bfloat16)


def test_eval_cache_is_invalidated():
    m = make_model()
    m.set_graph(*interactions(9, 14, 40))
    m.eval()
    t1 = m.propagated_table()
    assert m.propagated_table() is t1 and not t1.requires_grad
    m.train()
    assert m.propagated_table().requires_grad
    m.eval()
    t2 = m.propagated_table()
    assert t2 is not t1 and torch.equal(t2, t1)
    sd = {k: v * 2 for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    t3 = m.propagated_table()
    assert t3 is not t2 and torch.equal(t3, t2 * 2)
    m.set_graph(*interactions(9, 14, 40, seed=3))
    assert not torch.equal(m.propagated_table(), t3)
