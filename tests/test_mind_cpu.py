"""MIND on the CPU path (no GPU): ``cpu_path.mind_route`` against a plain fp64 restatement of
the contract, the gradient stop, a state_dict round trip, ``recommend`` and ``forward``
against brute force, and the registry.

Tolerance of the fp32 path against fp64: |got - want| <= 1e-5 max|want| per quantity (fp32
rounding 6e-8 per operation over the few hundred operations of a routing, as in
test_sasrec_cpu.py).
"""
import functools

import pytest
import torch

CPU_SHAPES = [(5, 1, 16, 1, 1, False), (7, 12, 32, 3, 3, False), (9, 20, 16, 8, 2, True)]


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def mind(items=50, emb_size=16, max_his_len=12, num_interests=3, routing_iters=3, dynamic_k=False,
         interest_pow=0.0, seed=2020, device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import MIND
    return MIND(CategoricalColumnWithIdentity(items, "iid"),
                CategoricalColumnWithIdentity(max_his_len + 1, "his_len"),
                CategoricalColumnWithIdentity(items, "his"),
                CategoricalColumnWithIdentity(2, "label"), emb_size=emb_size,
                max_his_len=max_his_len, num_interests=num_interests, routing_iters=routing_iters,
                dynamic_k=dynamic_k, interest_pow=interest_pow, random_seed=seed, device=device, **kw)


def active(lens, K, dyn):
    return torch.tensor([max(1, min(K, int(n).bit_length() - 1)) if dyn else K for n in lens.tolist()])


@functools.lru_cache(maxsize=None)
def case(B, L, D, K, R, dyn=False, device="cpu"):
    """(model, rows bf16 [B, L, D], his, his_len, dU).  Sample 0 has length 1, sample 1
    length L, sample 2 is the forced-valid PAD row (his[2, 0] == 0), samples 3.. lengths 2,
    4, 8, 16, 32 as far as L and B allow (with ``dyn``: every K' up to log2 L); the rest
    random lengths, tail-padded with 0.  Rows 0.3 N(0, 1) and route_weight at its initial
    scale: the logits stay O(1)."""
    dev = torch.device(device)
    g = torch.Generator().manual_seed(100 + L)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    for i, n in enumerate((1, L, 1, 2, 4, 8, 16, 32)):
        if i < B and n <= L:
            lens[i] = n
    his = torch.randint(1, 50, (B, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    if B > 2:
        his[2] = 0
    m = mind(emb_size=D, max_his_len=L, num_interests=K, routing_iters=R, dynamic_k=dyn, device=dev)
    rows = (0.3 * torch.randn(B, L, D, generator=g)).to(torch.bfloat16).to(dev)
    dU = torch.randn(B, K, D, generator=g).to(dev)
    return m, rows, his.to(dev), lens.to(dev), dU


def restate(x, his, lens, S, init, R, dyn, w_last=None):
    """The contract in plain fp64 torch -> (U, the last w).  With ``w_last`` only the last
    iteration runs, on that coupling as a constant."""
    (B, L, D), K = x.shape, init.shape[0]
    valid = his > 0
    valid[:, 0] = True
    on = torch.arange(K)[None, :, None] < active(lens, K, dyn)[:, None, None]
    h = x @ S.T
    hd = h.detach()
    b = init[:, :L].expand(B, K, L)
    for r in range(R):
        last = r == R - 1
        w = torch.softmax(b.masked_fill(~on, float("-inf")), dim=1)
        w = torch.where(on & valid[:, None, :], w, torch.zeros((), dtype=x.dtype)).detach()
        if w_last is not None:
            w, last = w_last, True
        z = w @ (h if last else hd)
        n2 = (z * z).sum(-1, keepdim=True)
        u = z * n2 / ((1 + n2) * (n2 + 1e-9).sqrt())
        if last:
            return u, w
        b = b + u.detach() @ hd.transpose(1, 2)


@functools.lru_cache(maxsize=None)
def ref64(B, L, D, K, R, dyn=False, device="cpu", last_only=False):
    """fp64 restatement and its gradients, rounding nothing (computed once) -> {U, dX, dS}."""
    m, rows, his, lens, dU = case(B, L, D, K, R, dyn, device)
    x = rows.detach().double().cpu().requires_grad_()
    S = m.route_weight.detach().double().cpu().requires_grad_()
    args = (his.cpu(), lens.cpu(), S, m.route_init.double().cpu(), R, dyn)
    w = restate(x, *args)[1] if last_only else None
    U, _ = restate(x, *args, w_last=w)
    U.backward(dU.double().cpu())
    return {"U": U.detach(), "dX": x.grad, "dS": S.grad}


def run(c, rows=None):
    """One forward + backward of dense.mind_route -> ({U, dX, dS}, U.grad_fn)."""
    from pytorchrec_amd import dense
    m, rows0, his, lens, dU = c
    m.route_weight.grad = None
    x = (rows0 if rows is None else rows).detach().clone().requires_grad_()
    U = dense.mind_route(x, his, lens, m)
    U.backward(dU)
    return {"U": U.detach(), "dX": x.grad, "dS": m.route_weight.grad.clone()}, U.grad_fn


def errs(got, want):
    """(max, mean) |got - want| relative to max |want|."""
    d = (got.detach().double().cpu() - want.double()).abs()
    mag = max(want.abs().max().item(), 1e-12)
    return d.max().item() / mag, d.mean().item() / mag


def batch(device="cpu", B=32, L=12, N=5, items=50):
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    his = torch.randint(1, items, (B, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    return {"iid": torch.randint(1, items, (B, N), generator=g).to(device), "his": his.to(device),
            "his_len": lens.to(device), "label": (torch.rand(B, N, generator=g) < 0.3).long().to(device)}


def brute_scores(m, data, bf16=False):
    """max over the active interests of U_bk . T_i for every item [B, items], id 0 out."""
    U = m._encode_history(data).detach()
    T = m.i_embeddings.table(0)[:, :m.emb_size].detach()
    if bf16:  # (retrieval.topk scores bf16(q) . bf16(T[i]) on a GPU)
        U, T = U.bfloat16(), T.bfloat16()
    s = torch.einsum("bkd,id->bki", U.double(), T.double())
    s = s.masked_fill(~m._active(data["his_len"]).unsqueeze(-1), float("-inf")).max(dim=1).values
    s[:, 0] = float("-inf")  # id 0 is the padding item (retrieval_low)
    return s


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,L,D,K,R,dyn", CPU_SHAPES)
def test_cpu_path_matches_fp64(B, L, D, K, R, dyn):
    ref = ref64(B, L, D, K, R, dyn)
    c = case(B, L, D, K, R, dyn)
    got, _ = run(c, rows=c[1].float())  # (an fp32 leaf: its gradient is not rounded to bf16)
    kp = active(c[3], K, dyn)
    if dyn:
        assert set(kp.tolist()) == {1, 2, 3, 4}
    off = torch.arange(K)[None, :] >= kp[:, None]
    assert (got["U"][off] == 0).all() and (ref["U"][off] == 0).all()
    # no two active interests of a sample tie
    gap = torch.cdist(ref["U"], ref["U"]) + 1e3 * (torch.eye(K) + off[:, :, None] + off[:, None, :])
    assert gap.min() > 1e-3
    for name, want in ref.items():
        assert torch.isfinite(want).all(), name
        emax, _ = errs(got[name], want)
        print(f"{name}: max error {emax:.2e} of magnitude {want.abs().max().item():.2e}")
        assert emax <= 1e-5, (name, emax)


def test_gradient_stops_at_the_routing_logits():
    """d route_weight of the contract is the last iteration's alone, its w a constant."""
    shape = (7, 12, 32, 3, 3, False)
    c = case(*shape)
    got, _ = run(c, rows=c[1].float())
    want = ref64(*shape, last_only=True)
    assert errs(got["dS"], want["dS"])[0] <= 1e-5 and errs(got["dX"], want["dX"])[0] <= 1e-5


def test_state_dict_round_trip_reproduces_forward():
    m = mind(emb_size=24, seed=1)  # (the bank pitches 24 -> 32 columns)
    sd = m.state_dict()
    assert set(sd) == {"i_embeddings.weight", "route_weight", "route_init"}
    assert tuple(sd["i_embeddings.weight"].shape) == (50, 24)
    other = mind(emb_size=24, seed=2)
    assert not torch.equal(other.route_init, m.route_init)
    other.load_state_dict(sd)
    data = batch()
    with torch.no_grad():
        a, b = m.eval()(data)[0], other.eval()(data)[0]
    assert a.shape == (32, 5) and torch.equal(a, b)


@pytest.mark.parametrize("exclude", [False, True])
def test_recommend_is_the_brute_force_top_k(exclude):
    from pytorchrec_amd import retrieval
    m = mind(dynamic_k=True).eval()
    with torch.no_grad():
        m.i_embeddings.weight.mul_(30.0)  # lively scores: N(0, 0.3) rows
    data = batch()
    s = brute_scores(m, data)
    ex = None
    if exclude:
        ex = retrieval.Exclusion.from_lists(data["his"], pad=0)
        s.scatter_(1, data["his"].long(), float("-inf"))  # (id 0 is out already)
    ids, scores = m.recommend(data, 7, exclude=ex)
    assert torch.equal(ids.long(), s.topk(7, dim=1).indices)
    assert torch.allclose(scores.double(), s.topk(7, dim=1).values, rtol=1e-5, atol=1e-6)


def test_forward_scores_the_best_active_interest():
    m = mind(dynamic_k=True).eval()
    data = batch()
    with torch.no_grad():
        pred, target = m(data)
    want = brute_scores(m, data).gather(1, data["iid"])
    assert target.shape == (32, 5) and torch.allclose(pred.double(), want, rtol=1e-5, atol=1e-9)


def test_registry_answers_mind():
    from pytorchrec_amd.model import MIND, get_model_type, model_name_list
    assert get_model_type("mind") is MIND and "mind" in model_name_list
    names = [a.name for a in MIND.get_argument_descriptions()]
    assert names == ["emb_size", "max_his_len", "num_interests", "routing_iters", "dynamic_k",
                     "interest_pow"]
