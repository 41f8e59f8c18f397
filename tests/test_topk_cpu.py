"""Full-catalogue top-K retrieval on the CPU (no GPU): ``cpu_path.topk`` against a brute
force, ``IModel.recommend`` of the five candidate-list models against their own
``forward``, ``topk_pos_rank`` / ``evaluate_full`` on hand-computed cases, and the
conditions the GPU suite's exact-integer cases rely on.

The oracle (``oracle``) is fp64 ``bf16(q) @ bf16(T).T (+ w)`` with excluded, out-of-range
and NaN entries at -inf, a stable argsort of the negated scores (score descending, id
ascending), padded to k with (-1, -inf); a selected -inf entry has id -1.

Two kinds of input:
  * exact integers (q, T in [-2, 2], w in [-3, 3]): every operand survives bf16 and every
    fp32 sum is exact in any order (|score| <= 4 * 64 + 3), so ids and scores are compared
    with ``torch.equal``.  These inputs are dense with ties: they test the tie rule;
  * Gaussian: ``robust_check``, which omits no case.  Per query (a) the scores do not
    increase and equal scores have ascending ids, (b) the ids are distinct, eligible and
    padded as specified, (c) each score is within tol of the oracle's for that id, (d) no
    eligible item left out beats the last returned score by more than the two tols.
    tol[b, i] = (D + 2) 2^-24 (sum_d |bf16 q . bf16 T| + |w|): the fp32 summation bound
    for any order of D products and one addition.

The helpers are shared with tests/test_gpu_topk.py.
"""
import numpy as np
import pytest
import torch

TQ, TI = 32, 128  # mrec_topk_tile_queries / _tile_items (test_exact_case_conditions pins them)


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def excluded_mask(excl, B, n_items):
    """excl = (csr_rows: list of id lists, row_of_query: list or None) -> bool [B, n_items]."""
    m = np.zeros((B, n_items), bool)
    if excl is None:
        return m
    csr, rows = excl
    for b in range(B):
        r = b if rows is None else int(rows[b])
        if 0 <= r < len(csr):
            ids = np.asarray(csr[r], np.int64)
            m[b, ids[(ids >= 0) & (ids < n_items)]] = True
    return m


def oracle(q, T, w, k, low, high, excl=None, const=None):
    """-> (ids int32 [B, k], scores fp64 [B, k], all scores fp64 [B, items] (-inf where not
    eligible), magnitude fp64 [B, items]).  ``const`` [B] is a per-query constant a model
    adds to the scores."""
    B, n_items = q.shape[0], T.shape[0]
    qb, Tb = bf16(q).astype(np.float64), bf16(T).astype(np.float64)
    s = np.full((B, n_items), -np.inf)
    mag = np.zeros((B, n_items))
    with np.errstate(invalid="ignore", over="ignore"):
        s[:, low:high] = qb @ Tb[low:high].T
        mag[:, low:high] = np.abs(qb) @ np.abs(Tb[low:high]).T
        if w is not None:
            s[:, low:high] += np.asarray(w, np.float64)[None, low:high]
            mag[:, low:high] += np.abs(np.asarray(w, np.float64))[None, low:high]
        if const is not None:
            s[:, low:high] += np.asarray(const, np.float64)[:, None]
            mag[:, low:high] += np.abs(np.asarray(const, np.float64))[:, None]
    s[np.isnan(s)] = -np.inf
    s[excluded_mask(excl, B, n_items)] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(s, order, 1)
    ids = order.astype(np.int32)
    if ids.shape[1] < k:
        ids = np.concatenate([ids, np.full((B, k - ids.shape[1]), -1, np.int32)], 1)
        sc = np.concatenate([sc, np.full((B, k - sc.shape[1]), -np.inf)], 1)
    ids[sc == -np.inf] = -1
    return ids, sc, s, mag


def assert_exact(ids, scores, q, T, w, k, low, high, excl=None):
    want_ids, want_s, _, _ = oracle(q, T, w, k, low, high, excl)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids)), "ids"
    assert torch.equal(scores.cpu(), torch.from_numpy(want_s.astype(np.float32))), "scores"


def robust_check(ids, scores, q, T, w, k, low, high, excl=None, const=None):
    ids, scores = ids.cpu().numpy().astype(np.int64), scores.cpu().numpy().astype(np.float64)
    B, D = q.shape
    assert ids.shape == (B, k) and scores.shape == (B, k)
    _, _, s, mag = oracle(q, T, w, k, low, high, excl, const)
    tol = (D + 2 + (const is not None)) * 2.0 ** -24 * mag  # (one more fp32 addition)
    for b in range(B):
        eligible = np.flatnonzero(s[b] > -np.inf)
        n_ret = min(k, eligible.size)
        got, sc = ids[b, :n_ret], scores[b, :n_ret]
        # (b) padding exactly as specified
        assert np.all(ids[b, n_ret:] == -1) and np.all(scores[b, n_ret:] == -np.inf), b
        assert np.all(got >= 0) and len(set(got.tolist())) == n_ret, b
        assert np.all(s[b, got] > -np.inf), (b, "an ineligible item was returned")
        # (a) the total order
        assert np.all(np.diff(sc) <= 0), b
        same = np.diff(sc) == 0
        assert np.all(np.diff(got)[same] > 0), (b, "equal scores out of id order")
        # (c) each score against the oracle's for that id
        assert np.all(np.abs(sc - s[b, got]) <= tol[b, got]), (b, np.max(np.abs(sc - s[b, got]) / tol[b, got]))
        # (d) nothing left out beats the last returned score
        rest = np.setdiff1d(eligible, got)
        if n_ret < k:
            assert rest.size == 0, b
        elif rest.size:
            last = got[-1]
            assert np.all(s[b, rest] <= sc[-1] + tol[b, rest] + tol[b, last]), b


def make_bank(T, w, dtype, device, lead_rows=5):
    """A two-table bank whose table 1 is T (+ w as the first-order column): table 0 and
    nothing else holds 1e30, the pad columns hold NaN."""
    from pytorchrec_amd.embedding import EmbeddingBank
    n, D = T.shape
    bank = EmbeddingBank([lead_rows, n], D, with_first_order=w is not None, dtype=dtype, device=device)
    with torch.no_grad():
        bank.weight.fill_(float("nan"))
        bank.weight[:lead_rows, :D + (w is not None)] = 1e30
        bank.table(1).copy_(torch.from_numpy(np.ascontiguousarray(T, np.float32)).to(dtype))
        if w is not None:
            bank.first_order(1).copy_(torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dtype))
    return bank


def exact_inputs(B, n, D, use_w, seed, low=3, tail=4):
    """Integer q [B, D], T [low + n + tail, D] (1e30 outside [low, low + n)) and w."""
    g = np.random.default_rng(seed)
    q = g.integers(-2, 3, (B, D)).astype(np.float32)
    T = np.full((low + n + tail, D), 1e30, np.float32)
    T[low:low + n] = g.integers(-2, 3, (n, D))
    w = None
    if use_w:
        w = np.full(low + n + tail, 1e30, np.float32)
        w[low:low + n] = g.integers(-3, 4, n)
    return q, T, w, low, low + n


def gauss_inputs(B, n, D, use_w, seed, low=3, tail=4):
    g = np.random.default_rng(seed)
    q = g.standard_normal((B, D)).astype(np.float32)
    T = np.full((low + n + tail, D), 1e30, np.float32)
    T[low:low + n] = g.standard_normal((n, D))
    w = None
    if use_w:
        w = np.full(low + n + tail, 1e30, np.float32)
        w[low:low + n] = g.standard_normal(n)
    return q, T, w, low, low + n


def random_exclusion(B, low, high, seed, per_row=9):
    """A CSR of four rows shared by the queries, addressed through a row index that
    repeats and that holds -1 and n_rows: -> (excl for the oracle, retrieval.Exclusion)."""
    from pytorchrec_amd.retrieval import Exclusion
    g = np.random.default_rng(seed)
    n_rows = 4
    csr = [sorted(set(g.integers(low, max(high, low + 1), per_row).tolist())) for _ in range(n_rows)]
    rows = g.integers(0, n_rows, B)
    if B > 0:
        rows[0] = -1
    if B > 1:
        rows[1] = n_rows
    off = np.zeros(n_rows + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in csr])
    items = np.concatenate([np.asarray(c, np.int32) for c in csr]) if off[-1] else np.zeros(1, np.int32)
    ex = Exclusion(torch.from_numpy(off), torch.from_numpy(items.astype(np.int32)),
                   torch.from_numpy(rows.astype(np.int32)))
    return (csr, rows.tolist()), ex


# (B, n, D, k, bank dtype, q dtype, use_w): every B in {1, TQ - 1, TQ + 1, 2 TQ + 3}, n in
# {1, k - 1, k, TI - 1, TI, TI + 1, 3 TI + 5}, D, k in {1, 7, 64, 128} and dtype at least once
# (an fp32 row of 64 elements has no room for w: 256 B is the widest bank row)
EXACT_CASES = [
    (1, 1, 8, 1, "f32", "f32", False),
    (TQ - 1, 6, 16, 7, "bf16", "f32", False),
    (TQ + 1, 7, 32, 7, "f32", "bf16", True),
    (2 * TQ + 3, TI - 1, 64, 64, "bf16", "bf16", False),
    (1, TI, 64, 128, "bf16", "f32", True),
    (TQ - 1, TI + 1, 8, 1, "bf16", "bf16", False),
    (TQ + 1, 3 * TI + 5, 16, 64, "f32", "f32", False),
    (2 * TQ + 3, 3 * TI + 5, 32, 128, "bf16", "f32", True),
    (TQ + 1, 63, 64, 64, "f32", "bf16", False),
    (2 * TQ + 3, 64, 8, 64, "bf16", "f32", True),
    (TQ - 1, TI - 1, 16, 128, "f32", "f32", False),
    (1, 3 * TI + 5, 32, 7, "bf16", "bf16", True),
    (2 * TQ + 3, TI, 16, 7, "f32", "bf16", False),
    (TQ - 1, 3 * TI + 5, 64, 1, "bf16", "bf16", True),
    (TQ + 1, TI + 1, 64, 128, "bf16", "f32", False),
    (2 * TQ + 3, 1, 32, 1, "f32", "f32", False),
    (TQ + 1, 3 * TI + 5, 8, 7, "bf16", "bf16", False),
    (1, TI + 1, 16, 64, "f32", "bf16", True),
]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def exact_case_seed(i):
    return 1000 + i


def funk(D=8, users=23, items=61, seed=7):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
    from pytorchrec_amd.model import FunkSVD
    return FunkSVD(C(users, "uid"), C(items, "iid"), C(2, "label"), emb_size=D, random_seed=seed)


def svdpp(D=8, users=23, items=61, seed=7, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
    from pytorchrec_amd.model import SVDPP
    return SVDPP(C(users, "uid"), C(items, "iid"), C(items, "iids"), C(2, "label"), emb_size=D,
                 random_seed=seed, **kw)


def sasrec(D=16, items=61, L=9, seed=7, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
    from pytorchrec_amd.model import SASRec
    return SASRec(C(items, "iid"), C(L + 1, "his_len"), C(items, "his"), C(2, "label"), emb_size=D,
                  hidden_size=D, max_his_len=L, num_layers=2, dropout=0.0, random_seed=seed, **kw)


def gru4rec(D=16, H=32, items=61, L=9, seed=7, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
    from pytorchrec_amd.model import GRU4Rec
    return GRU4Rec(C(items, "iid"), C(L + 1, "his_len"), C(items, "his"), C(2, "label"), emb_size=D,
                   hidden_size=H, random_seed=seed, **kw)


def ncf(D=8, users=23, items=61, seed=7, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
    from pytorchrec_amd.model import NCF
    return NCF(C(users, "uid"), C(items, "iid"), C(2, "label"), emb_size=D, layers=(16, 8),
               dropout=0.0, random_seed=seed, **kw)


MODELS = {"funksvd": funk, "svdpp": svdpp, "sasrec": sasrec, "gru4rec": gru4rec, "ncf": ncf}


def model_batch(kind, B, items, L=9, seed=3, users=23, device="cpu", id_dtype=torch.int64):
    """A batch dict without the item column."""
    g = torch.Generator().manual_seed(seed)
    if kind in ("funksvd", "svdpp", "ncf"):
        data = {"uid": torch.randint(0, users, (B,), generator=g)}
        if kind == "svdpp":
            iids = torch.randint(1, items, (B, 6), generator=g)
            iids[torch.rand(B, 6, generator=g) < 0.3] = 0
            data["iids"] = iids
    else:
        his_len = torch.randint(1, L + 1, (B,), generator=g)
        his = torch.randint(1, items, (B, L), generator=g)
        his[torch.arange(L).unsqueeze(0) >= his_len.unsqueeze(1)] = 0
        data = {"his": his, "his_len": his_len}
    return {k: v.to(device=device, dtype=id_dtype) for k, v in data.items()}


def brute_force(model, data, k, low, high, excl=None):
    """Top-k of the model's own forward over all items of [low, high): -> (ids [B, k],
    scores fp32 [B, k], all scores [B, items])."""
    items = model.iid_column.category_num
    B = next(iter(data.values())).shape[0]
    dev = next(model.parameters()).device
    id_dtype = next(iter(data.values())).dtype
    was = model.training
    model.eval()
    with torch.no_grad():
        d = dict(data)
        d["iid"] = torch.arange(items, device=dev, dtype=id_dtype).unsqueeze(0).expand(B, items).contiguous()
        s, _ = model(d)
    model.train(was)
    s = s.float().cpu().numpy().astype(np.float64)
    s[:, :low] = -np.inf
    s[:, high:] = -np.inf
    s[excluded_mask(excl, B, items)] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(s, order, 1).astype(np.float32), s


def assert_lists_agree(ids, scores, want_ids, want_scores, rtol, atol):
    """Scores close; ids equal wherever the neighbouring wanted scores are further apart
    than the bar."""
    ids, scores = np.asarray(ids), np.asarray(scores, np.float64)
    want_scores = np.asarray(want_scores, np.float64)
    np.testing.assert_allclose(scores, want_scores, rtol=rtol, atol=atol)
    bar = atol + rtol * np.abs(want_scores)
    gap_prev = np.abs(np.diff(want_scores, axis=1, prepend=np.inf))
    gap_next = np.abs(np.diff(want_scores, axis=1, append=-np.inf))
    clear = (gap_prev > 2 * bar) & (gap_next > 2 * bar)
    assert np.array_equal(ids[clear], np.asarray(want_ids)[clear])


# ---------------------------------------------------------------------------
# cpu_path.topk against the oracle
# ---------------------------------------------------------------------------

def _cpu_topk(q, T, w, k, low, high, ex=None, chunk=8192, dtype=torch.float32):
    from pytorchrec_amd import cpu_path
    bank = make_bank(T, w, dtype, "cpu")
    o = bank.row_offset[1]
    rows = bank.weight.detach()[o:o + T.shape[0]]
    triple = (ex.offsets, ex.items, ex.rows) if ex is not None else None
    return cpu_path.topk(rows, T.shape[1], torch.from_numpy(q), k, low, high, w is not None, triple,
                         chunk=chunk)


@pytest.mark.parametrize("n,k,chunk,use_w,low", [
    (100, 10, 50, False, 3),   # the chunk divides the range
    (100, 10, 7, True, 3),     # ... and does not
    (100, 10, 1000, False, 0),
    (9, 12, 4, True, 5),       # k > n
    (12, 12, 5, False, 2),     # k == n
    (0, 5, 8, False, 4),       # n == 0
    (1, 1, 1, True, 0),
])
@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_cpu_topk_matches_oracle(kind, n, k, chunk, use_w, low):
    B, D = 11, 16
    q, T, w, low, high = (exact_inputs if kind == "exact" else gauss_inputs)(B, n, D, use_w, 5, low=low)
    ids, scores = _cpu_topk(q, T, w, k, low, high, chunk=chunk)
    assert ids.dtype == torch.int32 and scores.dtype == torch.float32
    if kind == "exact":
        assert_exact(ids, scores, q, T, w, k, low, high)
    else:
        robust_check(ids, scores, q, T, w, k, low, high)


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_cpu_topk_exclusion_rows_and_nan_row(kind):
    """A shared CSR through a row index with repeats, -1 and n_rows; a NaN table row."""
    B, n, D, k = 13, 90, 8, 12
    q, T, w, low, high = (exact_inputs if kind == "exact" else gauss_inputs)(B, n, D, True, 9)
    T[low + 17] = np.nan
    excl, ex = random_exclusion(B, low, high, 4)
    ids, scores = _cpu_topk(q, T, w, k, low, high, ex, chunk=32)
    assert not (ids == low + 17).any()
    if kind == "exact":
        assert_exact(ids, scores, q, T, w, k, low, high, excl)
    else:
        robust_check(ids, scores, q, T, w, k, low, high, excl)


def test_exclusion_from_lists_and_whole_range():
    """from_lists sorts, de-duplicates, drops pad and negatives; a query whose whole range
    is excluded is all padding."""
    from pytorchrec_amd.retrieval import Exclusion
    B, n, D, k = 4, 20, 8, 5
    q, T, w, low, high = exact_inputs(B, n, D, False, 2, low=0, tail=0)
    lists = torch.tensor([[5, 3, 5, 0, -1, 3], [0, 0, 0, 0, 0, 0], [19, 1, 2, 0, 7, 7],
                          [4, 4, 4, 4, 4, 4]])
    ex = Exclusion.from_lists(lists, pad=0)
    assert ex.offsets.tolist() == [0, 2, 2, 6, 7] and ex.items[:7].tolist() == [3, 5, 1, 2, 7, 19, 4]
    assert ex.items.dtype == torch.int32 and ex.offsets.dtype == torch.int64 and ex.rows is None
    csr = [[3, 5], [], [1, 2, 7, 19], [4]]
    ids, scores = _cpu_topk(q, T, w, k, low, high, ex, chunk=6)
    assert_exact(ids, scores, q, T, w, k, low, high, (csr, None))
    whole = Exclusion.from_lists(torch.arange(n).unsqueeze(0).expand(B, n), pad=None)
    ids, scores = _cpu_topk(q, T, w, k, low, high, whole)
    assert (ids == -1).all() and (scores == float("-inf")).all()


def test_exclusion_from_sampler_rebases_items():
    from pytorchrec_amd.retrieval import Exclusion
    from pytorchrec_amd.sampling import NegativeSampler
    s = NegativeSampler([0, 0, 2, 2, 2], [12, 10, 15, 11, 15], low=10, high=30, n_users=3)
    ex = Exclusion.from_sampler(s, torch.tensor([2, 1, 0, 7]))
    assert ex.offsets.tolist() == [0, 2, 2, 4] and ex.items[:4].tolist() == [0, 2, 1, 5]
    assert ex.rows.tolist() == [2, 1, 0, 7]
    B, n, D, k = 4, 20, 8, 20
    q, T, w, low, high = exact_inputs(B, n, D, False, 6, low=0, tail=0)
    ids, scores = _cpu_topk(q, T, w, k, low, high, ex)
    assert_exact(ids, scores, q, T, w, k, low, high, ([[0, 2], [], [1, 5]], [2, 1, 0, 7]))
    s0 = NegativeSampler([0], [3], low=0, high=5, n_users=1)
    assert Exclusion.from_sampler(s0, torch.tensor([0])).items.data_ptr() == s0.items.data_ptr()


def test_retrieval_topk_on_a_cpu_bank_and_its_argument_errors():
    from pytorchrec_amd import retrieval
    B, n, D, k = 5, 40, 8, 6
    q, T, w, low, high = exact_inputs(B, n, D, True, 8)
    bank = make_bank(T, w, torch.float32, "cpu")
    ids, scores = retrieval.topk(bank, 1, torch.from_numpy(q), k, low=low, high=high, use_w=True)
    assert_exact(ids, scores, q, T, w, k, low, high)
    no_w = make_bank(T, None, torch.float32, "cpu")
    tq = torch.from_numpy(q)
    for bad in (dict(k=0), dict(k=k, low=high + 1, high=high), dict(k=k, high=T.shape[0] + 1),
                dict(k=k, use_w=True), dict(k=k, item_splits=0)):
        with pytest.raises(ValueError):
            retrieval.topk(no_w, 1, tq, **bad)
    with pytest.raises(ValueError):
        retrieval.topk(no_w, 2, tq, k)
    with pytest.raises(ValueError):
        retrieval.topk(no_w, 1, tq[:, :4], k)


def test_exact_case_conditions():
    """What the exact-integer GPU cases rely on: the library's tile sizes are the ones the
    shapes were chosen around, every operand is a bf16 value, every score is an integer
    small enough for fp32 to sum exactly in any order, and wherever the shape allows it the
    case has ties inside its top k and across its k-th place (so it tests the tie rule)."""
    from pytorchrec_amd import retrieval
    assert (retrieval.tile_queries(), retrieval.tile_items()) == (TQ, TI)
    seen = {"B": set(), "D": set(), "k": set(), "n": set()}
    for i, (B, n, D, k, bd, qd, use_w) in enumerate(EXACT_CASES):
        q, T, w, low, high = exact_inputs(B, n, D, use_w, exact_case_seed(i))
        assert np.array_equal(bf16(q), q) and np.array_equal(bf16(T[low:high]), T[low:high])
        assert w is None or np.array_equal(bf16(w[low:high]), w[low:high])
        _, _, s, mag = oracle(q, T, w, min(k, n), low, high)
        assert mag.max() <= 4 * 64 + 3 < 2 ** 24 and np.array_equal(s[:, low:high], np.round(s[:, low:high]))
        srt = -np.sort(-s[:, low:high], axis=1)
        if min(k, n) >= 2 and B * min(k, n) >= 32:
            assert (np.diff(srt[:, :k], axis=1) == 0).any(), (i, "no tie inside the top k")
        if n > k and B * k >= 7:
            assert (srt[:, k - 1] == srt[:, k]).any(), (i, "no tie across the k-th place")
        for name, v in (("B", B), ("D", D), ("k", k)):
            seen[name].add(v)
        seen["n"] |= {n} | {name for name, v in (("1", 1), ("k-1", k - 1), ("k", k)) if v == n}
    assert seen["B"] == {1, TQ - 1, TQ + 1, 2 * TQ + 3} and seen["D"] == {8, 16, 32, 64}
    assert seen["k"] == {1, 7, 64, 128}
    assert seen["n"] >= {"1", "k-1", "k", TI - 1, TI, TI + 1, 3 * TI + 5}


# ---------------------------------------------------------------------------
# IModel.recommend on CPU models
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(MODELS))
def test_recommend_equals_the_models_own_forward(kind):
    """recommend == the brute force over forward's scores of all items (the bar of a CPU
    forward in test_product_pins.py: rtol 1e-5, atol 1e-9), with an exclusion, a sub-range
    and the default range; the training flag is left as found."""
    from pytorchrec_amd.model.IModel import IModel
    m = MODELS[kind]()
    items, B, k = 61, 9, 7
    data = model_batch(kind, B, items)
    base = 1 if kind == "sasrec" else 0
    excl, ex = random_exclusion(B, 0, items, 11)
    for low, high, e, eo in ((None, None, None, None), (5, 50, ex, excl), (None, None, ex, excl)):
        lo, hi = (base if low is None else low), (items if high is None else high)
        want_ids, want_s, _ = brute_force(m, data, k, lo, hi, eo)
        for training in (True, False):
            m.train(training)
            ids, scores = m.recommend(data, k, exclude=e, low=low, high=high)
            assert m.training == training
            assert ids.dtype == torch.int32 and scores.dtype == torch.float32
            assert_lists_agree(ids.numpy(), scores.numpy(), want_ids, want_s, 1e-5, 1e-9)
            # the generic path through forward agrees in the same way
            ids2, scores2 = IModel.recommend_by_forward(m, data, k, exclude=e, low=low, high=high,
                                                        chunk=16)
            assert m.training == training
            assert_lists_agree(ids2.numpy(), scores2.numpy(), want_ids, want_s, 1e-5, 1e-9)
    if kind == "sasrec":
        ids, _ = m.recommend(data, items)  # more than the items: id 0 never, padding last
        assert not (ids == 0).any() and (ids[:, -1] == -1).all()


def test_ncf_takes_the_generic_path_and_ctr_models_refuse():
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C, NumericColumn
    from pytorchrec_amd.model import DeepFM
    from pytorchrec_amd.model.IModel import IModel
    assert type(ncf())._retrieval_query is IModel._retrieval_query
    for kind in ("funksvd", "svdpp", "sasrec", "gru4rec"):
        assert type(MODELS[kind]())._retrieval_query is not IModel._retrieval_query
    m = DeepFM([C(7, "a"), C(5, "b")], [NumericColumn("x")], C(2, "label"), emb_size=8, layers=(8,),
               random_seed=1)
    with pytest.raises(NotImplementedError, match="DeepFM"):
        m.recommend({"a": torch.zeros(2, dtype=torch.int64)}, 3)


def test_topk_pos_rank_hand_case():
    from pytorchrec_amd.metrics import NDCG, Hit, topk_pos_rank
    ids = np.array([[4, 9, 2], [7, 1, 3], [5, 6, -1], [0, 8, 2]])
    pos = np.array([2, 7, 9, 8])
    ranks = topk_pos_rank(ids, pos)
    assert ranks.dtype == np.int64 and ranks.tolist() == [3, 1, 4, 2]
    t = topk_pos_rank(torch.from_numpy(ids).int(), torch.from_numpy(pos))
    assert t.dtype == torch.int64 and t.tolist() == [3, 1, 4, 2]
    want = (1 / np.log2(4) + 1 + 1 / np.log2(3)) / 4
    assert abs(NDCG(0, 3).fast_calc(ranks) - want) < 1e-12
    assert Hit(0, 3).fast_calc(ranks) == 0.75 and Hit(0, 2).fast_calc(ranks) == 0.5


def test_evaluate_full_hand_case():
    """Three users, five items, planted tables: the positives' places among all items are
    1, 3 and (excluded training item aside) 2."""
    from pytorchrec_amd.sampling import NegativeSampler
    m = funk(D=8, users=3, items=5)
    with torch.no_grad():
        m.embeddings.weight.zero_()
        m.embeddings.table(0)[:, 0] = 1.0
        m.embeddings.table(1)[:, 0] = torch.tensor([5.0, 4.0, 3.0, 2.0, 1.0])
    rows = [{"uid": torch.tensor(u), "iid": torch.tensor(i)} for u, i in ((0, 0), (1, 2), (2, 2))]
    got = m.evaluate_full(rows, batch_size=2, k=3, pos_column=m.iid_column)
    assert set(got) == {"ndcg@3", "hit@3"}
    assert abs(got["ndcg@3"] - (1 + 0.5 + 0.5) / 3) < 1e-12 and got["hit@3"] == 1.0
    got = m.evaluate_full(rows, batch_size=3, k=2, pos_column=m.iid_column)
    assert abs(got["ndcg@2"] - 1 / 3) < 1e-12 and abs(got["hit@2"] - 1 / 3) < 1e-12
    sampler = NegativeSampler([2, 1], [0, 4], low=0, high=5, n_users=3)
    got = m.evaluate_full(rows, batch_size=2, k=2, pos_column=m.iid_column, exclude=sampler)
    # user 2 loses item 0: its positive moves from place 3 to 2; user 1's stays at 3
    assert abs(got["ndcg@2"] - (1 + 1 / np.log2(3)) / 3) < 1e-12 and abs(got["hit@2"] - 2 / 3) < 1e-12
