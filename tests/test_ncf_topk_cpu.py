"""Full-catalogue top-K retrieval for NCF on the CPU (no GPU): ``cpu_path.ncf_topk`` against
a brute force, the argument errors of ``retrieval.ncf_topk``, ``NCF.recommend`` on a CPU
model, and the conditions the GPU suite's exact-integer cases rely on.

The oracle is fp64 over every (user, item) pair -- the contract of include/mrec.h above
``mrec_ncf_topk``, nothing rounded -- with excluded, out-of-range and NaN entries at -inf,
a stable argsort of the negated scores (score descending, id ascending), padded to k with
(-1, -inf).

Two kinds of input:
  * exact integers, by the method of tests/test_gpu_ncf.py and with its weight
    construction: table rows hold -1 / 0 / 1, every W_l is sparse +-1 with a non-zero in
    every 16 x 16 block, biases are 0 .. 2, wp is in {+-1, +-2}.  Then every a, c, h_l and
    score is an integer that survives bf16 where the kernel rounds it and every fp32 sum
    is exact in any order, so ids and scores are compared with ``torch.equal``; integer
    scores are dense with ties, so this pins the tie rule.  ``exact_case`` asserts the
    conditions, ``test_exact_case_conditions`` checks them for every case of the matrix;
  * Gaussian: against ``NCF.forward`` over all items at the bar of a CPU forward
    (rtol 1e-5, atol 1e-9, ``assert_lists_agree`` of tests/test_topk_cpu.py).

The helpers are shared with tests/test_gpu_ncf_topk.py.
"""
import functools

import numpy as np
import pytest
import torch

from test_topk_cpu import assert_lists_agree, bf16, brute_force, excluded_mask, random_exclusion

TU, TI = 16, 64  # mrec_ncf_topk_tile_users / _tile_items (test_exact_case_conditions pins them)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
IDS = {"i32": torch.int32, "i64": torch.int64}
BIG = 1e30  # what a row nobody may read holds
# plans of 163,784 and 163,752 of the 163,840 bytes of LDS: the gate says yes, so they must launch
EDGE_SHAPES = ((16, (88, 120, 120), 64), (8, (104, 104, 56), 80))


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def exact_weights(rng, E, layers, nnz):
    """The weight construction of test_gpu_ncf._exact_inputs: ``nnz`` entries +-1 per
    output row, a non-zero in every 16 x 16 block (edge blocks too), biases 0 .. 2, wp in
    {+-1, +-2}."""
    ws, bs = [], []
    K = 2 * E
    for N in layers:
        w = np.zeros((N, K))
        for n in range(N):
            cols = rng.choice(K, size=min(nnz, K), replace=False)
            w[n, cols] = rng.choice([-1.0, 1.0], size=cols.size)
        for n0 in range(0, N, 16):
            for k0 in range(0, K, 16):
                blk = w[n0:n0 + 16, k0:k0 + 16]
                if not blk.any():
                    blk[rng.integers(blk.shape[0]), rng.integers(blk.shape[1])] = rng.choice([-1.0, 1.0])
        ws.append(w)
        bs.append(rng.integers(0, 3, size=N).astype(np.float64))
        K = N
    wp = rng.choice([-2.0, -1.0, 1.0, 2.0], size=E + K)
    return ws, bs, wp


def score64(c, rows=None):
    """fp64 restatement of the score contract for every (user of the batch, item):
    -> (s [B, all items], -inf outside [low, high); the parts a, c, h_l, g for the
    condition checks).  A NaN mf row gives NaN scores; a NaN mlp row does not (the ReLU)."""
    E, low, high = c["E"], c["low"], c["high"]
    u = c["uid"]
    mf_u, mf_i, mlp_u, mlp_i = (np.asarray(t, np.float64) for t in c["tables"])
    w0 = c["ws"][0]
    def relu(x):  # the kernels' x > 0 ? x : 0: a NaN pre-activation gives 0
        return np.where(x > 0, x, 0.0)

    with np.errstate(invalid="ignore"):
        a = c["bs"][0] + mlp_u[u] @ w0[:, :E].T                       # [B, N0]
        ci = mlp_i[low:high] @ w0[:, E:].T                            # [n, N0]
        hs = [relu(a[:, None, :] + ci[None])]
        for w, b in zip(c["ws"][1:], c["bs"][1:]):
            hs.append(relu(hs[-1] @ w.T + b))
        g = mf_u[u][:, None, :] * mf_i[low:high][None]                # [B, n, E]
        live = g @ c["wp"][:E] + hs[-1] @ c["wp"][E:]
    s = np.full((u.shape[0], mf_i.shape[0]), -np.inf)
    s[:, low:high] = live
    return s, dict(a=a, c=ci, hs=hs, g=g)


def select(s, k, excl=None):
    """The selection oracle over the scores s [B, all items] (-inf = not in range):
    -> (ids int32 [B, k], scores fp64 [B, k])."""
    s = np.array(s, np.float64)
    B, n_items = s.shape
    s[np.isnan(s)] = -np.inf
    s[excluded_mask(excl, B, n_items)] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(s, order, 1)
    ids = order.astype(np.int32)
    if ids.shape[1] < k:
        ids = np.concatenate([ids, np.full((B, k - ids.shape[1]), -1, np.int32)], 1)
        sc = np.concatenate([sc, np.full((B, k - sc.shape[1]), -np.inf)], 1)
    ids[sc == -np.inf] = -1
    return ids, sc


def assert_exact(ids, scores, c, k, excl=None):
    want_ids, want_s = select(score64(c)[0], k, excl)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids)), "ids"
    assert torch.equal(scores.cpu(), torch.from_numpy(want_s.astype(np.float32))), "scores"


def _bf16_exact(x):
    x = np.asarray(x, np.float64)
    return np.array_equal(bf16(x).astype(np.float64), x)


def assert_conditions(c):
    """What makes an exact case exact, and what makes it sensitive."""
    E = c["E"]
    s, parts = score64(c)
    live = s[:, c["low"]:c["high"]]
    lim = float(2 ** 24)
    u = c["uid"]
    mf_u, mf_i, mlp_u, mlp_i = c["tables"]
    w0 = c["ws"][0]
    # every a, c, h_l and score is an integer
    for name in ("a", "c", "g"):
        assert np.array_equal(parts[name], np.round(parts[name])), (c["name"], name)
    assert np.array_equal(live, np.round(live)), (c["name"], "score")
    # every value rounded to bf16 is <= 256 in magnitude and survives the round trip
    for t in (mf_u[u], mlp_u[u], mf_i[c["low"]:c["high"]], mlp_i[c["low"]:c["high"]], *c["ws"]):
        assert _bf16_exact(t) and np.abs(t).max() <= 256
    for l, h in enumerate(parts["hs"]):
        assert np.array_equal(h, np.round(h)) and _bf16_exact(h) and np.abs(h).max() <= 256, (c["name"], "h", l)
    # sum |terms| < 2^24 for every fp32 sum: exact in any order
    assert (np.abs(c["bs"][0]) + np.abs(mlp_u[u]) @ np.abs(w0[:, :E]).T).max() < lim
    assert (np.abs(mlp_i[c["low"]:c["high"]]) @ np.abs(w0[:, E:]).T).max() < lim
    for l in range(1, len(c["ws"])):
        assert (parts["hs"][l - 1] @ np.abs(c["ws"][l]).T + np.abs(c["bs"][l])).max() < lim
    assert (np.abs(parts["g"]) @ np.abs(c["wp"][:E]) + parts["hs"][-1] @ np.abs(c["wp"][E:])).max() < lim
    # every ReLU is active on 25-75 % of its elements over all (user, item) pairs
    for l, h in enumerate(parts["hs"]):
        active = float((h > 0).mean())
        assert 0.25 <= active <= 0.75, (c["name"], "relu", l, active)
    for w in c["ws"]:
        for n0 in range(0, w.shape[0], 16):
            for k0 in range(0, w.shape[1], 16):
                assert w[n0:n0 + 16, k0:k0 + 16].any(), (c["name"], "block", n0, k0)
    # each user's item scores take at least 3 distinct values (as far as it has items)
    n = live.shape[1]
    for b in range(live.shape[0]):
        assert len(set(live[b].tolist())) >= min(3, n), (c["name"], "distinct", b)


@functools.lru_cache(maxsize=None)
def exact_case(B, n, E, layers, seed, nnz=4, low=3, tail=4, check=True):
    """Integer inputs for B users and the items [low, low + n) of item tables with `low`
    rows before and `tail` after; the user tables have rows no uid names.  Rows nobody may
    read hold 1e30.  The batch repeats a user when it can.  Deterministic; the conditions
    are asserted."""
    rng = np.random.default_rng(4321 + seed)
    users, items = B + 3, low + n + tail
    uid = rng.integers(0, users, B)
    if B > 1:
        uid[-1] = uid[0]
    tables = []
    for f in range(4):
        rows = users if f % 2 == 0 else items
        t = np.full((rows, E), BIG)
        if f % 2 == 0:
            named = np.unique(uid)
            t[named] = rng.integers(-1, 2, size=(named.size, E))
        else:
            t[low:low + n] = rng.integers(-1, 2, size=(n, E))
        tables.append(t)
    tables = [tables[0], tables[1], tables[2], tables[3]]  # mf_u, mf_i, mlp_u, mlp_i
    ws, bs, wp = exact_weights(rng, E, layers, nnz)
    c = dict(name=f"B{B}_n{n}_E{E}_{'x'.join(map(str, layers))}_s{seed}", E=E, layers=tuple(layers), uid=uid,
             users=users, items=items, low=low, high=low + n, tables=tables, ws=ws, bs=bs, wp=wp)
    if check:
        assert_conditions(c)
    return c


# (B, items, E, layers, k, bank dtype, uid dtype, seed): every B in {1, TU - 1, TU + 1,
# 2 TU + 3}, items in {1, k - 1, k, TI - 1, TI, TI + 1, 3 TI + 5}, tower, k in {1, 7, 64, 128}
# and dtype at least once.  The seed is the first for which the conditions hold.
T5 = 3 * TI + 5
EXACT_CASES = [
    (1, 1, 8, (8,), 1, "f32", "i32", 0),
    (TU - 1, 6, 8, (16, 8), 7, "bf16", "i64", 0),
    (TU + 1, 7, 16, (32, 24, 8), 7, "f32", "i32", 0),
    (2 * TU + 3, TI - 1, 32, (24, 16), 64, "bf16", "i32", 0),
    (1, TI, 64, (128, 64, 32), 128, "bf16", "i64", 0),
    (TU - 1, TI + 1, 8, (8,), 1, "bf16", "i32", 0),
    (TU + 1, T5, 16, (32, 24, 8), 64, "f32", "i64", 0),
    (2 * TU + 3, T5, 32, (24, 16), 128, "bf16", "i32", 0),
    (TU + 1, TI - 1, 64, (128, 64, 32), 64, "f32", "i32", 0),
    (2 * TU + 3, TI, 8, (16, 8), 64, "bf16", "i64", 0),
    (TU - 1, 127, 16, (32, 24, 8), 128, "f32", "i32", 0),
    (1, T5, 32, (24, 16), 7, "bf16", "i64", 0),
    (2 * TU + 3, TI, 16, (32, 24, 8), 7, "f32", "i32", 0),
    (TU - 1, T5, 64, (128, 64, 32), 1, "bf16", "i32", 0),
    (TU + 1, TI + 1, 64, (128, 64, 32), 128, "bf16", "i64", 0),
    (2 * TU + 3, 1, 32, (24, 16), 1, "f32", "i64", 0),
]


def case_inputs(i):
    B, n, E, layers, k, bd, ud, seed = EXACT_CASES[i]
    return exact_case(B, n, E, layers, seed, nnz=3 if E == 64 else 4)


def make_bank(c, dtype, device, lead_rows=0):
    """The bank [mf_u, mf_i, mlp_u, mlp_i] of a case (after ``lead_rows`` rows of a table
    nobody reads, when asked for): -> (bank, table indices).  Pad columns hold NaN."""
    from pytorchrec_amd.embedding import EmbeddingBank
    E = c["E"]
    rows = [t.shape[0] for t in c["tables"]]
    bank = EmbeddingBank(([lead_rows] if lead_rows else []) + rows, E, dtype=dtype, device=device)
    first = 1 if lead_rows else 0
    with torch.no_grad():
        bank.weight.fill_(float("nan"))
        if lead_rows:
            bank.table(0).fill_(BIG)
        for f, t in enumerate(c["tables"]):
            bank.table(first + f).copy_(torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(dtype))
    return bank, tuple(range(first, first + 4))


def dense_params(c, device):
    f32 = dict(dtype=torch.float32, device=device)
    ws = [torch.tensor(w, **f32) for w in c["ws"]]
    bs = [torch.tensor(b, **f32) for b in c["bs"]]
    return ws, bs, torch.tensor(c["wp"], **f32)


def gauss_case(B, n, E, layers, seed, low=3, tail=4):
    """Gaussian tables (0.5 N(0, 1)) and dense parameters (0.3 N(0, 1)) in a case's form."""
    rng = np.random.default_rng(seed)
    users, items = B + 3, low + n + tail
    uid = rng.integers(0, users, B)
    tables = []
    for f in range(4):
        rows = users if f % 2 == 0 else items
        t = np.full((rows, E), BIG)
        if f % 2 == 0:
            t[:] = bf16(0.5 * rng.standard_normal((rows, E)))
        else:
            t[low:low + n] = bf16(0.5 * rng.standard_normal((n, E)))
        tables.append(t)
    ws, bs, K = [], [], 2 * E
    for N in layers:
        ws.append(0.3 * rng.standard_normal((N, K)).astype(np.float32).astype(np.float64))
        bs.append(0.3 * rng.standard_normal(N).astype(np.float32).astype(np.float64))
        K = N
    wp = 0.3 * rng.standard_normal(E + K).astype(np.float32).astype(np.float64)
    return dict(name=f"gauss{seed}", E=E, layers=tuple(layers), uid=uid, users=users, items=items, low=low,
                high=low + n, tables=tables, ws=ws, bs=bs, wp=wp)


def _cpu_ncf_topk(c, k, low, high, ex=None, chunk=8192, dtype=torch.float32, round_bf16=True):
    from pytorchrec_amd import cpu_path
    bank, tabs = make_bank(c, dtype, "cpu")
    tables = [bank.weight.detach()[bank.row_offset[t]:bank.row_offset[t] + bank.category_nums[t]] for t in tabs]
    ws, bs, wp = dense_params(c, "cpu")
    triple = (ex.offsets, ex.items, ex.rows) if ex is not None else None
    return cpu_path.ncf_topk(tables, c["E"], torch.from_numpy(c["uid"]), ws, bs, wp, k, low, high, triple,
                             chunk=chunk, round_bf16=round_bf16)


# ---------------------------------------------------------------------------
# cpu_path.ncf_topk against the brute force
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,chunk,E,layers,dtype,seed", [
    (100, 10, 50, 8, (16, 8), "f32", 50),      # the chunk divides the range
    (100, 10, 7, 16, (32, 24, 8), "bf16", 50),  # ... and does not
    (9, 12, 4, 8, (8,), "f32", 51),            # k > the eligible items, one layer
    (12, 12, 5, 32, (24, 16), "bf16", 50),     # k == n
    (0, 5, 8, 8, (16, 8), "f32", 50),          # an empty range (nothing to condition)
    (1, 1, 1, 8, (16, 8), "f32", 50),
])
def test_cpu_ncf_topk_matches_brute_force_on_exact_inputs(n, k, chunk, E, layers, dtype, seed):
    c = exact_case(11, n, E, layers, seed, check=n >= 9)
    ids, scores = _cpu_ncf_topk(c, k, c["low"], c["high"], chunk=chunk, dtype=DTYPES[dtype])
    assert ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert_exact(ids, scores, c, k)


def test_cpu_ncf_topk_exclusion_sub_range_and_nan_row():
    """A shared CSR through a row index with repeats, -1 and n_rows; a sub-range; an item
    whose rows are NaN is never returned; k above the eligible items pads."""
    c = exact_case(13, 90, 16, (32, 24, 8), 51)
    excl, ex = random_exclusion(13, c["low"], c["high"], 4)
    ids, scores = _cpu_ncf_topk(c, 12, c["low"], c["high"], ex, chunk=32)
    assert_exact(ids, scores, c, 12, excl)
    sub = dict(c, low=c["low"] + 20, high=c["low"] + 31)  # 11 items, some excluded: k = 12 pads
    ids, scores = _cpu_ncf_topk(c, 12, sub["low"], sub["high"], ex, chunk=5)
    assert_exact(ids, scores, sub, 12, excl)
    assert (ids[:, -1] == -1).all() and (scores[:, -1] == float("-inf")).all()
    nan = dict(c, tables=[t.copy() for t in c["tables"]])
    nan_id = c["low"] + 17
    nan["tables"][1][nan_id] = np.nan
    nan["tables"][3][nan_id] = np.nan
    half_id = c["low"] + 40  # only its mlp row is NaN: the ReLU stops that, the item is scored
    nan["tables"][3][half_id] = np.nan
    ids, scores = _cpu_ncf_topk(nan, 90, c["low"], c["high"], chunk=32)
    assert not (ids == nan_id).any() and (ids[:, -1] == -1).all() and (ids[:, -2] >= 0).all()
    assert (ids == half_id).any(1).all()
    assert_exact(ids, scores, nan, 90)


@pytest.mark.parametrize("E,layers", [(8, (16, 8)), (16, (32,)), (64, (128, 64, 32))])
def test_cpu_ncf_topk_matches_the_models_forward_on_gaussian_inputs(E, layers):
    """``retrieval.ncf_topk`` on a CPU model == the brute force over ``NCF.forward``'s scores
    of all items, at the bar of a CPU forward: with an exclusion, a sub-range, and k above
    the number of eligible items.  The models are as ``IModel`` initialises them (every
    tensor N(0, 0.01)), the inputs test_topk_cpu.py holds its models to this bar on: the
    two paths sum layer 0 in different orders, and the bar's atol is sized for scores of
    that scale."""
    from pytorchrec_amd import retrieval
    from test_ncf_cpu import ncf
    users, items, B = 23, 61, 9
    m = ncf(users=users, items=items, emb_size=E, layers=layers, seed=3 + E)
    data = {"uid": torch.randint(0, users, (B,), generator=torch.Generator().manual_seed(1))}
    excl, ex = random_exclusion(B, 0, items, 11)
    for low, high, k, e, eo in ((0, items, 7, None, None), (5, 50, 7, ex, excl), (40, 48, 12, ex, excl)):
        want_ids, want_s, _ = brute_force(m, data, min(k, high - low), low, high, eo)
        ids, scores = retrieval.ncf_topk(m, data["uid"], k, low=low, high=high, exclude=e)
        assert ids.dtype == torch.int32 and scores.dtype == torch.float32 and ids.shape == (B, k)
        n_ret = (want_s > -np.inf).sum(1)
        for b in range(B):  # the padding past the eligible items
            assert (ids[b, n_ret[b]:] == -1).all() and (scores[b, n_ret[b]:] == float("-inf")).all()
        kk = int(n_ret.min())
        assert_lists_agree(ids.numpy()[:, :kk], scores.numpy()[:, :kk], want_ids[:, :kk], want_s[:, :kk],
                           1e-5, 1e-9)


def test_exact_case_conditions():
    """What the exact-integer GPU cases rely on: the library's tile sizes are the ones the
    shapes were chosen around, the generator's conditions hold for every case, every
    required value of the matrix occurs, and the cases have ties inside their top k and
    across the k-th place wherever the shape allows it (so they test the tie rule)."""
    from pytorchrec_amd import retrieval
    assert (retrieval.ncf_tile_users(), retrieval.ncf_tile_items()) == (TU, TI)
    seen = {"B": set(), "tower": set(), "k": set(), "n": set(), "bd": set(), "ud": set()}
    for i, (B, n, E, layers, k, bd, ud, seed) in enumerate(EXACT_CASES):
        c = case_inputs(i)
        assert_conditions(c)
        assert c["uid"].shape == (B,) and (B == 1 or c["uid"][-1] == c["uid"][0])
        s = score64(c)[0][:, c["low"]:c["high"]]
        srt = -np.sort(-s, axis=1)
        if min(k, n) >= 2 and B * min(k, n) >= 32:
            assert (np.diff(srt[:, :k], axis=1) == 0).any(), (i, "no tie inside the top k")
        if n > k and B * k >= 32:
            assert (srt[:, k - 1] == srt[:, k]).any(), (i, "no tie across the k-th place")
        for name, v in (("B", B), ("tower", (E, layers)), ("k", k), ("bd", bd), ("ud", ud)):
            seen[name].add(v)
        seen["n"] |= {n} | {name for name, v in (("1", 1), ("k-1", k - 1), ("k", k)) if v == n}
    assert seen["B"] == {1, TU - 1, TU + 1, 2 * TU + 3}
    assert seen["tower"] == {(8, (8,)), (8, (16, 8)), (16, (32, 24, 8)), (32, (24, 16)), (64, (128, 64, 32))}
    assert seen["k"] == {1, 7, 64, 128} and seen["bd"] == {"f32", "bf16"} and seen["ud"] == {"i32", "i64"}
    assert seen["n"] >= {"1", "k-1", "k", TI - 1, TI, TI + 1, T5}


# ---------------------------------------------------------------------------
# retrieval.ncf_topk's arguments; NCF.recommend on a CPU model
# ---------------------------------------------------------------------------

def test_ncf_topk_argument_errors():
    from pytorchrec_amd import retrieval
    from test_ncf_cpu import ncf
    m = ncf(users=23, items=61)
    uid = torch.tensor([1, 5, 22])
    ids, scores = retrieval.ncf_topk(m, uid, 4)
    assert ids.shape == (3, 4) and scores.shape == (3, 4)
    for bad in (dict(k=0), dict(k=-3), dict(k=4, low=30, high=20), dict(k=4, high=62), dict(k=4, low=-1),
                dict(k=4, item_splits=0), dict(k=4, item_splits=65)):
        with pytest.raises(ValueError):
            retrieval.ncf_topk(m, uid, **bad)
    for bad_uid in (uid.reshape(3, 1), uid.float(), uid.to(torch.int16), torch.tensor(3)):
        with pytest.raises(ValueError):
            retrieval.ncf_topk(m, bad_uid, 4)
    for bad_uid in (torch.tensor([1, 23]), torch.tensor([-1, 2])):
        with pytest.raises(IndexError):
            retrieval.ncf_topk(m, bad_uid, 4)
    ids, scores = retrieval.ncf_topk(m, uid[:0], 4)
    assert ids.shape == (0, 4) and scores.shape == (0, 4)
    # the parameter tuple is the model, spelled out
    bank, ws, bs, wp = retrieval._ncf_params(m)
    a = retrieval.ncf_topk((bank, ws, bs, wp), uid.int(), 4, low=3)
    b = retrieval.ncf_topk(m, uid, 4, low=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ncf_topk_supported_names_the_compiled_shapes():
    from pytorchrec_amd import retrieval
    f32, b16 = torch.float32, torch.bfloat16
    for E, layers in ((8, (8,)), (8, (16, 8)), (16, (32, 24, 8)), (32, (24, 16)), (64, (128, 64, 32)),
                      (64, (64,)), (32, (64, 32, 16))):
        for k in (1, 128):
            assert retrieval.ncf_supported(E, layers, k, f32) and retrieval.ncf_supported(E, layers, k, b16)
    for E, layers, k, dt in ((12, (16, 8), 10, f32), (8, (136,), 10, f32), (8, (20, 8), 10, f32),
                             (8, (16, 8, 8, 8), 10, f32), (8, (), 10, f32), (8, (16, 8), 0, f32),
                             (8, (16, 8), 129, f32), (8, (16, 8), 10, torch.float16)):
        assert not retrieval.ncf_supported(E, layers, k, dt), (E, layers, k, dt)
    # the edge of the LDS plan (160 KB, all of it dynamic): the largest plans that fit and
    # the smallest that do not; tests/test_gpu_ncf_topk.py launches the ones that fit
    for E, layers, k in EDGE_SHAPES:
        assert retrieval.ncf_supported(E, layers, k, f32) and retrieval.ncf_supported(E, layers, k, b16)
    for E, layers, k in ((16, (104, 120, 24), 96), (64, (128, 128, 128), 1), (64, (88, 104, 120), 1)):
        assert not retrieval.ncf_supported(E, layers, k, f32), (E, layers, k)
    assert retrieval.ncf_default_splits(0, 100) == 1 and retrieval.ncf_default_splits(5, 0) == 1
    assert 1 <= retrieval.ncf_default_splits(TU + 1, T5) <= 4  # never more splits than tiles


def test_ncf_recommend_on_a_cpu_model_is_recommend_by_forward(monkeypatch):
    """A CPU model never takes the new path: ``recommend`` equals ``recommend_by_forward``
    bit for bit, with the switch on or off, and leaves the training flag as found."""
    from pytorchrec_amd import retrieval
    from pytorchrec_amd.model.IModel import IModel
    from test_ncf_cpu import ncf
    m = ncf(users=23, items=61)
    data = {"uid": torch.randint(0, 23, (9,), generator=torch.Generator().manual_seed(2))}
    excl, ex = random_exclusion(9, 0, 61, 11)
    calls = []
    monkeypatch.setattr(retrieval, "ncf_topk", lambda *a, **kw: calls.append(1))
    for fused in (True, False):
        monkeypatch.setattr(retrieval, "NCF_TOPK_FUSED", fused)
        for kw in (dict(), dict(exclude=ex, low=5, high=50)):
            for training in (True, False):
                m.train(training)
                got = m.recommend(data, 7, **kw)
                assert m.training == training
                want = IModel.recommend_by_forward(m, data, 7, **kw)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not calls
    with pytest.raises(ValueError):
        m.recommend(data, 0)
