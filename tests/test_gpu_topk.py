"""mrec_topk on the GPU: the fused score-and-select kernel pair (csrc/topk.hip) behind
``retrieval.topk`` and ``IModel.recommend``.

The oracle, the exact-integer inputs, ``robust_check`` and its derived tolerance are those
of tests/test_topk_cpu.py (its docstring states them).  Here:
  1. exact-integer edges: every tile boundary of queries and items, every D and k edge,
     both bank and query dtypes, operands and outputs as windows of larger allocations
     whose surroundings are NaN / 1e30 / guard values -- compared with ``torch.equal``;
  2. independence from the item-split count, from the run and from the bank's placement;
  3. the robust check on Gaussian inputs;
  4. argument errors, which launch nothing;
  5. the four dot-product models and ``evaluate_full`` on cuda:0.
"""
import numpy as np
import pytest
import torch

from test_topk_cpu import (DTYPES, EXACT_CASES, MODELS, TI, TQ, assert_exact, bf16, brute_force,
                           exact_case_seed, exact_inputs, gauss_inputs, make_bank, model_batch, oracle,
                           random_exclusion, robust_check)

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _query_window(q, dtype, dev):
    """q as a window of a larger allocation: ldq > D, NaN beyond D and below the batch."""
    B, D = q.shape
    buf = torch.full((B + 2, D + 5), NAN, dtype=dtype, device=dev)
    buf[:B, :D] = torch.from_numpy(q).to(dev)
    return buf[:B, :D]


def _run_in_windows(bank, qv, k, low, high, use_w, ex=None, splits=0):
    """One mrec_topk call into windows of guarded outputs; the guards must survive."""
    from pytorchrec_amd import retrieval
    B, dev = qv.shape[0], qv.device
    ids = torch.full((B + 3, k + 4), 7, dtype=torch.int32, device=dev)
    sc = torch.full((B + 3, k + 4), 7.0, dtype=torch.float32, device=dev)
    retrieval.topk_fused(bank, 1, qv, k, low, high, use_w, ex, splits, out_ids=ids[:B, :k],
                         out_scores=sc[:B, :k])
    assert (ids[:, k:] == 7).all() and (ids[B:] == 7).all(), "ids: a guard was written"
    assert (sc[:, k:] == 7.0).all() and (sc[B:] == 7.0).all(), "scores: a guard was written"
    return ids[:B, :k], sc[:B, :k]


# ---------------------------------------------------------------------------
# 1. exact-integer edges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(EXACT_CASES)))
def test_exact_integer_edges(gpu, case):
    B, n, D, k, bd, qd, use_w = EXACT_CASES[case]
    q, T, w, low, high = exact_inputs(B, n, D, use_w, exact_case_seed(case))
    bank = make_bank(T, w, DTYPES[bd], gpu)
    ids, sc = _run_in_windows(bank, _query_window(q, DTYPES[qd], gpu), k, low, high, use_w)
    assert_exact(ids, sc, q, T, w, k, low, high)


@pytest.mark.parametrize("bd,row_dtype", [("bf16", torch.int32), ("f32", torch.int64)])
def test_exact_exclusion_and_nan_row(gpu, bd, row_dtype):
    """A shared CSR addressed through excl_row with repeats, -1 and n_rows; a query whose
    whole range is excluded (all padding); an exclusion of exactly the would-be k-th item;
    a NaN table row, which is never returned."""
    from pytorchrec_amd.retrieval import Exclusion
    B, n, D, k = TQ + 1, 3 * TI + 5, 32, 7
    q, T, w, low, high = exact_inputs(B, n, D, True, 77)
    nan_id = low + 50
    T[nan_id] = np.nan
    plain_ids, _, _, _ = oracle(q, T, w, k, low, high)
    g = np.random.default_rng(5)
    csr = [list(range(low, high)), [int(plain_ids[1, k - 1])],
           sorted(set(g.integers(low, high, 40).tolist())), sorted(set(g.integers(low, high, 40).tolist()))]
    rows = [0, 1, -1, len(csr)] + [2 + (b % 2) for b in range(B - 4)]
    off = np.zeros(len(csr) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in csr])
    ex = Exclusion(torch.from_numpy(off), torch.from_numpy(np.concatenate(csr).astype(np.int32)),
                   torch.tensor(rows, dtype=row_dtype)).to(gpu)
    bank = make_bank(T, w, DTYPES[bd], gpu)
    for splits in (0, 1, 3):
        ids, sc = _run_in_windows(bank, _query_window(q, torch.float32, gpu), k, low, high, True, ex,
                                  splits)
        assert_exact(ids, sc, q, T, w, k, low, high, (csr, rows))
        assert (ids[0] == -1).all() and (sc[0] == float("-inf")).all()
        assert not (ids[1] == int(plain_ids[1, k - 1])).any()
        assert torch.equal(ids[2].cpu(), torch.from_numpy(plain_ids[2]))
        assert torch.equal(ids[3].cpu(), torch.from_numpy(plain_ids[3]))
        assert not (ids == nan_id).any()


def test_empty_batch_and_empty_range(gpu):
    from pytorchrec_amd import retrieval
    q, T, w, low, high = exact_inputs(5, 9, 16, False, 1)
    bank = make_bank(T, w, torch.float32, gpu)
    ids, sc = _run_in_windows(bank, _query_window(q, torch.float32, gpu), 4, low, low, False)
    assert (ids == -1).all() and (sc == float("-inf")).all()
    ids, sc = retrieval.topk(bank, 1, torch.zeros(0, 16, device=gpu), 4, low=low, high=high)
    assert ids.shape == (0, 4) and sc.shape == (0, 4)


# ---------------------------------------------------------------------------
# 2. geometry independence, repeatability, placement independence
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,bd,use_w", [("exact", "bf16", True), ("gauss", "f32", False),
                                           ("gauss", "bf16", True)])
def test_result_does_not_depend_on_geometry_run_or_placement(gpu, kind, bd, use_w):
    from pytorchrec_amd import retrieval
    B, n, D, k = TQ + 1, 3 * TI + 5, 64, 64
    q, T, w, low, high = (exact_inputs if kind == "exact" else gauss_inputs)(B, n, D, use_w, 21)
    excl, ex = random_exclusion(B, low, high, 8, per_row=30)
    bank = make_bank(T, w, DTYPES[bd], gpu)
    tq = torch.from_numpy(q).to(gpu)
    kw = dict(low=low, high=high, use_w=use_w, exclude=ex)
    first = retrieval.topk(bank, 1, tq, k, item_splits=1, **kw)
    assert retrieval.default_splits(B, n) > 1
    for splits in (1, 2, 3, None):
        again = retrieval.topk(bank, 1, tq, k, item_splits=splits, **kw)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), splits
    filler = torch.empty(12345, device=gpu)  # (moves the next allocation)
    moved = make_bank(T, w, DTYPES[bd], gpu, lead_rows=11)
    assert moved.row_offset[1] != bank.row_offset[1] and moved.weight.data_ptr() != bank.weight.data_ptr()
    other = retrieval.topk(moved, 1, tq, k, **kw)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    del filler


# ---------------------------------------------------------------------------
# 3. random parity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("bd", ["f32", "bf16"])
@pytest.mark.parametrize("D", [8, 16, 32, 64])
def test_gaussian_inputs_pass_the_robust_check(gpu, D, bd, extras, k):
    from pytorchrec_amd import retrieval
    B, n = 2 * TQ + 3, 4 * TI + 1
    use_w = extras and not (D == 64 and bd == "f32")  # (no room for w in a 256-B fp32 row)
    q, T, w, low, high = gauss_inputs(B, n, D, use_w, 100 + D + k)
    if w is not None and bd == "bf16":
        w = bf16(w)  # (what the bf16 bank holds)
    excl, ex = random_exclusion(B, low, high, 3, per_row=60) if extras else (None, None)
    bank = make_bank(T, w, DTYPES[bd], gpu)
    ids, sc = retrieval.topk(bank, 1, torch.from_numpy(q).to(gpu), k, low=low, high=high, use_w=use_w,
                             exclude=ex)
    robust_check(ids, sc, q, T, w, k, low, high, excl)


# ---------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------

def test_bad_arguments_are_value_errors_and_launch_nothing(gpu):
    from pytorchrec_amd import _mrec, retrieval
    B, n, D = 5, 300, 16
    q, T, w, low, high = exact_inputs(B, n, D, False, 4)
    bank = make_bank(T, None, torch.float32, gpu)
    tq = torch.from_numpy(q).to(gpu)
    ids = torch.full((B, 130), 7, dtype=torch.int32, device=gpu)
    sc = torch.full((B, 130), 7.0, dtype=torch.float32, device=gpu)
    need = int(_mrec.lib().mrec_topk_workspace_size(B, 8, 2))
    assert need == B * 2 * 8 * 8
    short = torch.empty(need - 1, dtype=torch.uint8, device=gpu)
    q24, T24, _, _, _ = exact_inputs(B, n, 24, False, 4)
    bank24 = make_bank(T24, None, torch.float32, gpu)
    bad = [dict(k=0), dict(k=129), dict(k=8, low=high, high=low), dict(k=8, use_w=True),
           dict(k=8, splits=2, workspace=short), dict(k=8, splits=65), dict(k=8, bank=bank24, q=q24)]
    for kw in bad:
        kw = dict(kw)
        b = kw.pop("bank", bank)
        qq = torch.from_numpy(kw.pop("q")).to(gpu) if "q" in kw else tq
        k = kw.pop("k")
        lo, hi = kw.pop("low", low), kw.pop("high", high)
        with pytest.raises(ValueError, match="MREC_EINVAL"):
            retrieval.topk_fused(b, 1, qq, k, lo, hi, kw.pop("use_w", False), None, kw.pop("splits", 0),
                                 out_ids=ids[:, :max(k, 1)], out_scores=sc[:, :max(k, 1)], **kw)
    torch.cuda.synchronize()
    assert (ids == 7).all() and (sc == 7.0).all()
    # a workspace of exactly the size works
    exact = torch.empty(need, dtype=torch.uint8, device=gpu)
    got = retrieval.topk_fused(bank, 1, tq, 8, low, high, False, None, 2, workspace=exact)
    assert_exact(got[0], got[1], q, T, None, 8, low, high)


def test_unsupported_dim_takes_the_torch_path_on_the_gpu(gpu):
    from pytorchrec_amd import retrieval
    B, n, D, k = 9, 200, 24, 12
    q, T, w, low, high = exact_inputs(B, n, D, True, 12)
    assert not retrieval.supported(D, k, torch.float32) and not retrieval.supported(16, 129, torch.float32)
    bank = make_bank(T, w, torch.float32, gpu)
    excl, ex = random_exclusion(B, low, high, 2)
    ids, sc = retrieval.topk(bank, 1, torch.from_numpy(q).to(gpu), k, low=low, high=high, use_w=True,
                             exclude=ex)
    assert ids.is_cuda and ids.dtype == torch.int32
    assert_exact(ids, sc, q, T, w, k, low, high, excl)


# ---------------------------------------------------------------------------
# 5. the models on cuda:0
# ---------------------------------------------------------------------------

def _gpu_model(kind, gpu, emb_dtype):
    m = MODELS[kind](D=16, emb_dtype=emb_dtype) if kind != "funksvd" else None
    if m is None:
        from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity as C
        from pytorchrec_amd.model import FunkSVD
        m = FunkSVD(C(23, "uid"), C(61, "iid"), C(2, "label"), emb_size=16, emb_dtype=emb_dtype,
                    random_seed=7)
    return m.to(gpu)


@pytest.mark.parametrize("kind,emb_dtype", [("funksvd", torch.float32), ("svdpp", torch.bfloat16),
                                            ("sasrec", torch.float32), ("gru4rec", torch.bfloat16)])
def test_models_recommend_on_the_gpu(gpu, kind, emb_dtype):
    """recommend passes the robust check against the oracle built from the model's own
    query and table (read back to the host), and agrees with the generic path through
    forward within the bars of a GPU forward (test_gpu_gru4rec._meets_bars)."""
    from test_gpu_gru4rec import _errs, _meets_bars
    from pytorchrec_amd.model.IModel import IModel
    m = _gpu_model(kind, gpu, emb_dtype)
    items, B, k = 61, TQ + 5, 10
    data = model_batch(kind, B, items, device=gpu)
    excl, ex = random_exclusion(B, 0, items, 6, per_row=12)
    ids, sc = m.recommend(data, k, exclude=ex)
    assert ids.is_cuda and ids.dtype == torch.int32 and sc.dtype == torch.float32
    m.eval()
    with torch.no_grad():
        q, bank, table, use_w, const = m._retrieval_query(data)
    T = bank.table(table).detach().float().cpu().numpy()
    w = bank.first_order(table).detach().float().cpu().numpy() if use_w else None
    low = 1 if kind == "sasrec" else 0
    robust_check(ids, sc, q.float().cpu().numpy(), T, w, k, low, items, excl,
                 None if const is None else const.detach().float().cpu().numpy())
    # the generic path scores the same items through forward
    ids2, sc2 = IModel.recommend_by_forward(m, data, k, exclude=ex, chunk=16)
    want = sc2.double().cpu()
    _meets_bars({(True, "prediction"): _errs(sc, want), (False, "prediction"): (0.0, 0.0)}, ["prediction"])
    bar = 3e-2 * float(want.abs().max())
    w_np = want.numpy()
    gap_prev = np.abs(np.diff(w_np, axis=1, prepend=np.inf))
    gap_next = np.abs(np.diff(w_np, axis=1, append=-np.inf))
    clear = (gap_prev > 2 * bar) & (gap_next > 2 * bar)
    assert np.array_equal(ids.cpu().numpy()[clear], ids2.cpu().numpy()[clear])


def test_sasrec_never_returns_the_padding_item_and_history_exclusion_is_exact(gpu):
    from pytorchrec_amd.retrieval import Exclusion
    m = _gpu_model("sasrec", gpu, torch.float32)
    items, B = 61, 7
    data = model_batch("sasrec", B, items, device=gpu)
    ids, sc = m.recommend(data, items)
    assert not (ids == 0).any() and (ids[:, :items - 1] > 0).all() and (ids[:, -1] == -1).all()
    ids, sc = m.recommend(data, items, exclude=Exclusion.from_lists(data["his"], pad=0))
    his = data["his"].cpu().numpy()
    for b in range(B):
        want = set(range(1, items)) - set(his[b].tolist())
        got = ids[b].cpu().numpy()
        assert set(got[got >= 0].tolist()) == want and (got >= 0).sum() == len(want)


def test_evaluate_full_matches_the_host_metrics(gpu):
    """NDCG@10 and Hit@10 over 40 users in batches of 16 == the host computation from the
    recommended lists of one call."""
    m = _gpu_model("funksvd", gpu, torch.float32)
    users, items, k = 23, 61, 10
    g = torch.Generator().manual_seed(1)
    uid = torch.randint(0, users, (40,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, items, (40,), generator=g, dtype=torch.int32)
    rows = [{"uid": u, "iid": i} for u, i in zip(uid, pos)]
    got = m.evaluate_full(rows, batch_size=16, k=k, pos_column=m.iid_column)
    ids, _ = m.recommend({"uid": uid.to(gpu)}, k)
    ids, p = ids.cpu().numpy(), pos.numpy()
    ranks = np.array([(np.flatnonzero(ids[b] == p[b])[0] + 1) if (ids[b] == p[b]).any() else k + 1
                      for b in range(40)])
    hit = ranks <= k
    assert abs(got[f"hit@{k}"] - hit.mean()) < 1e-12
    assert abs(got[f"ndcg@{k}"] - (1 / np.log2(ranks[hit] + 1)).sum() / 40) < 1e-12
    assert 0 < hit.sum() < 40
