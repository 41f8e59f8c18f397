"""GPU parity of the pooled multi-valued lookup (mrec_emb_pool_fwd and the bag
indirection of the embedding backward) and of the SVD++ model built on it.

Bars: the forward within the sequential fp32 sum's error bound of the fp64 value
((L + 2) 2^-24 of the sum of magnitudes, + one bf16 rounding for bf16 outputs); the
backward bitwise equal to the existing backward over the expanded gradient, on every
plan layout; dense gradients within the fp32 reordering tolerance of fp64 autograd;
the SVD++ model on the reference's own numbers (G4, G13).
"""
import numpy as np
import pytest
import torch

from conftest import golden
from test_pool_cpu import G13_KEYS, g4_magnitude, g4_state, svdpp

pytestmark = pytest.mark.gpu


def _bank(nums, dim, has_w, dtype, seed=0, scale=0.5):
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.embedding import EmbeddingBank
    assert _mrec.available(), "libmrec.so must be built and loadable on the GPU box"
    b = EmbeddingBank(nums, dim, with_first_order=has_w, dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        b.weight.copy_((torch.randn(b.weight.shape, generator=g) * scale).to(dtype))
    return b.zero_pad_()


def _clone_bank(src):
    from pytorchrec_amd.embedding import EmbeddingBank
    b = EmbeddingBank(src.category_nums, src.dim, with_first_order=src.has_w,
                      dtype=src.weight.dtype, device="cuda")
    with torch.no_grad():
        b.weight.copy_(src.weight)
    return b


def _bags(rng, B, L, rows, pad, zipf=False):
    """[B, L] ids per table: lengths 0..L (bag 0 empty, bag 1 full with a duplicate)."""
    out = []
    for r in rows:
        lo = 1 if pad == "zero" else 0
        if zipf:
            t = np.minimum(rng.zipf(1.3, (B, L)) - 1 + lo, r - 1)
        else:
            t = rng.integers(lo, r, (B, L))
        lens = rng.integers(0, L + 1, B)
        lens[0], lens[1] = 0, L
        t[np.arange(L)[None, :] >= lens[:, None]] = 0 if pad == "zero" else -1
        if L > 1:
            t[1, 1] = t[1, 0]
        out.append(t.astype(np.int64))
    return out


def _valid(t, pad):
    return t > 0 if pad == "zero" else t >= 0


def _scale64(n, mode):
    n = n.astype(np.float64)
    safe = np.maximum(n, 1.0)
    s = {"sum": np.ones_like(n), "mean": 1.0 / safe, "sqrtn": 1.0 / np.sqrt(safe)}[mode]
    return np.where(n > 0, s, 0.0)


def _pool64(bank, ids_np, mode, pad):
    """fp64 from the exactly widened bank: pooled [B, F*D], w [B, F], scale [B, F] and
    s * sum_j |v_j| for both."""
    W = bank.weight.detach().double().cpu().numpy()
    D = bank.dim
    v, w, s_all, mv, mw = [], [], [], [], []
    for f, t in enumerate(ids_np):
        ok = _valid(t, pad)
        rows = W[np.where(ok, t, 0) + bank.row_offset[f]] * ok[..., None]
        s = _scale64(ok.sum(1), mode)
        v.append(rows.sum(1)[:, :D] * s[:, None])
        mv.append(np.abs(rows).sum(1)[:, :D] * s[:, None])
        if bank.has_w:
            w.append(rows.sum(1)[:, D] * s)
            mw.append(np.abs(rows).sum(1)[:, D] * s)
        s_all.append(s)
    cat = (lambda xs: np.concatenate(xs, 1))
    stk = (lambda xs: np.stack(xs, 1) if xs else None)
    return cat(v), stk(w), stk(s_all), cat(mv), stk(mw)


GEOMETRIES = [  # every bank row width
    pytest.param(torch.bfloat16, 8, False, id="bf16-D8-16B"),
    pytest.param(torch.float32, 4, True, id="f32-D4w-32B"),
    pytest.param(torch.bfloat16, 16, True, id="bf16-D16w-64B"),
    pytest.param(torch.float32, 16, True, id="f32-D16w-128B"),
    pytest.param(torch.float32, 32, True, id="f32-D32w-256B"),
]


@pytest.mark.parametrize("dtype,D,has_w", GEOMETRIES)
@pytest.mark.parametrize("mode", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("pad", ["zero", "negative"])
def test_pool_forward_matches_fp64(gpu, dtype, D, has_w, mode, pad):
    """F = 2, B = 37, L = 9, tables of 37 and 5 rows (bags hold duplicates), int32 and
    int64 ids, fp32 and bf16 outputs, the pooled first-order weights, and the per-bag
    scale the backward uses (read from the autograd node)."""
    from pytorchrec_amd.embedding import pooled_gather
    B, L, nums = 37, 9, [37, 5]
    rng = np.random.default_rng(D * 10 + len(mode))
    bank = _bank(nums, D, has_w, dtype, seed=D)
    assert bank.row_stride * bank.weight.element_size() == {
        (torch.bfloat16, 8): 16, (torch.float32, 4): 32, (torch.bfloat16, 16): 64,
        (torch.float32, 16): 128, (torch.float32, 32): 256}[(dtype, D)]
    ids_np = _bags(rng, B, L, nums, pad)
    want, want_w, s64, mag, mag_w = _pool64(bank, ids_np, mode, pad)
    bank.use_fused_sgd(0.0)  # (so the node keeps the scale; lr 0: nothing moves)
    for id_dtype in (torch.int32, torch.int64):
        ids = [torch.from_numpy(t).to(gpu, id_dtype) for t in ids_np]
        for out_dtype in (torch.float32, torch.bfloat16):
            res = pooled_gather(bank, ids, mode=mode, pad=pad, out_dtype=out_dtype, with_w=has_w)
            out, w = res if has_w else (res, None)
            assert out.dtype == out_dtype and out.shape == (B, 2 * D)
            got = out.detach().float().cpu().numpy().astype(np.float64)
            bound = (L + 2) * 2.0 ** -24 * mag
            if out_dtype == torch.bfloat16:
                bound = bound + 2.0 ** -8 * np.abs(want)
            err = np.abs(got - want)
            assert np.all(err <= bound), (id_dtype, out_dtype, float((err - bound).max()))
            assert np.all(got[0] == 0)  # the empty bag: a zero row, not NaN
            if has_w:
                gw = w.detach().cpu().numpy().astype(np.float64)
                assert np.all(np.abs(gw - want_w) <= (L + 2) * 2.0 ** -24 * mag_w)
            s = out.grad_fn.scale.cpu().numpy()
            s32 = s64.astype(np.float32)
            assert np.all(np.abs(s.astype(np.float64) - s32) <= np.spacing(s32)), mode
            assert np.all(s[0] == 0) and np.all(s[s64 == 0] == 0)
            if mode == "sum":
                assert np.all(s[s64 > 0] == 1)


@pytest.mark.parametrize("dtype,D,has_w", GEOMETRIES)
def test_pool_single_id_bags_equal_gather_bitwise(gpu, dtype, D, has_w):
    """L = 1, sum, no padding, out dtype = bank dtype: the rows themselves."""
    from pytorchrec_amd.embedding import gather, pooled_gather
    nums, B = [37, 5], 41
    rng = np.random.default_rng(1)
    bank = _bank(nums, D, has_w, dtype, seed=2)
    with torch.no_grad():
        bank.weight[3, 0] = -0.0  # a negative zero survives the sum
    ids_np = [rng.integers(1, n, (B, 1)) for n in nums]
    ids_np[0][0, 0] = 3
    ids = [torch.from_numpy(t).to(gpu) for t in ids_np]
    with torch.no_grad():
        pooled = pooled_gather(bank, ids, mode="sum", pad="zero", with_w=has_w)
        plain = gather(bank, [t[:, 0].contiguous() for t in ids], with_w=has_w)
    if has_w:
        assert torch.equal(pooled[1].view(torch.int32), plain[1].view(torch.int32))
        pooled, plain = pooled[0], plain[0]
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(pooled.view(bits), plain.view(bits))


def test_pool_reads_strided_ids_in_place(gpu):
    from pytorchrec_amd.embedding import pooled_gather
    B, L, nums = 37, 9, [37, 5]
    rng = np.random.default_rng(4)
    bank = _bank(nums, 8, False, torch.float32)
    wide = [torch.from_numpy(np.concatenate([t, rng.integers(1, 5, (B, L))], 1)).to(gpu)
            for t in _bags(rng, B, L, nums, "zero")]
    views = [t[:, :L] for t in wide]
    assert views[0].stride() == (2 * L, 1) and not views[0].is_contiguous()
    from pytorchrec_amd import _mrec
    assert _mrec.IdsDesc.bags(views).struct.stride == 2 * L  # the view itself, no copy
    with torch.no_grad():
        got = pooled_gather(bank, views, mode="sqrtn")
        want = pooled_gather(bank, [v.contiguous() for v in views], mode="sqrtn")
    assert torch.equal(got, want)


def test_pool_out_of_range_ids(gpu):
    from pytorchrec_amd.embedding import pooled_gather
    rows = 7
    bank = _bank([rows], 8, False, torch.float32)
    good = torch.tensor([[1, 2, 3], [4, 0, 0]], device=gpu)
    for bad_id, pad in ((rows, "zero"), (rows, "negative"), (-1, "zero")):
        ids = good.clone()
        ids[0, 1] = bad_id
        with pytest.raises(IndexError):
            pooled_gather(bank, [ids], mode="sum", pad=pad)
    bank.check_ids = False
    ids = good.clone()
    ids[0, 1] = rows + 100000
    with torch.no_grad():
        out = pooled_gather(bank, [ids], mode="sum", pad="zero")
        skipped = pooled_gather(bank, [torch.tensor([[1, 0, 3], [4, 0, 0]], device=gpu)],
                                mode="sum", pad="zero")
    assert torch.isfinite(out).all() and torch.equal(out, skipped)


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,L", [(64, 9), (100, 50), (300, 50)],
                         ids=["hash-576", "sorted-5000", "large-15000"])
@pytest.mark.parametrize("update", ["sgd", "dense"])
@pytest.mark.parametrize("bank_dtype,out_dtype", [(torch.float32, torch.float32),
                                                  (torch.float32, torch.bfloat16),
                                                  (torch.bfloat16, torch.bfloat16)],
                         ids=["f32-f32", "f32-bf16", "bf16-bf16"])
def test_pool_backward_equals_expanded_gather_backward_bitwise(gpu, B, L, update, bank_dtype,
                                                               out_dtype):
    """pooled_gather + backward against gather(flat lookup ids, pad_negative) +
    backward of the expanded gradient (dout * scale repeated L times): the tables
    (fused SGD, RNE) or the dense gradients are bit-identical, on the hash layout, the
    sorted layout and the large-batch path."""
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.embedding import gather, pooled_gather
    assert (B * L <= _mrec.BWD_HASH_MAX_BATCH, B * L <= _mrec.BWD_MAX_BATCH) == {
        576: (True, True), 5000: (False, True), 15000: (False, False)}[B * L]
    nums, D = [1000, 37], 8
    rng = np.random.default_rng(B * L)
    a = _bank(nums, D, False, bank_dtype, seed=5)
    b = _clone_bank(a)
    for bank in (a, b):
        bank.stochastic_rounding = False  # RNE: no random bits in the comparison
        if update == "sgd":
            bank.use_fused_sgd(0.25)
    ids_np = _bags(rng, B, L, nums, "zero")
    ids = [torch.from_numpy(t).to(gpu, torch.int32) for t in ids_np]
    dout = torch.from_numpy(rng.standard_normal((B, 2 * D)).astype(np.float32)).to(gpu, out_dtype)
    out = pooled_gather(a, ids, mode="sqrtn", pad="zero", out_dtype=out_dtype)
    node = out.grad_fn
    scale, lookup = node.scale, [t.clone() for t in node.ids]
    for f in range(2):  # the padded id view the plan consumes
        want = np.where(ids_np[f] > 0, ids_np[f], -1).reshape(-1)
        assert np.array_equal(lookup[f].cpu().numpy(), want)
    out.backward(dout)
    expanded = torch.cat([dout[:, f * D:(f + 1) * D].float() * scale[:, f:f + 1] for f in range(2)],
                         1).repeat_interleave(L, 0)
    gather(b, lookup, out_dtype=torch.float32, pad_negative=True).backward(expanded)
    torch.cuda.synchronize()
    if update == "sgd":
        ga, gb, before = a.weight, b.weight, _bank(nums, D, False, bank_dtype, seed=5).weight
        assert not torch.equal(ga, before)
    else:
        ga, gb = a.weight.grad, b.weight.grad
        assert ga.abs().sum() > 0
    bits = torch.int16 if bank_dtype == torch.bfloat16 else torch.int32
    assert torch.equal(ga.view(bits), gb.view(bits))


@pytest.mark.parametrize("B,L,zipf", [(64, 9, False), (100, 50, True), (300, 50, True)],
                         ids=["hash", "sorted-zipf", "large-zipf"])
def test_pool_dense_grad_matches_fp64_autograd(gpu, B, L, zipf):
    """embedding -> mask -> sum -> scale in fp64 torch autograd on the CPU; the Zipf
    cases hold rows hit far more than 16 times (the workgroup / fixed-point sums)."""
    from pytorchrec_amd.embedding import pooled_gather
    nums, D = [200, 37], 8
    rng = np.random.default_rng(7 + B)
    bank = _bank(nums, D, True, torch.float32, seed=8)
    ids_np = _bags(rng, B, L, nums, "zero", zipf=zipf)
    if zipf:
        assert max(np.bincount(t[t > 0]).max() for t in ids_np) > 16
    dout = rng.standard_normal((B, 2 * D)).astype(np.float32)
    ids = [torch.from_numpy(t).to(gpu) for t in ids_np]
    out = pooled_gather(bank, ids, mode="sqrtn", pad="zero")
    out.backward(torch.from_numpy(dout).to(gpu))
    got = bank.weight.grad.cpu().numpy().astype(np.float64)
    W = bank.weight.detach().double().cpu().requires_grad_()
    parts, mag = [], np.zeros_like(got)  # mag: the sum of |s * dout| over a row's lookups
    for f, t in enumerate(ids_np):
        tt = torch.from_numpy(t)
        ok = (tt > 0).double()
        rows = W[torch.where(tt > 0, tt, torch.zeros_like(tt)) + bank.row_offset[f]]
        n = ok.sum(1)
        s = torch.where(n > 0, 1.0 / n.clamp(min=1).sqrt(), torch.zeros_like(n))
        parts.append((rows * ok.unsqueeze(-1)).sum(1)[:, :D] * s.unsqueeze(-1))
        term = np.abs(s.numpy()[:, None] * dout[:, f * D:(f + 1) * D].astype(np.float64))
        sel = (t > 0).reshape(-1)
        np.add.at(mag[:, :D], t.reshape(-1)[sel] + bank.row_offset[f], np.repeat(term, L, 0)[sel])
    (torch.cat(parts, 1) * torch.from_numpy(dout).double()).sum().backward()
    want = W.grad.numpy()
    assert np.abs(want).sum() > 0
    assert np.all(np.abs(got - want) <= 1e-6 * mag + 1e-30)
    assert np.all(got[0] == 0) and np.all(got[bank.row_offset[1]] == 0)  # the PAD rows


def test_pool_backward_bag_aligned_chunks(gpu, monkeypatch):
    """A bank past LARGE_MAX_ROWS with B * L > BWD_MAX_BATCH: plan / apply pairs over
    whole bags ((8192 // 50) * 50 lookups each), one fused SGD step per chunk.
    (Gradients of ~1e-3 on weights of ~0.5: an fp32 row sum of ~30 such terms is off
    by ~1e-10, far inside atol 1e-8; with O(1) updates a weight that cancels to ~1e-4
    would carry the 3e-8 rounding of its O(1) operands, which no fp32 update meets.)"""
    from pytorchrec_amd import _mrec, embedding
    monkeypatch.setattr(embedding, "LARGE_MAX_ROWS", 0)
    B, L, nums, D, lr = 300, 50, [500], 8, 0.25
    rng = np.random.default_rng(11)
    bank = _bank(nums, D, False, torch.float32, seed=9)
    w0 = bank.weight.detach().double().cpu().numpy()
    bank.use_fused_sgd(lr)
    ids_np = _bags(rng, B, L, nums, "zero")
    dout = (rng.standard_normal((B, D)) * 1e-3).astype(np.float32)
    out = embedding.pooled_gather(bank, [torch.from_numpy(ids_np[0]).to(gpu)], mode="sqrtn")
    out.backward(torch.from_numpy(dout).to(gpu))
    t = ids_np[0]
    s = _scale64((t > 0).sum(1), "sqrtn")
    want = w0.copy()
    bags = _mrec.BWD_MAX_BATCH // L
    assert 0 < bags < B
    for b0 in range(0, B, bags):  # fp64 SGD over the same chunks
        g = np.zeros_like(want)
        tt = t[b0:b0 + bags]
        term = np.repeat(s[b0:b0 + bags, None] * dout[b0:b0 + bags].astype(np.float64), L, 0)
        sel = (tt > 0).reshape(-1)
        np.add.at(g, tt.reshape(-1)[sel], term[sel])
        want -= lr * g
    np.testing.assert_allclose(bank.weight.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-8)
    with pytest.raises(ValueError):
        embedding._backward_into_bank(bank, None, 2 * (_mrec.BWD_MAX_BATCH + 1), None,
                                      bag=(_mrec.BWD_MAX_BATCH + 1, None))


def test_pool_fused_adam_matches_dense_adam(gpu):
    """Fused (lazy) Adam with L2 decay on a 64-row table: step 2's bags hold rows step 1
    did not touch, step 3 returns to step 1's rows.  Dense Adam moves every row at every
    step, and the loss is quadratic in the pooled vectors, so the forward has to read
    each stale row as of the last step (adam_current) for the gradients to agree."""
    from pytorchrec_amd.embedding import pooled_gather
    rows, D, B, L, lr = 64, 8, 24, 6, 0.05
    rng = np.random.default_rng(13)
    bank = _bank([rows], D, False, torch.float32, seed=10, scale=0.3)
    W = bank.weight.detach().double().cpu().clone().requires_grad_()
    opt = torch.optim.Adam([W], lr=lr, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05)
    bank.use_fused_optimizer("adam", {"lr": lr}, eps=1e-8, betas=(0.8, 0.99), weight_decay=0.05)
    halves = [(1, 32), (32, 64), (1, 32)]
    for lo, hi in halves:
        t = rng.integers(lo, hi, (B, L))
        t[np.arange(L)[None, :] >= rng.integers(1, L + 1, B)[:, None]] = 0
        c = rng.standard_normal((B, D))
        out = pooled_gather(bank, [torch.from_numpy(t).to(gpu)], mode="sqrtn", pad="zero")
        (0.5 * (out.double() - torch.from_numpy(c).to(gpu)) ** 2).sum().backward()
        tt = torch.from_numpy(t)
        ok = (tt > 0).double()
        pooled = (W[tt] * ok.unsqueeze(-1)).sum(1) / ok.sum(1).sqrt().unsqueeze(-1)
        opt.zero_grad()
        (0.5 * (pooled - torch.from_numpy(c)) ** 2).sum().backward()
        opt.step()
    bank.flush_optimizer()
    got = bank.weight.detach().cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, W.detach().numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# SVD++
# ---------------------------------------------------------------------------

def test_svdpp_prediction_matches_reference_g4_gpu(gpu):
    g = golden("g4_svdpp.npz")
    m = svdpp()
    m.load_state_dict(g4_state(g))
    m = m.to(gpu).eval()
    with torch.no_grad():
        pred, _ = m({"uid": torch.from_numpy(g["uid"]).to(gpu),
                     "iid": torch.from_numpy(g["iid"]).to(gpu),
                     "iids": torch.from_numpy(g["his"]).to(gpu)})
    err = np.abs(pred.cpu().numpy() - g["prediction"])
    assert np.all(err <= 1e-5 * (g4_magnitude(g) + 1e-30))


def test_svdpp_train_step_matches_reference_g13_gpu(gpu):
    """One IModel.train_step under compile(SGD): both banks train by the fused
    row-sparse SGD and land on the reference's own 'after' tables (G10 tolerance);
    rows no id touched keep their bits, the implicit table's PAD row 0 among them."""
    g = golden("g13_svdpp_sgd_step.npz")
    m = svdpp()
    m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), torch.nn.MSELoss(), [], gpu)
    assert m.embeddings.update == "sgd" and m.implicit_i_embeddings.update == "sgd"
    batch = {k: torch.from_numpy(g[k]) for k in ("uid", "iid", "iids", "label")}
    loss = float(m.train_step(batch)["loss"].detach())
    want = float(g["loss"])
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    sd = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    for key, k in G13_KEYS:
        np.testing.assert_allclose(sd[key], g[k + "_after"], rtol=1e-5, atol=1e-8, err_msg=key)
    touched = {"u": g["uid"], "i": g["iid"], "ub": g["uid"], "ib": g["iid"],
               "imp": g["iids"][g["iids"] > 0]}
    for key, k in G13_KEYS[:5]:
        rows = g[k + "_before"].shape[0]
        keep = np.setdiff1d(np.arange(rows), touched[k])
        assert keep.size and (k != "imp" or 0 in keep)
        assert np.array_equal(sd[key][keep].view(np.uint32), g[k + "_before"][keep].view(np.uint32)), key
        assert not np.array_equal(sd[key], g[k + "_before"]), key


def test_svdpp_sampled_branch_trains_gpu(gpu):
    """iid [B, N]: the history is pooled once per sample and repeated per candidate;
    one SGD step against the same model in fp64 torch autograd."""
    g = golden("g4_svdpp.npz")
    m = svdpp()
    state = g4_state(g)
    m.load_state_dict(state)
    lr, B, N = 0.5, 32, 4
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), torch.nn.MSELoss(), [], gpu)
    rng = np.random.default_rng(17)
    uid, his = torch.from_numpy(g["uid"][:B]).long(), torch.from_numpy(g["his"][:B]).long()
    iid = torch.from_numpy(rng.integers(0, 37, (B, N)))
    m.eval()
    with torch.no_grad():
        pred, tgt = m({"uid": uid.to(gpu), "iid": iid.to(gpu), "iids": his.to(gpu)})
    assert pred.shape == (B, N) and torch.equal(tgt[:, 0], torch.ones(B, device=gpu))
    assert float(tgt[:, 1:].abs().sum()) == 0
    m.train_step({"uid": uid, "iid": iid, "iids": his})
    P = {k: v.double().clone().requires_grad_() for k, v in state.items()}
    ok = (his > 0).double()
    imp = (P["implicit_i_embeddings.weight"][his] * ok.unsqueeze(-1)).sum(1) / ok.sum(1).sqrt()[:, None]
    u = P["u_embeddings.weight"][uid] + imp
    p64 = ((u[:, None, :] * P["i_embeddings.weight"][iid]).sum(-1) + P["u_bias.weight"][uid]
           + P["i_bias.weight"][iid][..., 0] + P["global_bias"])
    np.testing.assert_allclose(pred.cpu().numpy(), p64.detach().numpy(), rtol=1e-5, atol=1e-6)
    target = torch.zeros(B, N, dtype=torch.float64)
    target[:, 0] = 1
    ((p64 - target) ** 2).mean().backward()
    sd = m.state_dict()
    for k, p in P.items():
        want = (p - lr * p.grad).detach().numpy()
        np.testing.assert_allclose(sd[k].cpu().numpy(), want, rtol=1e-5, atol=1e-8, err_msg=k)
