"""Pooled multi-valued lookups and the SVD++ model on the CPU (no GPU needed):
``pooled_gather`` on a CPU bank against fp64 numpy, the registry entry, the
reference's checkpoint keys and RNG order (G13 'before'), the reference's own
prediction (G4) and one reference train step (G13).  The GPU runs of the same
properties are in test_gpu_pool.py."""
import numpy as np
import pytest
import torch

from conftest import golden


def _bank(rows, dim, with_w, seed=0):
    from pytorchrec_amd.embedding import EmbeddingBank
    bank = EmbeddingBank(rows, dim, with_first_order=with_w)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bank.weight.copy_(torch.randn(bank.weight.shape, generator=g))
    return bank.zero_pad_()


def pool_ref(bank, ids, mode, pad):
    """fp64: (pooled vectors [B, F*D], pooled w [B, F], scale [B, F], sum of |terms|)."""
    W = bank.weight.detach().double().numpy()
    D = bank.dim
    vs, ws, ss, mags = [], [], [], []
    for f, t in enumerate(ids):
        t = t.numpy().astype(np.int64)
        valid = t > 0 if pad == "zero" else t >= 0
        rows = W[np.where(valid, t, 0) + bank.row_offset[f]] * valid[..., None]
        n = valid.sum(1)
        with np.errstate(divide="ignore"):
            s = {"sum": (n > 0) * 1.0, "mean": np.where(n > 0, 1.0 / np.maximum(n, 1), 0.0),
                 "sqrtn": np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1)), 0.0)}[mode]
        vs.append(rows.sum(1)[:, :D] * s[:, None])
        ws.append(rows.sum(1)[:, D] * s if bank.has_w else np.zeros(len(t)))
        mags.append(np.abs(rows).sum(1)[:, :D] * s[:, None])
        ss.append(s)
    return (np.concatenate(vs, 1), np.stack(ws, 1), np.stack(ss, 1), np.concatenate(mags, 1))


def _bags(B, L, rows, pad, seed):
    rng = np.random.default_rng(seed)
    ids = []
    for r in rows:
        t = rng.integers(1 if pad == "zero" else 0, r, (B, L))
        lens = rng.integers(0, L + 1, B)
        lens[0], lens[1] = 0, L                      # an empty bag, a full one
        t[np.arange(L)[None, :] >= lens[:, None]] = 0 if pad == "zero" else -1
        t[1, 1] = t[1, 0]                            # a duplicate id inside a bag
        ids.append(torch.from_numpy(t))
    return ids


@pytest.mark.parametrize("mode", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("pad", ["zero", "negative"])
def test_pooled_gather_cpu_matches_fp64(mode, pad):
    from pytorchrec_amd.embedding import pooled_gather
    bank = _bank([37, 5], 8, True)
    B, L = 12, 9
    ids = _bags(B, L, bank.category_nums, pad, seed=3)
    out, w = pooled_gather(bank, ids, mode=mode, pad=pad, with_w=True)
    assert out.shape == (B, 2 * 8) and w.shape == (B, 2)
    want, want_w, _, mag = pool_ref(bank, ids, mode, pad)
    assert np.all(np.abs(out.detach().numpy() - want) <= (L + 2) * 2.0 ** -24 * mag + 1e-30)
    np.testing.assert_allclose(w.detach().numpy(), want_w, rtol=1e-5, atol=1e-6)
    assert np.all(out.detach().numpy()[0] == 0)      # the empty bag: a zero row
    # the duplicate counts twice, the empty bag gets no gradient
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(dout)
    g = bank.weight.grad.double().numpy()
    _, _, s, _ = pool_ref(bank, ids, mode, pad)
    want_g = np.zeros_like(g)
    for f, t in enumerate(ids):
        t = t.numpy()
        for b in range(B):
            for j in range(L):
                if (t[b, j] > 0) if pad == "zero" else (t[b, j] >= 0):
                    want_g[bank.row_offset[f] + t[b, j], :8] += (
                        s[b, f] * dout[b, f * 8:(f + 1) * 8].double().numpy())
    np.testing.assert_allclose(g, want_g, rtol=1e-5, atol=1e-6)
    dup = bank.row_offset[0] + int(ids[0][1, 0])
    assert np.any(g[dup] != 0)


def test_pooled_gather_cpu_out_of_range_raises():
    from pytorchrec_amd.embedding import pooled_gather
    bank = _bank([7], 8, False)
    ids = torch.tensor([[1, 2, 7]])
    with pytest.raises(IndexError):
        pooled_gather(bank, [ids])
    with pytest.raises(IndexError):                  # a negative id is no padding under "zero"
        pooled_gather(bank, [torch.tensor([[1, -1, 0]])], pad="zero")
    out = pooled_gather(bank, [torch.tensor([[1, -1, 0]])], pad="negative")
    want = (bank.weight[1, :8] + bank.weight[0, :8]).detach()
    np.testing.assert_allclose(out[0].detach().numpy(), want.numpy(), rtol=1e-6)


def test_pooled_gather_rejects_a_sharded_bank_and_bad_arguments():
    from pytorchrec_amd.embedding import pooled_gather
    bank = _bank([7], 8, False)
    with pytest.raises(ValueError):
        pooled_gather(bank, [torch.zeros(3, 2, dtype=torch.int64)], mode="max")
    with pytest.raises(ValueError):
        pooled_gather(bank, [torch.zeros(3, dtype=torch.int64)])
    with pytest.raises(ValueError):
        pooled_gather(bank, [torch.zeros(3, 2, dtype=torch.int64)], with_w=True)


# ---------------------------------------------------------------------------
# SVD++
# ---------------------------------------------------------------------------

REF_KEYS = {"u_embeddings.weight", "i_embeddings.weight", "implicit_i_embeddings.weight",
            "u_bias.weight", "i_bias.weight", "global_bias"}
G13_KEYS = (("u_embeddings.weight", "u"), ("i_embeddings.weight", "i"),
            ("implicit_i_embeddings.weight", "imp"), ("u_bias.weight", "ub"),
            ("i_bias.weight", "ib"), ("global_bias", "gb"))


def svdpp(device=None):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import SVDPP
    m = SVDPP(CategoricalColumnWithIdentity(50, "uid"), CategoricalColumnWithIdentity(37, "iid"),
              CategoricalColumnWithIdentity(37, "iids"), CategoricalColumnWithIdentity(2, "label"),
              emb_size=8, random_seed=2020)
    return m.to(device) if device is not None else m


def g4_state(g):
    return {"u_embeddings.weight": torch.from_numpy(g["u_table"]),
            "i_embeddings.weight": torch.from_numpy(g["i_table"]),
            "implicit_i_embeddings.weight": torch.from_numpy(g["imp_table"]),
            "u_bias.weight": torch.from_numpy(g["ub_table"]),
            "i_bias.weight": torch.from_numpy(g["ib_table"]),
            "global_bias": torch.tensor(float(g["global_bias"]))}


def g4_magnitude(g):
    """sum_d |u + imp| |i| + |ub| + |ib| + |gb| in fp64 (the rule of
    test_funksvd_sampled_branch_matches_reference_g11, extended by the added terms)."""
    u = g["u_table"].astype(np.float64)[g["uid"]]
    i = g["i_table"].astype(np.float64)[g["iid"]]
    his = g["his"]
    valid = his > 0
    imp = (g["imp_table"].astype(np.float64)[his] * valid[..., None]).sum(1)
    imp /= np.sqrt(valid.sum(1))[:, None]
    return ((np.abs(u + imp) * np.abs(i)).sum(-1) + np.abs(g["ub_table"][g["uid"], 0])
            + np.abs(g["ib_table"][g["iid"], 0]) + abs(float(g["global_bias"])))


def test_svdpp_is_registered():
    from pytorchrec_amd.model import SVDPP, get_model_type
    assert get_model_type("svdpp") is SVDPP
    names = [a.name for a in SVDPP.get_argument_descriptions()]
    assert names == ["emb_size"]
    SVDPP.check_argument_values({"emb_size": 8})
    with pytest.raises(AssertionError):
        SVDPP.check_argument_values({"emb_size": 0})


def test_svdpp_init_and_keys_match_reference_g13():
    """Seed 2020 -> exactly the six reference keys, tables bit-identical to the
    reference's own initialisation (the RNG is consumed in its order)."""
    g = golden("g13_svdpp_sgd_step.npz")
    sd = svdpp().state_dict()
    assert set(sd) == REF_KEYS
    for key, k in G13_KEYS:
        want = g[k + "_before"]
        assert tuple(sd[key].shape) == want.shape, key
        assert np.array_equal(sd[key].numpy().view(np.uint32), want.view(np.uint32)), key


def test_svdpp_prediction_matches_reference_g4():
    g = golden("g4_svdpp.npz")
    m = svdpp()
    m.load_state_dict(g4_state(g))
    m.eval()
    with torch.no_grad():
        pred, tgt = m({"uid": torch.from_numpy(g["uid"]), "iid": torch.from_numpy(g["iid"]),
                       "iids": torch.from_numpy(g["his"])})
    assert tgt is None and pred.shape == g["prediction"].shape
    assert np.all(np.abs(pred.numpy() - g["prediction"]) <= 1e-5 * (g4_magnitude(g) + 1e-30))
    sd = m.state_dict()                               # and saves back under the same keys
    assert np.array_equal(sd["u_bias.weight"].numpy(), g["ub_table"])
    assert np.array_equal(sd["implicit_i_embeddings.weight"].numpy(), g["imp_table"])
    assert sd["global_bias"].shape == () and float(sd["global_bias"]) == float(g["global_bias"])


def test_svdpp_cpu_train_step_matches_reference_g13():
    """One CPU train_step (MSE, SGD lr 0.5) from G13's inputs lands on the reference's
    own 'after' tables within the G10 tolerance (rtol 1e-5, atol 1e-8; loss 1e-5
    relative), which therefore holds for the reference's numbers before any GPU is
    involved."""
    g = golden("g13_svdpp_sgd_step.npz")
    m = svdpp()
    m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), torch.nn.MSELoss(), [],
              torch.device("cpu"))
    batch = {k: torch.from_numpy(g[k]) for k in ("uid", "iid", "iids", "label")}
    loss = float(m.train_step(batch)["loss"])
    want = float(g["loss"])
    print("loss", loss, want)
    assert abs(loss - want) <= 1e-5 * abs(want)
    sd = m.state_dict()
    for key, k in G13_KEYS:
        got, ref_after = sd[key].numpy(), g[k + "_after"]
        print(key, "max |diff|", float(np.max(np.abs(got - ref_after))))
        np.testing.assert_allclose(got, ref_after, rtol=1e-5, atol=1e-8, err_msg=key)
    assert not np.array_equal(sd["implicit_i_embeddings.weight"].numpy(), g["imp_before"])


def test_svdpp_sampled_branch_cpu():
    """iid [B, N]: prediction [B, N] equals the N single-item predictions, the target
    is [1, 0, ...]."""
    g = golden("g4_svdpp.npz")
    m = svdpp()
    m.load_state_dict(g4_state(g))
    m.eval()
    B, N = 16, 5
    rng = np.random.default_rng(5)
    iid = torch.from_numpy(rng.integers(0, 37, (B, N)))
    uid = torch.from_numpy(g["uid"][:B])
    his = torch.from_numpy(g["his"][:B])
    with torch.no_grad():
        pred, tgt = m({"uid": uid, "iid": iid, "iids": his})
        cols = [m({"uid": uid, "iid": iid[:, n].contiguous(), "iids": his})[0] for n in range(N)]
    assert pred.shape == (B, N) and tgt.dtype == torch.float32
    np.testing.assert_allclose(pred.numpy(), torch.stack(cols, 1).numpy(), rtol=1e-6, atol=1e-9)
    want_t = np.zeros((B, N), np.float32)
    want_t[:, 0] = 1
    assert np.array_equal(tgt.numpy(), want_t)
