"""SASRec on the CPU path (no GPU): the registry, the reference's checkpoint keys and RNG
order (G15 state A), its forward in two weight states, all ten gradients at lively
weights (G15 state B), one reference train step, a pair-wise ``fit`` on a small planted
sequence set, and the argument validation of the new libmrec exports.

Tolerances: the fp32 ones of the CPU golden step tests (G10 / G13): tensors rtol 1e-5 /
atol 1e-8 after the step, loss 1e-5 relative.  Forward values and gradients are sums of
terms of both signs, so their error is bounded against the tensor's own magnitude:
|got - want| <= 1e-5 max|want| (fp32 rounding 6e-8 per operation over the few hundred
operations of a two-layer block; the reference's own error is of that size too, its
softmax is shifted by another constant).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

KEYS = ("i_embeddings.weight", "p_embeddings.weight", "Q.weight", "K.weight", "W1.weight",
        "W1.bias", "W2.weight", "W2.bias", "layer_norm.weight", "layer_norm.bias")


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def sasrec(items=41, emb_size=16, max_his_len=12, num_layers=2, dropout=0.0, seed=2020,
           device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import SASRec
    return SASRec(CategoricalColumnWithIdentity(items, "iid"),
                  CategoricalColumnWithIdentity(max_his_len + 1, "his_len"),
                  CategoricalColumnWithIdentity(items, "his"),
                  CategoricalColumnWithIdentity(2, "label"), emb_size=emb_size,
                  hidden_size=emb_size, max_his_len=max_his_len, num_layers=num_layers,
                  dropout=dropout, random_seed=seed, device=device, **kw)


def g15_batch(g, device=None):
    return {k: torch.from_numpy(g[k]).to(device or "cpu") for k in ("iid", "his", "his_len", "label")}


def g15_state(g, which):
    return {k: torch.from_numpy(g[f"{which}::{k}"]) for k in KEYS}


def close_to_magnitude(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, mag = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print(f"{what}: max |diff| {err:.3e}, magnitude {mag:.3e}")
    assert err <= tol * mag, (what, err, mag)


def planted_sequences(users=160, items=61, groups=4, L=8, seed=5):
    """Users and items (1 .. items - 1; 0 is PAD) in `groups` groups; a user's history
    and positive come from its own group.  -> train columns (his, his_len, iid, uid),
    dev columns with the positive first of 20 candidates, the (uid, item) pairs."""
    rng = np.random.default_rng(seed)
    per = (items - 1) // groups
    his = np.zeros((users, L), np.int64)
    his_len = rng.integers(1, L + 1, size=users)
    pos, dev = np.empty(users, np.int64), np.empty((users, 20), np.int64)
    for u in range(users):
        own = 1 + (u % groups) * per + rng.permutation(per)
        his[u, :his_len[u]] = own[:his_len[u]]
        pos[u] = own[L]
        others = np.setdiff1d(np.arange(1, items), own)
        dev[u] = np.concatenate([own[L + 1:L + 2], rng.choice(others, 19, replace=False)])
    uid = np.arange(users)
    label = np.zeros((users, 20), np.int64)
    label[:, 0] = 1  # (evaluate wants the reference's label column: the positive first)
    return ({"his": his, "his_len": his_len, "iid": pos, "uid": uid},
            {"his": his, "his_len": his_len, "iid": dev, "uid": uid, "label": label},
            (np.repeat(uid, L + 1), np.concatenate([his, pos[:, None]], 1).reshape(-1)))


# ---------------------------------------------------------------------------
# registry, keys, initialisation, checkpoints
# ---------------------------------------------------------------------------

def test_registry_answers_sasrec():
    from pytorchrec_amd.model import SASRec, get_model_type, model_name_list
    assert get_model_type("sasrec") is SASRec and "sasrec" in model_name_list
    names = [a.name for a in SASRec.get_argument_descriptions()]
    assert names == ["emb_size", "max_his_len", "num_layers", "dropout"]


def test_init_and_keys_match_reference_g15():
    """Seed 2020 -> exactly the ten reference keys, every tensor bit-identical to the
    reference's own initialisation (the RNG is consumed in its order)."""
    g = golden("g15_sasrec.npz")
    assert tuple(g["keys"].tolist()) == KEYS
    sd = sasrec().state_dict()
    assert set(sd) == set(KEYS) and len(sd) == 10
    for k in KEYS:
        want = g[f"A::{k}"]
        assert tuple(sd[k].shape) == want.shape, k
        assert np.array_equal(sd[k].numpy().view(np.uint32), want.view(np.uint32)), k
    assert isinstance(sasrec().p_embeddings.weight, torch.nn.Parameter)
    assert sasrec().p_embeddings.weight.dtype == torch.float32


def test_reference_checkpoint_round_trips():
    g = golden("g15_sasrec.npz")
    m = sasrec(seed=1)
    m.load_state_dict(g15_state(g, "B"))
    sd = m.state_dict()
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"B::{k}"]), k
    # a table whose rows the bank pitches (D = 24 -> 32 columns) speaks [I, D] too
    m24 = sasrec(emb_size=24, seed=3)
    sd24 = m24.state_dict()
    assert tuple(sd24["i_embeddings.weight"].shape) == (41, 24)
    other = sasrec(emb_size=24, seed=4)
    other.load_state_dict(sd24)
    for k in KEYS:
        assert torch.equal(other.state_dict()[k], sd24[k]), k
    bad = dict(g15_state(g, "B"))
    bad["i_embeddings.weight"] = torch.zeros(40, 16)
    with pytest.raises(RuntimeError, match="size mismatch for i_embeddings.weight"):
        sasrec().load_state_dict(bad)
    bad = dict(g15_state(g, "B"))
    bad["Q.weight"] = torch.zeros(16, 15)
    with pytest.raises(RuntimeError, match="size mismatch for Q.weight"):
        sasrec().load_state_dict(bad)


# ---------------------------------------------------------------------------
# forward, gradients, one train step against the reference
# ---------------------------------------------------------------------------

def test_state_a_forward_matches_reference_g15():
    g = golden("g15_sasrec.npz")
    m = sasrec().eval()
    with torch.no_grad():
        pred, target = m(g15_batch(g))
    assert pred.shape == (24, 5) and target.dtype == torch.float32
    assert np.array_equal(target.numpy(), g["A_target"])
    close_to_magnitude(pred.numpy(), g["A_pred"], 1e-5, "state A prediction")
    batch = g15_batch(g)
    del batch["label"]
    assert m(batch)[1] is None


def test_state_b_forward_and_gradients_match_reference_g15():
    g = golden("g15_sasrec.npz")
    m = sasrec().eval()
    m.load_state_dict(g15_state(g, "B"))
    pred, _ = m(g15_batch(g))
    close_to_magnitude(pred.detach().numpy(), g["B_pred"], 1e-5, "state B prediction")
    pred.square().mean().backward()
    grads = dict(m.named_parameters())
    assert set(grads) == set(KEYS)
    for k in KEYS:
        close_to_magnitude(grads[k].grad.numpy()[:, :16] if k == "i_embeddings.weight"
                           else grads[k].grad.numpy(), g[f"B_grad::{k}"], 1e-5, "grad " + k)


def test_state_a_train_step_matches_reference_g15():
    """One CPU train_step (MSE, SGD lr 0.5) lands on the reference's own 'after'
    tensors within the G10 / G13 tolerance (rtol 1e-5, atol 1e-8; loss 1e-5 relative)."""
    g = golden("g15_sasrec.npz")
    m = sasrec()
    m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), torch.nn.MSELoss(), [],
              torch.device("cpu"))
    loss = float(m.train_step(g15_batch(g))["loss"].detach())
    want = float(g["A_loss"])
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    sd = m.state_dict()
    for k in KEYS:
        got, after = sd[k].numpy(), g[f"A_after::{k}"]
        print(k, "max |diff|", float(np.max(np.abs(got - after))))
        np.testing.assert_allclose(got, after, rtol=1e-5, atol=1e-8, err_msg=k)
    assert not np.array_equal(g["A::W2.weight"], g["A_after::W2.weight"])


def test_a_one_dimensional_iid_is_refused():
    g = golden("g15_sasrec.npz")
    batch = g15_batch(g)
    batch["iid"] = batch["iid"][:, 0]
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        sasrec()(batch)


def test_a_position_outside_the_table_is_an_index_error():
    g = golden("g15_sasrec.npz")
    batch = g15_batch(g)
    batch["his_len"] = batch["his_len"].clone()
    batch["his_len"][3] = 13
    with pytest.raises(IndexError):
        sasrec()(batch)


def test_dropout_runs_only_in_training():
    g = golden("g15_sasrec.npz")
    m = sasrec(dropout=0.5)
    m.load_state_dict(g15_state(g, "B"))
    with torch.no_grad():
        e1, e2 = m.eval()(g15_batch(g))[0], m.eval()(g15_batch(g))[0]
        t1 = m.train()(g15_batch(g))[0]
    assert torch.equal(e1, e2)
    close_to_magnitude(e1.numpy(), g["B_pred"], 1e-5, "eval with dropout configured")
    assert not torch.equal(e1, t1)


# ---------------------------------------------------------------------------
# fit(train_mode="pair_wise") + evaluate
# ---------------------------------------------------------------------------

def test_fit_pair_wise_and_evaluate():
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.metrics import get_metric
    from pytorchrec_amd.sampling import NegativeSampler
    train, dev, (pu, pi) = planted_sequences()
    m = sasrec(items=61, emb_size=16, max_his_len=8, num_layers=1, seed=11)
    metrics = [get_metric("ndcg@10"), get_metric("hit@10")]
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), BPRLoss(), metrics,
              torch.device("cpu"))
    m.set_negative_sampler(NegativeSampler(pu, pi, 1, 61, seed=3, n_users=160), n_neg=1,
                           uid_column=CategoricalColumnWithIdentity(160, "uid"),
                           iid_column=m.iid_column)
    hist = m.fit(ColumnarDataset(train), 64, 12, dev_dataset=ColumnarDataset(dev),
                 train_mode="pair_wise", verbose=0)
    print("loss per epoch:", [round(r["loss"], 4) for r in hist],
          "ndcg@10:", [round(r["ndcg@10"], 4) for r in hist])
    assert len(hist) == 12 and set(hist[0]) == {"loss", "ndcg@10", "hit@10"}
    assert hist[-1]["loss"] < 0.8 * hist[0]["loss"], (hist[0]["loss"], hist[-1]["loss"])
    got = m.evaluate(ColumnarDataset(dev), 50, verbose=0)
    assert got["ndcg@10"] == hist[-1]["ndcg@10"] and 0.0 <= got["hit@10"] <= 1.0
    assert m.predict(ColumnarDataset(dev), 77).shape == (160, 20)


# ---------------------------------------------------------------------------
# ABI: argument validation before any device work (no GPU present)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorchrec_amd import _mrec
    return _mrec.lib()


P = 4096  # a non-NULL address that is never dereferenced: validation comes first


def _args(**kw):
    from pytorchrec_amd import _mrec
    base = dict(rows=P, ld_rows=64, his=P, ld_his=50, his_len=P, pos=P, ld_pos=64, pos_rows=51,
                wq=P, ld_wq=64, wk=P, ld_wk=64, w1=P, ld_w1=64, b1=P, w2=P, ld_w2=64, b2=P,
                gamma=P, beta=P, eps=1e-5, num_layers=2, batch=8, L=50, D=64, hs=P, v=P,
                d_oob_flag=None, dv=P, d_rows=P, ld_drows=64, part=P, parts=8)
    base.update(kw)
    return _mrec.SasrecArgs(**base)


def _einval(lib, st, word):
    from pytorchrec_amd import _mrec
    assert st == _mrec.EINVAL, st
    assert word.encode() in lib.mrec_last_error(), lib.mrec_last_error()


def test_sasrec_exports_validate_their_arguments(lib):
    fwd, bwd = lib.mrec_sasrec_fwd, lib.mrec_sasrec_bwd
    for f in (fwd, bwd):
        _einval(lib, f(None, None), "NULL")
        for name in ("rows", "his", "his_len", "pos", "wq", "wk", "w1", "b1", "w2", "b2", "gamma",
                     "beta", "hs"):
            _einval(lib, f(ctypes.byref(_args(**{name: None})), None), "NULL")
        for d in (0, 8, 24, 128):
            _einval(lib, f(ctypes.byref(_args(D=d, ld_rows=128, ld_pos=128, ld_wq=128, ld_wk=128,
                                              ld_w1=128, ld_w2=128, ld_drows=128)), None),
                    "D must be")
        for n in (0, 65):
            _einval(lib, f(ctypes.byref(_args(L=n, ld_his=80)), None), "L <= 64")
        _einval(lib, f(ctypes.byref(_args(batch=-1)), None), "negative batch")
        _einval(lib, f(ctypes.byref(_args(num_layers=0)), None), "num_layers")
        for name in ("ld_rows", "ld_his", "ld_pos", "ld_wq", "ld_wk", "ld_w1", "ld_w2"):
            _einval(lib, f(ctypes.byref(_args(**{name: 8})), None), "leading dimension")
    _einval(lib, fwd(ctypes.byref(_args(v=None)), None), "NULL")
    for name in ("dv", "d_rows", "part"):
        _einval(lib, bwd(ctypes.byref(_args(**{name: None})), None), "NULL")
    _einval(lib, bwd(ctypes.byref(_args(ld_drows=8)), None), "d_rows")
    _einval(lib, bwd(ctypes.byref(_args(parts=7)), None), "parts")
    wg = lib.mrec_sasrec_wgrad
    _einval(lib, wg(None, 8, 100, P, None), "NULL")
    _einval(lib, wg(P, 8, 100, None, None), "NULL")
    _einval(lib, wg(P, 0, 100, P, None), "no partials")
    # host-only queries
    assert lib.mrec_sasrec_param_count(64, 51) == 4 * 64 * 64 + 4 * 64 + 51 * 64
    assert lib.mrec_sasrec_parts(0) == 1 and lib.mrec_sasrec_parts(3) == 3
    assert [lib.mrec_sasrec_supported(d, 50) for d in (16, 24, 32, 64, 128)] == [1, 0, 1, 1, 0]
    assert lib.mrec_sasrec_supported(64, 64) == 1 and lib.mrec_sasrec_supported(64, 65) == 0


def test_sasrec_supported_is_a_shape_question():
    from pytorchrec_amd import dense
    assert dense.sasrec_supported(64, 50, 2) is True
    assert dense.sasrec_supported(128, 50, 2) is False and dense.sasrec_supported(24, 50) is False
    assert dense.sasrec_supported(64, 65) is False and dense.sasrec_supported(64, 0) is False
    assert dense.sasrec_supported(64, 50, 2, dropout=0.5, training=True) is False
    assert dense.sasrec_supported(64, 50, 2, dropout=0.5, training=False) is True
