"""GRU4Rec on the CPU path (no GPU): the registry, the reference's checkpoint keys and RNG
order (G16 state A), its forward in two weight states, all six gradients and one SGD
step at lively weights (G16 state B), one reference train step, the dead ids, the errors,
a pair-wise ``fit`` on the planted sequence set, and the argument validation of the new
libmrec exports.

Tolerances: those of the CPU golden tests (G10 / G13 / G15): tensors rtol 1e-5 / atol 1e-8
after a step, loss 1e-5 relative; forward values and gradients |got - want| <= 1e-5
max|want| (a plain torch restatement of the recurrence is 3e-7 of each tensor's magnitude
from the reference's nn.GRU at these shapes).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from test_sasrec_cpu import close_to_magnitude, planted_sequences

KEYS = ("i_embeddings.weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0",
        "rnn.bias_hh_l0", "out.weight")


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def gru4rec(items=41, emb_size=16, hidden_size=32, max_his_len=12, seed=2020, device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import GRU4Rec
    return GRU4Rec(CategoricalColumnWithIdentity(items, "iid"),
                   CategoricalColumnWithIdentity(max_his_len + 1, "his_len"),
                   CategoricalColumnWithIdentity(items, "his"),
                   CategoricalColumnWithIdentity(2, "label"), emb_size=emb_size,
                   hidden_size=hidden_size, random_seed=seed, device=device, **kw)


def g16_batch(g, device=None):
    return {k: torch.from_numpy(g[k]).to(device or "cpu") for k in ("iid", "his", "his_len", "label")}


def g16_state(g, which):
    return {k: torch.from_numpy(g[f"{which}::{k}"]) for k in KEYS}


# ---------------------------------------------------------------------------
# registry, keys, initialisation, checkpoints
# ---------------------------------------------------------------------------

def test_registry_answers_gru4rec():
    from pytorchrec_amd.model import GRU4Rec, get_model_type, model_name_list
    assert get_model_type("gru4rec") is GRU4Rec and "gru4rec" in model_name_list
    names = [a.name for a in GRU4Rec.get_argument_descriptions()]
    assert names == ["emb_size", "hidden_size"]


def test_init_and_keys_match_reference_g16():
    """Seed 2020 -> exactly the six reference keys in its order, every tensor bit-identical
    to the reference's own initialisation (the RNG is consumed in its order)."""
    g = golden("g16_gru4rec.npz")
    assert tuple(g["keys"].tolist()) == KEYS
    sd = gru4rec().state_dict()
    assert tuple(sd) == KEYS
    for k in KEYS:
        want = g[f"A::{k}"]
        assert tuple(sd[k].shape) == want.shape, k
        assert np.array_equal(sd[k].numpy().view(np.uint32), want.view(np.uint32)), k
    assert not isinstance(gru4rec().rnn, torch.nn.GRU)


def test_reference_checkpoint_round_trips():
    g = golden("g16_gru4rec.npz")
    m = gru4rec(seed=1)
    m.load_state_dict(g16_state(g, "B"))
    sd = m.state_dict()
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"B::{k}"]), k
    # a table whose rows the bank pitches (E = 24 -> 32 columns) speaks [I, E] too
    m24 = gru4rec(emb_size=24, seed=3)
    sd24 = m24.state_dict()
    assert tuple(sd24["i_embeddings.weight"].shape) == (41, 24)
    other = gru4rec(emb_size=24, seed=4)
    other.load_state_dict(sd24)
    for k in KEYS:
        assert torch.equal(other.state_dict()[k], sd24[k]), k
    bad = dict(g16_state(g, "B"))
    bad["i_embeddings.weight"] = torch.zeros(40, 16)
    with pytest.raises(RuntimeError, match="size mismatch for i_embeddings.weight"):
        gru4rec().load_state_dict(bad)
    bad = dict(g16_state(g, "B"))
    bad["rnn.weight_hh_l0"] = torch.zeros(96, 31)
    with pytest.raises(RuntimeError, match="size mismatch for rnn.weight_hh_l0"):
        gru4rec().load_state_dict(bad)


# ---------------------------------------------------------------------------
# forward, gradients, train steps against the reference
# ---------------------------------------------------------------------------

def test_state_a_forward_matches_reference_g16():
    g = golden("g16_gru4rec.npz")
    m = gru4rec().eval()
    with torch.no_grad():
        pred, target = m(g16_batch(g))
    assert pred.shape == (24, 5) and target.dtype == torch.float32
    assert np.array_equal(target.numpy(), g["A_target"])
    close_to_magnitude(pred.numpy(), g["A_pred"], 1e-5, "state A prediction")
    batch = g16_batch(g)
    del batch["label"]
    assert m(batch)[1] is None


def test_state_b_forward_and_gradients_match_reference_g16():
    g = golden("g16_gru4rec.npz")
    m = gru4rec().eval()
    m.load_state_dict(g16_state(g, "B"))
    pred, _ = m(g16_batch(g))
    close_to_magnitude(pred.detach().numpy(), g["B_pred"], 1e-5, "state B prediction")
    pred.square().mean().backward()
    grads = dict(m.named_parameters())
    assert tuple(grads) == KEYS
    for k in KEYS:
        close_to_magnitude(grads[k].grad.numpy()[:, :16] if k == "i_embeddings.weight"
                           else grads[k].grad.numpy(), g[f"B_grad::{k}"], 1e-5, "grad " + k)


def _step_matches(m, batch, lr, want_after, loss_want=None):
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), torch.nn.MSELoss(), [],
              torch.device("cpu"))
    loss = float(m.train_step(batch)["loss"].detach())
    if loss_want is not None:
        assert abs(loss - loss_want) <= 1e-5 * abs(loss_want), (loss, loss_want)
    sd = m.state_dict()
    for k in KEYS:
        got, after = sd[k].numpy(), want_after(k)
        print(k, "max |diff|", float(np.max(np.abs(got - after))))
        np.testing.assert_allclose(got, after, rtol=1e-5, atol=1e-8, err_msg=k)


def test_state_a_train_step_matches_reference_g16():
    """One CPU train_step (MSE, SGD lr 0.5) lands on the reference's own 'after' tensors
    (rtol 1e-5, atol 1e-8; loss 1e-5 relative).  At this state the GRU's gradients are
    below atol: it pins the plumbing."""
    g = golden("g16_gru4rec.npz")
    _step_matches(gru4rec(), g16_batch(g), float(g["lr"]), lambda k: g[f"A_after::{k}"],
                  float(g["A_loss"]))
    assert not np.array_equal(g["A::out.weight"], g["A_after::out.weight"])


def test_state_b_sgd_step_matches_reference_g16():
    """One SGD step of lr 0.05 on prediction.square().mean() (MSE against a zero label) at
    the lively weights: every tensor moves by 1e-3 .. 1e-2 and lands on the reference's."""
    g = golden("g16_gru4rec.npz")
    m = gru4rec()
    m.load_state_dict(g16_state(g, "B"))
    batch = g16_batch(g)
    batch["label"] = torch.zeros_like(batch["label"])
    _step_matches(m, batch, float(g["lr_b"]), lambda k: g[f"B_after::{k}"])
    for k in KEYS:
        assert np.abs(g[f"B_after::{k}"] - g[f"B::{k}"]).max() > 1e-3, k


def test_ids_past_the_length_do_not_matter():
    g = golden("g16_gru4rec.npz")
    m = gru4rec().eval()
    m.load_state_dict(g16_state(g, "B"))
    batch = g16_batch(g)
    dead = torch.arange(12)[None, :] >= batch["his_len"][:, None]
    assert dead.any() and (batch["his"][dead] == 0).all()
    with torch.no_grad():
        a = m(batch)[0]
        batch["his"] = torch.where(dead, torch.full_like(batch["his"], 7), batch["his"])
        b = m(batch)[0]
    assert torch.equal(a, b)


def test_a_one_dimensional_iid_is_refused():
    g = golden("g16_gru4rec.npz")
    batch = g16_batch(g)
    batch["iid"] = batch["iid"][:, 0]
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        gru4rec()(batch)


@pytest.mark.parametrize("bad", [0, 13])
def test_a_length_outside_the_history_is_an_index_error(bad):
    g = golden("g16_gru4rec.npz")
    batch = g16_batch(g)
    batch["his_len"] = batch["his_len"].clone()
    batch["his_len"][3] = bad
    with pytest.raises(IndexError):
        gru4rec()(batch)


# ---------------------------------------------------------------------------
# fit(train_mode="pair_wise") + evaluate
# ---------------------------------------------------------------------------

def test_fit_pair_wise_and_evaluate():
    """The last epoch's loss is below 0.95 x the first's: the reference's own GRU4Rec,
    trained this way on this data with uniform negatives, reached 0.81 - 0.88 after 12
    epochs over three seeds; 0.95 asks for learning without pinning a seed's luck."""
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss
    from pytorchrec_amd.metrics import get_metric
    from pytorchrec_amd.sampling import NegativeSampler
    train, dev, (pu, pi) = planted_sequences()
    m = gru4rec(items=61, emb_size=16, hidden_size=32, max_his_len=8, seed=11)
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
    assert hist[-1]["loss"] < 0.95 * hist[0]["loss"], (hist[0]["loss"], hist[-1]["loss"])
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


P = 4096  # a non-NULL, 16-byte aligned address that is never dereferenced


def _args(lib, **kw):
    from pytorchrec_amd import _mrec
    base = dict(rows=P, ld_rows=64, his_len=P, order=None, w_ih=P, ld_ih=64, w_hh=P, ld_hh=64,
                b_ih=P, b_hh=P, E=64, H=64, L=50, batch=40, hs=P, h_last=P, d_oob_flag=None,
                dh_last=P, d_rows=P, ld_drows=64, part=P, parts=lib.mrec_gru_parts(40))
    base.update(kw)
    return _mrec.GruArgs(**base)


def _einval(lib, st, word):
    from pytorchrec_amd import _mrec
    assert st == _mrec.EINVAL, st
    assert word.encode() in lib.mrec_last_error(), lib.mrec_last_error()


def test_gru_exports_validate_their_arguments(lib):
    fwd, bwd = lib.mrec_gru_fwd, lib.mrec_gru_bwd
    for f in (fwd, bwd):
        _einval(lib, f(None, None), "NULL")
        for name in ("rows", "his_len", "w_ih", "w_hh", "b_ih", "b_hh", "hs"):
            _einval(lib, f(ctypes.byref(_args(lib, **{name: None})), None), "NULL")
        for d in (0, 8, 24, 128):
            wide = dict(ld_rows=128, ld_ih=128, ld_hh=128, ld_drows=128)
            _einval(lib, f(ctypes.byref(_args(lib, E=d, **wide)), None), "E and H must be")
            _einval(lib, f(ctypes.byref(_args(lib, H=d, **wide)), None), "E and H must be")
        for n in (0, 65):
            _einval(lib, f(ctypes.byref(_args(lib, L=n)), None), "L <= 64")
        _einval(lib, f(ctypes.byref(_args(lib, batch=-1)), None), "batch")
        for name in ("ld_rows", "ld_ih", "ld_hh"):
            _einval(lib, f(ctypes.byref(_args(lib, **{name: 8})), None), "leading dimension")
        _einval(lib, f(ctypes.byref(_args(lib, ld_rows=68)), None), "16-byte")
        _einval(lib, f(ctypes.byref(_args(lib, rows=P + 2)), None), "16-byte")
    _einval(lib, fwd(ctypes.byref(_args(lib, h_last=None)), None), "NULL")
    for name in ("dh_last", "d_rows", "part"):
        _einval(lib, bwd(ctypes.byref(_args(lib, **{name: None})), None), "NULL")
    _einval(lib, bwd(ctypes.byref(_args(lib, ld_drows=68)), None), "d_rows")
    _einval(lib, bwd(ctypes.byref(_args(lib, parts=lib.mrec_gru_parts(40) + 1)), None), "parts")
    # host-only queries
    assert lib.mrec_gru_param_count(16, 32) == 96 * 50
    assert lib.mrec_gru_param_count(64, 64) == 3 * 64 * (64 + 64 + 2)
    tile = lib.mrec_gru_tile()
    assert tile == 16
    assert lib.mrec_gru_parts(0) == 1 and lib.mrec_gru_parts(1) == 1
    assert lib.mrec_gru_parts(tile) == 1 and lib.mrec_gru_parts(tile + 1) == 2
    assert lib.mrec_gru_parts(1 << 20) >= 1


def test_gru_supported_is_a_shape_question(lib):
    from pytorchrec_amd import dense
    ok = (16, 32, 64)
    for e in (8, 16, 24, 32, 48, 64, 128):
        for h in (8, 16, 24, 32, 48, 64, 128):
            assert lib.mrec_gru_supported(e, h, 50) == int(e in ok and h in ok), (e, h)
    assert [lib.mrec_gru_supported(64, 64, n) for n in (0, 1, 64, 65)] == [0, 1, 1, 0]
    assert dense.gru_supported(64, 64, 50) is True and dense.gru_supported(24, 64, 50) is False
    assert dense.gru_supported(64, 48, 50) is False and dense.gru_supported(64, 64, 65) is False
    assert dense.GRU_FUSED is True
