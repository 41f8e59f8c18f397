"""NCF on the CPU path (no GPU): the registry, the reference's checkpoint keys and RNG
order (G17 state A), the reference's own forward through the model (G7, G17), all nine
gradients and one SGD step at lively weights (G17 state B), one reference train step, the
errors, dropout, a pair-wise ``fit`` on the planted set, and the argument validation of the
new libmrec exports.

Tolerances: those of the CPU golden tests (G10 / G13 / G15 / G16): tensors rtol 1e-5 /
atol 1e-8 after a step, loss 1e-5 relative; forward values and gradients |got - want| <=
1e-5 max|want|; G7 at the rtol 1e-5 / atol 1e-7 the oracle's own G7 test uses.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from test_ranking_cpu import planted_set
from test_sasrec_cpu import close_to_magnitude

TABLE_KEYS = ("mf_u_embeddings.weight", "mf_i_embeddings.weight", "mlp_u_embeddings.weight",
              "mlp_i_embeddings.weight")
KEYS = TABLE_KEYS + ("mlp.mlp.dense_0.linear.weight", "mlp.mlp.dense_0.linear.bias",
                     "mlp.mlp.dense_1.linear.weight", "mlp.mlp.dense_1.linear.bias",
                     "prediction.weight")
REQUIRED_SHAPES = ((8, [16, 8]), (16, [32, 16, 8]), (32, [64, 32, 16]), (64, [128, 64, 32]),
                   (64, [64]))


# ---------------------------------------------------------------------------
# shared helpers (the GPU suite imports them)
# ---------------------------------------------------------------------------

def ncf(users=50, items=37, emb_size=8, layers=(16, 8), dropout=0.0, seed=2020, device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity
    from pytorchrec_amd.model import NCF
    return NCF(CategoricalColumnWithIdentity(users, "uid"),
               CategoricalColumnWithIdentity(items, "iid"),
               CategoricalColumnWithIdentity(2, "label"), emb_size=emb_size, layers=layers,
               dropout=dropout, random_seed=seed, device=device, **kw)


def g17_batch(g, device=None):
    return {k: torch.from_numpy(g[k]).to(device or "cpu") for k in ("uid", "iid", "label")}


def g17_state(g, which):
    return {k: torch.from_numpy(g[f"{which}::{k}"]) for k in KEYS}


def g7_state(g):
    names = ("mf_u", "mf_i", "mlp_u", "mlp_i", "W0", "b0", "W1", "b1", "Wp")
    return {k: torch.from_numpy(g[n]) for k, n in zip(KEYS, names)}


def table_grads(m):
    """The bank's dense gradient cut into the reference's four tables [n, E]."""
    bank, E = m.embeddings, m.emb_size
    g = bank.weight.grad
    return {k: g[o:o + n, :E] for k, o, n in zip(TABLE_KEYS, bank.row_offset, bank.category_nums)}


def named_grads(m):
    out = dict(table_grads(m))
    out.update({k: p.grad for k, p in m.named_parameters() if k != "embeddings.weight"})
    return out


# ---------------------------------------------------------------------------
# registry, keys, initialisation, checkpoints
# ---------------------------------------------------------------------------

def test_registry_answers_ncf():
    from pytorchrec_amd.model import NCF, get_model_type, model_name_list
    assert get_model_type("ncf") is NCF and "ncf" in model_name_list
    names = [a.name for a in NCF.get_argument_descriptions()]
    assert names == ["emb_size", "layers", "dropout"]
    assert ncf(layers="[16, 8]").layers == [16, 8] and ncf(layers="16,8").layers == [16, 8]


def test_init_and_keys_match_reference_g17():
    """Seed 2020 -> exactly the nine reference keys in its order, every tensor bit-identical
    to the reference's own initialisation (the RNG is consumed in its order)."""
    g = golden("g17_ncf.npz")
    assert tuple(g["keys"].tolist()) == KEYS
    m = ncf()
    sd = m.state_dict()
    assert tuple(sd) == KEYS
    for k in KEYS:
        want = g[f"A::{k}"]
        assert tuple(sd[k].shape) == want.shape, k
        assert np.array_equal(sd[k].numpy().view(np.uint32), want.view(np.uint32)), k
    assert list(m.embeddings.category_nums) == [50, 37, 50, 37]


def test_reference_checkpoint_round_trips():
    g = golden("g17_ncf.npz")
    m = ncf(seed=1)
    m.load_state_dict(g17_state(g, "B"))
    sd = m.state_dict()
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"B::{k}"]), k
    other = ncf(seed=4)
    other.load_state_dict(sd)
    for k in KEYS:
        assert torch.equal(other.state_dict()[k], sd[k]), k
    bad = dict(g17_state(g, "B"))
    bad["mlp_i_embeddings.weight"] = torch.zeros(36, 8)
    with pytest.raises(RuntimeError, match="size mismatch for mlp_i_embeddings.weight"):
        ncf().load_state_dict(bad)
    bad = dict(g17_state(g, "B"))
    bad["mlp.mlp.dense_1.linear.weight"] = torch.zeros(8, 15)
    with pytest.raises(RuntimeError, match="size mismatch for mlp.mlp.dense_1.linear.weight"):
        ncf().load_state_dict(bad)
    missing = dict(g17_state(g, "B"))
    del missing["mf_i_embeddings.weight"]
    with pytest.raises(RuntimeError, match="mf_i_embeddings.weight"):
        ncf().load_state_dict(missing)


# ---------------------------------------------------------------------------
# forward, gradients, train steps against the reference
# ---------------------------------------------------------------------------

def test_g7_prediction_through_the_model():
    g = golden("g7_ncf.npz")
    m = ncf().eval()
    m.load_state_dict(g7_state(g))
    with torch.no_grad():
        pred, target = m({"uid": torch.from_numpy(g["uid"]), "iid": torch.from_numpy(g["iid"])})
    assert pred.shape == (32, 3) and pred.dtype == torch.float32
    assert torch.equal(target, torch.tensor([1.0, 0.0, 0.0]).expand(32, 3))
    np.testing.assert_allclose(pred.numpy(), g["prediction"], rtol=1e-5, atol=1e-7)


def test_state_a_forward_matches_reference_g17():
    g = golden("g17_ncf.npz")
    m = ncf().eval()
    with torch.no_grad():
        pred, target = m(g17_batch(g))
    assert pred.shape == (24, 5) and target.dtype == torch.float32
    assert np.array_equal(target.numpy(), g["A_target"])
    close_to_magnitude(pred.numpy(), g["A_pred"], 1e-5, "state A prediction")


def test_state_b_forward_and_gradients_match_reference_g17():
    g = golden("g17_ncf.npz")
    m = ncf().eval()
    m.load_state_dict(g17_state(g, "B"))
    pred, _ = m(g17_batch(g))
    close_to_magnitude(pred.detach().numpy(), g["B_pred"], 1e-5, "state B prediction")
    pred.square().mean().backward()
    grads = named_grads(m)
    assert set(grads) == set(KEYS)
    for k in KEYS:
        close_to_magnitude(grads[k].numpy(), g[f"B_grad::{k}"], 1e-5, "grad " + k)


def _tensors_match(m, want_after):
    sd = m.state_dict()
    for k in KEYS:
        got, after = sd[k].numpy(), want_after(k)
        print(k, "max |diff|", float(np.max(np.abs(got - after))))
        np.testing.assert_allclose(got, after, rtol=1e-5, atol=1e-8, err_msg=k)


def test_state_a_train_step_matches_reference_g17():
    """One CPU train_step (MSE against the model's own target, SGD lr 0.5) lands on the
    reference's own 'after' tensors (rtol 1e-5, atol 1e-8; loss 1e-5 relative)."""
    g = golden("g17_ncf.npz")
    m = ncf()
    m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), torch.nn.MSELoss(), [],
              torch.device("cpu"))
    loss = float(m.train_step(g17_batch(g))["loss"].detach())
    assert abs(loss - float(g["A_loss"])) <= 1e-5 * abs(float(g["A_loss"])), (loss, float(g["A_loss"]))
    _tensors_match(m, lambda k: g[f"A_after::{k}"])
    assert not np.array_equal(g["A::prediction.weight"], g["A_after::prediction.weight"])


def test_state_b_sgd_step_matches_reference_g17():
    """One SGD step of lr 0.05 on prediction.square().mean() at the lively weights: every
    tensor moves and lands on the reference's."""
    g = golden("g17_ncf.npz")
    m = ncf().eval()
    m.load_state_dict(g17_state(g, "B"))
    opt = torch.optim.SGD(m.parameters(), lr=float(g["lr_b"]))
    pred, _ = m(g17_batch(g))
    pred.square().mean().backward()
    opt.step()
    _tensors_match(m, lambda k: g[f"B_after::{k}"])
    for k in KEYS:
        assert np.abs(g[f"B_after::{k}"] - g[f"B::{k}"]).max() > 1e-4, k


def test_a_one_dimensional_iid_is_refused():
    g = golden("g17_ncf.npz")
    batch = g17_batch(g)
    batch["iid"] = batch["iid"][:, 0]
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        ncf()(batch)


@pytest.mark.parametrize("column,bad", [("uid", 50), ("uid", -1), ("iid", 37), ("iid", -1)])
def test_an_id_outside_its_table_is_an_index_error(column, bad):
    g = golden("g17_ncf.npz")
    batch = g17_batch(g)
    batch[column] = batch[column].clone()
    batch[column].reshape(-1)[3] = bad
    with pytest.raises(IndexError):
        ncf()(batch)


def test_dropout_is_active_in_training_only():
    g = golden("g17_ncf.npz")
    plain, dropped = ncf(), ncf(dropout=0.5)
    state = g17_state(g, "B")
    plain.load_state_dict(state)
    dropped.load_state_dict(state)
    batch = g17_batch(g)
    with torch.no_grad():
        want = plain.eval()(batch)[0]
        assert torch.equal(dropped.eval()(batch)[0], want)
        torch.manual_seed(0)
        got = dropped.train()(batch)[0]
        assert not torch.equal(got, want)
        assert torch.equal(plain.train()(batch)[0], want)


# ---------------------------------------------------------------------------
# fit(train_mode="pair_wise") + evaluate
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("loss_name", ["bpr", "top1"])
def test_fit_pair_wise_and_evaluate(loss_name):
    """The planted set of the ranking tests (a user's positives come from its own group):
    the last epoch's loss is below 0.9 x the first's, which asks for learning without
    pinning a seed's luck, and evaluate agrees with the last epoch's dev metrics."""
    from pytorchrec_amd.loader import ColumnarDataset
    from pytorchrec_amd.loss import BPRLoss, Top1Loss
    from pytorchrec_amd.metrics import get_metric
    from pytorchrec_amd.sampling import NegativeSampler
    tu, ti, du, dev = planted_set()
    train = ColumnarDataset({"uid": tu, "iid": ti})
    devset = ColumnarDataset({"uid": du, "iid": dev})
    m = ncf(users=200, items=120, emb_size=8, layers=[16, 8], seed=11)
    metrics = [get_metric("ndcg@10"), get_metric("hit@10")]
    loss = BPRLoss() if loss_name == "bpr" else Top1Loss()
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.02), loss, metrics, torch.device("cpu"))
    m.set_negative_sampler(NegativeSampler(tu, ti, 0, 120, seed=3, n_users=200))
    hist = m.fit(train, 256, 8, dev_dataset=devset, train_mode="pair_wise", verbose=0)
    print("loss per epoch:", [round(r["loss"], 4) for r in hist],
          "ndcg@10:", [round(r["ndcg@10"], 4) for r in hist])
    assert len(hist) == 8 and set(hist[0]) == {"loss", "ndcg@10", "hit@10"}
    assert hist[-1]["loss"] < 0.9 * hist[0]["loss"], (hist[0]["loss"], hist[-1]["loss"])
    got = m.evaluate(devset, 128, verbose=0)
    assert got["ndcg@10"] == hist[-1]["ndcg@10"] and 0.0 <= got["hit@10"] <= 1.0
    assert m.predict(devset, 77).shape == (200, 99)


# ---------------------------------------------------------------------------
# ABI: argument validation before any device work (no GPU present)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorchrec_amd import _mrec
    return _mrec.lib()


P = 4096  # a non-NULL, 16-byte aligned address that is never dereferenced


def widths_arr(widths):
    return (ctypes.c_int32 * max(len(widths), 1))(*widths)


def _args(lib, E=64, widths=(128, 64, 32), **kw):
    from pytorchrec_amd import _mrec
    a = _mrec.NcfArgs()
    nl = len(widths)
    base = dict(rows=P, ld_rows=4 * E, pairs=100, E=E, n_layers=nl, wp=P, pred=P, dpred=P, d_rows=P,
                ld_drows=4 * E, part=P, parts=lib.mrec_ncf_parts(100))
    base.update({k: v for k, v in kw.items() if k not in ("w", "b", "ld_w")})
    for k, v in base.items():
        setattr(a, k, v)
    for l in range(min(nl, 3)):
        a.widths[l] = widths[l]
        a.w[l], a.b[l] = P, P
        a.ld_w[l] = widths[l - 1] if l else 2 * E
    for name in ("w", "b", "ld_w"):
        for l, v in kw.get(name, {}).items():
            getattr(a, name)[l] = v
    return a


def _einval(lib, st, word):
    from pytorchrec_amd import _mrec
    assert st == _mrec.EINVAL, st
    assert word.encode() in lib.mrec_last_error(), lib.mrec_last_error()


def test_ncf_exports_validate_their_arguments(lib):
    fwd, bwd = lib.mrec_ncf_fwd, lib.mrec_ncf_bwd
    for f in (fwd, bwd):
        _einval(lib, f(None, None), "NULL")
        for name in ("rows", "wp"):
            _einval(lib, f(ctypes.byref(_args(lib, **{name: None})), None), "NULL")
        for l in range(3):
            _einval(lib, f(ctypes.byref(_args(lib, w={l: None})), None), "NULL")
            _einval(lib, f(ctypes.byref(_args(lib, b={l: None})), None), "NULL")
        for e in (0, 4, 24, 128):
            _einval(lib, f(ctypes.byref(_args(lib, E=e, ld_rows=512, ld_drows=512)), None), "unsupported shape")
        for widths in ((20,), (128, 64, 4), (136,), (128, 128, 128)):
            _einval(lib, f(ctypes.byref(_args(lib, widths=widths)), None), "unsupported shape")
        _einval(lib, f(ctypes.byref(_args(lib, n_layers=0)), None), "unsupported shape")
        _einval(lib, f(ctypes.byref(_args(lib, n_layers=4)), None), "unsupported shape")
        _einval(lib, f(ctypes.byref(_args(lib, pairs=-1)), None), "pairs")
        _einval(lib, f(ctypes.byref(_args(lib, ld_w={1: 64})), None), "leading dimension")
        _einval(lib, f(ctypes.byref(_args(lib, ld_rows=260)), None), "16-byte")
        _einval(lib, f(ctypes.byref(_args(lib, ld_rows=248)), None), "16-byte")
        _einval(lib, f(ctypes.byref(_args(lib, rows=P + 2)), None), "16-byte")
    _einval(lib, fwd(ctypes.byref(_args(lib, pred=None)), None), "NULL")
    for name in ("dpred", "d_rows", "part"):
        _einval(lib, bwd(ctypes.byref(_args(lib, **{name: None})), None), "NULL")
    _einval(lib, bwd(ctypes.byref(_args(lib, ld_drows=260)), None), "d_rows")
    _einval(lib, bwd(ctypes.byref(_args(lib, d_rows=P + 4)), None), "d_rows")
    _einval(lib, bwd(ctypes.byref(_args(lib, parts=lib.mrec_ncf_parts(100) - 1)), None), "parts")
    _einval(lib, bwd(ctypes.byref(_args(lib, parts=lib.mrec_ncf_parts(100) + 1)), None), "parts")
    # host-only queries
    assert lib.mrec_ncf_param_count(8, 2, widths_arr([16, 8])) == 16 * 16 + 8 * 16 + 16 + 8 + 16
    assert (lib.mrec_ncf_param_count(64, 3, widths_arr([128, 64, 32]))
            == 128 * 128 + 64 * 128 + 32 * 64 + 128 + 64 + 32 + 64 + 32)
    assert lib.mrec_ncf_param_count(24, 1, widths_arr([16])) == 0
    tile = lib.mrec_ncf_tile()
    assert tile >= 16 and tile % 16 == 0
    assert lib.mrec_ncf_parts(0) == 1 and lib.mrec_ncf_parts(1) == 1
    assert lib.mrec_ncf_parts(tile) == 1 and lib.mrec_ncf_parts(tile + 1) == 2
    assert lib.mrec_ncf_parts(1 << 20) >= 1


def test_ncf_supported_is_a_shape_question(lib):
    from pytorchrec_amd import dense
    for E, widths in REQUIRED_SHAPES:
        assert lib.mrec_ncf_supported(E, len(widths), widths_arr(widths)) == 1, (E, widths)
        assert dense.ncf_supported(E, widths) is True
    for E in (8, 16, 32, 64):
        for w in (8, 24, 40, 128):
            assert lib.mrec_ncf_supported(E, 1, widths_arr([w])) == 1, (E, w)
    assert lib.mrec_ncf_supported(24, 2, widths_arr([16, 8])) == 0
    assert lib.mrec_ncf_supported(8, 2, widths_arr([20, 8])) == 0
    assert lib.mrec_ncf_supported(8, 2, widths_arr([16, 136])) == 0
    assert lib.mrec_ncf_supported(8, 4, widths_arr([16, 8, 8, 8])) == 0
    assert lib.mrec_ncf_supported(8, 0, widths_arr([])) == 0
    assert lib.mrec_ncf_supported(8, 2, None) == 0
    assert dense.ncf_supported(24, [16, 8]) is False and dense.ncf_supported(8, [20]) is False
    assert dense.ncf_supported(8, [16, 8, 8, 8]) is False
    assert dense.NCF_FUSED is True
