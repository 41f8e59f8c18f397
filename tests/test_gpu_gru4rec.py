"""The fused GRU4Rec encoder (mrec_gru_fwd / _bwd + mrec_sasrec_wgrad, gru.hip) on the
GPU: parity with an fp64 restatement on every sample with the layered GPU path as the
yardstick, run-to-run bit equality, the dead positions, the tile order, saturated gates,
the fallbacks to the layered path, and golden G16 through the whole model.

Bars (those of test_gpu_sasrec.py): per quantity, max error <= max(tol, 1.5 x the layered
path's max error) with tol 3e-2 forward / 5e-2 gradients, relative to the quantity's
magnitude, and mean error <= max(3e-3, 1.5 x the layered path's mean error).  Both GPU
paths round x, the two weight matrices and h as a matmul operand to bf16; the fp64
restatement rounds nothing.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from test_gru4rec_cpu import KEYS, g16_batch, g16_state, gru4rec

pytestmark = pytest.mark.gpu

NAMES = ("W_ih", "W_hh", "b_ih", "b_hh")


def _params(m):
    from pytorchrec_amd import dense as D
    return D._gru_params(m)


def _second_tile_batch():
    """A batch with more tiles than workgroups: some workgroup takes a second tile."""
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    return (int(lib.mrec_gru_parts(1 << 20)) + 1) * int(lib.mrec_gru_tile()) + 3


def lively_(m, seed, scale=0.3):
    """State-B scale: the four GRU tensors ``scale`` N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in _params(m):
            p.copy_((scale * torch.randn(p.shape, generator=g)).to(p.device))
    return m


@functools.lru_cache(maxsize=None)
def _case(B, L, E, H, full=False, scale=0.3):
    """(model, rows bf16 [B, L, E], his_len, dh) on cuda:0.  Sample 0 has length 1, sample
    1 length L; the rest random lengths (all L with ``full``).  (24, 12, 16, 32) is G16's
    batch."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + L + B)
    if (B, L, E, H) == (24, 12, 16, 32):
        lens = torch.from_numpy(golden("g16_gru4rec.npz")["his_len"])
    else:
        lens = torch.full((B,), L) if full else torch.randint(1, L + 1, (B,), generator=g)
        if not full:
            lens[0] = 1
        lens[1] = L
    assert full or lens[0] == 1
    assert lens[1] == L
    m = lively_(gru4rec(items=50, emb_size=E, hidden_size=H, max_his_len=L, device=dev), 7 + E + H,
                scale)
    rows = (0.3 * torch.randn(B, L, E, generator=g)).to(torch.bfloat16).to(dev)
    dh = torch.randn(B, H, generator=g).to(dev)
    return m, rows, lens.to(dev), dh


@functools.lru_cache(maxsize=None)
def _ref64(B, L, E, H, full=False, scale=0.3):
    """fp64 torch restatement of the recurrence and its gradients (computed once)."""
    m, rows, lens, dh = _case(B, L, E, H, full, scale)
    x = rows.detach().double().cpu().requires_grad_()
    ps = [p.detach().double().cpu().requires_grad_() for p in _params(m)]
    w_ih, w_hh, b_ih, b_hh = ps
    lens = lens.cpu().long()
    h = torch.zeros(B, H, dtype=torch.float64)
    gx = x @ w_ih.T + b_ih
    for t in range(L):
        gh = h @ w_hh.T + b_hh
        xr, xz, xn = gx[:, t].split(H, 1)
        hr, hz, hn = gh.split(H, 1)
        r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        h = torch.where((lens > t)[:, None], (1 - z) * n + z * h, h)
    h.backward(dh.double().cpu())
    ref = {"h": h.detach(), "dX": x.grad}
    ref.update({"d" + n: p.grad for n, p in zip(NAMES, ps)})
    return ref


def _run(case, fused, monkeypatch, rows=None, order="auto"):
    """One forward + backward of dense.gru_encode -> {h, dX, d<param>}."""
    from pytorchrec_amd import dense as D
    m, rows0, lens, dh = case
    monkeypatch.setattr(D, "GRU_FUSED", fused)
    for p in _params(m):
        p.grad = None
    x = (rows0 if rows is None else rows).detach().clone().requires_grad_()
    h = D.gru_encode(x, lens, m.eval(), order=order)
    assert ("Gru" in type(h.grad_fn).__name__) == fused
    h.backward(dh)
    got = {"h": h.detach(), "dX": x.grad}
    got.update({"d" + n: p.grad.clone() for n, p in zip(NAMES, _params(m))})
    return got


def _errs(got, want):
    """(max, mean) |got - want| relative to max |want|."""
    d = (got.detach().double().cpu() - want.double()).abs()
    mag = max(want.abs().max().item(), 1e-12)
    return d.max().item() / mag, d.mean().item() / mag


def _meets_bars(errs, names):
    for name in names:
        (fmax, fmean), (lmax, lmean) = errs[(True, name)], errs[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} "
              f"mean {lmean:.2e}")
    for name in names:
        (fmax, fmean), (lmax, lmean) = errs[(True, name)], errs[(False, name)]
        tol = 3e-2 if name in ("h", "prediction", "loss") else 5e-2
        assert fmax <= max(tol, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


SHAPES = [(37, 1, 16, 16, False), (24, 12, 16, 32, False), (50, 37, 32, 64, False),
          (48, 64, 64, 64, True), (300, 50, 64, 16, False), (None, 3, 16, 16, False)]


@pytest.mark.parametrize("B,L,E,H,full", SHAPES)
def test_fused_encoder_matches_fp64_reference(gpu, monkeypatch, B, L, E, H, full):
    """h_last, the rows' gradient and all four dense gradients on every sample.  One step
    (h_-1 = 0: dW_hh is bitwise zero, db_hh is not), G16's batch with E < H, odd L with a
    ragged last tile, every sample at the full 64 steps, E > H with one wave per
    workgroup, and more tiles than workgroups (a workgroup's accumulators and h across
    its second tile)."""
    if B is None:
        B = _second_tile_batch()
    case, ref = _case(B, L, E, H, full), _ref64(B, L, E, H, full)
    errs = {}
    for fused in (True, False):
        got = _run(case, fused, monkeypatch)
        for name, t in got.items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errs[(fused, name)] = _errs(t, ref[name])
        if fused and L == 1:
            assert (got["dW_hh"].view(torch.int32) == 0).all()
            assert (got["db_hh"] != 0).any()
    _meets_bars(errs, list(ref))


def test_two_runs_are_bitwise_equal(gpu, monkeypatch):
    case = _case(300, 50, 64, 64)
    a, b = _run(case, True, monkeypatch), _run(case, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_dead_positions_get_zero_gradient_and_do_not_matter(gpu, monkeypatch):
    """dX is bitwise zero at t >= his_len and non-zero at live positions, and every output
    is bitwise unchanged when the rows there hold other finite values (1e3)."""
    case = _case(300, 50, 64, 64)
    m, rows, lens, dh = case
    live = torch.arange(50, device=rows.device)[None, :] < lens[:, None]
    assert (~live).any()
    a = _run(case, True, monkeypatch)
    assert a["dX"].dtype == torch.bfloat16
    assert (a["dX"][~live].view(torch.int16) == 0).all()
    assert (a["dX"][live].float().abs().sum(-1) > 0).all()
    loud = rows.clone()
    loud[~live] = 1e3
    b = _run(case, True, monkeypatch, rows=loud)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_the_tile_order_changes_nothing_per_sample(gpu, monkeypatch):
    """Batch order, sorted by length and a random permutation: h_last and dX are bitwise
    equal (samples are independent MFMA rows); the dense gradients agree to 1e-5 of their
    magnitude (only their summation order moved)."""
    case = _case(300, 50, 64, 64)
    lens = case[2]
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(4)).to(lens.device)
    base = _run(case, True, monkeypatch, order=None)
    for order in (torch.argsort(lens, descending=True), perm):
        got = _run(case, True, monkeypatch, order=order)
        for name in ("h", "dX"):
            assert torch.equal(got[name], base[name]), name
        for name in ("d" + n for n in NAMES):
            fmax, _ = _errs(got[name], base[name].double().cpu())
            print(f"{name}: {fmax:.2e}")
            assert fmax <= 1e-5, (name, fmax)


def test_saturated_gates_stay_finite(gpu, monkeypatch):
    """Weights and biases 10 N(0, 1): pre-activations of +-100 and beyond.  Every fused
    output is finite and h_last meets the forward bar."""
    shape = (16, 8, 16, 16, False, 10.0)
    case, ref = _case(*shape), _ref64(*shape)
    errs = {}
    for fused in (True, False):
        got = _run(case, fused, monkeypatch)
        if fused:
            for name, t in got.items():
                assert torch.isfinite(t.float()).all(), name
        errs[(fused, "h")] = _errs(got["h"], ref["h"])
    _meets_bars(errs, ["h"])


@pytest.mark.parametrize("E,H,L", [(24, 32, 12), (16, 48, 12), (16, 16, 65)])
def test_unsupported_shapes_take_the_layered_path(gpu, monkeypatch, E, H, L):
    from pytorchrec_amd import cpu_path, dense
    assert dense.GRU_FUSED
    B = 9
    m = lively_(gru4rec(items=50, emb_size=E, hidden_size=H, max_his_len=L, device=gpu), 3)
    g = torch.Generator().manual_seed(L)
    lens = torch.randint(1, L + 1, (B,), generator=g).to(gpu)
    rows = (0.3 * torch.randn(B, L, E, generator=g)).to(torch.bfloat16).to(gpu)
    dh = torch.randn(B, H, generator=g).to(gpu)

    def direct(x):
        return cpu_path.gru_encode(x, lens, *_params(m), rnd=cpu_path.bf16_round)

    out = []
    for fn in (lambda x: dense.gru_encode(x, lens, m), direct):
        for p in _params(m):
            p.grad = None
        x = rows.clone().requires_grad_()
        h = fn(x)
        assert "Gru" not in type(h.grad_fn).__name__
        h.backward(dh)
        out.append([h.detach(), x.grad] + [p.grad.clone() for p in _params(m)])
    for i, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), i


def test_the_switch_selects_the_layered_path_bit_for_bit(gpu, monkeypatch):
    from pytorchrec_amd import cpu_path
    case = _case(24, 12, 16, 32)
    m, rows, lens, dh = case
    got = _run(case, False, monkeypatch)
    for p in _params(m):
        p.grad = None
    x = rows.clone().requires_grad_()
    h = cpu_path.gru_encode(x, lens, *_params(m), rnd=cpu_path.bf16_round)
    h.backward(dh)
    want = [h.detach(), x.grad] + [p.grad for p in _params(m)]
    for a, b in zip(got.values(), want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# golden G16 through the model
# ---------------------------------------------------------------------------

def _g16_model(gpu, which):
    g = golden("g16_gru4rec.npz")
    m = gru4rec(device=gpu)
    assert m.i_embeddings.weight.dtype == torch.float32 and m.i_embeddings.weight.is_cuda
    assert all(p.is_cuda for p in m.parameters())
    if which == "B":
        m.load_state_dict(g16_state(g, "B"))
    return g, m


def test_g16_state_b_forward_through_the_model(gpu, monkeypatch):
    from pytorchrec_amd import dense as D
    errs = {}
    for fused in (True, False):
        monkeypatch.setattr(D, "GRU_FUSED", fused)
        g, m = _g16_model(gpu, "B")
        with torch.no_grad():
            pred, target = m.eval()(g16_batch(g, gpu))
        assert pred.shape == (24, 5) and np.array_equal(target.cpu().numpy(), g["A_target"])
        errs[(fused, "prediction")] = _errs(pred, torch.from_numpy(g["B_pred"]))
    _meets_bars(errs, ["prediction"])


@pytest.mark.parametrize("which", ["A", "B"])
def test_g16_train_step_through_the_model(gpu, monkeypatch, which):
    """One train_step from the seed-2020 initialisation (MSE, SGD lr 0.5) and one from the
    lively state B (MSE against a zero label = prediction.square().mean(), SGD lr 0.05):
    all six tensors after the step (and state A's loss) against the reference's, fused and
    layered."""
    from pytorchrec_amd import dense as D
    errs, calls = {}, []
    real = D._GruFn.apply
    monkeypatch.setattr(D._GruFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    for fused in (True, False):
        monkeypatch.setattr(D, "GRU_FUSED", fused)
        g, m = _g16_model(gpu, which)
        batch = g16_batch(g, gpu)
        if which == "A":
            sd = m.state_dict()
            for k in KEYS:  # the GPU-built model draws the same bits
                assert np.array_equal(sd[k].cpu().numpy().view(np.uint32),
                                      g[f"A::{k}"].view(np.uint32)), k
        else:
            batch["label"] = torch.zeros_like(batch["label"])
        lr = float(g["lr"] if which == "A" else g["lr_b"])
        m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), torch.nn.MSELoss(), [], gpu)
        loss = float(m.train_step(batch)["loss"].detach())
        assert np.isfinite(loss)
        if which == "A":
            errs[(fused, "loss")] = (abs(loss - float(g["A_loss"])) / abs(float(g["A_loss"])),) * 2
        sd = m.state_dict()
        for k in KEYS:
            errs[(fused, k)] = _errs(sd[k], torch.from_numpy(g[f"{which}_after::{k}"]))
            moved = torch.from_numpy(g[f"{which}_after::{k}"] - g[f"{which}::{k}"])
            dmax, _ = _errs(sd[k].cpu() - torch.from_numpy(g[f"{which}::{k}"]), moved)
            print(f"{'fused' if fused else 'layered'} {k}: update max {dmax:.2e} of its "
                  f"magnitude {moved.abs().max().item():.2e}")
    assert len(calls) == 1  # the fused step went through the kernels, exactly once
    _meets_bars(errs, (("loss",) if which == "A" else ()) + KEYS)


def test_padding_slots_equal_the_plain_ids(gpu):
    """``pad_skip`` (positions past the length as padding slots of the gather) against the
    plain ids: the same predictions bit for bit, the same tensors after one train step
    (dense ones bit for bit; the table to 1e-6 of its magnitude, its segment sums may run
    in another order), and a negative id is still an IndexError."""
    g = golden("g16_gru4rec.npz")
    out = {}
    for skip in (True, False):
        m = gru4rec(device=gpu)
        m.load_state_dict(g16_state(g, "B"))
        m.pad_skip = skip
        with torch.no_grad():
            pred = m.eval()(g16_batch(g, gpu))[0]
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.05), torch.nn.MSELoss(), [], gpu)
        m.train_step(g16_batch(g, gpu))
        out[skip] = (pred, m.state_dict())
    assert torch.equal(out[True][0], out[False][0])
    for k in KEYS:
        a, b = out[True][1][k], out[False][1][k]
        assert not torch.equal(a.cpu(), torch.from_numpy(g[f"B::{k}"])), k  # (the step moved it)
        if k == "i_embeddings.weight":
            torch.testing.assert_close(a, b, rtol=0, atol=1e-6 * b.abs().max().item())
        else:
            assert torch.equal(a, b), k
    m = gru4rec(device=gpu)
    assert int(g["his_len"][5]) >= 2
    for key, at in (("his", (5, 1)), ("his", (5, 0)), ("iid", (4, 2))):
        batch = g16_batch(g, gpu)
        batch[key] = batch[key].clone()
        batch[key][at] = -3
        with pytest.raises(IndexError):
            m.eval()(batch)


@pytest.mark.parametrize("bad", [0, 13])
def test_a_length_outside_the_history_is_an_index_error(gpu, bad):
    """The kernel clamps the length and sets the flag (nothing is read out of bounds);
    checking mode raises, the fast path stays finite."""
    g, m = _g16_model(gpu, "B")
    assert m.i_embeddings.check_ids
    batch = g16_batch(g, gpu)
    batch["his_len"] = batch["his_len"].clone()
    batch["his_len"][3] = bad
    with pytest.raises(IndexError):
        m.eval()(batch)
    m.i_embeddings.check_ids = False  # the fast path: no sync, a finite result
    with torch.no_grad():
        pred, _ = m(batch)
    assert torch.isfinite(pred).all()
