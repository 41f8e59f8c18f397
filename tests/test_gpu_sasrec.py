"""The fused SASRec encoder (mrec_sasrec_fwd / _bwd / _wgrad, sasrec.hip) on the GPU:
parity with an fp64 restatement on every sample with the layered GPU path as the
yardstick, run-to-run bit equality, the exactly-zero gradient of invalid positions, the
fallbacks to the layered path, and golden G15 through the whole model.

Bars (those of test_din_fused_unit_matches_fp64_reference): per quantity, max error <=
max(tol, 1.5 x the layered path's max error) with tol 3e-2 forward / 5e-2 gradients,
relative to the quantity's magnitude, and mean error <= max(3e-3, 1.5 x the layered
path's mean error).  Both GPU paths round X, the weights and the matmul operands to
bf16; the fp64 restatement rounds nothing.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from test_sasrec_cpu import KEYS, g15_batch, g15_state, sasrec

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 16, 1, False), (24, 12, 16, 2, False), (64, 37, 32, 3, False),
          (48, 64, 64, 2, True), (300, 50, 64, 2, False)]
NAMES = ("pos", "Wq", "Wk", "W1", "b1", "W2", "b2", "gamma", "beta")


def _params(m):
    from pytorchrec_amd import dense as D
    return D._sasrec_params(m)


def lively_(m, seed):
    """State-B scale: embeddings and Linears N(0, 0.3), LayerNorm 1 + 0.2 N / 0.2 N."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p, name in zip(_params(m), NAMES):
            n = torch.randn(p.shape, generator=g)
            p.copy_((1.0 + 0.2 * n if name == "gamma" else 0.2 * n if name == "beta"
                     else 0.3 * n).to(p.device))
    return m


@functools.lru_cache(maxsize=None)
def _case(B, L, D, layers, full):
    """(model, rows bf16 [B, L, D], his, his_len, dv) on cuda:0.  Sample 0 has length 1,
    sample 1 length L, sample 2 is the forced-valid PAD row (his[2, 0] == 0); the rest
    random lengths (all L with ``full``), tail-padded with 0.  (24, 12, 16, 2) is G15's
    batch."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + L)
    if (B, L, D, layers) == (24, 12, 16, 2):
        g15 = golden("g15_sasrec.npz")
        his, lens = torch.from_numpy(g15["his"]), torch.from_numpy(g15["his_len"])
    else:
        lens = torch.full((B,), L) if full else torch.randint(1, L + 1, (B,), generator=g)
        lens[0], lens[1], lens[2] = 1, L, 1
        his = torch.randint(1, 1000, (B, L), generator=g)
        his[torch.arange(L)[None, :] >= lens[:, None]] = 0
        his[2] = 0
    assert his[2, 0] == 0 and lens[0] == 1 and lens[1] == L and (his[1] > 0).all()
    m = lively_(sasrec(items=50, emb_size=D, max_his_len=L, num_layers=layers, device=dev), 7 + D)
    rows = (0.3 * torch.randn(B, L, D, generator=g)).to(torch.bfloat16).to(dev)
    dv = torch.randn(B, D, generator=g).to(dev)
    return m, rows, his.to(dev), lens.to(dev), dv


@functools.lru_cache(maxsize=None)
def _ref64(B, L, D, layers, full):
    """fp64 torch restatement of the encoder and its gradients (computed once)."""
    m, rows, his, lens, dv = _case(B, L, D, layers, full)
    x0 = rows.detach().double().cpu().requires_grad_()
    ps = [p.detach().double().cpu().requires_grad_() for p in _params(m)]
    pos_w, wq, wk, w1, b1, w2, b2, ga, be = ps
    his, hl = his.cpu(), lens.cpu().long()
    valid = his > 0
    valid[:, 0] = True
    pos = (hl[:, None] - torch.arange(L)[None, :]) * valid.long()
    x = x0 + pos_w[pos]
    for _ in range(layers):
        q, k = x @ wq.T, x @ wk.T
        s = (q @ k.transpose(1, 2)) * D ** -0.5
        a = torch.softmax(s.masked_fill(~valid[:, None, :], float("-inf")), -1)
        f = torch.relu(a @ k @ w1.T + b1)
        x = torch.nn.functional.layer_norm(x + f @ w2.T + b2, (D,), ga, be, m.layer_norm.eps)
    v = (x * valid[..., None]).sum(1) / hl[:, None].double()
    v.backward(dv.double().cpu())
    ref = {"v": v.detach(), "dX": x0.grad}
    ref.update({"d" + n: p.grad for n, p in zip(NAMES, ps)})
    return ref


def _run(case, fused, monkeypatch, rows=None):
    """One forward + backward of dense.sasrec_encode -> {v, dX, d<param>}."""
    from pytorchrec_amd import dense as D
    m, rows0, his, lens, dv = case
    monkeypatch.setattr(D, "SASREC_FUSED", fused)
    for p in _params(m):
        p.grad = None
    x = (rows0 if rows is None else rows).detach().clone().requires_grad_()
    v = D.sasrec_encode(x, his, lens, m.eval())
    assert ("Sasrec" in type(v.grad_fn).__name__) == fused
    v.backward(dv)
    got = {"v": v.detach(), "dX": x.grad}
    got.update({"d" + n: p.grad.clone() for n, p in zip(NAMES, _params(m))})
    return got


def _errs(got, want):
    """(max, mean) |got - want| relative to max |want|."""
    d = (got.detach().double().cpu() - want.double()).abs()
    mag = max(want.abs().max().item(), 1e-12)
    return d.max().item() / mag, d.mean().item() / mag


@pytest.mark.parametrize("B,L,D,layers,full", SHAPES)
def test_fused_encoder_matches_fp64_reference(gpu, monkeypatch, B, L, D, layers, full):
    """Forward v, the rows' gradient and all nine dense gradients on every sample.
    L = 1 (one key: the softmax gradient is exactly zero), G15's batch, odd L with three
    layers at D = 32, L = 64 (no padded rows), and B = 300 on 256 CUs (uneven samples
    per workgroup, gradients accumulated over samples and layers in registers)."""
    case, ref = _case(B, L, D, layers, full), _ref64(B, L, D, layers, full)
    errs = {}
    for fused in (True, False):
        got = _run(case, fused, monkeypatch)
        for name, t in got.items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errs[(fused, name)] = _errs(t, ref[name])
    for name in ref:
        (fmax, fmean), (lmax, lmean) = errs[(True, name)], errs[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} "
              f"mean {lmean:.2e}")
    for name in ref:
        (fmax, fmean), (lmax, lmean) = errs[(True, name)], errs[(False, name)]
        tol = 3e-2 if name == "v" else 5e-2
        assert fmax <= max(tol, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


def test_two_runs_are_bitwise_equal(gpu, monkeypatch):
    case = _case(300, 50, 64, 2, False)
    a, b = _run(case, True, monkeypatch), _run(case, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_invalid_positions_get_zero_gradient_and_do_not_matter(gpu, monkeypatch):
    """dX is bitwise zero at invalid positions, and v, dX and every dense gradient are
    bitwise unchanged when the item rows there hold other finite values (1e3)."""
    case = _case(300, 50, 64, 2, False)
    m, rows, his, lens, dv = case
    valid = his > 0
    valid[:, 0] = True
    assert (~valid).any()
    a = _run(case, True, monkeypatch)
    assert a["dX"].dtype == torch.bfloat16
    assert (a["dX"][~valid].view(torch.int16) == 0).all()
    assert (a["dX"][valid].float().abs().sum(-1) > 0).all()
    loud = rows.clone()
    loud[~valid] = 1e3
    b = _run(case, True, monkeypatch, rows=loud)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _direct_layered(m, rows, his, lens):
    from pytorchrec_amd import cpu_path, dense as D
    return cpu_path.sasrec_encode(rows, his, lens, *D._sasrec_params(m), m.layer_norm.eps,
                                  m.num_layers, dropout=m.dropout, training=m.training,
                                  rnd=cpu_path.bf16_round)


@pytest.mark.parametrize("D,L,dropout", [(24, 12, 0.0), (16, 65, 0.0), (16, 12, 0.5)])
def test_unsupported_shapes_and_dropout_take_the_layered_path(gpu, D, L, dropout):
    from pytorchrec_amd import dense
    assert dense.SASREC_FUSED
    B = 9
    m = lively_(sasrec(items=50, emb_size=D, max_his_len=L, num_layers=2, dropout=dropout,
                       device=gpu), 3)
    m.train()
    g = torch.Generator().manual_seed(L)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    his = torch.randint(1, 50, (B, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    his, lens = his.to(gpu), lens.to(gpu)
    rows = (0.3 * torch.randn(B, L, D, generator=g)).to(torch.bfloat16).to(gpu)
    dv = torch.randn(B, D, generator=g).to(gpu)
    out = []
    for fn in (lambda x: dense.sasrec_encode(x, his, lens, m), lambda x: _direct_layered(m, x, his, lens)):
        for p in _params(m):
            p.grad = None
        x = rows.clone().requires_grad_()
        torch.manual_seed(5)
        v = fn(x)
        assert "Sasrec" not in type(v.grad_fn).__name__
        v.backward(dv)
        out.append([v.detach(), x.grad] + [p.grad.clone() for p in _params(m)])
    for i, (a, b) in enumerate(zip(*out)):
        if i == 2:  # the position rows' gradient is torch's index_add_ (atomics: its
            # summation order is not fixed), every other op is the same call twice
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
        else:
            assert torch.equal(a, b), i
    if dropout:  # the same model in eval mode runs fused
        v = dense.sasrec_encode(rows.clone().requires_grad_(), his, lens, m.eval())
        assert "Sasrec" in type(v.grad_fn).__name__


def _g15_model(gpu, which):
    g = golden("g15_sasrec.npz")
    m = sasrec(device=gpu)
    assert m.i_embeddings.weight.dtype == torch.float32 and m.i_embeddings.weight.is_cuda
    if which == "B":
        m.load_state_dict(g15_state(g, "B"))
    return g, m


def test_g15_state_b_forward_through_the_model(gpu, monkeypatch):
    from pytorchrec_amd import dense as D
    errs = {}
    for fused in (True, False):
        monkeypatch.setattr(D, "SASREC_FUSED", fused)
        g, m = _g15_model(gpu, "B")
        with torch.no_grad():
            pred, target = m.eval()(g15_batch(g, gpu))
        assert pred.shape == (24, 5) and np.array_equal(target.cpu().numpy(), g["A_target"])
        errs[fused] = _errs(pred, torch.from_numpy(g["B_pred"]))
    print(f"prediction: fused max {errs[True][0]:.2e} mean {errs[True][1]:.2e} | layered max "
          f"{errs[False][0]:.2e} mean {errs[False][1]:.2e}")
    assert errs[True][0] <= max(3e-2, 1.5 * errs[False][0])
    assert errs[True][1] <= max(3e-3, 1.5 * errs[False][1])


def test_g15_state_a_train_step_through_the_model(gpu, monkeypatch):
    """One train_step (MSE, SGD lr 0.5) from the seed-2020 initialisation: the loss and
    all ten tensors after the step against the reference's, fused and layered."""
    from pytorchrec_amd import dense as D
    errs, calls = {}, []
    real = D._SasrecFn.apply
    monkeypatch.setattr(D._SasrecFn, "apply", lambda *a: (calls.append(1), real(*a))[1])
    for fused in (True, False):
        monkeypatch.setattr(D, "SASREC_FUSED", fused)
        g, m = _g15_model(gpu, "A")
        sd = m.state_dict()
        for k in KEYS:  # the GPU-built model draws the same bits
            assert np.array_equal(sd[k].cpu().numpy().view(np.uint32), g[f"A::{k}"].view(np.uint32)), k
        m.compile(torch.optim.SGD(m.get_parameters(), lr=float(g["lr"])), torch.nn.MSELoss(), [], gpu)
        loss = float(m.train_step(g15_batch(g, gpu))["loss"].detach())
        errs[(fused, "loss")] = (abs(loss - float(g["A_loss"])) / abs(float(g["A_loss"])),) * 2
        sd = m.state_dict()
        for k in KEYS:
            errs[(fused, k)] = _errs(sd[k], torch.from_numpy(g[f"A_after::{k}"]))
            moved = torch.from_numpy(g[f"A_after::{k}"] - g[f"A::{k}"])
            dmax, _ = _errs(sd[k].cpu() - torch.from_numpy(g[f"A::{k}"]), moved)
            print(f"{'fused' if fused else 'layered'} {k}: after-step max {errs[(fused, k)][0]:.2e}; "
                  f"update max {dmax:.2e} of its magnitude {moved.abs().max().item():.2e}")
    assert len(calls) == 1  # the fused pass went through the kernels
    for k in ("loss",) + KEYS:
        (fmax, fmean), (lmax, lmean) = errs[(True, k)], errs[(False, k)]
        tol = 3e-2 if k == "loss" else 5e-2
        assert fmax <= max(tol, 1.5 * lmax), (k, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (k, fmean, lmean)


def test_a_history_longer_than_the_table_is_an_index_error(gpu):
    """his_len > L: a position id past the table.  The kernel adds no position row for it
    and sets the flag (nothing is read out of bounds); checking mode raises."""
    g, m = _g15_model(gpu, "B")
    assert m.i_embeddings.check_ids
    batch = g15_batch(g, gpu)
    batch["his_len"] = batch["his_len"].clone()
    batch["his_len"][3] = 13
    with pytest.raises(IndexError):
        m.eval()(batch)
    m.i_embeddings.check_ids = False  # the fast path: no sync, a finite result
    with torch.no_grad():
        pred, _ = m(batch)
    assert torch.isfinite(pred).all()


def test_padding_slots_equal_the_plain_ids(gpu):
    """``pad_skip`` (masked history positions as padding slots of the gather) against the
    plain history ids: the same predictions bit for bit, the same tensors after one
    train step (dense ones bit for bit; the table to 1e-6 of its magnitude, its segment
    sums may run in another order), and a negative id is still an IndexError."""
    g = golden("g15_sasrec.npz")
    out = {}
    for skip in (True, False):
        m = sasrec(device=gpu)
        m.load_state_dict(g15_state(g, "B"))
        m.pad_skip = skip
        with torch.no_grad():
            pred = m.eval()(g15_batch(g, gpu))[0]
        m.compile(torch.optim.SGD(m.get_parameters(), lr=0.05), torch.nn.MSELoss(), [], gpu)
        m.train_step(g15_batch(g, gpu))
        out[skip] = (pred, m.state_dict())
    assert torch.equal(out[True][0], out[False][0])
    for k in KEYS:
        a, b = out[True][1][k], out[False][1][k]
        assert not torch.equal(a.cpu(), torch.from_numpy(g[f"B::{k}"])), k  # (the step moved it)
        if k == "i_embeddings.weight":
            torch.testing.assert_close(a, b, rtol=0, atol=1e-6 * b.abs().max().item())
        else:
            assert torch.equal(a, b), k
    m = sasrec(device=gpu)
    for key, at in (("his", (5, 1)), ("his", (5, 0)), ("iid", (4, 2))):
        batch = g15_batch(g, gpu)
        batch[key] = batch[key].clone()
        batch[key][at] = -3
        with pytest.raises(IndexError):
            m.eval()(batch)
