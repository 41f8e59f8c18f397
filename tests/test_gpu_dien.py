"""The fused DIEN interest evolution (mrec_interest_fwd / _bwd, augru.hip) on the GPU:
parity with ``cpu_path.interest_evolution`` in fp64 on the same bf16-rounded inputs, with
the layered GPU path as the yardstick; dead positions; run-to-run and tile-order bit
equality; saturated gates and scores; the fallbacks; one model train step.

Bars (test_gpu_gru4rec.py's): per quantity, max error <= max(tol, 1.5 x the layered
path's max error), tol 3e-2 forward / 5e-2 gradients, relative to the quantity's largest
magnitude.
"""
import functools

import pytest
import torch

from test_dien_cpu import dien, dien_batch

pytestmark = pytest.mark.gpu

NAMES = ("w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_ih2", "w_hh2", "b_ih2", "b_hh2")
FWD = ("v", "hs1", "loss")


def _second_tile_batch():
    """A batch with more tiles than workgroups: some workgroup takes a second tile."""
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    return (int(lib.mrec_interest_parts(1 << 20)) + 1) * int(lib.mrec_interest_tile()) + 3


@functools.lru_cache(maxsize=None)
def _case(B, L, E, H, full=False, scale=0.3):
    """(x bf16 [B, L, E], his_len, p, params, dv, d_hs1) on cuda:0; sample 0 has length 1 and
    sample 1 length L unless ``full`` (every length L)."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + 7 * B + L + E + H)
    lens = torch.full((B,), L) if full else torch.randint(1, L + 1, (B,), generator=g)
    if not full:
        lens[0], lens[1] = 1, L
    shapes = [(3 * H, E), (3 * H, H), (3 * H,), (3 * H,), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,)]
    params = tuple((scale * torch.randn(s, generator=g)).to(dev) for s in shapes)
    x = (0.3 * torch.randn(B, L, E, generator=g)).to(torch.bfloat16).to(dev)
    p = (0.5 * torch.randn(B, H, generator=g)).to(dev)
    dv, d_hs1 = torch.randn(B, H, generator=g).to(dev), torch.randn(B, L, H, generator=g).to(dev)
    return x, lens.to(torch.int32).to(dev), p, params, dv, d_hs1


def _run(case, mode, monkeypatch=None, x=None, d_hs1="case", order="auto"):
    """One forward + backward -> {v, hs1, dx, dp, d<param>}.  mode: "fused", "layered"
    (the torch-ops GPU path) or "fp64" (cpu_path on the CPU, nothing rounded)."""
    from pytorchrec_amd import cpu_path, dense as D
    x0, lens, p0, params, dv, dh1 = case
    dh1 = dh1 if isinstance(d_hs1, str) else d_hs1
    x = x0 if x is None else x
    if mode == "fp64":
        x, lens, p0, dv = x.double().cpu(), lens.cpu(), p0.double().cpu(), dv.double().cpu()
        params = [w.double().cpu() for w in params]
        dh1 = None if dh1 is None else dh1.double().cpu()
    x = x.detach().clone().requires_grad_()
    p = p0.detach().clone().requires_grad_()
    ws = [w.detach().clone().requires_grad_() for w in params]
    if mode == "fp64":
        v, hs1 = cpu_path.interest_evolution(x, lens, p, *ws)
    else:
        monkeypatch.setattr(D, "DIEN_FUSED", mode == "fused")
        v, hs1 = D.interest_evolution(x, lens, p, ws, order=order)
        assert ("Interest" in type(v.grad_fn).__name__) == (mode == "fused")
    # d_hs1 goes in as it is, dead positions included: nothing may read it there
    if dh1 is None:
        v.backward(dv)
    else:
        torch.autograd.backward([v, hs1], [dv, dh1])
    got = {"v": v.detach(), "hs1": hs1.detach(), "dx": x.grad, "dp": p.grad}
    got.update({"d" + n: w.grad for n, w in zip(NAMES, ws)})
    return got


_ref64 = functools.lru_cache(maxsize=None)(lambda *key: _run(_case(*key), "fp64"))


def _errs(got, want):
    d = (got.detach().double().cpu() - want.double()).abs()
    return d.max().item() / max(want.abs().max().item(), 1e-12)


def _meets_bars(fused, layered, ref):
    errs = {n: (_errs(fused[n], ref[n]), _errs(layered[n], ref[n])) for n in ref}
    for n, (f, l) in errs.items():
        print(f"{n}: fused {f:.2e} | layered {l:.2e}")
    for n, (f, l) in errs.items():
        assert torch.isfinite(fused[n].float()).all(), n
        assert f <= max(3e-2 if n in FWD else 5e-2, 1.5 * l), (n, f, l)


def _same_bits(a, b, names=None):
    for n in names or a:
        assert torch.equal(a[n].view(torch.int16 if a[n].dtype == torch.bfloat16 else torch.int32),
                           b[n].view(torch.int16 if b[n].dtype == torch.bfloat16 else torch.int32)), n


SHAPES = [(3, 1, 16, 16, False), (17, 5, 16, 16, False), (16, 64, 32, 64, True),
          (33, 12, 64, 32, False), (20, 7, 64, 64, False), (None, 3, 16, 16, False)]


@pytest.mark.parametrize("B,L,E,H,full", SHAPES)
def test_fused_interest_evolution_matches_fp64(gpu, monkeypatch, B, L, E, H, full):
    """v, hs1, dx, dp and the eight dense gradients.  One step (a = 1), a partial second
    tile, the longest history with E < H, E > H over three tiles, the register-heaviest
    shape, and more tiles than workgroups (a workgroup adds its second tile's gradients
    to its own partial)."""
    key = (_second_tile_batch() if B is None else B, L, E, H, full)
    case = _case(*key)
    _meets_bars(_run(case, "fused", monkeypatch), _run(case, "layered", monkeypatch), _ref64(*key))


def test_without_d_hs1(gpu, monkeypatch):
    case = _case(33, 12, 64, 32)
    ref = _run(case, "fp64", d_hs1=None)
    _meets_bars(_run(case, "fused", monkeypatch, d_hs1=None),
                _run(case, "layered", monkeypatch, d_hs1=None), ref)


def test_dead_positions_never_matter(gpu, monkeypatch):
    """NaN / inf rows and garbage d_hs1 at t >= his_len change no bit; dx and hs1 are
    bitwise zero there."""
    case = _case(33, 12, 64, 32)
    x, lens, _, _, _, dh1 = case
    dead = (torch.arange(12, device=x.device)[None] >= lens[:, None]).unsqueeze(-1)
    junk = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38], device=x.device)
    xj = torch.where(dead, junk.to(torch.bfloat16)[torch.arange(x.numel(), device=x.device) % 4].view_as(x), x)
    dj = torch.where(dead, junk[torch.arange(dh1.numel(), device=x.device) % 4].view_as(dh1), dh1)
    clean = _run(case, "fused", monkeypatch, x=torch.where(dead, torch.zeros_like(x), x),
                 d_hs1=torch.where(dead, torch.zeros_like(dh1), dh1))
    dirty = _run(case, "fused", monkeypatch, x=xj, d_hs1=dj)  # dj reaches the kernel unmasked
    _same_bits(clean, dirty)
    assert (dirty["dx"].view(torch.int16)[dead.expand_as(x)] == 0).all()
    assert (dirty["hs1"].view(torch.int32)[dead.expand_as(dh1)] == 0).all()


def test_bits_do_not_depend_on_the_run_or_the_tile_order(gpu, monkeypatch):
    case = _case(33, 12, 64, 32)
    a, b = _run(case, "fused", monkeypatch), _run(case, "fused", monkeypatch)
    _same_bits(a, b)
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    c = _run(case, "fused", monkeypatch, order=perm)
    _same_bits(a, c, ("v", "hs1", "dx", "dp"))  # per sample; the dense sums change their order
    big = _case(_second_tile_batch(), 3, 16, 16)
    _same_bits(_run(big, "fused", monkeypatch), _run(big, "fused", monkeypatch))


def test_saturated_gates_and_scores_stay_finite(gpu, monkeypatch):
    """Pre-activations ~1e4 and scores where one position dominates by ~1e4."""
    from pytorchrec_amd import dense as D
    x, lens, p, params, dv, dh1 = _case(20, 7, 64, 64, False, 300.0)
    got = _run((x * 10, lens, p * 2e4, params, dv, dh1), "fused", monkeypatch)
    for n, t in got.items():
        assert torch.isfinite(t.float()).all(), n
    # |h1| -> 1, so a sample's scores differ by ~|p| ~ 1e4: the dominated positions' a is 0
    monkeypatch.setattr(D, "DIEN_FUSED", True)
    v, _ = D.interest_evolution(x * 10, lens, p * 2e4, [w.detach().clone().requires_grad_() for w in params])
    a = v.grad_fn.att  # the attention weights the forward saved [B, L]
    live = torch.arange(7, device=a.device)[None] < lens[:, None]
    assert torch.isfinite(a).all() and (a[live] == 0).any() and (a[~live] == 0).all()
    assert torch.allclose(a.sum(1), torch.ones_like(a.sum(1)), atol=1e-5)


@pytest.mark.parametrize("E,H,L", [(24, 32, 12), (16, 48, 12), (16, 16, 65)])
def test_uncompiled_shapes_take_the_torch_ops_path(gpu, E, H, L):
    from pytorchrec_amd import dense as D
    assert not D.interest_supported(E, H, L)
    x, lens, p, params, _, _ = _case(5, L, E, H)
    v, hs1 = D.interest_evolution(x, lens, p, [w.requires_grad_() for w in params])
    assert "Interest" not in type(v.grad_fn).__name__ and v.shape == (5, H) and hs1.shape == (5, L, H)


def test_switch_gives_the_torch_ops_path_bit_for_bit(gpu, monkeypatch):
    from pytorchrec_amd import cpu_path
    case = _case(17, 5, 16, 16)
    x, lens, p, params, _, _ = case
    got = _run(case, "layered", monkeypatch)
    v, hs1 = cpu_path.interest_evolution(x, lens, p, *params, rnd=cpu_path.bf16_round)
    assert torch.equal(got["v"], v) and torch.equal(got["hs1"], hs1)


def test_model_train_step_fused_against_layered(gpu, monkeypatch):
    """One SGD step with the negative history and aux_weight = 1, fused against the layered
    GPU path: the loss, and every parameter's update within 5e-2 of the largest update of
    that parameter; the rows that only padded slots name are untouched."""
    from pytorchrec_amd import dense as D
    dev = torch.device("cuda:0")
    data = dien_batch(B=40, L=9, seed=5, device=dev)
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(D, "DIEN_FUSED", fused)
        m = dien(emb_size=16, device=dev, seed=11, neg=True, lr=0.5)
        g = torch.Generator().manual_seed(12)
        with torch.no_grad():  # lively weights and rows, so that every update is far above an ulp
            for w in m.parameters():
                if w is m.embeddings.weight:
                    w.mul_(30.0)
                else:
                    w.copy_((0.3 * torch.randn(w.shape, generator=g)).to(dev))
        before = {k: v.detach().float().clone() for k, v in m.state_dict().items()}
        loss = m.train_step(data)["loss"].detach().float().item()
        out[fused] = loss, {k: v.detach().float() - before[k] for k, v in m.state_dict().items()}, before
    (lf, df, before), (ll, dl, _) = out[True], out[False]
    print(f"loss fused {lf:.6f} layered {ll:.6f}")
    assert abs(lf - ll) <= 3e-2 * abs(ll)
    for k in dl:
        d, mag = (df[k] - dl[k]).abs().max().item(), dl[k].abs().max().item()
        print(f"{k}: update differs by {d:.2e} of {mag:.2e}")
        assert mag > 0 and d <= 5e-2 * mag, (k, d, mag)
    # the padded slots name id 0 of both tables, which no live position uses
    cat0 = m.embeddings.category_nums[0]
    rows = df[[k for k in df if "embeddings" in k][0]]
    assert rows.abs().sum() > 0 and (rows[0] == 0).all() and (rows[cat0] == 0).all()
