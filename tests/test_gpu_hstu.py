"""The fused HSTU encoder (mrec_hstu_fwd / _bwd, hstu.hip) on the GPU: parity with the fp64
restatement of test_hstu_cpu.py on every sample with the layered GPU path as the
yardstick, run-to-run bit equality, invalid positions, the dispatch, and the model.

Bars (those of test_gpu_sasrec.py): per quantity, relative to its magnitude, max error <=
max(tol, 1.5 x the layered path's max error) with tol 3e-2 forward / 5e-2 gradients, and
mean error <= max(3e-3, 1.5 x the layered path's mean error).  Both GPU paths round X, the
weights, the matmul operands and each layer's output to bf16; the fp64 restatement rounds
nothing.
"""
import pytest
import torch

from test_hstu_cpu import case, errs, hstu, lively_, params, ref64, run

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 16, 1, 1, False), (24, 12, 32, 2, 2, False), (64, 37, 64, 4, 3, False),
          (48, 64, 64, 1, 2, True), (300, 50, 64, 2, 2, False)]
BIG = (300, 50, 64, 2, 2, False)


def _run(shape, fused, monkeypatch, rows=None):
    from pytorchrec_amd import dense
    monkeypatch.setattr(dense, "HSTU_FUSED", fused)
    got, fn = run(case(*shape, device="cuda:0"), rows=rows)
    assert ("_HstuFn" in type(fn).__name__) == fused
    return got


def _within_bars(errors, names):
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} "
              f"mean {lmean:.2e}")
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        tol = 3e-2 if name in ("v", "loss") else 5e-2
        assert fmax <= max(tol, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


@pytest.mark.parametrize("B,L,D,H,layers,full", SHAPES)
def test_fused_encoder_matches_fp64_reference(gpu, monkeypatch, B, L, D, H, layers, full):
    """v, the rows' gradient and all ten dense gradients on every sample.  L = 1 (one key),
    two heads of 16, odd L with dh = 16 inside D = 64 (the zero-padded k step) and three
    layers, L = 64 with one head of 64 (no padded rows), and B = 300 on 256 CUs (uneven
    shares, gradients accumulated over samples).  The cases with two or more layers pin the
    causal mask: with one layer the output position attends everything valid."""
    shape = (B, L, D, H, layers, full)
    ref, _ = ref64(*shape, device="cuda:0")
    errors = {}
    for fused in (True, False):
        for name, t in _run(shape, fused, monkeypatch).items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errors[(fused, name)] = errs(t, ref[name])
    _within_bars(errors, list(ref))


def test_two_runs_are_bitwise_equal(gpu, monkeypatch):
    a, b = _run(BIG, True, monkeypatch), _run(BIG, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_invalid_positions_get_zero_gradient_and_do_not_matter(gpu, monkeypatch):
    """dX is bitwise zero at invalid positions, and every output is bitwise unchanged when
    the item rows there hold 1e3."""
    _, rows, his, _, _ = case(*BIG, device="cuda:0")
    valid = his > 0
    valid[:, 0] = True
    assert (~valid).any()
    a = _run(BIG, True, monkeypatch)
    assert a["dX"].dtype == torch.bfloat16
    assert (a["dX"][~valid].view(torch.int16) == 0).all()
    assert (a["dX"][valid].float().abs().sum(-1) > 0).all()
    loud = rows.clone()
    loud[~valid] = 1e3
    b = _run(BIG, True, monkeypatch, rows=loud)
    for name in a:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("D,H,L,dropout,fused", [(48, 1, 12, 0.0, False), (16, 1, 65, 0.0, False),
                                                 (16, 1, 12, 0.5, False), (32, 2, 12, 0.0, True)])
def test_dispatch(gpu, D, H, L, dropout, fused):
    """The layered path for a width, a length and (in training) a dropout the kernels do not
    cover; the fused path otherwise, and for the dropout model in eval mode."""
    from pytorchrec_amd import dense
    assert dense.HSTU_FUSED
    m = lively_(hstu(emb_size=D, max_his_len=L, num_heads=H, dropout=dropout, device=gpu), 3).train()
    g = torch.Generator().manual_seed(L)
    lens = torch.randint(1, L + 1, (9,), generator=g)
    his = torch.randint(1, 50, (9, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    rows = (0.3 * torch.randn(9, L, D, generator=g)).to(torch.bfloat16).to(gpu).requires_grad_()
    v = dense.hstu_encode(rows, his.to(gpu), lens.to(gpu), m)
    assert ("_HstuFn" in type(v.grad_fn).__name__) == fused
    v.sum().backward()
    assert torch.isfinite(v).all() and torch.isfinite(rows.grad.float()).all()
    if dropout:
        v = dense.hstu_encode(rows, his.to(gpu), lens.to(gpu), m.eval())
        assert "_HstuFn" in type(v.grad_fn).__name__


def _batch(gpu, B=32, L=12, N=5, items=50):
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    his = torch.randint(1, items, (B, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    return {"iid": torch.randint(1, items, (B, N), generator=g).to(gpu), "his": his.to(gpu),
            "his_len": lens.to(gpu), "label": (torch.rand(B, N, generator=g) < 0.3).long().to(gpu)}


def test_model_train_step_and_item_gradients(gpu, monkeypatch):
    """One ``hstu`` train step gives a finite loss that moves the encoder, and the item
    rows' gradient agrees between the fused and the layered encoder within the bars
    (the fp32 CPU path is the reference)."""
    from pytorchrec_amd import dense
    data = _batch(gpu)
    m = lively_(hstu(emb_size=32, device=gpu), 5)
    before = m.uvqk_weight.detach().clone()
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.01), torch.nn.MSELoss(), [], gpu)
    assert torch.isfinite(m.train_step(data)["loss"].detach()).item()
    assert not torch.equal(before, m.uvqk_weight.detach())
    state = lively_(hstu(emb_size=32), 5).state_dict()
    grads = {}
    for key, dev in ((True, gpu), (False, gpu), ("ref", "cpu")):
        monkeypatch.setattr(dense, "HSTU_FUSED", key is True)
        m = hstu(emb_size=32, device=dev if dev != "cpu" else None)
        m.load_state_dict(state)
        pred, _ = m.eval()({k: t.to(dev) for k, t in data.items()})
        pred.square().mean().backward()
        grads[key] = m.i_embeddings.weight.grad[:, :32]
    errors = {(k, "items"): errs(grads[k], grads["ref"].double()) for k in (True, False)}
    _within_bars(errors, ["items"])


def test_recommend_is_the_brute_force_top_k(gpu):
    m = lively_(hstu(emb_size=32, device=gpu), 5).eval()
    data = _batch(gpu)
    ids, _ = m.recommend(data, 7)
    with torch.no_grad():
        v = m._encode_history(data)
        T = m.i_embeddings.table(0)[:, :32]
        # (retrieval.topk scores bf16(q) . bf16(T[i]))
        scores = v.bfloat16().double() @ T.bfloat16().double().T
    scores[:, 0] = float("-inf")  # id 0 is the padding item (retrieval_low)
    assert torch.equal(ids.long(), scores.topk(7, dim=1).indices)
