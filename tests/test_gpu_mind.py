"""The fused MIND routing (mrec_mind_fwd / _bwd, mind.hip) on the GPU: parity with the fp64
restatement of test_mind_cpu.py on every sample with the layered GPU path as the yardstick,
run-to-run bit equality, invalid positions, the dispatch, and the model.

Bars (those of test_gpu_sasrec.py and test_gpu_hstu.py): per quantity, relative to its
magnitude, max error <= max(tol, 1.5 x the layered path's max error) with tol 3e-2 forward /
5e-2 gradients, and mean error <= max(3e-3, 1.5 x the layered path's mean error).  Both GPU
paths round X, S, H^ and the routing operands to bf16; the fp64 restatement rounds nothing.
"""
import pytest
import torch

from test_mind_cpu import batch, brute_scores, case, errs, mind, ref64, run

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 16, 1, 1, False), (24, 12, 32, 3, 3, False), (64, 37, 64, 8, 3, True),
          (48, 64, 64, 4, 2, False), (300, 50, 64, 4, 3, False), (2100, 12, 32, 3, 3, True)]
BIG = (300, 50, 64, 4, 3, False)
# more samples than the grid has waves (8 per workgroup, one workgroup per CU), and no
# multiple of 8: some waves route two samples through the same tiles, others one
MANY = SHAPES[-1]


def _run(shape, fused, monkeypatch, rows=None):
    from pytorchrec_amd import dense
    monkeypatch.setattr(dense, "MIND_FUSED", fused)
    got, fn = run(case(*shape, device="cuda:0"), rows=rows)
    assert ("_MindFn" in type(fn).__name__) == fused
    return got


def _within_bars(errors, names):
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} "
              f"mean {lmean:.2e}")
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        tol = 3e-2 if name == "U" else 5e-2
        assert fmax <= max(tol, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


@pytest.mark.parametrize("B,L,D,K,R,dyn", SHAPES)
def test_fused_routing_matches_fp64_reference(gpu, monkeypatch, B, L, D, K, R, dyn):
    """U, dX and dS on every sample.  One position and one interest; K = 3 padded to the
    16-row tile; odd L with all 8 interests and every K' (dynamic_k); L = 64 (no padded
    rows); B = 300 (dS summed over many workgroups); and B = 2100 (uneven shares of the
    persistent grid: waves that route two samples, with different K', through the same LDS
    tiles and add both to their dS accumulators, beside waves that route one)."""
    shape = (B, L, D, K, R, dyn)
    ref = ref64(*shape, device="cuda:0")
    errors = {}
    for fused in (True, False):
        for name, t in _run(shape, fused, monkeypatch).items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errors[(fused, name)] = errs(t, ref[name])
    _within_bars(errors, list(ref))


@pytest.mark.parametrize("shape", [BIG, MANY])
def test_two_runs_are_bitwise_equal(gpu, monkeypatch, shape):
    from pytorchrec_amd import _mrec
    if shape is MANY:  # the case is there for the waves that take a second sample
        assert 8 * _mrec.lib().mrec_mind_parts(shape[0]) < shape[0]
    a, b = _run(shape, True, monkeypatch), _run(shape, True, monkeypatch)
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


@pytest.mark.parametrize("D,K,L,fused", [(48, 3, 12, False), (16, 3, 65, False), (16, 9, 12, False),
                                         (32, 3, 12, True)])
def test_dispatch(gpu, D, K, L, fused):
    """The layered path for a width, a length and an interest count the kernels do not
    cover; the fused path otherwise."""
    from pytorchrec_amd import dense
    assert dense.MIND_FUSED
    m = mind(emb_size=D, max_his_len=L, num_interests=K, device=gpu)
    g = torch.Generator().manual_seed(L)
    lens = torch.randint(1, L + 1, (9,), generator=g)
    his = torch.randint(1, 50, (9, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    rows = (0.3 * torch.randn(9, L, D, generator=g)).to(torch.bfloat16).to(gpu).requires_grad_()
    U = dense.mind_route(rows, his.to(gpu), lens.to(gpu), m)
    assert ("_MindFn" in type(U.grad_fn).__name__) == fused
    U.sum().backward()
    assert torch.isfinite(U).all() and torch.isfinite(rows.grad.float()).all()


def test_model_train_step_and_item_gradients(gpu, monkeypatch):
    """One ``mind`` train step with softmax_shared gives a finite loss that moves
    route_weight, and with the soft readout (interest_pow = 4) the item rows' gradient of
    ``forward`` agrees between the fused and the layered routing within the bars (the fp32
    CPU model is the reference)."""
    from pytorchrec_amd import dense
    from pytorchrec_amd.loss import get_loss
    data = batch(gpu)
    m = mind(emb_size=32, device=gpu)
    before = m.route_weight.detach().clone()
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.01), get_loss("softmax_shared")(), [], gpu)
    m.set_shared_negatives("in_batch")
    assert torch.isfinite(m.train_step(data)["loss"].detach()).item()
    assert not torch.equal(before, m.route_weight.detach())
    with torch.no_grad():
        state = mind(emb_size=32, interest_pow=4.0).state_dict()
        state["i_embeddings.weight"] *= 30.0  # lively scores: N(0, 0.3) rows
    grads = {}
    for key, dev in ((True, gpu), (False, gpu), ("ref", "cpu")):
        monkeypatch.setattr(dense, "MIND_FUSED", key is True)
        m = mind(emb_size=32, interest_pow=4.0, device=dev if dev != "cpu" else None)
        m.load_state_dict(state)
        pred, _ = m.eval()({k: t.to(dev) for k, t in data.items()})
        pred.square().mean().backward()
        grads[key] = m.i_embeddings.weight.grad[:, :32]
    errors = {(k, "items"): errs(grads[k], grads["ref"].double()) for k in (True, False)}
    _within_bars(errors, ["items"])


def test_recommend_is_the_brute_force_top_k(gpu):
    m = mind(emb_size=32, dynamic_k=True, device=gpu).eval()
    with torch.no_grad():
        m.i_embeddings.weight.mul_(30.0)
    data = batch(gpu)
    ids, _ = m.recommend(data, 7)
    assert torch.equal(ids.long(), brute_scores(m, data, bf16=True).topk(7, dim=1).indices)
