"""The fused SR-GNN encoder (mrec_srgnn_fwd / _bwd, srgnn.hip) on the GPU: parity with the
node-space fp64 restatement of test_srgnn_cpu.py on every sample with the layered GPU path as
the yardstick, bit equality across runs, rows and batch orders, the dispatch, and the model.

Bars (those of test_gpu_sasrec.py's test_fused_encoder_matches_fp64_reference), per quantity
and relative to its magnitude: max error <= max(tol, 1.5 x the layered path's) with tol 3e-2
forward / 5e-2 gradients, and mean error <= max(3e-3, 1.5 x the layered path's).  Both GPU
paths round H, the edge projections, M and the six product matrices to bf16; the restatement
rounds nothing.
"""
import pytest
import torch

from test_srgnn_cpu import case, errs, ref64, run, srgnn

pytestmark = pytest.mark.gpu

# (B, L, D, steps, id vocabulary): one node and no edge; heavy repeats and the hand-made
# sessions; odd L and BPTT over three steps; L = 64 (no padded row) with repeats in every
# sample; uneven samples per workgroup and partials over many samples
SHAPES = [(37, 1, 16, 1, 1000), (33, 12, 16, 2, 4), (64, 37, 32, 3, 1000), (48, 64, 64, 2, 40),
          (300, 50, 64, 1, 1000)]
BIG = (300, 50, 64, 2, 200)


def _run(shape, fused, monkeypatch, rows=None, order=None):
    from pytorchrec_amd import dense
    monkeypatch.setattr(dense, "SRGNN_FUSED", fused)
    c = case(*shape, device="cuda:0")
    if order is not None:
        c = (c[0],) + tuple(t[order] for t in c[1:])
    got, fn = run(c, rows=rows)
    assert ("_SrgnnFn" in type(fn).__name__) == fused
    return got


@pytest.mark.parametrize("B,L,D,steps,vocab", SHAPES)
def test_fused_encoder_matches_fp64_reference(gpu, monkeypatch, B, L, D, steps, vocab):
    """v, dX and the sixteen dense gradients on every sample."""
    shape = (B, L, D, steps, vocab)
    ref = ref64(*shape, device="cuda:0")
    errors = {}
    for fused in (True, False):
        for name, t in _run(shape, fused, monkeypatch).items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errors[(fused, name)] = errs(t, ref[name])
    for name in ref:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} mean {lmean:.2e}")
    for name in ref:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        assert fmax <= max(3e-2 if name == "v" else 5e-2, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


def test_bits_depend_on_the_sample_alone(gpu, monkeypatch):
    """Two runs are bitwise equal; dX is bitwise zero at invalid and duplicate positions and
    non-zero at every representative; 1e3 in the rows at invalid and duplicate positions
    changes no bit; reversing the batch gives each sample the same v and dX bits."""
    from pytorchrec_amd import cpu_path
    _, rows, his, _, _ = case(*BIG, device="cuda:0")
    a, b = _run(BIG, True, monkeypatch), _run(BIG, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    valid, _, rep, _ = cpu_path.srgnn_graph(his)
    assert (~valid).any() and (valid & ~rep).any()
    assert a["dX"].dtype == torch.bfloat16
    assert (a["dX"][~rep].view(torch.int16) == 0).all()
    assert (a["dX"][rep].float().abs().sum(-1) > 0).all()
    loud = rows.clone()
    loud[~rep] = 1e3
    b = _run(BIG, True, monkeypatch, rows=loud)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    order = torch.arange(BIG[0] - 1, -1, -1, device=rows.device)
    b = _run(BIG, True, monkeypatch, order=order)
    assert torch.equal(a["v"][order], b["v"]) and torch.equal(a["dX"][order], b["dX"])


@pytest.mark.parametrize("D,L,steps", [(24, 12, 1), (16, 65, 1), (16, 12, 5)])
def test_unsupported_shapes_take_the_layered_path(gpu, monkeypatch, D, L, steps):
    """The layered path with the switch on: its grad_fn, and v bit for bit (torch's own
    backward of the gather adds with atomics, so its gradients are not compared by bits)."""
    from pytorchrec_amd import dense
    shape = (9, L, D, steps, 30)
    want = _run(shape, False, monkeypatch)
    monkeypatch.setattr(dense, "SRGNN_FUSED", True)
    got, fn = run(case(*shape, device="cuda:0"))
    assert "_SrgnnFn" not in type(fn).__name__
    assert torch.equal(got["v"], want["v"])
    for name in want:
        assert torch.allclose(got[name].float(), want[name].float(), rtol=1e-3, atol=1e-5), name


def test_model_trains_and_serves_through_the_fused_path(gpu, monkeypatch):
    """``softmax_shared`` train steps run both launches and lower the loss on a fixed batch;
    ``recommend`` returns k items by descending score."""
    from pytorchrec_amd import _mrec
    from pytorchrec_amd.loss import get_loss
    g = torch.Generator().manual_seed(5)
    B, L, items = 32, 12, 50
    lens = torch.randint(1, L + 1, (B,), generator=g)
    his = torch.randint(1, items, (B, L), generator=g)
    his[torch.arange(L)[None, :] >= lens[:, None]] = 0
    data = {"iid": torch.randint(1, items, (B, 5), generator=g), "his": his, "his_len": lens,
            "label": torch.zeros(B, 5, dtype=torch.long)}
    data["label"][:, 0] = 1
    data = {k: t.to(gpu) for k, t in data.items()}
    m = srgnn(items=items, emb_size=32, max_his_len=L, gnn_steps=2, device=gpu)
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.01), get_loss("softmax_shared")(), [], gpu)
    m.set_shared_negatives("in_batch")
    names = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda n, *a: names.append(n) or real(n, *a))
    losses = [m.train_step(data)["loss"].detach().item() for _ in range(6)]
    assert names.count("mrec_srgnn_fwd") == 6 and names.count("mrec_srgnn_bwd") == 6
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    ids, scores = m.recommend(data, 7)
    assert names.count("mrec_srgnn_fwd") == 7
    assert ids.shape == (B, 7) and (scores[:, :-1] >= scores[:, 1:]).all() and (ids > 0).all()
