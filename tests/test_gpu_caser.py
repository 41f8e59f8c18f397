"""The fused Caser encoder (mrec_caser_fwd / _bwd, caser.hip) on the GPU: parity with the
looped fp64 restatement of test_caser_cpu.py on every sample and filter with the layered GPU
path as the yardstick, bit equality across runs, rows and batch orders, the dispatch, and the
model.

The pooled maximum is discontinuous in its argmax, so v is compared with the restatement's own
pooling, the gradients with the restatement pooled at the path's own windows, and the windows
are checked separately: a chosen window may lie under the true maximum by at most the forward
bar, 3e-2 of max |pre|.  Bars (those of test_gpu_srgnn.py), per quantity and relative to its
magnitude: max error <= max(tol, 1.5 x the layered path's) with tol 3e-2 forward / 5e-2
gradients, and mean error <= max(3e-3, 1.5 x the layered path's).  Both GPU paths round X, the
three weights and z to bf16; the restatement rounds nothing.
"""
import pytest
import torch

from test_caser_cpu import caser, case, errs, ref64, run

pytestmark = pytest.mark.gpu

# (B, L, D, heights, n_h, n_v, id vocabulary): one position and one height; heights longer
# than some histories; odd L and n_h 32; L = 64 with no spare row, the tallest filter and the
# element budget's edge; an uneven last group of 12 and partials over many workgroups
SHAPES = [(37, 1, 16, (1,), 16, 1, 1000), (33, 12, 16, (1, 2, 3, 4), 16, 4, 1000),
          (64, 37, 32, (2, 3, 5), 32, 3, 1000), (48, 64, 64, (1, 3, 4, 8), 16, 8, 1000),
          (300, 50, 64, (2, 3, 4), 16, 4, 1000)]
BIG = SHAPES[-1]


def _run(shape, fused, monkeypatch, rows=None, order=None):
    from pytorchrec_amd import dense
    monkeypatch.setattr(dense, "CASER_FUSED", fused)
    c = case(*shape, device="cuda:0")
    if order is not None:
        c = (c[0],) + tuple(t[order] for t in c[1:])
    got, fn = run(c, rows=rows)
    assert ("_CaserFn" in type(fn).__name__) == fused
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_encoder_matches_fp64_reference(gpu, monkeypatch, shape):
    """v, the pooled windows, dX and every dense gradient on every sample and filter."""
    free = ref64(shape, device="cuda:0")
    errors = {}
    for fused in (True, False):
        got = _run(shape, fused, monkeypatch)
        ref = ref64(shape, pick=got.pop("pick"), device="cuda:0")
        gap = ref["gap"].max().item()
        print(f"fused {fused}: the pooled windows lie at most {gap:.2e} under the maximum")
        assert gap <= 3e-2, (fused, gap)
        for name, t in got.items():
            assert torch.isfinite(t.float()).all(), (fused, name)
            errors[(fused, name)] = errs(t, free["v"] if name == "v" else ref[name])
    names = [n for f, n in errors if f]
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} mean {lmean:.2e}")
    for name in names:
        (fmax, fmean), (lmax, lmean) = errors[(True, name)], errors[(False, name)]
        assert fmax <= max(3e-2 if name == "v" else 5e-2, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


def test_bits_depend_on_the_sample_alone(gpu, monkeypatch):
    """Two runs are bitwise equal; dX is bf16 and bitwise zero at invalid positions; 1e3 in the
    rows at invalid positions changes no bit; reversing the batch gives each sample the same v,
    pick and dX bits; the repeated-id sample pools at window 0."""
    _, rows, his, _, _ = case(*BIG, device="cuda:0")
    a, b = _run(BIG, True, monkeypatch), _run(BIG, True, monkeypatch)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    valid = his > 0
    valid[:, 0] = True
    assert (~valid).any() and a["dX"].dtype == torch.bfloat16
    assert (a["dX"][~valid].view(torch.int16) == 0).all()
    assert (a["pick"][3] == 0).all()
    loud = rows.clone()
    loud[~valid] = 1e3
    b = _run(BIG, True, monkeypatch, rows=loud)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    order = torch.arange(BIG[0] - 1, -1, -1, device=rows.device)
    b = _run(BIG, True, monkeypatch, order=order)
    for name in ("v", "dX"):
        assert torch.equal(a[name][order], b[name]), name
    assert torch.equal(a["pick"][order.cpu()], b["pick"])


@pytest.mark.parametrize("D,L,heights,n_h,n_v", [
    (24, 12, (1, 2), 16, 2), (16, 65, (1, 2), 16, 2), (16, 12, (2, 9), 16, 2), (16, 12, (1, 2), 24, 2),
    (16, 12, (1, 2), 16, 9), (64, 12, (1, 2, 3, 4), 32, 2)])
def test_unsupported_shapes_take_the_layered_path(gpu, monkeypatch, D, L, heights, n_h, n_v):
    """The layered path with the switch on: its grad_fn, and v bit for bit."""
    from pytorchrec_amd import dense
    shape = (9, L, D, heights, n_h, n_v, 30)
    want = _run(shape, False, monkeypatch)
    monkeypatch.setattr(dense, "CASER_FUSED", True)
    got, fn = run(case(*shape, device="cuda:0"))
    assert "_CaserFn" not in type(fn).__name__
    assert torch.equal(got["v"], want["v"])


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
    m = caser(items=items, emb_size=32, max_his_len=L, device=gpu)
    m.compile(torch.optim.Adam(m.get_parameters(), lr=0.01), get_loss("softmax_shared")(), [], gpu)
    m.set_shared_negatives("in_batch")
    names = []
    real = _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda n, *a: names.append(n) or real(n, *a))
    losses = [m.train_step(data)["loss"].detach().item() for _ in range(6)]
    assert names.count("mrec_caser_fwd") == 6 and names.count("mrec_caser_bwd") == 6
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    ids, scores = m.recommend(data, 7)
    assert names.count("mrec_caser_fwd") == 7
    assert ids.shape == (B, 7) and (scores[:, :-1] >= scores[:, 1:]).all() and (ids > 0).all()
