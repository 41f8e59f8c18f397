"""The fused DCN-Mix cross stack on the GPU (mrec_cross_mix_fwd / _bwd, csrc/cross_mix.hip).

Shapes.  A workgroup takes 16 samples; d goes in 32-wide k steps and 16-wide output tiles, K r
in 16-wide tiles of r / 16 per expert, the gate is one more tile when K > 1.  Hence B in {1, 5,
33, 70, 150} (less than a tile, a ragged last one, many), d in {8, 13, 40, 429, 512} (below a k
step, odd, the Criteo width, the maximum), K in {1, 2, 3, 4}, r in {16, 32, 64} with K r up to
256, 1 to 4 layers, x0 in bf16 and fp32.

Bars (test_gpu_sasrec.py's): per quantity, against fp64 on unrounded operands, max error <=
max(3e-2 forward / 5e-2 gradients, 1.5 x the layered GPU path's) and mean error <= max(3e-3,
1.5 x the layered path's), relative to the quantity's magnitude."""
import ctypes

import pytest
import torch

from test_dcnmix_cpu import RefDCNMix, copy_into_ref, dcnmix, mix_case, named_pairs, run, sample_loop
from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
KERNELS = ["mrec_cross_mix_fwd", "mrec_cross_mix_bwd"]
CASES = [(1, 8, 1, 16, 1, BF), (33, 13, 2, 16, 2, F32), (5, 40, 4, 16, 1, BF), (70, 429, 4, 64, 3, BF),
         (150, 512, 3, 32, 4, F32)]


def to_gpu(layers, gpu):
    return [tuple(None if w is None else w.float().to(gpu) for w in l) for l in layers]


def errs(got, want):
    """(max, mean) error relative to the quantity's magnitude."""
    got, want = got.double().cpu(), torch.as_tensor(want).double()
    diff = (got - want).abs()
    return float(diff.max() / want.abs().max()), float(diff.mean() / want.abs().max())


def quantities(res):
    y, dx, gs = res
    return {"x_L": y, "dx0": dx, **{f"layer{l}.d{k}": g for l, gd in enumerate(gs) for k, g in gd.items()}}


def within_the_bars(fused, layered, ref):
    for name, want in ref.items():
        (fmax, fmean), (lmax, lmean) = errs(fused[name], want), errs(layered[name], want)
        print(f"{name}: fused max {fmax:.2e} mean {fmean:.2e} | layered max {lmax:.2e} mean {lmean:.2e}")
        assert fmax <= max(3e-2 if name in ("x_L", "loss") else 5e-2, 1.5 * lmax), (name, fmax, lmax)
        assert fmean <= max(3e-3, 1.5 * lmean), (name, fmean, lmean)


def spy(monkeypatch):
    from pytorchrec_amd import _mrec
    calls, real = [], _mrec.call
    monkeypatch.setattr(_mrec, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("B,d,K,r,layers,dtype", CASES)
def test_gaussian_operands_against_fp64_by_the_layered_yardstick(gpu, monkeypatch, B, d, K, r, layers, dtype):
    from pytorchrec_amd import dense
    x0, L, dy = mix_case(B, d, K, r, layers, 7 + B)
    ref = quantities(sample_loop(x0, L, dy))
    args = (x0.to(gpu).to(dtype), to_gpu(L, gpu), dy.to(gpu).to(BF))
    calls = spy(monkeypatch)
    fused = quantities(run(dense.cross_mix, *args))
    assert [c for c in calls if c in KERNELS] == KERNELS
    monkeypatch.setattr(dense, "CROSS_MIX_FUSED", False)
    within_the_bars(fused, quantities(run(dense.cross_mix, *args)), ref)


@pytest.mark.parametrize("B,d,K,r,layers,dtype", CASES[1:4])
def test_zero_U_and_b_make_the_stack_the_identity(gpu, B, d, K, r, layers, dtype):
    """z = 0: x_L = bf16(x0) and dx0 = dy bit for bit, while dU still sees dz and s."""
    from pytorchrec_amd import dense
    x0, L, dy = mix_case(B, d, K, r, layers, 5)
    L = [(V, C, torch.zeros_like(U), torch.zeros_like(b), g) for V, C, U, b, g in L]
    x, dyb = x0.to(gpu).to(dtype), dy.to(gpu).to(BF)
    y, dx, gs = run(dense.cross_mix, x, to_gpu(L, gpu), dyb)
    assert torch.equal(y, x.to(BF)) and torch.equal(dx.to(BF), dyb) and dx.dtype == dtype
    assert all(bool(g["U"].any()) and not bool(g["V"].any()) for g in gs)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_strides_nan_pads_and_sentinels(gpu, dtype):
    """B = 33, d = 13, K = 2, r = 16, two layers through the library calls: x0 and dy are views
    with NaN in their pad columns and spare rows; y, saved, dx0 and the workspace sit inside
    sentinel-filled buffers.  Only the contract's elements are written, the results equal the
    tight call's, and the pad columns of the stored operands are zero."""
    from pytorchrec_amd import _mrec, dense
    B, d, K, r, nl = 33, 13, 2, 16, 2
    x0, L, dy = mix_case(B, d, K, r, nl, 9)
    L = to_gpu(L, gpu)
    want_y, want_dx, _ = run(dense.cross_mix, x0.to(gpu).to(dtype), L, dy.to(gpu).to(dtype))
    xb = torch.full((B + 2, 24), float("nan"), dtype=dtype, device=gpu)
    gb = torch.full((B + 2, 32), float("nan"), dtype=dtype, device=gpu)
    xb[:B, :d], gb[:B, :d] = x0.to(gpu), dy.to(gpu)
    yb = torch.full((B + 2, 24), 7.0, dtype=BF, device=gpu)
    sb = torch.full((nl, B + 3, 24), 7.0, dtype=BF, device=gpu)
    db = torch.full((B + 2, 24), 7.0, dtype=F32, device=gpu)
    nws = int(_mrec.lib().mrec_cross_mix_bwd_workspace_size(B, d, K, r, nl))
    ws = torch.full((nws + 256,), 0x5a, dtype=torch.uint8, device=gpu)
    a, keep = _mrec.CrossMixArgs(), []
    for l, (V, C, U, b, gate) in enumerate(L):
        keep.append(dense.cross_mix_images(V, C, U, gate)[0])
        a.w_img[l], a.bias[l] = keep[-1].data_ptr(), b.data_ptr()
    a.x0, a.x0_dtype, a.ld_x0 = xb.data_ptr(), _mrec.dtype_code(dtype), xb.stride(0)
    a.batch, a.d, a.K, a.r, a.layers, a.train = B, d, K, r, nl, 1
    a.y, a.ld_y = yb.data_ptr(), yb.stride(0)
    a.saved, a.ld_saved, a.saved_layer_stride = sb.data_ptr(), sb.stride(1), sb.stride(0)
    a.dy, a.dy_dtype, a.ld_dy = gb.data_ptr(), _mrec.dtype_code(dtype), gb.stride(0)
    a.dx0, a.ld_dx0 = db.data_ptr(), db.stride(0)
    a.workspace, a.workspace_bytes = ws.data_ptr() + 128, nws
    _mrec.call("mrec_cross_mix_fwd", ctypes.byref(a), _mrec.stream_handle())
    _mrec.call("mrec_cross_mix_bwd", ctypes.byref(a), _mrec.stream_handle())
    assert torch.equal(yb[:B, :d], want_y) and torch.equal(db[:B, :d].to(dtype), want_dx)
    for name, buf, cols in (("y", yb, d), ("dx0", db, d)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:B, :cols] = False
        assert bool((buf[mask] == 7.0).all()), f"{name}: wrote outside its elements"
    assert bool((sb[:, B:] == 7.0).all()) and bool((sb[:, :, 16:] == 7.0).all()), "saved: outside its rows"
    assert not bool(sb[:, :B, d:16].any()) and torch.equal(sb[0, :B, :d], xb[:B, :d].to(BF))
    assert bool((ws[:128] == 0x5a).all()) and bool((ws[128 + nws:] == 0x5a).all()), "workspace guards"
    ops, o, kr = {}, 0, K * r
    flat = ws[128:128 + nws].view(BF)
    for name, w in (("dz", 16), ("s", kr), ("du", kr), ("a", kr), ("dtl", kr + 16)):
        ops[name] = flat[o:o + nl * B * w].view(nl, B, w)
        o += nl * B * w
    assert all(bool(torch.isfinite(t.float()).all()) and bool(t.any()) for t in ops.values())
    assert not bool(ops["dz"][:, :, d:].any()) and not bool(ops["dtl"][:, :, kr + K:].any())


@pytest.mark.parametrize("B,d,K,r,layers,dtype", CASES[1:4])
def test_bits_do_not_depend_on_run_or_position(gpu, B, d, K, r, layers, dtype):
    from pytorchrec_amd import dense
    x0, L, dy = mix_case(B, d, K, r, layers, 12)
    L = to_gpu(L, gpu)
    go = lambda x, g: run(dense.cross_mix, x.to(gpu).to(dtype), L, g.to(gpu).to(BF))  # noqa: E731
    a, b = quantities(go(x0, dy)), quantities(go(x0, dy))
    for name in a:
        assert torch.equal(a[name], b[name]), name + " differs from run to run"
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
    keep = max(1, B // 2)
    c = quantities(go(torch.cat([x0[perm], x0[:keep]]), torch.cat([dy[perm], dy[:keep]])))
    e = quantities(go(x0[:keep], dy[:keep]))
    for name in ("x_L", "dx0"):
        assert torch.equal(c[name][:B], a[name][perm.to(gpu)]), name + " depends on the position"
        assert torch.equal(c[name][B:], a[name][:keep]) and torch.equal(e[name], a[name][:keep]), name


@pytest.mark.parametrize("how,d,K,r", [("switch", 40, 2, 16), ("r24", 40, 2, 24), ("d520", 520, 2, 16),
                                       ("K5", 40, 5, 16)])
def test_the_switch_and_unsupported_shapes_take_the_torch_ops(gpu, monkeypatch, how, d, K, r):
    from pytorchrec_amd import cpu_path, dense
    if how == "switch":
        monkeypatch.setattr(dense, "CROSS_MIX_FUSED", False)
    else:
        assert dense.CROSS_MIX_FUSED and not dense.cross_mix_supported(d, K, r, 2)
    x0, L, dy = mix_case(9, d, K, r, 2, 2)
    args = (x0.to(gpu).float(), to_gpu(L, gpu), dy.to(gpu).to(BF))
    calls = spy(monkeypatch)
    got = quantities(run(dense.cross_mix, *args))
    assert not set(KERNELS) & set(calls) and got["x_L"].dtype == BF
    want = quantities(run(cpu_path.cross_mix, *args, round_bf16=True))
    for name in want:
        assert torch.equal(got[name], want[name]), name


def test_empty_batch(gpu, monkeypatch):
    from pytorchrec_amd import dense
    _, L, _ = mix_case(1, 40, 2, 16, 2, 3)
    calls = spy(monkeypatch)
    empty = torch.zeros(0, 40, dtype=BF, device=gpu)
    y, dx, gs = run(dense.cross_mix, empty, to_gpu(L, gpu), empty)
    assert tuple(y.shape) == (0, 40) == tuple(dx.shape) and y.dtype == BF
    assert all(not bool(g.any()) for gd in gs for g in gd.values()) and len(gs[0]) == 5
    assert "mrec_cross_mix_bwd" not in calls


@pytest.mark.parametrize("emb_dtype", [F32, BF], ids=["fp32", "bf16"])
def test_dcnmix_train_step_matches_the_fp64_model(gpu, monkeypatch, emb_dtype):
    """One DCNMix train step (B = 256, 6 fields of 50 rows, 3 dense, D = 8: d = 51; two layers
    of 2 experts of rank 16; layers [64, 32]; BCE, plain SGD) against RefDCNMix in fp64 from
    identical weights: the loss and every parameter's update by the bars above, the layered
    GPU path (CROSS_MIX_FUSED = False) as the yardstick, the fused kernels taken; the images the
    fused SGD rewrote equal a fresh build from the updated parameters."""
    from pytorchrec_amd import dense
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    lr = 1e4 if emb_dtype == BF else 1.0
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(dense, "CROSS_MIX_FUSED", fused)
        m = dcnmix(rows=50, F=6, n_dense=3, D=8, layers=(64, 32), device=gpu, emb_dtype=emb_dtype, random_seed=2020)
        m.embeddings.stochastic_rounding = False
        with torch.no_grad():
            for name, p in m.named_parameters():
                p.mul_(1.0 if name.split(".")[-1] in ("V", "C", "U") else 30.0)
        r = RefDCNMix([50] * 6, 3, 8, 2, 2, 16, (64, 32))
        copy_into_ref(m, r)
        before = [b.detach().clone() for _, _, b in named_pairs(m, r)]
        data, ids, dn, label = ctr_batch(m, 256)
        m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], gpu)
        calls = spy(monkeypatch)
        loss = m.train_step({k: v.to(gpu) for k, v in data.items()})["loss"].detach()
        assert [c for c in calls if c in KERNELS] == (KERNELS if fused else [])
        for l in m.cross if fused else ():  # the fused SGD kept each layer's image current
            V, C, U, _, gate = l.weights()
            kept = V._mrec_ximg[1]
            assert dense.cross_mix_images(V, C, U, gate)[0] is kept
            del V._mrec_ximg
            assert torch.equal(dense.cross_mix_images(V, C, U, gate)[0], kept)
        out[fused] = {"loss": loss.reshape(1)}
        out[fused].update({n: g.detach().double().cpu() - old for (n, g, _), old in zip(named_pairs(m, r), before)})
    rloss = ref_train_step(r, lr, ids, dn.double(), label)
    ref = {"loss": torch.tensor([rloss])}
    ref.update({n: w.detach() - old for (n, _, w), old in zip(named_pairs(m, r), before)})
    assert all(float(v.abs().max()) > 0 for v in ref.values())
    within_the_bars(out[True], out[False], ref)
