"""CPU checks of the Compressed Interaction Network and the xDeepFM model (no GPU).

* ``cpu_path.cin`` -- the contract of include/mrec.h "CIN" in torch ops, chunked over the
  batch -- against an independent ``torch.einsum`` restatement in fp64 (forward and autograd's
  gradients), ``gradcheck``, and itself under other chunk sizes;
* the registry, the state-dict keys, the argument checks and the refusals of ``XDeepFM``;
* one CPU ``train_step`` of a tiny XDeepFM against the same model written here in torch fp64
  from identical weights (``RefXDeepFM``; the GPU test reuses it);
* ``mrec_cin_*``'s argument validation, which runs on the host before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step
from test_sasrec_cpu import close_to_magnitude


# ---------------------------------------------------------------------------
# restatements (shared with tests/test_gpu_xdeepfm.py)
# ---------------------------------------------------------------------------

def cin_einsum(x0, weights, m):
    """The contract as one einsum per layer, in the operands' dtype -> (p, [X^1 .. X^L])."""
    B = x0.shape[0]
    X0 = x0.reshape(B, m, -1)
    xs, xp = [], X0
    for W in weights:
        xp = torch.einsum("hij,bid,bjd->bhd", W, xp, X0)
        xs.append(xp)
    return torch.cat([x.sum(2) for x in xs], 1), xs


class RefXDeepFM(nn.Module):
    """xDeepFM in plain torch ops: nn.Embedding per field (and an [n, 1] first-order one), the
    CIN as einsums, Linear -> ReLU for the MLP, Linear(., 1) heads.  ``bf16_points=True`` is
    the same model with every tensor the GPU path stores or multiplies in bf16 rounded there,
    value and gradient (the x0 rows, the CIN's operands, Z, X^k and p as the head's input, the
    MLP's activations; the weights as MFMA operands), fp32 accumulation: what bf16 storage
    alone costs."""

    def __init__(self, category_nums, n_dense, emb_size, cin, layers, dtype=torch.float64,
                 bf16_points=False):
        super().__init__()
        m = len(category_nums)
        self.emb = nn.ModuleList([nn.Embedding(n, emb_size) for n in category_nums])
        self.first = nn.ModuleList([nn.Embedding(n, 1) for n in category_nums])
        self.dense_weight = nn.Parameter(torch.zeros(n_dense)) if n_dense else None
        self.global_bias = nn.Parameter(torch.zeros(1))
        self.cin = nn.ParameterList([nn.Parameter(torch.zeros(h, hp, m))
                                     for hp, h in zip([m, *cin[:-1]], cin)])
        self.cin_out = nn.Linear(sum(cin), 1, bias=False)
        self.mlp = nn.ModuleList([nn.Linear(a, b) for a, b in
                                  zip([m * emb_size + n_dense, *layers[:-1]], layers)])
        self.out = nn.Linear(layers[-1], 1)
        self.bf16_points = bf16_points
        self.to(dtype)

    def linears(self):
        return list(self.mlp) + [self.out]

    def forward(self, ids, dense):
        from oracle.models import _rb, _rbv
        rb = _rb if self.bf16_points else (lambda t: t)
        rbv = _rbv if self.bf16_points else (lambda t: t)
        B = ids.shape[0]
        v = rb(torch.stack([e(ids[:, f]) for f, e in enumerate(self.emb)], 1))  # [B, m, D]
        logit = self.global_bias + sum(e(ids[:, f]).squeeze(-1) for f, e in enumerate(self.first))
        if self.dense_weight is not None:
            logit = logit + dense @ self.dense_weight
        xp, ps = v, []
        for W in self.cin:
            Z = rb(xp.unsqueeze(2) * v.unsqueeze(1)).reshape(B, -1, v.shape[2])
            xk = torch.matmul(rbv(W).reshape(W.shape[0], -1), Z)
            ps.append(xk.sum(2))
            xp = rb(xk)
        logit = logit + (rb(torch.cat(ps, 1)) @ self.cin_out.weight.T).squeeze(-1)
        x = v.reshape(B, -1)
        if self.dense_weight is not None:
            x = torch.cat([x, rb(dense)], 1)
        for lin in self.mlp:
            x = rb(torch.relu(x @ rbv(lin.weight).T + lin.bias))
        return logit + (x @ self.out.weight.T + self.out.bias).squeeze(-1)


def xdeepfm(rows=30, F=4, n_dense=2, D=8, cin=(8, 8), layers=(16,), device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import XDeepFM
    sparse = [CategoricalColumnWithIdentity(rows, f"c{f}") for f in range(F)]
    dense = [NumericColumn(f"d{j}") for j in range(n_dense)]
    label = CategoricalColumnWithIdentity(2, "label")
    return XDeepFM(sparse, dense, label, emb_size=D, layers=layers, cin_layers=cin, device=device,
                   **kw)


def xdeepfm_linears(m):
    """The product model's MLP Linears and output layer in RefXDeepFM.linears() order."""
    return [x for x in m.mlp.modules() if isinstance(x, nn.Linear)] + [m.prediction]


def copy_into_ref(m, r):
    with torch.no_grad():
        for f in range(len(r.emb)):
            r.emb[f].weight.copy_(m.embeddings.table(f).to(r.emb[f].weight.dtype).cpu())
            r.first[f].weight.copy_(m.embeddings.first_order(f).to(r.emb[f].weight.dtype).cpu().unsqueeze(1))
        if r.dense_weight is not None:
            r.dense_weight.copy_(m.dense_weight.cpu())
        r.global_bias.copy_(m.global_bias.cpu())
        for a, b in zip(m.cin_weights, r.cin):
            b.copy_(a.cpu())
        r.cin_out.weight.copy_(m.cin_out.weight.cpu())
        for a, b in zip(xdeepfm_linears(m), r.linears()):
            b.weight.copy_(a.weight.cpu())
            b.bias.copy_(a.bias.cpu())


def named_pairs(m, r):
    """(name, the product model's tensor, the reference's) for every parameter."""
    out = []
    for f in range(len(r.emb)):
        out.append((f"table{f}", m.embeddings.table(f), r.emb[f].weight))
        out.append((f"w{f}", m.embeddings.first_order(f), r.first[f].weight[:, 0]))
    if r.dense_weight is not None:
        out.append(("dense_weight", m.dense_weight, r.dense_weight))
    out.append(("global_bias", m.global_bias, r.global_bias))
    for k, (a, b) in enumerate(zip(m.cin_weights, r.cin)):
        out.append((f"cin{k}", a, b))
    out.append(("cin_out", m.cin_out.weight, r.cin_out.weight))
    for i, (a, b) in enumerate(zip(xdeepfm_linears(m), r.linears())):
        out.append((f"W{i}", a.weight, b.weight))
        out.append((f"b{i}", a.bias, b.bias))
    return out


# ---------------------------------------------------------------------------
# cpu_path.cin
# ---------------------------------------------------------------------------

def cin_case(B, m, D, widths, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, m * D, generator=g, dtype=dtype)
    ws = [torch.randn(h, hp, m, generator=g, dtype=dtype) for hp, h in zip([m, *widths[:-1]], widths)]
    dp = torch.randn(B, sum(widths), generator=g, dtype=dtype)
    return x0, ws, dp


@pytest.mark.parametrize("m", [2, 5])
def test_cin_matches_the_einsum_restatement_in_fp64(m):
    from pytorchrec_amd import cpu_path
    x0, ws, dp = cin_case(3, m, 4, [8, 16], 10 + m)
    a = [x0.clone().requires_grad_(), *[w.clone().requires_grad_() for w in ws]]
    b = [x0.clone().requires_grad_(), *[w.clone().requires_grad_() for w in ws]]
    got = cpu_path.cin(a[0], a[1:])
    want, _ = cin_einsum(b[0], b[1:], m)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 24)
    close_to_magnitude(got.detach().numpy(), want.detach().numpy(), 1e-13, "p")
    got.backward(dp)
    want.backward(dp)
    for name, u, v in zip(("dx0", "dW1", "dW2"), a, b):
        close_to_magnitude(u.grad.numpy(), v.grad.numpy(), 1e-13, name)


@pytest.mark.parametrize("m", [2, 5])
def test_cin_gradcheck(m):
    from pytorchrec_amd import cpu_path
    x0, ws, _ = cin_case(3, m, 4, [8, 16], 20 + m)
    ins = (x0.requires_grad_(), *[w.requires_grad_() for w in ws])
    assert torch.autograd.gradcheck(lambda x, w1, w2: cpu_path.cin(x, [w1, w2], chunk=2), ins)


def test_cin_reads_a_strided_slice_and_checks_its_arguments():
    from pytorchrec_amd import cpu_path, dense
    x0, ws, _ = cin_case(5, 3, 4, [8], 3, torch.float32)
    wide = torch.full((5, 16), float("nan"))
    wide[:, :12] = x0
    assert torch.equal(cpu_path.cin(wide[:, :12], ws), cpu_path.cin(x0, ws))
    assert torch.equal(dense.cin(x0, 3, ws), cpu_path.cin(x0, ws))  # the CPU takes the torch ops
    with pytest.raises(ValueError):
        cpu_path.cin(x0, [])
    with pytest.raises(ValueError):
        cpu_path.cin(x0[:, :11], ws)
    with pytest.raises(ValueError):
        cpu_path.cin(x0, [ws[0], torch.zeros(8, 7, 3)])
    with pytest.raises(ValueError):
        dense.cin(x0, 4, ws)


def test_cin_does_not_depend_on_the_batch_chunking():
    """Forward and gradients per chunk size: a sample's p and dx0 are bit-equal (its own
    arithmetic only); dW sums the chunks in another order, so it agrees to fp32 rounding."""
    from pytorchrec_amd import cpu_path
    x0, ws, dp = cin_case(11, 5, 4, [8, 16], 4, torch.float32)
    outs = []
    for chunk in (1, 4, 11, 256):
        a = [x0.clone().requires_grad_(), *[w.clone().requires_grad_() for w in ws]]
        p = cpu_path.cin(a[0], a[1:], chunk=chunk)
        p.backward(dp)
        outs.append((p.detach(), *[t.grad for t in a]))
    for o in outs[1:]:
        close_to_magnitude(o[0].numpy(), outs[0][0].numpy(), 1e-6, "p")
        close_to_magnitude(o[1].numpy(), outs[0][1].numpy(), 1e-6, "dx0")
        for u, v in zip(o[2:], outs[0][2:]):
            close_to_magnitude(u.numpy(), v.numpy(), 1e-5, "dW")


def test_cin_bf16_rounding_points():
    """round_bf16 rounds x0, W, X^k as an operand and Z: with operands that bf16 holds and
    integer-valued products the rounded path equals the exact one."""
    from pytorchrec_amd import cpu_path
    g = torch.Generator().manual_seed(6)
    x0 = torch.randint(-1, 2, (4, 3 * 4), generator=g).float()
    ws = [torch.randint(-1, 2, (8, 3, 3), generator=g).float()]
    assert torch.equal(cpu_path.cin(x0, ws, round_bf16=True, x_dtype=torch.bfloat16), cpu_path.cin(x0, ws))
    x1 = x0 * (1 + 2.0 ** -10)  # not a bf16 value: the rounded path reads x0 instead
    assert torch.equal(cpu_path.cin(x1, ws, round_bf16=True), cpu_path.cin(x0, ws))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def test_registry_exports_and_arguments():
    import pytorchrec_amd.model as models
    from pytorchrec_amd.model import XDeepFM, get_model_type, model_name_list
    assert get_model_type("xdeepfm") is XDeepFM and "xdeepfm" in model_name_list
    assert models.XDeepFM is XDeepFM
    args = {a.name: a for a in XDeepFM.get_argument_descriptions()}
    assert list(args) == ["emb_size", "layers", "cin_layers", "dropout"]
    assert args["cin_layers"].default_value == "200,200,200"
    XDeepFM.check_argument_values({"emb_size": 16, "layers": "400,400", "cin_layers": "200,200,200",
                                   "dropout": 0.0})
    with pytest.raises(AssertionError):
        XDeepFM.check_argument_values({"emb_size": 16, "layers": "400", "cin_layers": "8", "dropout": 1.0})


def test_rejections():
    from pytorchrec_amd import sharding
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import XDeepFM
    with pytest.raises(ValueError, match="cin_layers"):
        xdeepfm(cin="")
    with pytest.raises(ValueError, match="cin_layers"):
        xdeepfm(cin=(8, 0))
    with pytest.raises(ValueError, match="sparse"):
        XDeepFM([], [NumericColumn("d0")], CategoricalColumnWithIdentity(2, "label"))
    with sharding.sharded_tables(None):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            xdeepfm()


def test_state_dict_keys_and_round_trip(tmp_path):
    m = xdeepfm(random_seed=3)
    keys = list(m.state_dict().keys())
    assert keys == ["dense_weight", "global_bias", "embeddings.weight", "cin_weights.0", "cin_weights.1",
                    "cin_out.weight", "mlp.mlp.dense_0.linear.weight", "mlp.mlp.dense_0.linear.bias",
                    "prediction.weight", "prediction.bias"]
    assert [tuple(w.shape) for w in m.cin_weights] == [(8, 4, 4), (8, 8, 4)]
    assert tuple(m.cin_out.weight.shape) == (1, 16) and m.cin_out.bias is None
    assert m.embeddings.has_w and m.x0_cols == 40
    # normal(0, 0.01) through the reset
    assert 0.005 < float(m.cin_weights[1].detach().std()) < 0.02
    data, *_ = ctr_batch(m, 6)
    m.eval()
    with torch.no_grad():
        logit, target = m(data)
    assert tuple(logit.shape) == (6,) and target.dtype == torch.float32
    path = str(tmp_path / "x.pt")
    torch.save(m.state_dict(), path)
    m2 = xdeepfm(random_seed=4)
    m2.eval()
    with torch.no_grad():
        assert not torch.equal(m2(data)[0], logit)
        m2.load_state_dict(torch.load(path))
        assert torch.equal(m2(data)[0], logit)
    m3 = xdeepfm(n_dense=0, cin="8", layers="16,8")  # the CLI string forms, no dense column
    assert m3.dense_weight is None and len(m3.cin_weights) == 1
    d3, *_ = ctr_batch(m3, 5)
    assert tuple(m3(d3)[0].shape) == (5,)


def test_forward_and_train_step_match_the_fp64_model():
    """B = 64, 4 fields of 30 rows, 2 dense, D = 8, cin [8, 8], layers [16]: the logits, the
    loss and every parameter update of one SGD step against RefXDeepFM in fp64 from identical
    weights, within 1e-5 of each tensor's magnitude (the fp32 CPU path).  An update is read
    back as after - before from fp32 parameters, which adds half an ulp of the parameter that
    no arithmetic of the step made: the learning rate is large enough that every tensor's
    update is at least 5 % of its parameters' size, so that this stays below the bound."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    B, lr = 64, 100.0
    m = xdeepfm(random_seed=11)
    with torch.no_grad():  # weights large enough that every layer matters
        for p in m.parameters():
            p.mul_(30.0)
    r = RefXDeepFM([30] * 4, 2, 8, (8, 8), (16,))
    copy_into_ref(m, r)
    data, ids, dense, label = ctr_batch(m, B)
    m.eval()
    with torch.no_grad():
        logit, target = m(data)
        close_to_magnitude(logit.numpy(), r(ids, dense.double()).detach().numpy(), 1e-5, "logit")
    assert torch.equal(target, label)
    pairs = named_pairs(m, r)
    before = [b.detach().clone() for _, _, b in pairs]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], torch.device("cpu"))
    loss = float(m.train_step(data)["loss"].detach())
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    print(f"loss {loss:.8f} against {rloss:.8f}")
    assert abs(loss - rloss) <= 1e-5 * abs(rloss)
    for (name, got, new), old in zip(named_pairs(m, r), before):
        want = (new.detach() - old).numpy()
        if name != "global_bias":  # (starts at zero)
            assert np.abs(want).max() > 0.05 * float(old.abs().max()), name
        close_to_magnitude((got.detach().double() - old).numpy(), want, 1e-5, f"{name} update")


# ---------------------------------------------------------------------------
# the library's argument checks (host only: nothing is launched)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorchrec_amd import _mrec
    return _mrec.lib()


def good_args(m=5, D=8, Hp=8, H=16, B=4):
    """A valid description over fake (aligned) addresses, fp32 throughout."""
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    a = _mrec.CinArgs()
    a.x0, a.x0_dtype, a.ld_x0 = 1 << 20, _mrec.F32, m * D
    a.xp, a.xp_dtype, a.ld_xp = 2 << 20, _mrec.F32, Hp * D
    a.w_fwd, a.ld_w_fwd = 3 << 20, Hp * lib.mrec_cin_field_pitch(m)
    a.w_bwd, a.ld_w_bwd = 4 << 20, lib.mrec_cin_bwd_cols(H)
    a.batch, a.n_fields, a.D, a.H_prev, a.H, a.x_dtype = B, m, D, Hp, H, _mrec.F32
    a.xk, a.ld_xk = 5 << 20, H * D
    a.p, a.ld_p = 6 << 20, H
    a.dxk, a.ld_dxk = 7 << 20, H * D
    a.dp, a.ld_dp = 8 << 20, H
    a.dxp, a.dxp_dtype, a.ld_dxp = 9 << 20, _mrec.F32, Hp * D
    a.dx0, a.ld_dx0 = 10 << 20, m * D
    a.dw = 11 << 20
    return a


def test_supported_answers_for_the_compiled_shapes(lib):
    from pytorchrec_amd import _mrec, dense
    f32, bf = _mrec.F32, _mrec.BF16
    for m in (2, 16, 17, 26, 32):
        for D in (8, 16, 32, 64):
            for H in (8, 24, 200, 256):
                assert lib.mrec_cin_supported(m, D, m, H, f32, bf) == 1
                assert lib.mrec_cin_supported(m, D, 200, H, bf, f32) == 1
    for m, D, Hp, H in ((1, 16, 1, 8), (33, 16, 33, 8), (26, 12, 26, 8), (26, 128, 26, 8), (26, 16, 26, 12),
                        (26, 16, 26, 264), (26, 16, 12, 8), (26, 16, 264, 8), (26, 16, 26, 0)):
        assert lib.mrec_cin_supported(m, D, Hp, H, f32, f32) == 0, (m, D, Hp, H)
    assert lib.mrec_cin_supported(26, 16, 26, 8, _mrec.I32, f32) == 0
    assert lib.mrec_cin_supported(26, 16, 26, 8, f32, 9) == 0
    assert [lib.mrec_cin_field_pitch(m) for m in (2, 16, 17, 32)] == [16, 16, 32, 32]
    assert [lib.mrec_cin_fwd_rows(h) for h in (8, 32, 200, 256)] == [32, 32, 224, 256]
    assert [lib.mrec_cin_bwd_cols(h) for h in (8, 24, 200, 256)] == [16, 32, 208, 256]
    assert dense.cin_supported(26, 16, [200, 200, 200], torch.bfloat16)
    assert dense.cin_supported(5, 8, [8, 16, 8, 16], torch.float32, torch.bfloat16)
    assert not dense.cin_supported(26, 16, [8] * 5)
    assert not dense.cin_supported(26, 16, [])
    assert not dense.cin_supported(33, 16, [8])
    assert not dense.cin_supported(26, 16, [8, 12])
    assert not dense.cin_supported(26, 12, [8])
    assert not dense.cin_supported(26, 16, [8], torch.float64)


def test_invalid_arguments_return_einval(lib):
    from pytorchrec_amd import _mrec
    both = ("mrec_cin_fwd", "mrec_cin_bwd")

    def refused(a, needle, fns=both):
        for fn in fns:
            st = getattr(lib, fn)(ctypes.byref(a) if a is not None else None, None)
            assert st == _mrec.EINVAL, fn
            msg = lib.mrec_last_error()
            assert msg and needle in msg, (fn, msg)

    refused(None, b"NULL")
    for field, value in (("D", 24), ("n_fields", 33), ("n_fields", 1), ("H", 12), ("H", 264), ("H_prev", 12)):
        a = good_args(); setattr(a, field, value)
        refused(a, b"unsupported shape")
    a = good_args(); a.ld_x0 = 5 * 8 + 2  # 168 bytes: not a multiple of 16
    refused(a, b"16-byte")
    a = good_args(); a.xp = (2 << 20) + 4
    refused(a, b"16-byte")
    a = good_args(); a.x0 = None
    refused(a, b"x0")
    a = good_args(); a.ld_xk = a.ld_xk - 8
    refused(a, b"xk", fns=both[:1])
    a = good_args(); a.p = None
    refused(a, b"p needs", fns=both[:1])
    a = good_args(); a.ld_w_fwd = a.ld_w_fwd - 8
    refused(a, b"w_fwd", fns=both[:1])
    a = good_args(); a.w_bwd = None
    refused(a, b"w_bwd", fns=both[1:])
    a = good_args(); a.dxk = None; a.dp = None
    refused(a, b"dp", fns=both[1:])
    a = good_args(); a.dxp = (9 << 20) + 8
    refused(a, b"dxp", fns=both[1:])
    a = good_args(); a.dx0 = None
    refused(a, b"dx0", fns=both[1:])
    a = good_args(); a.dw = None
    refused(a, b"dw", fns=both[1:])
    a = good_args(); a.x0_dtype = _mrec.I32
    refused(a, b"dtype")
    a = good_args(); a.x_dtype = 11
    refused(a, b"dtype")
    a = good_args(); a.batch = -1
    refused(a, b"batch")
    a = good_args(); a.batch = 1 << 31
    refused(a, b"batch")
    # batch = 0 launches nothing: no pointer is looked at
    a = good_args(); a.batch = 0; a.x0 = None; a.xk = None; a.dw = None
    assert lib.mrec_cin_fwd(ctypes.byref(a), None) == _mrec.OK
    assert lib.mrec_cin_bwd(ctypes.byref(a), None) == _mrec.OK
