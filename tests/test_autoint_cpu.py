"""CPU checks of the AutoInt interacting layers and the AutoInt model (no GPU).

* ``cpu_path.autoint`` -- the contract of include/mrec.h "AutoInt" in torch ops, chunked over
  the batch -- against a literal per-head, per-query loop in fp64, ``gradcheck``, the written
  backward formulas of the contract (the kernel works from them), and itself under other
  chunk sizes; its ``round_bf16`` rounding points;
* the registry, the state-dict keys, the argument checks and the refusals of ``AutoInt``;
* one CPU ``train_step`` of a tiny AutoInt against the same model written here in torch fp64
  from identical weights (``RefAutoInt``; the GPU test reuses it);
* ``mrec_autoint_*``'s argument validation, which runs on the host before any launch.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step
from test_sasrec_cpu import close_to_magnitude


# ---------------------------------------------------------------------------
# restatements (shared with tests/test_gpu_autoint.py)
# ---------------------------------------------------------------------------

def layer_loop(X, Wq, Wk, Wv, Wres, heads, scale):
    """One layer of the contract, literally: per sample, head and query.  X [B, m, d_in]."""
    B, m, _ = X.shape
    A = Wq.shape[0]
    hd = A // heads
    Y = torch.zeros(B, m, A, dtype=X.dtype)
    for b in range(B):
        Q, K, V = X[b] @ Wq.T, X[b] @ Wk.T, X[b] @ Wv.T
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            for i in range(m):
                s = torch.stack([scale * (Q[i, c] * K[j, c]).sum() for j in range(m)])
                e = torch.exp(s - s.max())
                p = e / e.sum()
                Y[b, i, c] = sum(p[j] * V[j, c] for j in range(m))
        if Wres is not None:
            Y[b] = Y[b] + X[b] @ Wres.T
    return torch.relu(Y)


def layer_backward(X, Wq, Wk, Wv, Wres, heads, scale, dY):
    """The written backward of the contract for one layer -> (dX, [dWq, dWk, dWv, dWres])."""
    B, m, _ = X.shape
    A = Wq.shape[0]
    hd = A // heads
    Q, K, V = X @ Wq.T, X @ Wk.T, X @ Wv.T
    Y = torch.zeros(B, m, A, dtype=X.dtype)
    Ps = []
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        P = torch.softmax(scale * Q[:, :, c] @ K[:, :, c].transpose(1, 2), -1)
        Ps.append(P)
        Y[:, :, c] = P @ V[:, :, c]
    if Wres is not None:
        Y = Y + X @ Wres.T
    dZ = dY * (Y > 0)
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    for h, P in enumerate(Ps):
        c = slice(h * hd, (h + 1) * hd)
        dV[:, :, c] = P.transpose(1, 2) @ dZ[:, :, c]
        dP = dZ[:, :, c] @ V[:, :, c].transpose(1, 2)
        dS = P * (dP - (dP * P).sum(-1, keepdim=True))
        dQ[:, :, c] = scale * dS @ K[:, :, c]
        dK[:, :, c] = scale * dS.transpose(1, 2) @ Q[:, :, c]
    dX = dQ @ Wq + dK @ Wk + dV @ Wv
    dWs = [torch.einsum("bia,bid->ad", g, X) for g in (dQ, dK, dV)]
    if Wres is not None:
        dX = dX + dZ @ Wres
        dWs.append(torch.einsum("bia,bid->ad", dZ, X))
    return dX, dWs


def stack_case(B, m, d_in, widths, seed, res=True, dtype=torch.float64, w_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, m * d_in, generator=g, dtype=dtype)
    layers, d = [], d_in
    for A in widths:
        ws = [torch.randn(A, d, generator=g, dtype=dtype) * (w_scale / math.sqrt(d)) for _ in range(4)]
        layers.append((ws[0], ws[1], ws[2], ws[3] if res else None))
        d = A
    dy = torch.randn(B, m * widths[-1], generator=g, dtype=dtype)
    return x0, layers, dy


def with_grad(x0, layers):
    x = x0.clone().requires_grad_()
    L = [tuple(None if w is None else w.clone().requires_grad_() for w in l) for l in layers]
    return x, L, [w for l in L for w in l if w is not None]


class RefAutoInt(nn.Module):
    """AutoInt in plain torch ops: nn.Embedding per field (and an [n, 1] first-order one), the
    interacting layers as batched matmuls and softmax, Linear -> ReLU for the MLP, Linear(., 1)
    heads.  ``bf16_points=True`` is the same model with every tensor the GPU path stores or
    multiplies in bf16 rounded there, value and gradient (the x0 rows, the layers' operands, Q,
    K, V, P, every layer's output, the MLP's activations; the weights as MFMA operands), fp32
    accumulation: what bf16 storage alone costs."""

    def __init__(self, category_nums, n_dense, emb_size, att_layers, heads, head_dim, layers, res=True,
                 scale=1.0, dtype=torch.float64, bf16_points=False):
        super().__init__()
        m, A = len(category_nums), heads * head_dim
        self.heads, self.scale = heads, scale
        self.emb = nn.ModuleList([nn.Embedding(n, emb_size) for n in category_nums])
        self.first = nn.ModuleList([nn.Embedding(n, 1) for n in category_nums])
        self.dense_weight = nn.Parameter(torch.zeros(n_dense)) if n_dense else None
        self.global_bias = nn.Parameter(torch.zeros(1))
        self.att = nn.ParameterList([nn.Parameter(torch.zeros(A, emb_size if k == 0 else A))
                                     for k in range(att_layers) for _ in range(4 if res else 3)])
        self.per = 4 if res else 3
        self.att_out = nn.Linear(m * A, 1, bias=False)
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
        X, m, H = v, v.shape[1], self.heads
        for k in range(len(self.att) // self.per):
            W = [rbv(w) for w in self.att[k * self.per:(k + 1) * self.per]]
            q, kk, vv = [rb(X @ w.T).view(B, m, H, -1).transpose(1, 2) for w in W[:3]]
            P = torch.softmax(self.scale * q @ kk.transpose(-1, -2), -1)
            O = (rb(P) @ vv).transpose(1, 2).reshape(B, m, -1)
            if self.per == 4:
                O = O + X @ W[3].T
            X = rb(torch.relu(O))
        logit = logit + (X.reshape(B, -1) @ self.att_out.weight.T).squeeze(-1)
        x = v.reshape(B, -1)
        if self.dense_weight is not None:
            x = torch.cat([x, rb(dense)], 1)
        for lin in self.mlp:
            x = rb(torch.relu(x @ rbv(lin.weight).T + lin.bias))
        return logit + (x @ self.out.weight.T + self.out.bias).squeeze(-1)


def autoint(rows=30, F=4, n_dense=2, D=8, att_layers=2, heads=2, head_dim=8, layers=(16,), device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import AutoInt
    sparse = [CategoricalColumnWithIdentity(rows, f"c{f}") for f in range(F)]
    dense = [NumericColumn(f"d{j}") for j in range(n_dense)]
    label = CategoricalColumnWithIdentity(2, "label")
    return AutoInt(sparse, dense, label, emb_size=D, layers=layers, att_layers=att_layers, att_heads=heads,
                   att_head_dim=head_dim, device=device, **kw)


def autoint_linears(m):
    """The product model's MLP Linears and output layer in RefAutoInt.linears() order."""
    return [x for x in m.mlp.modules() if isinstance(x, nn.Linear)] + [m.prediction]


def att_weights(m):
    return [w for l in m.att for w in l.weights() if w is not None]


def copy_into_ref(m, r):
    with torch.no_grad():
        for f in range(len(r.emb)):
            r.emb[f].weight.copy_(m.embeddings.table(f).to(r.emb[f].weight.dtype).cpu())
            r.first[f].weight.copy_(m.embeddings.first_order(f).to(r.emb[f].weight.dtype).cpu().unsqueeze(1))
        if r.dense_weight is not None:
            r.dense_weight.copy_(m.dense_weight.cpu())
        r.global_bias.copy_(m.global_bias.cpu())
        for a, b in zip(att_weights(m), r.att):
            b.copy_(a.cpu())
        r.att_out.weight.copy_(m.att_out.weight.cpu())
        for a, b in zip(autoint_linears(m), r.linears()):
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
    for k, (a, b) in enumerate(zip(att_weights(m), r.att)):
        out.append((f"att{k // r.per}.{'qkvr'[k % r.per]}", a, b))
    out.append(("att_out", m.att_out.weight, r.att_out.weight))
    for i, (a, b) in enumerate(zip(autoint_linears(m), r.linears())):
        out.append((f"W{i}", a.weight, b.weight))
        out.append((f"b{i}", a.bias, b.bias))
    return out


# ---------------------------------------------------------------------------
# cpu_path.autoint
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,res", [(2, True), (5, False)])
def test_autoint_matches_the_literal_loop_in_fp64(m, res):
    from pytorchrec_amd import cpu_path
    x0, layers, _ = stack_case(3, m, 4, [8, 6], 10 + m, res)
    got = cpu_path.autoint(x0, layers, 2, 0.7)
    X = x0.reshape(3, m, 4)
    for l in layers:
        X = layer_loop(X, *l, 2, 0.7)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, m * 6)
    close_to_magnitude(got.numpy(), X.reshape(3, -1).numpy(), 1e-13, "y")


@pytest.mark.parametrize("res", [True, False])
def test_autoint_gradcheck(res):
    from pytorchrec_amd import cpu_path
    x0, layers, _ = stack_case(3, 4, 4, [8, 4], 21, res)
    x, L, flat = with_grad(x0, layers)
    n = 4 if res else 3

    def f(x, *ws):
        ws = list(ws)
        ls = [tuple(ws[k * n:(k + 1) * n]) + (() if res else (None,)) for k in range(2)]
        return cpu_path.autoint(x, ls, 2, 0.5, chunk=2)
    assert torch.autograd.gradcheck(f, (x, *flat))


@pytest.mark.parametrize("res", [True, False])
def test_written_backward_formulas_equal_autograd(res):
    from pytorchrec_amd import cpu_path
    x0, layers, dy = stack_case(4, 5, 8, [16], 31, res)
    x, L, flat = with_grad(x0, layers)
    cpu_path.autoint(x, L, 2, 0.6).backward(dy)
    dX, dWs = layer_backward(x0.reshape(4, 5, 8), *layers[0], 2, 0.6, dy.reshape(4, 5, 16))
    close_to_magnitude(x.grad.numpy(), dX.reshape(4, -1).numpy(), 1e-12, "dX")
    assert len(dWs) == len(flat)
    for name, w, g in zip("qkvr", flat, dWs):
        close_to_magnitude(w.grad.numpy(), g.numpy(), 1e-12, "dW" + name)


def test_autoint_reads_a_strided_slice_and_checks_its_arguments():
    from pytorchrec_amd import cpu_path, dense
    x0, layers, _ = stack_case(5, 3, 4, [8], 3, dtype=torch.float32)
    wide = torch.full((5, 16), float("nan"))
    wide[:, :12] = x0
    assert torch.equal(cpu_path.autoint(wide[:, :12], layers, 2), cpu_path.autoint(x0, layers, 2))
    assert torch.equal(dense.autoint(x0, 3, layers, 2, 0.5), cpu_path.autoint(x0, layers, 2, 0.5))
    with pytest.raises(ValueError):
        cpu_path.autoint(x0, [], 2)
    with pytest.raises(ValueError):
        cpu_path.autoint(x0[:, :11], layers, 2)
    with pytest.raises(ValueError):
        cpu_path.autoint(x0, layers, 3)  # 3 heads do not divide 8
    with pytest.raises(ValueError):
        cpu_path.autoint(x0, [layers[0], layers[0]], 2)  # the second layer's d_in is 8, not 4
    with pytest.raises(ValueError):
        dense.autoint(x0, 5, layers, 2)


def test_autoint_does_not_depend_on_the_batch_chunking():
    """Forward and gradients per chunk size: a sample's y and dx are its own arithmetic only; dW
    sums the chunks in another order, so it agrees to fp32 rounding."""
    from pytorchrec_amd import cpu_path
    x0, layers, dy = stack_case(11, 5, 4, [8, 8], 4, dtype=torch.float32)
    outs = []
    for chunk in (1, 4, 11, 256):
        x, L, flat = with_grad(x0, layers)
        y = cpu_path.autoint(x, L, 2, chunk=chunk)
        y.backward(dy)
        outs.append((y.detach(), x.grad, *[w.grad for w in flat]))
    for o in outs[1:]:
        close_to_magnitude(o[0].numpy(), outs[0][0].numpy(), 1e-6, "y")
        close_to_magnitude(o[1].numpy(), outs[0][1].numpy(), 1e-6, "dx")
        for u, v in zip(o[2:], outs[0][2:]):
            close_to_magnitude(u.numpy(), v.numpy(), 1e-5, "dW")


def test_autoint_bf16_rounding_points():
    """round_bf16 rounds the operands (X, the weights), Q K V, P and, for a bf16 x_dtype, Y --
    and nothing else: each point is shown by one input that only that rounding changes."""
    from pytorchrec_amd import cpu_path
    eps = 1 + 2.0 ** -10  # bf16 rounds it away
    g = torch.Generator().manual_seed(6)
    x0 = torch.randint(-1, 2, (4, 3 * 4), generator=g).float()
    ws = [torch.randint(-1, 2, (8, 4), generator=g).float() for _ in range(4)]
    ws[0].zero_()  # uniform attention: P = 1/3, which bf16 does not hold
    lay = [tuple(ws)]

    def run(x, layer, **kw):
        return cpu_path.autoint(x, [layer], 2, 1.0, **kw)
    exact = run(x0, lay[0])
    # (1) operands: X and each weight
    assert torch.equal(run(x0 * eps, lay[0], round_bf16=True), run(x0, lay[0], round_bf16=True))
    for k in range(4):
        w2 = list(ws); w2[k] = ws[k] * eps
        assert torch.equal(run(x0, tuple(w2), round_bf16=True), run(x0, lay[0], round_bf16=True))
    # (2) P: the rounded path uses bf16(1/3)
    p3 = torch.tensor(1 / 3).bfloat16().float()
    V = (x0.reshape(4, 3, 4) @ ws[2].T)
    want = torch.relu(p3 * V.sum(1, keepdim=True).expand(4, 3, 8) + x0.reshape(4, 3, 4) @ ws[3].T)
    got = run(x0, lay[0], round_bf16=True).reshape(4, 3, 8)
    assert torch.equal(got, want) and not torch.equal(got, exact.reshape(4, 3, 8))
    # (3) Q, K, V: a value V = 257 (not bf16) becomes 256; the residual product stays unrounded
    xv = torch.zeros(1, 2 * 4); xv[0, 0] = 257.0
    wv = [torch.zeros(8, 4) for _ in range(4)]
    wv[2][0, 0] = 1.0
    y = run(xv.bfloat16().float(), tuple(wv), round_bf16=True)  # X itself rounds to 256 first
    assert float(y[0, 0]) == 128.0
    xv2 = torch.zeros(1, 2 * 4); xv2[0, 0] = 1.0; xv2[0, 1] = 2.0 ** -8
    wv2 = [torch.zeros(8, 4) for _ in range(4)]
    wv2[2][0, 0] = 1.0; wv2[2][0, 1] = 1.0  # V[0, 0] = 1 + 2^-8: rounds to 1 (ties to even)
    assert float(run(xv2, tuple(wv2), round_bf16=True)[0, 0]) == 0.5
    assert float(run(xv2, tuple(wv2))[0, 0]) == 0.5 * (1 + 2.0 ** -8)
    # (4) O + X Wres^T is added unrounded and Y is rounded only into a bf16 x_dtype
    wr = [torch.zeros(8, 4) for _ in range(4)]
    wr[3][0, 0] = 1.0; wr[3][0, 1] = 1.0
    assert float(run(xv2, tuple(wr), round_bf16=True)[0, 0]) == 1 + 2.0 ** -8
    yb = run(xv2, tuple(wr), round_bf16=True, x_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16 and float(yb[0, 0]) == 1.0
    # (5) S and the softmax are not rounded: scores 1 + 2^-8 apart from 1 give unequal weights
    ws5 = [torch.zeros(8, 4) for _ in range(4)]
    ws5[0][0, 0] = 1.0; ws5[1][0, 0] = 1.0; ws5[1][0, 1] = 1.0; ws5[2][0, 2] = 1.0
    x5 = torch.zeros(1, 2 * 4)
    x5[0, 0] = 1.0; x5[0, 2] = 256.0  # field 0: Q = 1, K = 1, V = 256
    x5[0, 4 + 1] = 2.0 ** -7; x5[0, 4 + 2] = -256.0  # field 1: K = 2^-7, V = -256
    y5 = run(x5, tuple(ws5), round_bf16=True)
    assert float(y5[0, 0]) > 0  # P(key 0) > 1/2 only if exp(1 - 2^-7) was not flattened


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def test_registry_exports_and_arguments():
    import pytorchrec_amd.model as models
    from pytorchrec_amd.model import AutoInt, get_model_type, model_name_list
    assert get_model_type("autoint") is AutoInt and "autoint" in model_name_list
    assert models.AutoInt is AutoInt
    args = {a.name: a for a in AutoInt.get_argument_descriptions()}
    assert list(args) == ["emb_size", "layers", "att_layers", "att_heads", "att_head_dim", "att_res",
                          "att_scaling", "dropout"]
    assert [args[k].default_value for k in args] == [16, "400,400", 3, 2, 32, True, False, 0.0]
    ok = {k: args[k].default_value for k in args}
    AutoInt.check_argument_values(ok)
    with pytest.raises(AssertionError):
        AutoInt.check_argument_values({**ok, "att_heads": 0})
    with pytest.raises(AssertionError):
        AutoInt.check_argument_values({**ok, "dropout": 1.0})


def test_rejections():
    from pytorchrec_amd import sharding
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import AutoInt
    with pytest.raises(ValueError, match="sparse"):
        AutoInt([], [NumericColumn("d0")], CategoricalColumnWithIdentity(2, "label"))
    with pytest.raises(ValueError, match="att_heads \\* att_head_dim"):
        autoint(att_size=24)
    with pytest.raises(ValueError, match="positive"):
        autoint(att_layers=0)
    with pytest.raises(ValueError, match="layers"):
        autoint(layers="")
    with sharding.sharded_tables(None):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            autoint()


def test_state_dict_keys_and_round_trip(tmp_path):
    m = autoint(random_seed=3)
    keys = list(m.state_dict().keys())
    att = [f"att.{k}.{n}.weight" for k in range(2) for n in ("query", "key", "value", "res")]
    assert keys == ["dense_weight", "global_bias", "embeddings.weight", *att, "att_out.weight",
                    "mlp.mlp.dense_0.linear.weight", "mlp.mlp.dense_0.linear.bias",
                    "prediction.weight", "prediction.bias"]
    assert [tuple(l.query.weight.shape) for l in m.att] == [(16, 8), (16, 16)]
    assert tuple(m.att_out.weight.shape) == (1, 4 * 16) and m.att_out.bias is None
    assert m.embeddings.has_w and m.x0_cols == 40 and m.att_size == 16
    assert 0.005 < float(m.att[1].key.weight.detach().std()) < 0.02  # normal(0, 0.01) through the reset
    data, *_ = ctr_batch(m, 6)
    m.eval()
    with torch.no_grad():
        logit, target = m(data)
    assert tuple(logit.shape) == (6,) and target.dtype == torch.float32
    path = str(tmp_path / "a.pt")
    torch.save(m.state_dict(), path)
    m2 = autoint(random_seed=4)
    m2.eval()
    with torch.no_grad():
        assert not torch.equal(m2(data)[0], logit)
        m2.load_state_dict(torch.load(path))
        assert torch.equal(m2(data)[0], logit)
    m3 = autoint(n_dense=0, att_layers=1, att_res=False, att_scaling=True, layers="16,8")
    assert m3.dense_weight is None and not hasattr(m3.att[0], "res")
    assert "att.0.res.weight" not in m3.state_dict()
    d3, *_ = ctr_batch(m3, 5)
    assert tuple(m3(d3)[0].shape) == (5,)


def test_forward_and_train_step_match_the_fp64_model():
    """B = 64, 4 fields of 30 rows, 2 dense, D = 8, two layers of 2 x 8, layers [16]: the
    logits, the loss and every parameter update of one SGD step against RefAutoInt in fp64 from
    identical weights, within 1e-5 of each tensor's magnitude (the fp32 CPU path).  An update
    is read back as after - before from fp32 parameters, which adds half an ulp of the
    parameter that no arithmetic of the step made: the learning rate is large enough that every
    tensor's update is at least 5 % of its parameters' size, so that this stays below the bound."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    B, lr = 64, 100.0
    m = autoint(random_seed=11)
    with torch.no_grad():  # weights large enough that every layer matters
        for p in m.parameters():
            p.mul_(30.0)
    r = RefAutoInt([30] * 4, 2, 8, 2, 2, 8, (16,))
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


def good_args(m=5, d_in=8, heads=2, hd=8, B=4):
    """A valid description over fake (aligned) addresses, fp32 throughout."""
    from pytorchrec_amd import _mrec
    lib = _mrec.lib()
    A = heads * hd
    a = _mrec.AutoIntArgs()
    a.x, a.x_dtype, a.ld_x = 1 << 20, _mrec.F32, m * d_in
    a.w_fwd, a.ld_w_fwd = 2 << 20, d_in
    a.w_bwd, a.ld_w_bwd = 3 << 20, lib.mrec_autoint_image_rows(A)
    a.has_res, a.batch, a.n_fields, a.d_in, a.heads, a.head_dim, a.A, a.scale = 1, B, m, d_in, heads, hd, A, 1.0
    a.y, a.y_dtype, a.ld_y = 4 << 20, _mrec.F32, m * A
    a.dy, a.dy_dtype, a.ld_dy = 5 << 20, _mrec.F32, m * A
    a.dx, a.dx_dtype, a.ld_dx = 6 << 20, _mrec.F32, m * d_in
    a.dw, a.workspace = 7 << 20, 8 << 20
    a.workspace_bytes = lib.mrec_autoint_bwd_workspace_size(B, d_in, A)
    return a


def test_supported_answers_for_the_compiled_shapes(lib):
    from pytorchrec_amd import _mrec, dense
    f32, bf = _mrec.F32, _mrec.BF16
    for m in (2, 16, 17, 26, 32):
        for d in (8, 16, 32, 64):
            for heads, hd in ((2, 8), (1, 16), (4, 8), (2, 16), (1, 32), (8, 8), (4, 16), (2, 32)):
                assert lib.mrec_autoint_supported(m, d, heads, hd, f32, bf) == 1, (m, d, heads, hd)
                assert lib.mrec_autoint_supported(m, d, heads, hd, bf, f32) == 1
    for m, d, heads, hd in ((1, 16, 2, 8), (33, 16, 2, 8), (26, 12, 2, 8), (26, 128, 2, 8), (26, 16, 2, 12),
                            (26, 16, 1, 8), (26, 16, 3, 8), (26, 16, 4, 32), (26, 16, 1, 64), (26, 16, 0, 16),
                            (26, 16, 2, 4), (26, 0, 2, 8)):
        assert lib.mrec_autoint_supported(m, d, heads, hd, f32, f32) == 0, (m, d, heads, hd)
    assert lib.mrec_autoint_supported(26, 16, 2, 32, _mrec.I32, f32) == 0
    assert lib.mrec_autoint_supported(26, 16, 2, 32, f32, 9) == 0
    assert [lib.mrec_autoint_image_rows(A) for A in (16, 32, 64)] == [64, 128, 256]
    assert lib.mrec_autoint_bwd_workspace_size(0, 16, 64) == 0
    small, big = lib.mrec_autoint_bwd_workspace_size(1, 8, 16), lib.mrec_autoint_bwd_workspace_size(4096, 64, 64)
    assert 0 < small < big and small % 16 == 0 and big % 16 == 0
    assert big >= 4096 * 4 * 64 * 26 * 2  # at least the (dZ | dQ | dK | dV) rows in bf16
    assert dense.autoint_supported(26, 16, [64, 64, 64], 2, torch.bfloat16)
    assert dense.autoint_supported(5, 8, [16, 16, 16, 16], 2, torch.float32, torch.bfloat16)
    assert not dense.autoint_supported(26, 16, [64] * 5, 2)
    assert not dense.autoint_supported(26, 16, [], 2)
    assert not dense.autoint_supported(33, 16, [64], 2)
    assert not dense.autoint_supported(26, 16, [64, 24], 2)
    assert not dense.autoint_supported(26, 12, [64], 2)
    assert not dense.autoint_supported(26, 16, [64], 3)
    assert not dense.autoint_supported(26, 16, [64], 2, torch.float64)


def test_invalid_arguments_return_einval(lib):
    from pytorchrec_amd import _mrec
    both = ("mrec_autoint_fwd", "mrec_autoint_bwd")

    def refused(a, needle, fns=both):
        for fn in fns:
            st = getattr(lib, fn)(ctypes.byref(a) if a is not None else None, None)
            assert st == _mrec.EINVAL, fn
            msg = lib.mrec_last_error()
            assert msg and needle in msg, (fn, msg)

    refused(None, b"NULL")
    for field, value in (("d_in", 24), ("n_fields", 33), ("n_fields", 1)):
        a = good_args(); setattr(a, field, value)
        refused(a, b"unsupported shape")
    a = good_args(); a.heads = 3
    refused(a, b"heads * head_dim")
    a = good_args(); a.A = 32
    refused(a, b"heads * head_dim")
    a = good_args(heads=6, hd=8)  # A = 48: consistent, not compiled
    refused(a, b"unsupported shape")
    a = good_args(); a.ld_x = 5 * 8 + 2  # 168 bytes: not a multiple of 16
    refused(a, b"16-byte")
    a = good_args(); a.y = (4 << 20) + 4
    refused(a, b"16-byte")
    for field in ("x", "y", "w_fwd"):
        a = good_args(); setattr(a, field, None)
        refused(a, field.encode())
    for field in ("dy", "dx", "w_bwd", "dw", "workspace"):
        a = good_args(); setattr(a, field, None)
        refused(a, field.encode(), fns=both[1:])
    a = good_args(); a.ld_y = a.ld_y - 8
    refused(a, b"y needs")
    a = good_args(); a.ld_dx = a.ld_dx - 4
    refused(a, b"dx needs", fns=both[1:])
    a = good_args(); a.dy = (5 << 20) + 8
    refused(a, b"dy needs", fns=both[1:])
    a = good_args(); a.ld_w_bwd = a.ld_w_bwd - 8
    refused(a, b"w_bwd", fns=both[1:])
    a = good_args(); a.workspace_bytes = a.workspace_bytes - 1
    refused(a, b"workspace smaller", fns=both[1:])
    a = good_args(); a.workspace = (8 << 20) + 8
    refused(a, b"workspace", fns=both[1:])
    a = good_args(); a.x_dtype = _mrec.I32
    refused(a, b"dtype")
    a = good_args(); a.dx_dtype = 11
    refused(a, b"dtype", fns=both[1:])
    a = good_args(); a.batch = -1
    refused(a, b"batch")
    a = good_args(); a.batch = 1 << 31
    refused(a, b"batch")
    # batch = 0 launches nothing: no pointer is looked at
    a = good_args(); a.batch = 0; a.x = None; a.y = None; a.dw = None; a.workspace = None
    assert lib.mrec_autoint_fwd(ctypes.byref(a), None) == _mrec.OK
    assert lib.mrec_autoint_bwd(ctypes.byref(a), None) == _mrec.OK
