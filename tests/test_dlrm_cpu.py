"""CPU checks of the DLRM dot interaction and the DLRM model (no GPU).

* ``cpu_path.dot_interact`` -- the contract of include/mrec.h "DLRM dot interaction" in torch
  ops -- against hand-written vectors (the pair order), a double-loop numpy fp64 restatement,
  ``gradcheck``, and the backward formula the header writes down;
* the registry, the state-dict keys, the argument checks and dropout behaviour of ``DLRM``;
* one CPU ``train_step`` of a tiny DLRM against the same model written here in torch fp64
  from identical weights (``RefDLRM``; the GPU test reuses it);
* ``mrec_dot_interact_*``'s argument validation, which runs on the host before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_sasrec_cpu import close_to_magnitude


# ---------------------------------------------------------------------------
# restatements (shared with tests/test_gpu_dlrm.py)
# ---------------------------------------------------------------------------

def pair_count(n):
    return n * (n - 1) // 2


def vectors(bot, rows, F, D):
    """[B, n, D] float64: t_0 = bot (when given), t_i = the fields of rows."""
    t = np.asarray(rows, np.float64)[:, :F * D].reshape(-1, F, D)
    if bot is not None:
        t = np.concatenate([np.asarray(bot, np.float64)[:, None, :D], t], 1)
    return t


def interact_loops(bot, rows, F, D, x_cols):
    """The forward contract as a double loop over the pairs, fp64."""
    t = vectors(bot, rows, F, D)
    B, n, _ = t.shape
    Dh = D if bot is not None else 0
    x = np.zeros((B, x_cols))
    for b in range(B):
        if bot is not None:
            x[b, :D] = t[b, 0]
        for i in range(n):
            for j in range(i):
                x[b, Dh + i * (i - 1) // 2 + j] = float(np.dot(t[b, i], t[b, j]))
    return x


def gram_of(dx, n, Dh):
    """G [B, n, n]: symmetric, zero diagonal, G[i, j] = dx[b, Dh + i(i-1)/2 + j] for i > j."""
    dx = np.asarray(dx, np.float64)
    G = np.zeros((dx.shape[0], n, n))
    for i in range(n):
        for j in range(i):
            G[:, i, j] = G[:, j, i] = dx[:, Dh + i * (i - 1) // 2 + j]
    return G


def interact_bwd_formula(bot, rows, F, D, dx):
    """The backward contract as written in the header, fp64 -> (dbot or None, drows)."""
    t = vectors(bot, rows, F, D)
    B, n, _ = t.shape
    Dh = D if bot is not None else 0
    dt = np.einsum("bij,bjd->bid", gram_of(dx, n, Dh), t)
    if bot is None:
        return None, dt.reshape(B, F * D)
    return dt[:, 0] + np.asarray(dx, np.float64)[:, :D], dt[:, 1:].reshape(B, F * D)


class RefDLRM(nn.Module):
    """DLRM in plain torch ops: nn.Embedding per field, Linear -> ReLU towers, the lower
    triangle of the Gram matrix of [bot, v_0 .. v_{F-1}] in tril_indices order, Linear(., 1).
    ``bf16_points=True`` is the same model with every tensor the GPU path stores in bf16
    rounded there, value and gradient (the dense input, the gathered rows, tower activations,
    x; the weights as GEMM operands), fp32 accumulation: what bf16 storage alone costs."""

    def __init__(self, category_nums, n_dense, emb_size, bottom, top, dtype=torch.float64,
                 bf16_points=False):
        super().__init__()
        self.emb = nn.ModuleList([nn.Embedding(n, emb_size) for n in category_nums])
        self.bottom = nn.ModuleList([nn.Linear(a, b) for a, b in zip([n_dense, *bottom[:-1]], bottom)]
                                    if n_dense else [])
        n = len(category_nums) + (1 if n_dense else 0)
        top_in = (emb_size if n_dense else 0) + pair_count(n)
        self.top = nn.ModuleList([nn.Linear(a, b) for a, b in zip([top_in, *top[:-1]], top)])
        self.out = nn.Linear(top[-1], 1)
        self.bf16_points = bf16_points
        self.to(dtype)

    def linears(self):
        return list(self.bottom) + list(self.top) + [self.out]

    def forward(self, ids, dense):
        from oracle.models import _rb
        rb = _rb if self.bf16_points else (lambda t: t)
        lin = (lambda x, m: x @ rb(m.weight).T + m.bias)
        vs = [rb(e(ids[:, f])) for f, e in enumerate(self.emb)]
        head = []
        if len(self.bottom):
            h = rb(dense)
            for m in self.bottom:
                h = rb(torch.relu(lin(h, m)))
            vs, head = [h] + vs, [h]
        t = torch.stack(vs, 1)
        z = torch.bmm(t, t.transpose(1, 2))
        li, lj = torch.tril_indices(t.shape[1], t.shape[1], -1, device=t.device)
        x = rb(torch.cat(head + [z[:, li, lj]], 1))
        for m in self.top:
            x = rb(torch.relu(lin(x, m)))
        return (x @ self.out.weight.T + self.out.bias).squeeze(-1)


def dlrm_linears(m):
    """The product model's Linears in RefDLRM.linears() order."""
    mods = ([m.bottom_mlp] if m.bottom_mlp is not None else []) + [m.top_mlp]
    return [x for mod in mods for x in mod.modules() if isinstance(x, nn.Linear)] + [m.prediction]


def dlrm(rows=20, F=5, n_dense=3, D=8, bottom=(8, 8), top=(16, 8), device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import DLRM
    sparse = [CategoricalColumnWithIdentity(rows, f"c{f}") for f in range(F)]
    dense = [NumericColumn(f"d{j}") for j in range(n_dense)]
    label = CategoricalColumnWithIdentity(2, "label")
    return DLRM(sparse, dense, label, emb_size=D, bottom_layers=bottom, top_layers=top,
                device=device, **kw)


def copy_into_ref(m, r):
    with torch.no_grad():
        for f, e in enumerate(r.emb):
            e.weight.copy_(m.embeddings.table(f).to(e.weight.dtype).cpu())
        for a, b in zip(dlrm_linears(m), r.linears()):
            b.weight.copy_(a.weight.to(b.weight.dtype).cpu())
            b.bias.copy_(a.bias.to(b.bias.dtype).cpu())


def dlrm_batch(m, B, seed=0):
    """-> (data dict for the product model, ids int64 [B, F], dense fp32 [B, n] or None,
    label fp32 [B])."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randint(0, c.category_num, (B,), generator=g)
                       for c in m.sparse_columns], 1)
    dense = torch.rand(B, len(m.dense_columns), generator=g) if m.dense_columns else None
    label = (torch.rand(B, generator=g) < 0.3).float()
    data = {c.feature_name: ids[:, f].to(torch.int32) for f, c in enumerate(m.sparse_columns)}
    data.update({c.feature_name: dense[:, j] for j, c in enumerate(m.dense_columns)})
    data["label"] = label.long()
    return data, ids, dense, label


def ref_train_step(r, lr, ids, dense, label):
    opt = torch.optim.SGD(r.parameters(), lr=lr)
    logit = r(ids, dense)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, label.to(logit.dtype))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


# ---------------------------------------------------------------------------
# cpu_path.dot_interact
# ---------------------------------------------------------------------------

def test_pair_order_is_literal():
    """n = 3, D = 2: x = [t0 | t1.t0, t2.t0, t2.t1 | 0 pad]."""
    from pytorchrec_amd import cpu_path
    bot = torch.tensor([[1., 2.]])
    rows = torch.tensor([[3., 4., 5., -6.]])
    x = cpu_path.dot_interact(bot, rows, 2, 2, 8)
    assert x.tolist() == [[1., 2., 3. + 8., 5. - 12., 15. - 24., 0., 0., 0.]]
    x = cpu_path.dot_interact(None, rows, 2, 2, 3)
    assert x.tolist() == [[15. - 24., 0., 0.]]
    n = 7
    li, lj = torch.tril_indices(n, n, -1)
    assert [(int(i), int(j)) for i, j in zip(li, lj)] == [(i, j) for i in range(n) for j in range(i)]
    assert all(i * (i - 1) // 2 + j == p for p, (i, j) in enumerate(zip(li.tolist(), lj.tolist())))


@pytest.mark.parametrize("with_bot", [True, False], ids=["bot", "nobot"])
@pytest.mark.parametrize("F,D", [(1, 8), (5, 16), (26, 16), (31, 8)])
def test_forward_matches_the_double_loop(F, D, with_bot):
    from pytorchrec_amd import cpu_path
    rng = np.random.default_rng(F * 100 + D)
    B = 3
    rows = rng.standard_normal((B, F * D))
    bot = rng.standard_normal((B, D)) if with_bot else None
    n = F + with_bot
    width = (D if with_bot else 0) + pair_count(n)
    for x_cols in (width, width + 5):
        want = interact_loops(bot, rows, F, D, x_cols)
        got = cpu_path.dot_interact(None if bot is None else torch.from_numpy(bot),
                                    torch.from_numpy(rows), F, D, x_cols)
        assert got.dtype == torch.float64 and tuple(got.shape) == (B, x_cols)
        if x_cols:  # (one field and no bottom vector: no pair, x is the pad alone)
            close_to_magnitude(got.numpy(), want, 1e-13, f"x F={F} D={D}")
        assert np.all(got.numpy()[:, width:] == 0)
    with pytest.raises(ValueError):
        cpu_path.dot_interact(None if bot is None else torch.from_numpy(bot), torch.from_numpy(rows),
                              F, D, width - 1)


def test_round_bf16_rounds_the_products_operands_only():
    from pytorchrec_amd import cpu_path
    g = torch.Generator().manual_seed(1)
    bot, rows = torch.randn(4, 8, generator=g), torch.randn(4, 24, generator=g)
    x = cpu_path.dot_interact(bot, rows, 3, 8, 16, round_bf16=True)
    want = interact_loops(bot.bfloat16().double().numpy(), rows.bfloat16().double().numpy(), 3, 8, 16)
    assert torch.equal(x[:, :8], bot)  # the copy of t_0 is not rounded
    close_to_magnitude(x[:, 8:].numpy(), want[:, 8:], 1e-6, "pairs of bf16 operands")
    assert not np.allclose(x[:, 8:14].numpy(), interact_loops(bot.numpy(), rows.numpy(), 3, 8, 16)[:, 8:14],
                           rtol=0, atol=1e-6)


def test_gradcheck_fp64():
    from pytorchrec_amd import cpu_path
    g = torch.Generator().manual_seed(2)
    bot = torch.randn(2, 8, generator=g, dtype=torch.float64, requires_grad=True)
    rows = torch.randn(2, 24, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda b, r: cpu_path.dot_interact(b, r, 3, 8, 16), (bot, rows))
    assert torch.autograd.gradcheck(lambda r: cpu_path.dot_interact(None, r, 3, 8, 5), (rows,))


@pytest.mark.parametrize("with_bot", [True, False], ids=["bot", "nobot"])
def test_written_backward_formula_is_autograd(with_bot):
    from pytorchrec_amd import cpu_path
    F, D, B = 5, 8, 3
    g = torch.Generator().manual_seed(3)
    bot = torch.randn(B, D, generator=g, dtype=torch.float64, requires_grad=True) if with_bot else None
    rows = torch.randn(B, F * D, generator=g, dtype=torch.float64, requires_grad=True)
    width = (D if with_bot else 0) + pair_count(F + with_bot)
    x = cpu_path.dot_interact(bot, rows, F, D, width + 3)
    dx = torch.randn(B, width + 3, generator=g, dtype=torch.float64)
    x.backward(dx)
    dbot, drows = interact_bwd_formula(None if bot is None else bot.detach().numpy(),
                                       rows.detach().numpy(), F, D, dx.numpy())
    close_to_magnitude(rows.grad.numpy(), drows, 1e-13, "drows")
    if with_bot:
        close_to_magnitude(bot.grad.numpy(), dbot, 1e-13, "dbot")
    G = gram_of(dx.numpy(), F + with_bot, D if with_bot else 0)
    assert np.all(G == G.transpose(0, 2, 1)) and np.all(np.einsum("bii->bi", G) == 0)


def test_dense_dot_interact_on_cpu_is_the_cpu_path():
    from pytorchrec_amd import cpu_path, dense
    g = torch.Generator().manual_seed(4)
    bot, rows = torch.randn(4, 8, generator=g), torch.randn(4, 40, generator=g)
    x = dense.dot_interact(bot, rows, 5)
    assert tuple(x.shape) == (4, 24) and x.dtype == torch.float32  # 8 + 15 = 23 -> 24
    assert torch.equal(x, cpu_path.dot_interact(bot, rows, 5, 8, 24))
    assert torch.equal(dense.dot_interact(None, rows, 5, x_cols=11), cpu_path.dot_interact(None, rows, 5, 8, 11))
    with pytest.raises(ValueError):
        dense.dot_interact(bot, rows, 5, x_cols=22)
    with pytest.raises(ValueError):
        dense.dot_interact(bot, rows, 3)
    assert dense.DOT_INTERACT is True


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def test_registry_and_arguments():
    from pytorchrec_amd.model import DLRM, get_model_type, model_name_list
    assert get_model_type("dlrm") is DLRM and "dlrm" in model_name_list
    names = [a.name for a in DLRM.get_argument_descriptions()]
    assert names == ["emb_size", "bottom_layers", "top_layers", "dropout"]
    DLRM.check_argument_values({"emb_size": 16, "bottom_layers": "512,256,64,16", "top_layers": "512,256",
                                "dropout": 0.0})
    with pytest.raises(AssertionError):
        DLRM.check_argument_values({"emb_size": 16, "bottom_layers": "64,16", "top_layers": "32",
                                    "dropout": 1.0})


def test_state_dict_keys():
    m = dlrm()
    assert list(m.state_dict().keys()) == [
        "embeddings.weight",
        "bottom_mlp.mlp.dense_0.linear.weight", "bottom_mlp.mlp.dense_0.linear.bias",
        "bottom_mlp.mlp.dense_1.linear.weight", "bottom_mlp.mlp.dense_1.linear.bias",
        "top_mlp.mlp.dense_0.linear.weight", "top_mlp.mlp.dense_0.linear.bias",
        "top_mlp.mlp.dense_1.linear.weight", "top_mlp.mlp.dense_1.linear.bias",
        "prediction.weight", "prediction.bias"]
    assert m.top_in == 8 + 15 and m.x_cols == 24
    assert tuple(m.top_mlp.mlp.dense_0.linear.weight.shape) == (16, 23)
    assert not m.embeddings.has_w
    m2 = dlrm(n_dense=0, bottom=())
    assert m2.bottom_mlp is None and m2.top_in == 10
    assert not any(k.startswith("bottom_mlp") for k in m2.state_dict())
    data, *_ = dlrm_batch(m2, 6)
    logit, target = m2(data)
    assert tuple(logit.shape) == (6,) and target.dtype == torch.float32


def test_bottom_must_end_at_emb_size():
    with pytest.raises(ValueError, match="emb_size"):
        dlrm(D=8, bottom=(8, 16))
    dlrm(D=8, bottom="16,8")  # the CLI string form


def test_sharded_tables_are_refused():
    from pytorchrec_amd import sharding
    with sharding.sharded_tables(None):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            dlrm()


def test_dropout_runs_in_train_mode_only():
    m = dlrm(dropout=0.5)
    data, *_ = dlrm_batch(m, 32)
    m.eval()
    with torch.no_grad():
        a, b = m(data)[0], m(data)[0]
    assert torch.equal(a, b)
    m.train()
    torch.manual_seed(0)
    with torch.no_grad():
        c = m(data)[0]
        d = m(data)[0]
    assert not torch.equal(c, d) and not torch.equal(a, c)


def test_forward_and_train_step_match_the_fp64_model():
    """B = 64, F = 5, 3 dense, D = 8, bottom [8, 8], top [16, 8]: the logits, the loss and
    every parameter update of one SGD step against RefDLRM in fp64 from identical weights,
    within 1e-5 of each tensor's magnitude (the fp32 CPU path).  An update is read back as
    after - before from fp32 parameters, which adds half an ulp of the parameter (2^-24 of
    it) that no arithmetic of the step made: the learning rate is large enough that every
    tensor's update is of its parameters' own size, so that this stays far below the bound."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    B, lr = 64, 200.0
    m = dlrm(random_seed=11)
    with torch.no_grad():  # weights large enough that every layer matters
        for p in m.parameters():
            p.mul_(20.0)
    r = RefDLRM([20] * 5, 3, 8, (8, 8), (16, 8))
    copy_into_ref(m, r)
    data, ids, dense, label = dlrm_batch(m, B)
    m.eval()
    with torch.no_grad():
        logit, target = m(data)
        close_to_magnitude(logit.numpy(), r(ids, dense.double()).numpy(), 1e-5, "logit")
    assert torch.equal(target, label)
    before_t = [e.weight.detach().clone() for e in r.emb]
    before_l = [(x.weight.detach().clone(), x.bias.detach().clone()) for x in r.linears()]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], torch.device("cpu"))
    loss = float(m.train_step(data)["loss"].detach())
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    print(f"loss {loss:.8f} against {rloss:.8f}")
    assert abs(loss - rloss) <= 1e-5 * abs(rloss)
    for f, e in enumerate(r.emb):
        want = (e.weight.detach() - before_t[f]).numpy()
        assert np.abs(want).max() > 0.05 * float(before_t[f].abs().max())
        close_to_magnitude((m.embeddings.table(f).detach().double() - before_t[f]).numpy(), want,
                           1e-5, f"table {f} update")
    for i, (a, b) in enumerate(zip(dlrm_linears(m), r.linears())):
        for name, got, new, old in (("W", a.weight, b.weight, before_l[i][0]),
                                    ("b", a.bias, b.bias, before_l[i][1])):
            want = (new.detach() - old).numpy()
            assert np.abs(want).max() > 0.05 * float(old.abs().max()), (name, i)
            close_to_magnitude((got.detach().double() - old).numpy(), want, 1e-5, f"{name}{i} update")


# ---------------------------------------------------------------------------
# the library's argument checks (host only: nothing is launched)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorchrec_amd import _mrec
    return _mrec.lib()


def good_args(F=5, D=8, B=4, bot=True):
    """A valid description over fake (aligned) addresses, fp32 throughout."""
    from pytorchrec_amd import _mrec
    n = F + bot
    width = (D if bot else 0) + pair_count(n)
    ld = (width + 7) // 8 * 8
    a = _mrec.DotInteractArgs()
    if bot:
        a.bot, a.bot_dtype, a.ld_bot = 1 << 20, _mrec.F32, D
    a.rows, a.rows_dtype, a.ld_rows = 2 << 20, _mrec.F32, F * D
    a.batch, a.n_fields, a.D = B, F, D
    a.x, a.x_dtype, a.ld_x, a.x_cols = 3 << 20, _mrec.F32, ld, width
    a.dx, a.dx_dtype, a.ld_dx = 4 << 20, _mrec.F32, ld
    a.dbot, a.ld_dbot = 5 << 20, D
    a.drows, a.ld_drows = 6 << 20, F * D
    return a


def test_supported_answers_for_the_compiled_shapes(lib):
    from pytorchrec_amd import _mrec, dense
    f32, bf = _mrec.F32, _mrec.BF16
    for D in (8, 16, 32, 64, 128):
        for F in (1, 26, 31):
            for dts in ((f32, f32, f32, f32), (bf, bf, bf, bf), (f32, bf, bf, f32), (bf, f32, f32, bf)):
                assert lib.mrec_dot_interact_supported(D, F, *dts) == 1
    for D, F in ((24, 26), (4, 26), (256, 26), (0, 1), (16, 0), (16, 32), (16, -1)):
        assert lib.mrec_dot_interact_supported(D, F, f32, f32, f32, f32) == 0
    assert lib.mrec_dot_interact_supported(16, 26, _mrec.I32, f32, f32, f32) == 0
    assert lib.mrec_dot_interact_supported(16, 26, f32, f32, f32, 9) == 0
    assert dense.dot_interact_supported(16, 26, torch.bfloat16, torch.bfloat16, torch.bfloat16, torch.bfloat16)
    assert not dense.dot_interact_supported(24, 26)
    assert not dense.dot_interact_supported(16, 32)
    assert not dense.dot_interact_supported(16, 26, torch.float64)


def test_invalid_arguments_return_einval(lib):
    from pytorchrec_amd import _mrec

    def refused(a, needle, fns=("mrec_dot_interact_fwd", "mrec_dot_interact_bwd")):
        for fn in fns:
            st = getattr(lib, fn)(ctypes.byref(a) if a is not None else None, None)
            assert st == _mrec.EINVAL, fn
            msg = lib.mrec_last_error()
            assert msg and needle in msg, (fn, msg)

    refused(None, b"NULL")
    a = good_args(); a.D = 24
    refused(a, b"unsupported shape")
    a = good_args(); a.n_fields = 32
    refused(a, b"unsupported shape")
    a = good_args(); a.x_cols = a.x_cols - 1
    refused(a, b"x_cols", fns=("mrec_dot_interact_fwd",))
    a = good_args(); a.ld_rows = 5 * 8 + 2  # 168 bytes: not a multiple of 16
    refused(a, b"16-byte")
    a = good_args(); a.ld_x = a.ld_x + 1
    refused(a, b"16-byte", fns=("mrec_dot_interact_fwd",))
    a = good_args(); a.dx = (4 << 20) + 4
    refused(a, b"16-byte", fns=("mrec_dot_interact_bwd",))
    a = good_args(); a.rows = None
    refused(a, b"rows")
    a = good_args(); a.rows_dtype = _mrec.I32
    refused(a, b"dtype")
    a = good_args(); a.x_dtype = 11
    refused(a, b"dtype")
    a = good_args(); a.batch = -1
    refused(a, b"batch")
    a = good_args(); a.batch = 1 << 31
    refused(a, b"batch")
    # batch = 0 launches nothing: no pointer is looked at
    a = good_args(); a.batch = 0; a.rows = None; a.x = None
    assert lib.mrec_dot_interact_fwd(ctypes.byref(a), None) == _mrec.OK
    assert lib.mrec_dot_interact_bwd(ctypes.byref(a), None) == _mrec.OK
