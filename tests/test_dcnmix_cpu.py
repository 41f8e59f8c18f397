"""CPU checks of the DCN-Mix cross stack and the DCNMix model (no GPU): ``cpu_path.cross_mix``
and its autograd against a per-sample fp64 loop written from include/mrec.h "DCN-Mix", the
registry, the host-only shape query at the envelope's edges, and one CPU ``train_step`` against
the model written here in torch fp64.  The restatements are shared with test_gpu_dcnmix.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from test_dlrm_cpu import dlrm_batch as ctr_batch, ref_train_step
from test_sasrec_cpu import close_to_magnitude

NAMES = ("V", "C", "U", "b", "gate")


def mix_case(B, d, K, r, layers, seed, dtype=torch.float64):
    """Operands that keep |x_l| of order 1 -> (x0, [(V, C, U, b, gate or None)], dy)."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std: (torch.randn(*s, generator=g, dtype=torch.float64) * std).to(dtype)  # noqa: E731
    L = [(n(K * r, d, std=d ** -0.5), n(K, r, r, std=r ** -0.5), n(d, K * r, std=(K * r) ** -0.5),
          n(d, std=0.1), n(K, d, std=d ** -0.5) if K > 1 else None) for _ in range(layers)]
    return n(B, d, std=0.5), L, n(B, d, std=1.0)


def sample_loop(x0, layers, dy):
    """The contract without rounding, one sample at a time in fp64 -> (x_L, dx0, per layer a
    dict of the parameter gradients)."""
    x0, dy = np.asarray(x0, np.float64), np.asarray(dy, np.float64)
    P = [{k: None if w is None else np.asarray(w.detach(), np.float64) for k, w in zip(NAMES, l)} for l in layers]
    K, r = P[0]["C"].shape[:2]
    grads = [{k: np.zeros_like(w) for k, w in p.items() if w is not None} for p in P]
    xL, dx0 = np.zeros_like(x0), np.zeros_like(x0)
    for n in range(x0.shape[0]):
        x, kept = x0[n], []
        for p in P:
            a = np.tanh((p["V"] @ x).reshape(K, r))
            c = np.tanh(np.einsum("ijk,ik->ij", p["C"], a))
            gam = np.ones(1)
            if K > 1:
                e = np.exp(p["gate"] @ x - (p["gate"] @ x).max())
                gam = e / e.sum()
            s = (gam[:, None] * c).reshape(-1)
            z = p["U"] @ s + p["b"]
            kept.append((x, a, c, gam, s, z))
            x = x0[n] * z + x
        xL[n], g = x, dy[n]
        for p, gr, (x, a, c, gam, s, z) in zip(P[::-1], grads[::-1], kept[::-1]):
            dz = g * x0[n]
            dx0[n] += g * z
            ds = (p["U"].T @ dz).reshape(K, r)
            e = (ds * c).sum(1)
            dlogit = gam * (e - (gam * e).sum())
            du = gam[:, None] * ds * (1 - c * c)
            dt = np.einsum("ikj,ik->ij", p["C"], du) * (1 - a * a)
            gr["U"] += np.outer(dz, s)
            gr["b"] += dz
            gr["C"] += np.einsum("ij,ik->ijk", du, a)
            gr["V"] += np.outer(dt.reshape(-1), x)
            g = g + p["V"].T @ dt.reshape(-1)
            if K > 1:
                gr["gate"] += np.outer(dlogit, x)
                g = g + p["gate"].T @ dlogit
        dx0[n] += g
    return xL, dx0, grads


def run(fn, x0, layers, dy, **kw):
    """fn(x0, layers) forward and backward on fresh leaves -> (y, dx0, per layer grads dict)."""
    x = x0.detach().clone().requires_grad_()
    L = [tuple(None if w is None else w.detach().clone().requires_grad_() for w in l) for l in layers]
    y = fn(x, L, **kw)
    y.backward(dy.to(y.dtype))
    return y.detach(), x.grad, [{k: w.grad for k, w in zip(NAMES, l) if w is not None} for l in L]


class RefDCNMix(nn.Module):
    """DCNMix in plain torch ops, fp64: nn.Embedding per field, x0 = [rows | dense], the cross
    stack as batched matmuls, Linear -> ReLU, Linear(., 1)."""

    def __init__(self, category_nums, n_dense, emb_size, n_cross, K, r, layers):
        super().__init__()
        d = len(category_nums) * emb_size + n_dense
        self.K, self.r = K, r
        self.emb = nn.ModuleList([nn.Embedding(n, emb_size) for n in category_nums])
        shapes = {"V": (K * r, d), "C": (K, r, r), "U": (d, K * r), "b": (d,), "gate": (K, d)}
        self.cross = nn.ModuleList([nn.ParameterDict({k: nn.Parameter(torch.zeros(s)) for k, s in shapes.items()
                                                      if K > 1 or k != "gate"}) for _ in range(n_cross)])
        self.mlp = nn.ModuleList([nn.Linear(a, b) for a, b in zip([d, *layers[:-1]], layers)])
        self.out = nn.Linear(layers[-1], 1)
        self.double()

    def forward(self, ids, dense):
        x0 = torch.cat([e(ids[:, f]) for f, e in enumerate(self.emb)] + ([dense] if dense is not None else []), 1)
        x = x0
        for p in self.cross:
            a = torch.tanh(x @ p["V"].T).view(-1, self.K, self.r)
            c = torch.tanh(torch.einsum("bik,ijk->bij", a, p["C"]))
            if self.K > 1:
                c = c * torch.softmax(x @ p["gate"].T, -1).unsqueeze(-1)
            x = x0 * (c.reshape(len(x), -1) @ p["U"].T + p["b"]) + x
        for lin in self.mlp:
            x = torch.relu(lin(x))
        return self.out(x).squeeze(-1)


def dcnmix(rows=30, F=3, n_dense=2, D=4, n_cross=2, K=2, r=16, layers=(16,), device=None, **kw):
    from pytorchrec_amd.feature_column import CategoricalColumnWithIdentity, NumericColumn
    from pytorchrec_amd.model import DCNMix
    sparse = [CategoricalColumnWithIdentity(rows, f"c{f}") for f in range(F)]
    dense = [NumericColumn(f"d{j}") for j in range(n_dense)]
    return DCNMix(sparse, dense, CategoricalColumnWithIdentity(2, "label"), emb_size=D, cross_layers=n_cross,
                  layers=layers, cross_rank=r, cross_experts=K, device=device, **kw)


def named_pairs(m, r):
    """(name, the product model's tensor, the reference's) for every parameter."""
    out = [(f"table{f}", m.embeddings.table(f), e.weight) for f, e in enumerate(r.emb)]
    for l, (a, b) in enumerate(zip(m.cross, r.cross)):
        out += [(f"cross{l}.{k}", w, b[k]) for k, w in zip(NAMES, a.weights()) if w is not None]
    lins = [x for x in m.mlp.modules() if isinstance(x, nn.Linear)] + [m.prediction]
    for i, (a, b) in enumerate(zip(lins, list(r.mlp) + [r.out])):
        out += [(f"W{i}", a.weight, b.weight), (f"b{i}", a.bias, b.bias)]
    return out


def copy_into_ref(m, r):
    with torch.no_grad():
        for _, a, b in named_pairs(m, r):
            b.copy_(a.detach().to(b.dtype).cpu())


@pytest.mark.parametrize("B,d,K,r,layers", [(5, 13, 2, 16, 2), (3, 40, 1, 16, 1)])
def test_cross_mix_and_its_autograd_match_the_per_sample_loop(B, d, K, r, layers):
    """The fp32 torch-ops path against the fp64 loop: 1e-5 of each quantity's magnitude, the
    bar test_autoint_cpu.py holds its fp32 path to."""
    from pytorchrec_amd import cpu_path
    x0, L, dy = mix_case(B, d, K, r, layers, 3, torch.float32)
    xL, dx0, grads = sample_loop(x0, L, dy)
    y, dx, gs = run(cpu_path.cross_mix, x0, L, dy)
    close_to_magnitude(y.numpy(), xL, 1e-5, "x_L")
    close_to_magnitude(dx.numpy(), dx0, 1e-5, "dx0")
    for l, (got, want) in enumerate(zip(gs, grads)):
        assert set(got) == set(want)
        for k in want:
            close_to_magnitude(got[k].numpy(), want[k], 1e-5, f"layer {l} d{k}")


def test_registry_answers_dcnmix():
    from pytorchrec_amd.model import DCNMix, get_model_type
    assert get_model_type("dcnmix") is DCNMix
    names = {a.name for a in DCNMix.get_argument_descriptions()}
    assert {"cross_rank", "cross_experts", "cross_layers", "layers"} <= names


@pytest.mark.parametrize("d,K,r,layers,ok", [(512, 4, 64, 4, True), (513, 4, 64, 4, False), (1, 1, 16, 1, True),
                                             (429, 1, 24, 3, False), (429, 5, 16, 3, False), (429, 5, 64, 3, False),
                                             (429, 4, 64, 5, False), (429, 4, 64, 3, True)])
def test_supported_at_the_edges_of_the_envelope(d, K, r, layers, ok):
    """Host only: d = 512 / 513, r = 24, K = 4 / 5, K r = 256 / 320, layers = 4 / 5."""
    from pytorchrec_amd import _mrec
    assert bool(_mrec.lib().mrec_cross_mix_supported(d, K, r, layers)) is ok


def test_train_step_matches_the_fp64_model():
    """B = 64, 3 fields of 30 rows, 2 dense, D = 4 (d = 14), two layers of 2 experts of rank
    16, layers [16]: the loss and every parameter's update of one SGD step against RefDCNMix
    from identical weights, within 1e-5 of each tensor's magnitude (the fp32 CPU path)."""
    from pytorchrec_amd.loss import BCEWithLogitsLoss
    B, lr = 64, 100.0
    m = dcnmix(random_seed=11)
    with torch.no_grad():  # weights large enough that every layer matters
        for name, p in m.named_parameters():
            p.mul_(1.0 if name.split(".")[-1] in ("V", "C", "U") else 30.0)
    r = RefDCNMix([30] * 3, 2, 4, 2, 2, 16, (16,))
    copy_into_ref(m, r)
    data, ids, dense, label = ctr_batch(m, B)
    before = [b.detach().clone() for _, _, b in named_pairs(m, r)]
    m.compile(torch.optim.SGD(m.get_parameters(), lr=lr), BCEWithLogitsLoss(), [], torch.device("cpu"))
    loss = float(m.train_step(data)["loss"].detach())
    rloss = ref_train_step(r, lr, ids, dense.double(), label)
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    for (name, got, new), old in zip(named_pairs(m, r), before):
        want = (new.detach() - old).numpy()
        assert np.abs(want).max() > 0, name
        close_to_magnitude((got.detach().double() - old).numpy(), want, 1e-5, f"{name} update")
