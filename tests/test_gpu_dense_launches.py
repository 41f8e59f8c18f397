"""Which libmrec launches one forward + backward of the dense ops enqueues, in which
order, and carrying which deferred work.

``_mrec.call`` is wrapped: every call is recorded and then passed on, so the kernels
still run.  A trace holds, per call, its name and

* for ``mrec_gemm_multi`` / ``mrec_gemm_multi_ex`` (and the ``reduce`` array of any
  entry point that takes one) each job's ``(M, N, K, split_k, phase, ones column,
  b_cols, C dtype)``, the epilogue's ``(sgd flag, lr, img_kind)`` and which of
  ``mask, add, ones_out, img_row, img_tr`` are null (1 = null);
* for ``mrec_tower_dw_ex`` ``(n_layers, batch, splits, n_out, n_in)`` and whether the
  head finish and the feed job are null;
* for ``mrec_ctr_head_finish`` and a head-finish job ``(B, H, ns, update, lr)`` and
  which of ``g, w, bias, ws, b2, dw_out, db_out, dws_out, db2_out`` are null.

No address is recorded.  Every case runs with the three gradient destinations: SGD
fused into the backward (``_mrec_sgd_group``), the data-parallel flat buffer
(``_mrec_dp_grad`` views, shaped as IModel.distribute shapes them) and gradients
returned to autograd.  Numerical parity is the business of test_gpu_dense.py,
test_gpu_tower.py and test_gpu_pins.py; here the gradients are only checked to have
arrived (finite and non-zero, the parameter or the flat buffer changed), so that a
trace cannot match on a path that did nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

from pytorchrec_amd import _mrec

pytestmark = pytest.mark.gpu

MODES = ("sgd", "dp", "ret")
LR = 0.1


# --------------------------------------------------------------------------------
# the recorder
# --------------------------------------------------------------------------------
def _null(*ptrs):
    return tuple(int(not p) for p in ptrs)


def _job(j):
    e = j.epi.contents
    return ((j.M, j.N, j.K, j.split_k, j.phase, j.b_ones_col, j.b_cols, j.c_dtype),
            (e.update, round(e.lr, 6), e.img_kind),
            _null(e.mask, e.add, e.ones_out, e.img_row, e.img_tr))


def _finish(f):
    return ((f.batch, f.H, f.ns, f.update, round(f.lr, 6)),
            _null(f.g, f.w, f.bias, f.ws, f.b2, f.dw_out, f.db_out, f.dws_out, f.db2_out))


def _event(name, args):
    ev = [name]
    for i, a in enumerate(args):  # a GemmCall array follows its length
        if isinstance(a, ctypes.Array) and a._type_ is _mrec.GemmCall:
            ev.append(tuple(_job(a[k]) for k in range(args[i - 1])))
    if name == "mrec_gemm_multi_ex":
        ev.append(_finish(args[3]._obj) if args[3] is not None else None)
    elif name == "mrec_tower_dw_ex":
        a = args[0]._obj
        n = a.n_layers
        ev.append((n, a.batch, a.splits, tuple(a.n_out[:n]), tuple(a.n_in[:n])))
        ev.append(_finish(args[1]._obj) if args[1] is not None else None)
        ev.append(int(args[2] is None))
    elif name == "mrec_ctr_head_finish":
        part, ldp, B, H, ns, g, update, lr = args[:8]
        ev.append(((B, H, ns, update, round(ctypes.c_float(lr).value, 6)), _null(g, *args[8:16])))
    return tuple(ev)


@pytest.fixture
def trace(monkeypatch):
    events = []
    real = _mrec.call

    def call(name, *args):
        events.append(_event(name, args))
        return real(name, *args)

    monkeypatch.setattr(_mrec, "call", call)
    return events


# --------------------------------------------------------------------------------
# the three destinations
# --------------------------------------------------------------------------------
def _mark(params, mode):
    if mode == "sgd":
        group = {"lr": LR}
        for p in params:
            p._mrec_sgd_group = group
    if mode != "dp":
        return
    layout, off = [], 0
    for p in params:
        n, k = (1, p.numel()) if p.dim() < 2 else p.shape
        ld = (k + 7) // 8 * 8
        layout.append((p, n, k, ld, off))
        off += n * ld
    flat = torch.zeros(off, dtype=torch.float32, device=params[0].device)
    for p, n, k, ld, o in layout:
        view = flat[o:o + n * ld].view(n, ld)[:, :k]
        p._mrec_dp_grad = view if p.dim() == 2 else view.reshape(-1)


def _arrived(t):
    return t is not None and bool(torch.isfinite(t).all()) and bool((t != 0).any())


def _finish_case(D, params, before, mode, no_dp):
    """``no_dp``: the parameters of an op without a data-parallel branch (cross, head),
    which returns their gradients in dp mode and leaves their flat views alone."""
    D.flush_pending()
    assert not D._PENDING and not D._FINISH and not D._FEED_JOB
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        if mode == "ret" or (mode == "dp" and any(p is q for q in no_dp)):
            assert _arrived(p.grad), i
            assert mode == "ret" or not bool((p._mrec_dp_grad != 0).any()), i
        elif mode == "sgd":
            assert p.grad is None and bool((p.detach() != before[i]).any()), i
            assert bool(torch.isfinite(p.detach()).all()), i
        else:
            assert p.grad is None and _arrived(p._mrec_dp_grad), i


def _rows(B, K, gpu, seed, scale=1.0):
    """bf16 [B, K] with 16-byte aligned rows and zero pad columns, as the models feed."""
    from pytorchrec_amd import dense as D
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, D._r8(K), dtype=torch.bfloat16, device=gpu)
    x[:, :K] = (torch.randn(B, K, generator=g) * scale).to(torch.bfloat16).to(gpu)
    return x[:, :K]


def _linears(dims, gpu, seed):
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(k, n).to(gpu) for k, n in dims]
    with torch.no_grad():
        for lin in lins:
            lin.weight.normal_(0, 1.0 / np.sqrt(lin.in_features))
            lin.bias.normal_(0.1, 0.1)
    return lins


def _labels(B, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, generator=g) < 0.3).float().to(gpu)


def _tower(widths, gpu, seed):
    from pytorchrec_amd.model.layer import MLP
    torch.manual_seed(seed)
    mlp = MLP(widths[0], list(widths[1:]), "relu", 0.0).to(gpu)
    head = torch.nn.Linear(widths[-1], 1).to(gpu)
    with torch.no_grad():
        for lin in [d.linear for d in mlp.mlp]:
            lin.weight.normal_(0, 1.0 / np.sqrt(lin.in_features))
            lin.bias.normal_(0.1, 0.1)
        head.weight.normal_(0, 1.0 / np.sqrt(widths[-1]))
        head.bias.fill_(0.05)
    return mlp, head


# --------------------------------------------------------------------------------
# the cases: each returns the parameters whose gradients the backward must deliver,
# those of them whose op has no data-parallel branch, and the forward + backward
# --------------------------------------------------------------------------------
def _case_mlp(D, gpu, B, mode):
    l1, l2, hd = _linears([(24, 40), (40, 16), (16, 1)], gpu, seed=B)
    g = torch.Generator().manual_seed(B + 1)
    xs = torch.rand(B, 3, generator=g).to(gpu)
    ws = (torch.randn(3, generator=g) * 0.1).to(gpu).requires_grad_()
    b2 = torch.full((1,), 0.02, device=gpu).requires_grad_()
    params = [l1.weight, l1.bias, l2.weight, l2.bias, hd.weight, hd.bias, ws, b2]
    _mark(params, mode)
    x = _rows(B, 24, gpu, seed=B + 2).requires_grad_()

    def run():
        h = D.linear(x, l1.weight, l1.bias, act="relu")
        h = D.linear(h, l2.weight, l2.bias, act="relu")
        loss, _ = D.ctr_head_bce(h, hd.weight, hd.bias, None, _labels(B, gpu, B + 3), xs=xs, ws=ws,
                                 b2=b2)
        loss.backward(D.grad_one(gpu))
    return params, [], run


def _case_cross_net(D, gpu, B, mode):
    c1, c2 = _linears([(24, 24), (24, 24)], gpu, seed=B + 10)
    params = [c1.weight, c1.bias, c2.weight, c2.bias]
    _mark(params, mode)
    x0 = _rows(B, 24, gpu, seed=B + 11).requires_grad_()
    g = _rows(B, 24, gpu, seed=B + 12, scale=0.1)

    def run():
        D.cross_net(x0, [c1.weight, c2.weight], [c1.bias, c2.bias]).backward(g)
    return params, [], run


def _case_cross(D, gpu, B, mode):
    c1, = _linears([(24, 24)], gpu, seed=B + 20)
    params = [c1.weight, c1.bias]
    _mark(params, mode)
    x0 = _rows(B, 24, gpu, seed=B + 21).requires_grad_()
    g = _rows(B, 24, gpu, seed=B + 22, scale=0.1)

    def run():
        D.cross(x0, x0, c1.weight, c1.bias).backward(g)
    return params, params, run


def _case_head(D, gpu, B, mode):
    l1, hd = _linears([(24, 16), (16, 1)], gpu, seed=B + 30)
    params = [l1.weight, l1.bias, hd.weight, hd.bias]
    _mark(params, mode)
    x = _rows(B, 24, gpu, seed=B + 31).requires_grad_()
    dz = torch.randn(B, generator=torch.Generator().manual_seed(B + 32)).to(gpu) * 0.1

    def run():
        h = D.linear(x, l1.weight, l1.bias, act="relu")
        D.head(h, hd.weight, hd.bias).backward(dz)
    return params, [hd.weight, hd.bias], run


def _case_tower(D, gpu, B, mode, C=0):
    mlp, head = _tower((24, 64, 32), gpu, seed=B + 40 + C)
    cross = _linears([(24, 24)] * C, gpu, seed=B + 41)
    params = (list(mlp.parameters()) + list(head.parameters())
              + [p for c in cross for p in c.parameters()])
    _mark(params, mode)
    x0 = _rows(B, 24, gpu, seed=B + 42).requires_grad_()
    y = _labels(B, gpu, B + 43)

    def run():
        assert D.tower_supported(x0, mlp, head, cross=cross or None)
        D.tower_bce(x0, mlp, head, None, y, cross=cross or None).backward(D.grad_one(gpu))
    return params, [], run


def _case_tower_cross(D, gpu, B, mode):
    return _case_tower(D, gpu, B, mode, C=1)


def _case_score_tower(D, gpu, B, mode):
    mlp, head = _tower((32, 48, 16), gpu, seed=B + 50)
    params = list(mlp.parameters()) + list(head.parameters())
    _mark(params, mode)
    x0 = _rows(B, 32, gpu, seed=B + 51).requires_grad_()
    ds = torch.randn(B, generator=torch.Generator().manual_seed(B + 52)).to(gpu) * 0.1

    def run():
        assert D.tower_supported(x0, mlp, head)
        D.score_tower(x0, mlp, head).backward(ds)
    return params, [], run


CASES = {
    "mlp-64": (_case_mlp, 64), "mlp-512": (_case_mlp, 512),
    "cross_net-64": (_case_cross_net, 64), "cross_net-512": (_case_cross_net, 512),
    "cross-64": (_case_cross, 64),
    "head-64": (_case_head, 64),
    "tower-128": (_case_tower, 128), "tower-512": (_case_tower, 512),
    "tower_cross-512": (_case_tower_cross, 512),
    "score_tower-512": (_case_score_tower, 512), "score_tower-128": (_case_score_tower, 128),
}


def run_case(name, mode, gpu, events):
    """One forward + backward of ``name`` with destination ``mode``; -> the trace."""
    from pytorchrec_amd import dense as D
    make, B = CASES[name]
    D.flush_pending()
    params, no_dp, run = make(D, gpu, B, mode)
    before = [p.detach().clone() for p in params]
    del events[:]
    run()
    _finish_case(D, params, before, mode, no_dp)
    return list(events)


# --------------------------------------------------------------------------------
# the expected traces
# --------------------------------------------------------------------------------
EXPECTED = {('cross-64', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',)],
 ('cross-64', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',)],
 ('cross-64', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',)],
 ('cross_net-512', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                           ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',),
                           ('mrec_gemm_multi',
                            (((512, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                             ((24, 24, 512, 2, 1, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)))),
                           ('mrec_dcn_cross_bwd_prep',),
                           ('mrec_gemm_multi',
                            (((512, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                             ((24, 24, 512, 2, 1, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                             ((24, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)))),
                           ('mrec_gemm_multi',
                            (((24, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),))],
 ('cross_net-512', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                            ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',), ('mrec_gemm',),
                            ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',), ('mrec_gemm',),
                            ('mrec_gemm',)],
 ('cross_net-512', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                            ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',),
                            ('mrec_gemm_multi',
                             (((512, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                              ((24, 24, 512, 2, 1, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)))),
                            ('mrec_dcn_cross_bwd_prep',),
                            ('mrec_gemm_multi',
                             (((512, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                              ((24, 24, 512, 2, 1, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),
                              ((24, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)))),
                            ('mrec_gemm_multi',
                             (((24, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),))],
 ('cross_net-64', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                          ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',),
                          ('mrec_gemm_multi',
                           (((64, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                            ((24, 24, 64, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)))),
                          ('mrec_dcn_cross_bwd_prep',),
                          ('mrec_gemm_multi',
                           (((64, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),
                            ((24, 24, 64, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('cross_net-64', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                           ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',), ('mrec_gemm',),
                           ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',), ('mrec_gemm',),
                           ('mrec_gemm',)],
 ('cross_net-64', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',),
                           ('mrec_gemm',), ('mrec_dcn_cross_bwd_prep',),
                           ('mrec_gemm_multi',
                            (((64, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),)),
                           ('mrec_gemm_multi',
                            (((24, 24, 64, 1, 0, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),)),
                           ('mrec_dcn_cross_bwd_prep',),
                           ('mrec_gemm_multi',
                            (((64, 24, 24, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 0, 1, 1, 1)),)),
                           ('mrec_gemm_multi',
                            (((24, 24, 64, 1, 0, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),))],
 ('head-64', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_head_fwd',), ('mrec_head_bwd',),
                     ('mrec_colsum',),
                     ('mrec_gemm_multi',
                      (((64, 24, 16, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),
                       ((16, 24, 64, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('head-64', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_head_fwd',), ('mrec_head_bwd',),
                      ('mrec_colsum',), ('mrec_gemm',), ('mrec_gemm',)],
 ('head-64', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_head_fwd',), ('mrec_head_bwd',),
                      ('mrec_colsum',),
                      ('mrec_gemm_multi',
                       (((64, 24, 16, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),)),
                      ('mrec_gemm_multi',
                       (((16, 24, 64, 1, 0, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),))],
 ('mlp-512', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                     ('mrec_ctr_head_fwd',),
                     ('mrec_gemm_multi_ex',
                      (((512, 40, 16, 1, 0, -1, 40, 1), (0, 0.0, 0), (0, 1, 1, 1, 1)),
                       ((16, 40, 512, 2, 1, 40, 40, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))),
                      ((512, 16, 3, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 0, 0))),
                     ('mrec_gemm_multi',
                      (((512, 24, 40, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),
                       ((40, 24, 512, 2, 1, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                       ((16, 40, 512, 2, 2, 40, 40, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)))),
                     ('mrec_gemm_multi',
                      (((40, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),))],
 ('mlp-512', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                      ('mrec_ctr_head_fwd',),
                      ('mrec_ctr_head_finish', ((512, 16, 3, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 0, 0))),
                      ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',)],
 ('mlp-512', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                      ('mrec_ctr_head_fwd',),
                      ('mrec_gemm_multi_ex',
                       (((512, 40, 16, 1, 0, -1, 40, 1), (0, 0.0, 0), (0, 1, 1, 1, 1)),
                        ((16, 40, 512, 2, 1, 40, 40, 0), (1, 0.1, 0), (1, 1, 0, 0, 0))),
                       ((512, 16, 3, 1, 0.1), (1, 0, 0, 0, 0, 1, 1, 1, 1))),
                      ('mrec_gemm_multi',
                       (((512, 24, 40, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),
                        ((40, 24, 512, 2, 1, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),
                        ((16, 40, 512, 2, 2, 40, 40, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)))),
                      ('mrec_gemm_multi',
                       (((40, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),))],
 ('mlp-64', 'dp'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                    ('mrec_ctr_head_fwd',),
                    ('mrec_gemm_multi_ex',
                     (((64, 40, 16, 1, 0, -1, 40, 1), (0, 0.0, 0), (0, 1, 1, 1, 1)),
                      ((16, 40, 64, 1, 0, 40, 40, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))),
                     ((64, 16, 3, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 0, 0))),
                    ('mrec_gemm_multi',
                     (((64, 24, 40, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),
                      ((40, 24, 64, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('mlp-64', 'ret'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                     ('mrec_ctr_head_fwd',),
                     ('mrec_ctr_head_finish', ((64, 16, 3, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 0, 0))),
                     ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',), ('mrec_gemm',)],
 ('mlp-64', 'sgd'): [('mrec_weight_prep',), ('mrec_gemm',), ('mrec_weight_prep',), ('mrec_gemm',),
                     ('mrec_ctr_head_fwd',),
                     ('mrec_gemm_multi_ex',
                      (((64, 40, 16, 1, 0, -1, 40, 1), (0, 0.0, 0), (0, 1, 1, 1, 1)),),
                      ((64, 16, 3, 1, 0.1), (1, 0, 0, 0, 0, 1, 1, 1, 1))),
                     ('mrec_gemm_multi',
                      (((16, 40, 64, 1, 0, 40, 40, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),)),
                     ('mrec_gemm_multi',
                      (((64, 24, 40, 1, 0, -1, 24, 1), (0, 0.0, 0), (1, 1, 1, 1, 1)),)),
                     ('mrec_gemm_multi',
                      (((40, 24, 64, 1, 0, 24, 24, 0), (1, 0.1, 0), (1, 1, 0, 0, 0)),))],
 ('score_tower-128', 'dp'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                             ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                             ('mrec_gemm_multi_ex',
                              (((48, 32, 128, 1, 0, 32, 32, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                               ((16, 48, 128, 1, 0, 48, 48, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))),
                              ((128, 16, 0, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 1, 1)))],
 ('score_tower-128', 'ret'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                              ('mrec_ctr_head_finish',
                               ((128, 16, 0, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 1, 1))),
                              ('mrec_gemm_multi',
                               (((48, 32, 128, 1, 0, 32, 32, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                                ((16, 48, 128, 1, 0, 48, 48, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('score_tower-128', 'sgd'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                              ('mrec_gemm_multi_ex',
                               (((48, 32, 128, 1, 0, 32, 32, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                                ((16, 48, 128, 1, 0, 48, 48, 0), (1, 0.1, 1), (1, 1, 0, 0, 0))),
                               ((128, 16, 0, 1, 0.1), (1, 0, 0, 1, 1, 1, 1, 1, 1)))],
 ('score_tower-512', 'dp'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                             ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                             ('mrec_tower_dw_ex', (2, 512, 2, (48, 16), (32, 48)),
                              ((512, 16, 0, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 1, 1)), 1),
                             ('mrec_gemm_multi',
                              (((48, 32, 512, 2, 2, 32, 32, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                               ((16, 48, 512, 2, 2, 48, 48, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('score_tower-512', 'ret'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                              ('mrec_ctr_head_finish',
                               ((512, 16, 0, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 1, 1))),
                              ('mrec_tower_dw_ex', (2, 512, 2, (48, 16), (32, 48)), None, 1),
                              ('mrec_gemm_multi',
                               (((48, 32, 512, 2, 2, 32, 32, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                                ((16, 48, 512, 2, 2, 48, 48, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('score_tower-512', 'sgd'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_fwd_bwd',), ('mrec_tower_fwd_bwd',),
                              ('mrec_tower_dw_ex', (2, 512, 2, (48, 16), (32, 48)),
                               ((512, 16, 0, 1, 0.1), (1, 0, 0, 1, 1, 1, 1, 1, 1)), 1),
                              ('mrec_gemm_multi',
                               (((48, 32, 512, 2, 2, 32, 32, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                                ((16, 48, 512, 2, 2, 48, 48, 0), (1, 0.1, 1), (1, 1, 0, 0, 0))))],
 ('tower-128', 'dp'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                       ('mrec_tower_fwd_bwd',),
                       ('mrec_gemm_multi_ex',
                        (((64, 24, 128, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                         ((32, 64, 128, 1, 0, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))),
                        ((128, 32, 0, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 1, 1)))],
 ('tower-128', 'ret'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                        ('mrec_tower_fwd_bwd',),
                        ('mrec_ctr_head_finish',
                         ((128, 32, 0, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 1, 1))),
                        ('mrec_gemm_multi',
                         (((64, 24, 128, 1, 0, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                          ((32, 64, 128, 1, 0, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('tower-128', 'sgd'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                        ('mrec_tower_fwd_bwd',),
                        ('mrec_gemm_multi_ex',
                         (((64, 24, 128, 1, 0, 24, 24, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                          ((32, 64, 128, 1, 0, 64, 64, 0), (1, 0.1, 1), (1, 1, 0, 0, 0))),
                         ((128, 32, 0, 1, 0.1), (1, 0, 0, 1, 1, 1, 1, 1, 1)))],
 ('tower-512', 'dp'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                       ('mrec_tower_fwd_bwd',),
                       ('mrec_tower_dw_ex', (2, 512, 2, (64, 32), (24, 64)),
                        ((512, 32, 0, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 1, 1)), 1),
                       ('mrec_gemm_multi',
                        (((64, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                         ((32, 64, 512, 2, 2, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('tower-512', 'ret'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                        ('mrec_tower_fwd_bwd',),
                        ('mrec_ctr_head_finish',
                         ((512, 32, 0, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 1, 1))),
                        ('mrec_tower_dw_ex', (2, 512, 2, (64, 32), (24, 64)), None, 1),
                        ('mrec_gemm_multi',
                         (((64, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                          ((32, 64, 512, 2, 2, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('tower-512', 'sgd'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                        ('mrec_tower_fwd_bwd',),
                        ('mrec_tower_dw_ex', (2, 512, 2, (64, 32), (24, 64)),
                         ((512, 32, 0, 1, 0.1), (1, 0, 0, 1, 1, 1, 1, 1, 1)), 1),
                        ('mrec_gemm_multi',
                         (((64, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                          ((32, 64, 512, 2, 2, 64, 64, 0), (1, 0.1, 1), (1, 1, 0, 0, 0))))],
 ('tower_cross-512', 'dp'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                             ('mrec_tower_weight_prep',), ('mrec_tower_fwd_bwd',),
                             ('mrec_tower_dw_ex', (3, 512, 2, (24, 64, 32), (24, 24, 64)),
                              ((512, 32, 0, 0, 0.0), (1, 1, 1, 1, 1, 0, 0, 1, 1)), 1),
                             ('mrec_gemm_multi',
                              (((24, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                               ((64, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                               ((32, 64, 512, 2, 2, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('tower_cross-512', 'ret'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_weight_prep',), ('mrec_tower_fwd_bwd',),
                              ('mrec_ctr_head_finish',
                               ((512, 32, 0, 0, 0.0), (0, 1, 1, 1, 1, 0, 0, 1, 1))),
                              ('mrec_tower_dw_ex', (3, 512, 2, (24, 64, 32), (24, 24, 64)), None,
                               1),
                              ('mrec_gemm_multi',
                               (((24, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                                ((64, 24, 512, 2, 2, 24, 24, 0), (0, 0.0, 0), (1, 1, 0, 1, 1)),
                                ((32, 64, 512, 2, 2, 64, 64, 0), (0, 0.0, 0), (1, 1, 0, 1, 1))))],
 ('tower_cross-512', 'sgd'): [('mrec_tower_weight_prep',), ('mrec_tower_weight_prep',),
                              ('mrec_tower_weight_prep',), ('mrec_tower_fwd_bwd',),
                              ('mrec_tower_dw_ex', (3, 512, 2, (24, 64, 32), (24, 24, 64)),
                               ((512, 32, 0, 1, 0.1), (1, 0, 0, 1, 1, 1, 1, 1, 1)), 1),
                              ('mrec_gemm_multi',
                               (((24, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                                ((64, 24, 512, 2, 2, 24, 24, 0), (1, 0.1, 1), (1, 1, 0, 0, 0)),
                                ((32, 64, 512, 2, 2, 64, 64, 0), (1, 0.1, 1), (1, 1, 0, 0, 0))))]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_launch_trace(gpu, trace, name, mode):
    got = run_case(name, mode, gpu, trace)
    want = EXPECTED[name, mode]
    assert len(got) == len(want), [e[0] for e in got]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
