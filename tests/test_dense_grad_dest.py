"""Which of the three gradient destinations dense._grad_dest picks (CPU tensors carrying
the markers IModel.compile / IModel.distribute set): fused SGD only when every
parameter decided together has a group with one common lr, the data-parallel flat
buffer only when SGD did not apply and every one has a view, else returned gradients.
"""
import torch

from pytorchrec_amd import _mrec
from pytorchrec_amd import dense as D

N, K = 3, 5


def _pair(bias=True):
    W = torch.nn.Parameter(torch.randn(N, K))
    b = torch.nn.Parameter(torch.randn(N)) if bias else None
    return W, b, (torch.zeros(N, 8), torch.zeros(K, 8))


def _views(*params):
    for p in params:
        p._mrec_dp_grad = torch.zeros(p.shape)


def _check_returned(d, bias=True):
    assert d.where == "ret" and set(d.kw) == {"out", "ones_out", "out_dtype"}
    assert d.kw["out"] is d.dW and d.kw["ones_out"] is d.db
    assert d.dW.shape == (N, K) and d.dW.dtype == torch.float32
    assert (d.db.shape == (N,) and d.db.dtype == torch.float32) if bias else d.db is None


def test_sgd_needs_a_group_with_one_common_lr_on_every_parameter():
    W, b, imgs = _pair()
    g = {"lr": 0.25}
    W._mrec_sgd_group = b._mrec_sgd_group = g
    _views(W, b)  # SGD wins over the flat buffer
    gen = getattr(W, "_mrec_gen", 0)
    d = D._grad_dest(W, b, imgs, "rowtr")
    assert d.where == "sgd" and d.dW is None and d.db is None
    assert d.kw["sgd_lr"] == 0.25 and d.kw["img_kind"] == _mrec.IMG_ROW_TR
    assert d.kw["out"].data_ptr() == W.data_ptr() and d.kw["ones_out"].data_ptr() == b.data_ptr()
    assert d.kw["img_row"] is imgs[0] and d.kw["img_tr"] is imgs[1]
    assert W._mrec_gen == gen + 1  # the in-place update was announced (images_updated)
    assert D._grad_dest(W, b, imgs, "tower").kw["img_kind"] == _mrec.IMG_TOWER

    b._mrec_sgd_group = {"lr": 0.5}  # a mixed lr: not fused; the views are complete -> DP
    assert D._grad_dest(W, b, imgs, "rowtr").where == "dp"
    del b._mrec_sgd_group  # a parameter without a group
    assert D._grad_dest(W, b, imgs, "rowtr").where == "dp"


def test_dp_needs_a_view_on_every_parameter():
    W, b, imgs = _pair()
    _views(W, b)
    gen = getattr(W, "_mrec_gen", 0)
    d = D._grad_dest(W, b, imgs, "rowtr")
    assert d.where == "dp" and d.dW is None and d.db is None
    assert d.kw == {"out": W._mrec_dp_grad, "ones_out": b._mrec_dp_grad,
                    "out_dtype": torch.float32}
    assert getattr(W, "_mrec_gen", 0) == gen  # no in-place update
    del b._mrec_dp_grad
    _check_returned(D._grad_dest(W, b, imgs, "rowtr"))
    # an op without a data-parallel branch (dense.cross) never picks the flat buffer
    _views(W, b)
    _check_returned(D._grad_dest(W, b, imgs, "rowtr", D._decide((W, b), dp=False)))


def test_returned_otherwise():
    W, b, imgs = _pair()
    _check_returned(D._grad_dest(W, b, imgs, "rowtr"))
    W._mrec_sgd_group = {"lr": 0.1}
    b._mrec_sgd_group = {"lr": 0.2}  # a mixed lr and no views
    _check_returned(D._grad_dest(W, b, imgs, "rowtr"))


def test_a_missing_bias_is_ignored_by_the_decision():
    W, _, imgs = _pair(bias=False)
    _check_returned(D._grad_dest(W, None, imgs, "rowtr"), bias=False)
    _views(W)
    d = D._grad_dest(W, None, imgs, "rowtr")
    assert d.where == "dp" and d.kw["ones_out"] is None
    W._mrec_sgd_group = {"lr": 0.1}
    d = D._grad_dest(W, None, imgs, "rowtr")
    assert d.where == "sgd" and d.kw["ones_out"] is None


def test_layers_decided_together_share_the_destination():
    """The tower decides once over every W and b of its launch: one layer without a
    group sends all of them to the next destination."""
    (W1, b1, i1), (W2, b2, i2) = _pair(), _pair()
    g = {"lr": 0.1}
    for p in (W1, b1, W2):
        p._mrec_sgd_group = g
    assert D._decide([W1, W2, b1, b2]) == (None, None)
    assert D._grad_dest(W1, b1, i1, "tower", (None, None)).where == "ret"
    _views(W1, b1, W2, b2)
    lr, views = D._decide([W1, W2, b1, b2])
    assert lr is None
    assert all(v is p._mrec_dp_grad for v, p in zip(views, (W1, W2, b1, b2)))
    b2._mrec_sgd_group = g
    assert D._decide([W1, W2, b1, b2]) == (0.1, None)
