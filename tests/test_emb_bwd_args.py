"""What the embedding-backward entry points refuse, one bad argument at a time.

Every case takes an argument list the entry point accepts, spoils exactly one value
and asserts MREC_EINVAL with a non-empty mrec_last_error() (or the MREC_ENOSPC of a
short workspace).  All of these checks run on the host before any launch, so a
refused call must leave the bank and the gradient buffer untouched.

* CPU part (unmarked): the large-batch entries -- mrec_emb_bwd_large_apply, _fused,
  _fused_ex, _fused_bag, _fused_given.  Nothing is dereferenced before the checks,
  so aligned fake addresses stand in for device memory.
* GPU part (marked gpu): the seven mrec_emb_bwd_apply* entries, whose layout rule
  needs a real mrec_emb_bwd_plan in the workspace first.  Every pointer there is a
  real, large-enough device buffer.
"""
import ctypes

import pytest

from pytorchrec_amd import _mrec

F, ROWS, D, B = 2, 32, 16, 8          # two tables of 32 rows, dim 16, batch 8
STRIDE_W = 32                          # bf16 row [v(16) | w | pad]: 64 bytes
LD = F * D                             # columns of dx / x0
CHUNK = 4                              # exchange view: 2 parts of 4 entries per table
REC = 36                               # bf16 wire record: 17 elements in 4-byte units
G_LD = 20                              # fp32 given rows: >= dim + w, a multiple of 4


@pytest.fixture(scope="module")
def lib():
    return _mrec.lib()


def _refused(lib, st, want=None):
    assert st == (_mrec.EINVAL if want is None else want), (st, lib.mrec_last_error())
    assert lib.mrec_last_error()


# --------------------------------------------------------------------------------
# argument lists by name: `a` holds every value any entry point takes
# --------------------------------------------------------------------------------
SRC = ("dx", "dx_dtype", "dx_ld", "dfm", "fm_sum", "x0", "x0_dtype", "x0_ld", "dw")
UPD = ("mode", "lr", "seed", "d_step", "grad")
CO = ("n_reduce", "reduce")
GIVEN = ("g_occ", "g_ld", "chunk", "chunk_stride")
WIRE = ("wire", "rec_bytes", "wire_dtype", "pref", "cap_rows", "chunk", "chunk_stride")
HEAD = ("bank", "batch", "ws", "ws_bytes")
LHEAD = ("bank", "ids", "batch", "ws", "ws_bytes", "oob")

ORDER = {
    "mrec_emb_bwd_apply": HEAD + SRC + UPD + ("stream",),
    "mrec_emb_bwd_apply_ex": HEAD + SRC + UPD + CO + ("stream",),
    "mrec_emb_bwd_apply_bag": HEAD + SRC + UPD + CO + ("stream", "bag_len", "bag_scale"),
    "mrec_emb_bwd_apply_given": HEAD + SRC + GIVEN + UPD + CO + ("stream",),
    "mrec_emb_bwd_apply_rec": HEAD + SRC + ("out",) + CO + ("stream",),
    "mrec_emb_bwd_apply_wire": HEAD + WIRE + UPD + CO + ("stream",),
    "mrec_emb_bwd_apply_wire_sgd": HEAD + WIRE + UPD + CO + ("sgd_table", "sgd_blocks", "stream"),
    "mrec_emb_bwd_large_apply": HEAD + SRC + UPD + ("stream",),
    "mrec_emb_bwd_large_fused": LHEAD + SRC + UPD + ("stream",),
    "mrec_emb_bwd_large_fused_ex": LHEAD + SRC + UPD + CO + ("stream",),
    "mrec_emb_bwd_large_fused_bag": LHEAD + SRC + UPD + CO + ("stream", "bag_len", "bag_scale"),
    "mrec_emb_bwd_large_fused_given": LHEAD + ("given",) + UPD + CO + ("stream",),
}


def _call(lib, name, a):
    """Call entry point `name` with the values of `a` in its own argument order."""
    a = dict(a)
    if "out" in ORDER[name]:
        out = a["out"]
        a["out"] = None if out is None else ctypes.byref(_mrec.GradRecords(*out))
    if "given" in ORDER[name]:
        a["given"] = ctypes.byref(_mrec.GivenGrads(
            a["g_occ"], a["g_ld"], a["chunk"], a["chunk_stride"], a["wire"], a["rec_bytes"],
            a["wire_dtype"], a["pref"], a["cap_rows"]))
    return getattr(lib, name)(*[a[k] for k in ORDER[name]])


def _accepted(p, **over):
    """An argument set every check accepts, from the addresses in `p`; no source of
    gradients is chosen yet (derived / given / wire below)."""
    a = dict(bank=p["bank"], ids=p["ids"], batch=B, ws=p["ws"], ws_bytes=p["ws_bytes"],
             oob=p["oob"], stream=None,
             dx=None, dx_dtype=_mrec.F32, dx_ld=0, dfm=None, fm_sum=None, x0=None,
             x0_dtype=_mrec.F32, x0_ld=0, dw=None,
             mode=_mrec.BWD_SGD, lr=0.1, seed=0, d_step=None, grad=p["grad"],
             n_reduce=0, reduce=None,
             g_occ=None, g_ld=0, chunk=0, chunk_stride=0,
             wire=None, rec_bytes=0, wire_dtype=_mrec.BF16, pref=None, cap_rows=0,
             out=(p["wire"], REC, p["pref"], CHUNK, B),
             bag_len=4, bag_scale=p["bag_scale"], sgd_table=None, sgd_blocks=0)
    a.update(over)
    return a


def _derived(p, **over):
    return _accepted(p, **{**dict(dx=p["dx"], dx_ld=LD), **over})


def _given(p, **over):
    return _accepted(p, **{**dict(g_occ=p["g_occ"], g_ld=G_LD, chunk=CHUNK,
                                  chunk_stride=F * CHUNK), **over})


def _wire(p, **over):
    return _accepted(p, **{**dict(wire=p["wire"], rec_bytes=REC, pref=p["pref"], cap_rows=B,
                                  chunk=CHUNK, chunk_stride=F * CHUNK), **over})


# one spoiled value per case: name -> the overrides, as a function of the addresses
DERIVED_CASES = {
    "dx_dtype": lambda p: dict(dx_dtype=_mrec.I32),
    "dx_ld_short": lambda p: dict(dx_ld=LD - 4),
    "dx_unaligned": lambda p: dict(dx=p["dx"] + 4),
    "dfm_without_fm_sum": lambda p: dict(dfm=p["dfm"], x0=p["x0"], x0_ld=LD),
    "x0_ld_short": lambda p: dict(dfm=p["dfm"], fm_sum=p["fm_sum"], x0=p["x0"], x0_ld=LD - 4),
}
# (the bag entries take no FM term at all: their dfm case is in BAG_CASES)
DERIVED_CASES_NO_FM = {k: DERIVED_CASES[k] for k in ("dx_dtype", "dx_ld_short", "dx_unaligned")}
UPDATE_CASES = {
    "mode_out_of_range": lambda p: dict(mode=6),
    "mode_negative": lambda p: dict(mode=-1),
    "dense_grad_without_grad": lambda p: dict(mode=_mrec.BWD_DENSE_GRAD, grad=None),
}
GIVEN_CASES = {
    "g_ld_short": lambda p: dict(g_ld=D),
    "g_ld_not_x4": lambda p: dict(g_ld=D + 2),
    "chunk_negative": lambda p: dict(chunk=-1),
    "chunk_stride_short": lambda p: dict(chunk_stride=F * CHUNK - 1),
}
WIRE_CASES = {
    "wire_dtype": lambda p: dict(wire_dtype=_mrec.I32),
    "rec_bytes_0": lambda p: dict(rec_bytes=0),
    "rec_bytes_6": lambda p: dict(rec_bytes=6),
    "record_narrower_than_row": lambda p: dict(rec_bytes=2 * D),
    "pref_null": lambda p: dict(pref=None),
    "cap_rows_0": lambda p: dict(cap_rows=0),
    "chunk_0": lambda p: dict(chunk=0),
}
BAG_CASES = {
    "bag_len_0": lambda p: dict(bag_len=0),
    "batch_not_multiple": lambda p: dict(bag_len=3),
    "bag_scale_null": lambda p: dict(bag_scale=None),
    "dfm_given": lambda p: dict(dfm=p["dfm"], fm_sum=p["fm_sum"], x0=p["x0"], x0_ld=LD),
}
REC_CASES = {
    "out_null": lambda p: dict(out=None),
    "rec_bytes_not_x4": lambda p: dict(out=(p["wire"], REC + 2, p["pref"], CHUNK, B)),
    "wire_null": lambda p: dict(out=(None, REC, p["pref"], CHUNK, B)),
    "cap_0": lambda p: dict(out=(p["wire"], REC, p["pref"], 0, B)),
    "record_narrower_than_row": lambda p: dict(out=(p["wire"], 2 * D, p["pref"], CHUNK, B)),
}
SGD_CASES = {
    "table_unaligned": lambda p: dict(sgd_table=p["sgd_table"] + 4, sgd_blocks=1),
    "blocks_without_table": lambda p: dict(sgd_table=None, sgd_blocks=1),
}


def _cases(entries, base, table):
    return [pytest.param(e, base, fn, id=f"{e[len('mrec_emb_bwd_'):]}-{c}")
            for e in entries for c, fn in table.items()]


# --------------------------------------------------------------------------------
# CPU part: the large-batch entries on fake addresses
# --------------------------------------------------------------------------------
LG_DERIVED = ("mrec_emb_bwd_large_apply", "mrec_emb_bwd_large_fused",
              "mrec_emb_bwd_large_fused_ex", "mrec_emb_bwd_large_fused_bag")
LG_ALL = LG_DERIVED + ("mrec_emb_bwd_large_fused_given",)


def _fake_bank(lib, dtype=_mrec.BF16, stride=STRIDE_W, has_w=1):
    rows = (ctypes.c_int64 * F)(*([ROWS] * F))
    offs = (ctypes.c_int64 * F)(*[f * ROWS for f in range(F)])
    bank = _mrec.TableBank(1 << 20, offs, rows, F, D, stride, has_w, dtype)
    ptrs = (ctypes.c_void_p * F)(*[(2 << 20) + 256 * f for f in range(F)])
    ids = _mrec.Ids(ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), _mrec.I32, 1)
    p = dict(bank=ctypes.byref(bank), ids=ctypes.byref(ids), ws=16 << 20,
             ws_bytes=lib.mrec_emb_bwd_large_workspace_size(ctypes.byref(bank), B), oob=3 << 20,
             dx=4 << 20, dfm=5 << 20, fm_sum=6 << 20, x0=7 << 20, dw=8 << 20, grad=9 << 20,
             g_occ=10 << 20, wire=11 << 20, pref=12 << 20, bag_scale=13 << 20,
             sgd_table=14 << 20, keep=(rows, offs, bank, ptrs, ids))
    assert p["ws_bytes"] > 0
    return p


@pytest.fixture(scope="module")
def fake(lib):
    return _fake_bank(lib)


def _source_of(entry):
    return _given if entry.endswith("_given") else _derived


@pytest.mark.parametrize("entry,base,spoil", _cases(LG_DERIVED[:3], _derived, DERIVED_CASES) +
                         _cases(LG_DERIVED[3:], _derived, DERIVED_CASES_NO_FM) +
                         _cases(LG_ALL, None, UPDATE_CASES) +
                         _cases(LG_ALL[-1:], _given, GIVEN_CASES) +
                         _cases(LG_ALL[-1:], _wire, WIRE_CASES) +
                         _cases(LG_DERIVED[-1:], _derived, BAG_CASES))
def test_large_entry_refuses_one_bad_argument(lib, fake, entry, base, spoil):
    base = base or _source_of(entry)
    _refused(lib, _call(lib, entry, base(fake, **spoil(fake))))


@pytest.mark.parametrize("entry", LG_DERIVED)
def test_large_entry_refuses_dw_on_a_bank_without_w(lib, entry):
    p = _fake_bank(lib, dtype=_mrec.F32, stride=D, has_w=0)
    _refused(lib, _call(lib, entry, _derived(p, dw=p["dw"])))


@pytest.mark.parametrize("case", ["both", "neither", "g_occ_chunk_0"])
def test_large_fused_given_takes_exactly_one_source(lib, fake, case):
    a = {"both": _given(fake, wire=fake["wire"], rec_bytes=REC, pref=fake["pref"], cap_rows=B),
         "neither": _accepted(fake, chunk=CHUNK, chunk_stride=F * CHUNK),
         "g_occ_chunk_0": _given(fake, chunk=0)}[case]
    _refused(lib, _call(lib, "mrec_emb_bwd_large_fused_given", a))


@pytest.mark.parametrize("entry", LG_ALL)
def test_large_entry_reports_a_short_workspace(lib, fake, entry):
    a = _source_of(entry)(fake, ws_bytes=fake["ws_bytes"] - 1)
    _refused(lib, _call(lib, entry, a), want=_mrec.ENOSPC)


# --------------------------------------------------------------------------------
# GPU part: the batched entries after one real plan per workspace
# --------------------------------------------------------------------------------
HASH_DERIVED = ("mrec_emb_bwd_apply", "mrec_emb_bwd_apply_ex", "mrec_emb_bwd_apply_bag",
                "mrec_emb_bwd_apply_given", "mrec_emb_bwd_apply_rec")
HASH_MODE = HASH_DERIVED[:4] + ("mrec_emb_bwd_apply_wire", "mrec_emb_bwd_apply_wire_sgd")
HASH_WIRE = HASH_MODE[-2:]
HASH_ALL = HASH_DERIVED + HASH_WIRE
SENTINEL = 0x5A


class _Planned:
    """A bank, a planned workspace and real buffers for every pointer argument."""

    def __init__(self, lib, dev, dtype, stride, has_w, batch):
        import torch
        self.torch = torch
        g = torch.Generator().manual_seed(7)
        self.weight = torch.randn(F * ROWS, stride, generator=g).to(dtype).to(dev)
        self.desc = _mrec.BankDesc(self.weight, [f * ROWS for f in range(F)], [ROWS] * F, D, has_w)
        self.id_t = [torch.randint(0, ROWS, (batch,), generator=g, dtype=torch.int32).to(dev)
                     for _ in range(F)]
        self.ids = _mrec.IdsDesc(self.id_t)
        nb = int(lib.mrec_emb_bwd_workspace_size(F, batch))
        self.ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        # every buffer is large enough for an accepted call of `batch` lookups
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.buf = dict(dx=f32(batch, LD + 4), dfm=f32(batch), fm_sum=f32(batch, D),
                        x0=f32(batch, LD + 4), dw=f32(batch), g_occ=f32(F * batch, G_LD),
                        wire=f32(F * batch, REC // 4 + 1), bag_scale=f32(batch, F),
                        pref=torch.zeros(F * batch, dtype=torch.int32, device=dev),
                        sgd_table=torch.zeros(int(lib.mrec_sgd_table_bytes()) + 16,
                                              dtype=torch.uint8, device=dev))
        self.grad = torch.full_like(self.weight.view(torch.uint8), SENTINEL)
        st = lib.mrec_emb_bwd_plan(self.desc.ref(), self.ids.ref(), batch, self.ws.data_ptr(), nb,
                                   self.oob.data_ptr(), None, _mrec.stream_handle(dev))
        assert st == _mrec.OK, lib.mrec_last_error()
        torch.cuda.synchronize(dev)
        self.bank_before = self.weight.view(torch.uint8).clone()
        self.p = dict(bank=self.desc.ref(), ids=self.ids.ref(), ws=self.ws.data_ptr(), ws_bytes=nb,
                      oob=self.oob.data_ptr(), grad=self.grad.data_ptr(),
                      **{k: v.data_ptr() for k, v in self.buf.items()})

    def untouched(self):
        torch = self.torch
        torch.cuda.synchronize(self.weight.device)
        assert torch.equal(self.weight.view(torch.uint8), self.bank_before)
        assert bool((self.grad == SENTINEL).all())


@pytest.fixture(scope="module")
def planned(lib, gpu):
    import torch
    return _Planned(lib, gpu, torch.bfloat16, STRIDE_W, True, B)


def _hash_source_of(entry):
    if "wire" in entry:
        return _wire
    return _derived


@pytest.mark.gpu
@pytest.mark.parametrize("entry,base,spoil", _cases(HASH_DERIVED[:2] + HASH_DERIVED[3:], _derived, DERIVED_CASES) +
                         _cases(HASH_DERIVED[2:3], _derived, DERIVED_CASES_NO_FM) +
                         _cases(HASH_MODE, None, UPDATE_CASES) +
                         _cases(HASH_DERIVED[3:4], _given, GIVEN_CASES) +
                         _cases(HASH_WIRE, _wire, WIRE_CASES) +
                         _cases(HASH_DERIVED[4:5], _derived, REC_CASES) +
                         _cases(HASH_DERIVED[2:3], _derived, BAG_CASES) +
                         _cases(HASH_WIRE[1:], _wire, SGD_CASES))
def test_batched_entry_refuses_one_bad_argument(lib, planned, entry, base, spoil):
    base = base or _hash_source_of(entry)
    p = planned.p
    _refused(lib, _call(lib, entry, base(p, **spoil(p))))
    planned.untouched()


@pytest.mark.gpu
def test_batched_given_refuses_g_occ_beside_dx(lib, planned):
    p = planned.p
    _refused(lib, _call(lib, "mrec_emb_bwd_apply_given", _given(p, dx=p["dx"], dx_ld=LD)))
    planned.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", HASH_DERIVED)
def test_batched_entry_refuses_dw_on_a_bank_without_w(lib, gpu, entry):
    import torch
    pl = _Planned(lib, gpu, torch.float32, D, False, B)
    _refused(lib, _call(lib, entry, _derived(pl.p, dw=pl.p["dw"])))
    pl.untouched()


@pytest.mark.gpu
def test_record_output_refuses_a_batch_of_the_sorted_layout(lib, gpu):
    import torch
    n = _mrec.BWD_HASH_MAX_BATCH + 1
    pl = _Planned(lib, gpu, torch.bfloat16, STRIDE_W, True, n)
    a = _derived(pl.p, batch=n, out=(pl.p["wire"], REC, pl.p["pref"], CHUNK, n))
    _refused(lib, _call(lib, "mrec_emb_bwd_apply_rec", a))
    pl.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", HASH_ALL)
def test_batched_entry_reports_a_short_workspace(lib, planned, entry):
    p = planned.p
    a = _hash_source_of(entry)(p, ws_bytes=p["ws_bytes"] - 1)
    _refused(lib, _call(lib, entry, a), want=_mrec.ENOSPC)
    planned.untouched()
