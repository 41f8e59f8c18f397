"""The fused tower (csrc/tower.hip, csrc/tower_dw.hip, tower_common.h: the entry
points mrec_tower_fwd_bwd and mrec_tower_dw) pinned to exact-integer expectations
at its edges, each against a plain fp64 restatement of include/mrec.h's contract.

Exact-integer method (as test_gpu_gemm_matrix.py has it for the GEMM).  x0 holds
-1 / 0 / 1, the weights are sparse with entries +-1, the biases, head_w, head_b, b2,
base, xs and ws are small integers and the given dz is +-2^-10 (or twice that).
Then every activation is a small integer and every gradient a small multiple of
2^-10: each value the kernel stores as bf16 is stored unchanged and each fp32 sum
is exact in any order, for any rotation of the k steps, any tile order, any split.
The expected value is computed in fp64 on the CPU and every comparison is
``torch.equal`` -- no tolerance; one dropped, doubled or misplaced term, tile, row
or store fails.  The only tolerances in this file are the BCE bars the layered head
already has (test_ctr_head_bce_fused_matches_torch): dz rtol 1e-5 / atol 1e-9, loss
rtol 1e-5 / atol 1e-6 -- the kernel's sigmoid uses __expf.  The BCE backward is tied
to the exact one instead: a GIVEN_DZ launch fed the BCE launch's own dz reproduces
every backward output bit for bit.

Three conditions on the inputs (not measurements: the generator asserts them, and
``test_case_conditions`` checks them on the CPU for every case of the matrix):

  * representable: x_c, z_c, every h_l, every dh_l, G_c, dz_c and dx0 survive a
    bf16 round trip;
  * order independent: for every fp32 accumulation (layer sums, head dot, head
    partials, dx0's G_0 + sum, dW over the batch) sum|terms| < 2^24 quanta (1 in the
    forward, the smallest |dz| in the backward);
  * sensitive: every 16 x 32 block of every weight (forward and backward blocking,
    edge blocks included) holds a non-zero, and for every layer, direction, 16-row
    block of the batch and (output tile, k step) pair the 16 x 16 partial product is
    non-zero somewhere; every ReLU is active on 25-75 % of its elements and every
    live row has dz != 0.  ``test_mutation_changes_expectation`` zeroes single
    weight blocks of the restatement and sees an expected output change.

Guards.  Every operand and output is a window of a larger allocation
(``_Guarded``).  x0 has ld = round8(K0) + 8 with pad columns [K0, round8) zero; what
the kernel must not read is NaN (rows >= B, columns >= round8, the elements of y /
dz_in / base / xs behind row B, everything around a weight image).  Outputs start
as 7.0: after the call the whole allocation equals the expected image -- live rows
exact, pad columns [N, round8(N)) zero, rows >= B, columns >= round8 and the
guards still 7.0; a k-fragment image equals the numpy layout of the expected
matrix over all mrec_kfrag_elems elements (rows >= B and the other half of the last
32-row step zero).  Nothing is read or written out of bounds, no case provokes a
fault.

What each shape of the matrix is there for:

  b1      B = 1, (7, 17), L = 1: x0's 16-byte chunk edge (K = 7); N = 17: a tile with
          one live column and a zero tile (ztiles > ntiles); no mask, dx0 straight
          from the head gradient; waves without a tile; ns = 0; H % 8 != 0
  b15     B = 15, (8, 16, 1): K = 8 (one whole chunk), N = 16, N = 1 (H = 1);
          ns = 1; base NULL
  b16     B = 16, (1, 128, 129): K = 1; N = 128 one tile per wave; N = 129: wave 0
          owns two tiles; the whole last 16-row half of a k-fragment step is zeroed
          by the only workgroup; head_b NULL
  b17     B = 17, (33, 400, 64): ksteps edge (K = 33: a 1-column k step); N = 400;
          a second block with one live row (12 non-zeros a row keep it sensitive);
          b2 NULL; h_out[0] NULL
  b33     B = 33, (32, 48, 33): K = 32 (one k step); the backward's 1-column k step
          (N = 33); B % 32 = 1; bias[0] NULL; dx0 NULL
  b32     B = 32, (45, 70, 33): both halves of one 32-row step owned (B % 32 = 0)
  rot     B = 277 = 16 * 17 + 5, (257, 512, 400): 9 k steps (a second group of TW_PF
          whose padded steps load from past the image), N = 512 four tiles per wave,
          a 16-step layer in both directions under every rotation blockIdx % 16, the
          last block partly dead; ns = 64
  k256    B = 48, (256, 512, 64): exactly TW_PF = 8 k steps, one group; K = 512
  deep    B = 77, (16, 64, 48, 32, 17): L = 4 with unequal widths (the ping-pong
          gradient blocks, s_g = stride(wmax)); z NULL in BCE mode
  c2      B = 48, (429, 400, 400, 400): the C2 tower (13-column last k step)
  x16     d = 16, C = 3, MLP (48, 32, 17), B = 40 (one dz magnitude, 2 / 4 non-zeros
          a cross / MLP row: three cross layers multiply the magnitudes)
  x45     d = 45, C = 2, MLP (70, 33), B = 77; a cross bias NULL
  x100    d = 100, C = 1, MLP (64,), B = 17
  x429    d = 429, C = 3, MLP (400, 400), B = 48 (one dz magnitude, 1 / 6 non-zeros
          a cross / MLP row plus the planted ones)
  dw*     (63, 64, 65, 63) at B = 17 / 77 / 277 / 520: n_out and n_in + 1 of
          mrec_tower_dw at the 64-tile edges (63 / 64 / 65 with n_in = 63 and 64)
  s520, s100  (45, 70, 33) through dense.score_tower: mrec_tower_dw at B = 520, the
          layered weight-gradient path at B = 100
  e520, e100  the same through dense.tower_bce, at B = 520 behind two cross layers
  (512 x 5 with one cross layer needs more than 160 KiB of LDS: the library's error)

Sections: 1 the generator, the restatement and their CPU checks; 2 raw
mrec_tower_fwd_bwd in guarded buffers (FORWARD, GIVEN_DZ, BCE; row-major and
k-fragment outputs); 3 mrec_tower_dw on the tower's own images + the REDUCE job and
the head finish; 4 dense.score_tower / dense.tower_bce on exact-integer modules.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ref
from test_gpu_dense import _kfrag_np
from test_gpu_gemm_matrix import _Guarded, _Job, _multi, _r8, _tower_elems, _vec1, _ws_bytes

gpu_test = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT = 7.0
NAN = float("nan")
Q = 2.0 ** -10  # the backward's quantum: the smallest |dz|
BCE, FORWARD, GIVEN_DZ = 0, 1, 2
REDUCE = 2


def _ceil(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# 1. the case matrix, the generator, the fp64 restatement
# ---------------------------------------------------------------------------

class Case:
    """widths = (K0, N1..NL); C cross layers of width K0; ``nnz`` / ``cnnz`` non-zeros
    per MLP / cross weight row; ``mags``: the dz magnitudes in units of 2^-10;
    ``null``: the optional pointers this case passes as NULL; ``logit0``: base
    cancels the rest of the logit and soft labels give the BCE mode the case's dz."""

    def __init__(self, name, widths, B, seed, C=0, nnz=8, cnnz=4, ns=5, mags=(1, 2), null=(),
                 logit0=False):
        self.name, self.widths, self.B, self.seed, self.C = name, tuple(widths), B, seed, C
        self.nnz, self.cnnz, self.ns, self.mags, self.null = nnz, cnnz, ns, mags, frozenset(null)
        self.L, self.logit0 = len(widths) - 1, logit0

    def __repr__(self):
        return self.name


CASES = [
    Case("b1", (7, 17), 1, 0, ns=0),
    Case("b15", (8, 16, 1), 15, 2, ns=1, null=("base",)),
    Case("b16", (1, 128, 129), 16, 6, null=("head_b",)),
    Case("b17", (33, 400, 64), 17, 1, nnz=12, null=("b2", "h_out")),
    Case("b33", (32, 48, 33), 33, 0, null=("bias0", "dx0")),
    Case("b32", (45, 70, 33), 32, 0),
    Case("rot", (257, 512, 400), 277, 1, ns=64),
    Case("k256", (256, 512, 64), 48, 1),
    Case("deep", (16, 64, 48, 32, 17), 77, 0, null=("z",)),
    Case("c2", (429, 400, 400, 400), 48, 0),
    Case("x16", (16, 48, 32, 17), 40, 0, C=3, nnz=4, cnnz=2, mags=(1,)),
    Case("x45", (45, 70, 33), 77, 0, C=2, null=("cbias1",)),
    Case("x100", (100, 64), 17, 12, C=1),
    Case("x429", (429, 400, 400), 48, 5, C=3, nnz=6, cnnz=1, mags=(1,)),
]
DW_CASES = [Case(f"dw{B}", (63, 64, 65, 63), B, seed)
            for B, seed in ((17, 7), (77, 0), (277, 1), (520, 0))]
# the wrappers' cases: scores (no base / side term), and BCE with z = 0 and soft labels
SCORE_CASES = [Case(f"s{B}", (45, 70, 33), B, seed, ns=0, null=("base", "b2"))
               for B, seed in ((520, 3), (100, 1))]
BCE_CASES = [Case("e520", (45, 70, 33), 520, 6, C=2, mags=(1,), logit0=True),
             Case("e100", (45, 70, 33), 100, 1, mags=(1,), logit0=True)]
ALL_CASES = CASES + DW_CASES + SCORE_CASES + BCE_CASES
BY_NAME = {c.name: c for c in ALL_CASES}


def _ids(cases):
    return [c.name for c in cases]


def _sparse_weight(rng, N, K, nnz):
    """[N, K] with entries +-1: ``nnz`` per row, then one more in every 16 x 32 block
    (forward blocking: 16 n x 32 k; backward blocking: 16 k x 32 n) still empty."""
    W = np.zeros((N, K))
    for n in range(N):
        cols = rng.choice(K, size=min(nnz, K), replace=False)
        W[n, cols] = rng.choice([-1.0, 1.0], size=cols.size)
    for (bn, bk) in ((16, 32), (32, 16)):
        for n0 in range(0, N, bn):
            for k0 in range(0, K, bk):
                blk = W[n0:n0 + bn, k0:k0 + bk]
                if not blk.any():
                    blk[rng.integers(blk.shape[0]), rng.integers(blk.shape[1])] = rng.choice([-1.0, 1.0])
    return W


def _generate(case):
    """The exact-integer inputs of ``case`` (fp64 numpy), without the conditions."""
    rng = np.random.default_rng([case.seed, case.B, case.C] + list(case.widths))
    B, L, ns, K0 = case.B, case.L, case.ns, case.widths[0]
    inp = SimpleNamespace(case=case)
    inp.x0 = rng.choice([-1.0, 0.0, 1.0], size=(B, K0), p=[0.4, 0.2, 0.4])
    inp.cross = []
    for c in range(case.C):
        b = np.zeros(K0) if f"cbias{c}" in case.null else rng.integers(-1, 2, K0).astype(np.float64)
        inp.cross.append((_sparse_weight(rng, K0, K0, case.cnnz), b))
    inp.layers = []
    for l in range(L):
        N, K = case.widths[l + 1], case.widths[l]
        b = np.zeros(N) if f"bias{l}" in case.null else rng.integers(-1, 3, N).astype(np.float64)
        inp.layers.append((_sparse_weight(rng, N, K, case.nnz), b))
    H = case.widths[L]
    inp.head_w = rng.choice([-2.0, -1.0, 1.0, 2.0], size=H)
    inp.head_b = 0.0 if "head_b" in case.null else float(rng.integers(-3, 4))
    inp.b2 = 0.0 if "b2" in case.null else float(rng.integers(-3, 4))
    inp.xs = rng.integers(-3, 4, (B, ns)).astype(np.float64)
    inp.ws = rng.integers(-2, 3, ns).astype(np.float64)
    inp.base = np.zeros(B)
    if "base" not in case.null:  # brings the logits into [-4, 4]: the BCE mode's dz stays alive
        inp.base = (0 if case.logit0 else rng.integers(-4, 5, B)) - _restate(inp, np.zeros(B)).z
    inp.dz = rng.choice([-1.0, 1.0], size=B) * rng.choice(np.array(case.mags, np.float64), size=B) * Q
    inp.y = (rng.random(B) < 0.4).astype(np.float64)
    if case.logit0:
        inp.y_soft = _soft_labels(inp.dz, B)
    return inp


def _soft_labels(dz, B):
    """fp32 labels y with (1/2 - y) / B == dz exactly in fp32, whether the division is
    done as such or as a product with fp32(1 / B), and 1/2 - y itself exact."""
    y = np.zeros(dz.size, np.float32)
    half, fB = np.float32(0.5), np.float32(B)
    for v in np.unique(dz):
        # the fp32 neighbours of 1/2 - B dz, nearest first
        cand = np.float32(0.5 - B * v) + np.arange(-64, 65, dtype=np.float32) * np.float32(2.0 ** -24)
        cand = cand[np.argsort(np.abs(np.arange(-64, 65)), kind="stable")]
        t = half - cand
        ok = (t * (np.float32(1.0) / fB) == np.float32(v)) & (t / fB == np.float32(v)) & \
            (t.astype(np.float64) == 0.5 - cand.astype(np.float64))
        assert ok.any(), f"no fp32 label gives dz = {v} at B = {B}"
        y[dz == v] = cand[ok][0]
    return y


def _restate(inp, dz=None):
    """include/mrec.h's contract of mrec_tower_fwd_bwd / mrec_tower_dw in fp64."""
    dz = inp.dz if dz is None else dz
    x0, hw, xs = inp.x0, inp.head_w, inp.xs
    B, L, C = x0.shape[0], len(inp.layers), len(inp.cross)
    r = SimpleNamespace()
    # x_0 = x0; z_c = x_c Wc_c^T + bc_c; x_{c+1} = x0 * z_c + x_c
    r.xc, r.zc = [x0], []
    for W, b in inp.cross:
        r.zc.append(r.xc[-1] @ W.T + b)
        r.xc.append(x0 * r.zc[-1] + r.xc[-1])
    # h_l = relu(h_{l-1} W_l^T + b_l), h_0 = x_C
    r.h = [r.xc[-1]]
    for W, b in inp.layers:
        r.h.append(np.maximum(r.h[-1] @ W.T + b, 0.0))
    r.z = r.h[L] @ hw + inp.head_b + inp.base + xs @ inp.ws + inp.b2
    # dh_L = dz head_w [h_L > 0]; dh_{l-1} = (dh_l W_l) [h_{l-1} > 0]; dx0 = dh_1 W_1
    r.dh = [None] * (L + 1)
    r.dh[L] = dz[:, None] * hw[None, :] * (r.h[L] > 0)
    for l in range(L, 1, -1):
        r.dh[l - 1] = (r.dh[l] @ inp.layers[l - 1][0]) * (r.h[l - 1] > 0)
    # G_C = the MLP's input gradient; dz_c = G_{c+1} x0; G_c = dz_c Wc_c + G_{c+1};
    # dx0 = G_0 + sum_c G_{c+1} z_c
    r.G = [None] * (C + 1)
    r.G[C] = r.dh[1] @ inp.layers[0][0]
    r.dzc = [None] * C
    for c in range(C - 1, -1, -1):
        r.dzc[c] = r.G[c + 1] * x0
        r.G[c] = r.dzc[c] @ inp.cross[c][0] + r.G[c + 1]
    r.dx0 = r.G[0] + sum((r.G[c + 1] * r.zc[c] for c in range(C)), np.zeros_like(x0))
    # head partials per 16 rows: [sum dz h_L | sum dz | sum dz xs]
    H, ns = hw.size, xs.shape[1]
    r.part = np.zeros((_ceil(B, 16), H + 1 + ns))
    for i in range(r.part.shape[0]):
        rows = slice(16 * i, 16 * i + 16)
        r.part[i, :H] = dz[rows] @ r.h[L][rows]
        r.part[i, H] = dz[rows].sum()
        r.part[i, H + 1:] = dz[rows] @ xs[rows]
    # dW_l = dY^T [X | 1]
    r.dW = [r.dh[l].T @ r.h[l - 1] for l in range(1, L + 1)]
    r.db = [r.dh[l].sum(0) for l in range(1, L + 1)]
    r.cdW = [r.dzc[c].T @ r.xc[c] for c in range(C)]
    r.cdb = [r.dzc[c].sum(0) for c in range(C)]
    r.dW_head, r.db_head, r.dws = r.h[L].T @ dz, dz.sum(), xs.T @ dz
    return r


def _outputs(r):
    """every expected output of a restatement, by name"""
    out = {"z": r.z, "dx0": r.dx0, "part": r.part, "dW_head": r.dW_head, "dws": r.dws}
    for name in ("xc", "zc", "h", "dh", "dzc", "dW", "db", "cdW", "cdb"):
        for i, v in enumerate(getattr(r, name)):
            if v is not None:
                out[f"{name}{i}"] = v
    return out


def _is_bf16(v):
    v = np.asarray(v, np.float64)
    return np.array_equal(ref.bf16_round(v.astype(np.float32)).astype(np.float64), v)


def _block_products_nonzero(X, W):
    """X [B, K] (B live rows), W [N, K]: for every 16-row block of X, every 16-row
    tile of W and every 32-wide k step, is X_blk W_tile^T (over that step) non-zero
    somewhere?"""
    B, K = X.shape
    N = W.shape[0]
    nb, nt = _ceil(B, 16), _ceil(N, 16)
    for k0 in range(0, K, 32):
        P = np.zeros((nb * 16, nt * 16))
        P[:B, :N] = X[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T
        if not (P.reshape(nb, 16, nt, 16) != 0).any(axis=(1, 3)).all():
            return False
    return True


def _blocks_planted(W):
    N, K = W.shape
    return all(W[n0:n0 + bn, k0:k0 + bk].any() for bn, bk in ((16, 32), (32, 16))
               for n0 in range(0, N, bn) for k0 in range(0, K, bk))


def _conditions(inp, r, dz=None):
    """The three conditions; returns the first one violated (None: all hold)."""
    dz = inp.dz if dz is None else dz
    L, C = len(inp.layers), len(inp.cross)
    q = np.abs(dz).min()
    # --- representable ---
    stored = {"x0": inp.x0, "dx0": r.dx0}
    for name, vals in (("x", r.xc), ("z_c", r.zc), ("h", r.h), ("dh", r.dh[1:]), ("G", r.G),
                       ("dz_c", r.dzc)):
        stored.update({f"{name}{i}": v for i, v in enumerate(vals)})
    for name, v in stored.items():
        if not _is_bf16(v):
            return f"{name} is not representable in bf16"
    if q <= 0 or not np.array_equal(np.round(dz / q), dz / q):
        return "a live row has dz == 0, or dz is no multiple of its smallest magnitude"
    # --- order independent: sum|terms| < 2^24 quanta ---
    a = np.abs
    sums = {"head dot": a(r.h[L]) @ a(inp.head_w) + abs(inp.head_b) + a(inp.base)
            + a(inp.xs) @ a(inp.ws) + abs(inp.b2),
            "partials": np.concatenate([a(dz) @ a(r.h[L]), [a(dz).sum()], a(dz) @ a(inp.xs)]) / q,
            "dx_C": a(r.dh[1]) @ a(inp.layers[0][0]) / q}
    for l in range(1, L + 1):
        W, b = inp.layers[l - 1]
        sums[f"h{l}"] = a(r.h[l - 1]) @ a(W).T + a(b)
        sums[f"dW{l}"] = a(r.dh[l]).T @ np.hstack([a(r.h[l - 1]), np.ones((dz.size, 1))]) / q
        if l > 1:
            sums[f"dh{l - 1}"] = a(r.dh[l]) @ a(W) / q
    acc = np.zeros_like(inp.x0)
    for c in range(C):
        W, b = inp.cross[c]
        sums[f"z_c{c}"] = a(r.xc[c]) @ a(W).T + a(b)
        sums[f"x{c + 1}"] = a(inp.x0 * r.zc[c]) + a(r.xc[c])
        sums[f"G{c}"] = (a(r.dzc[c]) @ a(W) + a(r.G[c + 1])) / q
        sums[f"cdW{c}"] = a(r.dzc[c]).T @ np.hstack([a(r.xc[c]), np.ones((dz.size, 1))]) / q
        acc += a(r.G[c + 1] * r.zc[c])
    if C:
        sums["dx0"] = (sums["G0"] + acc / q)
    for name, v in sums.items():
        if np.max(v) >= 2.0 ** 24:
            return f"{name}: sum|terms| reaches {np.max(v)} quanta"
    # --- sensitive ---
    for l in range(1, L + 1):
        W = inp.layers[l - 1][0]
        frac = (r.h[l] > 0).mean()
        if not 0.25 <= frac <= 0.75:
            return f"ReLU {l} is active on {frac:.2f} of its elements"
        if not _blocks_planted(W):
            return f"W{l} has an empty 16 x 32 block"
        if not _block_products_nonzero(r.h[l - 1], W):
            return f"forward layer {l}: a 16 x 16 partial product is zero"
        if not _block_products_nonzero(r.dh[l], W.T):
            return f"backward layer {l}: a 16 x 16 partial product is zero"
    for c in range(C):
        W = inp.cross[c][0]
        if not _blocks_planted(W):
            return f"Wc{c} has an empty 16 x 32 block"
        if not _block_products_nonzero(r.xc[c], W):
            return f"cross forward layer {c}: a 16 x 16 partial product is zero"
        if not _block_products_nonzero(r.dzc[c], W.T):
            return f"cross backward layer {c}: a 16 x 16 partial product is zero"
    return None


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, restatement) of a case, computed once and shared; the generator
    asserts the conditions"""
    inp = _generate(BY_NAME[name])
    r = _restate(inp)
    bad = _conditions(inp, r)
    assert bad is None, f"case {name}: {bad}"
    return inp, r


MUTATIONS = 48  # weight blocks zeroed per case (all of them where a case has fewer)


def _unseen_mutation(inp, r):
    """Zero single 16 x 32 blocks of a weight (forward blocking, and 32 x 16: the
    backward's) in the restatement -- every block of a small case, a fixed sample of
    ``MUTATIONS`` of a larger one -- and return the first that changes no expected
    output (None: each changes one)."""
    want = _outputs(r)
    blocks = []
    for kind, ws in (("layers", inp.layers), ("cross", inp.cross)):
        for i, (W, _) in enumerate(ws):
            for bn, bk in ((16, 32), (32, 16)):
                blocks += [(kind, i, n0, bn, k0, bk) for n0 in range(0, W.shape[0], bn)
                           for k0 in range(0, W.shape[1], bk)]
    if len(blocks) > MUTATIONS:
        pick = np.random.default_rng(inp.case.seed).choice(len(blocks), MUTATIONS, replace=False)
        blocks = [blocks[i] for i in sorted(pick)]
    for blk in blocks:
        kind, i, n0, bn, k0, bk = blk
        ws = getattr(inp, kind)
        W, b = ws[i]
        Wm = W.copy()
        Wm[n0:n0 + bn, k0:k0 + bk] = 0.0
        ws[i] = (Wm, b)
        try:
            got = _outputs(_restate(inp))
        finally:
            ws[i] = (W, b)
        if all(np.array_equal(got[k], want[k]) for k in want):
            return blk
    return None


def _search_seed(case, tries=400):
    """for whoever adds a case: the first seed whose inputs meet the conditions and
    the mutation self-check"""
    for seed in range(tries):
        case.seed = seed
        inp = _generate(case)
        r = _restate(inp)
        if _conditions(inp, r) is None and _unseen_mutation(inp, r) is None:
            return seed
    return None


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_case_conditions(case):
    """Every case's inputs are representable, order independent and sensitive (the
    generator's own assertion, and once more from here); the inputs are of the
    promised kind.  Runs without a GPU."""
    inp, r = _case(case.name)
    assert _conditions(inp, r) is None
    assert set(np.unique(inp.x0)) <= {-1.0, 0.0, 1.0}
    for W, b in inp.layers + inp.cross:
        assert set(np.unique(W)) <= {-1.0, 0.0, 1.0} and np.array_equal(b, np.round(b))
    assert set(np.unique(np.abs(inp.dz) / Q)) <= set(map(float, case.mags))
    for v in (inp.head_w, inp.base, inp.xs, inp.ws, np.array([inp.head_b, inp.b2])):
        assert np.array_equal(v, np.round(v))
    assert np.array_equal(r.z, np.round(r.z))
    if "base" not in case.null:  # the BCE mode's logits stay where sigmoid is not saturated
        assert np.abs(r.z).max() <= 4


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_restatement_equals_oracle(case):
    """The restatement against oracle/ref.py's mlp_fwd / mlp_bwd / dcn_cross_fwd /
    dcn_cross_bwd on the same inputs: nothing rounds, so plain equality."""
    inp, r = _case(case.name)
    L, C = len(inp.layers), len(inp.cross)
    xs, zs = ref.dcn_cross_fwd(inp.x0, inp.cross)
    acts = ref.mlp_fwd(xs[-1], inp.layers)
    for got, want in zip(r.xc + r.zc + r.h, xs + zs + acts):
        assert np.array_equal(got, want)
    z = acts[-1] @ inp.head_w + inp.head_b + inp.base + inp.xs @ inp.ws + inp.b2
    assert np.array_equal(r.z, z)
    dxc, lgr = ref.mlp_bwd(acts, inp.layers, inp.dz[:, None] * inp.head_w[None, :])
    dx0, cgr = ref.dcn_cross_bwd(xs, zs, inp.cross, dxc)
    assert np.array_equal(r.G[C], dxc) and np.array_equal(r.dx0, dx0)
    for l in range(L):
        assert np.array_equal(r.dW[l], lgr[l][0]) and np.array_equal(r.db[l], lgr[l][1])
    for c in range(C):
        assert np.array_equal(r.cdW[c], cgr[c][0]) and np.array_equal(r.cdb[c], cgr[c][1])
    assert np.array_equal(r.part.sum(0)[:inp.head_w.size], acts[-1].T @ inp.dz)
    assert np.array_equal(r.dW_head, acts[-1].T @ inp.dz) and r.db_head == inp.dz.sum()


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_mutation_changes_expectation(case):
    """Zeroing any single 16 x 32 block of a weight in the restatement changes at
    least one expected output (``_unseen_mutation``).  Runs without a GPU."""
    inp, r = _case(case.name)
    assert _unseen_mutation(inp, r) is None


# ---------------------------------------------------------------------------
# 2. raw mrec_tower_fwd_bwd in guarded buffers
# ---------------------------------------------------------------------------

def _t64(v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))


def _fvec(v, dev):
    """fp32 vector, NaN in front and behind"""
    return _vec1(_t64(v).reshape(-1), dev)


def _bits(v):
    """fp64 [rows, cols] (exact in bf16) -> the bf16 bits (int16 numpy)"""
    return _t64(v).to(BF16).view(torch.int16).numpy()


def _output(g, dev, live):
    """an output: the device copy starts as the sentinel everywhere, ``host`` is the
    expected image, ``live`` marks what holds computed values"""
    g.live = live
    g.dev = torch.full_like(g.host, SENT).to(dev)
    return g


def _rows_out(B, width, vals, dev):
    """row-major bf16 [B, round8(width) + 8] output with two more rows: live values
    ``vals`` (None: not known beforehand), pad columns zero, the rest sentinel"""
    g = _Guarded(B + 2, _r8(width) + 8, BF16, SENT)
    w = g.win()
    w[:B, width:_r8(width)] = 0
    live = torch.zeros(g.host.numel(), dtype=torch.bool)
    g.win(live)[:B, :width] = True
    if vals is not None:
        w[:B, :width] = _t64(vals).to(BF16)
    return _output(g, dev, live)


def _img_out(B, width, vals, dev):
    """k-fragment image of [B, width]: the numpy layout of ``vals`` over all
    mrec_kfrag_elems elements, zero wherever no live element lands"""
    g = _Guarded(1, _ceil(width, 16) * _ceil(B, 32) * 512, BF16, SENT)
    g.win().zero_()
    live = torch.zeros(g.host.numel(), dtype=torch.bool)
    g.win(live)[0] = torch.from_numpy(_kfrag_np(np.ones((B, width), np.int16)) != 0)
    if vals is not None:
        g.win()[0] = torch.from_numpy(_kfrag_np(_bits(vals))).view(BF16)
    return _output(g, dev, live)


def _f32_out(rows, ld, cols, vals, dev, written=True):
    """fp32 [rows, ld] output whose columns [0, cols) are written"""
    g = _Guarded(rows, ld, F32, SENT)
    live = torch.zeros(g.host.numel(), dtype=torch.bool)
    if written:
        g.win(live)[:, :cols] = True
        if vals is not None:
            g.win()[:, :cols] = _t64(vals).reshape(rows, cols).float()
    return _output(g, dev, live)


def _images(W, dev):
    """the fwd / bwd tower images of W by mrec_tower_weight_prep, NaN around them"""
    from pytorchrec_amd import _mrec
    N, K = W.shape
    src = torch.from_numpy(W.astype(np.float32)).contiguous().to(dev)
    imgs = [_Guarded(1, _tower_elems(N, K, bwd), BF16, NAN) for bwd in (0, 1)]
    for g in imgs:
        g.win().zero_()
        g.up(dev)
    _mrec.call("mrec_tower_weight_prep", src.data_ptr(), N, K, K, imgs[0].t.data_ptr(),
               imgs[1].t.data_ptr(), _mrec.stream_handle())
    return imgs


def _p(g):
    return None if g is None else g.t.data_ptr()


class _Launch:
    """one prepared mrec_tower_fwd_bwd call and its guarded outputs ``o``"""

    def __init__(self, args, o, keep):
        self.args, self.o, self.keep = args, o, keep

    def call(self):
        from pytorchrec_amd import _mrec
        _mrec.call("mrec_tower_fwd_bwd", ctypes.byref(self.args), _mrec.stream_handle())
        return self

    def adopt(self):
        """take the device's live values where the expectation is not known
        beforehand (the structure around them stays expected)"""
        for g in self.o.values():
            if g.adopt:
                got = g.dev.cpu()
                g.host[g.live] = got[g.live]

    def check(self):
        torch.cuda.synchronize()
        self.adopt()
        for name, g in self.o.items():
            g.check(name)


class _Tower:
    """a case on the device: guarded operands (uploaded once) and launches"""

    def __init__(self, dev, case, inp=None, r=None):
        self.dev, self.case = dev, case
        self.inp, self.r = _case(case.name) if inp is None else (inp, r)
        inp, B, K0, null = self.inp, case.B, case.widths[0], case.null
        self.x0 = _Guarded(B + 2, _r8(K0) + 8, BF16, NAN)
        w = self.x0.win()
        w[:B, :K0] = _t64(inp.x0).to(BF16)
        w[:B, K0:_r8(K0)] = 0
        self.x0.up(dev)
        self.imgs = [_images(W, dev) for W, _ in inp.layers]
        self.cimgs = [_images(W, dev) for W, _ in inp.cross]
        self.bias = [None if f"bias{l}" in null else _fvec(b, dev) for l, (_, b) in enumerate(inp.layers)]
        self.cbias = [None if f"cbias{c}" in null else _fvec(b, dev) for c, (_, b) in enumerate(inp.cross)]
        self.head_w = _fvec(inp.head_w, dev)
        self.head_b = None if "head_b" in null else _fvec([inp.head_b], dev)
        self.b2 = None if "b2" in null else _fvec([inp.b2], dev)
        self.base = None if "base" in null else _fvec(inp.base, dev)
        self.y, self.dz_in = _fvec(inp.y, dev), _fvec(inp.dz, dev)
        self.xs = self.ws = None
        if case.ns:
            self.xs = _Guarded(B + 1, case.ns + 3, F32, NAN)
            self.xs.win()[:B, :case.ns] = _t64(inp.xs).float()
            self.xs.up(dev)
            self.ws = _fvec(inp.ws, dev)

    def prepare(self, mode, kfrag=0, dz_in=None):
        """``dz_in``: a device fp32 [B] for GIVEN_DZ (None: the case's own, whose
        backward the restatement knows)."""
        from pytorchrec_amd import _mrec
        c, inp, r, dev = self.case, self.inp, self.r, self.dev
        B, L, C, W, ns = c.B, c.L, c.C, c.widths, c.ns
        fwd_only = mode == FORWARD
        know = mode == GIVEN_DZ and dz_in is None
        kfrag = 0 if fwd_only else kfrag

        def val(v):
            return v if know else None

        mk = _img_out if kfrag else _rows_out
        o = {}
        for l in range(L):
            o[f"dh{l}"] = mk(B, W[l + 1], val(r.dh[l + 1]), dev)
            if l < L - 1 and "h_out" not in c.null:
                o[f"h{l}"] = mk(B, W[l + 1], r.h[l + 1], dev)
        if "dx0" not in c.null:
            o["dx0"] = _rows_out(B, W[0], val(r.dx0), dev)
        if kfrag:
            o["x0_img"] = _img_out(B, W[0], inp.x0, dev)
            for cc in range(C):
                o[f"cx{cc}"] = _img_out(B, W[0], r.xc[cc + 1], dev)
                o[f"cdz{cc}"] = _img_out(B, W[0], val(r.dzc[cc]), dev)
        nparts, used = _ceil(B, 16), W[L] + 1 + ns
        assert nparts == int(_mrec.lib().mrec_ctr_head_parts(B))
        o["part"] = _f32_out(nparts, _r8(used) + 8, used, val(r.part), dev)
        if not (mode == BCE and "z" in c.null):
            o["z"] = _f32_out(1, B, B, r.z, dev, written=mode != GIVEN_DZ)
        o["dz"] = _f32_out(1, B, B, val(inp.dz), dev)
        o["loss_part"] = _f32_out(1, nparts, nparts, None, dev, written=mode == BCE)
        o["loss"] = _f32_out(1, 1, 1, None, dev, written=mode == BCE)
        for name, g in o.items():
            # the forward's outputs are exact in every mode; the backward's only under
            # the case's own dz; the loss never
            forward = name in ("z", "x0_img") or name[0] == "h" or name.startswith("cx")
            g.adopt = name in ("loss", "loss_part") or not (know or forward)
            if fwd_only and name != "z":
                g.host.fill_(SENT)  # FORWARD: nothing but z leaves
                g.adopt = False
        ticket = _Guarded(1, 1, torch.int32, 7)
        ticket.win().zero_()
        ticket.up(dev)
        ticket.adopt = False
        o["ticket"] = ticket

        a = _mrec.TowerArgs()
        a.batch, a.n_layers, a.kfrag, a.mode, a.n_cross = B, L, kfrag, mode, C
        for l in range(L + 1):
            a.width[l] = W[l]
        a.x0, a.ld_x0 = self.x0.t.data_ptr(), self.x0.ld
        for l in range(L):
            a.w_fwd[l], a.w_bwd[l] = _p(self.imgs[l][0]), _p(self.imgs[l][1])
            a.bias[l] = _p(self.bias[l])
            a.dh_out[l], a.ld_dh[l] = _p(o[f"dh{l}"]), 0 if kfrag else o[f"dh{l}"].ld
            if f"h{l}" in o:
                a.h_out[l], a.ld_h[l] = _p(o[f"h{l}"]), 0 if kfrag else o[f"h{l}"].ld
        for cc in range(C):
            a.cross_w_fwd[cc], a.cross_w_bwd[cc] = _p(self.cimgs[cc][0]), _p(self.cimgs[cc][1])
            a.cross_bias[cc] = _p(self.cbias[cc])
            if kfrag:
                a.cross_x_img[cc], a.cross_dz_img[cc] = _p(o[f"cx{cc}"]), _p(o[f"cdz{cc}"])
        a.head_w, a.head_b, a.base, a.b2 = _p(self.head_w), _p(self.head_b), _p(self.base), _p(self.b2)
        a.xs, a.ld_xs, a.ns, a.ws = _p(self.xs), self.xs.ld if ns else 0, ns, _p(self.ws)
        a.y = _p(self.y)
        if "dx0" in o:
            a.dx0, a.ld_dx0 = _p(o["dx0"]), o["dx0"].ld
        a.z, a.dz = _p(o.get("z")), _p(o["dz"])
        a.part, a.ldp = _p(o["part"]), o["part"].ld
        a.loss_part, a.ticket, a.loss = _p(o["loss_part"]), _p(ticket), _p(o["loss"])
        a.x0_img = _p(o.get("x0_img"))
        a.dz_in = _p(self.dz_in) if dz_in is None else dz_in.data_ptr()
        return _Launch(a, o, [dz_in])

    def launch(self, mode, kfrag=0, dz_in=None):
        return self.prepare(mode, kfrag, dz_in).call()


@functools.lru_cache(maxsize=None)
def _tower(name):
    return _Tower(torch.device("cuda:0"), BY_NAME[name])


@gpu_test
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_forward_scores_are_exact(gpu, case):
    """MREC_TOWER_FORWARD: z is bitwise the restatement's; no other output is
    touched (they are passed, and keep the sentinel)."""
    _tower(case.name).launch(FORWARD).check()


@gpu_test
@pytest.mark.parametrize("kfrag", [0, 1], ids=["rows", "kfrag"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_given_dz_backward_is_exact(gpu, case, kfrag):
    """MREC_TOWER_GIVEN_DZ: every dh_out[l], every h_out[l], dx0, dz and the head
    partials are bitwise the restatement's inside their guarded allocations (z is
    not written); with kfrag every image the tower writes (dh, h, x0 and the cross
    layers' x_{c+1} and dz_c) equals the numpy layout over all its elements, rows
    >= B and the unowned half of the last 32-row step zero over a sentinel prefill."""
    from pytorchrec_amd import _mrec
    t = _tower(case.name)
    run = t.launch(GIVEN_DZ, kfrag)
    if kfrag:
        for l in range(case.L):
            assert run.o[f"dh{l}"].ld == int(_mrec.lib().mrec_kfrag_elems(case.B, case.widths[l + 1]))
    run.check()


@gpu_test
@pytest.mark.parametrize("kfrag", [0, 1], ids=["rows", "kfrag"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_bce_mode_is_tied_to_the_exact_backward(gpu, case, kfrag):
    """MREC_TOWER_BCE: z, every h_out and the forward images bitwise; dz and the loss
    against fp64 (sigmoid(z) - y) / B and mean BCE within the layered head's bars
    (dz rtol 1e-5 atol 1e-9, loss rtol 1e-5 atol 1e-6); a GIVEN_DZ launch on the BCE
    launch's own dz reproduces every backward output bit for bit (same block index,
    rotation and code path: the backward verified exactly above); the ticket is zero
    afterwards; a second BCE launch gives bit-equal results.  Pads, dead rows and
    guards hold the expected image in all three."""
    inp, r = _case(case.name)
    t = _tower(case.name)
    a = t.launch(BCE, kfrag)
    torch.cuda.synchronize()
    want_loss, want_dz = ref.bce_with_logits(r.z, inp.y)
    torch.testing.assert_close(a.o["dz"].t[0].cpu().double(), _t64(want_dz), rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(a.o["loss"].t[0].cpu().double(), _t64([want_loss]), rtol=1e-5, atol=1e-6)
    a.check()
    b = t.launch(GIVEN_DZ, kfrag, dz_in=a.o["dz"].t[0])
    b.check()
    for name in b.o:
        if name not in ("z", "loss", "loss_part"):
            assert torch.equal(a.o[name].dev, b.o[name].dev), name
    again = t.launch(BCE, kfrag)
    again.check()
    for name in a.o:
        assert torch.equal(a.o[name].dev, again.o[name].dev), name


@gpu_test
def test_lds_plan_beyond_160_kib_is_an_error(gpu):
    """Four 512-wide layers on a 512-wide x0 with one cross layer need more than
    160 KiB of LDS: the library's error, no launch, no output touched."""
    from pytorchrec_amd import _mrec
    case = Case("lds", (512,) * 5, 16, 0, C=1)
    inp = _generate(case)
    run = _Tower(gpu, case, inp, _restate(inp)).prepare(GIVEN_DZ)
    with pytest.raises(_mrec.MrecError, match="LDS"):
        run.call()
    torch.cuda.synchronize()
    for name, g in run.o.items():
        if name != "ticket":
            assert torch.all(g.dev == SENT), name


# ---------------------------------------------------------------------------
# 3. mrec_tower_dw on the tower's own images, the REDUCE job, the head finish
# ---------------------------------------------------------------------------

def _check_nan(g, what):
    """``_Guarded.check`` for an allocation whose expected image holds NaN"""
    got, want = (torch.nan_to_num(x, nan=-12345.0) for x in (g.dev.cpu(), g.host))
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} elements differ"


def _head_finish(t, run, dev):
    """the head finish of the launch's partials: (job, guarded outputs with the
    exact dW_head, sum dz, dws, sum dz)"""
    from pytorchrec_amd import _mrec
    c, r = t.case, t.r
    H, ns = c.widths[-1], c.ns
    outs = {"dw": _f32_out(1, H, H, r.dW_head, dev), "db": _f32_out(1, 1, 1, [r.db_head], dev),
            "db2": _f32_out(1, 1, 1, [r.db_head], dev)}
    if ns:
        outs["dws"] = _f32_out(1, ns, ns, r.dws, dev)
    part = run.o["part"]
    job = _mrec.HeadFinishJob(_p(part), part.ld, c.B, H, ns, None, 0, 0.0, None, None, None, None,
                              _p(outs["dw"]), _p(outs["db"]), _p(outs.get("dws")), _p(outs["db2"]))
    return job, outs


DW_RUNS = [("dw17", 1, None), ("dw77", 2, None), ("dw277", 4, None), ("dw520", 4, "job"),
           ("dw520", 8, None), ("dw520", 1, None), ("x45", 2, "alone"), ("rot", 4, "job"),
           ("x429", 2, None), ("deep", 3, None)]


@gpu_test
@pytest.mark.parametrize("name,req,finish", DW_RUNS, ids=[f"{n}-s{s}-{f}" for n, s, f in DW_RUNS])
def test_tower_dw_weight_gradients_are_exact(gpu, name, req, finish):
    """The tower's own k-fragment images (no mrec_kfrag_pack) into mrec_tower_dw
    with NaN-filled slabs, then the generic REDUCE job: dW_l and db_l are bitwise
    dY^T X and sum dY for MLP and cross layers alike, pad columns zero, guards
    intact; one slice leaves the whole [dW | db | 0] in the slab.  ``splits`` is
    dense._eff_split's effective count.  ``finish``: the head partials reduced by a
    mrec_head_finish_job in the same launch, or by mrec_ctr_head_finish alone --
    exactly dW_head, sum dz and dws."""
    from pytorchrec_amd import _mrec, dense as D
    t = _tower(name)
    c, r, B = t.case, t.r, t.case.B
    run = t.launch(GIVEN_DZ, 1)
    run.check()
    o, C, L, W = run.o, c.C, c.L, c.widths
    lay = [(W[0], W[0], o[f"cdz{cc}"], o["x0_img"] if cc == 0 else o[f"cx{cc - 1}"], r.cdW[cc], r.cdb[cc])
           for cc in range(C)]
    lay += [(W[l + 1], W[l], o[f"dh{l}"], (o[f"cx{C - 1}"] if C else o["x0_img"]) if l == 0 else o[f"h{l - 1}"],
             r.dW[l], r.db[l]) for l in range(L)]
    splits = D._eff_split(B, req)
    a = _mrec.TowerDwArgs()
    a.n_layers, a.batch, a.splits = len(lay), B, splits
    slabs = []
    for i, (no, ni, dy, x, _, _) in enumerate(lay):
        ldws = _r8(ni + 1)
        if splits > 1:
            assert splits * no * ldws * 4 == int(_mrec.lib().mrec_gemm_workspace_size(no, ni, B, req)) \
                == _ws_bytes(no, ni, B, req)
        ws = _Guarded(splits * no, ldws, F32, NAN).up(gpu)
        slabs.append(ws)
        a.n_out[i], a.n_in[i], a.dy_img[i], a.x_img[i] = no, ni, _p(dy), _p(x)
        a.ws[i], a.ldws[i] = _p(ws), ldws
    fin = outs = None
    if finish:
        fin, outs = _head_finish(t, run, gpu)
    _mrec.call("mrec_tower_dw", ctypes.byref(a), ctypes.byref(fin) if finish == "job" else None,
               _mrec.stream_handle())
    if finish == "alone":
        _mrec.call("mrec_ctr_head_finish", fin.part, fin.ldp, fin.batch, fin.H, fin.ns, None, 0, 0.0,
                   None, None, None, None, fin.dw_out, fin.db_out, fin.dws_out, fin.db2_out,
                   _mrec.stream_handle())
    results, jobs = [], []
    for (no, ni, _, _, dW, db), ws in zip(lay, slabs):
        if splits == 1:  # the one slab is the result
            ws.win()[:, :ni] = _t64(dW).float()
            ws.win()[:, ni] = _t64(db).float()
            ws.win()[:, ni + 1:] = 0
            continue
        A = torch.full((B, _r8(no)), NAN, dtype=BF16, device=gpu)  # REDUCE reads no operand
        X = torch.full((B, _r8(ni)), NAN, dtype=BF16, device=gpu)
        Cg = _f32_out(no, _r8(ni) + 8, ni, dW, gpu)
        Cg.win()[:, ni:_r8(ni)] = 0
        dbg = _f32_out(1, no, no, db, gpu)
        results += [(Cg, "dW"), (dbg, "db")]
        jobs.append(_Job(no, ni, B, A, True, X, True, Cg.t, ones_out=dbg.t[0], split=req, ws=ws.t.reshape(-1)))
    for i in range(0, len(jobs), 4):
        _multi([j.call(REDUCE) for j in jobs[i:i + 4]])
    torch.cuda.synchronize()
    for ws in slabs:
        if splits > 1:  # every slab element was written, nothing around the slabs
            got = ws.win(ws.dev.cpu())
            assert not torch.isnan(got).any(), "a slab element was never written"
            ws.win().copy_(got)
        _check_nan(ws, "slabs")
    for g, what in results:
        g.check(what)
    for what, g in (outs or {}).items():
        g.check("head finish " + what)
    o["part"].check("part")


# ---------------------------------------------------------------------------
# 4. through the public wrappers
# ---------------------------------------------------------------------------

def _modules(inp, dev):
    """MLP, head and cross ``nn.Linear``s holding the generator's values"""
    from pytorchrec_amd.model.layer import MLP
    W = inp.case.widths
    mlp = MLP(W[0], list(W[1:]), "relu", 0.0).to(dev)
    head = torch.nn.Linear(W[-1], 1).to(dev)
    cross = [torch.nn.Linear(W[0], W[0]).to(dev) for _ in inp.cross]
    with torch.no_grad():
        for lin, (w, b) in zip([d.linear for d in mlp.mlp] + cross, inp.layers + inp.cross):
            lin.weight.copy_(_t64(w))
            lin.bias.copy_(_t64(b))
        head.weight.copy_(_t64(inp.head_w)[None, :])
        head.bias.fill_(inp.head_b)
    return mlp, head, cross


def _x0_rows(inp, dev):
    from pytorchrec_amd import dense as D
    B, K = inp.x0.shape
    x = torch.zeros(B, D._r8(K), dtype=BF16, device=dev)
    x[:, :K] = _t64(inp.x0).to(BF16).to(dev)
    return x[:, :K].detach().requires_grad_()


def _same(got, want, what):
    got = got.detach().cpu().double()
    assert torch.equal(got, _t64(want).reshape(got.shape)), what


def _check_param_grads(mlp, head, cross, r):
    lins = [d.linear for d in mlp.mlp]
    for i, lin in enumerate(lins):
        _same(lin.weight.grad, r.dW[i], f"dW{i}")
        _same(lin.bias.grad, r.db[i], f"db{i}")
    for i, lin in enumerate(cross):
        _same(lin.weight.grad, r.cdW[i], f"cross dW{i}")
        _same(lin.bias.grad, r.cdb[i], f"cross db{i}")
    _same(head.weight.grad, r.dW_head, "dW_head")
    _same(head.bias.grad, [r.db_head], "db_head")


@gpu_test
@pytest.mark.parametrize("case", SCORE_CASES, ids=_ids(SCORE_CASES))
def test_score_tower_wrapper_is_exact(gpu, case):
    """dense.score_tower on exact-integer modules: the scores, x0.grad and every
    weight.grad / bias.grad, head included, are bitwise the restatement's.  B = 520
    takes mrec_tower_dw (``_tdw_splits``), B = 100 the layered weight-gradient path:
    the buffer reuse of ``_tower_buffers``, the image cache and
    ``_tower_param_grads``, which the raw cases cannot see."""
    from pytorchrec_amd import dense as D
    inp, r = _case(case.name)
    assert bool(D._tdw_splits(case.B, list(case.widths))) == (case.B == 520)
    mlp, head, _ = _modules(inp, gpu)
    xg = _x0_rows(inp, gpu)
    assert D.tower_supported(xg, mlp, head)
    s = D.score_tower(xg, mlp, head)
    s.backward(_t64(inp.dz).float().to(gpu).reshape(s.shape))
    torch.cuda.synchronize()
    _same(s, r.z, "scores")
    _same(xg.grad, r.dx0, "x0.grad")
    _check_param_grads(mlp, head, [], r)


@gpu_test
@pytest.mark.parametrize("case", BCE_CASES, ids=_ids(BCE_CASES))
def test_tower_bce_wrapper_is_exact(gpu, case):
    """dense.tower_bce(..., cross=...) on exact-integer modules.  ``base`` cancels
    the rest of the logit (z = 0: sigmoid(z) = 1/2 exactly) and the labels are the
    generator's soft labels, so the launch's own dz = (1/2 - y) / B is +-2^-10 and the
    method carries through the BCE mode: the loss within rtol 1e-5 / atol 1e-6 of the
    fp64 mean BCE, every gradient bitwise the restatement's recomputed from the
    launch's own dz (read back through the ``base`` gradient; the conditions are
    asserted on it).  B = 520 (mrec_tower_dw; with cross layers) and B = 100 (the
    layered weight-gradient path)."""
    from pytorchrec_amd import dense as D
    inp, r = _case(case.name)
    assert not r.z.any()
    mlp, head, cross = _modules(inp, gpu)
    xg = _x0_rows(inp, gpu)
    assert D.tower_supported(xg, mlp, head, cross=cross or None)
    base = _t64(inp.base).float().to(gpu).requires_grad_()
    y = torch.from_numpy(inp.y_soft).to(gpu)
    xs = _t64(inp.xs).float().to(gpu)
    ws = _t64(inp.ws).float().to(gpu).requires_grad_()
    b2 = torch.full((1,), inp.b2, device=gpu).requires_grad_()
    loss = D.tower_bce(xg, mlp, head, base, y, xs=xs, ws=ws, b2=b2, cross=cross or None)
    loss.backward()
    torch.cuda.synchronize()
    want_loss, _ = ref.bce_with_logits(r.z, inp.y_soft.astype(np.float64))
    torch.testing.assert_close(loss.detach().cpu().double().reshape(1), _t64([want_loss]),
                               rtol=1e-5, atol=1e-6)
    dz = base.grad.cpu().double().numpy()
    r = _restate(inp, dz)
    assert _conditions(inp, r, dz) is None, _conditions(inp, r, dz)
    _same(xg.grad, r.dx0, "x0.grad")
    _check_param_grads(mlp, head, cross, r)
    _same(ws.grad, r.dws, "dws")
    _same(b2.grad, [r.db_head], "db2")
