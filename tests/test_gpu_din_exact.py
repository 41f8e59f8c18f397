"""The fused DIN attention unit (csrc/din_att.hip: mrec_din_att_fwd, mrec_din_att_bwd,
mrec_din_att_wgrad) pinned to exact expectations at its edges, against a plain fp64
restatement of include/mrec.h's contract.

Exact method.  q and k hold -1 / 0 / 1, W1 and W2 are sparse with entries +-1, b1, b2
and b3 are small integers and w3 is sparse with entries +-128.  Then X = [q | k | q - k
| q k], H1 and H2 are small integers and every score is b3 + 128 n.  Validity is the
contract's (his > 0 or j == 0).  Within a sample the valid positions at the maximum
score (the winners) tie exactly, every other valid score is at least 128 below:
__expf(s_j - m) is __expf(0) = 1 on a winner and 0 on a loser (128 > 150 ln 2 = 104,
below which fp32 has nothing but 0), so with 2^m winners a_j = 2^-m on them and
exactly 0 elsewhere, and the pooled u is a small multiple of 2^-m.  The generator masks
surplus winners (his = 0 at positions j > 0) down to a power of two, and by choosing
which winners it keeps it places the last non-zero a_j where a case needs it (the
backward's nv / act / kk0 / kk1 control flow hangs on that position).  Ties are natural
ones between different rows (planted copies would cancel dW2 and most of dW1).
In the backward g_j = du . k_j is an integer, ds_j = a_j (g_j - sum a_i g_i) a multiple
of 2^-2m and exactly 0 on every loser, sum_j ds_j = 0 exactly (db3 is bitwise zero).
The E columns are split into score columns S and value columns V: W1 is zero on the V
columns of its k, q - k and q k blocks and du is non-zero only on V, so that a_j du
(2^-m) and the MLP's part of dk (multiples of 128 2^-2m) never share a bf16 significand;
every case runs with S and V swapped as well, so every W1 column is non-zero somewhere.
The expectation is fp64 numpy and every GPU comparison is ``torch.equal``: this file has
no tolerance.

Conditions on the inputs (not measurements; ``test_case_conditions`` and
``test_matrix_is_sensitive`` check them on the CPU):

  * exact softmax: per sample the winners number 2^m, every other valid score is at
    least 128 below;
  * representable: X, H1, H2, u, dZ2, dZ1, dX and d_rows survive a bf16 round trip (H2
    and dX because the layered path rounds them, and for the same reason ds wherever
    w3 != 0);
  * order independent: for every fp32 accumulation (layer sums, score parts, pooled
    sum, g, sum a g, dX, the dq parts, dW1 / dW2 over rows and samples, the column
    partials, the partial sums) sum|terms| < 2^24 quanta, 1 in the forward and
    2^-2m (m the case's largest: no larger than its smallest |ds|) in the backward;
  * sensitive: over a shape family's cases every 16 x 16 tile of dW1 / dW2 and every
    16-column tile of db1 / db2 / dw3 has a non-zero expected element (but db2 and dw3
    at H2 = 1: the winners of a sample then share their one H2 value, so both are
    sums of ds alone, exactly zero); each ReLU is
    active on 25-75 % of its elements; at least 30 % of the samples have ds != 0
    (L = 1 has none: one position, a = 1, ds = 0); over the matrix the last position
    with a_j != 0 takes each of 1, 16, 17, 32, 33, 48, 49, 64 and the winner counts
    1, 2, 4, 8 all occur.  ``test_mutation_changes_expectation`` zeroes single
    16 x 32 blocks of W1 / W2, the k row of a winner, and unmasks a masked winner.

What each case is there for (G = mrec_din_att_parts(1 << 20), the workgroup count;
every family case also runs with S / V swapped, suffix ``s``):

  c4      (32, 80, 40) B = 64 L = 64: config C4's shape, every nv edge up to 64, one
          and two k steps of the dW accumulation (kk0)
  e68     (32, 68, 33) B = 40 L = 50: the smallest H1 / H2 of the family: one live
          column in the last H2 tile and in its k step
  e48     (32, 80, 48) B = 40 L = 64: the largest H2 of the family
  s24     (16, 24, 12) B = 64 L = 37: the small family, L no multiple of 16
  s20     (16, 20, 1) B = 40 L = 33: H2 = 1, the smallest H1
  s32     (16, 32, 16) B = 40 L = 17: the family's full tiles; one row in tile 1
  l1      L = 1, B = 37: one position (a = 1, ds = 0, dk = du); slot 1 idle everywhere
  l16     L = 16, B = 9: one whole row tile; a wave's second sample (B = 9) -- with b7
          and b8 the wave forward's batch edges 7, 8, 9
  b1      B = 1: one workgroup, slot 1 idle, one partial row
  b37     B = 37: slot 1 idle everywhere (as in every case with B <= G)
  bG+1    B = G + 1: one workgroup with both slots
  bG+9    B = G + 9 at L = 64 (sG+9: the small family): slot 1 with all four row tiles
          and two k steps (kk1), workgroups whose two slots differ in their k steps
          both ways; the other batches above G keep L <= 17
  b2G     B = 2G: every workgroup with both slots, one pair
  b2G+1   B = 2G + 1: one workgroup runs a second pair with slot 1 idle; its dq tail
          written inside the loop and once after it; the workgroup forward's 2G + 1
  b4G+3   B = 4G + 3: two pairs everywhere, three workgroups a third
  b8G+1   B = 8G + 1 (forward only): a wave's second sample in the wave forward
  t64     w3 = 0, L = 64, sample b has 2^(b % 7) valid positions (tails and holes):
          a = 1 / n, u the exact mean, dw3 != 0, dW1 = dW2 = db1 = db2 = 0, dk = a du
  tfull   w3 = 0, L = 16, every position of the batch valid

Sections: 1 the generator, the restatement and their CPU checks; 2 raw mrec_din_att_fwd
(both kernels) in guarded buffers; 3 raw mrec_din_att_bwd + mrec_din_att_wgrad; 4
dense.din_attention_top_rows on exact-integer modules; 5 device mutation evidence; 6 the
layered kernels of din.hip (feature builder and pooling, each way) on inputs of the same kind.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ref
from test_gpu_gemm_matrix import _Guarded, _vec1

gpu_test = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
SENT = 7.0
NAN = float("nan")
W3 = 128.0
NV_EDGES = (1, 16, 17, 32, 33, 48, 49, 64)


def _ceil(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def _G():
    """the backward's workgroup count: never hard-coded"""
    from pytorchrec_amd import _mrec
    return int(_mrec.lib().mrec_din_att_parts(1 << 20))


def _parts(B):
    from pytorchrec_amd import _mrec
    return int(_mrec.lib().mrec_din_att_parts(B))


# ---------------------------------------------------------------------------
# 1. the case matrix, the generator, the fp64 restatement
# ---------------------------------------------------------------------------

class Case:
    """shape = (E, H1, H2); B = bmul * G + badd; ``swap``: S / V swapped; ``tied``:
    w3 = 0 (None / "pow2" / "full"); ``nw3``: non-zeros of w3 (fewer: more ties; the
    short-L batch edges take 2); ``fwd_only``: a batch
    only the forward runs."""

    def __init__(self, name, shape, B, L, seed=0, swap=False, tied=None, nw3=4, fwd_only=False):
        self.name, self.shape, self.L, self.seed, self.swap = name, tuple(shape), L, seed, swap
        self.bmul, self.badd = B if isinstance(B, tuple) else (0, B)
        self.tied, self.nw3, self.fwd_only = tied, nw3, fwd_only

    @property
    def B(self):
        return self.bmul * _G() + self.badd

    def __repr__(self):
        return self.name


C4, E68, E48, S24, S20, S32 = (32, 80, 40), (32, 68, 33), (32, 80, 48), (16, 24, 12), (16, 20, 1), (16, 32, 16)
FAMILIES = {"c4": (C4, 64, 64), "e68": (E68, 40, 50), "e48": (E48, 40, 64),
            "s24": (S24, 64, 37), "s20": (S20, 40, 33), "s32": (S32, 40, 17)}
# found with _search_seed (the batches given in G at G = 256, the MI355X's)
SEEDS = {"c4": 2, "c4s": 4, "e68": 46, "e68s": 9, "e48": 5, "e48s": 6, "s24": 0, "s24s": 0, "s20": 1,
         "s20s": 3, "s32": 0, "s32s": 0, "l1": 0, "l16": 0, "b7": 9, "b8": 16, "b1": 22, "b37": 4,
         "bG+1": 0, "bG+9": 122, "sG+9": 4,
         "b2G": 34, "b2G+1": 66, "b4G+3": 6, "t64": 0, "t64s": 0, "tfull": 0, "b8G+1": 0}


def _mk(name, shape, B, L, **kw):
    return Case(name, shape, B, L, seed=SEEDS.get(name, 0), **kw)


FAMILY_CASES = [_mk(n + sfx, sh, B, L, swap=bool(sfx), nw3=4)
                for n, (sh, B, L) in FAMILIES.items() for sfx in ("", "s")]
EDGE_CASES = [
    _mk("l1", C4, 37, 1),
    _mk("l16", S24, 9, 16, nw3=2),
    _mk("b7", S24, 7, 17, nw3=2),
    _mk("b8", C4, 8, 33),
    _mk("b1", C4, 1, 64),
    _mk("b37", E48, 37, 50, swap=True),
    _mk("bG+1", S24, (1, 1), 17, nw3=2),
    _mk("bG+9", C4, (1, 9), 64, swap=True),
    _mk("sG+9", S24, (1, 9), 64),
    _mk("b2G", C4, (2, 0), 17, nw3=2),
    _mk("b2G+1", C4, (2, 1), 17, swap=True, nw3=2),
    _mk("b4G+3", S24, (4, 3), 16, nw3=2),
    _mk("t64", C4, 70, 64, tied="pow2"),
    _mk("t64s", S24, 35, 64, tied="pow2", swap=True),
    _mk("tfull", S32, 19, 16, tied="full"),
]
FWD_ONLY_CASES = [_mk("b8G+1", S24, (8, 1), 3, fwd_only=True)]
BWD_CASES = FAMILY_CASES + EDGE_CASES
ALL_CASES = BWD_CASES + FWD_ONLY_CASES
BY_NAME = {c.name: c for c in ALL_CASES}


def _ids(cases):
    return [c.name for c in cases]


def _family(case):
    return case.shape


def _sv(case):
    """(score columns, value columns) of the E embedding columns"""
    E = case.shape[0]
    lo, hi = np.arange(E // 2), np.arange(E // 2, E)
    return (hi, lo) if case.swap else (lo, hi)


def _sparse_rows(rng, N, cols, width, nnz):
    """[N, width] with entries +-1: ``nnz`` per row among ``cols``, then one more in
    every 16 x 32 block that has an allowed column and is still empty"""
    W = np.zeros((N, width))
    for n in range(N):
        c = rng.choice(cols, size=min(nnz, cols.size), replace=False)
        W[n, c] = rng.choice([-1.0, 1.0], size=c.size)
    for n0 in range(0, N, 16):
        for k0 in range(0, width, 32):
            ok = cols[(cols >= k0) & (cols < k0 + 32)]
            if ok.size and not W[n0:n0 + 16, k0:k0 + 32].any():
                W[rng.integers(n0, min(n0 + 16, N)), rng.choice(ok)] = rng.choice([-1.0, 1.0])
    return W


def _pow2_floor(n):
    return 1 << (int(n).bit_length() - 1)


def _generate(case):
    """The exact inputs of ``case`` (fp64 numpy; his int32), without the conditions."""
    E, H1, H2 = case.shape
    B, L = case.B, case.L
    rng = np.random.default_rng([case.seed, B, L, E, H1, H2, int(case.swap)])
    S, V = _sv(case)
    inp = SimpleNamespace(case=case)
    inp.q = rng.choice([-1.0, 0.0, 1.0], size=(B, E), p=[0.25, 0.5, 0.25])
    inp.k = rng.choice([-1.0, 0.0, 1.0], size=(B, L, E), p=[0.25, 0.5, 0.25])
    # W1: the q block free, the k / q - k / q k blocks on the score columns only
    cols1 = np.concatenate([np.arange(E)] + [blk * E + S for blk in (1, 2, 3)])
    inp.W1 = _sparse_rows(rng, H1, np.sort(cols1), 4 * E, 4)
    inp.b1 = rng.integers(0, 2, H1).astype(np.float64)
    inp.W2 = _sparse_rows(rng, H2, np.arange(H1), H1, 4)
    inp.b2 = rng.integers(-1, 2, H2).astype(np.float64)
    inp.w3 = np.zeros(H2)
    if not case.tied:
        # one non-zero in every 16-column tile of H2 first, the rest anywhere
        c = [int(rng.integers(t, min(t + 16, H2))) for t in range(0, H2, 16)] if case.nw3 >= _ceil(H2, 16) else []
        more = np.setdiff1d(np.arange(H2), c)
        c += list(rng.choice(more, size=min(max(case.nw3 - len(c), 0), more.size), replace=False))
        inp.w3[c] = rng.choice([-W3, W3], size=len(c))
        # a winner has the H2 columns with w3 > 0 active and those with w3 < 0 idle, so
        # the gradient flows through the former: one per tile of H2 (the first picks)
        # or at least one, and every 16-column tile of H1 feeds one of them with + 1
        pos = c[:max(_ceil(H2, 16) if case.nw3 >= _ceil(H2, 16) else 1, 1)]
        inp.w3[pos] = W3
        for h0 in range(0, H1, 16):
            if not (inp.W2[pos, h0:h0 + 16] > 0).any():
                inp.W2[rng.choice(pos), rng.integers(h0, min(h0 + 16, H1))] = 1.0
    inp.b3 = float(rng.integers(-3, 4))
    # dtop = [dq part: 4 non-zeros | du: 2 non-zeros, on the value columns]
    inp.dtop = np.zeros((B, 2 * E))
    for b in range(B):
        c = rng.choice(E, size=4, replace=False)
        inp.dtop[b, c] = rng.choice([-1.0, 1.0], size=4)
        c = rng.choice(V, size=2, replace=False)
        inp.dtop[b, E + c] = rng.choice([-1.0, 1.0], size=2)
    # validity: position 0 with his == 0, a lone position 0, interior holes, masked
    # tails, every position valid
    his = rng.integers(1, 1000, (B, L)).astype(np.int32)
    if case.tied == "pow2":  # 2^(b % 7) valid positions: position 0 and random others
        for b in range(B):
            n = min(1 << (b % 7), L)
            keep = np.concatenate([[0], 1 + rng.choice(L - 1, size=n - 1, replace=False)]) if n < L \
                else np.arange(L)
            if b % 2:  # a tail instead of holes
                keep = np.arange(n)
            his[b, np.setdiff1d(np.arange(L), keep)] = 0
            if b % 3 == 0:
                his[b, 0] = 0  # forced valid all the same
    elif not case.tied:
        for b in range(B):
            kind = b % 8
            if kind == 0:
                his[b, 0] = 0
            elif kind == 1 and b % 16 == 1:
                his[b, 1:] = 0
            elif kind in (2, 3):
                his[b, 1:][rng.random(L - 1) < 0.25] = 0
            elif kind in (4, 5) and L > 1:
                his[b, rng.integers(1, L):] = 0
        _mask_surplus_winners(inp, his, rng)
    inp.his = his
    return inp


def _scores(inp):
    """(X, H1, H2, s) of the attention MLP in fp64"""
    q, k = inp.q, inp.k
    qb = np.broadcast_to(q[:, None, :], k.shape)
    X = np.concatenate([qb, k, qb - k, qb * k], axis=-1)
    H1 = np.maximum(X @ inp.W1.T + inp.b1, 0.0)
    H2 = np.maximum(H1 @ inp.W2.T + inp.b2, 0.0)
    return X, H1, H2, H2 @ inp.w3 + inp.b3


def _mask_surplus_winners(inp, his, rng):
    """Per sample: the winners are the valid positions at the maximum score.  Keep a
    power of two of them (at most 8; position 0 cannot be masked), preferring as the
    last kept winner one that sits at an edge of the backward's control flow
    (position nv - 1 for nv in NV_EDGES, the wanted edge rotating with the sample),
    and mask the rest (his = 0).  ``inp.masked`` lists the masked (b, j)."""
    s = _scores(inp)[3]
    B, L = his.shape
    inp.masked = []
    for b in range(B):
        valid = his[b] > 0
        valid[0] = True
        win = np.flatnonzero(valid & (s[b] == s[b][valid].max()))
        edges = [e - 1 for e in NV_EDGES if e - 1 in win]
        if edges and b % 3 == 0:
            last = edges[(b // 3) % len(edges)]
        else:
            last = win[-1]
        cand = win[win <= last]
        if cand[0] == 0 and last != 0:
            must = [0, last]
        else:
            must = [last]
        n = max(_pow2_floor(min(cand.size, 8)) >> int(rng.random() < 0.25), len(must))
        rest = np.setdiff1d(cand, must)
        keep = np.concatenate([must, rng.choice(rest, size=n - len(must), replace=False)]).astype(int)
        drop = np.setdiff1d(win, keep)
        his[b, drop] = 0
        inp.masked += [(b, int(j)) for j in drop]


def _part_sums(Z, Xm, parts):
    """[parts, Z cols, Xm cols]: workgroup w's sum over its samples b = w (mod parts)
    and their rows of Z^T Xm (Z [B, L, n], Xm [B, L, m])"""
    B = Z.shape[0]
    out = np.zeros((parts, Z.shape[2], Xm.shape[2]))
    for b0 in range(0, B, parts):
        n = min(parts, B - b0)
        out[:n] += np.einsum("bln,blm->bnm", Z[b0:b0 + n], Xm[b0:b0 + n])
    return out


def _restate(inp, parts=None, absolute=False):
    """include/mrec.h's contract of the fused attention unit in fp64, every
    intermediate kept.  ``parts``: also the per-workgroup partials.  ``absolute``:
    every sum over absolute values of its terms (the order-independence bound)."""
    E = inp.q.shape[1]
    B, L, _ = inp.k.shape
    q, k, W1, W2, w3 = inp.q, inp.k, inp.W1, inp.W2, inp.w3
    r = SimpleNamespace()
    r.X, r.H1, r.H2, r.s = _scores(inp)
    r.valid = inp.his > 0
    r.valid[:, 0] = True
    # masked softmax: s - max is 0 on a winner, <= -128 on a loser, -inf where invalid;
    # a is what fp32 holds of it (exp(-128) is below fp32's smallest number)
    sm = np.where(r.valid, r.s, -np.inf)
    e = np.exp(sm - sm.max(-1, keepdims=True))
    r.a = (e / e.sum(-1, keepdims=True)).astype(np.float32).astype(np.float64)
    r.u = (r.a[..., None] * k).sum(1)
    r.top = np.concatenate([q, r.u], -1)
    # backward: g_j = du . k_j, ds_j = a_j (g_j - sum_i a_i g_i)
    dtq, du = inp.dtop[:, :E], inp.dtop[:, E:]
    r.g = (k * du[:, None, :]).sum(-1)
    r.ds = r.a * (r.g - (r.a * r.g).sum(-1, keepdims=True))
    r.dZ2 = r.ds[..., None] * w3 * (r.H2 > 0)
    r.dZ1 = (r.dZ2 @ W2) * (r.H1 > 0)
    r.dX = r.dZ1 @ W1
    dfq, dfk, dfd, dfm = (r.dX[..., i * E:(i + 1) * E] for i in range(4))
    # dk_j = a_j du + df_k - df_(q-k) + df_(q k) q; dq = dtop_q + sum_j (df_q + df_(q-k) + df_(q k) k_j)
    r.dk = r.a[..., None] * du[:, None, :] + dfk - dfd + dfm * q[:, None, :]
    r.dq = dtq + (dfq + dfd + dfm * k).sum(1)
    r.d_rows = np.concatenate([r.dq, r.dk.reshape(B * L, E)])
    ones = np.ones((B, L, 1))
    r.dW1 = np.einsum("bln,blm->nm", r.dZ1, r.X)
    r.dW2 = np.einsum("bln,blm->nm", r.dZ2, r.H1)
    r.db1, r.db2 = r.dZ1.sum((0, 1)), r.dZ2.sum((0, 1))
    r.dw3 = np.einsum("bl,bln->n", r.ds, r.H2)
    r.db3 = r.ds.sum()
    r.grads = np.concatenate([r.dW1.reshape(-1), r.dW2.reshape(-1), r.db1, r.db2, r.dw3, [r.db3]])
    if parts is not None:
        f = np.abs if absolute else (lambda v: v)
        pieces = [_part_sums(f(r.dZ1), f(r.X), parts).reshape(parts, -1),
                  _part_sums(f(r.dZ2), f(r.H1), parts).reshape(parts, -1),
                  _part_sums(f(r.dZ1), ones, parts).reshape(parts, -1),
                  _part_sums(f(r.dZ2), ones, parts).reshape(parts, -1),
                  _part_sums(f(r.H2), f(r.ds)[..., None], parts).reshape(parts, -1),
                  _part_sums(f(r.ds)[..., None], ones, parts).reshape(parts, -1)]
        r.part = np.concatenate(pieces, axis=1)
    return r


# what the device returns: a mutation has to change one of these
OUTPUTS = ("a", "top", "d_rows", "grads")


def _is_bf16(v):
    v = np.asarray(v, np.float64)
    return np.array_equal(ref.bf16_round(v.astype(np.float32)).astype(np.float64), v)


def _mmax(r):
    """the case's largest m: the winners of a sample number 2^m"""
    return int(np.log2((r.a != 0).sum(-1).max()))


def _conditions(inp, r):
    """The conditions of one case; returns the first one violated (None: all hold).
    ``r`` carries the partials."""
    case = inp.case
    E = inp.q.shape[1]
    B, L, _ = inp.k.shape
    # --- exact softmax ---
    sm = np.where(r.valid, r.s, -np.inf)
    top = sm.max(-1, keepdims=True)
    nwin = (sm == top).sum(-1)
    if not np.array_equal(nwin & (nwin - 1), np.zeros_like(nwin)):
        return "a sample's winners are no power of two"
    gap = np.where(r.valid & (sm != top), top - sm, np.inf)
    if gap.min() < W3:
        return f"a valid loser is only {gap.min()} below the maximum"
    if not np.array_equal(r.a, np.where(sm == top, 1.0 / nwin[:, None], 0.0)):
        return "a is not 2^-m on the winners and 0 elsewhere"
    # --- representable ---
    stored = ("X", "H1", "H2", "u") if case.fwd_only else ("X", "H1", "H2", "u", "dZ2", "dZ1", "dX", "d_rows")
    for name in stored + (() if case.tied or case.fwd_only else ("ds",)):
        if not _is_bf16(getattr(r, name)):
            return f"{name} is not representable in bf16"
    # --- order independent: sum|terms| < 2^24 quanta ---
    ab = np.abs
    du, dtq = inp.dtop[:, E:], inp.dtop[:, :E]
    quantum = 2.0 ** (-2 * _mmax(r))
    nz = ab(r.ds[r.ds != 0])
    if nz.size and (nz.min() < quantum or not np.array_equal(np.round(r.ds / quantum), r.ds / quantum)):
        return "ds is no multiple of 2^-2m"
    fwd = {"layer 1": ab(r.X) @ ab(inp.W1).T + ab(inp.b1),
           "layer 2": ab(r.H1) @ ab(inp.W2).T + ab(inp.b2),
           "score": ab(r.H2) @ ab(inp.w3) + abs(inp.b3),
           "pooled sum": (r.a[..., None] * ab(inp.k)).sum(1) * 2.0 ** _mmax(r)}
    dfq, dfk, dfd, dfm = (ab(r.dZ1) @ ab(inp.W1)[:, i * E:(i + 1) * E] for i in range(4))
    bwd = {"g": (ab(inp.k) * ab(du)[:, None, :]).sum(-1),
           "sum a g": (r.a * ab(r.g)).sum(-1),
           "dH1": ab(r.dZ2) @ ab(inp.W2),
           "dX": ab(r.dZ1) @ ab(inp.W1),
           "dk": r.a[..., None] * ab(du)[:, None, :] + dfk + dfd + dfm * ab(inp.q)[:, None, :],
           "dq": ab(dtq) + (dfq + dfd + dfm * ab(inp.k)).sum(1),
           "partials": inp.abs_part, "partial sums": inp.abs_part.sum(0)}
    for name, v in fwd.items():
        if np.max(v) >= 2.0 ** 24:
            return f"{name}: sum|terms| reaches {np.max(v)} quanta"
    for name, v in bwd.items():
        if not case.fwd_only and np.max(v) / quantum >= 2.0 ** 24:
            return f"{name}: sum|terms| reaches {np.max(v) / quantum} quanta"
    # --- sensitive (the tiles of dW1 / dW2: over the family, test_matrix_is_sensitive) ---
    if case.tied:
        if any(getattr(r, n).any() for n in ("dW1", "dW2", "db1", "db2")) or not r.dw3.any():
            return "an all-tied case has dW1 / dW2 / db1 / db2 != 0 or dw3 == 0"
        return None
    for name in ("H1", "H2"):
        frac = (getattr(r, name) > 0).mean()
        if not 0.25 <= frac <= 0.75:
            return f"ReLU {name} is active on {frac:.2f} of its elements"
    if L == 64 and B > _G():
        # slot 1 of the backward sees one and two k steps and every row tile, and some
        # workgroup pairs a sample that ends in rows 0..31 (slot 0) with one that has
        # ds != 0 in rows 32..63 (slot 1), and the other way round: each slot's k steps
        # follow its own sample
        G = _G()
        nv, late = _nv(r), (r.ds[:, 32:] != 0).any(-1)
        nv1 = nv[(np.arange(B) // G) % 2 == 1]
        if not (nv1.min() <= 16 and ((nv1 > 32) & (nv1 <= 48)).any() and nv1.max() > 48):
            return f"slot 1's samples end at {sorted(nv1)}"
        pairs = [(b, b + G) for b in range(B - G)]
        if not any(nv[b0] <= 32 and late[b1] for b0, b1 in pairs):
            return "no workgroup pairs a short slot-0 sample with a long slot-1 sample"
        if not any(late[b0] and nv[b1] <= 32 for b0, b1 in pairs):
            return "no workgroup pairs a long slot-0 sample with a short slot-1 sample"
    if L > 1 and not case.fwd_only and (r.ds != 0).any(-1).mean() < 0.30:
        return f"only {(r.ds != 0).any(-1).mean():.2f} of the samples have ds != 0"
    return None


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, restatement with the partials) of a case, computed once and shared;
    the generator asserts the conditions"""
    case = BY_NAME[name]
    inp = _generate(case)
    parts = _parts(case.B)
    r = _restate(inp, parts)
    inp.abs_part = _restate(inp, parts, absolute=True).part
    bad = _conditions(inp, r)
    assert bad is None, f"case {name}: {bad}"
    return inp, r


def _nv(r):
    """per sample the last position with a_j != 0, counted from 1"""
    L = r.a.shape[1]
    return L - np.argmax((r.a != 0)[:, ::-1], axis=1)


def _tiles_nonzero(M, rows=16, cols=16):
    """[tiles down, tiles across] bool: a non-zero in each rows x cols tile of M"""
    M = np.atleast_2d(M)
    n, m = _ceil(M.shape[0], rows), _ceil(M.shape[1], cols)
    P = np.zeros((n * rows, m * cols), bool)
    P[:M.shape[0], :M.shape[1]] = M != 0
    return P.reshape(n, rows, m, cols).any(axis=(1, 3))


MUTATIONS = 48  # weight blocks zeroed per case (all of them where a case has fewer)


def _blocks(inp):
    """the 16 x 32 blocks of W1 and W2 (at most MUTATIONS of them, a fixed sample; 12
    for the batches above G, whose shapes the family cases cover block by block)"""
    blocks = [(w, n0, k0) for w in ("W1", "W2") for n0 in range(0, getattr(inp, w).shape[0], 16)
              for k0 in range(0, getattr(inp, w).shape[1], 32)]
    cap = MUTATIONS if inp.case.bmul == 0 else 12
    if len(blocks) > cap:
        pick = np.random.default_rng(inp.case.seed).choice(len(blocks), cap, replace=False)
        blocks = [blocks[i] for i in sorted(pick)]
    return blocks


def _differs(r, want):
    return any(not np.array_equal(getattr(r, n), getattr(want, n)) for n in OUTPUTS)


def _unseen_mutation(inp, r):
    """Zero single 16 x 32 blocks of W1 / W2, zero the k row of a winner, unmask a
    masked winner -- in the restatement -- and return the first mutation that changes
    no expected output (None: each changes one)."""
    # (with w3 = 0 or one position the weights reach no output: a is 1 / n whatever they hold)
    for w, n0, k0 in ([] if inp.case.tied or inp.case.L == 1 else _blocks(inp)):
        W = getattr(inp, w)
        Wm = W.copy()
        Wm[n0:n0 + 16, k0:k0 + 32] = 0.0
        setattr(inp, w, Wm)
        try:
            if not _differs(_restate(inp), r):
                return (w, n0, k0)
        finally:
            setattr(inp, w, W)
    rng = np.random.default_rng(inp.case.seed + 1)
    winners = np.argwhere(r.a != 0)
    for b, j in winners[rng.choice(len(winners), size=min(8, len(winners)), replace=False)]:
        k = inp.k
        inp.k = k.copy()
        inp.k[b, j] = 0.0
        try:
            if k[b, j].any() and not _differs(_restate(inp), r):
                return ("k row", int(b), int(j))
        finally:
            inp.k = k
    for b, j in getattr(inp, "masked", [])[:8]:
        his = inp.his
        inp.his = his.copy()
        inp.his[b, j] = 5
        try:
            if not _differs(_restate(inp), r):
                return ("unmask", b, j)
        finally:
            inp.his = his
    return None


def _search_seed(case, tries=200):
    """for whoever adds a case: the first seed whose inputs meet the conditions and
    the mutation self-check"""
    for seed in range(tries):
        case.seed = seed
        inp = _generate(case)
        parts = _parts(case.B)
        r = _restate(inp, parts)
        inp.abs_part = _restate(inp, parts, absolute=True).part
        if _conditions(inp, r) is None and _unseen_mutation(inp, r) is None:
            return seed
    return None


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_case_conditions(case):
    """Every case's inputs give an exact softmax, are representable, order independent
    and sensitive (the generator's own assertion, and once more from here); the inputs
    are of the promised kind.  Runs without a GPU."""
    inp, r = _case(case.name)
    assert _conditions(inp, r) is None
    E = case.shape[0]
    S, V = _sv(case)
    for v in (inp.q, inp.k, inp.W1, inp.W2):
        assert set(np.unique(v)) <= {-1.0, 0.0, 1.0}
    assert set(np.unique(inp.w3)) <= {-W3, 0.0, W3}
    for v in (inp.b1, inp.b2, np.array([inp.b3]), inp.dtop):
        assert np.array_equal(v, np.round(v))
    assert not inp.dtop[:, E + S].any()
    for blk in (1, 2, 3):
        assert not inp.W1[:, blk * E + V].any()
    assert np.array_equal((r.s - inp.b3) / W3, np.round((r.s - inp.b3) / W3))
    assert r.db3 == 0.0 and np.array_equal(r.part.sum(0), r.grads)
    assert not r.ds[r.a == 0].any() and not r.dk[r.a == 0].any()
    if case.tied:  # a = 1 / n, u the exact mean, dk = a du
        n = r.valid.sum(-1)
        assert np.array_equal(r.a, r.valid / n[:, None])
        assert np.array_equal(r.u, (inp.k * r.valid[..., None]).sum(1) / n[:, None])
        assert np.array_equal(r.dk, r.a[..., None] * inp.dtop[:, None, E:])
        if case.tied == "pow2":
            assert set(n) == {1 << i for i in range(7)}
        else:
            assert (inp.his > 0).all()


def test_matrix_is_sensitive():
    """Over a shape family's cases every 16 x 16 tile of dW1 / dW2 and every 16-column
    tile of db1 / db2 / dw3 has a non-zero expected element; over the matrix the last
    position with a_j != 0 takes every edge of NV_EDGES, and every one but 1 (a lone
    winner has ds = 0) also with ds != 0 at that very position (and in slot 1 of the backward
    values in each of 1..16, 33..48 and 49..64), the winner counts 1, 2, 4, 8
    all occur (and 16, 32, 64 in the all-tied cases), and the validity kinds are all
    there.  Runs without a GPU."""
    nvs, live, counts, slot1 = set(), set(), set(), set()
    seen = {}
    his0 = lone = holes = False
    for case in BWD_CASES:
        inp, r = _case(case.name)
        nvs |= set(_nv(r))
        live |= set(_nv(r)[r.ds[np.arange(case.B), _nv(r) - 1] != 0])  # ... with a gradient there
        slot1 |= set(_nv(r)[(np.arange(case.B) // _G()) % 2 == 1])  # the samples slot 1 runs
        counts |= set((r.a != 0).sum(-1))
        v = inp.his > 0
        his0 |= bool((~v[:, 0]).any())
        lone |= bool((case.L > 1) and (~v[:, 1:]).all(-1).any())
        holes |= bool(case.L > 2 and (~v[:, 1:-1] & v[:, 2:]).any())
        if not case.tied:
            t = seen.setdefault(_family(case), {})
            for name in ("dW1", "dW2", "db1", "db2", "dw3"):
                t[name] = t.get(name, False) | _tiles_nonzero(getattr(r, name))
    assert set(NV_EDGES) <= nvs, sorted(set(NV_EDGES) - nvs)
    assert set(NV_EDGES[1:]) <= live, sorted(set(NV_EDGES[1:]) - live)
    assert min(slot1) <= 16 and any(32 < v <= 48 for v in slot1) and max(slot1) > 48, sorted(slot1)
    assert {1, 2, 4, 8, 16, 32, 64} <= counts
    assert his0 and lone and holes
    assert set(seen) == {f[0] for f in FAMILIES.values()}
    for fam, t in seen.items():
        for name, tiles in t.items():
            if fam[2] == 1 and name in ("db2", "dw3"):
                # one H2 column: the winners of a sample share its value (the score is
                # b3 + 128 H2), so sum ds relu' = sum ds H2 = 0 -- expected zeros
                assert not tiles.any()
                continue
            assert tiles.all(), (fam, name, np.argwhere(~tiles).tolist())


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_restatement_equals_oracle(case):
    """The restatement's forward against oracle/ref.py's din_attention_pool and
    din_softmax_pool, its pooling backward against din_softmax_pool_bwd, the MLP's
    backward against mlp_bwd.  Scores and everything downstream of a are equal as they
    stand; the oracle's own a and u keep fp64's exp(-128 n) = 1e-56 and less where fp32
    holds 0, so they are compared after the rounding to fp32 that defines a."""
    inp, r = _case(case.name)
    E = case.shape[0]
    B, L, _ = inp.k.shape
    layers = [(inp.W1, inp.b1), (inp.W2, inp.b2)]
    u, a, s = ref.din_attention_pool(inp.q, inp.k, ref.valid_his_index(inp.his), layers,
                                     (inp.w3[None, :], np.array([inp.b3])))
    assert np.array_equal(s, r.s)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), r.a)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), r.u)
    u2, a2 = ref.din_softmax_pool(r.s, r.valid, inp.k)
    assert np.array_equal(a2, a) and np.array_equal(u2, u)
    ds, dk = ref.din_softmax_pool_bwd(r.a, inp.k, inp.dtop[:, E:])
    assert np.array_equal(ds, r.ds) and np.array_equal(r.g, (inp.k * inp.dtop[:, None, E:]).sum(-1))
    acts = ref.mlp_fwd(r.X.reshape(B * L, 4 * E), layers)
    dX, grads = ref.mlp_bwd(acts, layers, r.ds.reshape(B * L, 1) * inp.w3[None, :])
    assert np.array_equal(acts[1].reshape(r.H1.shape), r.H1) and np.array_equal(acts[2].reshape(r.H2.shape), r.H2)
    assert np.array_equal(dX.reshape(r.dX.shape), r.dX)
    assert np.array_equal(grads[0][0], r.dW1) and np.array_equal(grads[0][1], r.db1)
    assert np.array_equal(grads[1][0], r.dW2) and np.array_equal(grads[1][1], r.db2)
    assert np.array_equal(acts[2].T @ r.ds.reshape(-1), r.dw3)
    dX = dX.reshape(B, L, 4, E)
    assert np.array_equal(r.dk, dk + dX[:, :, 1] - dX[:, :, 2] + dX[:, :, 3] * inp.q[:, None, :])


@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_mutation_changes_expectation(case):
    """Zeroing any single 16 x 32 block of W1 or W2, zeroing the k row of a winner or
    unmasking a masked winner changes at least one expected output of the restatement
    (``_unseen_mutation``).  Runs without a GPU."""
    inp, r = _case(case.name)
    assert _unseen_mutation(inp, r) is None


# ---------------------------------------------------------------------------
# 2. raw mrec_din_att_fwd in guarded buffers
# ---------------------------------------------------------------------------

def _t64(v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))


def _fvec(v, dev):
    """fp32 vector, NaN in front and behind"""
    return _vec1(_t64(v).reshape(-1), dev)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _check_bits(g, what):
    """``_Guarded.check`` bit for bit: for an allocation whose expected image holds NaN"""
    got, want = _bits(g.dev.cpu()), _bits(g.host)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} elements differ"


def _window(rows, ld, dtype, fill, vals, dev):
    """guarded [rows, ld] input whose columns [0, vals.shape[1]) hold ``vals``"""
    g = _Guarded(rows, ld, dtype, fill)
    g.win()[:, :vals.shape[1]] = _t64(vals).to(dtype)
    return g.up(dev)


def _output(rows, ld, dtype, dev, prefill=SENT):
    """guarded output: the device copy starts as ``prefill`` everywhere, ``host`` (the
    expected image) too until the caller edits its window"""
    g = _Guarded(rows, ld, dtype, prefill)
    g.dev = g.host.clone().to(dev)
    return g


class _Unit:
    """a case on the device: guarded operands (uploaded once) and the raw calls.
    rows has ld = E + 8 with NaN in the pad and around it, his ld = L + 3 with positive
    garbage past column L and around it, the fp32 masters ldw1 = 4E + 4 and ldw2 =
    H1 + 4 with NaN pads, dtop ld = 2E + 8."""

    def __init__(self, dev, case):
        self.dev, self.case = dev, case
        self.inp, self.r = inp, r = _case(case.name)
        E, H1, H2 = case.shape
        B, L = case.B, case.L
        self.P = 4 * E * H1 + H1 * H2 + H1 + 2 * H2 + 1
        self.rows = _window(B + B * L, E + 8, BF16, NAN, np.concatenate([inp.q, inp.k.reshape(B * L, E)]), dev)
        self.his = _Guarded(B, L + 3, I32, 9)
        self.his.win()[:, :L] = torch.from_numpy(inp.his)
        self.his.up(dev)
        self.w1 = _window(H1, 4 * E + 4, F32, NAN, inp.W1, dev)
        self.w2 = _window(H2, H1 + 4, F32, NAN, inp.W2, dev)
        self.b1, self.b2, self.w3, self.b3 = (_fvec(v, dev) for v in (inp.b1, inp.b2, inp.w3, [inp.b3]))
        self.dtop = _window(B, 2 * E + 8, BF16, NAN, inp.dtop, dev)
        self.a_in = _window(B, L, F32, NAN, r.a, dev)  # the restatement's a, for the backward
        self.inputs = {n: getattr(self, n) for n in ("rows", "his", "w1", "w2", "b1", "b2", "w3", "b3",
                                                     "dtop", "a_in")}

    def _weights(self, w1, w2):
        w1, w2 = w1 or self.w1, w2 or self.w2
        E, H1, H2 = self.case.shape
        return (w1.t.data_ptr(), w1.ld, self.b1.t.data_ptr(), H1, w2.t.data_ptr(), w2.ld,
                self.b2.t.data_ptr(), H2, self.w3.t.data_ptr(), self.b3.t.data_ptr())

    def fwd(self, w1=None, w2=None):
        """mrec_din_att_fwd into sentinel-filled outputs: (a, top) with the expected
        images: a the restatement's over all [B, L], top = [q | u | zeros to ldt]"""
        from pytorchrec_amd import _mrec
        c, r = self.case, self.r
        E, B, L = c.shape[0], c.B, c.L
        a = _output(B, L, F32, self.dev)
        a.win()[:] = _t64(r.a).float()
        top = _output(B, 2 * E + 5, BF16, self.dev)
        top.win()[:, :2 * E] = _t64(r.top).to(BF16)
        top.win()[:, 2 * E:] = 0
        _mrec.call("mrec_din_att_fwd", self.rows.t.data_ptr(), self.rows.ld, self.his.t.data_ptr(),
                   self.his.ld, B, L, E, *self._weights(w1, w2), a.t.data_ptr(), top.t.data_ptr(),
                   top.ld, _mrec.stream_handle())
        return a, top

    def bwd(self, a=None, w1=None, w2=None):
        """mrec_din_att_bwd on the restatement's a (or ``a``): (d_rows over a 7.0
        prefill, part over a NaN prefill) with the expected images"""
        from pytorchrec_amd import _mrec
        c, r = self.case, self.r
        E, B, L = c.shape[0], c.B, c.L
        parts = _parts(B)
        d_rows = _output(B + B * L, E + 8, BF16, self.dev)
        d_rows.win()[:, :E] = _t64(r.d_rows).to(BF16)
        part = _output(parts, self.P, F32, self.dev, prefill=NAN)
        part.win()[:] = _t64(r.part).float()
        _mrec.call("mrec_din_att_bwd", self.rows.t.data_ptr(), self.rows.ld, B, L, E,
                   *self._weights(w1, w2), (a or self.a_in).t.data_ptr(), self.dtop.t.data_ptr(),
                   self.dtop.ld, d_rows.t.data_ptr(), d_rows.ld, part.t.data_ptr(), parts,
                   _mrec.stream_handle())
        return d_rows, part

    def check_inputs(self):
        for name, g in self.inputs.items():
            _check_bits(g, f"input {name}")


@functools.lru_cache(maxsize=None)
def _unit(name):
    return _Unit(torch.device("cuda:0"), BY_NAME[name])


@gpu_test
@pytest.mark.parametrize("wg", [0, 1], ids=["wave", "workgroup"])
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_forward_is_exact(gpu, monkeypatch, case, wg):
    """mrec_din_att_fwd, the one-wave-per-sample kernel and MREC_DIN_FWD_WG=1: a is
    the restatement's bit for bit over all [B, L] (2^-m on the winners, zero at losers
    and invalid positions), top = [q | u | zeros to ldt] with ldt = 2E + 5, the 7.0
    around both and every operand untouched."""
    monkeypatch.setenv("MREC_DIN_FWD_WG", str(wg))
    u = _unit(case.name)
    a, top = u.fwd()
    torch.cuda.synchronize()
    _check_bits(a, "a")
    top.check("top")
    u.check_inputs()


# ---------------------------------------------------------------------------
# 3. raw mrec_din_att_bwd + mrec_din_att_wgrad
# ---------------------------------------------------------------------------

LR = 2.0 ** -4


@gpu_test
@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_backward_and_wgrad_are_exact(gpu, case):
    """mrec_din_att_bwd on the restatement's a: d_rows equals the expectation over the
    whole allocation (q rows, k rows, exact zeros at every loser and invalid position,
    the pad columns and guards still 7.0); every element of every partial is written
    over its NaN prefill and each partial row is its workgroup's sum (parts from
    mrec_din_att_parts).  Then mrec_din_att_wgrad both ways: into a flat vector -- all
    six gradients exact, db3 bitwise 0 -- and as in-place SGD with lr = 2^-4 on guarded
    masters: p - lr g exact, pads and guards untouched."""
    from pytorchrec_amd import _mrec
    u = _unit(case.name)
    inp, r = u.inp, u.r
    E, H1, H2 = case.shape
    parts = _parts(case.B)
    assert parts == min(case.B, _G()) and r.part.shape == (parts, u.P)
    assert u.P == int(_mrec.lib().mrec_din_att_param_count(E, H1, H2))
    d_rows, part = u.bwd()
    torch.cuda.synchronize()
    d_rows.check("d_rows")
    assert not torch.isnan(part.t).any(), "a partial element was never written"
    _check_bits(part, "partials")
    u.check_inputs()
    # the flat gradient vector
    grads = _output(1, u.P, F32, gpu)
    grads.win()[0] = _t64(r.grads).float()
    st = _mrec.stream_handle()
    _mrec.call("mrec_din_att_wgrad", part.t.data_ptr(), parts, E, H1, H2, grads.t.data_ptr(), 0.0,
               None, 0, None, None, 0, None, None, None, st)
    # in-place SGD on guarded masters
    want = [inp.W1 - LR * r.dW1, inp.b1 - LR * r.db1, inp.W2 - LR * r.dW2, inp.b2 - LR * r.db2,
            inp.w3 - LR * r.dw3, np.array([inp.b3 - LR * r.db3])]
    for v in want:  # a condition on the inputs: the update is exact in fp32
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    w1 = _window(H1, 4 * E + 4, F32, NAN, inp.W1, gpu)
    w2 = _window(H2, H1 + 4, F32, NAN, inp.W2, gpu)
    vecs = [_fvec(v, gpu) for v in (inp.b1, inp.b2, inp.w3, [inp.b3])]
    _mrec.call("mrec_din_att_wgrad", part.t.data_ptr(), parts, E, H1, H2, None, LR,
               w1.t.data_ptr(), w1.ld, vecs[0].t.data_ptr(), w2.t.data_ptr(), w2.ld,
               vecs[1].t.data_ptr(), vecs[2].t.data_ptr(), vecs[3].t.data_ptr(), st)
    torch.cuda.synchronize()
    grads.check("grads")
    assert int(_bits(grads.t[0, -1:].cpu())) == 0, "db3 is not bitwise zero"
    for g, v, what in zip([w1, vecs[0], w2, vecs[1], vecs[2], vecs[3]], want,
                          ("W1", "b1", "W2", "b2", "w3", "b3")):
        v = _t64(v).float()
        g.win()[:, :v.reshape(g.rows, -1).shape[1]] = v.reshape(g.rows, -1)
        _check_bits(g, f"SGD {what}")
    _check_bits(part, "partials after wgrad")


# ---------------------------------------------------------------------------
# 4. through the public wrapper
# ---------------------------------------------------------------------------

def _modules(inp, dev):
    """the attention MLP and Linear(H2, 1) holding the generator's values"""
    from pytorchrec_amd.model.layer import MLP
    E, H1, H2 = inp.case.shape
    att = MLP(4 * E, [H1, H2], "relu", 0.0).to(dev)
    out = torch.nn.Linear(H2, 1).to(dev)
    lins = [d.linear for d in att.mlp] + [out]
    with torch.no_grad():
        for lin, w, b in zip(lins, (inp.W1, inp.W2, inp.w3[None, :]), (inp.b1, inp.b2, [inp.b3])):
            lin.weight.copy_(_t64(w))
            lin.bias.copy_(_t64(b).reshape(-1))
    return att, out, lins


def _same(got, want, what):
    got = got.detach().cpu().double()
    assert torch.equal(got, _t64(want).reshape(got.shape)), what


@gpu_test
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("case", FAMILY_CASES, ids=_ids(FAMILY_CASES))
def test_top_rows_wrapper_is_exact(gpu, monkeypatch, case, fused):
    """dense.din_attention_top_rows on exact-integer modules, on the fused unit and on
    the layered kernels (mrec_din_feat_fwd, the GEMMs, mrec_din_pool_fwd / _bwd,
    mrec_din_feat_bwd_rows): top, rows.grad and the six parameter gradients are
    bitwise the restatement's.  What the layered path rounds to bf16 on the way (the
    features, H1, H2, ds, dZ2, dZ1, the features' gradient) is in the representability
    condition."""
    from pytorchrec_amd import dense as D
    inp, r = _case(case.name)
    E = case.shape[0]
    B, L = case.B, case.L
    monkeypatch.setattr(D, "DIN_FUSED", fused)
    att, out, lins = _modules(inp, gpu)
    assert D.din_att_supported(E, att, out)
    rows = _t64(np.concatenate([inp.q, inp.k.reshape(B * L, E)])).to(BF16).to(gpu).requires_grad_()
    his = torch.from_numpy(inp.his).to(gpu)
    top = D.din_attention_top_rows(rows, B, his, att, out)
    assert ("DinAtt" in type(top.grad_fn).__name__) == fused
    top.backward(_t64(inp.dtop).to(BF16).to(gpu))
    torch.cuda.synchronize()
    _same(top, r.top, "top")
    _same(rows.grad, r.d_rows, "rows.grad")
    for lin, dW, db, what in zip(lins, (r.dW1, r.dW2, r.dw3), (r.db1, r.db2, [r.db3]), "123"):
        _same(lin.weight.grad, dW, "dW" + what)
        _same(lin.bias.grad, db, "db" + what)


# ---------------------------------------------------------------------------
# 5. device mutation evidence
# ---------------------------------------------------------------------------

@gpu_test
@pytest.mark.parametrize("case", FAMILY_CASES, ids=_ids(FAMILY_CASES))
def test_device_mutations_are_caught(gpu, monkeypatch, case):
    """Zero single 16 x 32 blocks of the device W1 / W2 masters (the blocks of
    ``test_mutation_changes_expectation``, at most 48 per case): the fused forward or
    the backward fed the forward's own a no longer gives the unmutated expectation.
    Valid launches on valid buffers."""
    monkeypatch.setenv("MREC_DIN_FWD_WG", "0")
    u = _unit(case.name)
    E, H1, H2 = case.shape
    caught = tried = 0
    for w, n0, k0 in _blocks(u.inp):
        W = getattr(u.inp, w).copy()
        W[n0:n0 + 16, k0:k0 + 32] = 0.0
        g = _window(W.shape[0], W.shape[1] + 4, F32, NAN, W, gpu)
        kw = {"w1" if w == "W1" else "w2": g}
        a, top = u.fwd(**kw)
        d_rows, part = u.bwd(a=a, **kw)
        torch.cuda.synchronize()
        tried += 1
        caught += any(not torch.equal(_bits(x.dev.cpu()), _bits(x.host)) for x in (a, top, d_rows, part))
    print(f"{case.name}: {caught} / {tried} device mutations caught")
    assert caught == tried


# ---------------------------------------------------------------------------
# 6. the layered kernels of din.hip, on inputs of the same kind
# ---------------------------------------------------------------------------

FEAT_CASES = ["c4", "e68s", "s24", "s20s", "l1", "b2G+1"]


@gpu_test
@pytest.mark.parametrize("name", FEAT_CASES)
def test_layered_feature_kernels_are_exact(gpu, name):
    """mrec_din_feat_fwd writes exactly X = [q | k | q - k | q k] (ldf = 4E + 8, the pad
    and the guards still 7.0).  mrec_din_feat_bwd with a sparse -1 / 0 / 1 dfeat adds
    df_k - df_(q-k) + df_(q k) q to an integer fp32 dk in place (lddk = E + 4) and writes
    dq = dtop_q + sum_j (df_q + df_(q-k) + df_(q k) k_j) (lddq = E + 4);
    mrec_din_feat_bwd_rows gives the same two as one bf16 gradient of the gathered
    rows and leaves dk as it was.  All sums are small integers: exact in any order."""
    from pytorchrec_amd import _mrec
    u = _unit(name)
    inp, r, case = u.inp, u.r, u.case
    E, B, L = case.shape[0], case.B, case.L
    rng = np.random.default_rng(case.seed)
    st = _mrec.stream_handle()
    q_ptr, k_ptr, ld = u.rows.t.data_ptr(), u.rows.t[B:].data_ptr(), u.rows.ld
    feat = _output(B * L, 4 * E + 8, BF16, gpu)
    feat.win()[:, :4 * E] = _t64(r.X.reshape(B * L, 4 * E)).to(BF16)
    _mrec.call("mrec_din_feat_fwd", q_ptr, ld, k_ptr, ld, B, L, E, feat.t.data_ptr(), feat.ld, st)
    df = rng.choice([-1.0, 0.0, 1.0], size=(B, L, 4, E), p=[0.1, 0.8, 0.1])
    dk0 = rng.integers(-2, 3, (B, L, E)).astype(np.float64)
    dk = dk0 + df[:, :, 1] - df[:, :, 2] + df[:, :, 3] * inp.q[:, None, :]
    dq = inp.dtop[:, :E] + (df[:, :, 0] + df[:, :, 2] + df[:, :, 3] * inp.k).sum(1)
    assert _is_bf16(dq) and _is_bf16(dk)
    dfeat = _window(B * L, 4 * E + 8, BF16, NAN, df.reshape(B * L, 4 * E), gpu)
    outs = {"feat": feat}
    for rows_mode in (False, True):
        g_dk = _output(B * L, E + 4 + rows_mode, F32, gpu)  # E + 5: the kernel's scalar dk path
        g_dk.win()[:, :E] = _t64(dk0.reshape(B * L, E)).float()
        g_dk.up(gpu)
        head = (dfeat.t.data_ptr(), dfeat.ld, u.dtop.t.data_ptr(), u.dtop.ld, q_ptr, ld, k_ptr, ld, B, L, E,
                g_dk.t.data_ptr(), g_dk.ld)
        if rows_mode:
            d_rows = _output(B + B * L, E + 8, BF16, gpu)
            d_rows.win()[:, :E] = _t64(np.concatenate([dq, dk.reshape(B * L, E)])).to(BF16)
            _mrec.call("mrec_din_feat_bwd_rows", *head, d_rows.t.data_ptr(), d_rows.ld, st)
            outs.update({"d_rows": d_rows, "dk left alone": g_dk})
        else:
            g_dq = _output(B, E + 4, F32, gpu)
            g_dq.win()[:, :E] = _t64(dq).float()
            _mrec.call("mrec_din_feat_bwd", *head, g_dq.t.data_ptr(), g_dq.ld, st)
            g_dk.win()[:, :E] = _t64(dk.reshape(B * L, E)).float()
            outs.update({"dk": g_dk, "dq": g_dq})
    torch.cuda.synchronize()
    for what, g in outs.items():
        g.check(what)
    u.check_inputs()
    _check_bits(dfeat, "dfeat")


POOL_CASES = [(37, 64, 64), (9, 50, 32), (5, 17, 8), (6, 1, 16), (70, 33, 16)]


@gpu_test
@pytest.mark.parametrize("B,L,E", POOL_CASES, ids=[f"{B}x{L}x{E}" for B, L, E in POOL_CASES])
def test_layered_pooling_kernels_are_exact(gpu, B, L, E):
    """mrec_din_pool_fwd / mrec_din_pool_bwd with the scores planted directly as fp32
    (ld_s = 2): sample b has 2^m winners, m = b mod 7 as far as its valid positions
    allow, anywhere among them, every valid loser 128 or more below, and a finite
    3e38 at every invalid position (it must be masked, not compared).  a is 2^-m on
    the winners and zero elsewhere bit for bit, top = [q | u | zeros to ldt = 2E + 5],
    ds = a (g - sum a g) and dk = a du (fp32, lddk = E + 4) with an integer du."""
    from pytorchrec_amd import _mrec
    rng = np.random.default_rng([B, L, E])
    q = rng.choice([-1.0, 0.0, 1.0], size=(B, E))
    k = rng.choice([-1.0, 0.0, 1.0], size=(B, L, E))
    his = rng.integers(1, 1000, (B, L)).astype(np.int32)
    his[rng.random((B, L)) < 0.3] = 0
    his[np.arange(B) % 7 >= 3] = 7  # every position valid where many winners are wanted
    his[B - 1, 1:] = 0  # a lone position 0
    valid = ref.valid_his_index(his).astype(bool)
    s = np.full((B, L), 3e38)
    for b in range(B):
        v = np.flatnonzero(valid[b])
        n = min(1 << (b % 7), _pow2_floor(v.size))
        top = 128.0 * rng.integers(-2, 3)
        s[b, v] = top - 128.0 * rng.integers(1, 6, v.size)
        s[b, rng.choice(v, size=n, replace=False)] = top
    dtop = rng.integers(-3, 4, (B, 2 * E)).astype(np.float64)
    _, a = ref.din_softmax_pool(s, valid, k)
    a = a.astype(np.float32).astype(np.float64)  # what fp32 holds: exp(-128) and less is 0
    n = (a != 0).sum(-1)
    assert np.array_equal(a, (a != 0) / n[:, None])
    assert set(n) >= {1 << m for m in range(7) if 1 << m <= L and m < B - 1} and not (n & (n - 1)).any()
    u = (a[..., None] * k).sum(1)
    ds, dk = ref.din_softmax_pool_bwd(a, k, dtop[:, E:])
    assert _is_bf16(u)
    g_s = _window(B * L, 2, F32, NAN, s.reshape(B * L, 1), gpu)
    g_his = _Guarded(B, L + 3, I32, 9)
    g_his.win()[:, :L] = torch.from_numpy(his)
    g_his.up(gpu)
    g_q = _window(B, E + 8, BF16, NAN, q, gpu)
    g_k = _window(B * L, E + 8, BF16, NAN, k.reshape(B * L, E), gpu)
    g_dtop = _window(B, 2 * E + 8, BF16, NAN, dtop, gpu)
    o_a, o_top = _output(B, L, F32, gpu), _output(B, 2 * E + 5, BF16, gpu)
    o_a.win()[:] = _t64(a).float()
    o_top.win()[:, :2 * E] = _t64(np.concatenate([q, u], -1)).to(BF16)
    o_top.win()[:, 2 * E:] = 0
    st = _mrec.stream_handle()
    _mrec.call("mrec_din_pool_fwd", g_s.t.data_ptr(), g_s.ld, g_his.t.data_ptr(), g_his.ld,
               g_q.t.data_ptr(), g_q.ld, g_k.t.data_ptr(), g_k.ld, B, L, E, o_a.t.data_ptr(),
               o_top.t.data_ptr(), o_top.ld, st)
    g_a = _window(B, L, F32, NAN, a, gpu)
    o_ds, o_dk = _output(B, L, F32, gpu), _output(B * L, E + 4, F32, gpu)
    o_ds.win()[:] = _t64(ds).float()
    o_dk.win()[:, :E] = _t64(dk.reshape(B * L, E)).float()
    _mrec.call("mrec_din_pool_bwd", g_dtop.t.data_ptr(), g_dtop.ld, g_a.t.data_ptr(), g_k.t.data_ptr(),
               g_k.ld, B, L, E, o_ds.t.data_ptr(), o_dk.t.data_ptr(), o_dk.ld, st)
    torch.cuda.synchronize()
    _check_bits(o_a, "a")
    for what, g in (("top", o_top), ("ds", o_ds), ("dk", o_dk)):
        g.check(what)
    for what, g in (("s", g_s), ("his", g_his), ("q", g_q), ("k", g_k), ("dtop", g_dtop), ("a", g_a)):
        _check_bits(g, what)
