"""The reference's own CPU path for an EmbeddingBank on a CPU device.

Config C1 of BASELINE.json runs FM through the CLI on the CPU ("PyTorch CPU path
(plumbing, no GPU)").  For a bank whose weight lives on the CPU, the ops in
``embedding.py`` dispatch here: plain torch ``index_select`` gathers and autograd
dense gradients, exactly the arithmetic ``nn.Embedding`` does on CPU
(FunkSVD.py:47-51, IModel.py:116-125).  The bank ops of this module are never used
for a tensor on a GPU — those go through libmrec or raise.  ``neg_sample`` is the CPU
sampler of ``sampling.NegativeSampler``: the counter hash of ``mrec_neg_sample`` in
numpy.  ``sasrec_encode`` is the SASRec encoder in torch ops: the CPU path, and on a GPU
the layered path for the shapes and modes the fused kernels do not cover
(``dense.sasrec_encode`` decides); ``gru_encode`` is the same for the GRU4Rec recurrence
(``dense.gru_encode`` decides).  ``topk`` is ``mrec_topk``, the full-catalogue retrieval, in
torch ops, chunked over the items (``retrieval.topk`` decides).  ``shared_negative_loss`` is
``mrec_shneg_loss_fwd`` / ``_bwd``, the list-wise losses over a shared pool of negatives, in
differentiable torch ops (``loss.SharedNegativeLoss`` decides).  ``dot_interact`` is
``mrec_dot_interact_fwd`` / ``_bwd``, DLRM's pairwise dot interaction, in the same way
(``dense.dot_interact`` decides).  ``cin`` is ``mrec_cin_fwd`` / ``_bwd``, xDeepFM's Compressed
Interaction Network, chunked over the batch (``dense.cin`` decides).  ``autoint`` is
``mrec_autoint_fwd`` / ``_bwd``, AutoInt's interacting layers, in the same way
(``dense.autoint`` decides).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch


def _rows(bank, ids: List[torch.Tensor]) -> List[torch.Tensor]:
    out = []
    for f, t in enumerate(ids):
        t = t.long()
        n = bank.category_nums[f]
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise IndexError("index out of range in self")
        out.append(t + bank.row_offset[f])
    return out


def _weight(bank):
    """The weight as seen by autograd: the parameter itself in dense mode; in fused
    SGD mode a detached leaf whose gradient is applied as SGD by a hook."""
    if bank.update == "dense" or not torch.is_grad_enabled():
        return bank.weight
    w = bank.weight.detach().requires_grad_()
    lr = bank.current_lr()
    target = bank.weight

    def _sgd(g):
        with torch.no_grad():
            target.add_(g.to(target.dtype), alpha=-lr)
        return g

    w.register_hook(_sgd)
    return w


def gather(bank, ids, out_dtype, with_w: bool):
    w = _weight(bank)
    rows = _rows(bank, ids)
    v = torch.cat([w.index_select(0, r)[:, :bank.dim] for r in rows], dim=1).to(out_dtype)
    if with_w:
        ww = torch.stack([w.index_select(0, r)[:, bank.dim] for r in rows], dim=1).float()
        return v, ww
    return v


def pooled_gather(bank, ids, mode: str, pad: str, out_dtype, with_w: bool):
    """embedding -> mask -> sum over the bag -> scale (SVDPP.py:49-55), per field; the
    scale is 1, 1/n or 1/sqrt(n) (n = valid count), 0 for an empty bag."""
    w = _weight(bank)
    vs, ws = [], []
    for f, t in enumerate(ids):
        t = t.long()
        B, L = t.shape
        n = bank.category_nums[f]
        valid = t > 0 if pad == "zero" else t >= 0
        if bool(((t >= n) | ((t < 0) if pad == "zero" else torch.zeros_like(valid))).any()):
            raise IndexError("index out of range in self")
        safe = torch.where(valid, t, torch.zeros_like(t)) + bank.row_offset[f]
        rows = w.index_select(0, safe.reshape(-1)).reshape(B, L, -1).float()
        m = valid.float()
        cnt = m.sum(dim=1).double()
        if mode == "sum":
            scale = (cnt > 0).double()
        elif mode == "mean":
            scale = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
        else:
            scale = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0).sqrt(), torch.zeros_like(cnt))
        pooled = (rows * m.unsqueeze(-1)).sum(dim=1) * scale.float().unsqueeze(-1)
        vs.append(pooled[:, :bank.dim])
        if with_w:
            ws.append(pooled[:, bank.dim])
    v = torch.cat(vs, dim=1).to(out_dtype)
    if with_w:
        return v, torch.stack(ws, dim=1)
    return v


_NS_G = np.uint64(0x9E3779B97F4A7C15)


def _mix64(z):
    """The splitmix64 finaliser on a uint64 array (wrapping arithmetic)."""
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def neg_sample(uids, n_neg: int, keys, n_users: int, low: int, high: int, seed: int,
               step: int, max_attempts: int):
    """``mrec_neg_sample`` restated in numpy uint64 (the hash is written down in
    include/mrec.h), bit for bit: -> (int32 ``[B, n_neg]``, outputs left unresolved).
    ``keys``: the sorted int64 array ``uid << 32 | item bits`` of the users' items."""
    u = np.asarray(uids).astype(np.int64).reshape(-1)
    total = u.size * n_neg
    out = np.full(total, low, np.int32)
    if total == 0:
        return out.reshape(-1, n_neg), 0
    with np.errstate(over="ignore"):
        one = np.ones(1, np.uint64)
        key0 = _mix64(_mix64(one * np.uint64(seed & (2 ** 64 - 1)) + _NS_G)
                      + np.uint64(step & (2 ** 64 - 1)))
        key = _mix64(key0 + np.arange(total, dtype=np.uint64))
        uu = np.repeat(u, n_neg)
        known = (uu >= 0) & (uu < n_users)
        rng = np.uint64(high - low)
        todo = np.arange(total)
        for a in range(max_attempts):
            h = _mix64(key[todo] + np.uint64(a + 1) * _NS_G)
            item = (low + (((h >> np.uint64(32)) * rng) >> np.uint64(32)).astype(np.int64))
            out[todo] = item.astype(np.int32)
            probe = (uu[todo] << 32) | (item & 0xFFFFFFFF)
            at = np.searchsorted(keys, probe)
            taken = known[todo] & (at < keys.size)
            taken[taken] = keys[at[taken]] == probe[taken]
            todo = todo[taken]
            if todo.size == 0:
                break
    return out.reshape(-1, n_neg), int(todo.size)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> nearest bf16 -> fp32, with the identity as its gradient."""
    return t + (t.to(torch.bfloat16).float() - t).detach()


def sasrec_positions(his: torch.Tensor, his_len: torch.Tensor):
    """(valid [B, L] bool, position ids [B, L] int64) of a padded history:
    valid_j = his_j > 0 with valid_0 forced (utils.py:5-10), pos_j = (his_len - j) valid_j
    (utils.py:13-17)."""
    valid = his > 0
    valid[:, 0] = True
    j = torch.arange(his.shape[1], device=his.device)
    return valid, (his_len.long().unsqueeze(-1) - j) * valid.long()


def sasrec_encode(rows: torch.Tensor, his: torch.Tensor, his_len: torch.Tensor, pos_w, wq, wk, w1,
                  b1, w2, b2, gamma, beta, eps: float, num_layers: int, dropout: float = 0.0,
                  training: bool = False, rnd=None) -> torch.Tensor:
    """The SASRec encoder (SASRec.py:83-110) in fp32 torch ops; autograd is its backward.

    rows [B, L, D] item rows of the padded history, his [B, L] ids, his_len [B] ->
    v [B, D] = sum_{valid j} X_j / his_len after ``num_layers`` passes of the ONE shared
    block  Q = X Wq^T, K = X Wk^T, A = softmax_k(D^-0.5 Q K^T) over valid keys,
    X <- LayerNorm(X + dropout(relu(A K W1^T + b1) W2^T + b2)).  The softmax shift is the
    row maximum (the reference's global ``attention.max()`` is the same softmax on paper
    and NaN when the global maximum sits far above every valid score of a row).

    ``rnd`` rounds X, the four weight matrices and every matmul operand (identity
    here; ``bf16_round`` on a GPU, where this is the layered path whose rounding
    points are the fused kernel's).  A position id outside the table is IndexError."""
    r = rnd if rnd is not None else (lambda t: t)
    B, L, D = rows.shape
    valid, pos = sasrec_positions(his, his_len)
    if pos.numel() and (int(pos.min()) < 0 or int(pos.max()) >= pos_w.shape[0]):
        raise IndexError("index out of range in self")
    x = r(rows.float() + pos_w.float().index_select(0, pos.reshape(-1)).reshape(B, L, D))
    wq, wk, w1, w2 = (r(w.float()) for w in (wq, wk, w1, w2))
    key_mask = ~valid.unsqueeze(1)  # [B, 1, L]: every query row sees the valid keys
    scale = D ** -0.5
    for _ in range(num_layers):
        q, k = r(x @ wq.t()), r(x @ wk.t())
        s = torch.bmm(q, k.transpose(1, 2)) * scale
        a = torch.softmax(s.masked_fill(key_mask, float("-inf")), dim=-1)
        c = r(torch.bmm(r(a), k))
        f = r(torch.relu(c @ w1.t() + b1.float()))
        g = f @ w2.t() + b2.float()
        if training and dropout > 0:
            g = torch.nn.functional.dropout(g, p=dropout, training=True)
        x = r(torch.nn.functional.layer_norm(x + g, (D,), gamma.float(), beta.float(), eps))
    v = (x * valid.unsqueeze(-1).float()).sum(1)
    return v / his_len.unsqueeze(-1).float()


def gru_encode(rows: torch.Tensor, his_len: torch.Tensor, w_ih, w_hh, b_ih, b_hh,
               rnd=None, check: bool = True) -> torch.Tensor:
    """The GRU4Rec encoder (GRU4Rec.py:51-56: one-layer nn.GRU over the packed history,
    h_-1 = 0) in fp32 torch ops; autograd is its backward.

    rows [B, L, E] item rows of the history, his_len [B] in 1..L -> h_{his_len - 1} [B, H]:
        r, z = sigmoid(W_i{r,z} x_t + b_i{r,z} + W_h{r,z} h + b_h{r,z})
        n    = tanh(W_in x_t + b_in + r (W_hn h + b_hn));   h <- (1 - z) n + z h
    Sample b runs exactly his_len[b] steps (a ``where`` past the length freezes h), which
    is all the reference's sort / pack / unsort does; the rows at t >= his_len never
    matter.  A length outside 1..L is IndexError (the reference cannot pack it); with
    ``check`` off it is not looked at: 0 gives h = 0, more than L runs L steps.

    ``rnd`` rounds x, the two weight matrices and h as a matmul operand (identity here;
    ``bf16_round`` on a GPU, where this is the layered path whose rounding points are the
    fused kernel's)."""
    r_ = rnd if rnd is not None else (lambda t: t)
    B, L, E = rows.shape
    H = w_hh.shape[1]
    lens = his_len.reshape(-1).long()
    if check and B and (int(lens.min()) < 1 or int(lens.max()) > L):
        raise IndexError("index out of range in self")
    x = r_(rows.float())
    wi, wh = r_(w_ih.float()), r_(w_hh.float())
    gx = x @ wi.t() + b_ih.float()  # [B, L, 3H]: the input products do not depend on h
    h = torch.zeros(B, H, dtype=torch.float32, device=rows.device)
    for t in range(L):
        gh = r_(h) @ wh.t() + b_hh.float()
        xr, xz, xn = gx[:, t].split(H, dim=1)
        hr, hz, hn = gh.split(H, dim=1)
        r = torch.sigmoid(xr + hr)
        z = torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        h = torch.where((lens > t).unsqueeze(1), (1.0 - z) * n + z * h, h)
    return h


def ncf_score(rows: torch.Tensor, E: int, weights, biases, wp, rnd=None, dropout: float = 0.0,
              training: bool = False) -> torch.Tensor:
    """The NCF / NeuMF pair scorer (NCF.py:62-74) in fp32 torch ops; autograd is its
    backward.

    rows [pairs, 4E] = [mf_u | mf_i | mlp_u | mlp_i] (one gather over the bank [users,
    items, users, items]) -> pred [pairs]:
        g = mf_u * mf_i;  h_0 = [mlp_u | mlp_i];  h_{l+1} = dropout(relu(W_l h_l + b_l))
        pred = wp . [g | h_k]
    ``weights`` / ``biases`` are the hidden layers' nn.Linear parameters, ``wp`` the
    bias-free prediction weight [1, E + width_k] (or flat).

    ``rnd`` rounds each weight matrix and each MLP operand h_l (identity here;
    ``bf16_round`` on a GPU, where this is the layered path whose rounding points are the
    fused kernel's: g, h_k and the final dot stay fp32)."""
    r = rnd if rnd is not None else (lambda t: t)
    x = rows.float()
    g = x[:, :E] * x[:, E:2 * E]
    h = x[:, 2 * E:4 * E]
    for w, b in zip(weights, biases):
        h = torch.relu(r(h) @ r(w.float()).t() + b.float())
        if training and dropout > 0:
            h = torch.nn.functional.dropout(h, p=dropout, training=True)
    return torch.cat([g, h], dim=1) @ wp.float().reshape(-1)


def fm2(v: torch.Tensor) -> torch.Tensor:
    s = v.sum(dim=1)
    return 0.5 * (s * s - (v * v).sum(dim=1)).sum(dim=-1)


def interact(bank, ids, dense: Optional[torch.Tensor], dense_w, bias, use_fm2: bool,
             first_order: bool, x0_cols: int, x0_dtype):
    w = _weight(bank)
    rows = _rows(bank, ids)
    g = [w.index_select(0, r) for r in rows]
    return interact_rows(g, bank.dim, dense, dense_w, bias, use_fm2, first_order, x0_cols,
                         x0_dtype)


def interact_rows(g: List[torch.Tensor], dim: int, dense: Optional[torch.Tensor], dense_w, bias,
                  use_fm2: bool, first_order: bool, x0_cols: int, x0_dtype):
    """The interaction on already-gathered rows g[f] = [B, >= dim(+1)] (also the
    row-sharded CPU path, whose rows arrive through the exchange)."""
    v = torch.stack([x[:, :dim] for x in g], dim=1).float()  # [B, F, D]
    B = v.shape[0]
    logit = torch.zeros(B, dtype=torch.float32)
    if bias is not None:
        logit = logit + bias.float()
    if dense is not None and dense_w is not None:
        logit = logit + dense.float() @ dense_w.float()
    if use_fm2:
        logit = logit + fm2(v)
    if first_order:
        logit = logit + torch.stack([x[:, dim] for x in g], dim=1).float().sum(1)
    if not x0_cols:
        return logit
    parts = [v.reshape(B, -1)]
    if dense is not None:
        parts.append(dense.float())
    x0 = torch.cat(parts, dim=1)
    if x0.shape[1] < x0_cols:
        x0 = torch.nn.functional.pad(x0, (0, x0_cols - x0.shape[1]))
    return x0.to(x0_dtype), logit


def topk_exclusion_pairs(offsets, items, rows, batch: int, device):
    """The (query, item) pairs of a top-k exclusion, flat: CSR ``offsets`` / ``items``,
    query b using CSR row ``rows[b]`` (``b`` when None); a row index outside the CSR
    excludes nothing.  -> (query index int64 [P], item id int64 [P])."""
    off = offsets.to(device=device, dtype=torch.int64)
    n_rows = off.numel() - 1
    r = (torch.arange(batch, device=device) if rows is None
         else rows.to(device=device, dtype=torch.int64).reshape(-1))
    ok = (r >= 0) & (r < n_rows)
    rc = torch.where(ok, r, torch.zeros_like(r))
    start = off[rc]
    length = torch.where(ok, off[rc + 1] - start, torch.zeros_like(start))
    qidx = torch.repeat_interleave(torch.arange(batch, device=device), length)
    first = torch.cumsum(length, 0) - length
    pos = torch.arange(qidx.numel(), device=device) - first[qidx] + start[qidx]
    return qidx, items.to(device)[pos].to(torch.int64)


def topk(rows, dim: int, q, k: int, low: int, high: int, use_w: bool, exclude=None,
         chunk: int = 8192, round_bf16: bool = True):
    """``mrec_topk`` in torch ops (include/mrec.h "Retrieval"): the k best items of
    ``[low, high)`` per query by score descending, then id ascending, with the kernel's
    eligibility, exclusion and padding rules.  ``rows`` is the table ``[items,
    row_stride]`` (``[v(dim) | w | pad]``, on any device: it is read ``chunk`` rows at a
    time), ``exclude`` an ``(offsets, items, rows)`` triple or None.  Chunked over the
    items with a running merge: never more than ``[B, chunk]`` scores exist.
    ``round_bf16=False`` keeps q and the rows in fp32 (a CPU bank: what the CPU forward
    of a model computes, which never rounds).
    -> (ids int32 [B, k], scores float32 [B, k]) on q's device."""
    dev = q.device
    B = q.shape[0]
    def operand(t):
        return t.to(torch.bfloat16).float() if round_bf16 else t.float()

    qb = operand(q.detach()[:, :dim])
    neg_inf = float("-inf")
    best_s = torch.full((B, k), neg_inf, dtype=torch.float32, device=dev)
    best_i = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    pairs = None
    if exclude is not None and B > 0:
        pairs = topk_exclusion_pairs(exclude[0], exclude[1], exclude[2], B, dev)
    chunk = max(1, int(chunk))
    for c0 in range(low, high, chunk):
        c1 = min(high, c0 + chunk)
        blk = rows[c0:c1].detach().to(dev)
        s = qb @ operand(blk[:, :dim]).t()
        if use_w:
            s = s + blk[:, dim].float().unsqueeze(0)
        best_s, best_i = topk_fold(best_s, best_i, s, c0, pairs)
    return topk_finish(best_s, best_i)


def ncf_topk(tables, E: int, uid, weights, biases, wp, k: int, low: int, high: int, exclude=None,
             chunk: int = 8192, round_bf16: bool = True):
    """``mrec_ncf_topk`` in torch ops (include/mrec.h "NCF retrieval"): the k best items of
    ``[low, high)`` per user under the NeuMF scorer, with layer 0 split as the kernel
    splits it -- ``a = b_0 + W_0[:, :E] mlp_u`` once per user, ``c = W_0[:, E:] mlp_i`` once
    per item, ``h_1 = relu(a + c)`` -- and ``mrec_topk``'s selection rules.  ``tables`` are
    the four tables ``(mf_u, mf_i, mlp_u, mlp_i)`` as ``[rows, >= E]`` views on any device
    (the item tables are read ``chunk`` rows at a time), ``weights`` / ``biases`` / ``wp``
    as for ``ncf_score``, ``exclude`` an ``(offsets, items, rows)`` triple or None.  Chunked
    over the items with a running merge (``topk_fold``); the chunk shrinks so that the
    ``[B, chunk, width]`` activations stay small.  ``round_bf16`` applies the kernel's
    rounding points (table elements, weight matrices, each h_l that feeds a layer);
    False keeps fp32 throughout, which is what the CPU forward computes.  The ReLU is the
    kernels' ``x > 0 ? x : 0``: a NaN pre-activation gives 0, so only a NaN in the MF term
    makes a score NaN (and the item ineligible).
    -> (ids int32 [B, k], scores float32 [B, k]) on uid's device."""
    dev = uid.device
    B = int(uid.shape[0])
    r = bf16_round if round_bf16 else (lambda t: t)

    def relu(x):
        return torch.where(x > 0, x, torch.zeros_like(x))

    mf_u, mf_i, mlp_u, mlp_i = tables
    ws = [r(w.detach().float()).to(dev) for w in weights]
    bs = [b.detach().float().to(dev) for b in biases]
    wp = wp.detach().float().reshape(-1).to(dev)
    idx = uid.to(device=mf_u.device, dtype=torch.int64)
    mu = r(mf_u.detach()[idx, :E].float()).to(dev)
    a = r(mlp_u.detach()[idx, :E].float()).to(dev) @ ws[0][:, :E].t() + bs[0]
    best_s = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
    best_i = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    pairs = None
    if exclude is not None and B > 0:
        pairs = topk_exclusion_pairs(exclude[0], exclude[1], exclude[2], B, dev)
    widest = max([E] + [int(w.shape[0]) for w in ws])
    chunk = max(1, min(int(chunk), (1 << 24) // max(1, B * widest)))
    for c0 in range(low, high, chunk):
        c1 = min(high, c0 + chunk)
        g = mu.unsqueeze(1) * r(mf_i.detach()[c0:c1, :E].float()).to(dev).unsqueeze(0)
        c = r(mlp_i.detach()[c0:c1, :E].float()).to(dev) @ ws[0][:, E:].t()
        h = relu(a.unsqueeze(1) + c.unsqueeze(0))
        for w, b in zip(ws[1:], bs[1:]):
            h = relu(r(h) @ w.t() + b)
        s = g @ wp[:E] + h @ wp[E:]
        best_s, best_i = topk_fold(best_s, best_i, s, c0, pairs)
    return topk_finish(best_s, best_i)


def topk_fold(best_s, best_i, s, c0: int, pairs=None):
    """Fold the scores ``s [B, n]`` of items ``c0 .. c0 + n - 1`` into the running lists
    ``(best_s, best_i) [B, k]`` of a scan in ascending id order.  NaN scores and the
    excluded ``pairs`` (``topk_exclusion_pairs``) drop to -inf."""
    B, n = s.shape
    k = best_s.shape[1]
    neg_inf = float("-inf")
    s = torch.where(torch.isnan(s), torch.full_like(s, neg_inf), s) + 0.0  # (-0.0 -> +0.0)
    if pairs is not None:
        qidx, it = pairs
        m = (it >= c0) & (it < c0 + n)
        s[qidx[m], it[m] - c0] = neg_inf
    ids = torch.arange(c0, c0 + n, device=s.device).unsqueeze(0).expand(B, n)
    # kept ids are below the chunk's and ties within each part are in id order: a
    # stable descending sort of [kept | chunk] is the total order
    cs, order = torch.sort(torch.cat([best_s, s], 1), dim=1, descending=True, stable=True)
    return cs[:, :k].contiguous(), torch.gather(torch.cat([best_i, ids], 1), 1, order[:, :k])


def topk_finish(best_s, best_i):
    """-> (ids int32, scores float32): a slot whose score is -inf is padding, id -1."""
    best_i = torch.where(best_s == float("-inf"), torch.full_like(best_i, -1), best_i)
    return best_i.to(torch.int32), best_s


SHNEG_KINDS = ("softmax", "bpr", "top1")


def shared_negative_loss(q, pos, neg, kind: str, reduction: str = "mean", pos_id=None, neg_id=None,
                         pos_bias=None, neg_bias=None, round_bf16: bool = False):
    """``mrec_shneg_loss_fwd`` / ``_bwd`` in differentiable torch ops (include/mrec.h "Shared
    negatives"): every query ``q [B, D]`` ranked against its own positive row ``pos [B, D]``
    and one pool ``neg [S, D]`` shared by the batch; candidate j is masked for query b iff
    ``neg_id[j] == pos_id[b]``; the biases are constants added to the scores (no gradient).
    Arithmetic in fp32 (fp64 operands stay fp64), which is what the models' CPU forward
    computes; ``round_bf16`` rounds q and the rows to bf16 first, the kernel's operands (a
    GPU shape the kernel does not cover).  A candidate masked for every query is replaced
    by zeros, so whatever its row holds it changes nothing and gets a zero gradient.
    -> ``[B]`` for ``none``, else a scalar."""
    if kind not in SHNEG_KINDS:
        raise ValueError(f"kind must be one of {SHNEG_KINDS}, got {kind!r}")
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"reduction参数不合法: {reduction}")
    if (pos_id is None) != (neg_id is None):
        raise ValueError("pos_id and neg_id go together")
    dt = torch.float64 if q.dtype == torch.float64 else torch.float32
    qf, pf, nf = q.to(dt), pos.to(dt), neg.to(dt)
    if round_bf16:
        qf, pf, nf = bf16_round(qf), bf16_round(pf), bf16_round(nf)
    B, S = qf.shape[0], nf.shape[0]
    if pos_id is not None:
        mask = neg_id.reshape(1, S).to(torch.int64) == pos_id.reshape(B, 1).to(torch.int64)
        if B:
            nf = torch.where(mask.all(0).unsqueeze(1), torch.zeros_like(nf), nf)
    else:
        mask = torch.zeros(B, S, dtype=torch.bool, device=qf.device)
    s = qf @ nf.t()
    sp = (qf * pf).sum(1)
    if neg_bias is not None:
        s = s + neg_bias.detach().to(dt).reshape(1, S)
    if pos_bias is not None:
        sp = sp + pos_bias.detach().to(dt).reshape(B)
    s = torch.where(mask, torch.zeros_like(s), s)  # (a masked score is never looked at)
    n = (~mask).sum(1)
    if kind == "softmax":
        logits = torch.cat([sp.unsqueeze(1), s.masked_fill(mask, float("-inf"))], dim=1)
        loss = torch.logsumexp(logits, dim=1) - sp
    else:
        x = s - sp.unsqueeze(1)
        if kind == "bpr":
            t = torch.nn.functional.softplus(x)
        else:
            t = torch.sigmoid(x) + torch.sigmoid(s * s)
        loss = torch.where(mask, torch.zeros_like(t), t).sum(1) / n.clamp(min=1).to(dt)
    if reduction == "none":
        return loss
    return loss.sum() / max(B, 1) if reduction == "mean" else loss.sum()


def dot_interact(bot, rows, F: int, D: int, x_cols: Optional[int] = None, round_bf16: bool = False,
                 x_dtype=None):
    """``mrec_dot_interact_fwd`` / ``_bwd`` in differentiable torch ops (include/mrec.h "DLRM
    dot interaction"): per sample the n = F + 1 vectors t_0 = ``bot [B, D]``, t_i = field i - 1
    of ``rows [B, F * D]`` (``bot`` None: the F rows alone) ->
    ``x [B, x_cols] = [t_0 | t_i . t_j for 0 <= j < i < n | 0 pad]``, the pairs in the order of
    ``torch.tril_indices(n, n, -1)``; ``x_cols`` None is D + P exactly.  Arithmetic in fp32
    (fp64 operands stay fp64), which is what the model's CPU forward computes; ``round_bf16``
    rounds the operands of the products to bf16 first (identity gradient), the kernel's operand
    rounding: the GPU path of a shape the kernel does not cover, and its comparator.  The copy
    of t_0 is never rounded.  Autograd is the backward: G symmetric with a zero diagonal times
    the (rounded) vectors, plus dx[:, :D] for ``bot``.  -> x in ``x_dtype`` (None: the
    arithmetic's)."""
    dt = torch.float64 if rows.dtype == torch.float64 else torch.float32
    B = rows.shape[0]
    t = rows[:, :F * D].to(dt).reshape(B, F, D)
    head = []
    if bot is not None:
        b0 = bot[:, :D].to(dt)
        head = [b0]
        t = torch.cat([b0.unsqueeze(1), t], dim=1)
    n = t.shape[1]
    tb = bf16_round(t) if round_bf16 else t
    z = torch.bmm(tb, tb.transpose(1, 2))
    li, lj = torch.tril_indices(n, n, -1, device=rows.device)
    x = torch.cat(head + [z[:, li, lj]], dim=1)
    if x_cols is not None:
        if x_cols < x.shape[1]:
            raise ValueError(f"x_cols = {x_cols} is smaller than D + P = {x.shape[1]}")
        if x_cols > x.shape[1]:
            x = torch.nn.functional.pad(x, (0, x_cols - x.shape[1]))
    return x if x_dtype is None else x.to(x_dtype)


def _cin_layer(x0c, xpc, W, r):
    """One CIN layer on a batch chunk: x0c [b, m, D], xpc [b, Hp, D], W [H, Hp, m] ->
    X^k [b, H, D], through Z [b, Hp * m, D] rounded by ``r``."""
    b, m, D = x0c.shape
    Z = r((xpc.unsqueeze(2) * x0c.unsqueeze(1)).reshape(b, -1, D))
    return torch.matmul(W.reshape(W.shape[0], -1), Z)


class _CinFn(torch.autograd.Function):
    """The CIN in torch ops, forward and backward chunked over the batch so that the outer
    product Z [chunk, H_prev * m, D] exists for one chunk at a time (the backward re-forms
    it).  ``rnd`` (None or ``bf16_round``) is applied to x0, W, every X^{k-1} that enters a
    product, Z and dX^k: the kernels' rounding points.  ``store`` rounds X^k where the
    kernels store it in bf16."""

    @staticmethod
    def forward(ctx, x0, m, chunk, rnd, store, *weights):
        B = x0.shape[0]
        D = x0.shape[1] // m
        dt = torch.float64 if x0.dtype == torch.float64 else torch.float32
        r = rnd if rnd is not None else (lambda t: t)
        st = store if store is not None else (lambda t: t)
        Ws = [r(w.detach().to(dt)) for w in weights]
        xs = [torch.empty(B, w.shape[0], D, dtype=dt, device=x0.device) for w in Ws]
        x0r = r(x0.detach().to(dt).reshape(B, m, D))
        p = torch.empty(B, sum(w.shape[0] for w in Ws), dtype=dt, device=x0.device)
        for s in range(0, B, chunk):
            xp, off = x0r[s:s + chunk], 0
            for k, W in enumerate(Ws):
                xk = _cin_layer(x0r[s:s + chunk], xp, W, r)
                p[s:s + chunk, off:off + W.shape[0]] = xk.sum(2)  # from the unrounded sums
                off += W.shape[0]
                xs[k][s:s + chunk] = st(xk)
                xp = r(xs[k][s:s + chunk])
        ctx.save_for_backward(x0r, *xs)
        ctx.Ws, ctx.m, ctx.chunk, ctx.r = Ws, m, chunk, r
        ctx.in_dtypes = (x0.dtype, [w.dtype for w in weights])
        return p

    @staticmethod
    def backward(ctx, dp):
        x0r, *xs = ctx.saved_tensors
        Ws, m, chunk, r = ctx.Ws, ctx.m, ctx.chunk, ctx.r
        B, _, D = x0r.shape
        dt = x0r.dtype
        dp = dp.to(dt)
        offs = [0]
        for W in Ws:
            offs.append(offs[-1] + W.shape[0])
        dx0 = torch.zeros_like(x0r)
        dWs = [torch.zeros_like(W) for W in Ws]
        for s in range(0, B, chunk):
            x0c = x0r[s:s + chunk]
            b = x0c.shape[0]
            dxk = None
            for k in range(len(Ws) - 1, -1, -1):
                W = Ws[k]
                H, Hp = W.shape[0], W.shape[1]
                g = dp[s:s + chunk, offs[k]:offs[k + 1]].unsqueeze(2).expand(b, H, D)
                g = r(g if dxk is None else dxk + g)
                xp = x0c if k == 0 else r(xs[k - 1][s:s + chunk])
                Z = r((xp.unsqueeze(2) * x0c.unsqueeze(1)).reshape(b, Hp * m, D))
                dWs[k] += torch.einsum("bhd,bnd->hn", g, Z).reshape(H, Hp, m)
                dZ = torch.matmul(W.reshape(H, -1).t(), g).reshape(b, Hp, m, D)
                dx0[s:s + chunk] += (dZ * xp.unsqueeze(2)).sum(1)
                dxk = (dZ * x0c.unsqueeze(1)).sum(2)
            dx0[s:s + chunk] += dxk
        x_dt, w_dts = ctx.in_dtypes
        return (dx0.reshape(B, m * D).to(x_dt), None, None, None, None,
                *[g.to(t) for g, t in zip(dWs, w_dts)])


def cin(x0, weights, round_bf16: bool = False, x_dtype=None, chunk: int = 256):
    """``mrec_cin_fwd`` / ``_bwd`` over all layers in torch ops (include/mrec.h "CIN"):
    ``x0 [B, m * D]`` read as [B, m, D] (a strided column slice is fine), ``weights[k - 1]`` =
    W^k ``[H_k, H_{k-1}, m]`` with H_0 = m ->  ``p [B, sum_k H_k]``,
    p[b, off_k + h] = sum_d X^k[b, h, d],  X^k[b, h, d] = sum_{i, j} W^k[h, i, j] X^{k-1}[b, i, d]
    X^0[b, j, d]: identity activation, no bias, every map feeds the output and the next layer.
    Arithmetic in fp32 (fp64 operands stay fp64).  The outer product Z exists for ``chunk``
    samples at a time, in the forward and in the backward, which re-forms it.  ``round_bf16``
    rounds where the kernels round (operands, Z, dX^k; X^k too when ``x_dtype`` is bf16): the
    GPU path of a shape the kernels do not cover, and their comparator."""
    weights = list(weights)
    if not weights:
        raise ValueError("cin needs at least one layer")
    m = weights[0].shape[2]
    if x0.dim() != 2 or x0.shape[1] % m:
        raise ValueError(f"x0 must be [B, m * D] with m = {m} fields, got {tuple(x0.shape)}")
    hp = m
    for w in weights:
        if w.dim() != 3 or w.shape[1] != hp or w.shape[2] != m:
            raise ValueError(f"CIN weight must be [H, {hp}, {m}], got {tuple(w.shape)}")
        hp = w.shape[0]
    rnd = bf16_round_any if round_bf16 else None
    store = bf16_round_any if (round_bf16 and x_dtype == torch.bfloat16) else None
    return _CinFn.apply(x0, m, int(chunk), rnd, store, *weights)


def bf16_round_any(t: torch.Tensor) -> torch.Tensor:
    """nearest bf16 of a detached fp32 / fp64 tensor, in its own dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _ste(rnd):
    """``rnd`` as a straight-through rounding: the value is rounded, the gradient passes."""
    if rnd is None:
        return lambda t: t
    return lambda t: t + (rnd(t.detach()) - t.detach())


def _autoint_layer(X, Wq, Wk, Wv, Wres, heads, scale, r, st):
    """One interacting layer on a batch chunk: X [b, m, d_in] and the weights [A, d_in], both
    already rounded -> Y [b, m, A].  ``r`` rounds Q, K, V and P, ``st`` rounds Y."""
    b, m, _ = X.shape
    A = Wq.shape[0]
    hd = A // heads
    q = r(X @ Wq.t()).view(b, m, heads, hd).transpose(1, 2)
    k = r(X @ Wk.t()).view(b, m, heads, hd).transpose(1, 2)
    v = r(X @ Wv.t()).view(b, m, heads, hd).transpose(1, 2)
    P = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)  # shifted by the row's maximum
    O = (r(P) @ v).transpose(1, 2).reshape(b, m, A)
    if Wres is not None:
        O = O + X @ Wres.t()
    return st(torch.relu(O))


def _autoint_stack(xc, m, flat, has_res, heads, scale, rnd, store):
    """All layers on a chunk: xc [b, m * d_in] -> [b, m * A_last], in xc's arithmetic dtype."""
    r, st = _ste(rnd), _ste(store)
    X = r(xc.reshape(xc.shape[0], m, -1))
    it = iter(flat)
    for k, res in enumerate(has_res):
        Wq, Wk, Wv = r(next(it)), r(next(it)), r(next(it))
        Wres = r(next(it)) if res else None
        Y = _autoint_layer(X, Wq, Wk, Wv, Wres, heads, scale, r, st)
        X = r(Y) if k + 1 < len(has_res) else Y
    return X.reshape(X.shape[0], -1)


class _AutoIntFn(torch.autograd.Function):
    """The interacting stack in torch ops, forward and backward chunked over the batch: the
    [chunk, heads, m, m] scores exist for one chunk at a time, and the backward recomputes
    them from x0 (nothing else is kept), as the kernels do."""

    @staticmethod
    def forward(ctx, x0, meta, *flat):
        m, has_res, heads, scale, chunk, rnd, store = meta
        dt = torch.float64 if x0.dtype == torch.float64 else torch.float32
        ws = [w.detach().to(dt) for w in flat]
        xs = x0.detach().to(dt).contiguous()
        with torch.no_grad():
            ys = [_autoint_stack(xs[s:s + chunk], m, ws, has_res, heads, scale, rnd, store)
                  for s in range(0, x0.shape[0], chunk)]
        A = flat[-(4 if has_res[-1] else 3)].shape[0]  # the last layer's Wq
        y = torch.cat(ys) if ys else xs.new_zeros(0, m * A)
        ctx.save_for_backward(x0, *flat)
        ctx.meta = meta
        return y

    @staticmethod
    def backward(ctx, dy):
        x0, *flat = ctx.saved_tensors
        m, has_res, heads, scale, chunk, rnd, store = ctx.meta
        dt = torch.float64 if x0.dtype == torch.float64 else torch.float32
        ws = [w.detach().to(dt).requires_grad_(True) for w in flat]
        dx = torch.zeros(x0.shape, dtype=dt, device=x0.device)
        dws = [torch.zeros_like(w) for w in ws]
        dy = _ste(rnd)(dy.detach().to(dt))
        for s in range(0, x0.shape[0], chunk):
            with torch.enable_grad():
                xc = x0[s:s + chunk].detach().to(dt).contiguous().requires_grad_(True)
                y = _autoint_stack(xc, m, ws, has_res, heads, scale, rnd, store)
                gs = torch.autograd.grad(y, [xc] + ws, dy[s:s + chunk])
            dx[s:s + chunk] = gs[0]
            for a, g in zip(dws, gs[1:]):
                a += g
        return (dx.to(x0.dtype), None, *[g.to(w.dtype) for g, w in zip(dws, flat)])


def autoint(x0, layers, heads: int, scale: float = 1.0, round_bf16: bool = False, x_dtype=None,
            chunk: int = 256):
    """``mrec_autoint_fwd`` / ``_bwd`` over all layers in torch ops (include/mrec.h
    "AutoInt"): ``x0 [B, m * d_in]`` read as [B, m, d_in] (a strided column slice is fine),
    ``layers[k]`` = ``(Wq, Wk, Wv, Wres or None)`` in nn.Linear layout ``[A_k, A_(k-1)]`` ->
    ``[B, m * A_last]``.  Per layer Q, K, V = X W^T split into ``heads`` heads, P = softmax over
    the keys of scale * Q_h K_h^T, Y = relu([P_h V_h] + X Wres^T).  Arithmetic in fp32 (fp64
    operands stay fp64).  The scores exist for ``chunk`` samples at a time in both directions;
    the backward recomputes them.  ``round_bf16`` rounds exactly where the kernels' forward
    rounds: the operands (X, the weights, dY), Q K V, P, and Y when ``x_dtype`` is bf16; S, the
    softmax and O + X Wres^T stay unrounded.  The result comes in ``x_dtype`` (default: x0's).
    The GPU path of a shape the kernels do not cover, and their comparator."""
    layers = [tuple(l) for l in layers]
    if not layers:
        raise ValueError("autoint needs at least one layer")
    d_in = layers[0][0].shape[1]
    if x0.dim() != 2 or x0.shape[1] % d_in:
        raise ValueError(f"x0 must be [B, m * {d_in}], got {tuple(x0.shape)}")
    m, heads = x0.shape[1] // d_in, int(heads)
    flat, has_res, d = [], [], d_in
    for l in layers:
        if len(l) != 4:
            raise ValueError("a layer is (Wq, Wk, Wv, Wres or None)")
        A = l[0].shape[0]
        if heads < 1 or A % heads:
            raise ValueError(f"heads = {heads} does not divide the layer width {A}")
        for w in l:
            if w is not None and tuple(w.shape) != (A, d):
                raise ValueError(f"AutoInt weight must be [{A}, {d}], got {tuple(w.shape)}")
        flat += [w for w in l if w is not None]
        has_res.append(l[3] is not None)
        d = A
    rnd = bf16_round_any if round_bf16 else None
    store = bf16_round_any if (round_bf16 and x_dtype == torch.bfloat16) else None
    meta = (m, tuple(has_res), heads, float(scale), int(chunk), rnd, store)
    y = _AutoIntFn.apply(x0, meta, *flat)
    return y.to(x_dtype or x0.dtype)
