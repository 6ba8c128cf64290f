"""Float64 restatements of the causal sequence head and of training on every position (--seqAtt causal, --seqTargets
all), written from the contract and not from the kernels.

  causal attention on one slot's n tokens: e[j, s] = exp(q_j k_s / sqrt(d_k)) for s <= j only,
      a = e / (sum_{s <= j} e + 1e-8), ctx_j = sum_{s <= j} a[j, s] v_s
  every prefix a query: pre[b, j] = sum_{i <= j} x[b, i], Q[b, j] = leaky(pre[b, j]) + fu[u_b]
  targets: tgt[b, j] = s_{j+1} for j < n_b - 1, t_b for j = n_b - 1; -1 in the padding and in slots without a positive
  preLoss = sum over the rows with a target of (lse - z at the target) / their count, the eligible set of row (b, j) the
      one --predLoss softmax uses for user u_b

Two independent forms of the attention: the ragged one (a loop over slots, numpy and torch) and the dense one (all P
positions, P x P scores times the key mask times a lower-triangular mask; torch). Layer norm, leaky and the rest of
the objective are the oracle's and seq_att_ref's own functions."""
import numpy as np
import torch

import seq_att_ref as A
import softmax_cand_ref as C
import softmax_loss_ref as S
import softmax_pop_ref as Pop
from oracle import selfgnn_oracle as O


# ---- causal attention on one slot's tokens ---------------------------------------------------------------------------
def attn_tokens_np(q, k, v, heads):
    """q, k, v [n, d] -> (ctx [n, d], sum_{s <= j} |a[j, s] v_s| [n, d])."""
    n, d = q.shape
    dk = d // heads
    qh, kh, vh = (z.reshape(n, heads, dk).transpose(1, 0, 2) for z in (q, k, v))
    e = np.exp(qh @ kh.transpose(0, 2, 1) / np.sqrt(dk)) * np.tril(np.ones((n, n)))
    a = e / (e.sum(-1, keepdims=True) + 1e-8)
    merge = lambda z: z.transpose(1, 0, 2).reshape(n, d)
    return merge(a @ vh), merge(a @ np.abs(vh))


def attn_tokens_t(q, k, v, heads):
    """Token by token: row j over the keys 0..j, nothing else evaluated (differentiable torch)."""
    n, d = q.shape
    dk = d // heads
    qh, kh, vh = (z.reshape(n, heads, dk).permute(1, 0, 2) for z in (q, k, v))
    rows = []
    for j in range(n):
        e = torch.exp((qh[:, j:j + 1] @ kh[:, :j + 1].transpose(-1, -2)) / float(np.sqrt(dk)))       # [heads, 1, j + 1]
        a = e / (e.sum(-1, keepdim=True) + 1e-8)
        rows.append((a @ vh[:, :j + 1]).permute(1, 0, 2).reshape(d))
    return torch.stack(rows, 0)


def seq_attn_np(qkv, lens, P, heads):
    """The slab form of sagnn_seq_attn_masked_f32 with causal = 1: qkv [n_slots * P, 3d] float64 -> (ctx, term sums)."""
    d = qkv.shape[1] // 3
    ctx, terms = np.zeros((len(lens) * P, d)), np.zeros((len(lens) * P, d))
    for b, n in enumerate(lens):
        if n:
            r = qkv[b * P:b * P + n]
            ctx[b * P:b * P + n], terms[b * P:b * P + n] = attn_tokens_np(r[:, :d], r[:, d:2 * d], r[:, 2 * d:], heads)
    return ctx, terms


def seq_attn_t(qkv, lens, P, heads):
    """seq_attn_np in differentiable torch (float64), token by token."""
    d = qkv.shape[1] // 3
    rows = []
    for b, n in enumerate(lens):
        if n:
            r = qkv[b * P:b * P + n]
            rows.append(attn_tokens_t(r[:, :d], r[:, d:2 * d], r[:, 2 * d:], heads))
        rows.append(torch.zeros((P - n, d), dtype=qkv.dtype))
    return torch.cat(rows, 0)


def seq_attn_dense_t(qkv, lens, P, heads, causal=True):
    """The dense form: all P positions of every slot, P x P scores times the key mask (attn_mask of
    Utils/attention.py:40-41) and, causal, a lower-triangular mask; padded query rows zeroed at the end."""
    d = qkv.shape[1] // 3
    dk = d // heads
    B = len(lens)
    m = torch.as_tensor(np.arange(P)[None, :] < np.asarray(lens)[:, None], dtype=qkv.dtype)               # [B, P]
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, P, heads, dk).permute(0, 2, 1, 3) for i in range(3))
    mask = m[:, None, None, :]
    if causal:
        mask = mask * torch.tril(torch.ones((P, P), dtype=qkv.dtype))[None, None]
    scores = torch.exp(q @ k.transpose(-1, -2) / float(np.sqrt(dk))) * mask
    a = scores / (scores.sum(-1, keepdim=True) + 1e-8)
    return ((a @ v).permute(0, 2, 1, 3).reshape(B, P, d) * m[:, :, None]).reshape(B * P, d)


# ---- every prefix a query ----------------------------------------------------------------------------------------
def prefix_query_np(x, U, lens, P, leaky):
    """(Q [n_slots * P, d], sum of |terms| of the prefix sums plus |U|): zero rows in the padding."""
    d = x.shape[1]
    Q, terms = np.zeros((len(lens) * P, d)), np.zeros((len(lens) * P, d))
    for b, n in enumerate(lens):
        pre = np.cumsum(x[b * P:b * P + n], 0)
        Q[b * P:b * P + n] = O.leaky_relu(pre, leaky) + U[b]
        terms[b * P:b * P + n] = np.cumsum(np.abs(x[b * P:b * P + n]), 0) + np.abs(U[b])
    return Q, terms


def prefix_query_t(x, U, lens, P, leaky):
    d = x.shape[1]
    rows = []
    for b, n in enumerate(lens):
        if n:
            rows.append(A._lk_t(torch.cumsum(x[b * P:b * P + n], 0), leaky) + U[b])
        rows.append(torch.zeros((P - n, d), dtype=x.dtype))
    return torch.cat(rows, 0)


def prefix_query_bwd_np(x, dQ, lens, P, leaky):
    """(dx, dU, sum |terms| of dx, sum |terms| of dU) by the closed form: dx[b, i] = sum_{j >= i} dQ[b, j] slope(pre[b, j]),
    dU[b] = sum_j dQ[b, j]; slope = leaky where leaky * pre >= pre (the gradient goes to the first argument on ties)."""
    d = x.shape[1]
    dx, tx = np.zeros((len(lens) * P, d)), np.zeros((len(lens) * P, d))
    dU, tu = np.zeros((len(lens), d)), np.zeros((len(lens), d))
    for b, n in enumerate(lens):
        pre = np.cumsum(x[b * P:b * P + n], 0)
        t = dQ[b * P:b * P + n] * np.where(leaky * pre >= pre, leaky, 1.0)
        dx[b * P:b * P + n] = np.cumsum(t[::-1], 0)[::-1]
        tx[b * P:b * P + n] = np.cumsum(np.abs(t)[::-1], 0)[::-1]
        dU[b], tu[b] = dQ[b * P:b * P + n].sum(0), np.abs(dQ[b * P:b * P + n]).sum(0)
    return dx, dU, tx, tu


def seq_targets_np(items, seg_begin, seg_len, slot_user, slot_target, P, n_items):
    """(target, excl_row) int64 [n_slots * P] of sagnn_seq_targets_i32's contract."""
    items = np.asarray(items, dtype=np.int64)
    B = len(seg_len)
    target = np.full(B * P, -1, dtype=np.int64)
    for b in range(B):
        n = min(max(int(seg_len[b]), 0), P)
        if slot_target[b] < 0:
            continue
        for j in range(n):
            if j == n - 1:
                t = int(slot_target[b])
            else:
                e = int(seg_begin[b]) + j + 1
                t = int(items[e]) if 0 <= e < len(items) else -1
            target[b * P + j] = t if 0 <= t < n_items else -1
    return target, np.repeat(np.asarray(slot_user, dtype=np.int64), P)


def slot_targets(seq_items, positive):
    """The hand form for one slot: items s_0..s_{n-1} and positive t -> [s_1, ..., s_{n-1}, t]."""
    return list(seq_items[1:]) + [positive] if len(seq_items) else []


# ---- the head and the objective --------------------------------------------------------------------------------------
def torch_head_slabs(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky, attn=attn_tokens_t):
    """Per batch slot the last attention layer's rows x [n_b, d] (None for an empty slot), under causal attention."""
    out = []
    for it, p in A.slot_tokens(sequence, mask):
        if not len(it):
            out.append(None)
            continue
        x = A._ln_t(fi[torch.as_tensor(it)], ln_params[0]) + A._ln_t(pos_embed[torch.as_tensor(p)], ln_params[1])
        for i, w in enumerate(att_params):
            y = A._ln_t(x, ln_params[2 + i])
            x = A._lk_t(attn(y @ w["Wq"] + w["bq"], y @ w["Wk"] + w["bk"], y @ w["Wv"] + w["bv"], heads), leaky) + x
        out.append(x)
    return out


def torch_head_causal(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
    """att_user [B, d] under --seqAtt causal --seqPool sum: the sum of the slot's rows (an empty slot: zeros)."""
    slabs = torch_head_slabs(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky)
    return torch.stack([torch.zeros(fi.shape[1], dtype=fi.dtype) if x is None else x.sum(0) for x in slabs], 0)


def all_rows(batch):
    """The query rows of --seqTargets all for a host batch: (slot, token, user, target) int64 arrays, slot-major."""
    slots, users, targets = S.slot_triples(batch)
    tokens = A.slot_tokens(batch["sequence"], batch["mask"])
    rows = []
    for b, u, t in zip(slots, users, targets):
        it = tokens[b][0]
        rows += [(b, j, u, tg) for j, tg in enumerate(slot_targets(list(it), t))]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


def torch_train_loss_all(P, adj_list, tp_list, batch, cfg, banned, cand=None, bias=None):
    """The training objective under --seqAtt causal --seqTargets all --predLoss softmax in differentiable torch float64.
    cand (and bias): the step's candidate list (and its logQ offsets), None for the full catalogue. Returns
    (preLoss, sslloss, number of loss terms)."""
    _, ssl, fu, fi = O.torch_train_loss(P, adj_list, tp_list, batch, cfg)
    leaky, heads = cfg["leaky"], cfg["heads"]
    slabs = torch_head_slabs(fi, P["posEmbed"], P["ln"], P["att"], batch["sequence"], batch["mask"], heads, leaky)
    rows = all_rows(batch)
    if not len(rows):
        return (fu.sum() + fi.sum()) * 0.0, ssl, 0
    pre = {b: torch.cumsum(slabs[b], 0) for b in np.unique(rows[:, 0])}
    q = torch.stack([A._lk_t(pre[b][j], leaky) + fu[u] for b, j, u, _ in rows], 0)
    users, targets = rows[:, 2], rows[:, 3]
    n_items, inv_temp = fi.shape[0], 1.0 / cfg.get("temp", 1.0)
    if cand is None:
        el = S.eligible(len(rows), n_items, targets, banned[0], banned[1], users)
        loss = S.torch_softmax_loss(q, fi, targets, inv_temp, 1.0 / len(rows), el)
    else:
        ids, off = (np.asarray(cand, dtype=np.int64), np.zeros(n_items)) if bias is None else Pop.item_offsets(n_items, cand, bias)
        ptr, items = C.augmented(len(rows), n_items, ids, banned[0], banned[1], users)
        el = S.eligible(len(rows), n_items, targets, ptr, items, None)
        offm = np.broadcast_to(off, el.shape).copy()
        offm[np.arange(len(rows)), targets] = 0.0
        loss = Pop.torch_softmax_loss_pop(q, fi, targets, inv_temp, 1.0 / len(rows), el, offm)
    return loss.reshape(()), ssl, len(rows)
