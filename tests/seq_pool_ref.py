"""Float64 restatements of the additive-attention pooling of the sequence head (--seqPool additive),
written from the contract and not from the kernels. Slot b has n_b real tokens x_j (rows b * P + j of the slab):

  u_j = x_j Wa + ba,  t_j = tanh(u_j),  s_j = sum_c t_j[c] v[c],  w = softmax over j < n_b of s,
  att_user[b] = sum_{j < n_b} w_j x_j                                                      (an empty slot: zeros)

Two independent forms: the ragged one (a loop over slots on their real tokens only, numpy and torch) and the dense one
(all P positions of every slot, the mask applied to the scores as -inf before the softmax and to the pooled sum;
torch). The head that ends in it is seq_att_ref.torch_head_ragged's with the sum replaced."""
import numpy as np
import torch

import seq_att_ref as R


def addpool_np(x, Wa, ba, v, lens, P):
    """The slab form: x [n_slots * P, d] float64 -> (out [n_slots, d], w [n_slots * P] with zeros in the padding,
    term sums sum_j w_j |x_j| [n_slots, d])."""
    B, d = len(lens), x.shape[1]
    out, terms, w = np.zeros((B, d)), np.zeros((B, d)), np.zeros(B * P)
    for b, n in enumerate(lens):
        if not n:
            continue
        xb = x[b * P:b * P + n]
        s = np.tanh(xb @ Wa + ba) @ v
        e = np.exp(s - s.max())
        wb = e / e.sum()
        w[b * P:b * P + n] = wb
        out[b], terms[b] = wb @ xb, wb @ np.abs(xb)
    return out, w, terms


def pool_tokens_t(xb, Wa, ba, v):
    """One slot's real tokens xb [n, d] (n >= 1) -> its pooled row [d] (differentiable torch)."""
    return torch.softmax(torch.tanh(xb @ Wa + ba) @ v, 0) @ xb


def addpool_t(x, Wa, ba, v, lens, P):
    """addpool_np's out in differentiable torch (float64), slot by slot on the real tokens."""
    rows = [pool_tokens_t(x[b * P:b * P + n], Wa, ba, v) if n else torch.zeros(x.shape[1], dtype=x.dtype)
            for b, n in enumerate(lens)]
    return torch.stack(rows, 0)


def addpool_from_u_t(x, u, v, lens, P):
    """The pooling as the kernel sees it, with u a leaf of its own (the gradients dx direct, du and dv)."""
    rows = [torch.softmax(torch.tanh(u[b * P:b * P + n]) @ v, 0) @ x[b * P:b * P + n] if n
            else torch.zeros(x.shape[1], dtype=x.dtype) for b, n in enumerate(lens)]
    return torch.stack(rows, 0)


def addpool_dense_t(x, Wa, ba, v, lens, P):
    """The same pooling over all P positions of every slot: scores of the padding set to -inf before the softmax, the
    pooled sum masked. A slot without tokens has no finite score; its row is the contract's zeros."""
    B, d = len(lens), x.shape[1]
    m = torch.arange(P)[None, :] < torch.as_tensor(np.asarray(lens))[:, None]          # [B, P]
    xs = x.reshape(B, P, d)
    s = torch.tanh(xs @ Wa + ba) @ v
    s = torch.where(m, s, torch.full_like(s, -np.inf))
    some = m.any(1, keepdim=True)
    w = torch.softmax(torch.where(some, s, torch.zeros_like(s)), 1) * m
    return (w[:, :, None] * torch.where(m[:, :, None], xs, torch.zeros_like(xs))).sum(1)


def torch_head_additive(add):
    """seq_att_ref.torch_head_ragged ending in the additive pooling with add = (Wa, ba, v): a head= function for
    seq_att_ref.torch_train_loss_full."""
    Wa, ba, v = add

    def head(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
        rows = []
        for it, p in R.slot_tokens(sequence, mask):
            if not len(it):
                rows.append(torch.zeros(fi.shape[1], dtype=fi.dtype))
                continue
            x = R._ln_t(fi[torch.as_tensor(it)], ln_params[0]) + R._ln_t(pos_embed[torch.as_tensor(p)], ln_params[1])
            for i, w in enumerate(att_params):
                y = R._ln_t(x, ln_params[2 + i])
                x = R._lk_t(R.attn_tokens_t(y @ w["Wq"] + w["bq"], y @ w["Wk"] + w["bk"], y @ w["Wv"] + w["bv"], heads),
                            leaky) + x
            rows.append(pool_tokens_t(x, Wa, ba, v))
        return torch.stack(rows, 0)
    return head
