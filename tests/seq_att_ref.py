"""Float64 restatements of the head under --seqAtt full, written from the contract and not from the
kernels: every unmasked entry of a batch slot's sequence is a token, the attention layers run over the slot's real
tokens, the pooled sum feeds the pair score.

  x0[b, j]  = LN(fi[it[b, j]]; head_ln[0]) + LN(posEmbed[p[b, j]]; head_ln[1])          (per token over d, eps 1e-12)
  layer i:    y = LN(x_i; head_ln[2 + i]); q|k|v = y W + b; per head e[j, s] = exp(q_j k_s / sqrt(d_k)) over the
              slot's tokens, a = e / (sum_s e + 1e-8), ctx_j = sum_s a[j, s] v_s; x_{i+1} = leaky(ctx) + x_i
  att_user[b] = sum_j x_last[b, j]                                                       (an empty slot: zeros)

Two independent forms: the ragged one (a loop over slots on their real tokens only, numpy and torch) and the dense one
(all P positions of every slot, all P x P scores, multiplied by the attn_mask that Utils/attention.py:35-45 takes and
the reference never passes; torch). Layer norm, leaky and the rest of the objective are the oracle's own functions."""
import numpy as np
import torch

from oracle import selfgnn_oracle as O


def slot_tokens(sequence, mask):
    """Per batch slot (item ids, positions) of its unmasked entries, positions ascending."""
    sequence, keep = np.asarray(sequence, dtype=np.int64), np.asarray(mask) != 0
    return [(sequence[b][keep[b]], np.flatnonzero(keep[b])) for b in range(keep.shape[0])]


def _ln_np(x, gb):
    return O.layer_norm_td(x[:, None, :], gb[0], gb[1], 1e-12)[:, 0, :]


def _ln_t(x, gb):
    return O.torch_layer_norm_td(x[:, None, :], gb[0], gb[1], 1e-12)[:, 0, :]


def _lk_t(x, leaky):
    a = leaky * x
    return torch.where(a >= x, a, x)


# ---- the attention on one slot's tokens ----------------------------------------------------------------------------
def attn_tokens_np(q, k, v, heads):
    """q, k, v [n, d] -> (ctx [n, d], sum_s |a[j, s] v_s| [n, d])."""
    n, d = q.shape
    dk = d // heads
    qh, kh, vh = (z.reshape(n, heads, dk).transpose(1, 0, 2) for z in (q, k, v))
    e = np.exp(qh @ kh.transpose(0, 2, 1) / np.sqrt(dk))
    a = e / (e.sum(-1, keepdims=True) + 1e-8)
    merge = lambda z: z.transpose(1, 0, 2).reshape(n, d)
    return merge(a @ vh), merge(a @ np.abs(vh))


def attn_tokens_t(q, k, v, heads):
    n, d = q.shape
    dk = d // heads
    qh, kh, vh = (z.reshape(n, heads, dk).permute(1, 0, 2) for z in (q, k, v))
    e = torch.exp(qh @ kh.transpose(-1, -2) / float(np.sqrt(dk)))
    a = e / (e.sum(-1, keepdim=True) + 1e-8)
    return (a @ vh).permute(1, 0, 2).reshape(n, d)


def seq_attn_np(qkv, lens, P, heads):
    """The slab form of sagnn_seq_attn_f32's contract: qkv [n_slots * P, 3d] float64 -> (ctx, term sums), both
    [n_slots * P, d] with zero rows in the padding."""
    d = qkv.shape[1] // 3
    ctx, terms = np.zeros((len(lens) * P, d)), np.zeros((len(lens) * P, d))
    for b, n in enumerate(lens):
        if n:
            r = qkv[b * P:b * P + n]
            ctx[b * P:b * P + n], terms[b * P:b * P + n] = attn_tokens_np(r[:, :d], r[:, d:2 * d], r[:, 2 * d:], heads)
    return ctx, terms


def seq_attn_t(qkv, lens, P, heads):
    """seq_attn_np in differentiable torch (float64)."""
    d = qkv.shape[1] // 3
    rows = []
    for b, n in enumerate(lens):
        if n:
            r = qkv[b * P:b * P + n]
            rows.append(attn_tokens_t(r[:, :d], r[:, d:2 * d], r[:, 2 * d:], heads))
        rows.append(torch.zeros((P - n, d), dtype=qkv.dtype))
    return torch.cat(rows, 0)


# ---- the head ------------------------------------------------------------------------------------------------------
def head_ragged_np(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
    """att_user [B, d], slot by slot on the real tokens (numpy float64)."""
    out = np.zeros((np.asarray(mask).shape[0], fi.shape[1]), dtype=fi.dtype)
    for b, (it, p) in enumerate(slot_tokens(sequence, mask)):
        if not len(it):
            continue
        x = _ln_np(fi[it], ln_params[0]) + _ln_np(pos_embed[p], ln_params[1])
        for i, w in enumerate(att_params):
            y = _ln_np(x, ln_params[2 + i])
            ctx, _ = attn_tokens_np(y @ w["Wq"] + w["bq"], y @ w["Wk"] + w["bk"], y @ w["Wv"] + w["bv"], heads)
            x = O.leaky_relu(ctx, leaky) + x
        out[b] = x.sum(0)
    return out


def torch_head_ragged(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
    """head_ragged_np in differentiable torch (float64)."""
    rows = []
    for it, p in slot_tokens(sequence, mask):
        if not len(it):
            rows.append(torch.zeros(fi.shape[1], dtype=fi.dtype))
            continue
        x = _ln_t(fi[torch.as_tensor(it)], ln_params[0]) + _ln_t(pos_embed[torch.as_tensor(p)], ln_params[1])
        for i, w in enumerate(att_params):
            y = _ln_t(x, ln_params[2 + i])
            x = _lk_t(attn_tokens_t(y @ w["Wq"] + w["bq"], y @ w["Wk"] + w["bk"], y @ w["Wv"] + w["bv"], heads), leaky) + x
        rows.append(x.sum(0))
    return torch.stack(rows, 0)


def torch_head_dense(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
    """The same head on all P positions of every slot: P x P scores times attn_mask (the key's mask, broadcast over
    heads and queries: Utils/attention.py:40-41), pooled over the unmasked positions. Padded queries compute finite
    values nothing reads."""
    seq = torch.as_tensor(np.asarray(sequence), dtype=torch.long)
    m = torch.as_tensor(np.asarray(mask), dtype=fi.dtype)                               # [B, P]
    B, P = m.shape
    d = fi.shape[1]
    dk = d // heads
    ln = lambda x, gb: _ln_t(x.reshape(B * P, d), gb).reshape(B, P, d)
    x = ln(fi[seq], ln_params[0]) + ln(pos_embed[None].expand(B, -1, -1), ln_params[1])
    attn_mask = m[:, None, None, :]                                                      # [B, 1, 1, P]
    for i, w in enumerate(att_params):
        y = ln(x, ln_params[2 + i])
        q, k, v = ((y @ w["W" + c] + w["b" + c]).reshape(B, P, heads, dk).permute(0, 2, 1, 3) for c in "qkv")
        scores = torch.exp(q @ k.transpose(-1, -2) / float(np.sqrt(dk))) * attn_mask
        a = scores / (scores.sum(-1, keepdim=True) + 1e-8)
        x = _lk_t((a @ v).permute(0, 2, 1, 3).reshape(B, P, d), leaky) + x
    return (x * m[:, :, None]).sum(1)


def prediction_head_full(final_user, final_item, pos_embed, ln_params, att_params, uids, iids, sequence, mask, ulocs_seq,
                         heads, leaky):
    """oracle.prediction_head's pair scores with att_user from head_ragged_np (numpy float64)."""
    att_user = head_ragged_np(final_item, pos_embed, ln_params, att_params, sequence, mask, heads, leaky)
    pck_u, pck_i = final_user[uids], final_item[iids]
    return (pck_u * pck_i).sum(-1) + (O.leaky_relu(att_user[ulocs_seq], leaky) * pck_i).sum(-1)


def torch_train_loss_full(P, adj_list, tp_list, batch, cfg, head=torch_head_ragged):
    """The training objective under --seqAtt full in differentiable torch float64: the oracle's torch_train_loss
    supplies final_user / final_item (GNN stack + interval fusion) and the SSL loss; its collapsed-head preLoss is
    dropped and the pair scores are rebuilt on the head restated here. Returns (preLoss, sslloss, fu, fi)."""
    _, ssl, fu, fi = O.torch_train_loss(P, adj_list, tp_list, batch, cfg)
    leaky, heads = cfg["leaky"], cfg["heads"]
    att_user = head(fi, P["posEmbed"], P["ln"], P["att"], batch["sequence"], batch["mask"], heads, leaky)
    uids = torch.as_tensor(np.asarray(batch["uids"]), dtype=torch.long)
    iids = torch.as_tensor(np.asarray(batch["iids"]), dtype=torch.long)
    ulocs = torch.as_tensor(np.asarray(batch["uLocs_seq"]), dtype=torch.long)
    preds = (fu[uids] * fi[iids]).sum(-1) + (_lk_t(att_user[ulocs], leaky) * fi[iids]).sum(-1)
    n = preds.shape[0] // 2
    return torch.clamp(1.0 - (preds[:n] - preds[n:]), min=0).mean(), ssl, fu, fi
