"""Float64 restatements of the position-wise feed-forward block of the sequence head (--seqFFN), written
from the contract and not from the kernels. For every real token row x_j of a slab [n_slots * P, d]:

  z = LN(x_j; gamma, beta)  (per token over d, eps 1e-12),  a = z W1 + b1,  h = act(a),  out = x_j + h W2 + b2,
  act(a) = leaky * a where leaky * a >= a, else a (seq_att_ref._lk_t);  zero rows in the padding.

A parameter set p is a dict with the keys gamma, beta, W1, b1, W2, b2. The head that applies the block after each
attention layer is seq_att_ref.torch_head_ragged's (seq_causal_ref's attention under the causal mask), ending in the sum
or in seq_pool_ref's additive pooling."""
import numpy as np
import torch

import seq_att_ref as A
import seq_causal_ref as C
import seq_pool_ref as SP
from oracle import selfgnn_oracle as O

KEYS = ("gamma", "beta", "W1", "b1", "W2", "b2")


def ffn_tokens_np(x, p, leaky):
    """x [n, d] float64 -> (out [n, d], the term sums |x| + |b2| + |h| |W2| + (|z| |W1| + |b1|) |W2|)."""
    z = O.layer_norm_td(x[:, None, :], p["gamma"], p["beta"], 1e-12)[:, 0, :]
    a = z @ p["W1"] + p["b1"]
    h = np.where(leaky * a >= a, leaky * a, a)
    out = x + h @ p["W2"] + p["b2"]
    terms = np.abs(x) + np.abs(p["b2"]) + np.abs(h) @ np.abs(p["W2"]) + (np.abs(z) @ np.abs(p["W1"]) + np.abs(p["b1"])) @ np.abs(p["W2"])
    return out, terms


def seq_ffn_np(x, p, lens, P, leaky):
    """The slab form of sagnn_seq_ffn_f32's contract: x [n_slots * P, d] float64 -> (out, term sums), zero rows in the
    padding; the padded rows of x are not read."""
    out, terms = np.zeros_like(x, dtype=np.float64), np.zeros_like(x, dtype=np.float64)
    for b, n in enumerate(lens):
        if n:
            out[b * P:b * P + n], terms[b * P:b * P + n] = ffn_tokens_np(np.asarray(x[b * P:b * P + n], dtype=np.float64), p, leaky)
    return out, terms


def ffn_tokens_t(x, p, leaky):
    """ffn_tokens_np's out in differentiable torch."""
    z = A._ln_t(x, (p["gamma"], p["beta"]))
    return x + A._lk_t(z @ p["W1"] + p["b1"], leaky) @ p["W2"] + p["b2"]


def seq_ffn_t(x, p, lens, P, leaky):
    """seq_ffn_np's out in differentiable torch (float64), slot by slot on the real tokens."""
    rows = []
    for b, n in enumerate(lens):
        if n:
            rows.append(ffn_tokens_t(x[b * P:b * P + n], p, leaky))
        rows.append(torch.zeros((P - n, x.shape[1]), dtype=x.dtype))
    return torch.cat(rows, 0)


def torch_head_ffn_slabs(ffn_params, causal=False):
    """Per batch slot the rows x [n_b, d] after the last block (None for an empty slot): seq_causal_ref.torch_head_slabs
    with the feed-forward block ffn_params[i] after attention layer i."""
    attn = C.attn_tokens_t if causal else A.attn_tokens_t

    def slabs(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
        out = []
        for it, p in A.slot_tokens(sequence, mask):
            if not len(it):
                out.append(None)
                continue
            x = A._ln_t(fi[torch.as_tensor(it)], ln_params[0]) + A._ln_t(pos_embed[torch.as_tensor(p)], ln_params[1])
            for i, w in enumerate(att_params):
                y = A._ln_t(x, ln_params[2 + i])
                x = A._lk_t(attn(y @ w["Wq"] + w["bq"], y @ w["Wk"] + w["bk"], y @ w["Wv"] + w["bv"], heads), leaky) + x
                if ffn_params is not None:
                    x = ffn_tokens_t(x, ffn_params[i], leaky)
            out.append(x)
        return out
    return slabs


def torch_head_ffn(ffn_params, pool=None, causal=False, heads=None):
    """A head= function for seq_att_ref.torch_train_loss_full: the ragged head with the block after each attention
    layer, under either mask. pool: None for the sum over the tokens, or (Wa, ba, v) for the additive pooling. heads: the
    sequence head's own head count (--seqHeads), None for the one the objective passes. ffn_params None: no blocks."""
    slabs = torch_head_ffn_slabs(ffn_params, causal)

    def head(fi, pos_embed, ln_params, att_params, sequence, mask, fusion_heads, leaky):
        rows = []
        for x in slabs(fi, pos_embed, ln_params, att_params, sequence, mask, heads or fusion_heads, leaky):
            if x is None:
                rows.append(torch.zeros(fi.shape[1], dtype=fi.dtype))
            else:
                rows.append(x.sum(0) if pool is None else SP.pool_tokens_t(x, *pool))
        return torch.stack(rows, 0)
    return head
