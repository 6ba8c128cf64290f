"""Float64 restatement of the full-catalogue softmax training loss (--predLoss softmax), written from
the objective and not from the kernels.

  z[b, i]  = <Q[b], I[i]> * inv_temp
  E_b      = [0, n_items) minus row b's exclusion list, plus target[b] (the target is always eligible)
  loss     = scale * sum over rows with a target in [0, n_items) of ( ln sum_{i in E_b} exp(z[b, i]) - z[b, target[b]] )
  g[b, i]  = scale * inv_temp * (p[b, i] - [i == target[b]]),  p = exp(z - lse[b]) on E_b and 0 elsewhere
  dQ       = g I,  dI = g^T Q

Row b's list is list excl_row[b] of the CSR (excl_ptr, excl_items), or list b without excl_row; an excl_row value
outside [0, n_lists) is an empty list. A row whose target is outside [0, n_items) is skipped: zeros everywhere.

The model form: q[b] = leaky(att[b]) + fu[u_b] per active batch slot, I = fi, the exclusion table the per-user banned
lists, excl_row = the slots' users, scale = 1 / max(n_active, 1)."""
import numpy as np
import torch

from oracle import selfgnn_oracle as O


def eligible(n_queries, n_items, target, excl_ptr=None, excl_items=None, excl_row=None):
    """bool [n_queries, n_items]: the items row b sums over (all False for a skipped row)."""
    el = np.ones((n_queries, n_items), dtype=bool)
    target = np.asarray(target, dtype=np.int64)
    if excl_ptr is not None:
        excl_ptr, excl_items = np.asarray(excl_ptr, dtype=np.int64), np.asarray(excl_items, dtype=np.int64)
        n_lists = len(excl_ptr) - 1
        for b in range(n_queries):
            L = b if excl_row is None else int(excl_row[b])
            if 0 <= L < n_lists:
                ids = excl_items[excl_ptr[L]:excl_ptr[L + 1]]
                el[b, ids[(ids >= 0) & (ids < n_items)]] = False
    ok = (target >= 0) & (target < n_items)
    el[np.flatnonzero(ok), target[ok]] = True
    el[~ok] = False
    return el


def softmax_loss_np(Q, I, target, inv_temp=1.0, scale=None, excl_ptr=None, excl_items=None, excl_row=None):
    """numpy float64: dict with loss, lse [B], tscore [B], dQ, dI (for an upstream gradient of 1), p [B, n_items] and
    the eligibility mask."""
    Q, I = np.asarray(Q, dtype=np.float64), np.asarray(I, dtype=np.float64)
    B, n_items = Q.shape[0], I.shape[0]
    target = np.asarray(target, dtype=np.int64)
    scale = 1.0 / max(B, 1) if scale is None else scale
    el = eligible(B, n_items, target, excl_ptr, excl_items, excl_row)
    ok = el.any(1)
    z = (Q @ I.T) * inv_temp
    zm = np.where(el, z, -np.inf)
    lse = np.zeros(B)
    p = np.zeros_like(z)
    if ok.any():
        mx = zm[ok].max(1, keepdims=True)
        e = np.exp(zm[ok] - mx)
        lse[ok] = (mx + np.log(e.sum(1, keepdims=True)))[:, 0]
        p[ok] = e / e.sum(1, keepdims=True)
    t = np.where(ok, target, 0)
    tscore = np.where(ok, (Q * I[t]).sum(1), 0.0)
    loss = scale * (lse - tscore * inv_temp)[ok].sum()
    g = p.copy()
    g[np.flatnonzero(ok), t[ok]] -= 1.0
    g *= scale * inv_temp
    return {"loss": loss, "lse": lse, "tscore": tscore, "dQ": g @ I, "dI": g.T @ Q, "p": p, "eligible": el}


def torch_softmax_loss(Q, I, target, inv_temp, scale, el):
    """The same loss in differentiable torch: logsumexp over the logits with -inf added outside `el` (bool
    [B, n_items] from eligible()); works in the dtype of Q / I."""
    el = torch.as_tensor(el)
    ok = el.any(1)
    if not bool(ok.any()):
        return (Q.sum() + I.sum()) * 0.0
    z = (Q[ok] @ I.T) * inv_temp
    mask = torch.zeros_like(z).masked_fill(~el[ok], float("-inf"))
    lse = torch.logsumexp(z + mask, dim=1)
    t = torch.as_tensor(np.asarray(target, dtype=np.int64))[ok]
    return scale * (lse - z.gather(1, t[:, None])[:, 0]).sum()


def _lk_t(x, leaky):
    a = leaky * x
    return torch.where(a >= x, a, x)


def torch_head_collapsed(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
    """The reference's collapsed head (model.py:156-168) -> att_user [B, d]: the masked sums of the sequence's item
    rows and of the position rows make one token per slot, the attention layers run on length-1 sequences."""
    seq = torch.as_tensor(np.asarray(sequence), dtype=torch.long)
    m = torch.as_tensor(np.asarray(mask), dtype=fi.dtype)[:, None, :]
    att = O.torch_layer_norm_td(m @ fi[seq], *ln_params[0]) + O.torch_layer_norm_td(
        m @ pos_embed[None].expand(seq.shape[0], -1, -1), *ln_params[1])
    for i, p in enumerate(att_params):
        a1 = O.torch_mhsa_mean(O.torch_layer_norm_td(att, *ln_params[2 + i]), p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"],
                               p["bv"], heads)[:, None, :]
        att = _lk_t(a1, leaky) + att
    return att.sum(1)


def slot_triples(batch):
    """The distinct (slot, user, target) triples of the positive half of a batch, ascending by slot."""
    uids, iids, locs = (np.asarray(batch[k], dtype=np.int64) for k in ("uids", "iids", "uLocs_seq"))
    n = len(locs) // 2
    tri = np.unique(np.stack([locs[:n], uids[:n], iids[:n]], 1), axis=0) if n else np.zeros((0, 3), np.int64)
    assert len(np.unique(tri[:, 0])) == len(tri), "a slot holds one positive"
    return tri[:, 0], tri[:, 1], tri[:, 2]


def torch_train_loss_softmax(P, adj_list, tp_list, batch, cfg, banned, head=torch_head_collapsed):
    """The training objective under --predLoss softmax in differentiable torch float64: the oracle's torch_train_loss
    supplies final_user / final_item and the SSL loss, its hinge preLoss is dropped, and preLoss is the softmax loss
    of the active slots' queries q[b] = leaky(att_user[b]) + fu[u_b] against fi, user u_b's banned list left out.
    banned = (ban_ptr [U + 1], ban_items); cfg["temp"] is the temperature (default 1). Returns (preLoss, sslloss, fu, fi)."""
    _, ssl, fu, fi = O.torch_train_loss(P, adj_list, tp_list, batch, cfg)
    leaky, heads = cfg["leaky"], cfg["heads"]
    att_user = head(fi, P["posEmbed"], P["ln"], P["att"], batch["sequence"], batch["mask"], heads, leaky)
    slots, users, targets = slot_triples(batch)
    q = _lk_t(att_user[torch.as_tensor(slots)], leaky) + fu[torch.as_tensor(users)]
    el = eligible(len(slots), fi.shape[0], targets, banned[0], banned[1], users)
    pre = torch_softmax_loss(q, fi, targets, 1.0 / cfg.get("temp", 1.0), 1.0 / max(len(slots), 1), el)
    return pre.reshape(()), ssl, fu, fi


EPS32 = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)


def tolerance_terms(Q, I, target, res, inv_temp, scale):
    """The derived error bounds of a float32 evaluation, per unit of their constants K (res = softmax_loss_np's dict):
      T[b, i] = sum_k |Q[b, k] I[i, k]|,  A[b] = max_{i in E_b} T[b, i] * inv_temp,  w = scale * inv_temp,
      c[b, i] = p[b, i] (1 + A[b]) + [i == target[b]]
      |lse - ref|      <= K_l eps32 (1 + A[b])
      |dQ[b, c] - ref| <= K_q eps32 w sum_i c[b, i] |I[i, c]| + FLT_MIN w sum_i |I[i, c]|
      |dI[i, c] - ref| <= K_i eps32 w sum_b c[b, i] |Q[b, c]| + FLT_MIN w sum_b |Q[b, c]|
    Returns {"lse": (unit, floor), "dQ": (unit, floor), "dI": (unit, floor)}; the bound is K * unit + floor."""
    Q, I = np.abs(np.asarray(Q, dtype=np.float64)), np.abs(np.asarray(I, dtype=np.float64))
    el, p = res["eligible"], res["p"]
    ok = el.any(1)
    T = Q @ I.T
    A = np.where(ok, np.where(el, T, 0.0).max(1) * inv_temp, 0.0)
    w = abs(scale) * inv_temp
    c = p * (1.0 + A)[:, None]
    t = np.asarray(target, dtype=np.int64)
    c[np.flatnonzero(ok), t[ok]] += 1.0
    return {"lse": (EPS32 * (1.0 + A), np.zeros_like(A)),
            "dQ": (EPS32 * w * (c @ I), FLT_MIN * w * np.broadcast_to(I.sum(0), Q.shape)),
            "dI": (EPS32 * w * (c.T @ Q), FLT_MIN * w * np.broadcast_to(Q.sum(0), I.shape))}


def worst_ratio(got, want, unit, floor):
    """max over the elements of (|got - want| - floor)+ / unit: the K an evaluation needs (inf where unit is 0 and the
    error exceeds the floor)."""
    err = np.maximum(np.abs(np.asarray(got, dtype=np.float64) - want) - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / unit, 0.0)
    return float(r.max()) if r.size else 0.0
