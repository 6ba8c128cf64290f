"""Reference side of the popularity-weighted candidate softmax (--softmaxNegDist pop), written from the
contract in include/sagnn.h and not from the kernels:

  weights(deg, a)                     the integer mass w_i = max(1, rint(2^20 (deg_i + 1)^a)) and its prefix sum;
  draw(cum, n_cand, seed, step)       sagnn_sample_strata_w_i32 in Python-int and float64 arithmetic;
  softmax_loss_pop_np(...)            float64 loss and gradients over {target} + the live eligible candidates, each
                                      candidate's logit moved by its position's offset, the target's by nothing;
  torch_softmax_loss_pop / torch_train_loss_pop   the same loss in differentiable torch.

The live ids of a drawn list are distinct, so the objective is softmax_loss_ref's on the full table with every item
that is not a live candidate put on each row's list (softmax_cand_ref.augmented) and a per-item offset."""
import math

import numpy as np
import torch

import device_sampler_ref as S
import softmax_cand_ref as C
import softmax_loss_ref as R
from oracle import selfgnn_oracle as O

MASS = 1 << 20


def weights(deg, a):
    """(w, cum, W): Python-int weights per item, their inclusive prefix sum and the total. float64 power, round half
    to even (rint), at least 1."""
    w = [max(1, int(round(float(MASS) * float(int(g) + 1) ** float(a)))) for g in deg]
    cum, tot = [], 0
    for v in w:
        tot += v
        cum.append(tot)
    return w, cum, tot


def strata_bounds(W, n_cand):
    """lo_0 .. lo_{n_cand} as Python ints: lo_j = j (W // n_cand) + (j (W % n_cand)) // n_cand."""
    q, rem = divmod(int(W), int(n_cand))
    return [j * q + (j * rem) // n_cand for j in range(n_cand + 1)]


def draw(cum, n_cand, seed, step):
    """(cand int64 [n_cand], m int64 [n_cand], live bool [n_cand], bias float32 [n_cand]): m is the run length at the
    live positions and 0 elsewhere, bias ln(m) - ln(n_cand w_c / W) there (exactly 0 when m W == n_cand w_c) and -inf
    elsewhere."""
    cum = [int(v) for v in cum]
    W = cum[-1]
    if n_cand == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.float32)
    lo = strata_bounds(W, n_cand)
    words = S.philox4x32_10(np.arange(n_cand), 1, step, C.STRATA_STREAM, seed)
    cum_np = np.asarray(cum, dtype=np.int64)
    cand = np.zeros(n_cand, np.int64)
    for j in range(n_cand):
        x = (int(words[0][j]) << 32) | int(words[1][j])
        r = lo[j] + ((x * (lo[j + 1] - lo[j])) >> 64)
        cand[j] = int(np.searchsorted(cum_np, r, side="right"))
    m, live = np.zeros(n_cand, np.int64), np.zeros(n_cand, bool)
    bias = np.full(n_cand, -np.inf, dtype=np.float32)
    j = 0
    while j < n_cand:
        ub = j
        while ub < n_cand and cand[ub] == cand[j]:
            ub += 1
        c, run = int(cand[j]), ub - j
        wc = cum[c] - (cum[c - 1] if c else 0)
        live[j], m[j] = True, run
        bias[j] = 0.0 if run * W == n_cand * wc else np.float32(math.log(run) - math.log(float(n_cand) * float(wc) / float(W)))
        j = ub
    return cand, m, live, bias


def expected_count(cum, n_cand, i):
    """The exact expected number of draws of item i, sum_j |range_i & stratum_j| / |stratum_j|, as a Fraction."""
    from fractions import Fraction
    cum = [int(v) for v in cum]
    a, b = (cum[i - 1] if i else 0), cum[i]
    lo = strata_bounds(cum[-1], n_cand)
    tot = Fraction(0)
    for j in range(n_cand):
        ov = min(b, lo[j + 1]) - max(a, lo[j])
        if ov > 0:
            tot += Fraction(ov, lo[j + 1] - lo[j])
    return tot


def item_offsets(n_items, cand, bias):
    """(live ids ascending, off float64 [n_items]): the offset of each live candidate at its id, 0 elsewhere."""
    cand, bias = np.asarray(cand, dtype=np.int64), np.asarray(bias, dtype=np.float64)
    live = np.isfinite(bias)
    ids = cand[live]
    assert len(np.unique(ids)) == len(ids), "live positions hold distinct ids"
    off = np.zeros(n_items)
    off[ids] = bias[live]
    return ids, off


def softmax_loss_pop_np(Q, I, cand, bias, target, inv_temp=1.0, scale=None, excl_ptr=None, excl_items=None, excl_row=None):
    """softmax_loss_ref.softmax_loss_np's dict for the offset objective, dI full-size; "off" [B, n_items] is the
    offset each logit took (0 at the row's target)."""
    Q, I = np.asarray(Q, dtype=np.float64), np.asarray(I, dtype=np.float64)
    B, n_items = Q.shape[0], I.shape[0]
    target = np.asarray(target, dtype=np.int64)
    scale = 1.0 / max(B, 1) if scale is None else scale
    ids, off = item_offsets(n_items, cand, bias)
    ptr, items = C.augmented(B, n_items, ids, excl_ptr, excl_items, excl_row)
    el = R.eligible(B, n_items, target, ptr, items, None)
    ok = el.any(1)
    offm = np.broadcast_to(off, (B, n_items)).copy()
    offm[np.flatnonzero(ok), target[ok]] = 0.0                     # the target's own term takes no offset
    z = (Q @ I.T) * inv_temp
    zm = np.where(el, z + offm, -np.inf)
    lse, p = np.zeros(B), np.zeros_like(z)
    if ok.any():
        mx = zm[ok].max(1, keepdims=True)
        e = np.exp(zm[ok] - mx)
        lse[ok] = (mx + np.log(e.sum(1, keepdims=True)))[:, 0]
        p[ok] = e / e.sum(1, keepdims=True)
    t = np.where(ok, target, 0)
    tscore = np.where(ok, (Q * I[t]).sum(1), 0.0)
    g = p.copy()
    g[np.flatnonzero(ok), t[ok]] -= 1.0
    g *= scale * inv_temp
    return {"loss": scale * (lse - tscore * inv_temp)[ok].sum(), "lse": lse, "tscore": tscore, "dQ": g @ I, "dI": g.T @ Q,
            "p": p, "eligible": el, "off": np.where(el, offm, 0.0)}


def tolerance_terms(Q, I, target, res, inv_temp, scale):
    """softmax_loss_ref.tolerance_terms with A[b] taken over |z| + |bias|: A[b] = max_{i in E_b} (T[b, i] inv_temp +
    |off[b, i]|). Everything else is that function's, term by term."""
    Q, I = np.abs(np.asarray(Q, dtype=np.float64)), np.abs(np.asarray(I, dtype=np.float64))
    el, p = res["eligible"], res["p"]
    ok = el.any(1)
    A = np.where(ok, np.where(el, (Q @ I.T) * inv_temp + np.abs(res["off"]), 0.0).max(1), 0.0)
    w = abs(scale) * inv_temp
    c = p * (1.0 + A)[:, None]
    t = np.asarray(target, dtype=np.int64)
    c[np.flatnonzero(ok), t[ok]] += 1.0
    return {"lse": (R.EPS32 * (1.0 + A), np.zeros_like(A)),
            "dQ": (R.EPS32 * w * (c @ I), R.FLT_MIN * w * np.broadcast_to(I.sum(0), Q.shape)),
            "dI": (R.EPS32 * w * (c.T @ Q), R.FLT_MIN * w * np.broadcast_to(Q.sum(0), I.shape))}


def assemble_dI(n_items, cand, bias, dIc, target, dT):
    """float64 [n_items, d]: the dIc rows of the live positions at their ids, dT added at the rows' targets."""
    live = np.isfinite(np.asarray(bias, dtype=np.float64))
    return C.assemble_dI(n_items, np.asarray(cand)[live], np.asarray(dIc)[live], target, dT)


def torch_softmax_loss_pop(Q, I, target, inv_temp, scale, el, off):
    """The loss in differentiable torch: logsumexp over logits + off with -inf outside `el`; off [B, n_items] is 0 at
    the targets. Works in the dtype of Q / I."""
    el = torch.as_tensor(el)
    ok = el.any(1)
    if not bool(ok.any()):
        return (Q.sum() + I.sum()) * 0.0
    z = (Q[ok] @ I.T) * inv_temp
    shift = torch.as_tensor(np.asarray(off), dtype=z.dtype)[ok].masked_fill(~el[ok], float("-inf"))
    lse = torch.logsumexp(z + shift, dim=1)
    t = torch.as_tensor(np.asarray(target, dtype=np.int64))[ok]
    return scale * (lse - z.gather(1, t[:, None])[:, 0]).sum()


def torch_train_loss_pop(P, adj_list, tp_list, batch, cfg, banned, cand, bias, head=R.torch_head_collapsed):
    """softmax_loss_ref.torch_train_loss_softmax under the drawn (cand, bias): banned = the plain per-user table
    (ban_ptr, ban_items). Returns (preLoss, sslloss, fu, fi)."""
    _, ssl, fu, fi = O.torch_train_loss(P, adj_list, tp_list, batch, cfg)
    leaky, heads = cfg["leaky"], cfg["heads"]
    att_user = head(fi, P["posEmbed"], P["ln"], P["att"], batch["sequence"], batch["mask"], heads, leaky)
    slots, users, targets = R.slot_triples(batch)
    q = R._lk_t(att_user[torch.as_tensor(slots)], leaky) + fu[torch.as_tensor(users)]
    n_items = fi.shape[0]
    ids, off = item_offsets(n_items, cand, bias)
    ptr, items = C.augmented(len(slots), n_items, ids, banned[0], banned[1], users)
    el = R.eligible(len(slots), n_items, targets, ptr, items, None)
    offm = np.broadcast_to(off, el.shape).copy()
    offm[np.arange(len(slots)), targets] = 0.0
    pre = torch_softmax_loss_pop(q, fi, targets, 1.0 / cfg.get("temp", 1.0), 1.0 / max(len(slots), 1), el, offm)
    return pre.reshape(()), ssl, fu, fi
