"""float64 numpy restatements of the training-side operators, written from the formulas of include/sagnn.h
("Prediction head", "Training-side operators") and the reference lines it cites (model.py:166-205, 241-246), not from
the kernels. The tests hand them the SAME float32 values the kernels read.

Tie rule: tf.maximum(leaky*x, x) sends the gradient to its FIRST argument on ties (MaximumGrad tests x >= y), so the
slope is `leaky` wherever x <= leaky*x: x = 0 (either sign), and a product that is exactly 0, take `leaky`.

Every sum returns a Sum(value, mag, cnt): the float64 value, the float64 sum of the magnitudes of its addends and
the number of addends, per output element. An fp32 evaluation that forms each addend with at most three roundings
and adds the m addends in ANY order (float atomics, a shuffle tree) stays within (m + 4) * 2^-24 * mag of `value`
(bound() below): m - 1 additions plus the roundings of the addends, to first order in 2^-24."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

U24 = 2.0 ** -24                       # unit roundoff of fp32
Sum = namedtuple("Sum", "value mag cnt")


def bound(s, extra=4):
    """The derived error bound of a Sum evaluated in fp32, per element."""
    return (np.asarray(s.cnt, dtype=np.float64) + extra) * U24 * s.mag


def f64(x):
    return np.asarray(x, dtype=np.float64)


def leaky(x, a):
    return np.maximum(a * x, x)


def slope(x, a):
    """d/dx of tf.maximum(a*x, x): `a` wherever x <= a*x (the tie goes to the first argument)."""
    return np.where(x <= a * x, float(a), 1.0)


def _scatter(ids, n_rows, addends):
    """Sum of addends[e] into row ids[e]: Sum over [n_rows, d]."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    P = sp.csr_matrix((np.ones(n), (ids, np.arange(n))), shape=(n_rows, n))
    cnt = np.bincount(ids, minlength=n_rows).astype(np.float64)[:, None] * np.ones((1, addends.shape[1]))
    return Sum(P @ addends, P @ np.abs(addends), cnt)


def _add(a, b):
    return Sum(a.value + b.value, a.mag + b.mag, a.cnt + b.cnt)


# ---- prediction head (model.py:166-173) ---------------------------------------------------------------------------

def pair_score(U, I, S, A, uids, iids, locs, a):
    """preds[e] = <U[u], I[i]> + <leaky(S[l]), A[i]>; S None drops the second term. Sum over [n_pairs]."""
    t = f64(U)[uids] * f64(I)[iids]
    if S is not None:
        t = np.concatenate([t, leaky(f64(S)[locs], a) * f64(A)[iids]], axis=1)
    return Sum(t.sum(1), np.abs(t).sum(1), np.full(len(uids), t.shape[1], dtype=np.float64))


def pair_score_bwd(U, I, S, A, uids, iids, locs, a, g, alias_a=False):
    """Given g = dL/dpreds: dU[u] += g I[i]; dI[i] += g U[u]; dA[i] += g leaky(S[l]); dS[l] += g slope(S[l]) A[i].
    Returns {"dU", "dI"[, "dS", "dA"]} of Sums shaped like the tables. alias_a: A is I and dA is dI (the head's
    iEmbed_att IS final_item_vector, model.py:169-173): dI receives both sums and there is no "dA"."""
    U, I, g = f64(U), f64(I), f64(g)[:, None]
    out = {"dU": _scatter(uids, len(U), g * I[iids]), "dI": _scatter(iids, len(I), g * U[uids])}
    if S is not None:
        S, A = f64(S), f64(A)
        s = S[locs]
        out["dS"] = _scatter(locs, len(S), g * slope(s, a) * A[iids])
        dA = _scatter(iids, len(A), g * leaky(s, a))
        if alias_a:
            out["dI"] = _add(out["dI"], dA)
        else:
            out["dA"] = dA
    return out


def leaky_add(x, b, a):
    """out = max(a*x, x) + b in float32 (b None = 0): one product, one max, one sum, each correctly rounded."""
    x = np.asarray(x, dtype=np.float32)
    m = np.maximum(np.float32(a) * x, x)
    return m + (np.float32(0) if b is None else np.asarray(b, dtype=np.float32))


# ---- SSL branch (model.py:179-205) --------------------------------------------------------------------------------

def prod_leaky_sum(X, Y, uids, iids, a):
    """s[e] = sum_j leaky(X[u][j] * Y[i][j]). Sum over [n_pairs]."""
    t = leaky(f64(X)[uids] * f64(Y)[iids], a)
    return Sum(t.sum(1), np.abs(t).sum(1), np.full(len(uids), t.shape[1], dtype=np.float64))


def prod_leaky_sum_bwd(X, Y, uids, iids, a, g):
    """dX[u] += g slope(x y) y; dY[i] += g slope(x y) x (the product of two fp32 values is exact in float64, so an
    exact 0 is an exact 0 here too)."""
    X, Y = f64(X), f64(Y)
    x, y = X[uids], Y[iids]
    gs = f64(g)[:, None] * slope(x * y, a)
    return {"dX": _scatter(uids, len(X), gs * y), "dY": _scatter(iids, len(Y), gs * x)}


def meta_features(F, V, uids):
    """m[e] = [F[u] * V[u] | F[u] | V[u]] as float32: one correctly rounded product and two copies."""
    f, v = np.asarray(F, dtype=np.float32)[uids], np.asarray(V, dtype=np.float32)[uids]
    return np.concatenate([f * v, f, v], axis=1)


def meta_features_bwd(F, V, uids, dm):
    """dF[u] += dm0 V[u] + dm1; dV[u] += dm0 F[u] + dm2 with dm = [dm0 | dm1 | dm2]. Each pair contributes two
    addends per element (the product and the copy's gradient)."""
    F, V, dm = f64(F), f64(V), f64(dm)
    d = F.shape[1]
    g0, g1, g2 = dm[:, :d], dm[:, d:2 * d], dm[:, 2 * d:]
    return {"dF": _add(_scatter(uids, len(F), g0 * V[uids]), _scatter(uids, len(F), g1)),
            "dV": _add(_scatter(uids, len(V), g0 * F[uids]), _scatter(uids, len(V), g2))}


def leaky_fwd(x, a):
    """max(a*x, x) as float32."""
    x = np.asarray(x, dtype=np.float32)
    return np.maximum(np.float32(a) * x, x)


def leaky_bwd(x, g, a):
    """g * slope(x) as float32 (x the pre-activation)."""
    x, g = np.asarray(x, dtype=np.float32), np.asarray(g, dtype=np.float32)
    return np.where(x <= np.float32(a) * x, np.float32(a) * g, g)


def mul(x, y):
    return np.asarray(x, dtype=np.float32) * np.asarray(y, dtype=np.float32)


def mask_scale(g, mask, s):
    """out[r, 4l + j] = g * (bit j of mask[r, l] ? 1 : s) as float32."""
    g = np.asarray(g, dtype=np.float32)
    bits = ((np.asarray(mask, dtype=np.uint8)[:, :, None] >> np.arange(4, dtype=np.uint8)) & 1).reshape(g.shape)
    return np.where(bits != 0, g, np.float32(s) * g)


def rowdot_sigmoid(A, w3, b3, k):
    """z[e] = <A[e, :k], w3> + b3 as a Sum over [n] (k + 1 addends) and w = sigmoid(z)."""
    t = np.concatenate([f64(A)[:, :k] * f64(w3)[None, :k], np.full((len(A), 1), float(np.asarray(b3).reshape(-1)[0]))], axis=1)
    z = Sum(t.sum(1), np.abs(t).sum(1), np.full(len(A), k + 1, dtype=np.float64))
    with np.errstate(over="ignore"):
        return z, 1.0 / (1.0 + np.exp(-z.value))


def rowdot_sigmoid_bwd(A, w3, w, dw, k):
    """dz = dw w (1 - w); dA[e, :k] = dz w3 (one addend each); dw3 = sum_e dz A[e, :k]; db3 = sum_e dz."""
    A, w3, w, dw = f64(A)[:, :k], f64(w3)[:k], f64(w), f64(dw)
    dz = (dw * w * (1.0 - w))[:, None]
    dA = dz * w3[None, :]
    t = dz * A
    n = float(len(A))
    return {"dA": Sum(dA, np.abs(dA), np.ones_like(dA)),
            "dw3": Sum(t.sum(0), np.abs(t).sum(0), np.full(k, n)),
            "db3": Sum(dz.sum(0), np.abs(dz).sum(0), np.full(1, n))}


# ---- hinge losses (model.py:202, :244) ----------------------------------------------------------------------------

def hinge(pos, neg, scale, wp=None, wn=None, sp=None, sn=None):
    """loss = scale * sum max(0, 1 - S (pos - neg)), S = wp sp - wn sn (1 without weights; sp / sn constants).
    A row with h = 1 - S (pos - neg) <= 0 is inactive: no term, no gradient (d max(0, h) / dh = 0 at h = 0).
    Returns {"h", "loss": Sum over [1], "dpos", "dneg"[, "dwp", "dwn"]: Sums over [n]}."""
    pos, neg = f64(pos), f64(neg)
    delta = pos - neg
    one = np.ones_like(delta)
    if wp is None:
        S, Smag, Scnt = one, one, one
    else:
        wp, wn, sp, sn = f64(wp), f64(wn), f64(sp), f64(sn)
        S, Smag, Scnt = wp * sp - wn * sn, np.abs(wp * sp) + np.abs(wn * sn), 2 * one
    h = 1.0 - S * delta
    act = (h > 0).astype(np.float64)
    term = scale * h * act
    # a term is 1 - S delta: its magnitude counts both parts, 1 + |S delta| <= 1 + Smag |delta|
    tmag = abs(scale) * (1.0 + Smag * (np.abs(pos) + np.abs(neg))) * act
    out = {"h": h, "loss": Sum(term.sum(keepdims=True), tmag.sum(keepdims=True), np.full(1, float(len(h)))),
           "dpos": Sum(-scale * S * act, abs(scale) * Smag * act, Scnt),
           "dneg": Sum(scale * S * act, abs(scale) * Smag * act, Scnt)}
    if wp is not None:
        dmag = np.abs(pos) + np.abs(neg)
        out["dwp"] = Sum(-scale * delta * sp * act, abs(scale) * dmag * np.abs(sp) * act, 2 * one)
        out["dwn"] = Sum(scale * delta * sn * act, abs(scale) * dmag * np.abs(sn) * act, 2 * one)
    return out
