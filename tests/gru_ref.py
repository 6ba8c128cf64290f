"""float64 restatements of the GRU cell of the interval fusion (--rnnCell gru): TF 1.14 GRUCell with zero
initial state, restated from TF's documented source (no TensorFlow run pins the floating-point side), in numpy and in
differentiable torch, and the fusion composed with the oracle's layer norm and attention.

    [r | u] = sigmoid([x_s | h] Wg + bg)     Wg [2d, 2d], bg [2d]
    c       = tanh([x_s | r.h] Wc + bc)      Wc [2d, d],  bc [d]
    h'      = u.h + (1 - u).c                drop [n, t, d] scales the emitted h only
"""
import numpy as np

from oracle import selfgnn_oracle as O

GRU_KEYS = ("gru_Wg", "gru_bg", "gru_Wc", "gru_bc")


def _sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def gru(x, Wg, bg, Wc, bc, drop=None, want_saved=False):
    """numpy float64. x [n, t, d] -> h [n, t, d] (scaled by drop where given); want_saved: also gates [n, t, 2d] = r | u,
    cand [n, t, d] and the un-dropped h."""
    x, Wg, bg, Wc, bc = (np.asarray(a, dtype=np.float64) for a in (x, Wg, bg, Wc, bc))
    n, t, d = x.shape
    h = np.zeros((n, d))
    hs, gs, cs = [], [], []
    for s in range(t):
        g = _sigmoid(np.concatenate([x[:, s], h], axis=1) @ Wg + bg)
        r, u = g[:, :d], g[:, d:]
        c = np.tanh(np.concatenate([x[:, s], r * h], axis=1) @ Wc + bc)
        h = u * h + (1.0 - u) * c
        hs.append(h), gs.append(g), cs.append(c)
    raw = np.stack(hs, axis=1)
    out = raw if drop is None else raw * np.asarray(drop, dtype=np.float64)
    return (out, np.stack(gs, axis=1), np.stack(cs, axis=1), raw) if want_saved else out


def torch_gru(x, Wg, bg, Wc, bc, drop=None):
    """The block above op for op, in differentiable torch (float64 tensors in, float64 out)."""
    import torch
    n, t, d = x.shape
    h = torch.zeros((n, d), dtype=x.dtype)
    outs = []
    for s in range(t):
        g = torch.sigmoid(torch.cat([x[:, s, :], h], dim=1) @ Wg + bg)
        r, u = g[:, :d], g[:, d:]
        c = torch.tanh(torch.cat([x[:, s, :], r * h], dim=1) @ Wc + bc)
        h = u * h + (1.0 - u) * c
        outs.append(h)
    out = torch.stack(outs, dim=1)
    return out if drop is None else out * drop


def torch_interval_fusion_gru(x, p, heads, drop=None):
    """GRU -> the oracle's layer norm over (t, d) -> the oracle's attention + mean; p holds torch tensors."""
    h = torch_gru(x, *(p[k] for k in GRU_KEYS), drop=drop)
    y = O.torch_layer_norm_td(h, p["ln_gamma"], p["ln_beta"], 1e-12)
    return O.torch_mhsa_mean(y, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], heads)


def init_gru_params(d, rng, dtype=np.float32):
    """The four GRU tensors with every value drawn from rng: glorot-uniform kernels, and RANDOM biases (around TF's 1.0
    for the gates, around 0 for the candidate) so that a dropped bias shows."""
    return {"gru_Wg": O.xavier_uniform((2 * d, 2 * d), rng, dtype),
            "gru_bg": (1.0 + 0.3 * rng.standard_normal(2 * d)).astype(dtype),
            "gru_Wc": O.xavier_uniform((2 * d, d), rng, dtype),
            "gru_bc": (0.3 * rng.standard_normal(d)).astype(dtype)}


def init_fusion_params_gru(d, rng, dtype=np.float32):
    """The oracle's fusion parameters with the GRU's tensors in the LSTM's place."""
    p = O.init_fusion_params(d, rng, dtype)
    del p["lstm_W"], p["lstm_b"]
    return {**init_gru_params(d, rng, dtype), **p}


def bptt_steps(x, Wg, bg, Wc, bc, dh_ext, drop=None):
    """The per-step backward of DESIGN.md §22 written out in numpy float64, as the library's host loop sequences it:
    returns (dx, dWg, dbg, dWc, dbc) for dh_ext = the gradient at the emitted h."""
    x, Wg, bg, Wc, bc, dh_ext = (np.asarray(a, dtype=np.float64) for a in (x, Wg, bg, Wc, bc, dh_ext))
    n, t, d = x.shape
    _, gates, cand, h = gru(x, Wg, bg, Wc, bc, want_saved=True)
    dx = np.zeros_like(x)
    dWg, dbg, dWc, dbc = np.zeros_like(Wg), np.zeros_like(bg), np.zeros_like(Wc), np.zeros_like(bc)
    dh_rec = np.zeros((n, d))
    for s in range(t - 1, -1, -1):
        r, u, c = gates[:, s, :d], gates[:, s, d:], cand[:, s]
        hp = h[:, s - 1] if s > 0 else np.zeros((n, d))
        dh = dh_ext[:, s] * (1.0 if drop is None else np.asarray(drop, dtype=np.float64)[:, s]) + dh_rec
        # sagnn_gru_bwd_cand_f32
        da_c = dh * (1.0 - u) * (1.0 - c * c)
        du = dh * (hp - c)
        dh_rec = dh * u
        # dense_nn(da_c, Wc^T)
        dxc = da_c @ Wc.T
        dx_s, drh = dxc[:, :d], dxc[:, d:]
        # sagnn_gru_bwd_gates_f32
        da_g = np.concatenate([drh * hp * r * (1.0 - r), du * u * (1.0 - u)], axis=1)
        dh_rec = dh_rec + drh * r
        # dense_nn(da_g, Wg^T, accumulate)
        dxg = da_g @ Wg.T
        dx[:, s] = dx_s + dxg[:, :d]
        dh_rec = dh_rec + dxg[:, d:]
        # the weight gradients (after the loop in the library; h_{-1} = 0: no recurrent term at step 0)
        dWg[:d] += x[:, s].T @ da_g
        dWc[:d] += x[:, s].T @ da_c
        dbg += da_g.sum(0)
        dbc += da_c.sum(0)
        if s > 0:
            dWg[d:] += hp.T @ da_g
            dWc[d:] += (r * hp).T @ da_c
    return dx, dWg, dbg, dWc, dbc
