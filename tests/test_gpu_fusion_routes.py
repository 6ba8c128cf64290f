"""GPU parity: every forward route of the fusion selection table (csrc/engine.cpp) against the float64 oracle.

The ABI does not say which kernel ran; the cases below are written from the table, and tests/test_host.py pins the
selection itself. Each case names the table row it is there for. Tolerance: test_gpu_fusion's, never wider. Inputs are
screened on the CPU first: a row is used only if the float32 numpy oracle itself stays within a QUARTER of that tolerance
of the float64 one, so a kernel as exact as plain fp32 has three quarters of the bound to spare and a miss is the kernel's.
Every output, and every input, is a strided view of a NaN-filled buffer: a read of the padding poisons the result, a write
outside the view is found afterwards."""
import functools

import numpy as np
import pytest
import torch

from oracle import selfgnn_oracle as O
from sa_gnn_amd import _lib, ops
from test_gpu_fusion import ATOL, RTOL

pytestmark = pytest.mark.gpu

ATTN_KEYS = ("Wq", "bq", "Wk", "bk", "Wv", "bv")


# ---- layouts: (strides, offset) in floats; torch's device allocations start on a 512-byte boundary ------------------------

def x_layout(name, n, t, d):
    return {"padded": ((t * d + 4, d, 1), 4),            # aligned rows, four NaNs between the nodes
            "shift": ((t * d, d, 1), 5),                 # base one float past a 16-byte boundary
            "ld_n+1": ((t * d + 1, d, 1), 4),            # ld_n = t*d + 1
            "time_major": ((d, n * d + 2, 1), 4),        # [t, n, d] storage, ld_t = n*d + 2
            "time_major,vec": ((d, n * d + 4, 1), 4),    # [t, n, d] storage with 16-byte rows: ld_t = n*d + 4
            "shift,ld_n+1": ((t * d + 1, d, 1), 5)}[name]


class Slab:
    """`values` (or nothing yet) as a strided view of a NaN-filled device buffer."""

    def __init__(self, dev, shape, strides, offset, values=None):
        self.shape, self.strides, self.offset = tuple(shape), tuple(strides), offset
        size = offset + sum((s - 1) * st for s, st in zip(shape, strides)) + 1 + 4
        host = np.full(size, np.nan, dtype=np.float32)
        self.inside = np.zeros(size, dtype=bool)
        self._of(self.inside)[...] = True
        if values is not None:
            self._of(host)[...] = values
        self.buf = torch.from_numpy(host).to(dev)
        self.view = torch.as_strided(self.buf, self.shape, self.strides, offset)

    def _of(self, a):
        return np.lib.stride_tricks.as_strided(a[self.offset:], self.shape, [st * a.itemsize for st in self.strides])

    def read(self):
        """The view's values, once everything outside it is seen to be NaN still."""
        host = self.buf.cpu().numpy()
        assert np.isnan(host[~self.inside]).all(), "a write outside the view"
        return self._of(host).copy()


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def quarter_ok(a32, a64):
    """Rows at which the float32 oracle is within a quarter of the tolerance of the float64 one."""
    err = np.abs(a32.astype(np.float64) - a64)
    return (err <= 0.25 * (ATOL + RTOL * np.abs(a64))).reshape(len(a64), -1).all(axis=1)


def f64(p):
    return {k: v.astype(np.float64) for k, v in p.items()}


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def device_params(p, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in p.items()}


# ---- references, computed once per shape and shared ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lstm_reference(d, t, n):
    """x [n, t, d] standard normal, parameters, a 0 / 2 output mask, and float64 h without and with the mask."""
    rng = np.random.default_rng([1, d, t, n])
    m = n + n // 4 + 8                                   # spare rows for the screen
    x = rng.standard_normal((m, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    scale = ((rng.random((m, t, d)) < 0.5) * 2.0).astype(np.float32)
    p64 = f64(p)
    h32 = O.basic_lstm(x, p["lstm_W"], p["lstm_b"], 1.0)
    h64 = O.basic_lstm(x.astype(np.float64), p64["lstm_W"], p64["lstm_b"], 1.0)
    keep = np.flatnonzero(quarter_ok(h32, h64) & quarter_ok(h32 * scale, h64 * scale))[:n]
    assert len(keep) == n, f"only {len(keep)} of {m} rows pass the fp32 screen"
    return (p,) + frozen(x[keep], scale[keep], h64[keep], (h64 * scale)[keep])


def attention_outputs(x, p, heads):
    att = [p[k] for k in ATTN_KEYS]
    y = O.layer_norm_td(x, p["ln_gamma"], p["ln_beta"])
    return {"mhsa_mean": O.mhsa(x, *att, heads).mean(axis=1), "ln_mhsa_mean": O.mhsa(y, *att, heads).mean(axis=1),
            "interval_fusion": O.interval_fusion(x, p, heads)}


@functools.lru_cache(maxsize=None)
def attention_reference(d, heads, t, n):
    """x [n, t, d] standard normal, parameters and the float64 result of the three attention entries on it."""
    rng = np.random.default_rng([2, d, heads, t, n])
    m = n + n // 4 + 8
    x = rng.standard_normal((m, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    w32, w64 = attention_outputs(x, p, heads), attention_outputs(x.astype(np.float64), f64(p), heads)
    ok = np.ones(m, dtype=bool)
    for k in w64:
        ok &= quarter_ok(w32[k], w64[k])
    keep = np.flatnonzero(ok)[:n]
    assert len(keep) == n, f"only {len(keep)} of {m} rows pass the fp32 screen"
    x, = frozen(x[keep])
    return p, x, {k: frozen(v[keep])[0] for k, v in w64.items()}


# ---- LSTM forward --------------------------------------------------------------------------------------------------------
# (engine, d, t, n, layout). Layouts: an x layout of x_layout(); "h0_odd": h0 a row view with an odd stride;
# "h_unaligned": x aligned, `out` one float past a 16-byte boundary with ld_h = t*d + 1. Everywhere else `out` has
# ld_h = t*d + 4. n leaves a ragged last block: the Valu kernel takes (256 / d) * 4 rows per block, the fused ones 96.

def valu_rows(d):
    return 2 * (256 // d) * 4 + 3


LSTM_CASES = (
    # LSTM fwd, "any / otherwise / Valu": widths other than 32, 64, 128. d = 4 and 8 put 64 and 32 row slots in a block
    [("f16x2", d, t, n, "padded") for d, t, n in [(4, 64, 1031), (8, 3, 1000), (96, 5, 67), (160, 2, 33), (224, 1, 9), (252, 3, 19)]]
    # LSTM fwd, "valu / always / Valu": the widths the other engines take
    + [("valu", d, 4, valu_rows(d), "padded") for d in (32, 64, 128)]
    # LSTM fwd, rows 2-4 without "vec" -> "any / otherwise / Valu" (select_lstm_fwd's !vec), under both matrix engines
    + [(e, d, 5, valu_rows(d), lay) for e in ("f16x2", "f32") for d in (32, 64, 128)
       for lay in ("shift", "ld_n+1", "time_major", "h0_odd")]
    # LSTM fwd, "f16x2 / d = 128 ... h aligned / Split128" not met -> Valu
    + [("f16x2", 128, 5, 199, "h_unaligned")]
    # LSTM fwd, "F16x2" and "F32Mfma" rows ask for an aligned h (the f16 kernel stores 16-byte rows): not met -> Valu
    + [(e, d, 5, 199, "h_unaligned") for e in ("f16x2", "f32") for d in (32, 64)]
)


def lstm_out(dev, n, t, d, layout):
    return Slab(dev, (n, t, d), (t * d + 1, d, 1), 5) if layout == "h_unaligned" else Slab(dev, (n, t, d), (t * d + 4, d, 1), 4)


@pytest.mark.parametrize("engine,d,t,n,layout", LSTM_CASES, ids=lambda v: str(v))
def test_lstm_route(dev, engine, d, t, n, layout):
    """Plain, with a drop_scale mask, and cut in two with h0 / c0 / c_out (bit-identical to the whole)."""
    p, x, scale, want, want_dropped = lstm_reference(d, t, n)
    W, b = (torch.from_numpy(p[k]).to(dev) for k in ("lstm_W", "lstm_b"))
    xs = Slab(dev, (n, t, d), *x_layout(layout if layout in ("shift", "ld_n+1", "time_major") else "padded", n, t, d), values=x)
    with ops.engine(engine):
        whole = lstm_out(dev, n, t, d, layout)
        ops.lstm_fwd(xs.view, W, b, 1.0, out=whole.view)
        h = whole.read()
        close(h, want)
        if layout != "h0_odd":                           # that layout only differs in the continuation
            dropped = lstm_out(dev, n, t, d, layout)
            ops.lstm_fwd(xs.view, W, b, 1.0, drop_scale=torch.from_numpy(scale).to(dev), out=dropped.view)
            close(dropped.read(), want_dropped)
    # the continuation. t = 1 cannot be cut: there the explicit zero state stands in for the implicit one
    cut = t // 2
    parts = lstm_out(dev, n, t, d, layout)
    c = Slab(dev, (n, d), (d, 1), 4)
    if layout == "h0_odd":
        # the first part and the whole run on the Valu kernel, the second under the case's engine, which an unaligned h0
        # sends to the same kernel: equal bits
        with ops.engine("valu"):
            whole = lstm_out(dev, n, t, d, layout)
            ops.lstm_fwd(xs.view, W, b, 1.0, out=whole.view)
            h = whole.read()
            close(h, want)
            ops.lstm_fwd(xs.view[:, :cut], W, b, 1.0, out=parts.view[:, :cut], c_out=c.view)
        h0 = Slab(dev, (n, d), (d + 1, 1), 4, values=h[:, cut - 1])
        with ops.engine(engine):
            ops.lstm_fwd(xs.view[:, cut:], W, b, 1.0, out=parts.view[:, cut:], h0=h0.view, c0=c.view, c_out=c.view)
        h0.read()
    else:
        with ops.engine(engine):
            if cut:
                ops.lstm_fwd(xs.view[:, :cut], W, b, 1.0, out=parts.view[:, :cut], c_out=c.view)
                h0 = parts.view[:, cut - 1]
                if layout == "h_unaligned":              # an unaligned h0 would take the second part off the first's kernel
                    h0 = h0.contiguous()
            else:
                h0 = torch.zeros((n, d), device=dev)
                c.view.zero_()
            ops.lstm_fwd(xs.view[:, cut:], W, b, 1.0, out=parts.view[:, cut:], h0=h0, c0=c.view, c_out=c.view)
    assert np.array_equal(parts.read(), h), "a sequence cut in two differs from the whole"
    assert np.isfinite(c.read()).all()
    np.testing.assert_array_equal(xs.read(), x)


# ---- attention forward ---------------------------------------------------------------------------------------------------
# (engine, d, heads, t, n, x layout): ops.mhsa_mean, ops.ln_mhsa_mean and ops.interval_fusion each, `out` a row view with
# ld_out = d + 4. n leaves a ragged last block: 256 / d node slots in the Valu and wide kernels (halved until they fit
# 64 KiB of LDS), 4 * (32 / t) nodes in a tile of the matrix-core kernel.

def mfma_rows(t):
    return 4 * (32 // t) * 3 + 5


def wide_heads(d):
    return sorted({1, 16, 32, d})                        # 16 and 32 divide every wide d


ATTN_CASES = (
    # attention fwd, "f32,f16x2 / d % 32 = 0, 96 <= d <= 256 / Wide": the forward-only widths and the training ones
    [("f16x2", d, heads, t, 37, "padded") for d in (96, 160, 192, 224, 256) for heads in wide_heads(d) for t in (1, 7, 33)]
    # Wide at d = 128: heads other than 16 (d/heads = 1 is a power of two, but d is not 32 / 64), 16 heads at a t Split lacks
    + [("f16x2", 128, heads, 3, 37, "padded") for heads in (1, 8, 128)]
    + [("f16x2", 128, 16, t, 37, "padded") for t in (7, 10, 20, 32, 64)]
    # attention fwd, "f32,f16x2 / vec, d in {32, 64}, t <= 32, d/heads a power of 2 / F32Mfma": d_k from 1 to 64
    + [("f16x2", d, heads, t, mfma_rows(t), "padded") for d in (32, 64) for heads in sorted({1, 2, 8, 32, d}) for t in (1, 5, 12, 32)]
    # the same row under the f32 engine, where 16 heads do not go to Split
    + [("f32", d, 16, 3, mfma_rows(3), "padded") for d in (32, 64)]
    # attention fwd, "any / otherwise / Valu": widths no other row takes
    + [("f16x2", d, heads, t, 2 * (256 // d) + 1, "padded")
       for d, heads in [(4, 1), (4, 4), (8, 2), (48, 16), (100, 10), (252, 4)] for t in (1, 6)]
    # "otherwise / Valu": t > 32 at the F32Mfma widths. (64, 64) is t*d = 4096: one slot, exactly 64 KiB of LDS
    + [("f16x2", d, 16, t, 21, "padded") for d in (32, 64) for t in (33, 64)]
    # attention fwd, "valu / always / Valu"
    + [("valu", d, 16, 5, 2 * (256 // d) + 1, "padded") for d in (64, 128)]
    # rows 2-4 without "vec" -> Valu at d = 32 / 64; d = 128: Wide behind ln_mhsa_mean's layer norm, Valu in mhsa_mean (*)
    + [("f16x2", d, 16, 5, 21, lay) for d in (32, 64, 128) for lay in ("shift", "ld_n+1", "time_major", "shift,ld_n+1")]
    # Valu above 64 KiB of dynamic LDS: just above, d = 128 / 256 under the valu engine, (256, 40) = the 160 KiB cap itself
    + [("f16x2", 252, 4, 17, 9, "padded"), ("valu", 128, 16, 33, 9, "padded"), ("valu", 256, 16, 40, 9, "padded")]
    # Wide at its last t under the 160 KiB cap
    + [("f16x2", 256, 16, 53, 9, "padded")]
)


def attention_calls(x, pd, heads):
    att = [pd[k] for k in ATTN_KEYS]
    return {"mhsa_mean": lambda out: ops.mhsa_mean(x, *att, heads, out=out),
            "ln_mhsa_mean": lambda out: ops.ln_mhsa_mean(x, pd["ln_gamma"], pd["ln_beta"], *att, heads, out=out),
            "interval_fusion": lambda out: ops.interval_fusion(x, pd, heads, out=out)}


@pytest.mark.parametrize("engine,d,heads,t,n,layout", ATTN_CASES, ids=lambda v: str(v))
def test_attention_route(dev, engine, d, heads, t, n, layout):
    p, x, want = attention_reference(d, heads, t, n)
    pd = device_params(p, dev)
    xs = Slab(dev, (n, t, d), *x_layout(layout, n, t, d), values=x)
    with ops.engine(engine):
        for name, call in attention_calls(xs.view, pd, heads).items():
            out = Slab(dev, (n, d), (d + 4, 1), 4)
            call(out.view)
            np.testing.assert_allclose(out.read(), want[name], rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_array_equal(xs.read(), x)


def test_mhsa_mean_entry_without_a_workspace_at_a_wide_width(dev):
    """attention fwd, "Wide (*)": sagnn_mhsa_mean_f32 has no workspace and runs Valu where the table says Wide
    (ops.mhsa_mean calls the wide entry there, so this one goes through ctypes)."""
    d, heads, t, n = 128, 8, 3, 37
    p, x, want = attention_reference(d, heads, t, n)
    pd = device_params(p, dev)
    xs = Slab(dev, (n, t, d), *x_layout("padded", n, t, d), values=x)
    out = Slab(dev, (n, d), (d + 4, 1), 4)
    ops.check(_lib.load().sagnn_mhsa_mean_f32(xs.view.data_ptr(), t * d + 4, d, n, t, d, heads, *(pd[k].data_ptr() for k in ATTN_KEYS),
                                              out.view.data_ptr(), d + 4, ops._stream()))
    close(out.read(), want["mhsa_mean"])


@pytest.mark.parametrize("engine,d,t", [("valu", 256, 41), ("f16x2", 256, 54)], ids=["valu", "wide"])
def test_attention_past_the_lds_cap_is_a_dimension_error(dev, engine, d, t):
    """One node slot of t*d above 160 KiB (Valu: 4 t d floats, Wide: 3 t d): SAGNN_ERR_DIM from every entry, never a
    positive (HIP) code from a refused launch."""
    n, heads = 5, 16
    rng = np.random.default_rng(t)
    pd = device_params(O.init_fusion_params(d, rng), dev)
    x = torch.from_numpy(rng.standard_normal((n, t, d)).astype(np.float32)).to(dev)
    with ops.engine(engine):
        for name, call in attention_calls(x, pd, heads).items():
            with pytest.raises(_lib.SagnnError) as e:
                call(torch.empty((n, d), device=dev))
            assert e.value.code == -2, f"{name}: {e.value}"
    torch.cuda.synchronize()


# ---- layer norm ----------------------------------------------------------------------------------------------------------
# One wavefront per node, four nodes per block: n = 37. Rows 0, 5 and n - 1 are all zero: mean 0, variance 0, and
# x*inv + (beta - mean*inv) is beta exactly. No other constant rows: with eps = 1e-12 the fp32 rounding of their mean is
# amplified 1e6 times, in the float32 oracle as much as in any kernel.

LN_LAYOUTS = ("padded", "time_major", "shift", "ld_n+1", "shift,ld_n+1")


@functools.lru_cache(maxsize=None)
def layernorm_reference(d, t, n):
    rng = np.random.default_rng([3, d, t, n])
    m = n + n // 4 + 8
    x = (rng.standard_normal((m, t, d)) * 2 + 0.5).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    y32 = O.layer_norm_td(x, p["ln_gamma"], p["ln_beta"])
    y64 = O.layer_norm_td(x.astype(np.float64), *(p[k].astype(np.float64) for k in ("ln_gamma", "ln_beta")))
    keep = np.flatnonzero(quarter_ok(y32, y64))[:n]
    assert len(keep) == n
    x, y64 = x[keep], y64[keep]
    zero = [0, 5, n - 1]
    x[zero] = 0.0
    y64[zero] = p["ln_beta"].astype(np.float64)
    return (p, zero) + frozen(x, y64)


@pytest.mark.parametrize("layout", LN_LAYOUTS)
@pytest.mark.parametrize("d,t", [(4, 1), (8, 3), (252, 5), (64, 64)])
def test_layernorm_views(dev, d, t, layout):
    n = 37
    p, zero, x, want = layernorm_reference(d, t, n)
    gamma, beta = (torch.from_numpy(p[k]).to(dev) for k in ("ln_gamma", "ln_beta"))
    xs = Slab(dev, (n, t, d), *x_layout(layout, n, t, d), values=x)
    out = Slab(dev, (n, t, d), (t * d + 4, d, 1), 4)
    ops.layernorm_td(xs.view, gamma, beta, out=out.view)
    got = out.read()
    close(got, want)
    assert np.array_equal(got[zero], np.broadcast_to(p["ln_beta"], (len(zero), t, d)))
    np.testing.assert_array_equal(xs.read(), x)
    if layout != "time_major":                           # in place needs each node's (t, d) block dense
        ops.layernorm_td(xs.view, gamma, beta, out=xs.view)
        got = xs.read()
        close(got, want)
        assert np.array_equal(got[zero], np.broadcast_to(p["ln_beta"], (len(zero), t, d)))
