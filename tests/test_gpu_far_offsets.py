"""GPU parity at offsets past 2^31 elements: the fusion, dense and row-movement entries with operands whose checked rows
lie more than 2^29, 2^30 and 2^31 floats from the pointer the entry is given (a signed 32-bit byte offset, an unsigned one,
a signed 32-bit element index). The case tables and their arithmetic are tests/far_offsets_ref.py, checked on the CPU by
tests/test_far_offsets_host.py.

Every operand is a window of a device buffer filled with NaN on the device. After the call the number of non-NaN floats
in each output buffer, counted on the device in chunks, must equal the window's size, and the window must hold no NaN:
together they find a skipped row and a write outside the window anywhere in the buffer. Every entry is called on the test
thread through the raw library under the case's engine (Run holds it; the GNN stack goes through ops.gnn_stack /
ops.gnn_stack_bwd, which build the argument struct and pass the views' strides on unchanged); each case asserts the route label of the restated selectors.
Bounds are those of the route tests, never wider, on the references those tests screen (float32 within a quarter of the
bound). Each case prints its worst error as a fraction of its bound and its peak device memory before it asserts.

The accumulators dW and db are zero windows with a band of zeros and then NaNs around them (test_gpu_bwd_routes.Window).
Workspaces the library only scratches in are plain device tensors.

A case skips only when the device reports less free memory than the case's buffers need."""
import functools
import time

import numpy as np
import pytest
import torch

import far_offsets_ref as R
import gru_ref as G
from oracle import selfgnn_oracle as O
from sa_gnn_amd import _lib, ops
from test_gpu_backward import _close
from test_gpu_bwd_routes import Window, bptt_reference, front_fractions, front_reference, tail_reference
from test_gpu_dense_routes import NN_ATOL, NN_RTOL, TN_ATOL, TN_MAG, TN_RTOL
from test_gpu_f16_range import _per_row_ok
from test_gpu_fusion import ATOL, RTOL
from test_gpu_fusion_routes import ATTN_KEYS, attention_reference, device_params, f64, frozen, lstm_reference, quarter_ok

pytestmark = pytest.mark.gpu

CHUNK = 1 << 28                                          # floats per counting step: 1 GiB


class Far:
    """One operand: `op`'s window inside a NaN-filled device buffer, PAD NaNs before and after it."""

    def __init__(self, dev, op, values=None):
        self.op = op
        self.buf = torch.full((R.buffer_floats(op),), float("nan"), dtype=torch.float32, device=dev)
        self.view = torch.as_strided(self.buf, op.shape, op.strides, R.PAD)
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 0
        if values is not None:
            self.put(values)

    def put(self, values, nodes=None):
        v = torch.from_numpy(np.array(values, dtype=np.float32)).to(self.buf.device)   # a copy: the references are read-only
        if nodes is None:
            self.view.copy_(v)
        else:
            self.view[nodes] = v

    def numel(self):
        return int(np.prod(self.op.shape))

    def written(self):
        """How many floats of the whole buffer are not NaN."""
        return sum(int((c == c).sum()) for c in self.buf.split(CHUNK))

    def check_written(self, what):
        """Every element of the window stored, nothing outside it."""
        got = self.written()
        assert got == self.numel(), f"{what} {self.op.name}: {got} floats written in the buffer, the window holds {self.numel()}"
        assert not bool(torch.isnan(self.view).any()), f"{what} {self.op.name}: NaN inside the window"

    def read(self, nodes=None):
        return (self.view if nodes is None else self.view[nodes]).cpu().numpy()

    def free(self):
        self.buf = self.view = None


class Run:
    """A case's buffers, its engine, its memory check and its report. close(), which every test calls in a `finally`,
    restores the caller's engine and frees the buffers."""

    def __init__(self, dev, case):
        self.dev, self.case, self.fars, self.t0 = dev, case, [], time.perf_counter()
        need = R.case_bytes(case)
        assert need <= R.CAP_BYTES
        free = torch.cuda.mem_get_info(dev)[0]
        if free < need:
            pytest.skip(f"{R.case_id(case)}: needs {need} bytes of device memory, {free} free")
        torch.cuda.reset_peak_memory_stats(dev)
        self.engine = ops.engine(case.engine)            # every library call of the case runs under the case's engine
        self.engine.__enter__()

    def far(self, name, values=None):
        op, = (o for o in self.case.operands if o.name == name)
        f = Far(self.dev, op, values)
        self.fars.append(f)
        return f

    def report(self, **fractions):
        peak = torch.cuda.max_memory_allocated(self.dev)
        worst = " ".join(f"{k}={v:.4f}" for k, v in fractions.items())
        print(f"far_offsets|{R.case_id(self.case)}|n={self.case.n}|worst error / bound: {worst}|peak {peak / 2 ** 30:.2f} GiB"
              f"|{time.perf_counter() - self.t0:.2f} s")
        for k, v in fractions.items():
            assert v <= 1.0, f"{R.case_id(self.case)}: {k} at {v:.3f} of its bound"

    def close(self):
        self.engine.__exit__(None, None, None)
        for f in self.fars:
            f.free()
        self.fars.clear()
        torch.cuda.empty_cache()


def fraction(got, want, atol=ATOL, rtol=RTOL):
    return float((np.abs(got.astype(np.float64) - want) / (atol + rtol * np.abs(want))).max())


def close_fraction(got, want, floor=0.0):
    """The worst error as a fraction of test_gpu_backward._close's bound."""
    b = want.detach().numpy()
    return float((np.abs(got.astype(np.float64).reshape(b.shape) - b) / (1e-4 * np.abs(b) + 2e-5 * np.abs(b).max() + floor)).max())


def ids(cases):
    return [R.case_id(c) for c in cases]


def dev_f32(dev, a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)


def fill_normal(far, gen):
    """Standard normal over the whole window of a contiguous operand, drawn on the device."""
    far.buf[R.PAD:R.PAD + R.span(far.op)].normal_(generator=gen)


def sums(dev, rows, cols):
    """A [rows, cols] accumulator of zeros the kernels add to with float atomics, as test_gpu_bwd_routes guards them: a band
    of zeros and then NaNs on both sides, so that an add or a store outside it is found when it is read."""
    return Window(dev, rows, cols, 32 * cols, band=32 * cols)


def rows_not_zero(view):
    """How many nodes of a device view hold anything but exact zeros."""
    return int((view.reshape(view.shape[0], -1) != 0).any(dim=1).sum())


# ---- LSTM forward ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.LSTM_A, ids=ids(R.LSTM_A))
def test_lstm_far_by_stride(dev, case):
    """The guards at their edges are among these: ld_h = 2^22 - 4 runs F16x2, ld_h = 2^22 runs F32Mfma, ld_n = ld_h =
    2^24 - 4 is the last stride F32Mfma admits."""
    x_op, h_op = case.operands
    assert R.lstm_route(case.engine, case.d, case.t, h_op.strides[0]) == case.route
    p, x, _, want, _ = lstm_reference(case.d, case.t, case.n)
    run = Run(dev, case)
    try:
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, hs = run.far("x", x), run.far("h")
        with ops.engine(case.engine):
            ops.check(_lib.load().sagnn_lstm_fwd_f32(xs.ptr, x_op.strides[0], x_op.strides[1], case.n, case.t, case.d, W.data_ptr(),
                                                     b.data_ptr(), 1.0, None, hs.ptr, h_op.strides[0], ops._stream()))
        hs.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and np.array_equal(xs.read(), x), "x changed"
        run.report(h=fraction(hs.read(), want))
    finally:
        run.close()


@pytest.mark.parametrize("case", R.LSTM_STATE, ids=ids(R.LSTM_STATE))
def test_lstm_state_with_a_far_h_init(dev, case):
    """A sequence cut in two: the second call continues from h_init rows 2^26 floats apart."""
    d, t, n = case.d, case.t, case.n
    assert R.lstm_route(case.engine, d, t, t * d + 4) == case.route
    p, x, _, want, _ = lstm_reference(d, t, n)
    cut = t // 2
    run = Run(dev, case)
    try:
        lib = _lib.load()
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, hs, hi, c = run.far("x", x), run.far("h"), run.far("h_init"), run.far("c")
        ld_n, ld_h, ld_hi = xs.op.strides[0], hs.op.strides[0], hi.op.strides[0]
        with ops.engine(case.engine):
            ops.check(lib.sagnn_lstm_fwd_state_f32(xs.ptr, ld_n, d, n, cut, d, W.data_ptr(), b.data_ptr(), 1.0, None, None, 0, None,
                                                   hs.ptr, ld_h, c.ptr, ops._stream()))
            hi.view.copy_(hs.view[:, cut - 1])
            ops.check(lib.sagnn_lstm_fwd_state_f32(xs.ptr + 4 * cut * d, ld_n, d, n, t - cut, d, W.data_ptr(), b.data_ptr(), 1.0, None,
                                                   hi.ptr, ld_hi, c.ptr, hs.ptr + 4 * cut * d, ld_h, c.ptr, ops._stream()))
        hs.check_written(R.case_id(case))
        c.check_written(R.case_id(case))
        assert hi.written() == hi.numel()
        run.report(h=fraction(hs.read(), want))
    finally:
        run.close()


@pytest.mark.parametrize("case", R.LSTM_B, ids=ids(R.LSTM_B))
def test_lstm_far_by_count(dev, case):
    """The workload's own form: x the time-major [T, N, d] slab, h [n, t, d] dense and past 2^31 floats; plain, then with a
    0 / 2 output mask [n, t, d] of the same length. Inputs are standard normal drawn on the device; the checked nodes carry
    the screened rows of lstm_reference."""
    d, t, n = case.d, case.t, case.n
    x_op, h_op, _ = case.operands
    assert R.lstm_route(case.engine, d, t, t * d) == case.route
    chk = h_op.checked
    p, x, scale, want, want_dropped = lstm_reference(d, t, len(chk))
    run = Run(dev, case)
    try:
        lib = _lib.load()
        gen = torch.Generator(device=dev).manual_seed(31)
        nodes = torch.tensor(chk, device=dev)
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, hs = run.far("x"), run.far("h")
        xs.buf[R.PAD:R.PAD + R.span(x_op)].normal_(generator=gen)
        xs.put(x, nodes)
        with ops.engine(case.engine):
            ops.check(lib.sagnn_lstm_fwd_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, W.data_ptr(), b.data_ptr(), 1.0, None,
                                             hs.ptr, h_op.strides[0], ops._stream()))
        hs.check_written(R.case_id(case))
        f_plain = fraction(hs.read(nodes), want)
        hs.buf.fill_(float("nan"))
        drop = run.far("drop")
        drop.view.bernoulli_(0.5, generator=gen).mul_(2.0)
        drop.put(scale, nodes)
        with ops.engine(case.engine):
            ops.check(lib.sagnn_lstm_fwd_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, W.data_ptr(), b.data_ptr(), 1.0,
                                             drop.ptr, hs.ptr, h_op.strides[0], ops._stream()))
        hs.check_written(R.case_id(case) + " masked")
        f_masked = fraction(hs.read(nodes), want_dropped)
        run.report(h=f_plain, h_masked=f_masked)
    finally:
        run.close()


def lstm_saved(x, W, b):
    """numpy, in x's dtype: h, gates [n, t, 4d] = sigmoid(i) | tanh(j) | sigmoid(f + 1) | sigmoid(o) and cell, as
    sagnn_lstm_fwd_train_f32 stores them (oracle basic_lstm, keeping what it computes on the way)."""
    n, t, d = x.shape
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))             # noqa: E731
    h, c, one = np.zeros((n, d), x.dtype), np.zeros((n, d), x.dtype), np.asarray(1.0, x.dtype)
    hs, gs, cs = [], [], []
    for ts in range(t):
        gi, gj, gf, go = np.split(np.concatenate([x[:, ts], h], axis=1) @ W + b, 4, axis=1)
        act = [sig(gi), np.tanh(gj), sig(gf + one), sig(go)]
        c = c * act[2] + act[0] * act[1]
        h = np.tanh(c) * act[3]
        hs.append(h), gs.append(np.concatenate(act, axis=1)), cs.append(c)
    return tuple(np.stack(a, axis=1) for a in (hs, gs, cs))


@functools.lru_cache(maxsize=None)
def train_reference(d, t, n):
    """x, parameters, a 0 / 2 mask and float64 (h, gates, cell), on nodes where float32 numpy stays within a quarter of the
    bound of h (test_gpu_fusion's) on all three: gates and cell are what h is made of, one bounded function away."""
    rng = np.random.default_rng([17, d, t, n])
    m = n + n // 4 + 8
    x = rng.standard_normal((m, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    scale = ((rng.random((m, t, d)) < 0.5) * 2.0).astype(np.float32)
    p64 = f64(p)
    s32, s64 = lstm_saved(x, p["lstm_W"], p["lstm_b"]), lstm_saved(x.astype(np.float64), p64["lstm_W"], p64["lstm_b"])
    ok = np.ones(m, dtype=bool)
    for a32, a64 in zip(s32, s64):
        ok &= quarter_ok(a32, a64)
    ok &= quarter_ok(s32[0] * scale, s64[0] * scale)
    keep = np.flatnonzero(ok)[:n]
    assert len(keep) == n, f"only {len(keep)} of {m} rows pass the fp32 screen"
    return (p,) + frozen(x[keep], scale[keep], *(a[keep] for a in s64))


@pytest.mark.parametrize("case", R.TRAIN_B, ids=ids(R.TRAIN_B))
def test_lstm_train_far_by_count(dev, case):
    """sagnn_lstm_fwd_train_f32 with gates [n, t, 4d] past 2^31 floats: h, gates and cell at the checked nodes."""
    d, t, n = case.d, case.t, case.n
    masked = any(op.name == "drop" for op in case.operands)
    assert R.lstm_route(case.engine, d, t, t * d, train=True, drop=masked) == case.route
    x_op = case.operands[0]
    chk = x_op.checked
    p, x, scale, want_h, want_g, want_c = train_reference(d, t, len(chk))
    run = Run(dev, case)
    try:
        gen = torch.Generator(device=dev).manual_seed(32)
        nodes = torch.tensor(chk, device=dev)
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, hs, gs, cs = run.far("x"), run.far("h"), run.far("gates"), run.far("cell")
        fill_normal(xs, gen)
        xs.put(x, nodes)
        drop = None
        if masked:
            drop = run.far("drop")
            drop.view.bernoulli_(0.5, generator=gen).mul_(2.0)
            drop.put(scale, nodes)
        with ops.engine(case.engine):
            ops.check(_lib.load().sagnn_lstm_fwd_train_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, W.data_ptr(), b.data_ptr(),
                                                           1.0, drop.ptr if masked else None, hs.ptr, t * d, gs.ptr, cs.ptr, ops._stream()))
        for o in (hs, gs, cs):
            o.check_written(R.case_id(case))
        run.report(h=fraction(hs.read(nodes), want_h * scale if masked else want_h), gates=fraction(gs.read(nodes), want_g),
                   cell=fraction(cs.read(nodes), want_c))
    finally:
        run.close()


# ---- attention forward -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.ATTN_A, ids=ids(R.ATTN_A))
def test_attention_far_by_stride(dev, case):
    d, t, heads, n = case.d, case.t, case.heads, case.n
    assert R.attn_route(case.engine, d, t, heads) == case.route
    p, x, want = attention_reference(d, heads, t, n)
    run = Run(dev, case)
    try:
        lib = _lib.load()
        pd = device_params(p, dev)
        att = [pd[k].data_ptr() for k in ATTN_KEYS]
        xs, out = run.far("x", x), run.far("out")
        ld_n, ld_out = xs.op.strides[0], out.op.strides[0]
        with ops.engine(case.engine):
            if case.entry == "ln_mhsa_mean":
                need = int(lib.sagnn_ln_mhsa_mean_workspace_bytes(n, t, d, heads))
                assert need == R.attn_workspace_bytes(case.route, n, t, d)
                ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=dev)
                ops.check(lib.sagnn_ln_mhsa_mean_f32(xs.ptr, ld_n, d, n, t, d, heads, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(),
                                                     1e-12, *att, out.ptr, ld_out, ws.data_ptr(), need, ops._stream()))
            else:
                need = int(lib.sagnn_interval_fusion_workspace_bytes(n, t, d))
                ws = torch.empty(max(need // 4, 4), dtype=torch.float32, device=dev)
                ops.check(lib.sagnn_interval_fusion_f32(xs.ptr, ld_n, d, n, t, d, heads, pd["lstm_W"].data_ptr(), pd["lstm_b"].data_ptr(),
                                                        1.0, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(), 1e-12, *att, out.ptr,
                                                        ld_out, ws.data_ptr(), need, ops._stream()))
        out.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and np.array_equal(xs.read(), x), "x changed"
        run.report(out=fraction(out.read(), want[case.entry]))
    finally:
        run.close()


@pytest.mark.parametrize("case", R.ATTN_B, ids=ids(R.ATTN_B))
def test_attention_far_by_count(dev, case):
    """x the time-major [T, N, d] slab past 2^31 floats."""
    d, t, heads, n = case.d, case.t, case.heads, case.n
    assert R.attn_route(case.engine, d, t, heads) == case.route
    x_op = case.operands[0]
    chk = x_op.checked
    p, x, want = attention_reference(d, heads, t, len(chk))
    run = Run(dev, case)
    try:
        lib = _lib.load()
        gen = torch.Generator(device=dev).manual_seed(33)
        nodes = torch.tensor(chk, device=dev)
        pd = device_params(p, dev)
        att = [pd[k].data_ptr() for k in ATTN_KEYS]
        xs, out = run.far("x"), run.far("out")
        fill_normal(xs, gen)
        xs.put(x, nodes)
        with ops.engine(case.engine):
            if case.entry == "ln_mhsa_mean":
                assert int(lib.sagnn_ln_mhsa_mean_workspace_bytes(n, t, d, heads)) == 0
                ops.check(lib.sagnn_ln_mhsa_mean_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, heads, pd["ln_gamma"].data_ptr(),
                                                     pd["ln_beta"].data_ptr(), 1e-12, *att, out.ptr, d, None, 0, ops._stream()))
            else:
                ws = run.far("workspace")
                need = int(lib.sagnn_interval_fusion_workspace_bytes(n, t, d))
                assert need <= 4 * ws.numel()
                ops.check(lib.sagnn_interval_fusion_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, heads, pd["lstm_W"].data_ptr(),
                                                        pd["lstm_b"].data_ptr(), 1.0, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(),
                                                        1e-12, *att, out.ptr, d, ws.ptr, need, ops._stream()))
        out.check_written(R.case_id(case))
        assert xs.written() == xs.numel()
        run.report(out=fraction(out.read(nodes), want[case.entry]))
    finally:
        run.close()


# ---- attention backward front ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.FRONT_A, ids=ids(R.FRONT_A))
def test_front_far_by_stride(dev, case):
    d, t, heads, n = case.d, case.t, case.heads, case.n
    assert R.front_route(case.engine, d, t, heads) == case.route
    p, x, gout, want, _ = front_reference(d, t, heads, n)
    y64, dq64 = want[True]
    run = Run(dev, case)
    try:
        pd = device_params(p, dev)
        xs, g, dq, y = run.far("x", x), run.far("g_out", gout), run.far("dqkv"), run.far("y")
        with ops.engine(case.engine):
            assert ops.attn_bwd_front_supported(d, t, heads)
            ops.check(_lib.load().sagnn_attn_bwd_front_f32(
                xs.ptr, xs.op.strides[0], d, n, t, d, heads, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(), 1e-12, 1,
                *(pd[k].data_ptr() for k in ATTN_KEYS), g.ptr, g.op.strides[0], dq.ptr, y.ptr, ops._stream()))
        dq.check_written(R.case_id(case))
        y.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and g.written() == g.numel()
        got = dq.read()
        fy, fg, fn = (float(f.max()) for f in front_fractions(y.read().reshape(n, t, d), got, y64, dq64, n))
        _per_row_ok(got.reshape(n, -1), dq64.reshape(n, -1), f"{R.case_id(case)}: dqkv per node")
        run.report(y=fy, dqkv_global=fg, dqkv_node=fn)
    finally:
        run.close()


@pytest.mark.parametrize("case", R.FRONT_B, ids=ids(R.FRONT_B))
def test_front_far_by_count(dev, case):
    """dqkv [n t, 3d] past 2^31 floats, y with it."""
    d, t, heads, n = case.d, case.t, case.heads, case.n
    assert R.front_route(case.engine, d, t, heads) == case.route
    chk = case.operands[0].checked
    m = len(chk)
    p, x, gout, want, _ = front_reference(d, t, heads, m)
    y64, dq64 = want[True]
    run = Run(dev, case)
    try:
        gen = torch.Generator(device=dev).manual_seed(34)
        nodes = torch.tensor(chk, device=dev)
        pd = device_params(p, dev)
        xs, g, dq, y = run.far("x"), run.far("g_out"), run.far("dqkv"), run.far("y")
        fill_normal(xs, gen), fill_normal(g, gen)
        xs.put(x, nodes), g.put(gout, nodes)
        with ops.engine(case.engine):
            assert ops.attn_bwd_front_supported(d, t, heads)
            ops.check(_lib.load().sagnn_attn_bwd_front_f32(
                xs.ptr, t * d, d, n, t, d, heads, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(), 1e-12, 1,
                *(pd[k].data_ptr() for k in ATTN_KEYS), g.ptr, d, dq.ptr, y.ptr, ops._stream()))
        dq.check_written(R.case_id(case))
        y.check_written(R.case_id(case))
        got = dq.read(nodes).reshape(m * t, 3 * d)
        fy, fg, fn = (float(f.max()) for f in front_fractions(y.read(nodes), got, y64, dq64, m))
        _per_row_ok(got.reshape(m, -1), dq64.reshape(m, -1), f"{R.case_id(case)}: dqkv per node")
        run.report(y=fy, dqkv_global=fg, dqkv_node=fn)
    finally:
        run.close()


# ---- attention backward tail -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.TAIL_B, ids=ids(R.TAIL_B))
def test_tail_far_by_count(dev, case):
    """rows x 3d past 2^31 floats; dy is written in place over y. The gradient is zero everywhere but the checked rows,
    so float64's dW and db are sums over those rows alone and a mis-addressed far row loses its contribution; every other
    row of dy must come out exactly zero. Bounds: test_gpu_bwd_routes.test_tail_route's arithmetic kind."""
    d, rows = case.d, case.n
    assert R.tail_route(case.engine, d) == case.route
    chk = case.operands[1].checked
    y0, dqkv, W, (want_dy, want_dW, want_db) = tail_reference(d, len(chk), "arith")
    run = Run(dev, case)
    try:
        gen = torch.Generator(device=dev).manual_seed(35)
        nodes = torch.tensor(chk, device=dev)
        yw, gw = run.far("y"), run.far("dqkv")
        fill_normal(yw, gen)
        gw.view.zero_()
        yw.put(y0, nodes), gw.put(dqkv, nodes)
        Wd = dev_f32(dev, W)
        dW, db = sums(dev, d, 3 * d), sums(dev, 1, 3 * d)
        with ops.engine(case.engine):
            ops.check(_lib.load().sagnn_attn_bwd_tail_f32(yw.ptr, gw.ptr, rows, d, Wd.data_ptr(), dW.ptr, db.ptr,
                                                          ops._stream()))
        yw.check_written(R.case_id(case))
        assert gw.written() == gw.numel() and rows_not_zero(gw.view) == len(chk), "dqkv changed"
        assert rows_not_zero(yw.view) == len(chk), "dy of a row without gradient is not zero"
        got_dy, got_dW, got_db = yw.read(nodes), dW.read(), db.read()[0]
        _per_row_ok(got_dy, want_dy, f"{R.case_id(case)}: dy")
        y64, g64 = y0.astype(np.float64), dqkv.astype(np.float64)
        f_dy = float((np.abs(got_dy - want_dy).max(axis=1) / (1e-4 * np.abs(want_dy).max(axis=1))).max())
        f_dW = float((np.abs(got_dW - want_dW) / (1e-4 * np.abs(want_dW) + 2e-6 * (np.abs(y64).T @ np.abs(g64)))).max())
        f_db = float((np.abs(got_db - want_db) / (1e-4 * np.abs(want_db) + 2e-6 * np.abs(g64).sum(axis=0))).max())
        run.report(dy=f_dy, dW=f_dW, db=f_db)
    finally:
        run.close()


# ---- BPTT ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.BPTT_A, ids=ids(R.BPTT_A))
def test_bptt_far_by_stride(dev, case):
    """x and dh_ext at ld_n = ld_dhe = 2^25 - 4, the last stride the BPTT admits."""
    d, t, n = case.d, case.t, case.n
    workspace = case.route == "SplitDw"
    assert R.bptt_route(case.engine, d, workspace) == case.route
    p, x, dh, _, want = bptt_reference(d, t, n)
    want_dx, want_dW, want_db = want[False]
    run = Run(dev, case)
    try:
        lib = _lib.load()
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, dhe, dx = run.far("x", x), run.far("dh_ext", dh), run.far("dx")
        h, gates, cell = run.far("h"), run.far("gates"), run.far("cell")
        ws = run.far("workspace") if workspace else None
        ld = xs.op.strides[0]
        xf = run.far("x_fwd", x)
        dW, db = sums(dev, 2 * d, 4 * d), sums(dev, 1, 4 * d)
        with ops.engine(case.engine):
            ops.check(lib.sagnn_lstm_fwd_train_f32(xf.ptr, xf.op.strides[0], d, n, t, d, W.data_ptr(), b.data_ptr(), 1.0, None, h.ptr, t * d, gates.ptr,
                                                   cell.ptr, ops._stream()))
            for o in (h, gates, cell):
                o.check_written(R.case_id(case) + " forward")
            ops.check(lib.sagnn_lstm_bwd_ws_f32(xs.ptr, ld, d, h.ptr, gates.ptr, cell.ptr, dhe.ptr, dhe.op.strides[0], None, W.data_ptr(),
                                                dx.ptr, dW.ptr, db.ptr, n, t, d, ws.ptr if ws else None,
                                                4 * ws.numel() if ws else 0, ops._stream()))
        dx.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and dhe.written() == dhe.numel()
        got_dx = dx.read().reshape(n, t, d)
        floor = float(np.finfo(np.float32).eps) * np.sqrt(n * t)      # db cancels to ~0 in places: test_gpu_bwd_routes
        fr = {"dx": close_fraction(got_dx, want_dx), "dW": close_fraction(dW.read(), want_dW),
              "db": close_fraction(db.read()[0], want_db, floor)}
        print(f"far_offsets|{R.case_id(case)}|" + " ".join(f"{k}={v:.4f}" for k, v in fr.items()))
        what = R.case_id(case)
        _close(f"{what}: dx", torch.from_numpy(got_dx), want_dx)
        _close(f"{what}: dW", torch.from_numpy(dW.read()), want_dW)
        _close(f"{what}: db", torch.from_numpy(db.read()[0]), want_db, floor=floor)
        run.report(**fr)
    finally:
        run.close()


@pytest.mark.parametrize("case", R.BPTT_B, ids=ids(R.BPTT_B))
def test_bptt_far_by_count(dev, case):
    """gates [n, t, 4d] past 2^31 floats (and the SplitDw workspace [t, n, 4d] with them). The upstream gradient is zero
    everywhere but the checked nodes: float64's dW and db are sums over those nodes alone, and dx of every other node must
    come out exactly zero."""
    d, t, n = case.d, case.t, case.n
    workspace = case.route == "SplitDw"
    assert R.bptt_route(case.engine, d, workspace) == case.route
    x_op = case.operands[0]
    chk = x_op.checked
    m = len(chk)
    p, x, dh, _, want = bptt_reference(d, t, m)
    want_dx, want_dW, want_db = want[False]
    run = Run(dev, case)
    try:
        lib = _lib.load()
        gen = torch.Generator(device=dev).manual_seed(36)
        nodes = torch.tensor(chk, device=dev)
        W, b = dev_f32(dev, p["lstm_W"]), dev_f32(dev, p["lstm_b"])
        xs, dhe, dx = run.far("x"), run.far("dh_ext"), run.far("dx")
        h, gates, cell = run.far("h"), run.far("gates"), run.far("cell")
        ws = run.far("workspace") if workspace else None
        fill_normal(xs, gen)
        dhe.view.zero_()
        xs.put(x, nodes), dhe.put(dh, nodes)
        dW, db = sums(dev, 2 * d, 4 * d), sums(dev, 1, 4 * d)
        with ops.engine(case.engine):
            ops.check(lib.sagnn_lstm_fwd_train_f32(xs.ptr, x_op.strides[0], x_op.strides[1], n, t, d, W.data_ptr(), b.data_ptr(), 1.0, None,
                                                   h.ptr, t * d, gates.ptr, cell.ptr, ops._stream()))
            for o in (h, gates, cell):
                o.check_written(R.case_id(case) + " forward")
            ops.check(lib.sagnn_lstm_bwd_ws_f32(xs.ptr, x_op.strides[0], x_op.strides[1], h.ptr, gates.ptr, cell.ptr, dhe.ptr, t * d, None,
                                                W.data_ptr(), dx.ptr, dW.ptr, db.ptr, n, t, d, ws.ptr if ws else None,
                                                4 * ws.numel() if ws else 0, ops._stream()))
        dx.check_written(R.case_id(case))
        assert rows_not_zero(dx.view) == m, "dx of a node without gradient is not zero"
        got_dx = dx.read(nodes)
        floor = float(np.finfo(np.float32).eps) * np.sqrt(m * t)
        fr = {"dx": close_fraction(got_dx, want_dx), "dW": close_fraction(dW.read(), want_dW),
              "db": close_fraction(db.read()[0], want_db, floor)}
        print(f"far_offsets|{R.case_id(case)}|" + " ".join(f"{k}={v:.4f}" for k, v in fr.items()))
        what = R.case_id(case)
        _close(f"{what}: dx", torch.from_numpy(got_dx), want_dx)
        _close(f"{what}: dW", torch.from_numpy(dW.read()), want_dW)
        _close(f"{what}: db", torch.from_numpy(db.read()[0]), want_db, floor=floor)
        run.report(**fr)
    finally:
        run.close()


# ---- GRU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GRU_A, ids=ids(R.GRU_A))
def test_gru_far_by_stride(dev, case):
    d, t, n = case.d, case.t, case.n
    x_op, h_op = case.operands
    rng = np.random.default_rng([12, d, t, n])
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = G.init_gru_params(d, rng)
    w = [p[k] for k in G.GRU_KEYS]
    want = G.gru(x, *w)
    run = Run(dev, case)
    try:
        assert ops.gru_fused_supported(d)
        wd = [dev_f32(dev, a) for a in w]
        xs, hs = run.far("x", x), run.far("h")
        with ops.engine(case.engine):
            ops.check(_lib.load().sagnn_gru_fwd_f32(xs.ptr, x_op.strides[0], d, n, t, d, *(a.data_ptr() for a in wd), None, hs.ptr,
                                                    h_op.strides[0], None, None, None, 0, ops._stream()))
        hs.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and np.array_equal(xs.read(), x), "x changed"
        run.report(h=fraction(hs.read(), want))
    finally:
        run.close()


def gru_cand_reference(gates, cand, h, dh_ext, dh_rec, ts):
    """float64, the header's formulas: (da_c, du, dh_u) of gru_bwd_cand at step ts."""
    gates, cand, h, dh_ext, dh_rec = (np.asarray(a, dtype=np.float64) for a in (gates, cand, h, dh_ext, dh_rec))
    d = cand.shape[2]
    u, c = gates[:, ts, d:], cand[:, ts]
    hp = h[:, ts - 1] if ts > 0 else np.zeros_like(c)
    dh = dh_ext[:, ts] + dh_rec
    return dh * (1 - u) * (1 - c * c), dh * (hp - c), dh * u


def gru_gates_reference(gates, h, du, dh_u, d_rh, ts):
    """float64, the header's formulas: (da_g, d_rh on return, rh) of gru_bwd_gates at step ts."""
    gates, h, du, dh_u, d_rh = (np.asarray(a, dtype=np.float64) for a in (gates, h, du, dh_u, d_rh))
    d = h.shape[2]
    r, u = gates[:, ts, :d], gates[:, ts, d:]
    hp = h[:, ts - 1] if ts > 0 else np.zeros_like(r)
    return np.concatenate([d_rh * hp * r * (1 - r), du * u * (1 - u)], axis=1), dh_u + d_rh * r, r * hp


def gru_bwd_calls(lib, n, t, d, ts, f, ld_dhe, ld_dhr, ld_drh):
    """Both backward entries on the Far operands f[name]."""
    ops.check(lib.sagnn_gru_bwd_cand_f32(f["gates"].ptr, f["cand"].ptr, f["h"].ptr, f["dh_ext"].ptr, ld_dhe, None, f["dh_rec"].ptr, ld_dhr,
                                         f["da_c"].ptr, f["du"].ptr, f["dh_u"].ptr, n, t, d, ts, ops._stream()))
    ops.check(lib.sagnn_gru_bwd_gates_f32(f["gates"].ptr, f["h"].ptr, f["du"].ptr, f["dh_u"].ptr, f["d_rh"].ptr, ld_drh, f["da_g"].ptr,
                                          f["rh"].ptr, n, t, d, ts, ops._stream()))


@pytest.mark.parametrize("case", R.GRU_BWD_A, ids=ids(R.GRU_BWD_A))
def test_gru_bwd_far_by_stride(dev, case):
    """gru_bwd_cand with dh_ext and dh_rec, gru_bwd_gates with d_rh (read and written in place), rows 2^24 - 4 floats apart."""
    d, t, n, ts = case.d, case.t, case.n, 2
    rng = np.random.default_rng([21, n])
    val = {"gates": rng.random((n, t, 2 * d)), "cand": np.tanh(rng.standard_normal((n, t, d))), "h": rng.standard_normal((n, t, d)),
           "dh_ext": rng.standard_normal((n, t, d)), "dh_rec": rng.standard_normal((n, d)), "d_rh": rng.standard_normal((n, d)),
           "du": rng.standard_normal((n, d)), "dh_u": rng.standard_normal((n, d))}
    val = {k: v.astype(np.float32) for k, v in val.items()}
    ld = R.LD_GRU - 4
    run = Run(dev, case)
    try:
        lib = _lib.load()
        if case.entry == "gru_bwd_cand":
            inputs, outputs = ("gates", "cand", "h", "dh_ext", "dh_rec"), ("da_c", "du", "dh_u")
            want = gru_cand_reference(*(val[k] for k in inputs), ts)
        else:
            inputs, outputs = ("gates", "h", "du", "dh_u", "d_rh"), ("da_g", "d_rh", "rh")
            want = gru_gates_reference(*(val[k] for k in inputs), ts)
        f = {op.name: run.far(op.name, val[op.name] if op.name in inputs else None) for op in case.operands}
        if case.entry == "gru_bwd_cand":
            ops.check(lib.sagnn_gru_bwd_cand_f32(f["gates"].ptr, f["cand"].ptr, f["h"].ptr, f["dh_ext"].ptr, ld, None, f["dh_rec"].ptr, ld,
                                                 f["da_c"].ptr, f["du"].ptr, f["dh_u"].ptr, n, t, d, ts, ops._stream()))
        else:
            ops.check(lib.sagnn_gru_bwd_gates_f32(f["gates"].ptr, f["h"].ptr, f["du"].ptr, f["dh_u"].ptr, f["d_rh"].ptr, ld, f["da_g"].ptr,
                                                  f["rh"].ptr, n, t, d, ts, ops._stream()))
        fr = {}
        for name, w in zip(outputs, want):
            f[name].check_written(R.case_id(case))
            fr[name] = fraction(f[name].read(), w)
        for name in inputs:
            if name not in outputs:
                assert f[name].written() == f[name].numel() and np.array_equal(f[name].read(), val[name]), f"{name} changed"
        run.report(**fr)
    finally:
        run.close()


@pytest.mark.parametrize("case", R.GRU_B, ids=ids(R.GRU_B))
def test_gru_far_by_count(dev, case):
    """sagnn_gru_fwd_f32 in its training form with gates [n, t, 2d] past 2^31 floats: h, gates and cand at the checked nodes
    against float64; then gru_bwd_cand and gru_bwd_gates at the last step on what the forward stored, against the header's
    formulas in float64 on the stored values."""
    d, t, n = case.d, case.t, case.n
    chk = case.operands[0].checked
    m, ts = len(chk), t - 1
    rng = np.random.default_rng([22, d, t, m])
    x = rng.standard_normal((m, t, d)).astype(np.float32)
    p = G.init_gru_params(d, rng)
    w = [p[k] for k in G.GRU_KEYS]
    want_h, want_g, want_c, _ = G.gru(x, *w, want_saved=True)
    small = {k: rng.standard_normal(s).astype(np.float32) for k, s in (("dh_ext", (m, t, d)), ("dh_rec", (m, d)), ("d_rh", (m, d)))}
    run = Run(dev, case)
    try:
        lib = _lib.load()
        gen = torch.Generator(device=dev).manual_seed(38)
        nodes = torch.tensor(chk, device=dev)
        wd = [dev_f32(dev, a) for a in w]
        f = {op.name: run.far(op.name) for op in case.operands}
        for name in ("x", "dh_ext", "dh_rec", "d_rh"):
            fill_normal(f[name], gen)
        f["x"].put(x, nodes)
        for k, v in small.items():
            f[k].put(v, nodes)
        x_op = f["x"].op
        assert ops.gru_fused_supported(d)
        ops.check(lib.sagnn_gru_fwd_f32(f["x"].ptr, x_op.strides[0], x_op.strides[1], n, t, d, *(a.data_ptr() for a in wd), None, f["h"].ptr,
                                        t * d, f["gates"].ptr, f["cand"].ptr, None, 0, ops._stream()))
        fr = {}
        for name, want in (("h", want_h), ("gates", want_g), ("cand", want_c)):
            f[name].check_written(R.case_id(case))
            fr[name] = fraction(f[name].read(nodes), want)
        gru_bwd_calls(lib, n, t, d, ts, f, t * d, d, d)
        gates, cand, h = (f[k].read(nodes) for k in ("gates", "cand", "h"))
        da_c, du, dh_u = gru_cand_reference(gates, cand, h, small["dh_ext"], small["dh_rec"], ts)
        da_g, d_rh, rh = gru_gates_reference(gates, h, f["du"].read(nodes), f["dh_u"].read(nodes), small["d_rh"], ts)
        wants = {"da_c": da_c, "du": du, "dh_u": dh_u, "da_g": da_g, "d_rh": d_rh, "rh": rh}
        for name, want in wants.items():
            f[name].check_written(R.case_id(case))
            fr[name] = fraction(f[name].read(nodes), want)
        run.report(**fr)
    finally:
        run.close()


# ---- dense_nn --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.DENSE_A, ids=ids(R.DENSE_A))
def test_dense_nn_far_by_stride(dev, case):
    din, dout, n = case.d, case.heads, case.n
    rng = np.random.default_rng([13, din, dout, n])
    x = rng.standard_normal((n, din), dtype=np.float32)
    W = rng.standard_normal((din, dout), dtype=np.float32) / np.float32(din ** 0.5)
    bias = rng.standard_normal(dout, dtype=np.float32)
    want = x.astype(np.float64) @ W.astype(np.float64) + bias
    assert fraction(x @ W + bias, want, NN_ATOL, NN_RTOL) <= 0.25    # the float32 product itself: the screen
    run = Run(dev, case)
    try:
        Wd, bd = dev_f32(dev, W), dev_f32(dev, bias)
        xs, ys = run.far("X", x), run.far("Y")
        ops.check(_lib.load().sagnn_dense_nn_f32(xs.ptr, xs.op.strides[0], n, din, dout, Wd.data_ptr(), bd.data_ptr(), ys.ptr,
                                                 ys.op.strides[0], 0, ops._stream()))
        ys.check_written(R.case_id(case))
        assert xs.written() == xs.numel() and np.array_equal(xs.read(), x), "X changed"
        run.report(Y=fraction(ys.read(), want, NN_ATOL, NN_RTOL))
    finally:
        run.close()


def tn_fractions(got_W, got_b, x64, g64, weight=None):
    """dW and db as fractions of test_gpu_dense_routes.check_tn's bounds; rows x64 / g64 (float64), each counted `weight`
    times. The float32 numpy product must itself stay within a quarter: the screen."""
    w = np.ones(len(x64)) if weight is None else weight
    want, mag = (x64 * w[:, None]).T @ g64, (np.abs(x64) * w[:, None]).T @ np.abs(g64)
    want_b, mag_b = (g64 * w[:, None]).sum(axis=0), (np.abs(g64) * w[:, None]).sum(axis=0)
    bound, bound_b = TN_RTOL * np.abs(want) + TN_MAG * mag + TN_ATOL, TN_RTOL * np.abs(want_b) + TN_MAG * mag_b + TN_ATOL
    x32, g32, w32 = x64.astype(np.float32), g64.astype(np.float32), w.astype(np.float32)
    assert float((np.abs((x32 * w32[:, None]).T @ g32 - want) / bound).max()) <= 0.25
    return float((np.abs(got_W - want) / bound).max()), float((np.abs(got_b - want_b) / bound_b).max())


@pytest.mark.parametrize("case", R.DENSE_B, ids=ids(R.DENSE_B))
def test_dense_far_by_count(dev, case):
    """dense_nn with X and Y past 2^31 floats; dense_tn and dense_tn_seg with a gradient G that is zero everywhere but the
    checked rows, so that float64's dW and db are sums over those rows alone."""
    din, dout, n, t = case.d, case.heads, case.n, case.t
    a_op, b_op = case.operands
    chk = a_op.checked
    m = len(chk)
    rng = np.random.default_rng([19, din, dout, m])
    run = Run(dev, case)
    try:
        lib = _lib.load()
        gen = torch.Generator(device=dev).manual_seed(37)
        nodes = torch.tensor(chk, device=dev)
        xs = run.far(a_op.name)
        fill_normal(xs, gen)
        x = rng.standard_normal((m,) + a_op.shape[1:], dtype=np.float32)
        xs.put(x, nodes)
        if case.entry == "dense_nn":
            W = rng.standard_normal((din, dout), dtype=np.float32) / np.float32(din ** 0.5)
            bias = rng.standard_normal(dout, dtype=np.float32)
            want = x.astype(np.float64) @ W.astype(np.float64) + bias
            assert fraction(x @ W + bias, want, NN_ATOL, NN_RTOL) <= 0.25
            Wd, bd = dev_f32(dev, W), dev_f32(dev, bias)
            ys = run.far("Y")
            ops.check(lib.sagnn_dense_nn_f32(xs.ptr, din, n, din, dout, Wd.data_ptr(), bd.data_ptr(), ys.ptr, dout, 0, ops._stream()))
            ys.check_written(R.case_id(case))
            run.report(Y=fraction(ys.read(nodes), want, NN_ATOL, NN_RTOL))
            return
        gs = run.far("G")
        gs.view.zero_()
        g = rng.standard_normal((m,) + b_op.shape[1:], dtype=np.float32)
        gs.put(g, nodes)
        dW, db = sums(dev, din, dout), sums(dev, 1, dout)
        if case.entry == "dense_tn":
            ops.check(lib.sagnn_dense_tn_f32(xs.ptr, din, gs.ptr, dout, n, din, dout, dW.ptr, db.ptr, ops._stream()))
        else:   # segment s = step s: x[:, s] rows t*d apart against G[s] rows 4d apart
            ops.check(lib.sagnn_dense_tn_seg_f32(xs.ptr, a_op.strides[0], a_op.strides[1], gs.ptr, b_op.strides[0], b_op.strides[1], n, t,
                                                 din, dout, dW.ptr, db.ptr, ops._stream()))
        assert xs.written() == xs.numel() and gs.written() == gs.numel() and rows_not_zero(gs.view) == m
        f_W, f_b = tn_fractions(dW.read(), db.read()[0], x.reshape(-1, din).astype(np.float64),
                                g.reshape(-1, dout).astype(np.float64))
        run.report(dW=f_W, db=f_b)
    finally:
        run.close()


def test_dense_tn_seg_at_the_most_rows_a_call_admits(dev):
    """seg_rows * n_seg = 2^31 - 2^16, the 32-bit row index of the kernel one segment short of its limit. Segment s starts
    one row after segment s - 1 (x_seg = ldx), so row r of the operands is counted once for every (s, i) with s + i = r;
    G is zero but for 64 rows spread over the whole range."""
    seg_rows, n_seg, din, dout = (R.SEG_LIMIT[k] for k in ("seg_rows", "n_seg", "din", "dout"))
    assert R.T31 - seg_rows <= seg_rows * n_seg < R.T31
    total = seg_rows + n_seg - 1
    rng = np.random.default_rng(20)
    x = rng.standard_normal((total, din), dtype=np.float32)
    g = np.zeros((total, dout), dtype=np.float32)
    hot = np.unique(np.concatenate([[0, 1, n_seg - 1, seg_rows - 1, seg_rows, total - 2, total - 1], rng.integers(0, total, 57)]))
    g[hot] = rng.standard_normal((len(hot), dout), dtype=np.float32)
    r = hot.astype(np.int64)
    count = (np.minimum(r, n_seg - 1) - np.maximum(0, r - seg_rows + 1) + 1).astype(np.float64)   # s in [max(0, r-seg_rows+1), min(r, n_seg-1)]
    assert count.min() == 1 and count.max() == n_seg
    try:
        xd, gd = dev_f32(dev, x), dev_f32(dev, g)
        dW, db = sums(dev, din, dout), sums(dev, 1, dout)
        t0 = time.perf_counter()
        with ops.engine("f16x2"):
            ops.check(_lib.load().sagnn_dense_tn_seg_f32(xd.data_ptr(), din, din, gd.data_ptr(), dout, dout, seg_rows, n_seg, din, dout,
                                                         dW.ptr, db.ptr, ops._stream()))
        torch.cuda.synchronize()
        f_W, f_b = tn_fractions(dW.read(), db.read()[0], x[hot].astype(np.float64), g[hot].astype(np.float64), count)
        print(f"far_offsets|dense_tn_seg {seg_rows} x {n_seg} rows|worst error / bound: dW={f_W:.4f} db={f_b:.4f}|{time.perf_counter() - t0:.2f} s")
        assert f_W <= 1.0 and f_b <= 1.0
        assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(gd.cpu(), torch.from_numpy(g))
    finally:
        xd = gd = dW = db = None
        torch.cuda.empty_cache()


# ---- rows_gather / rows_scatter --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.ROWS, ids=ids(R.ROWS))
def test_rows_far_by_stride(dev, case):
    """Copies: the result is the source, bit for bit."""
    d, t, n = case.d, case.t, case.n
    rng = np.random.default_rng([14, n])
    values = rng.standard_normal((n, t, d)).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)
    run = Run(dev, case)
    try:
        lib = _lib.load()
        rows = torch.from_numpy(perm).to(dev)
        count = torch.tensor([n], dtype=torch.int32, device=dev)
        if case.entry == "rows_gather":
            xs, out = run.far("x", values), run.far("out")
            ops.check(lib.sagnn_rows_gather_f32(xs.ptr, xs.op.strides[0], d, n, t, d, rows.data_ptr(), n, count.data_ptr(), out.ptr,
                                                ops._stream()))
            out.check_written(R.case_id(case))
            assert np.array_equal(out.read(), values[perm])
            assert xs.written() == xs.numel()
        else:
            dst, src = run.far("dst"), run.far("src", values)
            ops.check(lib.sagnn_rows_scatter_f32(src.ptr, rows.data_ptr(), n, count.data_ptr(), t, d, dst.ptr, dst.op.strides[0], d, n,
                                                 ops._stream()))
            dst.check_written(R.case_id(case))
            assert np.array_equal(dst.read()[perm], values)
        run.report(copy=0.0)
    finally:
        run.close()


# ---- SpMM ------------------------------------------------------------------------------------------------------------------

def test_spmm_gathers_from_far_source_rows(dev):
    """sagnn_spmm_f32 over an X with ldx = 2^16: source rows from 8192, 16384 and 32768 on lie past the three thresholds.
    Every degree class (short, one wave, chunked with the fix-up), under test_gpu_spmm's row tolerance."""
    from test_gpu_spmm import assert_sum_close
    case, = R.SPMM
    n_rows, n_src, rowptr, colidx = R.spmm_graph()
    d = case.d
    rng = np.random.default_rng(16)
    x = rng.standard_normal((n_src, d)).astype(np.float32)
    idx = np.stack([np.repeat(np.arange(n_rows), np.diff(rowptr)), colidx], 1).astype(np.int32)
    want = O.message_propagate_zero_fill(x.astype(np.float64), idx, n_rows, 0.5)
    terms = O.message_propagate_zero_fill(np.abs(x).astype(np.float64), idx, n_rows, 1.0)
    run = Run(dev, case)
    try:
        plan = ops.SpmmPlan(rowptr, colidx, n_rows, n_src, device=dev, tuning=R.SPMM_TUNING)
        assert plan.info.n_long_rows > 0
        ws = plan.workspace(d)
        xs, out = run.far("X", x), run.far("out")
        ops.check(_lib.load().sagnn_spmm_f32(plan.handle, xs.ptr, xs.op.strides[0], d, None, 0, 0.5, out.ptr, out.op.strides[0], None, 0,
                                             None, 0, ops._ptr(ws), 0 if ws is None else ws.numel() * 4, ops._stream()))
        out.check_written(R.case_id(case))
        got = out.read()
        assert xs.written() == xs.numel()
        tol = 1e-4 * np.abs(want) + 1e-5 + 2e-7 * terms      # test_gpu_spmm.assert_sum_close
        f = float((np.abs(got.astype(np.float64) - want) / tol).max())
        print(f"far_offsets|{R.case_id(case)}|worst error / bound {f:.4f}")
        assert_sum_close(got, want, terms)
        run.report(out=f)
    finally:
        run.close()


@pytest.mark.parametrize("case", R.STACK, ids=ids(R.STACK))
def test_gnn_stack_far_slabs(dev, case):
    """sagnn_gnn_stack_f32 and _bwd_f32 over T = 4 interval graphs drawn like test_gpu_spmm's, every degree class in each,
    the [T, N, d] operands 2^30 - 4 floats apart. Forward: against the float64 oracle under test_gpu_spmm's row tolerance.
    Backward: bit for bit the same entry on dense slabs (no atomics: a row's result is a function of its inputs), which
    test_gpu_spmm and test_gpu_backward tie to the per-interval entry and to float64 autograd."""
    from sa_gnn_amd import graph
    from test_gpu_spmm import _intervals, assert_sum_close
    T, U, I, d, L = R.STACK_T, R.STACK_U, R.STACK_I, R.STACK_D, R.STACK_L
    rng = np.random.default_rng(18)
    mats = _intervals(rng, U, I, T, (0.004, 0.009, 0.002))
    a_u = rng.standard_normal((T, U, d)).astype(np.float32)
    a_i = rng.standard_normal((T, I, d)).astype(np.float32)
    run = Run(dev, case)
    try:
        pairs = [graph.interval_pair(m, dev, tuning=(8, 24, 64)) for m in mats]
        assert all(p[0].plan.info.n_long_rows > 0 and p[1].plan.info.n_long_rows > 0 for p in pairs)
        batch = ops.SpmmBatch([p[0].plan for p in pairs], [p[1].plan for p in pairs])
        mu = torch.zeros((T, L, U, d // 4), dtype=torch.uint8, device=dev)
        mi = torch.zeros((T, L, I, d // 4), dtype=torch.uint8, device=dev)
        in_u, in_i, out_u, out_i = run.far("in_u", a_u), run.far("in_i", a_i), run.far("out_u"), run.far("out_i")
        if case.entry == "gnn_stack":
            ops.gnn_stack(batch, in_u.view, in_i.view, L, 0.5, out_u.view, out_i.view, mask_u=mu, mask_i=mi)
            adjs = [O.trans_to_lsts(m)[0] for m in mats]
            tps = [O.trans_to_lsts(O.transpose(m))[0] for m in mats]
            want_u, want_i = O.gnn_stack(a_u.astype(np.float64), a_i.astype(np.float64), adjs, tps, L, 0.5)     # [N, T, d]
            terms_u, terms_i = O.gnn_stack(np.abs(a_u).astype(np.float64), np.abs(a_i).astype(np.float64), adjs, tps, L, 1.0)
            fr = {}
            for name, o, want, terms in (("user", out_u, want_u, terms_u), ("item", out_i, want_i, terms_i)):
                o.check_written(R.case_id(case))
                got = o.read().transpose(1, 0, 2)
                fr[name] = float((np.abs(got - want) / (1e-4 * np.abs(want) + 1e-5 + 2e-7 * terms)).max())
                assert_sum_close(got, want, terms)
        else:
            e_u, e_i = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev) for s in ((T, U, d), (T, I, d)))
            ops.gnn_stack(batch, e_u, e_i, L, 0.5, torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev),
                          mask_u=mu, mask_i=mi)
            ops.gnn_stack_bwd(batch, in_u.view, in_i.view, L, 0.5, mu, mi, out_u.view, out_i.view)
            want_u, want_i = torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev)
            ops.gnn_stack_bwd(batch, dev_f32(dev, a_u), dev_f32(dev, a_i), L, 0.5, mu, mi, want_u, want_i)
            for o, want in ((out_u, want_u), (out_i, want_i)):
                o.check_written(R.case_id(case))
                assert torch.equal(o.view, want), f"{o.op.name}: the far slabs differ from the dense ones"
            assert bool(want_u.abs().sum() > 0) and bool(want_i.abs().sum() > 0)
            fr = {"equal_bits": 0.0}
        assert in_u.written() == in_u.numel() and in_i.written() == in_i.numel()
        assert np.array_equal(in_u.read(), a_u) and np.array_equal(in_i.read(), a_i)
        run.report(**fr)
    finally:
        run.close()
