"""GPU parity: every backward route of the fusion selection table (csrc/engine.cpp) against float64, kernel by kernel.

The ABI does not say which kernel ran, and the engine is per calling thread: PyTorch runs a backward on a worker thread
whose engine is the default one, so nothing here goes through .backward(). Every kernel is called on the test thread
inside `with ops.engine(...)`. front_route / tail_route / bptt_route restate the three backward selectors from the C++
(source lines cited); every case names the table row it exists for and asserts that label, and tests/test_bwd_routes_host.py
checks on the CPU that the selectors agree with the library's queries and that the case lists reach every instantiation.

Front (sagnn_attn_bwd_front_f32): x and g_out standard normal, O.init_fusion_params; reference float64 torch autograd
(test_gpu_fusion_multitile.attn_bwd_front_reference). Nodes are screened on the CPU: one is used only if float32 autograd
of the same formula stays within a QUARTER of every bound, so a kernel as exact as plain fp32 has three quarters to spare.
Bounds, never wider:
  y              |err| <= 2e-5 + 1e-4 |want|                       (test_gpu_fusion_multitile._check)
  dqkv, global   |err| <= 1e-4 |want| + 2e-5 max |want|            (test_attn_bwd_front_many_tiles_per_block)
  dqkv, per node |err| <= 1e-4 max |want over the node's [t, 3d]|  (test_gpu_f16_range._per_row_ok, atol = 0)
x is a strided view of a NaN-filled buffer, g_out a row view with ld_g = d + 4 of another, dqkv and y are 16-byte-aligned
windows with 32 * 3d NaNs on both sides: a read of padding poisons the result, a write outside a window is found afterwards,
and a row the kernel skipped is still NaN. Every case prints its worst error as a fraction of each bound, next to the
float32 reference's, before it asserts.

Tail (sagnn_attn_bwd_tail_f32): an "exact" kind (integers in [-4, 4]: every product and partial sum is an integer far
below 2^24 and survives the two-piece f16 split, so any order of summation gives the int64 product bit for bit) and an
"arith" kind under the bounds of test_attn_bwd_tail_rows_of_any_scale. dW and db, which the kernels add to with float
atomics, start as zeros with a band of zeros and then NaNs on both sides: an add onto a NaN would not show.

BPTT (sagnn_lstm_bwd_ws_f32): the four cells of select_lstm_bwd against float64 autograd of O.torch_basic_lstm under
test_gpu_backward._close."""
import functools

import numpy as np
import pytest
import torch

from oracle import selfgnn_oracle as O
from sa_gnn_amd import _lib, ops
from test_gpu_backward import _close
from test_gpu_f16_range import _per_row_ok
from test_gpu_fusion_multitile import ATOL, RTOL, attn_bwd_front_reference
from test_gpu_fusion_routes import ATTN_KEYS, Slab, device_params, f64, x_layout

pytestmark = pytest.mark.gpu

ERR_DIM = -2                                             # SAGNN_ERR_DIM: what tests/test_host.py pins for an unsupported shape


# ---- the selection, restated -----------------------------------------------------------------------------------------------

SPECIALISED_T = (1, 2, 3, 4, 5, 6, 8, 12, 16)            # engine.h:32
MFMA_BWD_FRONT_T = (1, 2, 3, 4, 5, 6, 8)                 # engine.h:35
SPLIT_BWD_FRONT_T128 = (1, 2, 3, 4, 5, 6)                # engine.h:36
ENGINES = ("f16x2", "f32", "valu")


def front_route(engine, d, t, heads):
    """select_attn_bwd_front (engine.cpp:68-73)."""
    split = heads == 16 and (t in SPLIT_BWD_FRONT_T128 if d == 128 else d in (32, 64) and t in SPECIALISED_T)   # engine.cpp:89-92
    if engine != "f32" and split:                        # engine.cpp:69
        return "Split"
    mfma = d in (32, 64) and 1 <= t <= 32 and heads >= 1 and d % heads == 0 and (d // heads) & (d // heads - 1) == 0   # engine.cpp:94-98
    if mfma and d // heads in (2, 4) and t in MFMA_BWD_FRONT_T:   # engine.cpp:70-71
        return "F32Mfma"
    return "None"                                        # engine.cpp:72


def tail_route(engine, d):
    """select_attn_bwd_tail (engine.cpp:75-77)."""
    return "None" if d not in (32, 64) else "F32Mfma" if engine == "f32" else "F16x2"


def bptt_route(engine, d, workspace):
    """select_lstm_bwd (engine.cpp:79-81)."""
    return "None" if d not in (32, 64) else "SplitDw" if engine == "f16x2" and workspace else "OneLaunch"


def mfma_tile(t):
    return 4 * (32 // t)                                 # fusion_mfma.hip:973: four waves x (kRowsPerWave / t) nodes


def split_tile(t):
    return 64 // t                                       # attn_split.hip:543: NB = kRows / T, kRows = 64 (attn_split.hip:38)


def mfma_pairs(d, t, heads):
    return (32 // t) * heads                             # fusion_mfma.hip:536: (node, head) pairs of a wave, 64 lanes


def nodes_of(n, t, cus):
    """A case's node count. "steady": 2 CUs + 1 tiles of the F32Mfma front (fusion_mfma.hip:972-975 launches one block per
    CU), so every block loops, block 0 three times, and the last tile is ragged."""
    return 2 * cus * mfma_tile(t) + mfma_tile(t) // 2 + 1 if n == "steady" else n


def rows_of(rows, cus):
    """A tail case's row count. "steady": the F32Mfma tail launches 2 CUs blocks (attn_bwd_tail.hip:241), the F16x2 one
    CUs at d = 64 and 2 CUs at d = 32 (attn_bwd_tail_f16.hip:504); 5 CUs chunks of 32 rows and a last one of 3 give every
    block 2 to 3 chunks where 2 CUs blocks run and 5 to 6 where CUs do, and the ragged chunk is nobody's first."""
    return 32 * 5 * cus + 3 if rows == "steady" else rows


def bptt_nodes_of(n, cus):
    """"steady": the BPTT launches CUs blocks over chunks of 32 rows (lstm_bwd_mfma.hip:412-413): 2 to 3 chunks each, the last
    of 5 rows."""
    return 32 * (2 * cus + cus // 2) + 5 if n == "steady" else n


# ---- front cases: (engine, d, t, heads, n, the table row the case is there for) --------------------------------------------

# attn bwd front, "any / d in {32, 64}, d/heads in {2, 4}, t in {1..6, 8} / F32Mfma": ln_mhsa_mean_mfma_kernel<D, T, true>
# with attention_pairs_bwd<D, DK, QS, T>. Under f32 the 16-head shapes (d_k = 2 at d = 32, 4 at d = 64); under f16x2 the
# shapes Split does not take (d_k = 4 at d = 32, 2 at d = 64). n = 1, a tile less one node, a tile and one node: ragged
# tiles; at t = 3, 5, 6 a wave's 32-row tile uses 30 rows; a full wave has more than 64 pairs (the gpre[] select chain runs
# past its first entry) at every shape but (32, 4, 8), (32, 8, 16), (64, 8, 16) [64 pairs] and (32, 5, 8), (32, 6, 8),
# (32, 8, 8) [48, 40, 32].
MFMA_SHAPES = [("f32", 32, 16), ("f32", 64, 16), ("f16x2", 32, 8), ("f16x2", 64, 32)]
STEADY_T = {(32, 2): 1, (32, 4): 3, (64, 4): 5, (64, 2): 8}   # (d, d_k) -> the t of its steady-state case
FRONT_MFMA = (
    [(e, d, t, h, n, "F32Mfma") for e, d, h in MFMA_SHAPES for t in MFMA_BWD_FRONT_T for n in (1, mfma_tile(t) - 1, mfma_tile(t) + 1)]
    # the same row under valu: the shapes with heads != 16 (16 heads are Split's there)
    + [("valu", 32, 4, 8, mfma_tile(4) + 1, "F32Mfma"), ("valu", 64, 4, 32, mfma_tile(4) + 1, "F32Mfma")]
    # every block loops, the last tile is ragged: the only cases with more than a few thousand nodes
    + [(e, d, STEADY_T[d, d // h], h, "steady", "F32Mfma") for e, d, h in MFMA_SHAPES]
)
# attn bwd front, "f16x2,valu / heads = 16; d = 128 with t <= 6, d in {32, 64} with t in {1..6, 8, 12, 16} / Split"
FRONT_SPLIT = (
    [("f16x2", d, t, 16, n, "Split") for d, ts in [(128, SPLIT_BWD_FRONT_T128), (64, SPECIALISED_T), (32, SPECIALISED_T)]
     for t in ts for n in (1, split_tile(t) - 1, split_tile(t) + 1)]
    + [("valu", 64, 3, 16, split_tile(3) + 1, "Split"), ("valu", 128, 5, 16, split_tile(5) + 1, "Split")]
)
FRONT_CASES = FRONT_MFMA + FRONT_SPLIT
# attn bwd front, "any / otherwise / None": t outside the tables, d = 128 under f32, d_k = 8, d = 128 past t = 6
FRONT_NONE = [("f16x2", 64, 7, 16), ("f32", 64, 12, 16), ("f32", 128, 3, 16), ("f16x2", 64, 3, 8), ("f16x2", 128, 8, 16)]

# (apply_ln, y requested): layer norm with y, layer norm with y_out = NULL, no layer norm (gamma / beta NULL, y is x)
VARIANTS = ((True, True), (True, False), (False, False))
X_LAYOUTS = ("padded", "time_major,vec")                 # both keep x's rows 16-byte aligned, which the entry requires

# ---- tail cases: (engine, d, rows, route) ----------------------------------------------------------------------------------
# attn bwd tail, "f32 / d in {32, 64} / F32Mfma" and "f16x2,valu / d in {32, 64} / F16x2". Chunks of 32 rows: 1 and 3 rows
# (one chunk of fewer than four: the F16x2 kernel measures its largest row against its smallest), 31, 32, 33 and 35 (a last chunk of 1 and of 3),
# 66 (of 2), and the steady state.
TAIL_ROWS = (1, 3, 31, 32, 33, 35, 64 + 2, "steady")
TAIL_CASES = [(e, d, rows, tail_route(e, d)) for e in ENGINES for d in (32, 64) for rows in TAIL_ROWS]
TAIL_NONE = [(e, d) for e in ENGINES for d in (128, 96)]

# ---- BPTT cases: (engine, workspace, d, t, n, route): the four cells of select_lstm_bwd ------------------------------------
BPTT_CELLS = [("f16x2", False, "OneLaunch"), ("f16x2", True, "SplitDw"), ("f32", True, "OneLaunch"), ("valu", True, "OneLaunch")]
BPTT_CASES = [(e, ws, d, t, n, route) for e, ws, route in BPTT_CELLS for d in (32, 64) for t in (1, 2, 5) for n in (1, 31, 33, "steady")]


# ---- guarded outputs -------------------------------------------------------------------------------------------------------

class Window:
    """[rows, cols] contiguous floats, 16-byte aligned, in a device buffer: `guard` NaNs, `band` zeros, the window, `band`
    zeros, `guard` NaNs. The window starts as `values`, or as NaN (what a kernel must overwrite), or as zeros where there is
    a band (what a kernel adds to)."""

    def __init__(self, dev, rows, cols, guard, band=0, values=None):
        assert guard % 4 == 0 and band % 4 == 0
        self.rows, self.cols, self.lo, self.band = rows, cols, guard + band, band
        host = np.full(2 * self.lo + rows * cols, np.nan, dtype=np.float32)
        host[guard:len(host) - guard] = 0.0 if band else np.nan
        if values is not None:
            host[self.lo:self.lo + rows * cols] = np.asarray(values, dtype=np.float32).reshape(-1)
        self.before = host.copy()
        self.buf = torch.from_numpy(host).to(dev)
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 0

    def read(self, written=True):
        """The window's values, once everything around it is seen to be as it was."""
        host = self.buf.cpu().numpy()
        inside = np.zeros(len(host), dtype=bool)
        inside[self.lo:self.lo + self.rows * self.cols] = True
        assert np.array_equal(host[~inside], self.before[~inside], equal_nan=True), "a write outside the window"
        got = host[inside].reshape(self.rows, self.cols)
        if written:
            assert not np.isnan(got).any(), f"{int(np.isnan(got).any(axis=1).sum())} of {self.rows} rows hold NaN"
        return got

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.before, equal_nan=True)


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- the front -------------------------------------------------------------------------------------------------------------

def front_fractions(y, dqkv, y64, dq64, n):
    """Per node, the worst error as a fraction of each bound: y, dqkv global, dqkv per node."""
    e = np.abs(dqkv.astype(np.float64) - dq64)
    fy = (np.abs(y.astype(np.float64) - y64) / (ATOL + RTOL * np.abs(y64))).reshape(n, -1).max(axis=1)
    fg = (e / (1e-4 * np.abs(dq64) + 2e-5 * np.abs(dq64).max())).reshape(n, -1).max(axis=1)
    fn = e.reshape(n, -1).max(axis=1) / (1e-4 * np.abs(dq64).reshape(n, -1).max(axis=1))
    return fy, fg, fn


@functools.lru_cache(maxsize=None)
def front_reference(d, t, heads, n):
    """Parameters, x [n, t, d], g_out [n, d], and per apply_ln: (y, dqkv) in float64 and the float32 reference's worst
    fraction of each bound on the nodes kept."""
    rng = np.random.default_rng([4, d, t, heads, n])
    m = n + n // 4 + 8                                   # spare nodes for the screen
    x = rng.standard_normal((m, t, d)).astype(np.float32)
    gout = rng.standard_normal((m, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    refs, ok = {}, np.ones(m, dtype=bool)
    for ln in (True, False):
        y64, dq64 = attn_bwd_front_reference(x.astype(np.float64), f64(p), gout.astype(np.float64), heads, torch.float64, ln)
        y32, dq32 = attn_bwd_front_reference(x, p, gout, heads, torch.float32, ln)
        refs[ln] = (y64, dq64, y32, dq32)
        for f in front_fractions(y32, dq32, y64, dq64, m):
            ok &= f <= 0.25
    keep = np.flatnonzero(ok)[:n]
    assert len(keep) == n, f"only {len(keep)} of {m} nodes pass the fp32 screen"
    rows = (keep[:, None] * t + np.arange(t)).reshape(-1)
    want, ref32 = {}, {}
    for ln, (y64, dq64, y32, dq32) in refs.items():
        want[ln] = (y64[keep], dq64[rows])
        ref32[ln] = tuple(float(f.max()) for f in front_fractions(y32[keep], dq32[rows], *want[ln], n))
        assert max(ref32[ln]) <= 0.25                    # max |want| is now taken over the nodes kept
    return p, x[keep], gout[keep], want, ref32


def call_front(engine, xs, t, d, heads, pd, ln, g, dq, y):
    """The raw entry under `engine`; xs / g: Slab, dq / y: Window or None. Returns the code."""
    n = xs.shape[0]
    ld_n, ld_t = xs.strides[0], xs.strides[1]
    with ops.engine(engine):
        return _lib.load().sagnn_attn_bwd_front_f32(
            xs.view.data_ptr(), ld_n, ld_t, n, t, d, heads, pd["ln_gamma"].data_ptr() if ln else None,
            pd["ln_beta"].data_ptr() if ln else None, 1e-12, 1 if ln else 0, *(pd[k].data_ptr() for k in ATTN_KEYS),
            g.view.data_ptr(), g.strides[0], dq.ptr, None if y is None else y.ptr, ops._stream())


@pytest.mark.parametrize("engine,d,t,heads,n,route", FRONT_CASES, ids=lambda v: str(v))
def test_front_route(dev, engine, d, t, heads, n, route):
    assert front_route(engine, d, t, heads) == route
    with ops.engine(engine):                             # the table's note: under VALU the query answers 0, the entry still runs
        assert ops.attn_bwd_front_supported(d, t, heads) == (engine != "valu")
    n = nodes_of(n, t, cu_count(dev))
    p, x, gout, want, ref32 = front_reference(d, t, heads, n)
    pd = device_params(p, dev)
    guard = 32 * 3 * d
    g = Slab(dev, (n, d), (d + 4, 1), 4, values=gout)
    for layout in X_LAYOUTS:
        xs = Slab(dev, (n, t, d), *x_layout(layout, n, t, d), values=x)
        for ln, with_y in VARIANTS:
            what = f"{route} {engine} ({d}, {t}, {heads}) n={n} {layout} ln={int(ln)} y={int(with_y)}"
            dq, y = Window(dev, n * t, 3 * d, guard), Window(dev, n * t, d, guard)
            ops.check(call_front(engine, xs, t, d, heads, pd, ln, g, dq, y if with_y else None))
            y64, dq64 = want[ln]
            assert with_y or y.untouched(), f"{what}: y written though not asked for"
            got_y = y.read().reshape(n, t, d) if with_y else y64
            got = dq.read()
            fy, fg, fn = (float(f.max()) for f in front_fractions(got_y, got, y64, dq64, n))
            print(f"bwd_routes|front|{what}|kernel y={fy:.4f} global={fg:.4f} node={fn:.4f}"
                  f"|float32 y={ref32[ln][0]:.4f} global={ref32[ln][1]:.4f} node={ref32[ln][2]:.4f}")
            assert fy <= 1.0, f"{what}: y at {fy:.3f} of its bound"
            assert fg <= 1.0, f"{what}: dqkv at {fg:.3f} of the global bound"
            _per_row_ok(got.reshape(n, -1), dq64.reshape(n, -1), f"{what}: dqkv per node")
        np.testing.assert_array_equal(xs.read(), x)
    np.testing.assert_array_equal(g.read(), gout)


@pytest.mark.parametrize("engine,d,t,heads", FRONT_NONE, ids=lambda v: str(v))
def test_front_none_row_is_refused_with_nothing_written(dev, engine, d, t, heads):
    assert front_route(engine, d, t, heads) == "None"
    n = 5
    rng = np.random.default_rng([6, d, t, heads])
    pd = device_params(O.init_fusion_params(d, rng), dev)
    xs = Slab(dev, (n, t, d), *x_layout("padded", n, t, d), values=rng.standard_normal((n, t, d)).astype(np.float32))
    g = Slab(dev, (n, d), (d + 4, 1), 4, values=rng.standard_normal((n, d)).astype(np.float32))
    for ln in (True, False):
        dq, y = Window(dev, n * t, 3 * d, 32 * 3 * d), Window(dev, n * t, d, 32 * 3 * d)
        assert call_front(engine, xs, t, d, heads, pd, ln, g, dq, y) == ERR_DIM
        torch.cuda.synchronize()
        assert dq.untouched() and y.untouched()


def test_front_refuses_rows_that_are_not_16_byte_aligned(dev):
    """x_layout's "time_major" has ld_t = n d + 2: SAGNN_ERR_ALIGN (-3) on both rows of the table, nothing written."""
    n, t = 5, 3
    for engine, d, heads in [("f16x2", 64, 16), ("f32", 64, 16), ("f16x2", 32, 8)]:
        rng = np.random.default_rng([7, d, heads])
        pd = device_params(O.init_fusion_params(d, rng), dev)
        xs = Slab(dev, (n, t, d), *x_layout("time_major", n, t, d), values=rng.standard_normal((n, t, d)).astype(np.float32))
        g = Slab(dev, (n, d), (d + 4, 1), 4, values=rng.standard_normal((n, d)).astype(np.float32))
        dq, y = Window(dev, n * t, 3 * d, 32 * 3 * d), Window(dev, n * t, d, 32 * 3 * d)
        assert call_front(engine, xs, t, d, heads, pd, True, g, dq, y) == -3
        torch.cuda.synchronize()
        assert dq.untouched() and y.untouched()


@pytest.mark.parametrize("engine,d,t,heads", [("f16x2", 64, 3, 16), ("f32", 64, 3, 16), ("f16x2", 32, 2, 8), ("f16x2", 128, 2, 16)],
                         ids=lambda v: str(v))
def test_front_without_nodes_is_ok_and_writes_nothing(dev, engine, d, t, heads):
    assert front_route(engine, d, t, heads) != "None"
    rng = np.random.default_rng([8, d])
    pd = device_params(O.init_fusion_params(d, rng), dev)
    xs = Slab(dev, (1, t, d), *x_layout("padded", 1, t, d), values=rng.standard_normal((1, t, d)).astype(np.float32))
    g = Slab(dev, (1, d), (d + 4, 1), 4, values=rng.standard_normal((1, d)).astype(np.float32))
    dq, y = Window(dev, t, 3 * d, 32 * 3 * d), Window(dev, t, d, 32 * 3 * d)
    with ops.engine(engine):
        rc = _lib.load().sagnn_attn_bwd_front_f32(
            xs.view.data_ptr(), xs.strides[0], xs.strides[1], 0, t, d, heads, pd["ln_gamma"].data_ptr(), pd["ln_beta"].data_ptr(),
            1e-12, 1, *(pd[k].data_ptr() for k in ATTN_KEYS), g.view.data_ptr(), d + 4, dq.ptr, y.ptr, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert dq.untouched() and y.untouched()


# ---- the tail --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tail_reference(d, rows, kind):
    """y [rows, d], dqkv [rows, 3d], Wqkv [d, 3d] and float64 dy, dW, db (exact kind: the int64 products, exactly)."""
    rng = np.random.default_rng([9, d, rows, int(kind == "exact")])
    if kind == "exact":
        y, dqkv, W = (rng.integers(-4, 5, size=s).astype(np.float32) for s in ((rows, d), (rows, 3 * d), (d, 3 * d)))
        for a in (y, dqkv, W):                           # the f16 head of the split holds each value, the residual is zero
            assert np.array_equal(a.astype(np.float16).astype(np.float32), a)
        # the int64 products, taken through float64 BLAS: sums of integers below 2^53 are exact there in any order
        iy, ig, iW = (a.astype(np.float64) for a in (y, dqkv, W))
        # no partial sum, in any order, leaves the integers fp32 holds exactly
        assert max((np.abs(ig) @ np.abs(iW).T).max(), (np.abs(iy).T @ np.abs(ig)).max(), np.abs(ig).sum(axis=0).max()) < 2 ** 24
        out = tuple(a.astype(np.int64) for a in (ig @ iW.T, iy.T @ ig, ig.sum(axis=0)))
    else:
        y, dqkv = (rng.standard_normal(s).astype(np.float32) for s in ((rows, d), (rows, 3 * d)))
        W = (rng.standard_normal((d, 3 * d)) / d ** 0.5).astype(np.float32)
        y64, g64, W64 = (a.astype(np.float64) for a in (y, dqkv, W))
        out = g64 @ W64.T, y64.T @ g64, g64.sum(axis=0)
    return y, dqkv, W, out


def call_tail(engine, yw, gw, rows, d, W, dW, db):
    with ops.engine(engine):
        return _lib.load().sagnn_attn_bwd_tail_f32(yw.ptr, gw.ptr, rows, d, W.data_ptr(), dW.ptr, db.ptr, ops._stream())


@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("engine,d,rows,route", TAIL_CASES, ids=lambda v: str(v))
def test_tail_route(dev, engine, d, rows, route, kind):
    assert tail_route(engine, d) == route
    with ops.engine(engine):
        assert ops.attn_bwd_tail_supported(d) == (engine != "valu")
    rows = rows_of(rows, cu_count(dev))
    y, dqkv, W, (want_dy, want_dW, want_db) = tail_reference(d, rows, kind)
    guard = 32 * 3 * d
    yw, gw = Window(dev, rows, d, guard, values=y), Window(dev, rows, 3 * d, guard, values=dqkv)
    dW, db = Window(dev, d, 3 * d, guard, band=guard), Window(dev, 1, 3 * d, guard, band=guard)
    Wd = torch.from_numpy(W).to(dev)
    ops.check(call_tail(engine, yw, gw, rows, d, Wd, dW, db))
    got_dy, got_dW, got_db = yw.read(), dW.read(), db.read()[0]
    np.testing.assert_array_equal(gw.read(), dqkv)
    assert np.array_equal(Wd.cpu().numpy(), W)
    if kind == "exact":
        for name, got, want in (("dy", got_dy, want_dy), ("dW", got_dW, want_dW), ("db", got_db, want_db)):
            bad = np.argwhere(got != want)
            assert np.array_equal(got, want.astype(np.float32)), f"{name}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}"
        return
    # the bounds of test_attn_bwd_tail_rows_of_any_scale
    y64, g64 = y.astype(np.float64), dqkv.astype(np.float64)
    _per_row_ok(got_dy, want_dy, "dy")
    mag_dW, mag_db = np.abs(y64).T @ np.abs(g64), np.abs(g64).sum(axis=0)
    err = np.abs(got_dW.astype(np.float64) - want_dW)
    assert (err <= 1e-4 * np.abs(want_dW) + 2e-6 * mag_dW).all(), f"dW: worst err / sum|terms| = {(err / mag_dW).max():.3e}"
    err = np.abs(got_db.astype(np.float64) - want_db)
    assert (err <= 1e-4 * np.abs(want_db) + 2e-6 * mag_db).all(), f"db: worst err / sum|terms| = {(err / mag_db).max():.3e}"


@pytest.mark.parametrize("engine,d", TAIL_NONE, ids=lambda v: str(v))
def test_tail_none_row_is_refused_with_nothing_written(dev, engine, d):
    assert tail_route(engine, d) == "None"
    rows = 35
    y, dqkv, W, _ = tail_reference(d, rows, "arith")
    guard = 32 * 3 * d
    yw, gw = Window(dev, rows, d, guard, values=y), Window(dev, rows, 3 * d, guard, values=dqkv)
    dW, db = Window(dev, d, 3 * d, guard, band=guard), Window(dev, 1, 3 * d, guard, band=guard)
    assert call_tail(engine, yw, gw, rows, d, torch.from_numpy(W).to(dev), dW, db) == ERR_DIM
    torch.cuda.synchronize()
    assert yw.untouched() and dW.untouched() and db.untouched()


# ---- the BPTT --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bptt_reference(d, t, n):
    """x, the gradient dh at the emitted h, a 0 / 2 output-dropout scale, parameters, and per "dropped": float64 autograd's
    (dx, dW, db) of O.torch_basic_lstm for that gradient."""
    rng = np.random.default_rng([10, d, t, n])
    x, dh = (rng.standard_normal((n, t, d)).astype(np.float32) for _ in range(2))
    drop = ((rng.random((n, t, d)) < 0.5) * 2.0).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    want = {}
    for dropped in (False, True):
        tx, tW, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, p["lstm_W"], p["lstm_b"]))
        g = torch.tensor(dh * drop if dropped else dh, dtype=torch.float64)
        (O.torch_basic_lstm(tx, tW, tb, 1.0) * g).sum().backward()
        want[dropped] = (tx.grad, tW.grad, tb.grad)
    return p, x, dh, drop, want


@pytest.mark.parametrize("engine,workspace,d,t,n,route", BPTT_CASES, ids=lambda v: str(v))
def test_bptt_route(dev, engine, workspace, d, t, n, route):
    assert bptt_route(engine, d, workspace) == route
    n = bptt_nodes_of(n, cu_count(dev))
    p, x, dh, drop, want = bptt_reference(d, t, n)
    lib = _lib.load()
    W, b = (torch.from_numpy(p[k]).to(dev) for k in ("lstm_W", "lstm_b"))
    # [t, n, d] storage; the second pass of SplitDw reads x as 16-byte rows (lstm_bwd_mfma.hip:439), the one launch takes any
    xs = Slab(dev, (n, t, d), *x_layout("time_major,vec" if route == "SplitDw" else "time_major", n, t, d), values=x)
    dhd, dropd = torch.from_numpy(dh).to(dev), torch.from_numpy(drop).to(dev)
    guard = 32 * 4 * d
    nbytes = int(lib.sagnn_lstm_bwd_workspace_bytes(n, t, d)) if workspace else 0
    with ops.engine(engine):
        h, gates, cell = ops.lstm_fwd_train(xs.view, W, b)
        for dropped in (False, True):
            dx = Window(dev, n * t, d, guard)
            dW, db = Window(dev, 2 * d, 4 * d, guard, band=guard), Window(dev, 1, 4 * d, guard, band=guard)
            ws = torch.empty(nbytes // 4, device=dev) if workspace else None
            ops.check(lib.sagnn_lstm_bwd_ws_f32(
                xs.view.data_ptr(), xs.strides[0], xs.strides[1], h.data_ptr(), gates.data_ptr(), cell.data_ptr(), dhd.data_ptr(),
                t * d, dropd.data_ptr() if dropped else None, W.data_ptr(), dx.ptr, dW.ptr, db.ptr, n, t, d, ops._ptr(ws), nbytes,
                ops._stream()))
            want_dx, want_dW, want_db = want[dropped]
            what = f"{route} {engine} ({d}, {t}) n={n} dropped={int(dropped)}"
            _close(f"{what}: dx", torch.from_numpy(dx.read()), want_dx)
            _close(f"{what}: dW", torch.from_numpy(dW.read()), want_dW)
            # db cancels to ~0 in places: fp32 accumulation noise eps32 * sqrt(n t), the floor of test_generic_layernorm_td_bwd
            _close(f"{what}: db", torch.from_numpy(db.read()[0]), want_db, floor=float(np.finfo(np.float32).eps) * np.sqrt(n * t))
    np.testing.assert_array_equal(xs.read(), x)
    assert ops.get_engine() == "f16x2"
