"""The fusion backward on gradient rows that are exactly zero.

A training step under --fusion_rows all hands the interval fusion's backward an upstream gradient whose rows are zero for
every node outside the batch (the index scatters of the loss write batch rows only): 512 users of 48,653 on a Gowalla-shaped
step, so nearly every 32-row chunk the backward kernels walk holds nothing but zeros. --fusion_rows batch pads with zero
rows, the sequence slab has zero rows in its padding. A zero row has no scale, and the f16 x 2 kernels scale gradient rows:
these tests feed every backward kernel such gradients, at the row layouts below, and judge them against float64 at the
bars the suite already has for the same kernel. None of those bars has an absolute term where the float64 value is
exactly 0, so a zero gradient row must contribute exactly nothing and a node without gradient must get dx == 0.

Row layouts (a boolean mask over the gradient's rows, or over nodes): none, head (all but rows 0..31), one (row R // 3),
batch (each row with probability 1 / 95), alternate (the rows of every odd 32-row chunk), late (the last, ragged chunk
only), second_pass (the chunks >= the tail's grid, attn_bwd_tail_f16.hip launch(): every workgroup starts on zeros and
then meets data). Rows outside the mask are exact zeros, the others standard normal times a scale."""
import functools

import numpy as np
import pytest
import torch

from oracle import selfgnn_oracle as O
from sa_gnn_amd import _lib, ops
from test_gpu_bwd_routes import Window, call_front, cu_count, front_reference, front_route, mfma_tile, split_tile
from test_gpu_f16_range import SCALES, _per_row_ok
from test_gpu_fusion_multitile import ATOL, RTOL, attn_bwd_front_reference
from test_gpu_fusion_routes import Slab, device_params, f64, x_layout

pytestmark = pytest.mark.gpu

CHUNK = 32                                               # attn_bwd_tail_f16.hip: kRows
LAYOUTS = ("none", "head", "one", "batch", "alternate", "late", "second_pass")


def tail_blocks(rows, d, cus):
    """The grid of the f16 x 2 tail (attn_bwd_tail_f16.hip, launch())."""
    return min((rows + CHUNK - 1) // CHUNK, cus * (1 if d == 64 else 2))


def row_mask(layout, rows, rng, blocks=None):
    """The rows that are NOT zero."""
    r = np.arange(rows)
    if layout == "none":
        return np.zeros(rows, dtype=bool)
    if layout == "head":
        return r >= CHUNK
    if layout == "one":
        return r == rows // 3
    if layout == "batch":                                # (drawn again while empty: that would be "none")
        while True:
            m = rng.random(rows) < 1.0 / 95.0
            if m.any():
                return m
    if layout == "alternate":
        return (r // CHUNK) % 2 == 1
    if layout == "late":
        return r >= CHUNK * ((rows - 1) // CHUNK)
    if layout == "second_pass":
        return r // CHUNK >= blocks
    raise ValueError(layout)


def masked_normal(rng, mask, cols, scales):
    """[len(mask), cols] float32: standard normal times the row's scale inside the mask, exact zeros outside."""
    g = rng.standard_normal((len(mask), cols))
    sc = np.ones(len(mask)) if scales == "ones" else rng.choice(SCALES, size=len(mask))
    g = (g * sc[:, None]).astype(np.float32)
    g[~mask] = 0.0
    assert (np.abs(g[mask]).max(axis=1) > 0).all() and not g[~mask].any()
    return g


# ---- 1a: the tail alone ----------------------------------------------------------------------------------------------------

# (layout, rows): every layout at the sizes where it is not another one (head at 32 rows is none; late needs a ragged chunk)
TAIL_LAYOUT_ROWS = ([(lay, r) for lay in ("none", "one", "batch") for r in (32, 65, 1000)]
                    + [(lay, r) for lay in ("head", "alternate", "late") for r in (65, 1000)]
                    + [("second_pass", "second_pass")])
Y_KINDS = ("ordinary", "small", "padding")
TAIL_CASES = [(d, rows, layout, scales, ykind, engine) for d in (64, 32) for layout, rows in TAIL_LAYOUT_ROWS
              for scales in ("ones", "mixed") for ykind in Y_KINDS for engine in ("f16x2", "f32")]


@functools.lru_cache(maxsize=4)
def tail_inputs(d, rows, layout, scales, ykind, blocks):
    """y [rows, d], dqkv [rows, 3d], W [d, 3d], the mask, and float64 dy, dW, db with the sums of their terms' magnitudes."""
    rng = np.random.default_rng([11, d, rows, LAYOUTS.index(layout), scales == "ones", Y_KINDS.index(ykind)])
    mask = row_mask(layout, rows, rng, blocks)
    dqkv = masked_normal(rng, mask, 3 * d, scales)
    if ykind == "small":                                 # no |y| reaches 2^-3
        y = rng.uniform(-0.1, 0.1, size=(rows, d)).astype(np.float32)
    else:
        y = rng.standard_normal((rows, d)).astype(np.float32)
        if ykind == "padding":                           # what a layer norm leaves on an all-zero row: its beta
            y[~mask] = rng.uniform(-0.1, 0.1, size=d).astype(np.float32)
    W = (rng.standard_normal((d, 3 * d)) / d ** 0.5).astype(np.float32)
    y64, g64, W64 = y.astype(np.float64), dqkv.astype(np.float64), W.astype(np.float64)
    want = (g64 @ W64.T, y64.T @ g64, np.abs(y64).T @ np.abs(g64), g64.sum(0), np.abs(g64).sum(0))
    for a in (y, dqkv, W, mask) + want:
        a.flags.writeable = False
    return y, dqkv, W, mask, want


def tail_call_and_check(dev, d, rows, y, dqkv, W, mask, want_dy, want_dW, mag_dW, want_db, mag_db, engine, what):
    """The call and the bounds of test_attn_bwd_tail_rows_of_any_scale; mask: the rows that are not zero. Returns the redo count."""
    lib = _lib.load()
    yd, gd, Wd = (torch.from_numpy(a.copy()).to(dev) for a in (y, dqkv, W))
    dW = torch.zeros((d, 3 * d), device=dev)
    db = torch.zeros(3 * d, device=dev)
    ops.range_redo_count(reset=True)
    with ops.engine(engine):
        ops.check(lib.sagnn_attn_bwd_tail_f32(yd.data_ptr(), gd.data_ptr(), rows, d, Wd.data_ptr(), dW.data_ptr(),
                                              db.data_ptr(), None))
    redo = ops.range_redo_count()
    got_dy, got_dW, got_db = (a.cpu().numpy().astype(np.float64) for a in (yd, dW, db))
    err_dW, err_db = np.abs(got_dW - want_dW), np.abs(got_db - want_db)
    tol_dW, tol_db = 1e-4 * np.abs(want_dW) + 2e-6 * mag_dW, 1e-4 * np.abs(want_db) + 2e-6 * mag_db
    print(f"zero_grad_rows|tail|{what}|redo={redo} of {(rows + CHUNK - 1) // CHUNK} chunks"
          f"|finite={int(np.isfinite(got_dy).all() and np.isfinite(got_dW).all() and np.isfinite(got_db).all())}"
          f"|dW={np.nanmax(err_dW / (tol_dW + 1e-300)):.3g} db={np.nanmax(err_db / (tol_db + 1e-300)):.3g} of their bounds")
    assert np.isfinite(got_dW).all() and np.isfinite(got_db).all(), "non-finite dW / db"
    _per_row_ok(got_dy, want_dy, f"dy[{what}]")
    assert not got_dy[~mask].any()
    assert (err_dW <= tol_dW).all(), f"dW[{what}]: worst err / sum|terms| = {(err_dW / (mag_dW + 1e-300)).max():.3e}"
    assert (err_db <= tol_db).all(), f"db[{what}]: worst err / sum|terms| = {(err_db / (mag_db + 1e-300)).max():.3e}"
    if not mask.any():
        assert not got_dy.any() and not got_dW.any() and not got_db.any()
        assert redo == 0, f"{redo} fp32 redos on a gradient of zeros"
    if engine == "f32":
        assert redo == 0
    return redo


@pytest.mark.parametrize("d,rows,layout,scales,ykind,engine", TAIL_CASES, ids=lambda v: str(v))
def test_tail_zero_gradient_rows(dev, d, rows, layout, scales, ykind, engine):
    """sagnn_attn_bwd_tail_f32 as test_attn_bwd_tail_rows_of_any_scale calls it and at that test's bounds: dy per row at 1e-4
    of the row's largest float64 entry (a zero row: exactly 0), dW and db at 1e-4 |want| + 2e-6 sum |terms| (all rows zero:
    exactly 0), everything finite. The f32 tail never takes the fp32 redo, and no tail does on a gradient of zeros."""
    cus = cu_count(dev)
    two_passes = rows == "second_pass"
    if two_passes:                                       # every workgroup takes two chunks, the first a third, ragged one
        rows = CHUNK * 2 * cus * (1 if d == 64 else 2) + 7
    blocks = tail_blocks(rows, d, cus)
    y, dqkv, W, mask, (want_dy, want_dW, mag_dW, want_db, mag_db) = tail_inputs(d, rows, layout, scales, ykind, blocks)
    if two_passes:
        assert not mask[:CHUNK * blocks].any() and mask[CHUNK * blocks:].all() and mask.sum() > CHUNK
    tail_call_and_check(dev, d, rows, y, dqkv, W, mask, want_dy, want_dW, mag_dW, want_db, mag_db, engine,
                        f"d={d} rows={rows} {layout} {scales} {ykind} {engine}")


@pytest.mark.parametrize("engine", ["f16x2", "f32"])
@pytest.mark.parametrize("jump", [10, 11, 13])
@pytest.mark.parametrize("d", [64, 32])
def test_tail_small_y_under_a_jump_of_the_gradient_scale(dev, d, jump, engine):
    """No zero rows here: every |y| below 0.01 (layer-norm gains shrunk by training) and every workgroup's second chunk
    2^jump above its first. The running scale E is known one chunk late, so those rows enter 2^jump above E with the row
    factor 2^(jump + 6) on their y and in the "ones" operand of db. The y check sends a chunk to the fp32 path once a scaled
    entry reaches 32768, which such a y does not, and 2^16 is inf as an f16 piece: the kernel has to notice the factor
    itself. Same call and bounds as above."""
    cus = cu_count(dev)
    rows = CHUNK * 2 * cus * (1 if d == 64 else 2) + 7
    blocks = tail_blocks(rows, d, cus)
    rng = np.random.default_rng([15, d, jump])
    y = rng.uniform(-0.01, 0.01, size=(rows, d)).astype(np.float32)
    dqkv = rng.standard_normal((rows, 3 * d)).astype(np.float32)
    dqkv[CHUNK * blocks:] *= np.float32(2.0 ** jump)
    W = (rng.standard_normal((d, 3 * d)) / d ** 0.5).astype(np.float32)
    y64, g64, W64 = y.astype(np.float64), dqkv.astype(np.float64), W.astype(np.float64)
    tail_call_and_check(dev, d, rows, y, dqkv, W, np.ones(rows, dtype=bool), g64 @ W64.T, y64.T @ g64, np.abs(y64).T @ np.abs(g64),
                        g64.sum(0), np.abs(g64).sum(0), engine, f"d={d} rows={rows} jump=2^{jump} {engine}")


# ---- 1b: the LSTM weight-gradient pass -------------------------------------------------------------------------------------

@pytest.mark.parametrize("x_scale", [1.0, 0.05])
@pytest.mark.parametrize("layout", ["none", "one", "batch", "head"])
@pytest.mark.parametrize("d,t,n", [(64, 5, 5_003), (32, 6, 12_345)])
def test_lstm_weight_gradient_pass_on_zero_gradient_nodes(dev, d, t, n, layout, x_scale):
    """The tail's kernel in its LSTM form (ops.lstm_bwd(..., deferred_dw=True): sagnn_lstm_bwd_ws_f32 with a workspace) with dh
    zero outside the layout's nodes, by the method and at the bounds of test_lstm_weight_gradient_pass_at_any_gradient_scale:
    dx bit for bit the one-launch kernel's, db the one-launch kernel's up to the order of its float atomics (that test's
    assert_close; exactly equal where exactly zero), dW within 1e-6 of the sum of its terms' magnitudes of the float64 product
    of the stored gate gradients. x uniform in (-1, 1), and 0.05 of that (Xavier-sized embeddings: no row reaches 2^-3)."""
    from sa_gnn_amd.model import random_fusion_params
    lib = _lib.load()
    rng = np.random.default_rng([12, d, t, LAYOUTS.index(layout)])
    g = torch.Generator(device="cpu").manual_seed(d * 3 + t)
    x = ((torch.rand((n, t, d), generator=g) * 2 - 1) * x_scale).to(dev)
    p = random_fusion_params(d, dev, 11)
    h, gates, cell = ops.lstm_fwd_train(x, p["lstm_W"], p["lstm_b"])
    mask = row_mask(layout, n, rng)
    assert mask.any() == (layout != "none")
    dh = (torch.randn((n, t, d), generator=g) * torch.from_numpy(mask.astype(np.float32))[:, None, None]).to(dev)
    outs = []
    for use_ws in (False, True):
        dx = torch.empty((n, t, d), device=dev)
        dW = torch.zeros((2 * d, 4 * d), device=dev)
        db = torch.zeros(4 * d, device=dev)
        nbytes = int(lib.sagnn_lstm_bwd_workspace_bytes(n, t, d))
        ws = torch.zeros(nbytes // 4, device=dev) if use_ws else None
        ops.range_redo_count(reset=True)
        ops.check(lib.sagnn_lstm_bwd_ws_f32(x.data_ptr(), t * d, d, h.data_ptr(), gates.data_ptr(), cell.data_ptr(), dh.data_ptr(), t * d,
                                            None, p["lstm_W"].data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(), n, t, d,
                                            ops._ptr(ws), nbytes if use_ws else 0, None))
        outs.append((dx, dW, db, ws))
    redo = ops.range_redo_count()
    (dx0, dW0, db0, _), (dx1, dW1, db1, ws) = outs
    dx2, dW2, db2 = ops.lstm_bwd(x, h, gates, cell, dh, None, p["lstm_W"], deferred_dw=True)      # the wrapper, same entry
    dG = ws.view(t, n, 4 * d).double()                                                   # time-major
    xh = torch.cat([x.permute(1, 0, 2), torch.cat([torch.zeros((1, n, d), device=dev), h.permute(1, 0, 2)[:-1]])], dim=2).double()
    want = torch.einsum("tnk,tng->kg", xh, dG)
    mag = torch.einsum("tnk,tng->kg", xh.abs(), dG.abs())
    worst = {name: float(((got.double() - want).abs() / (1e-6 * mag + 1e-30)).max())
             for name, got in (("second pass", dW1), ("wrapper", dW2), ("one launch", dW0))}
    print(f"zero_grad_rows|lstm_dw|d={d} t={t} n={n} {layout} x*{x_scale}|redo={redo} of {(n * t + CHUNK - 1) // CHUNK} chunks"
          f"|db bit-equal={int(torch.equal(db0, db1))}|dW of its bound: {worst}")
    assert torch.equal(dx0, dx1) and torch.equal(dx0, dx2)
    assert bool(torch.isfinite(dW1).all()) and bool(torch.isfinite(dW2).all())
    for db in (db1, db2):
        torch.testing.assert_close(db, db0, rtol=1e-5, atol=1e-6 * float(db0.abs().max()))      # float atomics: order differs
        assert mask.sum() > 1 or torch.equal(db, db0)      # ... where more than one node has something to add
    tm = torch.from_numpy(mask).to(dev)
    assert int(torch.count_nonzero(dx1[~tm])) == 0 and int(torch.count_nonzero(dG[:, ~tm])) == 0
    assert (float(mag.max()) > 0) == (layout != "none")
    for name, f in worst.items():
        assert f <= 1.0, f"{name} [{layout}]: {f:.3e} of 1e-6 sum |terms|"
    if layout == "none":
        for a in (dx1, dW1, db1, dW2, db2, dW0, db0):
            assert int(torch.count_nonzero(a)) == 0
        assert redo == 0


# ---- 1c: the attention-backward front --------------------------------------------------------------------------------------

# one case per route of front_route: Split at three widths, F32Mfma at d / heads = 4 and 2 under both engines that reach it
FRONT_ZERO_CASES = [("f16x2", 64, 3, 16, "Split"), ("f16x2", 32, 4, 16, "Split"), ("f16x2", 128, 3, 16, "Split"),
                    ("f32", 64, 3, 16, "F32Mfma"), ("f32", 32, 4, 16, "F32Mfma"), ("f16x2", 64, 5, 32, "F32Mfma")]


def node_fractions(dq, dq64, n, mask):
    """The worst error as a fraction of test_front_route's two dqkv bounds (global, per node) over the nodes of `mask`."""
    e = np.abs(dq.astype(np.float64) - dq64)
    fg = (e / (1e-4 * np.abs(dq64) + 2e-5 * np.abs(dq64).max())).reshape(n, -1).max(axis=1)
    fn = e.reshape(n, -1).max(axis=1) / (1e-4 * np.abs(dq64).reshape(n, -1).max(axis=1) + 1e-300)
    return fg[mask], fn[mask]


@functools.lru_cache(maxsize=None)
def front_zero_reference(d, t, heads, n, layout):
    """test_gpu_bwd_routes.front_reference's screened nodes with g_out zero outside the layout's nodes: parameters, x, g_out,
    the mask, float64 (y, dqkv). The global bound follows the largest entry over the nodes that HAVE a gradient, so the
    float32 screen is repeated for them: a node at which float32 autograd leaves a quarter of a bound loses its gradient
    (under "one" the next node takes it)."""
    p, x, gout, _, _ = front_reference(d, t, heads, n)
    rng = np.random.default_rng([13, d, t, heads, LAYOUTS.index(layout)])
    mask = row_mask(layout, n, rng)
    for _ in range(n):
        g = np.where(mask[:, None], gout, np.float32(0.0))
        y64, dq64 = attn_bwd_front_reference(x.astype(np.float64), f64(p), g.astype(np.float64), heads, torch.float64, True)
        if not mask.any():
            break
        _, dq32 = attn_bwd_front_reference(x, p, g, heads, torch.float32, True)
        fg, fn = node_fractions(dq32, dq64, n, mask)
        over = np.flatnonzero(mask)[np.maximum(fg, fn) > 0.25]
        if len(over) == 0:
            break
        mask = mask.copy()
        mask[over] = False
        if layout == "one":
            mask[(over[0] + 1) % n] = True
    assert mask.any() == (layout != "none")
    return p, x, g, mask, y64, dq64


@pytest.mark.parametrize("layout", ["none", "one", "batch"])
@pytest.mark.parametrize("engine,d,t,heads,route", FRONT_ZERO_CASES, ids=lambda v: str(v))
def test_front_zero_gradient_nodes(dev, engine, d, t, heads, route, layout):
    """sagnn_attn_bwd_front_f32 as test_front_route calls it, g_out zero outside the layout's nodes: the dqkv rows of a node
    without gradient are exactly 0 (what the tail, and the padding rule of the sequence slab, rest on), y does not depend on
    g_out (bit for bit the y of a dense g_out), and the other nodes meet test_front_route's bounds."""
    assert front_route(engine, d, t, heads) == route
    tile = split_tile(t) if route == "Split" else mfma_tile(t)
    n = max(301, 2 * tile + 3)                           # several tiles, a ragged last one; ~3 nodes under "batch"
    p, x, gout, mask, y64, dq64 = front_zero_reference(d, t, heads, n, layout)
    _, _, dense, _, _ = front_reference(d, t, heads, n)
    pd = device_params(p, dev)
    guard = 32 * 3 * d
    xs = Slab(dev, (n, t, d), *x_layout("padded", n, t, d), values=x)
    ys = []
    for values in (gout, dense):
        g = Slab(dev, (n, d), (d + 4, 1), 4, values=values)
        dq, y = Window(dev, n * t, 3 * d, guard), Window(dev, n * t, d, guard)
        ops.check(call_front(engine, xs, t, d, heads, pd, True, g, dq, y))
        ys.append(y.read())
        if values is gout:
            got = dq.read()                              # no NaN left: every row was written, zero-gradient rows too
    assert np.array_equal(ys[0], ys[1]), "y depends on g_out"
    fy = float((np.abs(ys[0].reshape(n, t, d).astype(np.float64) - y64) / (ATOL + RTOL * np.abs(y64))).max())
    rows = np.repeat(mask, t)
    nz = int(np.count_nonzero(got[~rows]))
    fg, fn = node_fractions(got, dq64, n, mask) if mask.any() else (np.zeros(1), np.zeros(1))
    print(f"zero_grad_rows|front|{route} {engine} ({d}, {t}, {heads}) n={n} {layout}: {int(mask.sum())} nodes with a gradient"
          f"|non-zero entries in zero-gradient rows={nz}|y={fy:.4f} global={float(fg.max()):.4f} node={float(fn.max()):.4f}")
    assert not dq64[~rows].any()
    assert nz == 0, f"{nz} non-zero dqkv entries in the rows of nodes without gradient"
    assert fy <= 1.0
    assert float(fg.max()) <= 1.0, f"dqkv at {float(fg.max()):.3f} of the global bound"
    _per_row_ok(got.reshape(n, -1), dq64.reshape(n, -1), "dqkv per node")


# ---- 1d: the composed backward ---------------------------------------------------------------------------------------------

FUSION_NAMES = ("lstm_W", "lstm_b", "ln_gamma", "ln_beta", "Wq", "bq", "Wk", "bk", "Wv", "bv")


@functools.lru_cache(maxsize=2)
def fusion_zero_reference(d, t, n, layout, gain):
    """x, parameters (gain "init": as O.init_fusion_params draws them; a number: ln_gamma = that, ln_beta = 0, which bounds
    |y| by gain * sqrt(d - 1)), g_out zero outside the layout's nodes, and float64 autograd of O.torch_interval_fusion."""
    rng = np.random.default_rng([14, d, t, LAYOUTS.index(layout)])
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    if gain != "init":
        p["ln_gamma"] = np.full(d, gain, dtype=np.float32)
        p["ln_beta"] = np.zeros(d, dtype=np.float32)
        assert gain * np.sqrt(d - 1) < 0.125
    mask = row_mask(layout, n, rng)
    assert mask.any() == (layout != "none")
    gout = masked_normal(rng, mask, d, "ones")
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    (O.torch_interval_fusion(tx, tp, 16) * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    want = [tx.grad.numpy()] + [tp[k].grad.numpy() for k in FUSION_NAMES]
    assert not want[0][~mask].any()
    return x, p, gout, mask, want


@pytest.mark.parametrize("way", ["autograd", "direct-f32"])
@pytest.mark.parametrize("gain", ["init", 0.01])
@pytest.mark.parametrize("layout", ["none", "one", "batch"])
@pytest.mark.parametrize("d,t,n", [(64, 3, 9_001), (32, 4, 12_345), (64, 8, 2_003)])
def test_fusion_backward_on_zero_gradient_nodes(dev, d, t, n, layout, gain, way):
    """The whole fusion backward with g_out zero outside the layout's nodes, at the bounds of
    test_fusion_backward_dx_per_node_at_any_gradient_scale: dx per node at 1e-4 of the node's own largest entry (a node without
    gradient: exactly 0), parameter gradients at 1e-4 |b| + max(2e-5 max |b|, floor). "autograd": autograd.interval_fusion and
    .backward(), the default engine on the autograd thread, which is the path training takes (t = 8 defers the LSTM's weight
    gradient to the f16 x 2 pass); "direct-f32": the two halves called under ops.engine("f32") as that test calls them."""
    from sa_gnn_amd import autograd as ag
    x, p, gout, mask, want = fusion_zero_reference(d, t, n, layout, gain)
    xd, gd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(gout.copy()).to(dev)
    pd = {k: torch.from_numpy(v.copy()).to(dev) for k, v in p.items()}
    ops.range_redo_count(reset=True)
    if way == "autograd":
        for v in [xd] + list(pd.values()):
            v.requires_grad_(True)
        ag.interval_fusion(xd, pd, 16).backward(gd)
        grads = [xd.grad] + [pd[k].grad for k in FUSION_NAMES]
    else:
        with ops.engine("f32"):
            _, h, gates, cell = ag._fusion_forward(xd, *(pd[k] for k in FUSION_NAMES), 16, None)
            grads = ag._fusion_backward(xd, *(pd[k] for k in FUSION_NAMES if k != "lstm_b"), h, gates, cell, None, 16, gd)
    assert ops.get_engine() == "f16x2"
    redo = ops.range_redo_count()
    got = [g.detach().cpu().numpy().astype(np.float64) for g in grads]
    floor = 5e-6 * max(1.0, np.sqrt(n * t / 1000.0))      # accumulation noise of sums that cancel to ~0 (test_gpu_backward)
    frac = {}
    for k, a, b in zip(FUSION_NAMES, got[1:], want[1:]):
        frac[k] = float(np.nanmax(np.abs(a - b) / (1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), floor)))) if np.isfinite(a).all() else np.inf
    print(f"zero_grad_rows|fusion|({d}, {t}, {n}) {layout} gain={gain} {way}|redo={redo}|of their bounds: "
          + " ".join(f"{k}={v:.3g}" for k, v in frac.items()))
    _per_row_ok(got[0], want[0], "dx")
    assert not got[0][~mask].any()
    for k, a in zip(FUSION_NAMES, got[1:]):
        assert np.isfinite(a).all(), f"{k}: non-finite"
        assert frac[k] <= 1.0, f"{k}: {frac[k]:.3f} of its bound"
        if layout == "none":
            assert not a.any(), f"{k}: a gradient of zeros gave {np.abs(a).max():.3e}"


# ---- 1e: the training objective on a graph much larger than the batch ------------------------------------------------------

def _oracle_in(P, leaves, dtype):
    """The oracle's parameter structure of test_gpu_train._oracle_params with every leaf as a fresh leaf of `dtype`."""
    fresh = {id(v): v.detach().to(dtype).requires_grad_(True) for v in leaves.values()}

    def conv(o):
        if isinstance(o, torch.Tensor):
            return fresh[id(o)]
        if isinstance(o, dict):
            return {k: conv(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(conv(v) for v in o)
        return o

    return conv(P), {k: fresh[id(v)] for k, v in leaves.items()}


@pytest.mark.parametrize("gain", [1.0, 0.01])
@pytest.mark.parametrize("d,ssldim,att_layer", [(64, 48, 2), (32, 32, 1)])
def test_training_objective_gradients_on_a_graph_much_larger_than_the_batch(dev, d, ssldim, att_layer, gain):
    """train_loss and .backward() with 16 batch users of 1500 (1200 items), under --fusion_rows all and batch: nearly every
    32-row chunk of the fusion's upstream gradient is zero. Against float64 O.torch_train_loss at the bounds of
    test_training_objective_gradients, every gradient finite; the fusion layer norms' gains as initialised (1) and at 0.01,
    where no layer-normed entry of a zero-gradient chunk need reach 2^-3. Those bounds were set at gains of 1: a tensor at
    which float32 O.torch_train_loss on the CPU is itself not within a quarter of its bound is judged at four times the
    float32 restatement's error instead, and the test prints which (measured: mhsa1_q_bias at d = 64 and gain 0.01, float32
    at 0.277 of its bound; no tensor in the other three cases)."""
    from test_gpu_train import _oracle_params, _setup
    rec, handler, NNs, args = _setup(dev, d, ssldim, att_layer, U=1500, I=1200, nnz=(15000, 14000))
    try:
        with torch.no_grad():
            for gm, _ in (rec.ln[0], rec.ln[1]):
                gm.fill_(gain)
        np.random.seed(3)
        import random
        random.seed(3)
        batIds = np.random.permutation(args.user)[:args.batch]
        uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
        su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
        batch = {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si}
        P, leaves = _oracle_params(rec, NNs)
        adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
        tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
        cfg = {"T": 2, "L": 2, "leaky": 0.5, "heads": 16}
        opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, dict(batch), cfg)
        (opre + args.ssl_reg * ossl).backward()
        P32, leaves32 = _oracle_in(P, leaves, torch.float32)
        pre32, ssl32, _, _ = O.torch_train_loss(P32, adj, tp, dict(batch), cfg)
        (pre32 + args.ssl_reg * ssl32).backward()
        tols, widened = {}, []
        for name, leaf in leaves.items():
            if leaf.grad is None:
                continue
            b = leaf.grad.numpy()
            floor = max(5e-5 * np.abs(b).max(), 2e-5)
            if name.endswith("k_bias"):                  # analytically ~0: see test_training_objective_gradients
                floor = max(floor, 1e-3 * float(leaves[name.replace("k_bias", "k_kernel")].grad.abs().max()))
            tol = 2e-4 * np.abs(b) + floor
            err32 = np.abs(leaves32[name].grad.double().numpy() - b)
            if (err32 > 0.25 * tol).any():
                widened.append(f"{name} (float32 at {float((err32 / tol).max()):.3f} of the bound)")
                tol = np.maximum(tol, 4.0 * err32)
            tols[name] = tol
        print(f"zero_grad_rows|train|d={d} gain={gain}|judged at 4 x the float32 restatement's error: {widened or 'no tensor'}")
        for mode in ("all", "batch"):
            args.fusion_rows = mode
            for p in NNs.params.values():
                p.grad = None
            ops.range_redo_count(reset=True)
            pre, ssl = rec.train_loss(batch, keep_rate=1.0)
            (pre + args.ssl_reg * ssl).backward()
            redo = ops.range_redo_count()
            assert abs(float(pre.detach()) - float(opre.detach())) <= 1e-4 * max(abs(float(opre.detach())), 1.0)
            assert abs(float(ssl.detach()) - float(ossl.detach())) <= 1e-4 * max(abs(float(ossl.detach())), 1.0)
            checked, worst = 0, {}
            for name, leaf in leaves.items():
                got = NNs.params[name].grad
                if leaf.grad is None:
                    assert got is None or float(got.abs().max()) == 0.0, name
                    continue
                assert got is not None, f"no gradient reached {name}"
                a = got.cpu().double().numpy()
                assert np.isfinite(a).all(), f"--fusion_rows {mode}: {name} is not finite"
                worst[name] = float((np.abs(a - leaf.grad.numpy()) / tols[name]).max())
                checked += 1
            top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
            print(f"zero_grad_rows|train|d={d} gain={gain} --fusion_rows {mode}|redo={redo}|worst of their bounds: {top}")
            for name, f in worst.items():
                assert f <= 1.0, f"--fusion_rows {mode}: {name} at {f:.3f} of its bound"
            assert checked >= 20
    finally:
        args.fusion_rows = "all"
