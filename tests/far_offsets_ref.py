"""Case tables and index arithmetic of tests/test_gpu_far_offsets.py: operands whose checked rows lie more than 2^29, 2^30
and 2^31 floats from the pointer an entry is given. Nothing here touches a device; tests/test_far_offsets_host.py checks
the tables on the CPU.

Two kinds of case. Kind "A", far by stride: an operand the ABI gives a row stride gets the largest stride its route admits
(its guard less 4 where the library has one, else 2^26, or the largest power of two that keeps the case under CAP_BYTES), and
the fewest rows that give two full tiles of the kernel, a ragged one and four rows past 2^31 floats; every row is checked.
Kind "B", far by count: a contiguous operand, as the workload has it, long enough to carry its last 128 nodes and a ragged
tile past 2^31 floats; checked_nodes() names the nodes compared with float64.

An operand is (name, shape, strides, far, checked): shape and strides (in floats) of the window inside its NaN-filled
buffer, whether it is one of the case's far operands, and the checked nodes (None: every node; dimension 0 is the node)."""
import collections

import numpy as np

from test_gpu_bwd_routes import SPECIALISED_T, bptt_route, front_route, tail_route   # noqa: F401  (restated selectors)

T29, T30, T31 = 1 << 29, 1 << 30, 1 << 31
THRESHOLDS = (T29, T30, T31)                             # signed 32-bit bytes, unsigned 32-bit bytes, signed 32-bit elements
CAP_BYTES = 40 << 30                                     # a case's device bytes, summed from its shapes
PAD = 4                                                  # NaNs in front of and behind every window: 16 bytes

# the four host-side guards (include/sagnn.h, "Stride limits"): value, what the library does at it
LD_H_F16X2 = 1 << 22                                     # lstm_f16.hip / engine.cpp: reroute to F32Mfma
LD_MFMA = 1 << 24                                        # fusion_mfma.hip lstm_fwd_mfma: refuse (ld_n, ld_h)
LD_GRU = 1 << 24                                         # gru.hip gru_fwd_fused: refuse (ld_n, ld_h)
LD_BPTT = 1 << 25                                        # lstm_bwd_mfma.hip check_lstm_bwd: refuse (ld_n, ld_dhe)
LD_FREE = 1 << 26                                        # where no guard binds

Operand = collections.namedtuple("Operand", "name shape strides far checked")
Case = collections.namedtuple("Case", "kind entry engine d t heads n route tile operands note")


def stride_rows(ld, tile):
    """Kind A's row count: two full tiles and a ragged one, the last four rows past 2^31 floats."""
    n = max(2 * tile + 1, -(-T31 // ld) + 4)
    while n % tile == 0:
        n += 1
    return n


def span(op):
    """Floats from the window's first element to one past its last."""
    return sum((s - 1) * st for s, st in zip(op.shape, op.strides)) + 1


def buffer_floats(op):
    return span(op) + 2 * PAD


def case_bytes(case):
    """Device bytes of the case's buffers (weights and row lists are a few hundred KiB and not counted)."""
    return 4 * sum(buffer_floats(op) for op in case.operands)


def row_offsets(op):
    """Offsets in floats, from the pointer the entry is given, of the first element of every checked row: the checked
    nodes (dimension 0) at every index of the dimensions between the node and the row."""
    nodes = range(op.shape[0]) if op.checked is None else op.checked
    inner = [0]
    for size, st in zip(op.shape[1:-1], op.strides[1:-1]):
        inner = [o + i * st for o in inner for i in range(size)]
    return [i * op.strides[0] + o for i in nodes for o in inner]


def checked_nodes(n, node_floats, tile):
    """Kind B: the first 128 nodes, the 256 centred on each threshold crossing, the last 128 and the ragged tail."""
    keep = set(range(min(128, n)))
    for thr in THRESHOLDS:
        c = thr // node_floats
        keep.update(i for i in range(c - 128, c + 128) if 0 <= i < n)
    keep.update(range(max(0, n - 128 - n % tile), n))
    return tuple(sorted(keep))


def checked_nodes_time_major(n, row_floats, tile):
    """checked_nodes() for [T, N, row] storage: a threshold is crossed inside one step s, at node (thr mod N row) / row."""
    keep = set(range(min(128, n)))
    for thr in THRESHOLDS:
        c = (thr % (n * row_floats)) // row_floats
        keep.update(i for i in range(c - 128, c + 128) if 0 <= i < n)
    keep.update(range(max(0, n - 128 - n % tile), n))
    return tuple(sorted(keep))


def checked_nodes_both(n, t, d, tile):
    """A case that holds both the time-major [T, N, d] slab and node-major [n, t, d] operands of the same length: the
    crossing windows of both layouts."""
    return tuple(sorted(set(checked_nodes(n, t * d, tile)) | set(checked_nodes_time_major(n, d, tile))))


def crossing_nodes(op):
    """The node that holds float `thr`, per threshold, in the operand's own layout: node-major (the node stride is the
    largest) or time-major (a step's stride is N times the node's)."""
    n, ld_n = op.shape[0], op.strides[0]
    if len(op.shape) == 3 and op.strides[1] > ld_n:
        return [(thr % op.strides[1]) // ld_n for thr in THRESHOLDS]
    return [thr // ld_n for thr in THRESHOLDS]


def count_rows(node_floats, tile):
    """Kind B's node count: the last 128 nodes and a ragged tile past 2^31 floats."""
    n = -(-T31 // node_floats) + 128 + 1
    while n % tile == 0:
        n += 1
    return n


# ---- forward selectors, restated (csrc/engine.cpp:48-66) ---------------------------------------------------------------------

def lstm_route(engine, d, t, ld_h, train=False, drop=False):
    """select_lstm_fwd for 16-byte aligned x, h and mask."""
    if engine == "valu":
        return "Valu"
    if d in (32, 64):
        if engine == "f16x2" and not (train and drop) and ld_h < LD_H_F16X2 and t * d < 1 << 18:
            return "F16x2"
        return "F32Mfma"
    if d == 128 and engine == "f16x2":
        return "Split128"
    return "Valu"


def attn_route(engine, d, t, heads):
    """select_attn_fwd for a 16-byte aligned x."""
    if engine == "valu":
        return "Valu"
    if engine == "f16x2" and heads == 16 and d in (32, 64, 128) and t in SPECIALISED_T:
        return "Split"
    dk = d // heads
    if d in (32, 64) and 1 <= t <= 32 and d % heads == 0 and dk & (dk - 1) == 0:
        return "F32Mfma"
    if d not in (32, 64) and d % 32 == 0 and 32 <= d <= 256:
        return "Wide"
    return "Valu"


def attn_workspace_bytes(route, n, t, d):
    """What sagnn_ln_mhsa_mean_workspace_bytes reserves per route (csrc/engine.cpp:31-32)."""
    return {"Split": 0, "F32Mfma": 0, "Valu": n * t * d * 4, "Wide": n * t * d * 4 * 4}[route]


# ---- tiles: rows that share one base -------------------------------------------------------------------------------------

LSTM_TILE = {"F16x2": 96, "F32Mfma": 32, "Split128": 64}   # lstm_f16_kernel.h:37, fusion_mfma.hip:52, lstm_split128.hip:36


def lstm_tile(route, d):
    return LSTM_TILE.get(route, (256 // d) * 4)          # Valu: (256 / d) * 4 rows per block


def attn_tile(route, d, t):
    if route == "Split":
        return 64 // t                                   # attn_split.hip:38
    if route == "F32Mfma":
        return 4 * (32 // t)                             # fusion_mfma.hip:973
    return max(1, 256 // d)                              # Valu and Wide: node slots of a block


def ntd(name, n, t, d, ld_n, far, checked=None):
    return Operand(name, (n, t, d), (ld_n, d, 1), far, checked)


def rows(name, n, d, ld, far, checked=None):
    return Operand(name, (n, d), (ld, 1), far, checked)


def time_major(name, n, t, d, far, checked=None):
    """The [T, N, d] slab itself: ld_n = d, ld_t = N d."""
    return Operand(name, (n, t, d), (d, n * d, 1), far, checked)


# ---- kind A: LSTM forward -------------------------------------------------------------------------------------------------
# (engine, d, t, far operand, its stride): F16x2 and F32Mfma at both widths on x and on h, F32Mfma at the first ld_h the f16
# kernel declines, Split128 and Valu at d = 128. x has no guard on F16x2, Split128 and Valu: 2^26 where CAP_BYTES allows,
# 2^25 at the 96- and 64-row tiles.

def _lstm_a():
    spec = []
    for d in (32, 64):
        spec += [("f16x2", d, 16, "x", LD_FREE >> 1), ("f16x2", d, 16, "h", LD_H_F16X2 - 4),
                 ("f32", d, 16, "x", LD_MFMA - 4), ("f32", d, 16, "h", LD_MFMA - 4)]
    spec += [("f16x2", 64, 16, "h", LD_H_F16X2)]
    spec += [("f16x2", 128, 4, "x", LD_FREE >> 1), ("f16x2", 128, 4, "h", LD_FREE >> 1),
             ("valu", 128, 4, "x", LD_FREE), ("valu", 128, 4, "h", LD_FREE)]
    out = []
    for engine, d, t, far, ld in spec:
        ld_h = ld if far == "h" else t * d + 4
        route = lstm_route(engine, d, t, ld_h)
        tile = lstm_tile(route, d)
        n = stride_rows(ld, tile)
        ops = (ntd("x", n, t, d, ld if far == "x" else t * d + 4, far == "x"), ntd("h", n, t, d, ld_h, far == "h"))
        out.append(Case("A", "lstm_fwd", engine, d, t, 0, n, route, tile, ops, f"{far} ld={ld}"))
    return out


LSTM_A = _lstm_a()


def _lstm_state():
    """sagnn_lstm_fwd_state_f32 with h_init at a far ld_hi (F32Mfma reads it through 64-bit addresses: no guard)."""
    engine, d, t, ld = "f32", 64, 4, LD_FREE
    route = lstm_route(engine, d, t, t * d + 4)
    n = stride_rows(ld, lstm_tile(route, d))
    ops = (ntd("x", n, t, d, t * d + 4, False), ntd("h", n, t, d, t * d + 4, False), rows("h_init", n, d, ld, True),
           rows("c", n, d, d, False))
    return [Case("A", "lstm_fwd_state", engine, d, t, 0, n, route, lstm_tile(route, d), ops, f"h_init ld={ld}")]


LSTM_STATE = _lstm_state()


# ---- kind B: LSTM forward on the time-major slab, h past 2^31 -------------------------------------------------------------

def _lstm_b():
    out = []
    for engine, d in (("f16x2", 64), ("f32", 64), ("f16x2", 32), ("f32", 32)):
        t = 16
        route = lstm_route(engine, d, t, t * d)
        tile = lstm_tile(route, d)
        n = count_rows(t * d, tile)
        chk = checked_nodes_both(n, t, d, tile)
        ops = (time_major("x", n, t, d, True, chk), ntd("h", n, t, d, t * d, True, chk), ntd("drop", n, t, d, t * d, True, chk))
        out.append(Case("B", "lstm_fwd", engine, d, t, 0, n, route, tile, ops, "time-major x, h and mask past 2^31"))
    return out


LSTM_B = _lstm_b()


# ---- kind A: attention forward --------------------------------------------------------------------------------------------
# sagnn_ln_mhsa_mean_f32 on the four routes at t = 16, x and out both at 2^26 (no guard on any route);
# sagnn_interval_fusion_f32 likewise, but with x at the stride its LSTM admits: 2^24 - 4 (F32Mfma's guard) under f32.

ATTN_SHAPES = [("f16x2", 64, 16, 16), ("f32", 64, 16, 16), ("f16x2", 128, 16, 8), ("valu", 64, 16, 16)]   # engine, d, t, heads


def _attn_a():
    out = []
    for engine, d, t, heads in ATTN_SHAPES:
        route = attn_route(engine, d, t, heads)
        tile = attn_tile(route, d, t)
        n = stride_rows(LD_FREE, tile)
        ops = (ntd("x", n, t, d, LD_FREE, True), rows("out", n, d, LD_FREE, True))
        out.append(Case("A", "ln_mhsa_mean", engine, d, t, heads, n, route, tile, ops, f"x, out ld={LD_FREE}"))
        ld = LD_MFMA - 4 if engine == "f32" else LD_FREE
        tile = max(tile, lstm_tile(lstm_route(engine, d, t, t * d), d))   # the LSTM in front has the larger tile
        if 8 * stride_rows(ld, tile) * ld > CAP_BYTES:   # x and out at this stride: the 96-row LSTM tile at 2^26
            ld >>= 2
        n = stride_rows(ld, tile)
        ops = (ntd("x", n, t, d, ld, True), rows("out", n, d, ld, True))
        out.append(Case("A", "interval_fusion", engine, d, t, heads, n, route, tile, ops, f"x, out ld={ld}"))
    return out


ATTN_A = _attn_a()


# ---- kind A: attention backward front -------------------------------------------------------------------------------------

FRONT_SHAPES = [("f16x2", 64, 16, 16), ("f32", 64, 8, 16)]   # Split at its longest t, F32Mfma at its longest


def _front_a():
    out = []
    for engine, d, t, heads in FRONT_SHAPES:
        route = front_route(engine, d, t, heads)
        tile = 64 // t if route == "Split" else 4 * (32 // t)
        n = stride_rows(LD_FREE, tile)
        ops = (ntd("x", n, t, d, LD_FREE, True), rows("g_out", n, d, LD_FREE, True), rows("dqkv", n * t, 3 * d, 3 * d, False),
               rows("y", n * t, d, d, False))
        out.append(Case("A", "attn_bwd_front", engine, d, t, heads, n, route, tile, ops, f"x, g_out ld={LD_FREE}"))
    return out


FRONT_A = _front_a()


# ---- kind A: BPTT -----------------------------------------------------------------------------------------------------------

def _bptt_a():
    out = []
    for engine, ws in (("f32", False), ("f16x2", True)):
        d, t, ld = 64, 4, LD_BPTT - 4
        n = stride_rows(ld, 32)                          # lstm_bwd_mfma.hip:62
        ops = [ntd("x", n, t, d, ld, True), ntd("dh_ext", n, t, d, ld, True), rows("dx", n * t, d, d, False),
               ntd("x_fwd", n, t, d, t * d + 4, False),   # the training forward's own x: F32Mfma stops at ld_n = 2^24
               rows("h", n * t, d, d, False), rows("gates", n * t, 4 * d, 4 * d, False), rows("cell", n * t, d, d, False)]
        if ws:
            ops.append(rows("workspace", n * t, 4 * d, 4 * d, False))
        out.append(Case("A", "lstm_bwd_ws", engine, d, t, 0, n, bptt_route(engine, d, ws), 32, tuple(ops), f"x, dh_ext ld={ld}"))
    return out


BPTT_A = _bptt_a()


# ---- kind A: GRU ------------------------------------------------------------------------------------------------------------

def _gru_a():
    out = []
    for d in (32, 64):
        t, ld = 4, LD_GRU - 4
        n = stride_rows(ld, 32)                          # gru.hip:29
        for far in ("x", "h"):
            ops = (ntd("x", n, t, d, ld if far == "x" else t * d + 4, far == "x"),
                   ntd("h", n, t, d, ld if far == "h" else t * d + 4, far == "h"))
            out.append(Case("A", "gru_fwd", "f16x2", d, t, 0, n, "Fused", 32, ops, f"{far} ld={ld}"))
    return out


GRU_A = _gru_a()


def _gru_bwd_a():
    """The two element-wise backward entries with their strided operands 2^24 - 4 floats apart: dh_ext (ld_dhe) and dh_rec
    (ld_dhr) of gru_bwd_cand, d_rh (ld_drh, read and written) of gru_bwd_gates. No tile: a grid-stride loop over n d."""
    d, t, ld = 64, 4, LD_GRU - 4
    n = stride_rows(ld, 32)
    dense = (ntd("gates", n, t, 2 * d, t * 2 * d, False), ntd("cand", n, t, d, t * d, False), ntd("h", n, t, d, t * d, False))
    cand = dense + (ntd("dh_ext", n, t, d, ld, True), rows("dh_rec", n, d, ld, True), rows("da_c", n, d, d, False),
                    rows("du", n, d, d, False), rows("dh_u", n, d, d, False))
    gates = dense + (rows("du", n, d, d, False), rows("dh_u", n, d, d, False), rows("d_rh", n, d, ld, True),
                     rows("da_g", n, 2 * d, 2 * d, False), rows("rh", n, d, d, False))
    return [Case("A", "gru_bwd_cand", "f16x2", d, t, 0, n, "Step", 32, cand, f"dh_ext, dh_rec ld={ld}"),
            Case("A", "gru_bwd_gates", "f16x2", d, t, 0, n, "Step", 32, gates, f"d_rh ld={ld}")]


GRU_BWD_A = _gru_bwd_a()


def _gru_b():
    """The training forward with gates [n, t, 2d] past 2^31 floats, then both backward entries at its last step on what
    it stored."""
    d, t = 64, 16
    n = count_rows(t * 2 * d, 32)
    chk = checked_nodes(n, t * 2 * d, 32)
    ops = (time_major("x", n, t, d, False, chk), ntd("h", n, t, d, t * d, False, chk), ntd("gates", n, t, 2 * d, t * 2 * d, True, chk),
           ntd("cand", n, t, d, t * d, False, chk), ntd("dh_ext", n, t, d, t * d, False, chk), rows("dh_rec", n, d, d, False, chk),
           rows("da_c", n, d, d, False, chk), rows("du", n, d, d, False, chk), rows("dh_u", n, d, d, False, chk),
           rows("d_rh", n, d, d, False, chk), rows("da_g", n, 2 * d, 2 * d, False, chk), rows("rh", n, d, d, False, chk))
    return [Case("B", "gru_fwd+bwd", "f16x2", d, t, 0, n, "Fused", 32, ops, "gates past 2^31")]


GRU_B = _gru_b()


# ---- kind A: dense_nn -------------------------------------------------------------------------------------------------------

def _dense_a():
    out = []
    for din, dout in ((64, 192), (128, 64)):             # the resident-W kernel at two shapes (dense.hip), 32-row wave tiles
        n = stride_rows(LD_FREE, 32)
        ops = (rows("X", n, din, LD_FREE, True), rows("Y", n, dout, LD_FREE, True))
        out.append(Case("A", "dense_nn", "f16x2", din, 1, dout, n, "Resident", 32, ops, f"ldx, ldy={LD_FREE}"))
    return out


DENSE_A = _dense_a()


# ---- rows_gather / rows_scatter ---------------------------------------------------------------------------------------------

def _rows():
    """Every row of a 69-row source / target at ld_n = 2^26 is listed (fewer than 128 rows: the last 128 are all of them),
    in a shuffled order, so the ids on both sides of each threshold are moved."""
    d, t, ld = 64, 4, LD_FREE
    n = stride_rows(ld, 32)
    ops = (ntd("x", n, t, d, ld, True), ntd("out", n, t, d, t * d, False))
    return [Case("A", "rows_gather", "f16x2", d, t, 0, n, "Rows", 32, ops, f"source ld_n={ld}"),
            Case("A", "rows_scatter", "f16x2", d, t, 0, n, "Rows", 32,
                 (ntd("dst", n, t, d, ld, True), ntd("src", n, t, d, t * d, False)), f"target ld_n={ld}")]


ROWS = _rows()

# ---- sagnn_spmm_f32 gathering from an X with ldx = 2^16 over 40 k source rows ------------------------------------------------

SPMM_TUNING = (8, 128, 64)                               # every degree class at a size the oracle finishes instantly


def spmm_graph():
    """CSR of 2051 rows over 40003 sources: empty, short, one-wave and chunked rows, as tests/test_gpu_spmm.py draws them."""
    rng = np.random.default_rng(15)
    n_rows, n_src = 2051, 40003
    degs = rng.integers(0, 12, size=n_rows)
    degs[rng.choice(n_rows, 60, replace=False)] = rng.integers(13, 200, size=60)
    degs[[5, 400, 2050]] = [1400, 900, 3000]
    degs[[0, 1, 2, 100]] = 0
    cols = [np.sort(rng.choice(n_src, size=int(dg), replace=False)) for dg in degs]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    colidx = np.concatenate(cols).astype(np.int32)
    return n_rows, n_src, rowptr, colidx


def _spmm():
    n_rows, n_src, _, colidx = spmm_graph()
    d, ldx = 64, 1 << 16
    gathered = tuple(int(c) for c in np.unique(colidx))
    ops = (rows("X", n_src, d, ldx, True, gathered), rows("out", n_rows, d, d + 4, False))
    return [Case("S", "spmm", "f16x2", d, 1, 0, n_src, "Spmm", 16, ops, f"ldx={ldx}")]   # spmm.hip:45: 16 rows per wave


SPMM = _spmm()

# ---- sagnn_gnn_stack_f32 / _bwd_f32 with slab strides of 2^30 - 4 -----------------------------------------------------------
# T = 4 intervals: interval 1 starts past 2^29 floats, the rows of interval 2 pass 2^31 from its second row on, interval 3
# lies past 2^31. Inputs far and outputs far are separate cases: the four slabs together would take 48 GiB.

STACK_T, STACK_U, STACK_I, STACK_D, STACK_L = 4, 2051, 1531, 64, 2
STACK_SLAB = T30 - 4


def slabs(name, n_rows, far):
    return Operand(name, (STACK_T, n_rows, STACK_D), (STACK_SLAB if far else n_rows * STACK_D, STACK_D, 1), far, None)


def _stack():
    out = []
    for entry in ("gnn_stack", "gnn_stack_bwd"):
        for far in ("in", "out"):
            ops = (slabs("in_u", STACK_U, far == "in"), slabs("in_i", STACK_I, far == "in"),
                   slabs("out_u", STACK_U, far == "out"), slabs("out_i", STACK_I, far == "out"))
            out.append(Case("S", entry, "f16x2", STACK_D, STACK_T, 0, STACK_U, "Stack", 16, ops, f"{far} slabs={STACK_SLAB}"))
    return out


STACK = _stack()

# ---- kind B: the training forward, gates [n, t, 4d] past 2^31 ------------------------------------------------------------------
# (engine, d, mask) at both widths: F16x2 without a mask, F32Mfma with one under f16x2 (training with a mask leaves the f16
# kernel), and F32Mfma under f32 without and with a mask.

def _train_b():
    out = []
    for engine, d, mask in (("f16x2", 64, False), ("f16x2", 64, True), ("f32", 64, False), ("f32", 64, True),
                            ("f16x2", 32, False), ("f16x2", 32, True), ("f32", 32, False), ("f32", 32, True)):
        t = 16
        route = lstm_route(engine, d, t, t * d, train=True, drop=mask)
        tile = lstm_tile(route, d)
        n = count_rows(t * 4 * d, tile)
        chk = checked_nodes(n, t * 4 * d, tile)
        ops = [time_major("x", n, t, d, False, chk), ntd("h", n, t, d, t * d, False, chk),
               ntd("gates", n, t, 4 * d, t * 4 * d, True, chk), ntd("cell", n, t, d, t * d, False, chk)]
        if mask:
            ops.append(ntd("drop", n, t, d, t * d, False, chk))
        out.append(Case("B", "lstm_fwd_train", engine, d, t, 0, n, route, tile, tuple(ops), "gates past 2^31" + (", mask" if mask else "")))
    return out


TRAIN_B = _train_b()


# ---- kind B: attention forward on the time-major slab ------------------------------------------------------------------------

def _attn_b():
    out = []
    for engine, d, t, heads in (("f16x2", 64, 16, 16), ("f32", 64, 8, 32)):
        route = attn_route(engine, d, t, heads)
        tile = attn_tile(route, d, t)
        for entry in ("ln_mhsa_mean", "interval_fusion"):
            tl = tile if entry == "ln_mhsa_mean" else max(tile, lstm_tile(lstm_route(engine, d, t, t * d), d))
            n = count_rows(t * d, tl)
            chk = checked_nodes_both(n, t, d, tl)
            ops = [time_major("x", n, t, d, True, chk), rows("out", n, d, d, False, chk)]
            if entry == "interval_fusion":
                ops.append(ntd("workspace", n, t, d, t * d, False))   # the LSTM's h: sagnn_interval_fusion_workspace_bytes
            out.append(Case("B", entry, engine, d, t, heads, n, route, tl, tuple(ops), "time-major x past 2^31"))
    return out


ATTN_B = _attn_b()


# ---- kind B: attention backward front, dqkv [n t, 3d] past 2^31 --------------------------------------------------------------

def _front_b():
    out = []
    for engine, d, t, heads in FRONT_SHAPES:
        route = front_route(engine, d, t, heads)
        tile = 64 // t if route == "Split" else 4 * (32 // t)
        n = count_rows(t * 3 * d, tile)
        chk = checked_nodes(n, t * 3 * d, tile)
        ops = (ntd("x", n, t, d, t * d, False, chk), rows("g_out", n, d, d, False, chk),
               ntd("dqkv", n, t, 3 * d, t * 3 * d, True, chk), ntd("y", n, t, d, t * d, False, chk))
        out.append(Case("B", "attn_bwd_front", engine, d, t, heads, n, route, tile, ops, "dqkv past 2^31"))
    return out


FRONT_B = _front_b()


# ---- kind B: attention backward tail, rows x 3d past 2^31 --------------------------------------------------------------------

def _tail_b():
    out = []
    for engine, d in (("f16x2", 64), ("f32", 64), ("f16x2", 32), ("f32", 32)):
        rows_ = count_rows(3 * d, 32)                    # attn_bwd_tail.hip:26, attn_bwd_tail_f16.hip:40
        chk = checked_nodes(rows_, 3 * d, 32)
        ops = (rows("y", rows_, d, d, False, chk), rows("dqkv", rows_, 3 * d, 3 * d, True, chk))
        out.append(Case("B", "attn_bwd_tail", engine, d, 1, 0, rows_, tail_route(engine, d), 32, ops, "dqkv past 2^31"))
    return out


TAIL_B = _tail_b()


# ---- kind B: BPTT, gates [n, t, 4d] past 2^31 --------------------------------------------------------------------------------

def _bptt_b():
    out = []
    for engine, ws in (("f32", False), ("f16x2", True)):
        d, t = 64, 16
        n = count_rows(t * 4 * d, 32)
        chk = checked_nodes(n, t * 4 * d, 32)
        ops = [time_major("x", n, t, d, False, chk), ntd("dh_ext", n, t, d, t * d, False, chk), ntd("dx", n, t, d, t * d, False, chk),
               ntd("h", n, t, d, t * d, False), ntd("gates", n, t, 4 * d, t * 4 * d, True, chk), ntd("cell", n, t, d, t * d, False)]
        if ws:
            ops.append(rows("workspace", n * t, 4 * d, 4 * d, False))
        out.append(Case("B", "lstm_bwd_ws", engine, d, t, 0, n, bptt_route(engine, d, ws), 32, tuple(ops), "gates past 2^31"))
    return out


BPTT_B = _bptt_b()

# ---- kind B: dense products on contiguous rows past 2^31 ----------------------------------------------------------------------

def _dense_b():
    d = 64
    n = count_rows(d, 32)
    chk = checked_nodes(n, d, 32)
    out = [Case("B", "dense_nn", "f16x2", d, 1, d, n, "Resident", 32, (rows("X", n, d, d, True, chk), rows("Y", n, d, d, True, chk)),
                "X, Y past 2^31"),
           Case("B", "dense_tn", "f16x2", d, 1, d, n, "Tn", 32, (rows("X", n, d, d, True, chk), rows("G", n, d, d, True, chk)),
                "X, G past 2^31")]
    # the BPTT's weight gradient: x [n, t, d] node-major against gate gradients [t, n, 4d], one segment per step
    t = 16
    n = count_rows(t * 4 * d, 32)
    chk = checked_nodes_time_major(n, 4 * d, 32)
    out.append(Case("B", "dense_tn_seg", "f16x2", d, t, 4 * d, n, "GemmTn", 32,
                    (ntd("X", n, t, d, t * d, False, chk), time_major("G", n, t, 4 * d, True, chk)), "time-major G past 2^31"))
    return out


DENSE_B = _dense_b()

# sagnn_dense_tn_seg_f32 at the most rows one call admits (seg_rows * n_seg < 2^31) that memory allows: 2^31 - 2^16 rows in
# 2^15 - 1 segments of 2^16 rows, each segment one row further on than the one before, so that the operands stay small
SEG_LIMIT = dict(seg_rows=1 << 16, n_seg=(1 << 15) - 1, din=32, dout=32)

STRIDE_CASES = LSTM_A + LSTM_STATE + ATTN_A + FRONT_A + BPTT_A + GRU_A + GRU_BWD_A + DENSE_A + ROWS
COUNT_CASES = LSTM_B + TRAIN_B + ATTN_B + FRONT_B + TAIL_B + BPTT_B + DENSE_B + GRU_B
ALL_CASES = STRIDE_CASES + COUNT_CASES + SPMM + STACK


def case_id(case):
    return f"{case.kind}-{case.entry}-{case.engine}-d{case.d}-t{case.t}-{case.route}-{case.note.replace(' ', '_')}"


# ---- the two mutations the suite has to catch, by arithmetic ----------------------------------------------------------------

def wrap_i32(v):
    """A 64-bit value through a signed 32-bit variable."""
    return (v + T31) % (1 << 32) - T31
