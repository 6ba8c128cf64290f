"""CPU checks of tests/test_gpu_far_offsets.py: its case tables (tests/far_offsets_ref.py) against the three thresholds, the
tile sizes, the library's own queries and the memory cap; the four stride guards at their limit values; and, by arithmetic,
that two one-word mutations of the addressing code land on rows the GPU cases compare. No device is touched."""
import ctypes

import pytest

import far_offsets_ref as R
from sa_gnn_amd import _lib

ENGINE_CODE = {"f16x2": 0, "f32": 1, "valu": 2}
ERR_ARG = -5


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.sagnn_get_engine()
    yield lib
    lib.sagnn_set_engine(prev)


@pytest.fixture
def p():
    """A 16-byte aligned host address: the refusals below come before any device work, as in tests/test_host.py."""
    buf = (ctypes.c_float * 64)()
    yield (ctypes.addressof(buf) + 15) & ~15
    del buf


@pytest.mark.parametrize("case", R.ALL_CASES, ids=[R.case_id(c) for c in R.ALL_CASES])
def test_every_far_operand_has_checked_rows_on_both_sides_of_each_threshold(case):
    far = [op for op in case.operands if op.far]
    assert far, "a case without a far operand"
    for op in far:
        offs = R.row_offsets(op)
        for thr in R.THRESHOLDS:
            assert min(offs) < thr <= max(offs), f"{op.name}: no checked row on both sides of {thr} floats"
        if case.kind == "A":
            assert op.checked is None                    # every row is compared
    for op in case.operands:
        assert op.strides[-1] == 1 and all(st % 4 == 0 for st in op.strides[:-1]), "16-byte rows"


@pytest.mark.parametrize("case", R.ALL_CASES, ids=[R.case_id(c) for c in R.ALL_CASES])
def test_row_counts_tiles_and_bytes(case):
    assert case.n > 2 * case.tile and case.n % case.tile, "two full tiles and a ragged one"
    assert R.case_bytes(case) <= R.CAP_BYTES
    if case.kind == "A":                                 # the fewest rows that do it
        ld = max(op.strides[0] for op in case.operands if op.far)
        assert case.n == R.stride_rows(ld, case.tile)
        assert (case.n - 4) * ld >= R.T31 > (case.n - 6) * ld or case.n == 2 * case.tile + 1
    elif case.kind == "B":
        for op in case.operands:
            if op.far:
                chk = set(op.checked)
                assert set(range(128)) <= chk and set(range(case.n - 128 - case.n % case.tile, case.n)) <= chk
                for c in R.crossing_nodes(op):           # the 256 centred on each crossing, in the operand's own layout
                    assert {i for i in range(c - 128, c + 128) if 0 <= i < case.n} <= chk, (op.name, c)


def test_strides_are_the_last_each_guard_admits():
    lds = {(c.entry, c.engine, c.route, op.name): op.strides[0] for c in R.STRIDE_CASES for op in c.operands if op.far}
    for d in (32, 64):
        assert any(c.route == "F16x2" and c.d == d and c.operands[1].strides[0] == R.LD_H_F16X2 - 4 for c in R.LSTM_A)
        assert any(c.route == "F32Mfma" and c.d == d and c.operands[0].strides[0] == R.LD_MFMA - 4 for c in R.LSTM_A)
        assert any(c.route == "F32Mfma" and c.d == d and c.operands[1].strides[0] == R.LD_MFMA - 4 for c in R.LSTM_A)
    assert any(c.engine == "f16x2" and c.route == "F32Mfma" and c.operands[1].strides[0] == R.LD_H_F16X2 for c in R.LSTM_A)
    assert {c.route for c in R.LSTM_A} == {"F16x2", "F32Mfma", "Split128", "Valu"}
    for c in R.BPTT_A:
        assert lds[c.entry, c.engine, c.route, "x"] == lds[c.entry, c.engine, c.route, "dh_ext"] == R.LD_BPTT - 4
    assert {c.route for c in R.BPTT_A} == {"OneLaunch", "SplitDw"}
    for c in R.GRU_A:
        assert max(op.strides[0] for op in c.operands) == R.LD_GRU - 4
    for c in R.ATTN_A + R.FRONT_A + R.DENSE_A + R.ROWS:
        if c.entry != "interval_fusion":                 # its x is bound by the LSTM in front of the attention
            assert all(op.strides[0] == R.LD_FREE for op in c.operands if op.far)
    assert {c.route for c in R.ATTN_A} == {"Split", "F32Mfma", "Wide", "Valu"}
    assert {c.route for c in R.FRONT_A} == {"Split", "F32Mfma"}


def test_route_labels_agree_with_the_library_queries(lib):
    for c in R.ALL_CASES:
        assert lib.sagnn_set_engine(ENGINE_CODE[c.engine]) == 0
        if c.entry in ("ln_mhsa_mean", "interval_fusion"):
            assert R.attn_route(c.engine, c.d, c.t, c.heads) == c.route
            assert lib.sagnn_ln_mhsa_mean_workspace_bytes(c.n, c.t, c.d, c.heads) == R.attn_workspace_bytes(c.route, c.n, c.t, c.d), c
        elif c.entry == "attn_bwd_front":
            assert R.front_route(c.engine, c.d, c.t, c.heads) == c.route
            assert lib.sagnn_attn_bwd_front_supported(c.d, c.t, c.heads) == 1
        elif c.entry == "lstm_bwd_ws":
            assert R.bptt_route(c.engine, c.d, c.route == "SplitDw") == c.route and lib.sagnn_lstm_bwd_supported(c.d) == 1
        elif c.entry == "gru_fwd":
            assert lib.sagnn_gru_fused_supported(c.d) == 1 and lib.sagnn_gru_workspace_bytes(c.n, c.t, c.d) == 0
        elif c.entry == "attn_bwd_tail":
            assert R.tail_route(c.engine, c.d) == c.route and lib.sagnn_attn_bwd_tail_supported(c.d) == 1
    # the LSTM forward has no query: test_lstm_forward_limits below sees where the selection sends a stride through the
    # refusal each kernel words differently, and tests/test_host.py pins the selection table itself


def test_dense_labels_agree_with_the_restated_dense_selection():
    """The labels of the dense cases against nn_route / tn_route / seg_route of tests/test_gpu_dense_routes.py, which restate
    dense.hip and dense_gemm.hip line by line, at the CU counts those tests use."""
    import test_gpu_dense_routes as D
    for cus in (80, 256, 304):
        for c in R.DENSE_A + R.DENSE_B:
            din, dout = c.d, c.heads
            if c.entry == "dense_nn":
                assert c.route == "Resident" and D.nn_route(c.n, din, dout, cus) == ("resident", dout // 32)
            elif c.entry == "dense_tn":
                assert c.route == "Tn" and D.tn_route(c.n, din, dout, cus)[0] == "tn"
            else:
                assert c.route == "GemmTn" and D.seg_route(c.n, c.t, din, dout, cus)[:3] == ("gemm_tn", 1, 2)
        s = R.SEG_LIMIT
        assert D.seg_route(s["seg_rows"], s["n_seg"], s["din"], s["dout"], cus)[:3] == ("gemm_tn", 1, 1)


def lstm_fwd(lib, p, ld_n, ld_h, d=64, t=2):
    return lib.sagnn_lstm_fwd_f32(p, ld_n, d, 4, t, d, p, p, 1.0, None, p, ld_h, None)


def test_lstm_forward_limits(lib, p):
    """F32Mfma refuses ld_n = 2^24 and ld_h = 2^24 under both matrix engines, naming the limit; under f16x2 the message is
    the MFMA kernel's, which shows where the selection sends an ld_h of 2^22 and above. One step below, the checks pass
    and the call goes on to the device, which this test does not do."""
    for engine in ("f32", "f16x2"):
        assert lib.sagnn_set_engine(ENGINE_CODE[engine]) == 0
        for ld_n, ld_h in ((128, R.LD_MFMA), (R.LD_MFMA, R.LD_MFMA) if engine == "f32" else (128, R.LD_MFMA + 4)):
            assert lstm_fwd(lib, p, ld_n, ld_h) == ERR_ARG
            assert "MFMA LSTM" in _lib.last_error() and "2^24" in _lib.last_error()
    assert lib.sagnn_set_engine(ENGINE_CODE["f32"]) == 0
    assert lstm_fwd(lib, p, R.LD_MFMA, 128) == ERR_ARG and "2^24" in _lib.last_error()


def test_gru_limits(lib, p):
    for ld_n, ld_h in ((128, R.LD_GRU), (R.LD_GRU, 128)):
        assert lib.sagnn_gru_fwd_f32(p, ld_n, 64, 4, 2, 64, p, p, p, p, None, p, ld_h, None, None, None, 0, None) == ERR_ARG
        assert "GRU" in _lib.last_error() and "2^24" in _lib.last_error()


def test_bptt_limits(lib, p):
    for ws in (None, p):
        for ld_n, ld_dhe in ((R.LD_BPTT, 128), (128, R.LD_BPTT)):
            rc = lib.sagnn_lstm_bwd_ws_f32(p, ld_n, 64, p, p, p, p, ld_dhe, None, p, p, p, p, 4, 2, 64, ws, 4 * 2 * 4 * 64 * 4 if ws else 0,
                                           None)
            assert rc == ERR_ARG and "lstm_bwd" in _lib.last_error() and "2^25" in _lib.last_error()


# ---- two mutations, by arithmetic --------------------------------------------------------------------------------------------
# Neither mutant is run on a device: the wrapped address of each lies in front of the pointer the entry was given, outside
# any buffer of the test.

def test_a_32_bit_row0_in_the_f16_lstm_kernel_lands_on_checked_rows():
    """lstm_fwd_f16_kernel with `const int row0`: row0 * ld_h and (row0 + r) * ld_n still widen through the int64 stride,
    but drop + row0 * t * D (lstm_f16_kernel.h:187) is then a 32-bit product. In the kind B F16x2 cases the mask is
    [n, t, d] past 2^31 floats: the product wraps for every tile that starts at or past float 2^31, and every node of those
    tiles is among the checked last 128. Whether the compiler keeps that product in 32 bits was not read off the mutant's
    code (a signed product that feeds a pointer may legally be widened): the catch is a supposition to that extent."""
    for c in (c for c in R.TRAIN_B if c.route == "F16x2"):       # a second catcher: gates_out + row0 * t * NC (:183), NC = 4 D
        per_row = c.t * 4 * c.d
        starts = [tile * c.tile for tile in range(-(-c.n // c.tile)) if R.wrap_i32(tile * c.tile * per_row) != tile * c.tile * per_row]
        gates = next(op for op in c.operands if op.name == "gates")
        assert starts and all(R.wrap_i32(r * per_row) < 0 for r in starts) and set(range(starts[0], c.n)) <= set(gates.checked)
    for c in (c for c in R.LSTM_B if c.route == "F16x2"):
        drop = next(op for op in c.operands if op.name == "drop")
        wrapped = [tile * c.tile for tile in range(-(-c.n // c.tile)) if R.wrap_i32(tile * c.tile * c.t * c.d) != tile * c.tile * c.t * c.d]
        assert wrapped and all(R.wrap_i32(r * c.t * c.d) < 0 for r in wrapped)        # in front of the mask: not run
        hit = [i for i in drop.checked if i >= wrapped[0]]
        assert len(hit) == c.n - wrapped[0] > 0                                       # every node of the wrapped tiles is compared


def test_a_32_bit_gather_offset_in_the_spmm_lands_on_checked_rows():
    """spmm.hip:366 with (int)(c[u] * ldx): at ldx = 2^16 the product leaves 32 bits from source row 32768 on and turns
    negative; at the row strides the suite used before (a few hundred floats) it never does. The far SpMM case gathers
    such rows into most of its output rows, and the far rows_gather case moves rows of the same kind."""
    case, = R.SPMM
    X = case.operands[0]
    ldx = X.strides[0]
    bad = [c for c in X.checked if R.wrap_i32(c * ldx) != c * ldx]
    assert bad and min(bad) >= R.T31 // ldx and all(R.wrap_i32(c * ldx) < 0 for c in bad)   # in front of X: not run
    n_rows, _, rowptr, colidx = R.spmm_graph()
    hit = sum(1 for r in range(n_rows) if (colidx[rowptr[r]:rowptr[r + 1]] >= R.T31 // ldx).any())
    assert hit > n_rows // 2
    assert all(R.wrap_i32(r * 260) == r * 260 for r in (0, 131076))                         # the largest case before: no wrap
