"""GPU parity: every route of the dense-product selection (csrc/dense.hip, csrc/dense_gemm.hip) against float64.

The ABI does not say which kernel ran. nn_route / tn_route below restate the selection from the C++ (source lines cited),
every case names the label it was written for and asserts it against the device's CU count, and one CPU test checks that
the case lists reach every label at 256 CUs: a list that has drifted from the code fails instead of testing another kernel.

Two kinds of input per case. "exact": operands, bias and the pre-filled accumulator are integers in [-4, 4] held in float32;
the kernels multiply and add in fp32 (v_mfma_f32_32x32x2_f32, float atomics), every partial sum is an integer below 2^24, so
the result is exact in any order and is compared with np.array_equal against an int64 product: one swapped fragment, dropped
row or doubled db fails it. "arith": standard normal operands, W scaled by 1 / sqrt(din), against float64 with the bounds of
tests/test_gpu_dense.py; the float32 numpy product must itself stay within a quarter of the bound (asserted on the CPU).

X, G and Y are strided views of NaN-filled buffers (row strides cols + 4 and cols + 36, offset 4 floats, 16-byte aligned as
the entries require); dW and db are contiguous, cut out of a buffer with a band of zeros one 32-row tile deep and then NaNs
on both sides (an add onto a NaN would not show). After every call: everything outside the views is as it was, the inputs
are unchanged, pre-filled values are included exactly once."""
import numpy as np
import pytest
import torch

from sa_gnn_amd import ops
from test_gpu_fusion_routes import Slab

gpu = pytest.mark.gpu

NN_RTOL, NN_ATOL = 1e-4, 1e-5                            # tests/test_gpu_dense.py::test_dense_nn
TN_RTOL, TN_MAG, TN_ATOL = 1e-4, 1e-6, 1e-5              # tests/test_gpu_dense.py::test_dense_tn_seg


def cdiv(a, b):
    return -(-a // b)


# ---- the selection, restated -----------------------------------------------------------------------------------------------

LDS_FLOATS_FOR_W = (160 * 1024 - 4 * 32 * 32 * 4) // 4   # dense.hip:360 kLdsFloatsForW = 36864


def nn_route(n, din, dout, cus):
    """sagnn_dense_nn_f32 -> dense_nn_any (dense.hip:368-385), nn_piece (dense.hip:334-346), gemm_nn (dense_gemm.hip:245-266)."""
    if din * dout > LDS_FLOATS_FOR_W:                    # dense.hip:372
        by = cdiv(dout, 128)                             # dense_gemm.hip:247
        small = cdiv(n, 128) * by < 4 * (2 * cus)        # dense_gemm.hip:248-251
        return ("gemm_nn", 1 if small else 2)            # dense_gemm.hip:255-263
    slices = []
    for c0 in range(0, dout, 256):                       # dense.hip:373
        cw = min(256, dout - c0)                         # dense.hip:374
        kmax = min(LDS_FLOATS_FOR_W // cw // 32 * 32, din)   # dense.hip:375-376
        assert kmax == din, "the k0 loop (dense.hip:377) would run a second round"
        slices.append((cw, cw // 32))                    # dense.hip:336-345: CT = cw / 32
    return ("resident", slices[0][1]) if len(slices) == 1 else ("sliced", slices)


def tn_deal(din, dout):
    """tn_piece (dense.hip:348-358): the tile count, TPW, and how many tiles each of the four waves owns
    (dense_tn_kernel: wave w holds tiles w * TPW .. w * TPW + TPW - 1 of those that exist)."""
    tiles = (din // 32) * (dout // 32)                   # dense.hip:350
    tpw = cdiv(tiles, 4)                                 # dense.hip:351
    TPW = next(v for v in (1, 2, 3, 4, 8) if tpw <= v)   # dense.hip:352-356
    return tiles, TPW, [max(0, min(TPW, tiles - w * TPW)) for w in range(4)]


def gemm_tn_plan(n, din, dout, cus):
    """gemm_tn (dense_gemm.hip:282-300): mt, nt, splits launched, k_per, and whether ceil(n / 128) capped the splits."""
    mt, nt = cdiv(din, 128), cdiv(dout, 128)             # dense_gemm.hip:287
    wanted = cdiv(2 * cus, mt * nt)                      # dense_gemm.hip:289
    splits = max(1, min(wanted, cdiv(n, 128)))           # dense_gemm.hip:290-292
    k_per = cdiv(cdiv(n, splits), 32) * 32               # dense_gemm.hip:293-294
    return mt, nt, cdiv(n, k_per), k_per, wanted > cdiv(n, 128)   # dense_gemm.hip:295


def tn_route(n, din, dout, cus):
    """sagnn_dense_tn_f32 -> dense_tn_any (dense.hip:388-401), tn_piece (dense.hip:348-358), gemm_tn."""
    if din > 128 or dout > 256:                          # dense.hip:390
        return ("gemm_tn",) + gemm_tn_plan(n, din, dout, cus)[:4]
    return ("tn", tn_deal(din, dout)[1])                 # one piece: the r0 / c0 loops of dense.hip:391-399 run once


def seg_route(seg_rows, n_seg, din, dout, cus):
    """sagnn_dense_tn_seg_f32 (dense.hip:427-436): gemm_tn at every size."""
    return ("gemm_tn",) + gemm_tn_plan(seg_rows * n_seg, din, dout, cus)[:4]


# ---- cases: (din, dout, n, the label the case is there for) ----------------------------------------------------------------
# n is a number, or the name of a row count that depends on the CU count:

def rows_of(n, din, dout, cus):
    if n == "2 tiles":                                   # dense_nn_kernel: CUs blocks, block 0 .. 4 walk a second 128-row tile
        return 128 * cus + 5
    if n == "tm2":                                       # gemm_nn: ceil(n / 128) * by >= 8 CUs, the last row tile holds one row
        return 128 * cdiv(8 * cus, cdiv(dout, 128)) + 1
    if n == "2 chunks":                                  # dense_tn_kernel: at most 2 CUs blocks, each walks >= 2 chunks of 32
        return 32 * 2 * cus * 2 + 7                      # rows; the last chunk has 7
    if n == "uncapped":                                  # gemm_tn: ceil(n / 128) is above the splits wanted
        return 4 * 32 * cdiv(2 * cus, cdiv(din, 128) * cdiv(dout, 128)) + 33
    return n


# nn, W resident in LDS, one launch. 288 x 128 and 192 x 192 are the 160 KiB cap (36864 floats); 1152 x 32 has 36 K-chunks.
# n = 129: three waves of the last tile have no rows.
NN_RESIDENT = [(din, dout, n, ("resident", ct))
               for din, dout, ct in [(32, 32, 1), (96, 64, 2), (64, 96, 3), (288, 128, 4), (64, 160, 5), (192, 192, 6),
                                     (160, 224, 7), (128, 256, 8), (1152, 32, 1)]
               for n in (1, 31, 33, 127, 129, "2 tiles")]
# nn, column slices: 256 + 32, 256 + 256, 256 + 128 at the cap (96 x 384 = 36864), 4 x 256 + 128
NN_SLICED = [(din, dout, n, ("sliced", sl))
             for din, dout, sl in [(32, 288, [(256, 8), (32, 1)]), (64, 512, [(256, 8), (256, 8)]),
                                   (96, 384, [(256, 8), (128, 4)]), (32, 1152, [(256, 8)] * 4 + [(128, 4)])]
             for n in (1, 129, 1000)]
# gemm_nn, 64-row tiles: just above the cap; by = 3 with a last column tile 64 wide; a column tile with the col >= N guard
# in both halves of a wave pair (160 = 128 + 32); a full one
GEMM_NN_1 = [(din, dout, n, ("gemm_nn", 1))
             for din, dout in [(320, 128), (128, 320), (256, 160), (512, 256)] for n in (1, 63, 65, 1000)]
# gemm_nn, 128-row tiles: by = 16, and by = 17 with a last column tile 32 wide
GEMM_NN_2 = [(32, 2048, "tm2", ("gemm_nn", 2)), (32, 2080, "tm2", ("gemm_nn", 2))]
NN_CASES = NN_RESIDENT + NN_SLICED + GEMM_NN_1 + GEMM_NN_2

# tn, one piece: 1 tile (three waves clamped); 3 tiles; 5 tiles at TPW 2 (2, 2, 1, 0); 8 at TPW 2; 9 at TPW 3 (3, 3, 3, 0);
# 16 at TPW 4; 14 at TPW 4 (4, 4, 4, 2); 18 at TPW 8 (8, 8, 2, 0); 20 at TPW 8 (8, 8, 4, 0); 32 at TPW 8 (96 KiB of LDS)
TN_CASES = [(din, dout, n, ("tn", tpw))
            for din, dout, tpw in [(32, 32, 1), (32, 96, 1), (32, 160, 2), (64, 128, 2), (96, 96, 3), (128, 128, 4),
                                   (64, 224, 4), (96, 192, 8), (128, 160, 8), (128, 256, 8)]
            for n in (1, 31, 32, 33, "2 chunks")]


def gemm_tn_label(din, dout, n, cus):
    """What a gemm_tn case is there for, worked out by hand: n = 1 is one split of one 32-row step; n = 129 is capped at
    ceil(129 / 128) = 2 splits of ceil(65 / 32) * 32 = 96 rows; "uncapped" is 128 S + 33 rows for S wanted splits, so
    k_per = 128 + ceil(33 / S) rounded up = 160 (S >= 2) and the last of the ceil(n / 160) splits is ragged."""
    mt, nt = cdiv(din, 128), cdiv(dout, 128)
    if n == 1:
        return ("gemm_tn", mt, nt, 1, 32)
    if n == 129:
        return ("gemm_tn", mt, nt, 2, 96)
    return ("gemm_tn", mt, nt, cdiv(rows_of(n, din, dout, cus), 160), 160)


# gemm_tn: mt = 2 with a second row tile 32 wide (db from the mt = 0 blocks only); nt = 3 with a last column tile 32 wide;
# 2 x 4 tiles; mt = 3
GEMM_TN_CASES = [(din, dout, n, gemm_tn_label) for din, dout in [(160, 32), (32, 288), (256, 512), (384, 128)]
                 for n in (1, 129, "uncapped")]

# dense_tn_seg: (seg_rows, n_seg) = every row its own segment; a 32-row step straddles segments (33, 77); a split boundary
# inside a segment (4099). x node-major seen as [t, n, d], or time-major.
SEG_CASES = [(din, dout, seg_rows, n_seg, layout)
             for din, dout in [(32, 32), (128, 512), (96, 384)]
             for seg_rows, n_seg in [(1, 257), (33, 7), (77, 3), (4099, 2)] for layout in ("node", "time")]


def label_of(case, cus):
    din, dout, n, label = case
    return label(din, dout, n, cus) if callable(label) else label


def test_the_case_lists_reach_every_route_at_256_cus():
    cus = 256
    nn = [nn_route(rows_of(n, din, dout, cus), din, dout, cus) for din, dout, n, _ in NN_CASES]
    for case, got in zip(NN_CASES, nn):
        assert got == label_of(case, cus), case
    assert {l[1] for l in nn if l[0] == "resident"} == set(range(1, 9))
    last = {l[1][-1][0] for l in nn if l[0] == "sliced"}
    assert 256 in last and last - {256}, "sliced: a full and a partial last slice"
    assert {l[1] for l in nn if l[0] == "gemm_nn"} == {1, 2}

    tn = [tn_route(rows_of(n, din, dout, cus), din, dout, cus) for din, dout, n, _ in TN_CASES + GEMM_TN_CASES]
    for case, got in zip(TN_CASES + GEMM_TN_CASES, tn):
        assert got == label_of(case, cus), case
    assert {l[1] for l in tn if l[0] == "tn"} == {1, 2, 3, 4, 8}
    deals = [tn_deal(din, dout) for din, dout, n, _ in TN_CASES if n == 1]
    for TPW in (2, 4, 8):                                # a ragged deal and a full one
        assert any(T == TPW and tiles != 4 * T for tiles, T, _ in deals), TPW
        assert any(T == TPW and tiles == 4 * T for tiles, T, _ in deals), TPW
    assert any(T == 2 and per == [2, 2, 1, 0] for _, T, per in deals)
    assert any(T == 8 and 0 < per[2] < 8 and per[3] == 0 for _, T, per in deals), "one wave a partial set, one none"
    plans = [gemm_tn_plan(rows_of(n, din, dout, cus), din, dout, cus) for din, dout, n, _ in GEMM_TN_CASES]
    assert {p[4] for p in plans} == {True, False}, "gemm_tn: capped and uncapped splits"
    assert any(not p[4] and rows_of(c[2], c[0], c[1], cus) % p[3] for p, c in zip(plans, GEMM_TN_CASES)), "a ragged last split"
    assert any(p[0] >= 2 for p in plans) and any(p[1] > 1 and c[1] % 128 for p, c in zip(plans, GEMM_TN_CASES))
    for din, dout, seg_rows, n_seg, _ in SEG_CASES:
        assert seg_route(seg_rows, n_seg, din, dout, cus)[0] == "gemm_tn"
    k_per = {gemm_tn_plan(4099 * 2, din, dout, cus)[3] for din, dout, s, _, _ in SEG_CASES if s == 4099}
    assert all(4099 % k for k in k_per), "a split boundary inside a segment"


# ---- harness ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


class Guarded:
    """`values` as a contiguous device tensor cut out of a larger buffer: on either side a band of zeros, then 64 NaNs.
    dW and db are only ever added to, and a stray add onto a NaN leaves a NaN: the bands are what shows one, the NaNs
    show a stray store."""

    def __init__(self, dev, values, band):
        self.shape, self.lo, self.size = values.shape, 64 + band, values.size
        host = np.zeros(2 * self.lo + values.size, dtype=np.float32)
        host[:64] = host[-64:] = np.nan
        host[self.lo:self.lo + values.size] = values.ravel()
        self.buf = torch.from_numpy(host).to(dev)
        self.view = self.buf[self.lo:self.lo + values.size].view(self.shape)

    def read(self):
        host = self.buf.cpu().numpy()
        assert np.isnan(host[:64]).all() and np.isnan(host[-64:]).all(), "a store into the guard"
        lo, hi = host[64:self.lo], host[self.lo + self.size:-64]
        assert not lo.any() and not hi.any(), f"an add outside the tensor: {np.count_nonzero(lo)} elements below, {np.count_nonzero(hi)} above"
        return host[self.lo:self.lo + self.size].reshape(self.shape).copy()


def operands(kind, rng, *shapes):
    """exact: integers in [-4, 4] as float32. arith: standard normal."""
    if kind == "exact":
        return [rng.integers(-4, 5, size=s).astype(np.float32) for s in shapes]
    return [rng.standard_normal(s, dtype=np.float32) for s in shapes]


def imatmul(a, b):
    """int64 product of two float32 matrices that hold integers."""
    return (torch.from_numpy(a).long() @ torch.from_numpy(b).long()).numpy()


def pads(n):
    """Row paddings of (X, G or Y): cols + 4 and cols + 36, which operand gets which alternates with n."""
    return (4, 36) if n % 2 else (36, 4)


def report(route, din, dout, n, what, got, ref32, want, bound):
    """The worst error of the kernel and of the float32 numpy reference as fractions of the bound, printed, then asserted:
    the reference within a quarter (the screen), the kernel within the whole."""
    f_ref = float((np.abs(ref32.astype(np.float64) - want) / bound).max())
    f_got = float((np.abs(got.astype(np.float64) - want) / bound).max())
    print(f"DENSE_ROUTE_ERR route={route!r} din={din} dout={dout} n={n} {what}: kernel {f_got:.4f} float32 {f_ref:.4f} of the bound")
    assert f_ref <= 0.25, f"{what}: the float32 reference itself is at {f_ref:.3f} of the bound"
    assert f_got <= 1.0, f"{what}: {f_got:.3f} of the bound (float32 reference: {f_ref:.3f})"


# ---- nn --------------------------------------------------------------------------------------------------------------------

def run_nn(dev, route, kind, n, din, dout, with_bias, accumulate, sample=None):
    rng = np.random.default_rng([11, kind == "exact", n, din, dout, with_bias, accumulate])
    x, W, b, y0 = operands(kind, rng, (n, din), (din, dout), (dout,), (n, dout))
    if kind == "exact":
        assert 16 * din + 8 < 2 ** 24                    # |x w| <= 16 over K = din terms, then the bias and the old Y
    else:
        W /= np.float32(din ** 0.5)
    px, py = pads(n)
    xs = Slab(dev, (n, din), (din + px, 1), 4, values=x)
    ys = Slab(dev, (n, dout), (dout + py, 1), 4, values=y0 if accumulate else None)   # NaN where every element must be stored
    Wd, bd = torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)
    ops.dense_nn(xs.view, Wd, bd if with_bias else None, out=ys.view, accumulate=accumulate)
    got = ys.read()
    np.testing.assert_array_equal(xs.read(), x)
    assert np.array_equal(Wd.cpu().numpy(), W) and np.array_equal(bd.cpu().numpy(), b)
    if kind == "exact":
        want = imatmul(x, W)
        if with_bias:
            want += b.astype(np.int64)
        if accumulate:
            want += y0.astype(np.int64)
        assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {want.size} elements differ"
        return
    sel = slice(None) if sample is None else sample
    want = x[sel].astype(np.float64) @ W.astype(np.float64)
    ref32 = x[sel] @ W
    if with_bias:
        want, ref32 = want + b.astype(np.float64), ref32 + b
    if accumulate:
        want, ref32 = want + y0[sel].astype(np.float64), ref32 + y0[sel]
    assert np.isfinite(got).all()
    report(route, din, dout, n, "Y", got[sel], ref32, want, NN_ATOL + NN_RTOL * np.abs(want))


def nn_ids(cases):
    return [f"{din}x{dout}-n={n}" for din, dout, n, _ in cases]


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", NN_RESIDENT, ids=nn_ids(NN_RESIDENT))
def test_nn_resident(dev, cus, case, kind):
    """exact: bias=None, accumulate=True onto a pre-filled out. arith: bias, accumulate=False."""
    din, dout, n, label = case
    n = rows_of(n, din, dout, cus)
    assert nn_route(n, din, dout, cus) == label
    run_nn(dev, label, kind, n, din, dout, with_bias=kind == "arith", accumulate=kind == "exact")


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", NN_SLICED, ids=nn_ids(NN_SLICED))
def test_nn_sliced(dev, cus, case, kind):
    """The c0 > 0 launches: bias + c0, Y + c0 and W + c0 at ldw = dout. With bias; exact accumulates as well."""
    din, dout, n, label = case
    assert nn_route(n, din, dout, cus) == label
    run_nn(dev, label[0], kind, n, din, dout, with_bias=True, accumulate=kind == "exact")


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", GEMM_NN_1, ids=nn_ids(GEMM_NN_1))
def test_gemm_nn_64_row_tiles(dev, cus, case, kind):
    din, dout, n, label = case
    assert nn_route(n, din, dout, cus) == label
    for with_bias in (False, True):
        for accumulate in (False, True):
            run_nn(dev, label, kind, n, din, dout, with_bias, accumulate)


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", GEMM_NN_2, ids=nn_ids(GEMM_NN_2))
def test_gemm_nn_128_row_tiles(dev, cus, case, kind):
    """gemm_nn_kernel<2>: enough block tiles to fill the chip eight times over, the last row tile with one row. exact on all
    of the output; arith against float64 on 512 sampled rows and the last 129 (the kernel runs on all of them)."""
    din, dout, n, label = case
    n = rows_of(n, din, dout, cus)
    assert nn_route(n, din, dout, cus)[1] == 2 and nn_route(n, din, dout, cus) == label
    assert nn_route(n - 1 - 128, din, dout, cus)[1] == 1     # and one row tile fewer would not get there
    sample = np.concatenate([np.sort(np.random.default_rng(n).choice(n - 129, 512, replace=False)), np.arange(n - 129, n)])
    run_nn(dev, label, kind, n, din, dout, with_bias=True, accumulate=kind == "exact", sample=sample)


# ---- tn --------------------------------------------------------------------------------------------------------------------

def check_tn(route, kind, din, dout, n, x2, g2, dW0, db0, dW, db, with_db):
    """dW and db (Guarded) after one call on the rows x2 [n, din], g2 [n, dout], pre-filled with dW0 / db0."""
    got_W, got_b = dW.read(), db.read()
    if kind == "exact":
        want = imatmul(np.ascontiguousarray(x2.T), g2) + dW0.astype(np.int64)
        assert np.array_equal(got_W, want), f"dW: {np.count_nonzero(got_W != want)} of {want.size} elements differ"
        want_b = db0.astype(np.int64) + (g2.astype(np.int64).sum(axis=0) if with_db else 0)
        assert np.array_equal(got_b, want_b), f"db: {np.count_nonzero(got_b != want_b)} of {dout} elements differ"
        return
    x64, g64 = x2.astype(np.float64), g2.astype(np.float64)
    want = x64.T @ g64 + dW0
    bound = TN_RTOL * np.abs(want) + TN_MAG * (np.abs(x64).T @ np.abs(g64)) + TN_ATOL
    report(route, din, dout, n, "dW", got_W, x2.T @ g2 + dW0, want, bound)
    if with_db:
        want_b = g64.sum(axis=0) + db0
        bound_b = TN_RTOL * np.abs(want_b) + TN_MAG * np.abs(g64).sum(axis=0) + TN_ATOL
        report(route, din, dout, n, "db", got_b, g2.sum(axis=0, dtype=np.float32) + db0, want_b, bound_b)
    else:
        assert np.array_equal(got_b, db0)


def tn_targets(dev, kind, rng, din, dout):
    dW0, db0 = operands(kind, rng, (din, dout), (dout,))
    band = 32 * dout                                     # one stray 32-row tile of dW lands in the band, not past the buffer
    return dW0, db0, Guarded(dev, dW0, band), Guarded(dev, db0, band)


def run_tn(dev, route, kind, n, din, dout):
    rng = np.random.default_rng([12, kind == "exact", n, din, dout])
    x, g = operands(kind, rng, (n, din), (n, dout))
    if kind == "exact":
        assert 16 * n + 4 < 2 ** 24                      # |x g| <= 16 over K = n terms, then the old dW; db: 4 n + 4
    px, pg = pads(n)
    xs = Slab(dev, (n, din), (din + px, 1), 4, values=x)
    gs = Slab(dev, (n, dout), (dout + pg, 1), 4, values=g)
    for with_db in (True, False):
        dW0, db0, dW, db = tn_targets(dev, kind, rng, din, dout)
        ops.dense_tn(xs.view, gs.view, dW.view, db.view if with_db else None)
        check_tn(route, kind, din, dout, n, x, g, dW0, db0, dW, db, with_db)
    np.testing.assert_array_equal(xs.read(), x)
    np.testing.assert_array_equal(gs.read(), g)


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", TN_CASES, ids=nn_ids(TN_CASES))
def test_tn_resident(dev, cus, case, kind):
    din, dout, n, label = case
    n = rows_of(n, din, dout, cus)
    assert tn_route(n, din, dout, cus) == label
    run_tn(dev, label, kind, n, din, dout)


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", GEMM_TN_CASES, ids=nn_ids(GEMM_TN_CASES))
def test_gemm_tn(dev, cus, case, kind):
    """db at mt >= 2 is in the exact kind: a row tile other than the first adding it doubles it."""
    din, dout, n, _ = case
    label = label_of(case, cus)
    n = rows_of(n, din, dout, cus)
    assert tn_route(n, din, dout, cus) == label
    run_tn(dev, label[:3], kind, n, din, dout)


@gpu
@pytest.mark.parametrize("kind", ["exact", "arith"])
@pytest.mark.parametrize("case", SEG_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}x{c[3]}-{c[4]}" for c in SEG_CASES])
def test_tn_seg(dev, cus, case, kind):
    """All t segments with db, then the shifted pairing x[:t-1] against g[1:] without."""
    din, dout, n, t, layout = case
    label = seg_route(n, t, din, dout, cus)
    assert label[:3] == ("gemm_tn", cdiv(din, 128), cdiv(dout, 128))
    rng = np.random.default_rng([13, kind == "exact", n, t, din, dout])
    x, g = operands(kind, rng, (t, n, din), (t, n, dout))
    if kind == "exact":
        assert 16 * n * t + 4 < 2 ** 24
    x_strides = (din, t * din + 4, 1) if layout == "node" else (n * (din + 4) + 8, din + 4, 1)
    xs = Slab(dev, (t, n, din), x_strides, 4, values=x)
    gs = Slab(dev, (t, n, dout), (n * (dout + 36) + 4, dout + 36, 1), 4, values=g)
    for (xv, gv, x2, g2, with_db) in [(xs.view, gs.view, x, g, True), (xs.view[:t - 1], gs.view[1:], x[:t - 1], g[1:], False)]:
        dW0, db0, dW, db = tn_targets(dev, kind, rng, din, dout)
        ops.dense_tn_seg(xv, gv, dW.view, db.view if with_db else None)
        check_tn(("gemm_tn", "seg") + label[1:3], kind, din, dout, len(x2) * n, x2.reshape(-1, din), g2.reshape(-1, dout),
                 dW0, db0, dW, db, with_db)
    np.testing.assert_array_equal(xs.read(), x)
    np.testing.assert_array_equal(gs.read(), g)
