"""GPU parity of the training-side operators, one kernel at a time: every entry of csrc/train_ops.hip plus
sagnn_pair_score_f32, sagnn_leaky_add_f32, sagnn_mul_f32 and sagnn_mask_scale_f32, called directly through the C ABI on
float32 inputs and compared with the float64 restatement of the same values (train_ops_ref.py).

Tolerances are derived, not measured. A sum of m addends that fp32 atomics (or a shuffle tree) add in arbitrary order,
each addend formed with at most three roundings, is within (m + 4) * 2^-24 * sum |addend| of the exact sum; m and the
magnitudes come from the restatement (R.bound). Element-wise results are compared bit for bit. Every test prints the
largest error / bound ratio it met as "RATIO <entry> <value>".

Inputs are row views of wider slabs (ld = 2 d on the user side, 3 d on the item side; the rest of the slab is NaN, so
a wrong stride or column cannot go unnoticed) while the gradient outputs are dense, which is how the kernels address
them. Every id is valid and every size inside the documented limits: nothing here can fault."""
import numpy as np
import pytest
import torch

import train_ops_ref as R
from sa_gnn_amd import _lib, ops

pytestmark = pytest.mark.gpu

LEAKY = 0.5
PAIR_D = (4, 8, 16, 32, 64, 128, 256)


def _ppw(d):
    return 64 // (d // 4)                      # pairs per wavefront: d / 4 lanes per pair


def _pair_cases():
    cases = []
    for d in PAIR_D:
        for n in (1, _ppw(d) - 1, _ppw(d) + 1, 1000, 100003):
            if n > 0:                          # d = 256: ppw - 1 = 0 pairs, the case of the zero-pairs test below
                cases.append((d, n, "spread"))
        cases.append((d, 5000, "one_row"))
        cases.append((d, 1000, "untouched"))
    return cases


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _slab(vals, width, dev):
    """vals [rows, d] as columns [d, 2d) of a NaN-filled [rows, width * d] device slab: the view and its row stride."""
    rows, d = vals.shape
    slab = np.full((rows, width * d), np.nan, dtype=np.float32)
    slab[:, d:2 * d] = vals
    view = _dev(slab, dev)[:, d:2 * d]
    assert view.stride(0) == width * d and view.data_ptr() % 16 == 0
    return view, width * d


def _values(rng, rows, d, zeros=0.0):
    v = rng.standard_normal((rows, d)).astype(np.float32)
    if zeros:
        z = rng.random((rows, d))
        v[z < zeros] = 0.0
        v[z < zeros / 2] = -0.0
    return v


def _ids(rng, n, rows, pattern, hot):
    if pattern == "one_row":
        return np.full(n, hot, dtype=np.int32)
    if pattern == "untouched":
        return (3 * rng.integers(0, rows // 3, size=n)).astype(np.int32)      # two rows of three are never named
    return rng.integers(0, rows, size=n).astype(np.int32)


class PairCase:
    """Tables U [nu, d] (ld 2d), I / A [ni, d] (ld 3d), S [nl, d] (ld 2d) with exact zeros planted in S (and in U, which
    the SSL kernels read as X), ids and the upstream gradient g."""

    def __init__(self, dev, d, n, pattern):
        rng = np.random.default_rng(1000 * d + n)
        self.d, self.n, self.dev = d, n, dev
        self.nu, self.ni, self.nl = 1009, 2003, 509
        self.U, self.I = _values(rng, self.nu, d, zeros=0.1), _values(rng, self.ni, d)
        self.S, self.A = _values(rng, self.nl, d, zeros=0.15), _values(rng, self.ni, d)
        self.U[7, 0], self.S[3, 1] = 0.0, -0.0   # the rows every pair of "one_row" names hold a tie too
        m = max(n, 1)                          # n = 0 still hands the entries valid pointers
        self.uids = _ids(rng, m, self.nu, pattern, 7)
        self.iids = _ids(rng, m, self.ni, pattern, 11)
        self.locs = _ids(rng, m, self.nl, pattern, 3)
        self.g = rng.standard_normal(m).astype(np.float32)
        (self.Ud, self.ldu), (self.Id, self.ldi) = _slab(self.U, 2, dev), _slab(self.I, 3, dev)
        (self.Sd, self.lds), (self.Ad, self.lda) = _slab(self.S, 2, dev), _slab(self.A, 3, dev)
        self.ud, self.idd, self.ld, self.gd = (_dev(x, dev) for x in (self.uids, self.iids, self.locs, self.g))

    def zeros(self, rows, fill=0.0):
        return torch.full((rows, self.d), fill, dtype=torch.float32, device=self.dev)


_worst = {}


def _ratio(entry, err, b):
    """Records and returns the largest error / bound ratio; an element whose bound is 0 must be exact."""
    err, b = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert (err[b == 0] == 0).all(), f"{entry}: an element with no non-zero addend is not exactly 0"
    r = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    _worst[entry] = max(_worst.get(entry, 0.0), r)
    print(f"RATIO {entry} {r:.4f} (worst so far {_worst[entry]:.4f})")
    return r


def _check_sum(entry, got, want, extra=4):
    got = got.detach().double().cpu().numpy().reshape(np.shape(want.value))
    assert np.isfinite(got).all(), f"{entry}: non-finite output"
    assert (got[want.cnt == 0] == 0).all(), f"{entry}: a row no pair names is not exactly 0"
    r = _ratio(entry, np.abs(got - want.value), R.bound(want, extra))
    assert r <= 1.0, f"{entry}: error / bound = {r:.3f}"
    return got


def _check_rerun(entry, a, b, want):
    """Two runs of one accumulation differ by the order of the atomics only: inside the same bound, not bit-equal."""
    r = _ratio(entry + " (run to run)", np.abs(a.double().cpu().numpy() - b.double().cpu().numpy()), R.bound(want))
    assert r <= 1.0, f"{entry}: two runs differ by {r:.3f} bounds"


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_bits(got, want, what):
    want = np.ascontiguousarray(want, dtype=np.float32)
    bad = _bits(got).reshape(-1) != want.view(np.int32).reshape(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements differ in their bits, first at {np.flatnonzero(bad)[:5]}"


# ---- pair kernels ----------------------------------------------------------------------------------------------------

def _pair_bwd(lib, c, head, alias=False):
    dU, dI = c.zeros(c.nu), c.zeros(c.ni)
    dS = c.zeros(c.nl) if head else None
    dA = (dI if alias else c.zeros(c.ni)) if head else None
    A, lda = (c.Id, c.ldi) if alias else (c.Ad, c.lda)
    ops.check(lib.sagnn_pair_score_bwd_f32(
        c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.Sd.data_ptr() if head else None, c.lds if head else 0,
        A.data_ptr() if head else None, lda if head else 0, c.ud.data_ptr(), c.idd.data_ptr(),
        c.ld.data_ptr() if head else None, LEAKY, c.gd.data_ptr(), dU.data_ptr(), dI.data_ptr(), ops._ptr(dS),
        ops._ptr(dA), c.n, c.d, ops._stream()))
    out = {"dU": dU, "dI": dI}
    if head:
        out["dS"] = dS
        if not alias:
            out["dA"] = dA
    return out


@pytest.mark.parametrize("d,n,pattern", _pair_cases())
def test_train_ops_pair_score_forward(dev, d, n, pattern):
    """sagnn_pair_score_f32 against its own restatement, with and without the head term."""
    c = PairCase(dev, d, n, pattern)
    got = ops.pair_score(c.Ud, c.Id, c.ud, c.idd, S=c.Sd, A=c.Ad, locs=c.ld, leaky=LEAKY)
    _check_sum("pair_score", got, R.pair_score(c.U, c.I, c.S, c.A, c.uids, c.iids, c.locs, LEAKY))
    got = ops.pair_score(c.Ud, c.Id, c.ud, c.idd)
    _check_sum("pair_score", got, R.pair_score(c.U, c.I, None, None, c.uids, c.iids, None, LEAKY))


@pytest.mark.parametrize("d,n,pattern", _pair_cases())
def test_train_ops_pair_score_bwd(dev, d, n, pattern):
    """sagnn_pair_score_bwd_f32 in its three forms: with the head term, without it (S == NULL), and with the
    aliasing the host uses (A is I and dA is dI: both sums land in dI)."""
    lib = _lib.load()
    c = PairCase(dev, d, n, pattern)
    for form, head, alias in (("head", True, False), ("S == NULL", False, False), ("A is I", True, True)):
        got = _pair_bwd(lib, c, head, alias)
        want = R.pair_score_bwd(c.U, c.I, c.S if head else None, c.I if alias else c.A, c.uids,
                                c.iids, c.locs, LEAKY, c.g, alias_a=alias)
        assert set(got) == set(want)
        for k in got:
            _check_sum(f"pair_score_bwd {k}", got[k], want[k])
        if n >= 1000 and form == "head":
            again = _pair_bwd(lib, c, head, alias)
            for k in got:
                _check_rerun(f"pair_score_bwd {k}", got[k], again[k], want[k])
    if pattern == "untouched":
        assert (want["dU"].cnt[1::3] == 0).all() and (want["dU"].cnt[2::3] == 0).all()     # the case is what it says
    if pattern == "one_row":
        assert want["dU"].cnt[7, 0] == 5000 and want["dS"].cnt[3, 0] == 5000


def test_train_ops_pair_score_bwd_tie_slope_decides(dev):
    """Every S element is an exact zero (+0 or -0): dS is leaky * g * A everywhere, dA is 0 * g."""
    lib = _lib.load()
    c = PairCase(dev, 32, 300, "spread")
    c.S = np.where(np.arange(c.S.size).reshape(c.S.shape) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    c.Sd, c.lds = _slab(c.S, 2, dev)
    got = _pair_bwd(lib, c, True)
    want = R.pair_score_bwd(c.U, c.I, c.S, c.A, c.uids, c.iids, c.locs, LEAKY, c.g)
    assert np.abs(want["dS"].value).max() > 0.1 and (want["dA"].value == 0).all()
    for k in got:
        _check_sum(f"pair_score_bwd {k}", got[k], want[k])


@pytest.mark.parametrize("d,n,pattern", _pair_cases())
def test_train_ops_prod_leaky_sum(dev, d, n, pattern):
    """sagnn_prod_leaky_sum_f32 and its backward; X = the table with planted zeros, so some products are exactly 0."""
    lib = _lib.load()
    c = PairCase(dev, d, n, pattern)
    out = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_prod_leaky_sum_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.ud.data_ptr(), c.idd.data_ptr(),
                                           LEAKY, out.data_ptr(), n, d, ops._stream()))

    def bwd():
        dX, dY = c.zeros(c.nu), c.zeros(c.ni)
        ops.check(lib.sagnn_prod_leaky_sum_bwd_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.ud.data_ptr(),
                                                   c.idd.data_ptr(), LEAKY, c.gd.data_ptr(), dX.data_ptr(), dY.data_ptr(),
                                                   n, d, ops._stream()))
        return {"dX": dX, "dY": dY}
    got = bwd()
    assert (n * d < 1000 and pattern != "one_row") or ((c.U[c.uids] * c.I[c.iids]) == 0).any()  # the tie slope is in play
    _check_sum("prod_leaky_sum", out, R.prod_leaky_sum(c.U, c.I, c.uids, c.iids, LEAKY))
    want = R.prod_leaky_sum_bwd(c.U, c.I, c.uids, c.iids, LEAKY, c.g)
    for k in got:
        _check_sum(f"prod_leaky_sum_bwd {k}", got[k], want[k])
    if n >= 1000:
        again = bwd()
        for k in got:
            _check_rerun(f"prod_leaky_sum_bwd {k}", got[k], again[k], want[k])


@pytest.mark.parametrize("d", PAIR_D)
def test_train_ops_pair_entries_leave_outputs_alone_at_zero_pairs(dev, d):
    lib = _lib.load()
    c = PairCase(dev, d, 0, "spread")
    outs = [c.zeros(c.ni, 7.0) for _ in range(4)]
    one = torch.full((4,), 7.0, dtype=torch.float32, device=dev)
    p = [o.data_ptr() for o in outs]
    ops.check(lib.sagnn_pair_score_bwd_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.Sd.data_ptr(), c.lds,
                                           c.Ad.data_ptr(), c.lda, c.ud.data_ptr(), c.idd.data_ptr(), c.ld.data_ptr(), LEAKY,
                                           c.gd.data_ptr(), p[0], p[1], p[2], p[3], 0, d, ops._stream()))
    ops.check(lib.sagnn_prod_leaky_sum_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.ud.data_ptr(), c.idd.data_ptr(),
                                           LEAKY, one.data_ptr(), 0, d, ops._stream()))
    ops.check(lib.sagnn_prod_leaky_sum_bwd_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, c.ud.data_ptr(),
                                               c.idd.data_ptr(), LEAKY, c.gd.data_ptr(), p[0], p[1], 0, d, ops._stream()))
    ops.check(lib.sagnn_pair_score_f32(c.Ud.data_ptr(), c.ldu, c.Id.data_ptr(), c.ldi, None, 0, None, 0, c.ud.data_ptr(),
                                       c.idd.data_ptr(), None, LEAKY, one.data_ptr(), 0, d, ops._stream()))
    assert all(bool((o == 7.0).all()) for o in outs + [one])


# ---- meta-net features -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (4, 32, 48, 64, 256))
@pytest.mark.parametrize("n", (1, 257, 5000))
def test_train_ops_meta_features(dev, d, n):
    lib = _lib.load()
    rng = np.random.default_rng(d * 7 + n)
    nu = 50                                                       # far fewer users than rows: ids repeat
    F, V = _values(rng, nu, d, zeros=0.05), _values(rng, nu, d)
    uids = rng.integers(0, nu, size=n).astype(np.int32)
    dm = rng.standard_normal((n, 3 * d)).astype(np.float32)
    (Fd, ldf), (Vd, ldv) = _slab(F, 2, dev), _slab(V, 3, dev)
    ud, dmd = _dev(uids, dev), _dev(dm, dev)
    out = torch.empty((n, 3 * d), dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_meta_features_f32(Fd.data_ptr(), ldf, Vd.data_ptr(), ldv, ud.data_ptr(), out.data_ptr(), n, d,
                                          ops._stream()))
    _same_bits(out, R.meta_features(F, V, uids), "meta_features")
    dF = torch.zeros((nu, d), dtype=torch.float32, device=dev)
    dV = torch.zeros((nu, d), dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_meta_features_bwd_f32(Fd.data_ptr(), ldf, Vd.data_ptr(), ldv, ud.data_ptr(), dmd.data_ptr(),
                                              dF.data_ptr(), dV.data_ptr(), n, d, ops._stream()))
    want = R.meta_features_bwd(F, V, uids, dm)
    _check_sum("meta_features_bwd dF", dF, want["dF"])
    _check_sum("meta_features_bwd dV", dV, want["dV"])


# ---- element-wise entries: bit for bit ---------------------------------------------------------------------------------

COUNTS = (1, 3, 255, 257, 1000003)


def _elems(rng, count):
    x = rng.standard_normal(count).astype(np.float32)
    x[::5] = 0.0
    x[2::11] = -0.0
    return x


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("leaky", (0.5, 1.0))
def test_train_ops_leaky_both_modes(dev, count, leaky):
    """leaky = 1.0 makes leaky * x == x for EVERY x: the tie rule then gives slope `leaky` everywhere."""
    lib = _lib.load()
    rng = np.random.default_rng(count)
    a, g = _elems(rng, count), rng.standard_normal(count).astype(np.float32)
    ad, gd = _dev(a, dev), _dev(g, dev)
    out = torch.empty(count, dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_leaky_f32(ad.data_ptr(), None, out.data_ptr(), leaky, count, 0, ops._stream()))
    _same_bits(out, R.leaky_fwd(a, leaky), "leaky forward")
    ops.check(lib.sagnn_leaky_f32(ad.data_ptr(), gd.data_ptr(), out.data_ptr(), leaky, count, 1, ops._stream()))
    _same_bits(out, R.leaky_bwd(a, g, leaky), "leaky backward")
    if leaky == 0.5:
        zero = a == 0
        assert zero.any() and (out.cpu().numpy()[zero] == np.float32(0.5) * g[zero]).all()


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("leaky", (0.5, 1.0))
@pytest.mark.parametrize("with_b", (True, False))
def test_train_ops_leaky_add(dev, count, leaky, with_b):
    rng = np.random.default_rng(count + 1)
    a, b = _elems(rng, count), _elems(rng, count)[::-1].copy()
    got = ops.leaky_add(_dev(a, dev), _dev(b, dev) if with_b else None, leaky)
    _same_bits(got, R.leaky_add(a, b if with_b else None, leaky), "leaky_add")


@pytest.mark.parametrize("count", COUNTS)
def test_train_ops_mul(dev, count):
    rng = np.random.default_rng(count + 2)
    a, b = _elems(rng, count), rng.standard_normal(count).astype(np.float32)
    _same_bits(ops.mul(_dev(a, dev), _dev(b, dev)), R.mul(a, b), "mul")


@pytest.mark.parametrize("rows,d", [(1, 4), (3, 4), (255, 4), (257, 4), (1000003, 4), (1, 64), (3, 256), (255, 64), (257, 32),
                                    (4099, 256)])
def test_train_ops_mask_scale(dev, rows, d):
    """g and out as row views of wider slabs; every mask byte value occurs."""
    rng = np.random.default_rng(rows + d)
    g = _elems(rng, rows * d).reshape(rows, d)
    mask = rng.integers(0, 16, size=(rows, d // 4)).astype(np.uint8)
    gd, _ = _slab(g, 3, dev)
    out, _ = _slab(np.zeros((rows, d), dtype=np.float32), 2, dev)
    ops.mask_scale(gd, _dev(mask, dev), 0.5, out)
    _same_bits(out.contiguous(), R.mask_scale(g, mask, 0.5), "mask_scale")
    assert bool(torch.isnan(out._base[:, :d]).all()) and bool(torch.isnan(out._base[:, 2 * d:]).all())   # nothing else written


# ---- row-dot sigmoid -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (1, 31, 32, 48, 100))
@pytest.mark.parametrize("padded", (True, False))
@pytest.mark.parametrize("n", (1, 255, 257, 70001))
def test_train_ops_rowdot_sigmoid(dev, k, padded, n):
    """lda = k rounded up to 32 (what the host passes) and lda = k. Rows e % 50 == 1 / 2 have z = +100.25 / -99.75: w is
    exactly 1 / 0 there and nothing flows back."""
    lib = _lib.load()
    rng = np.random.default_rng(k * 1000 + n)
    lda = (k + 31) // 32 * 32 if padded else k
    A = np.full((n, lda), np.nan, dtype=np.float32)
    A[:, :k] = rng.standard_normal((n, k)).astype(np.float32)
    w3 = (rng.standard_normal(k) / np.sqrt(k)).astype(np.float32)
    w3[0] = 2.0
    b3 = np.array([0.25], dtype=np.float32)
    e = np.arange(n)
    hi, lo = e % 50 == 1, e % 50 == 2
    A[hi | lo, :k] = 0.0
    A[hi, 0], A[lo, 0] = 50.0, -50.0
    dw = rng.standard_normal(n).astype(np.float32)
    Ad, w3d, b3d, dwd = (_dev(x, dev) for x in (A, w3, b3, dw))
    w = torch.empty(n, dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_rowdot_sigmoid_f32(Ad.data_ptr(), lda, w3d.data_ptr(), b3d.data_ptr(), w.data_ptr(), n, k, ops._stream()))
    z, want_w = R.rowdot_sigmoid(A, w3, b3, k)
    got_w = w.double().cpu().numpy()
    assert np.isfinite(got_w).all()
    # |dw| <= 0.25 |dz| (the sigmoid's largest slope) + 4 * 2^-24 for expf and the division
    r = _ratio("rowdot_sigmoid", np.abs(got_w - want_w), 0.25 * R.bound(z) + 4 * R.U24)
    assert r <= 1.0, f"rowdot_sigmoid: error / bound = {r:.3f}"
    assert (got_w[hi] == 1.0).all() and (got_w[lo] == 0.0).all()

    dA = torch.full((n, lda), 9.0, dtype=torch.float32, device=dev)
    dw3 = torch.zeros(k, dtype=torch.float32, device=dev)
    db3 = torch.zeros(1, dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_rowdot_sigmoid_bwd_f32(Ad.data_ptr(), lda, w3d.data_ptr(), w.data_ptr(), dwd.data_ptr(), dA.data_ptr(),
                                               lda, dw3.data_ptr(), db3.data_ptr(), n, k, ops._stream()))
    want = R.rowdot_sigmoid_bwd(A, w3, w.cpu().numpy(), dw, k)          # the backward reads the fp32 w it is given
    assert bool((dA[:, k:] == 9.0).all()), "dA columns at or beyond k were written"
    got_dA = _check_sum("rowdot_sigmoid_bwd dA", dA[:, :k].contiguous(), want["dA"])
    assert (got_dA[hi | lo] == 0).all()
    _check_sum("rowdot_sigmoid_bwd dw3", dw3, want["dw3"])
    _check_sum("rowdot_sigmoid_bwd db3", db3, want["db3"])


# ---- hinge losses ----------------------------------------------------------------------------------------------------

def _hinge_case(n, weighted):
    """Rows e % 7 == 3 are built from dyadic values with h = 1 - S (pos - neg) exactly 0; every other row is moved
    until |h| >= 1e-3, so fp32 and float64 agree on which rows are active."""
    rng = np.random.default_rng(n + weighted)
    pos, neg = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    w = {}
    if weighted:
        w = dict(wp=rng.random(n).astype(np.float32), wn=rng.random(n).astype(np.float32),
                 sp=rng.standard_normal(n).astype(np.float32), sn=rng.standard_normal(n).astype(np.float32))
    tie = np.arange(n) % 7 == 3
    if weighted:                                   # S = 1 * 0.75 - 0.5 * 0.5 = 0.5, pos - neg = 2
        w["wp"][tie], w["sp"][tie], w["wn"][tie], w["sn"][tie] = 1.0, 0.75, 0.5, 0.5
        pos[tie], neg[tie] = 2.5, 0.5
    else:                                          # pos - neg = 1
        pos[tie], neg[tie] = 1.5, 0.5
    for _ in range(100):
        h = R.hinge(pos, neg, 1.0, **w)["h"]
        close = (np.abs(h) < 1e-3) & ~tie
        if not close.any():
            break
        pos[close] += np.float32(0.5)
    return pos, neg, w, tie


@pytest.mark.parametrize("n", (1, 63, 65, 100003))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("outputs", ("all", "no dpos/dneg", "no dwp/dwn", "loss only"))
def test_train_ops_hinge(dev, n, weighted, outputs):
    if not weighted and outputs == "no dwp/dwn":
        outputs = "all"                            # the plain form has no dwp / dwn: this IS its full form
    lib = _lib.load()
    scale, loss0 = 0.37, 3.25
    pos, neg, w, tie = _hinge_case(n, weighted)
    want = R.hinge(pos, neg, scale, **w)
    h = want["h"]
    assert (h[tie] == 0).all() and (np.abs(h[~tie]) >= 1e-3).all()          # no row is skipped: each is a tie or clear
    assert n < 7 or ((h > 0).any() and (h < 0).any())
    t = {k: _dev(v, dev) for k, v in dict(pos=pos, neg=neg, **w).items()}
    loss = torch.full((1,), loss0, dtype=torch.float32, device=dev)
    names = [k for k in ("dpos", "dneg", "dwp", "dwn") if (k in ("dpos", "dneg") and outputs in ("all", "no dwp/dwn")) or
             (k in ("dwp", "dwn") and weighted and outputs in ("all", "no dpos/dneg"))]
    g = {k: torch.full((n,), 9.0, dtype=torch.float32, device=dev) for k in names}
    ops.check(lib.sagnn_hinge_f32(t["pos"].data_ptr(), t["neg"].data_ptr(), ops._ptr(t.get("wp")), ops._ptr(t.get("wn")),
                                  ops._ptr(t.get("sp")), ops._ptr(t.get("sn")), scale, loss.data_ptr(), ops._ptr(g.get("dpos")),
                                  ops._ptr(g.get("dneg")), ops._ptr(g.get("dwp")), ops._ptr(g.get("dwn")), n, ops._stream()))
    # the loss accumulates into its starting value: one more addend
    total = R.Sum(want["loss"].value + loss0, want["loss"].mag + abs(loss0), want["loss"].cnt + 1)
    _check_sum("hinge loss", loss, total)
    for k in names:
        got = _check_sum(f"hinge {k}", g[k], want[k])
        assert (got[h <= 0] == 0).all(), f"{k}: an inactive row has a gradient"
