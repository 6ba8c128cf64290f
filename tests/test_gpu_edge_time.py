"""GPU suite of the time-aware messages of the interval SpMM (SpmmPlan(buckets=), ops.spmm_time, the time= arguments of
the stack entries, --edgeTime slot): every edge adds its own bucket's table row, exactly, for every row
class, lane-group width, table size and both weight forms; the training epilogue against float64; that a plan with
buckets runs what it ran on the entries without time; the stack, its adjoint and dTE against float64 autograd over the
dense terms of edge_time_ref, batched and per interval; the large-row-block instantiations; the Recommender.

The graph of parts 1-3 is 70 rows x 50 sources on the DEFAULT plan tuning (short <= 16 < medium <= 256 < long, chunks
of at most 256 edges): rows of degree 0, 1, 16, 17, 256, 257 (two chunks, the second ragged: 192 + 65) and 600 (three
chunks, 256 + 256 + 88), the last two through duplicated stored entries; the other rows have random degrees <= 40."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_time_ref as R
from test_gpu_edge_drop import TUNING, assert_sum_close

pytestmark = pytest.mark.gpu

N_ROWS, N_SRC = 70, 50
FIXED_DEG = [0, 1, 16, 17, 256, 257, 600]


def _graph(M, weighted, seed=0):
    """(rowptr, colidx, buckets uint16, weights or None) of the 70 x 50 graph; bucket ids cover [0, M) at random with the
    largest ids of the table (and, where M allows, ids >= 256 and >= 32768) present."""
    rng = np.random.default_rng(1000 + seed)
    deg = np.concatenate([FIXED_DEG, rng.integers(0, 41, N_ROWS - len(FIXED_DEG))])
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = rng.integers(0, N_SRC, rowptr[-1]).astype(np.int32)
    buckets = rng.integers(0, M, colidx.size).astype(np.int64)
    forced = [b for b in (M - 1, 256, 32768, 40000, M - 2) if 0 <= b < M]
    for j, b in enumerate(forced):                        # in the short, medium and both long rows
        for r in (2, 4, 5, 6):
            buckets[rowptr[r] + 3 * j + 1] = b
    w = np.exp2(rng.integers(-2, 3, colidx.size)).astype(np.float32) if weighted else None
    return rowptr, colidx, buckets.astype(np.uint16), w


def _row_sums(rowptr, colidx, buckets, w, x, te):
    """float64 s[r] = sum_e w[e] * (x[col[e]] + te[bucket[e]]) and the sum of the |terms|."""
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    wt = np.ones(colidx.size) if w is None else w.astype(np.float64)
    v = x.astype(np.float64)[colidx] + te.astype(np.float64)[buckets.astype(np.int64)]
    s, terms = np.zeros((rowptr.size - 1, x.shape[1])), np.zeros((rowptr.size - 1, x.shape[1]))
    np.add.at(s, rows, wt[:, None] * v)
    np.add.at(terms, rows, np.abs(wt[:, None] * v))
    return s, terms


def _check_classes(plan):
    deg = np.diff(plan._rowptr_host)
    assert list(deg[:7]) == FIXED_DEG and plan.info.n_long_rows == 2
    rows, e0, e1 = plan.chunks()
    assert list(e1 - e0) == [192, 65, 256, 256, 88]


# ---- 1. every edge adds its own table row, exactly ----------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", [1, 3, 300, 65535])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_each_edge_adds_its_own_bucket_row_exactly(dev, d, M, weighted):
    """X and TE hold small integers and the weights are powers of two in [1/4, 4]: every term is a multiple of 1/4 below
    2^12 and every sum stays below 2^22, so fp32 is exact in any order and the comparison is bit for bit. A truncated
    bucket id (ids >= 256) or a sign-extended one (ids >= 32768) reads another row of TE, which holds other integers."""
    from sa_gnn_amd import ops
    rowptr, colidx, buckets, w = _graph(M, weighted)
    if M > 256:
        assert (buckets >= 256).any()
    if M > 32768:
        assert (buckets >= 32768).any() and buckets.max() == M - 1
    rng = np.random.default_rng(d + M)
    x = rng.integers(-4, 5, (N_SRC, d)).astype(np.float32)
    te = rng.integers(-3, 4, (M, d)).astype(np.float32)
    te[np.arange(M) % 256 == 255] += 8.0                  # rows 256 apart differ: id & 255 cannot pass for id
    plan = ops.SpmmPlan(rowptr, colidx, N_ROWS, N_SRC, device=dev, weights=w, buckets=buckets, n_buckets=M)
    _check_classes(plan)
    s, _ = _row_sums(rowptr, colidx, buckets, w, x, te)
    want = s.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), s) and np.abs(s).max() < 2 ** 22
    got = ops.spmm_time(plan, torch.from_numpy(x).to(dev), 1.0, torch.from_numpy(te).to(dev), want_out=True)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # the time term is there: the product without it differs in every non-empty row (M = 1: by deg * TE[0])
    s0, _ = _row_sums(rowptr, colidx, buckets, w, x, np.zeros_like(te))
    assert (np.abs(s - s0).max(1)[np.diff(rowptr) > 0] > 0).all()


def test_large_row_block_variant_with_time(dev):
    """262,144 rows and a handful of edges: every launch takes the RPW = kRowsPerWave instantiation of its time kernel —
    one product unweighted and weighted, and one layer of the batched stack — on empty, short, medium and long rows,
    exactly (small integers as above)."""
    from sa_gnn_amd import ops
    U, I, d, M = 262144, 50, 32, 40000
    rng = np.random.default_rng(262144)
    deg = np.zeros(U, np.int64)
    deg[[5, 99999, 200000, U - 1]] = [3, 20, 300, 16]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = rng.integers(0, I, rowptr[-1]).astype(np.int32)
    buckets = rng.integers(0, M, colidx.size).astype(np.uint16)
    buckets[::7] = M - 1
    x = rng.integers(-4, 5, (I, d)).astype(np.float32)
    te = rng.integers(-3, 4, (M, d)).astype(np.float32)
    x_d, te_d = torch.from_numpy(x).to(dev), torch.from_numpy(te).to(dev)
    for w in (None, np.exp2(rng.integers(-2, 3, colidx.size)).astype(np.float32)):
        plan = ops.SpmmPlan(rowptr, colidx, U, I, device=dev, weights=w, buckets=buckets, n_buckets=M)
        assert plan.info.n_long_rows == 1 and plan.info.n_chunks == 2
        s, _ = _row_sums(rowptr, colidx, buckets, w, x, te)
        got = ops.spmm_time(plan, x_d, 1.0, te_d, want_out=True)
        np.testing.assert_array_equal(got.cpu().numpy(), s.astype(np.float32))
    # the batched kernel: the unweighted pair (the pattern and its exact transpose, buckets permuted alongside), one layer
    rows = np.repeat(np.arange(U), deg)
    order = np.argsort(colidx, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=I))]).astype(np.int32)
    pu = ops.SpmmPlan(rowptr, colidx, U, I, device=dev, buckets=buckets, n_buckets=M)
    pi = ops.SpmmPlan(rp_t, rows[order].astype(np.int32), I, U, device=dev, buckets=buckets[order], n_buckets=M)
    batch = ops.SpmmBatch([pu], [pi])
    u0 = rng.integers(-4, 5, (1, U, d)).astype(np.float32)
    te2 = rng.integers(-3, 4, (1, 1, 2, M, d)).astype(np.float32)
    ou, oi = torch.empty((1, U, d), device=dev), torch.empty((1, I, d), device=dev)
    ops.gnn_stack(batch, torch.from_numpy(u0).to(dev), x_d[None], 1, 0.5, ou, oi, time=torch.from_numpy(te2).to(dev))
    su, _ = _row_sums(rowptr, colidx, buckets, None, x, te2[0, 0, 0])
    si, _ = _row_sums(rp_t, rows[order], buckets[order], None, u0[0], te2[0, 0, 1])
    lk = lambda s: np.maximum(0.5 * s, s)
    np.testing.assert_array_equal(ou[0].cpu().numpy(), (2 * u0[0] + lk(su)).astype(np.float32))    # e^0 + e^1
    np.testing.assert_array_equal(oi[0].cpu().numpy(), (2 * x + lk(si)).astype(np.float32))


# ---- 2. the training epilogue vs float64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128])
def test_values_and_training_epilogue_vs_float64(dev, d):
    """Random data, sym-like weights in (0, 1], every operand of the training epilogue: residual, acc_in, acc_in2, the
    recorded mask, and out2 under a given mask. Tolerances: assert_sum_close, the rule test_gpu_adj_norm.py uses for the
    same quantities, with the |terms| of the sum including the table rows."""
    from sa_gnn_amd import ops
    M, leaky = 300, 0.5
    rowptr, colidx, buckets, _ = _graph(M, False, seed=d)
    rng = np.random.default_rng(170 + d)
    w = (1.0 / np.sqrt(rng.integers(1, 50, colidx.size) * rng.integers(1, 50, colidx.size))).astype(np.float32)
    plan = ops.SpmmPlan(rowptr, colidx, N_ROWS, N_SRC, device=dev, weights=w, buckets=buckets, n_buckets=M)
    x, te = rng.standard_normal((N_SRC, d)).astype(np.float32), rng.standard_normal((M, d)).astype(np.float32)
    res, acc, acc2 = (rng.standard_normal((N_ROWS, d)).astype(np.float32) for _ in range(3))
    bits_in = rng.integers(0, 16, (N_ROWS, d // 4)).astype(np.uint8)
    to = lambda a: torch.from_numpy(a).to(dev)
    out, acc_out, out2 = (torch.empty((N_ROWS, d), device=dev) for _ in range(3))
    m_out = torch.empty((N_ROWS, d // 4), dtype=torch.uint8, device=dev)
    ops.spmm_time(plan, to(x), leaky, to(te), residual=to(res), out=out, acc_in=to(acc), acc_in2=to(acc2), acc_out=acc_out,
                  mask_out=m_out, mask_in=to(bits_in), out2=out2, slope2=0.25)
    s, terms = _row_sums(rowptr, colidx, buckets, w, x, te)
    y = np.maximum(leaky * s, s) + res
    a = y + acc + acc2
    t_a = terms + np.abs(res) + np.abs(acc) + np.abs(acc2)
    assert_sum_close(out.cpu().numpy(), y, terms + np.abs(res))
    assert_sum_close(acc_out.cpu().numpy(), a, t_a)
    pos_in = ((bits_in[:, :, None] >> np.arange(4)) & 1).reshape(N_ROWS, d).astype(bool)
    assert_sum_close(out2.cpu().numpy(), np.where(pos_in, a, 0.25 * a), t_a)
    got_pos = ((m_out.cpu().numpy()[:, :, None] >> np.arange(4)) & 1).reshape(N_ROWS, d).astype(bool)
    deg = np.diff(rowptr)
    sure = np.abs(s) > 1e-4 * np.abs(s) + 1e-5 + 2e-7 * terms                    # the sign of s is not in doubt
    left_out = (~sure[deg > 0]).mean()
    print(f"d = {d}: {100 * left_out:.3f} % of the mask bits of non-empty rows left out")
    assert left_out <= 0.01
    assert np.array_equal(got_pos[sure], (s > 0)[sure]) and not got_pos[deg == 0].any()


# ---- 3. off means off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_off_means_off_and_a_zero_table_is_the_base_product(dev, weighted):
    from sa_gnn_amd import _lib, ops
    M, d = 300, 64
    rowptr, colidx, buckets, w = _graph(M, weighted)
    timed = ops.SpmmPlan(rowptr, colidx, N_ROWS, N_SRC, device=dev, weights=w, buckets=buckets, n_buckets=M)
    plain = ops.SpmmPlan(rowptr, colidx, N_ROWS, N_SRC, device=dev, weights=w)
    assert plain.buckets is None and plain.n_buckets == 0 and timed.n_buckets == M
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((N_SRC, d)).astype(np.float32)).to(dev)
    res = torch.from_numpy(rng.standard_normal((N_ROWS, d)).astype(np.float32)).to(dev)
    base = ops.spmm_ex(plain, x, 0.5, residual=res, want_out=True)
    # a plan with buckets on the entries without time: the same kernels, the same bits
    assert torch.equal(ops.spmm_ex(timed, x, 0.5, residual=res, want_out=True), base)
    assert torch.equal(ops.spmm(timed, x, 0.5, residual=res), base)
    # a table of zeros: x + 0 is x, and the sums are taken in the same order
    zero = torch.zeros((M, d), device=dev)
    assert torch.equal(ops.spmm_time(timed, x, 0.5, zero, residual=res, want_out=True), base)
    te = torch.from_numpy(rng.standard_normal((M, d)).astype(np.float32)).to(dev)
    assert not torch.equal(ops.spmm_time(timed, x, 0.5, te, residual=res, want_out=True), base)
    # a time entry on a plan without buckets, with a drop, or with another table size: refused before any launch
    with pytest.raises(ValueError, match="buckets"):
        ops.spmm_time(plain, x, 0.5, te, want_out=True)
    lib, e, out = _lib.load(), _lib.SpmmEpilogue(), torch.empty((N_ROWS, d), device=dev)
    e.leaky, e.out, e.ldo = 1.0, out.data_ptr(), d
    t = _lib.EdgeTimeArgs()
    t.te, t.n_buckets = te.data_ptr(), M
    drop = ops.EdgeDrop(1, 1, 0.5).struct()
    ws = timed.workspace(d)
    call = lambda plan, dr, tm: lib.sagnn_spmm_time_f32(plan.handle, x.data_ptr(), d, d, ctypes.byref(e), dr, ctypes.byref(tm),
                                                        ws.data_ptr(), ws.numel() * 4, None)
    assert call(plain, None, t) == -5 and "buckets" in _lib.last_error()
    assert call(timed, ctypes.byref(drop), t) == -5 and "drop" in _lib.last_error()
    t.n_buckets = M - 1
    assert call(timed, None, t) == -5 and "n_buckets" in _lib.last_error()
    torch.cuda.synchronize()


def test_the_stack_entries_without_time_ignore_the_buckets(dev):
    from sa_gnn_amd import graph, ops
    mats, mi, M = _intervals(np.random.default_rng(5), 23, 19)
    T, d, L = len(mats), 32, 2
    rng = np.random.default_rng(6)
    u0 = torch.from_numpy(rng.standard_normal((T, 23, d)).astype(np.float32)).to(dev)
    i0 = torch.from_numpy(rng.standard_normal((T, 19, d)).astype(np.float32)).to(dev)
    outs = []
    for time in (None, (mi, 1, M)):
        pairs = [graph.interval_pair(m, dev, tuning=TUNING, time=time) for m in mats]
        batch = ops.SpmmBatch([a.plan for a, _ in pairs], [t.plan for _, t in pairs])
        assert batch.n_buckets == (0 if time is None else M)
        ou, oi = torch.empty_like(u0), torch.empty_like(i0)
        ops.gnn_stack(batch, u0, i0, L, 0.5, ou, oi)
        outs.append((ou, oi))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # a batch of plans without buckets on the time entry: refused
    pairs = [graph.interval_pair(m, dev, tuning=TUNING) for m in mats]
    batch = ops.SpmmBatch([a.plan for a, _ in pairs], [t.plan for _, t in pairs])
    te = torch.zeros((T, L, 2, 1, d), device=dev)
    with pytest.raises(ValueError, match="buckets"):
        ops.gnn_stack(batch, u0, i0, L, 0.5, torch.empty_like(u0), torch.empty_like(i0), time=te)
    # a batch whose plans do not all carry buckets has none
    timed = [graph.interval_pair(m, dev, tuning=TUNING, time=(mi, 1, M)) for m in mats]
    mixed = ops.SpmmBatch([timed[0][0].plan] + [a.plan for a, _ in pairs[1:]], [t.plan for _, t in pairs])
    assert mixed.n_buckets == 0
    with pytest.raises(ValueError, match="buckets"):
        ops.gnn_stack(mixed, u0, i0, L, 0.5, torch.empty_like(u0), torch.empty_like(i0), time=te)


# ---- 4. the stack, its adjoint and dTE ----------------------------------------------------------------------------------
T0 = 1_600_000_000


def _intervals(rng, U, I):
    """Three interval matrices whose stored values are Unix timestamps over about six days: a random one with a
    duplicated (user, item) whose copies lie in different buckets (the later one stored FIRST) and one row past the long
    threshold of TUNING; an empty one; a sparser random one. Returns (mats, mi, M) for slot = 1 day."""
    def random_mat(p):
        m = sp.coo_matrix(rng.random((U, I)) < p)
        t = T0 + rng.integers(0, 6 * R.DAY, m.nnz)
        return m.row, m.col, t
    r, c, t = random_mat(0.3)
    keep = r != 2
    r, c, t = r[keep], c[keep], t[keep]
    long_row = np.arange(I)                               # user 2: every item, and (2, 7) twice, the later stamp first
    r = np.concatenate([r, np.full(I + 1, 2)])
    c = np.concatenate([c, [7], long_row])
    t = np.concatenate([t, [T0 + 5 * R.DAY + 5000], T0 + (long_row % 3) * R.DAY + 11])
    m0 = sp.coo_matrix((t.astype(np.int64), (r, c)), shape=(U, I))
    r2, c2, t2 = random_mat(0.1)
    m2 = sp.coo_matrix((t2.astype(np.int64), (r2, c2)), shape=(U, I))
    mats = [_csr_keeping_duplicates(m0), sp.csr_matrix((U, I), dtype=np.int64), _csr_keeping_duplicates(m2)]
    mi, max_time = R.time_process([mats[0], mats[2]], 1)
    return mats, mi, max_time + 1


def _csr_keeping_duplicates(coo):
    """A CSR with the COO's stored entries as they are (scipy's conversion would sum duplicated entries)."""
    order = np.argsort(coo.row, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(coo.row, minlength=coo.shape[0]))])
    return sp.csr_matrix((coo.data[order], coo.col[order], rowptr), shape=coo.shape)


@pytest.mark.parametrize("norm", ["none", "sym"])
@pytest.mark.parametrize("L", [2, 3])
def test_stack_adjoint_and_dte_vs_float64_autograd(dev, L, norm):
    """Outputs, dU, dI at the tolerances of the stack tests of test_gpu_adj_norm.py; dTE is scaled like dU. Batched and
    per interval agree bit for bit, and so do two runs (no atomics anywhere)."""
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import graph, ops
    U, I, d, leaky = 37, 29, 64, 0.5
    rng = np.random.default_rng(40 + L)
    mats, mi, M = _intervals(rng, U, I)
    T = len(mats)
    assert M == 7 and mats[0].nnz == len(R.latest(mats[0])) + 1                   # six days + the spare row; one duplicate
    assert R.bucket(R.latest(mats[0])[(2, 7)], mi, 1) == 5 and R.bucket(T0 + R.DAY + 11, mi, 1) == 1   # the two copies
    pairs = [graph.interval_pair(m, dev, tuning=TUNING, norm=norm, time=(mi, 1, M)) for m in mats]
    plans_u, plans_i = [a.plan for a, _ in pairs], [t.plan for _, t in pairs]
    assert plans_u[0].info.n_long_rows >= 1 and plans_u[1].nnz == 1
    assert (plans_u[0].partner_adjoint is not None) == (norm == "none")          # the duplicate: exact adjoints
    terms = [R.dense_terms(m, mi, 1, M, norm) for m in mats]
    u0, gu = (rng.standard_normal((T, U, d)).astype(np.float32) for _ in range(2))
    i0, gi = (rng.standard_normal((T, I, d)).astype(np.float32) for _ in range(2))
    te = rng.standard_normal((T, L, 2, M, d)).astype(np.float32)
    gu_d, gi_d = torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev)

    def run(pu, pi):
        tu, ti, tt = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (u0, i0, te))
        ou, oi = ag.gnn_stack(tu, ti, pu, pi, L, leaky, TE=tt)
        ((ou * gu_d).sum() + (oi * gi_d).sum()).backward()
        return ou.detach(), oi.detach(), tu.grad, ti.grad, tt.grad

    got = run(ops.SpmmBatch(plans_u, plans_i), None)
    want = R.stack_reference(terms, u0, i0, te, gu, gi, L, leaky)
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got[1].cpu().numpy(), want[1], rtol=1e-4, atol=1e-4)
    scale = max(float(np.abs(want[2]).max()), 1.0)
    np.testing.assert_allclose(got[2].cpu().numpy(), want[2], rtol=1e-4, atol=2e-6 * scale * L * 50)
    np.testing.assert_allclose(got[3].cpu().numpy(), want[3], rtol=1e-4, atol=2e-6 * scale * L * 50)
    scale_t = max(float(np.abs(want[4]).max()), 1.0)
    np.testing.assert_allclose(got[4].cpu().numpy(), want[4], rtol=1e-4, atol=2e-6 * scale_t * L * 50)
    assert want[4][0].any() and want[4][1, :, :, 0].any() and not want[4][1, :, :, 1:].any()   # the empty interval: bucket 0 alone
    for a, b in zip(got, run(plans_u, plans_i)):                                  # per interval: bit for bit
        assert torch.equal(a, b)
    assert torch.equal(run(ops.SpmmBatch(plans_u, plans_i), None)[4], got[4])     # and run to run
    # not the stack without time: its outputs differ, its gradients into the embeddings come from the same chain
    tu, ti = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (u0, i0))
    ou, _ = ag.gnn_stack(tu, ti, plans_u, plans_i, L, leaky)
    assert not torch.equal(ou.detach(), got[0])


# ---- 5. the Recommender -------------------------------------------------------------------------------------------------
def _tiny_dataset(U, I):
    """[trnMat, subMat[2], timeMat] with UNIQUE (user, item) pairs per interval and chosen timestamps: interval k covers
    days [10 k, 10 k + 10) after T0, every user has at least one interaction, so --slot 5 gives buckets 0 .. 3."""
    rng = np.random.default_rng(77)
    subs = []
    for k in range(2):
        on = rng.random((U, I)) < 0.07
        on[np.arange(U), (np.arange(U) + k) % I] = True
        r, c = np.nonzero(on)
        t = T0 + k * 10 * R.DAY + rng.integers(0, 10 * R.DAY, r.size)
        t[0], t[-1] = T0 + k * 10 * R.DAY, T0 + (k + 1) * 10 * R.DAY - 1
        subs.append(sp.csr_matrix((t.astype(np.intc), (r, c)), shape=(U, I)))
    union = sp.csr_matrix(((subs[0] + subs[1]) > 0).astype(np.float64))
    return [union, subs, sp.csr_matrix(subs[0].maximum(subs[1]))]


def _time_setup(dev, monkeypatch, edge_time, **extra):
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    flags = dict(edgeTime=edge_time, slot=5.0, adjNorm="none", evaluator="host", sampler="host", edgeKeepRate=1.0,
                 seqAtt="sum", predLoss="hinge", fusion_rows="all", graphNum=2, gnn_layer=2, latdim=32, leaky=0.5, ssldim=32,
                 att_layer=1, batch=16, pos_length=12, testSize=20, test=True, sslNum=3, pred_num=2, keepRate=1.0,
                 ssl_reg=0.5, reg=1e-2)
    flags.update(extra)                                   # the caller's flags override the defaults
    for k, v in flags.items():
        monkeypatch.setattr(args, k, v)
    U, I = 70, 60
    rng = np.random.default_rng(31)
    tmt = _tiny_dataset(U, I)
    tst_int = [int(rng.integers(0, I)) if u % 2 else None for u in range(U)]
    handler = DataHandler.from_memory(tmt, synthetic.make_sequence(tmt), tst_int,
                                      {u + 1: list(rng.integers(1, I + 1, size=30)) for u in range(U)})
    rec = Recommender(dev, handler)
    rec.prepareModel()
    g = torch.Generator(device="cpu").manual_seed(9)
    with torch.no_grad():
        for k in ("uEmbed", "iEmbed", "posEmbed", "timeEmbed"):
            NNs.params[k].mul_(20)
        for w in rec.time_weights:
            w.copy_(0.3 * torch.randn(w.shape, generator=g))
    return rec, handler, NNs, args


def _batch(rec, handler, args):
    np.random.seed(3)
    batIds = np.random.permutation(args.user)[:args.batch]
    uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
    su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
    return {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si}


def test_recommender_under_edge_time_none_leaves_the_time_variables_without_gradient(dev, monkeypatch):
    rec, handler, NNs, args = _time_setup(dev, monkeypatch, "none")
    assert rec.maxTime == 1 and tuple(rec.timeEmbed.shape) == (2, 32) and rec.time_tables() is None
    assert all(a.plan.buckets is None for a in rec.subAdj + rec.subTpAdj)
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(_batch(rec, handler, args), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    assert rec.timeEmbed.grad is None and all(w.grad is None for w in rec.time_weights) and rec.uEmbed.grad is not None


def test_recommender_under_edge_time_slot(dev, monkeypatch, tmp_path):
    from oracle import selfgnn_oracle as O
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import parallel
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _time_setup(dev, monkeypatch, "slot")
    T, L, d, M = 2, 2, 32, 5
    mi, max_time = R.time_process(handler.subMat, 5)
    assert (handler.timeMin, handler.maxTime) == (mi, max_time) == (T0, 4) and tuple(rec.timeEmbed.shape) == (M, d)
    assert len(rec.time_weights) == 2 * T * L and all(a.plan.n_buckets == M for a in rec.subAdj + rec.subTpAdj)
    used = np.unique(np.concatenate([a.plan._buckets_host for a in rec.subAdj]))
    assert list(used) == [0, 1, 2, 3]                                            # a few buckets; row 4 is the spare one
    batch = _batch(rec, handler, args)
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    time_names = ["timeEmbed"] + [k for k, v in NNs.params.items() if any(v is w for w in rec.time_weights)]
    assert len(time_names) == 1 + 2 * T * L
    for name in time_names:
        g = NNs.params[name].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in NNs.params.items()}

    # float64 autograd over the oracle's objective, its GNN stack with the time term of edge_time_ref
    P, leaves = _oracle_params(rec, NNs)
    t64 = lambda v: v.detach().cpu().double().requires_grad_(True)
    for name in time_names:
        leaves[name] = t64(NNs.params[name])
    w64 = torch.stack([leaves[n] for n in time_names[1:]]).view(T, L, 2, d, d)
    te64 = torch.matmul(leaves["timeEmbed"], w64)
    terms = [[torch.from_numpy(x) for x in R.dense_terms(m, mi, 5, M, "none")] for m in handler.subMat]
    calls = []

    def time_interval(u0, i0, adj_idx, tp_idx, n_layers, leaky):
        k = len(calls)
        calls.append(k)
        ou, oi = R.stack([terms[k]], u0[None], i0[None], te64[k][None], n_layers, leaky)
        return ou[0], oi[0]

    monkeypatch.setattr(O, "torch_gnn_interval", time_interval)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, batch, {"T": T, "L": L, "leaky": 0.5, "heads": 16})
    (opre + args.ssl_reg * ossl).backward()
    assert calls == [0, 1]
    assert abs(float(pre.detach()) - float(opre.detach())) <= 1e-4 * max(abs(float(opre.detach())), 1.0)
    assert abs(float(ssl.detach()) - float(ossl.detach())) <= 1e-4 * max(abs(float(ossl.detach())), 1.0)
    for name in time_names + ["uEmbed", "iEmbed"]:     # the training-gradient tolerance of test_gpu_train.py
        a, b = grads[name].cpu().double().numpy(), leaves[name].grad.numpy()
        floor = max(5e-5 * np.abs(b).max(), 2e-5)
        bad = np.abs(a - b) > 2e-4 * np.abs(b) + floor
        assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"

    # forward() runs the stack the training step runs (keep rate 1): bit for bit, batched and per interval
    uv, iv = ag.gnn_stack(rec.uEmbed, rec.iEmbed, *rec._stack_plans(), L, 0.5, TE=rec.time_tables())
    uvt, ivt = rec.propagate_intervals()
    assert torch.equal(uvt.permute(1, 0, 2), uv.detach()) and torch.equal(ivt.permute(1, 0, 2), iv.detach())
    uvt, ivt = uvt.clone(), ivt.clone()
    u2, i2 = rec.propagate_intervals(intervals=[0, 1])
    assert torch.equal(u2, uvt) and torch.equal(i2, ivt)

    # the captured forward replays the same stack, tables included
    want = rec.forward()[0].clone()
    replay = rec.capture_forward()
    assert torch.equal(replay()[0], want)

    # one row of timeEmbed moves the scores; the spare row moves nothing
    rec.forward()
    score = lambda: rec.predict(batch["uids"], batch["iids"], batch["sequence"], batch["mask"], batch["uLocs_seq"]).clone()
    base = score()
    with torch.no_grad():
        rec.timeEmbed[M - 1] += 1.0
    rec.forward()
    assert torch.equal(score(), base)
    with torch.no_grad():
        rec.timeEmbed[2] += 1.0
    rec.forward()
    moved = score()
    assert not torch.equal(moved, base)
    items, _ = rec.recommend(np.arange(4), k=5)
    assert items.shape == (4, 5)
    np.random.seed(1)
    host = rec.testEpoch()
    monkeypatch.setattr(args, "evaluator", "device")
    np.random.seed(1)
    assert rec.testEpoch() == host
    monkeypatch.setattr(args, "evaluator", "host")

    # a checkpoint round trip reproduces the scores; another flag or another --slot is refused
    for k, v in dict(epoch=1, save_path="time_ckpt", load_model="time_ckpt").items():
        monkeypatch.setattr(args, k, v)
    rec.saveHistory(str(tmp_path))
    state = torch.load(str(tmp_path / "Models" / "time_ckpt"), weights_only=True)
    assert state["edgeTime"] == {"mode": "slot", "slot": 5.0, "mi": T0, "M": M}
    with torch.no_grad():
        for p in NNs.params.values():
            p.zero_()
    rec.loadModel(str(tmp_path))
    rec.forward()
    assert torch.equal(score(), moved)
    monkeypatch.setattr(args, "slot", 2.5)
    with pytest.raises(ValueError, match="edgeTime"):
        rec.loadModel(str(tmp_path))
    monkeypatch.setattr(args, "slot", 5.0)
    monkeypatch.setattr(args, "edgeTime", "none")
    with pytest.raises(ValueError, match="edgeTime"):
        rec.loadModel(str(tmp_path))
    monkeypatch.setattr(args, "edgeTime", "slot")
    with pytest.raises(ValueError, match="edgeTime"):
        parallel.make_sharding(args.graphNum, 1, 0)


@pytest.mark.parametrize("flags", [dict(adjNorm="sym", predLoss="softmax"), dict(fusion_rows="batch", sampler="device"),
                                   dict(seqAtt="full", sampler="device")], ids=lambda f: "+".join(f"{k}={v}" for k, v in f.items()))
def test_edge_time_slot_trains_with_the_other_opt_in_flags(dev, monkeypatch, flags):
    """Both samplers, both --fusion_rows modes, --adjNorm sym, --seqAtt full and --predLoss softmax: a training step
    reaches timeEmbed and all 2 T L weights with finite, non-zero gradients."""
    rec, handler, NNs, args = _time_setup(dev, monkeypatch, "slot", **flags)
    assert all(a.plan.weighted == (args.adjNorm == "sym") and a.plan.n_buckets == 5 for a in rec.subAdj + rec.subTpAdj)
    np.random.seed(3)
    torch.manual_seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    batch = rec.sample_batch_device(bat, 7, 0) if args.sampler == "device" else rec._host_train_batch(bat)
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(batch, keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    assert bool(torch.isfinite(pre.detach()).all())
    for w in [rec.timeEmbed] + rec.time_weights:
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0
