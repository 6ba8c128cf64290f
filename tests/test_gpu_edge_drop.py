"""GPU suite of the edge dropout of the interval graphs: the mask the kernels apply, bit for bit against
the numpy restatement (edge_drop_ref), for every row class and lane-group width; the values and the training epilogue
against float64; the stack and its adjoint against torch float64 autograd over explicitly masked dense matrices; and the
Recommender's training loss with --edgeKeepRate. Graphs are tiny, with plan tuning (4, 16, 64) so that 40 rows hold
short, medium and chunked long rows; one test runs 262,144 rows, the smallest count that takes the large-row-block
instantiations of the kernels."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_drop_ref as R
from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu

TUNING = (4, 16, 64)
SEED, STEP = 0x1234_5678_9ABC_DEF, 5
N_ROWS = 40


def assert_sum_close(got, want, abs_terms):
    """The rule of test_gpu_spmm.py: 1e-4 |want| + 1e-5 + 3 eps32 sum|terms| (eps32 = 2^-24)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = 1e-4 * np.abs(want) + 1e-5 + 2e-7 * np.asarray(abs_terms, np.float64)
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} outside tolerance; worst {np.abs(got - want)[bad].max():.3e}"


def _graph(n_src, keep_fn):
    """Edge list (rows = users, 40 of them; columns = items) as CSR arrays with duplicates kept: row 0 has no edge,
    row 1 three edges that keep_fn drops, row 2 a duplicated entry, row 3 every item plus 20 or more duplicated entries
    (more than one chunk of 64), the others degrees 1 .. 40 (short <= 4 < medium <= 16 < long)."""
    rng = np.random.default_rng(n_src)
    rows = [[] for _ in range(N_ROWS)]
    dropped = [c for c in range(n_src) if not keep_fn(1, c)][:3]
    assert len(dropped) == 3
    rows[1] = dropped
    rows[2] = [3, 7, 7, n_src - 1]
    rows[3] = sorted(list(range(n_src)) + list(rng.choice(n_src, max(20, 72 - n_src), replace=n_src < 64)))
    degs = [1, 2, 3, 4, 5, 6, 9, 12, 16, 17, 20, 25, 31, 32] + list(rng.integers(1, min(n_src, 40), N_ROWS - 18))
    for r, dg in zip(range(4, N_ROWS), degs):
        rows[r] = sorted(rng.choice(n_src, int(dg), replace=False).tolist())
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32)
    colidx = np.array([c for x in rows for c in x], dtype=np.int32)
    count = np.zeros((N_ROWS, n_src), np.int64)
    for r, x in enumerate(rows):
        for c in x:
            count[r, c] += 1
    return rowptr, colidx, count


def _transpose_csr(count):
    """CSR arrays of count^T with multiplicities (the exact transpose)."""
    ct = count.T
    rowptr = np.concatenate([[0], np.cumsum(ct.sum(1))]).astype(np.int32)
    colidx = np.array([c for r in range(ct.shape[0]) for c in range(ct.shape[1]) for _ in range(ct[r, c])], np.int32)
    return rowptr, colidx


def _plans(dev, n_src, keep_fn):
    from sa_gnn_amd import ops
    rowptr, colidx, count = _graph(n_src, keep_fn)
    plan = ops.SpmmPlan(rowptr, colidx, N_ROWS, n_src, device=dev, tuning=TUNING)
    rp_t, ci_t = _transpose_csr(count)
    plan_t = ops.SpmmPlan(rp_t, ci_t, n_src, N_ROWS, device=dev, tuning=TUNING)
    assert plan.info.n_long_rows >= 5 and plan.info.n_chunks > plan.info.n_long_rows      # a row of several chunks
    deg = np.diff(rowptr)
    assert (deg == 0).any() and ((deg > 0) & (deg <= 4)).any() and ((deg > 4) & (deg <= 16)).any()
    return plan, plan_t, count, deg


@pytest.mark.parametrize("d", [64, 32, 128])
def test_mask_is_the_reference_mask_exactly(dev, d):
    from sa_gnn_amd import ops
    k, l, direction = 2, 1, 0
    tag = ops.edge_tag(k, l, direction)
    n_src = d
    mask = R.dense_mask(SEED, STEP, k, l, direction, N_ROWS, n_src, keep=0.5)
    plan, plan_t, count, deg = _plans(dev, n_src, lambda u, i: mask[u, i])
    drop = ops.EdgeDrop(SEED, STEP, 0.5)
    assert drop.scale == 2.0
    out = ops.spmm_drop(plan, torch.eye(n_src, d, device=dev), 0.5, drop, tag, True, want_out=True)
    want = (2 * count * mask).astype(np.float32)
    got = out.cpu().numpy()
    for name, rows in (("empty", deg == 0), ("short", (deg > 0) & (deg <= 4)), ("medium", (deg > 4) & (deg <= 16)),
                       ("long", deg > 16)):
        assert rows.any() and np.array_equal(got[rows], want[rows]), name
    assert not got[1].any() and count[1].sum() == 3            # the row whose every edge is dropped
    assert want[2, 7] in (0.0, 4.0)                             # the duplicated entry: both copies or neither
    # the transposed plan, rows = items, the same tag: the exact transpose of the mask
    out_t = ops.spmm_drop(plan_t, torch.eye(N_ROWS, d, device=dev), 0.5, drop, tag, False, want_out=True)
    w = min(N_ROWS, d)                                          # the identity shows the first d users
    assert np.array_equal(out_t.cpu().numpy()[:, :w], want.T[:, :w]) and not out_t.cpu().numpy()[:, w:].any()
    # another tag, another step: other masks
    for other in (ops.spmm_drop(plan, torch.eye(n_src, d, device=dev), 0.5, drop, tag ^ 1, True, want_out=True),
                  ops.spmm_drop(plan, torch.eye(n_src, d, device=dev), 0.5, ops.EdgeDrop(SEED, STEP + 1, 0.5), tag, True,
                                want_out=True)):
        assert not torch.equal(other, out)


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_values_and_training_epilogue_vs_float64(dev, d, keep):
    from sa_gnn_amd import ops
    k, l, direction, n_src, leaky = 1, 0, 1, 64, 0.5
    tag = ops.edge_tag(k, l, direction)
    # direction 1 = the item-side product: the plan's rows are ITEMS, its columns users
    mask = R.dense_mask(SEED, STEP, k, l, direction, n_src, N_ROWS, keep=keep).T          # [rows = items, cols = users]
    plan, _, count, deg = _plans(dev, n_src, lambda r, c: mask[r, c])
    rng = np.random.default_rng(d + int(keep * 10))
    x, res, acc = (rng.standard_normal(s).astype(np.float32) for s in ((n_src, d), (N_ROWS, d), (N_ROWS, d)))
    drop = ops.EdgeDrop(SEED, STEP, keep)
    out, acc_out = torch.empty((N_ROWS, d), device=dev), torch.empty((N_ROWS, d), device=dev)
    m_out = torch.empty((N_ROWS, d // 4), dtype=torch.uint8, device=dev)
    ops.spmm_drop(plan, torch.from_numpy(x).to(dev), leaky, drop, tag, False, residual=torch.from_numpy(res).to(dev),
                  out=out, acc_in=torch.from_numpy(acc).to(dev), acc_out=acc_out, mask_out=m_out)
    a = (count * mask).astype(np.float64)
    scale = float(np.float32(drop.scale))
    s = scale * (a @ x.astype(np.float64))
    terms = scale * (a @ np.abs(x).astype(np.float64))
    y = np.maximum(leaky * s, s) + res
    assert_sum_close(out.cpu().numpy(), y, terms + np.abs(res))
    assert_sum_close(acc_out.cpu().numpy(), y + acc, terms + np.abs(res) + np.abs(acc))
    bits = m_out.cpu().numpy()
    got_pos = ((bits[:, :, None] >> np.arange(4)) & 1).reshape(N_ROWS, d).astype(bool)
    sure = np.abs(s) > 1e-4 * np.abs(s) + 1e-5 + 2e-7 * terms                            # the sign of s is not in doubt
    assert np.array_equal(got_pos[sure], (s > 0)[sure]) and not got_pos[deg == 0].any()


def test_off_means_off_and_all_kept_is_the_undropped_product(dev):
    from sa_gnn_amd import ops
    n_src, d = 64, 64
    full = (1 << 32) - 1
    assert R.dense_mask(SEED, STEP, 0, 0, 0, N_ROWS, n_src, thresh=full).all()             # every test edge is kept
    plan, _, count, deg = _plans(dev, n_src, lambda u, i: (u + i) % 2 == 0)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((n_src, d)).astype(np.float32)).to(dev)
    res = torch.from_numpy(rng.standard_normal((N_ROWS, d)).astype(np.float32)).to(dev)
    base = ops.spmm_ex(plan, x, 0.5, residual=res, want_out=True)
    assert torch.equal(ops.spmm_ex(plan, x, 0.5, residual=res, want_out=True, _drop=None), base)
    kept = ops.spmm_drop(plan, x, 0.5, ops.EdgeDrop.raw(SEED, STEP, full, 1.0), 0, True, residual=res, want_out=True)
    short = deg <= 4
    assert torch.equal(kept[torch.from_numpy(short).to(dev)], base[torch.from_numpy(short).to(dev)])
    terms = count.astype(np.float64) @ np.abs(x.cpu().numpy()).astype(np.float64) + np.abs(res.cpu().numpy())
    assert_sum_close(kept.cpu().numpy(), base.cpu().numpy(), terms)


# ---- the stack and its adjoint ----------------------------------------------------------------------------------------
def _intervals(rng, U, I):
    """T = 3 interval matrices: a dense-ish one with a duplicated stored entry and a long row, an empty one, a sparse one."""
    a = (rng.random((U, I)) < 0.3)
    a[4, :] = True                                         # a long user row (29 > 16)
    a[9, :] = False                                        # an isolated user
    a = sp.csr_matrix(a.astype(np.intc))
    # duplicate the first stored entry of row 2 (kept by the indptr form of the constructor)
    r0, r1 = a.indptr[2], a.indptr[3]
    assert r1 > r0
    indices = np.concatenate([a.indices[:r0 + 1], a.indices[r0:r0 + 1], a.indices[r0 + 1:]])
    indptr = a.indptr.copy()
    indptr[3:] += 1
    dup = sp.csr_matrix((np.ones(indices.size, np.intc), indices, indptr), shape=(U, I))
    assert dup.nnz == a.nnz + 1
    empty = sp.csr_matrix((U, I), dtype=np.intc)
    sparse = sp.csr_matrix((rng.random((U, I)) < 0.08).astype(np.intc))
    return [dup, empty, sparse]


def _dense_counts(rowptr, colidx, shape):
    c = np.zeros(shape, np.float64)
    np.add.at(c, (np.repeat(np.arange(shape[0]), np.diff(rowptr)), colidx), 1.0)
    return c


def _stack_reference(mats, u0, i0, gu, gi, L, leaky, keep, seed, step):
    """torch float64 autograd over dense masked matrices from edge_drop_ref: outputs and dL/du0, dL/di0."""
    from sa_gnn_amd import graph
    T, U, _ = u0.shape
    I = i0.shape[1]
    scale = float(np.float32(1.0) / np.float32(keep))
    tu = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    ti = torch.tensor(i0, dtype=torch.float64, requires_grad=True)
    lk = lambda x: torch.where(leaky * x >= x, leaky * x, x)
    outs_u, outs_i = [], []
    for k, m in enumerate(mats):
        cu = _dense_counts(*graph.csr_arrays(m), (U, I))                            # what the forward plans store,
        ci = _dense_counts(*graph.csr_arrays(graph.transpose(m)), (I, U))          # the phantom edge of an empty one included
        eu, ei = [tu[k]], [ti[k]]
        for l in range(L):
            au = torch.from_numpy(scale * cu * R.dense_mask(seed, step, k, l, 0, U, I, keep=keep))
            ai = torch.from_numpy(scale * ci * R.dense_mask(seed, step, k, l, 1, U, I, keep=keep).T)
            nu, ni = lk(au @ ei[-1]) + eu[-1], lk(ai @ eu[-1]) + ei[-1]
            eu.append(nu)
            ei.append(ni)
        outs_u.append(sum(eu[1:], eu[0]))
        outs_i.append(sum(ei[1:], ei[0]))
    ou, oi = torch.stack(outs_u), torch.stack(outs_i)
    ((ou * torch.tensor(gu, dtype=torch.float64)).sum() + (oi * torch.tensor(gi, dtype=torch.float64)).sum()).backward()
    return ou.detach().numpy(), oi.detach().numpy(), tu.grad.numpy(), ti.grad.numpy()


@pytest.mark.parametrize("L", [2, 3])
def test_stack_and_adjoint_vs_float64_autograd(dev, L):
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import graph, ops
    T, U, I, d, leaky, keep = 3, 37, 29, 32, 0.5, 0.5
    rng = np.random.default_rng(40 + L)
    mats = _intervals(rng, U, I)
    u0, gu = (rng.standard_normal((T, U, d)).astype(np.float32) for _ in range(2))
    i0, gi = (rng.standard_normal((T, I, d)).astype(np.float32) for _ in range(2))
    want_u, want_i, want_du, want_di = _stack_reference(mats, u0, i0, gu, gi, L, leaky, keep, SEED, STEP)
    pairs = [graph.interval_pair(m, dev, tuning=TUNING) for m in mats]
    plans_u, plans_i = [a.plan for a, _ in pairs], [t.plan for _, t in pairs]
    assert plans_u[0].partner_adjoint is not None and plans_u[0].info.n_long_rows >= 1
    batch = ops.SpmmBatch(plans_u, plans_i)
    assert batch.adjoint() is not batch
    drop = ops.EdgeDrop(SEED, STEP, keep)
    gu_d, gi_d = torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev)

    def run(pu, pi, dr):
        tu = torch.from_numpy(u0).to(dev).requires_grad_(True)
        ti = torch.from_numpy(i0).to(dev).requires_grad_(True)
        ou, oi = ag.gnn_stack(tu, ti, pu, pi, L, leaky, drop=dr)
        ((ou * gu_d).sum() + (oi * gi_d).sum()).backward()
        return ou.detach(), oi.detach(), tu.grad, ti.grad

    got = run(batch, None, drop)
    np.testing.assert_allclose(got[0].cpu().numpy(), want_u, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got[1].cpu().numpy(), want_i, rtol=1e-4, atol=1e-4)
    scale = max(float(np.abs(want_du).max()), 1.0)
    np.testing.assert_allclose(got[2].cpu().numpy(), want_du, rtol=1e-4, atol=2e-6 * scale * L * 50)
    np.testing.assert_allclose(got[3].cpu().numpy(), want_di, rtol=1e-4, atol=2e-6 * scale * L * 50)
    # the per-interval form agrees with the batched form bit for bit; so does a second run
    for other in (run(plans_u, plans_i, drop), run(batch, None, ops.EdgeDrop(SEED, STEP, keep))):
        for a, b in zip(got, other):
            assert torch.equal(a, b)
    # another step: another result; no drop: the undropped entry's bits
    moved = run(batch, None, ops.EdgeDrop(SEED, STEP + 1, keep))
    assert not torch.equal(moved[0], got[0]) and not torch.equal(moved[2], got[2])
    plain = run(batch, None, None)
    ou = torch.empty((T, U, d), device=dev)
    oi = torch.empty((T, I, d), device=dev)
    ops.gnn_stack(batch, torch.from_numpy(u0).to(dev), torch.from_numpy(i0).to(dev), L, leaky, ou, oi)
    assert torch.equal(plain[0], ou) and torch.equal(plain[1], oi) and not torch.equal(plain[0], got[0])


# ---- the large-row-block variant (RPW = kRowsPerWave) ---------------------------------------------------------------------
BIG_U, BIG_I, BIG_D = 262144, 4096, 32      # kSmallRows users exactly: the launchers test n_rows < kSmallRows


def _big_matrix(rng, row1):
    """[BIG_U, BIG_I] stored pattern, about 660 k entries: user 0 empty, user 1 the items `row1`, user 2 a duplicated
    entry, user 3 300 items (five chunks of 64), user 4 ten items (medium), the others min of two draws from 0 .. 8
    unsorted random items (mean 2.5, so an item row of the transpose holds about 160; uniform degrees 0 .. 8 would store
    1.05 M entries, 256 per item row, and only cost host time)."""
    deg = np.minimum(rng.integers(0, 9, BIG_U), rng.integers(0, 9, BIG_U))
    deg[:5] = [0, len(row1), 4, 300, 10]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = rng.integers(0, BIG_I, rowptr[-1]).astype(np.int32)
    colidx[rowptr[1]:rowptr[2]] = row1
    colidx[rowptr[2]:rowptr[3]] = [3, 7, 7, BIG_I - 1]
    colidx[rowptr[3]:rowptr[4]] = rng.choice(BIG_I, 300, replace=False)
    return sp.csr_matrix((np.ones(colidx.size, np.intc), colidx, rowptr), shape=(BIG_U, BIG_I))


def _sparse_counts(rowptr, colidx, shape):
    """float64 CSR of the multiplicities of a stored pattern (the COO -> CSR conversion sums duplicates)."""
    rows = np.repeat(np.arange(shape[0]), np.diff(rowptr))
    return sp.coo_matrix((np.ones(colidx.size), (rows, colidx)), shape=shape).tocsr()


def _sparse_masked(counts, rows_are_users, drop, k, l, direction):
    """scale * counts with the entries edge_drop_ref drops removed; drop = None: counts."""
    if drop is None:
        return counts
    c = counts.tocoo()
    users, items = (c.row, c.col) if rows_are_users else (c.col, c.row)
    kept = R.keep_mask(drop.seed, drop.step, k, l, direction, users, items, thresh=drop.threshold)
    return sp.csr_matrix((float(np.float32(drop.scale)) * c.data * kept, (c.row, c.col)), shape=counts.shape)


def _sparse_stack_reference(cu, ci, u0, i0, L, leaky, drop):
    """The layer recurrence of _stack_reference in float64 on sparse matrices, forward only: cu[k] / ci[k] the user-side
    and item-side multiplicities of interval k. Returns the outputs and, for assert_sum_close, their abs_terms: with
    t^0 = 0, t^{l+1} = A (|e_other^l| + t_other^l) + |e^l| + t^l bounds what the roundings of layer l + 1 and the
    errors its inputs carry can sum to, in units of 3 eps32; the output sum_l e^l collects sum_l (|e^l| + t^l)."""
    lk = lambda x: np.maximum(leaky * x, x)
    outs, terms = ([], []), ([], [])
    for k in range(len(cu)):
        e, t = (u0[k].astype(np.float64), i0[k].astype(np.float64)), (np.zeros(u0[k].shape), np.zeros(i0[k].shape))
        out, term = list(e), [np.abs(e[0]), np.abs(e[1])]
        for l in range(L):
            au = _sparse_masked(cu[k], True, drop, k, l, 0)
            ai = _sparse_masked(ci[k], False, drop, k, l, 1)
            t = (au @ (np.abs(e[1]) + t[1]) + np.abs(e[0]) + t[0], ai @ (np.abs(e[0]) + t[0]) + np.abs(e[1]) + t[1])
            e = (lk(au @ e[1]) + e[0], lk(ai @ e[0]) + e[1])
            for side in (0, 1):
                out[side] = out[side] + e[side]
                term[side] = term[side] + np.abs(e[side]) + t[side]
        for side in (0, 1):
            outs[side].append(out[side])
            terms[side].append(term[side])
    return np.stack(outs[0]), np.stack(outs[1]), np.stack(terms[0]), np.stack(terms[1])


def test_large_row_block_variant_with_and_without_drop(dev):
    """262,144 users: every launch takes the RPW = kRowsPerWave instantiation of its kernel, per plan and batched,
    default and DROP, on rows of every class (the 4,096 item rows are all long, several chunks each)."""
    from sa_gnn_amd import graph, ops
    U, I, d, leaky, keep, T, L = BIG_U, BIG_I, BIG_D, 0.5, 0.5, 2, 2
    rng = np.random.default_rng(262144)
    drop = ops.EdgeDrop(SEED, STEP, keep)
    tag = ops.edge_tag(0, 1, 0)
    row1 = np.flatnonzero(~R.keep_mask(SEED, STEP, 0, 1, 0, np.full(I, 1), np.arange(I), keep=keep))[:3]
    mats = [_big_matrix(rng, row1), sp.csr_matrix((U, I), dtype=np.intc)]                # the second: the phantom edge alone
    pairs = [graph.interval_pair(m, dev, tuning=TUNING) for m in mats]
    plans_u, plans_i = [a.plan for a, _ in pairs], [t.plan for _, t in pairs]
    pu, pi = plans_u[0], plans_i[0]
    deg = np.diff(graph.csr_arrays(mats[0])[0])
    assert (deg == 0).any() and ((deg > 0) & (deg <= 4)).any() and ((deg > 4) & (deg <= 16)).any()
    assert pu.info.n_long_rows >= 1 and pu.info.n_chunks > pu.info.n_long_rows
    assert pi.info.n_long_rows == I and pi.info.n_chunks >= 2 * I
    assert plans_u[1].nnz == 1 and plans_i[1].nnz == 1
    cu = [_sparse_counts(*graph.csr_arrays(m), (U, I)) for m in mats]
    ci = [_sparse_counts(*graph.csr_arrays(graph.transpose(m)), (I, U)) for m in mats]
    assert cu[0][2, 7] == 2 and ci[0][7, 2] == 1 and pu.nnz > pi.nnz                     # the duplicated stored entry
    u0 = rng.standard_normal((T, U, d)).astype(np.float32)
    i0 = rng.standard_normal((T, I, d)).astype(np.float32)
    u0_d, i0_d = torch.from_numpy(u0).to(dev), torch.from_numpy(i0).to(dev)

    # (a), (b): one product on each orientation, default and dropped, with a residual
    for dr in (None, drop):
        for plan, counts, rows_are_users, x, x_d, res, res_d in ((pu, cu[0], True, i0[0], i0_d[0], u0[1], u0_d[1]),
                                                                   (pi, ci[0], False, u0[0], u0_d[0], i0[1], i0_d[1])):
            if dr is None:
                got = ops.spmm_ex(plan, x_d, leaky, residual=res_d, want_out=True)
            else:
                got = ops.spmm_drop(plan, x_d, leaky, dr, tag, rows_are_users, residual=res_d, want_out=True)
            a = _sparse_masked(counts, rows_are_users, dr, 0, 1, 0)
            s = a @ x.astype(np.float64)
            assert_sum_close(got.cpu().numpy(), np.maximum(leaky * s, s) + res, a @ np.abs(x).astype(np.float64) + np.abs(res))
            if dr is not None and rows_are_users:                                         # user 1: every edge dropped
                assert torch.equal(got[1], res_d[1]) and not torch.equal(got[2], res_d[2])

    # (c): the batched stack, and each interval of it through the per-plan entry, bit for bit
    batch = ops.SpmmBatch(plans_u, plans_i)
    for dr in (None, drop):
        ou, oi = torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev)
        ops.gnn_stack(batch, u0_d, i0_d, L, leaky, ou, oi, drop=dr)
        want_u, want_i, terms_u, terms_i = _sparse_stack_reference(cu, ci, u0, i0, L, leaky, dr)
        assert_sum_close(ou.cpu().numpy(), want_u, terms_u)
        assert_sum_close(oi.cpu().numpy(), want_i, terms_i)
        for k in range(T):
            ku, ki = torch.empty((U, d), device=dev), torch.empty((I, d), device=dev)
            ops.gnn_interval(plans_u[k], plans_i[k], u0_d[k], i0_d[k], L, leaky, ku, ki, drop=dr, interval=k)
            assert torch.equal(ku, ou[k]) and torch.equal(ki, oi[k])


# ---- Recommender ------------------------------------------------------------------------------------------------------
def _masked_oracle_interval(handler, keep, seed, step):
    """O.torch_gnn_interval with the edge masks of edge_drop_ref; torch_train_loss calls it for k = 0, 1, ... in order."""
    calls = []

    def interval(u0, i0, adj_idx, tp_idx, n_layers, leaky):
        k = len(calls)
        calls.append(k)
        U, I = u0.shape[0], i0.shape[0]
        scale = float(np.float32(1.0) / np.float32(keep))
        cu, ci = np.zeros((U, I)), np.zeros((I, U))
        np.add.at(cu, (np.asarray(adj_idx)[:, 0], np.asarray(adj_idx)[:, 1]), 1.0)
        np.add.at(ci, (np.asarray(tp_idx)[:, 0], np.asarray(tp_idx)[:, 1]), 1.0)
        lk = lambda x: torch.where(leaky * x >= x, leaky * x, x)
        eu, ei = [u0], [i0]
        for l in range(n_layers):
            au = torch.from_numpy(scale * cu * R.dense_mask(seed, step, k, l, 0, U, I, keep=keep))
            ai = torch.from_numpy(scale * ci * R.dense_mask(seed, step, k, l, 1, U, I, keep=keep).T)
            nu, ni = lk(au @ ei[-1]) + eu[-1], lk(ai @ eu[-1]) + ei[-1]
            eu.append(nu)
            ei.append(ni)
        return sum(eu[1:], eu[0]), sum(ei[1:], ei[0])

    return interval


def test_recommender_train_loss_with_edge_keep_rate(dev, monkeypatch):
    from test_gpu_train import _oracle_params, _setup
    rec, handler, NNs, args = _setup(dev, 32, 32, 1)
    monkeypatch.setattr(args, "edgeKeepRate", 0.5, raising=False)
    np.random.seed(3)
    batIds = np.random.permutation(args.user)[:args.batch]
    uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
    su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
    batch = {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si,
             "edge_seed": (SEED, STEP)}
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in NNs.params.items()}
    pre2, ssl2 = rec.train_loss(dict(batch), keep_rate=1.0)
    off = rec.train_loss(dict(batch), keep_rate=1.0, edge_keep=1.0)
    assert np.isfinite(float(pre)) and np.isfinite(float(ssl))
    assert float(pre2) == pytest.approx(float(pre), rel=1e-4) and float(ssl2) == pytest.approx(float(ssl), rel=1e-4)
    assert abs(float(off[0]) - float(pre)) > 1e-3 * abs(float(pre)) or abs(float(off[1]) - float(ssl)) > 1e-3 * abs(float(ssl))
    # float64 autograd over the oracle's objective, its GNN stack given the same masks
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    monkeypatch.setattr(O, "torch_gnn_interval", _masked_oracle_interval(handler, 0.5, SEED, STEP))
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, batch, {"T": 2, "L": 2, "leaky": 0.5, "heads": 16})
    (opre + args.ssl_reg * ossl).backward()
    assert abs(float(pre.detach()) - float(opre.detach())) <= 1e-4 * max(abs(float(opre)), 1.0)
    assert abs(float(ssl.detach()) - float(ossl.detach())) <= 1e-4 * max(abs(float(ossl)), 1.0)
    checked = 0
    for name, leaf in leaves.items():        # the training-gradient tolerance of test_gpu_train.py
        got, want = grads[name], leaf.grad
        if want is None:
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        assert got is not None, f"no gradient reached {name}"
        a, b = got.cpu().double().numpy(), want.numpy()
        floor = max(5e-5 * np.abs(b).max(), 2e-5)
        if name.endswith("k_bias"):
            floor = max(floor, 1e-3 * float(leaves[name.replace("k_bias", "k_kernel")].grad.abs().max()))
        bad = np.abs(a - b) > 2e-4 * np.abs(b) + floor
        assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"
        checked += 1
    assert checked >= 20


def test_inference_never_drops(dev, monkeypatch):
    from test_gpu_train import _setup
    rec, handler, NNs, args = _setup(dev, 32, 32, 1)
    res, outs = {}, {}
    for rate in (1.0, 0.5):
        monkeypatch.setattr(args, "edgeKeepRate", rate, raising=False)
        fu, fi = rec.forward()
        outs[rate] = (fu.clone(), fi.clone())
        np.random.seed(1)
        res[rate] = rec.testEpoch()
    assert torch.equal(outs[1.0][0], outs[0.5][0]) and torch.equal(outs[1.0][1], outs[0.5][1])
    assert res[1.0] == res[0.5]
