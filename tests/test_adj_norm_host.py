"""CPU suite of the opt-in symmetric degree normalisation (--adjNorm sym, graph.sym_norm_weights, SpmmPlan(weights=),
DESIGN.md §17): the weights against the numpy restatement (adj_norm_ref) bit for bit, the pattern rule (duplicates merged,
explicit zeros and the phantom edge kept), the flag, and the host-side checks of the weights. No GPU is touched."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import adj_norm_ref as R
from sa_gnn_amd import graph, ops

U, I = 9, 70


def _matrix():
    """[9, 70] stored pattern: user 0 a duplicated stored entry (item 5 twice), user 1 an explicit zero, user 2 empty,
    item 69 empty, user 3 a long row (every item but the last), the others a few items."""
    rows = [[5, 5, 8], [0, 3], [], list(range(I - 1)), [1, 2, 3, 4], [0], [8, 9, 10, 68], [7], [0, 1, 68]]
    vals = [[1, 1, 1], [1, 0], [], [1] * (I - 1), [1] * 4, [1], [1] * 4, [1], [1] * 3]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    m = sp.csr_matrix((np.array([v for x in vals for v in x], np.intc), np.array([c for r in rows for c in r], np.int32),
                       indptr), shape=(U, I))
    assert m.nnz == sum(len(r) for r in rows) and not m.has_canonical_format       # the duplicate and the zero are stored
    return m


def _merged(m):
    rp, ci = graph.merged_arrays(m)
    return rp, ci, np.repeat(np.arange(m.shape[0]), np.diff(rp))


def test_weights_equal_the_restatement_bit_for_bit():
    m = _matrix()
    rp, ci, rows = _merged(m)
    # the pattern: what csr_arrays emits, duplicates merged, the explicit zero an edge, the empty row and column empty
    raw_rp, raw_ci = graph.csr_arrays(m)
    assert raw_ci.size == m.nnz and ci.size == m.nnz - 1
    assert set(zip(rows.tolist(), ci.tolist())) == set(zip(np.repeat(np.arange(U), np.diff(raw_rp)).tolist(), raw_ci.tolist()))
    assert (1, 3) in set(zip(rows.tolist(), ci.tolist())) and rp[3] == rp[2] and 69 not in ci
    assert np.array_equal(R.pattern(m), sp.coo_matrix((np.ones(ci.size), (rows, ci)), shape=(U, I)).toarray() > 0)
    w = graph.sym_norm_weights(rp, ci, U, I)
    assert w.dtype == np.float32 and w.shape == ci.shape
    assert np.array_equal(w.view(np.uint32), R.weights(rp, ci, U, I).view(np.uint32))
    # and the dense formula: the same values placed at (user, item)
    dense = R.dense_sym(m)
    assert np.array_equal(dense[rows, ci].astype(np.float32).view(np.uint32), w.view(np.uint32))
    assert dense[3, 0] == np.float32(1.0 / np.sqrt(69.0 * 4.0))       # user 3 has 69 items, item 0 four users
    # on a pattern WITH duplicates the counts include them (the rule is "the pattern passed in")
    w_raw = graph.sym_norm_weights(raw_rp, raw_ci, U, I)
    assert np.array_equal(w_raw.view(np.uint32), R.weights(raw_rp, raw_ci, U, I).view(np.uint32))
    assert w_raw[0] == np.float32(1.0 / np.sqrt(3.0 * 3.0)) and w[0] == np.float32(1.0 / np.sqrt(2.0 * 2.0))   # (0, 5)


def test_forward_and_transposed_weights_agree_per_edge():
    m = _matrix()
    rp, ci, rows = _merged(m)
    w = graph.sym_norm_weights(rp, ci, U, I)
    order = np.argsort(ci, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=I))]).astype(np.int32)
    ci_t = rows[order].astype(np.int32)
    w_t = graph.sym_norm_weights(rp_t, ci_t, I, U)
    items_t = np.repeat(np.arange(I), np.diff(rp_t))
    fwd = {(u, i): x for u, i, x in zip(rows.tolist(), ci.tolist(), w.view(np.uint32).tolist())}
    tp = {(u, i): x for u, i, x in zip(ci_t.tolist(), items_t.tolist(), w_t.view(np.uint32).tolist())}
    assert fwd == tp and len(fwd) == ci.size


def test_empty_matrix_is_one_edge_of_weight_one():
    m = sp.csr_matrix((U, I), dtype=np.intc)
    rp, ci = graph.merged_arrays(m)
    assert ci.tolist() == [0] and rp.tolist() == [0] + [1] * U
    assert graph.sym_norm_weights(rp, ci, U, I).tolist() == [1.0]
    assert R.dense_sym(m)[0, 0] == 1.0 and R.dense_sym(m).sum() == 1.0


def test_row_sums_are_bounded_by_sqrt_of_the_row_degree():
    """sum_e w[e] over a row = deg_u^-1/2 sum_i deg_i^-1/2 <= sqrt(deg_u): holds for the rows, and the stack helper on the
    dense matrix computes what the weights say."""
    m = _matrix()
    rp, ci, rows = _merged(m)
    w = graph.sym_norm_weights(rp, ci, U, I).astype(np.float64)
    deg = np.diff(rp)
    sums = np.bincount(rows, weights=w, minlength=U)
    assert (sums <= np.sqrt(deg) * (1 + 1e-6)).all() and sums[2] == 0.0 and sums[3] > 1.0
    dense = R.dense_sym(m)
    assert np.allclose(dense.sum(1), sums, rtol=1e-12) and (dense.sum(0) <= np.sqrt((dense > 0).sum(0)) * (1 + 1e-6)).all()
    # one layer of the recurrence on all-ones embeddings with slope 1 returns 1 + the row sums, twice (e^0 + e^1)
    ones_u, ones_i = torch.ones((U, 1), dtype=torch.float64), torch.ones((I, 1), dtype=torch.float64)
    ou, oi = R.torch_interval(torch.from_numpy(dense), torch.from_numpy(dense.T.copy()), ones_u, ones_i, 1, 1.0)
    assert np.allclose(ou.numpy()[:, 0], 2.0 + sums, rtol=1e-12) and np.allclose(oi.numpy()[:, 0], 2.0 + dense.sum(0), rtol=1e-12)


def test_flag_parsing():
    from sa_gnn_amd import Params
    assert Params.build_parser().parse_args([]).adjNorm == "none" and Params.args.adjNorm == "none"
    assert Params.build_parser().parse_args(["--adjNorm", "sym"]).adjNorm == "sym"
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--adjNorm", "row"])


def test_prepare_model_refuses_an_unknown_norm(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    monkeypatch.setattr(args, "adjNorm", "row")
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    with pytest.raises(ValueError, match="adjNorm"):
        Recommender("cpu", None).prepareModel()                  # refused before the handler or a device is touched
    with pytest.raises(ValueError, match="norm"):
        graph.interval_pair(_matrix(), None, norm="row")


def test_parallel_setup_refuses_sym(monkeypatch):
    from sa_gnn_amd import parallel
    from sa_gnn_amd.Params import args
    assert parallel.make_sharding(3, 2, 0).T == 3
    monkeypatch.setattr(args, "adjNorm", "sym")
    for T, world in ((3, 2), (3, 8)):
        with pytest.raises(ValueError, match="adjNorm"):
            parallel.make_sharding(T, world, 0)


def test_plan_checks_the_weights_on_the_host():
    rp, ci = np.array([0, 1, 3], np.int32), np.array([0, 0, 1], np.int32)
    good = np.array([0.5, 1.0, 2.0], np.float32)
    make = lambda w: ops.SpmmPlan(rp, ci, 2, 2, device=None, weights=w)
    with pytest.raises(TypeError, match="float32"):
        make(good.astype(np.float64))
    with pytest.raises(TypeError, match="float32"):
        make(torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="expected 3"):
        make(good[:2])
    with pytest.raises(ValueError, match="expected 3"):
        make(np.ones((3, 1), np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        w = good.copy()
        w[1] = bad
        with pytest.raises(ValueError, match="NaN or Inf"):
            make(w)
    with pytest.raises(ValueError, match="host-only"):            # good weights: a host-only plan still takes none
        make(good)
    plan = make(None)
    assert not plan.weighted and plan.info.weighted == 0


def test_set_weights_entry_refuses_null_and_host_only_plans():
    import ctypes
    from sa_gnn_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    assert lib.sagnn_spmm_plan_set_weights(None, ctypes.addressof(buf)) == -1 and "plan is NULL" in _lib.last_error()
    plan = ops.SpmmPlan(np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), 2, 2, device=None)
    assert lib.sagnn_spmm_plan_set_weights(plan.handle, ctypes.addressof(buf)) == -5 and "host-only" in _lib.last_error()
    assert lib.sagnn_spmm_plan_set_weights(plan.handle, None) == -5 and "host-only" in _lib.last_error()
