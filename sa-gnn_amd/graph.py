"""Adjacency preparation: scipy CSR (as DataHandler loads it) -> int32 rowptr/colidx on the
device + SpMM plans. Replaces the O(nnz) Python loop of DataHandler.transToLsts
(reference DataHandler.py:47-69, whose normalised values are dead) and the SparseTensor
constants of Recommender.prepareModel (reference model.py:227-237), keeping their edge sets:

  * forward adjacency  = the STORED structure of subMat[k] (duplicates and explicit zeros are
    edges, because edge values are never read: model.py:84-86);
  * transposed adjacency = DataHandler.transpose (DataHandler.py:9-11): scipy's COO->CSR sums
    duplicates, so a duplicated (u, i) counts once there;
  * an empty matrix becomes one phantom edge (0, 0) (DataHandler.py:66-68).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .ops import SpmmPlan


def transpose(mat):
    """Same contract as the reference's DataHandler.transpose (DataHandler.py:9-11)."""
    return sp.csr_matrix(sp.coo_matrix(mat).transpose())


def csr_arrays(mat, phantom_edge: bool = True):
    """(rowptr int32 [n_rows+1], colidx int32 [nnz]) with the edge set transToLsts would emit.

    The reference walks sp.coo_matrix(mat) in stored order and TF's SegmentSum needs the row ids
    sorted; a matrix whose COO rows are not sorted is rejected here the way TF-CPU rejects it."""
    coo = sp.coo_matrix(mat)
    n_rows = int(mat.shape[0])
    row = np.asarray(coo.row, dtype=np.int64)
    col = np.asarray(coo.col, dtype=np.int32)
    if row.size and np.any(np.diff(row) < 0):
        raise ValueError("adjacency rows are not sorted (tf.math.segment_sum would raise)")
    if row.size == 0 and phantom_edge:
        row = np.zeros(1, dtype=np.int64)
        col = np.zeros(1, dtype=np.int32)
    if row.size > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31-1 edges")
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n_rows), out=rowptr[1:])
    return rowptr.astype(np.int32), np.ascontiguousarray(col)


def sym_norm_weights(rowptr, colidx, n_rows: int, n_src: int):
    """float32 w[e] = 1 / sqrt(deg_row[r(e)] * deg_col[colidx[e]]) for the stored pattern (rowptr, colidx): the values of
    D_r^-1/2 A D_c^-1/2 that the reference's transToLsts(norm=True) computes and then drops (DataHandler.py:53-59,
    model.py:84-86). deg_row / deg_col count the pattern's stored edges per row / per column, duplicates included;
    computed in float64 and rounded once."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    if rowptr.size != n_rows + 1 or (colidx.size and (colidx.min() < 0 or colidx.max() >= n_src)):
        raise ValueError("sym_norm_weights: rowptr / colidx do not describe an n_rows x n_src pattern")
    deg_row = np.diff(rowptr)
    deg_col = np.bincount(colidx, minlength=n_src)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), deg_row)
    prod = deg_row[rows].astype(np.float64) * deg_col[colidx].astype(np.float64)
    return (1.0 / np.sqrt(prod)).astype(np.float32)


DAY = 86400


def edge_buckets(t, mi: int, slot: float):
    """int64 day buckets of timestamps `t`: (t - mi) // (86400 * slot), the reference's DataHandler.timeProcess
    (DataHandler.py:136-150) restated on integers (slot: days per bucket, a positive whole number of seconds)."""
    width = int(round(DAY * float(slot)))
    if width < 1 or width != DAY * float(slot):
        raise ValueError(f"slot = {slot}: 86400 * slot must be a whole number of seconds >= 1")
    t = np.asarray(t).astype(np.int64)
    if t.size and int(t.min()) < int(mi):
        raise ValueError(f"edge_buckets: a timestamp {int(t.min())} lies before mi = {mi}")
    return (t - np.int64(mi)) // np.int64(width)


def _latest(keys, t):
    """(unique keys ascending, the LATEST of the timestamps `t` that share each key)."""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.lexsort((t, keys))
    k = keys[order]
    last = np.r_[k[1:] != k[:-1], True] if k.size else np.zeros(0, dtype=bool)
    return k[last], np.asarray(t)[order][last]


def _stored_times(mat):
    """(rows, cols, timestamps int64) of the stored entries of `mat` in csr_arrays order; empty for an empty matrix."""
    coo = sp.coo_matrix(mat)
    return np.asarray(coo.row, dtype=np.int64), np.asarray(coo.col, dtype=np.int64), np.asarray(coo.data).astype(np.int64)


def _as_u16(b, n_buckets: int):
    if b.size and int(b.max()) >= n_buckets:
        raise ValueError(f"time buckets: id {int(b.max())} outside a table of {n_buckets} rows")
    return np.ascontiguousarray(b.astype(np.uint16))


def _time_spec(time, sub_mat):
    """(mi, slot, n_buckets) of interval_pair's time=(mi, slot[, n_buckets]); n_buckets defaults to this matrix's own
    max bucket + 2 (maxTime + 1, the reference's spare row included). A model passes the count of ALL its intervals."""
    from .ops import check_n_buckets
    mi, slot = int(time[0]), time[1]
    if len(time) > 2:
        return mi, slot, check_n_buckets(time[2])
    t = _stored_times(sub_mat)[2]
    return mi, slot, check_n_buckets((int(edge_buckets(t, mi, slot).max()) if t.size else 0) + 2)


class IntervalAdj:
    """One direction of one interval graph: what the reference holds as a tf SparseTensor
    (model.py:234 / :236). `.indices`-style access is not offered: the kernels use CSR."""

    def __init__(self, rowptr, colidx, shape, device, tuning=None, validate=True, weights=None, buckets=None,
                 n_buckets=None):
        self.dense_shape = (int(shape[0]), int(shape[1]))
        self.plan = SpmmPlan(rowptr, colidx, self.dense_shape[0], self.dense_shape[1], device=device,
                             tuning=tuning, validate=validate, weights=weights, buckets=buckets, n_buckets=n_buckets)
        self.nnz = self.plan.nnz

    @classmethod
    def from_scipy(cls, mat, device, tuning=None, buckets=None, n_buckets=None):
        rowptr, colidx = csr_arrays(mat)
        return cls(rowptr, colidx, mat.shape, device, tuning=tuning, buckets=buckets, n_buckets=n_buckets)


def exact_transpose_arrays(mat):
    """CSR arrays of the transposed STORED pattern of `mat`, multiplicities kept (a duplicated
    (u, i) stays two edges) — the adjoint of csr_arrays(mat), unlike DataHandler.transpose."""
    coo = sp.coo_matrix(mat)
    n_cols = int(mat.shape[1])
    order = np.argsort(np.asarray(coo.col, dtype=np.int64), kind="stable")
    rowptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(coo.col, dtype=np.int64), minlength=n_cols), out=rowptr[1:])
    return rowptr.astype(np.int32), np.ascontiguousarray(np.asarray(coo.row, dtype=np.int32)[order])


NORMS = ("none", "sym")


def merged_arrays(mat):
    """csr_arrays(mat) with duplicated stored entries merged: each (row, column) once, columns ascending within a row.
    Explicit zeros stay edges and an empty matrix keeps its phantom edge (0, 0)."""
    rowptr, colidx = csr_arrays(mat)
    n_rows, n_cols = int(mat.shape[0]), int(mat.shape[1])
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rowptr))
    key = np.unique(rows * max(n_cols, 1) + colidx)
    rows, cols = key // max(n_cols, 1), key % max(n_cols, 1)
    rp = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=rp[1:])
    return rp.astype(np.int32), np.ascontiguousarray(cols.astype(np.int32))


def pair_buckets(sub_mat, mi: int, slot, norm="none"):
    """int64 bucket ids of the two patterns interval_pair(sub_mat, norm=norm) builds, each in its plan's colidx order
    (DESIGN.md §20): a stored entry keeps its own bucket where the pattern keeps duplicates (the user side under
    norm="none"); a MERGED edge takes the bucket of the latest of its duplicated entries (the item side, and both sides
    under norm="sym"); the phantom edge of an empty matrix has bucket 0."""
    rows, cols, t = _stored_times(sub_mat)
    if t.size == 0:
        z = np.zeros(1, dtype=np.int64)
        return z, z.copy()
    U, I = int(sub_mat.shape[0]), int(sub_mat.shape[1])
    _, t_tp = _latest(cols * U + rows, t)                 # by (item, user): the order of DataHandler.transpose's CSR
    if norm == "sym":
        key, t_fw = _latest(rows * max(I, 1) + cols, t)   # merged_arrays' order
        b_fw = edge_buckets(t_fw, mi, slot)
        return b_fw, b_fw[np.argsort(key % max(I, 1), kind="stable")]
    return edge_buckets(t, mi, slot), edge_buckets(t_tp, mi, slot)


def _sym_pair(sub_mat, device, tuning, time=None):
    """The sym-normalised pair: the merged pattern and its exact transpose, the same weight on both for one
    (user, item), so each direction is the other's adjoint, weights included."""
    U, I = int(sub_mat.shape[0]), int(sub_mat.shape[1])
    rp, ci = merged_arrays(sub_mat)
    w = sym_norm_weights(rp, ci, U, I)
    bk = dict(fwd={}, tp={})
    if time is not None:
        mi, slot, M = _time_spec(time, sub_mat)
        b_fw, b_tp = pair_buckets(sub_mat, mi, slot, "sym")
        bk = dict(fwd=dict(buckets=_as_u16(b_fw, M), n_buckets=M), tp=dict(buckets=_as_u16(b_tp, M), n_buckets=M))
    users = np.repeat(np.arange(U, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")                           # by item, users ascending within an item
    rp_t = np.zeros(I + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=I), out=rp_t[1:])
    fwd = IntervalAdj(rp, ci, (U, I), device, tuning=tuning, weights=w, **bk["fwd"])
    tp = IntervalAdj(rp_t.astype(np.int32), np.ascontiguousarray(users[order]), (I, U), device, tuning=tuning,
                     weights=np.ascontiguousarray(w[order]), **bk["tp"])
    return fwd, tp


def interval_pair(sub_mat, device, tuning=None, norm="none", time=None):
    """(subAdj[k], subTpAdj[k]) for one interval matrix (reference model.py:230-237).

    norm="sym" (not in the reference's graph): the pattern is what csr_arrays emits with duplicated
    stored entries MERGED, edge (u, i) weighs 1 / sqrt(deg_u * deg_i) with the degrees counted on that pattern
    (sym_norm_weights), the item-side plan is the exact transpose with the same weights, and no partner_adjoint is
    built: the pair is its own adjoint. norm="none" is everything below, unchanged.

    With duplicated stored entries the two patterns are NOT transposes of each other (forward
    counts a duplicate twice, DataHandler.transpose merges it — DataHandler.py:9-11), so the
    backward pass cannot reuse the partner as the adjoint the way it does for canonical matrices.
    The exact adjoints are then built as well and hung on the plans (`partner_adjoint`):
    d/d e_i of the user-side sum gathers through the forward pattern's true transpose (the
    duplicate counts twice, as TF's gather gradient does), d/d e_u of the item-side sum through
    the merged forward pattern.

    time=(mi, slot[, n_buckets]): the stored values of sub_mat are Unix timestamps and both plans carry
    the bucket id of every edge (pair_buckets), for the time entries; n_buckets is the model's table size M."""
    if norm not in NORMS:
        raise ValueError(f"norm = {norm!r}: one of {NORMS}")
    if norm == "sym":
        return _sym_pair(sub_mat, device, tuning, time)
    bk_fw = bk_tp = {}
    if time is not None:
        mi, slot, M = _time_spec(time, sub_mat)
        b_fw, b_tp = pair_buckets(sub_mat, mi, slot, "none")
        bk_fw, bk_tp = dict(buckets=_as_u16(b_fw, M), n_buckets=M), dict(buckets=_as_u16(b_tp, M), n_buckets=M)
    fwd = IntervalAdj.from_scipy(sub_mat, device, tuning, **bk_fw)
    tp_mat = transpose(sub_mat)
    tp = IntervalAdj.from_scipy(tp_mat, device, tuning, **bk_tp)
    if fwd.nnz != tp.nnz:
        U, I = fwd.dense_shape
        rp, ci = csr_arrays(transpose(tp_mat))                       # (A_tp)^T: rows = users, merged
        fwd.plan.partner_adjoint = SpmmPlan(rp, ci, U, I, device=device, tuning=tuning)
        rp, ci = exact_transpose_arrays(sub_mat)                     # (A_fwd)^T: rows = items, duplicates kept
        tp.plan.partner_adjoint = SpmmPlan(rp, ci, I, U, device=device, tuning=tuning)
    return fwd, tp
