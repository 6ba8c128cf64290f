"""Reference side of the sampled-candidate softmax loss (--softmaxNegs). No new math:

  the candidate objective of row b is softmax_loss_ref.softmax_loss_np on the FULL item table with the list
  list_b + ([0, n_items) minus cand), because the target is always eligible there too;

so this file only builds those augmented lists, restates the stratified draw of sagnn_sample_strata_i32 on top of
device_sampler_ref's Philox, and assembles a device result (dIc rows at `cand`, dT rows added at the targets) into a
full-size dI in float64."""
import numpy as np

import device_sampler_ref as S
import softmax_loss_ref as R

STRATA_STREAM = 0xFFFFFFFF      # the Philox stream word of the draw; the batch samplers use 0, 1 and 2 + k


def strata(n_items, n_cand, seed, step):
    """int64 [n_cand]: candidate j = lo_j + uniform(lo_{j+1} - lo_j), lo_j = floor(j n_items / n_cand), the uniform
    from the Philox block of counter (j, 0, step, 0xFFFFFFFF) under key seed."""
    if n_cand == 0:
        return np.zeros(0, np.int64)
    j = np.arange(n_cand, dtype=np.int64)
    lo = j * n_items // n_cand
    up = (j + 1) * n_items // n_cand
    return lo + S.uniform(seed, j, 0, step, STRATA_STREAM, up - lo)


def row_lists(n_queries, excl_ptr=None, excl_items=None, excl_row=None):
    """Row b's exclusion list as softmax_loss_ref.eligible reads it: one int64 array per row."""
    out = []
    for b in range(n_queries):
        ids = np.zeros(0, np.int64)
        if excl_ptr is not None:
            L = b if excl_row is None else int(excl_row[b])
            if 0 <= L < len(excl_ptr) - 1:
                ids = np.asarray(excl_items[excl_ptr[L]:excl_ptr[L + 1]], dtype=np.int64)
        out.append(ids)
    return out


def augmented(n_queries, n_items, cand, excl_ptr=None, excl_items=None, excl_row=None):
    """(ptr, items): one list per row b, list_b united with every item outside cand, ascending."""
    outside = np.setdiff1d(np.arange(n_items, dtype=np.int64), np.asarray(cand, dtype=np.int64))
    lists = [np.union1d(ids, outside) for ids in row_lists(n_queries, excl_ptr, excl_items, excl_row)]
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    items = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
    return ptr, items


def softmax_loss_cand_np(Q, I, cand, target, inv_temp=1.0, scale=None, excl_ptr=None, excl_items=None, excl_row=None):
    """softmax_loss_np of the candidate objective: its dict, dI full-size."""
    ptr, items = augmented(len(Q), len(I), cand, excl_ptr, excl_items, excl_row)
    return R.softmax_loss_np(Q, I, target, inv_temp, scale, ptr, items, None)


def assemble_dI(n_items, cand, dIc, target, dT):
    """float64 [n_items, d]: zeros, dIc added at rows cand, dT added at the rows' targets (rows with one)."""
    dIc, dT = np.asarray(dIc, dtype=np.float64), np.asarray(dT, dtype=np.float64)
    full = np.zeros((n_items, dT.shape[1] if dT.ndim == 2 else dIc.shape[1]))
    if len(cand):
        full[np.asarray(cand, dtype=np.int64)] += dIc
    target = np.asarray(target, dtype=np.int64)
    ok = (target >= 0) & (target < n_items)
    np.add.at(full, target[ok], dT[ok])
    return full
