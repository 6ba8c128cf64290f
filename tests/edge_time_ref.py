"""numpy / float64 torch restatement of the time-aware messages of the interval SpMM (--edgeTime slot),
written from the contract and not from graph.py:

  buckets    mi = the smallest stored timestamp over all interval matrices; bucket = (t - mi) // (86400 * slot) on
             integers; maxTime = largest bucket + 1; the table has M = maxTime + 1 rows (the reference's spare row);
  edges      a stored entry keeps its own bucket where the pattern keeps duplicates (the user side without
             normalisation); a MERGED edge (the item side, and both sides under the symmetric normalisation) takes the
             bucket of the LATEST of its duplicated entries; the phantom edge (0, 0) of an empty matrix has bucket 0;
  product    s[r] = sum_e w[e] * (X[col[e]] + TE[bucket[e]]) = A @ X + C @ TE with A the (weighted) adjacency and
             C[r, b] the summed weight of row r's edges in bucket b;
  gradient   dTE[b] = sum_{e: bucket[e] = b} w[e] * gm[row[e]] = C^T @ gm, which autograd yields from the line above.
"""
import numpy as np
import scipy.sparse as sp
import torch

import adj_norm_ref as N

DAY = 86400


def bucket(t, mi, slot):
    """One timestamp's bucket, on Python integers (no overflow at any size)."""
    width = DAY * slot
    assert width == int(width)
    return (int(t) - int(mi)) // int(width)


def time_process(mats, slot):
    """(mi, maxTime) of the reference's DataHandler.timeProcess over the interval matrices `mats`."""
    stamps = [int(t) for m in mats for t in sp.coo_matrix(m).data]
    mi = min(stamps)
    return mi, max(bucket(t, mi, slot) for t in stamps) + 1


def stored(mat):
    """[(user, item, timestamp)] of the stored entries in COO order."""
    c = sp.coo_matrix(mat)
    return [(int(u), int(i), int(t)) for u, i, t in zip(c.row, c.col, c.data)]


def latest(mat):
    """{(user, item): latest timestamp of its stored entries}."""
    out = {}
    for u, i, t in stored(mat):
        out[(u, i)] = max(t, out.get((u, i), t))
    return out


def pattern_buckets(mat, mi, slot, side, merged):
    """The bucket of every edge of one pattern in ITS edge order. side "user": rows are users, columns ascending only
    when merged (else stored order); side "item": rows are items, users ascending within an item, always merged."""
    ent = stored(mat)
    if not ent:
        return [0]
    if side == "user" and not merged:
        return [bucket(t, mi, slot) for _, _, t in ent]
    lt = latest(mat)
    keys = sorted(lt) if side == "user" else sorted(lt, key=lambda ui: (ui[1], ui[0]))
    return [bucket(lt[k], mi, slot) for k in keys]


def time_adjoint(rowptr, buckets, n_buckets, weights=None):
    """(rowptr, colidx, weights) of the CSR whose rows are buckets: the row of every edge, edge order kept in a bucket."""
    per = [[] for _ in range(n_buckets)]
    for r in range(len(rowptr) - 1):
        for e in range(rowptr[r], rowptr[r + 1]):
            per[buckets[e]].append((r, None if weights is None else weights[e]))
    rp = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    ci = np.array([r for p in per for r, _ in p], np.int32)
    w = None if weights is None else np.array([x for p in per for _, x in p], np.float32)
    return rp, ci, w


def dense_terms(mat, mi, slot, M, norm):
    """float64 (A_user [U, I], C_user [U, M], A_item [I, U], C_item [I, M]) of one interval matrix under norm "none" or
    "sym": s_user = A_user @ e_item + C_user @ TE_user, s_item = A_item @ e_user + C_item @ TE_item."""
    U, I = mat.shape
    a_u, a_i = np.zeros((U, I)), np.zeros((I, U))
    c_u, c_i = np.zeros((U, M)), np.zeros((I, M))
    ent = stored(mat)
    if not ent:                                          # the phantom edge
        a_u[0, 0] = a_i[0, 0] = c_u[0, 0] = c_i[0, 0] = 1.0
        return a_u, c_u, a_i, c_i
    lt = latest(mat)
    if norm == "sym":
        w = N.dense_sym(mat)
        for (u, i), t in lt.items():
            a_u[u, i] = a_i[i, u] = w[u, i]
            c_u[u, bucket(t, mi, slot)] += w[u, i]
            c_i[i, bucket(t, mi, slot)] += w[u, i]
        return a_u, c_u, a_i, c_i
    for u, i, t in ent:                                  # the user side keeps duplicates, each with its own bucket
        a_u[u, i] += 1.0
        c_u[u, bucket(t, mi, slot)] += 1.0
    for (u, i), t in lt.items():                         # the item side merges them: the latest
        a_i[i, u] = 1.0
        c_i[i, bucket(t, mi, slot)] += 1.0
    return a_u, c_u, a_i, c_i


def leaky_max(x, leaky):
    return torch.where(leaky * x >= x, leaky * x, x)


def stack(terms, u0, i0, te, n_layers, leaky):
    """The stack on float64 torch tensors: terms[k] = dense_terms of interval k (as tensors), u0 [T, U, d], i0 [T, I, d],
    te [T, L, 2, M, d]. e^{l+1} = leaky(A e_other^l + C TE[k, l, dir]) + e^l; outputs sum_l e^l."""
    outs_u, outs_i = [], []
    for k, (a_u, c_u, a_i, c_i) in enumerate(terms):
        eu, ei = [u0[k]], [i0[k]]
        for l in range(n_layers):
            nu = leaky_max(a_u @ ei[-1] + c_u @ te[k, l, 0], leaky) + eu[-1]
            ni = leaky_max(a_i @ eu[-1] + c_i @ te[k, l, 1], leaky) + ei[-1]
            eu.append(nu)
            ei.append(ni)
        outs_u.append(sum(eu[1:], eu[0]))
        outs_i.append(sum(ei[1:], ei[0]))
    return torch.stack(outs_u), torch.stack(outs_i)


def stack_reference(terms, u0, i0, te, gu, gi, n_layers, leaky):
    """float64 autograd of `stack` for L = <out_u, gu> + <out_i, gi>: (out_u, out_i, dU, dI, dTE) as numpy."""
    t64 = lambda x, g=False: torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=g)
    tu, ti, tt = t64(u0, True), t64(i0, True), t64(te, True)
    ou, oi = stack([tuple(t64(x) for x in tm) for tm in terms], tu, ti, tt, n_layers, leaky)
    ((ou * t64(gu)).sum() + (oi * t64(gi)).sum()).backward()
    return ou.detach().numpy(), oi.detach().numpy(), tu.grad.numpy(), ti.grad.numpy(), tt.grad.numpy()
