"""numpy restatement of the symmetric degree normalisation of the interval graphs (--adjNorm sym), written
from the contract and not from graph.py:

  pattern  the stored entries of the interval matrix in COO order, explicit zeros included, duplicated (user, item)
           entries MERGED into one edge; an empty matrix is the single phantom edge (0, 0);
  degrees  deg_u = edges of user u in that pattern, deg_i = edges of item i;
  weight   w(u, i) = float32(1 / sqrt(float64(deg_u * deg_i))): float64 arithmetic, one rounding.

Dense float64 helpers restate the stack recurrence of include/sagnn.h on such weighted matrices."""
import numpy as np
import scipy.sparse as sp
import torch


def weights(rowptr, colidx, n_rows, n_src):
    """w[e] for the pattern (rowptr, colidx) as given: row and column counts of that pattern, duplicates included."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    deg_row = rowptr[1:] - rowptr[:-1]
    deg_col = np.zeros(n_src, np.int64)
    for c in colidx:
        deg_col[c] += 1
    out = np.empty(colidx.size, np.float32)
    for r in range(n_rows):
        for e in range(rowptr[r], rowptr[r + 1]):
            out[e] = np.float32(1.0 / np.sqrt(np.float64(deg_row[r]) * np.float64(deg_col[colidx[e]])))
    return out


def pattern(mat):
    """The merged pattern of an interval matrix as a boolean [U, I] array (the phantom edge of an empty one included)."""
    coo = sp.coo_matrix(mat)
    p = np.zeros(mat.shape, bool)
    p[coo.row, coo.col] = True
    if coo.row.size == 0:
        p[0, 0] = True
    return p


def dense_sym(mat):
    """float64 [U, I]: diag(du)^-1/2 P diag(di)^-1/2 with each entry rounded to float32 once, as the plans store it."""
    return dense_sym_of_pattern(pattern(mat))


def dense_sym_of_pattern(p):
    """dense_sym for a boolean pattern given directly."""
    p = np.asarray(p, bool)
    du, di = p.sum(1).astype(np.float64), p.sum(0).astype(np.float64)
    with np.errstate(divide="ignore"):
        w = 1.0 / np.sqrt(du[:, None] * di[None, :])
    return np.where(p, w, 0.0).astype(np.float32).astype(np.float64)


def sparse_sym(mat):
    """dense_sym as a float64 scipy CSR, for matrices too large to hold densely."""
    coo = sp.coo_matrix(mat)
    row, col = (coo.row, coo.col) if coo.row.size else (np.zeros(1, np.int64), np.zeros(1, np.int64))
    p = sp.coo_matrix((np.ones(row.size), (row, col)), shape=mat.shape).tocsr()        # sums duplicates
    p.data[:] = 1.0                                                                      # ... into one edge
    du, di = np.asarray(p.sum(1)).ravel(), np.asarray(p.sum(0)).ravel()
    c = p.tocoo()
    w = (1.0 / np.sqrt(du[c.row] * di[c.col])).astype(np.float32).astype(np.float64)
    return sp.csr_matrix((w, (c.row, c.col)), shape=mat.shape)


def torch_interval(au, ai, u0, i0, n_layers, leaky):
    """One interval of the stack on dense float64 torch matrices au [U, I] (user side) and ai [I, U] (item side):
    e^{l+1} = leaky(A e_other^l) + e^l, outputs sum_l e^l (tf.maximum(leaky x, x))."""
    lk = lambda x: torch.where(leaky * x >= x, leaky * x, x)
    eu, ei = [u0], [i0]
    for _ in range(n_layers):
        nu, ni = lk(au @ ei[-1]) + eu[-1], lk(ai @ eu[-1]) + ei[-1]
        eu.append(nu)
        ei.append(ni)
    return sum(eu[1:], eu[0]), sum(ei[1:], ei[0])


def stack_reference(a_user, a_item, u0, i0, gu, gi, n_layers, leaky):
    """torch float64 autograd over per-layer dense matrices: a_user[k][l] [U, I], a_item[k][l] [I, U] (numpy float64).
    Returns the outputs [T, U, d], [T, I, d] and dL/du0, dL/di0 for L = <out_u, gu> + <out_i, gi>."""
    tu = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    ti = torch.tensor(i0, dtype=torch.float64, requires_grad=True)
    lk = lambda x: torch.where(leaky * x >= x, leaky * x, x)
    outs_u, outs_i = [], []
    for k in range(len(a_user)):
        eu, ei = [tu[k]], [ti[k]]
        for l in range(n_layers):
            au, ai = torch.from_numpy(a_user[k][l]), torch.from_numpy(a_item[k][l])
            nu, ni = lk(au @ ei[-1]) + eu[-1], lk(ai @ eu[-1]) + ei[-1]
            eu.append(nu)
            ei.append(ni)
        outs_u.append(sum(eu[1:], eu[0]))
        outs_i.append(sum(ei[1:], ei[0]))
    ou, oi = torch.stack(outs_u), torch.stack(outs_i)
    ((ou * torch.tensor(gu, dtype=torch.float64)).sum() + (oi * torch.tensor(gi, dtype=torch.float64)).sum()).backward()
    return ou.detach().numpy(), oi.detach().numpy(), tu.grad.numpy(), ti.grad.numpy()
