"""numpy restatement of sagnn_candidate_rank_f32's contract (include/sagnn.h, "Sampled-candidate evaluation") in the
reference's own terms: sort the candidates by score, descending and stable (ties keep candidate order), and take the
position of the target's first entry in that list (reference model.py:484-510). The kernel counts instead of
sorting; the tests compare the two exactly."""
import numpy as np


def rank_by_sort(scores, cand, target):
    """scores float [B, C], cand int [B, C], target int [B] -> int64 [B]: the target's position in the stable
    descending order of its row (NaN read as -inf); -1 when the row holds no copy of the target or target < 0."""
    s = np.where(np.isnan(scores), -np.inf, np.asarray(scores, dtype=np.float64))
    cand, target = np.asarray(cand), np.asarray(target)
    out = np.full(len(target), -1, dtype=np.int64)
    for b in range(len(target)):
        if target[b] < 0:
            continue
        order = np.argsort(-s[b], kind="stable")
        at = np.flatnonzero(cand[b][order] == target[b])
        if at.size:
            out[b] = at[0]
    return out


def head_scores(U, I, S, A, uids, cand, leaky):
    """float64 head scores <U[u], I[c]> + <leaky(S[b]), A[c]> [B, C] (exact for the integer-valued data the tests use)."""
    U, I, S, A = (np.asarray(x, dtype=np.float64) for x in (U, I, S, A))
    lk = np.maximum(leaky * S, S)
    return np.einsum("bd,bcd->bc", U[uids], I[cand]) + np.einsum("bd,bcd->bc", lk, A[cand])
