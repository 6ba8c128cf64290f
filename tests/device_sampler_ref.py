"""numpy restatement of the device sampler's contract (include/sagnn.h, "Device sampling of the training batch"),
written from the reference's loops (model.py:252-339, DataHandler.py:28-41) and the Philox4x32-10 definition. The
device sampler's tests compare the kernels with it bit for bit."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 on uint32 counters (arrays broadcast), key = (seed low word, seed high word)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
    return [x.astype(np.uint32) for x in c]


def uniform(seed, user, j, step, stream, n):
    """Uniform integers on [0, n): the high 64 bits of ((w0 << 32) | w1) * n, as int64."""
    w = philox4x32_10(user, j, step, stream, seed)
    xh, xl = w[0].astype(np.uint64), w[1].astype(np.uint64)
    n = np.asarray(n, dtype=np.uint64)
    return ((xh * n + ((xl * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def rth_allowed(banned, r):
    """The r-th item (0-based) of [0, n) not in the sorted unique list `banned`."""
    banned = np.asarray(banned, dtype=np.int64)
    return np.asarray(r, dtype=np.int64) + np.searchsorted(banned - np.arange(banned.size), r, side="right")


def banned_lists(handler, n_items):
    """Per user the sorted distinct items negSamp never returns: the trnMat row, the last item, the test item."""
    out = []
    for u, q in enumerate(handler.sequence):
        row = handler.trnMat[u].toarray().reshape(-1)
        ban = set(np.flatnonzero(row != 0).tolist())
        if len(q):
            ban.add(int(q[-1]))
        t = handler.tstInt[u]
        if t is not None and 0 <= int(t) < n_items:
            ban.add(int(t))
        out.append(np.array(sorted(ban), dtype=np.int64))
    return out


def sample_train(handler, n_items, bat, n_slots, tsn, pred_num, P, seed, step):
    """(uids, iids, uLocs_seq, seg_begin, seg_len) as sagnn_sample_train_i32 writes them; seg_begin indexes the
    concatenation of handler.sequence."""
    lens = np.array([len(q) for q in handler.sequence], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])
    bans = banned_lists(handler, n_items)
    pos_u, pos_i, neg_i, locs = [], [], [], []
    seg_begin, seg_len = np.zeros(n_slots, np.int64), np.zeros(n_slots, np.int32)
    for b, u in enumerate(bat):
        q = np.asarray(handler.sequence[u], dtype=np.int64)
        n_pos = len(q) - 1
        samp = max(min(tsn, n_pos), 0)
        hi = max(min(pred_num + 1, n_pos - 3), 1)
        choose = 1 + int(uniform(seed, u, 0, step, 0, hi))
        m = max(n_pos - choose, 0)
        seg_len[b] = min(m, P)
        seg_begin[b] = starts[u] + m - seg_len[b]
        if samp == 0:
            continue
        r = uniform(seed, np.full(samp, u), np.arange(samp), step, 1, n_items - bans[u].size)
        pos_u += [u] * samp
        pos_i += [int(q[n_pos - choose])] * samp
        neg_i += rth_allowed(bans[u], r).tolist()
        locs += [b] * samp
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    return i32(pos_u + pos_u), i32(pos_i + neg_i), i32(locs + locs), seg_begin, seg_len


def sample_ssl(handler, bat, ssl_num, seed, step):
    """Per interval k (uids, iids, uLocs_seq) as sagnn_sample_ssl_i32 writes them: pairs interleaved, both items drawn
    with replacement from the row's distinct items with a non-zero value (the reference's `toarray() != 0`)."""
    out = []
    for k, mat in enumerate(handler.subMat):
        us, its, ls = [], [], []
        for b, u in enumerate(bat):
            cand = np.flatnonzero(np.asarray(mat[u].toarray()).reshape(-1) != 0)
            npair = min(ssl_num, cand.size // 2)
            if npair == 0:
                continue
            j = np.arange(2 * npair)
            its += cand[uniform(seed, np.full(j.size, u), j, step, 2 + k, cand.size)].tolist()
            us += [u] * (2 * npair)
            ls += [b] * (2 * npair)
        out.append(tuple(np.asarray(v, dtype=np.int32) for v in (us, its, ls)))
    return out
