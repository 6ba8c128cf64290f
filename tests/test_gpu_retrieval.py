"""GPU suite: full-catalogue top-K retrieval (sagnn_score_topk_f32 / ops.score_topk / Recommender.recommend and
testEpochFull) against float64 references kept in this file."""
import numpy as np
import pytest
import torch

from sa_gnn_amd import ops

EPS32 = float(np.finfo(np.float32).eps)


def _i32(dev, v):
    return torch.as_tensor(np.asarray(v, dtype=np.int32), device=dev)


def _host(outs):
    return [None if t is None else t.cpu().numpy() for t in outs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _exact_oracle(Q, I, k, rowptr=None, excl=None, target=None):
    """Reference top-k / rank in float64 for data whose fp32 products and sums are exact (small integers)."""
    S = Q.astype(np.float64) @ I.astype(np.float64).T               # NaN rows / items give NaN scores
    B, n = S.shape
    items = np.full((B, k), -1, np.int64)
    scores = np.full((B, k), -np.inf)
    ranks = np.zeros(B, np.int64)
    for b in range(B):
        elig = np.ones(n, bool)
        if rowptr is not None:
            elig[excl[rowptr[b]:rowptr[b + 1]]] = False
        t = None if target is None else int(target[b])
        if t is not None:
            elig[t] = True
        s = S[b]
        ok = np.flatnonzero(elig & ~np.isnan(s))
        order = ok[np.lexsort((ok, -s[ok]))]
        m = min(k, order.size)
        items[b, :m], scores[b, :m] = order[:m], s[order[:m]]
        if t is not None:
            if np.isnan(s[t]):
                ranks[b] = int(elig.sum())                           # a NaN target: every eligible item
            else:
                ranks[b] = int(((s[ok] > s[t]) | ((s[ok] == s[t]) & (ok < t))).sum())
    return items, scores, ranks


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 64, 128])
def test_topk_matches_float64_within_rounding(dev, d):
    rng = np.random.default_rng(d)
    combos = [(1, 1, 1), (17, 7, 10), (17, 512, 128), (4099, 7, 20), (4099, 512, 128), (52619, 512, 10),
              (52619, 1, 128), (1_000_003, 1, 20), (1_000_003, 7, 10)]
    for n_items, B, k in combos:
        Q = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(dev)
        I = torch.from_numpy(rng.standard_normal((n_items, d)).astype(np.float32)).to(dev)
        items, scores, _ = _host(ops.score_topk(Q, I, k))
        Q64, I64 = Q.double(), I.double()
        kk = min(k, n_items)
        for b0 in range(0, B, 32):
            s64 = Q64[b0:b0 + 32] @ I64.T
            tol = 4 * EPS32 * (Q64[b0:b0 + 32].abs() @ I64.abs().T)
            top = torch.topk(s64, kk, dim=1).indices.cpu().numpy()
            s64, tol = s64.cpu().numpy(), tol.cpu().numpy()
            for r in range(s64.shape[0]):
                b, g = b0 + r, items[b0 + r, :kk]
                assert (g >= 0).all() and (items[b, kk:] == -1).all() and np.isneginf(scores[b, kk:]).all(), (n_items, B, k, b)
                assert len(set(g.tolist())) == kk and (np.diff(scores[b, :kk]) <= 0).all()
                assert (np.abs(scores[b, :kk] - s64[r, g]) <= tol[r, g]).all(), (n_items, B, k, b)
                kth, tk = s64[r, top[r, -1]], tol[r, top[r, -1]]
                for i in set(g.tolist()) ^ set(top[r].tolist()):
                    assert abs(s64[r, i] - kth) <= tol[r, i] + tk, (n_items, B, k, b, i)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 64, 128])
def test_topk_exact_order_ties_exclusions_and_nan(dev, d):
    rng = np.random.default_rng(100 + d)
    B, n_items = 40, 4099
    Q = rng.integers(-3, 4, (B, d)).astype(np.float32)              # integer data: exact in fp32, many exact ties
    I = rng.integers(-3, 4, (n_items, d)).astype(np.float32)
    rows = [np.sort(rng.integers(0, n_items, int(rng.integers(0, 40)))) for _ in range(B)]   # duplicates allowed
    target = rng.integers(0, n_items, B)
    rows[1] = np.sort(np.append(rows[1], target[1]))                # row 1 excludes its own target: still ranked
    keep = np.array([5, 17, 4000])
    rows[2] = np.setdiff1d(np.arange(n_items), keep)                # row 2: three eligible items, fewer than k
    target[2] = 17
    Q[3, 0] = np.nan                                                # row 3: a NaN query row returns nothing
    I[7, 3] = np.nan                                                # item 7 scores NaN everywhere: never returned
    target[4] = 7                                                   # row 4: a NaN target is a miss
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    excl = np.concatenate(rows)
    for k in (1, 10, 128):
        want_i, want_s, want_r = _exact_oracle(Q, I, k, rowptr, excl, target)
        got_i, got_s, got_r = _host(ops.score_topk(torch.from_numpy(Q).to(dev), torch.from_numpy(I).to(dev), k,
                                                   excl=(rowptr, excl), target=_i32(dev, target)))
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_s, want_s.astype(np.float32))
        np.testing.assert_array_equal(got_r, want_r)
        for b in range(B):
            assert not (set(got_i[b].tolist()) & (set(rows[b].tolist()) - {int(target[b])}))
        assert (got_i[3] == -1).all() and np.isneginf(got_s[3]).all()
        assert (got_i[2, min(k, 3):] == -1).all() and set(got_i[2, :min(k, 3)].tolist()) <= set(keep.tolist())
        assert got_r[4] >= n_items - rows[4].size and 7 not in got_i


@pytest.mark.gpu
def test_topk_row_outputs_do_not_depend_on_batch_or_stride(dev):
    rng = np.random.default_rng(7)
    d, n_items, B, k = 64, 52619, 512, 20
    Q = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(dev)
    I = torch.from_numpy(rng.standard_normal((n_items, d)).astype(np.float32)).to(dev)
    tgt = _i32(dev, rng.integers(0, n_items, B))
    full = _host(ops.score_topk(Q, I, k, target=tgt))
    Ipad = torch.zeros((n_items, d + 12), device=dev)
    Ipad[:, :d] = I
    for a, b in zip(full, _host(ops.score_topk(Q, Ipad[:, :d], k, target=tgt))):
        assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip(full, _host(ops.score_topk(Q, I, k, target=tgt))):          # run to run
        assert np.array_equal(_bits(a), _bits(b))
    for r in (0, 13, 511):
        alone = _host(ops.score_topk(Q[r:r + 1], I, k, target=tgt[r:r + 1]))
        first = _host(ops.score_topk(torch.cat([Q[r:r + 1], Q[:511]]), I, k, target=torch.cat([tgt[r:r + 1], tgt[:511]])))
        last = _host(ops.score_topk(torch.cat([Q[:511], Q[r:r + 1]]), I, k, target=torch.cat([tgt[:511], tgt[r:r + 1]])))
        for j in range(3):
            for got in (alone[j][0], first[j][0], last[j][511]):
                assert np.array_equal(_bits(got), _bits(full[j][r])), (r, j)
    items, _, rank = full
    t_host = tgt.cpu().numpy()
    for b in range(B):
        hit = np.flatnonzero(items[b] == t_host[b])
        assert hit.tolist() == ([rank[b]] if rank[b] < k else []), b


@pytest.mark.gpu
def test_topk_graph_replay_matches_eager(dev):
    rng = np.random.default_rng(3)
    d, n_items, B, k = 32, 52619, 64, 10
    Q = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(dev)
    I = torch.from_numpy(rng.standard_normal((n_items, d)).astype(np.float32)).to(dev)
    tgt = _i32(dev, rng.integers(0, n_items, B))
    eager = [t.clone() for t in ops.score_topk(Q, I, k, target=tgt)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.score_topk(Q, I, k, target=tgt)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _small_recommender(dev):
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    rng = np.random.default_rng(12)
    args.graphNum, args.gnn_layer, args.latdim, args.leaky = 3, 2, 64, 0.5
    args.att_layer, args.batch, args.pos_length, args.testSize, args.test, args.shoot = 2, 64, 20, 50, True, 10
    U, I = 150, 120
    tmt = synthetic.make_trn_mat_time(U, I, [1500, 1400, 1300])
    seq = synthetic.make_sequence(tmt)
    tst_int = [int(rng.integers(0, I)) if u % 3 else None for u in range(U)]
    test_dict = {u + 1: list(rng.integers(1, I + 1, size=60)) for u in range(U)}
    handler = DataHandler.from_memory(tmt, seq, tst_int, test_dict)
    rec = Recommender(dev, handler)
    rec.prepareModel()
    g = torch.Generator(device="cpu").manual_seed(5)
    with torch.no_grad():
        for name in list(NNs.params):
            if name.endswith("bias") or name.endswith("beta"):
                NNs.params[name].copy_(0.1 * torch.randn(NNs.params[name].shape, generator=g))
        for key in ("uEmbed", "iEmbed", "posEmbed"):
            NNs.params[key].mul_(30)
    rec.forward()
    return rec, handler, args


def _pair_scores_and_tol(rec, bat, args):
    """predict() for every (user of bat, item) pair, and a bound on its distance to the retrieval score."""
    from sa_gnn_amd.Utils import NNLayers as NNs
    n_items = args.item
    sequence, mask, start, seq_end = rec._test_sequences(bat)
    B = len(bat)
    uL, iL, uLs = np.repeat(bat, n_items), np.tile(np.arange(n_items), B), np.repeat(np.arange(B), n_items)
    p = rec.predict(uL, iL, sequence, mask, uLs).cpu().numpy().astype(np.float64).reshape(B, n_items)
    att = rec._head_att(sequence, mask)[:B].double().cpu().numpy()
    fu = rec.final_user_vector.double().cpu().numpy()[bat]
    fi = rec.final_item_vector.double().cpu().numpy()
    tol = 8 * EPS32 * ((np.abs(fu) + np.abs(np.maximum(NNs.leaky * att, att))) @ np.abs(fi).T)
    return p, tol, start, seq_end


@pytest.mark.gpu
def test_recommender_recommend_and_full_ranking(dev):
    rec, handler, args = _small_recommender(dev)
    before = rec.testEpoch()
    users = np.arange(0, args.user, 2)
    items, scores = rec.recommend(users, k=10)
    assert items.shape == (len(users), 10) and scores.shape == (len(users), 10)
    trn = handler.trnMat.tocsr()
    for st in range(0, len(users), args.batch):
        bat = users[st:st + args.batch]
        p, tol, _, _ = _pair_scores_and_tol(rec, bat, args)
        for r, u in enumerate(bat):
            got = items[st + r]
            ok = got >= 0
            assert ok.any()
            assert not (set(got[ok].tolist()) & set(trn.indices[trn.indptr[u]:trn.indptr[u + 1]].tolist()))
            assert (np.abs(scores[st + r][ok] - p[r, got[ok]]) <= tol[r, got[ok]]).all(), u
    full = rec.testEpochFull()
    # brute force from predict(): bounds on each rank that let every near-tie fall either way
    flat, _ = rec._flat_sequences()
    ids = handler.tstUsrs
    lo_hr, hi_hr, lo_nd, hi_nd = (np.zeros(3) for _ in range(4))
    for st in range(0, len(ids), args.batch):
        bat = np.asarray(ids[st:st + args.batch], dtype=np.int64)
        p, tol, start, seq_end = _pair_scores_and_tol(rec, bat, args)
        for r, u in enumerate(bat):
            t = int(handler.tstInt[u])
            elig = np.ones(args.item, bool)
            elig[flat[start[r]:seq_end[r]]] = False
            elig[t] = False                                          # the target does not count against itself
            e = np.flatnonzero(elig)
            lo = int((p[r, e] > p[r, t] + tol[r, e] + tol[r, t]).sum())
            hi = int((p[r, e] >= p[r, t] - tol[r, e] - tol[r, t]).sum())
            for j, kk in enumerate((args.shoot, 5, 20)):
                lo_hr[j] += hi < kk
                hi_hr[j] += lo < kk
                lo_nd[j] += 1 / np.log2(hi + 2) if hi < kk else 0.0
                hi_nd[j] += 1 / np.log2(lo + 2) if lo < kk else 0.0
    n = len(ids)
    for j, (h, g) in enumerate((("HR", "NDCG"), ("HR5", "NDCG5"), ("HR20", "NDCG20"))):
        assert lo_hr[j] / n - 1e-12 <= full[h] <= hi_hr[j] / n + 1e-12, (h, full[h], lo_hr[j] / n, hi_hr[j] / n)
        assert lo_nd[j] / n - 1e-9 <= full[g] <= hi_nd[j] / n + 1e-9, (g, full[g], lo_nd[j] / n, hi_nd[j] / n)
    assert 0 < full["HR20"] <= 1
    assert rec.testEpoch() == before
