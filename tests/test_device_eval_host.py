"""CPU suite: the device evaluator's argument checks (sagnn_candidate_rank_f32), the rank rule restated in numpy
against Recommender.calcRes, the host-side tables of model.DeviceEvaluator against the host path's own batches, the
ExclusionCSR checks and the --evaluator flag. Every library call here is rejected before any device work, so no GPU
is needed."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import candidate_rank_ref as R
from sa_gnn_amd import _lib, ops


def _rank(lib, p, **over):
    a = dict(U=p, ldu=64, I=p, ldi=64, S=p, lds=64, A=p, lda=64, uids=p, cand=p, ldc=1000, target=p, leaky=0.5, B=8,
             C=1000, d=64, rank=p, scores=None, ld_scores=0)
    a.update(over)
    return lib.sagnn_candidate_rank_f32(*a.values(), None)


def test_candidate_rank_rejects_every_invalid_argument():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    cases = [(dict(**{k: None}), -1, "null u, i, uids, cand, target or rank")
             for k in ("U", "I", "uids", "cand", "target", "rank")]
    cases += [
        (dict(S=None), -1, "s and a go together"), (dict(A=None), -1, "s and a go together"),
        (dict(d=24, ldu=24, ldi=24, lds=24, lda=24), -2, "d = 24"), (dict(d=0), -2, "d = 0"),
        (dict(d=260, ldu=260, ldi=260, lds=260, lda=260), -2, "d = 260"), (dict(d=2), -2, "d = 2"),
        (dict(C=0, ldc=0), -5, "c = 0"), (dict(C=-1), -5, "c = -1"), (dict(C=8193, ldc=8193), -5, "c = 8193"),
        (dict(B=-1), -5, "n_rows = -1"), (dict(B=1 << 31), -5, "n_rows"),
        (dict(ldc=999), -5, "ldc = 999 < c = 1000"),
        (dict(scores=p, ld_scores=999), -5, "ld_scores = 999 < c = 1000"),
        (dict(ldu=66), -3, "strides"), (dict(ldi=65), -3, "strides"), (dict(lds=62), -3, "strides"),
        (dict(lda=63), -3, "strides"), (dict(ldu=60), -5, ">= d"), (dict(lda=32), -5, ">= d"),
        (dict(U=p + 4), -3, "16-byte aligned"), (dict(I=p + 8), -3, "16-byte aligned"),
        (dict(S=p + 4), -3, "16-byte aligned"), (dict(A=p + 12), -3, "16-byte aligned"),
    ]
    for over, code, text in cases:
        assert _rank(lib, p, **over) == code, over
        assert text in _lib.last_error().lower(), (over, _lib.last_error())
    # without the head term S / A / lds / lda are not read; the limits on C are inclusive; no row: nothing to do
    assert _rank(lib, p, S=None, A=None, lds=3, lda=1, B=0) == 0
    assert _rank(lib, p, C=8192, ldc=8192, B=0) == 0 and _rank(lib, p, C=1, ldc=1, B=0) == 0


def _random_case(rng, B, C, n_items):
    scores = rng.integers(-3, 4, size=(B, C)).astype(np.float32)             # many ties
    scores[rng.random((B, C)) < 0.1] = np.nan
    scores[rng.random((B, C)) < 0.05] = -np.inf
    scores[rng.random(B) < 0.1] = np.nan                                     # all-NaN rows
    cand = rng.integers(0, n_items, size=(B, C))
    target = cand[np.arange(B), rng.integers(0, C, size=B)]                  # a copy somewhere, often several
    absent = rng.random(B) < 0.15
    target[absent] = n_items + 1                                             # no copy
    target[rng.random(B) < 0.05] = -1
    return scores, cand, target


def test_restatement_matches_calcRes():
    from sa_gnn_amd.model import Recommender
    rng = np.random.default_rng(4)
    for trial in range(40):
        B, C = int(rng.integers(1, 30)), int(rng.integers(1, 60))
        scores, cand, target = _random_case(rng, B, C, n_items=int(rng.integers(2, 12)))
        # the target's copies all NaN: the best copy sits at -inf behind every number
        scores[0, cand[0] == target[0]] = np.nan
        rank = R.rank_by_sort(scores, cand, target)
        tst = [None if t < 0 else int(t) for t in target]
        for shoot in (1, 3, 10, C + 1):
            got = Recommender.calcRes(scores, tst, list(cand), shoot=shoot)
            want = []
            for k in (shoot, 5, 20):
                hit = (rank >= 0) & (rank < k)
                want += [float(hit.sum()), float((1.0 / np.log2(rank[hit] + 2)).sum())]
            assert got == tuple(want), (trial, shoot)
        # row by row: calcRes counts a hit at shoot = rank + 1 and none at shoot = rank
        for b in range(B):
            one = lambda k: Recommender.calcRes(scores[b:b + 1], tst[b:b + 1], [cand[b]], shoot=k)[0]
            if rank[b] < 0:
                assert one(C + 1) == 0.0, (trial, b)
            else:
                assert one(int(rank[b]) + 1) == 1.0 and one(int(rank[b])) == 0.0, (trial, b, rank[b])


@pytest.fixture
def args_restored():
    from sa_gnn_amd.Params import args
    saved = dict(vars(args))
    yield args
    vars(args).clear()
    vars(args).update(saved)


def _rec(seqs, n_items, tst, test_dict):
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.model import Recommender
    U = len(seqs)
    h = DataHandler.from_memory([sp.csr_matrix((U, n_items)), [sp.csr_matrix((U, n_items))], None], seqs, tst, test_dict)
    rec = Recommender.__new__(Recommender)
    rec.handler, rec.device = h, torch.device("cpu")
    return rec, h


def _dataset(seed, U=23, I=17, testSize=6):
    rng = np.random.default_rng(seed)
    seqs = [list(rng.integers(0, I, size=int(rng.integers(1, 12)))) for _ in range(U)]
    tst = [int(rng.integers(0, I)) if u % 4 else None for u in range(U)]
    test_dict = {u + 1: [int(v) for v in rng.integers(1, I + 1, size=testSize + 2)] for u in range(U)}
    return seqs, I, tst, test_dict


@pytest.mark.parametrize("test_mode", [True, False])
@pytest.mark.parametrize("pos_length", [4, 200])
def test_evaluator_tables_equal_the_host_batches(args_restored, test_mode, pos_length):
    from sa_gnn_amd.model import DeviceEvaluator
    args = args_restored
    seqs, I, tst, test_dict = _dataset(7)
    rec, h = _rec(seqs, I, tst, test_dict)
    args.batch, args.pos_length, args.testSize, args.test = 5, pos_length, 6, test_mode
    E = DeviceEvaluator(rec)
    ids = h.tstUsrs
    assert E.n == len(ids) and E.users.tolist() == list(ids)
    assert E.cand.shape == (len(ids), args.testSize) and E.cand.dtype == np.int32
    flat, _ = rec._flat_sequences()
    assert len(E.chunks) == -(-len(ids) // args.batch)
    for c, st in enumerate(range(0, len(ids), args.batch)):
        bat = np.asarray(ids[st:st + args.batch])
        _, iLocs, temTst, tstLocs, sequence, mask, _, val_list = rec.sampleTestBatch(bat)
        target = temTst if args.test else val_list
        assert E.cand[st:st + len(bat)].tolist() == np.stack(tstLocs).tolist()
        assert E.target[st:st + len(bat)].tolist() == [int(t) for t in target[:len(bat)]]
        st_, nb, rowptr, items, pos = E.chunks[c]
        assert (st_, nb) == (st, len(bat))
        for got, want in zip((rowptr, items, pos), rec._masked_sum_csr(sequence, mask)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert len(rowptr) == args.batch + 1                                  # the host's padded batch
        _, _, start, seq_end = rec._test_sequences(bat)
        for r in range(len(bat)):
            a, e = E.excl_rowptr[st + r], E.excl_rowptr[st + r + 1]
            assert E.excl_items[a:e].tolist() == sorted(flat[start[r]:seq_end[r]].tolist())
    ops.check_exclusions(E.excl_rowptr, E.excl_items, E.n, I)


def test_evaluator_rejects_what_it_cannot_rank(args_restored):
    from sa_gnn_amd.model import DeviceEvaluator
    args = args_restored
    args.batch, args.pos_length, args.testSize, args.test = 5, 8, 6, True
    seqs, I, tst, test_dict = _dataset(8)
    DeviceEvaluator(_rec(seqs, I, tst, test_dict)[0])                        # the valid set builds
    for bad in (0, I + 1):                                                   # 1-indexed ids outside [1, I]
        td = dict(test_dict)
        td[2] = list(td[2])
        td[2][3] = bad
        with pytest.raises(ValueError, match=f"candidate {bad} of user 2"):
            DeviceEvaluator(_rec(seqs, I, tst, td)[0])
    td = dict(test_dict)
    td[2] = td[2][:args.testSize - 2]
    with pytest.raises(ValueError, match="testSize - 1"):
        DeviceEvaluator(_rec(seqs, I, tst, td)[0])
    for bad in (I, -3):
        t2 = list(tst)
        t2[1] = bad
        with pytest.raises(ValueError, match=f"target of test user 1 is {bad}"):
            DeviceEvaluator(_rec(seqs, I, t2, test_dict)[0])
    args.test = False
    s2 = [list(q) for q in seqs]
    s2[3] = []
    rec, _ = _rec(s2, I, tst, test_dict)
    rec.handler.sequence = s2
    with pytest.raises(ValueError, match="user 3 has an empty sequence"):
        DeviceEvaluator(rec)
    args.test = True
    DeviceEvaluator(rec)                                                     # the test target does not need one
    args.testSize = 8193
    with pytest.raises(ValueError, match="testSize = 8193"):
        DeviceEvaluator(rec)


def test_exclusion_csr_is_checked_once_and_sliced_without_copies():
    with pytest.raises(ValueError, match="monotone"):
        ops.ExclusionCSR(np.array([0, 2, 1, 4]), np.array([1, 3, 4, 5]), 3, 10, "cpu")
    with pytest.raises(ValueError, match="outside"):
        ops.ExclusionCSR(np.array([0, 2, 2, 4]), np.array([1, 3, 4, 10]), 3, 10, "cpu")
    with pytest.raises(ValueError, match="ascending"):
        ops.ExclusionCSR(np.array([0, 2, 2, 4]), np.array([3, 1, 4, 5]), 3, 10, "cpu")
    ex = ops.ExclusionCSR(np.array([0, 2, 2, 5]), np.array([3, 3, 0, 4, 9]), 3, 10, "cpu")
    assert ex.rowptr.dtype == torch.int32 and ex.items.tolist() == [3, 3, 0, 4, 9]
    v = ex.rows(1, 3)
    assert v.n_rows == 2 and v.rowptr.tolist() == [2, 2, 5] and v.items.data_ptr() == ex.items.data_ptr()
    with pytest.raises(ValueError, match="outside"):
        ex.rows(2, 4)
    empty = ops.ExclusionCSR(np.zeros(3, np.int64), np.zeros(0, np.int64), 2, 10, "cpu")
    assert empty.items.numel() == 1                                          # a valid pointer, never read
    # score_topk refuses a CSR of another shape before any device work
    with pytest.raises(ValueError, match="ExclusionCSR of 3 rows"):
        ops.score_topk(torch.zeros((2, 64)), torch.zeros((10, 64)), 5, excl=ex)


def test_evaluator_flag():
    from sa_gnn_amd.Params import parse_args
    assert parse_args([]).evaluator == "host"
    assert parse_args(["--evaluator", "device"]).evaluator == "device"
    with pytest.raises(SystemExit):
        parse_args(["--evaluator", "gpu"])
