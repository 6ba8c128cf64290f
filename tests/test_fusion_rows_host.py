"""CPU suite of --fusion_rows: the flag, the argument checks of the row-subset entries (sagnn_rows_mark_i32,
sagnn_rows_mark_seg_i32, sagnn_rows_compact_i32, sagnn_rows_gather_f32, sagnn_rows_scatter_f32) and the numpy
reference of the rows a host-sampled batch touches, which the GPU suite compares the device compaction against.
Every library call here is rejected before any device work, so no GPU is needed."""
import ctypes

import numpy as np
import pytest

import fusion_rows_ref as R
from sa_gnn_amd import Params, _lib


@pytest.fixture(scope="module")
def buf():
    b = (ctypes.c_float * 4096)()
    return b, ctypes.addressof(b)


def _check(fn, lib, p, cases):
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, over
        assert text in _lib.last_error().lower(), (over, _lib.last_error())


def _mark(lib, p, **over):
    a = dict(ids=p, n=10, N=100, flags=p)
    a.update(over)
    return lib.sagnn_rows_mark_i32(*a.values(), None)


def _mark_seg(lib, p, **over):
    a = dict(seq=p, nflat=10, segb=p, segl=p, ns=4, P=6, N=100, flags=p)
    a.update(over)
    return lib.sagnn_rows_mark_seg_i32(*a.values(), None)


def _compact(lib, p, **over):
    a = dict(flags=p, N=100, rows=p, cap=50, count=p, ws=p, ws_bytes=1024)
    a.update(over)
    return lib.sagnn_rows_compact_i32(*a.values(), None)


def _gather(lib, p, **over):
    a = dict(x=p, ld_n=64, ld_t=6400, N=100, t=3, d=64, rows=p, cap=50, count=None, out=p)
    a.update(over)
    return lib.sagnn_rows_gather_f32(*a.values(), None)


def _scatter(lib, p, **over):
    a = dict(src=p, rows=p, cap=50, count=p, t=3, d=64, dst=p, ld_n=64, ld_t=6400, N=100)
    a.update(over)
    return lib.sagnn_rows_scatter_f32(*a.values(), None)


def test_fusion_rows_flag():
    assert Params.parse_args([]).fusion_rows == "all"
    assert Params.parse_args(["--fusion_rows", "batch"]).fusion_rows == "batch"
    assert Params.parse_args(["--fusion_rows", "all"]).fusion_rows == "all"
    for bad in ("none", "Batch", ""):
        with pytest.raises(SystemExit):
            Params.parse_args(["--fusion_rows", bad])


def test_mark_entries_reject_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    _check(_mark, lib, p, [(dict(ids=None), -1, "null pointer"), (dict(flags=None), -1, "null pointer"),
                           (dict(n=-1), -5, "negative count"), (dict(N=-1), -5, "n_rows = -1"),
                           (dict(N=1 << 31), -5, "n_rows")])
    _check(_mark_seg, lib, p, [(dict(**{k: None}), -1, "null pointer") for k in ("seq", "segb", "segl", "flags")] + [
        (dict(nflat=-1), -5, "negative count"), (dict(ns=-1), -5, "negative count"), (dict(P=-1), -5, "negative count"),
        (dict(N=-1), -5, "n_rows = -1"), (dict(N=1 << 31), -5, "n_rows")])


def test_compact_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    need = lib.sagnn_rows_compact_workspace_bytes(100)
    assert need == 2 * 4 and lib.sagnn_rows_compact_workspace_bytes(15_000_000) == (15_000_000 // 4096 + 2) * 4
    _check(_compact, lib, p, [(dict(**{k: None}), -1, "null pointer") for k in ("flags", "rows", "count")] + [
        (dict(N=-1), -5, "n_rows = -1"), (dict(N=1 << 31), -5, "n_rows"),
        (dict(cap=-1), -5, "negative count"), (dict(cap=0), -5, "cap = 0, need >= 1"),
        (dict(cap=101), -5, "cap = 101 > n_rows = 100"),
        (dict(flags=p + 4), -3, "16-byte aligned"),
        (dict(ws=None), -6, "workspace"), (dict(ws_bytes=need - 1), -6, "workspace"),
    ])


@pytest.mark.parametrize("fn,ptrs", [(_gather, ("x", "rows", "out")), (_scatter, ("src", "rows", "count", "dst"))])
def test_gather_scatter_reject_every_invalid_argument(buf, fn, ptrs):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 66, 260)]
    cases += [(dict(t=0), -2, "t = 0"), (dict(t=-1), -2, "t = -1")]
    cases += [(dict(N=-1), -5, "n_rows = -1"), (dict(N=1 << 31), -5, "n_rows"), (dict(cap=-1), -5, "negative count"),
              (dict(cap=101), -5, "cap = 101 > n_rows = 100")]
    cases += [(dict(ld_n=60), -5, "ld_n >= d"), (dict(ld_t=-4), -5, "ld_t >= 0")]
    cases += [(dict(ld_n=66), -3, "16-byte aligned"), (dict(ld_t=6402), -3, "16-byte aligned")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in ptrs if k not in ("rows", "count")]
    _check(fn, lib, p, cases)


def test_touched_rows_reference_on_a_hand_made_batch():
    batch = {"uids": [3, 3, 1, 1], "iids": [7, 7, 2, 9], "suids": [[5, 5], [], [1, 1, 3, 3]],
             "siids": [[0, 4], [], [4, 8, 8, 11]], "sequence": [[0, 0, 6, 2], [0, 9, 9, 10]],
             "mask": [[0, 0, 1, 1], [0, 1, 1, 1]]}
    src = R.touched_sources(batch)
    assert src["items"]["sequence"].tolist() == [6, 2, 9, 9, 10]
    users, items, caps = R.touched_rows(batch, 6, 12)
    assert users.tolist() == [1, 3, 5]
    assert items.tolist() == [0, 2, 4, 6, 7, 8, 9, 10, 11]
    assert caps == (min(6, 4 + 2 + 4), min(12, 4 + 2 + 4 + 5))
    # segments read as sagnn_seq_sum_f32 reads them: at most P entries from seg_begin
    flat = np.arange(20, 40)
    assert R.segment_items(flat, [0, 5, 12], [3, 0, 9], 4).tolist() == [20, 21, 22, 32, 33, 34, 35]


def test_touched_rows_reference_on_a_host_sampled_batch():
    """On a batch of the host samplers: every id of every list is in its side's set, the sets hold nothing else, they
    are ascending and unique, and the host-known capacities bound them."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    saved = {k: getattr(args, k, None) for k in ("graphNum", "batch", "pos_length", "pred_num", "sslNum", "test", "user",
                                                 "item")}
    try:
        args.graphNum, args.batch, args.pos_length, args.pred_num, args.sslNum, args.test = 2, 16, 12, 2, 3, True
        U, I = 70, 60
        np.random.seed(7)
        tmt = synthetic.make_trn_mat_time(U, I, [700, 650])
        seq = synthetic.make_sequence(tmt)
        rng = np.random.default_rng(2)
        h = DataHandler.from_memory(tmt, seq, [int(rng.integers(0, I)) if u % 2 else None for u in range(U)], None)
        args.user, args.item = U, I
        rec = Recommender.__new__(Recommender)
        rec.handler = h
        bat = np.random.permutation(U)[:args.batch]
        b = rec._host_train_batch(bat)
        users, items, (cap_u, cap_i) = R.touched_rows(b, U, I)
        src = R.touched_sources(b)
        for side, rows in (("users", users), ("items", items)):
            assert (np.diff(rows) > 0).all()
            allv = np.concatenate(list(src[side].values()))
            assert set(rows.tolist()) == set(allv.tolist())
            for name, v in src[side].items():
                assert np.isin(v, rows).all(), name
        assert set(users.tolist()) <= set(bat.tolist())          # users are the batch's own users
        assert len(users) <= cap_u and len(items) <= cap_i
        assert len(src["items"]["sequence"]) == int((np.asarray(b["mask"]) != 0).sum())
    finally:
        for k, v in saved.items():
            setattr(args, k, v)
