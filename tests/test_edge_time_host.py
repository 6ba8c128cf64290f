"""Host suite of the time-aware messages (--edgeTime slot): the buckets of graph.py against the restated
timeProcess of edge_time_ref, the rule for merged edges, the time-adjoint arrays, the limits and the flags. No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import edge_time_ref as R

T0 = 2 ** 31 - 3 * R.DAY            # timestamps on both sides of 2^31: int32 arithmetic would wrap


def _mat(entries, shape):
    """A CSR keeping the stored entries [(user, item, timestamp)] as they are, duplicates included."""
    entries = sorted(entries, key=lambda e: e[0])
    rows = np.array([e[0] for e in entries], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=shape[0]))])
    return sp.csr_matrix((np.array([e[2] for e in entries], np.int64), np.array([e[1] for e in entries], np.int64), rowptr),
                         shape=shape)


def _mats():
    rng = np.random.default_rng(0)
    ent = [(int(u), int(i), int(T0 + rng.integers(0, 9 * R.DAY))) for u, i in zip(*np.nonzero(rng.random((11, 7)) < 0.4))]
    ent = [e for e in ent if e[:2] != (3, 2)]
    ent += [(3, 2, T0 + 8 * R.DAY + 5), (3, 2, T0 + R.DAY), (3, 2, T0 + 4 * R.DAY)]     # (3, 2) three times, the latest first
    return [_mat(ent, (11, 7)), sp.csr_matrix((11, 7), dtype=np.int64), _mat([(0, 0, T0), (10, 6, T0 + 9 * R.DAY - 1)], (11, 7))]


@pytest.mark.parametrize("slot", [1, 2, 0.5])
def test_buckets_equal_the_restated_time_process_near_2_31(slot):
    from sa_gnn_amd import graph
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    mats = _mats()
    mi, max_time = R.time_process([m for m in mats if m.nnz], slot)
    assert mi == T0 and max(int(m.data.max()) for m in mats if m.nnz) > 2 ** 31
    old = args.slot
    try:
        args.slot = slot
        assert DataHandler.timeProcess(None, mats) == (mi, max_time)
    finally:
        args.slot = old
    for m in mats:
        t = sp.coo_matrix(m).data
        got = graph.edge_buckets(t, mi, slot)
        assert got.dtype == np.int64 and list(got) == [R.bucket(x, mi, slot) for x in t]
    assert max_time == int(np.ceil(9 / slot))
    with pytest.raises(ValueError, match="before"):
        graph.edge_buckets([mi - 1], mi, slot)


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_merged_edges_take_the_latest_bucket_and_unmerged_duplicates_keep_theirs(norm):
    from sa_gnn_amd import graph
    mats = _mats()
    mi, _ = R.time_process([m for m in mats if m.nnz], 1)
    for m in mats:
        b_fw, b_tp = graph.pair_buckets(m, mi, 1, norm)
        assert list(b_fw) == R.pattern_buckets(m, mi, 1, "user", norm == "sym")
        assert list(b_tp) == R.pattern_buckets(m, mi, 1, "item", True)
        # in the order of the arrays the plans are built from
        if norm == "none":
            rp, ci = graph.csr_arrays(m)
            rp_t, ci_t = graph.csr_arrays(graph.transpose(m))
        else:
            rp, ci = graph.merged_arrays(m)
            users = np.repeat(np.arange(m.shape[0]), np.diff(rp))
            order = np.argsort(ci, kind="stable")
            rp_t, ci_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=m.shape[1]))]), users[order]
        assert len(b_fw) == len(ci) and len(b_tp) == len(ci_t)
        if m.nnz:
            lt = R.latest(m)
            items = np.repeat(np.arange(m.shape[1]), np.diff(rp_t))
            assert [R.bucket(lt[(int(u), int(i))], mi, 1) for u, i in zip(ci_t, items)] == list(b_tp)
    # the duplicated pair: three stored copies in buckets that differ; merged, the latest (8)
    m = mats[0]
    rp, ci = graph.csr_arrays(m)
    b_fw, b_tp = graph.pair_buckets(m, mi, 1, "none")
    copies = sorted(b_fw[rp[3]:rp[4]][ci[rp[3]:rp[4]] == 2])
    assert copies == [1, 4, 8]
    rp_t, ci_t = graph.csr_arrays(graph.transpose(m))
    assert b_tp[rp_t[2]:rp_t[3]][ci_t[rp_t[2]:rp_t[3]] == 3] == [8]
    # the phantom edge of the empty matrix
    assert [list(b) for b in graph.pair_buckets(mats[1], mi, 1, norm)] == [[0], [0]]


def test_time_adjoint_is_the_stable_bucket_sort_of_row_and_weight():
    from sa_gnn_amd import ops
    rng = np.random.default_rng(1)
    deg = rng.integers(0, 9, 30)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    buckets = rng.integers(0, 6, rowptr[-1])
    buckets[buckets == 4] = 5                                                    # an empty bucket
    w = rng.random(rowptr[-1]).astype(np.float32)
    for weights in (None, w):
        got = ops.time_adjoint_arrays(rowptr, buckets, 7, weights)
        want = R.time_adjoint(rowptr, buckets, 7, weights)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[2] is None and want[2] is None) or np.array_equal(got[2], want[2])
    assert got[0][5] == got[0][4] and got[0][7] == rowptr[-1]


def test_a_table_of_65536_rows_is_refused_and_the_message_names_slot():
    from sa_gnn_amd import graph, ops
    assert ops.check_n_buckets(65535) == 65535
    for m in (65536, 0):
        with pytest.raises(ValueError, match="--slot"):
            ops.check_n_buckets(m)
    far = _mat([(0, 0, T0), (1, 1, T0 + 65534 * R.DAY)], (2, 2))                 # buckets 0 .. 65534: M = 65536
    with pytest.raises(ValueError, match="--slot"):
        graph.interval_pair(far, None, time=(T0, 1))
    with pytest.raises(ValueError, match="--slot"):
        graph.interval_pair(far, None, time=(T0, 1, 65536))
    # host-side checks of a plan's buckets (a host-only plan takes none, like weights)
    rp, ci = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
    with pytest.raises(TypeError, match="uint16"):
        ops.SpmmPlan(rp, ci, 1, 2, buckets=np.array([0, 1], np.int32), n_buckets=2)
    with pytest.raises(ValueError, match="expected 2 values"):
        ops.SpmmPlan(rp, ci, 1, 2, buckets=np.array([0], np.uint16), n_buckets=2)
    with pytest.raises(ValueError, match="outside"):
        ops.SpmmPlan(rp, ci, 1, 2, buckets=np.array([0, 2], np.uint16), n_buckets=2)
    with pytest.raises(ValueError, match="together"):
        ops.SpmmPlan(rp, ci, 1, 2, buckets=np.array([0, 1], np.uint16))
    with pytest.raises(ValueError, match="host-only"):
        ops.SpmmPlan(rp, ci, 1, 2, buckets=np.array([0, 1], np.uint16), n_buckets=2)


def test_flag_parsing():
    from sa_gnn_amd import Params
    assert Params.parse_args([]).edgeTime == "none" and Params.args.edgeTime == "none"
    ns = Params.parse_args(["--edgeTime", "slot", "--slot", "7"])
    assert ns.edgeTime == "slot" and ns.slot == 7.0
    with pytest.raises(SystemExit):
        Params.parse_args(["--edgeTime", "day"])
    text = Params.build_parser().format_help()
    assert "dead code only" not in text.split("--slot")[1].split("--graphSampleN")[0] and "days per time bucket" in text


def _handler(monkeypatch, **flags):
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    for k, v in dict(graphNum=2, gnn_layer=2, latdim=32, **flags).items():
        monkeypatch.setattr(args, k, v)
    tmt = synthetic.make_trn_mat_time(20, 15, [60, 50])
    return DataHandler.from_memory(tmt, synthetic.make_sequence(tmt)), args


def test_refused_with_edge_dropout_and_on_the_interval_parallel_path(monkeypatch):
    from sa_gnn_amd import parallel
    from sa_gnn_amd.model import Recommender
    handler, args = _handler(monkeypatch, edgeTime="slot", edgeKeepRate=0.5)
    assert handler.maxTime > 1
    with pytest.raises(ValueError, match="edgeKeepRate"):
        Recommender("cpu", handler).prepareModel()
    monkeypatch.setattr(args, "edgeKeepRate", 1.0)
    with pytest.raises(ValueError, match="edgeTime"):
        parallel.make_sharding(args.graphNum, 1, 0)
    monkeypatch.setattr(args, "edgeTime", "day")
    with pytest.raises(ValueError, match="edgeTime"):
        Recommender("cpu", handler).prepareModel()
    monkeypatch.setattr(args, "edgeTime", "none")
    parallel.make_sharding(args.graphNum, 1, 0)


def test_edge_time_none_keeps_max_time_1_and_the_registry(monkeypatch):
    """Under none the handler runs no timeProcess and the model registers what it registered: timeEmbed [2, d] and
    2 T L weights [d, d] named as before, all L2-regularised (ours() on the CPU registry; no GPU call is reached)."""
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    handler, args = _handler(monkeypatch, edgeTime="none")
    assert handler.maxTime == 1 and handler.timeMin == 0
    rec = Recommender("cpu", handler)
    rec.maxTime = handler.maxTime
    NNs.reset("cpu")
    monkeypatch.setattr(Recommender, "forward", lambda self: (None, None))
    rec.ours()
    assert tuple(NNs.params["timeEmbed"].shape) == (2, 32)
    names = [k for k in NNs.params if k.startswith("defaultParamName")]
    assert names[:8] == ["defaultParamName%d" % i for i in range(1, 9)] and len(rec.time_weights) == 8
    assert all(NNs.params[n] is w and n in NNs.regParams and tuple(w.shape) == (32, 32) for n, w in zip(names, rec.time_weights))
    assert rec.time_tables() is None
    # under slot the table grows to maxTime + 1 rows and TE is one batched product in registration order
    monkeypatch.setattr(args, "edgeTime", "slot")
    handler.prepareGlobalData()
    assert handler.maxTime > 1
    rec.maxTime = handler.maxTime
    NNs.reset("cpu")
    rec.ours()
    te = rec.time_tables()
    assert tuple(te.shape) == (2, 2, 2, handler.maxTime + 1, 32)
    assert np.allclose(te[1, 0, 1].detach().numpy(), (rec.timeEmbed @ rec.time_weights[5]).detach().numpy(), atol=1e-6)
