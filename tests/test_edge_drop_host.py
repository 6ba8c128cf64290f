"""CPU suite of the edge dropout of the interval graphs (--edgeKeepRate, ops.EdgeDrop, sagnn_spmm_drop_f32 and the GNN stack
entries under SAGNN_EDGES_DROP): the threshold and the mask restated in numpy (edge_drop_ref), the entries' argument checks
(all refused before any device work, so no GPU is needed), the flag's range check and what trainEpoch draws from np.random."""
import ctypes

import numpy as np
import pytest
import torch

import edge_drop_ref as R
from sa_gnn_amd import _lib, ops

SEED = 0x5EED0FED6E5       # picked once; the data below are fixed, so the statistical checks are deterministic


@pytest.mark.parametrize("keep,want", [(0.5, 1 << 31), (0.9, 3865470566), (1.0 - 2.0 ** -30, (1 << 32) - 4),
                                       (1.0, (1 << 32) - 1)])
def test_threshold(keep, want):
    assert R.threshold(keep) == want
    e = ops.EdgeDrop(SEED, 3, keep)
    assert e.threshold == want and e.struct().keep_threshold == want
    assert e.scale == float(np.float32(1.0) / np.float32(keep)) and e.struct().scale == np.float32(e.scale)
    assert (e.struct().seed, e.struct().step) == (SEED, 3)


def test_threshold_is_capped_and_the_rate_is_checked():
    assert R.threshold(1.0) == 2 ** 32 - 1 and R.threshold(np.nextafter(1.0, 0.0)) <= 2 ** 32 - 1
    for bad in (0.0, -0.1, 1.5, float("nan"), 2.0 ** -40):
        with pytest.raises(ValueError):
            ops.EdgeDrop(1, 0, bad)
    with pytest.raises(ValueError):
        ops.EdgeDrop(1, 1 << 32, 0.5)
    assert ops.edge_tag(5, 3, 1) == R.tag(5, 3, 1) == (5 << 8) | (3 << 1) | 1


def _pairs(n):
    j = np.arange(n, dtype=np.int64)        # n distinct (user, item) pairs
    return j % 48653, (j // 48653) * 7919 + (j * 31) % 7919


@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_kept_fraction(keep):
    n = 200_000
    u, i = _pairs(n)
    assert len(set(zip(u.tolist(), i.tolist()))) == n
    frac = R.keep_mask(SEED, 11, 2, 1, 0, u, i, keep).mean()
    assert abs(frac - keep) <= 4.0 * np.sqrt(keep * (1.0 - keep) / n), frac


def test_draws_of_different_tags_and_steps_differ():
    u, i = _pairs(4096)
    base = R.keep_mask(SEED, 11, 2, 1, 0, u, i, 0.5)
    assert np.array_equal(base, R.keep_mask(SEED, 11, 2, 1, 0, u, i, 0.5))
    for other in (R.keep_mask(SEED, 11, 2, 1, 1, u, i, 0.5), R.keep_mask(SEED, 11, 2, 2, 0, u, i, 0.5),
                  R.keep_mask(SEED, 11, 3, 1, 0, u, i, 0.5), R.keep_mask(SEED, 12, 2, 1, 0, u, i, 0.5),
                  R.keep_mask(SEED + 1, 11, 2, 1, 0, u, i, 0.5)):
        # independent fair draws agree on about half of 4096 edges: 2048 +- 4 sigma = 128
        assert abs(int((other == base).sum()) - 2048) <= 128
    # the mask of a pair does not depend on its position among the others
    p = np.random.default_rng(0).permutation(u.size)
    assert np.array_equal(R.keep_mask(SEED, 11, 2, 1, 0, u[p], i[p], 0.5), base[p])


# ---- the C entries: every bad sagnn_edge_drop is refused before anything else is looked at ---------------------------
def _drop(**over):
    a = dict(seed=SEED, step=1, keep_threshold=1 << 31, scale=2.0)
    a.update(over)
    return _lib.EdgeDropArgs(a["seed"], a["step"], a["keep_threshold"], a["scale"])


def _spmm(lib, p, drop, plan=None):
    e = _lib.SpmmEpilogue()
    return lib.sagnn_spmm_drop_f32(plan, p, 64, 64, ctypes.byref(e), drop, 5, 1, None, 0, None)


def _gnn_args(p, drop, L, k=0):
    """A sagnn_gnn_args with edges = DROP and every operand given; drop: None or a ctypes.byref of the struct."""
    a = _lib.GnnArgs(d=64, n_layers=L, leaky=0.5, edges=_lib.EDGES_DROP, interval=k)
    if drop is not None:
        a.drop = ctypes.pointer(drop._obj)
    for side in (a.user, a.item):
        side.in_, side.ld_in, side.out, side.ld_out, side.scratch, side.mask = p, 64, p, 64, p, p
    return ctypes.byref(a)


def _interval(lib, p, drop, fn="sagnn_gnn_interval_f32", L=2, k=0):
    return getattr(lib, fn)(None, None, _gnn_args(p, drop, L, k), None)


def _stack(lib, p, drop, fn="sagnn_gnn_stack_f32", L=2):
    return getattr(lib, fn)(None, _gnn_args(p, drop, L), None)


BAD = [(dict(keep_threshold=0), "keep_threshold = 0"), (dict(scale=0.0), "scale"), (dict(scale=-2.0), "scale"),
       (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale")]


def test_drop_entries_exist_and_reject_bad_arguments():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    calls = [lambda d: _spmm(lib, p, d),
             lambda d: _interval(lib, p, d), lambda d: _interval(lib, p, d, "sagnn_gnn_interval_bwd_f32"),
             lambda d: _stack(lib, p, d), lambda d: _stack(lib, p, d, "sagnn_gnn_stack_bwd_f32")]
    for call in calls:
        assert call(None) == -1 and "sagnn_edge_drop is null" in _lib.last_error().lower()
        for over, text in BAD:
            assert call(ctypes.byref(_drop(**over))) == -5, over
            assert text in _lib.last_error().lower(), (over, _lib.last_error())
        # a good struct gets as far as the next check: the NULL plan / batch
        assert call(ctypes.byref(_drop())) == -1 and "edge drop" not in _lib.last_error().lower()
    good = ctypes.byref(_drop())
    for fn in ("sagnn_gnn_interval_f32", "sagnn_gnn_interval_bwd_f32"):
        assert _interval(lib, p, good, fn, L=128) == -5 and "n_layers = 128" in _lib.last_error()
        assert _interval(lib, p, good, fn, L=127) == -1
        assert _interval(lib, p, good, fn, k=1 << 23) == -5 and "interval" in _lib.last_error()
        assert _interval(lib, p, good, fn, k=-1) == -5 and "interval" in _lib.last_error()
        assert _interval(lib, p, good, fn, k=(1 << 23) - 1) == -1
    for fn in ("sagnn_gnn_stack_f32", "sagnn_gnn_stack_bwd_f32"):
        assert _stack(lib, p, good, fn, L=128) == -5 and "n_layers = 128" in _lib.last_error()


def test_spmm_drop_on_a_host_only_plan_checks_the_drop_first():
    """A host-only plan (no device touched): a bad sagnn_edge_drop is reported ahead of the plan's own refusal."""
    plan = ops.SpmmPlan(np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), 2, 2, device=None)
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert _spmm(lib, p, ctypes.byref(_drop(keep_threshold=0)), plan.handle) == -5
    assert "keep_threshold" in _lib.last_error()
    assert _spmm(lib, p, ctypes.byref(_drop()), plan.handle) == -5 and "host-only" in _lib.last_error()


# ---- the flag ---------------------------------------------------------------------------------------------------------
class _Opt:
    def step(self, grads):
        pass


def _stub_recommender(n_users):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender

    class Stub(Recommender):          # trainEpoch's own code on the CPU: sampling, loss and optimiser stubbed out
        def __init__(self):
            self.device, self.optimizer, self.seen = torch.device("cpu"), _Opt(), []

        def _host_train_batch(self, batIds):
            return {}

        def _trainable(self):
            return {}

        def train_loss(self, batch, keep_rate=None, edge_keep=None):
            self.seen.append(batch.get("edge_seed"))
            z = torch.zeros(1, requires_grad=True)
            return z * 1.0, z * 2.0

    NNs.reset("cpu")
    args.user, args.trnNum, args.batch, args.sampler = n_users, 40, 16, "host"
    return Stub(), args


@pytest.mark.parametrize("rate", [0.0, 1.5, -0.5])
def test_edge_keep_rate_outside_range_is_refused(rate):
    from sa_gnn_amd import Params
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    assert Params.build_parser().parse_args([]).edgeKeepRate == 1.0
    assert Params.build_parser().parse_args(["--edgeKeepRate", "0.7"]).edgeKeepRate == 0.7
    old = args.edgeKeepRate
    args.edgeKeepRate = rate
    args.user, args.item = 10, 10
    try:
        with pytest.raises(ValueError, match="edgeKeepRate"):
            Recommender("cpu", None).prepareModel()        # refused before the handler or a device is touched
    finally:
        args.edgeKeepRate = old


def test_train_epoch_draws_nothing_extra_from_numpy_with_the_flag_off():
    rec, args = _stub_recommender(100)
    old = args.edgeKeepRate
    try:
        # what the parent path draws in an epoch of the host sampler: the permutation of the users, nothing else
        np.random.seed(7)
        np.random.permutation(100)
        want_next = np.random.random()
        args.edgeKeepRate = 1.0
        np.random.seed(7)
        rec.trainEpoch()
        assert np.random.random() == want_next
        assert rec.seen == [None, None, None]
        # with the flag on: one 63-bit seed per epoch after the permutation, and the step index per batch
        args.edgeKeepRate = 0.5
        np.random.seed(7)
        np.random.permutation(100)
        seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
        want_next = np.random.random()
        rec.seen.clear()
        np.random.seed(7)
        rec.trainEpoch()
        assert np.random.random() == want_next
        assert rec.seen == [(seed, 0), (seed, 1), (seed, 2)]
    finally:
        args.edgeKeepRate = old
