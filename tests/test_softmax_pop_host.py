"""CPU suite of the popularity-weighted candidate softmax (--softmaxNegDist pop): the flags and
prepareModel's refusals, the integer item weights, the argument checks of the new C entries (each rejected before any
device work, so no GPU is needed), and the properties of the restated draw: non-decreasing, run lengths that add up to
n_cand, the exact expected draw count against n_cand w_i / W, and the identity list under equal weights."""
import numpy as np
import pytest
import torch

import softmax_args_host as H
import softmax_pop_ref as P
from sa_gnn_amd import _lib, ops


def test_flags_parse_and_default_to_uniform():
    from sa_gnn_amd import Params
    ns = Params.build_parser().parse_args([])
    assert ns.softmaxNegDist == "uniform" and ns.softmaxNegPow == 0.75
    assert Params.args.softmaxNegDist == "uniform" and Params.args.softmaxNegPow == 0.75
    ns = Params.build_parser().parse_args(["--predLoss", "softmax", "--softmaxNegs", "64", "--softmaxNegDist", "pop",
                                           "--softmaxNegPow", "0.5"])
    assert ns.softmaxNegDist == "pop" and ns.softmaxNegPow == 0.5 and isinstance(ns.softmaxNegPow, float)
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--softmaxNegDist", "zipf"])
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--softmaxNegPow", "much"])
    text = " ".join(Params.build_parser().format_help().lower().split())
    assert "--softmaxnegdist" in text and "--softmaxnegpow" in text and "logq" in text


class _PastTheChecks(Exception):
    pass


def test_prepare_model_refusals(monkeypatch):
    from sa_gnn_amd import model
    from sa_gnn_amd.Params import args

    def stop(*a, **k):
        raise _PastTheChecks()
    monkeypatch.setattr(model.NNs, "reset", stop)      # the first thing prepareModel does after its checks
    for k, v in (("user", 10), ("item", 10)):
        monkeypatch.setattr(args, k, v, raising=False)
    for k, v in (("predLoss", "softmax"), ("fusion_rows", "all"), ("softmaxNegs", 5), ("softmaxNegDist", "pop")):
        monkeypatch.setattr(args, k, v)
    prepare = lambda: model.Recommender("cpu", None).prepareModel()     # noqa: E731
    with pytest.raises(_PastTheChecks):
        prepare()
    monkeypatch.setattr(args, "fusion_rows", "batch")                   # combines with the row subset, as --softmaxNegs
    with pytest.raises(_PastTheChecks):
        prepare()
    monkeypatch.setattr(args, "softmaxNegDist", "zipf")
    with pytest.raises(ValueError, match="--softmaxNegDist zipf: one of"):
        prepare()
    monkeypatch.setattr(args, "softmaxNegDist", "pop")
    monkeypatch.setattr(args, "fusion_rows", "all")
    monkeypatch.setattr(args, "softmaxNegs", 0)
    with pytest.raises(ValueError, match=r"--softmaxNegDist pop needs --predLoss softmax and --softmaxNegs > 0"):
        prepare()
    monkeypatch.setattr(args, "predLoss", "hinge")
    with pytest.raises(ValueError, match=r"--softmaxNegDist pop needs --predLoss softmax and --softmaxNegs > 0"):
        prepare()
    monkeypatch.setattr(args, "predLoss", "softmax")
    monkeypatch.setattr(args, "softmaxNegs", 5)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        monkeypatch.setattr(args, "softmaxNegPow", bad)
        with pytest.raises(ValueError, match="--softmaxNegPow"):
            prepare()
    for good in (0.0, 0.75, 1.0):
        monkeypatch.setattr(args, "softmaxNegPow", good)
        with pytest.raises(_PastTheChecks):
            prepare()
    monkeypatch.setattr(args, "softmaxNegPow", 7.0)                     # read only under pop
    monkeypatch.setattr(args, "softmaxNegDist", "uniform")
    with pytest.raises(_PastTheChecks):
        prepare()
    monkeypatch.setattr(args, "predLoss", "hinge")
    monkeypatch.setattr(args, "softmaxNegs", 0)
    with pytest.raises(_PastTheChecks):
        prepare()


def test_weights_on_degree_zero_a_huge_degree_and_the_total_limit():
    from sa_gnn_amd import model
    deg = np.array([0, 1, 2, 7, 200_000, 2 ** 31 - 1, 0], dtype=np.int64)
    for a in (0.0, 0.5, 0.75, 1.0):
        cum, total = model.pop_cum(deg, a)
        w, rcum, rtot = P.weights(deg, a)
        assert cum.dtype == np.int64 and cum.tolist() == rcum and total == rtot == int(cum[-1])
        assert w[0] == w[-1] == 1 << 20 and min(w) >= 1                # degree 0: (0 + 1)^a = 1
    assert P.weights(deg, 0.0)[0] == [1 << 20] * len(deg)
    assert P.weights(deg, 1.0)[0][5] == (1 << 20) * 2 ** 31             # the huge degree, exact in float64
    assert model.pop_cum(np.array([2 ** 42 - 2]), 1.0)[1] == 2 ** 62 - 2 ** 20
    with pytest.raises(ValueError, match="2\\^62"):
        model.pop_cum(np.array([2 ** 42 - 1]), 1.0)                     # W == 2^62
    with pytest.raises(ValueError, match="2\\^62"):
        model.pop_cum(np.full(4096, 2 ** 31 - 1), 1.0)                  # 4096 x 2^51 = 2^63: caught before int64 wraps
    for bad in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="softmaxNegPow"):
            model.pop_cum(deg, bad)


def test_item_degrees_count_stored_non_zero_entries():
    import scipy.sparse as sp
    from sa_gnn_amd import model
    m = sp.coo_matrix((np.array([1, 1, 0, 2, 1, 1]), (np.array([0, 1, 2, 0, 3, 3]), np.array([0, 0, 1, 3, 3, 3]))), shape=(4, 5))
    assert model.item_degrees(m.tocsr(), 5).tolist() == [2, 0, 0, 2, 0]      # an explicit zero and a duplicate
    assert model.item_degrees(m.tocsr(), 7).tolist() == [2, 0, 0, 2, 0, 0, 0]


def test_weighted_draw_rejects_every_invalid_argument_without_a_device():
    lib = _lib.load()
    buf, p = H.aligned_buffer()

    def f(**o):
        a = dict(cum=p, ni=100, total=1 << 30, n_cand=40, seed=1, step=0, cand=p, bias=p)
        a.update(o)
        return lib.sagnn_sample_strata_w_i32(*a.values(), None)
    for over, code, text in [(dict(ni=0), -5, "n_items"), (dict(ni=1 << 31), -5, "n_items"), (dict(total=0), -5, "total"),
                             (dict(total=1 << 62), -5, "total"), (dict(n_cand=-1), -5, "n_cand"),
                             (dict(n_cand=1 << 31), -5, "n_cand"), (dict(total=39), -5, "n_cand"),
                             (dict(cum=None), -1, "null cum"), (dict(cand=None), -1, "null cand or bias"),
                             (dict(bias=None), -1, "null cand or bias")]:
        assert f(**over) == code, (over, _lib.last_error())
        assert text in _lib.last_error().lower(), (over, _lib.last_error())
    assert f(n_cand=0, cand=None, bias=None) == 0                       # nothing to draw: no launch
    cum = torch.ones(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="cum"):                        # a host tensor: refused before any device call
        ops.sample_strata_weighted(cum, 4, 2, 1, 0)
    del buf


@pytest.mark.parametrize("name", ["fwd", "bwd"])
def test_the_offset_entries_reject_what_the_plain_ones_do_and_a_null_bias(name):
    lib = _lib.load()
    buf, p = H.aligned_buffer()
    for over, code, text in [(dict(bias=None), -1, "null bias"), (dict(cand=None), -1, "null cand"), (dict(Q=None), -1, "q or i"),
                             (dict(n_cand=101), -5, "n_cand"), (dict(d=48, ldq=48, ldi=48), -2, "d = 48"),
                             (dict(inv_temp=0.0), -5, "inv_temp"), (dict(ws_bytes=16), -6, "workspace"),
                             (dict(ldq=66), -3, "ldq")]:
        base = H.softmax_args(p, _lib.SOFTMAX_CAND_BIAS, **over)       # every field by name, the entry's own and the other's
        assert H.call(lib, name == "bwd", base) == code, (over, _lib.last_error())
        assert text in _lib.last_error().lower() and "softmax_loss_candb" in _lib.last_error(), (over, _lib.last_error())
        assert _lib.last_error().startswith("softmax_loss_candb_bwd: " if name == "bwd" else "softmax_loss_candb: ")
    del buf


def test_scatter_rejects_every_invalid_argument_without_a_device():
    lib = _lib.load()
    buf, p = H.aligned_buffer()

    def f(**o):
        a = dict(dIc=p, lddic=64, cand=p, bias=p, n_cand=40, ni=100, d=64, dI=p, lddi=64)
        a.update(o)
        return lib.sagnn_softmax_cand_scatter_f32(*a.values(), None)
    for over, code, text in [(dict(dIc=None), -1, "null"), (dict(cand=None), -1, "null"), (dict(bias=None), -1, "null"),
                             (dict(dI=None), -1, "null"), (dict(d=48), -2, "d = 48"), (dict(ni=0), -5, "n_items"),
                             (dict(n_cand=101), -5, "n_cand"), (dict(n_cand=-1), -5, "n_cand"), (dict(lddic=66), -3, "lddic / lddi"),
                             (dict(lddi=32), -5, ">= d"), (dict(dI=p + 4), -3, "16-byte"), (dict(dIc=p + 8), -3, "16-byte")]:
        assert f(**over) == code, (over, _lib.last_error())
        assert text in _lib.last_error().lower(), (over, _lib.last_error())
    assert f(n_cand=0, dIc=None, cand=None, bias=None) == 0
    del buf


def test_ops_wrappers_check_the_bias_before_any_device_call():
    Q, I = torch.zeros((3, 64)), torch.zeros((10, 64))         # host tensors: a device call would fail differently
    t, cand = torch.zeros(3, dtype=torch.int32), torch.arange(4, dtype=torch.int32)
    with pytest.raises(TypeError, match="device tensor"):
        ops.softmax_loss_cand(Q, I, cand, t, bias=torch.zeros(4))
    with pytest.raises(TypeError, match="device tensor"):
        ops.softmax_loss_cand_bwd(Q, I, cand, t, torch.zeros(3), torch.ones(1), bias=torch.zeros(4))


def _zipf_cum(n_items, a, seed=5, hub=None):
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.zipf(1.3, n_items), 50_000).astype(np.int64)
    if hub is not None:
        deg[hub[0]] = hub[1]
    return P.weights(deg, a)


@pytest.mark.parametrize("n_items,n_cand", [(1, 1), (17, 5), (700, 300), (4099, 64), (300, 300)])
def test_the_restated_draw_is_non_decreasing_and_its_runs_add_up(n_items, n_cand):
    w, cum, W = _zipf_cum(n_items, 0.75)
    for seed, step in ((0, 0), (0x9E3779B97F4A7C15, 3), (2 ** 64 - 1, 2 ** 32 - 1)):
        cand, m, live, bias = P.draw(cum, n_cand, seed, step)
        assert cand.shape == m.shape == live.shape == bias.shape == (n_cand,) and bias.dtype == np.float32
        assert (np.diff(cand) >= 0).all() and cand[0] >= 0 and cand[-1] < n_items
        assert live[0] and np.array_equal(live[1:], np.diff(cand) != 0)         # live = the first position of a run
        assert int(m[live].sum()) == n_cand and not m[~live].any()
        assert np.isfinite(bias[live]).all() and np.isneginf(bias[~live]).all()
        lo = P.strata_bounds(W, n_cand)
        for j in range(n_cand):                                        # each draw inside its stratum's items
            first = int(np.searchsorted(np.asarray(cum), lo[j], side="right"))
            last = int(np.searchsorted(np.asarray(cum), lo[j + 1] - 1, side="right"))
            assert first <= cand[j] <= last
        again = P.draw(cum, n_cand, seed, step)
        assert all(np.array_equal(x, y) for x, y in zip((cand, m, live, bias), again))   # a pure function
    if n_cand >= 64:
        assert not np.array_equal(P.draw(cum, n_cand, 1, 0)[0], P.draw(cum, n_cand, 1, 1)[0])
        assert not np.array_equal(P.draw(cum, n_cand, 1, 0)[0], P.draw(cum, n_cand, 2, 0)[0])
    assert all(len(x) == 0 for x in P.draw(cum, 0, 1, 1))


def test_weighted_draw_sets_counter_word_one_of_the_strata_stream():
    import device_sampler_ref as S
    n_cand, seed, step = 8, 99, 7
    w, cum, W = P.weights([3] * 1000, 1.0)                              # equal weights 4 * 2^20: item = mass // weight
    words = S.philox4x32_10(np.arange(n_cand), 1, step, 0xFFFFFFFF, seed)
    lo = P.strata_bounds(W, n_cand)
    want = [(lo[j] + ((((int(words[0][j]) << 32) | int(words[1][j])) * (lo[j + 1] - lo[j])) >> 64)) // w[0] for j in range(n_cand)]
    assert P.draw(cum, n_cand, seed, step)[0].tolist() == want
    other = S.philox4x32_10(np.arange(n_cand), 0, step, 0xFFFFFFFF, seed)          # the uniform draw's blocks
    assert not np.array_equal(other[0], words[0])


def test_exact_expected_draw_count_agrees_with_the_bias_denominator():
    """E[#draws of i] = sum_j |range_i & stratum_j| / |stratum_j| exactly, against e_i = n_cand w_i / W: the strata
    sizes differ from W / n_cand by less than one unit of mass, so the relative difference is at most n_cand / W.
    Deterministic: no sampling."""
    from fractions import Fraction
    n_items, n_cand = 700, 300
    w, cum, W = _zipf_cum(n_items, 0.75, hub=(300, 200_000))
    worst = Fraction(0)
    for i in range(n_items):
        exact = P.expected_count(cum, n_cand, i)
        e = Fraction(n_cand * w[i], W)
        worst = max(worst, abs(exact - e) / e)
    print(f"worst relative difference {float(worst):.3e}, bound n_cand / W = {n_cand / W:.3e}")
    assert worst <= Fraction(n_cand, W)
    assert sum(P.expected_count(cum, n_cand, i) for i in range(n_items)) == n_cand


@pytest.mark.parametrize("n", [1, 7, 300])
def test_equal_weights_and_every_item_give_the_identity_list_and_zero_biases(n):
    for deg, a in (([0] * n, 0.75), ([4] * n, 1.0), (list(range(n)), 0.0)):
        w, cum, W = P.weights(deg, a)
        cand, m, live, bias = P.draw(cum, n, 12345, 6)
        assert cand.tolist() == list(range(n)) and live.all() and (m == 1).all()
        assert (bias == 0.0).all() and not np.signbit(bias).any()


def test_the_offset_objective_agrees_with_torch_autograd():
    """softmax_loss_pop_np against torch float64 autograd on the differentiable form, a drawn list with repeats, lists
    and a skipped row; and the bias makes the candidate sum the draw-count-weighted one."""
    nq, ni, d, inv_temp, scale = 9, 40, 8, 1.0 / 0.7, 0.31
    rng = np.random.default_rng(2)
    Q, I = rng.standard_normal((nq, d)), rng.standard_normal((ni, d))
    w, cum, W = _zipf_cum(ni, 1.0, seed=3, hub=(11, 400))
    cand, m, live, bias = P.draw(cum, 25, 7, 1)
    assert (m > 1).any()
    target = rng.integers(0, ni, nq)
    target[2], target[3] = -1, cand[m.argmax()]
    lists = [np.sort(rng.integers(0, ni, 6)) for _ in range(nq)]
    lists[4] = np.sort(np.concatenate([lists[4], [cand[m.argmax()]]]))
    ptr, items = np.concatenate([[0], np.cumsum([len(v) for v in lists])]), np.concatenate(lists)
    ref = P.softmax_loss_pop_np(Q, I, cand, bias, target, inv_temp, scale, ptr, items)
    q, i = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(I).requires_grad_(True)
    loss = P.torch_softmax_loss_pop(q, i, target, inv_temp, scale, ref["eligible"], ref["off"])
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(abs(ref["loss"]), 1.0)
    np.testing.assert_allclose(q.grad.numpy(), ref["dQ"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(i.grad.numpy(), ref["dI"], rtol=1e-11, atol=1e-13)
    b = 0                                                               # sum_live exp(z + bias) = sum_draws exp(z) / e
    z = (Q[b] @ I.T) * inv_temp
    ids = [int(c) for c in cand if ref["eligible"][b, c] and c != target[b]]
    by_draw = sum(np.exp(z[c]) / (25 * w[c] / W) for c in ids) + np.exp(z[target[b]])
    assert abs(np.log(by_draw) - ref["lse"][b]) <= 1e-6                 # the biases are float32
