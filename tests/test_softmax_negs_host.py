"""CPU suite of the sampled-candidate softmax loss (--softmaxNegs): the flag, prepareModel's refusals
and the one combination it now lets through, the argument checks of the C entries (each rejected before any device
work, so no GPU is needed), the workspace size, the numpy restatement of the stratified draw and its inclusion
frequencies, and the augmented-list reference against torch float64 autograd on a direct masked logsumexp."""
import numpy as np
import pytest
import torch

import softmax_args_host as H
import softmax_cand_ref as C
import softmax_loss_ref as R
from sa_gnn_amd import _lib, ops


def test_flag_parses_and_defaults_to_the_whole_catalogue():
    from sa_gnn_amd import Params
    ns = Params.build_parser().parse_args([])
    assert ns.softmaxNegs == 0 and Params.args.softmaxNegs == 0
    ns = Params.build_parser().parse_args(["--predLoss", "softmax", "--softmaxNegs", "4096"])
    assert ns.softmaxNegs == 4096 and isinstance(ns.softmaxNegs, int)
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--softmaxNegs", "many"])
    text = " ".join(Params.build_parser().format_help().lower().split())
    assert "--softmaxnegs" in text and text.count("not in the reference") >= 3


class _PastTheChecks(Exception):
    pass


def test_prepare_model_refusals_and_the_combination_it_now_allows(monkeypatch):
    from sa_gnn_amd import model
    from sa_gnn_amd.Params import args

    def stop(*a, **k):
        raise _PastTheChecks()
    monkeypatch.setattr(model.NNs, "reset", stop)      # the first thing prepareModel does after its checks
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    monkeypatch.setattr(args, "predLoss", "softmax")
    monkeypatch.setattr(args, "fusion_rows", "all")
    monkeypatch.setattr(args, "softmaxNegs", -1)
    with pytest.raises(ValueError, match="softmaxNegs"):
        model.Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "softmaxNegs", 11)
    with pytest.raises(ValueError, match="softmaxNegs 11 exceeds the 10 items"):
        model.Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "softmaxNegs", 5)
    monkeypatch.setattr(args, "predLoss", "hinge")
    with pytest.raises(ValueError, match=r"--softmaxNegs 5 needs --predLoss softmax: --predLoss hinge"):
        model.Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "softmaxNegs", 0)         # the default is fine under hinge
    with pytest.raises(_PastTheChecks):
        model.Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "predLoss", "softmax")
    monkeypatch.setattr(args, "fusion_rows", "batch")
    with pytest.raises(ValueError, match="every item row"):           # N == 0: refused as before, same message
        model.Recommender("cpu", None).prepareModel()
    for n in (1, 5, 10):                                              # N > 0: softmax + batch rows is allowed
        monkeypatch.setattr(args, "softmaxNegs", n)
        with pytest.raises(_PastTheChecks):
            model.Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "latdim", 96)                           # the latdim check stays
    with pytest.raises(ValueError, match="latdim"):
        model.Recommender("cpu", None).prepareModel()


def _fwd(lib, p, **o):
    return H.call(lib, False, H.softmax_args(p, _lib.SOFTMAX_CAND, **o))


def _bwd(lib, p, **o):
    return H.call(lib, True, H.softmax_args(p, _lib.SOFTMAX_CAND, **o))


@pytest.mark.parametrize("name", ["fwd", "bwd"])
def test_both_cand_entries_reject_every_invalid_argument_without_a_device(name):
    lib = _lib.load()
    buf, p = H.aligned_buffer()
    fn = _fwd if name == "fwd" else _bwd
    cases = [
        (dict(Q=None), -1, "q or i"), (dict(I=None), -1, "q or i"), (dict(target=None), -1, "target"),
        (dict(ptr=p), -1, "excl_ptr"), (dict(items=p), -1, "excl_ptr"), (dict(row=p), -1, "excl_row"),
        (dict(d=24, ldq=24, ldi=24), -2, "d = 24"), (dict(d=256, ldq=256, ldi=256), -2, "d = 256"), (dict(d=0), -2, "d = 0"),
        (dict(nq=-1), -5, "n_queries"), (dict(ni=0), -5, "n_items"), (dict(ni=1 << 31), -5, "n_items"),
        (dict(inv_temp=0.0), -5, "inv_temp"), (dict(inv_temp=-2.0), -5, "inv_temp"),
        (dict(inv_temp=float("inf")), -5, "inv_temp"), (dict(inv_temp=float("nan")), -5, "inv_temp"),
        (dict(scale=float("nan")), -5, "scale"), (dict(scale=float("inf")), -5, "scale"),
        (dict(ptr=p, items=p, n_lists=-1), -5, "n_lists"), (dict(ptr=p, items=p, n_lists=7), -5, "exclusion lists"),
        (dict(ldq=66), -3, "ldq"), (dict(ldi=65), -3, "ldi"), (dict(ldq=60), -5, ">= d"), (dict(ldi=32), -5, ">= d"),
        (dict(Q=p + 4), -3, "16-byte aligned"), (dict(I=p + 8), -3, "16-byte aligned"),
        (dict(cand=None), -1, "null cand"), (dict(n_cand=-1), -5, "n_cand"), (dict(n_cand=101), -5, "n_cand"),
        (dict(ws_bytes=16), -6, "workspace"), (dict(ws=None), -6, "workspace"), (dict(ws=p + 4), -3, "workspace"),
    ]
    if name == "fwd":
        cases += [(dict(**{k: None}), -1, "loss, lse or tscore") for k in ("loss", "lse", "tscore")]
    else:
        cases += [(dict(lse=None), -1, "lse or g"), (dict(g=None), -1, "lse or g")]
        cases += [(dict(**{k: None}), -1, "dq, dic or dt") for k in ("dQ", "dIc", "dT")]
        cases += [(dict(**{k: 66}), -3, "lddq / lddic / lddt") for k in ("lddq", "lddic", "lddt")]
        cases += [(dict(**{k: 60}), -5, ">= d") for k in ("lddq", "lddic", "lddt")]
        cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in ("dQ", "dIc", "dT")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
        assert _lib.last_error().startswith("softmax_loss_cand_bwd: " if name == "bwd" else "softmax_loss_cand: ")
    del buf     # a valid argument set gets past the checks only with a GPU: none of the above touched one


def test_sample_strata_rejects_every_invalid_argument_without_a_device():
    lib = _lib.load()
    buf, p = H.aligned_buffer()
    f = lib.sagnn_sample_strata_i32
    for a, code, text in [((0, 0, 1, 0, p), -5, "n_items"), ((-3, 0, 1, 0, p), -5, "n_items"), ((1 << 31, 5, 1, 0, p), -5, "n_items"),
                          ((10, -1, 1, 0, p), -5, "n_cand"), ((10, 11, 1, 0, p), -5, "n_cand"), ((10, 5, 1, 0, None), -1, "null cand")]:
        assert f(*a, None) == code, (a, _lib.last_error())
        assert text in _lib.last_error().lower(), (a, _lib.last_error())
    assert f(10, 0, 1, 0, None, None) == 0          # nothing to draw: no launch, a null list is fine
    for a in [(0, 0, 1, 0), (10, 11, 1, 0), (10, -1, 1, 0), (10, 5, -1, 0), (10, 5, 1 << 64, 0), (10, 5, 1, -1), (10, 5, 1, 1 << 32)]:
        with pytest.raises(ValueError, match="sample_strata"):
            ops.sample_strata(*a, "cuda")
    with pytest.raises(TypeError, match="GPU device"):
        ops.sample_strata(10, 5, 1, 0, "cpu")
    del buf


def test_target_add_rejects_every_invalid_argument_without_a_device():
    lib = _lib.load()
    buf, p = H.aligned_buffer()

    def f(**o):
        a = dict(dT=p, lddt=64, target=p, nq=8, ni=100, d=64, dI=p, lddi=64)
        a.update(o)
        return lib.sagnn_softmax_target_add_f32(*a.values(), None)
    for over, code, text in [(dict(dT=None), -1, "null"), (dict(target=None), -1, "null"), (dict(dI=None), -1, "null"),
                             (dict(d=48), -2, "d = 48"), (dict(nq=-1), -5, "n_queries"), (dict(ni=0), -5, "n_items"),
                             (dict(lddt=66), -3, "lddt / lddi"), (dict(lddi=66), -3, "lddt / lddi"), (dict(lddt=60), -5, ">= d"),
                             (dict(lddi=32), -5, ">= d"), (dict(dT=p + 4), -3, "16-byte"), (dict(dI=p + 8), -3, "16-byte")]:
        assert f(**over) == code, (over, _lib.last_error())
        assert text in _lib.last_error().lower(), (over, _lib.last_error())
    del buf


def test_ops_wrappers_check_before_any_device_call():
    Q, I = torch.zeros((3, 64)), torch.zeros((10, 64))         # host tensors: a device call would fail differently
    t, cand = torch.zeros(3, dtype=torch.int32), torch.arange(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="cand"):
        ops.softmax_loss_cand(Q, I, torch.zeros((2, 2), dtype=torch.int32), t)
    with pytest.raises(ValueError, match="d = 48"):
        ops.softmax_loss_cand(torch.zeros((3, 48)), torch.zeros((10, 48)), cand, t)
    with pytest.raises(ValueError, match="inv_temp"):
        ops.softmax_loss_cand(Q, I, cand, t, inv_temp=0.0)
    with pytest.raises(TypeError, match="device tensor"):          # what a host tensor gets: no device call was made
        ops.softmax_loss_cand(Q, I, cand, t)
    with pytest.raises(TypeError, match="device tensor"):
        ops.softmax_loss_cand_bwd(Q, I, cand, t, torch.zeros(3), torch.ones(1))


def test_cand_workspace_is_monotone():
    f = _lib.load().sagnn_softmax_loss_cand_workspace_bytes
    cands = (0, 1, 17, 127, 128, 129, 4096, 32768, 32769, 52619, 131072, 131073, 1_000_003, (1 << 31) - 1)
    for d in (32, 64, 128):
        for nq in (1, 16, 33, 512):
            by_c = [f(nq, nc, d) for nc in cands]
            assert all(a <= b for a, b in zip(by_c, by_c[1:])) and by_c[0] < by_c[-1], (d, nq, by_c)
        for nc in cands:
            by_n = [f(n, nc, d) for n in (1, 7, 16, 17, 33, 511, 512, 513, 4096)]
            assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] < by_n[-1], (d, nc, by_n)
    for nc in cands[1:]:
        by_d = [f(512, nc, d) for d in (32, 64, 128)]
        assert by_d[0] < by_d[1] < by_d[2], (nc, by_d)
    assert f(0, 100, 64) == 0 and f(-1, 100, 64) == 0 and f(8, -1, 64) == 0
    assert f(8, 0, 64) > 0      # no candidates is legal: the forward still holds one loss term per row


@pytest.mark.parametrize("n_items,n_cand", [(1, 1), (17, 5), (50, 10), (4099, 64), (52619, 4096), (300, 300), (7, 1),
                                            ((1 << 31) - 1, 1000)])
def test_numpy_strata_draw(n_items, n_cand):
    seed, step = 0x1234567890ABCDEF, 3
    c = C.strata(n_items, n_cand, seed, step)
    j = np.arange(n_cand, dtype=np.int64)
    lo, up = j * n_items // n_cand, (j + 1) * n_items // n_cand
    assert c.dtype == np.int64 and c.shape == (n_cand,)
    assert ((c >= lo) & (c < up)).all()                               # each id inside its stratum
    assert (np.diff(c) > 0).all() and c[0] >= 0 and c[-1] < n_items   # hence ascending and distinct
    sizes = up - lo
    assert sizes.max() - sizes.min() <= 1 and sizes.sum() == n_items
    assert np.array_equal(c, C.strata(n_items, n_cand, seed, step))   # a pure function of its arguments
    if n_cand == n_items:
        assert np.array_equal(c, np.arange(n_items))
    elif n_cand >= 5:
        assert not np.array_equal(c, C.strata(n_items, n_cand, seed, step + 1))
        assert not np.array_equal(c, C.strata(n_items, n_cand, seed + 1, step))
    assert C.strata(n_items, 0, seed, step).shape == (0,)


def test_strata_draw_uses_its_own_stream_word():
    """The block is philox(counter = (j, 0, step, 0xFFFFFFFF), key = seed) and the draw the high half of the 64-bit
    word times the stratum's size."""
    import device_sampler_ref as S
    seed, step, n_items, n_cand = 99, 7, 1000, 8
    w = S.philox4x32_10(np.arange(n_cand), 0, step, 0xFFFFFFFF, seed)
    word = (w[0].astype(object) << 32) | w[1].astype(object)
    want = [125 * j + int((int(word[j]) * 125) >> 64) for j in range(n_cand)]
    assert C.strata(n_items, n_cand, seed, step).tolist() == want


def test_inclusion_frequency_is_uniform():
    """n_items = 50, N = 10, steps 0..1999 under one seed: every item is drawn with probability 1 / 5, so its count is
    binomial(2000, 0.2): mean 400, sd sqrt(2000 * 0.2 * 0.8) = 17.9, and 6 sd = 107.3 -> within 108 of 400. The draw
    is a pure function of the seed, so this is a constant, not a chance."""
    counts = np.zeros(50, np.int64)
    for step in range(2000):
        counts[C.strata(50, 10, 20261020, step)] += 1
    print("inclusion counts: min %d max %d" % (counts.min(), counts.max()))
    assert counts.sum() == 20000
    assert (np.abs(counts - 400) <= 108).all(), counts


def _case(seed, nq, ni, d, skip=()):
    rng = np.random.default_rng(seed)
    Q, I = rng.standard_normal((nq, d)), rng.standard_normal((ni, d))
    target = rng.integers(0, ni, nq)
    target[list(skip)] = -1
    lists = [np.sort(rng.integers(0, ni, rng.integers(0, max(ni // 3, 1) + 1))) for _ in range(nq + 2)]
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
    return Q, I, target, ptr, np.concatenate(lists).astype(np.int64)


@pytest.mark.parametrize("excl_row", [False, True])
@pytest.mark.parametrize("n_cand", [0, 1, 6, 23])
def test_augmented_lists_agree_with_torch_autograd_on_a_masked_logsumexp(excl_row, n_cand):
    nq, ni, d, inv_temp, scale = 9, 23, 8, 1.0 / 0.7, 0.31
    Q, I, target, ptr, items = _case(1, nq, ni, d, skip=(2,))
    rows = np.array([3, 0, 1, nq + 1, -1, 99, 4, 4, 2]) if excl_row else None
    cand = C.strata(ni, n_cand, 5, 0)
    ref = C.softmax_loss_cand_np(Q, I, cand, target, inv_temp, scale, ptr, items, rows)
    # the eligible set written out directly: candidates off the row's list, plus the target
    el = np.zeros((nq, ni), dtype=bool)
    for b, ids in enumerate(C.row_lists(nq, ptr, items, rows)):
        if target[b] < 0:
            continue
        el[b, np.setdiff1d(cand, ids)] = True
        el[b, target[b]] = True
    assert np.array_equal(el, ref["eligible"])
    q, i = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(I).requires_grad_(True)
    z = (q @ i.T) * inv_temp
    ok = torch.from_numpy(el.any(1))
    lse = torch.logsumexp(z.masked_fill(~torch.from_numpy(el), float("-inf"))[ok], dim=1)
    tz = z[ok].gather(1, torch.from_numpy(target)[ok][:, None])[:, 0]
    loss = scale * (lse - tz).sum()
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(abs(ref["loss"]), 1.0)
    np.testing.assert_allclose(q.grad.numpy(), ref["dQ"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(i.grad.numpy(), ref["dI"], rtol=1e-11, atol=1e-13)
    if n_cand == 0:         # only the target is left: p = 1, no loss and no gradient
        assert abs(ref["loss"]) <= 1e-12 and np.abs(ref["dQ"]).max() <= 1e-12 and np.abs(ref["dI"]).max() <= 1e-12
    # a device-shaped result (dIc at the candidates, dT at the targets) assembles to the reference dI
    g = ref["p"].copy()
    okb = target >= 0
    g[np.flatnonzero(okb), target[okb]] -= 1.0
    g *= scale * inv_temp
    gt = np.where(okb, g[np.arange(nq), np.where(okb, target, 0)], 0.0)
    gc = g.copy()
    gc[np.flatnonzero(okb), target[okb]] = 0.0
    full = C.assemble_dI(ni, cand, gc[:, cand].T @ Q, target, gt[:, None] * Q)
    np.testing.assert_allclose(full, ref["dI"], rtol=1e-11, atol=1e-13)
