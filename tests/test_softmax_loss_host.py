"""CPU suite of the opt-in full-catalogue softmax loss (--predLoss softmax): the float64 restatement
against torch autograd, the flags, prepareModel's refusals, the argument checks of both C entries and of the ops
wrappers (each rejected before any device work, so no GPU is needed), the workspace size, and the banned-table helper
the device sampler and the loss share."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import softmax_args_host as H
import softmax_loss_ref as R
from sa_gnn_amd import _lib, ops


def _case(seed, nq, ni, d, skip=()):
    rng = np.random.default_rng(seed)
    Q, I = rng.standard_normal((nq, d)), rng.standard_normal((ni, d))
    target = rng.integers(0, ni, nq)
    target[list(skip)] = -1
    lists = [np.sort(rng.integers(0, ni, rng.integers(0, max(ni // 3, 1) + 1))) for _ in range(nq + 2)]
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
    return Q, I, target, ptr, np.concatenate(lists).astype(np.int64)


@pytest.mark.parametrize("excl_row", [False, True])
def test_numpy_restatement_agrees_with_torch_autograd(excl_row):
    nq, ni, d, inv_temp, scale = 9, 23, 8, 1.0 / 0.7, 0.31
    Q, I, target, ptr, items = _case(0, nq, ni, d, skip=(2,))
    rows = np.array([3, 0, 1, nq + 1, -1, 99, 4, 4, 2]) if excl_row else None      # -1 / 99: an empty list
    ref = R.softmax_loss_np(Q, I, target, inv_temp, scale, ptr, items, rows)
    el = R.eligible(nq, ni, target, ptr, items, rows)
    assert el[np.arange(nq) != 2, target[np.arange(nq) != 2]].all() and not el[2].any()      # the target always counts
    if excl_row:
        assert el[4].all() and el[5].all()
    q, i = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(I).requires_grad_(True)
    loss = R.torch_softmax_loss(q, i, target, inv_temp, scale, el)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    np.testing.assert_allclose(q.grad.numpy(), ref["dQ"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(i.grad.numpy(), ref["dI"], rtol=1e-11, atol=1e-13)
    assert not ref["dQ"][2].any() and ref["lse"][2] == 0 and ref["tscore"][2] == 0
    # a row that excludes everything but its target: p = 1 there, so no gradient and no loss
    all_items = np.arange(ni)
    one = R.softmax_loss_np(Q[:1], I, target[:1], inv_temp, 1.0, np.array([0, ni]), all_items)
    assert abs(one["loss"]) <= 1e-12 and np.abs(one["dQ"]).max() <= 1e-12


def test_flags_parse_and_default_to_hinge():
    from sa_gnn_amd import Params
    ns = Params.build_parser().parse_args([])
    assert ns.predLoss == "hinge" and ns.softmaxTemp == 1.0 and Params.args.predLoss == "hinge" and Params.args.softmaxTemp == 1.0
    ns = Params.build_parser().parse_args(["--predLoss", "softmax", "--softmaxTemp", "0.25"])
    assert ns.predLoss == "softmax" and ns.softmaxTemp == 0.25
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--predLoss", "bpr"])
    text = " ".join(Params.build_parser().format_help().lower().split())
    assert "--predloss {hinge,softmax}" in text and "--softmaxtemp" in text and text.count("not in the reference") >= 2


def test_prepare_model_refuses_bad_flag_combinations(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    monkeypatch.setattr(args, "predLoss", "softmax")
    monkeypatch.setattr(args, "fusion_rows", "batch")
    with pytest.raises(ValueError, match="every item row"):          # says why, before the handler or the device is touched
        Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "fusion_rows", "all")
    for temp in (0.0, -1.0, float("nan")):
        monkeypatch.setattr(args, "softmaxTemp", temp)
        with pytest.raises(ValueError, match="softmaxTemp"):
            Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "predLoss", "hinge")                    # the temperature is checked under either loss
    with pytest.raises(ValueError, match="softmaxTemp"):
        Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "softmaxTemp", 1.0)
    monkeypatch.setattr(args, "predLoss", "bpr")
    with pytest.raises(ValueError, match="predLoss"):
        Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "predLoss", "softmax")
    monkeypatch.setattr(args, "latdim", 96)
    with pytest.raises(ValueError, match="latdim"):
        Recommender("cpu", None).prepareModel()


def _fwd(lib, p, **o):
    return H.call(lib, False, H.softmax_args(p, _lib.SOFTMAX_FULL, **o))


def _bwd(lib, p, **o):
    return H.call(lib, True, H.softmax_args(p, _lib.SOFTMAX_FULL, **o))


@pytest.mark.parametrize("name", ["fwd", "bwd"])
def test_both_entries_reject_every_invalid_argument_without_a_device(name):
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
        (dict(ws_bytes=16), -6, "workspace"), (dict(ws=None), -6, "workspace"), (dict(ws=p + 4), -3, "workspace"),
    ]
    if name == "fwd":
        cases += [(dict(**{k: None}), -1, "loss, lse or tscore") for k in ("loss", "lse", "tscore")]
    else:
        cases += [(dict(lse=None), -1, "lse or g"), (dict(g=None), -1, "lse or g"), (dict(dQ=None), -1, "dq or di"),
                  (dict(dI=None), -1, "dq or di"), (dict(lddq=66), -3, "lddq"), (dict(lddi=60), -5, ">= d"),
                  (dict(dQ=p + 4), -3, "16-byte aligned"), (dict(dI=p + 4), -3, "16-byte aligned")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
        assert _lib.last_error().startswith("softmax_loss_bwd: " if name == "bwd" else "softmax_loss: ")
    del buf     # a valid argument set gets past the checks only with a GPU: none of the above touched one


@pytest.mark.parametrize("backward", [False, True])
def test_the_mode_is_named_by_its_field_and_a_contradiction_is_refused_without_a_device(backward):
    """A NULL struct, a mode outside the three, and candidate fields that the mode does not take: each refused with its
    code and a message naming the field, ahead of every other check (the struct's other fields are all NULL here)."""
    lib = _lib.load()
    buf, p = H.aligned_buffer()
    F, C = _lib.SOFTMAX_FULL, _lib.SOFTMAX_CAND
    assert H.call(lib, backward, None) == -1 and "sagnn_softmax_args is null" in _lib.last_error().lower()
    for mode, fields, code, text in [(3, {}, -5, "mode = 3"), (-1, {}, -5, "mode = -1"),
                                     (F, dict(cand=p), -5, "softmax_full with a cand"),
                                     (F, dict(bias=p), -5, "softmax_full with a bias"),
                                     (F, dict(n_cand=5), -5, "n_cand = 5"),
                                     (C, dict(bias=p), -5, "softmax_cand with a bias")]:
        # on a struct with nothing else set, then on an otherwise valid one
        for args in (_lib.SoftmaxArgs(mode=mode, **fields), H.softmax_args(p, mode, **fields)):
            assert H.call(lib, backward, args) == code, (mode, fields, _lib.last_error())
            assert text in _lib.last_error().lower(), (mode, fields, _lib.last_error())
    del buf


def test_workspace_is_monotone():
    f = _lib.load().sagnn_softmax_loss_workspace_bytes
    items = (1, 17, 127, 128, 129, 4099, 32768, 32769, 52619, 131072, 131073, 1_000_003, 5_000_000, (1 << 31) - 1)
    for d in (32, 64, 128):
        for nq in (1, 16, 33, 512):
            by_i = [f(nq, ni, d) for ni in items]
            assert all(a <= b for a, b in zip(by_i, by_i[1:])) and by_i[0] < by_i[-1], (d, nq, by_i)
        for ni in items:
            by_n = [f(n, ni, d) for n in (1, 7, 16, 17, 33, 511, 512, 513, 4096)]
            assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] < by_n[-1], (d, ni, by_n)
    for ni in items:
        by_d = [f(512, ni, d) for d in (32, 64, 128)]
        assert by_d[0] < by_d[1] < by_d[2], (ni, by_d)
    assert f(0, 100, 64) == 0 and f(8, 0, 64) == 0


def test_ops_softmax_loss_checks_before_any_device_call():
    Q, I = torch.zeros((3, 64)), torch.zeros((10, 64))         # host tensors: a device call would fail differently
    t = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="d = 48"):
        ops.softmax_loss(torch.zeros((3, 48)), torch.zeros((10, 48)), t)
    with pytest.raises(ValueError, match=r"\[B, d\]"):
        ops.softmax_loss(torch.zeros(64), I, t)
    with pytest.raises(ValueError, match="n_items"):
        ops.softmax_loss(Q, torch.zeros((0, 64)), t)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inv_temp"):
            ops.softmax_loss(Q, I, t, inv_temp=bad)
    with pytest.raises(ValueError, match="scale"):
        ops.softmax_loss(Q, I, t, scale=float("nan"))
    with pytest.raises(TypeError, match="device tensor"):          # what a host tensor gets: no device call was made
        ops.softmax_loss(Q, I, t)
    with pytest.raises(TypeError, match="device tensor"):
        ops.softmax_loss_bwd(Q, I, t, torch.zeros(3), torch.ones(1))


class _Handler:
    def __init__(self, sequence, trn, tst):
        self.sequence, self.trnMat, self.tstInt = sequence, trn, tst
        self.subMat = [sp.csr_matrix(trn)]


def test_banned_table_is_what_the_device_sampler_holds():
    """A hand-made handler: the table per user is the sorted distinct union of its trnMat row (non-zero values), its
    last item and its test item; DeviceSampler holds exactly the helper's arrays."""
    from sa_gnn_amd.model import DeviceSampler, banned_table
    I = 9
    sequence = [[1, 2, 3], [4], [], [0, 8, 8, 5]]
    trn = sp.lil_matrix((4, I))
    trn[0, 1] = trn[0, 2] = 1
    trn[1, 7] = 2
    trn[3, 0] = trn[3, 8] = 1
    trn = sp.csr_matrix(trn)
    trn.data[trn.indices == 7] = 0                                    # a stored zero does not ban
    tst = [6, None, 2, 0]
    h = _Handler(sequence, trn, tst)
    ptr, items = banned_table(h, I)
    want = [[1, 2, 3, 6], [4], [2], [0, 5, 8]]
    assert ptr.dtype == np.int64 and items.dtype == np.int32
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert items.tolist() == sum(want, [])
    S = DeviceSampler(h, "cpu", I, 40, 3)
    assert torch.equal(S.ban_ptr, torch.from_numpy(ptr)) and torch.equal(S.ban_items, torch.from_numpy(items))
    # the sampler's checks and messages are what they were
    with pytest.raises(ValueError, match=r"sequence of user 3 holds item 9, outside \[0, 9\)"):
        DeviceSampler(_Handler([[1], [2], [], [9]], trn, tst), "cpu", I, 40, 3)
    with pytest.raises(ValueError, match="every item is banned"):
        DeviceSampler(_Handler([[0, 1], [0]], sp.csr_matrix(np.ones((2, 2))), [None, None]), "cpu", 2, 40, 3)
