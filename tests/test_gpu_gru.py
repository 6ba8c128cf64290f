"""GPU suite of the opt-in GRU cell of the interval fusion (--rnnCell gru): the fused forward kernel
(d = 32 / 64) and the per-step route (every other multiple of 32) against the float64 restatement of gru_ref, the
training forward, the fusion's backward under both --fusion_rows modes against float64 autograd, then the Recommender
under the flag (training objective, training steps, graph replay, evaluators, checkpoints) and the untouched default."""
import numpy as np
import pytest
import torch

import gru_ref as G
from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 2e-5          # the bar of tests/test_gpu_fusion.py

FORWARD_CASES = [(64, 3, 1000), (32, 1, 77), (64, 16, 130), (32, 6, 33), (64, 2, 1), (128, 6, 301), (96, 5, 64), (256, 2, 33)]


def _case(d, t, n, seed, x_scale=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, t, d)) * x_scale).astype(np.float32)
    p = G.init_gru_params(d, rng)
    return rng, x, [p[k] for k in G.GRU_KEYS]


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _close(got, want, name):
    got, want = got.cpu().numpy().astype(np.float64), np.asarray(want)
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, worst err / tol {(err / (ATOL + RTOL * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=name)


@pytest.mark.parametrize("d,t,n", FORWARD_CASES)
def test_forward_against_float64(dev, d, t, n):
    """Without and with a drop_scale of {0, 2}, and once with x given as [t, n, d] storage viewed [n, t, d]."""
    from sa_gnn_amd import ops
    assert ops.gru_fused_supported(d) == (d in (32, 64))               # d = 128, 96, 256: the per-step route
    rng, x, w = _case(d, t, n, 7 * d + t + n)
    wd = _dev(dev, *w)
    (xd,) = _dev(dev, x)
    want = G.gru(x, *w)
    _close(ops.gru_fwd(xd, *wd), want, "h")
    scale = ((rng.random((n, t, d)) < 0.5) * 2.0).astype(np.float32)
    _close(ops.gru_fwd(xd, *wd, drop_scale=_dev(dev, scale)[0]), G.gru(x, *w, drop=scale), "h under drop_scale")
    slab = _dev(dev, x.transpose(1, 0, 2))[0]                           # [t, n, d] storage
    got = ops.gru_fwd(slab.permute(1, 0, 2), *wd)
    _close(got, want, "h from the [t, n, d] layout")
    assert torch.equal(got, ops.gru_fwd(xd, *wd))                       # the layout of x does not reach the arithmetic


def test_many_tiles_per_workgroup(dev):
    """547 tiles of 128 rows on at most 256 workgroups: a block takes three tiles, the last tile holds 113 rows."""
    from sa_gnn_amd import ops
    d, t, n = 32, 2, 70001
    assert -(-n // 128) == 547 and n - 546 * 128 == 113
    _, x, w = _case(d, t, n, 11)
    _close(ops.gru_fwd(*_dev(dev, x, *w)), G.gru(x, *w), "h")


@pytest.mark.parametrize("d", [32, 64])
def test_saturated_gates(dev, d):
    """x scaled by 40, as in test_lstm_saturated_gates: the exp2-based sigmoid / tanh clamp to 0 / 1 / -1, no NaN."""
    from sa_gnn_amd import ops
    n, t = 257, 4
    _, x, w = _case(d, t, n, d, x_scale=40.0)
    got = ops.gru_fwd(*_dev(dev, x, *w))
    assert bool(torch.isfinite(got).all())
    _close(got, G.gru(x, *w), "h at saturated gates")
    h, gates, cand = ops.gru_fwd_train(*_dev(dev, x, *w))
    assert bool(torch.isfinite(gates).all()) and bool(torch.isfinite(cand).all())
    assert float(gates.min()) >= 0.0 and float(gates.max()) <= 1.0 and float(cand.abs().max()) <= 1.0


@pytest.mark.parametrize("d,t,n", [(64, 5, 300), (128, 3, 300)])
def test_rows_are_independent_and_runs_are_identical(dev, d, t, n):
    """Rows 5..260 as their own call equal the same rows of the full call bit for bit (--fusion_rows batch relies on it),
    and two runs of one call are bit-identical."""
    from sa_gnn_amd import ops
    _, x, w = _case(d, t, n, 3 * d)
    xd, *wd = _dev(dev, x, *w)
    full = ops.gru_fwd(xd, *wd)
    assert torch.equal(ops.gru_fwd(xd[5:261].contiguous(), *wd), full[5:261])
    assert torch.equal(ops.gru_fwd(xd, *wd), full)


@pytest.mark.parametrize("d,t,n", [(64, 6, 257), (32, 3, 130), (64, 1, 40), (128, 4, 90)])
def test_training_forward(dev, d, t, n):
    """gru_fwd_train's h is gru_fwd's bit for bit; gates (r | u) and cand against float64."""
    from sa_gnn_amd import ops
    _, x, w = _case(d, t, n, 5 * d + t)
    xd, *wd = _dev(dev, x, *w)
    h, gates, cand = ops.gru_fwd_train(xd, *wd)
    assert torch.equal(h, ops.gru_fwd(xd, *wd))
    _, want_g, want_c, want_h = G.gru(x, *w, want_saved=True)
    _close(h, want_h, "h")
    _close(gates, want_g, "gates")
    _close(cand, want_c, "cand")


def _fusion_case(d, t, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = G.init_fusion_params_gru(d, rng)
    gout = rng.standard_normal((n, d)).astype(np.float32)
    return rng, x, p, gout


def _grad_check(name, a, b, n, t):
    """The tolerance rule of tests/test_gpu_backward.py::test_interval_fusion_backward_vs_autograd, as written there."""
    a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    tol = 1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), 8e-6 * max(1.0, np.sqrt(n * t / 1000.0)))
    err = np.abs(a - b)
    print(f"{name}: worst |err| {err.max():.3e}, scale {np.abs(b).max():.3e}, worst err / tol {(err / tol).max():.3f}")
    bad = err > tol
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {err[bad].max():.3e} (scale {np.abs(b).max():.3e})"


@pytest.mark.parametrize("d,t,n,heads,dropout", [(64, 3, 300, 16, False), (32, 2, 130, 16, False), (64, 1, 70, 16, False),
                                                 (32, 6, 53, 16, False), (64, 16, 23, 16, False), (128, 3, 90, 16, False),
                                                 (64, 4, 97, 16, True)])
def test_fusion_backward_against_float64_autograd(dev, d, t, n, heads, dropout):
    """ag.interval_fusion with a GRU parameter dict: the output, dx and all twelve parameter gradients."""
    from sa_gnn_amd import autograd as ag
    rng, x, p, gout = _fusion_case(d, t, n, d + t + n)
    drop = ((rng.random((n, t, d)) < 0.5) * 2.0).astype(np.float32) if dropout else None
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    out = G.torch_interval_fusion_gru(tx, tp, heads, drop=None if drop is None else torch.from_numpy(drop).double())
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    # x given as a [t, n, d] storage viewed [n, t, d] (the GNN slab's layout)
    xd = _dev(dev, x.transpose(1, 0, 2))[0].permute(1, 0, 2).requires_grad_(True)
    pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
    got = ag.interval_fusion(xd, pd, heads, drop_scale=None if drop is None else _dev(dev, drop)[0])
    np.testing.assert_allclose(got.detach().cpu().numpy(), out.detach().numpy(), rtol=RTOL, atol=ATOL)
    got.backward(torch.from_numpy(gout).to(dev))
    assert len(p) == 12
    _grad_check("dx", xd.grad, tx.grad, n, t)
    for k in p:
        _grad_check("d" + k, pd[k].grad, tp[k].grad, n, t)


def test_fusion_backward_per_step_weight_gradients(dev, monkeypatch):
    """With DEFERRED_DW_LIMIT at zero the weight gradients are per-step products: the same gradients as the segmented
    products after the loop, within the rule."""
    from sa_gnn_amd import autograd as ag
    d, t, n, heads = 64, 3, 150, 16
    _, x, p, gout = _fusion_case(d, t, n, 99)
    grads = []
    for limit in (ag.DEFERRED_DW_LIMIT, 0):
        monkeypatch.setattr(ag, "DEFERRED_DW_LIMIT", limit)
        xd = _dev(dev, x)[0].requires_grad_(True)
        pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
        ag.interval_fusion(xd, pd, heads).backward(torch.from_numpy(gout).to(dev))
        grads.append({"x": xd.grad, **{k: v.grad for k, v in pd.items()}})
    for k in grads[0]:
        _grad_check("d" + k, grads[1][k], grads[0][k], n, t)


def test_fusion_rows_subset_against_all(dev):
    """IntervalFusionRowsFn under the GRU: a 40-row subset of 300 gives the `all` mode's gradients for those rows and
    for every parameter; every other row's gradient is exactly zero. Also an empty subset: zeros everywhere."""
    from sa_gnn_amd import autograd as ag
    from test_gpu_fusion_rows import _compact
    d, T, N, heads = 64, 3, 300, 16
    rng, x, p, _ = _fusion_case(d, T, N, 17)
    ids = np.sort(rng.choice(N, 40, replace=False))
    untouched = torch.from_numpy(np.setdiff1d(np.arange(N), ids)).to(dev)
    rows, count, _ = _compact(dev, N, [ids], 64)
    g_np = rng.standard_normal((N, d)).astype(np.float32)
    g_np[untouched.cpu().numpy()] = 0.0                                 # the loss reads the touched rows only
    g = torch.from_numpy(g_np).to(dev)
    slab = _dev(dev, x.transpose(1, 0, 2))[0].requires_grad_(True)      # [T, N, d]
    pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
    outs, grads = [], []
    for mode in ("all", "batch"):
        for v in list(pd.values()) + [slab]:
            v.grad = None
        xv = slab.permute(1, 0, 2)
        out = ag.interval_fusion(xv, pd, heads) if mode == "all" else ag.interval_fusion_rows(xv, rows, count, 40, pd, heads)
        (out * g).sum().backward()
        outs.append(out.detach())
        grads.append({k: v.grad.detach().clone() for k, v in pd.items()} | {"x": slab.grad.detach().clone().permute(1, 0, 2)})
    r = torch.from_numpy(ids).to(dev)
    assert torch.equal(outs[1][r], outs[0][r])                          # rows are independent: bit-identical
    assert int(torch.count_nonzero(outs[1][untouched])) == 0
    for k in pd:
        _grad_check("d" + k, grads[1][k], grads[0][k], 40, T)
    _grad_check("dx", grads[1]["x"][r], grads[0]["x"][r], 40, T)
    assert int(torch.count_nonzero(grads[1]["x"][untouched])) == 0
    rows0, count0, _ = _compact(dev, N, [[]], 4)
    for cap in (1, 0):
        for v in list(pd.values()) + [slab]:
            v.grad = None
        out = ag.interval_fusion_rows(slab.permute(1, 0, 2), rows0, count0, cap, pd, heads)
        out.sum().backward()
        assert int(torch.count_nonzero(out)) == 0 and int(torch.count_nonzero(slab.grad)) == 0
        assert all(v.grad is not None and v.grad.shape == v.shape and int(torch.count_nonzero(v.grad)) == 0 for v in pd.values())


def test_ops_interval_fusion_dispatches_on_the_cell(dev):
    """ops.interval_fusion with a GRU dict against float64 (fused d and a per-step d); an LSTM dict gives the same
    bits before and after a GRU call in the same process; a dict with both cells or neither is refused."""
    from sa_gnn_amd import ops
    for d, t, n in ((64, 3, 200), (128, 2, 70)):
        rng, x, p, _ = _fusion_case(d, t, n, d + 1)
        pd = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
        lstm = {k: torch.from_numpy(v).to(dev) for k, v in O.init_fusion_params(d, rng).items()}
        (xd,) = _dev(dev, x)
        before = ops.interval_fusion(xd, lstm, 16)
        got = ops.interval_fusion(xd, pd, 16)
        with torch.no_grad():
            want = G.torch_interval_fusion_gru(torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in p.items()}, 16)
        _close(got, want.numpy(), f"fusion under the GRU at d = {d}")
        assert torch.equal(ops.interval_fusion(xd, lstm, 16), before)
        with pytest.raises(ValueError, match="not both"):
            ops.interval_fusion(xd, {**lstm, **pd}, 16)
        with pytest.raises(KeyError, match="found neither"):
            ops.interval_fusion(xd, {k: v for k, v in pd.items() if not k.startswith("gru_")}, 16)


# ---- the Recommender under --rnnCell gru -------------------------------------------------------------------------------
GRU_NAMES = ("rnn_gru_gates_kernel", "rnn_gru_gates_bias", "rnn_gru_candidate_kernel", "rnn_gru_candidate_bias")
LSTM_NAMES = ("rnn_lstm_kernel", "rnn_lstm_bias")


def _gru_setup(dev, monkeypatch, d=64, ssldim=48, att_layer=2, cell="gru", **flags):
    from test_gpu_seq_att import _full_setup
    from sa_gnn_amd.Params import args as the_args
    for k, v in {"rnnCell": cell, "seqPool": "sum", "predLoss": "hinge", "edgeTime": "none", **flags}.items():
        monkeypatch.setattr(the_args, k, v)
    return _full_setup(dev, monkeypatch, d, ssldim, att_layer, mode="sum")


def _oracle_params_gru(rec, NNs):
    """test_gpu_train._oracle_params with the GRU's four leaves travelling where the LSTM kernel does (lstm_W: a tuple)."""
    leaves = {}

    def leaf(name):
        if name not in leaves:
            leaves[name] = NNs.params[name].detach().cpu().double().requires_grad_(True)
        return leaves[name]

    inv = {id(v): k for k, v in NNs.params.items()}
    mh = lambda att: {k: leaf(inv[id(v)]) for k, v in att.weights().items()}
    P = {"uEmbed": leaf("uEmbed"), "iEmbed": leaf("iEmbed"), "posEmbed": leaf("posEmbed"),
         "meta2_W": leaf("meta2"), "meta2_b": leaf("meta2Bias"), "meta3_W": leaf("meta3"), "meta3_b": leaf("meta3Bias")}
    for key, (gm, bt), att in (("fuse_u", rec.ln[0], rec.multihead_self_attention0),
                                ("fuse_i", rec.ln[1], rec.multihead_self_attention1)):
        P[key] = {"lstm_W": tuple(leaf(n) for n in GRU_NAMES), "lstm_b": None, "ln_gamma": leaf(inv[id(gm)]),
                  "ln_beta": leaf(inv[id(bt)]), **mh(att)}
    P["ln"] = [(leaf(inv[id(gm)]), leaf(inv[id(bt)])) for gm, bt in rec.head_ln]
    P["att"] = [mh(a) for a in rec.multihead_self_attention_sequence]
    return P, leaves


@pytest.mark.parametrize("d,fusion_rows", [(64, "all"), (32, "batch"), (128, "all")])
def test_train_loss_under_gru_against_float64(dev, monkeypatch, d, fusion_rows):
    from test_gpu_seq_att import CFG, _grad_close, _host_batch, _loss_and_grads
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch, d=d, fusion_rows=fusion_rows)
    assert all(n in NNs.params for n in GRU_NAMES) and not any(n in NNs.params for n in LSTM_NAMES)
    batch = _host_batch(rec, handler, args)
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    P, leaves = _oracle_params_gru(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    # a run-time patch in this test: the oracle's objective with its recurrent cell routed to the GRU restatement
    monkeypatch.setattr(O, "torch_basic_lstm", lambda x, W, b, forget_bias=1.0: G.torch_gru(x, *W))
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, batch, CFG)
    (opre + args.ssl_reg * ossl).backward()
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    checked = 0
    for name, leaf in leaves.items():
        got, want = grads[name], leaf.grad
        if want is None:
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        assert got is not None, f"no gradient reached {name}"
        extra = 0.0
        if name.endswith("k_bias"):    # analytically ~0: the noise of terms as large as the key kernel's gradient
            extra = 1e-3 * float(leaves[name.replace("k_bias", "k_kernel")].grad.abs().max())
        _grad_close(got.cpu().double().numpy(), want.numpy(), name, extra)
        checked += 1
    assert checked >= 22 and all(leaves[n].grad is not None and float(leaves[n].grad.abs().max()) > 0 for n in GRU_NAMES)


@pytest.mark.parametrize("fusion_rows", ["all", "batch"])
def test_three_training_steps_stay_finite(dev, monkeypatch, fusion_rows):
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch, 64, 32, 1, fusion_rows=fusion_rows)
    for k, v in (("trnNum", 48), ("lr", 5e-3), ("keepRate", 0.5), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay", 1.0)):
        monkeypatch.setattr(args, k, v)
    monkeypatch.setattr(args, "decay_step", args.trnNum // args.batch)
    np.random.seed(0)
    torch.manual_seed(0)
    before = {n: NNs.params[n].detach().clone() for n in GRU_NAMES}
    loss = rec.trainEpoch()["Loss"]
    assert rec.optimizer.global_step == 3 and np.isfinite(loss), loss
    assert all(float((NNs.params[n].detach() - before[n]).abs().max()) > 0 for n in GRU_NAMES)        # all four train
    assert all(bool(torch.isfinite(v).all()) for v in NNs.params.values())
    fu, fi = rec.forward()
    assert bool(torch.isfinite(fu).all()) and bool(torch.isfinite(fi).all())


def test_graph_replay_equals_eager(dev, monkeypatch):
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch)
    replay = rec.capture_forward()
    with torch.no_grad():
        NNs.params["rnn_gru_gates_bias"].add_(0.25)
    fu_g, fi_g = (t.clone() for t in replay())
    fu_e, fi_e = rec.forward()
    assert torch.equal(fu_g, fu_e) and torch.equal(fi_g, fi_e)


def test_evaluators_and_recommend_agree(dev, monkeypatch):
    from test_gpu_seq_att import EPS32
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch)
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    monkeypatch.setattr(args, "evaluator", "device")
    assert rec.testEpoch() == host and rec.testEpochFull() == host_full
    monkeypatch.setattr(args, "evaluator", "host")
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    p_full = rec.predict(users, target, sequence, mask, np.arange(len(users))).cpu().numpy().astype(np.float64)
    items, scores = rec.recommend(users, k=args.item, exclude_seen=False)
    at = np.array([scores[r][np.flatnonzero(items[r] == target[r])[0]] for r in range(len(users))], dtype=np.float64)
    att = rec._head_att(sequence, mask)[:len(users)].double().cpu().numpy()
    fu = rec.final_user_vector.double().cpu().numpy()[users]
    fi = rec.final_item_vector.double().cpu().numpy()[target]
    terms = ((np.abs(fu) + np.abs(np.maximum(args.leaky * att, att))) * np.abs(fi)).sum(1)
    assert (np.abs(at - p_full) <= 1e-4 * np.abs(p_full) + 1e-5 + 3 * EPS32 * terms).all()


def test_checkpoint_carries_the_cell(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch)
    for k, v in (("epoch", 1), ("save_path", "gru_ckpt"), ("load_model", "gru_ckpt")):
        monkeypatch.setattr(args, k, v)
    with torch.no_grad():
        NNs.params["rnn_gru_gates_kernel"].mul_(1.5)                  # away from what a fresh build draws
    want = rec.testEpochFull()
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "gru_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["rnnCell"] == "gru" and all(n in state["params"] for n in GRU_NAMES)
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpochFull() == want
    assert torch.equal(NNs.params["rnn_gru_gates_kernel"], state["params"]["rnn_gru_gates_kernel"].to(dev))
    monkeypatch.setattr(args, "rnnCell", "lstm")
    rec3 = Recommender(dev, handler)
    rec3.prepareModel()
    with pytest.raises(ValueError, match="--rnnCell gru, this run has --rnnCell lstm"):
        rec3.loadModel(str(tmp_path))
    # the other direction, and a checkpoint without the key is an LSTM model
    want3 = rec3.testEpochFull()
    rec3.saveHistory(str(tmp_path))
    state = torch.load(path, weights_only=True)
    assert state["rnnCell"] == "lstm" and not any(n in state["params"] for n in GRU_NAMES)
    del state["rnnCell"]
    torch.save(state, path)
    rec4 = Recommender(dev, handler)
    rec4.prepareModel()
    rec4.loadModel(str(tmp_path))
    assert rec4.testEpochFull() == want3
    monkeypatch.setattr(args, "rnnCell", "gru")
    rec5 = Recommender(dev, handler)
    rec5.prepareModel()
    with pytest.raises(ValueError, match="--rnnCell lstm, this run has --rnnCell gru"):
        rec5.loadModel(str(tmp_path))


def test_off_means_off(dev, monkeypatch):
    """Under the default no GRU variable exists and no GRU entry is called; every variable up to and including the LSTM
    kernel holds what the seeded initialiser stream gives when drawn in registration order with the LSTM's shapes (so
    nothing moved before or at the cell), two fresh models agree bit for bit, and a GRU model at the same seed differs from
    the default only from the cell on: its four variables stand where the LSTM's two stood."""
    from test_gpu_seq_att import _host_batch, _loss_and_grads
    from sa_gnn_amd import ops
    from sa_gnn_amd.model import Recommender
    from sa_gnn_amd.Params import args as the_args
    assert the_args.rnnCell == "lstm"

    def boom(*a, **k):
        raise AssertionError("a GRU entry was called under --rnnCell lstm")
    for name in ("gru_fwd", "gru_fwd_train", "gru_bwd_cand", "gru_bwd_gates"):
        monkeypatch.setattr(ops, name, boom)
    runs = []
    for _ in range(2):
        rec, handler, NNs, args = _gru_setup(dev, monkeypatch, cell="lstm")
        assert not any(n.startswith("rnn_gru") for n in NNs.params) and set(rec.rnn_cell) == {"lstm_W", "lstm_b"}
        pre, ssl, _ = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
        runs.append((pre, ssl, rec.testEpoch(), rec.testEpochFull()))
    assert runs[0] == runs[1]
    monkeypatch.undo()
    rec, handler, NNs, args = _gru_setup(dev, monkeypatch, cell="lstm")
    Recommender(dev, handler).prepareModel()                         # fresh initial values, no test-side edits
    start = {k: v.detach().clone() for k, v in NNs.params.items()}
    order = list(NNs.params)
    d = args.latdim
    assert tuple(start["rnn_lstm_kernel"].shape) == (2 * d, 4 * d) and tuple(start["rnn_lstm_bias"].shape) == (4 * d,)
    assert not start["rnn_lstm_bias"].cpu().numpy().any()
    gen = torch.Generator(device="cpu").manual_seed(100)             # NNLayers.reset's seed (reference main.py:21-23)
    at = order.index("rnn_lstm_kernel")
    for name in order[:at + 1]:
        shape = tuple(start[name].shape)
        rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        lim = float(np.sqrt(6.0 / ((shape[-2] + shape[-1]) * rf)))
        want = torch.rand(shape, generator=gen, dtype=torch.float32) * (2 * lim) - lim
        assert torch.equal(start[name].cpu(), want), name
    monkeypatch.setattr(args, "rnnCell", "gru")
    Recommender(dev, handler).prepareModel()
    assert list(NNs.params) == order[:at] + list(GRU_NAMES) + order[at + 2:]
    for name in order[:at]:
        assert torch.equal(NNs.params[name].detach(), start[name]), name
    Wg, bg, Wc, bc = (NNs.params[n].detach() for n in GRU_NAMES)
    assert tuple(Wg.shape) == (2 * d, 2 * d) and tuple(Wc.shape) == (2 * d, d)
    assert float(Wg.abs().max()) <= np.sqrt(6.0 / (4 * d)) and float(Wc.abs().max()) <= np.sqrt(6.0 / (3 * d))
    assert float(Wg.std()) > 0.4 * np.sqrt(6.0 / (4 * d)) and float(Wc.std()) > 0.4 * np.sqrt(6.0 / (3 * d))
    assert torch.equal(bg, torch.ones_like(bg)) and not bc.cpu().numpy().any()
    assert all(NNs.params[n].requires_grad and n not in NNs.regParams for n in GRU_NAMES)
