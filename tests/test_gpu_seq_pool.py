"""GPU suite of the opt-in additive-attention pooling of the sequence head (--seqPool additive): the two
new kernels against the float64 restatements of seq_pool_ref, autograd.SeqAddPoolFn against float64 autograd, then the
head they finish inside the Recommender (training objective, both batch forms, --fusion_rows batch, evaluators,
checkpoints, --predLoss softmax) and the untouched default."""
import numpy as np
import pytest
import torch

import seq_att_ref as R
import seq_pool_ref as SP
from oracle import selfgnn_oracle as O
from test_gpu_seq_att import (CFG, EPS32, QK_NOISE, _full_setup, _grad_close, _head_qk_names, _host_batch, _lens,
                              _loss_and_grads, _pad_rows, _value_close)

pytestmark = pytest.mark.gpu

ADD_NAMES = ("additive_attention0_kernel", "additive_attention0_bias", "additive_attention0_query")


def _pool_case(d, q, P, seed, lens=None):
    """x: layer-normed rows; Wa Xavier-uniform; v uniform in (-0.1, 0.1); u = x Wa + ba rounded to float32 (the kernels'
    input; the restatements read the same float32 values)."""
    rng = np.random.default_rng(seed)
    lens = _lens(P) if lens is None else lens
    x = O.layer_norm_td(rng.standard_normal((len(lens) * P, d))[:, None, :], np.ones(d), np.zeros(d), 1e-12)[:, 0, :]
    x = x.astype(np.float32)
    lim = np.sqrt(6.0 / (d + q))
    Wa = rng.uniform(-lim, lim, (d, q)).astype(np.float32)
    ba = (0.1 * rng.standard_normal(q)).astype(np.float32)
    v = rng.uniform(-0.1, 0.1, q).astype(np.float32)
    u = (x.astype(np.float64) @ Wa.astype(np.float64) + ba).astype(np.float32)
    g = rng.standard_normal((len(lens), d)).astype(np.float32)
    return lens, x, Wa, ba, v, u, g


def _poisoned(lens, P, x, u, g):
    """Copies with NaN where the contract says nothing is read: padded rows of x and u, the g rows of empty slots."""
    pad = _pad_rows(lens, P)
    xp, up, gp = x.copy(), u.copy(), g.copy()
    xp[pad], up[pad] = np.nan, np.nan
    gp[[b for b, n in enumerate(lens) if n == 0]] = np.nan
    return pad, xp, up, gp


def _run_kernels(dev, lens, P, x, u, v, g):
    from sa_gnn_amd import ops
    t = lambda a: torch.from_numpy(a).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out, w = ops.seq_addpool(t(x), t(u), t(v), lens_d, P, want_weights=True)
    dx, du, dv = ops.seq_addpool_bwd(t(x), t(u), t(v), t(g), lens_d, P)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (out, w, dx, du, dv))


def _reference(lens, P, x, u, v, g):
    """float64 on the float32 values: (out, w, terms) of the contract and autograd's (dx direct, du, dv), u a leaf."""
    x64, u64, v64 = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, u, v))
    out = SP.addpool_from_u_t(x64, u64, v64, lens, P)
    g64 = np.where(np.isnan(g), 0.0, g).astype(np.float64)
    (out * torch.from_numpy(g64)).sum().backward()
    want_w, terms = np.zeros(len(lens) * P), np.zeros(out.shape)
    for b, n in enumerate(lens):
        if n:
            s = np.tanh(u[b * P:b * P + n].astype(np.float64)) @ v.astype(np.float64)
            e = np.exp(s - s.max())
            want_w[b * P:b * P + n] = e / e.sum()
            terms[b] = want_w[b * P:b * P + n] @ np.abs(x[b * P:b * P + n].astype(np.float64))
    return out.detach().numpy(), want_w, terms, x64.grad.numpy(), u64.grad.numpy(), v64.grad.numpy()


def _zeros_where_the_contract_says(lens, P, pad, out, w, dx, du):
    empty = [b for b, n in enumerate(lens) if n == 0]
    assert not out[empty].any() and not w[pad].any() and not dx[pad].any() and not du[pad].any()
    sums = w.reshape(len(lens), P).astype(np.float64).sum(1)
    full = [b for b, n in enumerate(lens) if n]
    assert np.abs(sums[full] - 1.0).max() <= 1e-5 and not sums[empty].any()


@pytest.mark.parametrize("P", [8, 70, 256])
@pytest.mark.parametrize("d,q", [(32, 32), (64, 64), (128, 32)])
def test_pooling_forward_and_backward_against_float64(dev, d, q, P):
    lens, x, Wa, ba, v, u, g = _pool_case(d, q, P, 31 + P + d + q)
    pad, xp, up, gp = _poisoned(lens, P, x, u, g)
    out, w, dx, du, dv = _run_kernels(dev, lens, P, xp, up, v, gp)
    for name, a in (("out", out), ("w", w), ("dx", dx), ("du", du), ("dv", dv)):
        assert np.isfinite(a).all(), name
    _zeros_where_the_contract_says(lens, P, pad, out, w, dx, du)
    want, want_w, terms, wdx, wdu, wdv = _reference(lens, P, x, u, v, g)
    assert not wdx[pad].any() and not wdu[pad].any()
    _value_close(out, want, terms, "out")
    _value_close(w, want_w, 0.0 * want_w, "w")
    _grad_close(dx.astype(np.float64), wdx, "dx (direct)")
    _grad_close(du.astype(np.float64), wdu, "du")
    _grad_close(dv.astype(np.float64), wdv, "dv")


def test_dv_part_rows_of_empty_slots_are_zero(dev):
    """dv is the ascending sum of the per-slot rows; with only empty slots every row, and dv, is exactly zero, and
    with no slots at all the backward still writes its zero dv."""
    from sa_gnn_amd import ops
    P, d, q = 8, 32, 32
    for n in (3, 0):
        lens_d = torch.zeros(n, dtype=torch.int32, device=dev)
        x = torch.full((n * P, d), float("nan"), device=dev)
        u = torch.full((n * P, q), float("nan"), device=dev)
        g = torch.full((n, d), float("nan"), device=dev)
        v = torch.ones(q, device=dev)
        dx, du, dv = ops.seq_addpool_bwd(x, u, v, g, lens_d, P)
        assert not dx.cpu().numpy().any() and not du.cpu().numpy().any() and not dv.cpu().numpy().any()
        assert dv.shape == (q,) and tuple(ops.seq_addpool(x, u, v, lens_d, P).shape) == (n, d)


@pytest.mark.parametrize("d,q", [(32, 32), (64, 64), (128, 32)])
def test_pooling_beyond_the_exp_range_of_float32(dev, d, q):
    """v scaled until the largest |s_j| is 150: exp overflows float32 beyond 88, and a softmax without the shift
    returns inf / inf there. Values at the plain value tolerance; the gradients are checked for finiteness and zero
    padding only (a float32 restatement of the contract on the CPU reached 0.37 of the gradient tolerance at this scale:
    too little margin to promise)."""
    P = 70
    lens, x, Wa, ba, v, u, g = _pool_case(d, q, P, 77 + d + q)
    t64 = np.tanh(u.astype(np.float64))
    s = np.concatenate([t64[b * P:b * P + n] @ v.astype(np.float64) for b, n in enumerate(lens)])
    v = (v * np.float32(150.0 / np.abs(s).max() * (1 + 1e-6))).astype(np.float32)
    s = np.concatenate([t64[b * P:b * P + n] @ v.astype(np.float64) for b, n in enumerate(lens)])
    assert np.abs(s).max() >= 150.0 * (1 - 1e-5)
    pad, xp, up, gp = _poisoned(lens, P, x, u, g)
    out, w, dx, du, dv = _run_kernels(dev, lens, P, xp, up, v, gp)
    for name, a in (("out", out), ("w", w), ("dx", dx), ("du", du), ("dv", dv)):
        assert np.isfinite(a).all(), name
    _zeros_where_the_contract_says(lens, P, pad, out, w, dx, du)
    want, want_w, terms, _, _, _ = _reference(lens, P, x, u, v, g)
    _value_close(out, want, terms, "out at |s| <= 150")


def test_tanh_saturates_without_nan(dev):
    """|u| far beyond where tanh is +-1 in float32 (and where exp of it overflows): finite results, and the scores are
    the signed sums of v."""
    P, d, q = 8, 32, 32
    lens, x, Wa, ba, v, u, g = _pool_case(d, q, P, 3, lens=[3, 8])
    u = (u * np.float32(1e30)).astype(np.float32)
    out, w, dx, du, dv = _run_kernels(dev, lens, P, x, u, v, g)
    for name, a in (("out", out), ("w", w), ("dx", dx), ("du", du), ("dv", dv)):
        assert np.isfinite(a).all(), name
    want, want_w, terms, _, _, _ = _reference(lens, P, x, u, v, g)
    _value_close(out, want, terms, "out with saturated tanh")
    assert not du.any()                                               # 1 - t^2 is exactly 0 there


def test_pooling_is_bit_identical_between_runs(dev):
    P, d, q = 200, 64, 64
    lens, x, Wa, ba, v, u, g = _pool_case(d, q, P, 5)
    a, b = _run_kernels(dev, lens, P, x, u, v, g), _run_kernels(dev, lens, P, x, u, v, g)
    for name, p, r in zip(("out", "w", "dx", "du", "dv"), a, b):
        assert np.array_equal(p, r), name


@pytest.mark.parametrize("d,q,P,lens", [(64, 64, 70, None), (32, 64, 72, [0, 1, 72, 0, 7, 40]), (128, 32, 8, None)])
def test_seq_addpool_fn_against_float64_autograd(dev, d, q, P, lens):
    """autograd.SeqAddPoolFn (dense_nn -> seq_addpool; seq_addpool_bwd -> dense_tn -> dense_nn accumulating): output and
    all four gradients. One case has whole chunks of 32 and more zero gradient rows at the head of the slab (slots 0 and
    3 empty at P = 72), which the row-wise products between the kernels see."""
    from sa_gnn_amd import autograd as ag
    lens, x, Wa, ba, v, u, g = _pool_case(d, q, P, 13 + d + q, lens=lens)
    leaves = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (x, Wa, ba, v)]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ag.SeqAddPoolFn.apply(*leaves, lens_d, P)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    l64 = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, Wa, ba, v)]
    want = SP.addpool_t(*l64, lens, P)
    (want * torch.from_numpy(g.astype(np.float64))).sum().backward()
    _, _, terms = SP.addpool_np(*(a.astype(np.float64) for a in (x, Wa, ba, v)), lens, P)
    _value_close(out.detach().cpu().numpy(), want.detach().numpy(), terms, "pooled output")
    assert not leaves[0].grad.cpu().numpy()[_pad_rows(lens, P)].any()
    for name, got, ref in zip(("dx", "dWa", "dba", "dv"), leaves, l64):
        assert bool(torch.isfinite(got.grad).all()), name
        _grad_close(got.grad.cpu().double().numpy(), ref.grad.numpy(), name)


# ---- the Recommender under --seqAtt full --seqPool additive --------------------------------------------------------
def _add_setup(dev, monkeypatch, d=64, ssldim=48, att_layer=2, pool="additive", **flags):
    from sa_gnn_amd.Params import args as the_args
    for k, val in {"seqPool": pool, "query_vector_dim": 64, "predLoss": "hinge", **flags}.items():
        monkeypatch.setattr(the_args, k, val)
    return _full_setup(dev, monkeypatch, d, ssldim, att_layer)


def test_train_loss_under_additive_against_float64(dev, monkeypatch):
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _add_setup(dev, monkeypatch)
    batch = _host_batch(rec, handler, args)
    assert (np.asarray(batch["mask"]).sum(1) > 1).any()              # real sequences: more than one token per slot
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    P, leaves = _oracle_params(rec, NNs)
    for n in ADD_NAMES:
        leaves[n] = NNs.params[n].detach().cpu().double().requires_grad_(True)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    head = SP.torch_head_additive(tuple(leaves[n] for n in ADD_NAMES))
    opre, ossl, _, _ = R.torch_train_loss_full(P, adj, tp, batch, CFG, head=head)
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
    assert checked >= 23
    _, v_names = _head_qk_names(rec, NNs)
    v_scale = max(float(grads[n].abs().max()) for n in v_names)
    for n in ADD_NAMES:
        print(f"{n}: max |grad| {float(grads[n].abs().max()):.3e} (value kernels {v_scale:.3e})")
        assert float(grads[n].abs().max()) > QK_NOISE * v_scale and float(leaves[n].grad.abs().max()) > QK_NOISE * v_scale, n


def test_device_sampled_batch_gives_the_host_forms_loss(dev, monkeypatch):
    from test_gpu_device_sampler import _host_form
    rec, handler, NNs, args = _add_setup(dev, monkeypatch)
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = rec.sample_batch_device(bat, 31337, 2)
    hb = _host_form(rec, b, args)
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, b)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"preLoss device {pre_d!r} host {pre_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed") + ADD_NAMES:
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_fusion_rows_batch_equals_all_under_additive(dev, monkeypatch, sampler):
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _add_setup(dev, monkeypatch)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    b = rec._host_train_batch(bat) if sampler == "host" else rec.sample_batch_device(bat, 2024, 1)
    res = _both_modes(rec, NNs, args, b, 1.0)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    assert rec.fusion_rows_counts[1] < args.item or rec.fusion_rows_counts[0] < args.user
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    assert all(ga[n] is not None for n in ADD_NAMES)
    _check_against(gb, ga, ga, "batch vs all under additive")


def test_evaluators_and_recommend_under_additive(dev, monkeypatch):
    rec, handler, NNs, args = _add_setup(dev, monkeypatch)
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    monkeypatch.setattr(args, "evaluator", "device")
    assert rec.testEpoch() == host and rec.testEpochFull() == host_full
    monkeypatch.setattr(args, "evaluator", "host")
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    locs = np.arange(len(users))
    p_full = rec.predict(users, target, sequence, mask, locs).cpu().numpy().astype(np.float64)
    items, scores = rec.recommend(users, k=args.item, exclude_seen=False)
    at = np.array([scores[r][np.flatnonzero(items[r] == target[r])[0]] for r in range(len(users))], dtype=np.float64)
    att = rec._head_att(sequence, mask)[:len(users)].double().cpu().numpy()
    fu = rec.final_user_vector.double().cpu().numpy()[users]
    fi = rec.final_item_vector.double().cpu().numpy()[target]
    terms = ((np.abs(fu) + np.abs(np.maximum(args.leaky * att, att))) * np.abs(fi)).sum(1)
    print(f"recommend vs predict: worst {np.abs(at - p_full).max():.3e} at scale {np.abs(p_full).max():.3e}")
    assert (np.abs(at - p_full) <= 1e-4 * np.abs(p_full) + 1e-5 + 3 * EPS32 * terms).all()
    # the pooling is in these scores: the same model scores differently with the plain sum
    monkeypatch.setattr(args, "seqPool", "sum")
    assert not np.array_equal(rec.predict(users, target, sequence, mask, locs).cpu().numpy().astype(np.float64), p_full)


def test_checkpoint_carries_the_flag(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _add_setup(dev, monkeypatch)
    for k, v in (("epoch", 1), ("save_path", "pool_ckpt"), ("load_model", "pool_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "pool_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["seqPool"] == "additive" and all(n in state["params"] for n in ADD_NAMES)
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()                                               # fresh registry, fresh random init
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
    monkeypatch.setattr(args, "seqPool", "sum")
    rec3 = Recommender(dev, handler)
    rec3.prepareModel()
    with pytest.raises(ValueError, match="--seqPool"):
        rec3.loadModel(str(tmp_path))
    # a checkpoint without the key is a sum-pooling model
    want3 = rec3.testEpoch()
    rec3.saveHistory(str(tmp_path))
    state = torch.load(path, weights_only=True)
    assert state["seqPool"] == "sum" and not any(n in state["params"] for n in ADD_NAMES)
    del state["seqPool"]
    torch.save(state, path)
    rec4 = Recommender(dev, handler)
    rec4.prepareModel()
    rec4.loadModel(str(tmp_path))
    assert rec4.testEpoch() == want3
    monkeypatch.setattr(args, "seqPool", "additive")
    rec5 = Recommender(dev, handler)
    rec5.prepareModel()
    with pytest.raises(ValueError, match="--seqPool"):
        rec5.loadModel(str(tmp_path))


def _finite_after(rec, NNs, args, handler):
    for k, v in NNs.params.items():
        assert bool(torch.isfinite(v).all()), k
    rec.forward()
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    assert bool(torch.isfinite(rec.predict(users, target, sequence, mask, np.arange(len(users)))).all())


def test_three_steps_under_the_softmax_loss_stay_finite(dev, monkeypatch):
    rec, handler, NNs, args = _add_setup(dev, monkeypatch, 64, 32, 1, predLoss="softmax", softmaxTemp=1.0)
    for k, v in (("trnNum", 48), ("lr", 5e-3), ("keepRate", 1.0), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay", 1.0)):
        monkeypatch.setattr(args, k, v)
    monkeypatch.setattr(args, "decay_step", args.trnNum // args.batch)
    np.random.seed(0)
    torch.manual_seed(0)
    before = {n: NNs.params[n].detach().clone() for n in ADD_NAMES}
    loss = rec.trainEpoch()["Loss"]
    assert rec.optimizer.global_step == 3 and np.isfinite(loss), loss
    assert all(float((NNs.params[n].detach() - before[n]).abs().max()) > 0 for n in ADD_NAMES)      # all three train
    _finite_after(rec, NNs, args, handler)


def test_training_steps_under_additive_stay_finite(dev, monkeypatch):
    """Forty optimiser steps at a large learning rate: losses and every parameter stay finite and the evaluator still
    ranks, as in test_training_steps_under_full_stay_finite."""
    rec, handler, NNs, args = _add_setup(dev, monkeypatch, 64, 32, 1)
    for k, v in (("trnNum", 64), ("lr", 2e-2), ("keepRate", 1.0), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay", 1.0)):
        monkeypatch.setattr(args, k, v)
    monkeypatch.setattr(args, "decay_step", args.trnNum // args.batch)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["Loss"] for _ in range(10)]          # 4 steps each
    assert rec.optimizer.global_step == 40 and np.isfinite(losses).all(), losses
    _finite_after(rec, NNs, args, handler)


def test_off_means_off(dev, monkeypatch):
    """--seqAtt full --seqPool sum: no additive variable, neither new entry is called, two fresh models give
    bit-identical losses and testEpoch(), and at the same seed a model built under additive starts every other variable
    where the sum model starts it."""
    from sa_gnn_amd import ops
    from sa_gnn_amd.model import Recommender
    from sa_gnn_amd.Params import args as the_args
    assert the_args.seqPool == "sum"

    def boom(*a, **k):
        raise AssertionError("an additive-pooling entry was called under --seqPool sum")
    monkeypatch.setattr(ops, "seq_addpool", boom)
    monkeypatch.setattr(ops, "seq_addpool_bwd", boom)
    runs = []
    for _ in range(2):
        rec, handler, NNs, args = _add_setup(dev, monkeypatch, pool="sum")
        assert not any(n.startswith("additive_attention0") for n in NNs.params) and rec.additive_attention0 is None
        pre, ssl, _ = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
        runs.append((pre, ssl, rec.testEpoch(), rec.testEpochFull()))
    assert runs[0] == runs[1]
    Recommender(dev, handler).prepareModel()                         # fresh initial values, no test-side edits
    start = {k: v.detach().clone() for k, v in NNs.params.items()}
    order = list(NNs.params)
    monkeypatch.setattr(args, "seqPool", "additive")
    Recommender(dev, handler).prepareModel()
    assert list(NNs.params) == order + list(ADD_NAMES)               # defined after every other variable
    for k, v in start.items():
        assert torch.equal(NNs.params[k].detach(), v), k
    Wa, ba, v = (NNs.params[n].detach() for n in ADD_NAMES)
    lim = float(np.sqrt(6.0 / (args.latdim + args.query_vector_dim)))
    assert tuple(Wa.shape) == (args.latdim, args.query_vector_dim) and float(Wa.abs().max()) <= lim and float(Wa.std()) > 0.4 * lim
    assert not ba.cpu().numpy().any() and float(v.abs().max()) < 0.1 and float(v.std()) > 0.03
    assert all(NNs.params[n].requires_grad and n not in NNs.regParams for n in ADD_NAMES)
