"""GPU suite of --seqHeads: the matrix-core attention kernels at head widths 16, 32 and 64 against the
float64 restatements of seq_att_ref / seq_causal_ref (values, gradients, padding, determinism, causality, overflow), then
the sequence head with a head count of its own inside the Recommender (training objective under both samplers and
masks, --fusion_rows batch, --seqTargets all, --seqPool additive, inference, checkpoints) and the untouched default."""
import functools

import numpy as np
import pytest
import torch

import seq_att_ref as A
import seq_causal_ref as C
from oracle import selfgnn_oracle as O
from test_gpu_seq_att import (CFG, EPS32, _full_setup, _grad_close, _host_batch, _loss_and_grads, _pad_rows)

pytestmark = pytest.mark.gpu

SHAPES = [(32, 2), (64, 4), (64, 2), (64, 1), (128, 4)]          # d_k 16, 16, 32, 64, 32


def _lens(P):
    """Every tile edge of a 16- and a 32-wide tiling, the empty slot, and the full slot last: the slab ends at the buffer's end."""
    return [min(n, P) for n in (0, 1, 15, 16, 17, 31, 32, 33, 64, 65, P)]


@functools.lru_cache(maxsize=None)
def _case(d, heads, P, seed=0):
    """q|k|v as test_gpu_seq_att._qkv_case builds them (layer-normed rows through Xavier-uniform weights), on _lens(P)."""
    rng = np.random.default_rng(1000 * d + 10 * heads + P + seed)
    lens = _lens(P)
    x = rng.standard_normal((len(lens) * P, d))
    y = O.layer_norm_td(x[:, None, :], np.ones(d), np.zeros(d), 1e-12)[:, 0, :]
    p = O.init_fusion_params(d, rng, np.float64)
    qkv = np.concatenate([y @ p["W" + c] + p["b" + c] for c in "qkv"], axis=1).astype(np.float32)
    g = rng.standard_normal((len(lens) * P, d)).astype(np.float32)
    qkv.setflags(write=False)
    g.setflags(write=False)
    return lens, qkv, g


def _score_scale(qkv, lens, P, d, heads, causal):
    """S: the largest sum_c |q_c k_c| / sqrt(d_k) over the (query, key) pairs the kernel evaluates."""
    dk = d // heads
    qh, kh = (np.abs(qkv[:, i * d:(i + 1) * d]).astype(np.float64).reshape(-1, heads, dk) for i in range(2))
    S = 0.0
    for b, n in enumerate(lens):
        if n:
            s = np.einsum("jhc,shc->hjs", qh[b * P:b * P + n], kh[b * P:b * P + n])
            S = max(S, (np.tril(s) if causal else s).max())
    return S / np.sqrt(dk)


def _ctx_close(got, want, terms, S, dk, name):
    """The project's value tolerance plus the rounding of a d_k-term score (test_attention_beyond_the_exp_range_of_float32)."""
    tol = 1e-4 * np.abs(want) + 1e-5 + (3 * EPS32 + 2 * (dk + 4) * EPS32 * S) * terms
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, worst err / tol {(err / tol).max():.3f} (S = {S:.2f})")
    assert (err <= tol).all(), f"{name}: {(err > tol).sum()}/{err.size} off, worst {err.max():.3e}"


def _run(dev, lens, qkv, g, P, heads, causal):
    from sa_gnn_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv_d = torch.from_numpy(np.array(qkv)).to(dev)
    ctx = ops.seq_attn_wide(qkv_d, lens_d, P, heads, causal)
    dqkv = ops.seq_attn_wide_bwd(qkv_d, torch.from_numpy(np.array(g)).to(dev), lens_d, P, heads, causal)
    torch.cuda.synchronize()
    return ctx.cpu().numpy(), dqkv.cpu().numpy()


def _reference(qkv, g, lens, P, heads, causal):
    R = C if causal else A
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    form = C.seq_attn_dense_t if causal and P > 64 else R.seq_attn_t        # the dense form: the same function, P x P at once
    (form(q64, lens, P, heads) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return want, terms, q64.grad.numpy()


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("P", [8, 72, 256])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_forward_and_backward_against_float64(dev, d, heads, P, causal):
    lens, qkv, g = _case(d, heads, P)
    pad = _pad_rows(lens, P)
    g_poison = g.copy()
    g_poison[pad] = np.nan                                           # padded rows of g_ctx are never read
    ctx, dqkv = _run(dev, lens, qkv, g_poison, P, heads, bool(causal))
    assert not ctx[pad].any() and not dqkv[pad].any()                # exact zeros in the padding
    want, terms, wg = _reference(qkv, g, lens, P, heads, causal)
    _ctx_close(ctx, want, terms, _score_scale(qkv, lens, P, d, heads, causal), d // heads, "ctx")
    assert not wg[pad].any()
    for i, name in enumerate(("dq", "dk", "dv")):
        _grad_close(dqkv[:, i * d:(i + 1) * d].astype(np.float64), wg[:, i * d:(i + 1) * d], name)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,heads,P", [(64, 1, 72), (64, 4, 8), (128, 4, 256)])
def test_padding_is_masked_by_select(dev, d, heads, P, causal):
    """The padded rows of qkv refilled with values of magnitude 1e3 (their scores reach 1e6 * d_k, far beyond exp's
    range): every real row keeps its bits, the padding stays exact zeros."""
    lens, qkv, g = _case(d, heads, P)
    pad = _pad_rows(lens, P)
    ctx, dqkv = _run(dev, lens, qkv, g, P, heads, causal)
    loud = qkv.copy()
    loud[pad] = np.where(np.random.default_rng(1).random((len(pad), 3 * d)) < 0.5, -1e3, 1e3).astype(np.float32)
    ctx2, dqkv2 = _run(dev, lens, loud, g, P, heads, causal)
    assert np.array_equal(ctx, ctx2) and np.array_equal(dqkv, dqkv2)
    assert not ctx2[pad].any() and not dqkv2[pad].any() and np.abs(ctx).max() > 0 and np.abs(dqkv).max() > 0


@pytest.mark.parametrize("causal", [False, True])
def test_runs_repeat_bit_for_bit(dev, causal):
    lens, qkv, g = _case(64, 1, 256)
    a, b = _run(dev, lens, qkv, g, 256, 1, causal), _run(dev, lens, qkv, g, 256, 1, causal)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.isfinite(a[0]).all() and np.isfinite(a[1]).all()


@pytest.mark.parametrize("d,heads,P,t", [(64, 1, 256, 129), (64, 4, 72, 16), (32, 2, 8, 3), (128, 4, 72, 47)])
def test_a_token_sees_no_later_token(dev, d, heads, P, t):
    """Causality as a property: moving token t leaves the ctx rows before it bit-identical, and a gradient that is
    non-zero in the rows <= j_max only gives exact zeros in dk, dv beyond j_max."""
    rng = np.random.default_rng(t)
    _, qkv, g = _case(d, heads, P)
    lens = [P, min(P, t + 1)]
    qkv, g = qkv[:2 * P].copy(), g[:2 * P].copy()
    ctx, _ = _run(dev, lens, qkv, g, P, heads, True)
    moved = qkv.copy()
    moved[t] += rng.standard_normal(3 * d).astype(np.float32)
    ctx2, _ = _run(dev, lens, moved, g, P, heads, True)
    assert np.array_equal(ctx[:t], ctx2[:t]) and (ctx[t:P] != ctx2[t:P]).any(1).all() and np.array_equal(ctx[P:], ctx2[P:])
    ctx3, _ = _run(dev, lens, moved, g, P, heads, False)
    assert (ctx3[:t] != ctx[:t]).any(1).all()                        # bidirectional: every row sees token t
    g[t + 1:P] = 0.0
    _, dqkv = _run(dev, lens, qkv, g, P, heads, True)
    assert not dqkv[t + 1:P, d:].any() and dqkv[:t + 1, d:].any(1).all()


@pytest.mark.parametrize("causal", [0, 1])
def test_beyond_the_exp_range_of_float32(dev, causal):
    """test_attention_beyond_the_exp_range_of_float32's construction at (64, 2), P = 70: scores up to +-150."""
    d, heads, P = 64, 2, 70
    dk = d // heads
    lens, qkv, g = _case(d, heads, P, seed=7)
    qkv = qkv.copy()
    qh, kh = qkv[:, :d].reshape(-1, heads, dk), qkv[:, d:2 * d].reshape(-1, heads, dk)
    worst = max(np.abs(np.einsum("jhc,shc->hjs", qh[b * P:b * P + n], kh[b * P:b * P + n])).max() for b, n in enumerate(lens) if n)
    qkv[:, :2 * d] *= np.float32(np.sqrt(150.0 * np.sqrt(dk) / worst))      # q and k alike: the largest |score| becomes 150
    S = _score_scale(qkv, lens, P, d, heads, False)
    assert S >= 150.0 * (1 - 1e-5)
    pad = _pad_rows(lens, P)
    ctx, dqkv = _run(dev, lens, qkv, g, P, heads, bool(causal))
    assert np.isfinite(ctx).all() and np.isfinite(dqkv).all() and not ctx[pad].any() and not dqkv[pad].any()
    R = C if causal else A
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    _ctx_close(ctx, want, terms, S, dk, "ctx at |score| <= 150")
    dv = []
    for gg in (g.astype(np.float64), np.abs(g).astype(np.float64)):     # a >= 0: |g| gives sum_j a |g_j|, the terms of dv
        q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
        (R.seq_attn_t(q64, lens, P, heads) * torch.from_numpy(gg)).sum().backward()
        dv.append(q64.grad.numpy()[:, 2 * d:])
    _ctx_close(dqkv[:, 2 * d:], dv[0], dv[1], S, dk, "dv at |score| <= 150")


# ---- the Recommender under --seqHeads --------------------------------------------------------------------------------
def _heads_setup(dev, monkeypatch, seq_heads=2, mode="full", setup=_full_setup, **kw):
    from sa_gnn_amd.Params import args
    monkeypatch.setattr(args, "seqHeads", seq_heads)
    return setup(dev, monkeypatch, mode=mode, **kw) if setup is _full_setup else setup(dev, monkeypatch, **kw)


def _with_heads(head, heads):
    """A restated head with its own head count: the objective passes cfg["heads"], the interval fusion's, to both."""
    return lambda fi, pos, ln, att, sequence, mask, _fusion_heads, leaky: head(fi, pos, ln, att, sequence, mask, heads, leaky)


def _spy_attention(monkeypatch):
    from sa_gnn_amd import ops
    counts = {}
    for name in ("seq_attn", "seq_attn_bwd", "seq_attn_wide", "seq_attn_wide_bwd", "seq_attn_wide_supported"):
        def spy(*a, _real=getattr(ops, name), _name=name, **k):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return counts


def _check_grads(grads, leaves, least=20):
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
    assert checked >= least


@pytest.mark.parametrize("sampler", ["host", "device"])
@pytest.mark.parametrize("mode", ["full", "causal"])
def test_train_loss_against_float64_with_sixteen_heads_in_the_fusion_and_two_in_the_head(dev, monkeypatch, mode, sampler):
    from test_gpu_device_sampler import _host_form
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _heads_setup(dev, monkeypatch, 2, mode)
    assert args.num_attention_heads == 16 and CFG["heads"] == 16
    counts = _spy_attention(monkeypatch)
    if sampler == "host":
        batch = host = _host_batch(rec, handler, args)
    else:
        batch = rec.sample_batch_device(np.random.default_rng(3).permutation(args.user)[:args.batch - 3], 31337, 2)
        host = _host_form(rec, batch, args)
    assert (np.asarray(host["mask"]).sum(1) > 1).any()               # real sequences: more than one token per slot
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_attn_wide", 0) > 0 and counts.get("seq_attn_wide_bwd", 0) > 0 and "seq_attn" not in counts
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    head = C.torch_head_causal if mode == "causal" else A.torch_head_ragged
    opre, ossl, _, _ = A.torch_train_loss_full(P, adj, tp, host, CFG, head=_with_heads(head, 2))
    (opre + args.ssl_reg * ossl).backward()
    shared = float(A.torch_train_loss_full(P, adj, tp, host, CFG, head=head)[0].detach())      # 16 heads in both
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r} (a shared head count of 16: {shared!r}); sslloss {ssl!r} vs {ossl!r}")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    assert abs(opre - shared) > 1e-3 * max(abs(opre), 1.0)           # the head count is part of the function
    _check_grads(grads, leaves)


def test_sixteen_heads_reach_the_narrow_entries_with_the_bits_of_the_default(dev, monkeypatch):
    """--seqHeads 16 at latdim 64 against --seqHeads 0 --num_attention_heads 16 on two fresh models: both reach the
    narrow entries and none of the wide ones, and the two losses have the same bits. The gradients are compared as
    test_gpu_seq_att.py::test_off_means_off compares two runs of one configuration: bit-identity does not hold for them
    between any two runs of this objective, because its backward sums with float atomics (sagnn_pair_score_bwd_f32, the
    gather's scatter and the weight gradients; on an MI355X the two runs here differed by 3.9e-3 in uEmbed's gradient, at
    the scale of the SSL term's 1e5), so they are held to test_gpu_fusion_rows.py's bound for such pairs of runs."""
    from test_gpu_fusion_rows import _check_against
    runs = []
    for seq_heads in (16, 0):
        rec, handler, NNs, args = _heads_setup(dev, monkeypatch, seq_heads)
        counts = _spy_attention(monkeypatch)
        pre, ssl, grads = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
        runs.append((pre, ssl, {k: g for k, g in grads.items() if NNs.params[k].requires_grad}))
        assert counts.get("seq_attn", 0) > 0 and counts.get("seq_attn_bwd", 0) > 0
        assert "seq_attn_wide" not in counts and "seq_attn_wide_bwd" not in counts
        monkeypatch.undo()
    (pre_a, ssl_a, g_a), (pre_b, ssl_b, g_b) = runs
    assert pre_a == pre_b and ssl_a == ssl_b
    assert any(g is not None for g in g_a.values())
    worst = max(float((g_a[k] - g_b[k]).abs().max()) for k in g_a if g_a[k] is not None)
    print(f"largest gradient difference between --seqHeads 16 and --seqHeads 0: {worst!r}")
    _check_against(g_b, g_a, g_a, "--seqHeads 16 vs --seqHeads 0")


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_fusion_rows_batch_equals_all(dev, monkeypatch, sampler):
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _heads_setup(dev, monkeypatch, 2)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    b = rec._host_train_batch(bat) if sampler == "host" else rec.sample_batch_device(bat, 2024, 1)
    res = _both_modes(rec, NNs, args, b, 1.0)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    assert rec.fusion_rows_counts[1] < args.item or rec.fusion_rows_counts[0] < args.user
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    _check_against(gb, ga, ga, "batch vs all under --seqHeads 2")


def test_every_position_a_target_runs_a_finite_step_and_matches_float64_on_the_loss(dev, monkeypatch):
    """--seqTargets all at latdim 32, --seqHeads 2 (d_k 16), 16 heads in the fusion."""
    import test_gpu_seq_causal as T
    from sa_gnn_amd.model import banned_table
    from test_gpu_softmax_loss import _oracle_params
    rec, handler, NNs, args = _heads_setup(dev, monkeypatch, 2, setup=T._setup)
    counts = _spy_attention(monkeypatch)
    batch, host = T._batch(rec, handler, args, "host")
    pre, ssl, grads = T._loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_attn_wide_bwd", 0) > 0 and "seq_attn" not in counts
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())
    slabs = C.torch_head_slabs
    monkeypatch.setattr(C, "torch_head_slabs", lambda fi, pos, ln, att, seq, mask, _h, leaky: slabs(fi, pos, ln, att, seq, mask, 2, leaky))
    Pm, _ = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, n_terms = C.torch_train_loss_all(Pm, adj, tp, host, T.CFG, banned_table(handler, args.item))
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"{n_terms} terms; preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert np.isfinite(pre) and abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)


def test_additive_pooling_runs_a_finite_step_and_matches_float64_on_the_loss(dev, monkeypatch):
    import seq_pool_ref as SP
    import test_gpu_seq_pool as T
    from test_gpu_train import _oracle_params
    from sa_gnn_amd.Params import args as the_args
    monkeypatch.setattr(the_args, "seqHeads", 2)
    rec, handler, NNs, args = T._add_setup(dev, monkeypatch)
    counts = _spy_attention(monkeypatch)
    batch = _host_batch(rec, handler, args)
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_attn_wide_bwd", 0) > 0 and "seq_attn" not in counts
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())
    P, _ = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    head = SP.torch_head_additive(tuple(NNs.params[n].detach().cpu().double() for n in T.ADD_NAMES))
    opre, ossl, _, _ = A.torch_train_loss_full(P, adj, tp, batch, CFG, head=_with_heads(head, 2))
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert np.isfinite(pre) and abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)


def test_evaluators_and_recommend(dev, monkeypatch):
    rec, handler, NNs, args = _heads_setup(dev, monkeypatch, 2)
    counts = _spy_attention(monkeypatch)
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    assert counts.get("seq_attn_wide", 0) > 0 and "seq_attn" not in counts
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
    monkeypatch.setattr(args, "seqHeads", 0)                          # the head count is part of the function
    assert np.abs(rec.predict(users, target, sequence, mask, locs).cpu().numpy() - p_full).max() > 1e-4 * np.abs(p_full).max()


def test_checkpoint_carries_the_head_count(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _heads_setup(dev, monkeypatch, 2)
    for k, v in (("epoch", 1), ("save_path", "heads_ckpt"), ("load_model", "heads_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "heads_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["seqHeads"] == 2 and state["seqAtt"] == "full"
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()                                               # fresh registry, fresh random init
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
    for other in (4, 0):
        monkeypatch.setattr(args, "seqHeads", other)
        with pytest.raises(ValueError, match="heads"):
            rec2.loadModel(str(tmp_path))
    del state["seqHeads"]
    torch.save(state, path)
    rec2.loadModel(str(tmp_path))                                     # no key: not checked


@pytest.mark.parametrize("mode", ["sum", "full"])
def test_off_means_off(dev, monkeypatch, mode):
    """--seqHeads 0: a training step and a test epoch call none of the new entries, under the default head and under
    --seqAtt full at the default 16 heads, and two fresh models give the same bits in the losses and in testEpoch()."""
    from sa_gnn_amd.Params import args as the_args
    assert the_args.seqHeads == 0 and the_args.seqAtt == "sum"
    runs = []
    for _ in range(2):
        rec, handler, NNs, args = _full_setup(dev, monkeypatch, mode=mode)
        counts = _spy_attention(monkeypatch)
        pre, ssl, _ = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
        runs.append((pre, ssl, rec.testEpoch()))
        assert not any(k.startswith("seq_attn_wide") for k in counts), counts
        assert ("seq_attn" in counts) == (mode == "full")
        monkeypatch.undo()
    assert runs[0] == runs[1]
