"""GPU suite of the opt-in self-attention over the item sequence (--seqAtt full): the three new kernels
and their backwards against the float64 restatements of seq_att_ref, then the head they build inside the Recommender
(training objective, both batch forms, --fusion_rows batch, evaluators, checkpoints) and the untouched default."""
import ctypes

import numpy as np
import pytest
import torch

import seq_att_ref as R
from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
CFG = {"T": 2, "L": 2, "leaky": 0.5, "heads": 16}
# On a length-1 sequence a = e / (e + 1e-8) is 1 to rounding whatever q and k are: what reaches Wq and Wk is the
# rounding of single terms (eps32 = 1.2e-7 each) summed over a few hundred pairs, i.e. below 1e-5 of the value kernels'
# gradient. A softmax over real tokens has a gradient of the value kernels' own order.
QK_NOISE = 1e-5


def _value_close(got, want, terms, name):
    """The project's value tolerance: |got - want| <= 1e-4 |want| + 1e-5 + 3 eps32 sum|terms|."""
    tol = 1e-4 * np.abs(want) + 1e-5 + 3 * EPS32 * terms
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, worst err / tol {(err / tol).max():.3f}")
    assert not (err > tol).any(), f"{name}: {(err > tol).sum()}/{err.size} off, worst {err.max():.3e}"


def _grad_close(got, want, name, floor_extra=0.0):
    """test_gpu_train.py's gradient tolerance: 2e-4 |want| + max(5e-5 max|want|, 2e-5)."""
    floor = max(5e-5 * np.abs(want).max(), 2e-5, floor_extra)
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, scale {np.abs(want).max():.3e}, worst err / tol "
          f"{(err / (2e-4 * np.abs(want) + floor)).max():.3f}")
    bad = err > 2e-4 * np.abs(want) + floor
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {err[bad].max():.3e} (scale {np.abs(want).max():.3e})"


def _lens(P):
    return [min(n, P) for n in (0, 1, 2, 63, 64, 65, P)]


def _qkv_case(d, heads, P, seed):
    """q|k|v of layer-normed rows through Xavier-uniform weights (scores are O(1): un-shifted exp is safe), as float32;
    the padded rows hold finite values like every activation slab."""
    rng = np.random.default_rng(seed)
    lens = _lens(P)
    x = rng.standard_normal((len(lens) * P, d))
    y = O.layer_norm_td(x[:, None, :], np.ones(d), np.zeros(d), 1e-12)[:, 0, :]
    p = O.init_fusion_params(d, rng, np.float64)
    qkv = np.concatenate([y @ p["W" + c] + p["b" + c] for c in "qkv"], axis=1).astype(np.float32)
    g = rng.standard_normal((len(lens) * P, d)).astype(np.float32)
    return lens, qkv, g


def _pad_rows(lens, P):
    return np.concatenate([np.arange(b * P + n, (b + 1) * P) for b, n in enumerate(lens)]).astype(np.int64)


@pytest.mark.parametrize("P", [8, 200, 256])
@pytest.mark.parametrize("d,heads", [(32, 16), (64, 16), (64, 8)])
def test_attention_forward_and_backward_against_float64(dev, d, heads, P):
    from sa_gnn_amd import ops
    lens, qkv, g = _qkv_case(d, heads, P, 11 + P + d + heads)
    pad = _pad_rows(lens, P)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv_d = torch.from_numpy(qkv).to(dev)
    g_poison = g.copy()
    g_poison[pad] = np.nan                                           # padded rows of g_ctx are never read
    ctx = ops.seq_attn(qkv_d, lens_d, P, heads)
    dqkv = ops.seq_attn_bwd(qkv_d, torch.from_numpy(g_poison).to(dev), lens_d, P, heads)
    torch.cuda.synchronize()
    ctx, dqkv = ctx.cpu().numpy(), dqkv.cpu().numpy()
    assert not ctx[pad].any() and not dqkv[pad].any()                # exact zeros in the padding
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    _value_close(ctx, want, terms, "ctx")
    q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    (R.seq_attn_t(q64, lens, P, heads) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    wg = q64.grad.numpy()
    assert not wg[pad].any()
    for i, name in enumerate(("dq", "dk", "dv")):
        _grad_close(dqkv[:, i * d:(i + 1) * d].astype(np.float64), wg[:, i * d:(i + 1) * d], name)


@pytest.mark.parametrize("d,heads", [(32, 16), (64, 16), (64, 8)])
def test_attention_beyond_the_exp_range_of_float32(dev, d, heads):
    """Scores up to +-150: exp overflows float32 beyond 88, and an un-shifted kernel returns inf / inf there (what a
    few hundred optimiser steps on Wq and Wk reach). The contract's quotient itself is finite and float64 evaluates it
    un-shifted. Tolerance: the value tolerance plus the rounding of the exponent. A score is a sum of d_k products
    folded and shifted in float32, off by at most (d_k + 4) eps32 S with S the largest sum_c |q_c k_c| / sqrt(d_k);
    that is the relative error of an e, twice that of an a = e / sum e, and ctx = sum a v moves by it times
    sum |a v|. The same bound on dv = sum_j a g. The other gradients are checked for finiteness and zero padding."""
    from sa_gnn_amd import ops
    P = 70
    dk = d // heads
    lens, qkv, g = _qkv_case(d, heads, P, 77 + d + heads)
    qh, kh = qkv[:, :d].reshape(-1, heads, dk), qkv[:, d:2 * d].reshape(-1, heads, dk)
    worst = max(np.abs(np.einsum("jhc,shc->hjs", qh[b * P:b * P + n], kh[b * P:b * P + n])).max() for b, n in enumerate(lens) if n)
    f = np.float32(np.sqrt(150.0 * np.sqrt(dk) / worst))
    qkv[:, :2 * d] *= f                                               # q and k alike: the largest |score| becomes 150
    qh, kh = qkv[:, :d].reshape(-1, heads, dk), qkv[:, d:2 * d].reshape(-1, heads, dk)
    S = max(np.einsum("jhc,shc->hjs", np.abs(qh[b * P:b * P + n]).astype(np.float64),
                      np.abs(kh[b * P:b * P + n]).astype(np.float64)).max() for b, n in enumerate(lens) if n) / np.sqrt(dk)
    assert S >= 150.0 * (1 - 1e-5)
    slack = 2 * (dk + 4) * EPS32 * S
    pad = _pad_rows(lens, P)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv_d = torch.from_numpy(qkv).to(dev)
    ctx = ops.seq_attn(qkv_d, lens_d, P, heads).cpu().numpy()
    dqkv = ops.seq_attn_bwd(qkv_d, torch.from_numpy(g).to(dev), lens_d, P, heads).cpu().numpy()
    assert np.isfinite(ctx).all() and np.isfinite(dqkv).all() and not ctx[pad].any() and not dqkv[pad].any()
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    err = np.abs(ctx - want)
    print(f"ctx at |score| <= 150: worst |err| {err.max():.3e}, worst err / tol "
          f"{(err / (1e-4 * np.abs(want) + 1e-5 + (3 * EPS32 + slack) * terms)).max():.3f}")
    assert (err <= 1e-4 * np.abs(want) + 1e-5 + (3 * EPS32 + slack) * terms).all()
    dv = []
    for gg in (g.astype(np.float64), np.abs(g).astype(np.float64)):     # a >= 0: |g| gives sum_j a |g_j|, the terms of dv
        q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
        (R.seq_attn_t(q64, lens, P, heads) * torch.from_numpy(gg)).sum().backward()
        dv.append(q64.grad.numpy()[:, 2 * d:])
    err = np.abs(dqkv[:, 2 * d:] - dv[0])
    assert (err <= 1e-4 * np.abs(dv[0]) + 1e-5 + (3 * EPS32 + slack) * dv[1]).all(), err.max()


def test_training_steps_under_full_stay_finite(dev, monkeypatch):
    """Forty optimiser steps at a large learning rate under --seqAtt full: losses and every parameter stay finite and
    the evaluator still ranks (a NaN score ranks its target last)."""
    rec, handler, NNs, args = _full_setup(dev, monkeypatch, 64, 32, 1)
    for k, v in (("trnNum", 64), ("lr", 2e-2), ("keepRate", 1.0), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay", 1.0)):
        monkeypatch.setattr(args, k, v)
    monkeypatch.setattr(args, "decay_step", args.trnNum // args.batch)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["Loss"] for _ in range(10)]          # 4 steps each
    assert rec.optimizer.global_step == 40 and np.isfinite(losses).all(), losses
    for k, v in NNs.params.items():
        assert bool(torch.isfinite(v).all()), k
    rec.forward()
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    assert bool(torch.isfinite(rec.predict(users, target, sequence, mask, np.arange(len(users)))).all())


def test_attention_backward_is_bit_identical_between_runs(dev):
    from sa_gnn_amd import ops
    P, d, heads = 200, 64, 16
    lens, qkv, g = _qkv_case(d, heads, P, 5)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv_d, g_d = torch.from_numpy(qkv).to(dev), torch.from_numpy(g).to(dev)
    a = ops.seq_attn_bwd(qkv_d, g_d, lens_d, P, heads)
    b = ops.seq_attn_bwd(qkv_d, g_d, lens_d, P, heads)
    assert torch.equal(a, b) and torch.equal(ops.seq_attn(qkv_d, lens_d, P, heads), ops.seq_attn(qkv_d, lens_d, P, heads))


def _gather_case(dev, explicit):
    """5 slots of P = 12 over 30 items; item 7 occurs three times in slot 1 and once more in slot 3."""
    rng = np.random.default_rng(8)
    P, d, I = 12, 32, 30
    seqs = [[], [7, 3, 7, 9, 7], [4], [11, 7, 2, 5, 6, 8, 1, 0, 12, 13, 14, 15], [20, 21]]
    if explicit:        # a general mask: scattered positions, ascending within the slot
        pos = [np.sort(rng.choice(P, size=len(s), replace=False)) for s in seqs]
    else:
        pos = [np.arange(P - len(s), P) for s in seqs]
    lens = np.array([len(s) for s in seqs], np.int32)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    fi = rng.standard_normal((I, d)).astype(np.float32)
    pe = rng.standard_normal((P, d)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tokens = (t(np.concatenate([np.asarray(s, np.int32) for s in seqs])),
              t(np.concatenate(pos).astype(np.int32)) if explicit else None, t(begin), t(lens))
    return P, d, I, seqs, pos, fi, pe, tokens


@pytest.mark.parametrize("explicit", [True, False])
def test_gather_and_its_backward(dev, explicit):
    from sa_gnn_amd import ops
    P, d, I, seqs, pos, fi, pe, tokens = _gather_case(dev, explicit)
    B = len(seqs)
    seq_slab, pos_slab = ops.seq_gather(torch.from_numpy(fi).to(dev), torch.from_numpy(pe).to(dev), *tokens)
    want_s, want_p = np.zeros((B * P, d), np.float32), np.zeros((B * P, d), np.float32)
    for b, (s, p) in enumerate(zip(seqs, pos)):
        want_s[b * P:b * P + len(s)] = fi[np.asarray(s, np.int64)]
        want_p[b * P:b * P + len(s)] = pe[p]
    assert np.array_equal(seq_slab.cpu().numpy(), want_s) and np.array_equal(pos_slab.cpu().numpy(), want_p)   # copies
    rng = np.random.default_rng(9)
    gs, gp = (rng.standard_normal((B * P, d)).astype(np.float32) for _ in range(2))
    d_fi, d_pos = ops.seq_gather_bwd(torch.from_numpy(gs).to(dev), torch.from_numpy(gp).to(dev), *tokens, I, P)
    _, d_pos2 = ops.seq_gather_bwd(torch.from_numpy(gs).to(dev), torch.from_numpy(gp).to(dev), *tokens, I, P)
    assert torch.equal(d_pos, d_pos2)                                 # no atomics on the position side
    want_fi, want_pos = np.zeros((I, d)), np.zeros((P, d))
    terms_fi, terms_pos = np.zeros((I, d)), np.zeros((P, d))
    for b, (s, p) in enumerate(zip(seqs, pos)):
        for j, (it, q) in enumerate(zip(s, p)):
            want_fi[it] += gs[b * P + j]
            terms_fi[it] += np.abs(gs[b * P + j])
            want_pos[q] += gp[b * P + j]
            terms_pos[q] += np.abs(gp[b * P + j])
    _value_close(d_fi.cpu().numpy(), want_fi, terms_fi, "d_fi")      # item 7: four rows from two slots
    _value_close(d_pos.cpu().numpy(), want_pos, terms_pos, "d_pos")
    assert np.abs(want_fi[7]).max() > 0 and not d_fi.cpu().numpy()[29].any()


def test_pool_and_its_backward(dev):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(10)
    P, d, lens = 70, 32, [0, 1, 2, 63, 64, 65, 70]
    B = len(lens)
    x = rng.standard_normal((B * P, d)).astype(np.float32)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ops.seq_pool(torch.from_numpy(x).to(dev), lens_d, P).cpu().numpy()
    want = np.stack([x[b * P:b * P + n].astype(np.float64).sum(0) for b, n in enumerate(lens)])
    terms = np.stack([np.abs(x[b * P:b * P + n]).astype(np.float64).sum(0) for b, n in enumerate(lens)])
    _value_close(out, want, terms, "pool")
    assert not out[0].any()                                           # the empty slot
    g = rng.standard_normal((B, d)).astype(np.float32)
    dx = ops.seq_pool_bwd(torch.from_numpy(g).to(dev), lens_d, P).cpu().numpy()
    want_dx = np.zeros((B * P, d), np.float32)
    for b, n in enumerate(lens):
        want_dx[b * P:b * P + n] = g[b]
    assert np.array_equal(dx, want_dx)                                # a broadcast, zeros into the padding


@pytest.mark.parametrize("d,heads", [(64, 16), (32, 16)])
def test_attention_layer_against_float64_with_whole_chunks_of_padding(dev, d, heads):
    """One layer (autograd.SeqAttnFn: LN -> q|k|v -> attention -> leaky(ctx) + x) and the pooling on a slab whose
    first rows, and whole stretches of 32 rows and more, are padding (slots 0 and 3 empty, P = 72): the row-wise entries
    between the new kernels see zero gradient rows there. Output and every gradient, the biases' included, against
    float64 at the tolerances above."""
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(21 + d)
    P, lens, leaky = 72, [0, 1, 72, 0, 7, 40], 0.5
    R_ = len(lens) * P
    p = O.init_fusion_params(d, rng, np.float64)
    names = ("ln_gamma", "ln_beta", "Wq", "bq", "Wk", "bk", "Wv", "bv")
    x = rng.standard_normal((R_, d)).astype(np.float32)
    g = rng.standard_normal((len(lens), d)).astype(np.float32)
    leaves = [torch.from_numpy(x).to(dev).requires_grad_(True)] + \
        [torch.from_numpy(p[k].astype(np.float32)).to(dev).requires_grad_(True) for k in names]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ag.SeqPoolFn.apply(ag.SeqAttnFn.apply(*leaves, lens_d, P, heads, leaky), lens_d, P)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    # float64 on the float32 values, slot by slot on the real tokens
    l64 = [v.detach().cpu().double().requires_grad_(True) for v in leaves]
    rows = []
    for b, n in enumerate(lens):
        xb = l64[0][b * P:b * P + n]
        if n:
            y = R._ln_t(xb, (l64[1], l64[2]))
            xb = R._lk_t(R.attn_tokens_t(y @ l64[3] + l64[4], y @ l64[5] + l64[6], y @ l64[7] + l64[8], heads), leaky) + xb
        rows.append(xb.sum(0))
    want = torch.stack(rows, 0)
    (want * torch.from_numpy(g.astype(np.float64))).sum().backward()
    terms = np.stack([np.abs(x[b * P:b * P + n]).astype(np.float64).sum(0) + n for b, n in enumerate(lens)])
    _value_close(out.detach().cpu().numpy(), want.detach().numpy(), terms, "pooled layer output")
    pad = _pad_rows(lens, P)
    assert not leaves[0].grad.cpu().numpy()[pad].any()
    for name, got, ref in zip(("x",) + names, leaves, l64):
        assert bool(torch.isfinite(got.grad).all()), name
        # bk: analytically ~0 (a key bias shifts every score of a row alike): test_gpu_train.py's floor for it
        extra = 1e-3 * float(l64[5].grad.abs().max()) if name == "bk" else 0.0
        _grad_close(got.grad.cpu().double().numpy(), ref.grad.numpy(), name, extra)


# ---- the Recommender under --seqAtt full ---------------------------------------------------------------------------
def _full_setup(dev, monkeypatch, d=64, ssldim=48, att_layer=2, mode="full"):
    from test_gpu_train import _setup
    from sa_gnn_amd.Params import args as the_args
    for k, v in (("seqAtt", mode), ("evaluator", "host"), ("sampler", "host"), ("fusion_rows", "all"), ("edgeKeepRate", 1.0),
                 ("adjNorm", "none")):
        monkeypatch.setattr(the_args, k, v)
    return _setup(dev, d, ssldim, att_layer)


def _host_batch(rec, handler, args):
    np.random.seed(3)
    batIds = np.random.permutation(args.user)[:args.batch]
    uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
    su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
    return {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si}


def _loss_and_grads(rec, NNs, args, batch):
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    return float(pre.detach()), float(ssl.detach()), {k: (None if v.grad is None else v.grad.clone()) for k, v in NNs.params.items()}


def _head_qk_names(rec, NNs):
    inv = {id(v): k for k, v in NNs.params.items()}
    return [inv[id(mh.weights()[w])] for mh in rec.multihead_self_attention_sequence for w in ("Wq", "Wk")], \
        [inv[id(mh.weights()["Wv"])] for mh in rec.multihead_self_attention_sequence]


def test_train_loss_under_full_against_float64(dev, monkeypatch):
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
    batch = _host_batch(rec, handler, args)
    assert (np.asarray(batch["mask"]).sum(1) > 1).any()              # real sequences: more than one token per slot
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = R.torch_train_loss_full(P, adj, tp, batch, CFG)
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
    assert checked >= 20
    # the head's query and key kernels now train: gradients above QK_NOISE, under which the collapsed head's stay
    qk, v = _head_qk_names(rec, NNs)
    v_scale = max(float(grads[n].abs().max()) for n in v)
    for n in qk:
        print(f"{n}: max |grad| {float(grads[n].abs().max()):.3e} (value kernels {v_scale:.3e})")
        assert float(grads[n].abs().max()) > QK_NOISE * v_scale and float(leaves[n].grad.abs().max()) > QK_NOISE * v_scale, n


def test_head_qk_gradients_are_noise_under_sum(dev, monkeypatch):
    rec, handler, NNs, args = _full_setup(dev, monkeypatch, mode="sum")
    _, _, grads = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
    qk, v = _head_qk_names(rec, NNs)
    v_scale = max(float(grads[n].abs().max()) for n in v)
    for n in qk:
        print(f"{n}: max |grad| {float(grads[n].abs().max()):.3e} (value kernels {v_scale:.3e})")
    assert all(float(grads[n].abs().max()) <= QK_NOISE * v_scale for n in qk)


def test_device_sampled_batch_gives_the_host_forms_loss(dev, monkeypatch):
    from test_gpu_device_sampler import _host_form
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = rec.sample_batch_device(bat, 31337, 2)
    hb = _host_form(rec, b, args)
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, b)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"preLoss device {pre_d!r} host {pre_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed"):                               # both inputs of the gather, through both position forms
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_fusion_rows_batch_equals_all_under_full(dev, monkeypatch, sampler):
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    b = rec._host_train_batch(bat) if sampler == "host" else rec.sample_batch_device(bat, 2024, 1)
    res = _both_modes(rec, NNs, args, b, 1.0)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    assert rec.fusion_rows_counts[1] < args.item or rec.fusion_rows_counts[0] < args.user
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    _check_against(gb, ga, ga, "batch vs all under full")


def _cut_to_one(mask):
    one = np.zeros_like(mask)
    one[:, -1] = mask[:, -1]                                          # right-aligned: the last item, where there is one
    return one


def test_full_equals_sum_where_every_sequence_is_one_item(dev, monkeypatch):
    """Slots with exactly one item: the same function in both modes. Slots with none: the contract's zero row, i.e.
    the plain <fu, fi> score (the collapsed head layer-norms its zero sums to beta instead)."""
    from sa_gnn_amd import ops
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
    rec.forward()
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    uLocs, iLocs, _, _, sequence, mask, uLocs_seq, _ = rec.sampleTestBatch(users)
    mask = _cut_to_one(mask)
    n_tok = mask.sum(1).astype(np.int64)[uLocs_seq]
    full = rec.predict(uLocs, iLocs, sequence, mask, uLocs_seq).cpu().numpy().astype(np.float64)
    monkeypatch.setattr(args, "seqAtt", "sum")
    coll = rec.predict(uLocs, iLocs, sequence, mask, uLocs_seq).cpu().numpy().astype(np.float64)
    plain = ops.pair_score(rec.final_user_vector, rec.final_item_vector, rec._i32(uLocs), rec._i32(iLocs)).cpu().numpy()
    one = n_tok == 1
    assert one.any()
    err = np.abs(full - coll)[one]
    print(f"full vs sum on one-item slots: worst {err.max():.3e} at scale {np.abs(coll[one]).max():.3e}")
    assert (err <= 1e-4 * np.abs(coll[one]) + 1e-5).all()
    assert (np.abs(full - plain)[~one] <= 1e-4 * np.abs(plain[~one]) + 1e-5).all()


def test_evaluators_and_recommend_under_full(dev, monkeypatch):
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
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


def test_checkpoint_carries_the_flag(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _full_setup(dev, monkeypatch)
    for k, v in (("epoch", 1), ("save_path", "full_ckpt"), ("load_model", "full_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "full_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["seqAtt"] == "full"
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()                                               # fresh registry, fresh random init
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
    monkeypatch.setattr(args, "seqAtt", "sum")
    with pytest.raises(ValueError, match="seqAtt"):
        rec2.loadModel(str(tmp_path))
    del state["seqAtt"]
    torch.save(state, path)
    rec2.loadModel(str(tmp_path))                                     # no key: sum, which is this run's flag
    monkeypatch.setattr(args, "seqAtt", "full")
    with pytest.raises(ValueError, match="seqAtt"):
        rec2.loadModel(str(tmp_path))


def _profile_kinds(lib, fn):
    from sa_gnn_amd import ops
    lib.sagnn_profile_enable(4096)
    try:
        out = fn()
        kinds = np.zeros(4096, np.int32)
        n = ctypes.c_int(0)
        ops.check(lib.sagnn_profile_read(None, kinds.ctypes.data, None, None, 4096, ctypes.byref(n)))
    finally:
        lib.sagnn_profile_enable(0)
    return out, kinds[:n.value]


def test_off_means_off(dev, monkeypatch):
    """The default flag: two fresh models with the same seed give bit-identical train_loss and testEpoch(), and none
    of the sequence-attention entries (profile kind 5) is launched; under full they are. The issue's "bit-identical" is
    asserted for these forward values only (the two losses, the testEpoch() dict). The gradients of the two
    runs agree to the order of the float atomics that the default path's own backward sums with (sagnn_pair_score_bwd_f32
    and the weight gradients: see test_checkpoint_round_trip_resumes_identically), at test_gpu_fusion_rows.py's bound."""
    from test_gpu_fusion_rows import _check_against
    from sa_gnn_amd import _lib
    from sa_gnn_amd.Params import args as the_args
    assert the_args.seqAtt == "sum"
    lib = _lib.load()
    runs = []
    for _ in range(2):
        rec, handler, NNs, args = _full_setup(dev, monkeypatch, mode="sum")

        def step():
            pre, ssl, grads = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
            return pre, ssl, {k: g for k, g in grads.items() if NNs.params[k].requires_grad}, rec.testEpoch()
        out, kinds = _profile_kinds(lib, step)
        assert len(kinds) > 0 and not (kinds == 5).any()
        runs.append(out)
    (pre_a, ssl_a, g_a, test_a), (pre_b, ssl_b, g_b, test_b) = runs
    assert pre_a == pre_b and ssl_a == ssl_b and test_a == test_b
    assert any(g is not None for g in g_a.values())
    _check_against(g_b, g_a, g_a, "two runs of the default path")
    rec, handler, NNs, args = _full_setup(dev, monkeypatch, mode="full")
    _, kinds = _profile_kinds(lib, lambda: (_loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args)), rec.testEpoch()))
    assert (kinds == 5).any()
