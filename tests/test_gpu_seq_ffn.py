"""GPU suite of --seqFFN: the fused feed-forward kernels against the float64 restatement of seq_ffn_ref
(values, all seven gradients, padding, determinism, independence of a row from its place in a tile, offsets past 2^31),
then the block inside the Recommender (training objective under both samplers and masks, --fusion_rows batch,
--seqTargets all, --seqPool additive, inference, checkpoints, a few optimiser steps) and the untouched default."""
import functools

import numpy as np
import pytest
import torch

import seq_att_ref as A
import seq_causal_ref as C
import seq_ffn_ref as F
from oracle import selfgnn_oracle as O
from test_gpu_seq_att import (CFG, EPS32, _full_setup, _grad_close, _host_batch, _loss_and_grads, _pad_rows, _value_close)

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (32, 128), (64, 64), (64, 256), (128, 128)]
GRADS = ("dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2")


def _lens(P):
    """Every tile edge of a 16-wide tiling, the empty slot, and the full slot last: the slab ends at the buffer's end."""
    return [min(n, P) for n in (0, 1, 15, 16, 17, 31, 32, 33, 64, 65, P)]


def _params(rng, d, f):
    lim = np.sqrt(6.0 / (d + f))
    p = {"gamma": 1 + 0.1 * rng.standard_normal(d), "beta": 0.1 * rng.standard_normal(d),
         "W1": rng.uniform(-lim, lim, (d, f)), "b1": 0.1 * rng.standard_normal(f),
         "W2": rng.uniform(-lim, lim, (f, d)), "b2": 0.1 * rng.standard_normal(d)}
    return {k: v.astype(np.float32) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _case(d, f, P):
    rng = np.random.default_rng(1000 * d + 10 * f + P)
    lens = _lens(P)
    x = rng.standard_normal((len(lens) * P, d)).astype(np.float32)
    g = rng.standard_normal((len(lens) * P, d)).astype(np.float32)
    p = _params(rng, d, f)
    for a in (x, g, *p.values()):
        a.setflags(write=False)
    return lens, x, g, p


@functools.lru_cache(maxsize=None)
def _reference(d, f, P, leaky):
    """(out, term sums, the seven gradients) in float64 on the float32 inputs of _case; computed once per case."""
    lens, x, g, p = _case(d, f, P)
    return _reference_of(lens, x, g, p, P, leaky)


def _reference_of(lens, x, g, p, P, leaky):
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    out, terms = F.seq_ffn_np(x.astype(np.float64), p64, lens, P, leaky)
    leaves = [torch.from_numpy(np.nan_to_num(x).astype(np.float64)).requires_grad_(True)]
    leaves += [torch.from_numpy(p64[k]).requires_grad_(True) for k in F.KEYS]
    (F.seq_ffn_t(leaves[0], dict(zip(F.KEYS, leaves[1:])), lens, P, leaky) * torch.from_numpy(np.nan_to_num(g).astype(np.float64))).sum().backward()
    return out, terms, [t.grad.numpy() for t in leaves]


def _run(dev, lens, x, g, p, P, leaky):
    """(out, dx, dgamma, dbeta, dW1, db1, dW2, db2) of the two entries as numpy arrays."""
    from sa_gnn_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    x_d, g_d = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(g)).to(dev)
    pd = [torch.from_numpy(np.array(p[k])).to(dev) for k in F.KEYS]
    out = ops.seq_ffn(x_d, *pd, lens_d, P, leaky)
    grads = ops.seq_ffn_bwd(x_d, g_d, *pd, lens_d, P, leaky)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (out, *grads)]


def _poisoned(lens, x, g, P, fill=np.nan):
    pad = _pad_rows(lens, P)
    x2, g2 = x.copy(), g.copy()
    if np.isscalar(fill):
        x2[pad], g2[pad] = fill, fill
    else:
        x2[pad], g2[pad] = fill(x2[pad].shape), fill(g2[pad].shape)
    return pad, x2, g2


@pytest.mark.parametrize("leaky", [0.5, 0.0])
@pytest.mark.parametrize("P", [8, 72, 256])
@pytest.mark.parametrize("d,f", SHAPES)
def test_forward_and_backward_against_float64(dev, d, f, P, leaky):
    lens, x, g, p = _case(d, f, P)
    pad, xn, gn = _poisoned(lens, x, g, P)                             # NaN in the padded rows of x and g: never read
    got = _run(dev, lens, xn, gn, p, P, leaky)
    assert not got[0][pad].any() and not got[1][pad].any()            # exact zeros in the padding
    want, terms, wg = _reference(d, f, P, leaky)
    _value_close(got[0].astype(np.float64), want, terms, "out")
    assert not wg[0][pad].any()
    for name, a, b in zip(GRADS, got[1:], wg):
        assert a.shape == b.shape, name
        _grad_close(a.astype(np.float64), b, name)


@pytest.mark.parametrize("d,f,P", [(64, 256, 72), (32, 32, 8), (128, 128, 256)])
def test_runs_repeat_and_the_padding_is_not_read(dev, d, f, P):
    """Two runs give the same bits in all eight outputs, and refilling the padded rows of x and g with +-1e3 leaves
    every bit."""
    lens, x, g, p = _case(d, f, P)
    a, b = _run(dev, lens, x, g, p, P, 0.5), _run(dev, lens, x, g, p, P, 0.5)
    rng = np.random.default_rng(1)
    pad, xl, gl = _poisoned(lens, x, g, P, lambda shape: np.where(rng.random(shape) < 0.5, -1e3, 1e3).astype(np.float32))
    c = _run(dev, lens, xl, gl, p, P, 0.5)
    for name, u, v, w in zip(("out",) + GRADS, a, b, c):
        assert np.isfinite(u).all() and np.abs(u).max() > 0, name
        assert np.array_equal(u, v), f"{name}: two runs differ"
        assert np.array_equal(u, w), f"{name}: the padding was read"


@pytest.mark.parametrize("d,f,P", [(64, 256, 72), (32, 128, 256), (128, 128, 72)])
def test_a_row_does_not_depend_on_its_place_in_a_tile(dev, d, f, P):
    """The same token rows, moved on by 5 places (the last 5 first), dealt into slots of 64: the first arrangement's
    slots start at token 0, 1 or 2 mod 16 and the second's at 0, so every row changes lane and most change tile. Each
    row keeps its bits in out and dx."""
    lens, x, g, p = _case(d, f, P)
    real = np.setdiff1d(np.arange(len(x)), _pad_rows(lens, P))
    n = len(real)
    lens2 = [64] * (n // 64) + ([n % 64] if n % 64 else [])
    assert sum(lens2) == n and max(lens2) <= P
    real2 = np.roll(np.setdiff1d(np.arange(len(lens2) * P), _pad_rows(lens2, P)), -5)      # token k sits at place k + 5
    assert ((real % P) % 16 != (real2 % P) % 16).all()                # every row changes lane
    x2, g2 = np.zeros((len(lens2) * P, d), np.float32), np.zeros((len(lens2) * P, d), np.float32)
    x2[real2], g2[real2] = x[real], g[real]
    a, b = _run(dev, lens, x, g, p, P, 0.5), _run(dev, lens2, x2, g2, p, P, 0.5)
    assert np.array_equal(a[0][real], b[0][real2]) and np.array_equal(a[1][real], b[1][real2])
    assert np.abs(a[0][real]).max() > 0 and np.abs(a[1][real]).max() > 0
    for name, u, v in zip(GRADS[1:], a[2:], b[2:]):                   # the sums run in another order: close, not equal
        _grad_close(v.astype(np.float64), u.astype(np.float64), name)


def test_offsets_past_2_to_the_31(dev):
    """16,400 slots of P = 256 at (64, 256), all empty but the last three (17, 0 and 256 tokens): the workspace rows of
    the last slot lie past 2^31 elements."""
    from sa_gnn_amd import ops
    n, P, d, f, leaky = 16400, 256, 64, 256, 0.5
    if torch.cuda.mem_get_info()[0] < 16 * 2 ** 30:
        pytest.skip("needs 16 GB of free device memory")
    assert (n - 1) * P * 2 * f > 2 ** 31
    rng = np.random.default_rng(9)
    tail = [17, 0, 256]
    xs, gs = (rng.standard_normal((3 * P, d)).astype(np.float32) for _ in range(2))
    pad, xs, gs = _poisoned(tail, xs, gs, P)
    p = _params(rng, d, f)
    lens = torch.zeros(n, dtype=torch.int32, device=dev)
    lens[-3:] = torch.tensor(tail, dtype=torch.int32, device=dev)
    x, g = (torch.full((n * P, d), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    x[-3 * P:], g[-3 * P:] = torch.from_numpy(xs).to(dev), torch.from_numpy(gs).to(dev)
    pd = [torch.from_numpy(p[k]).to(dev) for k in F.KEYS]
    out = ops.seq_ffn(x, *pd, lens, P, leaky)
    assert int(torch.count_nonzero(out[:-3 * P])) == 0
    got = [out[-3 * P:].cpu().numpy()]
    del out
    grads = ops.seq_ffn_bwd(x, g, *pd, lens, P, leaky)
    assert int(torch.count_nonzero(grads[0][:-3 * P])) == 0
    got += [grads[0][-3 * P:].cpu().numpy()] + [t.cpu().numpy() for t in grads[1:]]
    del grads, x, g
    torch.cuda.empty_cache()
    assert not got[0][pad].any() and not got[1][pad].any()
    want, terms, wg = _reference_of(tail, xs, gs, p, P, leaky)
    _value_close(got[0].astype(np.float64), want, terms, "out")
    for name, a, b in zip(GRADS, got[1:], wg):
        _grad_close(a.astype(np.float64), b, name)


# ---- the Recommender under --seqFFN ----------------------------------------------------------------------------------
def _ffn_setup(dev, monkeypatch, ffn=64, mode="full", heads=0, setup=_full_setup, **kw):
    from sa_gnn_amd.Params import args
    monkeypatch.setattr(args, "seqFFN", ffn)
    monkeypatch.setattr(args, "seqHeads", heads)
    out = setup(dev, monkeypatch, mode=mode, **kw) if setup is _full_setup else setup(dev, monkeypatch, **kw)
    g = torch.Generator(device="cpu").manual_seed(17)                 # the setups draw the variables named *bias / *beta
    with torch.no_grad():
        for name, v in out[2].params.items():
            if name.startswith("seq_ffn") and name[-3:] in ("_b1", "_b2"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
    return out


def _ffn_names(args):
    return [[f"seq_ffn{i}_{s}" for s in ("ln_gamma", "ln_beta", "W1", "b1", "W2", "b2")] for i in range(args.att_layer)]


def _ffn_leaves(NNs, args, leaves=None):
    """The blocks' parameters as float64 leaves, one dict per attention layer; added to `leaves` under their names."""
    out = []
    for names in _ffn_names(args):
        t = [NNs.params[n].detach().cpu().double().requires_grad_(True) for n in names]
        if leaves is not None:
            leaves.update(zip(names, t))
        out.append(dict(zip(F.KEYS, t)))
    return out


def _spy(monkeypatch):
    from sa_gnn_amd import ops
    counts = {}
    for name in ("seq_ffn", "seq_ffn_bwd", "seq_ffn_supported"):
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


def _graphs(handler):
    return [O.trans_to_lsts(m)[0] for m in handler.subMat], [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]


@pytest.mark.parametrize("sampler,mode,heads", [("host", "full", 0), ("device", "full", 2), ("host", "causal", 0),
                                                ("device", "causal", 0)])
def test_train_loss_against_float64(dev, monkeypatch, sampler, mode, heads):
    from test_gpu_device_sampler import _host_form
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 64, mode, heads)
    counts = _spy(monkeypatch)
    if sampler == "host":
        batch = host = _host_batch(rec, handler, args)
    else:
        batch = rec.sample_batch_device(np.random.default_rng(3).permutation(args.user)[:args.batch - 3], 31337, 2)
        host = _host_form(rec, batch, args)
    assert (np.asarray(host["mask"]).sum(1) > 1).any()               # real sequences: more than one token per slot
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_ffn") == args.att_layer and counts.get("seq_ffn_bwd") == args.att_layer
    P, leaves = _oracle_params(rec, NNs)
    ffn = _ffn_leaves(NNs, args, leaves)
    adj, tp = _graphs(handler)
    causal = mode == "causal"
    opre, ossl, _, _ = A.torch_train_loss_full(P, adj, tp, host, CFG, head=F.torch_head_ffn(ffn, causal=causal, heads=heads or None))
    (opre + args.ssl_reg * ossl).backward()
    without = float(A.torch_train_loss_full(P, adj, tp, host, CFG, head=F.torch_head_ffn(None, causal=causal, heads=heads or None))[0].detach())
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r} (without the blocks: {without!r}); sslloss {ssl!r} vs {ossl!r}")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    assert abs(pre - without) > 1e-4 * max(abs(without), 1.0)        # the blocks are part of the function
    _check_grads(grads, leaves, least=20 + 6 * args.att_layer)
    for names in _ffn_names(args):
        for n in names:
            assert float(grads[n].abs().max()) > 0, n


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_fusion_rows_batch_equals_all(dev, monkeypatch, sampler):
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 64)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    b = rec._host_train_batch(bat) if sampler == "host" else rec.sample_batch_device(bat, 2024, 1)
    res = _both_modes(rec, NNs, args, b, 1.0)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    assert rec.fusion_rows_counts[1] < args.item or rec.fusion_rows_counts[0] < args.user
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    _check_against(gb, ga, ga, "batch vs all under --seqFFN 64")


def test_every_position_a_target_runs_a_finite_step_and_matches_float64_on_the_loss(dev, monkeypatch):
    """--seqTargets all with --predLoss softmax at latdim 32."""
    import test_gpu_seq_causal as T
    from sa_gnn_amd.model import banned_table
    from test_gpu_softmax_loss import _oracle_params
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 128, setup=T._setup)
    counts = _spy(monkeypatch)
    batch, host = T._batch(rec, handler, args, "host")
    pre, ssl, grads = T._loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_ffn_bwd") == args.att_layer
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())
    monkeypatch.setattr(C, "torch_head_slabs", F.torch_head_ffn_slabs(_ffn_leaves(NNs, args), causal=True))
    Pm, _ = _oracle_params(rec, NNs)
    adj, tp = _graphs(handler)
    opre, ossl, n_terms = C.torch_train_loss_all(Pm, adj, tp, host, T.CFG, banned_table(handler, args.item))
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"{n_terms} terms; preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert np.isfinite(pre) and abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)


def test_additive_pooling_runs_a_finite_step_and_matches_float64_on_the_loss(dev, monkeypatch):
    import test_gpu_seq_pool as T
    from test_gpu_train import _oracle_params
    from sa_gnn_amd.Params import args as the_args
    monkeypatch.setattr(the_args, "seqFFN", 64)
    rec, handler, NNs, args = T._add_setup(dev, monkeypatch)
    counts = _spy(monkeypatch)
    batch = _host_batch(rec, handler, args)
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    assert counts.get("seq_ffn_bwd") == args.att_layer
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())
    P, _ = _oracle_params(rec, NNs)
    adj, tp = _graphs(handler)
    pool = tuple(NNs.params[n].detach().cpu().double() for n in T.ADD_NAMES)
    opre, ossl, _, _ = A.torch_train_loss_full(P, adj, tp, batch, CFG, head=F.torch_head_ffn(_ffn_leaves(NNs, args), pool=pool))
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert np.isfinite(pre) and abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)


def test_evaluators_recommend_and_the_float64_head(dev, monkeypatch):
    from test_gpu_train import _oracle_params
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 64)
    counts = _spy(monkeypatch)
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    assert counts.get("seq_ffn", 0) > 0 and "seq_ffn_bwd" not in counts
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
    # the head's rows against the float64 head on the model's own final item vectors, with and without the blocks
    P, _ = _oracle_params(rec, NNs)
    with torch.no_grad():
        fi64 = rec.final_item_vector.double().cpu()
        want = F.torch_head_ffn(_ffn_leaves(NNs, args))(fi64, P["posEmbed"], P["ln"], P["att"], sequence, mask, CFG["heads"], args.leaky)
        bare = F.torch_head_ffn(None)(fi64, P["posEmbed"], P["ln"], P["att"], sequence, mask, CFG["heads"], args.leaky)
    want, bare = want.numpy()[:len(users)], bare.numpy()[:len(users)]
    _grad_close(att, want, "att_user against the float64 head")
    assert np.abs(bare - want).max() > 1e-2 * np.abs(want).max()
    monkeypatch.setattr(args, "seqFFN", 0)                            # the blocks are part of the function
    assert np.abs(rec.predict(users, target, sequence, mask, locs).cpu().numpy() - p_full).max() > 1e-4 * np.abs(p_full).max()


def test_checkpoint_carries_the_hidden_width(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 64)
    for k, v in (("epoch", 1), ("save_path", "ffn_ckpt"), ("load_model", "ffn_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "ffn_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["seqFFN"] == 64 and state["seqAtt"] == "full" and "seq_ffn1_W2" in state["params"]
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()                                               # fresh registry, fresh random init
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
    for other in (128, 0):
        monkeypatch.setattr(args, "seqFFN", other)
        with pytest.raises(ValueError, match="seqFFN"):
            rec2.loadModel(str(tmp_path))
    del state["seqFFN"]                                               # no key: counts as 0
    torch.save(state, path)
    monkeypatch.setattr(args, "seqFFN", 64)
    with pytest.raises(ValueError, match="seqFFN 0"):
        rec2.loadModel(str(tmp_path))


def test_training_steps_stay_finite(dev, monkeypatch):
    """Forty optimiser steps at ten times the learning rate: losses and every parameter stay finite, the blocks'
    parameters move, and the evaluator still ranks."""
    rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 256, d=64, ssldim=32, att_layer=1)
    for k, v in (("trnNum", 64), ("lr", 2e-2), ("keepRate", 1.0), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay", 1.0)):
        monkeypatch.setattr(args, k, v)
    monkeypatch.setattr(args, "decay_step", args.trnNum // args.batch)
    start = {n: NNs.params[n].detach().clone() for n in _ffn_names(args)[0]}
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["Loss"] for _ in range(10)]          # 4 steps each
    assert rec.optimizer.global_step == 40 and np.isfinite(losses).all(), losses
    for k, v in NNs.params.items():
        assert bool(torch.isfinite(v).all()), k
    for n, v in start.items():
        assert not torch.equal(NNs.params[n], v), f"{n} did not train"
    rec.forward()
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    assert bool(torch.isfinite(rec.predict(users, target, sequence, mask, np.arange(len(users)))).all())


def _raising_ops(monkeypatch):
    from sa_gnn_amd import ops

    def refuse(*a, **k):
        raise AssertionError("a --seqFFN entry was called")
    for name in ("seq_ffn", "seq_ffn_bwd", "seq_ffn_supported"):
        monkeypatch.setattr(ops, name, refuse)


@pytest.mark.parametrize("mode", ["sum", "full"])
def test_off_means_off(dev, monkeypatch, mode):
    """--seqFFN 0: the parameter names, shapes and initial values and both losses have the bits of a run with the new
    ops replaced by functions that raise; under --seqFFN F every pre-existing variable starts with the bits it has at 0."""
    from sa_gnn_amd.Params import args as the_args
    assert the_args.seqFFN == 0 and the_args.seqAtt == "sum"
    runs = []
    for raising in (False, True):
        if raising:
            _raising_ops(monkeypatch)
        rec, handler, NNs, args = _full_setup(dev, monkeypatch, mode=mode)
        init = {k: v.detach().cpu().clone() for k, v in NNs.params.items()}
        assert rec.seq_ffn == [] and not any(k.startswith("seq_ffn") for k in init)
        pre, ssl, _ = _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args))
        runs.append((init, pre, ssl, rec.testEpoch()))
        monkeypatch.undo()
    (init_a, *rest_a), (init_b, *rest_b) = runs
    assert rest_a == rest_b and list(init_a) == list(init_b)
    for k in init_a:
        assert init_a[k].shape == init_b[k].shape and torch.equal(init_a[k], init_b[k]), k
    if mode == "full":
        rec, handler, NNs, args = _ffn_setup(dev, monkeypatch, 64)
        names = [n for layer in _ffn_names(args) for n in layer]
        assert list(NNs.params) == list(init_a) + names               # defined after every other variable
        for k in init_a:
            assert torch.equal(NNs.params[k].detach().cpu(), init_a[k]), k
        from sa_gnn_amd.model import Recommender
        rec = Recommender(dev, handler)
        rec.prepareModel()                                            # the initial values as prepareModel leaves them
        d = args.latdim
        assert len(rec.seq_ffn) == args.att_layer
        for gm, bt, W1, b1, W2, b2 in rec.seq_ffn:
            assert W1.shape == (d, 64) and W2.shape == (64, d) and b1.shape == (64,) and b2.shape == (d,)
            assert gm.shape == (d,) and bt.shape == (d,)
            assert bool((gm == 1).all()) and not bt.any() and not b1.any() and not b2.any() and W1.any() and W2.any()
        assert list(NNs.params) == list(init_a) + names and not any(n in NNs.regParams for n in names)   # none L2-regularised
