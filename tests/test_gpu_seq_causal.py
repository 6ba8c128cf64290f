"""GPU suite of the causal sequence head and of training on every position (--seqAtt causal, --seqTargets all;
DESIGN.md §26): the causal form of the two attention kernels, the prefix-query kernels, the target kernel and the target
scatter against the float64 restatements of seq_causal_ref, then the Recommender under the two flags (training
objective in every candidate mode and under both samplers, --fusion_rows batch, inference, checkpoints) and the
untouched defaults. Tolerances: test_gpu_seq_att.py's value tolerance and test_gpu_train.py's gradient tolerance."""

import numpy as np
import pytest
import torch

import seq_att_ref as A
import seq_causal_ref as R
from oracle import selfgnn_oracle as O
from test_gpu_seq_att import EPS32, _grad_close, _pad_rows, _value_close

pytestmark = pytest.mark.gpu

CFG = {"T": 2, "L": 2, "leaky": 0.5, "heads": 16}
LENS = {8: [0, 1, 2, 7, 8], 200: [0, 1, 63, 64, 65, 129, 200], 256: [256, 1]}


def _qkv_case(d, heads, P, seed, lens=None):
    """test_gpu_seq_att.py's construction (layer-normed rows through Xavier-uniform weights) at this suite's lengths."""
    rng = np.random.default_rng(seed)
    lens = LENS[P] if lens is None else lens
    x = rng.standard_normal((len(lens) * P, d))
    y = O.layer_norm_td(x[:, None, :], np.ones(d), np.zeros(d), 1e-12)[:, 0, :]
    p = O.init_fusion_params(d, rng, np.float64)
    qkv = np.concatenate([y @ p["W" + c] + p["b" + c] for c in "qkv"], axis=1).astype(np.float32)
    g = rng.standard_normal((len(lens) * P, d)).astype(np.float32)
    return lens, qkv, g


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the causal attention kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [8, 200, 256])
@pytest.mark.parametrize("d,heads", [(32, 16), (64, 8), (64, 16)])
def test_causal_attention_forward_and_backward_against_float64(dev, d, heads, P):
    from sa_gnn_amd import ops
    lens, qkv, g = _qkv_case(d, heads, P, 3 + P + d + heads)
    pad = _pad_rows(lens, P)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    qkv_d = _dev(dev, qkv)
    g_poison = g.copy()
    if len(pad):
        g_poison[pad] = np.nan                                        # padded rows of g_ctx are never read
    ctx = ops.seq_attn(qkv_d, lens_d, P, heads, causal=True)
    dqkv = ops.seq_attn_bwd(qkv_d, _dev(dev, g_poison), lens_d, P, heads, causal=True)
    torch.cuda.synchronize()
    ctx, dqkv = ctx.cpu().numpy(), dqkv.cpu().numpy()
    assert not ctx[pad].any() and not dqkv[pad].any()                 # exact zeros in the padding
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    _value_close(ctx, want, terms, "ctx")
    q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    (R.seq_attn_dense_t(q64, lens, P, heads) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    wg = q64.grad.numpy()
    assert not wg[pad].any()
    for i, name in enumerate(("dq", "dk", "dv")):
        _grad_close(dqkv[:, i * d:(i + 1) * d].astype(np.float64), wg[:, i * d:(i + 1) * d], name)


@pytest.mark.parametrize("d,heads,P,j", [(64, 16, 200, 129), (32, 16, 8, 3), (64, 8, 200, 64)])
def test_a_token_sees_no_later_token(dev, d, heads, P, j):
    """Forward: another q|k|v row at token j leaves the ctx rows before j bit for bit. Backward: a gradient that is
    non-zero in row i alone leaves exact zeros in dk and dv of every later key (and in dq of every other query)."""
    from sa_gnn_amd import ops
    lens, qkv, g = _qkv_case(d, heads, P, 17 + d + heads, lens=[P, max(j + 1, 2)])
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ctx = ops.seq_attn(_dev(dev, qkv), lens_d, P, heads, causal=True).cpu().numpy()
    moved = qkv.copy()
    moved[j] = np.random.default_rng(1).standard_normal(3 * d).astype(np.float32)
    moved[P + j] += 1.0
    ctx2 = ops.seq_attn(_dev(dev, moved), lens_d, P, heads, causal=True).cpu().numpy()
    for b in range(2):
        assert np.array_equal(ctx[b * P:b * P + j], ctx2[b * P:b * P + j])
        assert (ctx[b * P + j:b * P + lens[b]] != ctx2[b * P + j:b * P + lens[b]]).any(1).all()     # token j and the later ones moved
    full = ops.seq_attn(_dev(dev, qkv), lens_d, P, heads).cpu().numpy()
    full2 = ops.seq_attn(_dev(dev, moved), lens_d, P, heads).cpu().numpy()
    assert (full[:j] != full2[:j]).any()                              # the bidirectional form does see it
    one = np.zeros_like(g)
    one[j], one[P + j] = g[j], g[P + j]
    dqkv = ops.seq_attn_bwd(_dev(dev, qkv), _dev(dev, one), lens_d, P, heads, causal=True).cpu().numpy()
    for b in range(2):
        rows = dqkv[b * P:(b + 1) * P]
        assert not rows[j + 1:, d:].any()                             # dk, dv of the keys after the query
        assert not rows[:j, :d].any() and not rows[j + 1:, :d].any()  # dq of the other queries
        assert rows[:j + 1, d:2 * d].any(1).all() and rows[:j + 1, 2 * d:].any(1).all() and rows[j, :d].any()


def test_causal_is_full_on_one_token_and_zero_is_the_old_entry_and_runs_repeat(dev):
    from sa_gnn_amd import _lib, ops
    P, d, heads = 200, 64, 16
    lens, qkv, g = _qkv_case(d, heads, P, 5)
    qkv_d, g_d = _dev(dev, qkv), _dev(dev, g)
    short = torch.tensor([min(n, 1) for n in lens], dtype=torch.int32, device=dev)
    assert torch.equal(ops.seq_attn(qkv_d, short, P, heads, causal=True), ops.seq_attn(qkv_d, short, P, heads))
    assert torch.equal(ops.seq_attn_bwd(qkv_d, g_d, short, P, heads, causal=True), ops.seq_attn_bwd(qkv_d, g_d, short, P, heads))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    lib, n = _lib.load(), len(lens)
    ctx0 = torch.empty((n * P, d), dtype=torch.float32, device=dev)
    dqkv0 = torch.empty((n * P, 3 * d), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ops.check(lib.sagnn_seq_attn_masked_f32(qkv_d.data_ptr(), lens_d.data_ptr(), n, P, d, heads, 0, ctx0.data_ptr(), stream))
    ops.check(lib.sagnn_seq_attn_masked_bwd_f32(qkv_d.data_ptr(), g_d.data_ptr(), lens_d.data_ptr(), n, P, d, heads, 0,
                                                dqkv0.data_ptr(), stream))
    assert torch.equal(ctx0, ops.seq_attn(qkv_d, lens_d, P, heads)) and torch.equal(dqkv0, ops.seq_attn_bwd(qkv_d, g_d, lens_d, P, heads))
    a = ops.seq_attn_bwd(qkv_d, g_d, lens_d, P, heads, causal=True)
    b = ops.seq_attn_bwd(qkv_d, g_d, lens_d, P, heads, causal=True)
    assert torch.equal(a, b) and not torch.equal(a, dqkv0)
    assert torch.equal(ops.seq_attn(qkv_d, lens_d, P, heads, causal=True), ops.seq_attn(qkv_d, lens_d, P, heads, causal=True))
    with pytest.raises(ValueError, match="causal"):
        ops.seq_attn(qkv_d, lens_d, P, heads, causal=2)


@pytest.mark.parametrize("d,heads", [(32, 16), (64, 16), (64, 8)])
def test_causal_attention_beyond_the_exp_range_of_float32(dev, d, heads):
    """test_gpu_seq_att.py's construction and tolerance: scores up to +-150 over a slot's tokens (the causal rows see a
    subset of them), float64 un-shifted. The value tolerance plus 2 (d_k + 4) eps32 S on ctx and on dv."""
    from sa_gnn_amd import ops
    P = 70
    dk = d // heads
    lens, qkv, g = _qkv_case(d, heads, P, 77 + d + heads, lens=[0, 1, 2, 63, 64, 65, 70])
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
    qkv_d = _dev(dev, qkv)
    ctx = ops.seq_attn(qkv_d, lens_d, P, heads, causal=True).cpu().numpy()
    dqkv = ops.seq_attn_bwd(qkv_d, _dev(dev, g), lens_d, P, heads, causal=True).cpu().numpy()
    assert np.isfinite(ctx).all() and np.isfinite(dqkv).all() and not ctx[pad].any() and not dqkv[pad].any()
    want, terms = R.seq_attn_np(qkv.astype(np.float64), lens, P, heads)
    err = np.abs(ctx - want)
    print(f"ctx at |score| <= 150: worst |err| {err.max():.3e}, worst err / tol "
          f"{(err / (1e-4 * np.abs(want) + 1e-5 + (3 * EPS32 + slack) * terms)).max():.3f}")
    assert (err <= 1e-4 * np.abs(want) + 1e-5 + (3 * EPS32 + slack) * terms).all()
    dv = []
    for gg in (g.astype(np.float64), np.abs(g).astype(np.float64)):     # a >= 0: |g| gives sum_j a |g_j|, the terms of dv
        q64 = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
        (R.seq_attn_dense_t(q64, lens, P, heads) * torch.from_numpy(gg)).sum().backward()
        dv.append(q64.grad.numpy()[:, 2 * d:])
    err = np.abs(dqkv[:, 2 * d:] - dv[0])
    assert (err <= 1e-4 * np.abs(dv[0]) + 1e-5 + (3 * EPS32 + slack) * dv[1]).all(), err.max()


# ---- every prefix a query ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,d", [(8, 32), (200, 64), (256, 32)])
def test_prefix_query_and_its_backward_against_float64(dev, P, d):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(P + d)
    lens, leaky = LENS[P], 0.5
    B = len(lens)
    pad = _pad_rows(lens, P)
    x = rng.standard_normal((B * P, d)).astype(np.float32)
    U = rng.standard_normal((B, d)).astype(np.float32)
    dQ = rng.standard_normal((B * P, d)).astype(np.float32)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    x_d, U_d = _dev(dev, x), _dev(dev, U)
    Q = ops.seq_prefix_query(x_d, U_d, lens_d, P, leaky)
    want, terms = R.prefix_query_np(x.astype(np.float64), U.astype(np.float64), lens, P, leaky)
    _value_close(Q.cpu().numpy(), want, terms, "Q")
    assert not Q.cpu().numpy()[pad].any()                             # exact zeros in the padding
    # the slot's last real row: the bits of the pooled row's query
    pooled = ops.leaky_add(ops.seq_pool(x_d, lens_d, P), U_d, leaky)
    last = torch.tensor([b * P + n - 1 for b, n in enumerate(lens) if n], device=dev)
    some = torch.tensor([b for b, n in enumerate(lens) if n], device=dev)
    assert torch.equal(Q.index_select(0, last), pooled.index_select(0, some))
    dQ_poison = dQ.copy()
    if len(pad):
        dQ_poison[pad] = np.nan                                       # padded rows of dQ are never read
    dx, dU = ops.seq_prefix_query_bwd(x_d, _dev(dev, dQ_poison), lens_d, P, leaky)
    dx2, dU2 = ops.seq_prefix_query_bwd(x_d, _dev(dev, dQ_poison), lens_d, P, leaky)
    assert torch.equal(dx, dx2) and torch.equal(dU, dU2)              # no atomics
    wdx, wdU, tx, tu = R.prefix_query_bwd_np(x.astype(np.float64), dQ.astype(np.float64), lens, P, leaky)
    _value_close(dx.cpu().numpy(), wdx, tx, "dx")
    _value_close(dU.cpu().numpy(), wdU, tu, "dU")
    assert not dx.cpu().numpy()[pad].any() and not dU.cpu().numpy()[[b for b, n in enumerate(lens) if n == 0]].any()
    zx, zu = ops.seq_prefix_query_bwd(x_d, torch.zeros_like(x_d), lens_d, P, leaky)
    assert not bool(zx.any()) and not bool(zu.any())                  # a zero dQ: zero gradients, not -0 sums of NaN
    # the autograd node hands both through
    xl, Ul = x_d.clone().requires_grad_(True), U_d.clone().requires_grad_(True)
    from sa_gnn_amd import autograd as ag
    (ag.SeqPrefixQueryFn.apply(xl, Ul, lens_d, P, leaky) * _dev(dev, np.nan_to_num(dQ_poison))).sum().backward()
    assert torch.equal(xl.grad, dx) and torch.equal(Ul.grad, dU)


def _token_case(dev):
    """Five slots at P = 4 over 50 items: three tokens, an inactive slot, an empty one, six items cut to P, one token."""
    seqs = [[5, 6, 7], [8, 9], [], [10, 11, 12, 13, 14, 15], [49]]
    positives, users = [20, -1, 21, 22, 23], [3, 0, 4, 5, 6]
    lens = np.array([len(s) for s in seqs], np.int32)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    items = np.concatenate([np.asarray(s, np.int32) for s in seqs])
    return 4, 50, items, begin, lens, np.asarray(users, np.int32), np.asarray(positives, np.int32)


def test_targets_equal_the_restatement_on_host_built_tokens(dev):
    from sa_gnn_amd import ops
    P, n_items, items, begin, lens, users, positives = _token_case(dev)
    target, excl_row = ops.seq_targets(_dev(dev, items), _dev(dev, begin), _dev(dev, lens), _dev(dev, users), _dev(dev, positives),
                                       P, n_items)
    want_t, want_r = R.seq_targets_np(items, begin, lens, users, positives, P, n_items)
    assert target.dtype == torch.int32 and target.cpu().tolist() == want_t.tolist() and excl_row.cpu().tolist() == want_r.tolist()
    assert want_t.tolist()[:4] == [6, 7, 20, -1] and want_t.tolist()[12:16] == [11, 12, 13, 22]
    # ids outside the catalogue (a smaller n_items) give no target
    target, _ = ops.seq_targets(_dev(dev, items), _dev(dev, begin), _dev(dev, lens), _dev(dev, users), _dev(dev, positives), P, 12)
    assert target.cpu().tolist() == R.seq_targets_np(items, begin, lens, users, positives, P, 12)[0].tolist()
    # more than one block of rows
    rng = np.random.default_rng(2)
    P, B = 200, 9
    lens = rng.integers(0, 260, B).astype(np.int32)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    items = rng.integers(0, 300, int(lens.sum())).astype(np.int32)
    users, positives = rng.integers(0, 40, B).astype(np.int32), rng.integers(-1, 300, B).astype(np.int32)
    target, excl_row = ops.seq_targets(_dev(dev, items), _dev(dev, begin), _dev(dev, lens), _dev(dev, users), _dev(dev, positives),
                                       P, 300)
    want_t, want_r = R.seq_targets_np(items, begin, lens, users, positives, P, 300)
    assert target.cpu().tolist() == want_t.tolist() and excl_row.cpu().tolist() == want_r.tolist()


def test_target_scatter_against_add_at(dev):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(6)
    for d, n_rows, n_items in ((32, 700, 11), (64, 300, 5), (128, 65, 40)):
        dT = rng.standard_normal((n_rows, d)).astype(np.float32)
        target = rng.integers(-1, n_items + 1, n_rows).astype(np.int32)          # -1 and n_items: rows without a target
        target[:50] = 3                                                           # many rows share a target
        base = rng.standard_normal((n_items, d)).astype(np.float32)
        dI = ops.softmax_target_scatter(_dev(dev, base), _dev(dev, dT), _dev(dev, target)).cpu().numpy()
        ok = (target >= 0) & (target < n_items)
        want, terms = base.astype(np.float64), np.abs(base).astype(np.float64)
        np.add.at(want, target[ok], dT[ok].astype(np.float64))
        np.add.at(terms, target[ok], np.abs(dT[ok]).astype(np.float64))
        _value_close(dI, want, terms, f"dI d={d}")


# ---- the Recommender under --seqAtt causal / --seqTargets all ------------------------------------------------------
def _setup(dev, monkeypatch, att="causal", targets="all", negs=0, dist="uniform", d=32, att_layer=2, sampler="host",
           rows="all", loss="softmax"):
    """A tiny model: test_gpu_softmax_loss.py's toy data (70 users, 60 items, 2 intervals) at d = 32, pos_length 8, batch 8.
    With 40 users the same recipe leaves the SSL hinge of the embeddings scaled by 20 so ill-conditioned that meta2's
    gradient, which none of this suite's code touches, misses the gradient tolerance in float32 (2.1 of it, the same
    figure under every head and loss mode); on the data the other suites use its worst ratio is 0.13."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    for k, v in (("predLoss", loss), ("softmaxTemp", 1.0), ("softmaxNegs", negs), ("softmaxNegDist", dist), ("softmaxNegPow", 0.75),
                 ("seqAtt", att), ("seqTargets", targets), ("seqPool", "sum"), ("evaluator", "host"), ("sampler", sampler),
                 ("fusion_rows", rows), ("edgeKeepRate", 1.0), ("adjNorm", "none"), ("edgeTime", "none"), ("rnnCell", "lstm"),
                 ("graphNum", 2), ("gnn_layer", 2), ("latdim", d), ("leaky", 0.5), ("ssldim", 32), ("att_layer", att_layer),
                 ("batch", 8), ("pos_length", 8), ("testSize", 20), ("test", True), ("sslNum", 3), ("pred_num", 2), ("keepRate", 1.0),
                 ("ssl_reg", 0.5), ("reg", 1e-2), ("trnNum", args.trnNum), ("lr", args.lr), ("decay_step", args.decay_step),
                 ("epoch", args.epoch), ("save_path", args.save_path), ("load_model", args.load_model)):
        monkeypatch.setattr(args, k, v)
    rng = np.random.default_rng(31)
    U, I = 70, 60
    tmt = synthetic.make_trn_mat_time(U, I, [700, 650])
    seq = synthetic.make_sequence(tmt)
    tst_int = [int(rng.integers(0, I)) if u % 2 else None for u in range(U)]
    handler = DataHandler.from_memory(tmt, seq, tst_int, {u + 1: list(rng.integers(1, I + 1, size=30)) for u in range(U)})
    rec = Recommender(dev, handler)
    rec.prepareModel()
    g = torch.Generator(device="cpu").manual_seed(9)
    with torch.no_grad():
        for name in list(NNs.params):
            if name.endswith("bias") or name.endswith("beta") or name.endswith("Bias"):
                NNs.params[name].copy_(0.1 * torch.randn(NNs.params[name].shape, generator=g))
        for k in ("uEmbed", "iEmbed", "posEmbed"):
            NNs.params[k].mul_(20)
    return rec, handler, NNs, args


def _batch(rec, handler, args, sampler):
    """(the batch train_loss takes, its host form for the restatement)."""
    from test_gpu_device_sampler import _host_form
    from test_gpu_softmax_loss import _host_batch
    if sampler == "host":
        b = _host_batch(rec, handler, args)
        mask = np.array(b["mask"], copy=True)      # ragged slots: one without tokens, one with one, one with three
        mask[0, :] = 0
        mask[1, :-1] = 0
        mask[2, :-3] = 0
        b = dict(b, mask=mask)
        return b, b
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 1]      # one slot left without a user
    b = rec.sample_batch_device(bat, 31337, 2)
    return b, _host_form(rec, b, args)


def test_targets_equal_the_restatement_on_device_sampled_tokens(dev, monkeypatch):
    """ops.seq_targets on the device sampler's own arrays (the flat seq_items every slot's segment points into, the
    batch's seq_seg) with the slot tables the model builds (Recommender._active_slots / _slot_users_targets), against
    the numpy restatement on the arrays read back and on users / positives taken from the batch's pair lists. The last
    slot has no user (inactive); at pos_length 3 most segments are longer than the slab and are cut; one active slot is
    emptied. Exact."""
    from sa_gnn_amd import ops
    rec, handler, NNs, args = _setup(dev, monkeypatch, sampler="device")
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 1]
    b = rec.sample_batch_device(bat, 31337, 2)
    seq_items = rec._device_sampler().seq_items
    seg_begin, seg_len = b["seq_seg"]
    slot_user, slot_target = rec._slot_users_targets(*rec._active_slots(b))
    # the slot tables, restated from the pair lists: the first pair of each slot in the positive half
    uids, iids, locs = (b[k].cpu().numpy().astype(np.int64) for k in ("uids", "iids", "uLocs_seq"))
    n = len(locs) // 2
    want_user, want_target = np.zeros(args.batch, np.int64), np.full(args.batch, -1, np.int64)
    for e in range(n - 1, -1, -1):
        want_user[locs[e]], want_target[locs[e]] = uids[e], iids[e]
    assert slot_user.cpu().tolist() == want_user.tolist() and slot_target.cpu().tolist() == want_target.tolist()
    assert want_target[args.batch - 1] == -1 and (want_target[:args.batch - 1] >= 0).sum() >= 4
    items_h, begin_h, len_h = seq_items.cpu().numpy(), seg_begin.cpu().numpy(), seg_len.cpu().numpy()
    assert len_h[args.batch - 1] == 0 and len_h.max() > 3 and len(items_h) > int(len_h.sum())      # a shared flat array
    emptied = seg_len.clone()
    first_active = int(np.flatnonzero((want_target >= 0) & (len_h > 1))[0])
    emptied[first_active] = 0                                          # an active slot without tokens
    for P, lens_d in ((args.pos_length, seg_len), (3, seg_len), (args.pos_length, emptied)):
        target, excl_row = ops.seq_targets(seq_items, seg_begin, lens_d, slot_user, slot_target, P, args.item)
        want_t, want_r = R.seq_targets_np(items_h, begin_h, lens_d.cpu().numpy(), want_user, want_target, P, args.item)
        assert target.cpu().tolist() == want_t.tolist() and excl_row.cpu().tolist() == want_r.tolist(), P
        assert (want_t.reshape(args.batch, P)[args.batch - 1] == -1).all() and (want_t >= 0).sum() > (want_target >= 0).sum()
    # what train_loss hands the loss entries is this call's output
    seen = {}
    real = ops.seq_targets

    def spy(*a, **k):
        seen["out"] = real(*a, **k)
        return seen["out"]
    monkeypatch.setattr(ops, "seq_targets", spy)
    rec.train_loss(dict(b), keep_rate=1.0)
    want_t, want_r = R.seq_targets_np(items_h, begin_h, len_h, want_user, want_target, args.pos_length, args.item)
    assert seen["out"][0].cpu().tolist() == want_t.tolist() and seen["out"][1].cpu().tolist() == want_r.tolist()


def _loss_and_grads(rec, NNs, args, batch):
    from test_gpu_softmax_loss import _loss_and_grads as run
    return run(rec, NNs, args, batch)


def _check_all_grads(grads, leaves):
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


@pytest.mark.parametrize("sampler", ["host", "device"])
@pytest.mark.parametrize("negs,dist", [(0, "uniform"), (16, "uniform"), (16, "pop")])
def test_train_loss_on_every_position_against_float64(dev, monkeypatch, negs, dist, sampler):
    _compare_all(dev, monkeypatch, negs, dist, sampler)


def _compare_all(dev, monkeypatch, negs, dist, sampler):
    from sa_gnn_amd import ops
    from sa_gnn_amd.model import banned_table
    from test_gpu_softmax_loss import _oracle_params
    rec, handler, NNs, args = _setup(dev, monkeypatch, negs=negs, dist=dist, sampler=sampler)
    batch, host = _batch(rec, handler, args, sampler)
    batch, host = dict(batch, cand_seed=(77, 3)), dict(host)
    cand = bias = None
    if negs and dist == "pop":
        cand, bias = (v.cpu().numpy() for v in ops.sample_strata_weighted(*rec._pop_cum_device(), negs, 77, 3))
    elif negs:
        cand = ops.sample_strata(args.item, negs, 77, 3, dev).cpu().numpy()
    rows = R.all_rows(host)
    n_slots = len(np.unique(rows[:, 0]))
    print(f"{len(rows)} loss terms from {n_slots} slots (last: one per slot with a positive)")
    assert len(rows) > 2 * n_slots                                    # real sequences: several tokens per slot
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    Pm, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, n_terms = R.torch_train_loss_all(Pm, adj, tp, host, CFG, banned_table(handler, args.item), cand, bias)
    (opre + args.ssl_reg * ossl).backward()
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert n_terms == len(rows)
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    _check_all_grads(grads, leaves)


def test_train_loss_under_causal_with_the_last_target_against_float64(dev, monkeypatch):
    """--seqAtt causal alone (--seqTargets last): test_gpu_softmax_loss.py's objective on the causal head."""
    import softmax_loss_ref as S
    from sa_gnn_amd.model import banned_table
    from test_gpu_softmax_loss import _oracle_params
    rec, handler, NNs, args = _setup(dev, monkeypatch, targets="last")
    batch, _ = _batch(rec, handler, args, "host")
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    Pm, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = S.torch_train_loss_softmax(Pm, adj, tp, batch, CFG, banned_table(handler, args.item), head=R.torch_head_causal)
    (opre + args.ssl_reg * ossl).backward()
    opre_full = float(S.torch_train_loss_softmax(Pm, adj, tp, batch, CFG, banned_table(handler, args.item),
                                                 head=A.torch_head_ragged)[0].detach())
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r} (bidirectional: {opre_full!r})")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(opre - opre_full) > 1e-3 * max(abs(opre), 1.0)
    _check_all_grads(grads, leaves)


@pytest.mark.parametrize("negs", [0, 16])
def test_the_last_tokens_rows_are_the_rows_of_last(dev, monkeypatch, negs):
    """The lse of each slot's last token under all has the bits of the row last computes for the slot: the loss entry's
    rows do not depend on the batch around them, so this pins the query construction and the eligible sets."""
    from sa_gnn_amd import ops
    rec, handler, NNs, args = _setup(dev, monkeypatch, negs=negs)
    batch, host = _batch(rec, handler, args, "host")
    seen = {}
    entry = "softmax_loss_cand" if negs else "softmax_loss"
    real = getattr(ops, entry)

    def spy(Q, I, *a, **k):
        out = real(Q, I, *a, **k)
        target = a[1] if negs else a[0]
        seen[args.seqTargets] = (Q.clone(), target.clone(), out[1].clone())
        return out
    monkeypatch.setattr(ops, entry, spy)
    for mode in ("all", "last"):
        monkeypatch.setattr(args, "seqTargets", mode)
        rec.train_loss(dict(batch, cand_seed=(5, 1)), keep_rate=1.0)
    (Qa, ta, la), (Ql, tl, ll) = seen["all"], seen["last"]
    P = args.pos_length
    n_tok = np.asarray(host["mask"]).sum(1).astype(np.int64)
    slots = np.unique(np.asarray(host["uLocs_seq"])[:len(host["uLocs_seq"]) // 2])
    keep = [i for i, b in enumerate(slots) if n_tok[b] > 0]
    rows = torch.tensor([int(slots[i]) * P + int(n_tok[slots[i]]) - 1 for i in keep], device=dev)
    keep = torch.tensor(keep, device=dev)
    assert len(keep) >= 4 and Qa.shape[0] == args.batch * P and Ql.shape[0] == len(slots)
    assert torch.equal(Qa.index_select(0, rows), Ql.index_select(0, keep))
    assert torch.equal(ta.index_select(0, rows), tl.index_select(0, keep))
    assert torch.equal(la.index_select(0, rows), ll.index_select(0, keep))


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_fusion_rows_batch_gives_the_loss_and_gradients_of_all_rows(dev, monkeypatch, sampler):
    """Nothing new is marked for --fusion_rows batch: the targets are sequence items and the positives in iids."""
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _setup(dev, monkeypatch, negs=16, sampler=sampler)
    batch, _ = _batch(rec, handler, args, sampler)
    res = _both_modes(rec, NNs, args, dict(batch, cand_seed=(5, 1)), 1.0)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    users, items = rec.fusion_rows_counts
    print(f"touched users {users} items {items}; preLoss all {pa!r} batch {pb!r}")
    assert items < args.item or users < args.user
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    _check_against(gb, ga, ga, "batch vs all under --seqTargets all")


def test_one_token_per_sequence_makes_all_last_and_causal_full(dev, monkeypatch):
    from test_gpu_fusion_rows import _check_against
    rec, handler, NNs, args = _setup(dev, monkeypatch)
    batch, _ = _batch(rec, handler, args, "host")
    mask = np.zeros_like(np.asarray(batch["mask"]))
    mask[:, -1] = 1                                                   # every slot: the one item at its last position
    batch = dict(batch, mask=mask)
    out = {}
    for att, targets in (("causal", "all"), ("causal", "last"), ("full", "last")):
        monkeypatch.setattr(args, "seqAtt", att)
        monkeypatch.setattr(args, "seqTargets", targets)
        out[att, targets] = _loss_and_grads(rec, NNs, args, batch)
    (pa, sa, ga), (pl, sl, gl), (pf, sf, gf) = out["causal", "all"], out["causal", "last"], out["full", "last"]
    print(f"preLoss all {pa!r} last {pl!r} full {pf!r}")
    assert pl == pf and sl == sf                                      # the same bits from the attention, the same loss entry
    assert abs(pa - pl) <= 1e-6 * max(abs(pl), 1.0) and sa == sl      # the mean: scale in the entry or a division after it
    trainable = {k: g for k, g in gl.items() if NNs.params[k].requires_grad}
    _check_against(ga, gl, trainable, "all vs last on one-token sequences")
    _check_against(gf, gl, trainable, "full vs causal on one-token sequences")


def test_inference_under_causal(dev, monkeypatch):
    """predict against the float64 restatement of the causal head on the model's own final vectors (the value tolerance),
    the device evaluators against the host ones, recommend against predict (test_gpu_seq_att.py's checks under full)."""
    rec, handler, NNs, args = _setup(dev, monkeypatch, targets="last", loss="hinge")
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    monkeypatch.setattr(args, "evaluator", "device")
    assert rec.testEpoch() == host and rec.testEpochFull() == host_full
    monkeypatch.setattr(args, "evaluator", "host")
    users = np.asarray(handler.tstUsrs, dtype=np.int64)[:args.batch]
    sequence, mask, _, _, target, _ = rec._test_batch(users)
    assert (np.asarray(mask).sum(1) > 1).any()
    locs = np.arange(len(users))
    got = rec.predict(users, target, sequence, mask, locs).cpu().numpy().astype(np.float64)
    t64 = lambda v: v.detach().double().cpu()
    ln = [(t64(g), t64(b)) for g, b in rec.head_ln]
    att_p = [{k: t64(v) for k, v in mh.weights().items()} for mh in rec.multihead_self_attention_sequence]
    fu, fi = t64(rec.final_user_vector), t64(rec.final_item_vector)
    att = R.torch_head_causal(fi, t64(rec.posEmbed), ln, att_p, sequence, mask, args.num_attention_heads, args.leaky)[:len(users)]
    both = A.torch_head_ragged(fi, t64(rec.posEmbed), ln, att_p, sequence, mask, args.num_attention_heads, args.leaky)[:len(users)]
    lk = A._lk_t(att, args.leaky)
    want = ((fu[users] + lk) * fi[target]).sum(1).numpy()
    terms = (((fu[users].abs() + lk.abs()) * fi[target].abs()).sum(1)).numpy()
    # the head's own rounding: test_gpu_seq_att.py bounds a pooled layer output by 1e-4 |att| + 1e-5 per element
    head = ((1e-4 * lk.abs() + 1e-5) * fi[target].abs()).sum(1).numpy()
    err = np.abs(got - want)
    print(f"predict under causal: worst |err| {err.max():.3e} at scale {np.abs(want).max():.3e}")
    assert (err <= 1e-4 * np.abs(want) + 1e-5 + 3 * EPS32 * terms + head).all()
    assert np.abs(want - ((fu[users] + A._lk_t(both, args.leaky)) * fi[target]).sum(1).numpy()).max() > 1e-3   # not the full head
    items, scores = rec.recommend(users, k=args.item, exclude_seen=False)
    at = np.array([scores[r][np.flatnonzero(items[r] == target[r])[0]] for r in range(len(users))], dtype=np.float64)
    assert (np.abs(at - got) <= 1e-4 * np.abs(got) + 1e-5 + 3 * EPS32 * terms).all()


def test_checkpoint_stores_and_checks_causal(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _setup(dev, monkeypatch)
    for k, v in (("epoch", 1), ("save_path", "causal_ckpt"), ("load_model", "causal_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    state = torch.load(str(tmp_path / "Models" / "causal_ckpt"), weights_only=True)
    assert state["seqAtt"] == "causal" and "seqTargets" not in state   # the target mode is not part of the model
    monkeypatch.setattr(args, "seqTargets", "last")
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
    for other in ("full", "sum"):
        monkeypatch.setattr(args, "seqAtt", other)
        with pytest.raises(ValueError, match="seqAtt"):
            rec2.loadModel(str(tmp_path))
    state["seqAtt"] = "full"
    torch.save(state, str(tmp_path / "Models" / "causal_ckpt"))
    monkeypatch.setattr(args, "seqAtt", "causal")
    with pytest.raises(ValueError, match="seqAtt"):                    # a full checkpoint under causal
        rec2.loadModel(str(tmp_path))


def test_training_steps_on_every_position_stay_finite_and_improve(dev, monkeypatch):
    rec, handler, NNs, args = _setup(dev, monkeypatch, negs=16, sampler="device", rows="batch", att_layer=1)
    for k, v in (("trnNum", 32), ("lr", 5e-3), ("keepRate", 0.5), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay_step", 32 // args.batch)):
        monkeypatch.setattr(args, k, v)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["preLoss"] for _ in range(8)]
    print("preLoss per epoch:", losses)
    assert all(np.isfinite(losses)) and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert all(bool(torch.isfinite(p).all()) for p in NNs.params.values())


# ---- off means off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("att", ["sum", "full"])
def test_off_means_off(dev, monkeypatch, att):
    """With the defaults, and with --seqAtt full, a seeded step calls none of the new wrappers, hands ops.seq_attn /
    seq_attn_bwd the argument lists they had, and its attention layer returns, forward and backward, the bits of the same
    composition made from ops calls that reach the old entries only. Two fresh models give bit-identical losses and
    test epochs, and gradients equal to the order of the float atomics the default backward sums with, at
    test_gpu_fusion_rows.py's bound (what test_gpu_seq_att.py::test_off_means_off asserts of the parent's path)."""
    from sa_gnn_amd import autograd as ag, ops
    from sa_gnn_amd.Params import args as the_args
    from test_gpu_fusion_rows import _check_against
    from test_gpu_softmax_loss import _host_batch
    assert the_args.seqAtt == "sum" and the_args.seqTargets == "last" and the_args.seqMask == "none"

    def never(*a, **k):
        raise AssertionError("a wrapper of --seqAtt causal / --seqTargets all ran with the flags off")
    for name in ("seq_prefix_query", "seq_prefix_query_bwd", "seq_targets", "softmax_target_scatter"):
        monkeypatch.setattr(ops, name, never)
    calls = []
    real_f, real_b = ops.seq_attn, ops.seq_attn_bwd

    def fwd(*a, **k):
        calls.append((len(a), k))
        return real_f(*a, **k)

    def bwd(*a, **k):
        calls.append((len(a), k))
        return real_b(*a, **k)
    monkeypatch.setattr(ops, "seq_attn", fwd)
    monkeypatch.setattr(ops, "seq_attn_bwd", bwd)
    runs = []
    for _ in range(2):
        rec, handler, NNs, args = _setup(dev, monkeypatch, att=att, targets="last", negs=16, rows="batch")
        pre, ssl, grads = _loss_and_grads(rec, NNs, args, dict(_host_batch(rec, handler, args), cand_seed=(5, 1)))
        runs.append((pre, ssl, rec.testEpoch(), {k: g for k, g in grads.items() if NNs.params[k].requires_grad}))
    assert runs[0][:3] == runs[1][:3]
    assert sum(g is not None for g in runs[0][3].values()) >= 20
    _check_against(runs[1][3], runs[0][3], runs[0][3], f"two runs under --seqAtt {att}")
    if att == "sum":
        assert not calls
        return
    assert calls and all(c == (4, {}) or c == (5, {}) for c in calls)          # (qkv, seg_len, P, heads) / with g_ctx: no mask
    # one layer, by hand from the old entries
    rng = np.random.default_rng(12)
    P, d, heads, lens = 8, 32, 16, [0, 1, 2, 7, 8]
    p = O.init_fusion_params(d, rng, np.float32)
    names = ("ln_gamma", "ln_beta", "Wq", "bq", "Wk", "bk", "Wv", "bv")
    x = _dev(dev, rng.standard_normal((len(lens) * P, d)).astype(np.float32)).requires_grad_(True)
    w = {k: _dev(dev, p[k].astype(np.float32)).requires_grad_(True) for k in names}
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    g = _dev(dev, rng.standard_normal((len(lens) * P, d)).astype(np.float32))
    g[torch.from_numpy(_pad_rows(lens, P)).to(dev)] = 0.0              # the layer's contract: zero gradient rows in the padding
    out = ag.SeqAttnFn.apply(x, *(w[k] for k in names), lens_d, P, heads, 0.5)
    out.backward(g)
    with torch.no_grad():
        xd, wd = x.detach(), {k: v.detach() for k, v in w.items()}
        R_ = xd.shape[0]
        y = ops.layernorm_td(xd.view(R_, 1, d), wd["ln_gamma"], wd["ln_beta"]).view(R_, d)
        Wqkv = torch.cat([wd["Wq"], wd["Wk"], wd["Wv"]], 1).contiguous()
        qkv = ops.dense_nn(y, Wqkv, torch.cat([wd["bq"], wd["bk"], wd["bv"]]).contiguous())
        att_ = real_f(qkv, lens_d, P, heads)
        assert torch.equal(out.detach(), ops.leaky_add(att_, xd, 0.5))
        # the backward, by hand from the old backward entry and the row-wise ops SeqAttnFn.backward names. The slab's 40
        # rows give the weight-gradient product at most two partial sums onto zero, so its float atomics have one result
        dqkv = real_b(qkv, ops.leaky_bwd(att_, g, 0.5), lens_d, P, heads)
        dW, db = torch.zeros((d, 3 * d), device=dev), torch.zeros(3 * d, device=dev)
        ops.dense_tn(y, dqkv, dW, db)
        dy = ops.dense_nn(dqkv, Wqkv.t().contiguous(), None).view(R_, 1, d)
        dy, _, _ = ops.layernorm_td_bwd(xd.view(R_, 1, d), dy, wd["ln_gamma"], out=dy)
        assert torch.equal(x.grad, ops.leaky_add(dy.view(R_, d), g, 1.0))
        for i, c in enumerate("qkv"):
            assert torch.equal(w["W" + c].grad, dW[:, i * d:(i + 1) * d]), c
            assert torch.equal(w["b" + c].grad, db[i * d:(i + 1) * d]), c
