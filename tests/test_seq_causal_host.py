"""CPU suite of the causal sequence head and of training on every position (--seqAtt causal, --seqTargets all;
DESIGN.md §26): the float64 restatements of seq_causal_ref agree with each other and with torch autograd, the causal
form is the dense form under a lower-triangular mask, the target rule holds on hand-written sequences, the flags
parse and prepareModel refuses the combinations the issue names, and the new entries reject bad arguments before any
device work (so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
import torch

import seq_att_ref as A
import seq_causal_ref as R
from sa_gnn_amd import _lib


@pytest.mark.parametrize("d,heads,P,lens", [(16, 4, 6, [0, 1, 6, 3]), (32, 16, 9, [9, 2, 0, 5]), (32, 4, 5, [1, 1, 4])])
def test_causal_restatements_agree_and_equal_the_dense_form_under_a_lower_triangular_mask(d, heads, P, lens):
    rng = np.random.default_rng(d + heads + P)
    qkv = rng.standard_normal((len(lens) * P, 3 * d))
    ctx, terms = R.seq_attn_np(qkv, lens, P, heads)
    ragged = R.seq_attn_t(torch.from_numpy(qkv), lens, P, heads).numpy()
    dense = R.seq_attn_dense_t(torch.from_numpy(qkv), lens, P, heads).numpy()
    np.testing.assert_allclose(ragged, ctx, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dense, ctx, rtol=1e-13, atol=1e-13)
    assert (terms >= np.abs(ctx) - 1e-12).all()
    # the dense form without the triangle is the bidirectional restatement: the mask is the only difference
    full, _ = A.seq_attn_np(qkv, lens, P, heads)
    np.testing.assert_allclose(R.seq_attn_dense_t(torch.from_numpy(qkv), lens, P, heads, causal=False).numpy(), full,
                               rtol=1e-13, atol=1e-13)
    for b, n in enumerate(lens):
        if n:                       # a slot's last token sees every token: the row the bidirectional form gives it
            np.testing.assert_allclose(ctx[b * P + n - 1], full[b * P + n - 1], rtol=1e-13, atol=1e-13)
        if n > 1:
            assert np.abs(ctx[b * P:b * P + n - 1] - full[b * P:b * P + n - 1]).max() > 1e-6


def test_causal_gradients_agree_between_the_ragged_and_the_dense_form():
    rng = np.random.default_rng(3)
    d, heads, P, lens = 16, 4, 7, [0, 1, 7, 4]
    qkv = rng.standard_normal((len(lens) * P, 3 * d))
    g = torch.from_numpy(rng.standard_normal((len(lens) * P, d)))
    grads = []
    for form in (R.seq_attn_t, R.seq_attn_dense_t):
        leaf = torch.from_numpy(qkv).requires_grad_(True)
        (form(leaf, lens, P, heads) * g).sum().backward()
        grads.append(leaf.grad.numpy())
    np.testing.assert_allclose(grads[0], grads[1], rtol=1e-11, atol=1e-12)
    for b, n in enumerate(lens):
        assert not grads[0][b * P + n:(b + 1) * P].any()


def test_a_later_token_does_not_move_an_earlier_row_of_the_restatement():
    rng = np.random.default_rng(4)
    d, heads, P, lens = 16, 4, 6, [6]
    qkv = rng.standard_normal((P, 3 * d))
    ctx, _ = R.seq_attn_np(qkv, lens, P, heads)
    moved = qkv.copy()
    moved[3] += 1.0
    ctx2, _ = R.seq_attn_np(moved, lens, P, heads)
    assert np.array_equal(ctx[:3], ctx2[:3]) and (ctx[3:] != ctx2[3:]).any(1).all()


def test_prefix_query_restatements_agree_with_autograd():
    rng = np.random.default_rng(5)
    d, P, lens, leaky = 8, 6, [0, 1, 6, 3], 0.5
    x = rng.standard_normal((len(lens) * P, d))
    U = rng.standard_normal((len(lens), d))
    dQ = rng.standard_normal((len(lens) * P, d))
    Q, terms = R.prefix_query_np(x, U, lens, P, leaky)
    xt, Ut = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(U).requires_grad_(True)
    Qt = R.prefix_query_t(xt, Ut, lens, P, leaky)
    np.testing.assert_allclose(Qt.detach().numpy(), Q, rtol=1e-13, atol=1e-13)
    (Qt * torch.from_numpy(dQ)).sum().backward()
    dx, dU, tx, tu = R.prefix_query_bwd_np(x, dQ, lens, P, leaky)
    np.testing.assert_allclose(xt.grad.numpy(), dx, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(Ut.grad.numpy(), dU, rtol=1e-12, atol=1e-13)
    assert (terms >= np.abs(Q) - 1e-12).all() and (tx >= np.abs(dx) - 1e-12).all() and (tu >= np.abs(dU) - 1e-12).all()
    for b, n in enumerate(lens):
        assert not Q[b * P + n:(b + 1) * P].any() and not dx[b * P + n:(b + 1) * P].any()
        if n:                       # the last real row is the pooled row's query
            np.testing.assert_allclose(Q[b * P + n - 1], np.maximum(leaky * x[b * P:b * P + n].sum(0), x[b * P:b * P + n].sum(0)) + U[b],
                                       rtol=1e-13, atol=1e-13)


def test_targets_on_hand_written_sequences():
    P, n_items = 4, 50
    #        slot 0: three tokens     slot 1: inactive   slot 2: empty   slot 3: six items, cut to P   slot 4: one token
    seqs = [[5, 6, 7], [8, 9], [], [10, 11, 12, 13, 14, 15], [49]]
    positives = [20, -1, 21, 22, 23]
    users = [3, 0, 4, 5, 6]
    items = np.concatenate([np.asarray(s, np.int64) for s in seqs])
    lens = np.array([len(s) for s in seqs])
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]])
    target, excl_row = R.seq_targets_np(items, begin, lens, users, positives, P, n_items)
    want = [6, 7, 20, -1,
            -1, -1, -1, -1,
            -1, -1, -1, -1,
            11, 12, 13, 22,            # the slab holds the first P items; its last token trains against the positive
            23, -1, -1, -1]
    assert target.tolist() == want
    assert excl_row.tolist() == [u for u in users for _ in range(P)]
    assert R.slot_targets([5, 6, 7], 20) == [6, 7, 20] and R.slot_targets([], 21) == [] and R.slot_targets([49], 23) == [23]
    # ids outside the catalogue give no target: a positive of 50 and a sequence item of 50
    target, _ = R.seq_targets_np(np.array([1, 50, 2]), [0], [3], [0], [50], P, n_items)
    assert target.tolist() == [-1, 2, -1, -1]


def test_flags_parse_and_default_to_the_present_behaviour():
    """The causal head form is args.seqAtt == "causal"; on the command line it is spelled --seqAtt full --seqMask causal,
    because --seqAtt's own choices stay {sum, full} (tests/test_seq_att_host.py pins them)."""
    from sa_gnn_amd import Params
    p = Params.build_parser()
    d = p.parse_args([])
    assert d.seqTargets == "last" and d.seqMask == "none" and d.seqAtt == "sum"
    assert Params.args.seqTargets == "last" and Params.args.seqMask == "none"
    ns = Params.parse_args(["--seqAtt", "full", "--seqMask", "causal", "--seqTargets", "all"])
    assert ns.seqAtt == "causal" and ns.seqTargets == "all"
    assert Params.parse_args(["--seqAtt", "full"]).seqAtt == "full" and Params.parse_args(["--seqMask", "none"]).seqAtt == "sum"
    assert Params.parse_args([], namespace=ns).seqAtt == "causal"                  # a second pass over the same namespace
    for bad in (["--seqMask", "causal"], ["--seqAtt", "sum", "--seqMask", "causal"], ["--seqTargets", "every"],
                ["--seqMask", "triangle"]):
        with pytest.raises(SystemExit):
            Params.parse_args(bad)
    text = " ".join(p.format_help().lower().split())
    assert "--seqtargets {last,all}" in text and "--seqmask {none,causal}" in text and "--seqatt {sum,full}" in text
    assert "contributes nothing" in text and "not in the reference" in text


@pytest.mark.parametrize("over,missing", [(dict(seqAtt="full"), "--seqAtt causal"), (dict(seqAtt="sum"), "--seqAtt causal"),
                                          (dict(predLoss="hinge"), "--predLoss softmax"),
                                          (dict(seqPool="additive"), "--seqPool sum")])
def test_prepare_model_refuses_all_without_the_flags_it_needs(monkeypatch, over, missing):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    for k, v in dict(dict(seqTargets="all", seqAtt="causal", predLoss="softmax", seqPool="sum", softmaxNegs=0, user=10, item=10),
                     **over).items():
        monkeypatch.setattr(args, k, v, raising=False)
    with pytest.raises(ValueError, match="--seqTargets all needs " + missing):
        Recommender("cpu", None).prepareModel()              # refused before the handler or the device is touched


def test_prepare_model_refuses_an_unknown_target_mode_and_causal_on_an_unsupported_shape(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    monkeypatch.setattr(args, "seqTargets", "every")
    with pytest.raises(ValueError, match="seqTargets"):
        Recommender("cpu", None).prepareModel()
    monkeypatch.setattr(args, "seqTargets", "last")
    monkeypatch.setattr(args, "seqAtt", "causal")
    for k, v in dict(latdim=64, num_attention_heads=4, pos_length=200).items():
        monkeypatch.setattr(args, k, v)
    with pytest.raises(ValueError, match="seqAtt causal is not available"):
        Recommender("cpu", None).prepareModel()


# ---- argument checks of the new entries ----------------------------------------------------------------------------
def _attn(lib, p, **o):
    a = dict(qkv=p, segl=p, ns=4, P=20, d=64, heads=16, causal=1, ctx=p)
    a.update(o)
    return lib.sagnn_seq_attn_masked_f32(*a.values(), None)


def _attn_bwd(lib, p, **o):
    a = dict(qkv=p, g=p, segl=p, ns=4, P=20, d=64, heads=16, causal=1, dqkv=p)
    a.update(o)
    return lib.sagnn_seq_attn_masked_bwd_f32(*a.values(), None)


def _prefix(lib, p, **o):
    a = dict(x=p, ldx=64, segl=p, U=p, ldu=64, ns=4, P=20, d=64, leaky=0.5, Q=p, ldq=64)
    a.update(o)
    return lib.sagnn_seq_prefix_query_f32(*a.values(), None)


def _prefix_bwd(lib, p, **o):
    a = dict(x=p, ldx=64, segl=p, dQ=p, lddq=64, ns=4, P=20, d=64, leaky=0.5, dx=p, lddx=64, dU=p, lddu=64)
    a.update(o)
    return lib.sagnn_seq_prefix_query_bwd_f32(*a.values(), None)


def _targets(lib, p, **o):
    a = dict(seq=p, nflat=10, segb=p, segl=p, su=p, st=p, ns=4, P=20, ni=50, tgt=p, row=p)
    a.update(o)
    return lib.sagnn_seq_targets_i32(*a.values(), None)


def _scatter(lib, p, **o):
    a = dict(dT=p, lddt=64, tgt=p, n=4, ni=50, d=64, dI=p, lddi=64)
    a.update(o)
    return lib.sagnn_softmax_target_scatter_f32(*a.values(), None)


ENTRIES = {
    "attn": (_attn, ("qkv", "segl", "ctx"), ("qkv", "ctx"), ()),
    "attn_bwd": (_attn_bwd, ("qkv", "g", "segl", "dqkv"), ("qkv", "g", "dqkv"), ()),
    "prefix": (_prefix, ("x", "segl", "U", "Q"), ("x", "U", "Q"), ("ldx", "ldu", "ldq")),
    "prefix_bwd": (_prefix_bwd, ("x", "segl", "dQ", "dx", "dU"), ("x", "dQ", "dx", "dU"), ("ldx", "lddq", "lddx", "lddu")),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_slab_entry_rejects_invalid_arguments_without_a_device(name):
    fn, ptrs, feats, lds = ENTRIES[name]
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 66)]
    cases += [(dict(P=257), -2, "pos_length = 257"), (dict(P=0), -2, "pos_length = 0"), (dict(ns=-1), -5, "negative count")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in feats]
    cases += [(dict(**{k: 66}), -3, "16-byte aligned") for k in lds] + [(dict(**{k: 60}), -5, "< d = 64") for k in lds]
    if name.startswith("attn"):
        cases += [(dict(heads=4), -2, "d / heads = 16"), (dict(heads=7), -2, "does not divide"),
                  (dict(causal=2), -5, "causal = 2"), (dict(causal=-1), -5, "causal = -1")]
    else:
        cases += [(dict(d=260), -2, "d = 260")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
    assert fn(lib, p, ns=0) == 0                                    # nothing to do: returns before any launch
    if name.startswith("attn"):
        assert fn(lib, p, ns=0, causal=0) == 0


def test_targets_and_scatter_reject_invalid_arguments_without_a_device():
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    for k in ("seq", "segb", "segl", "su", "st", "tgt", "row"):
        assert _targets(lib, p, **{k: None}) == -1 and "null pointer" in _lib.last_error().lower(), k
    for over, code, text in ((dict(P=0), -2, "pos_length = 0"), (dict(P=257), -2, "pos_length = 257"), (dict(ns=-1), -5, "negative count"),
                             (dict(nflat=-1), -5, "negative count"), (dict(ni=0), -5, "n_items = 0"), (dict(ni=2 ** 31), -5, "2^31")):
        assert _targets(lib, p, **over) == code and text in _lib.last_error().lower(), (over, _lib.last_error())
    assert _targets(lib, p, ns=0) == 0
    for k in ("dT", "tgt", "dI"):
        assert _scatter(lib, p, **{k: None}) == -1, k
    for over, code, text in ((dict(d=48), -2, "d = 48"), (dict(n=-1), -5, "n_rows = -1"), (dict(ni=0), -5, "n_items = 0"),
                             (dict(lddt=66), -3, "multiples of 4"), (dict(lddi=60), -5, ">= d"), (dict(dT=p + 4), -3, "16-byte aligned")):
        assert _scatter(lib, p, **over) == code and text in _lib.last_error().lower(), (over, _lib.last_error())
    assert _scatter(lib, p, n=0) == 0
