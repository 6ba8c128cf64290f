"""CPU suite of --seqHeads: the flag parses, prepareModel refuses what the issue names and lets the
supported head counts through, the wide entries' `supported` table and argument checks hold without a device, the narrow
entries keep their own table, and the float64 restatements agree with each other at 1, 2 and 4 heads."""
import ctypes

import numpy as np
import pytest
import torch

import seq_att_ref as A
import seq_causal_ref as R
from sa_gnn_amd import _lib
from sa_gnn_amd.model import Recommender, seq_heads


def test_flag_parses_and_defaults_to_zero():
    from sa_gnn_amd import Params
    p = Params.build_parser()
    assert p.parse_args([]).seqHeads == 0 and Params.args.seqHeads == 0
    ns = Params.parse_args(["--seqAtt", "full", "--seqHeads", "2"])
    assert ns.seqHeads == 2 and ns.seqAtt == "full" and ns.num_attention_heads == 16
    assert Params.parse_args(["--seqAtt", "full", "--seqMask", "causal", "--seqHeads", "1"]).seqAtt == "causal"
    with pytest.raises(SystemExit):
        Params.parse_args(["--seqHeads", "two"])
    text = " ".join(p.format_help().lower().split())
    assert "--seqheads" in text and text.count("seqheads") >= 2          # its own entry and --seqAtt's help


def _args(monkeypatch, **over):
    from sa_gnn_amd.Params import args
    base = dict(seqAtt="full", seqHeads=0, latdim=64, num_attention_heads=16, pos_length=200, user=10, item=10)
    for k, v in dict(base, **over).items():
        monkeypatch.setattr(args, k, v, raising=False)
    return args


@pytest.mark.parametrize("over,text", [
    (dict(seqAtt="sum", seqHeads=4), "--seqAtt"),
    (dict(seqHeads=3), "seqHeads 3"),
    (dict(seqHeads=64), "seqHeads 64"),                       # d_k 1
    (dict(latdim=128, seqHeads=1), "seqHeads 1"),             # d_k 128
    (dict(seqHeads=2, pos_length=257), "pos_length = 257"),
    (dict(seqAtt="causal", seqHeads=3), "seqHeads 3"),
    (dict(seqHeads=-1), "seqHeads -1"),
])
def test_prepare_model_refuses(monkeypatch, over, text):
    _args(monkeypatch, **over)
    with pytest.raises(ValueError, match=text):
        Recommender("cpu", None).prepareModel()              # refused before the handler or the device is touched


@pytest.mark.parametrize("mode", ["full", "causal"])
@pytest.mark.parametrize("heads", [4, 2, 1, 16])
def test_prepare_model_lets_the_supported_head_counts_through(monkeypatch, heads, mode):
    """Up to the point the refusal tests reach: with no handler, prepareModel gets past every flag check and fails on
    the first thing it asks of the handler, never with a ValueError."""
    _args(monkeypatch, seqHeads=heads, seqAtt=mode, num_attention_heads=16)
    assert seq_heads() == heads
    with pytest.raises(AttributeError):
        Recommender("cpu", None).prepareModel()


def test_zero_follows_num_attention_heads_and_keeps_the_old_refusal(monkeypatch):
    _args(monkeypatch, seqHeads=0, num_attention_heads=4)
    assert seq_heads() == 4
    with pytest.raises(ValueError, match="seqAtt full is not available"):
        Recommender("cpu", None).prepareModel()
    _args(monkeypatch, seqHeads=0, num_attention_heads=8)
    assert seq_heads() == 8


def _want(d, heads, P):
    return d > 0 and d % 4 == 0 and heads > 0 and d % heads == 0 and d // heads in (16, 32, 64) and 1 <= P <= 256


def test_wide_supported_table():
    from sa_gnn_amd import ops
    lib = _lib.load()
    hits = 0
    for d in range(0, 136):
        for heads in (0, 1, 2, 3, 4, 8, 16, 32):
            for P in (0, 1, 8, 200, 256, 257):
                want = _want(d, heads, P)
                hits += want
                assert lib.sagnn_seq_attn_wide_supported(d, heads, P) == (0 if want else -2), (d, heads, P)
                if not want:
                    assert _lib.last_error()
    assert hits > 0
    assert ops.seq_attn_wide_supported(64, 2, 200) is None and "16, 32 or 64" in ops.seq_attn_wide_supported(64, 16, 200)
    assert "pos_length = 257" in ops.seq_attn_wide_supported(64, 2, 257)


def test_the_narrow_entries_keep_their_table():
    lib = _lib.load()
    for d in range(0, 136):
        for heads in (0, 1, 2, 3, 4, 8, 16, 32):
            for P in (0, 1, 8, 200, 256, 257):
                narrow = d > 0 and d % 4 == 0 and heads > 0 and d % heads == 0 and d // heads in (2, 4, 8) and 1 <= P <= 256
                assert lib.sagnn_seq_attn_supported(d, heads, P) == (0 if narrow else -2), (d, heads, P)
                assert not (narrow and _want(d, heads, P))
    assert lib.sagnn_seq_attn_supported(64, 4, 200) == -2 and "d / heads = 16" in _lib.last_error()


# ---- argument checks of the new entries ----------------------------------------------------------------------------
def _attn(lib, p, **o):
    a = dict(qkv=p, segl=p, ns=4, P=20, d=64, heads=2, causal=1, ctx=p)
    a.update(o)
    return lib.sagnn_seq_attn_wide_f32(*a.values(), None)


def _attn_bwd(lib, p, **o):
    a = dict(qkv=p, g=p, segl=p, ns=4, P=20, d=64, heads=2, causal=1, dqkv=p)
    a.update(o)
    return lib.sagnn_seq_attn_wide_bwd_f32(*a.values(), None)


ENTRIES = {
    "attn": (_attn, ("qkv", "segl", "ctx"), ("qkv", "ctx")),
    "attn_bwd": (_attn_bwd, ("qkv", "g", "segl", "dqkv"), ("qkv", "g", "dqkv")),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_wide_entries_reject_invalid_arguments_without_a_device(name):
    fn, ptrs, feats = ENTRIES[name]
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 66)]
    cases += [(dict(P=257), -2, "pos_length = 257"), (dict(P=0), -2, "pos_length = 0"), (dict(ns=-1), -5, "negative count")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in feats]
    cases += [(dict(heads=0), -2, "heads = 0"), (dict(heads=8), -2, "d / heads = 8"), (dict(d=128, heads=1), -2, "d / heads = 128"),
              (dict(heads=7), -2, "does not divide"), (dict(causal=2), -5, "causal = 2"), (dict(causal=-1), -5, "causal = -1")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
    for heads in (4, 2, 1):
        assert fn(lib, p, ns=0, heads=heads) == 0                    # nothing to do: returns before any launch
    assert fn(lib, p, ns=0, causal=0) == 0


def test_the_dispatch_is_by_head_width(monkeypatch):
    """SeqAttnFn's choice: d // heads <= 8 keeps the calls it made before, with their argument lists; from 16 on the
    wide pair. Checked on the Python side with the ops replaced, so no device is needed."""
    from sa_gnn_amd import autograd as ag, ops
    calls = []
    R_, d, P = 8, 64, 4
    fake = lambda name, cols: (lambda qkv, *a: (calls.append((name,) + tuple(a[-3:] if name.endswith("bwd") else a[1:])),
                                                torch.zeros((R_, cols)))[1])
    monkeypatch.setattr(ops, "layernorm_td", lambda x, g, b: x)
    monkeypatch.setattr(ops, "dense_nn", lambda y, W, b: torch.zeros((R_, 3 * d)))
    monkeypatch.setattr(ops, "leaky_add", lambda a, x, s: a + x)
    for name, cols in (("seq_attn", d), ("seq_attn_wide", d), ("seq_attn_bwd", 3 * d), ("seq_attn_wide_bwd", 3 * d)):
        monkeypatch.setattr(ops, name, fake(name, cols))
    x, v, W = torch.zeros((R_, d)), torch.zeros(d), torch.zeros((d, d))
    seg = torch.tensor([4, 2], dtype=torch.int32)
    for heads, causal in ((16, False), (8, True), (4, False), (1, True)):
        ag.SeqAttnFn.apply(x, v, v, W, v, W, v, W, v, seg, P, heads, 0.5, *((True,) if causal else ()))
    assert calls == [("seq_attn", P, 16), ("seq_attn", P, 8, True), ("seq_attn_wide", P, 4, False), ("seq_attn_wide", P, 1, True)]


# ---- the references themselves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 2, 4])
def test_restatements_agree_at_few_wide_heads(heads):
    rng = np.random.default_rng(heads)
    d, P, lens = 64, 9, [0, 1, 9, 5]
    qkv = rng.standard_normal((len(lens) * P, 3 * d)) * 0.5
    t = torch.from_numpy(qkv)
    full, terms = A.seq_attn_np(qkv, lens, P, heads)
    np.testing.assert_allclose(A.seq_attn_t(t, lens, P, heads).numpy(), full, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(R.seq_attn_dense_t(t, lens, P, heads, causal=False).numpy(), full, rtol=1e-12, atol=1e-13)
    causal, cterms = R.seq_attn_np(qkv, lens, P, heads)
    np.testing.assert_allclose(R.seq_attn_t(t, lens, P, heads).numpy(), causal, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(R.seq_attn_dense_t(t, lens, P, heads).numpy(), causal, rtol=1e-12, atol=1e-13)
    assert (terms >= np.abs(full) - 1e-12).all() and (cterms >= np.abs(causal) - 1e-12).all()
    other, _ = A.seq_attn_np(qkv, lens, P, 16)
    assert np.abs(other - full).max() > 1e-3                            # the head count is part of the function
    g = torch.from_numpy(rng.standard_normal((len(lens) * P, d)))
    grads = []
    for form in (R.seq_attn_t, R.seq_attn_dense_t):
        leaf = torch.from_numpy(qkv).requires_grad_(True)
        (form(leaf, lens, P, heads) * g).sum().backward()
        grads.append(leaf.grad.numpy())
    np.testing.assert_allclose(grads[0], grads[1], rtol=1e-10, atol=1e-12)
