"""CPU suite of the opt-in self-attention over the item sequence (--seqAtt full): the two float64
restatements of seq_att_ref agree, they reduce to the oracle's collapsed head where every slot holds at most one
token, the flag, sagnn_seq_attn_supported's table and the argument checks of every new entry (each rejected before
any device work, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
import torch

import seq_att_ref as R
from oracle import selfgnn_oracle as O
from sa_gnn_amd import _lib


def _head_case(seed, B, P, d, I, layers, lens):
    rng = np.random.default_rng(seed)
    fi = rng.standard_normal((I, d))
    pe = rng.standard_normal((P, d))
    ln = [(1.0 + 0.1 * rng.standard_normal(d), 0.1 * rng.standard_normal(d)) for _ in range(2 + layers)]
    att = []
    for _ in range(layers):
        p = O.init_fusion_params(d, rng, np.float64)
        att.append({k: p[k] for k in ("Wq", "bq", "Wk", "bk", "Wv", "bv")})
    sequence = rng.integers(0, I, size=(B, P))
    mask = np.zeros((B, P), np.float32)
    for b, n in enumerate(lens):                       # a general mask: n positions anywhere in the row
        mask[b, rng.choice(P, size=n, replace=False)] = 1
    return fi, pe, ln, att, sequence, mask


def _as_t(ln, att):
    t = torch.from_numpy
    return [(t(g), t(b)) for g, b in ln], [{k: t(v) for k, v in w.items()} for w in att]


@pytest.mark.parametrize("seed,heads", [(0, 16), (1, 8), (2, 4)])
def test_ragged_and_dense_restatements_agree(seed, heads):
    B, P, d = 9, 12, 32
    lens = [0, 1, 2, 5, 12, 7, 3, 11, 1]
    fi, pe, ln, att, sequence, mask = _head_case(seed, B, P, d, 40, 2, lens)
    a = R.head_ragged_np(fi, pe, ln, att, sequence, mask, heads, 0.5)
    ln_t, att_t = _as_t(ln, att)
    b = R.torch_head_ragged(torch.from_numpy(fi), torch.from_numpy(pe), ln_t, att_t, sequence, mask, heads, 0.5).numpy()
    c = R.torch_head_dense(torch.from_numpy(fi), torch.from_numpy(pe), ln_t, att_t, sequence, mask, heads, 0.5).numpy()
    scale = np.abs(a).max()
    assert np.abs(a - c).max() <= 1e-12 * scale and np.abs(b - c).max() <= 1e-12 * scale
    assert not a[0].any() and not c[0].any()                          # the empty slot pools to a zero row


def test_ragged_and_dense_gradients_agree():
    B, P, d, heads = 5, 8, 32, 16
    fi, pe, ln, att, sequence, mask = _head_case(3, B, P, d, 20, 2, [0, 1, 3, 8, 5])
    grads = []
    for head in (R.torch_head_ragged, R.torch_head_dense):
        ln_t, att_t = _as_t(ln, att)
        leaves = [torch.from_numpy(fi).requires_grad_(True), torch.from_numpy(pe).requires_grad_(True)]
        leaves += [v.requires_grad_(True) for gb in ln_t for v in gb] + [v.requires_grad_(True) for w in att_t for v in w.values()]
        out = head(leaves[0], leaves[1], ln_t, att_t, sequence, mask, heads, 0.5)
        (out * torch.from_numpy(np.random.default_rng(4).standard_normal(out.shape))).sum().backward()
        grads.append([v.grad.numpy() for v in leaves])
    for ga, gb in zip(*grads):
        assert np.abs(ga - gb).max() <= 1e-11 * max(np.abs(gb).max(), 1.0)


def test_full_equals_the_collapsed_head_where_slots_hold_at_most_one_token():
    """Every slot holds at most one token. A slot with exactly one is the same function in both modes (the masked sum
    of one token is that token), pair by pair. A slot with none is not: the contract pools it to a zero row, so its
    pairs score <fu, fi> alone, while the collapsed head layer-norms its all-zero sums to beta and runs the layers on
    that. Both halves are asserted; none of the pairs is left out."""
    B, P, d, heads, I, U = 6, 10, 32, 16, 30, 12
    lens = np.array([0, 1, 1, 0, 1, 1])
    fi, pe, ln, att, sequence, mask = _head_case(5, B, P, d, I, 2, lens)
    rng = np.random.default_rng(6)
    fu = rng.standard_normal((U, d))
    uids, iids, locs = rng.integers(0, U, 40), rng.integers(0, I, 40), rng.integers(0, B, 40)
    want = O.prediction_head(fu, fi, pe, ln, att, uids, iids, sequence, mask, locs, heads, 0.5)
    got = R.prediction_head_full(fu, fi, pe, ln, att, uids, iids, sequence, mask, locs, heads, 0.5)
    one = lens[locs] == 1
    assert one.any() and (~one).any()
    np.testing.assert_allclose(got[one], want[one], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got[~one], (fu[uids] * fi[iids]).sum(-1)[~one], rtol=1e-12, atol=1e-12)


def test_slab_attention_restatements_agree():
    rng = np.random.default_rng(7)
    P, d, heads, lens = 6, 16, 4, [0, 1, 6, 3]
    qkv = rng.standard_normal((len(lens) * P, 3 * d))
    ctx, terms = R.seq_attn_np(qkv, lens, P, heads)
    got = R.seq_attn_t(torch.from_numpy(qkv), lens, P, heads).numpy()
    np.testing.assert_allclose(got, ctx, rtol=1e-13, atol=1e-13)
    assert (terms >= np.abs(ctx) - 1e-12).all() and not ctx[:P].any() and not ctx[P + 1:2 * P].any()


def test_flag_parses_and_defaults_to_sum():
    from sa_gnn_amd import Params
    assert Params.build_parser().parse_args([]).seqAtt == "sum" and Params.args.seqAtt == "sum"
    assert Params.build_parser().parse_args(["--seqAtt", "full"]).seqAtt == "full"
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--seqAtt", "causal"])
    assert "--seqatt {sum,full}" in " ".join(Params.build_parser().format_help().lower().split())


def test_prepare_model_refuses_full_on_an_unsupported_configuration(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    monkeypatch.setattr(args, "seqAtt", "full")
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    for over in (dict(latdim=64, num_attention_heads=4, pos_length=200), dict(latdim=64, num_attention_heads=16, pos_length=257)):
        for k, v in over.items():
            monkeypatch.setattr(args, k, v)
        with pytest.raises(ValueError, match="seqAtt full"):
            Recommender("cpu", None).prepareModel()              # refused before the handler or the device is touched
    monkeypatch.setattr(args, "seqAtt", "causal")
    with pytest.raises(ValueError, match="seqAtt"):
        Recommender("cpu", None).prepareModel()


def test_supported_table():
    lib = _lib.load()
    for d in range(0, 80):
        for heads in (0, 1, 2, 3, 4, 8, 16, 32):
            for P in (0, 1, 8, 200, 256, 257):
                want = d > 0 and d % 4 == 0 and heads > 0 and d % heads == 0 and d // heads in (2, 4, 8) and 1 <= P <= 256
                assert lib.sagnn_seq_attn_supported(d, heads, P) == (0 if want else -2), (d, heads, P)
    assert lib.sagnn_seq_attn_supported(64, 16, 200) == 0                 # the defaults
    assert lib.sagnn_seq_attn_supported(128, 16, 200) == 0 and lib.sagnn_seq_attn_supported(256, 16, 200) == -2


# ---- argument checks: name -> (call builder, pointer arguments, feature pointers, strides) ------------------------
def _gather(lib, p, **o):
    a = dict(fi=p, ldf=64, ni=50, pe=p, ldp=64, P=20, seq=p, nflat=10, pos=p, segb=p, segl=p, ns=4, d=64, ss=p, ps=p, ldo=64)
    a.update(o)
    return lib.sagnn_seq_gather_f32(*a.values(), None)


def _gather_bwd(lib, p, **o):
    a = dict(gs=p, gp=p, ldg=64, seq=p, nflat=10, pos=p, segb=p, segl=p, ns=4, P=20, d=64, dfi=p, lddfi=64, ni=50, dpos=p,
             lddpos=64)
    a.update(o)
    return lib.sagnn_seq_gather_bwd_f32(*a.values(), None)


def _attn(lib, p, **o):
    a = dict(qkv=p, segl=p, ns=4, P=20, d=64, heads=16, ctx=p)
    a.update(o)
    return lib.sagnn_seq_attn_f32(*a.values(), None)


def _attn_bwd(lib, p, **o):
    a = dict(qkv=p, g=p, segl=p, ns=4, P=20, d=64, heads=16, dqkv=p)
    a.update(o)
    return lib.sagnn_seq_attn_bwd_f32(*a.values(), None)


def _pool(lib, p, **o):
    a = dict(x=p, ldx=64, segl=p, ns=4, P=20, d=64, out=p, ldo=64)
    a.update(o)
    return lib.sagnn_seq_pool_f32(*a.values(), None)


def _pool_bwd(lib, p, **o):
    a = dict(g=p, ldg=64, segl=p, ns=4, P=20, d=64, dx=p, ldx=64)
    a.update(o)
    return lib.sagnn_seq_pool_bwd_f32(*a.values(), None)


ENTRIES = {
    "gather": (_gather, ("fi", "pe", "seq", "segb", "segl", "ss", "ps"), ("fi", "pe", "ss", "ps"), ("ldf", "ldp", "ldo")),
    "gather_bwd": (_gather_bwd, ("gs", "gp", "seq", "segb", "segl", "dfi", "dpos"), ("gs", "gp", "dfi", "dpos"),
                   ("ldg", "lddfi", "lddpos")),
    "attn": (_attn, ("qkv", "segl", "ctx"), ("qkv", "ctx"), ()),
    "attn_bwd": (_attn_bwd, ("qkv", "g", "segl", "dqkv"), ("qkv", "g", "dqkv"), ()),
    "pool": (_pool, ("x", "segl", "out"), ("x", "out"), ("ldx", "ldo")),
    "pool_bwd": (_pool_bwd, ("g", "segl", "dx"), ("g", "dx"), ("ldg", "ldx")),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_entry_rejects_invalid_arguments_without_a_device(name):
    fn, ptrs, feats, lds = ENTRIES[name]
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 66)]
    cases += [(dict(P=257), -2, "pos_length = 257"), (dict(P=0), -2, "pos_length = 0"), (dict(ns=-1), -5, "negative count")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in feats]                # a misaligned slab
    cases += [(dict(**{k: 66}), -3, "16-byte aligned") for k in lds] + [(dict(**{k: 60}), -5, "< d = 64") for k in lds]
    if name.startswith("attn"):
        cases += [(dict(heads=4), -2, "d / heads = 16"), (dict(heads=0), -2, "heads = 0"), (dict(heads=7), -2, "does not divide"),
                  (dict(d=36, heads=16), -2, "does not divide")]
    if name.startswith("gather"):
        cases += [(dict(ni=0), -5, "n_items = 0"), (dict(nflat=-1), -5, "negative count")]
        if name == "gather":
            assert fn(lib, p, pos=None, ns=0) == 0                 # NULL positions are the right-aligned form, not an error
    if not name.startswith("attn"):
        cases += [(dict(d=260), -2, "d = 260")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
    if name != "gather_bwd":                                        # (it still writes d_pos for no slots)
        assert fn(lib, p, ns=0) == 0                                # nothing to do: returns before any launch
