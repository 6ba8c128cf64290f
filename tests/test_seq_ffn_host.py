"""CPU suite of --seqFFN: the flag parses, prepareModel refuses what the issue names before any forward,
the entries' `supported` table, argument checks and workspace query hold without a device, SeqFfnFn's gradients agree
with torch autograd when the ops are replaced by the float64 restatement, the two float64 forms agree with each other,
and checkpoints carry the hidden width."""
import ctypes

import numpy as np
import pytest
import torch

import seq_ffn_ref as F
from sa_gnn_amd import _lib
from sa_gnn_amd.model import Recommender


def test_flag_parses_and_defaults_to_zero():
    from sa_gnn_amd import Params
    p = Params.build_parser()
    assert p.parse_args([]).seqFFN == 0 and Params.args.seqFFN == 0
    ns = Params.parse_args(["--seqAtt", "full", "--seqFFN", "256"])
    assert ns.seqFFN == 256 and ns.seqAtt == "full"
    assert Params.parse_args(["--seqAtt", "full", "--seqMask", "causal", "--seqFFN", "64"]).seqAtt == "causal"
    with pytest.raises(SystemExit):
        Params.parse_args(["--seqFFN", "wide"])
    assert "--seqffn" in " ".join(p.format_help().lower().split())


def _args(monkeypatch, **over):
    from sa_gnn_amd.Params import args
    base = dict(seqAtt="full", seqHeads=0, seqFFN=0, latdim=64, num_attention_heads=16, pos_length=200, user=10, item=10)
    for k, v in dict(base, **over).items():
        monkeypatch.setattr(args, k, v, raising=False)
    return args


@pytest.mark.parametrize("over,text", [
    (dict(seqAtt="sum", seqFFN=64), "needs --seqAtt full"),
    (dict(seqFFN=-16), "seqFFN -16"),
    (dict(seqFFN=40), "f = 40"),
    (dict(seqFFN=8), "f = 8"),
    (dict(seqFFN=272), "f = 272"),
    (dict(latdim=128, num_attention_heads=16, seqFFN=256), "d \\* f"),
    (dict(seqAtt="causal", seqFFN=40), "f = 40"),
    (dict(seqFFN=64, pos_length=257), "pos_length = 257"),
])
def test_prepare_model_refuses(monkeypatch, over, text):
    _args(monkeypatch, **over)
    with pytest.raises(ValueError, match=text):
        Recommender("cpu", None).prepareModel()              # refused before the handler or the device is touched


@pytest.mark.parametrize("mode", ["full", "causal"])
@pytest.mark.parametrize("latdim,heads,ffn", [(64, 16, 256), (64, 16, 16), (32, 16, 128), (128, 16, 128)])
def test_prepare_model_lets_the_supported_widths_through(monkeypatch, latdim, heads, ffn, mode):
    """With no handler, prepareModel gets past every flag check, the library's included, and fails on the first thing it
    asks of the handler: the interval matrices of None."""
    from sa_gnn_amd import ops
    _args(monkeypatch, seqFFN=ffn, seqAtt=mode, latdim=latdim, num_attention_heads=heads)
    asked = []
    real = ops.seq_ffn_supported
    monkeypatch.setattr(ops, "seq_ffn_supported", lambda *a: (asked.append(a), real(*a))[1])
    with pytest.raises(AttributeError, match="'NoneType' object has no attribute 'subMat'"):
        Recommender("cpu", None).prepareModel()
    assert asked == [(latdim, ffn, 200)]


def _want(d, f, P):
    return d in (32, 64, 128) and f % 16 == 0 and 16 <= f <= 256 and d * f <= 16384 and 1 <= P <= 256


def test_supported_table():
    from sa_gnn_amd import ops
    lib = _lib.load()
    hits = 0
    for d in range(0, 136):
        for f in range(0, 273):
            for P in (0, 1, 256, 257):
                want = _want(d, f, P)
                hits += want
                assert lib.sagnn_seq_ffn_supported(d, f, P) == (0 if want else -2), (d, f, P)
    assert hits == 2 * (16 + 16 + 8)
    assert lib.sagnn_seq_ffn_supported(128, 256, 200) == -2 and "d * f" in _lib.last_error()
    assert ops.seq_ffn_supported(64, 256, 200) is None and ops.seq_ffn_supported(128, 128, 256) is None
    assert "f = 40" in ops.seq_ffn_supported(64, 40, 200) and "pos_length = 257" in ops.seq_ffn_supported(64, 64, 257)
    assert "d = 48" in ops.seq_ffn_supported(48, 64, 200)


# ---- argument checks of the entries --------------------------------------------------------------------------------
FIELDS = ("x", "seg_len", "gamma", "beta", "W1", "b1", "W2", "b2")


def _struct(p, **o):
    a = dict(x=p, ldx=64, seg_len=p, n_slots=4, pos_length=20, d=64, f=128, gamma=p, beta=p, ln_eps=1e-12, W1=p, b1=p, W2=p,
             b2=p, leaky=0.5)
    a.update({k: v for k, v in o.items() if k in a})
    return _lib.SeqFfnArgs(**a)


def _fwd(lib, p, **o):
    r = dict(out=p, ld_out=64)
    r.update({k: v for k, v in o.items() if k in r})
    return lib.sagnn_seq_ffn_f32(None if o.get("args_null") else ctypes.byref(_struct(p, **o)), r["out"], r["ld_out"], None)


def _bwd(lib, p, **o):
    r = dict(g=p, ldg=64, dx=p, ld_dx=64, dgamma=p, dbeta=p, dW1=p, db1=p, dW2=p, db2=p, ws=p, ws_bytes=1 << 40)
    r.update({k: v for k, v in o.items() if k in r})
    return lib.sagnn_seq_ffn_bwd_f32(None if o.get("args_null") else ctypes.byref(_struct(p, **o)), *r.values(), None)


ENTRIES = {
    "fwd": (_fwd, ("out",), ("out",), ("ld_out",)),
    "bwd": (_bwd, ("g", "dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2"), ("g", "dx"), ("ldg", "ld_dx")),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_entries_reject_invalid_arguments_without_a_device(name):
    fn, ptrs, rows, strides = ENTRIES[name]
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    cases = [(dict(args_null=True), -1, "null args")]
    cases += [(dict(**{k: None}), -1, "null pointer") for k in FIELDS + ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 16, 48, 96, 256)]
    cases += [(dict(f=f), -2, f"f = {f}") for f in (0, 8, 40, 272)]
    cases += [(dict(d=128, f=256), -2, "d * f"), (dict(pos_length=257), -2, "pos_length = 257"),
              (dict(pos_length=0), -2, "pos_length = 0"), (dict(n_slots=-1), -5, "negative count")]
    cases += [(dict(leaky=v), -5, "leaky") for v in (1.0, -0.1, 2.0, float("nan"))]
    cases += [(dict(ln_eps=v), -5, "ln_eps") for v in (-1e-3, 0.0, 2.0, float("nan"))]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in tuple(k for k in FIELDS if k != "seg_len") + rows]
    cases += [(dict(**{k: v}), -3, "multiple of 4") for k in ("ldx",) + strides for v in (63, 66, 32)]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
    if name == "fwd":
        assert fn(lib, p, n_slots=0) == 0                            # nothing to do: returns before any launch
    else:
        for over in (dict(ws=None), dict(ws_bytes=0), dict(ws=p + 4),
                     dict(ws_bytes=lib.sagnn_seq_ffn_bwd_workspace_bytes(4, 20, 64, 128) - 1)):
            assert fn(lib, p, **over) == -6 and "workspace" in _lib.last_error(), over


def test_workspace_query():
    lib = _lib.load()
    q = lib.sagnn_seq_ffn_bwd_workspace_bytes
    for n, P, d, f in ((0, 8, 32, 32), (1, 1, 32, 16), (11, 72, 64, 256), (512, 200, 64, 256), (16400, 256, 64, 256)):
        need = q(n, P, d, f)
        assert need % 16 == 0 and need >= 4 * (n * P * 2 * f + 2 * d * f + f + 3 * d), (n, P, d, f)     # the slab and one partial
        assert need <= 4 * (n * P * 2 * f + 256 * (2 * d * f + f + d) + 4096 * 2 * d)
    assert q(16400, 256, 64, 256) > 4 * 2 ** 31                                  # 64-bit: the far-offset case
    assert q(4, 20, 128, 256) == 0 and q(4, 300, 64, 64) == 0 and q(-1, 20, 64, 64) == 0
    assert q(8, 72, 64, 64) == q(8, 72, 64, 64)                                  # a function of the shape only


# ---- the autograd function with the ops replaced by the float64 restatement ----------------------------------------
def _params(rng, d, f):
    lim = np.sqrt(6.0 / (d + f))
    return {"gamma": 1 + 0.1 * rng.standard_normal(d), "beta": 0.1 * rng.standard_normal(d),
            "W1": rng.uniform(-lim, lim, (d, f)), "b1": 0.1 * rng.standard_normal(f),
            "W2": rng.uniform(-lim, lim, (f, d)), "b2": 0.1 * rng.standard_normal(d)}


def test_autograd_function_against_torch_autograd(monkeypatch):
    from sa_gnn_amd import autograd as ag, ops
    rng = np.random.default_rng(5)
    d, f, P, lens, leaky = 32, 48, 5, [0, 5, 1, 3], 0.5
    p = {k: torch.from_numpy(v) for k, v in _params(rng, d, f).items()}
    x = torch.from_numpy(rng.standard_normal((len(lens) * P, d)))
    g = torch.from_numpy(rng.standard_normal((len(lens) * P, d)))
    pad = np.concatenate([np.arange(b * P + n, (b + 1) * P) for b, n in enumerate(lens)])
    g[pad] = 0.0                                                       # the contract of the incoming gradient
    calls = []

    def fwd(x, gamma, beta, W1, b1, W2, b2, seg_len, P_, leaky_):
        calls.append("seq_ffn")
        assert not any(t.requires_grad for t in (x, gamma, beta, W1, b1, W2, b2))
        return F.seq_ffn_t(x, dict(zip(F.KEYS, (gamma, beta, W1, b1, W2, b2))), seg_len.tolist(), P_, leaky_)

    def bwd(x, g_, gamma, beta, W1, b1, W2, b2, seg_len, P_, leaky_):
        calls.append("seq_ffn_bwd")
        leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, W1, b1, W2, b2)]
        with torch.enable_grad():
            out = F.seq_ffn_t(leaves[0], dict(zip(F.KEYS, leaves[1:])), seg_len.tolist(), P_, leaky_)
            (out * g_).sum().backward()
        return tuple(t.grad for t in leaves)

    monkeypatch.setattr(ops, "seq_ffn", fwd)
    monkeypatch.setattr(ops, "seq_ffn_bwd", bwd)
    seg = torch.tensor(lens, dtype=torch.int32)
    mine = [t.clone().requires_grad_(True) for t in (x, *(p[k] for k in F.KEYS))]
    out = ag.SeqFfnFn.apply(*mine, seg, P, leaky)
    (out * g).sum().backward()
    assert calls == ["seq_ffn", "seq_ffn_bwd"]                        # the backward is one call
    ref = [t.clone().requires_grad_(True) for t in (x, *(p[k] for k in F.KEYS))]
    want = F.seq_ffn_t(ref[0], dict(zip(F.KEYS, ref[1:])), lens, P, leaky)
    (want * g).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), want.detach().numpy(), rtol=1e-13, atol=1e-14)
    assert not out.detach().numpy()[pad].any()
    for a, b, name in zip(mine, ref, ("x",) + F.KEYS):
        assert a.grad is not None and float(b.grad.abs().max()) > 0, name
        np.testing.assert_allclose(a.grad.numpy(), b.grad.numpy(), rtol=1e-12, atol=1e-13, err_msg=name)
    assert not mine[0].grad.numpy()[pad].any()


# ---- the references themselves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaky", [0.5, 0.0])
def test_restatements_agree(leaky):
    rng = np.random.default_rng(11)
    d, f, P, lens = 32, 64, 7, [0, 1, 7, 4]
    p = _params(rng, d, f)
    x = rng.standard_normal((len(lens) * P, d))
    out, terms = F.seq_ffn_np(x, p, lens, P, leaky)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    np.testing.assert_allclose(F.seq_ffn_t(torch.from_numpy(x), pt, lens, P, leaky).numpy(), out, rtol=1e-12, atol=1e-13)
    pad = np.concatenate([np.arange(b * P + n, (b + 1) * P) for b, n in enumerate(lens)])
    assert not out[pad].any() and not terms[pad].any() and (terms >= np.abs(out) - 1e-12).all()
    loud = x.copy()
    loud[pad] = np.nan                                                # the padding is not read
    assert np.array_equal(F.seq_ffn_np(loud, p, lens, P, leaky)[0], out)
    # by hand on one token: the layer norm, both products, the leaky convention and the plain residual
    j = 2 * P + 3
    z = (x[j] - x[j].mean()) / np.sqrt(x[j].var() + 1e-12) * p["gamma"] + p["beta"]
    a = z @ p["W1"] + p["b1"]
    h = np.where(a > 0, a, leaky * a)                                 # leaky in [0, 1): the same function
    np.testing.assert_allclose(out[j], x[j] + h @ p["W2"] + p["b2"], rtol=1e-12, atol=1e-13)
    other, _ = F.seq_ffn_np(x, dict(p, b2=p["b2"] + 1.0), lens, P, leaky)
    real = np.setdiff1d(np.arange(len(x)), pad)
    np.testing.assert_allclose(other[real] - out[real], 1.0, rtol=0, atol=1e-12)


def test_head_with_no_blocks_is_the_ragged_head():
    import seq_att_ref as A
    import seq_causal_ref as C
    from oracle import selfgnn_oracle as O
    rng = np.random.default_rng(2)
    d, B, P, n_items = 32, 3, 6, 9
    fi, pos = torch.from_numpy(rng.standard_normal((n_items, d))), torch.from_numpy(rng.standard_normal((P, d)))
    ln = [(torch.ones(d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64))] * 3
    att = [{k: torch.from_numpy(v) for k, v in O.init_fusion_params(d, rng, np.float64).items() if k[0] in "Wb" and k[1] in "qkv"}]
    seq, mask = rng.integers(0, n_items, (B, P)), (rng.random((B, P)) < 0.6).astype(np.float64)
    mask[1] = 0
    for causal, ref in ((False, A.torch_head_ragged), (True, C.torch_head_causal)):
        want = ref(fi, pos, ln, att, seq, mask, 2, 0.5)
        got = F.torch_head_ffn(None, causal=causal)(fi, pos, ln, att, seq, mask, 2, 0.5)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-13, atol=1e-14)
        p = [{k: torch.from_numpy(v) for k, v in _params(rng, d, 16).items()}]
        with_ffn = F.torch_head_ffn(p, causal=causal)(fi, pos, ln, att, seq, mask, 2, 0.5)
        assert float((with_ffn - want).abs().max()) > 1e-3 and not with_ffn[1].any()
        assert float((F.torch_head_ffn(p, causal=causal, heads=4)(fi, pos, ln, att, seq, mask, 2, 0.5) - with_ffn).abs().max()) > 1e-6


# ---- checkpoints ---------------------------------------------------------------------------------------------------
def test_checkpoint_key(monkeypatch, tmp_path):
    from sa_gnn_amd.Utils import NNLayers as NNs
    args = _args(monkeypatch, seqFFN=64, epoch=1, save_path="ffn_ckpt", load_model="ffn_ckpt", adjNorm="none", seqPool="sum",
                 rnnCell="lstm", edgeTime="none")
    NNs.reset("cpu")
    rec = Recommender("cpu", None)
    rec.metrics = {}
    rec.saveHistory(str(tmp_path))
    path = str(tmp_path / "Models" / "ffn_ckpt")
    state = torch.load(path, weights_only=True)
    assert state["seqFFN"] == 64 and state["seqAtt"] == "full"
    with pytest.raises(FileNotFoundError):                            # past every flag check: the history of another name
        monkeypatch.setattr(args, "load_model", "ffn_ckpt")
        (tmp_path / "History" / "ffn_ckpt.his").unlink()
        rec.loadModel(str(tmp_path))
    for other in (0, 128):
        monkeypatch.setattr(args, "seqFFN", other)
        with pytest.raises(ValueError, match="seqFFN 64"):
            rec.loadModel(str(tmp_path))
    del state["seqFFN"]                                               # a checkpoint from before the flag counts as 0
    torch.save(state, path)
    monkeypatch.setattr(args, "seqFFN", 0)
    with pytest.raises(FileNotFoundError):
        rec.loadModel(str(tmp_path))
    monkeypatch.setattr(args, "seqFFN", 64)
    with pytest.raises(ValueError, match="seqFFN 0"):
        rec.loadModel(str(tmp_path))
    monkeypatch.setattr(args, "seqAtt", "sum")                        # the collapsed head stores no width
    monkeypatch.setattr(args, "seqFFN", 0)
    rec.saveHistory(str(tmp_path))
    assert "seqFFN" not in torch.load(path, weights_only=True)
