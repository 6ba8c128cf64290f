"""CPU suite: the argument checks of the training-side operators (csrc/train_ops.hip: sagnn_pair_score_bwd_f32,
sagnn_prod_leaky_sum_f32 / _bwd, sagnn_meta_features_f32 / _bwd, sagnn_leaky_f32, sagnn_rowdot_sigmoid_f32 / _bwd,
sagnn_hinge_f32) and the feature widths the fusion trains at (sagnn_attn_bwd_f32, sagnn_layernorm_td_bwd_f32,
autograd.interval_fusion). Every library call here is rejected, or returns at a count of 0, before any device work,
so no GPU is needed."""
import ctypes

import pytest

from sa_gnn_amd import _lib

NULL, DIM, ALIGN, ARG = -1, -2, -3, -5
BIG = 1 << 40          # a count no single launch holds, at any d


def _pair_bwd(lib, p, **over):
    a = dict(U=p, ldu=64, I=p, ldi=64, S=p, lds=64, A=p, lda=64, uids=p, iids=p, locs=p, leaky=0.5, g=p, dU=p, dI=p, dS=p,
             dA=p, n=100, d=64)
    a.update(over)
    return lib.sagnn_pair_score_bwd_f32(*a.values(), None)


def _pls(lib, p, **over):
    a = dict(X=p, ldx=64, Y=p, ldy=64, uids=p, iids=p, leaky=0.5, out=p, n=100, d=64)
    a.update(over)
    return lib.sagnn_prod_leaky_sum_f32(*a.values(), None)


def _pls_bwd(lib, p, **over):
    a = dict(X=p, ldx=64, Y=p, ldy=64, uids=p, iids=p, leaky=0.5, g=p, dX=p, dY=p, n=100, d=64)
    a.update(over)
    return lib.sagnn_prod_leaky_sum_bwd_f32(*a.values(), None)


def _meta(lib, p, **over):
    a = dict(F=p, ldf=64, V=p, ldv=64, uids=p, out=p, n=100, d=64)
    a.update(over)
    return lib.sagnn_meta_features_f32(*a.values(), None)


def _meta_bwd(lib, p, **over):
    a = dict(F=p, ldf=64, V=p, ldv=64, uids=p, dm=p, dF=p, dV=p, n=100, d=64)
    a.update(over)
    return lib.sagnn_meta_features_bwd_f32(*a.values(), None)


def _leaky(lib, p, **over):
    a = dict(a=p, g=p, out=p, leaky=0.5, n=100, backward=1)
    a.update(over)
    return lib.sagnn_leaky_f32(*a.values(), None)


def _rowdot(lib, p, **over):
    a = dict(A=p, lda=64, w3=p, b3=p, out=p, n=100, k=48)
    a.update(over)
    return lib.sagnn_rowdot_sigmoid_f32(*a.values(), None)


def _rowdot_bwd(lib, p, **over):
    a = dict(A=p, lda=64, w3=p, w=p, dw=p, dA=p, ldda=64, dw3=p, db3=p, n=100, k=48)
    a.update(over)
    return lib.sagnn_rowdot_sigmoid_bwd_f32(*a.values(), None)


def _hinge(lib, p, **over):
    a = dict(pos=p, neg=p, wp=p, wn=p, sp=p, sn=p, scale=0.5, loss=p, dpos=p, dneg=p, dwp=p, dwn=p, n=100)
    a.update(over)
    return lib.sagnn_hinge_f32(*a.values(), None)


def _check(fn, lib, p, cases):
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (over, _lib.last_error())
        assert text in _lib.last_error().lower(), (over, _lib.last_error())


@pytest.fixture(scope="module")
def buf():
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    return b, p + (-p % 16)


PAIR_BAD_D = (0, 2, 12, 24, 66, 96, 260, 512)      # not 4 * a power of two, or beyond 256
ROW_BAD_D = (0, 2, 66, 260)                        # not a multiple of 4 in [4, 256]


def _rows(lds, feats, p):
    """The stride / alignment cases of every float4-addressed operand: (stride names, pointer names)."""
    cases = [(dict(**{k: 66}), ALIGN, "16-byte aligned") for k in lds]
    cases += [(dict(**{k: 60}), ARG, "< d = 64") for k in lds]
    cases += [(dict(**{k: p + 4}), ALIGN, "16-byte aligned") for k in feats]
    return cases


def test_pair_score_bwd_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), NULL, "null pointer") for k in ("U", "I", "uids", "iids", "g", "dU", "dI")]
    # S, A, locs, dS and dA are one optional group: any one missing, or any one given alone, is refused
    cases += [(dict(**{k: None}), NULL, "go together") for k in ("S", "A", "locs", "dS", "dA")]
    none = dict(S=None, A=None, locs=None, dS=None, dA=None)
    cases += [(dict(none, **{k: p}), NULL, "go together") for k in none]
    cases += [(dict(d=d), DIM, f"d = {d}") for d in PAIR_BAD_D]
    cases += [(dict(n=-1), ARG, "negative count")]
    cases += _rows(("ldu", "ldi", "lds", "lda"), ("U", "I", "S", "A"), p)
    cases += [(dict(n=BIG, d=d, ldu=256, ldi=256, lds=256, lda=256), ARG, "grid too large") for d in (4, 64, 256)]
    _check(_pair_bwd, lib, p, cases)
    # without the head term its strides are not read
    assert _pair_bwd(lib, p, n=0, lds=1, lda=1, **none) == 0
    assert _pair_bwd(lib, p, n=0) == 0


@pytest.mark.parametrize("fn,ptrs", [(_pls, ("X", "Y", "uids", "iids", "out")),
                                     (_pls_bwd, ("X", "Y", "uids", "iids", "g", "dX", "dY"))])
def test_prod_leaky_sum_entries_reject_every_invalid_argument(buf, fn, ptrs):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), NULL, "null pointer") for k in ptrs]
    cases += [(dict(d=d), DIM, f"d = {d}") for d in PAIR_BAD_D]
    cases += [(dict(n=-1), ARG, "negative count")]
    cases += _rows(("ldx", "ldy"), ("X", "Y"), p)
    cases += [(dict(n=BIG, d=d, ldx=256, ldy=256), ARG, "grid too large") for d in (4, 64, 256)]
    _check(fn, lib, p, cases)
    assert fn(lib, p, n=0) == 0


@pytest.mark.parametrize("fn,ptrs,dense", [(_meta, ("F", "V", "uids", "out"), "out"),
                                           (_meta_bwd, ("F", "V", "uids", "dm", "dF", "dV"), "dm")])
def test_meta_features_entries_reject_every_invalid_argument(buf, fn, ptrs, dense):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), NULL, "null pointer") for k in ptrs]
    cases += [(dict(d=d), DIM, f"d = {d}") for d in ROW_BAD_D]
    cases += [(dict(n=-1), ARG, "negative count")]
    cases += _rows(("ldf", "ldv"), ("F", "V", dense), p)
    cases += [(dict(n=BIG, d=d, ldf=256, ldv=256), ARG, "grid too large") for d in (4, 64, 256)]
    _check(fn, lib, p, cases)
    for d in (4, 48, 256):                         # any multiple of 4 up to 256, not only the pair kernels' widths
        assert fn(lib, p, n=0, d=d, ldf=d, ldv=d) == 0


def test_leaky_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    _check(_leaky, lib, p, [
        (dict(a=None), NULL, "null pointer"), (dict(out=None), NULL, "null pointer"), (dict(g=None), NULL, "null pointer"),
        (dict(n=-1), ARG, "negative count"), (dict(n=1 << 40), ARG, "grid too large"),
    ])
    assert _leaky(lib, p, n=0) == 0
    assert _leaky(lib, p, n=0, g=None, backward=0) == 0          # the forward mode reads no g


@pytest.mark.parametrize("fn,ptrs,lds", [(_rowdot, ("A", "w3", "b3", "out"), ("lda",)),
                                         (_rowdot_bwd, ("A", "w3", "w", "dw", "dA", "dw3", "db3"), ("lda", "ldda"))])
def test_rowdot_sigmoid_entries_reject_every_invalid_argument(buf, fn, ptrs, lds):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), NULL, "null pointer") for k in ptrs]
    cases += [(dict(k=k), ARG, f"k = {k}") for k in (0, -1, 8193)]
    cases += [(dict(**{k: 47}), ARG, f"{k} = 47 < k = 48") for k in lds]
    cases += [(dict(**{k: 0}), ARG, "< k = 48") for k in lds]
    cases += [(dict(n=-1), ARG, "negative count"), (dict(n=1 << 40), ARG, "grid too large")]
    _check(fn, lib, p, cases)
    assert fn(lib, p, n=0) == 0
    assert fn(lib, p, n=0, k=1, **{k: 1 for k in lds}) == 0      # a stride of exactly k is legal, and needs no alignment


def test_hinge_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    plain = dict(wp=None, wn=None, sp=None, sn=None, dwp=None, dwn=None)
    cases = [(dict(**{k: None}), NULL, "null pointer") for k in ("pos", "neg", "loss")]
    cases += [(dict(**{k: None}), NULL, "wp, wn, sp and sn go together") for k in ("wp", "wn", "sp", "sn")]
    cases += [(dict(plain, **{k: p}), NULL, "wp, wn, sp and sn go together") for k in ("wp", "wn", "sp", "sn")]
    # the gradient outputs are written in pairs: one of a pair alone is refused, in both forms
    cases += [(dict(dpos=None), NULL, "dpos and dneg go together"), (dict(dneg=None), NULL, "dpos and dneg go together"),
              (dict(dwp=None), NULL, "dwp and dwn go together"), (dict(dwn=None), NULL, "dwp and dwn go together"),
              (dict(plain, dpos=None), NULL, "dpos and dneg go together"),
              (dict(plain, dneg=None), NULL, "dpos and dneg go together"),
              (dict(plain, dwp=p), NULL, "dwp and dwn go together"),
              (dict(plain, dwp=p, dwn=p), ARG, "without wp")]
    cases += [(dict(n=-1), ARG, "negative count"), (dict(n=1 << 40), ARG, "grid too large")]
    _check(_hinge, lib, p, cases)
    # every legal combination of absent outputs
    for over in (dict(), dict(dpos=None, dneg=None), dict(dwp=None, dwn=None), dict(dpos=None, dneg=None, dwp=None, dwn=None),
                 plain, dict(plain, dpos=None, dneg=None)):
        assert _hinge(lib, p, n=0, **over) == 0, over


# ---- which feature widths train ---------------------------------------------------------------------------------------
# The generic backward of the interval fusion needs d to be a multiple of 32 (the dense products) AND 64 % d == 0 or
# d % 64 == 0 (sagnn_attn_bwd_f32 / sagnn_layernorm_td_bwd_f32: a lane's elements fall in a fixed set of columns):
# d in {32, 64, 128, 192, 256}. n = 0 returns before any device work.
TRAINS = (32, 64, 128, 192, 256)


@pytest.mark.parametrize("d", range(32, 257, 32))
def test_which_d_the_generic_backward_accepts(buf, d):
    lib, p = _lib.load(), buf[1]
    rc_attn = lib.sagnn_attn_bwd_f32(p, p, d, 0, 3, d, d // 2, None)     # d_k = 2: a power of two at every d
    err_attn = _lib.last_error()
    rc_ln = lib.sagnn_layernorm_td_bwd_f32(p, 3 * d, p, 3 * d, 0, 3, d, p, 1e-12, p, 3 * d, p, p, None)
    err_ln = _lib.last_error()
    if d in TRAINS:
        assert (rc_attn, rc_ln) == (0, 0), (err_attn, err_ln)
    else:
        assert d in (96, 160, 224)
        assert (rc_attn, rc_ln) == (DIM, DIM)
        for err in (err_attn, err_ln):
            assert f"d = {d}: need 64 % d == 0 or d % 64 == 0" in err, err


@pytest.mark.parametrize("d", (96, 160, 224, 16, 48, 288))
def test_interval_fusion_refuses_a_d_it_cannot_train_before_the_forward(d):
    """autograd.interval_fusion / interval_fusion_rows raise on the width alone: the tensors here live on the CPU, so
    reaching any library call would fail differently (a TypeError from the tensor checks)."""
    import torch

    from sa_gnn_amd import autograd as ag
    assert ag.TRAINABLE_D == TRAINS
    x = torch.zeros((2, 3, d), requires_grad=True)
    with pytest.raises(ValueError, match=rf"d = {d}: the interval fusion trains at d in \(32, 64, 128, 192, 256\)"):
        ag.interval_fusion(x, {}, 16)
    with pytest.raises(ValueError, match=rf"d = {d}: the interval fusion trains at d in \(32, 64, 128, 192, 256\)"):
        ag.interval_fusion_rows(x, torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 2, {}, 16)


@pytest.mark.parametrize("d", TRAINS)
def test_interval_fusion_accepts_every_d_that_trains(d):
    """The width check lets these through: what stops the call is the next check (the parameters)."""
    import torch

    from sa_gnn_amd import autograd as ag
    with pytest.raises(KeyError):
        ag.interval_fusion(torch.zeros((2, 3, d)), {}, 16)
