"""The wrappers autograd.py calls (ops.lstm_fwd_train ... ops.hinge) against the raw positional call of the same entry on the
same inputs, bit for bit, and their refusals with nothing launched. What the entries compute is held against float64
elsewhere (test_gpu_train_ops.py, test_gpu_backward.py, ...): here only the binding can be wrong — a stride, a count, an
argument out of place, an output that is not zeroed.

Shapes are the smallest at which that can show: d = 32, tables of 7 and 9 rows held in slabs with row stride d + 4 (NaN
in the padding), 0 / 1 / 5 pairs with distinct ids, n = 3 nodes of t = 2 intervals dense and as the permuted view of
[t, n, d] storage, k = 48 row-dot columns inside 64.

Why bit for bit holds although several outputs are accumulated with float atomics: with distinct ids every row of a pair
or meta-feature gradient has the addends of ONE thread, added in program order (dI under the A-is-I aliasing takes two,
both from the pair's own lanes). Every other accumulating entry runs ONE workgroup at these sizes, read off its launch
geometry: the hinge loss and the row-dot's dw3 / db3 (n = 5 <= 256 rows per block), the layer norm's dgamma / dbeta
(16 nodes per block), the BPTT's and the attention tail's dW / db (one chunk of 32 rows; the second-pass weight gradient
likewise). So no output here is compared under a bound instead.

layernorm_td_bwd takes ONE node stride per operand (each node's (t, d) block contiguous), as its entry does: the
permuted view cannot be handed to either call, so that layout is checked to be refused and its contiguous copy compared;
a padded node stride is the layout that exercises the stride instead."""
import pytest
import torch

from sa_gnn_amd import _lib, ops

pytestmark = pytest.mark.gpu

D, PAD = 32, 4
NU, NI, NL = 7, 9, 7
UIDS, IIDS, LOCS = (3, 0, 6, 2, 5), (8, 1, 4, 0, 7), (2, 6, 1, 4, 0)        # distinct within each list
N, T, HEADS = 3, 2, 16
LEAKY = 0.5


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _rand(dev, seed, *shape):
    return torch.randn(shape, generator=_gen(seed)).to(dev)


def _slab(dev, seed, rows, cols=D):
    """[rows, cols] random values as the leading columns of a [rows, cols + PAD] slab, NaN in the padding."""
    full = torch.full((rows, cols + PAD), float("nan"))
    full[:, :cols] = torch.randn((rows, cols), generator=_gen(seed))
    view = full.to(dev)[:, :cols]
    assert view.stride(0) == cols + PAD and view.data_ptr() % 16 == 0
    return view


def _ids(dev, values, n):
    """The first n ids, and the pointer a raw call hands over (a stand-in when n = 0: the entries refuse NULL)."""
    t = torch.tensor(values[:n], dtype=torch.int32, device=dev)
    return t, (t.data_ptr() if n else torch.zeros(4, dtype=torch.int32, device=dev).data_ptr())


def _vals(dev, seed, n):
    t = _rand(dev, seed, n)
    return t, (t.data_ptr() if n else torch.zeros(4, device=dev).data_ptr())


def _raw(name, *args):
    ops.check(getattr(_lib.load(), name)(*args, ops._stream()))


def _same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(want).all()), f"{what}: the raw call's result is not finite"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ from the raw call's"


def _zeros(dev, *shape):
    return torch.zeros(shape, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("form", ("head", "no head", "A is I"))
def test_pair_score_bwd(dev, n, form):
    U, I, S, A = _slab(dev, 1, NU), _slab(dev, 2, NI), _slab(dev, 3, NL), _slab(dev, 4, NI)
    (uids, up), (iids, ip), (locs, lp) = _ids(dev, UIDS, n), _ids(dev, IIDS, n), _ids(dev, LOCS, n)
    g, gp = _vals(dev, 5, n)
    head = form != "no head"
    if form == "A is I":
        A = I
    dU, dI, dS = _zeros(dev, NU, D), _zeros(dev, NI, D), _zeros(dev, NL, D)
    dA = dI if A is I else _zeros(dev, NI, D)
    ld = D + PAD
    _raw("sagnn_pair_score_bwd_f32", U.data_ptr(), ld, I.data_ptr(), ld, S.data_ptr() if head else None, ld if head else 0,
         A.data_ptr() if head else None, ld if head else 0, up, ip, lp if head else None, LEAKY, gp, dU.data_ptr(), dI.data_ptr(),
         dS.data_ptr() if head else None, dA.data_ptr() if head else None, n, D)
    got = ops.pair_score_bwd(U, I, uids, iids, g, **(dict(S=S, A=A, locs=locs) if head else {}), leaky=LEAKY)
    _same(got[0], dU, "dU")
    _same(got[1], dI, "dI")
    if not head:
        assert got[2] is None and got[3] is None
        return
    _same(got[2], dS, "dS")
    if form == "A is I":
        assert got[3] is got[1]
    else:
        _same(got[3], dA, "dA")
    if n == 5:
        assert int((dU != 0).any(1).sum()) == 5 and int((dS != 0).any(1).sum()) == 5      # the case is what it says


@pytest.mark.parametrize("n", (0, 1, 5))
def test_prod_leaky_sum_and_bwd(dev, n):
    X, Y = _slab(dev, 6, NU), _slab(dev, 7, NI)
    (uids, up), (iids, ip) = _ids(dev, UIDS, n), _ids(dev, IIDS, n)
    g, gp = _vals(dev, 8, n)
    ld = D + PAD
    out = torch.full((max(n, 1),), 7.0, device=dev)
    _raw("sagnn_prod_leaky_sum_f32", X.data_ptr(), ld, Y.data_ptr(), ld, up, ip, LEAKY, out.data_ptr(), n, D)
    _same(ops.prod_leaky_sum(X, Y, uids, iids, LEAKY), out[:n], "prod_leaky_sum")
    dX, dY = _zeros(dev, NU, D), _zeros(dev, NI, D)
    _raw("sagnn_prod_leaky_sum_bwd_f32", X.data_ptr(), ld, Y.data_ptr(), ld, up, ip, LEAKY, gp, dX.data_ptr(), dY.data_ptr(), n, D)
    got = ops.prod_leaky_sum_bwd(X, Y, uids, iids, LEAKY, g)
    _same(got[0], dX, "dX")
    _same(got[1], dY, "dY")


@pytest.mark.parametrize("n", (0, 1, 5))
def test_meta_features_and_bwd(dev, n):
    F, V = _slab(dev, 9, NU), _slab(dev, 10, NU)
    uids, up = _ids(dev, UIDS, n)
    dm = _rand(dev, 11, max(n, 1), 3 * D)
    ld = D + PAD
    out = torch.full((max(n, 1), 3 * D), 7.0, device=dev)
    _raw("sagnn_meta_features_f32", F.data_ptr(), ld, V.data_ptr(), ld, up, out.data_ptr(), n, D)
    _same(ops.meta_features(F, V, uids), out[:n], "meta_features")
    dF, dV = _zeros(dev, NU, D), _zeros(dev, NU, D)
    _raw("sagnn_meta_features_bwd_f32", F.data_ptr(), ld, V.data_ptr(), ld, up, dm.data_ptr(), dF.data_ptr(), dV.data_ptr(), n, D)
    got = ops.meta_features_bwd(F, V, uids, dm[:n])
    _same(got[0], dF, "dF")
    _same(got[1], dV, "dV")


def test_rowdot_sigmoid_and_bwd(dev):
    """k = 48 of kp = 64 stored columns, the rows of A another PAD floats apart; columns >= k hold NaN and must not be read."""
    n, k, kp = 5, 48, 64
    A = _slab(dev, 12, n, kp)
    A[:, k:] = float("nan")
    w3, b3, dw = _rand(dev, 13, k) * 0.2, _rand(dev, 14, 1), _rand(dev, 15, n)
    w = torch.empty(n, device=dev)
    _raw("sagnn_rowdot_sigmoid_f32", A.data_ptr(), kp + PAD, w3.data_ptr(), b3.data_ptr(), w.data_ptr(), n, k)
    _same(ops.rowdot_sigmoid(A, w3, b3, k), w, "w")
    dA, dw3, db3 = _zeros(dev, n, kp), _zeros(dev, k), _zeros(dev, 1)
    _raw("sagnn_rowdot_sigmoid_bwd_f32", A.data_ptr(), kp + PAD, w3.data_ptr(), w.data_ptr(), dw.data_ptr(), dA.data_ptr(), kp,
         dw3.data_ptr(), db3.data_ptr(), n, k)
    got = ops.rowdot_sigmoid_bwd(A, w3, w, dw, k)
    for name, a, b in zip(("dA", "dw3", "db3"), got, (dA, dw3, db3)):
        _same(a, b, name)
    assert bool((got[0][:, k:] == 0).all()) and bool((got[0][:, :k] != 0).any())


def test_leaky_and_bwd(dev):
    a, g = _rand(dev, 16, 5, 64), _rand(dev, 17, 5, 64)
    a[0, :8] = 0.0                                                    # ties: the slope is `leaky`
    out = torch.empty_like(a)
    _raw("sagnn_leaky_f32", a.data_ptr(), None, out.data_ptr(), LEAKY, a.numel(), 0)
    _same(ops.leaky(a, LEAKY), out, "leaky")
    _raw("sagnn_leaky_f32", a.data_ptr(), g.data_ptr(), out.data_ptr(), LEAKY, a.numel(), 1)
    _same(ops.leaky_bwd(a, g, LEAKY), out, "leaky_bwd")


@pytest.mark.parametrize("weighted", (False, True))
def test_hinge(dev, weighted):
    n, scale = 5, 0.37
    pos, neg = _rand(dev, 18, n), _rand(dev, 19, n)
    w = [_rand(dev, 20 + j, n) for j in range(4)] if weighted else [None] * 4
    loss = _zeros(dev, 1)
    grads = [torch.full((n,), 9.0, device=dev) for _ in range(4 if weighted else 2)] + [None] * (0 if weighted else 2)
    _raw("sagnn_hinge_f32", pos.data_ptr(), neg.data_ptr(), *(ops._ptr(v) for v in w), scale, loss.data_ptr(),
         *(ops._ptr(v) for v in grads), n)
    got = ops.hinge(pos, neg, *w, scale=scale)
    assert float(loss) != 0.0
    _same(got[0], loss, "loss")
    for name, a, b in zip(("dpos", "dneg", "dwp", "dwn"), got[1:], grads):
        if b is None:
            assert a is None, f"{name}: the plain form has no weight gradients"
        else:
            _same(a, b, name)


def _ntd_input(dev, seed, layout):
    """x [N, T, D]: dense, or the permuted view of [T, N, D] storage (the GNN slab's layout)."""
    if layout == "dense":
        return _rand(dev, seed, N, T, D)
    return _rand(dev, seed, T, N, D).permute(1, 0, 2)


def _lstm_params(dev):
    return _rand(dev, 30, 2 * D, 4 * D) * 0.2, _rand(dev, 31, 4 * D) * 0.1


@pytest.mark.parametrize("layout", ("dense", "permuted"))
def test_lstm_forward_and_bptt(dev, layout):
    """lstm_fwd_train, then lstm_bwd in both forms (the weight gradient inside the launch / deferred to the second pass, with
    and without a dropout scale) on what it stored."""
    assert ops.lstm_bwd_supported(D)
    x = _ntd_input(dev, 32, layout)
    W, b = _lstm_params(dev)
    h, gates, cell = (torch.empty((N, T, w), device=dev) for w in (D, 4 * D, D))
    _raw("sagnn_lstm_fwd_train_f32", x.data_ptr(), x.stride(0), x.stride(1), N, T, D, W.data_ptr(), b.data_ptr(), 1.0, None,
         h.data_ptr(), T * D, gates.data_ptr(), cell.data_ptr())
    got = ops.lstm_fwd_train(x, W, b)
    for name, a, want in zip(("h", "gates", "cell"), got, (h, gates, cell)):
        _same(a, want, name)
    dh = _rand(dev, 33, N, T, D)
    drop = (torch.rand((N, T, D), generator=_gen(34)) < 0.5).float().mul(2.0).to(dev)
    nbytes = ops.lstm_bwd_workspace_bytes(N, T, D)
    assert nbytes == N * T * 4 * D * 4
    for deferred in (False, True):
        for mask in (None, drop):
            dx, dW, db = torch.empty((N, T, D), device=dev), _zeros(dev, 2 * D, 4 * D), _zeros(dev, 4 * D)
            ws = torch.empty(nbytes // 4, device=dev) if deferred else None
            _raw("sagnn_lstm_bwd_ws_f32", x.data_ptr(), x.stride(0), x.stride(1), h.data_ptr(), gates.data_ptr(), cell.data_ptr(),
                 dh.data_ptr(), T * D, ops._ptr(mask), W.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(), N, T, D,
                 ops._ptr(ws), nbytes if deferred else 0)
            got = ops.lstm_bwd(x, h, gates, cell, dh, mask, W, deferred_dw=deferred)
            for name, a, want in zip(("dx", "dW", "db"), got, (dx, dW, db)):
                _same(a, want, f"{name} (deferred_dw={deferred}, drop={'yes' if mask is not None else 'no'})")
            assert bool((dW != 0).any())


@pytest.mark.parametrize("ts", (T - 1, 0))
def test_lstm_bwd_step(dev, ts):
    """The last step (no recurrent gradients) and an earlier one, its dh_rec the strided right half of a [n, t, 2d] block."""
    gates, cell, dh = torch.sigmoid(_rand(dev, 35, N, T, 4 * D)), _rand(dev, 36, N, T, D), _rand(dev, 37, N, T, D)
    dxh, dc_in = _rand(dev, 38, N, T, 2 * D), _rand(dev, 39, N, D)
    last = ts == T - 1
    dh_rec = None if last else dxh[:, ts + 1, D:]
    want = torch.empty((N, 4 * D), device=dev), torch.empty((N, D), device=dev)
    _raw("sagnn_lstm_bwd_step_f32", gates.data_ptr(), cell.data_ptr(), dh.data_ptr(), T * D, None, ops._ptr(dh_rec), T * 2 * D,
         None if last else dc_in.data_ptr(), want[0].data_ptr(), want[1].data_ptr(), N, T, D, ts)
    got = torch.empty((N, 4 * D), device=dev), torch.empty((N, D), device=dev)
    ops.lstm_bwd_step(gates, cell, dh, None, dh_rec, None if last else dc_in, got[0], got[1], ts)
    _same(got[0], want[0], "dgates")
    _same(got[1], want[1], "dc_out")


@pytest.mark.parametrize("layout", ("dense", "padded", "permuted"))
def test_layernorm_td_bwd(dev, layout):
    """Into a new tensor and in place (out=g). "padded": every node's (t, d) block PAD floats apart."""
    if layout == "padded":
        x, g0 = (_slab(dev, s, N, T * D).view(N, T, D) for s in (40, 41))
        assert x.stride() == (T * D + PAD, D, 1)
    else:
        x, g0 = _ntd_input(dev, 40, layout), _ntd_input(dev, 41, layout)
    gamma = _rand(dev, 42, D)
    if layout == "permuted":                                          # not expressible: one node stride per operand
        with pytest.raises(ValueError, match="x"):
            ops.layernorm_td_bwd(x, g0.contiguous(), gamma)
        with pytest.raises(ValueError, match="g"):
            ops.layernorm_td_bwd(x.contiguous(), g0, gamma)
        x, g0 = x.contiguous(), g0.contiguous()
    ld = x.stride(0)
    dx, dgamma, dbeta = torch.empty((N, T, D), device=dev), _zeros(dev, D), _zeros(dev, D)
    _raw("sagnn_layernorm_td_bwd_f32", x.data_ptr(), ld, g0.data_ptr(), ld, N, T, D, gamma.data_ptr(), 1e-12, dx.data_ptr(), T * D,
         dgamma.data_ptr(), dbeta.data_ptr())
    got = ops.layernorm_td_bwd(x, g0, gamma)
    assert got[0].is_contiguous()
    for name, a, want in zip(("dx", "dgamma", "dbeta"), got, (dx, dgamma, dbeta)):
        _same(a, want, name)
    g = g0.clone() if layout != "padded" else torch.as_strided(g0._base.clone(), g0.shape, g0.stride())
    got = ops.layernorm_td_bwd(x, g, gamma, out=g)
    assert got[0] is g
    for name, a, want in zip(("dx in place", "dgamma", "dbeta"), got, (dx, dgamma, dbeta)):
        _same(a.contiguous(), want, name)


def _attn_params(dev):
    out = []
    for j in range(3):
        out += [_rand(dev, 50 + 2 * j, D, D) * 0.2, _rand(dev, 51 + 2 * j, D) * 0.1]
    return out


@pytest.mark.parametrize("layout", ("dense", "permuted"))
@pytest.mark.parametrize("ln", (True, False))
def test_attn_bwd_front(dev, layout, ln):
    """With the layer norm (y returned) and without (gamma None: y is x, not written); g_out with padded rows."""
    assert ops.attn_bwd_front_supported(D, T, HEADS)
    x, g_out = _ntd_input(dev, 56, layout), _slab(dev, 57, N)
    gamma, beta = (_rand(dev, 58, D), _rand(dev, 59, D)) if ln else (None, None)
    w = _attn_params(dev)
    dqkv = torch.empty((N * T, 3 * D), device=dev)
    y = torch.empty((N * T, D), device=dev) if ln else None
    _raw("sagnn_attn_bwd_front_f32", x.data_ptr(), x.stride(0), x.stride(1), N, T, D, HEADS, ops._ptr(gamma), ops._ptr(beta), 1e-12,
         int(ln), *(v.data_ptr() for v in w), g_out.data_ptr(), D + PAD, dqkv.data_ptr(), ops._ptr(y))
    got_y, got_dqkv = ops.attn_bwd_front(x, gamma, beta, *w, HEADS, g_out)
    _same(got_dqkv, dqkv, "dqkv")
    if ln:
        _same(got_y, y, "y")
        assert ops.attn_bwd_front(x, gamma, beta, *w, HEADS, g_out, want_y=False)[0] is None
    else:
        assert got_y is None


def test_attn_bwd_and_tail(dev):
    assert ops.attn_bwd_tail_supported(D)
    qkv0, g_out, y0 = _rand(dev, 60, N * T, 3 * D), _slab(dev, 61, N), _rand(dev, 62, N * T, D)
    want = qkv0.clone()
    _raw("sagnn_attn_bwd_f32", want.data_ptr(), g_out.data_ptr(), D + PAD, N, T, D, HEADS)
    qkv = qkv0.clone()
    assert ops.attn_bwd(qkv, g_out, N, T, HEADS) is qkv
    _same(qkv, want, "dqkv")
    assert not torch.equal(qkv, qkv0)
    Wqkv = _rand(dev, 63, D, 3 * D) * 0.2
    dy, dW, db = y0.clone(), _zeros(dev, D, 3 * D), _zeros(dev, 3 * D)
    _raw("sagnn_attn_bwd_tail_f32", dy.data_ptr(), want.data_ptr(), N * T, D, Wqkv.data_ptr(), dW.data_ptr(), db.data_ptr())
    y, got_dW, got_db = y0.clone(), _zeros(dev, D, 3 * D), _zeros(dev, 3 * D)
    assert ops.attn_bwd_tail(y, qkv, Wqkv, got_dW, got_db) is y
    for name, a, b in (("dy", y, dy), ("dWqkv", got_dW, dW), ("dbqkv", got_db, db)):
        _same(a, b, name)


class Launched(Exception):
    """A refused call must not get as far as asking for the library."""


def test_unchecked_ids_and_counts_are_refused_with_nothing_launched(dev, monkeypatch):
    U, I, S = _slab(dev, 70, NU), _slab(dev, 71, NI), _slab(dev, 72, NL)
    n = 5
    (uids, _), (iids, _), (locs, _) = _ids(dev, UIDS, n), _ids(dev, IIDS, n), _ids(dev, LOCS, n)
    g, dm = _rand(dev, 73, n), _rand(dev, 74, n, 3 * D)
    wide = _rand(dev, 75, NI, 2 * D)
    strided = torch.zeros(2 * n, dtype=torch.int32, device=dev)[::2]

    def load():
        raise Launched
    monkeypatch.setattr(ops._lib, "load", load)
    pair = lambda **kw: ops.pair_score_bwd(U, I, kw.get("uids", uids), kw.get("iids", iids), kw.get("g", g), S=S,    # noqa: E731
                                           A=kw.get("A", I), locs=kw.get("locs", locs), leaky=LEAKY)
    with pytest.raises(Launched):                                     # the control: these arguments are accepted
        pair()
    for name in ("uids", "iids", "locs"):
        with pytest.raises(TypeError, match=name):
            pair(**{name: locals()[name].long()})
        with pytest.raises(TypeError, match=name):
            pair(**{name: strided})
    with pytest.raises(ValueError, match="^g:"):
        pair(g=g[:4])
    with pytest.raises(ValueError, match="^A:"):
        pair(A=wide)
    for fn, tail in ((ops.prod_leaky_sum, (LEAKY,)), (ops.prod_leaky_sum_bwd, (LEAKY, g))):
        with pytest.raises(Launched):
            fn(U, I, uids, iids, *tail)
        with pytest.raises(TypeError, match="uids"):
            fn(U, I, uids.long(), iids, *tail)
        with pytest.raises(TypeError, match="iids"):
            fn(U, I, uids, iids.long(), *tail)
        with pytest.raises(TypeError, match="iids"):
            fn(U, I, uids, strided, *tail)
        with pytest.raises(ValueError, match="^Y:"):
            fn(U, wide, uids, iids, *tail)
    with pytest.raises(ValueError, match="^g:"):
        ops.prod_leaky_sum_bwd(U, I, uids, iids, LEAKY, g[:4])
    for fn, tail in ((ops.meta_features, ()), (ops.meta_features_bwd, (dm,))):
        with pytest.raises(Launched):
            fn(U, U, uids, *tail)
        with pytest.raises(TypeError, match="uids"):
            fn(U, U, uids.long(), *tail)
        with pytest.raises(TypeError, match="uids"):
            fn(U, U, strided, *tail)
        with pytest.raises(ValueError, match="^V:"):
            fn(U, wide[:NU], uids, *tail)
    with pytest.raises(ValueError, match="^dm:"):
        ops.meta_features_bwd(U, U, uids, dm[:4])
