"""GPU parity of the backward pass of the interval stack against
torch.autograd over the oracle's torch restatement (CPU, float64)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu


def _case(rng, U, I, dens, d):
    m = sp.csr_matrix((rng.random((U, I)) < dens).astype(np.intc))
    u0 = rng.standard_normal((U, d)).astype(np.float32)
    i0 = rng.standard_normal((I, d)).astype(np.float32)
    gu = rng.standard_normal((U, d)).astype(np.float32)
    gi = rng.standard_normal((I, d)).astype(np.float32)
    return m, u0, i0, gu, gi


@pytest.mark.parametrize("d,L,tuning", [(64, 2, None), (32, 1, (4, 8, 64)), (128, 3, (8, 16, 64)), (64, 3, (2, 4, 64))])
def test_gnn_interval_backward_vs_autograd(dev, d, L, tuning):
    from sa_gnn_amd import graph, ops
    rng = np.random.default_rng(d * 10 + L)
    U, I = 157, 211
    m, u0, i0, gu, gi = _case(rng, U, I, 0.07, d)
    m = m.tolil()
    m[5, :] = 0                      # an isolated user: s = 0 exactly, the tie case of tf.maximum
    m = sp.csr_matrix(m)
    adj_idx, tp_idx = O.trans_to_lsts(m)[0], O.trans_to_lsts(O.transpose(m))[0]
    # oracle: torch autograd in float64
    tu = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    ti = torch.tensor(i0, dtype=torch.float64, requires_grad=True)
    ou, oi = O.torch_gnn_interval(tu, ti, adj_idx, tp_idx, L, 0.5)
    (ou * torch.tensor(gu, dtype=torch.float64)).sum().add((oi * torch.tensor(gi, dtype=torch.float64)).sum()).backward()
    # HIP path
    fwd, tp = graph.interval_pair(m, dev, tuning=tuning)
    mask_u = torch.empty((L, U, d // 4), dtype=torch.uint8, device=dev)
    mask_i = torch.empty((L, I, d // 4), dtype=torch.uint8, device=dev)
    uo = torch.empty((U, d), device=dev)
    io = torch.empty((I, d), device=dev)
    ops.gnn_interval(fwd.plan, tp.plan, torch.from_numpy(u0).to(dev), torch.from_numpy(i0).to(dev), L, 0.5, uo, io,
                     mask_u=mask_u, mask_i=mask_i)
    np.testing.assert_allclose(uo.cpu().numpy(), ou.detach().numpy(), rtol=1e-4, atol=1e-4)
    du, di = ops.gnn_interval_bwd(fwd.plan, tp.plan, torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev),
                                  L, 0.5, mask_u, mask_i)
    scale = max(float(tu.grad.abs().max()), 1.0)
    np.testing.assert_allclose(du.cpu().numpy(), tu.grad.numpy(), rtol=1e-4, atol=2e-6 * scale * L * 50)
    np.testing.assert_allclose(di.cpu().numpy(), ti.grad.numpy(), rtol=1e-4, atol=2e-6 * scale * L * 50)


def test_autograd_function_end_to_end(dev):
    """ag.gnn_interval inside a torch graph: gradients of a scalar loss w.r.t. the embedding tables."""
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import graph
    rng = np.random.default_rng(3)
    U, I, d, L = 90, 120, 64, 2
    m, u0, i0, _, _ = _case(rng, U, I, 0.1, d)
    fwd, tp = graph.interval_pair(m, dev)
    pu = torch.from_numpy(u0).to(dev).requires_grad_(True)
    pi = torch.from_numpy(i0).to(dev).requires_grad_(True)
    uo, io = ag.gnn_interval(pu, pi, fwd.plan, tp.plan, L, 0.5)
    loss = (uo ** 2).sum() * 0.5 + (io[:, :8] * 3.0).sum()
    loss.backward()
    tu = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    ti = torch.tensor(i0, dtype=torch.float64, requires_grad=True)
    ou, oi = O.torch_gnn_interval(tu, ti, O.trans_to_lsts(m)[0], O.trans_to_lsts(O.transpose(m))[0], L, 0.5)
    ((ou ** 2).sum() * 0.5 + (oi[:, :8] * 3.0).sum()).backward()
    s = float(tu.grad.abs().max())
    np.testing.assert_allclose(pu.grad.cpu().numpy(), tu.grad.numpy(), rtol=2e-4, atol=1e-5 * s)
    np.testing.assert_allclose(pi.grad.cpu().numpy(), ti.grad.numpy(), rtol=2e-4, atol=1e-5 * s)


# Shapes whose backward takes the generic entries: no fused attention-backward front (t or d_k outside its table, or
# d > 128), and beyond d = 64 neither the fused tail nor the one-launch BPTT. d = 192 with 16 heads has d_k = 12.
GENERIC_ROUTE = {(256, 3, 90, 16), (256, 12, 19, 16), (192, 4, 61, 16), (128, 8, 41, 16), (128, 20, 17, 16), (64, 7, 53, 16),
                 (64, 10, 37, 16), (64, 20, 23, 16), (32, 7, 45, 8), (64, 3, 300, 8)}


@pytest.mark.parametrize("d,t,n,heads", [(64, 3, 300, 16), (32, 2, 130, 16), (64, 1, 70, 16), (64, 5, 97, 4), (128, 3, 90, 16),
                                          (64, 8, 41, 16), (32, 6, 53, 16), (64, 12, 19, 16), (64, 16, 23, 16), (32, 12, 31, 16), (32, 16, 17, 16),
                                          (64, 2, 1000, 16), (64, 4, 77, 16), (64, 5, 61, 16), (64, 6, 37, 16),
                                          (32, 1, 33, 16), (32, 3, 90, 16), (32, 4, 70, 16), (32, 5, 45, 16), (32, 8, 29, 16)]
                         + sorted(GENERIC_ROUTE, reverse=True))
def test_interval_fusion_backward_vs_autograd(dev, d, t, n, heads):
    """Every gradient of the fusion (x and all ten parameter tensors) against float64 autograd. The shapes of
    GENERIC_ROUTE must run the generic entries (test ids: "generic" selects the per-kernel tests below, these cases
    assert their route here)."""
    from sa_gnn_amd import _lib, ops
    from sa_gnn_amd import autograd as ag
    if (d, t, n, heads) in GENERIC_ROUTE:
        # the backward runs on PyTorch's autograd thread, whose engine is the default one, as this thread's is
        assert ag.FUSED_ATTN_BWD and ag.FUSED_BPTT and _lib.load().sagnn_get_engine() == 0
        assert not ops.attn_bwd_front_supported(d, t, heads), "layernorm_td + dense_nn + sagnn_attn_bwd_f32 must run"
        if d > 64:
            assert not ops.attn_bwd_tail_supported(d), "dense_tn + dense_nn must run"
            assert not ops.lstm_bwd_supported(d), "the sagnn_lstm_bwd_step_f32 loop must run"
    rng = np.random.default_rng(d + t + n)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    gout = rng.standard_normal((n, d)).astype(np.float32)
    # oracle
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    out = O.torch_interval_fusion(tx, tp, heads)
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    # HIP path; x given as a [t, n, d] storage viewed [n, t, d] (the exchange layout)
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev).permute(1, 0, 2).requires_grad_(True)
    pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
    got = ag.interval_fusion(xd, pd, heads)
    np.testing.assert_allclose(got.detach().cpu().numpy(), out.detach().numpy(), rtol=1e-4, atol=2e-5)
    got.backward(torch.from_numpy(gout).to(dev))

    def check(name, a, b):
        a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().numpy()
        # relative bar 1e-4 plus an absolute floor: some gradients are analytically ~0 (a key bias
        # shifts every score of a row alike; only the 1e-8 in the normaliser breaks the symmetry),
        # what remains of them is fp32 accumulation noise over n*t rows: eps32 * sqrt(n*t), 8e-6 at n*t ~ 1e3 (the rule of
        # test_training_forward_and_backward_many_tiles_per_block; a random sweep of shapes — tools/fuzz_gpu.py — meets
        # |dWk| ~ 9e-6 with an error of 5.02e-6 at n*t ~ 2e3)
        tol = 1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), 8e-6 * max(1.0, np.sqrt(n * t / 1000.0)))
        bad = np.abs(a - b) > tol
        assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"

    check("dx", xd.grad, tx.grad)
    for k in p:
        check("d" + k, pd[k].grad, tp[k].grad)


@pytest.mark.parametrize("d,t,n,heads", [(64, 3, 300, 16), (32, 4, 70, 16)])
def test_interval_fusion_backward_generic_under_valu(dev, d, t, n, heads):
    """Under the VALU engine the attention backward has no fused kernels at any shape: layernorm_td + dense_nn +
    sagnn_attn_bwd_f32, then dense_tn / dense_nn. The engine is per calling thread and torch runs a backward on a
    thread of its own, so the two halves are called here directly, on the thread that selected the engine."""
    from sa_gnn_amd import ops
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(d + t + n)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    gout = rng.standard_normal((n, d)).astype(np.float32)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    out = O.torch_interval_fusion(tx, tp, heads)
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev).permute(1, 0, 2)
    pd = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    names = ("lstm_W", "lstm_b", "ln_gamma", "ln_beta", "Wq", "bq", "Wk", "bk", "Wv", "bv")
    with ops.engine("valu"):
        assert not ops.attn_bwd_front_supported(d, t, heads) and not ops.attn_bwd_tail_supported(d)
        got, h, gates, cell = ag._fusion_forward(xd, *(pd[k] for k in names), heads, None)
        grads = ag._fusion_backward(xd, *(pd[k] for k in names if k != "lstm_b"), h, gates, cell, None, heads,
                                    torch.from_numpy(gout).to(dev))
    assert ops.get_engine() == "f16x2"
    np.testing.assert_allclose(got.cpu().numpy(), out.detach().numpy(), rtol=1e-4, atol=2e-5)
    for name, a, b in [("dx", grads[0], tx.grad)] + [("d" + k, g, tp[k].grad) for k, g in zip(names, grads[1:])]:
        a, b = a.cpu().numpy().astype(np.float64), b.numpy()
        tol = 1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), 8e-6 * max(1.0, np.sqrt(n * t / 1000.0)))   # the rule of the test above
        bad = np.abs(a - b) > tol
        assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"


# ---- the generic backward entries, one kernel at a time ----------------------------------------------------------------
# Tolerance: |got - want| <= 1e-4 |want| + 2e-5 max |want| (the rule of the composite test without its floor); the
# atomically accumulated dgamma / dbeta add the eps32 * sqrt(n * t) floor that test documents.

def _close(name, got, want, floor=0.0):
    a, b = got.detach().double().cpu().numpy().reshape(want.shape), want.detach().numpy()
    assert np.isfinite(a).all(), f"{name}: non-finite"
    tol = 1e-4 * np.abs(b) + 2e-5 * np.abs(b).max() + floor
    bad = np.abs(a - b) > tol
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"


# (d, t, extra node stride). Vector kernel: d a power of two, t * d <= 2048, 16-byte rows. Scalar kernel: the rest.
LN_VECTOR = [(64, 3, 0), (32, 1, 0), (128, 16, 0)]
LN_SCALAR = [(192, 3, 0), (128, 20, 0), (256, 12, 0), (64, 33, 0), (64, 3, 2)]


def _ln_cases():
    # n = 20011 (more nodes than the persistent grid has waves) where n * t * d stays near 1e7
    return [(d, t, x, n) for d, t, x in LN_VECTOR + LN_SCALAR for n in (1, 5, 4099, 20011) if n < 20011 or t * d <= 576]


@pytest.mark.parametrize("d,t,extra,n", _ln_cases())
def test_generic_layernorm_td_bwd(dev, d, t, extra, n):
    """sagnn_layernorm_td_bwd_f32 alone against float64 autograd of O.torch_layer_norm_td, out of place and with dh
    aliasing dy. A node stride of t * d + 2 is legal for the scalar kernel only."""
    from sa_gnn_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(d * t + n)
    ld = t * d + extra
    h = (rng.standard_normal((n, t, d)) * 1.5 + 0.3).astype(np.float32)
    dy = rng.standard_normal((n, t, d)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    th, tg = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (h, gamma))
    tb = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    (O.torch_layer_norm_td(th, tg, tb) * torch.tensor(dy, dtype=torch.float64)).sum().backward()

    def slab(v):
        buf = torch.full((n, ld), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :t * d] = torch.from_numpy(v.reshape(n, t * d)).to(dev)
        return buf
    hd, dyd, gd = slab(h), slab(dy), torch.from_numpy(gamma).to(dev)
    floor = float(np.finfo(np.float32).eps) * np.sqrt(n * t)
    for alias in (False, True):
        dh = dyd if alias else torch.full((n, ld), float("nan"), dtype=torch.float32, device=dev)
        dgamma, dbeta = torch.zeros(d, device=dev), torch.zeros(d, device=dev)
        ops.check(lib.sagnn_layernorm_td_bwd_f32(hd.data_ptr(), ld, dyd.data_ptr(), ld, n, t, d, gd.data_ptr(), 1e-12,
                                                 dh.data_ptr(), ld, dgamma.data_ptr(), dbeta.data_ptr(), ops._stream()))
        _close("dh", dh[:, :t * d], th.grad.reshape(n, t * d))
        _close("dgamma", dgamma, tg.grad, floor)
        _close("dbeta", dbeta, tb.grad, floor)
        assert extra == 0 or bool(torch.isnan(dh[:, t * d:]).all())            # the gap between nodes is not written


def _attn_slots(d, heads, t):
    """Nodes per block of sagnn_attn_bwd_f32: 256 / d, halved until their LDS (Q|K|V, the score tiles, g where d_k is
    not a power of two) fits 64 KiB."""
    dk = d // heads
    per_slot = 4 * (3 * t * d + heads * (t * t + 2 * t) + (d if dk & (dk - 1) else 0))
    slots = max(256 // d, 1)
    while slots > 1 and slots * per_slot > 64 * 1024:
        slots >>= 1
    assert slots * per_slot <= 160 * 1024
    return slots


# (d, heads, t): every d, every d_k of {1, 2, 4, 16} at every d, every t; d = 192 / 16 heads is d_k = 12
ATTN_SHAPES = [(16, 16, 1), (16, 8, 7), (16, 4, 32), (16, 1, 10), (16, 16, 20), (16, 8, 2),
               (32, 32, 2), (32, 16, 10), (32, 8, 20), (32, 2, 7), (32, 8, 32), (32, 16, 1),
               (64, 64, 7), (64, 32, 1), (64, 16, 20), (64, 4, 32), (64, 16, 2), (64, 16, 10),
               (128, 128, 2), (128, 64, 10), (128, 32, 7), (128, 8, 32), (128, 32, 20), (128, 8, 1),
               (192, 48, 1), (192, 12, 7), (192, 96, 2), (192, 192, 10), (192, 12, 20), (192, 12, 32), (192, 16, 4),
               (256, 256, 1), (256, 128, 2), (256, 64, 7), (256, 16, 10), (256, 16, 20), (256, 16, 12)]     # d = 256 at t = 32 is beyond the entry's LDS limit


def _attn_cases():
    out = []
    for d, heads, t in ATTN_SHAPES:
        slots = _attn_slots(d, heads, t)
        ns = {1, slots - 1, slots + 1}
        if t * d <= 256:               # n * t * 3d near 1e7; at d >= 192 (one node per block) the 16 384-block cap bites
            ns.add(20011)
        out += [(d, heads, t, n) for n in sorted(ns) if n > 0]
    return out


def _attn_mean(q, k, v, heads):
    """O.torch_mhsa_mean from its Q, K, V on (Utils/attention.py:35-45, :74-78, model.py:154-155)."""
    n, t, d = q.shape
    dk = d // heads
    q, k, v = (z.reshape(n, t, heads, dk).permute(0, 2, 1, 3) for z in (q, k, v))
    scores = torch.exp((q @ k.transpose(-1, -2)) / float(np.sqrt(dk)))
    attn = scores / (scores.sum(dim=-1, keepdim=True) + 1e-8)
    return (attn @ v).permute(0, 2, 1, 3).reshape(n, t, d).mean(dim=1)


def test_generic_attn_mean_is_the_oracle():
    """_attn_mean above IS O.torch_mhsa_mean once Q, K, V are formed (a CPU check of the test's own reference)."""
    rng = np.random.default_rng(4)
    x = torch.tensor(rng.standard_normal((5, 3, 32)))
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in O.init_fusion_params(32, rng).items()}
    want = O.torch_mhsa_mean(x, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], 8)
    got = _attn_mean(x @ p["Wq"] + p["bq"], x @ p["Wk"] + p["bk"], x @ p["Wv"] + p["bv"], 8)
    assert torch.equal(got, want)


@pytest.mark.parametrize("d,heads,t,n", _attn_cases())
def test_generic_attn_bwd_f32(dev, d, heads, t, n):
    """sagnn_attn_bwd_f32 alone: Q|K|V [n, t, 3d] -> dQ|dK|dV in place against float64 autograd of the attention +
    mean on the same Q, K, V; g_out is a row view of a wider slab."""
    from sa_gnn_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(d * 100 + t * 7 + heads)
    qkv = (rng.standard_normal((n, t, 3 * d)) * 0.7).astype(np.float32)
    g = rng.standard_normal((n, d)).astype(np.float32)
    tq = torch.tensor(qkv, dtype=torch.float64, requires_grad=True)
    out = _attn_mean(tq[:, :, :d], tq[:, :, d:2 * d], tq[:, :, 2 * d:], heads)
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    qd = torch.from_numpy(qkv).to(dev)
    gslab = torch.full((n, 2 * d), float("nan"), dtype=torch.float32, device=dev)
    gslab[:, d:] = torch.from_numpy(g).to(dev)
    ops.check(lib.sagnn_attn_bwd_f32(qd.data_ptr(), gslab[:, d:].data_ptr(), 2 * d, n, t, d, heads, ops._stream()))
    for i, name in enumerate(("dQ", "dK", "dV")):
        _close(name, qd[:, :, i * d:(i + 1) * d].contiguous(), tq.grad[:, :, i * d:(i + 1) * d])


@pytest.mark.parametrize("d", (32, 96, 256))
@pytest.mark.parametrize("ts", (0, 2, 4))
@pytest.mark.parametrize("drop", (False, True))
def test_generic_lstm_bwd_step(dev, d, ts, drop):
    """sagnn_lstm_bwd_step_f32 alone, t = 5: the first step (no previous cell), a middle one, and the last (dh_rec and
    dc_in NULL), against float64 autograd of one step of O.torch_basic_lstm from its gate pre-activations:
    c = c_prev sigmoid(f + 1) + sigmoid(i) tanh(j), h = tanh(c) sigmoid(o), loss = <dh, h> + <dc_in, c>."""
    from sa_gnn_amd import _lib, ops
    lib = _lib.load()
    n, t = 257, 5
    last = ts == t - 1
    rng = np.random.default_rng(d + ts + 10 * drop)
    G = torch.tensor(rng.standard_normal((n, 4 * d)), dtype=torch.float64, requires_grad=True)
    cp = torch.tensor(rng.standard_normal((n, d)) if ts > 0 else np.zeros((n, d)), dtype=torch.float64, requires_grad=True)
    gi, gj, gf, go = torch.split(G, d, dim=1)
    acts = (torch.sigmoid(gi), torch.tanh(gj), torch.sigmoid(gf + 1.0), torch.sigmoid(go))
    c = cp * acts[2] + acts[0] * acts[1]
    hh = torch.tanh(c) * acts[3]
    dh_ext = rng.standard_normal((n, t, d)).astype(np.float32)
    scale = ((rng.random((n, t, d)) < 0.5) * 2.0).astype(np.float32)
    dh_rec = rng.standard_normal((n, d)).astype(np.float32)
    dc_in = rng.standard_normal((n, d)).astype(np.float32)
    dh = torch.tensor(dh_ext[:, ts], dtype=torch.float64)
    if drop:
        dh = dh * torch.tensor(scale[:, ts], dtype=torch.float64)
    if not last:
        dh = dh + torch.tensor(dh_rec, dtype=torch.float64)
    loss = (hh * dh).sum()
    if not last:
        loss = loss + (c * torch.tensor(dc_in, dtype=torch.float64)).sum()
    loss.backward()
    # what the training forward stores: activations [n, t, 4d] and cell states [n, t, d]; the other steps hold noise
    gates = rng.standard_normal((n, t, 4 * d)).astype(np.float32)
    cell = rng.standard_normal((n, t, d)).astype(np.float32)
    gates[:, ts] = torch.cat(acts, dim=1).detach().numpy().astype(np.float32)
    cell[:, ts] = c.detach().numpy().astype(np.float32)
    if ts > 0:
        cell[:, ts - 1] = cp.detach().numpy().astype(np.float32)
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    gd, cd, dhd, sd, dcd = to(gates), to(cell), to(dh_ext), to(scale), to(dc_in)
    rec = torch.full((n, 2 * d), float("nan"), dtype=torch.float32, device=dev)      # [dx | dh_rec] rows, as the host keeps them
    rec[:, d:] = to(dh_rec)
    dgates = torch.full((n, 4 * d), float("nan"), dtype=torch.float32, device=dev)
    dc_out = torch.full((n, d), float("nan"), dtype=torch.float32, device=dev)
    ops.check(lib.sagnn_lstm_bwd_step_f32(gd.data_ptr(), cd.data_ptr(), dhd.data_ptr(), t * d, sd.data_ptr() if drop else None,
                                          None if last else rec[:, d:].data_ptr(), 2 * d, None if last else dcd.data_ptr(),
                                          dgates.data_ptr(), dc_out.data_ptr(), n, t, d, ts, ops._stream()))
    _close("dgates", dgates, G.grad)
    _close("dc_out", dc_out, cp.grad)


def test_interval_fusion_backward_with_output_dropout(dev):
    """DropoutWrapper(output_keep_prob): the mask scales the emitted h only; gradients follow."""
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(77)
    n, t, d, heads = 150, 3, 64, 16
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    scale = ((rng.random((n, t, d)) < 0.5) * 2.0).astype(np.float32)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    h = O.torch_basic_lstm(tx, tp["lstm_W"], tp["lstm_b"]) * torch.tensor(scale, dtype=torch.float64)
    out = O.torch_mhsa_mean(O.torch_layer_norm_td(h, tp["ln_gamma"], tp["ln_beta"]), tp["Wq"], tp["bq"], tp["Wk"],
                            tp["bk"], tp["Wv"], tp["bv"], heads)
    out.square().sum().backward()
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
    got = ag.interval_fusion(xd, pd, heads, drop_scale=torch.from_numpy(scale).to(dev))
    np.testing.assert_allclose(got.detach().cpu().numpy(), out.detach().numpy(), rtol=1e-4, atol=2e-5)
    got.square().sum().backward()
    for name, a, b in [("dx", xd.grad, tx.grad)] + [("d" + k, pd[k].grad, tp[k].grad) for k in p]:
        a, b = a.cpu().numpy().astype(np.float64), b.numpy()
        tol = 1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), 2e-5)   # floor: see the test above
        assert (np.abs(a - b) <= tol).all(), name


@pytest.mark.parametrize("d,t,n", [(64, 4, 20011), (32, 3, 33000)])
def test_fused_bptt_matches_step_loop(dev, d, t, n, monkeypatch):
    """sagnn_lstm_bwd_f32 (one launch, gate gradients on chip) against the per-step entries it
    replaces, at sizes where every block walks several chunks and the last chunk is ragged."""
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(d * t)
    p = O.init_fusion_params(d, rng)
    x = torch.from_numpy(rng.standard_normal((n, t, d)).astype(np.float32)).to(dev)
    gout = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    scale = torch.from_numpy(((rng.random((n, t, d)) < 0.7) / 0.7).astype(np.float32)).to(dev)
    grads = {}
    for mode in ("fused", "steps"):
        monkeypatch.setattr(ag, "FUSED_BPTT", mode == "fused")
        xd = x.clone().requires_grad_(True)
        pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
        ag.interval_fusion(xd, pd, 16, drop_scale=scale).backward(gout)
        grads[mode] = {"x": xd.grad, **{k: pd[k].grad for k in ("lstm_W", "lstm_b")}}
    for k in grads["fused"]:
        a, b = grads["fused"][k].double().cpu().numpy(), grads["steps"][k].double().cpu().numpy()
        tol = 1e-4 * np.abs(b) + 2e-5 * np.abs(b).max()
        assert (np.abs(a - b) <= tol).all(), f"{k}: worst {np.abs(a - b).max():.3e} (scale {np.abs(b).max():.3e})"


def test_adam_step_matches_tf_formula(dev):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(1000).astype(np.float32)
    params = {"w": torch.from_numpy(p0.copy()).to(dev)}
    opt = ops.Adam(params, lr=1e-2, decay=0.96, decay_step=2, reg=1e-2, reg_names={"w"})
    p, m, v = p0.astype(np.float64), np.zeros(1000), np.zeros(1000)
    for step in range(1, 6):
        g = rng.standard_normal(1000).astype(np.float32)
        opt.step({"w": torch.from_numpy(g).to(dev)})
        lr = 1e-2 * 0.96 ** ((step - 1) // 2)
        gg = g + 2 * 1e-2 * p
        m = 0.9 * m + 0.1 * gg
        v = 0.999 * v + 0.001 * gg * gg
        p = p - lr * np.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step) * m / (np.sqrt(v) + 1e-8)
    np.testing.assert_allclose(params["w"].cpu().numpy(), p, rtol=1e-4, atol=1e-5)


def test_adam_multi_more_tensors_than_one_table_with_an_empty_one(dev):
    """sagnn_adam_multi_f32 walks its tensors in tables of 48 non-empty ones. 60 tensors with an empty one in the
    first table: the second launch must start where the first stopped — every tensor takes exactly ONE step."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(5)
    sizes = [int(s) for s in rng.integers(4, 3000, size=60)]
    sizes[10] = 0
    p0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    g0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    params = {f"w{i}": torch.from_numpy(a.copy()).to(dev) for i, a in enumerate(p0)}
    opt = ops.Adam(params, lr=1e-2, reg=1e-2, reg_names={f"w{i}" for i in range(0, 60, 2)})
    opt.step({f"w{i}": torch.from_numpy(g).to(dev) for i, g in enumerate(g0)})
    for i in range(60):
        gg = g0[i].astype(np.float64) + (2 * 1e-2 * p0[i] if i % 2 == 0 else 0.0)
        m, v = 0.1 * gg, 0.001 * gg * gg
        want = p0[i] - 1e-2 * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (np.sqrt(v) + 1e-8)
        np.testing.assert_allclose(params[f"w{i}"].cpu().numpy(), want, rtol=1e-4, atol=1e-5, err_msg=f"tensor {i}")


def test_gnn_interval_backward_with_duplicated_stored_entries(dev):
    """A subMat with a duplicated stored (u, i): the forward counts it twice on the user side and once
    on the item side (DataHandler.transpose merges it, DataHandler.py:9-11), so the two patterns are
    not transposes of each other and the backward needs the exact adjoints (graph.interval_pair)."""
    from sa_gnn_amd import graph, ops
    rng = np.random.default_rng(99)
    U, I, d, L = 61, 83, 64, 2
    base = sp.csr_matrix((rng.random((U, I)) < 0.08).astype(np.intc))
    indptr, indices = base.indptr.copy(), base.indices.copy()
    # duplicate the first stored entry of rows 3, 10 and 40 (and one of them twice)
    rows, cols = [], []
    for r in range(U):
        cs = list(indices[indptr[r]:indptr[r + 1]])
        if r in (3, 10, 40) and cs:
            cs = [cs[0]] * (3 if r == 10 else 2) + cs[1:]
        rows += [r] * len(cs)
        cols += cs
    ptr = np.zeros(U + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=U), out=ptr[1:])
    m = sp.csr_matrix((np.ones(len(cols), dtype=np.intc), np.asarray(cols, dtype=np.int32), ptr), shape=(U, I))
    adj_idx, tp_idx = O.trans_to_lsts(m)[0], O.trans_to_lsts(O.transpose(m))[0]
    assert len(adj_idx) > len(tp_idx)                        # the quirk is present
    u0 = rng.standard_normal((U, d)).astype(np.float32)
    i0 = rng.standard_normal((I, d)).astype(np.float32)
    gu = rng.standard_normal((U, d)).astype(np.float32)
    gi = rng.standard_normal((I, d)).astype(np.float32)
    tu = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    ti = torch.tensor(i0, dtype=torch.float64, requires_grad=True)
    ou, oi = O.torch_gnn_interval(tu, ti, adj_idx, tp_idx, L, 0.5)
    ((ou * torch.tensor(gu, dtype=torch.float64)).sum() + (oi * torch.tensor(gi, dtype=torch.float64)).sum()).backward()
    fwd, tp = graph.interval_pair(m, dev)
    assert fwd.plan.partner_adjoint is not None and tp.plan.partner_adjoint is not None
    mask_u = torch.empty((L, U, d // 4), dtype=torch.uint8, device=dev)
    mask_i = torch.empty((L, I, d // 4), dtype=torch.uint8, device=dev)
    uo, io = torch.empty((U, d), device=dev), torch.empty((I, d), device=dev)
    ops.gnn_interval(fwd.plan, tp.plan, torch.from_numpy(u0).to(dev), torch.from_numpy(i0).to(dev), L, 0.5, uo, io,
                     mask_u=mask_u, mask_i=mask_i)
    np.testing.assert_allclose(uo.cpu().numpy(), ou.detach().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(io.cpu().numpy(), oi.detach().numpy(), rtol=1e-4, atol=1e-4)
    du, di = ops.gnn_interval_bwd(fwd.plan, tp.plan, torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev),
                                  L, 0.5, mask_u, mask_i)
    scale = max(float(tu.grad.abs().max()), 1.0)
    np.testing.assert_allclose(du.cpu().numpy(), tu.grad.numpy(), rtol=1e-4, atol=1e-4 * scale)
    np.testing.assert_allclose(di.cpu().numpy(), ti.grad.numpy(), rtol=1e-4, atol=1e-4 * scale)
    # a hand-made pair without the adjoints is refused instead of giving silently wrong gradients
    fwd.plan.partner_adjoint = tp.plan.partner_adjoint = None
    with pytest.raises(ValueError, match="transposed pair"):
        ops.gnn_interval_bwd(fwd.plan, tp.plan, torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev), L, 0.5,
                             mask_u, mask_i)
