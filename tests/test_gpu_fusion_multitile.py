"""GPU parity of the persistent fusion kernels in their steady state.

lstm_fwd_mfma_kernel, ln_mhsa_mean_mfma_kernel and the attention-backward front walk
`for tile = blockIdx.x; tile < n_tiles; tile += gridDim.x` with one block per CU (256): a block
takes a second tile only above 32,768 rows (LSTM) / 256 * 4 * (32 / t) nodes (attention). The
node counts here force >= 3 tiles per block with a ragged last tile, so the next-tile prefetch,
the reuse of the LDS staging tiles across tiles and the tail predicates are checked against the
numpy oracle (reference model.py:135-155), not only against another HIP path. fp32, 1e-4."""
import numpy as np
import pytest
import torch

from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 2e-5

# (d, t, n): 100,003 rows = 782 LSTM tiles (3-4 per block, 35 rows in the last); 70,001 at t = 16
# = 8,751 attention tiles (34 per block, one node in the last)
CASES = [(64, 2, 100_003), (64, 3, 100_003), (64, 16, 70_001), (32, 2, 100_003), (32, 16, 70_001), (32, 3, 131_077),
         # d = 128 (config 3): one LSTM launch per step over (row tiles) x (4 hidden slices), attention over two column halves
         (128, 6, 70_001), (128, 3, 50_003)]


def _params(d, rng, dev):
    p = O.init_fusion_params(d, rng)
    return p, {k: torch.from_numpy(v).to(dev) for k, v in p.items()}


def _check(got, want, what):
    got = got.cpu().numpy()
    err = np.abs(got - want)
    tol = ATOL + RTOL * np.abs(want)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.size} off, worst {err.max():.3e}, first bad row "
                           f"{int(np.argwhere(bad)[0][0])} of {got.shape[0]}")


@pytest.mark.parametrize("d,t,n", CASES)
def test_lstm_many_tiles_per_block(dev, d, t, n):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(d * 100 + t)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p, pd = _params(d, rng, dev)
    ops.range_redo_count(reset=True)
    got = ops.lstm_fwd(torch.from_numpy(x).to(dev), pd["lstm_W"], pd["lstm_b"], 1.0)
    assert ops.range_redo_count() == 0, "ordinary data must stay on the matrix-core path (no fp32 redo of a tile)"
    _check(got, O.basic_lstm(x, p["lstm_W"], p["lstm_b"], 1.0), "lstm_fwd")


@pytest.mark.parametrize("d,t,n", CASES)
def test_ln_mhsa_mean_many_tiles_per_block(dev, d, t, n):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(d * 100 + t + 1)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p, pd = _params(d, rng, dev)
    ops.range_redo_count(reset=True)
    got = ops.ln_mhsa_mean(torch.from_numpy(x).to(dev), pd["ln_gamma"], pd["ln_beta"], pd["Wq"], pd["bq"], pd["Wk"],
                           pd["bk"], pd["Wv"], pd["bv"], 16)
    assert ops.range_redo_count() == 0, "ordinary data must stay on the matrix-core path"
    y = O.layer_norm_td(x, p["ln_gamma"], p["ln_beta"])
    want = O.mhsa(y, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], 16).mean(axis=1)
    _check(got, want, "ln_mhsa_mean")


@pytest.mark.parametrize("d,t,n", CASES)
def test_interval_fusion_many_tiles_per_block(dev, d, t, n):
    """sagnn_interval_fusion_f32 on the exchange layout: [t, n, d] storage viewed [n, t, d]."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(d * 100 + t + 2)
    xs = rng.standard_normal((t, n, d)).astype(np.float32)
    p, pd = _params(d, rng, dev)
    ops.range_redo_count(reset=True)
    got = ops.interval_fusion(torch.from_numpy(xs).to(dev).permute(1, 0, 2), pd, 16)
    assert ops.range_redo_count() == 0, "ordinary data must stay on the matrix-core path"
    _check(got, O.interval_fusion(np.ascontiguousarray(xs.transpose(1, 0, 2)), p, 16), "interval_fusion")


@pytest.mark.parametrize("d,t,n", [(64, 2, 100_003), (64, 3, 70_001), (32, 4, 100_003), (128, 4, 70_001), (64, 12, 20_011), (64, 16, 9_001)])
def test_training_forward_and_backward_many_tiles_per_block(dev, d, t, n):
    """The training forward (sagnn_lstm_fwd_train_f32 storing gates / cell + the fused LN/attention
    kernel) and the whole backward (attention-backward front and tail, LN backward, one-launch BPTT)
    at sizes where every block loops: fused output, dx and every parameter gradient against float64
    autograd over the oracle's torch restatement. d = 128 (config 3) takes the generic backward: per-step
    gate backward + one tiled-GEMM product per step, the weight gradient as two segmented products after
    the loop (dense_gemm.hip)."""
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(d + t)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p = O.init_fusion_params(d, rng)
    gout = rng.standard_normal((n, d)).astype(np.float32)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    out = O.torch_interval_fusion(tx, tp, 16)
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    pd = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in p.items()}
    from sa_gnn_amd import ops
    ops.range_redo_count(reset=True)
    got = ag.interval_fusion(xd, pd, 16)
    _check(got.detach(), out.detach().numpy(), "training forward")
    got.backward(torch.from_numpy(gout).to(dev))
    # (one chunk at most where the tail's ragged last chunk has fewer than four rows: with nothing to measure an absurd row
    # against, the kernel evaluates such a chunk in fp32 when it is a block's first)
    assert ops.range_redo_count() <= (1 if (n * t) % 32 in (1, 2, 3) else 0), "ordinary data and O(1) gradients must stay on the matrix-core path"
    for name, a, b in [("dx", xd.grad, tx.grad)] + [("d" + k, pd[k].grad, tp[k].grad) for k in p]:
        a, b = a.cpu().numpy().astype(np.float64), b.numpy()
        # parameter gradients are sums over n*t rows of O(1) terms. Some are analytically ~0 (a key
        # bias shifts every score of a row alike; only the 1e-8 in the normaliser breaks the symmetry:
        # |dbk| ~ 2e-5 here), so what the fp32 sum leaves is accumulation noise ~ eps32 * sqrt(n*t):
        # the absolute floor of test_gpu_backward (8e-6 at n*t ~ 1e3: 5e-6 held on the parametrised shapes, a random sweep met 7.7e-6 at n*t = 2220) grows with sqrt(n*t)
        floor = 8e-6 * max(1.0, np.sqrt(n * t / 1000.0))
        tol = 1e-4 * np.abs(b) + max(2e-5 * np.abs(b).max(), floor)
        bad = np.abs(a - b) > tol
        assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"


def attn_bwd_front_reference(x, p, gout, heads, dtype=torch.float64, layer_norm=True):
    """What sagnn_attn_bwd_front_f32 computes, by torch autograd in `dtype`: y = LN(x) [n, t, d] (x itself without layer
    norm) and the gradient [n*t, 3d] of sum(out * gout) at Q|K|V = y W + b, out the mean over t of the attention."""
    n, t, d = x.shape
    dk = d // heads
    tx = torch.tensor(x, dtype=dtype)
    tp = {k: torch.tensor(v, dtype=dtype) for k, v in p.items()}
    y = O.torch_layer_norm_td(tx, tp["ln_gamma"], tp["ln_beta"]) if layer_norm else tx
    qkv = torch.cat([y @ tp["Wq"] + tp["bq"], y @ tp["Wk"] + tp["bk"], y @ tp["Wv"] + tp["bv"]], dim=2).requires_grad_(True)
    q, k, v = (qkv[:, :, i * d:(i + 1) * d].reshape(n, t, heads, dk).permute(0, 2, 1, 3) for i in range(3))
    scores = torch.exp((q @ k.transpose(-1, -2)) / float(np.sqrt(dk)))      # Utils/attention.py:38-44
    attn = scores / (scores.sum(dim=-1, keepdim=True) + 1e-8)
    out = (attn @ v).permute(0, 2, 1, 3).reshape(n, t, d).mean(dim=1)
    (out * torch.tensor(gout, dtype=dtype)).sum().backward()
    return y.numpy(), qkv.grad.numpy().reshape(n * t, 3 * d)


@pytest.mark.parametrize("d,t,n", [(64, 2, 100_003), (64, 8, 70_001), (32, 3, 100_003), (128, 6, 20_011), (128, 1, 5_003),
                                   (64, 12, 20_011), (64, 16, 30_001), (32, 16, 9_001), (32, 8, 20_011), (32, 12, 5_003)])
def test_attn_bwd_front_many_tiles_per_block(dev, d, t, n):
    """sagnn_attn_bwd_front_f32 alone: y = LN(x) and dQ|dK|dV against float64 autograd (d = 128: d_k = 8, the two
    column halves of Q|K|V in separate workgroups, y stored by one of them)."""
    from sa_gnn_amd import ops
    assert ops.attn_bwd_front_supported(d, t, 16)
    rng = np.random.default_rng(d * 7 + t)
    heads = 16
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p, pd = _params(d, rng, dev)
    gout = rng.standard_normal((n, d)).astype(np.float32)
    y, want = attn_bwd_front_reference(x, p, gout, heads)
    y_got, dqkv = ops.attn_bwd_front(torch.from_numpy(x).to(dev), pd["ln_gamma"], pd["ln_beta"], pd["Wq"], pd["bq"],
                                     pd["Wk"], pd["bk"], pd["Wv"], pd["bv"], heads, torch.from_numpy(gout).to(dev))
    _check(y_got.view(n, t, d), y, "y")
    err = np.abs(dqkv.cpu().numpy() - want)
    assert (err <= 1e-4 * np.abs(want) + 2e-5 * np.abs(want).max()).all(), f"dqkv worst {err.max():.3e}"


@pytest.mark.parametrize("d,t,n", [(64, 3, 20_011), (32, 16, 9_001), (128, 6, 10_007)])
def test_split_engine_matches_f32_mfma_engine(dev, d, t, n):
    """The fusion GEMMs run on the 16-bit matrix cores over SPLIT fp32 operands: two round-to-nearest f16 pieces and
    three piece products. That is fp32-grade arithmetic, not a half-precision GEMM: against the exact-fp32 engine
    (v_mfma_f32_32x32x2_f32, an fmaf chain; sagnn_set_engine(SAGNN_ENGINE_F32); at d = 128 the VALU LSTM + f32-MFMA
    dense products) the outputs differ by a few 1e-7 on h and 1e-6 on the fused rows, and both are equally far from
    the float64 result."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(d + t)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    p, pd = _params(d, rng, dev)
    xd = torch.from_numpy(x).to(dev)
    outs = {}
    for mode in ("f16x2", "f32"):
        with ops.engine(mode):
            h = ops.lstm_fwd(xd, pd["lstm_W"], pd["lstm_b"], 1.0)
            f = ops.ln_mhsa_mean(h, pd["ln_gamma"], pd["ln_beta"], pd["Wq"], pd["bq"], pd["Wk"], pd["bk"], pd["Wv"], pd["bv"], 16)
        outs[mode] = (h.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.float64))
    assert ops.get_engine() == "f16x2"
    x64 = x.astype(np.float64)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    h64 = O.basic_lstm(x64, p64["lstm_W"], p64["lstm_b"], 1.0)
    f64 = O.mhsa(O.layer_norm_td(h64, p64["ln_gamma"], p64["ln_beta"]), p64["Wq"], p64["bq"], p64["Wk"], p64["bk"], p64["Wv"],
                 p64["bv"], 16).mean(axis=1)
    e_f32 = max(np.abs(outs["f32"][0] - h64).max(), np.abs(outs["f32"][1] - f64).max())
    assert np.abs(outs["f16x2"][0] - outs["f32"][0]).max() <= 5e-6
    assert np.abs(outs["f16x2"][1] - outs["f32"][1]).max() <= 2e-5
    e_split = max(np.abs(outs["f16x2"][0] - h64).max(), np.abs(outs["f16x2"][1] - f64).max())
    assert e_split <= 2e-5 and e_split <= 3 * e_f32 + 1e-6, (e_split, e_f32)


@pytest.mark.parametrize("d,t,n", [(64, 3, 1_000), (32, 4, 777), (64, 2, 40_003), (128, 3, 700)])
def test_lstm_inputs_beyond_the_f16_range(dev, d, t, n):
    """The f16 pieces of the default LSTM engine hold |v| <= 65504. A workgroup that meets a larger x (here 1e6 and
    3e38 in a few rows, next to ordinary and to tiny rows) re-evaluates its 96-row tile with fp32 fmaf chains
    (lstm_f16_kernel.h): every row — the huge ones, their tile neighbours and the untouched tiles — must still match the
    oracle, as TF's fp32 MatMul would."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(5 * d + t)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    x[5, 0, 3] = 1e6
    x[5, t - 1, :] = -2e5
    x[n // 2, 1, 7] = 3e38
    x[n - 1, 0, :] *= 1e5
    x[7] *= 1e-7                                   # denormal heads: the residual piece carries the value
    x[200 % n, :, :] *= 1e-30
    p, pd = _params(d, rng, dev)
    ops.range_redo_count(reset=True)
    got = ops.lstm_fwd(torch.from_numpy(x).to(dev), pd["lstm_W"], pd["lstm_b"], 1.0)
    assert ops.range_redo_count() >= 4                      # the tiles that hold those rows went through the fp32 pass
    want = O.basic_lstm(x.astype(np.float64), p["lstm_W"].astype(np.float64), p["lstm_b"].astype(np.float64), 1.0)
    assert np.isfinite(got.cpu().numpy()).all()
    _check(got, want.astype(np.float32), "lstm_fwd beyond the f16 range")


@pytest.mark.parametrize("d,t,n", [(64, 16, 300), (32, 3, 1_000), (128, 6, 500), (64, 2, 20_001)])
def test_attention_operands_beyond_the_f16_range(dev, d, t, n):
    """The attention products run on f16 pieces as well. A layer-norm gain of 4e4 puts y beyond 65504 in most
    tiles (every workgroup then rebuilds its Q|K|V records with fp32 fmaf chains); with the projections scaled down
    by the same factor the scores stay ordinary, so the result is checked against the oracle at full accuracy."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(3 * d + t)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    x[n // 3] *= 30.0                                # a spiky node: its normalised rows reach |y| ~ 1e5
    p = O.init_fusion_params(d, rng)
    p["ln_gamma"] = (p["ln_gamma"] * 4e4).astype(np.float32)
    for k in ("Wq", "Wk", "Wv"):
        p[k] = (p[k] * 2.5e-5).astype(np.float32)
    pd = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    got = ops.ln_mhsa_mean(torch.from_numpy(x).to(dev), pd["ln_gamma"], pd["ln_beta"], pd["Wq"], pd["bq"], pd["Wk"],
                           pd["bk"], pd["Wv"], pd["bv"], 16)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    y = O.layer_norm_td(x.astype(np.float64), p64["ln_gamma"], p64["ln_beta"])
    assert np.abs(y).max() > 65504
    want = O.mhsa(y, p64["Wq"], p64["bq"], p64["Wk"], p64["bk"], p64["Wv"], p64["bv"], 16).mean(axis=1)
    _check(got, want.astype(np.float32), "ln_mhsa_mean beyond the f16 range")


def test_lstm_training_forward_beyond_the_f16_range(dev):
    """Same for the training forward (stores gate activations and cell states) and for a continued state."""
    from sa_gnn_amd import ops
    d, t, n = 64, 3, 500
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, t, d)).astype(np.float32)
    x[100, 1, 5] = 7e4
    p, pd = _params(d, rng, dev)
    xd = torch.from_numpy(x).to(dev)
    h, gates, cell = ops.lstm_fwd_train(xd, pd["lstm_W"], pd["lstm_b"])
    # the stored activations (sigmoid(i), tanh(j), sigmoid(f + 1), sigmoid(o)) and cell states, float64, as O.basic_lstm steps
    x64, W64, b64 = x.astype(np.float64), p["lstm_W"].astype(np.float64), p["lstm_b"].astype(np.float64)
    hh, cc = np.zeros((n, d)), np.zeros((n, d))
    want_g, want_c = np.zeros((n, t, 4 * d)), np.zeros((n, t, d))
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    for ts in range(t):
        gi, gj, gf, go = np.split(np.concatenate([x64[:, ts], hh], axis=1) @ W64 + b64, 4, axis=1)
        act = [sig(gi), np.tanh(gj), sig(gf + 1.0), sig(go)]
        cc = cc * act[2] + act[0] * act[1]
        hh = np.tanh(cc) * act[3]
        want_g[:, ts], want_c[:, ts] = np.concatenate(act, axis=1), cc
    _check(h, O.basic_lstm(x64, W64, b64, 1.0).astype(np.float32), "h")
    _check(gates, want_g.astype(np.float32), "gates")
    _check(cell, want_c.astype(np.float32), "cell")
