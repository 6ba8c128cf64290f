"""GPU suite of --fusion_rows batch: the row compaction (sagnn_rows_mark_i32 / _mark_seg_i32 / _compact_i32) against
np.unique, gather / scatter against torch indexing, interval_fusion_rows against interval_fusion on the same slab,
train_loss in batch mode against all mode and the float64 oracle, and whole epochs in batch mode."""
import numpy as np
import pytest
import torch

import fusion_rows_ref as R

pytestmark = pytest.mark.gpu

TOL_REL, TOL_MAX, TOL_ABS = 2e-4, 5e-5, 2e-5        # test_training_objective_gradients' tolerance formula


def _close(a, b, name):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    tol = TOL_REL * np.abs(b) + max(TOL_MAX * np.abs(b).max(), TOL_ABS)
    bad = np.abs(a - b) > tol
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"


def _compact(dev, N, id_lists, cap):
    from sa_gnn_amd import ops
    flags = torch.zeros(N, dtype=torch.uint8, device=dev)
    for ids in id_lists:
        ops.rows_mark(torch.as_tensor(np.asarray(ids, dtype=np.int32)).to(dev), flags)
    rows, count = ops.rows_compact(flags, cap)
    return rows, count, flags


@pytest.mark.parametrize("N,lists,cap", [
    (1000, [[5, 5, 5, 999, 0, 17, 17], [17, 3]], 12),                   # duplicates, both ends of the table
    (1000, [[], []], 7),                                                 # no ids: count 0
    (4097, [np.arange(4097)[::-1], np.arange(0, 4097, 3)], 4097),        # every row touched: count = N = cap
    (5003, [np.random.default_rng(0).integers(0, 5003, 2000)], 2000),   # N not a multiple of the tile
    (4_500_000, [np.random.default_rng(1).integers(0, 4_500_000, 300_000), np.arange(4_400_000, 4_500_000, 7)],
     400_000),                                                           # many workgroups (1099 tiles)
])
def test_compaction_equals_np_unique(dev, N, lists, cap):
    rows, count, flags = _compact(dev, N, lists, cap)
    want = np.unique(np.concatenate([np.asarray(v, dtype=np.int64) for v in lists])) if any(len(v) for v in lists) \
        else np.zeros(0, np.int64)
    assert count.is_cuda and count.dtype == torch.int32 and count.numel() == 1
    n = int(count.item())
    got = rows.cpu().numpy().astype(np.int64)
    assert n == len(want)
    assert got[:n].tolist() == want.tolist()                             # ascending
    assert ((got[n:] >= 0) & (got[n:] < N)).all()                        # padding: valid ids
    assert int(flags.sum()) == 0                                         # the flags were cleared as they were read
    # the cleared buffer serves the next compaction as it is
    from sa_gnn_amd import ops
    ops.rows_mark(torch.tensor([N - 1, 0], dtype=torch.int32, device=dev), flags)
    rows2, count2 = ops.rows_compact(flags, min(cap, N) if N > 1 else 1)
    assert int(count2.item()) == 2 and rows2[:2].tolist() == [0, N - 1]


def test_marking_segments_equals_marking_the_flat_items(dev):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(3)
    N, P, B, n_flat = 3000, 12, 64, 2000
    flat = rng.integers(0, N, n_flat).astype(np.int32)
    seg_len = np.concatenate([[0, P, P + 5], rng.integers(0, P + 1, B - 3)]).astype(np.int32)   # one longer than P
    seg_begin = rng.integers(0, n_flat - P - 5, B).astype(np.int64)
    flags = torch.zeros(N, dtype=torch.uint8, device=dev)
    ops.rows_mark_segments(*(torch.from_numpy(a).to(dev) for a in (flat, seg_begin, seg_len)), P, flags)
    rows, count = ops.rows_compact(flags, N)
    items = R.segment_items(flat, seg_begin, seg_len, P)
    flat_rows, flat_count, _ = _compact(dev, N, [items], N)
    n = int(count.item())
    assert n == int(flat_count.item()) == len(np.unique(items))
    assert torch.equal(rows[:n], flat_rows[:n])


def test_gather_and_scatter_are_exact(dev):
    from sa_gnn_amd import ops
    rng = np.random.default_rng(4)
    T, N, d = 3, 777, 64
    slab = torch.from_numpy(rng.standard_normal((T, N, d)).astype(np.float32)).to(dev)
    x = slab.permute(1, 0, 2)                                            # [N, T, d] view: node stride d, interval N d
    ids = np.unique(rng.integers(0, N, 200))
    rows, count, _ = _compact(dev, N, [ids], 256)
    n = len(ids)
    r = rows[:n].long()
    g = ops.rows_gather(x, rows)
    assert g.shape == (256, T, d) and torch.equal(g[:n], x[r])
    mask = (torch.rand((N, T, d), device=dev) < 0.5).float() * 2           # full-size dropout rows, dense [N, T, d]
    assert torch.equal(ops.rows_gather(mask, rows)[:n], mask[r])
    y = torch.from_numpy(rng.standard_normal((N, d)).astype(np.float32)).to(dev)
    gy = ops.rows_gather(y, rows, count)
    assert torch.equal(gy[:n], y[r]) and int(torch.count_nonzero(gy[n:])) == 0   # padding slots are zeros
    src = torch.from_numpy(rng.standard_normal((256, d)).astype(np.float32)).to(dev)
    out = ops.rows_scatter(src, rows, count, torch.zeros((N, d), device=dev))
    want = torch.zeros((N, d), device=dev)
    want[r] = src[:n]
    assert torch.equal(out, want)                                        # untouched rows exactly zero
    src3 = torch.from_numpy(rng.standard_normal((256, T, d)).astype(np.float32)).to(dev)
    dx = torch.zeros((T, N, d), device=dev).permute(1, 0, 2)
    ops.rows_scatter(src3, rows, count, dx)
    want3 = torch.zeros((N, T, d), device=dev)
    want3[r] = src3[:n]
    assert torch.equal(dx, want3)


def _fusion_params(dev, d, seed):
    from sa_gnn_amd.model import random_fusion_params
    return {k: v.requires_grad_(True) for k, v in random_fusion_params(d, dev, seed).items()}


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("T", [2, 3, 4, 8])
def test_interval_fusion_rows_against_interval_fusion(dev, d, T):
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(10 * d + T)
    N, heads = 700, 16
    slab = torch.from_numpy(rng.standard_normal((T, N, d)).astype(np.float32)).to(dev).requires_grad_(True)
    ids = np.unique(rng.integers(0, N, 180))
    n = len(ids)
    rows, count, _ = _compact(dev, N, [ids], 256)
    drop = ((torch.rand((N, T, d), device=dev) < 0.5).float() * 2)
    g_np = rng.standard_normal((N, d)).astype(np.float32)
    untouched = np.setdiff1d(np.arange(N), ids)
    g_np[untouched] = 0.0                                               # the loss reads the touched rows only
    g = torch.from_numpy(g_np).to(dev)
    p = _fusion_params(dev, d, 5)
    grads = []
    outs = []
    for mode in ("all", "batch"):
        for v in list(p.values()) + [slab]:
            v.grad = None
        x = slab.permute(1, 0, 2)
        out = ag.interval_fusion(x, p, heads, drop_scale=drop) if mode == "all" else \
            ag.interval_fusion_rows(x, rows, count, n, p, heads, drop_scale=drop)
        (out * g).sum().backward()
        outs.append(out.detach())
        grads.append({k: v.grad.detach().clone() for k, v in p.items()} | {"x": slab.grad.detach().clone()})
    (ga, gb), r = grads, torch.from_numpy(ids).to(dev)
    assert torch.equal(outs[1][r], outs[0][r])                          # touched rows: bit-identical
    assert int(torch.count_nonzero(outs[1][torch.from_numpy(untouched).to(dev)])) == 0
    for k in p:
        _close(gb[k], ga[k], k)
    dxa, dxb = ga["x"].permute(1, 0, 2), gb["x"].permute(1, 0, 2)       # [N, T, d]
    _close(dxb[r], dxa[r], "dx")
    assert int(torch.count_nonzero(dxb[torch.from_numpy(untouched).to(dev)])) == 0


def test_empty_row_set_gives_zeros(dev):
    from sa_gnn_amd import autograd as ag
    rng = np.random.default_rng(6)
    T, N, d = 3, 300, 64
    slab = torch.from_numpy(rng.standard_normal((T, N, d)).astype(np.float32)).to(dev).requires_grad_(True)
    rows, count, _ = _compact(dev, N, [[]], 4)
    assert int(count.item()) == 0
    p = _fusion_params(dev, d, 2)
    for cap in (1, 0):
        for v in list(p.values()) + [slab]:
            v.grad = None
        out = ag.interval_fusion_rows(slab.permute(1, 0, 2), rows, count, cap, p, 16)
        assert int(torch.count_nonzero(out)) == 0
        (out * torch.ones_like(out)).sum().backward()
        assert int(torch.count_nonzero(slab.grad)) == 0
        for k, v in p.items():
            assert v.grad is not None and int(torch.count_nonzero(v.grad)) == 0, k


def _both_modes(rec, NNs, args, batch, keep_rate):
    params = {k: p for k, p in NNs.params.items() if p.requires_grad}
    res = {}
    for mode in ("all", "batch"):
        args.fusion_rows = mode
        try:
            for p in params.values():
                p.grad = None
            pre, ssl = rec.train_loss(batch, keep_rate=keep_rate)
            (pre + args.ssl_reg * ssl).backward()
        finally:
            args.fusion_rows = "all"
        res[mode] = (float(pre.detach()), float(ssl.detach()),
                     {k: None if p.grad is None else p.grad.detach().clone() for k, p in params.items()})
    return res


def _check_against(got, want, leaves_or_grads, name):
    for k, w in leaves_or_grads.items():
        g = got[k]
        if w is None:
            assert g is None or float(g.abs().max()) == 0.0, (name, k)
            continue
        assert g is not None, (name, k)
        a, b = g.cpu().double().numpy(), w.cpu().double().numpy()
        floor = max(TOL_MAX * np.abs(b).max(), TOL_ABS)
        if k.endswith("k_bias"):       # analytically ~0: the noise of terms as large as the key kernel's gradient
            floor = max(floor, 1e-3 * float(leaves_or_grads[k.replace("k_bias", "k_kernel")].abs().max()))
        bad = np.abs(a - b) > TOL_REL * np.abs(b) + floor
        assert not bad.any(), f"{name} {k}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e}"


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_train_loss_batch_rows_against_all_rows_and_the_oracle(dev, sampler):
    from oracle import selfgnn_oracle as O
    from test_gpu_device_sampler import _host_form
    from test_gpu_train import _oracle_params, _setup
    rec, handler, NNs, args = _setup(dev, 64, 48, 2)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    if sampler == "host":
        b = rec._host_train_batch(bat)
        g = torch.Generator(device="cpu").manual_seed(4)
        for key, n in (("drop_u", args.user), ("drop_i", args.item)):
            b[key] = ((torch.rand((n, args.graphNum, args.latdim), generator=g) < 0.5).float() * 2.0).to(dev)
        keep, ob = None, dict(b, drop_u=b["drop_u"].cpu().double(), drop_i=b["drop_i"].cpu().double())
        lst = lambda v: np.asarray(v).tolist()   # noqa: E731
        ob = dict(ob, uids=lst(ob["uids"]), iids=lst(ob["iids"]), uLocs_seq=lst(ob["uLocs_seq"]),
                  suids=[lst(v) for v in ob["suids"]], siids=[lst(v) for v in ob["siids"]])
    else:
        b = rec.sample_batch_device(bat, 2024, 1)
        keep, ob = 1.0, _host_form(rec, b, args)
    res = _both_modes(rec, NNs, args, b, keep)
    (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
    # the touched rows are the numpy reference's
    users, items, _ = R.touched_rows(b, args.user, args.item, args.pos_length, rec._device_sampler().seq_items
                                     if sampler == "device" else None)
    assert rec.fusion_rows_counts == (len(users), len(items))
    assert len(items) < args.item or len(users) < args.user
    # the hinge sums use float atomics: equal up to the order of that sum
    assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
    _check_against(gb, ga, ga, "batch vs all")
    # the float64 oracle on the same batch and masks
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, ob, {"T": 2, "L": 2, "leaky": 0.5, "heads": 16})
    (opre + args.ssl_reg * ossl).backward()
    opre, ossl = float(opre.detach()), float(ossl.detach())
    assert abs(pb - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(sb - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    _check_against(gb, {k: leaves[k].grad for k in leaves}, {k: leaves[k].grad for k in leaves}, "batch vs oracle")


def _epochs(dev, sampler, n):
    from test_gpu_train import _setup
    np.random.seed(0)
    torch.manual_seed(0)
    rec, handler, NNs, args = _setup(dev, 64, 32, 1)
    args.trnNum, args.lr, args.keepRate, args.ssl_reg, args.reg = 64, 5e-3, 0.5, 1e-3, 1e-4
    args.decay_step = args.trnNum // args.batch
    np.random.seed(0)
    torch.manual_seed(0)
    args.sampler, args.fusion_rows = sampler, "batch"
    try:
        losses, counts = [], []
        for _ in range(n):
            losses.append(rec.trainEpoch()["preLoss"])
            counts.append(rec.fusion_rows_counts)                       # the last step's touched users / items
    finally:
        args.sampler, args.fusion_rows = "host", "all"
    return losses, counts, {k: p.detach().clone() for k, p in NNs.params.items()}


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_train_epochs_in_batch_mode(dev, sampler):
    losses, counts, _ = _epochs(dev, sampler, 8)
    assert all(np.isfinite(losses)) and min(losses[-3:]) < losses[0] and np.mean(losses[-3:]) < np.mean(losses[:3])
    # the same seeds again: the same batches, touched rows and dropout masks. The loss and weight-gradient sums use
    # float atomics (see test_checkpoint_round_trip_resumes_identically), and Adam turns the last-bit noise of
    # gradients that are analytically ~0 into steps of +-lr, which keepRate 0.5 training then amplifies from epoch to
    # epoch: the first epochs agree to that noise, not bit for bit
    losses2, counts2, _ = _epochs(dev, sampler, 2)
    assert counts2 == counts[:2]
    np.testing.assert_allclose(losses2, losses[:2], rtol=1e-4)
