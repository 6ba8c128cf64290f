"""GPU suite of the popularity-weighted candidate softmax (--softmaxNegDist pop): the weighted draw
against its restatement (softmax_pop_ref.draw), sagnn_softmax_loss_f32's offset mode and its backward against float64 over lists
with repeated ids, the contracts (dead rows, row independence, bit-identical runs, the zero-offset case against the
entries without an offset), then the flag inside the Recommender.

Tolerances: softmax_loss_ref.tolerance_terms' bounds with A[b] taken over |z| + |bias| (softmax_pop_ref.tolerance_terms)
and the constants of test_gpu_softmax_negs.py (K_LSE 16, K_DQ 32, K_DI 32). The offset adds one float32 add per logit,
of a term that A now counts. The device dI is assembled in float64 from the live dIc rows and dT."""
import numpy as np
import pytest
import torch

import softmax_cand_ref as C
import softmax_loss_ref as R
import softmax_pop_ref as P
from oracle import selfgnn_oracle as O
from test_gpu_softmax_loss import (CFG, K_DI, K_DQ, K_LSE, _grad_close, _host_batch, _lists, _loss_and_grads, _oracle_params,
                                   _setup, _t)
from test_gpu_softmax_negs import _excl

pytestmark = pytest.mark.gpu


def _cum(n_items, a=0.75, seed=5, hub=None, cap=50_000):
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.zipf(1.3, n_items), cap).astype(np.int64)
    if hub is not None:
        deg[hub[0]] = hub[1]
    return P.weights(deg, a)


def _draw_dev(dev, cum, W, n_cand, seed, step):
    from sa_gnn_amd import ops
    cand, bias = ops.sample_strata_weighted(_t(dev, np.asarray(cum, dtype=np.int64), np.int64), W, n_cand, seed, step)
    assert cand.dtype == torch.int32 and bias.dtype == torch.float32 and cand.shape == bias.shape == (n_cand,)
    return cand, bias


def _ulps(a, b):
    """Distance in float32 units in the last place between finite arrays (0 for equal values, -0.0 == 0.0)."""
    ia, ib = (np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(v < 0, -(v & 0x7FFFFFFF), v) for v in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("n_items,n_cand", [(1, 1), (17, 5), (700, 300), (4099, 64), (300, 300)])
def test_device_draw_equals_the_restatement(dev, n_items, n_cand):
    w, cum, W = _cum(n_items, hub=(n_items // 3, 200_000))
    for seed, step in ((0, 0), (0x9E3779B97F4A7C15, 3), (2 ** 64 - 1, 2 ** 32 - 1)):
        cand, bias = (v.cpu().numpy() for v in _draw_dev(dev, cum, W, n_cand, seed, step))
        rc, m, live, rb = P.draw(cum, n_cand, seed, step)
        assert cand.tolist() == rc.tolist(), (seed, step)
        assert np.array_equal(np.isneginf(bias), ~live) and np.isfinite(bias[live]).all(), (seed, step)
        u = _ulps(bias[live], rb[live])
        print(f"({n_items}, {n_cand}) seed {seed} step {step}: {int(live.sum())} live, longest run {int(m.max())}, worst bias ulp {int(u.max())}")
        assert (u <= 2).all()
        assert np.array_equal(bias[live][rb[live] == 0.0], rb[live][rb[live] == 0.0]) and not np.signbit(bias[live][rb[live] == 0.0]).any()
    assert all(v.shape == (0,) for v in _draw_dev(dev, cum, W, 0, 1, 1))


@pytest.mark.parametrize("n", [1, 300, 4099])
def test_equal_weights_and_every_item_give_the_identity_and_zero_biases_on_the_device(dev, n):
    w, cum, W = P.weights([2] * n, 0.75)
    cand, bias = _draw_dev(dev, cum, W, n, 99, 4)
    assert cand.cpu().tolist() == list(range(n))
    assert not bias.cpu().numpy().view(np.int32).any()                 # +0.0, every bit


def _run(dev, Q, I, cand, bias, target, inv_temp, scale, ptr=None, items=None, rows=None, g=1.0):
    from sa_gnn_amd import ops
    Qd = Q if isinstance(Q, torch.Tensor) else _t(dev, Q, np.float32)
    Id, tg, cd, bd = _t(dev, I, np.float32), _t(dev, target, np.int32), _t(dev, cand, np.int32), _t(dev, bias, np.float32)
    excl, rd = _excl(dev, ptr, items), None if rows is None else _t(dev, rows, np.int32)
    loss, lse, ts = ops.softmax_loss_cand(Qd, Id, cd, tg, inv_temp, scale, excl, rd, bias=bd)
    gd = torch.full((1,), g, dtype=torch.float32, device=dev)
    dQ, dIc, dT = ops.softmax_loss_cand_bwd(Qd, Id, cd, tg, lse, gd, inv_temp, scale, excl, rd, bias=bd)
    torch.cuda.synchronize()
    assert dIc.shape == (len(cand), I.shape[1]) and dT.shape == dQ.shape == (len(target), I.shape[1])
    out = {"loss": float(loss), "lse": lse.cpu().numpy(), "tscore": ts.cpu().numpy(), "dQ": dQ.cpu().numpy(),
           "dIc": dIc.cpu().numpy(), "dT": dT.cpu().numpy()}
    out["dI"] = P.assemble_dI(len(I), cand, bias, out["dIc"], target, out["dT"])
    return out


def _check(got, Q, I, cand, bias, target, inv_temp, scale, ptr=None, items=None, rows=None, name="", g=1.0):
    """Every output against float64 under the derived bounds; prints the K each output needs before it asserts."""
    ref = P.softmax_loss_pop_np(Q, I, cand, bias, target, inv_temp, scale, ptr, items, rows)
    terms = P.tolerance_terms(Q, I, target, ref, inv_temp, scale)
    need = {k: R.worst_ratio(got[k] / (g if k in ("dQ", "dI") else 1.0), ref[k], *terms[k]) for k in ("lse", "dQ", "dI")}
    plain = R.tolerance_terms(Q, I, target, ref, inv_temp, scale)      # the target's score takes no offset
    need["tscore"] = R.worst_ratio(got["tscore"], ref["tscore"], plain["lse"][0] / inv_temp, 0.0)
    loss_tol = abs(scale) * (2 * K_LSE * terms["lse"][0]).sum() + 4 * R.EPS32 * abs(ref["loss"])
    print(f"{name}: K needed lse {need['lse']:.2f} / {K_LSE}, tscore {need['tscore']:.2f} / {K_LSE}, dQ {need['dQ']:.2f} / {K_DQ}, "
          f"dI {need['dI']:.2f} / {K_DI}; loss {got['loss']!r} vs {ref['loss']!r} (tol {loss_tol:.3e})")
    for k in ("lse", "tscore", "dQ", "dIc", "dT"):
        assert np.isfinite(got[k]).all(), f"{name}: {k} holds inf or NaN"
    assert need["lse"] <= K_LSE and need["tscore"] <= K_LSE and need["dQ"] <= K_DQ and need["dI"] <= K_DI, (name, need)
    assert np.isfinite(got["loss"]) and abs(got["loss"] - ref["loss"]) <= loss_tol, name
    dead = ~np.isfinite(np.asarray(bias, dtype=np.float64))
    assert not got["dIc"][dead].any(), f"{name}: a dead position has a dIc row"
    tgt = np.asarray(target, dtype=np.int64)
    assert not got["dT"][~((tgt >= 0) & (tgt < len(I)))].any(), f"{name}: a skipped row has a dT row"
    return ref, terms


def _case(seed, ni, nq, d):
    rng = np.random.default_rng(seed)
    return rng, (rng.standard_normal((nq, d)) * 0.7).astype(np.float32), (rng.standard_normal((ni, d)) * 0.7).astype(np.float32)


def _hit_lists(rng, nq, ni, cand, n_lists=None):
    """_lists plus five candidate ids on every list, so that the lists hit candidates and not only 2 % at random."""
    ptr, items = _lists(rng, nq, ni, n_lists)
    lists = [items[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]
    lists = [np.sort(np.concatenate([v, cand[rng.integers(0, len(cand), min(len(cand), 5))]])) for v in lists]
    return np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64), np.concatenate(lists)


@pytest.mark.parametrize("temp", [1.0, 0.25])
@pytest.mark.parametrize("nq", [1, 17, 33, 40])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_forward_and_both_gradients_against_float64(dev, d, nq, temp):
    ni = 700
    rng, Q, I = _case(1000 * d + nq, ni, nq, d)
    w, cum, W = _cum(ni, hub=(300, 200_000), cap=5000)
    by_row = temp != 1.0
    scale, g = 1.0 / nq, 0.5
    for n_cand in (5, 130, 300):                                   # one tile; across the first chunk boundary; three chunks
        cand, m, live, bias = P.draw(cum, n_cand, 31 + d, nq)
        target = rng.integers(0, ni, nq)
        target[::2] = cand[rng.integers(0, n_cand, len(target[::2]))]          # every other row's target is a candidate
        ptr, items = _hit_lists(rng, nq, ni, cand, nq + 3 if by_row else None)
        rows = rng.integers(0, nq + 3, nq) if by_row else None
        got = _run(dev, Q, I, cand, bias, target, 1.0 / temp, scale, ptr, items, rows, g=g)
        _check(got, Q, I, cand, bias, target, 1.0 / temp, scale, ptr, items, rows,
               name=f"d {d} nq {nq} temp {temp} n_cand {n_cand} (longest run {int(m.max())})", g=g)


def _duplicate_case():
    """700 items, 300 candidates, a hub at id 300 whose run crosses position 128 (the first chunk boundary) and three
    multiples of 16 (tile boundaries), and a run of length 2 across a multiple of 16. Asserted on the restatement."""
    w, cum, W = _cum(700, seed=1300, hub=(300, 200_000), cap=5000)
    cand, m, live, bias = P.draw(cum, 300, 77, 3)
    lb = int(np.flatnonzero(cand == 300)[0])
    ub = lb + int(m[lb])
    assert 40 <= 300 * w[300] / W <= 80 and lb < 128 < ub - 1 and sum(1 for k in range(lb + 1, ub) if k % 16 == 0) >= 3, (lb, ub)
    short = [int(p) for p in np.flatnonzero(live & (m == 2)) if (p + 1) % 16 == 0]
    assert short, "no run of length 2 across a tile boundary"
    return cum, W, cand, m, live, bias, 300, int(cand[short[0]])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_runs_across_tile_and_chunk_boundaries(dev, d):
    cum, W, cand, m, live, bias, hub, short = _duplicate_case()
    ni, nq = 700, 21
    rng, Q, I = _case(500 + d, ni, nq, d)
    got_cand, got_bias = _draw_dev(dev, cum, W, 300, 77, 3)            # the device's own list and offsets go in
    assert got_cand.cpu().tolist() == cand.tolist()
    bias_dev = got_bias.cpu().numpy()
    assert np.array_equal(np.isneginf(bias_dev), ~live)
    target = rng.integers(0, ni, nq)
    outside = [k for k in range(ni) if k not in cand]
    target[[0, 2, 4]] = outside[:3]
    lists = [np.sort(rng.integers(0, ni, 14)) for _ in range(nq)]
    lists[0] = np.sort(np.concatenate([lists[0], [hub]]))              # the hub on the row's list
    target[1] = hub                                                    # the hub the row's target
    lists[1] = lists[1][lists[1] != hub]
    lists[2] = lists[2][lists[2] != hub]                               # the hub a plain candidate of the row
    target[3] = hub                                                    # on the list and the target
    lists[3] = np.sort(np.concatenate([lists[3], [hub, hub]]))
    lists[4] = np.sort(np.concatenate([lists[4], [short]]))            # the short run likewise
    target[5] = target[6] = short
    lists[6] = np.sort(np.concatenate([lists[6], [short]]))
    lists[7] = np.unique(cand)                                         # every live candidate listed: only the target is left
    target[7] = outside[3]
    lists[8] = np.arange(ni)                                           # ... with the target a candidate on its own list
    target[8] = hub
    target[9] = -1
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    items = np.concatenate(lists)
    scale = 1.0 / nq
    got = _run(dev, Q, I, cand, bias_dev, target, 1.0, scale, ptr, items)
    ref, terms = _check(got, Q, I, cand, bias_dev, target, 1.0, scale, ptr, items, name=f"duplicates d {d}")
    assert not ref["eligible"][0, hub] and not ref["eligible"][4, short]
    for b, c in ((1, hub), (3, hub), (5, short), (6, short)):          # a target: eligible, no offset
        assert ref["eligible"][b, c] and ref["off"][b, c] == 0.0
    assert ref["eligible"][2, hub] and ref["off"][2, hub] == bias_dev[np.flatnonzero(cand == hub)[0]] != 0.0
    for b in (7, 8):                                                   # p(target) = 1: no loss, no gradient, to the tolerance
        assert ref["eligible"][b].sum() == 1
        assert abs(got["lse"][b] - got["tscore"][b]) <= 2 * K_LSE * terms["lse"][0][b]
        assert (np.abs(got["dQ"][b]) <= K_DQ * terms["dQ"][0][b] + terms["dQ"][1][b]).all()
    for k in ("lse", "tscore", "dQ", "dT"):
        assert not got[k][9].any(), k
    # the hub's live row collects every row that holds it; the rest of its run nothing
    j = int(np.flatnonzero(cand == hub)[0])
    assert got["dIc"][j].any() and not got["dIc"][j + 1:j + int(m[j])].any()


def test_no_candidates_and_rows_without_a_target(dev):
    ni, nq, d = 700, 40, 32
    rng, Q, I = _case(10, ni, nq, d)
    target = rng.integers(0, ni, nq)
    ptr, items = _lists(rng, nq, ni)
    none = np.zeros(0, np.int64), np.zeros(0, np.float32)
    got = _run(dev, Q, I, *none, target, 2.0, 1.0 / nq, ptr, items)
    _check(got, Q, I, *none, target, 2.0, 1.0 / nq, ptr, items, name="n_cand 0")
    assert np.array_equal(got["lse"], got["tscore"] * np.float32(2.0)) and got["loss"] == 0.0
    assert not got["dQ"].any() and not got["dT"].any() and got["dIc"].shape == (0, d)
    w, cum, W = _cum(ni, hub=(300, 200_000), cap=5000)
    cand, m, live, bias = P.draw(cum, 130, 4, 0)
    skipped = np.array([0, 5, 15, 16, 17, 39])
    target[skipped] = -1
    got = _run(dev, Q, I, cand, bias, target, 1.0, 1.0 / nq, ptr, items)
    _check(got, Q, I, cand, bias, target, 1.0, 1.0 / nq, ptr, items, name="some rows skipped")
    for k in ("lse", "tscore", "dQ", "dT"):
        assert not got[k][skipped].any(), k
    target[:] = ni                                                     # every row skipped
    got = _run(dev, Q, I, cand, bias, target, 1.0, 1.0 / nq, ptr, items)
    assert got["loss"] == 0.0 and not got["dIc"].any() and not got["dI"].any() and not got["dQ"].any()


@pytest.mark.parametrize("d", [32, 64, 128])
def test_zero_offsets_give_the_bits_of_the_entries_without_an_offset(dev, d):
    """Equal weights and n_cand == n_items: the drawn list is arange and every bias +0.0; loss, lse, dQ, dIc and dT are
    those of ops.softmax_loss_cand on arange, bit for bit."""
    from sa_gnn_amd import ops
    ni, nq = 333, 40
    rng, Q, I = _case(300 + d, ni, nq, d)
    w, cum, W = P.weights([1] * ni, 0.75)
    cand, bias = _draw_dev(dev, cum, W, ni, 5, 2)
    assert cand.cpu().tolist() == list(range(ni)) and not bias.cpu().numpy().view(np.int32).any()
    target = rng.integers(0, ni, nq)
    target[3] = -1
    ptr, items = _lists(rng, nq, ni)
    Qd, Id, tg, excl = _t(dev, Q, np.float32), _t(dev, I, np.float32), _t(dev, target, np.int32), _excl(dev, ptr, items)
    g = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    for temp in (1.0, 0.3):
        a = ops.softmax_loss_cand(Qd, Id, cand, tg, 1.0 / temp, 1.0 / nq, excl, None)
        b = ops.softmax_loss_cand(Qd, Id, cand, tg, 1.0 / temp, 1.0 / nq, excl, None, bias=bias)
        ga = ops.softmax_loss_cand_bwd(Qd, Id, cand, tg, a[1], g, 1.0 / temp, 1.0 / nq, excl, None)
        gb = ops.softmax_loss_cand_bwd(Qd, Id, cand, tg, b[1], g, 1.0 / temp, 1.0 / nq, excl, None, bias=bias)
        for name, x, y in zip(("loss", "lse", "tscore", "dQ", "dIc", "dT"), a + ga, b + gb):
            assert torch.equal(x, y), (name, temp)


def test_a_rows_outputs_do_not_depend_on_the_batch(dev):
    from sa_gnn_amd import ops
    cum, W, cand, m, live, bias, hub, short = _duplicate_case()
    ni, nq, d = 700, 70, 64
    rng, Q, I = _case(11, ni, nq, d)
    target = rng.integers(0, ni, nq)
    target[::3] = cand[rng.integers(0, len(cand), len(target[::3]))]
    ptr, items = _hit_lists(rng, nq, ni, cand)
    rows = rng.permutation(nq)
    Id, tg, rd, cd, bd = (_t(dev, I, np.float32), _t(dev, target, np.int32), _t(dev, rows, np.int32), _t(dev, cand, np.int32),
                          _t(dev, bias, np.float32))
    excl, Qd = _excl(dev, ptr, items), _t(dev, Q, np.float32)
    g = torch.ones(1, dtype=torch.float32, device=dev)
    _, lse, ts = ops.softmax_loss_cand(Qd, Id, cd, tg, 1.0, 0.5, excl, rd, bias=bd)
    dQ, _, dT = ops.softmax_loss_cand_bwd(Qd, Id, cd, tg, lse, g, 1.0, 0.5, excl, rd, bias=bd)
    for b in (0, 15, 16, 23, 33, 64, 69):
        q1, t1, r1 = _t(dev, Q[b:b + 1], np.float32), tg[b:b + 1].contiguous(), rd[b:b + 1].contiguous()
        _, lse1, ts1 = ops.softmax_loss_cand(q1, Id, cd, t1, 1.0, 0.5, excl, r1, bias=bd)
        dQ1, _, dT1 = ops.softmax_loss_cand_bwd(q1, Id, cd, t1, lse1, g, 1.0, 0.5, excl, r1, bias=bd)
        assert torch.equal(lse1, lse[b:b + 1]) and torch.equal(ts1, ts[b:b + 1]), b
        assert torch.equal(dQ1[0], dQ[b]) and torch.equal(dT1[0], dT[b]), b


def test_two_runs_are_bit_identical_with_repeated_ids_and_shared_targets(dev):
    from sa_gnn_amd import autograd as ag
    cum, W, cand, m, live, bias, hub, short = _duplicate_case()
    ni, nq, d = 700, 70, 128
    rng, Q, I = _case(12, ni, nq, d)
    target = rng.integers(0, ni, nq)
    target[:3] = hub                                                   # shared targets: a repeated candidate ...
    outside = next(k for k in range(ni) if k not in cand)
    target[10:14] = outside                                            # ... and an item outside the list
    target[20] = -1
    ptr, items = _hit_lists(rng, nq, ni, cand)
    a = _run(dev, Q, I, cand, bias, target, 0.5, 1.0 / nq, ptr, items)
    b = _run(dev, Q, I, cand, bias, target, 0.5, 1.0 / nq, ptr, items)
    assert a["loss"] == b["loss"]
    for k in ("lse", "tscore", "dQ", "dIc", "dT"):
        assert np.array_equal(a[k], b[k]), k
    cd, bd, tg, excl = _t(dev, cand, np.int32), _t(dev, bias, np.float32), _t(dev, target, np.int32), _excl(dev, ptr, items)
    grads = []
    for _ in range(2):
        q, i = _t(dev, Q, np.float32).requires_grad_(True), _t(dev, I, np.float32).requires_grad_(True)
        loss = ag.SoftmaxLossCandFn.apply(q, i, cd, tg, 0.5, 1.0 / nq, excl, None, bd)
        (loss * 2.0).sum().backward()
        grads.append((float(loss.detach()), q.grad.clone(), i.grad.clone()))
    assert grads[0][0] == grads[1][0] == a["loss"]
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
    full = grads[0][2].cpu().double().numpy() / 2.0
    ref = P.softmax_loss_pop_np(Q, I, cand, bias, target, 0.5, 1.0 / nq, ptr, items)
    terms = P.tolerance_terms(Q, I, target, ref, 0.5, 1.0 / nq)
    # float32 sums of at most four dT rows and one dIc row on top of the kernel's own bound
    need = R.worst_ratio(full, ref["dI"], terms["dI"][0], terms["dI"][1])
    print(f"assembled dI: K needed {need:.2f} / {K_DI} + 4 (the float32 adds of the shared rows)")
    assert need <= K_DI + 4
    # the live rows bit for bit where no target adds to them; nothing anywhere else
    tg_ids = set(target[target >= 0].tolist())
    for j in np.flatnonzero(live):
        if int(cand[j]) not in tg_ids:
            assert np.array_equal(grads[0][2][int(cand[j])].cpu().numpy(), np.float32(2.0) * a["dIc"][j]), j
    untouched = np.setdiff1d(np.arange(ni), np.concatenate([cand, target[target >= 0]]))
    assert not full[untouched].any()


# ---- the Recommender under --softmaxNegDist pop ----------------------------------------------------------------------
def _setup_pop(dev, monkeypatch, n, dist="pop", a=0.75, **kw):
    from sa_gnn_amd.Params import args
    monkeypatch.setattr(args, "softmaxNegs", n)
    monkeypatch.setattr(args, "softmaxNegDist", dist)
    monkeypatch.setattr(args, "softmaxNegPow", a)
    return _setup(dev, monkeypatch, **kw)


def _restated(handler, args, n, seed, step):
    from sa_gnn_amd import model
    w, cum, W = P.weights(model.item_degrees(handler.trnMat, args.item), args.softmaxNegPow)
    return (cum, W) + P.draw(cum, n, seed, step)


@pytest.mark.parametrize("n", [7, 40])
@pytest.mark.parametrize("d,ssldim,att_layer,temp", [(64, 48, 2, 1.0), (32, 32, 1, 0.5)])
def test_train_loss_under_pop_against_float64(dev, monkeypatch, d, ssldim, att_layer, temp, n):
    from sa_gnn_amd import ops
    from sa_gnn_amd.model import banned_table
    rec, handler, NNs, args = _setup_pop(dev, monkeypatch, n, d=d, ssldim=ssldim, att_layer=att_layer, temp=temp)
    batch = dict(_host_batch(rec, handler, args), cand_seed=(77, 3))
    cum, W, cand, m, live, bias = _restated(handler, args, n, 77, 3)
    cum_d, W_d = rec._pop_cum_device()
    assert W_d == W and cum_d.cpu().tolist() == cum
    got_cand, got_bias = (v.cpu().numpy() for v in ops.sample_strata_weighted(cum_d, W_d, n, 77, 3))
    assert got_cand.tolist() == cand.tolist() and np.array_equal(np.isneginf(got_bias), ~live)
    assert (_ulps(got_bias[live], bias[live]) <= 2).all()
    print(f"N {n}: {int(live.sum())} live positions, longest run {int(m.max())}")
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    Pm, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(mm)[0] for mm in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(mm))[0] for mm in handler.subMat]
    opre, ossl, _, _ = P.torch_train_loss_pop(Pm, adj, tp, batch, dict(CFG, temp=temp), banned_table(handler, args.item),
                                              cand, got_bias)
    (opre + args.ssl_reg * ossl).backward()
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"N {n}: preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
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


def test_batch_rows_and_the_device_sampler_give_what_all_rows_and_the_host_form_give(dev, monkeypatch):
    from test_gpu_device_sampler import _host_form
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _setup_pop(dev, monkeypatch, 25)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    dev_batch = dict(rec.sample_batch_device(bat, 2024, 1), cand_seed=(5, 1))
    for b in (dict(rec._host_train_batch(bat), cand_seed=(5, 1)), dev_batch):
        res = _both_modes(rec, NNs, args, b, 1.0)
        (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
        users, items = rec.fusion_rows_counts
        print(f"touched users {users} items {items}; preLoss all {pa!r} batch {pb!r}")
        assert items < args.item or users < args.user
        assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
        _check_against(gb, ga, ga, "batch vs all")
    hb = dict(_host_form(rec, dev_batch, args), cand_seed=(5, 1))
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, dev_batch)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"preLoss device {pre_d!r} host {pre_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed", "uEmbed"):
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)
    assert _loss_and_grads(rec, NNs, args, dict(dev_batch, cand_seed=(5, 2)))[0] != pre_d     # another step, another list


def test_uniform_is_untouched(dev, monkeypatch):
    """With the flag at its default train_loss draws the uniform strata, hands the loss no offsets (so the entries
    without one run) and returns their loss bit for bit; the weighted draw is never called."""
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import ops
    from sa_gnn_amd.Params import args as the_args
    assert the_args.softmaxNegDist == "uniform"
    rec, handler, NNs, args = _setup_pop(dev, monkeypatch, 13, dist="uniform")

    def never(*a, **k):
        raise AssertionError("the weighted draw ran under --softmaxNegDist uniform")
    monkeypatch.setattr(ops, "sample_strata_weighted", never)
    seen = []
    real = ops.softmax_loss_cand

    def spy(Q, I, cand, target, inv_temp=1.0, scale=None, excl=None, excl_row=None, bias=None):
        out = real(Q, I, cand, target, inv_temp, scale, excl, excl_row, bias)
        seen.append((Q.clone(), I.clone(), cand.clone(), target.clone(), inv_temp, scale, excl, excl_row, bias, out[0].clone()))
        return out
    monkeypatch.setattr(ops, "softmax_loss_cand", spy)
    batch = dict(_host_batch(rec, handler, args), cand_seed=(77, 3))
    pre = rec.train_loss(dict(batch), keep_rate=1.0)[0]
    assert len(seen) == 1
    Q, I, cand, target, inv_temp, scale, excl, excl_row, bias, loss = seen[0]
    assert bias is None and cand.cpu().tolist() == C.strata(args.item, 13, 77, 3).tolist()
    again = real(Q, I, cand, target, inv_temp, scale, excl, excl_row)[0]       # the entry without an offset, directly
    assert torch.equal(pre.detach().reshape(1), loss) and torch.equal(again, loss)
    assert ag.SoftmaxLossCandFn.apply(Q, I, cand, target, inv_temp, scale, excl, excl_row).equal(loss)


def test_train_epochs_stay_finite_and_improve(dev, monkeypatch):
    """--softmaxNegDist pop with --fusion_rows batch and --sampler device. trainEpoch draws no seed of its own for it."""
    rec, handler, NNs, args = _setup_pop(dev, monkeypatch, 16, d=64, ssldim=32, att_layer=1)
    for k, v in (("trnNum", 64), ("lr", 5e-3), ("keepRate", 0.5), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay_step", 64 // args.batch),
                 ("fusion_rows", "batch"), ("sampler", "device")):
        monkeypatch.setattr(args, k, v)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["preLoss"] for _ in range(8)]
    after = np.random.randint(0, 2 ** 31)
    print("preLoss per epoch:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert all(bool(torch.isfinite(p).all()) for p in NNs.params.values())
    monkeypatch.setattr(args, "softmaxNegDist", "uniform")             # the numpy stream a uniform run consumes is the same
    np.random.seed(0)
    for _ in range(8):
        rec.trainEpoch()
    assert np.random.randint(0, 2 ** 31) == after


def test_checkpoint_saved_under_pop_loads_under_uniform_and_under_hinge(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _setup_pop(dev, monkeypatch, 13)
    for k, v in (("epoch", 1), ("save_path", "pop_ckpt"), ("load_model", "pop_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    state = torch.load(str(tmp_path / "Models" / "pop_ckpt"), weights_only=True)
    assert "softmaxNegDist" not in state and "softmaxNegPow" not in state     # the flags are not part of the model
    for loss, negs in (("softmax", 13), ("hinge", 0)):
        monkeypatch.setattr(args, "softmaxNegDist", "uniform")
        monkeypatch.setattr(args, "softmaxNegs", negs)
        monkeypatch.setattr(args, "predLoss", loss)
        rec2 = Recommender(dev, handler)
        rec2.prepareModel()
        assert rec2.testEpoch() != want
        rec2.loadModel(str(tmp_path))
        assert rec2.testEpoch() == want
