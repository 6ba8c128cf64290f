"""GPU suite of the sampled-candidate softmax loss (--softmaxNegs): the stratified draw against its numpy
restatement, sagnn_softmax_loss_f32's candidate mode and its backward against the float64 restatement (softmax_cand_ref: the
full-table reference with every non-candidate put on the row's list), their contracts (row independence, bit-identical
runs, skipped rows), then the flag inside the Recommender.

Tolerances: softmax_loss_ref.tolerance_terms with the constants of test_gpu_softmax_loss.py (K_LSE 16, K_DQ 32,
K_DI 32: 4 x float32-CPU against float64). The arithmetic per element is that suite's; the device dI is assembled in
float64 (dIc at the candidates, dT added at the targets), which adds no rounding of its own."""
import numpy as np
import pytest
import torch

import softmax_cand_ref as C
import softmax_loss_ref as R
from oracle import selfgnn_oracle as O
from test_gpu_softmax_loss import (CFG, K_DI, K_DQ, K_LSE, _grad_close, _host_batch, _lists, _loss_and_grads, _oracle_params,
                                   _profile_kinds, _setup, _t)

pytestmark = pytest.mark.gpu


def _excl(dev, ptr, items):
    if ptr is None:
        return None
    return _t(dev, ptr, np.int64), (_t(dev, items, np.int32) if len(items) else torch.zeros(1, dtype=torch.int32, device=dev))


def _run(dev, Q, I, cand, target, inv_temp, scale, ptr=None, items=None, rows=None, g=1.0):
    from sa_gnn_amd import ops
    Qd = Q if isinstance(Q, torch.Tensor) else _t(dev, Q, np.float32)
    Id, tg, cd = _t(dev, I, np.float32), _t(dev, target, np.int32), _t(dev, cand, np.int32)
    excl, rd = _excl(dev, ptr, items), None if rows is None else _t(dev, rows, np.int32)
    loss, lse, ts = ops.softmax_loss_cand(Qd, Id, cd, tg, inv_temp, scale, excl, rd)
    gd = torch.full((1,), g, dtype=torch.float32, device=dev)
    dQ, dIc, dT = ops.softmax_loss_cand_bwd(Qd, Id, cd, tg, lse, gd, inv_temp, scale, excl, rd)
    torch.cuda.synchronize()
    assert dIc.shape == (len(cand), I.shape[1]) and dT.shape == dQ.shape == (len(target), I.shape[1])
    out = {"loss": float(loss), "lse": lse.cpu().numpy(), "tscore": ts.cpu().numpy(), "dQ": dQ.cpu().numpy(),
           "dIc": dIc.cpu().numpy(), "dT": dT.cpu().numpy()}
    out["dI"] = C.assemble_dI(len(I), cand, out["dIc"], target, out["dT"])
    return out


def _check(got, Q, I, cand, target, inv_temp, scale, ptr=None, items=None, rows=None, name="", g=1.0):
    """Every output against float64 under the derived bounds; prints the K each output needs before it asserts."""
    ref = C.softmax_loss_cand_np(Q, I, cand, target, inv_temp, scale, ptr, items, rows)
    terms = R.tolerance_terms(Q, I, target, ref, inv_temp, scale)
    need = {k: R.worst_ratio(got[k] / (g if k in ("dQ", "dI") else 1.0), ref[k], *terms[k]) for k in ("lse", "dQ", "dI")}
    need["tscore"] = R.worst_ratio(got["tscore"], ref["tscore"], terms["lse"][0] / inv_temp, 0.0)
    loss_tol = abs(scale) * (2 * K_LSE * terms["lse"][0]).sum() + 4 * R.EPS32 * abs(ref["loss"])
    print(f"{name}: K needed lse {need['lse']:.2f} / {K_LSE}, tscore {need['tscore']:.2f} / {K_LSE}, dQ {need['dQ']:.2f} / {K_DQ}, "
          f"dI {need['dI']:.2f} / {K_DI}; loss {got['loss']!r} vs {ref['loss']!r} (tol {loss_tol:.3e})")
    for k in ("lse", "tscore", "dQ", "dIc", "dT"):
        assert np.isfinite(got[k]).all(), f"{name}: {k} holds inf or NaN"
    assert need["lse"] <= K_LSE and need["tscore"] <= K_LSE and need["dQ"] <= K_DQ and need["dI"] <= K_DI, (name, need)
    assert np.isfinite(got["loss"]) and abs(got["loss"] - ref["loss"]) <= loss_tol, name
    # dT[b] is the target's term alone and dIc holds nothing of it
    tgt = np.asarray(target, dtype=np.int64)
    ok = (tgt >= 0) & (tgt < len(I))
    assert not got["dT"][~ok].any(), f"{name}: a skipped row has a dT row"
    return ref, terms


@pytest.mark.parametrize("n_items,n_cand", [(1, 1), (17, 5), (4099, 64), (52619, 4096), (300, 300)])
def test_device_draw_equals_the_numpy_restatement(dev, n_items, n_cand):
    from sa_gnn_amd import ops
    for seed, step in ((0, 0), (0x9E3779B97F4A7C15, 3), (2 ** 64 - 1, 2 ** 32 - 1)):
        got = ops.sample_strata(n_items, n_cand, seed, step, dev)
        assert got.dtype == torch.int32 and got.shape == (n_cand,) and got.device.type == "cuda"
        assert got.cpu().numpy().tolist() == C.strata(n_items, n_cand, seed, step).tolist(), (seed, step)
    assert ops.sample_strata(n_items, 0, 1, 1, dev).shape == (0,)


N_CANDS = (0, 1, 15, 16, 17, 63, 64, 65, 130)      # 130 crosses the 128-position chunk; 16 / 64: the tile and the span


@pytest.mark.parametrize("temp", [1.0, 0.25])
@pytest.mark.parametrize("nq", [1, 7, 17, 40, 70])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_forward_and_both_gradients_against_float64(dev, d, nq, temp):
    ni = 4099
    rng = np.random.default_rng(1000 * d + nq)
    Q = (rng.standard_normal((nq, d)) * 0.7).astype(np.float32)
    I = (rng.standard_normal((ni, d)) * 0.7).astype(np.float32)
    by_row = temp != 1.0                                           # one temperature through excl_row, one through list b
    scale, g = 1.0 / nq, 0.5                                       # an upstream gradient other than 1 (a power of two)
    for n_cand in N_CANDS:
        cand = np.sort(rng.choice(ni, n_cand, replace=False))
        target = rng.integers(0, ni, nq)
        if n_cand:                                                 # every other row's target is a candidate
            target[::2] = cand[rng.integers(0, n_cand, len(target[::2]))]
        ptr, items = _lists(rng, nq, ni, nq + 3 if by_row else None)
        if n_cand:                                                 # lists that hit candidates, not only the 2 % at random
            lists = [items[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]
            lists = [np.sort(np.concatenate([v, cand[rng.integers(0, n_cand, min(n_cand, 5))]])) for v in lists]
            ptr, items = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64), np.concatenate(lists)
        rows = rng.integers(0, nq + 3, nq) if by_row else None
        got = _run(dev, Q, I, cand, target, 1.0 / temp, scale, ptr, items, rows, g=g)
        _check(got, Q, I, cand, target, 1.0 / temp, scale, ptr, items, rows, name=f"d {d} nq {nq} temp {temp} n_cand {n_cand}", g=g)
        if n_cand == 0:                                            # lse = z(b, t): no loss, no gradient, exactly
            assert np.array_equal(got["lse"], got["tscore"] * np.float32(1.0 / temp)) and got["loss"] == 0.0
            assert not got["dQ"].any() and not got["dT"].any() and got["dIc"].shape == (0, d)


@pytest.mark.parametrize("ni,n_cand,nq,d", [(52619, 33000, 33, 64), (17000, 16400, 17, 32), (9000, 8200, 17, 128)])
def test_the_chunk_size_steps_up_and_long_lists(dev, ni, n_cand, nq, d):
    """chunk_items(33000) = 144 > 128; and from 256 spans of 64 positions (32 at d = 128) on, the dIc kernel runs its
    wide form: 16,384 candidates at d = 32 / 64, 8,192 at d = 128. Every shorter list of this suite runs the narrow one."""
    rng = np.random.default_rng(77 + d)
    Q = (rng.standard_normal((nq, d)) * 0.7).astype(np.float32)
    I = (rng.standard_normal((ni, d)) * 0.7).astype(np.float32)
    cand = np.sort(rng.choice(ni, n_cand, replace=False))
    target = rng.integers(0, ni, nq)
    ptr, items = _lists(rng, nq, ni)
    got = _run(dev, Q, I, cand, target, 1.0, 1.0 / nq, ptr, items)
    _check(got, Q, I, cand, target, 1.0, 1.0 / nq, ptr, items, name=f"ni {ni} n_cand {n_cand} d {d}")


def _pattern_case(seed, ni, nq, d):
    rng = np.random.default_rng(seed)
    Q = (rng.standard_normal((nq, d)) * 0.7).astype(np.float32)
    I = (rng.standard_normal((ni, d)) * 0.7).astype(np.float32)
    return rng, Q, I


@pytest.mark.parametrize("d", [32, 64, 128])
def test_candidate_and_list_patterns(dev, d):
    """One batch whose rows each hold one sharp pattern, over a candidate list clustered inside one 16-id window plus a
    few far ids (so that one tile's ids span the catalogue)."""
    ni, nq = 4099, 21
    rng, Q, I = _pattern_case(200 + d, ni, nq, d)
    cand = np.sort(np.concatenate([np.arange(1600, 1616)[rng.random(16) < 0.7], [5, 700, 1599, 1616, 3000, 4090],
                                   rng.choice(np.arange(2000, 2900), 90, replace=False)]))
    n_cand = len(cand)
    target = rng.integers(0, ni, nq)
    lists = [np.sort(rng.integers(0, ni, 40)) for _ in range(nq)]
    lists[0] = np.arange(0, cand[0])                               # wholly below cand[0]
    lists[1] = np.arange(cand[-1] + 1, ni)                         # wholly above cand[-1]
    lists[2] = np.arange(3001, 4090)                               # between the last two candidates: hits none
    lists[3] = cand.copy()                                         # every candidate: only the target remains
    target[3] = 1234                                               # ... a target outside cand
    lists[4] = np.arange(0, ni)                                    # everything, the target a candidate on its own list
    target[4] = cand[7]
    target[5] = cand[0]                                            # a candidate target on its own list, others eligible
    lists[5] = np.sort(np.concatenate([lists[5], [cand[0]] * 2, cand[3:6]]))
    target[6] = next(t for t in range(1601, 1700) if t not in cand)        # outside cand, inside the cluster's id range
    target[7] = target[8] = cand[20]                               # two rows share a candidate target
    target[9] = target[10] = target[11] = 3500                     # three rows share a target outside cand
    target[12] = -1                                                # no target
    target[13] = ni                                                # just past the table: skipped as well
    lists[14] = cand[::2].copy()                                   # every other candidate
    lists[15] = np.sort(np.concatenate([cand[-3:], cand[-3:]]))    # duplicated entries on the last candidates
    target[16] = cand[-1]
    target[17] = 0
    target[18] = ni - 1
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    items = np.concatenate(lists)
    scale = 1.0 / nq
    got = _run(dev, Q, I, cand, target, 1.0, scale, ptr, items)
    ref, terms = _check(got, Q, I, cand, target, 1.0, scale, ptr, items, name=f"patterns d {d} n_cand {n_cand}")
    for b in (3, 4):                                               # p(target) = 1: no loss, no gradient, to the tolerance
        assert abs(got["lse"][b] - got["tscore"][b]) <= 2 * K_LSE * terms["lse"][0][b]
        assert (np.abs(got["dQ"][b]) <= K_DQ * terms["dQ"][0][b] + terms["dQ"][1][b]).all()
        assert ref["eligible"][b].sum() == 1
    for b in (12, 13):
        for k in ("lse", "tscore", "dQ", "dT"):
            assert not got[k][b].any(), (k, b)
    assert ref["eligible"][5, cand[0]] and ref["p"][5, cand[0]] > 0 and not ref["eligible"][5, cand[3:6]].any()
    for b in (0, 1, 2):                                            # these lists hit no candidate
        assert len(lists[b]) > 0 and ref["eligible"][b].sum() == n_cand + (target[b] not in cand)
    # the shared targets: each row's dT is its own term, the assembled row their sum
    assert got["dT"][9].any() and got["dT"][10].any() and not np.array_equal(got["dT"][9], got["dT"][10])


@pytest.mark.parametrize("all_rows", [False, True])
def test_rows_without_a_target_are_skipped(dev, all_rows):
    ni, nq, d, n_cand = 4099, 40, 32, 130
    rng, Q, I = _pattern_case(10, ni, nq, d)
    cand = C.strata(ni, n_cand, 4, 0)
    target = rng.integers(0, ni, nq)
    skipped = np.arange(nq) if all_rows else np.array([0, 5, 15, 16, 17, 39])
    target[skipped] = -1
    ptr, items = _lists(rng, nq, ni)
    got = _run(dev, Q, I, cand, target, 1.0, 1.0 / nq, ptr, items)
    for k in ("lse", "tscore", "dQ", "dT"):
        assert not got[k][skipped].any(), k
    if all_rows:
        assert got["loss"] == 0.0 and not got["dIc"].any() and not got["dI"].any()
    else:
        _check(got, Q, I, cand, target, 1.0, 1.0 / nq, ptr, items, name="some rows skipped")


@pytest.mark.parametrize("d", [32, 64, 128])
def test_all_candidates_agree_with_the_full_entry(dev, d):
    """cand = arange(n_items): the objective of ops.softmax_loss. Both sit within the bounds of the same reference,
    so they differ by at most twice the bound; bit equality is not asked (the target is merged separately here)."""
    from sa_gnn_amd import ops
    ni, nq = 4099, 40
    rng, Q, I = _pattern_case(300 + d, ni, nq, d)
    target = rng.integers(0, ni, nq)
    target[3] = -1
    ptr, items = _lists(rng, nq, ni)
    cand = np.arange(ni)
    scale = 1.0 / nq
    got = _run(dev, Q, I, cand, target, 2.0, scale, ptr, items)
    ref, terms = _check(got, Q, I, cand, target, 2.0, scale, ptr, items, name=f"arange d {d}")
    full_ref = R.softmax_loss_np(Q, I, target, 2.0, scale, ptr, items)
    assert np.array_equal(ref["eligible"], full_ref["eligible"])
    Qd, Id, tg = _t(dev, Q, np.float32), _t(dev, I, np.float32), _t(dev, target, np.int32)
    excl = _excl(dev, ptr, items)
    loss, lse, ts = ops.softmax_loss(Qd, Id, tg, 2.0, scale, excl)
    dQ, dI = ops.softmax_loss_bwd(Qd, Id, tg, lse, torch.ones(1, device=dev), 2.0, scale, excl)
    full = {"lse": lse.cpu().numpy(), "dQ": dQ.cpu().numpy(), "dI": dI.cpu().numpy()}
    for k, K in (("lse", K_LSE), ("dQ", K_DQ), ("dI", K_DI)):
        diff = np.abs(got[k].astype(np.float64) - full[k])
        assert (diff <= 2 * (K * terms[k][0] + terms[k][1])).all(), k
    assert np.array_equal(ts.cpu().numpy(), got["tscore"])         # the same tile arithmetic on the same two rows
    assert abs(float(loss) - got["loss"]) <= 2 * (abs(scale) * (2 * K_LSE * terms["lse"][0]).sum() + 4 * R.EPS32 * abs(ref["loss"]))


@pytest.mark.parametrize("padded", [False, True])
def test_a_rows_outputs_do_not_depend_on_the_batch(dev, padded):
    """lse, tscore and the dQ and dT rows of row b, bit for bit, in a call of 70 rows and in a call of that row alone."""
    from sa_gnn_amd import ops
    ni, nq, d, n_cand = 4099, 70, 64, 130
    rng, Q, I = _pattern_case(11, ni, nq, d)
    cand = np.sort(rng.choice(ni, n_cand, replace=False))
    target = rng.integers(0, ni, nq)
    target[::3] = cand[rng.integers(0, n_cand, len(target[::3]))]
    ptr, items = _lists(rng, nq, ni)
    rows = rng.permutation(nq)
    Id, tg, rd, cd = _t(dev, I, np.float32), _t(dev, target, np.int32), _t(dev, rows, np.int32), _t(dev, cand, np.int32)
    excl = _excl(dev, ptr, items)
    Qd = _t(dev, Q, np.float32)
    if padded:                                                     # the same rows at a stride of d + 12
        buf = torch.full((nq, d + 12), 7.0, dtype=torch.float32, device=dev)
        buf[:, :d] = Qd
        Qd = buf[:, :d]
    g = torch.ones(1, dtype=torch.float32, device=dev)
    scale = 0.5                                                    # the same scale in both calls: scale is an input
    _, lse, ts = ops.softmax_loss_cand(Qd, Id, cd, tg, 1.0, scale, excl, rd)
    dQ, _, dT = ops.softmax_loss_cand_bwd(Qd, Id, cd, tg, lse, g, 1.0, scale, excl, rd)
    for b in (0, 15, 16, 23, 39, 64, 69):
        q1, t1, r1 = _t(dev, Q[b:b + 1], np.float32), tg[b:b + 1].contiguous(), rd[b:b + 1].contiguous()
        _, lse1, ts1 = ops.softmax_loss_cand(q1, Id, cd, t1, 1.0, scale, excl, r1)
        dQ1, _, dT1 = ops.softmax_loss_cand_bwd(q1, Id, cd, t1, lse1, g, 1.0, scale, excl, r1)
        assert torch.equal(lse1, lse[b:b + 1]) and torch.equal(ts1, ts[b:b + 1]), b
        assert torch.equal(dQ1[0], dQ[b]) and torch.equal(dT1[0], dT[b]), b


def test_two_runs_are_bit_identical(dev):
    from sa_gnn_amd import autograd as ag
    ni, nq, d, n_cand = 4099, 70, 128, 333
    rng, Q, I = _pattern_case(12, ni, nq, d)
    cand = np.sort(rng.choice(ni, n_cand, replace=False))
    target = rng.integers(0, ni, nq)
    target[:3] = cand[5]                                           # shared targets, inside and outside cand
    target[10:14] = 2000 if 2000 not in cand else 2001
    target[20] = -1
    ptr, items = _lists(rng, nq, ni)
    a = _run(dev, Q, I, cand, target, 0.5, 1.0 / nq, ptr, items)
    b = _run(dev, Q, I, cand, target, 0.5, 1.0 / nq, ptr, items)
    assert a["loss"] == b["loss"]
    for k in ("lse", "tscore", "dQ", "dIc", "dT"):
        assert np.array_equal(a[k], b[k]), k
    # the autograd function's assembled full-size dI
    cd, tg, excl = _t(dev, cand, np.int32), _t(dev, target, np.int32), _excl(dev, ptr, items)
    grads = []
    for _ in range(2):
        q, i = _t(dev, Q, np.float32).requires_grad_(True), _t(dev, I, np.float32).requires_grad_(True)
        loss = ag.SoftmaxLossCandFn.apply(q, i, cd, tg, 0.5, 1.0 / nq, excl, None)
        (loss * 2.0).sum().backward()
        grads.append((float(loss.detach()), q.grad.clone(), i.grad.clone()))
    assert grads[0][0] == grads[1][0] == a["loss"]
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
    full = grads[0][2].cpu().double().numpy() / 2.0
    ref = C.softmax_loss_cand_np(Q, I, cand, target, 0.5, 1.0 / nq, ptr, items)
    terms = R.tolerance_terms(Q, I, target, ref, 0.5, 1.0 / nq)
    # float32 sums of at most four dT rows and one dIc row on top of the kernel's own bound
    need = R.worst_ratio(full, ref["dI"], terms["dI"][0], terms["dI"][1])
    print(f"assembled dI: K needed {need:.2f} / {K_DI} + 4 (the float32 adds of the shared rows)")
    assert need <= K_DI + 4
    untouched = np.setdiff1d(np.arange(ni), np.concatenate([cand, target[target >= 0]]))
    assert not full[untouched].any()


# ---- the Recommender under --softmaxNegs ---------------------------------------------------------------------------
def _setup_negs(dev, monkeypatch, n, **kw):
    from sa_gnn_amd.Params import args
    monkeypatch.setattr(args, "softmaxNegs", n)
    return _setup(dev, monkeypatch, **kw)


def _cand_banned(handler, args, cand):
    """The banned table with every item outside cand added to each user's list: eligibility = cand + the target."""
    from sa_gnn_amd.model import banned_table
    ptr, items = banned_table(handler, args.item)
    return C.augmented(args.user, args.item, cand, ptr, items, None)


@pytest.mark.parametrize("n", [7, "all"])
@pytest.mark.parametrize("d,ssldim,att_layer,temp", [(64, 48, 2, 1.0), (32, 32, 1, 0.5)])
def test_train_loss_under_softmax_negs_against_float64(dev, monkeypatch, d, ssldim, att_layer, temp, n):
    from sa_gnn_amd import ops
    n = 60 if n == "all" else n
    rec, handler, NNs, args = _setup_negs(dev, monkeypatch, n, d=d, ssldim=ssldim, att_layer=att_layer, temp=temp)
    assert n < args.item or n == args.item == 60
    batch = dict(_host_batch(rec, handler, args), cand_seed=(77, 3))
    cand = ops.sample_strata(args.item, n, 77, 3, dev).cpu().numpy()           # read back from the device
    assert len(cand) == n and cand.tolist() == C.strata(args.item, n, 77, 3).tolist()
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = R.torch_train_loss_softmax(P, adj, tp, batch, dict(CFG, temp=temp), _cand_banned(handler, args, cand))
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


def test_batch_rows_give_what_all_rows_give(dev, monkeypatch):
    from test_gpu_fusion_rows import _both_modes, _check_against
    rec, handler, NNs, args = _setup_negs(dev, monkeypatch, 9)
    np.random.seed(3)
    bat = np.random.permutation(args.user)[:args.batch]
    for b in (dict(rec._host_train_batch(bat), cand_seed=(5, 1)), dict(rec.sample_batch_device(bat, 2024, 1), cand_seed=(5, 1))):
        res = _both_modes(rec, NNs, args, b, 1.0)
        (pa, sa, ga), (pb, sb, gb) = res["all"], res["batch"]
        users, items = rec.fusion_rows_counts
        print(f"touched users {users} items {items}; preLoss all {pa!r} batch {pb!r}")
        assert items < args.item or users < args.user
        assert abs(pb - pa) <= 1e-6 * max(abs(pa), 1.0) and abs(sb - sa) <= 1e-6 * max(abs(sa), 1.0)
        _check_against(gb, ga, ga, "batch vs all")


def test_device_sampled_batch_gives_the_host_forms_loss(dev, monkeypatch):
    from test_gpu_device_sampler import _host_form
    rec, handler, NNs, args = _setup_negs(dev, monkeypatch, 11)
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = dict(rec.sample_batch_device(bat, 31337, 2), cand_seed=(8, 2))
    hb = dict(_host_form(rec, b, args), cand_seed=(8, 2))
    assert "active" in b and "active" not in hb
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, b)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"preLoss device {pre_d!r} host {pre_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed", "uEmbed"):
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)
    other = _loss_and_grads(rec, NNs, args, dict(b, cand_seed=(8, 3)))[0]      # another step: another candidate set
    assert other != pre_d


def test_train_epochs_stay_finite_and_improve(dev, monkeypatch):
    """--softmaxNegs with --fusion_rows batch and --sampler device, the combination the flag exists for."""
    rec, handler, NNs, args = _setup_negs(dev, monkeypatch, 16, d=64, ssldim=32, att_layer=1)
    for k, v in (("trnNum", 64), ("lr", 5e-3), ("keepRate", 0.5), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay_step", 64 // args.batch),
                 ("fusion_rows", "batch"), ("sampler", "device")):
        monkeypatch.setattr(args, k, v)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["preLoss"] for _ in range(8)]
    print("preLoss per epoch:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert all(bool(torch.isfinite(p).all()) for p in NNs.params.values())
    assert rec.fusion_rows_counts[1] <= args.item
    res = rec.testEpoch()
    assert 0.0 <= res["HR"] <= 1.0 and 0.0 <= res["NDCG"] <= 1.0


def test_off_means_off(dev, monkeypatch):
    """With N = 0 a step records no launch of the new profile kind (7) and the kinds it recorded before: none of 6
    under hinge, the two of 6 under softmax. With N > 0 the two launches are of kind 7 and none of kind 6."""
    from sa_gnn_amd import _lib
    from sa_gnn_amd.Params import args as the_args
    assert the_args.softmaxNegs == 0
    lib = _lib.load()
    step = lambda rec, handler, NNs, args: _profile_kinds(      # noqa: E731
        lib, lambda: _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args)))[1]
    hinge = step(*_setup(dev, monkeypatch, loss="hinge"))
    assert len(hinge) > 0 and not (hinge == 6).any() and not (hinge == 7).any()
    full = step(*_setup(dev, monkeypatch, loss="softmax"))
    assert (full == 6).sum() == 2 and not (full == 7).any()
    negs = step(*_setup_negs(dev, monkeypatch, 13, loss="softmax"))
    assert (negs == 7).sum() == 2 and not (negs == 6).any()
    # nothing else differs between the two softmax steps
    assert sorted(full[full != 6].tolist()) == sorted(negs[negs != 7].tolist())


def test_checkpoint_saved_with_candidates_loads_without_them_and_under_hinge(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _setup_negs(dev, monkeypatch, 13)
    for k, v in (("epoch", 1), ("save_path", "negs_ckpt"), ("load_model", "negs_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    state = torch.load(str(tmp_path / "Models" / "negs_ckpt"), weights_only=True)
    assert "softmaxNegs" not in state and "predLoss" not in state              # the flag is not part of the model
    for loss in ("softmax", "hinge"):
        monkeypatch.setattr(args, "softmaxNegs", 0)
        monkeypatch.setattr(args, "predLoss", loss)
        rec2 = Recommender(dev, handler)
        rec2.prepareModel()
        assert rec2.testEpoch() != want
        rec2.loadModel(str(tmp_path))
        assert rec2.testEpoch() == want
