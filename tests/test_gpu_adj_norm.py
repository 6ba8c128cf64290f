"""GPU suite of the edge-weighted interval SpMM and the opt-in symmetric degree normalisation (SpmmPlan(weights=),
graph.interval_pair(norm="sym"), --adjNorm sym): each edge's own weight, exactly, for every row class and
lane-group width; values and the training epilogue against float64; that a plan without weights runs what it ran; the
stack and its adjoint against torch float64 autograd over the dense D^-1/2 P D^-1/2 of adj_norm_ref, alone and under edge
dropout; the large-row-block instantiations; the Recommender. Graphs follow test_gpu_edge_drop.py: 40 rows with plan
tuning (4, 16, 64), so short, medium and chunked long rows all occur."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import adj_norm_ref as R
import edge_drop_ref as D
from oracle import selfgnn_oracle as O
from test_gpu_edge_drop import (BIG_D, BIG_I, BIG_U, N_ROWS, SEED, STEP, TUNING, _big_matrix, _graph, _intervals,
                                _sparse_stack_reference, assert_sum_close)

pytestmark = pytest.mark.gpu


def _weighted_plans(dev, n_src, w_of):
    """The 40-row graph of the edge-drop suite (row 1 = items 0, 1, 2) with weights w_of(nnz), and its exact transpose
    carrying the same weight per stored copy. Returns the plans, the float64 dense sums of weights [40, n_src], the
    multiplicities and the row degrees."""
    from sa_gnn_amd import ops
    rowptr, colidx, count = _graph(n_src, lambda u, i: i >= 3)
    w = w_of(colidx.size).astype(np.float32)
    rows = np.repeat(np.arange(N_ROWS), np.diff(rowptr))
    plan = ops.SpmmPlan(rowptr, colidx, N_ROWS, n_src, device=dev, tuning=TUNING, weights=w)
    order = np.argsort(colidx, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n_src))]).astype(np.int32)
    plan_t = ops.SpmmPlan(rp_t, rows[order].astype(np.int32), n_src, N_ROWS, device=dev, tuning=TUNING, weights=w[order])
    assert plan.weighted and plan.info.weighted == 1 and plan_t.info.weighted == 1
    deg = np.diff(rowptr)
    # the row classes: empty, short <= 4, medium <= 16, long in several chunks, a duplicated entry
    assert plan.info.n_long_rows >= 5 and plan.info.n_chunks > plan.info.n_long_rows and count.max() >= 2
    assert (deg == 0).any() and ((deg > 0) & (deg <= 4)).any() and ((deg > 4) & (deg <= 16)).any() and (deg > 16).any()
    dense = np.zeros((N_ROWS, n_src), np.float64)
    np.add.at(dense, (rows, colidx), w.astype(np.float64))
    return plan, plan_t, dense, count, deg, (rowptr, colidx, w)


def _classes(deg):
    return (("empty", deg == 0), ("short", (deg > 0) & (deg <= 4)), ("medium", (deg > 4) & (deg <= 16)), ("long", deg > 16))


# ---- 1. each edge gets its own weight, exactly -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128])
def test_each_edge_gets_its_own_weight_exactly(dev, d):
    """X = I and w[e] = 2^((7 e mod 11) - 5): out[r, c] is the sum of the weights of the copies of (r, c), and sums of
    powers of two within 11 binades are exact in fp32 whatever the order, so the comparison is bit for bit."""
    from sa_gnn_amd import ops
    n_src = d
    pow2 = lambda nnz: np.exp2((7 * np.arange(nnz)) % 11 - 5.0)
    plan, plan_t, dense, count, deg, _ = _weighted_plans(dev, n_src, pow2)
    want = dense.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), dense)                       # the expected sums are fp32 numbers
    assert len(np.unique(want[count > 0])) >= 11 and (want[2, 7] != want[2, 3])
    got = ops.spmm_ex(plan, torch.eye(n_src, d, device=dev), 1.0, want_out=True).cpu().numpy()
    for name, rows in _classes(deg):
        assert rows.any() and np.array_equal(got[rows], want[rows]), name
    # the transposed plan with the permuted weights: the transpose, for the first d users the identity shows
    got_t = ops.spmm_ex(plan_t, torch.eye(N_ROWS, d, device=dev), 1.0, want_out=True).cpu().numpy()
    w = min(N_ROWS, d)
    assert np.array_equal(got_t[:, :w], want.T[:, :w]) and not got_t[:, w:].any()


# ---- 2. values and the training epilogue vs float64 ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128])
def test_values_and_training_epilogue_vs_float64(dev, d):
    from sa_gnn_amd import ops
    n_src, leaky = 64, 0.5
    rng = np.random.default_rng(170 + d)
    plan, _, dense, count, deg, _ = _weighted_plans(dev, n_src, lambda nnz: rng.uniform(0.05, 2.0, nnz))
    x, res, acc = (rng.standard_normal(s).astype(np.float32) for s in ((n_src, d), (N_ROWS, d), (N_ROWS, d)))
    out, acc_out = torch.empty((N_ROWS, d), device=dev), torch.empty((N_ROWS, d), device=dev)
    m_out = torch.empty((N_ROWS, d // 4), dtype=torch.uint8, device=dev)
    ops.spmm_ex(plan, torch.from_numpy(x).to(dev), leaky, residual=torch.from_numpy(res).to(dev), out=out,
                acc_in=torch.from_numpy(acc).to(dev), acc_out=acc_out, mask_out=m_out)
    s = dense @ x.astype(np.float64)
    terms = np.abs(dense) @ np.abs(x).astype(np.float64)                         # (|w| . count) @ |x|
    y = np.maximum(leaky * s, s) + res
    assert_sum_close(out.cpu().numpy(), y, terms + np.abs(res))
    assert_sum_close(acc_out.cpu().numpy(), y + acc, terms + np.abs(res) + np.abs(acc))
    bits = m_out.cpu().numpy()
    got_pos = ((bits[:, :, None] >> np.arange(4)) & 1).reshape(N_ROWS, d).astype(bool)
    sure = np.abs(s) > 1e-4 * np.abs(s) + 1e-5 + 2e-7 * terms                    # the sign of s is not in doubt
    left_out = (~sure[deg > 0]).mean()
    print(f"d = {d}: {100 * left_out:.3f} % of the mask bits of non-empty rows left out")
    assert left_out <= 0.01
    assert np.array_equal(got_pos[sure], (s > 0)[sure]) and not got_pos[deg == 0].any()


# ---- 3. off means off ---------------------------------------------------------------------------------------------------
def test_off_means_off_and_all_ones_is_the_unweighted_product(dev):
    from sa_gnn_amd import _lib, ops
    n_src, d = 64, 64
    plan_w, _, dense, count, deg, (rowptr, colidx, w) = _weighted_plans(dev, n_src, lambda nnz: np.ones(nnz))
    assert np.array_equal(dense, count)
    plain = ops.SpmmPlan(rowptr, colidx, N_ROWS, n_src, device=dev, tuning=TUNING)
    none = ops.SpmmPlan(rowptr, colidx, N_ROWS, n_src, device=dev, tuning=TUNING, weights=None)
    assert not plain.weighted and plain.info.weighted == 0 and not none.weighted and none.info.weighted == 0
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((n_src, d)).astype(np.float32)).to(dev)
    res = torch.from_numpy(rng.standard_normal((N_ROWS, d)).astype(np.float32)).to(dev)
    base = ops.spmm(plain, x, 0.5, residual=res)                                 # today's entry on today's plan
    assert torch.equal(ops.spmm_ex(plain, x, 0.5, residual=res, want_out=True), base)
    assert torch.equal(ops.spmm_ex(none, x, 0.5, residual=res, want_out=True), base)
    ones = ops.spmm_ex(plan_w, x, 0.5, residual=res, want_out=True)
    short = torch.from_numpy(deg <= 4).to(dev)
    assert torch.equal(ones[short], base[short])
    terms = count.astype(np.float64) @ np.abs(x.cpu().numpy()).astype(np.float64) + np.abs(res.cpu().numpy())
    assert_sum_close(ones.cpu().numpy(), base.cpu().numpy(), terms)
    # clearing the weights of a plan puts it back on the unweighted kernels: the same bits again
    _lib.check(_lib.load().sagnn_spmm_plan_set_weights(plan_w.handle, None))
    assert torch.equal(ops.spmm_ex(plan_w, x, 0.5, residual=res, want_out=True), base)
    _lib.check(_lib.load().sagnn_spmm_plan_set_weights(plan_w.handle, plan_w.weights.data_ptr()))
    assert torch.equal(ops.spmm_ex(plan_w, x, 0.5, residual=res, want_out=True), ones)


def test_a_batch_mixing_weighted_and_unweighted_plans_is_refused(dev):
    from sa_gnn_amd import _lib, graph, ops
    m = sp.csr_matrix((np.random.default_rng(1).random((12, 9)) < 0.4).astype(np.intc))
    fw, tw = graph.interval_pair(m, dev, norm="sym")
    fn, tn = graph.interval_pair(m, dev)
    assert fw.plan.weighted and tw.plan.weighted and not fn.plan.weighted
    for pu, pi in (([fw.plan, fn.plan], [tw.plan, tn.plan]), ([fw.plan], [tn.plan]), ([fn.plan], [tw.plan])):
        with pytest.raises(ValueError, match="weights"):
            ops.SpmmBatch(pu, pi)
    # the library refuses it as well, with a message that says why
    lib, h = _lib.load(), ctypes.c_void_p()
    PU, PI = (ctypes.c_void_p * 1)(fw.plan.handle), (ctypes.c_void_p * 1)(tn.plan.handle)
    assert lib.sagnn_spmm_batch_create(PU, PI, 1, ctypes.byref(h)) == -5 and not h.value
    assert "edge weights" in _lib.last_error()
    assert ops.SpmmBatch([fw.plan], [tw.plan]).weighted and not ops.SpmmBatch([fn.plan], [tn.plan]).weighted


# ---- 4. the stack and its adjoint ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
def test_sym_stack_and_adjoint_vs_float64_autograd(dev, L):
    from sa_gnn_amd import autograd as ag
    from sa_gnn_amd import graph, ops
    T, U, I, d, leaky, keep = 3, 37, 29, 32, 0.5, 0.5
    rng = np.random.default_rng(40 + L)
    mats = _intervals(rng, U, I)
    u0, gu = (rng.standard_normal((T, U, d)).astype(np.float32) for _ in range(2))
    i0, gi = (rng.standard_normal((T, I, d)).astype(np.float32) for _ in range(2))
    sym = [R.dense_sym(m) for m in mats]
    assert sym[1].sum() == 1.0 and sym[1][0, 0] == 1.0                            # the empty interval: the phantom edge
    pairs = [graph.interval_pair(m, dev, tuning=TUNING, norm="sym") for m in mats]
    plans_u, plans_i = [a.plan for a, _ in pairs], [t.plan for _, t in pairs]
    assert all(p.weighted and p.partner_adjoint is None for p in plans_u + plans_i)
    assert plans_u[0].nnz == plans_i[0].nnz == mats[0].nnz - 1                    # the duplicated entry is merged
    assert plans_u[0].info.n_long_rows >= 1
    batch = ops.SpmmBatch(plans_u, plans_i)
    assert batch.adjoint() is batch
    gu_d, gi_d = torch.from_numpy(gu).to(dev), torch.from_numpy(gi).to(dev)

    def run(pu, pi, dr):
        tu = torch.from_numpy(u0).to(dev).requires_grad_(True)
        ti = torch.from_numpy(i0).to(dev).requires_grad_(True)
        ou, oi = ag.gnn_stack(tu, ti, pu, pi, L, leaky, drop=dr)
        ((ou * gu_d).sum() + (oi * gi_d).sum()).backward()
        return ou.detach(), oi.detach(), tu.grad, ti.grad

    def check(got, a_user, a_item):
        want_u, want_i, want_du, want_di = R.stack_reference(a_user, a_item, u0, i0, gu, gi, L, leaky)
        np.testing.assert_allclose(got[0].cpu().numpy(), want_u, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got[1].cpu().numpy(), want_i, rtol=1e-4, atol=1e-4)
        scale = max(float(np.abs(want_du).max()), 1.0)
        np.testing.assert_allclose(got[2].cpu().numpy(), want_du, rtol=1e-4, atol=2e-6 * scale * L * 50)
        np.testing.assert_allclose(got[3].cpu().numpy(), want_di, rtol=1e-4, atol=2e-6 * scale * L * 50)

    got = run(batch, None, None)
    check(got, [[a] * L for a in sym], [[np.ascontiguousarray(a.T)] * L for a in sym])
    for a, b in zip(got, run(plans_u, plans_i, None)):                            # per interval: bit for bit
        assert torch.equal(a, b)
    # not the unnormalised stack
    plain_pairs = [graph.interval_pair(m, dev, tuning=TUNING) for m in mats]
    plain = run([a.plan for a, _ in plain_pairs], [t.plan for _, t in plain_pairs], None)
    assert not torch.equal(plain[0], got[0]) and not torch.equal(plain[2], got[2])
    # edge dropout on top: the masks of edge_drop_ref times the same weights, scaled by 1 / keep
    drop = ops.EdgeDrop(SEED, STEP, keep)
    scale = float(np.float32(1.0) / np.float32(keep))
    a_user = [[scale * sym[k] * D.dense_mask(SEED, STEP, k, l, 0, U, I, keep=keep) for l in range(L)] for k in range(T)]
    a_item = [[np.ascontiguousarray((scale * sym[k] * D.dense_mask(SEED, STEP, k, l, 1, U, I, keep=keep)).T)
               for l in range(L)] for k in range(T)]
    dropped = run(batch, None, drop)
    check(dropped, a_user, a_item)
    assert not torch.equal(dropped[0], got[0])
    for a, b in zip(dropped, run(plans_u, plans_i, drop)):
        assert torch.equal(a, b)


# ---- 5. the large-row-block instantiations ------------------------------------------------------------------------------
def test_large_row_block_variant_weighted(dev):
    """262,144 users: every launch takes the RPW = kRowsPerWave instantiation of its weighted kernel, per plan and
    batched, on rows of every class (the 4,096 item rows are all long)."""
    from sa_gnn_amd import graph, ops
    U, I, d, leaky, T, L = BIG_U, BIG_I, BIG_D, 0.5, 2, 2
    rng = np.random.default_rng(262145)
    mats = [_big_matrix(rng, [5, 9, 11]), sp.csr_matrix((U, I), dtype=np.intc)]
    pairs = [graph.interval_pair(m, dev, tuning=TUNING, norm="sym") for m in mats]
    plans_u, plans_i = [a.plan for a, _ in pairs], [t.plan for _, t in pairs]
    pu, pi = plans_u[0], plans_i[0]
    deg = np.diff(pu.rowptr.cpu().numpy())
    assert (deg == 0).any() and ((deg > 0) & (deg <= 4)).any() and ((deg > 4) & (deg <= 16)).any()
    assert pu.info.n_long_rows >= 1 and pu.info.n_chunks > pu.info.n_long_rows
    assert pi.info.n_long_rows == I and pi.info.n_chunks >= 2 * I
    assert plans_u[1].nnz == 1 and plans_i[1].nnz == 1 and pu.nnz == pi.nnz and pu.weighted and pi.weighted
    au = [R.sparse_sym(m) for m in mats]
    ai = [a.T.tocsr() for a in au]
    assert au[0].nnz == pu.nnz and au[0][2, 7] == np.float32(1.0 / np.sqrt(3.0 * ai[0][7].nnz))   # the merged duplicate
    u0 = rng.standard_normal((T, U, d)).astype(np.float32)
    i0 = rng.standard_normal((T, I, d)).astype(np.float32)
    u0_d, i0_d = torch.from_numpy(u0).to(dev), torch.from_numpy(i0).to(dev)
    # one product on each orientation, with a residual
    for plan, a, x, x_d, res, res_d in ((pu, au[0], i0[0], i0_d[0], u0[1], u0_d[1]), (pi, ai[0], u0[0], u0_d[0], i0[1], i0_d[1])):
        got = ops.spmm_ex(plan, x_d, leaky, residual=res_d, want_out=True)
        s = a @ x.astype(np.float64)
        assert_sum_close(got.cpu().numpy(), np.maximum(leaky * s, s) + res, abs(a) @ np.abs(x).astype(np.float64) + np.abs(res))
    # the batched stack, and each interval of it through the per-plan entry, bit for bit
    batch = ops.SpmmBatch(plans_u, plans_i)
    ou, oi = torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev)
    ops.gnn_stack(batch, u0_d, i0_d, L, leaky, ou, oi)
    want_u, want_i, terms_u, terms_i = _sparse_stack_reference(au, ai, u0, i0, L, leaky, None)   # w > 0: |w| = w
    assert_sum_close(ou.cpu().numpy(), want_u, terms_u)
    assert_sum_close(oi.cpu().numpy(), want_i, terms_i)
    for k in range(T):
        ku, ki = torch.empty((U, d), device=dev), torch.empty((I, d), device=dev)
        ops.gnn_interval(plans_u[k], plans_i[k], u0_d[k], i0_d[k], L, leaky, ku, ki)
        assert torch.equal(ku, ou[k]) and torch.equal(ki, oi[k])


# ---- 6. the Recommender -------------------------------------------------------------------------------------------------
def _sym_oracle_interval(u0, i0, adj_idx, tp_idx, n_layers, leaky):
    """O.torch_gnn_interval on the normalised dense matrices: the pattern is the index list's set of (user, item)."""
    p = np.zeros((u0.shape[0], i0.shape[0]), bool)
    p[np.asarray(adj_idx)[:, 0], np.asarray(adj_idx)[:, 1]] = True
    a = R.dense_sym_of_pattern(p)
    return R.torch_interval(torch.from_numpy(a), torch.from_numpy(np.ascontiguousarray(a.T)), u0, i0, n_layers, leaky)


def test_recommender_under_adj_norm_sym(dev, monkeypatch, tmp_path):
    from sa_gnn_amd import parallel
    from test_gpu_train import _oracle_params, _setup
    from sa_gnn_amd.Params import args as the_args
    monkeypatch.setattr(the_args, "adjNorm", "sym")
    monkeypatch.setattr(the_args, "evaluator", "host")
    monkeypatch.setattr(the_args, "edgeKeepRate", 1.0)
    rec, handler, NNs, args = _setup(dev, 32, 32, 1)
    assert args is the_args and all(a.plan.weighted for a in rec.subAdj + rec.subTpAdj)
    np.random.seed(3)
    batIds = np.random.permutation(args.user)[:args.batch]
    uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
    su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
    batch = {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si}
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in NNs.params.items()}
    # float64 autograd over the oracle's objective, its GNN stack normalised
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    monkeypatch.setattr(O, "torch_gnn_interval", _sym_oracle_interval)
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, batch, {"T": 2, "L": 2, "leaky": 0.5, "heads": 16})
    (opre + args.ssl_reg * ossl).backward()
    assert abs(float(pre.detach()) - float(opre.detach())) <= 1e-4 * max(abs(float(opre)), 1.0)
    assert abs(float(ssl.detach()) - float(ossl.detach())) <= 1e-4 * max(abs(float(ossl)), 1.0)
    checked = 0
    for name, leaf in leaves.items():        # the training-gradient tolerance of test_gpu_train.py
        got, want = grads[name], leaf.grad
        if want is None:
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        assert got is not None, f"no gradient reached {name}"
        a, b = got.cpu().double().numpy(), want.numpy()
        floor = max(5e-5 * np.abs(b).max(), 2e-5)
        if name.endswith("k_bias"):
            floor = max(floor, 1e-3 * float(leaves[name.replace("k_bias", "k_kernel")].grad.abs().max()))
        bad = np.abs(a - b) > 2e-4 * np.abs(b) + floor
        assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b)[bad].max():.3e} (scale {np.abs(b).max():.3e})"
        checked += 1
    assert checked >= 20

    # the device evaluator equals the host evaluator under sym
    fu_sym = rec.forward()[0].clone()
    np.random.seed(1)
    host = rec.testEpoch()
    monkeypatch.setattr(args, "evaluator", "device")
    np.random.seed(1)
    assert rec.testEpoch() == host
    monkeypatch.setattr(args, "evaluator", "host")

    # a checkpoint saved under sym does not load under none; a checkpoint without the key counts as none
    monkeypatch.setattr(args, "epoch", 1)
    monkeypatch.setattr(args, "save_path", "sym_ckpt")
    monkeypatch.setattr(args, "load_model", "sym_ckpt")
    rec.saveHistory(str(tmp_path))
    rec.loadModel(str(tmp_path))
    saved = {k: v.detach().clone() for k, v in NNs.params.items()}
    state = torch.load(str(tmp_path / "Models" / "sym_ckpt"), weights_only=True)
    assert state["adjNorm"] == "sym"
    monkeypatch.setattr(args, "adjNorm", "none")
    with pytest.raises(ValueError, match="adjNorm"):
        rec.loadModel(str(tmp_path))
    del state["adjNorm"]
    torch.save(state, str(tmp_path / "Models" / "sym_ckpt"))
    rec.loadModel(str(tmp_path))                                     # no key: none, which is this run's flag
    monkeypatch.setattr(args, "adjNorm", "sym")
    with pytest.raises(ValueError, match="adjNorm"):
        rec.loadModel(str(tmp_path))

    # the interval-parallel set-up refuses sym
    with pytest.raises(ValueError, match="adjNorm"):
        parallel.make_sharding(args.graphNum, 1, 0)

    # the same parameters in an unnormalised model: another forward()
    monkeypatch.setattr(args, "adjNorm", "none")
    rec.prepareModel()
    assert not any(a.plan.weighted for a in rec.subAdj + rec.subTpAdj)
    with torch.no_grad():
        for k, v in saved.items():
            NNs.params[k].copy_(v)
    fu_none = rec.forward()[0]
    assert fu_none.shape == fu_sym.shape and not torch.equal(fu_none, fu_sym)
    assert float((fu_none - fu_sym).abs().max()) > 1e-3 * float(fu_sym.abs().max())
