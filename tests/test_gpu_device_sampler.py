"""GPU suite: the device sampler (sagnn_sample_train_i32 / sagnn_sample_ssl_i32 through
Recommender.sample_batch_device) and the head's segment sums (sagnn_seq_sum_f32 / _bwd through SeqSumFn):
bit-exact against the numpy restatement, the reference's contracts, distributions, per-user independence, the loss
and its gradients against the host-sampled form and the oracle, and whole epochs with --sampler device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.stats import chisquare

import device_sampler_ref as R

pytestmark = pytest.mark.gpu

I_TOY, P_TOY, PRED_TOY, SSL_TOY = 30, 6, 5, 3


def _toy_handler():
    """Hand-made users: n_pos 0..4 (users 0-4), n_pos 11 > pos_length with its test item inside the seen set (5),
    exactly one allowed negative (6), a 4-item allowed set (7), hi = pred_num + 1 with distinct items (8), random
    users after that. subMat row 5 of interval 0 holds a duplicated entry and an explicit zero; row 9 of interval 1
    holds 7 distinct items."""
    from sa_gnn_amd.DataHandler import DataHandler
    rng = np.random.default_rng(5)
    I = I_TOY
    seqs = [[3], [4, 5], [1, 2, 3], [7, 8, 9, 10], [11, 12, 13, 14, 15], rng.permutation(12).tolist(),
            [i for i in rng.permutation(I).tolist() if i != 17], rng.permutation(I)[:25].tolist(), list(range(10, 25))]
    seqs += [rng.integers(0, I, size=int(rng.integers(5, 20))).tolist() for _ in range(7)]
    U = len(seqs)
    unseen7 = next(i for i in range(I) if i not in seqs[7])
    tst = [None, 20, None, 0, 29, 4, None, unseen7, 2] + [int(rng.integers(0, I)) if u % 2 else None for u in range(9, U)]
    subs = []
    for k in range(2):
        rows = [rng.choice(I, size=int(rng.integers(0, 9)), replace=False).tolist() for _ in range(U)]
        data = [[1] * len(r) for r in rows]
        if k == 0:
            rows[5], data[5] = [6, 2, 6, 9, 1], [1, 3, 1, 0, 2]          # 6 twice, an explicit zero at 9
        else:
            rows[9], data[9] = [0, 3, 5, 8, 13, 21, 27], [1] * 7
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        subs.append(sp.csr_matrix((np.concatenate(data).astype(np.intc), np.concatenate(rows).astype(np.int32), indptr),
                                  shape=(U, I)))
    return DataHandler.from_memory([sp.csr_matrix((U, I)), subs, None], seqs, tst, None)


@pytest.fixture
def toy(dev):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    h = _toy_handler()
    args.batch, args.pos_length, args.pred_num, args.sslNum = 20, P_TOY, PRED_TOY, SSL_TOY
    rec = Recommender.__new__(Recommender)
    rec.handler, rec.device = h, dev
    return rec, h, args


def _np(t):
    return t.cpu().numpy().astype(np.int64) if t.dtype in (torch.int32, torch.int64) else t.cpu().numpy()


def test_exact_against_the_numpy_restatement(toy):
    rec, h, args = toy
    assert h.subMat[0].indptr[6] - h.subMat[0].indptr[5] == 5                 # stored as given: duplicate and zero
    U = len(h.sequence)
    for seed, step, bat in ((0x1234ABCD5678, 7, np.random.default_rng(0).permutation(U)),
                            ((1 << 64) - 12345, 123456, np.arange(U)[::-1][:11])):
        got = rec.sample_batch_device(bat, seed, step)
        want = R.sample_train(h, I_TOY, bat, args.batch, 40, PRED_TOY, P_TOY, seed, step)
        for name, w in zip(("uids", "iids", "uLocs_seq"), want[:3]):
            assert _np(got[name]).tolist() == w.tolist(), name
        assert _np(got["seq_seg"][0]).tolist() == want[3].tolist()
        assert _np(got["seq_seg"][1]).tolist() == want[4].tolist()
        ssl = R.sample_ssl(h, bat, SSL_TOY, seed, step)
        for k, (su, si, _) in enumerate(ssl):
            assert _np(got["suids"][k]).tolist() == su.tolist(), k
            assert _np(got["siids"][k]).tolist() == si.tolist(), k
        # the cases the toy set is built to cover
        seg_len = _np(got["seq_seg"][1])
        assert (seg_len[len(bat):] == 0).all() and seg_len.max() == P_TOY
        iids, n = _np(got["iids"]), len(_np(got["iids"])) // 2
        if 6 in bat:
            assert (iids[n:][_np(got["uids"])[n:] == 6] == 17).all()          # the one allowed item
        if 5 in bat:
            rows = _np(got["siids"][0])[_np(got["suids"][0]) == 5]
            assert set(rows.tolist()) <= {1, 2, 6} and 9 not in rows


def test_contracts_on_a_gowalla_shaped_batch(dev):
    """tests/test_host.py::test_sampler_invariants on the device sampler, plus the host sampler's per-user counts."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    U, I = 6000, 7000
    tmt = synthetic.make_trn_mat_time(U, I, [60000, 55000, 50000])
    seq = synthetic.make_sequence(tmt)
    rng = np.random.default_rng(2)
    tst = [int(rng.integers(0, I)) if u % 3 else None for u in range(U)]
    h = DataHandler.from_memory(tmt, seq, tst, None)
    args.graphNum, args.batch, args.pos_length, args.sslNum, args.pred_num = 3, 512, 200, 40, 5
    rec = Recommender.__new__(Recommender)
    rec.handler, rec.device = h, dev
    bat = rng.permutation(U)[:500]
    b = rec.sample_batch_device(bat, 99, 3)
    uids, iids, locs = _np(b["uids"]), _np(b["iids"]), _np(b["uLocs_seq"])
    n = len(uids) // 2
    assert n > 0 and (uids[:n] == uids[n:]).all() and (locs[:n] == locs[n:]).all() and (bat[locs] == uids).all()
    neg = iids[n:]
    assert (np.asarray(h.trnMat[uids[n:], neg]).ravel() == 0).all()
    assert all(neg[e] != seq[uids[e]][-1] and neg[e] != tst[uids[e]] for e in range(n))
    assert all(iids[e] in seq[uids[e]][:-1][-(args.pred_num + 1):] for e in range(n))
    seg_begin, seg_len = _np(b["seq_seg"][0]), _np(b["seq_seg"][1])
    flat = np.concatenate([np.asarray(q) for q in seq])
    assert (flat[seg_begin[locs[:n]] + seg_len[locs[:n]]] == iids[:n]).all()   # a segment ends right before the positive
    assert (seg_len <= args.pos_length).all() and (seg_len[len(bat):] == 0).all()
    np.random.seed(0)
    _, _, _, _, uL_h = rec.sampleTrainBatch(bat, h.trnMat, None, 40, as_arrays=True)
    assert np.bincount(locs[:n], minlength=len(bat)).tolist() == np.bincount(uL_h[:len(uL_h) // 2], minlength=len(bat)).tolist()
    su_h, _, sl_h = rec.sampleSslBatch(bat, h.subMat, False, as_arrays=True)
    for k in range(3):
        su, si = _np(b["suids"][k]), _np(b["siids"][k])
        assert len(su) % 2 == 0 and (su[0::2] == su[1::2]).all()
        assert (np.asarray(h.subMat[k][su, si]).ravel() != 0).all()
        assert np.bincount(np.searchsorted(np.sort(bat), su), minlength=len(bat)).tolist() == \
            np.bincount(np.searchsorted(np.sort(bat), np.asarray(su_h[k])), minlength=len(bat)).tolist()


def test_distributions(toy):
    """Fixed seed, many steps: negatives of user 7 (4 allowed items), `choose` of user 8 (hi = 6), SSL draws of
    user 9 in interval 1 (7 items) are uniform (chi-square, p > 1e-4; deterministic since the seed is fixed)."""
    rec, h, args = toy
    allowed7 = sorted(set(range(I_TOY)) - set(h.sequence[7]) - {h.tstInt[7]})
    assert len(allowed7) == 4
    negs, pos8, ssl9 = [], [], []
    for step in range(1500):
        b = rec.sample_batch_device([7, 8, 9], 2024, step)
        uids, iids = _np(b["uids"]), _np(b["iids"])
        n = len(uids) // 2
        negs.append(iids[n:][uids[n:] == 7])
        pos8.append(iids[:n][uids[:n] == 8][0])
        su, si = _np(b["suids"][1]), _np(b["siids"][1])
        ssl9.append(si[su == 9])
    negs, ssl9 = np.concatenate(negs), np.concatenate(ssl9)
    choose = len(h.sequence[8]) - 1 - np.asarray(pos8) + 10          # posset[-choose] = 10 + n_pos - choose
    assert set(negs.tolist()) == set(allowed7) and set(choose.tolist()) == set(range(1, 7))
    assert set(ssl9.tolist()) == {0, 3, 5, 8, 13, 21, 27}
    for x, cats in ((negs, allowed7), (choose, range(1, 7)), (ssl9, [0, 3, 5, 8, 13, 21, 27])):
        counts = [(x == c).sum() for c in cats]
        assert chisquare(counts).pvalue > 1e-4, counts


def test_a_users_draws_do_not_depend_on_the_batch(toy):
    rec, h, args = toy

    def draws(b, u, slot):
        uids, iids, locs = _np(b["uids"]), _np(b["iids"]), _np(b["uLocs_seq"])
        n = len(uids) // 2
        s0, sl = _np(b["seq_seg"][0])[slot], _np(b["seq_seg"][1])[slot]
        out = [iids[:n][uids[:n] == u].tolist(), iids[n:][uids[n:] == u].tolist(), int(sl),
               _np(rec._device_sampler().seq_items)[s0:s0 + sl].tolist()]
        out += [_np(b["siids"][k])[_np(b["suids"][k]) == u].tolist() for k in range(2)]
        assert (locs[:n][uids[:n] == u] == slot).all()
        return out

    a = rec.sample_batch_device([5, 9, 2, 7], 77, 11)
    b = rec.sample_batch_device([11, 7, 0, 3, 5, 14], 77, 11)
    c = rec.sample_batch_device([7, 5], 77, 12)
    assert draws(a, 5, 0) == draws(b, 5, 4) and draws(a, 7, 3) == draws(b, 7, 1)
    assert draws(a, 7, 3)[1] != draws(c, 7, 0)[1]                      # 24 negatives over 4 items: a new step differs
    assert draws(a, 5, 0) != draws(c, 5, 1)


def _host_form(rec, b, args):
    """A device batch in the host samplers' format: lists + dense sequence / mask [args.batch, pos_length]."""
    flat = _np(rec._device_sampler().seq_items)
    P = args.pos_length
    seg_begin, seg_len = _np(b["seq_seg"][0]), _np(b["seq_seg"][1])
    sequence = np.zeros((args.batch, P), dtype=np.int64)
    mask = np.zeros((args.batch, P), dtype=np.float32)
    for s in range(args.batch):
        L = int(seg_len[s])
        if L:
            sequence[s, P - L:] = flat[seg_begin[s]:seg_begin[s] + L]
            mask[s, P - L:] = 1
    lst = lambda t: _np(t).tolist()
    return {"uids": lst(b["uids"]), "iids": lst(b["iids"]), "uLocs_seq": lst(b["uLocs_seq"]), "sequence": sequence,
            "mask": mask, "suids": [lst(t) for t in b["suids"]], "siids": [lst(t) for t in b["siids"]]}


def test_loss_matches_the_host_form_and_the_oracle(dev):
    from oracle import selfgnn_oracle as O
    from test_gpu_train import _oracle_params, _setup
    rec, handler, NNs, args = _setup(dev, 64, 48, 2)                 # pos_length 12: every segment is a short row
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = rec.sample_batch_device(bat, 31337, 2)
    hb = _host_form(rec, b, args)
    params = {k: p for k, p in NNs.params.items() if p.requires_grad}
    grads = []
    for batch in (b, hb):
        for p in params.values():
            p.grad = None
        pre, ssl = rec.train_loss(batch, keep_rate=1.0)
        (pre + args.ssl_reg * ssl).backward()
        grads.append(({k: None if p.grad is None else p.grad.detach().clone() for k, p in params.items()}, pre, ssl))
    (gd, pre_d, ssl_d), (gh, pre_h, ssl_h) = grads
    # the head's sums: ascending from 0.0f over rows of <= 16 entries, equal to the CSR SpMM's bit for bit
    from sa_gnn_amd import ops
    fi = rec.forward()[1]
    seq_d, pos_d = ops.seq_sum(fi, rec.posEmbed.detach(), rec._device_sampler().seq_items, *b["seq_seg"])
    pi, pp = rec._masked_sum_plans(hb["sequence"], hb["mask"])
    assert torch.equal(seq_d, ops.spmm(pi, fi, 1.0)) and torch.equal(pos_d, ops.spmm(pp, rec.posEmbed.detach(), 1.0))
    # the losses themselves are reduced with float atomics (sagnn_hinge_f32): equal up to the order of that sum
    for x, y in ((pre_d, pre_h), (ssl_d, ssl_h)):
        assert abs(float(x.detach()) - float(y.detach())) <= 1e-6 * max(abs(float(y.detach())), 1.0)
    for k in params:
        if gh[k] is None:
            assert gd[k] is None or float(gd[k].abs().max()) == 0.0, k
            continue
        a, w = gd[k].cpu().double().numpy(), gh[k].cpu().double().numpy()
        floor = 1e-5 * np.abs(w).max()
        if k.endswith("k_bias"):       # analytically ~0: what is left is run-to-run noise of the key kernel's terms
            floor = max(floor, 1e-3 * float(gh[k.replace("k_bias", "k_kernel")].abs().max()))
        assert np.all(np.abs(a - w) <= 1e-4 * np.abs(w) + floor), k
    # the converted batch through the oracle: every leaf gradient of the device-sampled step (fi and posEmbed among
    # the inputs of the masked sums) within tests/test_gpu_train.py's tolerances
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    opre, ossl, _, _ = O.torch_train_loss(P, adj, tp, hb, {"T": 2, "L": 2, "leaky": 0.5, "heads": 16})
    (opre + args.ssl_reg * ossl).backward()
    assert abs(float(pre_d) - float(opre)) <= 1e-4 * max(abs(float(opre)), 1.0)
    for name in ("posEmbed", "iEmbed", "uEmbed"):
        a, w = gd[name].cpu().double().numpy(), leaves[name].grad.numpy()
        tol = 2e-4 * np.abs(w) + max(5e-5 * np.abs(w).max(), 2e-5)
        assert not (np.abs(a - w) > tol).any(), name


def test_seq_sum_against_the_csr_spmm(dev):
    """pos_length 200: segments of up to 200 items against the per-batch CSR SpMM (bit for bit on rows of <= 16
    entries, the SpMM's short class; reordered sums beyond), and the backward against float64."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(8)
    n_items, d, P, B, n_flat = 500, 64, 200, 96, 6000
    fi = torch.from_numpy(rng.standard_normal((n_items, d)).astype(np.float32)).to(dev)
    pe = torch.from_numpy(rng.standard_normal((P, d)).astype(np.float32)).to(dev)
    flat = rng.integers(0, n_items, n_flat).astype(np.int32)
    seg_len = np.concatenate([np.arange(0, 20), rng.integers(0, P + 1, B - 20)]).astype(np.int32)
    seg_begin = rng.integers(0, n_flat - P, B).astype(np.int64)
    args_d = [torch.from_numpy(a).to(dev) for a in (flat, seg_begin, seg_len)]
    seq_tok, pos_tok = ops.seq_sum(fi, pe, *args_d)
    rowptr = np.concatenate([[0], np.cumsum(seg_len)]).astype(np.int32)
    items = np.concatenate([flat[a:a + n] for a, n in zip(seg_begin, seg_len)]).astype(np.int32)
    pos = np.concatenate([np.arange(P - n, P) for n in seg_len]).astype(np.int32)
    want_s = ops.spmm(ops.SpmmPlan(rowptr, items, B, n_items, device=dev), fi, 1.0)
    want_p = ops.spmm(ops.SpmmPlan(rowptr, pos, B, P, device=dev), pe, 1.0)
    short = torch.from_numpy(seg_len <= 16).to(dev)
    assert torch.equal(seq_tok[short], want_s[short]) and torch.equal(pos_tok[short], want_p[short])
    torch.testing.assert_close(seq_tok, want_s, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(pos_tok, want_p, rtol=1e-5, atol=1e-4)
    g_s = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(dev)
    g_p = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(dev)
    d_fi, d_pos = ops.seq_sum_bwd(g_s, g_p, *args_d, n_items, P)
    _, d_pos2 = ops.seq_sum_bwd(g_s, g_p, *args_d, n_items, P)
    assert torch.equal(d_pos, d_pos2)                                         # no atomics on this side
    gs, gp = g_s.cpu().double().numpy(), g_p.cpu().double().numpy()
    want_fi, want_pos = np.zeros((n_items, d)), np.zeros((P, d))
    for b in range(B):
        np.add.at(want_fi, flat[seg_begin[b]:seg_begin[b] + seg_len[b]], gs[b])
        want_pos[P - seg_len[b]:] += gp[b]
    np.testing.assert_allclose(d_fi.cpu().numpy(), want_fi, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(d_pos.cpu().numpy(), want_pos, rtol=1e-5, atol=1e-4)


def test_train_epochs_with_the_device_sampler(dev):
    from test_gpu_train import _setup
    rec, handler, NNs, args = _setup(dev, 64, 32, 1)
    args.trnNum, args.lr, args.keepRate, args.ssl_reg, args.reg = 64, 5e-3, 0.5, 1e-3, 1e-4
    args.decay_step = args.trnNum // args.batch
    np.random.seed(0)
    torch.manual_seed(0)
    trainable = {k: p for k, p in NNs.params.items() if p.requires_grad}
    before = {k: p.detach().clone() for k, p in trainable.items()}
    args.sampler = "device"
    try:
        res = [rec.trainEpoch() for _ in range(2)]
    finally:
        args.sampler = "host"
    assert all(np.isfinite(r["Loss"]) and np.isfinite(r["preLoss"]) for r in res)
    still = [k for k, p in trainable.items() if torch.equal(p.detach(), before[k])]
    assert not still, f"Adam left {still[:5]} unchanged"
