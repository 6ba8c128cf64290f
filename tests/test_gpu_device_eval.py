"""GPU suite: the device evaluator. sagnn_candidate_rank_f32 (through ops.candidate_rank) against the numpy
restatement of the rank rule on exact integer-valued data, its scores bit for bit against sagnn_pair_score_f32, its
independence of the batch, the head kernels' independence of the chunk a row sits in, and
Recommender.testEpoch / testEpochFull under --evaluator device against the host evaluator (equal dicts)."""
import numpy as np
import pytest
import torch

import candidate_rank_ref as R
from sa_gnn_amd import ops

pytestmark = pytest.mark.gpu


def _i32(dev, v):
    return torch.as_tensor(np.asarray(v, dtype=np.int32), device=dev)


def _f32(dev, v):
    return torch.as_tensor(np.asarray(v, dtype=np.float32), device=dev)


def _int_case(rng, B, C, d, n_users=40, n_items=300):
    """Small integers everywhere: every product and partial sum is exact in fp32, so the kernel's scores equal the
    float64 restatement and every tie is a real tie. Some U / I rows are NaN; targets have several copies, none
    (an id absent from the row) or are negative."""
    U = rng.integers(-2, 3, size=(n_users, d)).astype(np.float32)
    I = rng.integers(-2, 3, size=(n_items, d)).astype(np.float32)
    S = rng.integers(-2, 3, size=(B, d)).astype(np.float32)
    U[3] = np.nan
    I[[5, 17]] = np.nan
    uids = rng.integers(0, n_users, size=B)
    cand = rng.integers(0, min(n_items, 2 * C + 3), size=(B, C))              # few distinct ids: repeated copies
    target = cand[np.arange(B), rng.integers(0, C, size=B)]
    target[rng.random(B) < 0.15] = n_items + 7
    target[rng.random(B) < 0.1] = -1
    uids[0] = 3                                                               # a NaN user: every score NaN
    return U, I, S, uids, cand, target


@pytest.mark.parametrize("d", [4, 32, 64, 128, 256])
@pytest.mark.parametrize("C", [1, 7, 1000, 4096])
def test_ranks_equal_the_restatement(dev, d, C):
    rng = np.random.default_rng(d * 10007 + C)
    B = 37 if C < 4096 else 9
    U, I, S, uids, cand, target = _int_case(rng, B, C, d)
    rank, scores = ops.candidate_rank(_f32(dev, U), _f32(dev, I), _i32(dev, uids), _i32(dev, cand), _i32(dev, target),
                                      S=_f32(dev, S), A=_f32(dev, I), leaky=0.5, want_scores=True)
    want_s = R.head_scores(U, I, S, I, uids, cand, 0.5)
    np.testing.assert_array_equal(scores.cpu().numpy(), want_s.astype(np.float32))
    assert rank.dtype == torch.int64
    np.testing.assert_array_equal(rank.cpu().numpy(), R.rank_by_sort(want_s, cand, target))
    # without the head term
    rank2, sc2 = ops.candidate_rank(_f32(dev, U), _f32(dev, I), _i32(dev, uids), _i32(dev, cand), _i32(dev, target),
                                    want_scores=True)
    want2 = R.head_scores(U, I, np.zeros_like(S), I, uids, cand, 0.5)
    np.testing.assert_array_equal(sc2.cpu().numpy(), want2.astype(np.float32))
    np.testing.assert_array_equal(rank2.cpu().numpy(), R.rank_by_sort(want2, cand, target))


def test_ties_and_copies_at_minus_infinity(dev):
    """Hand-made rows: the best copy's tie rule, a copy behind equal scores, all copies NaN (rank among -inf)."""
    d = 4
    I = np.array([[1, 0, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0], [np.nan, 0, 0, 0], [-np.inf, 0, 0, 0], [3, 0, 0, 0]],
                 dtype=np.float32)
    U = np.array([[1, 0, 0, 0]], dtype=np.float32)
    cand = np.array([[0, 1, 2, 0, 5],        # target 0: copies at 0 and 3, both 1.0; 2 (score 1) ties before copy 3
                     [2, 0, 1, 5, 0],        # target 0: first copy at 1 ties with cand 2 at 0 -> rank 1 + (2, 5) = 3
                     [3, 4, 3, 1, 3],        # target 3: every copy NaN -> p = -inf; j < f = 0: none; > -inf: item 1
                     [4, 3, 1, 4, 3],        # target 3: NaN copies; f = 1; -inf at 0 counts, 1 above
                     [1, 1, 1, 1, 1]],       # target 0: no copy
                    dtype=np.int32)
    target = np.array([0, 0, 3, 3, 0], dtype=np.int32)
    rank, _ = ops.candidate_rank(_f32(dev, U), _f32(dev, I), _i32(dev, [0] * 5), _i32(dev, cand), _i32(dev, target))
    want = R.rank_by_sort(R.head_scores(U, I, np.zeros((5, d)), I, [0] * 5, cand, 1.0), cand, target)
    assert want.tolist() == [2, 3, 1, 2, -1]
    assert rank.cpu().numpy().tolist() == want.tolist()


@pytest.mark.parametrize("d", [4, 32, 64, 128, 256])
def test_scores_are_bit_identical_to_pair_score(dev, d):
    rng = np.random.default_rng(d)
    B, C, n_users, n_items = 29, 173, 50, 400
    U = torch.randn((n_users, d), device=dev) * 3
    I = torch.randn((n_items, d), device=dev) * 3
    S = torch.randn((B, d), device=dev) * 3
    uids = rng.integers(0, n_users, size=B)
    cand = rng.integers(0, n_items, size=(B, C))
    target = cand[:, -1]
    _, scores = ops.candidate_rank(U, I, _i32(dev, uids), _i32(dev, cand), _i32(dev, target), S=S, A=I, leaky=0.2,
                                   want_scores=True)
    ref = ops.pair_score(U, I, _i32(dev, np.repeat(uids, C)), _i32(dev, cand.reshape(-1)), S=S, A=I,
                         locs=_i32(dev, np.repeat(np.arange(B), C)), leaky=0.2)
    assert torch.equal(scores.reshape(-1).view(torch.int32), ref.view(torch.int32))


def test_rows_do_not_depend_on_the_batch(dev):
    rng = np.random.default_rng(11)
    d, B, C = 64, 50, 301
    U = torch.randn((80, d), device=dev)
    I = torch.randn((500, d), device=dev)
    S = torch.randn((B, d), device=dev)
    uids, cand = rng.integers(0, 80, size=B), rng.integers(0, 40, size=(B, C))    # ties of equal items: many copies
    target = cand[:, 5].copy()
    args = lambda rows: (_i32(dev, uids[rows]), _i32(dev, cand[rows]), _i32(dev, target[rows]))
    rank, sc = ops.candidate_rank(U, I, *args(np.arange(B)), S=S, A=I, leaky=0.3, want_scores=True)
    perm = rng.permutation(B)
    rank_p, sc_p = ops.candidate_rank(U, I, *args(perm), S=S[torch.as_tensor(perm, device=dev)].contiguous(), A=I,
                                      leaky=0.3, want_scores=True)
    assert torch.equal(rank[torch.as_tensor(perm, device=dev)], rank_p)
    assert torch.equal(sc[torch.as_tensor(perm, device=dev)].view(torch.int32), sc_p.view(torch.int32))
    for b in (0, 17, B - 1):
        r1, s1 = ops.candidate_rank(U, I, *args([b]), S=S[b:b + 1], A=I, leaky=0.3, want_scores=True)
        assert int(r1) == int(rank[b]) and torch.equal(s1[0].view(torch.int32), sc[b].view(torch.int32))
    # a candidate matrix with a row stride wider than C (a column slice) reads the same rows
    wide = _i32(dev, np.concatenate([cand, cand[:, :7]], axis=1))[:, :C]
    r_w, s_w = ops.candidate_rank(U, I, _i32(dev, uids), wide, _i32(dev, target), S=S, A=I, leaky=0.3, want_scores=True)
    assert torch.equal(r_w, rank) and torch.equal(s_w.view(torch.int32), sc.view(torch.int32))


# ---- the Recommender ------------------------------------------------------------------------------------------------
def _recommender(dev, pos_length, test_mode, seed=12):
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    rng = np.random.default_rng(seed)
    args.graphNum, args.gnn_layer, args.latdim, args.leaky, args.ssldim = 3, 2, 64, 0.5, 32
    args.att_layer, args.batch, args.pos_length, args.testSize, args.test, args.shoot = 2, 32, pos_length, 50, test_mode, 10
    args.sslNum, args.pred_num, args.keepRate, args.ssl_reg, args.reg = 3, 2, 1.0, 1e-3, 1e-4
    args.trnNum, args.lr, args.sampler, args.evaluator = 64, 5e-3, "host", "host"
    args.decay_step = args.trnNum // args.batch
    U, I = 150, 120
    tmt = synthetic.make_trn_mat_time(U, I, [1500, 1400, 1300])
    seq = synthetic.make_sequence(tmt)
    tst_int = [int(rng.integers(0, I)) if (u % 3 and len(seq[u])) else None for u in range(U)]
    test_dict = {u + 1: list(rng.integers(1, I + 1, size=60)) for u in range(U)}
    handler = DataHandler.from_memory(tmt, seq, tst_int, test_dict)
    rec = Recommender(dev, handler)
    rec.prepareModel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name in list(NNs.params):
            if name.endswith("bias") or name.endswith("beta") or name.endswith("Bias"):
                NNs.params[name].copy_(0.1 * torch.randn(NNs.params[name].shape, generator=g))
        for key in ("uEmbed", "iEmbed", "posEmbed"):
            NNs.params[key].mul_(30)
    return rec, handler, args


def _both(rec, args, full):
    fn = rec.testEpochFull if full else rec.testEpoch
    args.evaluator = "host"
    host = fn()
    args.evaluator = "device"
    try:
        device = fn()
    finally:
        args.evaluator = "host"
    return host, device


@pytest.mark.parametrize("pos_length", [12, 200])
def test_device_epochs_equal_the_host_epochs(dev, pos_length):
    rec, handler, args = _recommender(dev, pos_length, True)
    assert max(len(q) for q in handler.sequence) > 12                        # pos_length 12 cuts sequences
    for test_mode in (True, False):
        args.test = test_mode
        for full in (False, True):
            host, device = _both(rec, args, full)
            assert device == host, (test_mode, full, host, device)
            assert 0 < host["HR20"] <= 1
        E = rec._dev_eval[1]
        assert (E.target == (np.array([handler.tstInt[u] for u in E.users]) if test_mode else
                             np.array([handler.sequence[u][-1] for u in E.users]))).all()
    args.test = True                                                        # flipping back rebuilds the tables
    tables = rec._dev_eval[1]
    host, device = _both(rec, args, False)
    assert rec._dev_eval[1] is not tables and device == host
    # a training epoch moves the parameters: still equal; the host results do not depend on a device evaluation
    np.random.seed(0)
    torch.manual_seed(0)
    rec.trainEpoch()
    for full in (False, True):
        host, device = _both(rec, args, full)
        assert device == host, (full, host, device)
        args.evaluator = "host"
        assert (rec.testEpochFull() if full else rec.testEpoch()) == host
    args.evaluator = "host"


def test_head_kernels_do_not_depend_on_the_chunk(dev):
    """Each head kernel (the masked-sum SpMM, layernorm_td, mhsa_mean at t = 1, leaky_add) gives a row the same bits
    whatever else its launch holds: another order of the rows, fewer rows, more padding slots."""
    from sa_gnn_amd.Utils import NNLayers as NNs
    rec, handler, args = _recommender(dev, 200, True)
    rec.forward()
    assert args.att_layer == 2
    ids = np.asarray(handler.tstUsrs)[:40]
    seq, mask, _, _ = rec._test_sequences(ids[:32])                          # 32 of the users in 32 slots
    args.batch = 64
    seq64, mask64, _, _ = rec._test_sequences(ids)                           # all 40 in 64 slots
    args.batch = 32
    perm = np.random.default_rng(1).permutation(40)
    seq_p, mask_p = seq64.copy(), mask64.copy()
    seq_p[:40], mask_p[:40] = seq64[perm], mask64[perm]
    fi, pos = rec.final_item_vector, rec.posEmbed.detach()
    d = fi.shape[1]

    def stages(sequence, mask):
        """_head_att_plans one kernel at a time."""
        pi, pp = rec._masked_sum_plans(sequence, mask)
        B = len(sequence)
        ln = lambda x, gb: ops.layernorm_td(x.view(B, 1, d), gb[0].detach(), gb[1].detach()).view(B, d)
        out = {"spmm_items": ops.spmm(pi, fi, 1.0), "spmm_pos": ops.spmm(pp, pos, 1.0)}
        out["layernorm_items"] = ln(out["spmm_items"], rec.head_ln[0])
        out["layernorm_pos"] = ln(out["spmm_pos"], rec.head_ln[1])
        att = out["leaky_add"] = ops.leaky_add(out["layernorm_items"], out["layernorm_pos"], 1.0)
        for i, mh in enumerate(rec.multihead_self_attention_sequence):
            x = out[f"layernorm_{i}"] = ln(att, rec.head_ln[2 + i])
            a1 = out[f"mhsa_mean_{i}"] = mh.attention_mean(x.view(B, 1, d)).reshape(B, d)
            att = out[f"leaky_add_{i}"] = ops.leaky_add(a1, att, NNs.leaky)
        assert torch.equal(att.view(torch.int32), rec._head_att(sequence, mask).view(torch.int32))
        return out

    bits = lambda t: t.contiguous().view(torch.int32).cpu().numpy()
    base = {k: bits(v) for k, v in stages(seq64, mask64).items()}
    part = {k: bits(v) for k, v in stages(seq, mask).items()}                # rows 0..31 of the 40 in 32 slots
    shuf = {k: bits(v) for k, v in stages(seq_p, mask_p).items()}
    for k in base:
        assert np.array_equal(part[k], base[k][:32]), k
        assert np.array_equal(shuf[k][:40], base[k][perm]), k
