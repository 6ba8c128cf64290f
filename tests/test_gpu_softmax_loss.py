"""GPU suite of the opt-in full-catalogue softmax loss (--predLoss softmax): sagnn_softmax_loss_f32 and
its backward against the float64 restatement of softmax_loss_ref, their contracts (row independence, bit-identical
runs, skipped rows), then the loss inside the Recommender (training objective under both heads, both batch forms,
epochs, checkpoints) and the untouched default.

Tolerances (softmax_loss_ref.tolerance_terms): the form is derived, the constants are measured. Each K is 4 x the worst
ratio that plain float32 torch on the CPU reaches against float64 in the same units, rounded up to a power of two
(tools/measure_softmax_loss_tolerance.py: nq 7-40, n_items 17-52,619, d 32-128, input scale 0.5-2, temperature
0.125-4). Measured worst float32-CPU ratios: lse 2.20, dQ 6.66, dI 5.66."""
import ctypes

import numpy as np
import pytest
import torch

import softmax_loss_ref as R
from oracle import selfgnn_oracle as O

pytestmark = pytest.mark.gpu

K_LSE, K_DQ, K_DI = 16, 32, 32      # 4 x (2.20, 6.66, 5.66), rounded up to powers of two
CFG = {"T": 2, "L": 2, "leaky": 0.5, "heads": 16}


def _lists(rng, nq, ni, n_lists=None):
    """Random ascending exclusion lists with duplicates on about 2 % of the items (at least one entry each)."""
    n_lists = nq if n_lists is None else n_lists
    lists = [np.sort(rng.integers(0, ni, max(1, ni // 50))) for _ in range(n_lists)]
    lists = [np.sort(np.concatenate([v, v[:2]])) for v in lists]                       # duplicated ids
    return np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64), np.concatenate(lists).astype(np.int32)


def _run(dev, Q, I, target, inv_temp, scale, ptr=None, items=None, rows=None, g=1.0):
    from sa_gnn_amd import ops
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    Qd = Q if isinstance(Q, torch.Tensor) else t(Q, np.float32)
    Id, tg = t(I, np.float32), t(target, np.int32)
    excl = None if ptr is None else (t(ptr, np.int64), t(items, np.int32) if len(items) else torch.zeros(1, dtype=torch.int32, device=dev))
    rd = t(rows, np.int32)
    loss, lse, ts = ops.softmax_loss(Qd, Id, tg, inv_temp, scale, excl, rd)
    gd = torch.full((1,), g, dtype=torch.float32, device=dev)
    dQ, dI = ops.softmax_loss_bwd(Qd, Id, tg, lse, gd, inv_temp, scale, excl, rd)
    torch.cuda.synchronize()
    return {"loss": float(loss), "lse": lse.cpu().numpy(), "tscore": ts.cpu().numpy(), "dQ": dQ.cpu().numpy(), "dI": dI.cpu().numpy()}


def _check(got, Q, I, target, inv_temp, scale, ptr=None, items=None, rows=None, name=""):
    """Every output against float64 under the derived bounds; prints the K each output needs before it asserts."""
    ref = R.softmax_loss_np(Q, I, target, inv_temp, scale, ptr, items, rows)
    terms = R.tolerance_terms(Q, I, target, ref, inv_temp, scale)
    need = {k: R.worst_ratio(got[k], ref[k], *terms[k]) for k in ("lse", "dQ", "dI")}
    # the target's score is one dot product: eps32 sum |q e|, which A bounds (A is that sum's maximum times inv_temp)
    ts_unit = terms["lse"][0] / inv_temp
    need["tscore"] = R.worst_ratio(got["tscore"], ref["tscore"], ts_unit, 0.0)
    loss_tol = abs(scale) * (2 * K_LSE * terms["lse"][0]).sum() + 4 * R.EPS32 * abs(ref["loss"])
    print(f"{name}: K needed lse {need['lse']:.2f} / {K_LSE}, tscore {need['tscore']:.2f} / {K_LSE}, dQ {need['dQ']:.2f} / {K_DQ}, "
          f"dI {need['dI']:.2f} / {K_DI}; loss {got['loss']!r} vs {ref['loss']!r} (tol {loss_tol:.3e})")
    for k in ("lse", "tscore", "dQ", "dI"):
        assert np.isfinite(got[k]).all(), f"{name}: {k} holds inf or NaN"
    assert need["lse"] <= K_LSE and need["tscore"] <= K_LSE and need["dQ"] <= K_DQ and need["dI"] <= K_DI, (name, need)
    assert np.isfinite(got["loss"]) and abs(got["loss"] - ref["loss"]) <= loss_tol, name
    return ref


SHAPES = [(ni, nq, d) for d in (32, 64, 128) for ni, nq in ((1, 1), (17, 7), (4099, 17), (4099, 40))] + [(52619, 33, 64)]


@pytest.mark.parametrize("temp", [1.0, 0.25])
@pytest.mark.parametrize("ni,nq,d", SHAPES)
def test_forward_and_both_gradients_against_float64(dev, ni, nq, d, temp):
    rng = np.random.default_rng(1000 * d + ni + nq)
    Q = (rng.standard_normal((nq, d)) * 0.7).astype(np.float32)
    I = (rng.standard_normal((ni, d)) * 0.7).astype(np.float32)
    target = rng.integers(0, ni, nq)
    by_row = temp != 1.0                                           # one temperature through excl_row, one through list b
    ptr, items = _lists(rng, nq, ni, nq + 3 if by_row else None)
    rows = rng.integers(0, nq + 3, nq) if by_row else None
    scale, g = 1.0 / nq, 0.5                                       # an upstream gradient other than 1
    got = _run(dev, Q, I, target, 1.0 / temp, scale, ptr, items, rows, g=g)
    got["dQ"], got["dI"] = got["dQ"] / g, got["dI"] / g            # exact: g is a power of two
    _check(got, Q, I, target, 1.0 / temp, scale, ptr, items, rows, name=f"ni {ni} nq {nq} d {d} temp {temp}")


def test_zero_queries_count_the_distinct_eligible_items(dev):
    """Q = 0: lse[b] = ln(number of distinct eligible items): the ragged last tile, the chunk seams (multiples of 128)
    and duplicated exclusion ids all show up as a wrong count."""
    ni, nq, d = 4099, 40, 64
    rng = np.random.default_rng(5)
    I = rng.standard_normal((ni, d)).astype(np.float32)
    Q = np.zeros((nq, d), np.float32)
    target = rng.integers(0, ni, nq)
    lists = []
    for b in range(nq):
        seam = 128 * rng.integers(1, 32)
        v = np.concatenate([rng.integers(0, ni, 60), np.arange(seam - 3, seam + 3), [ni - 1, ni - 1, ni - 2, 0], [target[b]] * (b % 2)])
        lists.append(np.sort(v))
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
    items = np.concatenate(lists)
    got = _run(dev, Q, I, target, 1.0, 1.0 / nq, ptr, items)
    count = np.array([ni - len(np.setdiff1d(np.unique(lists[b]), [target[b]])) for b in range(nq)])
    err = np.abs(got["lse"] - np.log(count))
    print(f"worst |lse - ln(count)| {err.max():.3e}, bound {K_LSE * R.EPS32:.3e}")
    assert (err <= K_LSE * R.EPS32).all()                          # A_b = 0
    assert (np.rint(np.exp(got["lse"].astype(np.float64))) == count).all()
    _check(got, Q, I, target, 1.0, 1.0 / nq, ptr, items, name="Q = 0")


@pytest.mark.parametrize("d", [32, 64, 128])
def test_integer_data_gives_the_exact_target_score(dev, d):
    ni, nq = 4099, 40
    rng = np.random.default_rng(d)
    Q, I = rng.integers(-3, 4, (nq, d)).astype(np.float32), rng.integers(-3, 4, (ni, d)).astype(np.float32)
    target = rng.integers(0, ni, nq)
    target[:3] = [0, ni - 1, 4096]                                 # first row, last row, the ragged tile
    got = _run(dev, Q, I, target, 0.125, 1.0 / nq)
    want = (Q.astype(np.float64) * I[target].astype(np.float64)).sum(1)
    assert (got["tscore"].astype(np.float64) == want).all()
    _check(got, Q, I, target, 0.125, 1.0 / nq, name=f"integers d {d}")


def test_rows_that_exclude_whole_chunks_everything_or_their_target(dev):
    ni, nq, d = 4099, 19, 64
    rng = np.random.default_rng(8)
    Q, I = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32)
    target = rng.integers(0, ni, nq)
    target[0], target[1], target[2], target[3] = 3000, 1000, 77, 4098
    lists = [np.sort(rng.integers(0, ni, 40)) for _ in range(nq)]
    lists[0] = np.arange(0, 2048)                                  # whole chunks without an eligible item
    lists[1] = np.arange(0, 2048)                                  # ... but for the target inside them
    lists[2] = np.arange(0, ni)                                    # everything but the target
    lists[3] = np.arange(0, ni)                                    # the same with the target in the last, ragged tile
    lists[4] = np.sort(np.concatenate([lists[4], [target[4]] * 2]))        # its own target: still counts
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
    items = np.concatenate(lists)
    got = _run(dev, Q, I, target, 1.0, 1.0, ptr, items)
    ref = _check(got, Q, I, target, 1.0, 1.0, ptr, items, name="sharp exclusions")
    terms = R.tolerance_terms(Q, I, target, ref, 1.0, 1.0)
    for b in (2, 3):                                               # p(target) = 1: no loss, no gradient, to the tolerance
        assert abs(got["lse"][b] - got["tscore"][b]) <= 2 * K_LSE * terms["lse"][0][b]
        assert (np.abs(got["dQ"][b]) <= K_DQ * terms["dQ"][0][b] + terms["dQ"][1][b]).all()
    assert ref["p"][4, target[4]] > 0 and ref["eligible"][4, target[4]]


def test_logits_beyond_the_exp_range_of_float32(dev):
    ni, nq, d = 4099, 17, 64
    rng = np.random.default_rng(9)
    Q, I = (rng.standard_normal((nq, d)) * 3).astype(np.float32), (rng.standard_normal((ni, d)) * 3).astype(np.float32)
    target = rng.integers(0, ni, nq)
    ptr, items = _lists(rng, nq, ni)
    z = (Q.astype(np.float64) @ I.T.astype(np.float64)) * 2.0
    assert np.abs(z).max() > 200 and z.max() > 200 and z.min() < -200
    got = _run(dev, Q, I, target, 2.0, 1.0 / nq, ptr, items)
    _check(got, Q, I, target, 2.0, 1.0 / nq, ptr, items, name="|z| > 200")


@pytest.mark.parametrize("skip_all", [False, True])
def test_rows_without_a_target_are_skipped(dev, skip_all):
    ni, nq, d = 4099, 40, 32
    rng = np.random.default_rng(10)
    Q, I = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32)
    target = rng.integers(0, ni, nq)
    skipped = np.arange(nq) if skip_all else np.array([0, 5, 15, 16, 17, 39])
    target[skipped] = -1
    if not skip_all:
        target[5] = ni                                             # just past the table: skipped as well
    ptr, items = _lists(rng, nq, ni)
    got = _run(dev, Q, I, target, 1.0, 1.0 / nq, ptr, items)
    for k in ("lse", "tscore", "dQ"):
        assert not got[k][skipped].any(), k
    if skip_all:
        assert got["loss"] == 0.0 and not got["dI"].any()
    else:
        _check(got, Q, I, target, 1.0, 1.0 / nq, ptr, items, name="some rows skipped")


def _t(dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)


@pytest.mark.parametrize("padded", [False, True])
def test_a_rows_outputs_do_not_depend_on_the_batch(dev, padded):
    """lse, tscore and the dQ row of row b, bit for bit, in a call of 40 rows and in a call of that row alone."""
    from sa_gnn_amd import ops
    ni, nq, d = 4099, 40, 64
    rng = np.random.default_rng(11)
    Q, I = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32)
    target = rng.integers(0, ni, nq)
    ptr, items = _lists(rng, nq, ni)
    rows = rng.permutation(nq)
    Id, tg, rd = _t(dev, I, np.float32), _t(dev, target, np.int32), _t(dev, rows, np.int32)
    excl = (_t(dev, ptr, np.int64), _t(dev, items, np.int32))
    Qd = _t(dev, Q, np.float32)
    if padded:                                                     # the same rows at a stride of d + 12
        buf = torch.full((nq, d + 12), 7.0, dtype=torch.float32, device=dev)
        buf[:, :d] = Qd
        Qd = buf[:, :d]
    g = torch.ones(1, dtype=torch.float32, device=dev)
    scale = 0.5                                                    # the same scale in both calls: scale is an input
    _, lse, ts = ops.softmax_loss(Qd, Id, tg, 1.0, scale, excl, rd)
    dQ, _ = ops.softmax_loss_bwd(Qd, Id, tg, lse, g, 1.0, scale, excl, rd)
    for b in (0, 15, 16, 23, 39):
        q1 = _t(dev, Q[b:b + 1], np.float32)
        _, lse1, ts1 = ops.softmax_loss(q1, Id, tg[b:b + 1].contiguous(), 1.0, scale, excl, rd[b:b + 1].contiguous())
        dQ1, _ = ops.softmax_loss_bwd(q1, Id, tg[b:b + 1].contiguous(), lse1, g, 1.0, scale, excl, rd[b:b + 1].contiguous())
        assert torch.equal(lse1, lse[b:b + 1]) and torch.equal(ts1, ts[b:b + 1]) and torch.equal(dQ1[0], dQ[b]), b


def test_two_runs_are_bit_identical(dev):
    ni, nq, d = 4099, 40, 128
    rng = np.random.default_rng(12)
    Q, I = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32)
    target = rng.integers(0, ni, nq)
    ptr, items = _lists(rng, nq, ni)
    a = _run(dev, Q, I, target, 0.5, 1.0 / nq, ptr, items)
    b = _run(dev, Q, I, target, 0.5, 1.0 / nq, ptr, items)
    assert a["loss"] == b["loss"]
    for k in ("lse", "tscore", "dQ", "dI"):
        assert np.array_equal(a[k], b[k]), k


# ---- the Recommender under --predLoss softmax ----------------------------------------------------------------------
def _setup(dev, monkeypatch, d=64, ssldim=48, att_layer=2, loss="softmax", temp=1.0, seq_att="sum"):
    """test_gpu_train.py's toy model (70 users, 60 items, 2 intervals) under the given loss flags."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.Utils import NNLayers as NNs
    from sa_gnn_amd.model import Recommender
    for k, v in (("predLoss", loss), ("softmaxTemp", temp), ("seqAtt", seq_att), ("evaluator", "host"), ("sampler", "host"),
                 ("fusion_rows", "all"), ("edgeKeepRate", 1.0), ("adjNorm", "none"), ("graphNum", 2), ("gnn_layer", 2),
                 ("latdim", d), ("leaky", 0.5), ("ssldim", ssldim), ("att_layer", att_layer), ("batch", 16), ("pos_length", 12),
                 ("testSize", 20), ("test", True), ("sslNum", 3), ("pred_num", 2), ("keepRate", 1.0), ("ssl_reg", 0.5),
                 ("reg", 1e-2), ("trnNum", args.trnNum), ("lr", args.lr), ("decay_step", args.decay_step),
                 ("epoch", args.epoch), ("save_path", args.save_path), ("load_model", args.load_model)):
        monkeypatch.setattr(args, k, v)
    rng = np.random.default_rng(31)
    U, I = 70, 60
    tmt = synthetic.make_trn_mat_time(U, I, [700, 650])
    seq = synthetic.make_sequence(tmt)
    tst_int = [int(rng.integers(0, I)) if u % 2 else None for u in range(U)]
    handler = DataHandler.from_memory(tmt, seq, tst_int, {u + 1: list(rng.integers(1, I + 1, size=30)) for u in range(U)})
    rec = Recommender(dev, handler)
    rec.prepareModel()
    g = torch.Generator(device="cpu").manual_seed(9)
    with torch.no_grad():
        for name in list(NNs.params):
            if name.endswith("bias") or name.endswith("beta") or name.endswith("Bias"):
                NNs.params[name].copy_(0.1 * torch.randn(NNs.params[name].shape, generator=g))
        for k in ("uEmbed", "iEmbed", "posEmbed"):
            NNs.params[k].mul_(20)
    return rec, handler, NNs, args


def _oracle_params(rec, NNs):
    """The model's variables as float64 leaves in the oracle's layout (name -> leaf for the gradient comparison)."""
    leaves = {}
    inv = {id(v): k for k, v in NNs.params.items()}

    def leaf(name):
        if name not in leaves:
            leaves[name] = NNs.params[name].detach().cpu().double().requires_grad_(True)
        return leaves[name]

    mh = lambda att: {k: leaf(inv[id(v)]) for k, v in att.weights().items()}
    P = {"uEmbed": leaf("uEmbed"), "iEmbed": leaf("iEmbed"), "posEmbed": leaf("posEmbed"),
         "meta2_W": leaf("meta2"), "meta2_b": leaf("meta2Bias"), "meta3_W": leaf("meta3"), "meta3_b": leaf("meta3Bias")}
    for key, (gm, bt), att in (("fuse_u", rec.ln[0], rec.multihead_self_attention0), ("fuse_i", rec.ln[1], rec.multihead_self_attention1)):
        P[key] = dict({"lstm_W": leaf("rnn_lstm_kernel"), "lstm_b": leaf("rnn_lstm_bias"), "ln_gamma": leaf(inv[id(gm)]),
                       "ln_beta": leaf(inv[id(bt)])}, **mh(att))
    P["ln"] = [(leaf(inv[id(gm)]), leaf(inv[id(bt)])) for gm, bt in rec.head_ln]
    P["att"] = [mh(a) for a in rec.multihead_self_attention_sequence]
    return P, leaves


def _grad_close(got, want, name, floor_extra=0.0):
    """The gradient tolerance of test_gpu_train.py and test_gpu_seq_att.py: 2e-4 |want| + max(5e-5 max|want|, 2e-5)."""
    floor = max(5e-5 * np.abs(want).max(), 2e-5, floor_extra)
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, scale {np.abs(want).max():.3e}, worst err / tol "
          f"{(err / (2e-4 * np.abs(want) + floor)).max():.3f}")
    bad = err > 2e-4 * np.abs(want) + floor
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {err[bad].max():.3e} (scale {np.abs(want).max():.3e})"


def _host_batch(rec, handler, args):
    np.random.seed(3)
    batIds = np.random.permutation(args.user)[:args.batch]
    uL, iL, sequence, mask, uLs = rec.sampleTrainBatch(batIds, handler.trnMat, handler.timeMat, 5)
    su, si, _ = rec.sampleSslBatch(batIds, handler.subMat, False)
    return {"uids": uL, "iids": iL, "uLocs_seq": uLs, "sequence": sequence, "mask": mask, "suids": su, "siids": si}


def _loss_and_grads(rec, NNs, args, batch):
    for p in NNs.params.values():
        p.grad = None
    pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
    (pre + args.ssl_reg * ssl).backward()
    return float(pre.detach()), float(ssl.detach()), {k: (None if v.grad is None else v.grad.clone()) for k, v in NNs.params.items()}


@pytest.mark.parametrize("d,ssldim,att_layer,temp,seq_att", [(64, 48, 2, 1.0, "sum"), (32, 32, 1, 0.5, "sum"), (64, 48, 2, 1.0, "full")])
def test_train_loss_under_softmax_against_float64(dev, monkeypatch, d, ssldim, att_layer, temp, seq_att):
    import seq_att_ref
    from sa_gnn_amd.model import banned_table
    rec, handler, NNs, args = _setup(dev, monkeypatch, d, ssldim, att_layer, temp=temp, seq_att=seq_att)
    batch = _host_batch(rec, handler, args)
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    P, leaves = _oracle_params(rec, NNs)
    adj = [O.trans_to_lsts(m)[0] for m in handler.subMat]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in handler.subMat]
    head = seq_att_ref.torch_head_ragged if seq_att == "full" else R.torch_head_collapsed
    opre, ossl, _, _ = R.torch_train_loss_softmax(P, adj, tp, batch, dict(CFG, temp=temp), banned_table(handler, args.item), head=head)
    (opre + args.ssl_reg * ossl).backward()
    opre, ossl = float(opre.detach()), float(ossl.detach())
    print(f"preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
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


def test_device_sampled_batch_gives_the_host_forms_loss(dev, monkeypatch):
    from test_gpu_device_sampler import _host_form
    rec, handler, NNs, args = _setup(dev, monkeypatch)
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = rec.sample_batch_device(bat, 31337, 2)
    hb = _host_form(rec, b, args)
    assert "active" in b and "active" not in hb
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, b)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"preLoss device {pre_d!r} host {pre_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed", "uEmbed"):
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)


def test_train_epochs_under_softmax_stay_finite_and_improve(dev, monkeypatch):
    """test_train_epoch_runs_and_improves_loss under the softmax loss."""
    rec, handler, NNs, args = _setup(dev, monkeypatch, 64, 32, 1)
    for k, v in (("trnNum", 64), ("lr", 5e-3), ("keepRate", 0.5), ("ssl_reg", 1e-3), ("reg", 1e-4), ("decay_step", 64 // args.batch)):
        monkeypatch.setattr(args, k, v)
    np.random.seed(0)
    torch.manual_seed(0)
    losses = [rec.trainEpoch()["preLoss"] for _ in range(8)]
    print("preLoss per epoch:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and np.mean(losses[-3:]) < np.mean(losses[:3])
    assert all(bool(torch.isfinite(p).all()) for p in NNs.params.values())
    res = rec.testEpoch()
    assert 0.0 <= res["HR"] <= 1.0 and 0.0 <= res["NDCG"] <= 1.0


def _profile_kinds(lib, fn):
    from sa_gnn_amd import ops
    lib.sagnn_profile_enable(4096)
    try:
        out = fn()
        kinds = np.zeros(4096, np.int32)
        n = ctypes.c_int(0)
        ops.check(lib.sagnn_profile_read(None, kinds.ctypes.data, None, None, 4096, ctypes.byref(n)))
    finally:
        lib.sagnn_profile_enable(0)
    return out, kinds[:n.value]


def test_off_means_off(dev, monkeypatch):
    """Under the default flag a training step launches nothing of the new profile kind (6); under softmax it does: the
    forward and the backward entry, once each."""
    from sa_gnn_amd import _lib
    from sa_gnn_amd.Params import args as the_args
    assert the_args.predLoss == "hinge" and the_args.softmaxTemp == 1.0
    lib = _lib.load()
    rec, handler, NNs, args = _setup(dev, monkeypatch, loss="hinge")
    _, kinds = _profile_kinds(lib, lambda: _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args)))
    assert len(kinds) > 0 and not (kinds == 6).any()
    rec, handler, NNs, args = _setup(dev, monkeypatch, loss="softmax")
    _, kinds = _profile_kinds(lib, lambda: _loss_and_grads(rec, NNs, args, _host_batch(rec, handler, args)))
    assert (kinds == 6).sum() == 2


def test_checkpoint_saved_under_softmax_loads_under_hinge(dev, monkeypatch, tmp_path):
    from sa_gnn_amd.model import Recommender
    rec, handler, NNs, args = _setup(dev, monkeypatch)
    for k, v in (("epoch", 1), ("save_path", "softmax_ckpt"), ("load_model", "softmax_ckpt")):
        monkeypatch.setattr(args, k, v)
    want = rec.testEpoch()
    rec.saveHistory(str(tmp_path))
    state = torch.load(str(tmp_path / "Models" / "softmax_ckpt"), weights_only=True)
    assert "predLoss" not in state and "softmaxTemp" not in state          # the flag is not part of the model
    monkeypatch.setattr(args, "predLoss", "hinge")
    rec2 = Recommender(dev, handler)
    rec2.prepareModel()
    assert rec2.testEpoch() != want
    rec2.loadModel(str(tmp_path))
    assert rec2.testEpoch() == want
