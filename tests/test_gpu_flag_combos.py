"""GPU suite of the training objective under COMBINED opt-in flags: Recommender.train_loss and every
parameter gradient against the composed float64 objective of flag_combo_ref, on the eight cases that cover every legal
pair of non-default values (test_flag_combo_host.py asserts the cover):

  1  G N T F A S D  d = 64   fused GRU, weighted + time SpMM, softmax through the additive pool
  2  G N E F A B D  d = 32   fused GRU, drop + weighted SpMM, compacted rows, hinge
  3  T B D          d = 32   LSTM, unweighted time form under compacted rows
  4  G S E          d = 128  per-step GRU route, softmax with edge drop, collapsed head
  5  G N T C L S K P D  d = 64   every position against popularity candidates: the target scatter's dI into the weighted + time SpMM
  6  E C L S K B D      d = 32   every position against uniform candidates under compacted rows and edge drop
  7  N F A S K P B      d = 32   the candidate loss's backward through the additive pool into compacted rows
  8  G E C A S K P      d = 128  causal attention under the additive pool, the popularity draw next to edge drop

on the 70-user, 60-item, 2-interval timestamped dataset of test_gpu_edge_time.py. Tolerances are the sibling tests':
losses at 1e-4 max(|want|, 1), gradients at test_gpu_seq_att._grad_close with the key biases' floor. Only case 3 has
leaves judged otherwise: those named in flag_combo_ref.F32_EXCEPTIONS[3], where float32 on the CPU is itself not within a
quarter of that tolerance (test_flag_combo_host.py measures it), at max(tolerance, 4 x the float32-CPU error), the rule
of test_gpu_zero_grad_rows.py."""
import numpy as np
import pytest
import torch

import flag_combo_ref as C
import fusion_rows_ref as FR
from test_flag_combo_host import host_batch, oracle_run, setup_case

pytestmark = pytest.mark.gpu

# compared leaves at least: the 37 (LSTM) / 39 (GRU) variables every case has and a loss reaches, + 9 under T (timeEmbed
# and the 2 T L time weights, without a gradient on both sides otherwise), + 3 under A
MIN_COMPARED = {1: 39 + 9 + 3, 2: 39 + 3, 3: 37 + 9, 4: 39, 5: 39 + 9, 6: 37, 7: 37 + 3, 8: 39 + 3}


def _device_candidates(rec, handler, args, letters, dev):
    """The step's list as the device draws it under CAND_SEED, read back (test_gpu_seq_causal._compare_all): equal to the
    restatement's ids and live positions; the device's own offsets go into the float64 objective."""
    from sa_gnn_amd import ops
    cand, bias = C.step_candidates(letters, handler, args.item)
    if cand is None:
        return None
    if bias is None:
        got = ops.sample_strata(args.item, args.softmaxNegs, *C.CAND_SEED, dev).cpu().numpy()
        assert got.tolist() == cand.tolist()
        return got, None
    got, gb = (v.cpu().numpy() for v in ops.sample_strata_weighted(*rec._pop_cum_device(), args.softmaxNegs, *C.CAND_SEED))
    assert got.tolist() == cand.tolist() and np.array_equal(np.isfinite(gb), np.isfinite(bias))
    assert np.allclose(gb[np.isfinite(gb)], bias[np.isfinite(bias)], rtol=1e-6, atol=1e-6)
    return got, gb


def _loss_and_grads(rec, NNs, args, batch):
    from test_gpu_seq_att import _loss_and_grads as run
    return run(rec, NNs, args, batch)                     # train_loss(dict(batch), keep_rate=1.0), then backward


def _moved(a, b):
    """The `off` comparison of test_recommender_train_loss_with_edge_keep_rate: either loss differs by more than 1e-3."""
    return abs(b[0] - a[0]) > 1e-3 * abs(a[0]) or abs(b[1] - a[1]) > 1e-3 * abs(a[1])


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_train_loss_and_every_gradient_against_the_composed_float64_objective(dev, monkeypatch, case):
    from test_gpu_seq_att import QK_NOISE, _grad_close, _head_qk_names
    letters, latdim = C.CASES[case]
    rec, handler, NNs, args = setup_case(dev, monkeypatch, letters, latdim)
    batch, obatch = host_batch(letters, rec, handler, args)
    cands = _device_candidates(rec, handler, args, letters, dev)
    pre, ssl, grads = _loss_and_grads(rec, NNs, args, batch)
    if "B" in letters:                                    # the compacted rows are the reference's, and a real subset
        users, items, _ = FR.touched_rows(batch if cands is None else dict(batch, cand=cands[0]), args.user, args.item)
        assert rec.fusion_rows_counts == (len(users), len(items)) and len(users) < args.user
        assert len(items) < args.item or "K" in letters   # 16 candidates can complete the 60 items: case 6 touches them all
        assert "D" not in letters or tuple(batch["drop_u"].shape) == (len(users), args.graphNum, latdim)
    opre, ossl, want = oracle_run(letters, rec, handler, NNs, args, obatch, monkeypatch, candidates=cands)
    print(f"flag_combos|gpu|case {case} {letters} d={latdim}|preLoss {pre!r} vs {opre!r}; sslloss {ssl!r} vs {ossl!r}")
    assert abs(pre - opre) <= 1e-4 * max(abs(opre), 1.0) and abs(ssl - ossl) <= 1e-4 * max(abs(ossl), 1.0)
    err32 = {}
    if C.F32_EXCEPTIONS[case]:
        _, _, g32 = oracle_run(letters, rec, handler, NNs, args, obatch, monkeypatch, dtype=torch.float32, candidates=cands)
        err32 = {n: np.abs(g32[n] - want[n]) for n in C.F32_EXCEPTIONS[case]}
    assert set(want) == set(NNs.params) == set(grads)
    compared, worst = 0, {}
    for name in NNs.params:                               # every variable: compared, or without a gradient on both sides
        got = grads[name]
        if want[name] is None:
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        assert got is not None, f"no gradient reached {name}"
        a = got.cpu().double().numpy()
        assert np.isfinite(a).all(), name
        extra = C.k_bias_floor(name, want)
        tol = C.grad_tolerance(want[name], extra)
        if name in err32:
            tol = np.maximum(tol, 4.0 * err32[name])
        worst[name] = float((np.abs(a - want[name]) / tol).max())
        print(f"flag_combos|gpu|case {case} {letters} d={latdim}|{name}|{worst[name]:.3f} of the tolerance"
              + (" (4 x float32-CPU rule)" if name in err32 else ""))
        if name in err32:
            assert worst[name] <= 1.0, f"{name} at {worst[name]:.3f} of max(tolerance, 4 x the float32-CPU error)"
        else:
            _grad_close(a, want[name], name, extra)
        compared += 1
    print(f"flag_combos|gpu|case {case} {letters} d={latdim}|{compared} leaves compared, worst "
          f"{max(worst, key=worst.get)} at {max(worst.values()):.3f}")
    assert compared >= MIN_COMPARED[case]
    # the flag-specific variables really train
    trains = lambda n: want[n] is not None and float(np.abs(want[n]).max()) > 0 and float(grads[n].abs().max()) > 0
    if "G" in letters:
        assert all(trains(n) for n in C.GRU_NAMES) and "rnn_lstm_kernel" not in NNs.params
    time = C.time_names(rec, NNs.params)
    assert len(time) == 1 + 2 * args.graphNum * args.gnn_layer
    if "T" in letters:
        assert all(trains(n) for n in time)
    else:
        assert all(want[n] is None for n in time)
    if "A" in letters:
        assert all(trains(n) for n in C.ADD_NAMES)
    if "F" in letters or "C" in letters:                  # above the noise under which the collapsed head's stay
        qk, v = _head_qk_names(rec, NNs)
        v_scale = max(float(grads[n].abs().max()) for n in v)
        assert all(float(grads[n].abs().max()) > QK_NOISE * v_scale and float(np.abs(want[n]).max()) > QK_NOISE * v_scale for n in qk)


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_each_flag_of_the_case_moves_the_result(dev, monkeypatch, case):
    """Any one flag of the case back at its default: preLoss or sslloss moves by more than 1e-3 relative. Two flags cannot
    be judged that way. F under A is judged without A on both sides (A alone without F is refused). B must NOT move the
    result (it fuses the rows the loss reads, test_gpu_fusion_rows.py): there the losses agree to that file's 1e-6 and the
    run is shown to have compacted. What a newer flag needs stays legal on both sides: P is judged against uniform
    candidates and L against last as they are; C against F, without the L that needs C; K without the P that needs it and
    the B that S takes only under K; S without K, P, L and B."""
    letters, latdim = C.CASES[case]
    seen = {}

    def losses(on):
        key = "".join(c for c in C.LETTERS if c in on)
        if key not in seen:
            rec, handler, NNs, args = setup_case(dev, monkeypatch, key, latdim)
            batch, _ = host_batch(key, rec, handler, args)
            pre, ssl = rec.train_loss(dict(batch), keep_rate=1.0)
            seen[key] = (float(pre.detach()), float(ssl.detach()), getattr(rec, "fusion_rows_counts", None), (args.user, args.item))
        return seen[key]

    base = losses(letters)
    assert np.isfinite(base[0]) and np.isfinite(base[1])
    for c in letters:
        rest = letters.replace(c, "")
        if c == "B":
            off = losses(rest)
            assert abs(off[0] - base[0]) <= 1e-6 * max(abs(base[0]), 1.0) and abs(off[1] - base[1]) <= 1e-6 * max(abs(base[1]), 1.0)
            assert base[2][1] < base[3][1] or base[2][0] < base[3][0]
            continue
        drop = lambda s, cs: "".join(x for x in s if x not in cs)      # noqa: E731
        if c == "F" and "A" in letters:
            on, off = losses(rest.replace("A", "") + "F"), losses(rest.replace("A", ""))
        elif c == "C":
            on, off = losses(drop(letters, "L")), losses(drop(letters, "LC") + "F")
        elif c == "K":
            on, off = losses(drop(letters, "PB")), losses(drop(letters, "PBK"))
        elif c == "S" and set(letters) & set("KPLB"):
            on, off = losses(drop(letters, "KPLB")), losses(drop(letters, "KPLBS"))
        else:
            on, off = base, losses(rest)
        print(f"flag_combos|gpu|case {case} {letters}|{c} off: preLoss {on[0]:.6g} -> {off[0]:.6g}, sslloss {on[1]:.6g} -> {off[1]:.6g}")
        assert _moved(on, off), f"case {case}: switching {c} off moves neither loss"


@pytest.mark.parametrize("case", [1, 2, 5, 7])
def test_device_sampled_batch_gives_the_host_forms_loss(dev, monkeypatch, case):
    """The segment path into the full head, not the CSR path: a device-sampled batch against its host form, at the bound
    of test_gpu_seq_pool.py's test of the same name, under the same edge seed and output-dropout masks."""
    from test_gpu_device_sampler import _host_form
    from test_gpu_seq_att import _grad_close
    letters, latdim = C.CASES[case]
    rec, handler, NNs, args = setup_case(dev, monkeypatch, letters, latdim)
    bat = np.random.default_rng(3).permutation(args.user)[:args.batch - 3]
    b = rec.sample_batch_device(bat, 31337, 2)
    hb = _host_form(rec, b, args)
    seq_items = rec._device_sampler().seq_items
    masks, _ = C.output_drop(letters, b, args.user, args.item, args.graphNum, latdim, args.pos_length, seq_items)
    rows_d = FR.touched_rows(b, args.user, args.item, args.pos_length, seq_items)
    rows_h = FR.touched_rows(hb, args.user, args.item)
    assert np.array_equal(rows_d[0], rows_h[0]) and np.array_equal(rows_d[1], rows_h[1])
    for batch in (b, hb):
        if "D" in letters:
            batch.update({k: v.to(dev) for k, v in masks.items()})
        if "E" in letters:
            batch["edge_seed"] = C.EDGE_SEED
        if "K" in letters:
            batch["cand_seed"] = C.CAND_SEED
    pre_d, ssl_d, gd = _loss_and_grads(rec, NNs, args, b)
    pre_h, ssl_h, gh = _loss_and_grads(rec, NNs, args, hb)
    print(f"flag_combos|gpu|case {case} {letters}|device batch: preLoss {pre_d!r} host form {pre_h!r}; sslloss {ssl_d!r} {ssl_h!r}")
    assert abs(pre_d - pre_h) <= 1e-4 * abs(pre_h) + 1e-5 and abs(ssl_d - ssl_h) <= 1e-4 * abs(ssl_h) + 1e-5
    for name in ("posEmbed", "iEmbed") + (C.ADD_NAMES if "A" in letters else ()):
        _grad_close(gd[name].cpu().double().numpy(), gh[name].cpu().double().numpy(), name)


@pytest.mark.parametrize("case", [1, 3, 5])
def test_captured_forward_and_device_evaluators(dev, monkeypatch, case):
    """The captured forward replays what forward() computes, bit for bit, after a row of timeEmbed is edited in place (the
    time tables are part of the capture), and the device evaluator gives the host evaluator's results."""
    letters, latdim = C.CASES[case]
    rec, handler, NNs, args = setup_case(dev, monkeypatch, letters, latdim)
    np.random.seed(1)
    host, host_full = rec.testEpoch(), rec.testEpochFull()
    monkeypatch.setattr(args, "evaluator", "device")
    np.random.seed(1)
    assert rec.testEpoch() == host and rec.testEpochFull() == host_full
    monkeypatch.setattr(args, "evaluator", "host")
    before = rec.forward()[0].clone()
    replay = rec.capture_forward()
    with torch.no_grad():
        rec.timeEmbed[2] += 1.0
    fu_g, fi_g = (t.clone() for t in replay())
    fu_e, fi_e = rec.forward()
    assert torch.equal(fu_g, fu_e) and torch.equal(fi_g, fi_e) and not torch.equal(fu_e, before)
