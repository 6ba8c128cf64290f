"""GPU suite of the softmax-loss entries on slab-shaped input: what --seqTargets all hands
sagnn_softmax_loss_f32 and its backward, kernel by kernel. Every token of every batch slot is a query row; most rows
carry target -1, a slot's rows share one exclusion list through excl_row, rows share targets, the call runs with
scale = 1 and an upstream gradient g = 1 / count from a device tensor that is no power of two, and Q is a row view with
ldq = d + 12. softmax_slab_ref builds the slab (264 rows: skipped tiles, wavefronts and a skipped 64-row lookup group
between live rows, tiles with one live row, the last row live or skipped) and a longer one (2,560 rows).

References: softmax_loss_ref.softmax_loss_np, softmax_cand_ref.softmax_loss_cand_np, softmax_pop_ref.softmax_loss_pop_np
with excl_row, each computed once per case and shared. Bounds: their tolerance_terms with the sibling suites' constants
(K_LSE 16, K_DQ 32, K_DI 32) and test_gpu_softmax_negs._check's loss tolerance; test_softmax_slab_host.py shows on the
CPU that float32 needs at most a quarter of each constant on these very inputs.

What a skipped row must not do (include/sagnn.h: zeros in its own outputs, nothing added to dI) is asked for every FINITE
Q row, which is what the header requires of a skipped row: zeros and +-3e38 give the same bits in every output. A NaN or
an infinity there is not covered: di_kernel's second product takes the row as its A operand against G = 0, and 0 x NaN
reaches every dI / dIc row of the span in all three modes (measured; DESIGN.md §27 has the two forms of a select that
were tried and what they cost). So the suite pins the other side instead: sagnn_seq_prefix_query_f32, which builds the
slab's Q, writes exact zeros into every padded row whatever the padding of its input holds."""
import numpy as np
import pytest
import torch

import softmax_cand_ref as C
import softmax_pop_ref as P
import softmax_slab_ref as S
from test_gpu_softmax_loss import K_DI, K_DQ, K_LSE, _t

pytestmark = pytest.mark.gpu

ROW_KEYS = ("lse", "tscore", "dQ", "dT")            # what a row owns: a function of that row alone


def _run(dev, c, Q=None, target=None, excl_row=None):
    """The case's forward and backward through ops, as _softmax_pre_loss_all calls the entries: scale 1, g = 1 / count on
    the device, Q a view of a wider buffer. Q / target / excl_row replace the case's. float32 numpy arrays; loss [1]."""
    from sa_gnn_amd import ops
    Q = c["Q"] if Q is None else Q
    target, excl_row = (c["target"] if target is None else target), (c["excl_row"] if excl_row is None else excl_row)
    d = c["d"]
    buf = torch.full((len(Q), d + 12), 7.0, dtype=torch.float32, device=dev)
    buf[:, :d] = _t(dev, Q, np.float32)
    Qd, Id, tg, rd = buf[:, :d], _t(dev, c["I"], np.float32), _t(dev, target, np.int32), _t(dev, excl_row, np.int32)
    excl = (_t(dev, c["ptr"], np.int64), _t(dev, c["items"], np.int32))
    g = torch.full((1,), float(c["g"]), dtype=torch.float32, device=dev)
    it = c["inv_temp"]
    if c["mode"] == "full":
        loss, lse, ts = ops.softmax_loss(Qd, Id, tg, it, 1.0, excl, rd)
        dQ, dI = ops.softmax_loss_bwd(Qd, Id, tg, lse, g, it, 1.0, excl, rd)
        out = {"dI": dI}
    else:
        cd, bd = _t(dev, c["cand"], np.int32), None if c["bias"] is None else _t(dev, c["bias"], np.float32)
        loss, lse, ts = ops.softmax_loss_cand(Qd, Id, cd, tg, it, 1.0, excl, rd, bias=bd)
        dQ, dIc, dT = ops.softmax_loss_cand_bwd(Qd, Id, cd, tg, lse, g, it, 1.0, excl, rd, bias=bd)
        assert dIc.shape == (len(c["cand"]), d) and dT.shape == dQ.shape == (len(Q), d)
        out = {"dIc": dIc, "dT": dT}
    torch.cuda.synchronize()
    out.update(loss=loss, lse=lse, tscore=ts, dQ=dQ)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _full_dI(c, out, target=None):
    """The device result as a full-size float64 dI for an upstream gradient of 1 (assembled in float64: no rounding added)."""
    target = c["target"] if target is None else target
    if c["mode"] == "full":
        dI = out["dI"].astype(np.float64)
    elif c["mode"] == "cand":
        dI = C.assemble_dI(c["n_items"], c["cand"], out["dIc"], target, out["dT"])
    else:
        dI = P.assemble_dI(c["n_items"], c["cand"], c["bias"], out["dIc"], target, out["dT"])
    return dI / float(c["g"])


def _bound(c, key, K):
    unit, floor = c["terms"][key]
    return K * unit + floor


def _check(c, out):
    """Every output against the case's float64 reference; prints the K each one needs before it asserts."""
    got = {"lse": out["lse"], "tscore": out["tscore"], "dQ": out["dQ"].astype(np.float64) / float(c["g"]), "dI": _full_dI(c, out)}
    need = S.needs(c, got)
    loss, want, tol = float(out["loss"][0]), c["ref"]["loss"], S.loss_tolerance(c, K_LSE)
    print(f"softmax_slab|gpu|{c['name']}|K needed lse {need['lse']:.2f} / {K_LSE}, tscore {need['tscore']:.2f} / {K_LSE}, "
          f"dQ {need['dQ']:.2f} / {K_DQ}, dI {need['dI']:.2f} / {K_DI}; loss {loss!r} vs {want!r} (tol {tol:.3e})")
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{c['name']}: {k} holds inf or NaN"
    assert need["lse"] <= K_LSE and need["tscore"] <= K_LSE and need["dQ"] <= K_DQ and need["dI"] <= K_DI, (c["name"], need)
    assert abs(loss - want) <= tol, c["name"]
    skipped = ~c["structure"]["live"]
    for k in ROW_KEYS:
        assert k not in out or not out[k][skipped].any(), f"{c['name']}: a skipped row has a {k}"
    if c["bias"] is not None:
        assert not out["dIc"][~np.isfinite(c["bias"])].any(), f"{c['name']}: a dead position has a dIc row"


def _same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype == np.float32 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


# ---- 1. against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_items,n_cand,d,temp", S.CASES)
def test_the_slab_against_float64(dev, mode, n_items, n_cand, d, temp):
    c = S.case(mode, n_items, n_cand, d, temp)
    S.assert_small_structure(c)
    _check(c, _run(dev, c))


# ---- 3. skipped rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_live", [True, False])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("mode,n_items,n_cand", S.MODES)
def test_a_skipped_row_adds_nothing_whatever_finite_values_its_query_row_holds(dev, mode, n_items, n_cand, d, last_live):
    """Zeros in the row's own outputs, and every output of the call bit-identical whether the skipped rows of Q hold
    zeros or +-3e38 (finite, as include/sagnn.h requires of them; their scores overflow to inf and NaN inside the
    kernels): the values are read (the scores' A rows, the clamped rows past the last tile) and must not count.
    last_live = False: the slab's last row is skipped, so the clamped reads land on such a row."""
    c = S.build(mode, n_items, n_cand, d, 1.0, last_live=last_live, ref=False)
    S.assert_small_structure(c)
    skipped = ~c["structure"]["live"]
    base = _run(dev, c)
    for k, v in base.items():
        assert np.isfinite(v).all(), k
    for k in ROW_KEYS:
        assert k not in base or not base[k][skipped].any(), k
    assert base["loss"][0] > 0 and base["dQ"][~skipped].any(1).all()
    huge = np.where(np.arange(len(skipped) * d).reshape(-1, d) % 2 == 0, np.float32(3e38), np.float32(-3e38))
    Q = np.where(skipped[:, None], huge, c["Q"]).astype(np.float32)
    assert np.array_equal(Q[~skipped], c["Q"][~skipped]) and (np.abs(Q[skipped]) == np.float32(3e38)).all()
    _same_bits(base, _run(dev, c, Q=Q), f"{c['name']}: skipped rows of Q filled with +-3e38")
    # every row skipped, the formerly live rows of Q as they are
    none = _run(dev, c, target=np.full(len(skipped), -1))
    assert none["loss"][0] == 0.0 and all(not v.any() for v in none.values()), {k: bool(v.any()) for k, v in none.items()}


@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_prefix_kernel_leaves_exact_zeros_in_every_padded_row(dev, d):
    """The finite-Q requirement of the loss entries is met by construction: ops.seq_prefix_query writes +0.0 into every
    padded row of the slab and never reads the padding of x, which here holds NaN and +-3e38. Slot lengths: the small
    slab's token counts (0, 1, a full slot of 24). The real rows have the bits of the run on a zero-padded x."""
    from sa_gnn_amd import ops
    lens = np.array([n for n, _, _, _, _ in S.small_spec()], dtype=np.int32)
    real = (np.arange(S.POS)[None, :] < lens[:, None]).reshape(-1)
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((S.N_SLOTS * S.POS, d)) * 0.7).astype(np.float32)
    U = _t(dev, rng.standard_normal((S.N_SLOTS, d)), np.float32)
    bad = np.where(np.arange(x.size).reshape(x.shape) % 3 == 0, np.float32(np.nan), np.where(np.arange(x.size).reshape(x.shape) % 3 == 1,
                                                                                        np.float32(3e38), np.float32(-3e38)))
    ld = _t(dev, lens, np.int32)
    clean = ops.seq_prefix_query(_t(dev, np.where(real[:, None], x, 0.0), np.float32), U, ld, S.POS, 0.5).cpu().numpy()
    dirty = ops.seq_prefix_query(_t(dev, np.where(real[:, None], x, bad), np.float32), U, ld, S.POS, 0.5).cpu().numpy()
    assert (~real).sum() == 264 - lens.sum() and not dirty[~real].view(np.uint32).any()          # +0.0, every bit
    assert np.isfinite(dirty).all() and dirty[real].any(1).all()
    assert np.array_equal(clean.view(np.uint32), dirty.view(np.uint32))


# ---- 4. row independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_items,n_cand", S.MODES)
def test_live_rows_alone_give_the_slabs_rows(dev, mode, n_items, n_cand):
    """What a compaction of the rows with a target leans on: a call on the live rows alone (their excl_row values, the
    same candidates, the same scale and g) gives each row's lse, tscore, dQ and dT bit for bit; dI / dIc and the loss sum
    the same terms in another order and agree within twice their bounds. Two slab runs agree in every bit."""
    c = S.case(mode, n_items, n_cand, 64, 0.25)
    live = c["structure"]["live"]
    a = _run(dev, c)
    _same_bits(a, _run(dev, c), f"{c['name']}: two runs")
    b = _run(dev, c, Q=c["Q"][live], target=c["target"][live], excl_row=c["excl_row"][live])
    for k in ROW_KEYS:
        if k in a:
            assert np.array_equal(a[k][live].view(np.uint32), b[k].view(np.uint32)), (c["name"], k)
    g = float(c["g"])
    key = "dI" if mode == "full" else "dIc"
    rows = slice(None) if mode == "full" else c["cand"]
    diff = np.abs(a[key].astype(np.float64) - b[key]) / g
    bound = 2 * _bound(c, "dI", K_DI)[rows]
    tol = S.loss_tolerance(c, K_LSE)
    print(f"softmax_slab|gpu|{c['name']}|slab vs live rows: {key} at {float((diff / bound).max()):.3f} of twice its bound, "
          f"loss {abs(float(a['loss'][0]) - float(b['loss'][0])) / (2 * tol):.3f}")
    assert (diff <= bound).all(), (c["name"], key)
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 2 * tol
    if c["bias"] is not None:
        assert not a["dIc"][~np.isfinite(c["bias"])].any() and not b["dIc"][~np.isfinite(c["bias"])].any()


# ---- 5. dI assembly at the autograd level -------------------------------------------------------------------------------
def _autograd(dev, c, scatter_targets=None):
    """(loss / count, dQ, full-size dI) of the autograd function through .backward(), as _softmax_pre_loss_all builds it."""
    from sa_gnn_amd import autograd as ag
    q = _t(dev, c["Q"], np.float32).requires_grad_(True)
    i = _t(dev, c["I"], np.float32).requires_grad_(True)
    tg, rd = _t(dev, c["target"], np.int32), _t(dev, c["excl_row"], np.int32)
    excl = (_t(dev, c["ptr"], np.int64), _t(dev, c["items"], np.int32))
    count = (tg >= 0).sum().clamp(min=1).to(torch.float32)
    if c["mode"] == "full":
        total = ag.SoftmaxLossFn.apply(q, i, tg, c["inv_temp"], 1.0, excl, rd)
    else:
        bd = None if c["bias"] is None else _t(dev, c["bias"], np.float32)
        total = ag.SoftmaxLossCandFn.apply(q, i, _t(dev, c["cand"], np.int32), tg, c["inv_temp"], 1.0, excl, rd, bd, scatter_targets)
    (total / count).sum().backward()
    torch.cuda.synchronize()
    return float(total.detach()), q.grad.cpu().numpy(), i.grad.cpu().numpy()


def _check_autograd(c, total, dQ, dI, what):
    g = float(c["g"])
    need = {k: S.R.worst_ratio(v.astype(np.float64) / g, c["ref"][k], *c["terms"][k]) for k, v in (("dQ", dQ), ("dI", dI))}
    tol = S.loss_tolerance(c, K_LSE)
    print(f"softmax_slab|gpu|{c['name']}|{what}: K needed dQ {need['dQ']:.2f} / {K_DQ}, assembled dI {need['dI']:.2f} / {K_DI}; "
          f"loss {total!r} vs {c['ref']['loss']!r} (tol {tol:.3e})")
    assert np.isfinite(dQ).all() and np.isfinite(dI).all()
    assert need["dQ"] <= K_DQ and need["dI"] <= K_DI and abs(total - c["ref"]["loss"]) <= tol, (c["name"], what, need)


@pytest.mark.parametrize("mode,n_items,n_cand", [m for m in S.MODES if m[0] != "full"])
def test_the_target_scatter_assembles_the_full_size_dI(dev, mode, n_items, n_cand):
    """ag.SoftmaxLossCandFn with scatter_targets=True (float atomics: up to 24 rows of this slab add into one dI row)
    against float64 at the kernel's own K_DI, and against the ordered assembly (scatter_targets=False) within twice it."""
    c = S.case(mode, n_items, n_cand, 64, 0.25)
    total, dQ, dI = _autograd(dev, c, True)
    _check_autograd(c, total, dQ, dI, "scatter_targets=True")
    total2, dQ2, dI2 = _autograd(dev, c, False)
    _check_autograd(c, total2, dQ2, dI2, "scatter_targets=False")
    assert total == total2 and np.array_equal(dQ.view(np.uint32), dQ2.view(np.uint32))
    diff = np.abs(dI.astype(np.float64) - dI2) / float(c["g"])
    assert (diff <= 2 * _bound(c, "dI", K_DI)).all()
    untouched = np.setdiff1d(np.arange(n_items), np.concatenate([c["cand"], c["target"][c["target"] >= 0]]))
    assert len(untouched) and not dI[untouched].any() and not dI2[untouched].any()


def test_the_full_function_on_the_slab(dev):
    c = S.case("full", 4099, 0, 64, 0.25)
    _check_autograd(c, *_autograd(dev, c), "SoftmaxLossFn")


# ---- 6. a longer slab ---------------------------------------------------------------------------------------------------
def test_a_longer_slab_against_float64(dev):
    """40 slots x 64 positions, about 15 % live: 80 row pairs per chunk in the chunk kernels' grids, 40 trips of
    di_kernel's query loop, 10 of loss_sum_kernel's."""
    c = S.case(*S.LONG_CASE, long=True)
    assert len(c["target"]) == 2560 and 0.10 < c["structure"]["live"].mean() < 0.20
    _check(c, _run(dev, c))
