"""GPU suite of the SpMM selection: variant (row block of a wave) x lane-group width x form x entry, every cell against
float64 (tests/spmm_routes_ref.py), forward and adjoint, and against its neighbours bit for bit.

The variant of a launch depends on the row count alone (262,144 rows and more take 16 rows per wave), so the graphs have
many rows and little work: every row is empty except three windows of a few hundred rows, at rows 0, across a 64-row
block boundary near the middle, and at the end, where the last wave is cut to 1, 15 or 16 rows. The operands are drawn on
the device, only the window rows exist on the host, and the empty rows are held on the device to their closed form: with
leaky(0) = 0 their output is the residual or the running sum bit for bit. The small variant runs the same windows in a
pattern of fewer rows, and its window rows must equal the large variant's exactly: the summation order of a row does
not depend on the row block.

The bar is assert_sum_close of test_gpu_spmm.py (1e-4 relative + 1e-5 + 2e-7 sum|terms|) with the abs_terms recurrence of
test_gpu_edge_drop.py; a gradient's terms are the adjoint's own sum of absolute values. Where the float64 row sum cannot
tell the sign of an activation's input within that bar, the adjoint reference takes the slope the kernel recorded."""
import re

import numpy as np
import pytest
import torch

import spmm_routes_ref as R

pytestmark = pytest.mark.gpu

T, L, LEAKY = 2, 2, 0.5
N_SRC = 3001                 # items: a few thousand, not a multiple of 64
K_BLOCKS = 3                 # n_rows = 262144 + 64 * K_BLOCKS + r
TAIL_R = (1, 15, 16)         # the last wave holds r rows, the last block three idle waves
SEED, STEP, KEEP = 0x1234_5678_9ABC_DEF, 5, 0.5
BUCKETS = (3, 300)
D_THRESHOLD = min(int(np.floor(KEEP * 2.0 ** 32)), 2 ** 32 - 1)      # edge_drop_ref.threshold(KEEP)

# (d, form, r, M, wide): each case runs both variants and both entries, so it reaches four cells (_case returns the ones
# it ran, and the test holds them against cells_of). r and M rotate so that every width and every form meets every r,
# and both time forms both table sizes (tests/test_spmm_routes_host.py). wide: the second tuning of d = 256, whose short
# threshold lies past the 64-lane group (spmm_routes_ref.tuning_for); every form runs it too.
CASES = [(d, form, TAIL_R[(di + fi) % 3], BUCKETS[(di + fi) % 2], False)
         for di, d in enumerate(R.WIDTHS) for fi, form in enumerate(R.FORMS)]
CASES += [(d, form, TAIL_R[(fi + 1) % 3], BUCKETS[fi % 2], True) for d in R.WIDE_WIDTHS for fi, form in enumerate(R.FORMS)]
ASYMMETRIC = [(64, "plain", 16, 3, 13), (64, "drop+weights", 1, 3, 13), (128, "time", 15, 300, 13)]   # (..., I < 16)
SHORT_EXACT = [(d, R.lpr(d) + 16) for d in R.BWD_WIDTHS]           # (d, short_thresh > LPR)


def cells_of(case):
    d, form = case[0], case[1]
    return {(v, d, form, e) for v in R.VARIANTS for e in R.ENTRIES}


def assert_sum_close(got, want, abs_terms, what=""):
    """The rule of test_gpu_spmm.py: 1e-4 |want| + 1e-5 + 3 eps32 sum|terms| (eps32 = 2^-24)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = 1e-4 * np.abs(want) + 1e-5 + 2e-7 * np.asarray(abs_terms, np.float64)
    bad = np.abs(got - want) > tol
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} outside tolerance; worst {np.abs(got - want)[bad].max():.3e}; "
                           f"first at {tuple(np.argwhere(bad)[0])}")


def _drop(ops):
    return ops.EdgeDrop(SEED, STEP, KEEP)


def _plans(dev, pat, form, M):
    """The user-side and item-side plans of the pattern and of the empty interval with its phantom (0, 0) edge."""
    from sa_gnn_amd import ops
    weights, _, timed = R.form_flags(form)
    pu, pi = [], []
    for p in (pat, R.phantom(pat.n_rows, pat.n_src, pat.d, pat.wide)):
        rp_t, ci_t, order = p.transposed()
        kw, kw_t = {}, {}
        if weights:
            kw["weights"], kw_t["weights"] = p.weights, np.ascontiguousarray(p.weights[order])
        if timed:
            kw.update(buckets=p.buckets[M], n_buckets=M)
            kw_t.update(buckets=np.ascontiguousarray(p.buckets[M][order]), n_buckets=M)
        pu.append(ops.SpmmPlan(p.rowptr, p.colidx, p.n_rows, p.n_src, device=dev, tuning=pat.tuning, **kw))
        pi.append(ops.SpmmPlan(rp_t, ci_t, p.n_src, p.n_rows, device=dev, tuning=pat.tuning, **kw_t))
    return pu, pi


def _host_operands(d, n_win, n_src, M, seed):
    """float32 host values of everything the reference reads: the users' window rows, every item row, the time table."""
    rng = np.random.default_rng([seed, d, n_src])
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"u0": g(T, n_win, d), "gu": g(T, n_win, d), "i0": g(T, n_src, d), "gi": g(T, n_src, d), "te": g(T, L, 2, M, d)}


def _unpack(bits, d):
    """[.., rows, d/4] uint8 activation masks -> [.., rows, d] bool."""
    b = bits.cpu().numpy()
    return ((b[..., None] >> np.arange(4)) & 1).reshape(*b.shape[:-1], d).astype(bool)


def _run(dev, pat, form, M, host, bwd):
    """Every entry on one pattern. Asserts what needs no reference: the empty rows' closed forms on the device and the
    batched entry against the per-interval entry bit for bit. Returns the window rows (and every item row) on the host."""
    from sa_gnn_amd import ops
    _, dropped, timed = R.form_flags(form)
    d, U, I = pat.d, pat.n_rows, pat.n_src
    pu, pi = _plans(dev, pat, form, M)
    batch = ops.SpmmBatch(pu, pi)
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    win = torch.from_numpy(pat.win).to(dev)
    empty = torch.ones(U, dtype=torch.bool, device=dev)
    empty[win] = False
    u0, gu = (torch.randn((T, U, d), generator=gen, device=dev) for _ in range(2))
    u0[:, win], gu[:, win] = torch.from_numpy(host["u0"]).to(dev), torch.from_numpy(host["gu"]).to(dev)
    i0, gi = torch.from_numpy(host["i0"]).to(dev), torch.from_numpy(host["gi"]).to(dev)
    te = torch.from_numpy(host["te"]).to(dev) if timed else None
    drop = _drop(ops) if dropped else None
    got = {"ran": set()}                        # (variant, entry) of the launches on the user rows, as they are made

    # one product through spmm_ex / spmm_drop / spmm_time: residual and running sum
    out, acc_out = torch.empty((U, d), device=dev), torch.empty((U, d), device=dev)
    kw = dict(residual=u0[1], out=out, acc_in=gu[0], acc_out=acc_out)
    if dropped:
        ops.spmm_drop(pu[0], i0[0], LEAKY, drop, ops.edge_tag(0, 1, 0), True, **kw)
    elif timed:
        ops.spmm_time(pu[0], i0[0], LEAKY, te[0, 1, 0], **kw)
    else:
        ops.spmm_ex(pu[0], i0[0], LEAKY, **kw)
    got["ran"].add((R.variant(pu[0].n_rows), "per-plan"))
    assert bool((out == u0[1]).all(1)[empty].all()), "an empty row's out is its residual"
    assert bool((acc_out == gu[0] + u0[1]).all(1)[empty].all()), "an empty row's running sum is acc_in + residual"
    got["prod_out"], got["prod_acc"] = out[win].cpu(), acc_out[win].cpu()
    del out, acc_out

    # the stack, batched; then each interval through the per-plan entry
    ou, oi = torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev)
    mu = torch.empty((T, L, U, d // 4), dtype=torch.uint8, device=dev)
    mi = torch.empty((T, L, I, d // 4), dtype=torch.uint8, device=dev)
    ops.gnn_stack(batch, u0, i0, L, LEAKY, ou, oi, mask_u=mu, mask_i=mi, drop=drop, time=te)
    got["ran"].add((R.batch_variant(batch.U, batch.I), "batched"))
    assert bool((ou == (u0 + u0) + u0).all(2)[:, empty].all()), "an empty row's stack output is (e0 + e0) + e0"
    assert not bool(mu[:, :, empty].any()), "an empty row's activation passes nothing through"
    for k in range(T):
        ku, ki = torch.empty((U, d), device=dev), torch.empty((I, d), device=dev)
        mku, mki = torch.empty_like(mu[k]), torch.empty_like(mi[k])
        ops.gnn_interval(pu[k], pi[k], u0[k], i0[k], L, LEAKY, ku, ki, mask_u=mku, mask_i=mki, drop=drop, interval=k,
                         time=None if te is None else te[k])
        got["ran"].add((R.variant(pu[k].n_rows), "per-plan"))
        assert torch.equal(ku, ou[k]) and torch.equal(ki, oi[k]), f"interval {k}: batched and per-plan outputs differ"
        assert torch.equal(mku, mu[k]) and torch.equal(mki, mi[k]), f"interval {k}: batched and per-plan masks differ"
    got["out_u"], got["out_i"] = ou[:, win].cpu(), oi.cpu()
    got["pos_u"], got["pos_i"] = _unpack(mu[:, :, win], d), _unpack(mi, d)
    del ou, ku

    if bwd:
        du, di = torch.empty((T, U, d), device=dev), torch.empty((T, I, d), device=dev)
        dte = torch.empty_like(te) if timed else None
        ops.gnn_stack_bwd(batch, gu, gi, L, LEAKY, mu, mi, du, di, drop=drop, time=te, grad_time=dte)
        assert bool((du == gu + (gu + gu)).all(2)[:, empty].all()), "an empty row's gradient is G + (G + G)"
        for k in range(T):
            dte_k = torch.empty_like(te[k]) if timed else None
            ku, ki = ops.gnn_interval_bwd(pu[k], pi[k], gu[k], gi[k], L, LEAKY, mu[k].contiguous(), mi[k].contiguous(),
                                          drop=drop, interval=k, time=None if te is None else te[k], grad_time=dte_k)
            assert torch.equal(ku, du[k]) and torch.equal(ki, di[k]), f"interval {k}: batched and per-plan gradients differ"
            assert dte is None or torch.equal(dte_k, dte[k]), f"interval {k}: batched and per-plan dTE differ"
        got["du"], got["di"] = du[:, win].cpu(), di.cpu()
        if timed:
            got["dte"] = dte.cpu()
    return got


def _check(pat, form, M, host, got, bwd):
    """The window rows of one pattern against float64."""
    _, dropped, timed = R.form_flags(form)
    d = pat.d
    rows_local = np.full(pat.n_rows, -1, np.int64)
    rows_local[pat.win] = np.arange(pat.win.size)
    drop = (SEED, STEP, D_THRESHOLD, 1.0 / KEEP) if dropped else None
    edges = [R.edge_list(p, rows_local, form, drop, k, M, L) for k, p in enumerate((pat, R.phantom(pat.n_rows, pat.n_src, d, pat.wide)))]
    u0, i0, gu, gi = (R.f64(host[n]) for n in ("u0", "i0", "gu", "gi"))
    te = R.f64(host["te"]) if timed else None
    y, acc, terms = R.one_product(edges[0], 1, 0, i0[0], None if te is None else te[0, 1, 0], LEAKY, u0[1], gu[0])
    assert_sum_close(got["prod_out"], y, terms, "one product, out")
    assert_sum_close(got["prod_acc"], acc, terms + gu[0].abs(), "one product, acc_out")
    ref = R.stack(edges, u0, i0, te, L, LEAKY, terms=True)
    assert_sum_close(got["out_u"], ref["out_u"], ref["terms_u"], "stack, users")
    assert_sum_close(got["out_i"], ref["out_i"], ref["terms_i"], "stack, items")
    # the recorded slopes: the sign of the float64 row sum wherever the bar leaves it no doubt
    slopes = []
    for k in range(T):
        slopes.append([])
        for l in range(L):
            pair = []
            for side, name in enumerate(("pos_u", "pos_i")):
                s, t = ref["sums"][k][l][side], ref["sum_terms"][k][l][side]
                sure = (s.abs() > 1e-4 * s.abs() + 1e-5 + 2e-7 * t).numpy()
                pos = got[name][k, l]
                assert np.array_equal(pos[sure], (s > 0).numpy()[sure]), f"activation mask, interval {k} layer {l} side {side}"
                assert not pos[(s == 0).numpy()].any()
                pair.append(torch.from_numpy(pos))
            slopes[-1].append(tuple(pair))
    if bwd:
        (du, di, dte), (t_du, t_di, t_dte) = R.stack_grads(edges, u0, i0, te, gu, gi, L, LEAKY, slopes)
        assert_sum_close(got["du"], du, t_du, "adjoint, users")
        assert_sum_close(got["di"], di, t_di, "adjoint, items")
        if timed:
            assert_sum_close(got["dte"], dte, t_dte, "adjoint, dTE")



def _case(dev, d, form, n_rows, M, n_src, twin, bwd=None, wide=False):
    """One pattern of n_rows rows (either side of 262,144) through every entry and against float64; twin: the large
    variant against the small one on the same windows. Returns the (variant, entry) pairs whose launches it made.
    tools/fuzz_gpu.py draws its row counts through this."""
    from sa_gnn_amd import ops
    bwd = d in R.BWD_WIDTHS if bwd is None else bwd
    big = R.pattern(d, n_rows, n_src, wide=wide)
    assert not twin or (R.variant(n_rows) == "large" and R.batch_variant(n_rows, n_src) == "large" and R.variant(n_src) == "small")
    assert _drop(ops).threshold == D_THRESHOLD and _drop(ops).scale == 1.0 / KEEP
    host = _host_operands(d, big.win.size, n_src, M, 7)
    got = _run(dev, big, form, M, host, bwd)
    _check(big, form, M, host, got, bwd)
    if not twin:
        return got["ran"]
    small = R.small_twin(big)
    assert R.batch_variant(small.n_rows, n_src) == "small" and small.win.size == big.win.size
    got_s = _run(dev, small, form, M, host, bwd)
    _check(small, form, M, host, got_s, bwd)
    # a row's summation order does not depend on the row block: the two variants agree bit for bit. A drop decides by
    # the user id, which the last window does not keep, and everything downstream of a product inherits that.
    same = slice(0, big.windows[0][1] + big.windows[1][1]) if R.form_flags(form)[1] else slice(None)
    for name in ("prod_out", "prod_acc"):
        assert torch.equal(got[name][same], got_s[name][same]), name
    if not R.form_flags(form)[1]:
        for name in got:
            a, b = got[name], got_s[name]
            if name != "ran":
                assert torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b), f"{name}: the variants differ"
    return got["ran"] | got_s["ran"]


@pytest.mark.parametrize("d,form,r,M,wide", CASES, ids=[f"d{d}{'w' * w}-{f}-r{r}-M{M}" for d, f, r, M, w in CASES])
def test_every_cell_against_float64_and_its_twin(dev, d, form, r, M, wide):
    ran = _case(dev, d, form, R.large_rows(K_BLOCKS, r), M, N_SRC, twin=True, wide=wide)
    assert {(v, d, form, e) for v, e in ran} == cells_of((d, form, r, M, wide)), "the case table promises these cells"


@pytest.mark.parametrize("d,form,r,M,n_items", ASYMMETRIC)
def test_asymmetric_batch_runs_few_item_rows_in_the_large_variant(dev, d, form, r, M, n_items):
    """U >= 262,144 with I < 16: the batch runs the item segments through the 16-row instantiation (one wave, cut), their
    own plans the small one; _run holds the two entries together bit for bit, _check both against float64. The cases of
    test_every_cell do the same at I = 3001, which is not a multiple of 64."""
    assert R.batch_variant(R.large_rows(K_BLOCKS, r), n_items) == "large" and R.variant(n_items) == "small" and N_SRC % 64
    _case(dev, d, form, R.large_rows(K_BLOCKS, r), M, n_items, twin=False)


@pytest.mark.parametrize("d,short_t", SHORT_EXACT)
def test_short_rows_are_the_sequential_sum(dev, d, short_t):
    """test_spmm_short_rows_bit_exact for the 16-row variant, with a short threshold past the lane group (the reload of a
    row's later slices): every short row equals the float32 sum in edge order exactly."""
    from sa_gnn_amd import ops
    rng = np.random.default_rng(d)
    n_rows, n_src, W = R.large_rows(1, 15), 257, 160
    starts = (0, 131072 - 32, (n_rows - W + 15) // 16 * 16)
    deg = np.zeros(n_rows, np.int64)
    for s in starts:
        n = min(W, n_rows - s)
        deg[s:s + n] = np.concatenate([[0, short_t, 1, R.lpr(d), R.lpr(d) + 1, short_t], rng.integers(0, short_t + 1, W - 6)])[:n]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = rng.integers(0, n_src, rowptr[-1]).astype(np.int32)
    plan = ops.SpmmPlan(rowptr, colidx, n_rows, n_src, device=dev, tuning=(short_t, 2 * short_t, 64))
    assert R.variant(n_rows) == "large" and plan.info.n_long_rows == 0 and deg.max() == short_t > R.lpr(d)
    x = rng.standard_normal((n_src, d)).astype(np.float32)
    y = ops.spmm(plan, torch.from_numpy(x).to(dev), LEAKY)
    rows = np.flatnonzero(deg)
    want = np.zeros((rows.size, d), np.float32)
    for j, row in enumerate(rows):
        for e in range(rowptr[row], rowptr[row + 1]):
            want[j] += x[colidx[e]]
    want = np.maximum(np.float32(LEAKY) * want, want)
    np.testing.assert_array_equal(y[torch.from_numpy(rows).to(dev)].cpu().numpy(), want)
    assert int(torch.count_nonzero(y.any(1))) <= rows.size


@pytest.mark.parametrize("form", ["weights", "time+weights"])
@pytest.mark.parametrize("d,wide", [(d, False) for d in R.BWD_WIDTHS] + [(d, True) for d in R.WIDE_WIDTHS])
def test_a_weight_travels_only_with_its_own_slice(dev, d, wide, form):
    """The short-row loop hands the next iteration's indices, weights and buckets over while the current gathers fly; a
    lane without an edge in the next slice must not keep the weight it held for this one. No finite weight can show that
    (a lane without an edge gathers zero), so the weights of the short rows of every other iteration are overwritten
    with infinity on the device: those rows turn non-finite, and every other row keeps its bits."""
    from sa_gnn_amd import ops
    M, G = 3, R.group(d)
    pat = R.pattern(d, R.large_rows(K_BLOCKS, 15), N_SRC, wide=wide)
    assert R.variant(pat.n_rows) == "large" and R.short_iters("large", d) >= 2
    plan = _plans(dev, pat, form, M)[0][0]
    gen = torch.Generator(device=dev).manual_seed(d)
    x, te = torch.randn((N_SRC, d), generator=gen, device=dev), torch.randn((M, d), generator=gen, device=dev)
    run = (lambda: ops.spmm_time(plan, x, LEAKY, te, want_out=True)) if R.form_flags(form)[2] else (lambda: ops.spmm_ex(plan, x, LEAKY, want_out=True))
    clean = run()
    labels = [label for label, block in R.window_blocks(d, wide) for _ in block]
    degs = R.window_degrees(d, wide)
    assert not wide or "wide_short" in labels
    pos = np.array([i for i, label in enumerate(labels) if label in ("ramp_up", "ramp_down", "alt_row", "wide_short")
                    and ((i % 16) // G) % 2 == 0 and degs[i] > 0])
    rows = np.concatenate([start + pos[pos < length] for start, length in pat.windows])
    assert all(R.row_class(x_, pat.tuning) == "short" for x_ in pat.deg[rows])
    plan.weights[torch.from_numpy(np.flatnonzero(np.isin(pat.rows, rows))).to(dev)] = float("inf")
    poisoned = run()
    others = torch.ones(pat.n_rows, dtype=torch.bool, device=dev)
    others[torch.from_numpy(rows).to(dev)] = False
    assert not bool(torch.isfinite(poisoned[~others]).all(1).any()), "a poisoned row stayed finite"
    assert torch.equal(poisoned[others], clean[others]), "a row changed with the weights of another row"


@pytest.mark.parametrize("var", R.VARIANTS)
def test_strided_operands_and_untouched_padding(dev, var):
    """[N, T, d] column views and padded row strides through the batched entry, on each variant: the same bits as the
    contiguous call, and the NaN padding between rows still NaN."""
    from sa_gnn_amd import ops
    d, form, M, pad = 64, "plain", 3, 8
    pat = R.pattern(d, R.large_rows(K_BLOCKS, 15), N_SRC)
    if var == "small":
        pat = R.small_twin(pat)
    U, I = pat.n_rows, pat.n_src
    assert R.batch_variant(U, I) == var
    pu, pi = _plans(dev, pat, form, M)
    batch = ops.SpmmBatch(pu, pi)
    gen = torch.Generator(device=dev).manual_seed(5)
    nan = float("nan")
    plain_in = [torch.randn((T, n, d), generator=gen, device=dev) for n in (U, I)]
    plain_out = [torch.empty((T, n, d), device=dev) for n in (U, I)]
    ops.gnn_stack(batch, plain_in[0], plain_in[1], L, LEAKY, plain_out[0], plain_out[1])
    padded_in = [torch.full((T, n, d + pad), nan, device=dev) for n in (U, I)]          # rows d + pad apart
    padded_out = [torch.full((n, T, d + pad), nan, device=dev) for n in (U, I)]         # [N, T, d + pad]: interval columns
    for x, xp in zip(plain_in, padded_in):
        xp[:, :, :d] = x
    views = [op.permute(1, 0, 2)[:, :, :d] for op in padded_out]
    ops.gnn_stack(batch, padded_in[0][:, :, :d], padded_in[1][:, :, :d], L, LEAKY, views[0], views[1])
    for v, want, xp, op in zip(views, plain_out, padded_in, padded_out):
        assert torch.equal(v, want) and not bool(torch.isnan(want).any())
        assert bool(torch.isnan(xp[:, :, d:]).all()) and bool(torch.isnan(op[:, :, d:]).all())


def test_the_refused_neighbours_are_refused(dev):
    """The cells next to the table that spmm_routes_ref.REFUSED names: a drop with a time term, and the widths check_d
    turns away."""
    from sa_gnn_amd import ops
    from sa_gnn_amd._lib import SagnnError
    plan = ops.SpmmPlan(np.array([0, 1], np.int32), np.array([0], np.int32), 1, 1, device=dev, buckets=np.zeros(1, np.uint16), n_buckets=3)
    batch = ops.SpmmBatch([plan], [plan])
    for d in (2, 6, 260):
        assert not R.check_d(d)
        with pytest.raises((SagnnError, ValueError), match=re.escape(R.REFUSED[f"d={d}"])):
            ops.spmm(plan, torch.zeros((1, d), device=dev), LEAKY)
    x = torch.zeros((1, 1, 8), device=dev)
    with pytest.raises((SagnnError, ValueError), match=R.REFUSED["drop+time"]):
        ops.gnn_stack(batch, x, x.clone(), 1, LEAKY, torch.empty_like(x), torch.empty_like(x), drop=_drop(ops),
                      time=torch.zeros((1, 1, 2, 3, 8), device=dev))
