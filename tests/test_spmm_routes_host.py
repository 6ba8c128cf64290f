"""CPU checks of tests/test_gpu_spmm_routes.py: the restated SpMM selection (spmm_routes_ref) against the case table, which
must reach every cell of variant x width x form x entry; the window layout against the kernel logic each of its blocks is
there for; and the float64 reference against a dense restatement and a finite difference. No device is touched."""
import itertools

import numpy as np
import torch

import edge_time_ref as E
import spmm_routes_ref as R
import test_gpu_spmm_routes as G


def test_case_table_reaches_every_cell():
    reached = set().union(*(G.cells_of(c) for c in G.CASES))
    assert reached == R.all_cells() and len(reached) == 2 * 6 * 6 * 2
    # no cell of the table is refused; the refusals lie next to it
    assert all(R.check_d(d) for d in R.WIDTHS) and not any(R.check_d(d) for d in (0, 2, 6, 260))
    for w, dr, tm in itertools.product((False, True), repeat=3):
        if dr and tm:
            try:
                R.form_name(w, dr, tm)
                raise AssertionError("drop + time has a name")
            except ValueError as e:
                assert str(e) == R.REFUSED["drop+time"]
        else:
            assert R.form_flags(R.form_name(w, dr, tm)) == (w, dr, tm)
    assert {R.form_name(*f) for f in itertools.product((False, True), repeat=3) if not (f[1] and f[2])} == set(R.FORMS)
    # what a case runs is what its cells say: the row counts on each side of kSmallRows, per plan and per batch
    assert len(G.CASES) == 36 + 6 and {(d, f) for d, f, r, M, wide in G.CASES if wide} == set(itertools.product(R.WIDE_WIDTHS, R.FORMS))
    for d, form, r, M, wide in G.CASES:
        big = R.large_rows(G.K_BLOCKS, r)
        twin = R.small_twin(R.pattern(d, big, G.N_SRC, wide=wide))
        assert R.variant(twin.n_rows) == "small" and R.batch_variant(twin.n_rows, G.N_SRC) == "small"
        assert big == 262144 + 64 * G.K_BLOCKS + r and R.variant(big) == "large" and R.batch_variant(big, G.N_SRC) == "large"
        assert R.variant(G.N_SRC) == "small" and R.batch_variant(G.N_SRC, G.N_SRC) == "small"
        last_wave = big % 16 or 16
        assert last_wave == r % 16 or (r == 16 and last_wave == 16)
        assert (big % 64 + 15) // 16 == 1, "the last block holds one wave with rows and three idle ones"
    assert R.variant(262143) == "small" and R.variant(262144) == "large" and R.batch_variant(262144, 5) == "large"
    assert {G.TAIL_R[i] % 16 or 16 for i in range(3)} == {1, 15, 16}
    for d in R.WIDTHS:
        assert {r for d2, f, r, M, wide in G.CASES if d2 == d and not wide} == set(G.TAIL_R)
    for form in R.FORMS:
        assert {r for d, f, r, M, wide in G.CASES if f == form} == set(G.TAIL_R)
        if form.startswith("time"):
            assert {M for d, f, r, M, wide in G.CASES if f == form} == set(G.BUCKETS) == {3, 300}
    assert {r for d, f, r, M, wide in G.CASES if wide} == set(G.TAIL_R)
    # lane groups and loop counts: the 16-row variant at d = 64 / 128 / 256 runs 4 / 8 / 16 short-loop iterations, the
    # small variant at d <= 64 exactly one
    assert [R.lpr(d) for d in R.WIDTHS] == [8, 8, 16, 16, 32, 64]
    assert [R.lpr(d) for d in (32, 33, 64, 65, 128, 129, 256)] == [8, 16, 16, 32, 32, 64, 64]
    assert [R.short_iters("large", d) for d in (32, 64, 128, 256)] == [2, 4, 8, 16]
    assert [R.short_iters("small", d) for d in (4, 32, 48, 64, 128, 256)] == [1, 1, 1, 1, 2, 4]
    assert [R.rpw("small", d) for d in (32, 64, 128, 256)] == [8, 4, 4, 4] and R.rpw("large", 64) == 16
    assert sorted({R.lpr(d) for d in R.BWD_WIDTHS}) == [8, 16, 32, 64] and set(R.BWD_WIDTHS) <= set(R.WIDTHS)
    # the asymmetric batch: few item rows in the 16-row variant; the bit-exact cases past the lane group
    assert all(n < 16 and R.batch_variant(R.large_rows(G.K_BLOCKS, r), n) == "large" for _, _, r, _, n in G.ASYMMETRIC)
    assert G.N_SRC % 64 != 0 and all(st > R.lpr(d) for d, st in G.SHORT_EXACT) and [d for d, _ in G.SHORT_EXACT] == [32, 64, 128, 256]


def _classes(degs, tuning):
    return [R.row_class(x, tuning) for x in degs]


def test_window_layout_names_every_piece_of_kernel_logic():
    # short rows wider than a lane group run at EVERY lane-group width: LPR = 64 through the second tuning of d = 256
    assert {R.lpr(d) for d in R.WIDTHS if R.tuning_for(d)[0] > R.lpr(d)} | {R.lpr(d) for d in R.WIDE_WIDTHS} == {8, 16, 32, 64}
    for d, wide in [(d, False) for d in R.WIDTHS] + [(d, True) for d in R.WIDE_WIDTHS]:
        st, lt, ch = tuning = R.tuning_for(d, wide)
        lanes, G_ = R.lpr(d), R.group(d)
        blocks = dict(R.window_blocks(d, wide))
        assert all(len(b) == 16 for b in blocks.values())
        assert d != 32 or (tuning == R.DEFAULT_TUNING and st > lanes)                      # the defaults, where 16 > 8
        # degree ramps: 0 .. short_thresh up, down, alternating by row and by iteration (both phases)
        assert blocks["ramp_up"] == sorted(blocks["ramp_up"]) and blocks["ramp_up"][0] == 0 and blocks["ramp_up"][-1] == st
        assert blocks["ramp_down"] == blocks["ramp_up"][::-1] and blocks["alt_row"] == [0, st] * 8
        its = lambda b: [tuple(b[i:i + G_]) for i in range(0, 16, G_)]
        assert its(blocks["alt_iter"]) == [(0,) * G_, (st,) * G_] * (8 // G_)
        assert its(blocks["alt_iter_inv"]) == [(st,) * G_, (0,) * G_] * (8 // G_)
        # short rows wider than a lane group in one iteration with narrower ones
        assert ("wide_short" in blocks) == (lanes < 64 or wide)
        if "wide_short" in blocks:
            ws = its(blocks["wide_short"])
            assert st > lanes and any(max(t) > lanes for t in ws) and all(max(t) <= st for t in ws)
            assert G_ == 1 or all(max(t) > lanes and min(t) <= lanes for t in ws)
        # every class at every position modulo G
        seen = {(i % G_, c) for s in range(4) for i, c in enumerate(_classes(blocks[f"mixed_{s}"], tuning))}
        assert seen == set(itertools.product(range(G_), ("empty", "short", "medium", "long")))
        # 16 medium rows (every ballot bit), 16 long rows (nothing for the row wave to finish)
        assert set(_classes(blocks["all_medium_0"], tuning)) == {"medium"} and set(_classes(blocks["all_long"], tuning)) == {"long"}
        medium = {x for b in blocks.values() for x in b if R.row_class(x, tuning) == "medium"}
        assert ({129} if wide else {63, 64, 65, 129}) <= medium and {x % (G_ * R.UNROLL) for x in medium} == set(range(G_ * R.UNROLL))
        assert not wide or (st > 65 and {63, 64, 65} <= {x for b in blocks.values() for x in b})        # short rows there
        cuts = [R.chunks_of(x, ch) for b in blocks.values() for x in b if R.row_class(x, tuning) == "long"]
        assert any(len(c) >= 3 and c[-1] == 1 for c in cuts) and all(sum(c) > lt for c in cuts)
        assert any(len(c) == 1 for c in cuts) == (d != 32), "the default thresholds have no long row of one chunk"
        assert blocks["tail_mix"][0] > 0, "a last wave of one row holds a row with edges"
        # the pattern: three windows, 16-aligned, the middle one across a 64-row block boundary, the last one cut
        for r in G.TAIL_R:
            pat = R.pattern(d, R.large_rows(G.K_BLOCKS, r), G.N_SRC, wide=wide)
            (s0, W), (s1, _), (s2, n2) = pat.windows
            assert s0 == 0 and s1 % 64 == 32 and s1 // 64 != (s1 + W - 1) // 64 and s2 % 16 == 0 and s2 + n2 == pat.n_rows
            assert (n2 % 16 or 16) == (r % 16 or 16) and pat.n_rows - pat.win.size == int((pat.deg == 0).sum()) - int((pat.deg[pat.win] == 0).sum())
            assert pat.rowptr[-1] == pat.colidx.size < 120_000 and pat.colidx.max() < G.N_SRC
            dup = [row for row in pat.win if pat.deg[row] >= 2 and pat.colidx[pat.rowptr[row]] == pat.colidx[pat.rowptr[row] + 1]]
            assert {"short", "medium"} <= {R.row_class(pat.deg[row], tuning) for row in dup}
            assert (pat.weights == 0).any() and (pat.weights < 0).any()
            small = R.small_twin(pat)
            assert R.variant(small.n_rows) == "small" and small.windows[:2] == pat.windows[:2] and small.windows[2][1] == n2
            assert np.array_equal(small.colidx, pat.colidx) and np.array_equal(small.weights, pat.weights)
            assert np.array_equal(small.deg[small.win], pat.deg[pat.win]) and np.array_equal(small.buckets[300], pat.buckets[300])
            rp_t, ci_t, order = pat.transposed()
            assert np.array_equal(pat.colidx[order], np.repeat(np.arange(G.N_SRC), np.diff(rp_t))) and np.array_equal(pat.rows[order], ci_t)


def _cut_down(d, form, M):
    """A pattern of the generator with few rows and 97 items, its phantom interval, and float64 operands."""
    pat = R.pattern(d, 1200 + 15, 97, seed=3)
    rows_local = np.full(pat.n_rows, -1, np.int64)
    rows_local[pat.win] = np.arange(pat.win.size)
    drop = (G.SEED, G.STEP, G.D_THRESHOLD, 1.0 / G.KEEP) if R.form_flags(form)[1] else None
    edges = [R.edge_list(p, rows_local, form, drop, k, M, G.L) for k, p in enumerate((pat, R.phantom(pat.n_rows, 97, d)))]
    host = G._host_operands(d, pat.win.size, 97, M, 11)
    te = R.f64(host["te"]) if R.form_flags(form)[2] else None
    return pat, edges, tuple(R.f64(host[n]) for n in ("u0", "i0", "gu", "gi")), te


def test_reference_agrees_with_its_dense_restatement():
    for form, M in zip(R.FORMS, (3, 3, 3, 3, 3, 300)):
        pat, edges, (u0, i0, gu, gi), te = _cut_down(8, form, M)
        ref = R.stack(edges, u0, i0, te, G.L, G.LEAKY, terms=True)
        want_u, want_i = R.dense_stack(edges, u0, i0, te, G.L, G.LEAKY)
        np.testing.assert_allclose(ref["out_u"].numpy(), want_u, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref["out_i"].numpy(), want_i, rtol=1e-12, atol=1e-12)
        # the terms bound the values they belong to, and the rows outside every edge keep (e0 + e0) + e0
        assert bool((ref["terms_u"] >= ref["out_u"].abs() - 1e-9).all()) and bool((ref["terms_i"] >= ref["out_i"].abs() - 1e-9).all())
        lone = pat.deg[pat.win] == 0
        lone[0] = False                                                                   # row 0 holds the phantom edge
        np.testing.assert_allclose(ref["out_u"][:, lone].numpy(), 3 * u0[:, lone].numpy(), rtol=1e-15)
        if R.form_flags(form)[1]:                                                          # a drop removes edges
            kept = [float((c != 0).double().mean()) for c in edges[0]["coef"][0]]
            assert all(0.3 < x < 0.6 for x in kept) and not torch.equal(edges[0]["coef"][0][0], edges[0]["coef"][1][0])
        # one product, dense
        y, acc, terms = R.one_product(edges[0], 1, 0, i0[0], None if te is None else te[0, 1, 0], G.LEAKY, u0[1], gu[0])
        a = np.zeros((u0.shape[1], 97))
        np.add.at(a, (edges[0]["u"].numpy(), edges[0]["i"].numpy()), edges[0]["coef"][1][0].numpy())
        s = a @ i0[0].numpy()
        if te is not None:
            c = np.zeros((u0.shape[1], M))
            np.add.at(c, (edges[0]["u"].numpy(), edges[0]["b"].numpy()), edges[0]["coef"][1][0].numpy())
            s = s + c @ te[0, 1, 0].numpy()
        np.testing.assert_allclose(y.numpy(), np.maximum(G.LEAKY * s, s) + u0[1].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(acc.numpy(), y.numpy() + gu[0].numpy(), rtol=1e-15)
        assert bool((terms >= (y - u0[1]).abs() - 1e-9).all())


def test_reference_gradients_agree_with_a_finite_difference():
    for form in ("weights", "drop", "time+weights"):
        pat, edges, (u0, i0, gu, gi), te = _cut_down(8, form, 3)
        ref = R.stack(edges, u0, i0, te, G.L, G.LEAKY)
        slopes = [[(su > 0, si > 0) for su, si in sk] for sk in ref["sums"]]
        (du, di, dte), (t_du, t_di, t_dte) = R.stack_grads(edges, u0, i0, te, gu, gi, G.L, G.LEAKY, slopes)
        loss = lambda u, i, t: float(((lambda r: (r["out_u"] * gu).sum() + (r["out_i"] * gi).sum())(R.stack(edges, u, i, t, G.L, G.LEAKY))))
        rng = np.random.default_rng(5)
        vu, vi = R.f64(rng.standard_normal(u0.shape)), R.f64(rng.standard_normal(i0.shape))
        vt = None if te is None else R.f64(rng.standard_normal(te.shape))
        eps = 1e-7                          # the stack is piecewise linear: exact up to the rows whose sign flips within eps
        plus = loss(u0 + eps * vu, i0 + eps * vi, None if te is None else te + eps * vt)
        minus = loss(u0 - eps * vu, i0 - eps * vi, None if te is None else te - eps * vt)
        want = float((du * vu).sum() + (di * vi).sum() + (0 if te is None else (dte * vt).sum()))
        assert abs((plus - minus) / (2 * eps) - want) <= 1e-5 * max(abs(want), 1.0)
        assert bool((t_du >= du.abs() - 1e-9).all()) and bool((t_di >= di.abs() - 1e-9).all())
        assert te is None or bool((t_dte >= dte.abs() - 1e-9).all())


def test_buckets_and_time_adjoint_are_those_of_edge_time_ref():
    """The time forms take the pattern's buckets as tests/edge_time_ref.py states them: one id per stored edge in edge order,
    s[r] = sum_e w[e] (X[col[e]] + TE[bucket[e]]); the plan's dTE pattern is edge_time_ref.time_adjoint of them, and the
    reference's dTE (autograd) is that pattern applied to the masked gradient."""
    from sa_gnn_amd import ops
    pat = R.pattern(8, 1200 + 1, 97, seed=3)
    for M in G.BUCKETS:
        b = pat.buckets[M]
        assert b.dtype == np.uint16 and b.size == pat.colidx.size and b.max() < M and len(set(b.tolist())) == min(M, 300)
        want = E.time_adjoint(pat.rowptr, b, M, pat.weights)
        got = ops.time_adjoint_arrays(pat.rowptr, b, M, pat.weights)
        assert all(np.array_equal(a, c) for a, c in zip(got, want))
    assert R.phantom(5, 3, 8).buckets[3].tolist() == [0]                                   # the phantom edge: bucket 0
    # one layer, slope 1: dTE[0, 0, 0] = C^T gu with C[r, b] the summed weight of row r's edges in bucket b
    pat2, edges, (u0, i0, gu, gi), te = _cut_down(8, "time+weights", 3)
    ones = [[(torch.ones_like(u0[0], dtype=torch.bool), torch.ones_like(i0[0], dtype=torch.bool))]] * 2
    (du, di, dte), _ = R.stack_grads(edges, u0, i0, te[:, :1], gu, gi, 1, 1.0, ones)
    rp, ci, w = E.time_adjoint(pat2.rowptr, pat2.buckets[3], 3, pat2.weights)
    rows_local = np.full(pat2.n_rows, -1, np.int64)
    rows_local[pat2.win] = np.arange(pat2.win.size)
    want = np.stack([(w[rp[b]:rp[b + 1], None].astype(np.float64) * gu[0].numpy()[rows_local[ci[rp[b]:rp[b + 1]]]]).sum(0) for b in range(3)])
    np.testing.assert_allclose(dte[0, 0, 0].numpy(), want, rtol=1e-12, atol=1e-12)
