"""CPU checks of tests/test_gpu_bwd_routes.py: its Python restatement of the three backward selectors against the library's
own queries, and its case lists against the instantiations they are there to reach. No device is touched."""
import itertools

from sa_gnn_amd import _lib
import test_gpu_bwd_routes as R


def test_python_selectors_agree_with_the_library_queries():
    """Over the domain of the golden sweep (tests/test_host.py::engine_selection_sweep): 3 engines x d in {4, 8, .., 256} x
    t in 1..32 x heads in {1, 2, 4, .., 32}. The table's note on VALU, stated here: the two attention _supported queries
    answer 0 under it although the _f32 entries run the f16x2 choice, which is what front_route / tail_route give."""
    lib = _lib.load()
    prev = lib.sagnn_get_engine()
    try:
        for code, engine in enumerate(R.ENGINES):
            assert lib.sagnn_set_engine(code) == 0
            valu = engine == "valu"
            for d in range(4, 257, 4):
                assert lib.sagnn_attn_bwd_tail_supported(d) == (0 if valu else int(R.tail_route(engine, d) != "None")), (engine, d)
                assert lib.sagnn_lstm_bwd_supported(d) == int(R.bptt_route(engine, d, False) != "None"), (engine, d)
                assert (R.bptt_route(engine, d, True) != "None") == (R.bptt_route(engine, d, False) != "None")
                for t, heads in itertools.product(range(1, 33), (1, 2, 4, 8, 16, 32)):
                    want = 0 if valu else int(R.front_route(engine, d, t, heads) != "None")
                    assert lib.sagnn_attn_bwd_front_supported(d, t, heads) == want, (engine, d, t, heads)
                    if valu:                             # the entry's choice under VALU is the f16x2 one
                        assert R.front_route("valu", d, t, heads) == R.front_route("f16x2", d, t, heads)
            if valu:
                assert all(R.tail_route("valu", d) == R.tail_route("f16x2", d) for d in range(4, 257, 4))
    finally:
        lib.sagnn_set_engine(prev)


def test_case_lists_reach_every_instantiation():
    for case in R.FRONT_CASES:
        engine, d, t, heads, n, route = case
        assert R.front_route(engine, d, t, heads) == route, case
    # F32Mfma: ln_mhsa_mean_mfma_kernel<D, T, true> with attention_pairs_bwd<D, DK, QS, T>: 2 x 7 x 2 = 28
    mfma = {(d, t, d // h) for e, d, t, h, n, r in R.FRONT_CASES if r == "F32Mfma"}
    assert mfma == set(itertools.product((32, 64), R.MFMA_BWD_FRONT_T, (2, 4))) and len(mfma) == 28
    # ... each at n = 1 and on both sides of a tile, 16 heads under f32 and (32, 8) / (64, 32 heads) under f16x2
    # (R.MFMA_SHAPES); each (d, d_k) under valu where it can
    # be reached (16 heads are Split's there), and once in the steady state
    for e, d, h in R.MFMA_SHAPES:
        for t in R.MFMA_BWD_FRONT_T:
            ns = {n for e2, d2, t2, h2, n, r in R.FRONT_MFMA if (e2, d2, t2, h2) == (e, d, t, h)}
            assert {1, R.mfma_tile(t) - 1, R.mfma_tile(t) + 1} <= ns, (e, d, t, h)
        assert (e, d, R.STEADY_T[d, d // h], h, "steady", "F32Mfma") in R.FRONT_MFMA
    assert sorted(R.STEADY_T.values()) == [1, 3, 5, 8] and set(R.STEADY_T) == set(itertools.product((32, 64), (2, 4)))
    assert {(d, d // h) for e, d, t, h, n, r in R.FRONT_MFMA if e == "valu"} == {(32, 4), (64, 2)}
    # both sides of the gpre[] select chain: full waves of at most 64 pairs and of more
    pairs = {(d, t, h): R.mfma_pairs(d, t, h) for e, d, t, h, n, r in R.FRONT_MFMA if n != 1}
    assert any(v <= 64 for v in pairs.values()) and all(pairs[64, t, 32] > 64 for t in R.MFMA_BWD_FRONT_T)
    assert all(pairs[32, t, 8] > 64 for t in (1, 2, 3)) and all(pairs[32, t, 8] <= 64 for t in (4, 5, 6, 8))
    # a steady-state count makes every block of one per CU loop and leaves a ragged last tile, at any CU count
    for cus in (1, 80, 256, 304):
        for t in R.STEADY_T.values():
            tiles, rest = divmod(R.nodes_of("steady", t, cus), R.mfma_tile(t))
            assert tiles == 2 * cus and 0 < rest < R.mfma_tile(t)
    # Split: ln_mhsa_split_kernel<D, T, LP, true> at d = 128 for t = 1..6 and at d = 32 / 64 for every t of the forward
    split = {(d, t) for e, d, t, h, n, r in R.FRONT_CASES if r == "Split" and e == "f16x2"}
    assert split == ({(128, t) for t in R.SPLIT_BWD_FRONT_T128} | set(itertools.product((32, 64), R.SPECIALISED_T)))
    assert {(d) for e, d, t, h, n, r in R.FRONT_CASES if r == "Split" and e == "valu"} == {64, 128}
    for d, t in split:
        ns = {n for e, d2, t2, h, n, r in R.FRONT_SPLIT if (d2, t2) == (d, t)}
        assert {R.split_tile(t) - 1, R.split_tile(t) + 1} <= ns
    # the None rows: a t outside both tables under f16x2 and under f32, d = 128 under f32, d_k = 8, d = 128 past t = 6
    assert set(R.FRONT_NONE) == {("f16x2", 64, 7, 16), ("f32", 64, 12, 16), ("f32", 128, 3, 16), ("f16x2", 64, 3, 8), ("f16x2", 128, 8, 16)}
    assert all(R.front_route(*c) == "None" for c in R.FRONT_NONE)
    # tail: both routes at both widths, F16x2 under both engines that reach it; every small-row edge and a steady state
    assert {(e, d, r) for e, d, rows, r in R.TAIL_CASES} == (
        {("f32", d, "F32Mfma") for d in (32, 64)} | {(e, d, "F16x2") for e in ("f16x2", "valu") for d in (32, 64)})
    for e, d in {(e, d) for e, d, rows, r in R.TAIL_CASES}:
        assert {rows for e2, d2, rows, r in R.TAIL_CASES if (e2, d2) == (e, d)} == {1, 3, 31, 32, 33, 35, 66, "steady"}
    for cus in (1, 80, 256, 304):
        chunks, rest = divmod(R.rows_of("steady", cus), 32)
        assert chunks + 1 >= 2 * (2 * cus) and 0 < rest < 4      # every block of the widest launch has >= 2 chunks
        assert chunks >= 2 * cus, "the ragged chunk (index `chunks`) would be a block's first"
    assert {d for e, d in R.TAIL_NONE} == {96, 128} and all(R.tail_route(e, d) == "None" for e, d in R.TAIL_NONE)
    # BPTT: the four cells of select_lstm_bwd: lstm_bwd_mfma_kernel<D, true> and <D, false> + the weight-gradient pass
    assert {(e, ws, r) for e, ws, d, t, n, r in R.BPTT_CASES} == {
        ("f16x2", False, "OneLaunch"), ("f16x2", True, "SplitDw"), ("f32", True, "OneLaunch"), ("valu", True, "OneLaunch")}
    for e, ws, d, t, n, r in R.BPTT_CASES:
        assert R.bptt_route(e, d, ws) == r
    assert {(r, d, t, n) for e, ws, d, t, n, r in R.BPTT_CASES} == set(
        itertools.product(("OneLaunch", "SplitDw"), (32, 64), (1, 2, 5), (1, 31, 33, "steady")))
    for cus in (1, 80, 256, 304):
        chunks, rest = divmod(R.bptt_nodes_of("steady", cus), 32)
        assert chunks + 1 >= 2 * cus and 0 < rest < 32
