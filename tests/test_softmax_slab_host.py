"""CPU checks of the slab-shaped softmax-loss cases: the builder's structure, and the rule the sibling
suites derive their constants by (K = 4 x float32 on the CPU): every case test_gpu_softmax_slab.py runs must, in float32
torch on the CPU, need at most a quarter of K_LSE, K_DQ and K_DI against float64. An input that misses that is changed,
never the bound. The printed ratios are the table of profiles/softmax_slab.txt."""
import numpy as np
import pytest

import softmax_slab_ref as S
from test_gpu_softmax_loss import K_DI, K_DQ, K_LSE


@pytest.mark.parametrize("last_live", [True, False])
@pytest.mark.parametrize("mode,n_items,n_cand", S.MODES)
def test_the_small_slab_holds_the_structure_it_promises(mode, n_items, n_cand, last_live):
    c = S.build(mode, n_items, n_cand, 32, 1.0, last_live=last_live)
    S.assert_small_structure(c)
    live = c["structure"]["live"]
    assert int(live.sum()) == (112 if last_live else 108) and float(c["g"]) == float(np.float32(1.0 / live.sum()))
    assert np.log2(float(c["g"])) % 1 != 0                 # an upstream gradient that is no power of two
    again = S.build(mode, n_items, n_cand, 32, 1.0, last_live=last_live)
    assert all(np.array_equal(c[k], again[k]) for k in ("Q", "I", "target", "excl_row", "ptr", "items"))


def test_the_long_slab_makes_every_loop_take_several_trips():
    c = S.build(*S.LONG_CASE, long=True)
    rows, live = len(c["target"]), c["structure"]["live"]
    assert rows == S.LONG_SLOTS * S.LONG_POS == 2560 and 0.10 < live.mean() < 0.20
    assert rows // 256 >= 4 and rows // S.GROUP >= 4 and len(c["cand"]) > 2 * 128       # loss_sum, di_kernel's groups, chunks
    assert c["structure"]["skipped_groups"] and min(c["structure"]["rows_per_list"].values()) >= 3


def _screen(c):
    got = S.float32_eval(c)
    need = S.needs(c, got)
    tol = S.loss_tolerance(c, K_LSE)
    print(f"softmax_slab|cpu32|{c['name']}|lse {need['lse']:.2f} / {K_LSE // 4}, tscore {need['tscore']:.2f} / {K_LSE // 4}, "
          f"dQ {need['dQ']:.2f} / {K_DQ // 4}, dI {need['dI']:.2f} / {K_DI // 4}, loss {abs(got['loss'] - c['ref']['loss']) / tol:.3f} of its tolerance")
    assert need["lse"] <= K_LSE / 4 and need["tscore"] <= K_LSE / 4 and need["dQ"] <= K_DQ / 4 and need["dI"] <= K_DI / 4, need
    assert abs(got["loss"] - c["ref"]["loss"]) <= tol / 4


@pytest.mark.parametrize("mode,n_items,n_cand,d,temp", S.CASES)
def test_float32_on_the_cpu_needs_at_most_a_quarter_of_each_constant(mode, n_items, n_cand, d, temp):
    _screen(S.build(mode, n_items, n_cand, d, temp))


def test_float32_on_the_cpu_needs_at_most_a_quarter_of_each_constant_on_the_long_slab():
    _screen(S.build(*S.LONG_CASE, long=True))
