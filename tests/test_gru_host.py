"""CPU suite of the opt-in GRU cell of the interval fusion (--rnnCell gru): the float64 restatements of
gru_ref agree with each other, the per-step backward formulas the library's host loop sequences equal float64 autograd,
the zero-state shortcut, the flag, prepareModel's and the interval-parallel path's refusals, sagnn_gru_fused_supported's
table and the argument checks of the new entries (each rejected before any device work, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
import torch

import gru_ref as G
from sa_gnn_amd import _lib


def _case(seed, n, t, d, with_drop):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, t, d))
    p = G.init_gru_params(d, rng, np.float64)
    drop = ((rng.random((n, t, d)) < 0.5) * 2.0) if with_drop else None
    return rng, x, [p[k] for k in G.GRU_KEYS], drop


@pytest.mark.parametrize("with_drop", [False, True])
def test_numpy_and_torch_restatements_agree(with_drop):
    _, x, w, drop = _case(1, 9, 5, 8, with_drop)
    a = G.gru(x, *w, drop=drop)
    t = torch.from_numpy
    b = G.torch_gru(t(x), *(t(v) for v in w), drop=None if drop is None else t(drop)).numpy()
    assert np.abs(a - b).max() <= 1e-12
    out, gates, cand, raw = G.gru(x, *w, drop=drop, want_saved=True)
    assert np.array_equal(out, a) and gates.shape == (9, 5, 16) and cand.shape == (9, 5, 8)
    assert np.array_equal(out, raw if drop is None else raw * drop)   # the state itself is never dropped


@pytest.mark.parametrize("with_drop", [False, True])
def test_step_formulas_equal_float64_autograd(with_drop):
    """DESIGN.md §22's per-step backward (gru_ref.bptt_steps restates it as the host loop sequences the entries) against
    autograd of torch_gru: dx and all four parameter gradients, t = 3, n = 7, d = 8."""
    rng, x, w, drop = _case(2, 7, 3, 8, with_drop)
    g = rng.standard_normal((7, 3, 8))
    leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (x, *w)]
    # dh_ext is the gradient at the EMITTED h: the drop scale is applied inside the step, as in the library
    (G.torch_gru(*leaves, drop=None if drop is None else torch.from_numpy(drop)) * torch.from_numpy(g)).sum().backward()
    got = G.bptt_steps(x, *w, g, drop=drop)
    for name, a, leaf in zip(("dx", "dWg", "dbg", "dWc", "dbc"), got, leaves):
        want = leaf.grad.numpy()
        assert np.abs(a - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), name


def test_one_step_is_the_zero_state_shortcut():
    """t = 1: h = (1 - u) tanh(x Wc[:d] + bc) with u from the x half alone; neither recurrent half contributes."""
    _, x, (Wg, bg, Wc, bc), _ = _case(3, 6, 1, 8, False)
    d = 8
    u = 1.0 / (1.0 + np.exp(-(x[:, 0] @ Wg[:d, d:] + bg[d:])))
    want = (1.0 - u) * np.tanh(x[:, 0] @ Wc[:d] + bc)
    assert np.abs(G.gru(x, Wg, bg, Wc, bc)[:, 0] - want).max() <= 1e-14
    # rows d..2d-1 of either kernel do not reach the first step's result
    rng = np.random.default_rng(4)
    Wg2, Wc2 = Wg.copy(), Wc.copy()
    Wg2[d:], Wc2[d:] = rng.standard_normal((d, 2 * d)), rng.standard_normal((d, d))
    assert np.array_equal(G.gru(x, Wg2, bg, Wc2, bc), G.gru(x, Wg, bg, Wc, bc))


def test_flag_parses_and_defaults_to_lstm():
    from sa_gnn_amd import Params
    assert Params.build_parser().parse_args([]).rnnCell == "lstm" and Params.args.rnnCell == "lstm"
    assert Params.build_parser().parse_args(["--rnnCell", "gru"]).rnnCell == "gru"
    with pytest.raises(SystemExit):
        Params.build_parser().parse_args(["--rnnCell", "rnn"])
    text = " ".join(Params.build_parser().format_help().lower().split())
    assert "--rnncell {lstm,gru}" in text and "model.py:135-136" in text


def test_prepare_model_refuses_a_bad_cell_and_a_bad_width(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    monkeypatch.setattr(args, "user", 10, raising=False)
    monkeypatch.setattr(args, "item", 10, raising=False)
    for cell, d, text in (("rnn", 64, "--rnnCell rnn: one of"), ("gru", 48, "--rnnCell gru needs latdim.*got 48"),
                          ("gru", 288, "--rnnCell gru needs latdim.*got 288"), ("gru", 16, "--rnnCell gru needs latdim.*got 16")):
        monkeypatch.setattr(args, "rnnCell", cell)
        monkeypatch.setattr(args, "latdim", d)
        with pytest.raises(ValueError, match=text):
            Recommender("cpu", None).prepareModel()              # refused before the handler or the device is touched


def test_interval_sharding_refuses_gru(monkeypatch):
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.parallel import IntervalSharding
    assert IntervalSharding(4, 2, 0).rounds == 2
    monkeypatch.setattr(args, "rnnCell", "gru")
    with pytest.raises(ValueError, match="--rnnCell gru is not supported by the interval-parallel path"):
        IntervalSharding(4, 2, 0)


def test_fusion_cell_dispatch_refuses_both_or_neither():
    from sa_gnn_amd import ops
    lstm, gru = dict.fromkeys(ops.LSTM_KEYS), dict.fromkeys(ops.GRU_KEYS)
    assert ops.fusion_cell(lstm) == "lstm" and ops.fusion_cell(gru) == "gru"
    with pytest.raises(ValueError, match="not both"):
        ops.fusion_cell({**lstm, **gru})
    with pytest.raises(KeyError, match="found neither"):
        ops.fusion_cell({"ln_gamma": None})
    with pytest.raises(KeyError, match="missing"):
        ops.fusion_cell({"gru_Wg": None, "gru_bg": None})


def test_supported_table():
    lib = _lib.load()
    for d, want in {32: 1, 64: 1, 128: 0, 48: 0, 0: 0, 96: 0, 256: 0}.items():
        assert lib.sagnn_gru_fused_supported(d) == want, d
    assert lib.sagnn_gru_workspace_bytes(1000, 6, 64) == 0 and lib.sagnn_gru_workspace_bytes(1000, 6, 32) == 0
    assert lib.sagnn_gru_workspace_bytes(1000, 6, 128) == 1000 * 3 * 128 * 4
    assert lib.sagnn_gru_workspace_bytes(0, 6, 128) == 0


# ---- argument checks: name -> (call builder, required pointers, pointers that must be 16-byte aligned) ---------------
def _fwd(lib, p, **o):
    a = dict(x=p, ld_n=3 * 64, ld_t=64, n=4, t=3, d=64, Wg=p, bg=p, Wc=p, bc=p, drop=None, h=p, ld_h=3 * 64, gates=None,
             cand=None, ws=None, ws_bytes=0)
    a.update(o)
    return lib.sagnn_gru_fwd_f32(*a.values(), None)


def _cand(lib, p, **o):
    a = dict(gates=p, cand=p, h=p, dh=p, ld_dhe=3 * 64, drop=None, dh_rec=None, ld_dhr=0, da_c=p, du=p, dh_u=p, n=4, t=3, d=64, ts=1)
    a.update(o)
    return lib.sagnn_gru_bwd_cand_f32(*a.values(), None)


def _gates(lib, p, **o):
    a = dict(gates=p, h=p, du=p, dh_u=p, d_rh=p, ld_drh=64, da_g=p, rh=None, n=4, t=3, d=64, ts=1)
    a.update(o)
    return lib.sagnn_gru_bwd_gates_f32(*a.values(), None)


ENTRIES = {
    "fwd": (_fwd, ("x", "Wg", "bg", "Wc", "bc", "h"), ("x", "Wg", "Wc", "h")),
    "bwd_cand": (_cand, ("gates", "cand", "h", "dh", "da_c", "du", "dh_u"), ()),
    "bwd_gates": (_gates, ("gates", "h", "du", "dh_u", "d_rh", "da_g"), ()),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_entry_rejects_invalid_arguments_without_a_device(name):
    fn, ptrs, aligned = ENTRIES[name]
    lib = _lib.load()
    b = (ctypes.c_float * 4096)()
    p = ctypes.addressof(b)
    p += (-p) % 16
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(n=-1), -5, "negative count"), (dict(t=0), -2, "t = 0")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in aligned]
    if name == "fwd":
        cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 16, 48, 288)]
        cases += [(dict(t=65), -2, "t = 65"), (dict(gates=p), -1, "both gates and cand"), (dict(cand=p), -1, "both gates and cand"),
                  (dict(gates=p, cand=p, drop=p), -5, "drop_scale must be null"), (dict(drop=p + 4), -3, "16-byte aligned"),
                  (dict(gates=p + 4, cand=p), -3, "16-byte aligned"), (dict(ld_n=194), -3, "16-byte aligned"),
                  (dict(ld_t=66), -3, "16-byte aligned"), (dict(ld_h=194), -3, "16-byte aligned"),
                  (dict(ld_t=28), -5, "smaller than d = 64"), (dict(ld_n=28), -5, "smaller than d = 64"),
                  (dict(ld_h=128), -5, "ld_h smaller than t*d"),
                  (dict(d=128, ld_n=384, ld_t=128, ld_h=384), -6, "workspace needs 6144 bytes"),
                  (dict(d=128, ld_n=384, ld_t=128, ld_h=384, ws=p, ws_bytes=6000), -6, "workspace needs 6144 bytes"),
                  (dict(d=128, ld_n=384, ld_t=128, ld_h=384, ws=p + 4, ws_bytes=6144), -3, "workspace must be 16-byte aligned")]
    else:
        cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 260)] + [(dict(ts=3), -2, "ts = 3"), (dict(ts=-1), -2, "ts = -1")]
        cases += [(dict(ld_dhe=128), -5, "smaller than t*d"), (dict(dh_rec=p, ld_dhr=32), -5, "smaller than d")] \
            if name == "bwd_cand" else [(dict(ld_drh=32), -5, "smaller than d")]
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, (name, over, _lib.last_error())
        assert text in _lib.last_error().lower(), (name, over, _lib.last_error())
    assert fn(lib, p, n=0) == 0                                       # nothing to do: returns before any launch
