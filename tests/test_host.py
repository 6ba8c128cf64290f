"""CPU suite, part 2: the C-ABI library loads and exports every symbol include/sagnn.h declares,
the host-side logic behind it (plan chunking, CSR validation, argument errors) and the Python
host mirror (Params, DataHandler contract, synthetic writer). No GPU compute is called."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
from sa_gnn_amd import _lib
from sa_gnn_amd.ops import SpmmPlan


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "sagnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sagnn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    names = _header_symbols()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in sagnn.h but not exported by libsagnn.so"
    assert sorted(_lib.SIGNATURES) == names, "ctypes SIGNATURES table out of sync with sagnn.h"
    assert lib.sagnn_version() == 10500


def test_csr_check_errors():
    lib = _lib.load()
    rp = np.array([0, 2, 2, 3], np.int32)
    ci = np.array([1, 0, 2], np.int32)
    assert lib.sagnn_csr_check_host(rp.ctypes.data, ci.ctypes.data, 3, 3, 3) == 0
    bad = np.array([1, 0, 3], np.int32)
    assert lib.sagnn_csr_check_host(rp.ctypes.data, bad.ctypes.data, 3, 3, 3) == -4
    assert "colidx" in _lib.last_error()
    dec = np.array([0, 2, 1, 3], np.int32)
    assert lib.sagnn_csr_check_host(dec.ctypes.data, ci.ctypes.data, 3, 3, 3) == -4
    assert lib.sagnn_csr_check_host(rp.ctypes.data, ci.ctypes.data, 3, 3, 4) == -4
    assert lib.sagnn_csr_check_host(None, ci.ctypes.data, 3, 3, 3) == -1
    with pytest.raises(_lib.SagnnError):
        SpmmPlan(rp, bad, 3, 3)


def test_plan_chunking_host_only():
    """Long rows are cut into equal chunks (multiples of 64, <= chunk_edges), consecutive and in
    edge order; short/medium rows need no metadata."""
    rng = np.random.default_rng(0)
    deg = rng.integers(0, 40, size=500)
    deg[7] = 5000
    deg[123] = 2049
    deg[499] = 130000
    deg[300] = 2048          # == long_thresh: stays a medium row
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = np.zeros(rowptr[-1], np.int32)
    dflt = SpmmPlan(rowptr, colidx, 500, 1).info
    assert (dflt.short_thresh, dflt.long_thresh, dflt.chunk_edges) == (16, 256, 256)
    plan = SpmmPlan(rowptr, colidx, 500, 1, tuning=(16, 2048, 1024))
    info = plan.info
    assert (info.short_thresh, info.long_thresh, info.chunk_edges) == (16, 2048, 1024)
    assert info.on_device == 0 and info.max_degree == 130000
    assert info.n_long_rows == 3
    rows, e0, e1 = plan.chunks()
    assert len(rows) == info.n_chunks
    for r in (7, 123, 499):
        sel = rows == r
        b, e = e0[sel], e1[sel]
        assert b[0] == rowptr[r] and e[-1] == rowptr[r + 1]
        np.testing.assert_array_equal(b[1:], e[:-1])
        lens = e - b
        assert lens.max() <= 1024 and np.all(lens[:-1] % 64 == 0) and np.all(lens[:-1] == lens[0])
        assert len(b) == -(-deg[r] // 1024)
    assert 300 not in rows
    assert plan.workspace_bytes(64) == info.n_chunks * 64 * 4
    # custom tuning: everything above 8 edges is "long", 64-edge chunks
    plan2 = SpmmPlan(rowptr, colidx, 500, 1, tuning=(4, 8, 64))
    assert plan2.info.n_long_rows == int((deg > 8).sum())
    r2, b2, e2 = plan2.chunks()
    assert np.all(e2 - b2 <= 64)
    # spmm on a host-only plan is refused, not silently skipped
    lib = _lib.load()
    rc = lib.sagnn_spmm_f32(plan.handle, None, 0, 64, None, 0, 0.5, None, 0, None, 0, None, 0, None, 0, None)
    assert rc == -5 and "host-only" in _lib.last_error()


def test_plan_rejects_bad_rowptr():
    with pytest.raises(_lib.SagnnError):
        SpmmPlan(np.array([0, 3, 2], np.int32), np.zeros(2, np.int32), 2, 4, validate=False)
    with pytest.raises(ValueError):
        SpmmPlan(np.array([0, 1], np.int32), np.zeros(1, np.int32), 2, 4)
    with pytest.raises(TypeError):
        SpmmPlan(np.array([0, 1, 1], np.int64), np.zeros(1, np.int32), 2, 4)


def test_fusion_argument_errors_without_gpu():
    lib = _lib.load()
    assert lib.sagnn_lstm_fwd_f32(None, 0, 0, 4, 2, 64, None, None, 1.0, None, None, 0, None) == -1
    assert lib.sagnn_lstm_fwd_f32(None, 0, 0, 4, 2, 62, None, None, 1.0, None, None, 0, None) == -2
    assert lib.sagnn_mhsa_mean_f32(None, 0, 0, 4, 2, 64, 7, None, None, None, None, None, None, None, 0, None) == -2
    assert lib.sagnn_interval_fusion_workspace_bytes(10, 3, 64) == 10 * 3 * 64 * 4
    assert lib.sagnn_interval_fusion_workspace_bytes(10, 3, 128) == 10 * 3 * 128 * 4 + 10 * 3 * 3 * 128 * 4
    assert lib.sagnn_interval_fusion_workspace_bytes(10, 3, 48) == 10 * 3 * 48 * 4
    assert lib.sagnn_layernorm_td_f32(None, 0, 0, 0, 0, 64, None, None, 1e-12, None, 0, None) == -2
    # training entries: dimension and pointer checks come before any device work
    assert lib.sagnn_lstm_bwd_supported(64) == 1 and lib.sagnn_lstm_bwd_supported(128) == 0
    assert lib.sagnn_lstm_bwd_f32(None, 64, 64, None, None, None, None, 128, None, None, None, None, None, 4, 2, 128, None) == -2
    assert lib.sagnn_lstm_bwd_f32(None, 64, 64, None, None, None, None, 128, None, None, None, None, None, 4, 2, 64, None) == -1
    assert lib.sagnn_attn_bwd_front_supported(64, 2, 16) == 1
    assert lib.sagnn_attn_bwd_front_supported(64, 7, 16) == 0 and lib.sagnn_attn_bwd_front_supported(64, 2, 4) == 0
    assert lib.sagnn_attn_bwd_front_f32(None, 0, 0, 4, 7, 64, 16, None, None, 1e-12, 1, None, None, None, None, None, None,
                                        None, 64, None, None, None) == -2
    assert lib.sagnn_attn_bwd_front_f32(None, 0, 0, 4, 2, 64, 16, None, None, 1e-12, 1, None, None, None, None, None, None,
                                        None, 64, None, None, None) == -1
    assert lib.sagnn_ln_mhsa_mean_workspace_bytes(10, 3, 64, 16) == 0          # normalised in registers
    assert lib.sagnn_ln_mhsa_mean_workspace_bytes(10, 3, 128, 16) == 0         # d = 128, 16 heads: the split-bf16 fused kernel
    assert lib.sagnn_ln_mhsa_mean_workspace_bytes(10, 3, 128, 8) == 10 * 3 * 128 * 4 + 10 * 3 * 3 * 128 * 4   # wide path
    assert lib.sagnn_ln_mhsa_mean_f32(None, 0, 0, 4, 2, 64, 16, None, None, 1e-12, None, None, None, None, None, None,
                                      None, 64, None, 0, None) == -1


def test_unaligned_attention_calls_are_refused_before_any_launch():
    """An x off a 16-byte boundary never runs fused (csrc/engine.cpp): sagnn_ln_mhsa_mean_f32 then needs the workspace its
    query, which assumes aligned x, answers 0 for; the wide entry takes aligned rows only. Both say so before a launch.
    (The t*d caps of the Valu and wide launchers come after a successful launch set-up: tests/test_gpu_fusion_routes.py.)"""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.sagnn_ln_mhsa_mean_workspace_bytes(4, 2, 64, 16) == 0
    ln = lambda x, ws, nbytes: lib.sagnn_ln_mhsa_mean_f32(x, 128, 64, 4, 2, 64, 16, p, p, 1e-12, p, p, p, p, p, p, p, 64, ws,   # noqa: E731
                                                          nbytes, None)
    assert ln(p + 4, None, 0) == -6 and "workspace" in _lib.last_error()
    assert ln(p + 4, p, 4 * 2 * 64 * 4 - 4) == -6                                     # one float short of y
    assert lib.sagnn_ln_mhsa_mean_f32(p, 129, 64, 4, 2, 64, 16, p, p, 1e-12, p, p, p, p, p, p, p, 64, None, 0, None) == -6
    wide = lambda x, ld_n: lib.sagnn_mhsa_mean_wide_f32(x, ld_n, 128, 4, 2, 128, 8, p, p, p, p, p, p, p, 128, p, 4096 * 4, None)   # noqa: E731
    assert wide(p + 4, 256) == -3 and wide(p, 257) == -3


def test_fusion_entries_refuse_the_same_calls_with_the_same_codes():
    """The eight fusion entries and the code each malformed call returns, one literal per (call, entry), recorded from the
    library before its launchers took argument structs. Every call is one valid host-memory call (n = 4, t = 2, d = 64,
    16 heads; the wide entry d = 128, 8 heads) with one or two arguments changed; the valid call itself is never made and
    none of these reaches a launch. `_` marks an entry that does not read the argument or does not check it before its
    first launch (the wide entry's and interval_fusion's ld_out; an unaligned x where a VALU kernel takes it). Where two
    faults meet, the code says which check comes first: interval_fusion looks at its workspace before heads and
    pointers, the backward front at the shape before pointers."""
    lib = _lib.load()
    buf = (ctypes.c_float * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    seq, qkv = "x ld_n ld_t n t d", "Wq bq Wk bk Wv bv"
    lstm = f"{seq} W b forget_bias drop"
    entries = {   # in the column order of `cases`
        "sagnn_lstm_fwd_f32": f"{lstm} h ld_h stream",
        "sagnn_lstm_fwd_state_f32": f"{lstm} h_init ld_hi c_init h ld_h c_final stream",
        "sagnn_lstm_fwd_train_f32": f"{lstm} h ld_h gates cell stream",
        "sagnn_mhsa_mean_f32": f"{seq} heads {qkv} out ld_out stream",
        "sagnn_mhsa_mean_wide_f32": f"{seq} heads {qkv} out ld_out ws ws_bytes stream",
        "sagnn_ln_mhsa_mean_f32": f"{seq} heads gamma beta eps {qkv} out ld_out ws ws_bytes stream",
        "sagnn_interval_fusion_f32": f"{seq} heads W b forget_bias gamma beta eps {qkv} out ld_out ws ws_bytes stream",
        "sagnn_attn_bwd_front_f32": f"{seq} heads gamma beta eps apply_ln {qkv} g_out ld_g dqkv y_out stream",
    }
    valid = dict(x=p, ld_n=128, ld_t=64, n=4, t=2, d=64, heads=16, W=p, b=p, forget_bias=1.0, drop=None, h=p, ld_h=128,
                 gates=p, cell=p, h_init=p, ld_hi=64, c_init=p, c_final=p, gamma=p, beta=p, eps=1e-12, apply_ln=1, out=p,
                 ld_out=64, ws=p, ws_bytes=4 * 2 * 64 * 4, g_out=p, ld_g=64, dqkv=p, y_out=p, stream=None,
                 **dict.fromkeys(qkv.split(), p))
    wide = dict(d=128, heads=8, ld_n=256, ld_t=128, ld_out=128, ws_bytes=4 * 2 * 3 * 128 * 4)
    d128 = dict(d=128, ld_n=256, ld_t=128, ld_g=128)
    _ = None
    cases = [
        # changed arguments                     fwd state train mhsa wide  ln fusion front
        (dict(x=None),                          (-1, -1, -1, -1, -1, -1, -1, -1)),
        (dict(W=None),                          (-1, -1, -1,  _,  _,  _, -1,  _)),
        (dict(b=None),                          (-1, -1, -1,  _,  _,  _, -1,  _)),
        (dict(h=None),                          (-1, -1, -1,  _,  _,  _,  _,  _)),
        (dict(gates=None),                      ( _,  _, -1,  _,  _,  _,  _,  _)),
        (dict(cell=None),                       ( _,  _, -1,  _,  _,  _,  _,  _)),
        (dict(h_init=None),                     ( _, -1,  _,  _,  _,  _,  _,  _)),   # c_init without h_init
        (dict(c_init=None),                     ( _, -1,  _,  _,  _,  _,  _,  _)),   # h_init without c_init
        (dict(gamma=None),                      ( _,  _,  _,  _,  _, -1, -1, -1)),
        (dict(beta=None),                       ( _,  _,  _,  _,  _, -1, -1, -1)),
        *[(dict([(w, None)]),                   ( _,  _,  _, -1, -1, -1, -1, -1)) for w in qkv.split()],
        (dict(out=None),                        ( _,  _,  _, -1, -1, -1, -1,  _)),
        (dict(g_out=None),                      ( _,  _,  _,  _,  _,  _,  _, -1)),
        (dict(dqkv=None),                       ( _,  _,  _,  _,  _,  _,  _, -1)),
        (dict(ws=None),                         ( _,  _,  _,  _, -6,  _, -6,  _)),
        (dict(d=62),                            (-2, -2, -2, -2, -2, -2, -2, -2)),
        (dict(d=100, heads=4),                  ( _,  _,  _,  _, -2,  _,  _,  _)),   # a multiple of 4, not of 32
        (dict(t=0),                             (-2, -2, -2, -2, -2, -2, -2, -2)),
        (dict(t=65),                            (-2, -2, -2, -2, -2, -2, -2, -2)),
        (dict(t=7),                             ( _,  _,  _,  _,  _,  _,  _, -2)),   # no backward front for it
        (dict(d128, t=8),                       ( _,  _,  _,  _,  _,  _,  _, -2)),   # d = 128: the front stops at t = 6
        (dict(heads=7),                         ( _,  _,  _, -2, -2, -2, -2, -2)),
        (dict(heads=4),                         ( _,  _,  _,  _,  _,  _,  _, -2)),   # d / heads = 16: no backward front
        (dict(ld_n=60),                         (-5, -5, -5, -5, -5, -5, -5, -5)),
        (dict(ld_t=60),                         (-5, -5, -5, -5, -5, -5, -5, -5)),
        (dict(ld_n=128, ld_t=128),              (-5, -5, -5, -5, -5, -5, -5, -5)),   # neither node- nor time-major
        (dict(ld_out=60),                       ( _,  _,  _, -5,  _, -5,  _,  _)),
        (dict(ld_g=60),                         ( _,  _,  _,  _,  _,  _,  _, -5)),
        (dict(ld_h=124),                        (-5, -5, -5,  _,  _,  _,  _,  _)),
        (dict(ld_hi=60),                        ( _, -5,  _,  _,  _,  _,  _,  _)),
        (dict(x=p + 4),                         ( _,  _,  _,  _, -3,  _,  _, -3)),
        (dict(ld_n=257),                        ( _,  _,  _,  _, -3,  _,  _,  _)),
        (dict(ld_n=129),                        ( _,  _,  _,  _,  _,  _,  _, -3)),
        (dict(g_out=p + 4),                     ( _,  _,  _,  _,  _,  _,  _, -3)),
        (dict(ld_g=66),                         ( _,  _,  _,  _,  _,  _,  _, -3)),
        (dict(dqkv=p + 4),                      ( _,  _,  _,  _,  _,  _,  _, -3)),
        (dict(y_out=p + 4),                     ( _,  _,  _,  _,  _,  _,  _, -3)),
        (dict(ws_bytes=4 * 2 * 3 * 128 * 4 - 4), ( _,  _,  _,  _, -6,  _,  _,  _)),   # one float short
        (dict(ws_bytes=4 * 2 * 64 * 4 - 4),     ( _,  _,  _,  _,  _,  _, -6,  _)),
        (dict(x=p + 4, ws_bytes=4 * 2 * 64 * 4 - 4), ( _,  _,  _,  _,  _, -6,  _,  _)),   # unaligned: y needs room
        (dict(x=p + 4, ws=None),                ( _,  _,  _,  _,  _, -6,  _,  _)),
        (dict(n=0),                             ( 0,  0,  0,  0,  0,  0,  0,  0)),
        (dict(n=0, ws=None),                    ( _,  _,  _,  _,  0,  0,  0,  _)),
        (dict(n=0, x=None),                     (-1, -1, -1, -1, -1, -1,  0, -1)),
        (dict(n=-1),                            (-5, -5, -5, -5, -5, -5, -5, -5)),
        # two faults in one call
        (dict(d=62, x=None),                    (-2, -2, -2, -2, -2, -2, -2, -2)),
        (dict(t=65, x=None),                    (-2, -2, -2, -2, -2, -2, -2, -2)),
        (dict(heads=7, Wq=None),                ( _,  _,  _, -2, -2, -2, -2, -2)),
        (dict(ws_bytes=4 * 2 * 3 * 128 * 4 - 4, out=None), ( _,  _,  _,  _, -1,  _,  _,  _)),
        (dict(ws_bytes=4 * 2 * 64 * 4 - 4, out=None), ( _,  _,  _,  _,  _,  _, -6,  _)),
        (dict(ws_bytes=4 * 2 * 64 * 4 - 4, heads=7), ( _,  _,  _,  _,  _,  _, -6,  _)),
        (dict(x=p + 4, ws_bytes=4 * 2 * 64 * 4 - 4, out=None), ( _,  _,  _,  _,  _, -1,  _,  _)),
        (dict(t=7, x=None),                     (-1, -1, -1, -1, -1, -1, -6, -2)),   # fusion: t = 7 outgrows the workspace
        (dict(t=12, x=None),                    ( _,  _,  _,  _,  _,  _,  _, -1)),   # a supported shape: on to the pointers
        (dict(d128, t=6, x=None),               ( _,  _,  _,  _,  _,  _,  _, -1)),
        (dict(d128, t=8, x=None),               ( _,  _,  _,  _,  _,  _,  _, -2)),
        (dict(ld_n=60, ld_out=60),              ( _,  _,  _, -5,  _, -5,  _,  _)),
        (dict(ld_n=60, x=p + 4),                ( _,  _,  _,  _, -5,  _,  _, -5)),   # strides before alignment
    ]
    assert lib.sagnn_get_engine() == 0
    got = []
    for changed, codes in cases:
        for (name, params), want in zip(entries.items(), codes):
            if want is None:
                continue
            params = params.split()
            assert set(changed) & set(params), (name, changed)     # never the valid call
            args = {**valid, **(wide if "wide" in name else {}), **changed}
            rc = getattr(lib, name)(*[args[k] for k in params])
            got.append((name, changed, rc, want))
    assert [g for g in got if g[2] != g[3]] == []
    # under the fp32 engine the backward front has no t = 12 kernel, and says so before it looks at x
    assert lib.sagnn_set_engine(1) == 0
    try:
        front = lambda t: lib.sagnn_attn_bwd_front_f32(None, 128, 64, 4, t, 64, 16, p, p, 1e-12, 1, p, p, p, p, p, p, p, 64, p, p, None)   # noqa: E731
        assert (front(8), front(12)) == (-1, -2)
    finally:
        lib.sagnn_set_engine(0)


def test_round3_entries_reject_bad_arguments_without_gpu():
    """The entries added in round 3 validate before they touch a device: segmented weight gradient, BPTT with scratch."""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    # dense_tn_seg: din / dout multiples of 32, 16-byte rows, segment strides multiples of 4 floats, dW given
    assert lib.sagnn_dense_tn_seg_f32(p, 64, 4096, p, 128, 4096, 10, 3, 48, 128, p, None, None) == -2
    assert lib.sagnn_dense_tn_seg_f32(p, 64, 4098, p, 128, 4096, 10, 3, 64, 128, p, None, None) == -3
    assert lib.sagnn_dense_tn_seg_f32(p, 62, 4096, p, 128, 4096, 10, 3, 64, 128, p, None, None) == -3
    assert lib.sagnn_dense_tn_seg_f32(p, 64, 4096, p, 128, 4096, 10, 3, 64, 128, None, None, None) == -1
    assert lib.sagnn_dense_tn_seg_f32(p, 64, 4096, p, 128, 4096, 0, 3, 64, 128, p, None, None) == 0      # nothing to add
    # lstm_bwd_ws: the scratch size is the gate gradients', a short one is an error (not a silent one-launch fallback)
    assert lib.sagnn_lstm_bwd_workspace_bytes(1000, 5, 64) == 1000 * 5 * 256 * 4
    assert lib.sagnn_lstm_bwd_workspace_bytes(0, 5, 64) == 0
    args = (p, 320, 64, p, p, p, p, 320, None, p, p, p, p, 10, 5)
    assert lib.sagnn_lstm_bwd_ws_f32(*args, 64, p, 16, None) == -6
    assert lib.sagnn_lstm_bwd_ws_f32(*args, 48, p, 1 << 20, None) == -2
    assert lib.sagnn_lstm_bwd_ws_f32(p, 320, 64, None, p, p, p, 320, None, p, p, p, p, 10, 5, 64, p, 1 << 20, None) == -1
    msg = ctypes.create_string_buffer(256)
    lib.sagnn_last_error(msg, 256)
    assert b"null" in msg.value.lower()


def _gnn_args(user, item, d, L, leaky=0.5, **over):
    """A sagnn_gnn_args of plain edges; user / item: (in, ld_in, slab_in, out, ld_out, slab_out, scratch, mask)."""
    a = _lib.GnnArgs(d=d, n_layers=L, leaky=leaky, **over)
    for side, values in ((a.user, user), (a.item, item)):
        for (name, _), v in zip(_lib.GnnSide._fields_, values):
            setattr(side, name, v)
    return a


def test_gnn_stack_entries_reject_malformed_calls_without_gpu():
    """The four entries of the GNN stack (one interval / a batch, forward / backward) and the code each malformed call
    returns; every one of them returns before a launch. Plans built with device=None are host-only: a well-formed
    forward on them is refused as such (-5), and that refusal comes before the forward's look at d. A batch cannot be
    built without a device, so here the batched entries only see a NULL one (tests/test_gpu_spmm.py has their table)."""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    mbuf = (ctypes.c_uint8 * 4096)()
    m = ctypes.addressof(mbuf)

    def host_plan(rows, cols):
        return SpmmPlan(np.arange(rows + 1, dtype=np.int32), np.zeros(rows, np.int32), rows, cols)

    pu, pi, other = host_plan(3, 4), host_plan(4, 3), host_plan(5, 3)
    U, I = pu.handle, pi.handle

    def fwd(plan_user=U, plan_item=I, u0=p, d=64, L=1, scratch=None, mask_u=None, mask_i=None, **over):
        a = _gnn_args((u0, 64, 0, p, 64, 0, scratch, mask_u), (p, 64, 0, p, 64, 0, scratch, mask_i), d, L, **over)
        return lib.sagnn_gnn_interval_f32(plan_user, plan_item, ctypes.byref(a), None)

    def bwd(plan_user=U, plan_item=I, G_u=p, d=64, L=1, scratch=p, mask_u=m, mask_i=m):
        a = _gnn_args((G_u, 64, 0, p, 64, 0, scratch, mask_u), (p, 64, 0, p, 64, 0, scratch, mask_i), d, L)
        return lib.sagnn_gnn_interval_bwd_f32(plan_user, plan_item, ctypes.byref(a), None)

    thin = ctypes.byref(_gnn_args((p, 64, 0, p, 64, 0, None, None), (p, 64, 0, p, 64, 0, None, None), 64, 1))
    full = ctypes.byref(_gnn_args((p, 64, 0, p, 64, 0, p, m), (p, 64, 0, p, 64, 0, p, m), 64, 1))
    drop, time = _lib.EdgeDropArgs(1, 1, 1 << 31, 2.0), _lib.EdgeTimeArgs()

    table = [
        ("forward, NULL plan", fwd(plan_user=None), -1),
        ("forward, NULL embedding", fwd(u0=None), -1),
        ("forward, n_layers = 0", fwd(L=0), -5),
        ("forward, d = 62 (host-only plan refused first)", fwd(d=62), -5),
        ("forward, one mask without the other", fwd(mask_u=m), -1),
        ("forward, two layers without scratch", fwd(L=2), -1),
        ("forward, not a transposed pair", fwd(plan_item=other.handle), -5),
        ("forward, well-formed on host-only plans", fwd(L=2, scratch=p, mask_u=m, mask_i=m), -5),
        ("backward, NULL plan", bwd(plan_item=None), -1),
        ("backward, NULL gradient", bwd(G_u=None), -1),
        ("backward, n_layers = 0", bwd(L=0), -5),
        ("backward, d = 62", bwd(d=62), -2),
        ("backward, one mask without the other", bwd(mask_i=None), -1),
        ("backward, no scratch", bwd(scratch=None), -1),
        ("backward, not a transposed pair", bwd(plan_item=other.handle), -5),
        ("batched forward, NULL batch",
         lib.sagnn_gnn_stack_f32(None, thin, None), -1),
        ("batched backward, NULL batch", lib.sagnn_gnn_stack_bwd_f32(None, full, None), -1),
        # the struct itself: refused before the plans are looked at, like everything above before any launch
        ("NULL args", lib.sagnn_gnn_interval_f32(U, I, None, None), -1),
        ("NULL args, backward", lib.sagnn_gnn_interval_bwd_f32(U, I, None, None), -1),
        ("NULL args, batched", lib.sagnn_gnn_stack_f32(None, None, None), -1),
        ("NULL args, batched backward", lib.sagnn_gnn_stack_bwd_f32(None, None, None), -1),
        ("edges outside the three forms", fwd(edges=3), -5),
        ("edges negative", fwd(edges=-1), -5),
        ("plain edges with a drop struct", fwd(drop=ctypes.pointer(drop)), -5),
        ("plain edges with a time struct", fwd(time=ctypes.pointer(time)), -5),
    ]
    assert [(name, rc) for name, rc, _ in table] == [(name, want) for name, _, want in table]
    # the thin forward without masks goes the same way
    assert fwd(L=0) == -5 and "n_layers = 0" in _lib.last_error()


def test_gnn_args_layout_matches_the_header():
    """GnnArgs / GnnSide mirror sagnn_gnn_args / sagnn_gnn_side field for field (names and order from the header's text),
    and the library reads the fields where ctypes puts them: values from both ends of the struct come back in refusal
    messages, on host-only plans."""
    text = open(os.path.join(ROOT, "include", "sagnn.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]

    assert fields("sagnn_gnn_side") == [n.rstrip("_") for n, _ in _lib.GnnSide._fields_]
    assert fields("sagnn_gnn_args") == [n for n, _ in _lib.GnnArgs._fields_]
    # LP64: 3 pointers + 4 int64 + 2 pointers a side; then 4 x 4 bytes, 2 pointers, int + padding, pointer, size_t
    assert ctypes.sizeof(_lib.GnnSide) == 64 and ctypes.sizeof(_lib.GnnArgs) == 2 * 64 + 16 + 16 + 8 + 16
    assert (_lib.EDGES_PLAIN, _lib.EDGES_DROP, _lib.EDGES_TIME) == tuple(
        int(re.search(r"SAGNN_EDGES_%s = (\d+)" % n, text).group(1)) for n in ("PLAIN", "DROP", "TIME"))

    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    pu = SpmmPlan(np.arange(4, dtype=np.int32), np.zeros(3, np.int32), 3, 4)
    pi = SpmmPlan(np.arange(5, dtype=np.int32), np.zeros(4, np.int32), 4, 3)
    drop = ctypes.pointer(_lib.EdgeDropArgs(1, 1, 1 << 31, 2.0))
    side = (p, 64, 0, p, 64, 0, p, p)
    for entry in (lib.sagnn_gnn_interval_f32, lib.sagnn_gnn_interval_bwd_f32):
        call = lambda a: entry(pu.handle, pi.handle, ctypes.byref(a), None)   # noqa: E731
        assert call(_gnn_args(side, side, 64, 128, edges=_lib.EDGES_DROP, drop=drop)) == -5
        assert "n_layers = 128" in _lib.last_error()
        assert call(_gnn_args(side, side, 64, 2, edges=_lib.EDGES_DROP, drop=drop, interval=(1 << 23) + 5)) == -5
        assert "interval %d" % ((1 << 23) + 5) in _lib.last_error()
    # the item side's ld_in. The forward refuses a host-only plan before it looks at i0 (tests/test_gpu_spmm.py has that
    # row on device plans); the backward reads the same field as G_i and reaches it here.
    a = _gnn_args(side, (p, 60, 0, p, 64, 0, p, p), 64, 2)
    assert lib.sagnn_gnn_interval_bwd_f32(pu.handle, pi.handle, ctypes.byref(a), None) == -5
    assert "G_i: ld 60 < d 64" in _lib.last_error()


def test_softmax_args_layout_matches_the_header():
    """SoftmaxArgs mirrors sagnn_softmax_args field for field (names and order from the header's text), and the library
    reads the fields where ctypes puts them: a value from the first field and one from the last come back in refusals."""
    import softmax_args_host as H
    text = open(os.path.join(ROOT, "include", "sagnn.h")).read()
    body = re.search(r"typedef struct sagnn_softmax_args \{(.*?)\} sagnn_softmax_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in _lib.SoftmaxArgs._fields_] and names[0] == "Q" and names[-1] == "workspace_bytes"
    # LP64, every member 8 bytes but d and mode (4 + 4 padding each) and the two floats (one 8-byte slot together):
    # Q ldq I ldi n_queries n_items = 48; d = 8; target = 8; inv_temp scale = 8; excl_ptr excl_items excl_row n_lists = 32;
    # mode = 8; cand n_cand bias = 24; loss lse tscore = 24; g dQ lddq dI lddi dT lddt = 56; workspace workspace_bytes = 16
    assert ctypes.sizeof(_lib.SoftmaxArgs) == 48 + 8 + 8 + 8 + 32 + 8 + 24 + 24 + 56 + 16 == 232
    assert (_lib.SOFTMAX_FULL, _lib.SOFTMAX_CAND, _lib.SOFTMAX_CAND_BIAS) == tuple(
        int(re.search(r"SAGNN_SOFTMAX_%s = (\d+)" % n, text).group(1)) for n in ("FULL", "CAND", "CAND_BIAS"))

    lib = _lib.load()
    buf, p = H.aligned_buffer()
    for backward in (False, True):
        for mode in (_lib.SOFTMAX_FULL, _lib.SOFTMAX_CAND, _lib.SOFTMAX_CAND_BIAS):
            assert H.call(lib, backward, H.softmax_args(p, mode, Q=p + 4)) == -3
            assert "Q and I must be 16-byte aligned" in _lib.last_error()
            assert H.call(lib, backward, H.softmax_args(p, mode, workspace_bytes=48)) == -6      # 512 are needed at least
            assert "workspace of 48 bytes" in _lib.last_error()
    del buf


def test_params_match_reference_flags():
    from sa_gnn_amd import Params
    a = Params.parse_args([])
    # names/defaults of reference Params.py:5-50 used by the path
    assert (a.graphNum, a.gnn_layer, a.latdim, a.leaky, a.keepRate, a.num_attention_heads) == (8, 2, 64, 0.5, 0.5, 16)
    assert (a.batch, a.trnNum, a.decay_step, a.data, a.pos_length, a.att_layer) == (512, 10000, 19, "yelp", 200, 4)
    # the reference's shell lines parse unchanged (gowalla.sh / amazon.sh)
    g = Params.parse_args("--data gowalla --lr 2e-3 --reg 1e-2 --temp 0.1 --ssl_reg 1e-6 --save_path gowalla "
                          "--epoch 150 --batch 512 --sslNum 40 --graphNum 3 --gnn_layer 2 --att_layer 1 "
                          "--test True --testSize 1000 --ssldim 48".split())
    assert (g.graphNum, g.gnn_layer, g.data, g.test, g.ssldim) == (3, 2, "gowalla", True, 48)
    assert Params.parse_args(["--test", "False"]).test is True     # type=bool quirk (Params.py:47-49)


def test_synthetic_writer_and_datahandler_contract(tmp_path):
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    tmt = synthetic.make_trn_mat_time(300, 200, [1500, 1200, 0], seed0=1000)
    assert len(tmt) == 3 and len(tmt[1]) == 3
    for s in tmt[1]:
        assert sp.isspmatrix_csr(s) and s.dtype == np.intc and s.shape == (300, 200)
    assert tmt[1][0].data.min() > 1_000_000_000          # values are Unix timestamps
    assert tmt[1][2].nnz == 0
    seq = synthetic.make_sequence(tmt)
    assert len(seq) == 300 and sum(len(s) for s in seq) == sum(s.nnz for s in tmt[1])
    h = DataHandler.from_memory(tmt, seq)
    assert (args.user, args.item) == (300, 200) and h.maxTime == 1
    assert h.trnMat.shape == (300, 200) and len(h.subMat) == 3
    # same objects through the reference's pickle files
    import pickle
    d = tmp_path / "synth"
    d.mkdir()
    for name, obj in (("trn_mat_time", tmt), ("sequence", seq), ("tst_int", [None] * 299 + [5])):
        with open(d / name, "wb") as f:
            pickle.dump(obj, f)
    args.data = "synth"
    h2 = DataHandler(root=str(tmp_path))
    h2.LoadData()
    assert list(h2.tstUsrs) == [299] and (h2.subMat[0] != tmt[1][0]).nnz == 0
    args.data = "yelp"


def test_powerlaw_generator_properties():
    from sa_gnn_amd import synthetic
    u, i = synthetic.powerlaw_edges(20000, 10000, 200000, seed=1000)
    key = u * 10000 + i
    assert u.numel() <= 200000 and u.numel() > 150000
    assert torch.all(key[1:] > key[:-1])                 # sorted by (user, item), unique
    (rp_u, ci_u), (rp_i, ci_i) = synthetic.csr_pair_from_edges(u, i, 20000, 10000)
    assert rp_u[-1] == u.numel() == rp_i[-1]
    a = sp.csr_matrix((np.ones(u.numel()), ci_u.numpy(), rp_u.numpy()), shape=(20000, 10000))
    b = sp.csr_matrix((np.ones(u.numel()), ci_i.numpy(), rp_i.numpy()), shape=(10000, 20000))
    assert (a - b.T).nnz == 0
    du, di = np.diff(rp_u.numpy()), np.diff(rp_i.numpy())
    assert du.max() > 20 * du.mean() / 4 and di.max() > 30 * di.mean()      # heavy tails
    u2, i2 = synthetic.powerlaw_edges(20000, 10000, 200000, seed=1000)
    assert torch.equal(u, u2) and torch.equal(i, i2)     # deterministic in the seed


def test_write_dataset_roundtrip(tmp_path):
    """The on-disk writer emits what DataHandler.LoadData (the reference's loader contract) reads."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    tmt, seq, tst, tdict = synthetic.write_dataset(str(tmp_path / "toy"), 120, 90, [500, 400], test_size=20)
    args.data = "toy"
    h = DataHandler(root=str(tmp_path))
    h.LoadData()
    args.data = "yelp"
    assert (args.user, args.item) == (120, 90) and len(h.subMat) == 2
    assert len(h.tstUsrs) == 60 and h.tstInt[0] == tst[0] and h.tstInt[1] is None
    assert h.test_dict[1] == tdict[1] and min(min(v) for v in h.test_dict.values()) >= 1
    assert h.sequence == seq


def test_sampler_invariants():
    """Vectorised samplers keep the reference's contracts (model.py:252-339): mirrored halves,
    negatives never interacted with nor the last / test item, SSL pairs interleaved and drawn
    from the user's items of that interval."""
    from sa_gnn_amd import synthetic
    from sa_gnn_amd.DataHandler import DataHandler
    from sa_gnn_amd.Params import args
    from sa_gnn_amd.model import Recommender
    args.graphNum, args.batch, args.pos_length, args.sslNum, args.pred_num = 3, 64, 20, 5, 2
    U, I = 300, 200
    tmt = synthetic.make_trn_mat_time(U, I, [3000, 2500, 2000])
    seq = synthetic.make_sequence(tmt)
    tst = [(u * 7) % I if u % 2 else None for u in range(U)]
    h = DataHandler.from_memory(tmt, seq, tst, None)
    rec = Recommender.__new__(Recommender)
    rec.handler = h
    np.random.seed(0)
    bat = np.random.permutation(U)[:64]
    uL, iL, sq, mk, uLs = rec.sampleTrainBatch(bat, h.trnMat, None, 7)
    n = len(uL) // 2
    assert n > 0 and uL[:n] == uL[n:] and uLs[:n] == uLs[n:] and sq.shape == (64, 20)
    for e in range(n):
        u = uL[e]
        assert iL[e] in seq[u][:-1]                                   # positive: an earlier item of the user
        assert h.trnMat[u, iL[n + e]] == 0 and iL[n + e] != seq[u][-1] and iL[n + e] != tst[u]
        assert bat[uLs[e]] == u
    assert set(np.unique(mk)) <= {0.0, 1.0} and np.all((sq != 0) <= (mk != 0) + (sq == 0))
    su, si, sl = rec.sampleSslBatch(bat, h.subMat)
    for k in range(3):
        assert len(su[k]) % 2 == 0 and su[k][0::2] == su[k][1::2]
        for e in range(len(su[k])):
            assert h.subMat[k][su[k][e], si[k][e]] != 0


def test_calc_res_counts_match_the_reference_loop_on_ties_and_duplicates():
    """Recommender.calcRes ranks without sorting (rank = #(pred > p) + #(earlier candidates with pred == p) of the
    best-ranked copy of the target item). Against the oracle's restatement of the reference's sort + list.index loop
    (model.py:484-510) on heavily tied scores and candidate lists that repeat item ids (a pre-drawn negative may
    be the held-out item itself; equal items have equal scores)."""
    from oracle import selfgnn_oracle as O
    from sa_gnn_amd.model import Recommender
    rng = np.random.default_rng(0)
    for _ in range(100):
        B, C = 13, 29
        locs = [rng.integers(0, 12, size=C) for _ in range(B)]
        tem = [int(l[-1]) for l in locs]                                  # the positive is the last candidate
        preds = np.round(rng.standard_normal((B, C)), 1).astype(np.float32)
        for b in range(B):
            for c in range(C):
                preds[b, c] = preds[b, np.argmax(locs[b] == locs[b][c])]
        np.testing.assert_allclose(Recommender.calcRes(preds, tem, locs, shoot=10), O.calc_res(preds, tem, locs, shoot=10))


def test_calc_res_counts_a_nan_score_as_a_miss():
    """A diverged model scores NaN. The reference's sort leaves a NaN positive where it is — last — so it misses;
    the sort-free count must not turn `NaN > x == False` into rank 0 (HR = 1). +-inf keep their meaning."""
    from oracle import selfgnn_oracle as O
    from sa_gnn_amd.model import Recommender
    rng = np.random.default_rng(1)
    B, C = 5, 100
    locs = [list(rng.permutation(1000)[:C]) for _ in range(B)]
    tem = [l[-1] for l in locs]
    preds = rng.standard_normal((B, C))
    preds[0, :] = np.nan             # everything NaN
    preds[1, -1] = np.nan            # only the positive
    preds[2, :50] = np.nan           # half of the negatives: the positive competes with the finite half only
    preds[2, -1] = 10.0
    preds[3, -1] = np.inf
    preds[4, -1] = -np.inf
    got = [Recommender.calcRes(preds[j:j + 1], tem[j:j + 1], locs[j:j + 1], shoot=10) for j in range(B)]
    assert got[0] == (0.0,) * 6 and got[1] == (0.0,) * 6 and got[4] == (0.0,) * 6
    assert got[3] == (1.0,) * 6
    for j in (0, 1, 3, 4):           # where Python's sort is well defined with a NaN in the list
        assert got[j] == O.calc_res(preds[j:j + 1], tem[j:j + 1], locs[j:j + 1], shoot=10)
    assert got[2][0] == 1.0


def test_engine_is_chosen_per_thread_through_the_abi():
    """sagnn_set_engine / sagnn_get_engine: no environment switch, no process-wide state."""
    import threading
    lib = _lib.load()
    assert lib.sagnn_get_engine() == 0
    assert lib.sagnn_set_engine(1) == 0 and lib.sagnn_get_engine() == 1
    seen = []
    th = threading.Thread(target=lambda: seen.append(lib.sagnn_get_engine()))
    th.start(); th.join()
    assert seen == [0]                                   # another thread still runs the default
    assert lib.sagnn_set_engine(7) < 0 and lib.sagnn_get_engine() == 1
    assert lib.sagnn_set_engine(0) == 0


SELECTION_GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_selection.npz")


def engine_selection_sweep(lib):
    """Every kernel-selection answer the ABI gives without a device, over engine (f16x2, f32, valu) x d in {4, 8, .., 256}
    x t in 1..32 x heads in {1, 2, 4, .., 32}; byte counts at n = 2. tests/golden/engine_selection.npz holds this sweep of
    the build before the selection moved into csrc/engine.cpp: np.savez_compressed(SELECTION_GOLDEN, **sweep)."""
    ds, ts, hs = range(4, 257, 4), range(1, 33), (1, 2, 4, 8, 16, 32)
    shape = (3, len(ds), len(ts), len(hs))
    out = {"attn_bwd_front_supported": np.zeros(shape, np.int32), "ln_mhsa_mean_workspace_bytes": np.zeros(shape, np.int32),
           "interval_fusion_workspace_bytes": np.zeros(shape[:3], np.int32),
           "attn_bwd_tail_supported": np.zeros(shape[:2], np.int32), "lstm_bwd_supported": np.zeros(shape[:2], np.int32)}
    prev = lib.sagnn_get_engine()
    try:
        for e in range(3):
            assert lib.sagnn_set_engine(e) == 0
            for i, d in enumerate(ds):
                out["attn_bwd_tail_supported"][e, i] = lib.sagnn_attn_bwd_tail_supported(d)
                out["lstm_bwd_supported"][e, i] = lib.sagnn_lstm_bwd_supported(d)
                for j, t in enumerate(ts):
                    out["interval_fusion_workspace_bytes"][e, i, j] = lib.sagnn_interval_fusion_workspace_bytes(2, t, d)
                    for k, h in enumerate(hs):
                        out["attn_bwd_front_supported"][e, i, j, k] = lib.sagnn_attn_bwd_front_supported(d, t, h)
                        out["ln_mhsa_mean_workspace_bytes"][e, i, j, k] = lib.sagnn_ln_mhsa_mean_workspace_bytes(2, t, d, h)
    finally:
        lib.sagnn_set_engine(prev)
    return out


def test_engine_selection_answers_match_the_golden_sweep():
    """The _supported and workspace queries answer from csrc/engine.cpp's selectors: a moved boundary changes a point."""
    got = engine_selection_sweep(_lib.load())
    want = np.load(SELECTION_GOLDEN)
    assert sorted(want.files) == sorted(got)
    axes = ("engine", "d", "t", "heads")
    for name in want.files:
        bad = np.argwhere(want[name] != got[name])
        assert bad.size == 0, f"{name}: {len(bad)} points differ, first at {dict(zip(axes, bad[0].tolist()))} (indices)"


def test_adam_multi_batches_skip_empty_tensors_without_stepping_any_twice():
    """More than 48 tensors (one launch's table) with an empty one among them: host-side argument walk only — the
    launch itself needs a GPU (tests/test_gpu_train.py); here the walk must terminate and reject nothing."""
    import ctypes
    lib = _lib.load()
    assert lib.sagnn_adam_multi_f32(0, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 1, None) == 0



def test_bench_starts_its_own_ranks_when_started_bare(monkeypatch):
    """`python bench.py --gpus N` is how the driver starts every bench (BENCH_rNN.json `cmd`): with N > 1 and no
    WORLD_SIZE in the environment the process must start N ranks under torch.distributed.run as a CHILD (before any
    GPU call), pass its own arguments through and exit with the child's code."""
    import subprocess
    import bench
    cmd = bench.launch_command(8, ["--gpus", "8", "--steps", "3", "--warmup", "1"], 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"]
    seen = {}

    def fake_run(c, env=None, **kw):
        seen["cmd"], seen["env"] = c, env
        return subprocess.CompletedProcess(c, 7)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--dist-backend", "gloo", "--scale", "0.004", "--intervals", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                       # the launcher's exit code is the parent's
    assert seen["cmd"][-8:] == ["--gpus", "2", "--dist-backend", "gloo", "--scale", "0.004", "--intervals", "4"]
    assert "--nproc-per-node=2" in seen["cmd"] and seen["env"]["MASTER_ADDR"] == "127.0.0.1"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # under a launcher (WORLD_SIZE set) a rank count that disagrees with --gpus is still refused
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "agree" in str(e.value.code)


def test_bench_dump_outputs_samples_rows_within_budget(tmp_path, monkeypatch):
    """bench.dump_outputs: float32 files, whole arrays when they fit, else the same seeded, sorted row sample in every
    call; the files stay under the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    g = torch.Generator().manual_seed(0)
    big = torch.randn((3, 20_000, 16), generator=g)                    # 3.8 MB: sampled
    small = torch.randn((1000, 16), generator=g, dtype=torch.float64)  # 64 kB: whole, stored as float32
    info = [bench.dump_outputs(str(tmp_path / s), {"big": big, "small": small}) for s in ("a", "b")]
    assert info[0] == info[1]
    k = (1 << 19) // (3 * 16 * 4)
    assert info[0] == {"big": {"shape": [3, k, 16], "rows_of": 20_000}, "small": {"shape": [1000, 16], "rows_of": 1000}}
    rows = np.sort(np.random.default_rng(0).choice(20_000, k, replace=False))
    for s in ("a", "b"):
        b, m = np.load(tmp_path / s / "big.npy"), np.load(tmp_path / s / "small.npy")
        assert b.dtype == np.float32 and m.dtype == np.float32
        np.testing.assert_array_equal(b, big.numpy()[:, rows, :])
        np.testing.assert_array_equal(m, small.float().numpy())
    assert sum(os.path.getsize(p) for p in (tmp_path / "a").iterdir()) <= (1 << 20) + 2 * 128
