"""CPU suite: argument checks of the full-catalogue retrieval entry (sagnn_score_topk_f32) and of ops.score_topk.
Every call here is rejected before any device work, so no GPU is needed."""
import ctypes

import numpy as np
import pytest
import torch

from sa_gnn_amd import _lib, ops


def _call(lib, buf, **over):
    p = ctypes.addressof(buf)
    a = dict(Q=p, ldq=64, I=p, ldi=64, nq=8, ni=100, d=64, k=10, rowptr=None, excl=None, target=None, items=p,
             scores=p, rank=None, ws=p, ws_bytes=1 << 30)
    a.update(over)
    return lib.sagnn_score_topk_f32(a["Q"], a["ldq"], a["I"], a["ldi"], a["nq"], a["ni"], a["d"], a["k"], a["rowptr"],
                                    a["excl"], a["target"], a["items"], a["scores"], a["rank"], a["ws"], a["ws_bytes"],
                                    None)


def test_score_topk_rejects_every_invalid_argument():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    cases = [
        (dict(Q=None), -1, "q or i"), (dict(I=None), -1, "q or i"),
        (dict(items=None), -1, "topk_items"), (dict(scores=None), -1, "topk_items"),
        (dict(rowptr=p), -1, "excl_rowptr"), (dict(excl=p), -1, "excl_rowptr"),
        (dict(target=p), -1, "target_rank"), (dict(rank=p), -1, "target_rank"),
        (dict(k=0), -5, "k = 0"), (dict(k=129), -5, "k = 129"),
        (dict(d=24, ldq=24, ldi=24), -2, "d = 24"), (dict(d=256, ldq=256, ldi=256), -2, "d = 256"),
        (dict(ldq=66), -3, "ldq"), (dict(ldi=65), -3, "ldi"),
        (dict(ni=0), -5, "n_items"), (dict(ni=1 << 31), -5, "n_items"),
        (dict(ws_bytes=16), -6, "workspace"), (dict(ws=None), -6, "workspace"),
    ]
    for over, code, text in cases:
        assert _call(lib, buf, **over) == code, over
        assert text in _lib.last_error().lower(), (over, _lib.last_error())
    # a valid argument set gets past the checks only with a GPU: none of the above touched one


def test_score_topk_workspace_is_monotone():
    lib = _lib.load()
    f = lib.sagnn_score_topk_workspace_bytes
    for ni in (1, 4099, 52619, 1_000_003, 5_000_000):
        for d in (32, 64, 128):
            by_k = [f(512, ni, d, k) for k in (1, 2, 10, 20, 100, 128)]
            assert all(a < b for a, b in zip(by_k, by_k[1:])), (ni, d, by_k)
            by_n = [f(n, ni, d, 10) for n in (1, 7, 15, 16, 17, 33, 511, 512, 513)]
            assert all(a < b for a, b in zip(by_n, by_n[1:])), (ni, d, by_n)
    assert f(0, 100, 64, 10) == 0


def test_ops_score_topk_checks_exclusions_before_any_device_call():
    Q, I = torch.zeros((3, 64)), torch.zeros((10, 64))         # host tensors: a device call would fail differently
    with pytest.raises(ValueError, match="monotone"):
        ops.score_topk(Q, I, 5, excl=(np.array([0, 2, 1, 4]), np.array([1, 3, 4, 5])))
    with pytest.raises(ValueError, match="outside"):
        ops.score_topk(Q, I, 5, excl=(np.array([0, 2, 2, 4]), np.array([1, 3, 4, 10])))
    with pytest.raises(ValueError, match="outside"):
        ops.score_topk(Q, I, 5, excl=(np.array([0, 2, 2, 4]), np.array([-1, 3, 4, 5])))
    with pytest.raises(ValueError, match="ascending"):
        ops.score_topk(Q, I, 5, excl=(np.array([0, 2, 2, 4]), np.array([3, 1, 4, 5])))
    with pytest.raises(ValueError, match="entries"):
        ops.score_topk(Q, I, 5, excl=(np.array([0, 2, 4]), np.array([1, 3, 4, 5])))
    # a valid CSR (duplicates allowed, empty rows, rows may restart lower) passes the check
    rp, it = ops.check_exclusions(np.array([0, 2, 2, 5]), np.array([3, 3, 0, 4, 9]), 3, 10)
    assert rp.dtype == np.int32 and it.tolist() == [3, 3, 0, 4, 9]
