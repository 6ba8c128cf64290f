"""A sagnn_softmax_args that passes every host check of both softmax-loss entries, for the CPU suites that then break one
field at a time: the entries refuse before any device work, so no GPU is needed. Every field is set by name."""
import ctypes

from sa_gnn_amd import _lib

# the short names the suites' override tables use
_FIELD = dict(nq="n_queries", ni="n_items", ptr="excl_ptr", items="excl_items", row="excl_row", ws="workspace",
              ws_bytes="workspace_bytes", dIc="dI", lddic="lddi")


def aligned_buffer():
    """(the buffer to keep alive, a 16-byte aligned address inside it)"""
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    return buf, p + (-p) % 16


def softmax_args(p, mode, **over):
    """Valid operands of `mode` at the address p, those of both entries at once (an entry does not read the other's), with
    `over` on top. FULL leaves cand / n_cand / bias / dT at zero, CAND leaves bias."""
    a = dict(Q=p, ldq=64, I=p, ldi=64, n_queries=8, n_items=100, d=64, target=p, inv_temp=1.0, scale=0.125, excl_ptr=None,
             excl_items=None, excl_row=None, n_lists=0, mode=mode, loss=p, lse=p, tscore=p, g=p, dQ=p, lddq=64, dI=p,
             lddi=64, workspace=p, workspace_bytes=1 << 30)
    if mode != _lib.SOFTMAX_FULL:
        a.update(cand=p, n_cand=40, dT=p, lddt=64)
    if mode == _lib.SOFTMAX_CAND_BIAS:
        a.update(bias=p)
    a.update({_FIELD.get(k, k): v for k, v in over.items()})
    return _lib.SoftmaxArgs(**a)


def call(lib, backward, args):
    entry = lib.sagnn_softmax_loss_bwd_f32 if backward else lib.sagnn_softmax_loss_f32
    return entry(ctypes.byref(args) if args is not None else None, None)
