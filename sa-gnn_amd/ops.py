"""Tensor-level wrappers over the C ABI (include/sagnn.h): PyTorch-ROCm tensors in, HIP kernels
out. torch is used for device memory and streams only — no arithmetic happens in torch here."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import PlanInfo, Tuning, check

SUPPORTED_D = tuple(range(4, 257, 4))

# sagnn_set_engine (include/sagnn.h): arithmetic engine of the GEMM-shaped fusion stages, per calling thread
ENGINES = {"f16x2": 0, "f32": 1, "valu": 2}


def set_engine(name: str) -> None:
    check(_lib.load().sagnn_set_engine(ENGINES[name]))


def get_engine() -> str:
    code = _lib.load().sagnn_get_engine()
    return next(k for k, v in ENGINES.items() if v == code)


def range_redo_count(reset: bool = False) -> int:
    """sagnn_range_redo_count: tiles / chunks the f16 x 2 kernels re-evaluated in fp32 since the last reset."""
    n = ctypes.c_int64(0)
    check(_lib.load().sagnn_range_redo_count(ctypes.byref(n), 1 if reset else 0))
    return int(n.value)


class engine:
    """`with ops.engine("f32"): ...` — runs the block under that engine and restores the caller's."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        self.prev = get_engine()
        set_engine(self.name)
        return self

    def __exit__(self, *exc):
        set_engine(self.prev)
        return False


def _stream() -> int:
    # the raw handle of torch's current stream; torch.cuda.current_stream() builds a Stream object per call
    # (10 us, a few hundred times per training step)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _f32_rows(name: str, t: torch.Tensor | None, d: int, rows: int | None = None):
    """Checks a [rows, d] fp32 device matrix view with unit inner stride; returns its row stride."""
    if t is None:
        return 0
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a float32 device tensor, got {t.dtype} on {t.device}")
    if t.dim() != 2 or t.shape[1] != d or t.stride(1) != 1:
        raise ValueError(f"{name}: expected shape [rows, {d}] with unit inner stride, got "
                         f"{tuple(t.shape)} strides {t.stride()}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{name}: expected {rows} rows, got {t.shape[0]}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), d)


def _f32_flat(name: str, t: torch.Tensor, numel: int) -> int:
    """data_ptr of a contiguous float32 device tensor of `numel` elements (any shape), checked; a valid pointer also
    for an empty one."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a float32 device tensor")
    if not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} contiguous elements, got shape {tuple(t.shape)} strides {t.stride()}")
    return _ptr_or_empty(t)


def _ptr_or_empty(t: torch.Tensor) -> int:
    """data_ptr, or a valid stand-in for an empty tensor (whose data_ptr is 0): the entries refuse NULL at any count."""
    return t.data_ptr() or _empty_ptr(t.device)


def _one_device(ref: torch.Tensor, **others):
    """Every tensor among `others` (None = not given) lives on ref's device."""
    for name, t in others.items():
        if t is not None and t.device != ref.device:
            raise ValueError(f"{name} on {t.device}, expected {ref.device}")


def _check_weights(weights, nnz: int) -> torch.Tensor:
    """The edge weights of a plan as a host float32 tensor: nnz finite values (TypeError / ValueError otherwise)."""
    w = torch.as_tensor(weights)
    if w.dtype != torch.float32:
        raise TypeError(f"weights must be float32, got {w.dtype}")
    if w.dim() != 1 or w.numel() != nnz:
        raise ValueError(f"weights: expected {nnz} values (one per stored edge, in colidx order), got shape {tuple(w.shape)}")
    w = w.detach().cpu()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("weights: NaN or Inf among the edge weights")
    return w


MAX_BUCKETS = 65535      # bucket ids travel as uint16


def check_n_buckets(n_buckets: int) -> int:
    """The size M of a time table: 1 <= M <= 65535, refused otherwise with the flag that shrinks it."""
    n_buckets = int(n_buckets)
    if not 1 <= n_buckets <= MAX_BUCKETS:
        raise ValueError(f"edge time: {n_buckets} time buckets, the bucket ids are uint16 and the table holds at most "
                         f"{MAX_BUCKETS} rows: choose a larger --slot (days per bucket)")
    return n_buckets


def _check_buckets(buckets, n_buckets: int, nnz: int) -> torch.Tensor:
    """The bucket ids of a plan as a host uint16 tensor: nnz values < n_buckets (TypeError / ValueError otherwise)."""
    n_buckets = check_n_buckets(n_buckets)
    b = np.asarray(buckets.detach().cpu().numpy() if isinstance(buckets, torch.Tensor) else buckets)
    if b.dtype != np.uint16:
        raise TypeError(f"buckets must be uint16, got {b.dtype}")
    if b.ndim != 1 or b.size != nnz:
        raise ValueError(f"buckets: expected {nnz} values (one per stored edge, in colidx order), got shape {b.shape}")
    if b.size and int(b.max()) >= n_buckets:
        raise ValueError(f"buckets: id {int(b.max())} outside [0, {n_buckets})")
    return torch.from_numpy(np.ascontiguousarray(b))


def time_adjoint_arrays(rowptr, buckets, n_buckets: int, weights=None):
    """The "time adjoint" of a pattern with bucket ids: the CSR whose rows are buckets and whose column indices are the
    ROW of each edge, in stable bucket order (edge order kept within a bucket), the weights permuted alongside.
    dTE = (this pattern) . gm. Returns (rowptr int32 [n_buckets + 1], colidx int32 [nnz], weights or None)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    b = np.asarray(buckets, dtype=np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int32), np.diff(rowptr))
    order = np.argsort(b, kind="stable")
    rp = np.zeros(int(n_buckets) + 1, dtype=np.int64)
    np.cumsum(np.bincount(b, minlength=int(n_buckets)), out=rp[1:])
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float32)[order])
    return rp.astype(np.int32), np.ascontiguousarray(rows[order]), w


class SpmmPlan:
    """Degree-class plan for one CSR adjacency (sagnn_spmm_plan_*). Owns the device CSR copies.

    rowptr / colidx: int32, numpy or torch (host or device). With device=None a host-only plan
    is built (no GPU touched) for inspecting the chunking.

    weights: None (the unweighted sum, the kernels of a plan without weights), or nnz finite float32 values in colidx
    order, numpy or torch: every product on this plan then sums w[e] * X[colidx[e]] (sagnn_spmm_plan_set_weights,
    DESIGN.md §17). They are checked on the host; the plan keeps the device copy alive. For a correct backward pass
    the adjoint plan must carry the same weight for the same (user, item): graph.interval_pair(norm="sym") builds
    such pairs.

    buckets / n_buckets: None, or nnz uint16 bucket ids in colidx order, each < n_buckets <= 65535 (checked on the host):
    the time entries (spmm_time, gnn_interval / gnn_stack with time=) then add TE[bucket[e]] to what edge e gathers
    (sagnn_spmm_plan_set_buckets). The entries without time ignore them. `time_adjoint` is the plan of
    the dTE reduction, built on first use."""

    def __init__(self, rowptr, colidx, n_rows: int, n_src: int, device=None,
                 tuning: tuple[int, int, int] | None = None, validate: bool = True, weights=None, buckets=None,
                 n_buckets: int | None = None):
        lib = _lib.load()
        self._lib = lib
        self._h = ctypes.c_void_p()
        self.n_rows, self.n_src = int(n_rows), int(n_src)
        rp_t = torch.as_tensor(rowptr)
        ci_t = torch.as_tensor(colidx)
        if rp_t.dtype != torch.int32 or ci_t.dtype != torch.int32:
            raise TypeError("rowptr/colidx must be int32")
        if rp_t.numel() != self.n_rows + 1:
            raise ValueError(f"rowptr has {rp_t.numel()} entries, expected n_rows+1 = {self.n_rows + 1}")
        self.nnz = int(ci_t.numel())
        w_t = None if weights is None else _check_weights(weights, self.nnz)
        if w_t is not None and device is None:
            raise ValueError("weights: a host-only plan (device=None) takes no weights")
        if (buckets is None) != (n_buckets is None):
            raise ValueError("buckets: give buckets and n_buckets together")
        b_t = None if buckets is None else _check_buckets(buckets, n_buckets, self.nnz)
        if b_t is not None and device is None:
            raise ValueError("buckets: a host-only plan (device=None) takes no buckets")
        rp_h = rp_t.cpu().contiguous()
        self._rowptr_host = rp_h.numpy()
        if validate:
            ci_h = ci_t.cpu().contiguous()
            check(lib.sagnn_csr_check_host(rp_h.data_ptr(), ci_h.data_ptr(), self.n_rows, self.n_src,
                                           self.nnz))
        tun = None
        if tuning is not None:
            tun = Tuning(int(tuning[0]), int(tuning[1]), int(tuning[2]), 0)
        if device is None:
            self.rowptr = self.colidx = None
            d_rp = d_ci = None
        else:
            self.rowptr = rp_t.to(device).contiguous()
            self.colidx = ci_t.to(device).contiguous()
            if self.colidx.numel() == 0:  # keep a valid pointer for the (unused) argument
                self.colidx = torch.zeros(1, dtype=torch.int32, device=device)
            d_rp, d_ci = self.rowptr.data_ptr(), self.colidx.data_ptr()
        check(lib.sagnn_spmm_plan_create(rp_h.data_ptr(), d_rp, d_ci, self.n_rows, self.n_src,
                                         self.nnz, ctypes.byref(tun) if tun else None,
                                         ctypes.byref(self._h)))
        info = PlanInfo()
        check(lib.sagnn_spmm_plan_get_info(self._h, ctypes.byref(info)))
        self.info = info
        self.device = device
        self._ws: dict[int, torch.Tensor] = {}
        # plan of the partner's exact transpose when the (user, item) pair of an interval is not a
        # transposed pair (duplicated stored entries, graph.interval_pair); None = the pair is exact
        self.partner_adjoint: SpmmPlan | None = None
        self.weights = None
        if w_t is not None:
            self.weights = w_t.to(device).contiguous()
            if self.weights.numel() == 0:  # a valid pointer: the plan counts as weighted
                self.weights = torch.zeros(1, dtype=torch.float32, device=device)
            check(lib.sagnn_spmm_plan_set_weights(self._h, self.weights.data_ptr()))
            check(lib.sagnn_spmm_plan_get_info(self._h, ctypes.byref(info)))
        self.buckets, self.n_buckets = None, 0
        self._tuning = tuning
        self._time_adjoint: SpmmPlan | None = None
        if b_t is not None:
            self._buckets_host = b_t.numpy()
            self._weights_host = None if w_t is None else w_t.numpy()
            self.n_buckets = int(n_buckets)
            self.buckets = b_t.to(device).contiguous()
            if self.buckets.numel() == 0:
                self.buckets = torch.zeros(1, dtype=torch.uint16, device=device)
            check(lib.sagnn_spmm_plan_set_buckets(self._h, self.buckets.data_ptr(), self.n_buckets))

    @property
    def time_adjoint(self) -> "SpmmPlan":
        """The plan of this product's dTE reduction (time_adjoint_arrays), built on the first backward."""
        if self.buckets is None:
            raise ValueError("time_adjoint: the plan has no buckets")
        if self._time_adjoint is None:
            rp, ci, w = time_adjoint_arrays(self._rowptr_host, self._buckets_host, self.n_buckets, self._weights_host)
            self._time_adjoint = SpmmPlan(rp, ci, self.n_buckets, self.n_rows, device=self.device, tuning=self._tuning,
                                          validate=False, weights=w)
        return self._time_adjoint

    @property
    def weighted(self) -> bool:
        return self.weights is not None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.sagnn_spmm_plan_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def chunks(self):
        """(rows, e_begin, e_end) int32 arrays of the long-row chunk list."""
        n = int(self.info.n_chunks)
        rows = np.empty(n, np.int32)
        e0 = np.empty(n, np.int32)
        e1 = np.empty(n, np.int32)
        check(self._lib.sagnn_spmm_plan_copy_chunks(self._h, rows.ctypes.data, e0.ctypes.data,
                                                    e1.ctypes.data, n))
        return rows, e0, e1

    def workspace_bytes(self, d: int) -> int:
        return int(self._lib.sagnn_spmm_workspace_bytes(self._h, int(d)))

    def workspace(self, d: int) -> torch.Tensor | None:
        need = self.workspace_bytes(d)
        if need == 0:
            return None
        ws = self._ws.get(d)
        if ws is None:
            ws = torch.empty(need // 4, dtype=torch.float32, device=self.device)
            self._ws[d] = ws
        return ws


def spmm(plan: SpmmPlan, x: torch.Tensor, leaky: float, residual: torch.Tensor | None = None,
         out: torch.Tensor | None = None, acc_in: torch.Tensor | None = None,
         acc_out: torch.Tensor | None = None, want_out: bool = True) -> torch.Tensor | None:
    """y = max(leaky*(A·x), A·x) + residual;  out = y;  acc_out = acc_in + y  (sagnn_spmm_f32).

    Replaces Recommender.messagePropagate (reference model.py:80-92) and, through
    residual/acc_*, the adds of model.py:124-127. Returns `out` (allocated if want_out and not
    given)."""
    d = int(x.shape[1])
    ldx = _f32_rows("x", x, d, plan.n_src)
    if out is None and want_out:
        out = torch.empty((plan.n_rows, d), dtype=torch.float32, device=x.device)
    ldr = _f32_rows("residual", residual, d, plan.n_rows)
    ldo = _f32_rows("out", out, d, plan.n_rows)
    ldai = _f32_rows("acc_in", acc_in, d, plan.n_rows)
    ldao = _f32_rows("acc_out", acc_out, d, plan.n_rows)
    ws = plan.workspace(d)
    check(plan._lib.sagnn_spmm_f32(plan.handle, _ptr(x), ldx, d, _ptr(residual), ldr, float(leaky),
                                   _ptr(out), ldo, _ptr(acc_in), ldai, _ptr(acc_out), ldao,
                                   _ptr(ws), 0 if ws is None else ws.numel() * 4, _stream()))
    return out


def _call(entry, args: tuple, form_args: tuple, ws):
    """entry(*args, *form_args, workspace, workspace_bytes, stream): the one-product entries end with these three, and
    the drop and time forms take sagnn_spmm_ex_f32's arguments with their own just ahead of them."""
    check(entry(*args, *form_args, _ptr(ws), 0 if ws is None else ws.numel() * 4, _stream()))


def spmm_ex(plan: SpmmPlan, x: torch.Tensor | None, leaky: float, residual=None, out=None, acc_in=None, acc_out=None,
            acc_in2=None, mask_out=None, mask_in=None, out2=None, slope2: float = 1.0, want_out: bool = False,
            _drop=None, _time=None):
    """sagnn_spmm_ex_f32: spmm plus the training epilogue — mask_out [rows, d/4] uint8 records the activation slopes,
    out2 = v * (mask_in bit ? 1 : slope2) with v the accumulated value if acc_out is given, acc_in2 a second addend."""
    ref = next(t_ for t_ in (x, residual, out, acc_out, out2) if t_ is not None)
    d = int(ref.shape[1])
    if out is None and want_out:
        out = torch.empty((plan.n_rows, d), dtype=torch.float32, device=ref.device)
    e = _lib.SpmmEpilogue()
    e.leaky, e.slope2 = float(leaky), float(slope2)
    e.residual, e.ldr = _ptr(residual), _f32_rows("residual", residual, d, plan.n_rows)
    e.out, e.ldo = _ptr(out), _f32_rows("out", out, d, plan.n_rows)
    e.acc_in, e.ld_acc_in = _ptr(acc_in), _f32_rows("acc_in", acc_in, d, plan.n_rows)
    e.acc_out, e.ld_acc_out = _ptr(acc_out), _f32_rows("acc_out", acc_out, d, plan.n_rows)
    e.acc_in2, e.ld_acc_in2 = _ptr(acc_in2), _f32_rows("acc_in2", acc_in2, d, plan.n_rows)
    e.out2, e.ldo2 = _ptr(out2), _f32_rows("out2", out2, d, plan.n_rows)
    for name, m in (("mask_out", mask_out), ("mask_in", mask_in)):
        if m is not None:
            _masks(name, m, (plan.n_rows, d // 4))
    e.mask_out, e.mask_in = _ptr(mask_out), _ptr(mask_in)
    ldx = _f32_rows("x", x, d, plan.n_src) if x is not None else d
    ws = plan.workspace(d)
    entry, form_args = plan._lib.sagnn_spmm_ex_f32, ()
    if _drop is not None:       # spmm_drop
        drop, tag, rows_are_users = _drop
        entry, form_args = plan._lib.sagnn_spmm_drop_f32, (ctypes.byref(drop.struct()), tag, int(rows_are_users))
    if _time is not None:       # spmm_time: its `drop` must be NULL
        et = _EdgeTime(_te_table("te", _time.view(1, 1, *_time.shape) if _time.dim() == 2 else _time, (1, 1),
                                 plan.n_buckets, d), plan.n_buckets, stack=False)
        entry, form_args = plan._lib.sagnn_spmm_time_f32, (None, ctypes.byref(et.args))
    _call(entry, (plan.handle, _ptr(x), ldx, d, ctypes.byref(e)), form_args, ws)
    return out


class EdgeDrop:
    """Edge dropout of the interval graphs for one training step (sagnn_edge_drop, include/sagnn.h): every edge of
    every (interval, layer, direction) product is kept with probability `keep`, by a Philox draw keyed on
    (seed, step, interval, layer, direction, user id, item id), and the row sums are scaled by 1 / keep. The threshold
    and the scale are fixed here, once, so that host and device never disagree about a rounding. Not in the reference:
    its edgeDropout rewrites edge values that messagePropagate never reads (model.py:93-102, :84-86)."""

    def __init__(self, seed: int, step: int, keep: float):
        keep = float(keep)
        if not 0.0 < keep <= 1.0:
            raise ValueError(f"EdgeDrop: keep = {keep}, need 0 < keep <= 1")
        if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(step) < 2 ** 32:
            raise ValueError(f"EdgeDrop: seed = {seed}, step = {step}: need 0 <= seed < 2^64, 0 <= step < 2^32")
        self.seed, self.step, self.keep = int(seed), int(step), keep
        self.threshold = min(int(math.floor(keep * 2.0 ** 32)), 2 ** 32 - 1)
        self.scale = float(np.float32(1.0) / np.float32(keep))
        if self.threshold == 0:
            raise ValueError(f"EdgeDrop: keep = {keep} is below 2^-32: no edge would be kept")

    @classmethod
    def raw(cls, seed: int, step: int, threshold: int, scale: float) -> "EdgeDrop":
        """An EdgeDrop with the threshold and the scale given directly (tests and benchmarks: threshold 2^32 - 1 with
        scale 1 keeps every edge, which leaves the cost of the draw alone)."""
        self = cls(seed, step, 1.0)
        self.threshold, self.scale, self.keep = int(threshold), float(scale), int(threshold) / 2.0 ** 32
        return self

    def struct(self) -> "_lib.EdgeDropArgs":
        return _lib.EdgeDropArgs(self.seed, self.step, self.threshold, self.scale)


def edge_tag(interval: int, layer: int, direction: int) -> int:
    """The tag of one product of the stack: direction 0 = user-side (A e_i), 1 = item-side (A^T e_u)."""
    return (int(interval) << 8) | (int(layer) << 1) | int(direction)


def spmm_drop(plan: SpmmPlan, x: torch.Tensor | None, leaky: float, drop: EdgeDrop, tag: int, rows_are_users: bool,
              residual=None, out=None, acc_in=None, acc_out=None, acc_in2=None, mask_out=None, mask_in=None, out2=None,
              slope2: float = 1.0, want_out: bool = False):
    """sagnn_spmm_drop_f32: spmm_ex as one masked product — edge (user, item) takes part iff `drop` keeps it under `tag`;
    rows_are_users says whether the plan's rows are users (its column indices items) or the other way round."""
    return spmm_ex(plan, x, leaky, residual, out, acc_in, acc_out, acc_in2, mask_out, mask_in, out2, slope2, want_out,
                   _drop=(drop, int(tag), bool(rows_are_users)))


def _te_table(name: str, te: torch.Tensor, lead: tuple, n_buckets: int, d: int) -> torch.Tensor:
    if te.dtype != torch.float32 or not te.is_cuda or tuple(te.shape) != (*lead, n_buckets, d) or not te.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 device tensor {[*lead, n_buckets, d]}, got "
                         f"{tuple(te.shape)} {te.dtype} on {te.device}")
    return te


def _need_buckets(what: str, n_buckets: int) -> int:
    if not n_buckets:
        raise ValueError(f"{what}: a time table was given but the plans carry no buckets (SpmmPlan(..., buckets=, n_buckets=))")
    return n_buckets


class _EdgeTime:
    """The sagnn_edge_time of one call: TE [..., L, 2, M, d] (an interval entry: [L, 2, M, d] of its interval, `interval`
    0) and, for a backward entry, dTE with the time-adjoint plans or batch. Keeps what it points to alive."""

    def __init__(self, te: torch.Tensor, n_buckets: int, stack: bool, dte: torch.Tensor | None = None, adj=None, d: int = 0):
        a = _lib.EdgeTimeArgs()
        a.te, a.n_buckets = te.data_ptr(), int(n_buckets)
        a.stride_dir = te.stride(-3)
        a.stride_layer = te.stride(-4)
        a.stride_interval = te.stride(0) if stack else 0
        self.keep = [te, dte, adj]
        if dte is not None:
            a.dte = dte.data_ptr()
            if stack:
                a.adj_batch = adj.handle
                ws = adj.workspace(d)
            else:
                a.adj_user, a.adj_item = adj[0].handle, adj[1].handle
                ws = _interval_ws(adj[0], adj[1], d)
            self.keep.append(ws)
            a.adj_workspace, a.adj_workspace_bytes = _ptr(ws), 0 if ws is None else ws.numel() * 4
        self.args = a


def spmm_time(plan: SpmmPlan, x: torch.Tensor | None, leaky: float, te: torch.Tensor, residual=None, out=None, acc_in=None,
              acc_out=None, acc_in2=None, mask_out=None, mask_in=None, out2=None, slope2: float = 1.0,
              want_out: bool = False):
    """sagnn_spmm_time_f32: spmm_ex with the time term — edge e gathers x[colidx[e]] + te[bucket[e]]; te [n_buckets, d]
    float32, the plan built with buckets."""
    if plan.buckets is None:
        raise ValueError("spmm_time: the plan has no buckets (SpmmPlan(..., buckets=, n_buckets=))")
    return spmm_ex(plan, x, leaky, residual, out, acc_in, acc_out, acc_in2, mask_out, mask_in, out2, slope2, want_out,
                   _time=te)


def mask_scale(g: torch.Tensor, mask: torch.Tensor, slope: float, out: torch.Tensor):
    """out = g * (mask bit ? 1 : slope) (sagnn_mask_scale_f32); g / out [rows, d] views, mask [rows, d/4] uint8."""
    rows, d = int(g.shape[0]), int(g.shape[1])
    _masks("mask", mask, (rows, d // 4))
    check(_lib.load().sagnn_mask_scale_f32(_ptr(g), _f32_rows("g", g, d, rows), _ptr(mask), float(slope), _ptr(out),
                                           _f32_rows("out", out, d, rows), rows, d, _stream()))
    return out


def _interval_ws(plan_user: SpmmPlan, plan_item: SpmmPlan, d: int):
    wu, wi = plan_user.workspace(d), plan_item.workspace(d)
    return wu if (wi is None or (wu is not None and wu.numel() >= wi.numel())) else wi


def _scratch(name: str, s: torch.Tensor | None, k: int, rows: int, d: int, device):
    """A contiguous float32 scratch of at least k * rows * d elements: `s` checked, or a new one."""
    if s is None:
        return torch.empty(k * rows * d, dtype=torch.float32, device=device)
    if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() < k * rows * d:
        raise ValueError(f"{name}: need a contiguous float32 buffer of {k}*{rows}*{d} elements")
    return s


def _masks(name: str, m: torch.Tensor, shape: tuple):
    """The activation masks of a stack: a contiguous uint8 tensor of prod(shape) elements."""
    if m.dtype != torch.uint8 or not m.is_contiguous() or m.numel() != int(np.prod(shape)):
        raise ValueError(f"{name}: need a contiguous uint8 tensor {list(shape)}")
    return m


def _adjoint_pair(plan_user: SpmmPlan, plan_item: SpmmPlan):
    """The (user, item) plans the backward of an interval runs on: rows = users gathers through (item-side forward
    pattern)^T, rows = items through (user-side)^T. A transposed pair is its own adjoint; a pair with duplicated stored
    entries carries the exact adjoints (graph.interval_pair); any other pair is refused."""
    adj_u, adj_i = plan_user.partner_adjoint, plan_item.partner_adjoint
    if (adj_u is None) != (adj_i is None):
        raise ValueError("give the exact adjoint of both plans or of neither")
    if adj_u is not None:
        return adj_u, adj_i
    if plan_user.nnz != plan_item.nnz:
        raise ValueError(f"plans are not a transposed pair (nnz {plan_user.nnz} vs {plan_item.nnz}: duplicated stored "
                         "entries?) — build them with graph.interval_pair, which adds the exact adjoints")
    return plan_user, plan_item


def _gnn_args(user: tuple, item: tuple, d: int, n_layers: int, leaky: float, drop, interval: int, et, ws):
    """The sagnn_gnn_args of one stack call. user / item: (in, ld_in, slab_in, out, ld_out, slab_out, scratch, mask) of
    that node type; drop: an EdgeDrop or None; et: an _EdgeTime or None (a time call of one interval is given the TE of
    its own interval, so its `interval` is 0). The struct holds its sagnn_edge_drop / sagnn_edge_time (ctypes keeps
    the target of a pointer field); the caller holds `et`, and with it the tables and the adjoint workspace, until the
    call is over."""
    if et is not None and drop is not None:
        raise ValueError("edge dropout and time do not combine: give `drop` or `time`, not both")
    a = _lib.GnnArgs()
    for side, (x, ld_in, slab_in, out, ld_out, slab_out, scratch, mask) in ((a.user, user), (a.item, item)):
        side.in_, side.ld_in, side.slab_in = _ptr(x), ld_in, slab_in
        side.out, side.ld_out, side.slab_out = _ptr(out), ld_out, slab_out
        side.scratch, side.mask = _ptr(scratch), _ptr(mask)
    a.d, a.n_layers, a.leaky = d, int(n_layers), float(leaky)
    a.workspace, a.workspace_bytes = _ptr(ws), 0 if ws is None else ws.numel() * 4
    if et is not None:
        a.edges, a.time = _lib.EDGES_TIME, ctypes.pointer(et.args)
    elif drop is not None:
        a.edges, a.drop, a.interval = _lib.EDGES_DROP, ctypes.pointer(drop.struct()), int(interval)
    return a


def gnn_interval(plan_user: SpmmPlan, plan_item: SpmmPlan, u0: torch.Tensor, i0: torch.Tensor,
                 n_layers: int, leaky: float, user_out: torch.Tensor, item_out: torch.Tensor,
                 scratch_u: torch.Tensor | None = None, scratch_i: torch.Tensor | None = None,
                 mask_u: torch.Tensor | None = None, mask_i: torch.Tensor | None = None,
                 drop: EdgeDrop | None = None, interval: int = 0, time: torch.Tensor | None = None):
    """One interval of the GNN loop (reference model.py:118-129): sagnn_gnn_interval_f32; with `drop`, edge
    dropout under the tags of interval `interval` (SAGNN_EDGES_DROP).
    user_out / item_out are [rows, d] views (any row stride, e.g. a column of an [N, T, d] slab).
    mask_u [L, U, d/4] / mask_i [L, I, d/4] uint8 (both or neither) record the activation masks
    the backward pass needs.
    time: TE [L, 2, M, d] of this interval (layer, direction: 0 = the user-side product, 1 = the item-side one), the
    plans built with buckets (SAGNN_EDGES_TIME); not with `drop`."""
    d = int(u0.shape[1])
    U, I = plan_user.n_rows, plan_item.n_rows
    ld_u0 = _f32_rows("u0", u0, d, U)
    ld_i0 = _f32_rows("i0", i0, d, I)
    ld_uo = _f32_rows("user_out", user_out, d, U)
    ld_io = _f32_rows("item_out", item_out, d, I)
    if n_layers > 1:
        scratch_u = _scratch("scratch_u", scratch_u, 2, U, d, u0.device)
        scratch_i = _scratch("scratch_i", scratch_i, 2, I, d, u0.device)
    if mask_u is not None:
        _masks("mask_u", mask_u, (n_layers, U, d // 4))
    if mask_i is not None:
        _masks("mask_i", mask_i, (n_layers, I, d // 4))
    ws = _interval_ws(plan_user, plan_item, d)
    et = None if time is None else _EdgeTime(
        _te_table("time", time, (n_layers, 2), _need_buckets("gnn_interval", plan_user.n_buckets), d), plan_user.n_buckets,
        stack=False)
    args = _gnn_args((u0, ld_u0, 0, user_out, ld_uo, 0, scratch_u, mask_u),
                     (i0, ld_i0, 0, item_out, ld_io, 0, scratch_i, mask_i), d, n_layers, leaky, drop, interval, et, ws)
    check(plan_user._lib.sagnn_gnn_interval_f32(plan_user.handle, plan_item.handle, ctypes.byref(args), _stream()))
    return user_out, item_out


def gnn_interval_bwd(plan_user: SpmmPlan, plan_item: SpmmPlan, grad_user_out: torch.Tensor,
                     grad_item_out: torch.Tensor, n_layers: int, leaky: float, mask_u: torch.Tensor,
                     mask_i: torch.Tensor, grad_u0: torch.Tensor | None = None,
                     grad_i0: torch.Tensor | None = None, scratch_u: torch.Tensor | None = None,
                     scratch_i: torch.Tensor | None = None, drop: EdgeDrop | None = None, interval: int = 0,
                     time: torch.Tensor | None = None, grad_time: torch.Tensor | None = None):
    """Backward of gnn_interval (sagnn_gnn_interval_bwd_f32): dL/d(user_out), dL/d(item_out) and the
    recorded masks -> dL/d u0 [U, d], dL/d i0 [I, d]. `drop` / `interval`: those of the forward call.
    `time`: the TE [L, 2, M, d] of the forward call; dTE is written to grad_time (same
    shape) through the forward plans' time adjoints."""
    d = int(grad_user_out.shape[1])
    U, I = plan_user.n_rows, plan_item.n_rows
    et = None
    if time is not None:
        M = _need_buckets("gnn_interval_bwd", plan_user.n_buckets)
        et = _EdgeTime(_te_table("time", time, (n_layers, 2), M, d), M, stack=False,
                       dte=_te_table("grad_time", grad_time, (n_layers, 2), M, d),
                       adj=(plan_user.time_adjoint, plan_item.time_adjoint), d=d)
    plan_user, plan_item = _adjoint_pair(plan_user, plan_item)
    ld_gu = _f32_rows("grad_user_out", grad_user_out, d, U)
    ld_gi = _f32_rows("grad_item_out", grad_item_out, d, I)
    dev = grad_user_out.device
    if grad_u0 is None:
        grad_u0 = torch.empty((U, d), dtype=torch.float32, device=dev)
    if grad_i0 is None:
        grad_i0 = torch.empty((I, d), dtype=torch.float32, device=dev)
    ld_du = _f32_rows("grad_u0", grad_u0, d, U)
    ld_di = _f32_rows("grad_i0", grad_i0, d, I)
    scratch_u = _scratch("scratch_u", scratch_u, 4, U, d, dev)
    scratch_i = _scratch("scratch_i", scratch_i, 4, I, d, dev)
    _masks("mask_u", mask_u, (n_layers, U, d // 4))
    _masks("mask_i", mask_i, (n_layers, I, d // 4))
    ws = _interval_ws(plan_user, plan_item, d)
    args = _gnn_args((grad_user_out, ld_gu, 0, grad_u0, ld_du, 0, scratch_u, mask_u),
                     (grad_item_out, ld_gi, 0, grad_i0, ld_di, 0, scratch_i, mask_i), d, n_layers, leaky, drop, interval, et, ws)
    check(plan_user._lib.sagnn_gnn_interval_bwd_f32(plan_user.handle, plan_item.handle, ctypes.byref(args), _stream()))
    return grad_u0, grad_i0


class SpmmBatch:
    """The T interval plans of a model tied into one launch per layer (sagnn_spmm_batch_*): what the reference's
    `for k in range(args.graphNum)` loop (model.py:118) becomes when its 2 T L SpMMs are launch-bound. Keeps the
    plans alive. `adjoint()` is the batch the backward pass runs on (the same one unless a matrix holds duplicated
    stored entries, graph.interval_pair)."""

    def __init__(self, plans_user, plans_item, _time_batch: bool = False):
        if len(plans_user) != len(plans_item) or not plans_user:
            raise ValueError("one user-side and one item-side plan per interval")
        self.plans_user, self.plans_item = list(plans_user), list(plans_item)
        self.weighted = self.plans_user[0].weighted
        if any(p.weighted != self.weighted for p in self.plans_user + self.plans_item):
            raise ValueError("SpmmBatch: some plans carry edge weights and others do not; give all 2 T plans weights or none")
        # buckets: all 2 T plans with one bucket count, or the batch has none (the time entries then refuse it)
        counts = {p.n_buckets for p in self.plans_user + self.plans_item}
        self.n_buckets = counts.pop() if len(counts) == 1 else 0
        self.T, self.U, self.I = len(plans_user), plans_user[0].n_rows, plans_item[0].n_rows
        self.device = plans_user[0].device
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        PU = (ctypes.c_void_p * self.T)(*[p.handle for p in self.plans_user])
        PI = (ctypes.c_void_p * self.T)(*[p.handle for p in self.plans_item])
        create = self._lib.sagnn_spmm_time_batch_create if _time_batch else self._lib.sagnn_spmm_batch_create
        check(create(PU, PI, self.T, ctypes.byref(self._h)))
        self._time_adjoint: SpmmBatch | None = None
        self.nnz = sum(p.nnz for p in self.plans_user) + sum(p.nnz for p in self.plans_item)
        self._ws: dict[int, torch.Tensor] = {}
        self._adjoint: SpmmBatch | None = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.sagnn_spmm_batch_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def workspace(self, d: int):
        need = int(self._lib.sagnn_spmm_batch_workspace_bytes(self._h, int(d)))
        if need == 0:
            return None
        ws = self._ws.get(d)
        if ws is None:
            ws = torch.empty(need // 4, dtype=torch.float32, device=self.device)
            self._ws[d] = ws
        return ws

    @property
    def time_adjoint(self) -> "SpmmBatch":
        """The 2 T time-adjoint plans as one batch (sagnn_spmm_time_batch_create): the dTE reduction of a layer is one
        launch. Built on the first backward."""
        if not self.n_buckets:
            raise ValueError("time_adjoint: the batch's plans have no buckets")
        if self._time_adjoint is None:
            self._time_adjoint = SpmmBatch([p.time_adjoint for p in self.plans_user],
                                           [p.time_adjoint for p in self.plans_item], _time_batch=True)
        return self._time_adjoint

    def adjoint(self) -> "SpmmBatch":
        pairs = [_adjoint_pair(pu, pi) for pu, pi in zip(self.plans_user, self.plans_item)]
        if all(adj_u is pu for (adj_u, _), pu in zip(pairs, self.plans_user)):
            return self
        if self._adjoint is None:
            self._adjoint = SpmmBatch([a for a, _ in pairs], [a for _, a in pairs])
        return self._adjoint


def _slab(name: str, x: torch.Tensor, T: int, rows: int, d: int):
    """x indexed [interval, row, feature] with unit feature stride (any other strides: [T, N, d] storage or a
    permuted view of [N, T, d]); returns (ld, slab) in elements."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 3 or tuple(x.shape) != (T, rows, d) or x.stride(2) != 1:
        raise ValueError(f"{name}: expected a float32 device tensor indexed [{T}, {rows}, {d}] with unit feature stride, "
                         f"got {tuple(x.shape)} strides {x.stride()}")
    ld = int(x.stride(1)) if rows > 1 else max(int(x.stride(1)), d)
    slab = int(x.stride(0)) if T > 1 else 0
    return ld, slab


def gnn_stack(batch: SpmmBatch, u0: torch.Tensor, i0: torch.Tensor, n_layers: int, leaky: float,
              user_out: torch.Tensor, item_out: torch.Tensor, scratch_u: torch.Tensor | None = None,
              scratch_i: torch.Tensor | None = None, mask_u: torch.Tensor | None = None, mask_i: torch.Tensor | None = None,
              drop: EdgeDrop | None = None, time: torch.Tensor | None = None):
    """Every interval of the GNN loop (reference model.py:118-129) in one launch per layer: sagnn_gnn_stack_f32; with
    `drop`, edge dropout (SAGNN_EDGES_DROP).
    u0 [T, U, d], i0 [T, I, d]; user_out / item_out indexed [T, N, d] (e.g. `x.permute(1, 0, 2)` of the [N, T, d]
    tensor the fusion reads); mask_u [T, L, U, d/4] / mask_i [T, L, I, d/4] uint8 for training.
    time: TE [T, L, 2, M, d], the batch's plans built with buckets (SAGNN_EDGES_TIME); not with `drop`."""
    T, U, I = batch.T, batch.U, batch.I
    d = int(u0.shape[2])
    ld_u0, sl_u0 = _slab("u0", u0, T, U, d)
    ld_i0, sl_i0 = _slab("i0", i0, T, I, d)
    ld_uo, sl_uo = _slab("user_out", user_out, T, U, d)
    ld_io, sl_io = _slab("item_out", item_out, T, I, d)
    if n_layers > 1:
        scratch_u = _scratch("scratch_u", scratch_u, 2 * T, U, d, u0.device)
        scratch_i = _scratch("scratch_i", scratch_i, 2 * T, I, d, u0.device)
    if mask_u is not None:
        _masks("mask_u", mask_u, (T, n_layers, U, d // 4))
    if mask_i is not None:
        _masks("mask_i", mask_i, (T, n_layers, I, d // 4))
    ws = batch.workspace(d)
    et = None if time is None else _EdgeTime(
        _te_table("time", time, (T, n_layers, 2), _need_buckets("gnn_stack", batch.n_buckets), d), batch.n_buckets,
        stack=True)
    args = _gnn_args((u0, ld_u0, sl_u0, user_out, ld_uo, sl_uo, scratch_u, mask_u),
                     (i0, ld_i0, sl_i0, item_out, ld_io, sl_io, scratch_i, mask_i), d, n_layers, leaky, drop, 0, et, ws)
    check(batch._lib.sagnn_gnn_stack_f32(batch.handle, ctypes.byref(args), _stream()))
    return user_out, item_out


def gnn_stack_bwd(batch: SpmmBatch, grad_user_out: torch.Tensor, grad_item_out: torch.Tensor, n_layers: int, leaky: float,
                  mask_u: torch.Tensor, mask_i: torch.Tensor, grad_u0: torch.Tensor, grad_i0: torch.Tensor,
                  scratch_u: torch.Tensor | None = None, scratch_i: torch.Tensor | None = None,
                  drop: EdgeDrop | None = None, time: torch.Tensor | None = None, grad_time: torch.Tensor | None = None):
    """Backward of gnn_stack (sagnn_gnn_stack_bwd_f32) on the batch's adjoint patterns: gradients at the interval
    outputs [T, N, d] (any strides) -> dL/d u0 [T, U, d], dL/d i0 [T, I, d]. `drop`: that of the forward call.
    `time`: the TE [T, L, 2, M, d] of the forward call; dTE is written to grad_time (same
    shape) through the batch's time adjoint, one launch per layer."""
    adj = batch.adjoint()
    T, U, I = batch.T, batch.U, batch.I
    d = int(grad_user_out.shape[2])
    et = None
    if time is not None:
        M = _need_buckets("gnn_stack_bwd", batch.n_buckets)
        et = _EdgeTime(_te_table("time", time, (T, n_layers, 2), M, d), M, stack=True,
                       dte=_te_table("grad_time", grad_time, (T, n_layers, 2), M, d), adj=batch.time_adjoint, d=d)
    ld_gu, sl_gu = _slab("grad_user_out", grad_user_out, T, U, d)
    ld_gi, sl_gi = _slab("grad_item_out", grad_item_out, T, I, d)
    ld_du, sl_du = _slab("grad_u0", grad_u0, T, U, d)
    ld_di, sl_di = _slab("grad_i0", grad_i0, T, I, d)
    dev = grad_user_out.device
    scratch_u = _scratch("scratch_u", scratch_u, 4 * T, U, d, dev)
    scratch_i = _scratch("scratch_i", scratch_i, 4 * T, I, d, dev)
    _masks("mask_u", mask_u, (T, n_layers, U, d // 4))
    _masks("mask_i", mask_i, (T, n_layers, I, d // 4))
    ws = adj.workspace(d)
    args = _gnn_args((grad_user_out, ld_gu, sl_gu, grad_u0, ld_du, sl_du, scratch_u, mask_u),
                     (grad_item_out, ld_gi, sl_gi, grad_i0, ld_di, sl_di, scratch_i, mask_i), d, n_layers, leaky, drop, 0, et, ws)
    check(adj._lib.sagnn_gnn_stack_bwd_f32(adj.handle, ctypes.byref(args), _stream()))
    return grad_u0, grad_i0


def _ntd(name: str, x: torch.Tensor, dense_td: bool = False):
    """x is indexed [node, interval, feature]; any node/interval strides (so a permuted view of
    [t, n, d] storage works). Returns n, t, d, ld_n, ld_t."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 3:
        raise TypeError(f"{name}: expected a float32 device tensor indexed [n, t, d]")
    n, t, d = (int(v) for v in x.shape)
    if x.stride(2) != 1:
        raise ValueError(f"{name}: the feature axis must have unit stride")
    ld_n = int(x.stride(0)) if n > 1 else max(int(x.stride(0)), d)
    ld_t = int(x.stride(1)) if t > 1 else max(int(x.stride(1)), d)
    if dense_td and ld_t != d:
        raise ValueError(f"{name}: the (t, d) block of each node must be contiguous")
    return n, t, d, ld_n, ld_t


def _vec(name: str, v: torch.Tensor, numel: int):
    if v.dtype != torch.float32 or not v.is_cuda or not v.is_contiguous() or v.numel() != numel:
        raise ValueError(f"{name}: expected a contiguous float32 device tensor of {numel} elements")
    return v.data_ptr()


def _attn_ptrs(d: int, Wq, bq, Wk, bk, Wv, bv):
    """The six checked pointers of the attention's dense layers, in the order every attention entry takes them."""
    return (_vec("Wq", Wq, d * d), _vec("bq", bq, d), _vec("Wk", Wk, d * d), _vec("bk", bk, d), _vec("Wv", Wv, d * d),
            _vec("bv", bv, d))


def _wide(d: int) -> bool:
    """d handled by the 'wide' MFMA composition (multiples of 32 other than the fused 32 / 64)."""
    return d % 32 == 0 and d not in (32, 64) and _lib.load().sagnn_get_engine() != ENGINES["valu"]


def _x_vec(x: torch.Tensor, ld_n: int, ld_t: int) -> bool:
    """x rows 16-byte aligned: what csrc/engine.cpp calls "vec" and the aligned-only entries require."""
    return x.data_ptr() % 16 == 0 and ld_n % 4 == 0 and ld_t % 4 == 0


def lstm_fwd(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, forget_bias: float = 1.0,
             drop_scale: torch.Tensor | None = None, out: torch.Tensor | None = None,
             h0: torch.Tensor | None = None, c0: torch.Tensor | None = None, c_out: torch.Tensor | None = None):
    """BasicLSTMCell over T (reference model.py:135-146): sagnn_lstm_fwd_state_f32. x [n, t, d].
    h0 [n, d] (any row stride) + c0 [n, d]: state to continue from (default: zero state, as the
    reference); c_out [n, d]: receives the cell state after the last step. Cutting a sequence into
    consecutive calls gives bit-identical results to one call."""
    n, t, d, ld, ldt = _ntd("x", x)
    if out is None:
        out = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    _, _, _, ldh, _ = _ntd("out", out, dense_td=True)
    if drop_scale is not None and (not drop_scale.is_contiguous() or drop_scale.shape != x.shape):
        raise ValueError("drop_scale must be contiguous [n, t, d]")
    if (h0 is None) != (c0 is None):
        raise ValueError("give both h0 and c0 or neither")
    ld_hi = 0
    if h0 is not None:
        ld_hi = _f32_rows("h0", h0, d, n)
        if _f32_rows("c0", c0, d, n) != d:
            raise ValueError("c0 must be contiguous [n, d]")
    if c_out is not None and _f32_rows("c_out", c_out, d, n) != d:
        raise ValueError("c_out must be contiguous [n, d]")
    lib = _lib.load()
    check(lib.sagnn_lstm_fwd_state_f32(x.data_ptr(), ld, ldt, n, t, d, _vec("W", W, 8 * d * d),
                                       _vec("b", b, 4 * d), float(forget_bias), _ptr(drop_scale), _ptr(h0), ld_hi,
                                       _ptr(c0), out.data_ptr(), ldh, _ptr(c_out), _stream()))
    return out


def _ntd_dense(name: str, x: torch.Tensor, n: int, t: int, d: int) -> int:
    """x [n, t, d] float32 on the device with each node's (t, d) block contiguous; returns its node stride."""
    xn, xt, xd, ld_n, _ = _ntd(name, x, dense_td=True)
    if (xn, xt, xd) != (n, t, d):
        raise ValueError(f"{name}: expected shape [{n}, {t}, {d}], got {tuple(x.shape)}")
    return ld_n if n > 1 else max(ld_n, t * d)


def lstm_fwd_train(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, forget_bias: float = 1.0):
    """The training forward of the LSTM (sagnn_lstm_fwd_train_f32): x [n, t, d] (any node / interval strides) ->
    (h [n, t, d] un-dropped, gates [n, t, 4d], cell [n, t, d]) as lstm_bwd / lstm_bwd_step read them."""
    n, t, d, ld_n, ld_t = _ntd("x", x)
    W_p, b_p = _f32_flat("W", W, 8 * d * d), _f32_flat("b", b, 4 * d)
    _one_device(x, W=W, b=b)
    h = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    gates = torch.empty((n, t, 4 * d), dtype=torch.float32, device=x.device)
    cell = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_lstm_fwd_train_f32(x.data_ptr(), ld_n, ld_t, n, t, d, W_p, b_p, float(forget_bias), None,
                                               h.data_ptr(), t * d, gates.data_ptr(), cell.data_ptr(), _stream()))
    return h, gates, cell


def lstm_bwd_supported(d: int) -> bool:
    """Whether the one-launch BPTT (lstm_bwd) runs at this width under the calling thread's engine."""
    return bool(_lib.load().sagnn_lstm_bwd_supported(int(d)))


def lstm_bwd_workspace_bytes(n: int, t: int, d: int) -> int:
    """Bytes of gate gradients ([t, n, 4d]) lstm_bwd keeps for a deferred weight gradient."""
    return int(_lib.load().sagnn_lstm_bwd_workspace_bytes(int(n), int(t), int(d)))


def lstm_bwd(x: torch.Tensor, h: torch.Tensor, gates: torch.Tensor, cell: torch.Tensor, dh: torch.Tensor,
             drop: torch.Tensor | None, W: torch.Tensor, deferred_dw: bool):
    """Whole BPTT in one launch (sagnn_lstm_bwd_ws_f32, d in {32, 64}): x [n, t, d] (any node / interval strides), h /
    gates / cell as lstm_fwd_train stored them, dh [n, t, d] (each node's block contiguous) = the gradient at the emitted
    h, drop None or the [n, t, d] scale of the emitted h -> (dx [n, t, d], dW [2d, 4d], db [4d]).
    deferred_dw: keep the gate gradients ([t, n, 4d], allocated here) and take the weight gradient as a second pass on
    the f16 x 2 engine instead of the BPTT launch's fp32-MFMA product."""
    n, t, d, ld_n, ld_t = _ntd("x", x)
    h_p, g_p, c_p = _f32_flat("h", h, n * t * d), _f32_flat("gates", gates, n * t * 4 * d), _f32_flat("cell", cell, n * t * d)
    ld_dh = _ntd_dense("dh", dh, n, t, d)
    drop_p = None if drop is None else _f32_flat("drop", drop, n * t * d)
    W_p = _f32_flat("W", W, 8 * d * d)
    _one_device(x, h=h, gates=gates, cell=cell, dh=dh, drop=drop, W=W)
    dev = x.device
    dx = torch.empty((n, t, d), dtype=torch.float32, device=dev)
    dW = torch.zeros((2 * d, 4 * d), dtype=torch.float32, device=dev)
    db = torch.zeros(4 * d, dtype=torch.float32, device=dev)
    need = lstm_bwd_workspace_bytes(n, t, d) if deferred_dw else 0
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
    check(_lib.load().sagnn_lstm_bwd_ws_f32(x.data_ptr(), ld_n, ld_t, h_p, g_p, c_p, dh.data_ptr(), ld_dh, drop_p, W_p,
                                            dx.data_ptr(), dW.data_ptr(), db.data_ptr(), n, t, d, _ptr(ws), need, _stream()))
    return dx, dW, db


def lstm_bwd_step(gates: torch.Tensor, cell: torch.Tensor, dh: torch.Tensor, drop: torch.Tensor | None,
                  dh_rec: torch.Tensor | None, dc_in: torch.Tensor | None, dgates: torch.Tensor, dc_out: torch.Tensor,
                  ts: int):
    """Step ts of the generic BPTT (sagnn_lstm_bwd_step_f32): gates [n, t, 4d] / cell [n, t, d] of lstm_fwd_train,
    dh [n, t, d] the gradient at the emitted h (drop: its [n, t, d] scale, or None), dh_rec [n, d] (any row stride)
    and dc_in [n, d] the recurrent gradients from step ts + 1 (both None at the last step) -> dgates [n, 4d] and
    dc_out [n, d], written."""
    if gates.dim() != 3 or gates.shape[2] % 4:
        raise ValueError(f"gates: expected [n, t, 4d], got {tuple(gates.shape)}")
    n, t, d = int(gates.shape[0]), int(gates.shape[1]), int(gates.shape[2]) // 4
    g_p, c_p = _f32_flat("gates", gates, n * t * 4 * d), _f32_flat("cell", cell, n * t * d)
    ld_dh = _ntd_dense("dh", dh, n, t, d)
    drop_p = None if drop is None else _f32_flat("drop", drop, n * t * d)
    if (dh_rec is None) != (dc_in is None):
        raise ValueError("dh_rec and dc_in go together (both, or neither at the last step)")
    ld_rec = _f32_rows("dh_rec", dh_rec, d, n)
    dc_in_p = None if dc_in is None else _f32_flat("dc_in", dc_in, n * d)
    dg_p, dc_p = _f32_flat("dgates", dgates, n * 4 * d), _f32_flat("dc_out", dc_out, n * d)
    _one_device(gates, cell=cell, dh=dh, drop=drop, dh_rec=dh_rec, dc_in=dc_in, dgates=dgates, dc_out=dc_out)
    check(_lib.load().sagnn_lstm_bwd_step_f32(g_p, c_p, dh.data_ptr(), ld_dh, drop_p, _ptr(dh_rec), ld_rec, dc_in_p, dg_p,
                                              dc_p, n, t, d, int(ts), _stream()))


def gru_fused_supported(d: int) -> bool:
    """Whether the GRU forward runs as one launch persistent over t at this width (sagnn_gru_fused_supported: d = 32,
    64); elsewhere gru_fwd runs one step at a time."""
    return bool(_lib.load().sagnn_gru_fused_supported(int(d)))


def _gru_fwd(x, Wg, bg, Wc, bc, drop_scale, out, gates, cand):
    n, t, d, ld_n, ld_t = _ntd("x", x)
    w_p = (_f32_flat("Wg", Wg, 4 * d * d), _f32_flat("bg", bg, 2 * d), _f32_flat("Wc", Wc, 2 * d * d), _f32_flat("bc", bc, d))
    drop_p = None if drop_scale is None else _f32_flat("drop_scale", drop_scale, n * t * d)
    ld_h = _ntd_dense("out", out, n, t, d)
    _one_device(x, Wg=Wg, bg=bg, Wc=Wc, bc=bc, drop_scale=drop_scale, out=out)
    lib = _lib.load()
    need = int(lib.sagnn_gru_workspace_bytes(n, t, d))
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device) if need else None
    check(lib.sagnn_gru_fwd_f32(x.data_ptr(), ld_n, ld_t, n, t, d, *w_p, drop_p, _ptr_or_empty(out), ld_h, _ptr(gates),
                                _ptr(cand), _ptr(ws), need, _stream()))


def gru_fwd(x: torch.Tensor, Wg: torch.Tensor, bg: torch.Tensor, Wc: torch.Tensor, bc: torch.Tensor,
            drop_scale: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """TF 1.14 GRUCell over T, zero initial state (--rnnCell gru): sagnn_gru_fwd_f32. x [n, t, d] (any
    node / interval strides), Wg [2d, 2d] (r | u), bg [2d], Wc [2d, d], bc [d], drop_scale None or [n, t, d] contiguous
    (scales the emitted h only) -> h [n, t, d] (`out`: each node's block contiguous). Exact fp32 under every engine."""
    n, t, d = (int(v) for v in x.shape)
    if out is None:
        out = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    _gru_fwd(x, Wg, bg, Wc, bc, drop_scale, out, None, None)
    return out


def gru_fwd_train(x: torch.Tensor, Wg: torch.Tensor, bg: torch.Tensor, Wc: torch.Tensor, bc: torch.Tensor):
    """The training forward of the GRU: -> (h [n, t, d] un-dropped, gates [n, t, 2d] = r | u, cand [n, t, d]) as
    gru_bwd_cand / gru_bwd_gates read them. h is gru_fwd's bit for bit."""
    n, t, d = (int(v) for v in x.shape)
    h = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    gates = torch.empty((n, t, 2 * d), dtype=torch.float32, device=x.device)
    cand = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    _gru_fwd(x, Wg, bg, Wc, bc, None, h, gates, cand)
    return h, gates, cand


def gru_bwd_cand(gates: torch.Tensor, cand: torch.Tensor, h: torch.Tensor, dh: torch.Tensor, drop: torch.Tensor | None,
                 dh_rec: torch.Tensor | None, da_c: torch.Tensor, du: torch.Tensor, dh_u: torch.Tensor, ts: int):
    """Step ts of the GRU's BPTT, candidate half (sagnn_gru_bwd_cand_f32): gates / cand / h of gru_fwd_train, dh
    [n, t, d] the gradient at the emitted h (drop: its scale or None), dh_rec [n, d] (any row stride) the recurrent
    gradient from step ts + 1 (None at the last step) -> da_c, du, dh_u, each [n, d] contiguous, written."""
    n, t, d = (int(v) for v in cand.shape)
    g_p, c_p, h_p = _f32_flat("gates", gates, n * t * 2 * d), _f32_flat("cand", cand, n * t * d), _f32_flat("h", h, n * t * d)
    ld_dh = _ntd_dense("dh", dh, n, t, d)
    drop_p = None if drop is None else _f32_flat("drop", drop, n * t * d)
    ld_rec = _f32_rows("dh_rec", dh_rec, d, n)
    outs = (_f32_flat("da_c", da_c, n * d), _f32_flat("du", du, n * d), _f32_flat("dh_u", dh_u, n * d))
    _one_device(gates, cand=cand, h=h, dh=dh, drop=drop, dh_rec=dh_rec, da_c=da_c, du=du, dh_u=dh_u)
    check(_lib.load().sagnn_gru_bwd_cand_f32(g_p, c_p, h_p, _ptr_or_empty(dh), ld_dh, drop_p, _ptr(dh_rec), ld_rec, *outs,
                                             n, t, d, int(ts), _stream()))


def gru_bwd_gates(gates: torch.Tensor, h: torch.Tensor, du: torch.Tensor, dh_u: torch.Tensor, d_rh: torch.Tensor,
                  da_g: torch.Tensor, rh: torch.Tensor | None, ts: int):
    """Step ts of the GRU's BPTT, gate half (sagnn_gru_bwd_gates_f32): d_rh [n, d] (any row stride) holds d(r.h_prev)
    and becomes the recurrent gradient dh_u + d(r.h_prev) r; da_g [n, 2d] and, when given, rh [n, d] = r.h_prev are
    written (both contiguous)."""
    n, t, d = (int(v) for v in h.shape)
    g_p, h_p = _f32_flat("gates", gates, n * t * 2 * d), _f32_flat("h", h, n * t * d)
    du_p, dhu_p = _f32_flat("du", du, n * d), _f32_flat("dh_u", dh_u, n * d)
    ld_drh = _f32_rows("d_rh", d_rh, d, n)
    dag_p = _f32_flat("da_g", da_g, n * 2 * d)
    rh_p = None if rh is None else _f32_flat("rh", rh, n * d)
    _one_device(gates, h=h, du=du, dh_u=dh_u, d_rh=d_rh, da_g=da_g, rh=rh)
    check(_lib.load().sagnn_gru_bwd_gates_f32(g_p, h_p, du_p, dhu_p, _ptr_or_empty(d_rh), ld_drh, dag_p, rh_p, n, t, d, int(ts),
                                              _stream()))


def layernorm_td(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12,
                 out: torch.Tensor | None = None):
    """layer_norm over (t, d) per node (reference model.py:152-153): sagnn_layernorm_td_f32."""
    n, t, d, ld, ldt = _ntd("x", x)
    if out is None:
        out = torch.empty((n, t, d), dtype=torch.float32, device=x.device)
    _, _, _, ldy, _ = _ntd("out", out, dense_td=True)
    check(_lib.load().sagnn_layernorm_td_f32(x.data_ptr(), ld, ldt, n, t, d, _vec("gamma", gamma, d),
                                             _vec("beta", beta, d), float(eps), out.data_ptr(), ldy,
                                             _stream()))
    return out


def layernorm_td_bwd(x: torch.Tensor, g: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-12,
                     out: torch.Tensor | None = None):
    """Backward of layernorm_td (sagnn_layernorm_td_bwd_f32): x the forward's input and g the gradient at its output,
    both [n, t, d] with each node's (t, d) block contiguous (any node stride) -> (dx, dgamma [d], dbeta [d]). dx goes
    to `out` (the same layout; out=g runs in place) or to a new tensor."""
    n, t, d, ld_x, _ = _ntd("x", x, dense_td=True)
    if n == 1:
        ld_x = max(ld_x, t * d)
    ld_g = _ntd_dense("g", g, n, t, d)
    gamma_p = _f32_flat("gamma", gamma, d)
    _one_device(x, g=g, gamma=gamma, out=out)
    if out is None:
        out, ld_o = torch.empty((n, t, d), dtype=torch.float32, device=x.device), t * d
    else:
        ld_o = _ntd_dense("out", out, n, t, d)
    dgamma = torch.zeros(d, dtype=torch.float32, device=x.device)
    dbeta = torch.zeros(d, dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_layernorm_td_bwd_f32(x.data_ptr(), ld_x, g.data_ptr(), ld_g, n, t, d, gamma_p, float(eps),
                                                 out.data_ptr(), ld_o, dgamma.data_ptr(), dbeta.data_ptr(), _stream()))
    return out, dgamma, dbeta


def mhsa_mean(x: torch.Tensor, Wq, bq, Wk, bk, Wv, bv, heads: int, out: torch.Tensor | None = None):
    """MultiHeadSelfAttention + mean over T (reference Utils/attention.py:55-78, model.py:154-155):
    sagnn_mhsa_mean_f32. x [n, t, d] -> [n, d]."""
    n, t, d, ld, ldt = _ntd("x", x)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    ldo = _f32_rows("out", out, d, n)
    lib = _lib.load()
    if _wide(d) and _x_vec(x, ld, ldt):      # the wide entry takes aligned rows only; sagnn_mhsa_mean_f32 takes any
        ws = torch.empty(int(lib.sagnn_mhsa_wide_workspace_bytes(n, t, d)) // 4, dtype=torch.float32, device=x.device)
        check(lib.sagnn_mhsa_mean_wide_f32(x.data_ptr(), ld, ldt, n, t, d, int(heads), *_attn_ptrs(d, Wq, bq, Wk, bk, Wv, bv),
                                           out.data_ptr(), ldo, ws.data_ptr(), ws.numel() * 4, _stream()))
        return out
    check(lib.sagnn_mhsa_mean_f32(x.data_ptr(), ld, ldt, n, t, d, int(heads), *_attn_ptrs(d, Wq, bq, Wk, bk, Wv, bv),
                                  out.data_ptr(), ldo, _stream()))
    return out


def ln_mhsa_mean(x: torch.Tensor, gamma, beta, Wq, bq, Wk, bk, Wv, bv, heads: int, eps: float = 1e-12,
                 out: torch.Tensor | None = None):
    """layer_norm over (T, d) -> MHSA -> mean (reference model.py:152-155) in one call:
    sagnn_ln_mhsa_mean_f32 (fused on the matrix-core path). x [n, t, d] -> [n, d]."""
    n, t, d, ld, ldt = _ntd("x", x)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    ldo = _f32_rows("out", out, d, n)
    lib = _lib.load()
    if _x_vec(x, ld, ldt):
        need = int(lib.sagnn_ln_mhsa_mean_workspace_bytes(n, t, d, int(heads)))
    else:   # the query assumes aligned x (sagnn.h); an unaligned one runs unfused: y, plus Q|K|V where that is Wide
        need = n * t * d * 4 + int(lib.sagnn_mhsa_wide_workspace_bytes(n, t, d))
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device) if need else None
    check(lib.sagnn_ln_mhsa_mean_f32(
        x.data_ptr(), ld, ldt, n, t, d, int(heads), _vec("gamma", gamma, d), _vec("beta", beta, d), float(eps),
        *_attn_ptrs(d, Wq, bq, Wk, bk, Wv, bv), out.data_ptr(), ldo, _ptr(ws), need, _stream()))
    return out


def attn_bwd_front_supported(d: int, t: int, heads: int) -> bool:
    """Whether attn_bwd_front covers the shape under the calling thread's engine."""
    return bool(_lib.load().sagnn_attn_bwd_front_supported(int(d), int(t), int(heads)))


def attn_bwd_front(x: torch.Tensor, gamma, beta, Wq, bq, Wk, bk, Wv, bv, heads: int, g_out: torch.Tensor,
                   want_y: bool = True):
    """The front of the attention backward in one launch (sagnn_attn_bwd_front_f32): y = LN(x), Q|K|V = y W + b and the
    attention backward for g_out [n, d] (any row stride). x [n, t, d] (any node / interval strides) ->
    (y [n*t, d] or None, dqkv [n*t, 3d]). gamma None = no layer norm (y = x, not written)."""
    n, t, d, ld_n, ld_t = _ntd("x", x)
    if (gamma is None) != (beta is None):
        raise ValueError("gamma and beta go together (both, or neither for no layer norm)")
    gamma_p, beta_p = (None, None) if gamma is None else (_f32_flat("gamma", gamma, d), _f32_flat("beta", beta, d))
    w_p = _attn_ptrs(d, Wq, bq, Wk, bk, Wv, bv)
    ld_g = _f32_rows("g_out", g_out, d, n)
    _one_device(x, gamma=gamma, beta=beta, Wq=Wq, bq=bq, Wk=Wk, bk=bk, Wv=Wv, bv=bv, g_out=g_out)
    dqkv = torch.empty((n * t, 3 * d), dtype=torch.float32, device=x.device)
    y = torch.empty((n * t, d), dtype=torch.float32, device=x.device) if (want_y and gamma is not None) else None
    check(_lib.load().sagnn_attn_bwd_front_f32(x.data_ptr(), ld_n, ld_t, n, t, d, int(heads), gamma_p, beta_p, 1e-12,
                                               0 if gamma is None else 1, *w_p, g_out.data_ptr(), ld_g, dqkv.data_ptr(),
                                               _ptr(y), _stream()))
    return y, dqkv


def attn_bwd(qkv: torch.Tensor, g_out: torch.Tensor, n: int, t: int, heads: int):
    """The attention backward of mhsa_mean (sagnn_attn_bwd_f32), in place: qkv [n*t, 3d] contiguous (Q | K | V rows as
    y W + b produced them) becomes dQ | dK | dV for g_out [n, d] (any row stride). Returns qkv."""
    if qkv.dim() != 2 or qkv.shape[1] % 3:
        raise ValueError(f"qkv: expected [n*t, 3d], got {tuple(qkv.shape)}")
    n, t, d = int(n), int(t), int(qkv.shape[1]) // 3
    qkv_p = _f32_flat("qkv", qkv, n * t * 3 * d)
    ld_g = _f32_rows("g_out", g_out, d, n)
    _one_device(qkv, g_out=g_out)
    check(_lib.load().sagnn_attn_bwd_f32(qkv_p, g_out.data_ptr(), ld_g, n, t, d, int(heads), _stream()))
    return qkv


def attn_bwd_tail_supported(d: int) -> bool:
    """Whether attn_bwd_tail runs at this width under the calling thread's engine."""
    return bool(_lib.load().sagnn_attn_bwd_tail_supported(int(d)))


def attn_bwd_tail(y2: torch.Tensor, dqkv: torch.Tensor, Wqkv: torch.Tensor, dWqkv: torch.Tensor, dbqkv: torch.Tensor):
    """The tail of the attention backward in one pass over dqkv [rows, 3d] (sagnn_attn_bwd_tail_f32): dWqkv [d, 3d] +=
    y2^T dqkv, dbqkv [3d] += its column sums (zero both first) and dy = dqkv Wqkv^T written OVER y2 [rows, d]; all
    contiguous, Wqkv = [Wq | Wk | Wv]. Returns y2, now dy."""
    if y2.dim() != 2:
        raise ValueError(f"y2: expected [rows, d], got {tuple(y2.shape)}")
    rows, d = int(y2.shape[0]), int(y2.shape[1])
    y_p, dqkv_p = _f32_flat("y2", y2, rows * d), _f32_flat("dqkv", dqkv, rows * 3 * d)
    W_p, dW_p, db_p = _f32_flat("Wqkv", Wqkv, 3 * d * d), _f32_flat("dWqkv", dWqkv, 3 * d * d), _f32_flat("dbqkv", dbqkv, 3 * d)
    _one_device(y2, dqkv=dqkv, Wqkv=Wqkv, dWqkv=dWqkv, dbqkv=dbqkv)
    check(_lib.load().sagnn_attn_bwd_tail_f32(y_p, dqkv_p, rows, d, W_p, dW_p, db_p, _stream()))
    return y2


LSTM_KEYS = ("lstm_W", "lstm_b")
GRU_KEYS = ("gru_Wg", "gru_bg", "gru_Wc", "gru_bc")


def fusion_cell(p: dict) -> str:
    """"lstm" or "gru": which recurrent cell a fusion parameter dict carries (all of LSTM_KEYS, or all of GRU_KEYS).
    Both cells: ValueError; neither, or part of one: KeyError, as reading the missing key would raise."""
    has = [any(k in p for k in keys) for keys in (LSTM_KEYS, GRU_KEYS)]
    if has[0] and has[1]:
        raise ValueError("fusion parameters: give the LSTM's (lstm_W, lstm_b) or the GRU's (gru_Wg, gru_bg, gru_Wc, gru_bc), not both")
    keys = GRU_KEYS if has[1] else LSTM_KEYS
    missing = [k for k in keys if k not in p]
    if missing:
        raise KeyError(f"fusion parameters: missing {missing}" + ("" if any(has) else " (found neither cell)"))
    return "gru" if has[1] else "lstm"


def interval_fusion(x: torch.Tensor, p: dict, heads: int, out: torch.Tensor | None = None,
                    workspace: torch.Tensor | None = None):
    """LSTM -> layer_norm -> MHSA -> mean (reference model.py:135-155): sagnn_interval_fusion_f32.
    p: lstm_W [2d,4d], lstm_b [4d], ln_gamma [d], ln_beta [d], Wq/bq/Wk/bk/Wv/bv.
    With gru_Wg [2d,2d], gru_bg [2d], gru_Wc [2d,d], gru_bc [d] in place of lstm_W / lstm_b (--rnnCell gru): the GRU
    (gru_fwd) into the workspace, then ln_mhsa_mean on it. A dict with both cells or neither is refused."""
    lib = _lib.load()
    n, t, d, ld, ldt = _ntd("x", x)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    ldo = _f32_rows("out", out, d, n)
    if fusion_cell(p) == "gru":
        if workspace is None or workspace.numel() * workspace.element_size() < n * t * d * 4 or workspace.dtype != torch.float32:
            workspace = torch.empty(max(n * t * d, 1), dtype=torch.float32, device=x.device)
        h = gru_fwd(x, *(p[k] for k in GRU_KEYS), out=workspace.view(-1)[:n * t * d].view(n, t, d))
        return ln_mhsa_mean(h, p["ln_gamma"], p["ln_beta"], *(p[k] for k in ("Wq", "bq", "Wk", "bk", "Wv", "bv")), heads, out=out)
    need = int(lib.sagnn_interval_fusion_workspace_bytes(n, t, d))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=x.device)
    check(lib.sagnn_interval_fusion_f32(
        x.data_ptr(), ld, ldt, n, t, d, int(heads), _vec("lstm_W", p["lstm_W"], 8 * d * d),
        _vec("lstm_b", p["lstm_b"], 4 * d), 1.0, _vec("ln_gamma", p["ln_gamma"], d),
        _vec("ln_beta", p["ln_beta"], d), 1e-12, *_attn_ptrs(d, *(p[k] for k in ("Wq", "bq", "Wk", "bk", "Wv", "bv"))),
        out.data_ptr(), ldo, workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()))
    return out


def dense_nn(x: torch.Tensor, W: torch.Tensor, bias: torch.Tensor | None = None, out: torch.Tensor | None = None,
             accumulate: bool = False):
    """Y (+)= X @ W + bias on the matrix cores (sagnn_dense_nn_f32). x [n, din] (row stride free),
    W [din, dout] contiguous."""
    n, din = int(x.shape[0]), int(x.shape[1])
    dout = int(W.shape[1])
    ldx = _f32_rows("x", x, din)
    if out is None:
        out = torch.empty((n, dout), dtype=torch.float32, device=x.device)
    ldy = _f32_rows("out", out, dout, n)
    check(_lib.load().sagnn_dense_nn_f32(x.data_ptr(), ldx, n, din, dout, _vec("W", W, din * dout),
                                         None if bias is None else _vec("bias", bias, dout), out.data_ptr(), ldy,
                                         int(accumulate), _stream()))
    return out


def dense_tn(x: torch.Tensor, g: torch.Tensor, dW: torch.Tensor, db: torch.Tensor | None = None):
    """dW += X^T @ G, db += colsum(G) (sagnn_dense_tn_f32). Accumulates: zero dW/db first."""
    n, din = int(x.shape[0]), int(x.shape[1])
    dout = int(g.shape[1])
    ldx = _f32_rows("x", x, din)
    ldg = _f32_rows("g", g, dout, n)
    check(_lib.load().sagnn_dense_tn_f32(x.data_ptr(), ldx, g.data_ptr(), ldg, n, din, dout,
                                         _vec("dW", dW, din * dout), None if db is None else _vec("db", db, dout),
                                         _stream()))
    return dW


def dense_tn_seg(x: torch.Tensor, g: torch.Tensor, dW: torch.Tensor, db: torch.Tensor | None = None):
    """dW += sum_s x[s]^T @ g[s], db += column sums of g (sagnn_dense_tn_seg_f32): x [s, n, din], g [s, n, dout] as
    VIEWS with any segment / row strides (unit column stride) — e.g. x.permute(1, 0, 2) of a node-major [n, t, d]
    against gate gradients stored [t, n, 4d]: a whole BPTT's weight gradient in one launch. Accumulates."""
    if x.dim() != 3 or g.dim() != 3 or x.shape[:2] != g.shape[:2]:
        raise ValueError(f"dense_tn_seg: need x [s, n, din] and g [s, n, dout], got {tuple(x.shape)} / {tuple(g.shape)}")
    for name, v in (("x", x), ("g", g)):
        if v.dtype != torch.float32 or not v.is_cuda or v.stride(2) != 1:
            raise ValueError(f"dense_tn_seg: {name} must be float32 on the GPU with unit column stride")
    s_, n, din = (int(v) for v in x.shape)
    dout = int(g.shape[2])
    if s_ == 0 or n == 0:
        return dW
    check(_lib.load().sagnn_dense_tn_seg_f32(x.data_ptr(), int(x.stride(1)), int(x.stride(0)), g.data_ptr(), int(g.stride(1)),
                                             int(g.stride(0)), n, s_, din, dout, _vec("dW", dW, din * dout),
                                             None if db is None else _vec("db", db, dout), _stream()))
    return dW


def mul(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None):
    """out = a * b element-wise (sagnn_mul_f32); contiguous float32 tensors of equal size."""
    if out is None:
        out = torch.empty_like(a)
    for name, x in (("a", a), ("b", b), ("out", out)):
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != a.numel():
            raise ValueError(f"{name}: need contiguous float32 tensors of equal size")
        if x.device != a.device:          # e.g. a dropout mask left on the host: its pointer would fault the kernel
            raise ValueError(f"{name} is on {x.device}, a on {a.device}: need all three on one device")
    check(_lib.load().sagnn_mul_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()))
    return out


class Adam:
    """tf.train.AdamOptimizer with the reference's staircase exponential decay and L2 weights
    (model.py:245-250): state per parameter tensor, ONE sagnn_adam_multi_f32 launch per step.

    A parameter whose gradient is None still takes the step when it is L2-regularised: TF
    differentiates loss + reg*Regularize(), so timeEmbed and the dead [d, d] weights of
    model.py:81 receive 2*reg*w and decay. Un-regularised tensors without a gradient are left
    alone (TF's minimize skips variables with no gradient)."""

    def __init__(self, params: dict, lr: float, decay: float = 1.0, decay_step: int = 1, reg: float = 0.0,
                 reg_names=(), beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
        self.params = params
        self.lr0, self.decay, self.decay_step, self.reg = lr, decay, max(int(decay_step), 1), reg
        self.reg_names = set(reg_names)
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        self.global_step = 0

    def learning_rate(self) -> float:
        return self.lr0 * self.decay ** (self.global_step // self.decay_step)     # staircase=True

    def step(self, grads: dict):
        lr = self.learning_rate()
        self.global_step += 1
        names, keep = [], []
        for k, g in grads.items():
            if g is None and not (k in self.reg_names and self.reg != 0.0):
                continue
            p = self.params[k]
            if not p.is_contiguous():
                raise ValueError(f"parameter {k!r} must be contiguous")
            if g is not None:
                g = g.contiguous()
                if g.numel() != p.numel() or g.dtype != torch.float32:
                    raise ValueError(f"gradient of {k!r}: expected {p.numel()} float32 elements")
                keep.append(g)                      # alive until the launch is queued
            names.append((k, g))
        n = len(names)
        if n == 0:
            return
        P, G, M, V = ((ctypes.c_void_p * n)() for _ in range(4))
        C, L2 = (ctypes.c_int64 * n)(), (ctypes.c_float * n)()
        for i, (k, g) in enumerate(names):
            p = self.params[k]
            P[i], G[i], M[i], V[i] = p.data_ptr(), (None if g is None else g.data_ptr()), self.m[k].data_ptr(), self.v[k].data_ptr()
            C[i], L2[i] = p.numel(), (self.reg if k in self.reg_names else 0.0)
        check(_lib.load().sagnn_adam_multi_f32(n, P, G, M, V, C, L2, lr, self.b1, self.b2, self.eps, self.global_step,
                                               _stream()))

    def state_dict(self) -> dict:
        """Slots and step counter, as tf.train.Saver stores them with the variables (model.py:512-520)."""
        out = {"global_step": torch.tensor(self.global_step, dtype=torch.int64)}
        for k in self.params:
            out["m/" + k] = self.m[k].detach().cpu()
            out["v/" + k] = self.v[k].detach().cpu()
        return out

    def load_state_dict(self, state: dict):
        want = {"global_step"} | {"m/" + k for k in self.params} | {"v/" + k for k in self.params}
        if set(state) != want:
            raise KeyError(f"optimizer state keys differ: missing {sorted(want - set(state))[:4]}, "
                           f"unexpected {sorted(set(state) - want)[:4]}")
        for k in self.params:
            for slot, name in ((self.m, "m/"), (self.v, "v/")):
                if tuple(state[name + k].shape) != tuple(slot[k].shape):
                    raise ValueError(f"optimizer slot {name + k}: shape {tuple(state[name + k].shape)} != {tuple(slot[k].shape)}")
                slot[k].copy_(state[name + k])
        self.global_step = int(state["global_step"])


def leaky_add(a: torch.Tensor, b: torch.Tensor | None, leaky: float, out: torch.Tensor | None = None):
    """out = max(leaky*a, a) + b (sagnn_leaky_add_f32); contiguous float32."""
    if out is None:
        out = torch.empty_like(a)
    for name, x in (("a", a), ("b", b), ("out", out)):
        if x is not None and (x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != a.numel()):
            raise ValueError(f"{name}: need contiguous float32 tensors of equal size")
    check(_lib.load().sagnn_leaky_add_f32(a.data_ptr(), _ptr(b), out.data_ptr(), float(leaky), a.numel(), _stream()))
    return out


def leaky(a: torch.Tensor, leaky: float):
    """out = max(leaky*a, a) (sagnn_leaky_f32, forward form); contiguous float32."""
    n = int(a.numel()) if isinstance(a, torch.Tensor) else 0
    a_p = _f32_flat("a", a, n)
    out = torch.empty_like(a)
    check(_lib.load().sagnn_leaky_f32(a_p, None, _ptr_or_empty(out), float(leaky), n, 0, _stream()))
    return out


def leaky_bwd(a: torch.Tensor, g: torch.Tensor, leaky: float):
    """da = g * (the slope of max(leaky*a, a) at a: `leaky` wherever a <= leaky*a) (sagnn_leaky_f32, backward form); a the
    pre-activation, contiguous float32 tensors of equal size."""
    n = int(a.numel()) if isinstance(a, torch.Tensor) else 0
    a_p, g_p = _f32_flat("a", a, n), _f32_flat("g", g, n)
    _one_device(a, g=g)
    out = torch.empty_like(a)
    check(_lib.load().sagnn_leaky_f32(a_p, g_p, _ptr_or_empty(out), float(leaky), n, 1, _stream()))
    return out


def pair_score(U: torch.Tensor, I: torch.Tensor, uids: torch.Tensor, iids: torch.Tensor, S: torch.Tensor | None = None,
               A: torch.Tensor | None = None, locs: torch.Tensor | None = None, leaky: float = 1.0):
    """preds[e] = <U[uids[e]], I[iids[e]]> + <leaky(S[locs[e]]), A[iids[e]]> (sagnn_pair_score_f32)."""
    d = int(U.shape[1])
    n = int(uids.numel())
    out = torch.empty(n, dtype=torch.float32, device=U.device)
    for name, x in (("uids", uids), ("iids", iids), ("locs", locs)):
        if x is not None and (x.dtype != torch.int32 or not x.is_contiguous() or x.numel() != n):
            raise ValueError(f"{name}: need a contiguous int32 tensor of {n} elements")
    check(_lib.load().sagnn_pair_score_f32(
        U.data_ptr(), _f32_rows("U", U, d), I.data_ptr(), _f32_rows("I", I, d), _ptr(S),
        0 if S is None else _f32_rows("S", S, d), _ptr(A), 0 if A is None else _f32_rows("A", A, d),
        uids.data_ptr(), iids.data_ptr(), _ptr(locs), float(leaky), out.data_ptr(), n, d, _stream()))
    return out


def _zeros_like_table(t: torch.Tensor) -> torch.Tensor:
    """The dense zero gradient of a table (the kernels add into dense rows whatever the table's own stride)."""
    return torch.zeros(tuple(t.shape), dtype=torch.float32, device=t.device)


def pair_score_bwd(U: torch.Tensor, I: torch.Tensor, uids: torch.Tensor, iids: torch.Tensor, g: torch.Tensor,
                   S: torch.Tensor | None = None, A: torch.Tensor | None = None, locs: torch.Tensor | None = None,
                   leaky: float = 1.0):
    """Gradients of pair_score for g [n_pairs] (sagnn_pair_score_bwd_f32, a scatter with float atomics): returns
    (dU, dI, dS, dA), dense and shaped like their tables; dS and dA are None without the second term. S, A and locs are
    given together or not at all. When A is I, dA IS dI: both sums land in the one tensor."""
    if U.dim() != 2:
        raise ValueError(f"U: expected a [rows, d] table, got {tuple(U.shape)}")
    d, n = int(U.shape[1]), int(uids.numel())
    ldu, ldi = _f32_rows("U", U, d), _f32_rows("I", I, d)
    head = S is not None
    if (A is not None) != head or (locs is not None) != head:
        raise ValueError("S, A and locs go together (all or none)")
    lds, lda = _f32_rows("S", S, d), _f32_rows("A", A, d)
    uids_p, iids_p = _idx_ptr("uids", uids, torch.int32, n), _idx_ptr("iids", iids, torch.int32, n)
    locs_p = _idx_ptr("locs", locs, torch.int32, n) if head else None
    g_p = _f32_flat("g", g, n)
    _one_device(U, I=I, S=S, A=A, uids=uids, iids=iids, locs=locs, g=g)
    dU, dI = _zeros_like_table(U), _zeros_like_table(I)
    dS = _zeros_like_table(S) if head else None
    dA = (dI if A is I else _zeros_like_table(A)) if head else None
    check(_lib.load().sagnn_pair_score_bwd_f32(U.data_ptr(), ldu, I.data_ptr(), ldi, _ptr(S), lds, _ptr(A), lda, uids_p, iids_p,
                                               locs_p, float(leaky), g_p, dU.data_ptr(), dI.data_ptr(), _ptr(dS), _ptr(dA),
                                               n, d, _stream()))
    return dU, dI, dS, dA


def _pair_args(X, Y, uids, iids):
    """The checked leading arguments of the SSL pair entries and (n_pairs, d)."""
    if X.dim() != 2:
        raise ValueError(f"X: expected a [rows, d] table, got {tuple(X.shape)}")
    d, n = int(X.shape[1]), int(uids.numel())
    lead = (X.data_ptr(), _f32_rows("X", X, d), Y.data_ptr(), _f32_rows("Y", Y, d), _idx_ptr("uids", uids, torch.int32, n),
            _idx_ptr("iids", iids, torch.int32, n))
    _one_device(X, Y=Y, uids=uids, iids=iids)
    return lead, n, d


def prod_leaky_sum(X: torch.Tensor, Y: torch.Tensor, uids: torch.Tensor, iids: torch.Tensor, leaky: float):
    """s[e] = sum_j leaky(X[uids[e]][j] * Y[iids[e]][j]) (sagnn_prod_leaky_sum_f32) -> [n_pairs]."""
    lead, n, d = _pair_args(X, Y, uids, iids)
    out = torch.empty(n, dtype=torch.float32, device=X.device)
    check(_lib.load().sagnn_prod_leaky_sum_f32(*lead, float(leaky), _ptr_or_empty(out), n, d, _stream()))
    return out


def prod_leaky_sum_bwd(X: torch.Tensor, Y: torch.Tensor, uids: torch.Tensor, iids: torch.Tensor, leaky: float,
                       g: torch.Tensor):
    """Gradients of prod_leaky_sum for g [n_pairs] (sagnn_prod_leaky_sum_bwd_f32, a scatter with float atomics):
    (dX, dY), dense and shaped like their tables."""
    lead, n, d = _pair_args(X, Y, uids, iids)
    g_p = _f32_flat("g", g, n)
    _one_device(X, g=g)
    dX, dY = _zeros_like_table(X), _zeros_like_table(Y)
    check(_lib.load().sagnn_prod_leaky_sum_bwd_f32(*lead, float(leaky), g_p, dX.data_ptr(), dY.data_ptr(), n, d, _stream()))
    return dX, dY


def _meta_args(F, V, uids):
    """The checked leading arguments of the meta-feature entries and (n, d). F and V are tables over the same users."""
    if F.dim() != 2:
        raise ValueError(f"F: expected a [rows, d] table, got {tuple(F.shape)}")
    d, n = int(F.shape[1]), int(uids.numel())
    ldf, ldv = _f32_rows("F", F, d), _f32_rows("V", V, d, int(F.shape[0]))
    lead = (F.data_ptr(), ldf, V.data_ptr(), ldv, _idx_ptr("uids", uids, torch.int32, n))
    _one_device(F, V=V, uids=uids)
    return lead, n, d


def meta_features(F: torch.Tensor, V: torch.Tensor, uids: torch.Tensor):
    """m[e] = [F[u] * V[u] | F[u] | V[u]], u = uids[e] (sagnn_meta_features_f32) -> [n, 3d] contiguous."""
    lead, n, d = _meta_args(F, V, uids)
    out = torch.empty((n, 3 * d), dtype=torch.float32, device=F.device)
    check(_lib.load().sagnn_meta_features_f32(*lead, _ptr_or_empty(out), n, d, _stream()))
    return out


def meta_features_bwd(F: torch.Tensor, V: torch.Tensor, uids: torch.Tensor, dm: torch.Tensor):
    """Gradients of meta_features for dm [n, 3d] contiguous (sagnn_meta_features_bwd_f32, a scatter with float
    atomics): (dF, dV), dense and shaped like their tables."""
    lead, n, d = _meta_args(F, V, uids)
    if dm.dim() != 2 or dm.shape[1] != 3 * d:
        raise ValueError(f"dm: expected [{n}, {3 * d}], got {tuple(dm.shape)}")
    dm_p = _f32_flat("dm", dm, n * 3 * d)
    _one_device(F, dm=dm)
    dF, dV = _zeros_like_table(F), _zeros_like_table(V)
    check(_lib.load().sagnn_meta_features_bwd_f32(*lead, dm_p, dF.data_ptr(), dV.data_ptr(), n, d, _stream()))
    return dF, dV


def _rowdot_A(A: torch.Tensor, k: int) -> tuple[int, int]:
    """A [n, kp] float32 with kp >= k columns and unit inner stride (the row-dot reads the first k): (n, row stride)."""
    if not isinstance(A, torch.Tensor) or A.dim() != 2 or A.shape[1] < k:
        raise ValueError(f"A: expected [n, at least {k}], got {tuple(A.shape) if isinstance(A, torch.Tensor) else type(A)}")
    return int(A.shape[0]), _f32_rows("A", A, int(A.shape[1]))


def rowdot_sigmoid(A: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, k: int):
    """w[e] = sigmoid(<A[e, :k], w3> + b3) (sagnn_rowdot_sigmoid_f32): A [n, kp >= k] (any row stride), w3 [k], b3 [1]
    -> [n]."""
    k = int(k)
    n, lda = _rowdot_A(A, k)
    w3_p, b3_p = _f32_flat("w3", w3, k), _f32_flat("b3", b3, 1)
    _one_device(A, w3=w3, b3=b3)
    out = torch.empty(n, dtype=torch.float32, device=A.device)
    check(_lib.load().sagnn_rowdot_sigmoid_f32(_ptr_or_empty(A), lda, w3_p, b3_p, _ptr_or_empty(out), n, k, _stream()))
    return out


def rowdot_sigmoid_bwd(A: torch.Tensor, w3: torch.Tensor, w: torch.Tensor, dw: torch.Tensor, k: int):
    """Gradients of rowdot_sigmoid given its output w [n] and dw [n] (sagnn_rowdot_sigmoid_bwd_f32): (dA shaped like A,
    contiguous, columns >= k zero; dw3 [k]; db3 [1])."""
    k = int(k)
    n, lda = _rowdot_A(A, k)
    kp = int(A.shape[1])
    w3_p, w_p, dw_p = _f32_flat("w3", w3, k), _f32_flat("w", w, n), _f32_flat("dw", dw, n)
    _one_device(A, w3=w3, w=w, dw=dw)
    dA = _zeros_like_table(A)
    dw3 = torch.zeros(k, dtype=torch.float32, device=A.device)
    db3 = torch.zeros(1, dtype=torch.float32, device=A.device)
    check(_lib.load().sagnn_rowdot_sigmoid_bwd_f32(_ptr_or_empty(A), lda, w3_p, w_p, dw_p, _ptr_or_empty(dA), kp,
                                                   dw3.data_ptr(), db3.data_ptr(), n, k, _stream()))
    return dA, dw3, db3


def hinge(pos: torch.Tensor, neg: torch.Tensor, wp: torch.Tensor | None = None, wn: torch.Tensor | None = None,
          sp: torch.Tensor | None = None, sn: torch.Tensor | None = None, scale: float = 1.0):
    """loss = scale * sum max(0, 1 - S * (pos - neg)), S = wp * sp - wn * sn, or 1 without weights (sagnn_hinge_f32);
    contiguous float32 [n] each, the four weights given together or not at all (sp / sn are constants). Returns
    (loss [1], dpos, dneg, dwp, dwn): the gradients of the loss, dwp / dwn None without weights."""
    n = int(pos.numel()) if isinstance(pos, torch.Tensor) else 0
    pos_p, neg_p = _f32_flat("pos", pos, n), _f32_flat("neg", neg, n)
    weights = {"wp": wp, "wn": wn, "sp": sp, "sn": sn}
    weighted = wp is not None
    if any((v is not None) != weighted for v in weights.values()):
        raise ValueError("wp, wn, sp and sn go together (all or none)")
    w_p = [_f32_flat(k, v, n) for k, v in weights.items()] if weighted else [None] * 4
    _one_device(pos, neg=neg, **weights)
    dev = pos.device
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    dpos, dneg = torch.empty_like(pos), torch.empty_like(neg)
    dwp, dwn = (torch.empty_like(wp), torch.empty_like(wn)) if weighted else (None, None)
    check(_lib.load().sagnn_hinge_f32(pos_p, neg_p, *w_p, float(scale), loss.data_ptr(), _ptr_or_empty(dpos),
                                      _ptr_or_empty(dneg), _ptr_or_empty(dwp) if weighted else None,
                                      _ptr_or_empty(dwn) if weighted else None, n, _stream()))
    return loss, dpos, dneg, dwp, dwn


_topk_ws: dict = {}      # device -> workspace of sagnn_score_topk_f32, grown on demand (no allocation once warm)


def _topk_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    ws = _topk_ws.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _topk_ws[device] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    return ws


def check_exclusions(rowptr, items, n_rows: int, n_items: int):
    """Validates an exclusion CSR on the host (rowptr [n_rows + 1] from 0, monotone, ending at len(items); ids in
    [0, n_items), ascending within a row) and returns it as int32 numpy arrays."""
    as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    rp, it = as_np(rowptr).astype(np.int64).reshape(-1), as_np(items).astype(np.int64).reshape(-1)
    if rp.size != n_rows + 1 or rp[0] != 0 or rp[-1] != it.size:
        raise ValueError(f"excl rowptr: need {n_rows + 1} entries from 0 to len(items) = {it.size}")
    if (np.diff(rp) < 0).any():
        raise ValueError("excl rowptr: not monotone")
    if it.size and (it.min() < 0 or it.max() >= n_items):
        raise ValueError(f"excl items: ids outside [0, {n_items})")
    row = np.repeat(np.arange(n_rows), np.diff(rp))
    if ((np.diff(it) < 0) & (row[1:] == row[:-1])).any():
        raise ValueError("excl items: ids must be ascending within a row")
    return rp.astype(np.int32), it.astype(np.int32)


class ExclusionCSR:
    """An exclusion CSR for score_topk, checked once on the host (check_exclusions) and uploaded once: rowptr int32
    [n_rows + 1] into items int32, both on `device`. rows(lo, hi) is the CSR of rows [lo, hi) as a view (rowptr
    entries index the shared items array directly, so nothing is rebased or copied)."""

    def __init__(self, rowptr, items, n_rows: int, n_items: int, device):
        rp, it = check_exclusions(rowptr, items, n_rows, n_items)
        self.n_rows, self.n_items = int(n_rows), int(n_items)
        self.rowptr = torch.from_numpy(rp).to(device)
        # an empty items array still needs a valid pointer (never read: every row is empty)
        self.items = torch.from_numpy(it).to(device) if it.size else torch.zeros(1, dtype=torch.int32, device=device)

    def rows(self, lo: int, hi: int) -> "ExclusionCSR":
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.n_rows:
            raise ValueError(f"rows [{lo}, {hi}) outside [0, {self.n_rows})")
        view = ExclusionCSR.__new__(ExclusionCSR)
        view.n_rows, view.n_items = hi - lo, self.n_items
        view.rowptr, view.items = self.rowptr[lo:hi + 1], self.items
        return view


def score_topk(Q: torch.Tensor, I: torch.Tensor, k: int, excl=None, target=None):
    """The best k items of every row of Q over the whole item table I (sagnn_score_topk_f32): score <Q[b], I[i]> in
    fp32, higher first, equal scores to the lower id, NaN never returned. excl = (rowptr, items): a CSR of item ids
    per row left out (checked on the host, then uploaded), or an ExclusionCSR (checked and uploaded already);
    target [B]: items whose rank is returned (always eligible).
    Returns (items int32 [B, k], scores float32 [B, k], rank int64 [B] or None); empty slots hold -1 / -inf."""
    lib = _lib.load()
    if Q.dim() != 2:
        raise ValueError(f"Q: expected [B, d], got {tuple(Q.shape)}")
    B, d = int(Q.shape[0]), int(Q.shape[1])
    n_items = int(I.shape[0]) if I.dim() == 2 else 0
    pre = isinstance(excl, ExclusionCSR)
    if pre and (excl.n_rows != B or excl.n_items != n_items):
        raise ValueError(f"excl: an ExclusionCSR of {excl.n_rows} rows over {excl.n_items} items, "
                         f"Q has {B} rows and I {n_items} items")
    ex = None if (excl is None or pre) else check_exclusions(excl[0], excl[1], B, n_items)
    ldq, ldi = _f32_rows("Q", Q, d), _f32_rows("I", I, d)
    dev = Q.device
    if I.device != dev:
        raise ValueError(f"I on {I.device}, Q on {dev}")
    rp_d = it_d = tg_d = rank = None
    if pre:
        if excl.rowptr.device != dev:
            raise ValueError(f"excl on {excl.rowptr.device}, Q on {dev}")
        rp_d, it_d = excl.rowptr, excl.items
    elif ex is not None:
        rp, it = ex
        rp_d = torch.from_numpy(rp).to(dev)
        it_d = torch.from_numpy(it).to(dev) if it.size else torch.zeros(1, dtype=torch.int32, device=dev)
    if target is not None:
        tg_d = torch.as_tensor(target, device=dev)
        if tg_d.dtype != torch.int32 or tg_d.dim() != 1 or tg_d.numel() != B or not tg_d.is_contiguous():
            raise ValueError(f"target: need a contiguous int32 vector of {B} elements")
        rank = torch.empty(B, dtype=torch.int64, device=dev)
    items = torch.empty((B, int(k)), dtype=torch.int32, device=dev)
    scores = torch.empty((B, int(k)), dtype=torch.float32, device=dev)
    need = int(lib.sagnn_score_topk_workspace_bytes(B, n_items, d, int(k)))
    ws = _topk_workspace(dev, need) if need else None
    check(lib.sagnn_score_topk_f32(Q.data_ptr(), ldq, I.data_ptr(), ldi, B, n_items, d, int(k), _ptr(rp_d), _ptr(it_d),
                                   _ptr(tg_d), items.data_ptr(), scores.data_ptr(), _ptr(rank), _ptr(ws), need, _stream()))
    return items, scores, rank


_softmax_ws: dict = {}   # (cand, device, n_queries, positions, d) -> workspace of a softmax-loss entry and its backward


def _softmax_workspace(device: torch.device, B: int, n_pos: int, d: int, cand: bool = False):
    """The cached workspace of sagnn_softmax_loss_f32 over n_pos = n_items positions, or with `cand` that of its
    candidate modes over n_pos = n_cand, shared with the entry's backward, and its size in bytes."""
    key = (cand, device, B, n_pos, d)
    ws = _softmax_ws.get(key)
    if ws is None:
        lib = _lib.load()
        bytes_fn = lib.sagnn_softmax_loss_cand_workspace_bytes if cand else lib.sagnn_softmax_loss_workspace_bytes
        need = int(bytes_fn(B, n_pos, d))
        if len(_softmax_ws) >= 8:      # a training run has one or two sizes (the last batch of an epoch is shorter)
            _softmax_ws.clear()
        ws = _softmax_ws[key] = (torch.empty(max(need, 256), dtype=torch.uint8, device=device), need)
    return ws


def _lse_g_check(lse, g, B: int, dev):
    """The backward wrappers' check of the forward's lse [B] and the upstream scalar g."""
    for name, t, n in (("lse", lse, B), ("g", g, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() \
                or t.numel() != n:
            raise ValueError(f"{name}: need a contiguous float32 tensor of {n} elements on {dev}")


def _softmax_struct(mode, Q, I, target, inv_temp, scale, excl, excl_row, cand=None, bias=None):
    """Host checks of the four softmax-loss wrappers, once and before any device call. Returns a SoftmaxArgs with the
    mode, the shared operands and, in a candidate mode, cand / n_cand / bias set (the outputs and the workspace are the
    caller's), and (B, n_items, d, n_cand)."""
    full = mode == _lib.SOFTMAX_FULL
    if not full and (not isinstance(cand, torch.Tensor) or cand.dim() != 1):
        raise ValueError("cand: expected int32 [n_cand]")
    if not isinstance(Q, torch.Tensor) or Q.dim() != 2:
        raise ValueError(f"Q: expected [B, d], got {tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q)}")
    B, d = int(Q.shape[0]), int(Q.shape[1])
    if d not in (32, 64, 128):
        raise ValueError(f"softmax_loss: d = {d}, need 32, 64 or 128")
    n_items = int(I.shape[0]) if isinstance(I, torch.Tensor) and I.dim() == 2 else 0
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"I: expected [n_items, {d}] with 1 <= n_items < 2^31")
    inv_temp = float(inv_temp)
    if not (inv_temp > 0.0 and np.isfinite(inv_temp)):
        raise ValueError(f"inv_temp = {inv_temp}: need a finite value > 0")
    scale = 1.0 / max(B, 1) if scale is None else float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"scale = {scale} is not finite")
    ldq, ldi = _f32_rows("Q", Q, d), _f32_rows("I", I, d)
    dev = Q.device
    if I.device != dev:
        raise ValueError(f"I on {I.device}, Q on {dev}")
    tgt = _idx_ptr("target", target, torch.int32, B)
    if target.device != dev:
        raise ValueError(f"target on {target.device}, Q on {dev}")
    ptr_p = items_p = row_p = None
    n_lists = 0
    if excl is None:
        if excl_row is not None:
            raise ValueError("excl_row without excl")
    else:
        ex_ptr, ex_items = excl
        if not isinstance(ex_ptr, torch.Tensor) or ex_ptr.dim() != 1 or ex_ptr.numel() < 1:
            raise ValueError("excl: expected (ptr int64 [n_lists + 1], items int32) device tensors")
        n_lists = int(ex_ptr.numel()) - 1
        ptr_p = _idx_ptr("excl ptr", ex_ptr, torch.int64)
        items_p = _idx_ptr("excl items", ex_items, torch.int32)
        if ex_ptr.device != dev or ex_items.device != dev:
            raise ValueError(f"excl on {ex_ptr.device} / {ex_items.device}, Q on {dev}")
        if excl_row is not None:
            row_p = _idx_ptr("excl_row", excl_row, torch.int32, B)
            if excl_row.device != dev:
                raise ValueError(f"excl_row on {excl_row.device}, Q on {dev}")
        elif n_lists < B:
            raise ValueError(f"excl: {n_lists} lists for {B} rows and no excl_row")
    a = _lib.SoftmaxArgs(mode=mode, Q=Q.data_ptr(), ldq=ldq, I=I.data_ptr(), ldi=ldi, n_queries=B, n_items=n_items, d=d,
                         target=tgt, inv_temp=inv_temp, scale=scale, excl_ptr=ptr_p, excl_items=items_p, excl_row=row_p,
                         n_lists=n_lists)
    if full:
        return a, (B, n_items, d, 0)
    n_cand = int(cand.numel())
    if n_cand > n_items:
        raise ValueError(f"cand: {n_cand} candidates for {n_items} items")
    a.cand, a.n_cand = _idx_ptr("cand", cand, torch.int32), n_cand
    if cand.device != dev:
        raise ValueError(f"cand on {cand.device}, Q on {dev}")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.dim() != 1 or bias.numel() != n_cand \
                or not bias.is_contiguous() or bias.device != dev:
            raise ValueError(f"bias: need a contiguous float32 vector of {n_cand} elements on {dev}")
        # an empty tensor's data_ptr is 0; the entry reads no offset at n_cand == 0
        a.bias = bias.data_ptr() if n_cand else None
    return a, (B, n_items, d, n_cand)


def _softmax_call(entry, a, dev, B: int, n_pos: int, d: int) -> None:
    """Sets the workspace of n_pos positions on the filled struct and calls one of the two entries with it."""
    ws, need = _softmax_workspace(dev, B, n_pos, d, cand=a.mode != _lib.SOFTMAX_FULL)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    check(entry(ctypes.byref(a), _stream()))


def softmax_loss(Q: torch.Tensor, I: torch.Tensor, target: torch.Tensor, inv_temp: float = 1.0, scale: float | None = None,
                 excl=None, excl_row: torch.Tensor | None = None):
    """Full-catalogue softmax cross-entropy (sagnn_softmax_loss_f32): z[b, i] = <Q[b], I[i]> * inv_temp,
    loss = scale * sum_b (lse[b] - z[b, target[b]]), lse[b] = ln sum exp z[b, i] over row b's eligible items: all of
    [0, n_items) except its exclusion list, the target always eligible. target int32 [B], rows with a target outside
    [0, n_items) are skipped. excl = (ptr int64 [n_lists + 1], items int32) device tensors, lists ascending; row b uses
    list excl_row[b] (int32 [B]) or list b. scale defaults to 1 / max(B, 1).
    Returns (loss [1], lse [B], tscore [B] = <Q[b], I[target[b]]>); the logits are never stored."""
    a, (B, n_items, d, _) = _softmax_struct(_lib.SOFTMAX_FULL, Q, I, target, inv_temp, scale, excl, excl_row)
    dev = Q.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lse, tscore = _out(B, torch.float32, dev), _out(B, torch.float32, dev)
    a.loss, a.lse, a.tscore = loss.data_ptr(), lse.data_ptr(), tscore.data_ptr()
    _softmax_call(_lib.load().sagnn_softmax_loss_f32, a, dev, B, n_items, d)
    return loss, lse, tscore


def softmax_loss_bwd(Q: torch.Tensor, I: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, g: torch.Tensor,
                     inv_temp: float = 1.0, scale: float | None = None, excl=None, excl_row: torch.Tensor | None = None):
    """Gradients of softmax_loss (sagnn_softmax_loss_bwd_f32) given the forward's lse [B] and the upstream scalar g (a
    1-element float32 device tensor): returns (dQ [B, d], dI [n_items, d]), every row written, the logits recomputed."""
    a, (B, n_items, d, _) = _softmax_struct(_lib.SOFTMAX_FULL, Q, I, target, inv_temp, scale, excl, excl_row)
    dev = Q.device
    _lse_g_check(lse, g, B, dev)
    dQ = torch.empty((max(B, 1), d), dtype=torch.float32, device=dev)[:B]
    dI = torch.empty((n_items, d), dtype=torch.float32, device=dev)
    a.lse, a.g = lse.data_ptr() if B else dQ.data_ptr(), g.data_ptr()
    a.dQ, a.lddq, a.dI, a.lddi = dQ.data_ptr(), d, dI.data_ptr(), d
    _softmax_call(_lib.load().sagnn_softmax_loss_bwd_f32, a, dev, B, n_items, d)
    return dQ, dI


def sample_strata(n_items: int, n_cand: int, seed: int, step: int, device) -> torch.Tensor:
    """The candidate list of --softmaxNegs (sagnn_sample_strata_i32): int32 [n_cand] on `device`, candidate j one
    uniform draw from [floor(j n_items / n_cand), floor((j + 1) n_items / n_cand)) keyed by (seed, step, j): strictly
    ascending and distinct, a pure function of its arguments, arange(n_items) when n_cand == n_items."""
    n_items, n_cand, seed, step = int(n_items), int(n_cand), int(seed), int(step)
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"sample_strata: n_items = {n_items}, need 1 <= n_items < 2^31")
    if n_cand < 0 or n_cand > n_items:
        raise ValueError(f"sample_strata: n_cand = {n_cand}, need 0 <= n_cand <= n_items = {n_items}")
    if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 32:
        raise ValueError(f"sample_strata: seed = {seed}, step = {step}, need 0 <= seed < 2^64 and 0 <= step < 2^32")
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"sample_strata: expected a GPU device, got {device}")
    cand = _out(n_cand, torch.int32, device)
    check(_lib.load().sagnn_sample_strata_i32(n_items, n_cand, seed, step, cand.data_ptr(), _stream()))
    return cand


def sample_strata_weighted(cum: torch.Tensor, total: int, n_cand: int, seed: int, step: int):
    """The candidate list of --softmaxNegDist pop (sagnn_sample_strata_w_i32): cum int64 [n_items] on the device, the
    inclusive prefix sum of the items' integer weights, total = its last entry W as a host int (no read-back here).
    Returns (cand int32 [n_cand], bias float32 [n_cand]): candidate j is the item whose mass holds one uniform draw from
    stratum j of [0, W), keyed by (seed, step, j); the list is non-decreasing, the first position of a run of equal ids
    carries bias = ln(run length) - ln(n_cand w_c / W), the others -inf. A pure function of its arguments."""
    total, n_cand, seed, step = int(total), int(n_cand), int(seed), int(step)
    if not isinstance(cum, torch.Tensor) or cum.dim() != 1 or cum.dtype != torch.int64 or not cum.is_cuda \
            or not cum.is_contiguous() or not 1 <= cum.numel() < 2 ** 31:
        raise ValueError("sample_strata_weighted: cum: need a contiguous int64 device vector [n_items], 1 <= n_items < 2^31")
    if not 1 <= total < 2 ** 62:
        raise ValueError(f"sample_strata_weighted: total = {total}, need 1 <= total < 2^62")
    if n_cand < 0 or n_cand >= 2 ** 31 or n_cand > total:
        raise ValueError(f"sample_strata_weighted: n_cand = {n_cand}, need 0 <= n_cand <= total = {total} and n_cand < 2^31")
    if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 32:
        raise ValueError(f"sample_strata_weighted: seed = {seed}, step = {step}, need 0 <= seed < 2^64 and 0 <= step < 2^32")
    cand, bias = _out(n_cand, torch.int32, cum.device), _out(n_cand, torch.float32, cum.device)
    check(_lib.load().sagnn_sample_strata_w_i32(cum.data_ptr(), int(cum.numel()), total, n_cand, seed, step, cand.data_ptr(),
                                                bias.data_ptr(), _stream()))
    return cand, bias


def softmax_loss_cand(Q: torch.Tensor, I: torch.Tensor, cand: torch.Tensor, target: torch.Tensor, inv_temp: float = 1.0,
                      scale: float | None = None, excl=None, excl_row: torch.Tensor | None = None,
                      bias: torch.Tensor | None = None):
    """softmax_loss over a candidate list (sagnn_softmax_loss_f32, SAGNN_SOFTMAX_CAND): cand int32 [n_cand], strictly ascending
    ids of [0, n_items) (not checked: they address rows of I); row b sums over the candidates outside its exclusion list and
    other than target[b], plus target[b] itself, exactly once. n_cand == 0 is legal. The other arguments and the
    returned (loss [1], lse [B], tscore [B]) are those of softmax_loss.
    With bias float32 [n_cand] (SAGNN_SOFTMAX_CAND_BIAS, what sample_strata_weighted draws) cand is non-decreasing
    with adjacent repeats, position j adds bias[j] to its logit and counts only where bias[j] > -inf; the target's own
    term takes no offset."""
    mode = _lib.SOFTMAX_CAND if bias is None else _lib.SOFTMAX_CAND_BIAS
    a, (B, n_items, d, n_cand) = _softmax_struct(mode, Q, I, target, inv_temp, scale, excl, excl_row, cand, bias)
    dev = Q.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lse, tscore = (torch.empty(max(B, 1), dtype=torch.float32, device=dev) for _ in range(2))
    a.loss, a.lse, a.tscore = loss.data_ptr(), lse.data_ptr(), tscore.data_ptr()
    _softmax_call(_lib.load().sagnn_softmax_loss_f32, a, dev, B, n_cand, d)
    return loss, lse[:B], tscore[:B]


def softmax_loss_cand_bwd(Q: torch.Tensor, I: torch.Tensor, cand: torch.Tensor, target: torch.Tensor, lse: torch.Tensor,
                          g: torch.Tensor, inv_temp: float = 1.0, scale: float | None = None, excl=None,
                          excl_row: torch.Tensor | None = None, bias: torch.Tensor | None = None):
    """Gradients of softmax_loss_cand (sagnn_softmax_loss_bwd_f32, same mode) given the forward's lse [B] and the upstream
    scalar g (a 1-element float32 device tensor): returns (dQ [B, d], dIc [n_cand, d], dT [B, d]), every row written.
    Row j of dIc is the candidates' share of dI[cand[j]], dT[b] the target's share of dI[target[b]]. With the forward's
    bias (SAGNN_SOFTMAX_CAND_BIAS) the dIc rows of the positions at -inf are zeros."""
    mode = _lib.SOFTMAX_CAND if bias is None else _lib.SOFTMAX_CAND_BIAS
    a, (B, n_items, d, n_cand) = _softmax_struct(mode, Q, I, target, inv_temp, scale, excl, excl_row, cand, bias)
    dev = Q.device
    _lse_g_check(lse, g, B, dev)
    # one row at least behind every output: an empty tensor's data_ptr is 0 and the entry refuses NULL at any count
    dQ = torch.empty((max(B, 1), d), dtype=torch.float32, device=dev)
    dT = torch.empty((max(B, 1), d), dtype=torch.float32, device=dev)
    dIc = torch.empty((max(n_cand, 1), d), dtype=torch.float32, device=dev)
    a.lse, a.g = lse.data_ptr() if B else dQ.data_ptr(), g.data_ptr()
    a.dQ, a.lddq, a.dI, a.lddi, a.dT, a.lddt = dQ.data_ptr(), d, dIc.data_ptr(), d, dT.data_ptr(), d
    _softmax_call(_lib.load().sagnn_softmax_loss_bwd_f32, a, dev, B, n_cand, d)
    return dQ[:B], dIc[:n_cand], dT[:B]


def softmax_cand_scatter(dI: torch.Tensor, dIc: torch.Tensor, cand: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """dI[cand[j]] = dIc[j] in place for every position with bias[j] > -inf (sagnn_softmax_cand_scatter_f32): the live
    rows of softmax_loss_cand_bwd's dIc into a full-size dI. The live ids are distinct, so every row has one writer."""
    n_cand, d = int(dIc.shape[0]), int(dIc.shape[1])
    if bias.dtype != torch.float32 or bias.numel() != n_cand or not bias.is_contiguous() or cand.numel() != n_cand:
        raise ValueError(f"softmax_cand_scatter: need cand and a contiguous float32 bias of {n_cand} elements")
    _one_device(dI, dIc=dIc, cand=cand, bias=bias)
    check(_lib.load().sagnn_softmax_cand_scatter_f32(dIc.data_ptr() if n_cand else None, _f32_rows("dIc", dIc, d) if n_cand else d,
                                                     _idx_ptr("cand", cand, torch.int32), bias.data_ptr() if n_cand else None,
                                                     n_cand, int(dI.shape[0]), d, dI.data_ptr(), _f32_rows("dI", dI, d),
                                                     _stream()))
    return dI


def softmax_target_add(dI: torch.Tensor, dT: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """dI[target[b]] += dT[b] in place for every row with a target in [0, n_items) (sagnn_softmax_target_add_f32): rows
    that share a target are added in ascending b by one thread, so the result is the same in every run."""
    B, d = int(dT.shape[0]), int(dT.shape[1])
    check(_lib.load().sagnn_softmax_target_add_f32(dT.data_ptr() if B else dI.data_ptr(), _f32_rows("dT", dT, d) if B else d,
                                                   _idx_ptr("target", target, torch.int32, B), B, int(dI.shape[0]), d,
                                                   dI.data_ptr(), _f32_rows("dI", dI, d), _stream()))
    return dI


def softmax_target_scatter(dI: torch.Tensor, dT: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """softmax_target_add for row counts far beyond a batch (sagnn_softmax_target_scatter_f32, --seqTargets all): the same
    sum dI[target[r]] += dT[r] in place, with float atomics, so equal between runs up to the order of summation."""
    B, d = int(dT.shape[0]), int(dT.shape[1])
    _one_device(dI, dT=dT, target=target)
    check(_lib.load().sagnn_softmax_target_scatter_f32(dT.data_ptr() if B else dI.data_ptr(), _f32_rows("dT", dT, d) if B else d,
                                                       _idx_ptr("target", target, torch.int32, B), B, int(dI.shape[0]), d,
                                                       dI.data_ptr(), _f32_rows("dI", dI, d), _stream()))
    return dI


def candidate_rank(U: torch.Tensor, I: torch.Tensor, uids: torch.Tensor, cand: torch.Tensor, target: torch.Tensor,
                   S: torch.Tensor | None = None, A: torch.Tensor | None = None, leaky: float = 1.0,
                   want_scores: bool = False):
    """The target's rank among each row's candidates (sagnn_candidate_rank_f32): scores[b, j] = <U[uids[b]], I[c]> +
    <leaky(S[b]), A[c]> for c = cand[b, j], bit-identical to pair_score; rank[b] = #(scores above the best target
    copy) + #(earlier candidates tied with it), NaN read as -inf, -1 when the row holds no copy or target[b] < 0
    (Recommender.calcRes). uids / target int32 [B], cand int32 [B, C] with unit inner stride; ids are not checked.
    Returns (rank int64 [B], scores float32 [B, C] or None)."""
    d = int(U.shape[1])
    if cand.dim() != 2 or cand.dtype != torch.int32 or not cand.is_cuda or cand.stride(1) != 1:
        raise ValueError("cand: need an int32 device matrix [B, C] with unit inner stride")
    B, C = int(cand.shape[0]), int(cand.shape[1])
    ldc = cand.stride(0) if B > 1 else C
    cand_ptr = cand.data_ptr() if cand.numel() else _idx_ptr("cand", cand.new_zeros(0), torch.int32)
    dev = U.device
    rank = torch.empty(B, dtype=torch.int64, device=dev)
    scores = torch.empty((B, C), dtype=torch.float32, device=dev) if want_scores else None
    check(_lib.load().sagnn_candidate_rank_f32(
        U.data_ptr(), _f32_rows("U", U, d), I.data_ptr(), _f32_rows("I", I, d), _ptr(S),
        0 if S is None else _f32_rows("S", S, d, B), _ptr(A), 0 if A is None else _f32_rows("A", A, d),
        _idx_ptr("uids", uids, torch.int32, B), cand_ptr, ldc,
        _idx_ptr("target", target, torch.int32, B), float(leaky), B, C, d, _idx_ptr("rank", rank, torch.int64),
        _ptr(scores), C, _stream()))
    return rank, scores


# ---- device sampling of the training batch (sampler.hip) ---------------------------------------------------------
_empty_ptrs: dict = {}   # device -> a 16-byte buffer standing in for empty tensors (an empty tensor's data_ptr is 0)


def _empty_ptr(device) -> int:
    buf = _empty_ptrs.get(device)
    if buf is None:
        buf = _empty_ptrs[device] = torch.zeros(4, dtype=torch.int32, device=device)
    return buf.data_ptr()


def _idx_ptr(name: str, t: torch.Tensor, dtype, numel: int | None = None) -> int:
    """data_ptr of a contiguous index tensor on the device, checked; a valid pointer also for an empty one."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous {dtype} device tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")
    return t.data_ptr() if t.numel() else _empty_ptr(t.device)


def _out(n: int, dtype, device) -> torch.Tensor:
    return torch.empty(max(int(n), 1), dtype=dtype, device=device)[:int(n)]


def sample_train(bat_ids: torch.Tensor, n_slots: int, seq_ptr: torch.Tensor, seq_items: torch.Tensor,
                 ban_ptr: torch.Tensor, ban_items: torch.Tensor, n_items: int, train_sample_num: int, pred_num: int,
                 pos_length: int, pair_off: torch.Tensor, n_pairs: int, seed: int, step: int):
    """One training batch drawn on the device (sagnn_sample_train_i32). bat_ids int32 [B]; seq_ptr / ban_ptr int64
    [U + 1] into int32 seq_items / ban_items (banned rows sorted, unique); pair_off int64 [B]: where slot b's pairs
    start, n_pairs their total. Returns uids, iids, uLocs_seq (int32 [2 n_pairs], positives first) and the head's
    sequence segments seg_begin (int64 [n_slots]), seg_len (int32 [n_slots])."""
    B, U = int(bat_ids.numel()), int(seq_ptr.numel()) - 1
    dev = bat_ids.device
    uids, iids, locs = (_out(2 * n_pairs, torch.int32, dev) for _ in range(3))
    seg_begin, seg_len = _out(n_slots, torch.int64, dev), _out(n_slots, torch.int32, dev)
    check(_lib.load().sagnn_sample_train_i32(
        _idx_ptr("bat_ids", bat_ids, torch.int32), B, int(n_slots), _idx_ptr("seq_ptr", seq_ptr, torch.int64),
        _idx_ptr("seq_items", seq_items, torch.int32), _idx_ptr("ban_ptr", ban_ptr, torch.int64, U + 1),
        _idx_ptr("ban_items", ban_items, torch.int32), U, int(n_items), int(train_sample_num), int(pred_num),
        int(pos_length), _idx_ptr("pair_off", pair_off, torch.int64, B), int(n_pairs), int(seed), int(step),
        _idx_ptr("uids", uids, torch.int32), _idx_ptr("iids", iids, torch.int32), _idx_ptr("uLocs_seq", locs, torch.int32),
        _idx_ptr("seg_begin", seg_begin, torch.int64), _idx_ptr("seg_len", seg_len, torch.int32), _stream()))
    return uids, iids, locs, seg_begin, seg_len


def sample_ssl(bat_ids: torch.Tensor, sub_ptr: torch.Tensor, sub_items: torch.Tensor, ssl_num: int,
               ssl_off: torch.Tensor, n_out: int, seed: int, step: int):
    """The SSL pairs of every interval in one launch (sagnn_sample_ssl_i32). sub_ptr int64 [T, U + 1] into int32
    sub_items (distinct items per row); ssl_off int64 [T, B]: where slot b's pairs of interval k start in the
    concatenated outputs of n_out entries. Returns uids, iids, uLocs_seq (int32 [n_out], pairs interleaved)."""
    T, B = int(sub_ptr.shape[0]), int(bat_ids.numel())
    U = int(sub_ptr.shape[1]) - 1
    dev = bat_ids.device
    uids, iids, locs = (_out(n_out, torch.int32, dev) for _ in range(3))
    check(_lib.load().sagnn_sample_ssl_i32(
        _idx_ptr("bat_ids", bat_ids, torch.int32), B, T, _idx_ptr("sub_ptr", sub_ptr, torch.int64),
        _idx_ptr("sub_items", sub_items, torch.int32), U, int(ssl_num), _idx_ptr("ssl_off", ssl_off, torch.int64, T * B),
        int(n_out), int(seed), int(step), _idx_ptr("uids", uids, torch.int32), _idx_ptr("iids", iids, torch.int32),
        _idx_ptr("uLocs_seq", locs, torch.int32), _stream()))
    return uids, iids, locs


def seq_sum(fi: torch.Tensor, pos_embed: torch.Tensor, seq_items: torch.Tensor, seg_begin: torch.Tensor,
            seg_len: torch.Tensor):
    """The head's masked sums over sequence segments (sagnn_seq_sum_f32): seq_tok[b] = sum of fi over the
    segment's items, pos_tok[b] = sum of the last seg_len[b] rows of pos_embed. Returns two [n_slots, d] tensors."""
    d, P, n = int(fi.shape[1]), int(pos_embed.shape[0]), int(seg_len.numel())
    seq_tok = torch.empty((n, d), dtype=torch.float32, device=fi.device)
    pos_tok = torch.empty((n, d), dtype=torch.float32, device=fi.device)
    check(_lib.load().sagnn_seq_sum_f32(
        fi.data_ptr(), _f32_rows("fi", fi, d), int(fi.shape[0]), pos_embed.data_ptr(), _f32_rows("pos_embed", pos_embed, d),
        P, _idx_ptr("seq_items", seq_items, torch.int32), int(seq_items.numel()),
        _idx_ptr("seg_begin", seg_begin, torch.int64, n), _idx_ptr("seg_len", seg_len, torch.int32), n, d,
        seq_tok.data_ptr(), pos_tok.data_ptr(), d, _stream()))
    return seq_tok, pos_tok


def seq_sum_bwd(g_seq: torch.Tensor, g_pos: torch.Tensor, seq_items: torch.Tensor, seg_begin: torch.Tensor,
                seg_len: torch.Tensor, n_items: int, pos_length: int):
    """Gradients of seq_sum (sagnn_seq_sum_bwd_f32): d_fi [n_items, d] (a scatter with float atomics) and
    d_pos [pos_length, d] (deterministic). g_seq / g_pos: contiguous [n_slots, d]."""
    n, d = int(seg_len.numel()), int(g_seq.shape[1])
    ld = _f32_rows("g_seq", g_seq, d, n)
    if _f32_rows("g_pos", g_pos, d, n) != ld:
        raise ValueError("g_seq and g_pos need the same row stride")
    d_fi = torch.zeros((int(n_items), d), dtype=torch.float32, device=g_seq.device)
    d_pos = torch.empty((int(pos_length), d), dtype=torch.float32, device=g_seq.device)
    check(_lib.load().sagnn_seq_sum_bwd_f32(
        g_seq.data_ptr(), g_pos.data_ptr(), ld, _idx_ptr("seq_items", seq_items, torch.int32), int(seq_items.numel()),
        _idx_ptr("seg_begin", seg_begin, torch.int64, n), _idx_ptr("seg_len", seg_len, torch.int32), n, int(pos_length), d,
        d_fi.data_ptr(), d, int(n_items), d_pos.data_ptr(), d, _stream()))
    return d_fi, d_pos


# ---- row subsets of the interval fusion (fusion_rows.hip) ---------------------------------------------------------
def _flags(name: str, flags: torch.Tensor) -> int:
    if flags.dtype != torch.uint8 or not flags.is_cuda or not flags.is_contiguous() or flags.dim() != 1:
        raise TypeError(f"{name}: expected a contiguous uint8 device vector")
    return flags.data_ptr() if flags.numel() else _idx_ptr(name, flags.new_zeros(0, dtype=torch.int32), torch.int32)


def rows_mark(ids: torch.Tensor, flags: torch.Tensor):
    """flags[ids[i]] = 1 for every id in [0, len(flags)) (sagnn_rows_mark_i32); ids int32 on the device."""
    check(_lib.load().sagnn_rows_mark_i32(_idx_ptr("ids", ids, torch.int32), int(ids.numel()), int(flags.numel()),
                                          _flags("flags", flags), _stream()))


def rows_mark_segments(seq_items: torch.Tensor, seg_begin: torch.Tensor, seg_len: torch.Tensor, max_len: int,
                       flags: torch.Tensor):
    """Marks the items of the device sampler's sequence segments, j < min(seg_len[b], max_len) (sagnn_rows_mark_seg_i32)."""
    n = int(seg_len.numel())
    check(_lib.load().sagnn_rows_mark_seg_i32(
        _idx_ptr("seq_items", seq_items, torch.int32), int(seq_items.numel()), _idx_ptr("seg_begin", seg_begin, torch.int64, n),
        _idx_ptr("seg_len", seg_len, torch.int32), n, int(max_len), int(flags.numel()), _flags("flags", flags), _stream()))


def rows_compact(flags: torch.Tensor, cap: int, rows: torch.Tensor | None = None, count: torch.Tensor | None = None):
    """The flagged rows in ascending order (sagnn_rows_compact_i32), clearing the flags. Returns rows int32 [cap] (slots
    past the count hold row 0) and count int32 [1] on the device: the count never goes through the host here."""
    n, dev = int(flags.numel()), flags.device
    if rows is None:
        rows = _out(cap, torch.int32, dev)
    if count is None:
        count = torch.empty(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = int(lib.sagnn_rows_compact_workspace_bytes(n))
    ws = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
    check(lib.sagnn_rows_compact_i32(_flags("flags", flags), n, _idx_ptr("rows", rows, torch.int32, int(cap)), int(cap),
                                     _idx_ptr("count", count, torch.int32, 1), ws.data_ptr(), ws.numel() * 4, _stream()))
    return rows, count


def rows_gather(x: torch.Tensor, rows: torch.Tensor, count: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """out[j] = x[rows[j]] for x [N, t, d] (any node / interval strides) or [N, d] (sagnn_rows_gather_f32); out is dense
    [cap, t, d] / [cap, d] with cap = len(rows). With count (int32 [1] on the device) slots j >= count are zeros."""
    flat = x.dim() == 2
    xv = x.unsqueeze(1) if flat else x
    N, t, d, ld_n, ld_t = _ntd("x", xv)
    cap = int(rows.numel())
    if out is None:
        out = torch.empty((cap, d) if flat else (cap, t, d), dtype=torch.float32, device=x.device)
    if not out.is_contiguous() or out.numel() != cap * t * d:
        raise ValueError("out: expected a contiguous tensor of cap * t * d elements")
    if cap == 0:
        return out
    check(_lib.load().sagnn_rows_gather_f32(
        x.data_ptr(), ld_n, ld_t, N, t, d, _idx_ptr("rows", rows, torch.int32), cap,
        None if count is None else _idx_ptr("count", count, torch.int32, 1), out.data_ptr(), _stream()))
    return out


def rows_scatter(src: torch.Tensor, rows: torch.Tensor, count: torch.Tensor, out: torch.Tensor):
    """out[rows[j]] = src[j] for j < count (sagnn_rows_scatter_f32): src dense [cap, t, d] / [cap, d], out [N, t, d]
    (any node / interval strides) or [N, d]. No other row of out is written."""
    flat = out.dim() == 2
    ov = out.unsqueeze(1) if flat else out
    N, t, d, ld_n, ld_t = _ntd("out", ov)
    cap = int(rows.numel())
    if not src.is_contiguous() or src.dtype != torch.float32 or src.numel() != cap * t * d:
        raise ValueError("src: expected a contiguous float32 tensor of cap * t * d elements")
    if cap == 0:
        return out
    check(_lib.load().sagnn_rows_scatter_f32(
        src.data_ptr(), _idx_ptr("rows", rows, torch.int32), cap, _idx_ptr("count", count, torch.int32, 1), t, d,
        out.data_ptr(), ld_n, ld_t, N, _stream()))
    return out


# ---- self-attention over the item sequence (seq_attn.hip; --seqAtt full) ------------------------------------------
def seq_attn_supported(d: int, heads: int, pos_length: int) -> str | None:
    """None when sagnn_seq_attn_f32 / _bwd_f32 take the shape (sagnn_seq_attn_supported), else the library's reason."""
    return None if _lib.load().sagnn_seq_attn_supported(int(d), int(heads), int(pos_length)) == 0 else _lib.last_error()


def _seq_tokens(seq_items, seq_pos, seg_begin, seg_len):
    """The checked pointers of a slab's token description: (items, n_flat, positions or None, seg_begin, seg_len, n_slots)."""
    n = int(seg_len.numel())
    n_flat = int(seq_items.numel())
    return (_idx_ptr("seq_items", seq_items, torch.int32), n_flat,
            None if seq_pos is None else _idx_ptr("seq_pos", seq_pos, torch.int32, n_flat),
            _idx_ptr("seg_begin", seg_begin, torch.int64, n), _idx_ptr("seg_len", seg_len, torch.int32), n)


def seq_gather(fi: torch.Tensor, pos_embed: torch.Tensor, seq_items: torch.Tensor, seq_pos: torch.Tensor | None,
               seg_begin: torch.Tensor, seg_len: torch.Tensor):
    """The token slabs of the sequence attention (sagnn_seq_gather_f32): two [n_slots * P, d] tensors, P =
    len(pos_embed); row b * P + j holds fi[item] / pos_embed[position] of slot b's token j, zeros in the padding.
    seq_pos None: right-aligned positions P - n_b + j."""
    d, P = int(fi.shape[1]), int(pos_embed.shape[0])
    items, n_flat, pos, beg, ln, n = _seq_tokens(seq_items, seq_pos, seg_begin, seg_len)
    seq_slab = torch.empty((n * P, d), dtype=torch.float32, device=fi.device)
    pos_slab = torch.empty((n * P, d), dtype=torch.float32, device=fi.device)
    check(_lib.load().sagnn_seq_gather_f32(
        fi.data_ptr(), _f32_rows("fi", fi, d), int(fi.shape[0]), pos_embed.data_ptr(), _f32_rows("pos_embed", pos_embed, d),
        P, items, n_flat, pos, beg, ln, n, d, seq_slab.data_ptr(), pos_slab.data_ptr(), d, _stream()))
    return seq_slab, pos_slab


def seq_gather_bwd(g_seq: torch.Tensor, g_pos: torch.Tensor, seq_items: torch.Tensor, seq_pos: torch.Tensor | None,
                   seg_begin: torch.Tensor, seg_len: torch.Tensor, n_items: int, pos_length: int):
    """Gradients of seq_gather (sagnn_seq_gather_bwd_f32): d_fi [n_items, d] (a scatter with float atomics) and d_pos
    [pos_length, d] (deterministic). g_seq / g_pos: [n_slots * pos_length, d] with one row stride."""
    items, n_flat, pos, beg, ln, n = _seq_tokens(seq_items, seq_pos, seg_begin, seg_len)
    P, d = int(pos_length), int(g_seq.shape[1])
    ld = _f32_rows("g_seq", g_seq, d, n * P)
    if _f32_rows("g_pos", g_pos, d, n * P) != ld:
        raise ValueError("g_seq and g_pos need the same row stride")
    d_fi = torch.zeros((int(n_items), d), dtype=torch.float32, device=g_seq.device)
    d_pos = torch.empty((P, d), dtype=torch.float32, device=g_seq.device)
    check(_lib.load().sagnn_seq_gather_bwd_f32(g_seq.data_ptr(), g_pos.data_ptr(), ld, items, n_flat, pos, beg, ln, n, P, d,
                                               d_fi.data_ptr(), d, int(n_items), d_pos.data_ptr(), d, _stream()))
    return d_fi, d_pos


def _slab_rows(name: str, t: torch.Tensor, cols: int, rows: int) -> int:
    if _f32_rows(name, t, cols, rows) != cols:
        raise ValueError(f"{name}: expected a contiguous [{rows}, {cols}] tensor")
    return t.data_ptr()


def _causal_flag(causal) -> int:
    if causal not in (False, True, 0, 1):
        raise ValueError(f"causal = {causal!r}: need a bool")
    return int(causal)


def seq_attn(qkv: torch.Tensor, seg_len: torch.Tensor, pos_length: int, heads: int, causal: bool = False):
    """The ragged attention over each slot's real tokens (sagnn_seq_attn_f32): qkv [n_slots * P, 3d] contiguous ->
    ctx [n_slots * P, d], zero rows in the padding. causal=True (sagnn_seq_attn_masked_f32, --seqAtt causal): token j
    attends to tokens 0..j of its slot only."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(qkv.shape[1]) // 3
    ctx = torch.empty((n * P, d), dtype=torch.float32, device=qkv.device)
    if _causal_flag(causal):
        check(_lib.load().sagnn_seq_attn_masked_f32(_slab_rows("qkv", qkv, 3 * d, n * P),
                                                    _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, int(heads), 1,
                                                    ctx.data_ptr(), _stream()))
        return ctx
    check(_lib.load().sagnn_seq_attn_f32(_slab_rows("qkv", qkv, 3 * d, n * P), _idx_ptr("seg_len", seg_len, torch.int32), n, P,
                                         d, int(heads), ctx.data_ptr(), _stream()))
    return ctx


def seq_attn_bwd(qkv: torch.Tensor, g_ctx: torch.Tensor, seg_len: torch.Tensor, pos_length: int, heads: int,
                 causal: bool = False):
    """(qkv, g_ctx [n_slots * P, d]) -> dqkv [n_slots * P, 3d] (sagnn_seq_attn_bwd_f32; causal=True:
    sagnn_seq_attn_masked_bwd_f32): zero rows in the padding, bit-identical between runs."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(qkv.shape[1]) // 3
    dqkv = torch.empty((n * P, 3 * d), dtype=torch.float32, device=qkv.device)
    if _causal_flag(causal):
        check(_lib.load().sagnn_seq_attn_masked_bwd_f32(_slab_rows("qkv", qkv, 3 * d, n * P),
                                                        _slab_rows("g_ctx", g_ctx, d, n * P),
                                                        _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, int(heads), 1,
                                                        dqkv.data_ptr(), _stream()))
        return dqkv
    check(_lib.load().sagnn_seq_attn_bwd_f32(_slab_rows("qkv", qkv, 3 * d, n * P), _slab_rows("g_ctx", g_ctx, d, n * P),
                                             _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, int(heads), dqkv.data_ptr(),
                                             _stream()))
    return dqkv


def seq_attn_wide_supported(d: int, heads: int, pos_length: int) -> str | None:
    """None when sagnn_seq_attn_wide_f32 / _bwd_f32 take the shape (d / heads in {16, 32, 64}; --seqHeads), else the
    library's reason."""
    return None if _lib.load().sagnn_seq_attn_wide_supported(int(d), int(heads), int(pos_length)) == 0 else _lib.last_error()


def seq_attn_wide(qkv: torch.Tensor, seg_len: torch.Tensor, pos_length: int, heads: int, causal: bool = False):
    """seq_attn at head widths 16, 32 and 64, on the fp32 matrix cores (sagnn_seq_attn_wide_f32): the same contract."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(qkv.shape[1]) // 3
    ctx = torch.empty((n * P, d), dtype=torch.float32, device=qkv.device)
    check(_lib.load().sagnn_seq_attn_wide_f32(_slab_rows("qkv", qkv, 3 * d, n * P), _idx_ptr("seg_len", seg_len, torch.int32),
                                              n, P, d, int(heads), _causal_flag(causal), ctx.data_ptr(), _stream()))
    return ctx


def seq_attn_wide_bwd(qkv: torch.Tensor, g_ctx: torch.Tensor, seg_len: torch.Tensor, pos_length: int, heads: int,
                      causal: bool = False):
    """seq_attn_bwd at head widths 16, 32 and 64 (sagnn_seq_attn_wide_bwd_f32): zero rows in the padding, bit-identical
    between runs."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(qkv.shape[1]) // 3
    dqkv = torch.empty((n * P, 3 * d), dtype=torch.float32, device=qkv.device)
    check(_lib.load().sagnn_seq_attn_wide_bwd_f32(_slab_rows("qkv", qkv, 3 * d, n * P), _slab_rows("g_ctx", g_ctx, d, n * P),
                                                  _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, int(heads),
                                                  _causal_flag(causal), dqkv.data_ptr(), _stream()))
    return dqkv


# ---- position-wise feed-forward block of the sequence head (seq_ffn.hip; --seqFFN) ---------------------------------
def seq_ffn_supported(d: int, f: int, pos_length: int) -> str | None:
    """None when sagnn_seq_ffn_f32 / _bwd_f32 take the shape (d in {32, 64, 128}, f a multiple of 16 in [16, 256],
    d * f <= 16384, 1 <= pos_length <= 256), else the library's reason."""
    return None if _lib.load().sagnn_seq_ffn_supported(int(d), int(f), int(pos_length)) == 0 else _lib.last_error()


def _seq_ffn_args(x, gamma, beta, W1, b1, W2, b2, seg_len, pos_length, leaky, eps):
    """The checked sagnn_seq_ffn_args of a call, with (n_slots, P, d, f)."""
    n, P = int(seg_len.numel()), int(pos_length)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("x: expected a [n_slots * pos_length, d] tensor")
    d = int(x.shape[1])
    if not isinstance(W1, torch.Tensor) or W1.dim() != 2 or int(W1.shape[0]) != d:
        raise ValueError(f"W1: expected a [{d}, f] tensor")
    f = int(W1.shape[1])
    ldx = _f32_rows("x", x, d, n * P)
    _one_device(x, gamma=gamma, beta=beta, W1=W1, b1=b1, W2=W2, b2=b2, seg_len=seg_len)
    args = _lib.SeqFfnArgs(_ptr_or_empty(x), ldx, _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, f, _vec("gamma", gamma, d),
                           _vec("beta", beta, d), float(eps), _vec("W1", W1, d * f), _vec("b1", b1, f), _vec("W2", W2, f * d),
                           _vec("b2", b2, d), float(leaky))
    if tuple(W2.shape) != (f, d):
        raise ValueError(f"W2: expected shape [{f}, {d}], got {tuple(W2.shape)}")
    return args, n, P, d, f


def seq_ffn(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor,
            b2: torch.Tensor, seg_len: torch.Tensor, pos_length: int, leaky: float, eps: float = 1e-12):
    """out = x + act(LN(x) W1 + b1) W2 + b2 on every real token row of the slab x [n_slots * P, d], exact zeros in the
    padding (sagnn_seq_ffn_f32); act(a) = leaky * a where leaky * a >= a, else a. W1 [d, f], W2 [f, d]."""
    args, n, P, d, _ = _seq_ffn_args(x, gamma, beta, W1, b1, W2, b2, seg_len, pos_length, leaky, eps)
    out = torch.empty((n * P, d), dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_seq_ffn_f32(ctypes.byref(args), _ptr_or_empty(out), d, _stream()))
    return out


def seq_ffn_bwd(x: torch.Tensor, g: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor,
                W2: torch.Tensor, b2: torch.Tensor, seg_len: torch.Tensor, pos_length: int, leaky: float, eps: float = 1e-12):
    """Gradients of seq_ffn (sagnn_seq_ffn_bwd_f32): (dx [n_slots * P, d] with zero rows in the padding, dgamma, dbeta,
    dW1, db1, dW2, db2), all written; no atomics, bit-identical between runs. Padded rows of x and g are not read."""
    args, n, P, d, f = _seq_ffn_args(x, gamma, beta, W1, b1, W2, b2, seg_len, pos_length, leaky, eps)
    ldg = _f32_rows("g", g, d, n * P)
    _one_device(x, g=g)
    dev = x.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    dx, dgamma, dbeta, dW1, db1, dW2, db2 = new(n * P, d), new(d), new(d), new(d, f), new(f), new(f, d), new(d)
    need = int(_lib.load().sagnn_seq_ffn_bwd_workspace_bytes(n, P, d, f))
    if need == 0:
        raise _lib.SagnnError(-2, _lib.last_error())
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    check(_lib.load().sagnn_seq_ffn_bwd_f32(ctypes.byref(args), _ptr_or_empty(g), ldg, _ptr_or_empty(dx), d, dgamma.data_ptr(),
                                            dbeta.data_ptr(), dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), db2.data_ptr(),
                                            ws.data_ptr(), need, _stream()))
    return dx, dgamma, dbeta, dW1, db1, dW2, db2


def seq_pool(x: torch.Tensor, seg_len: torch.Tensor, pos_length: int):
    """out[b] = the sum of slot b's real token rows of x [n_slots * P, d] (sagnn_seq_pool_f32) -> [n_slots, d]."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(x.shape[1])
    out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_seq_pool_f32(x.data_ptr(), _f32_rows("x", x, d, n * P), _idx_ptr("seg_len", seg_len, torch.int32),
                                         n, P, d, out.data_ptr(), d, _stream()))
    return out


def seq_pool_bwd(g: torch.Tensor, seg_len: torch.Tensor, pos_length: int):
    """dx[b * P + j] = g[b] for slot b's real tokens, zeros in the padding (sagnn_seq_pool_bwd_f32) -> [n_slots * P, d]."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(g.shape[1])
    dx = torch.empty((n * P, d), dtype=torch.float32, device=g.device)
    check(_lib.load().sagnn_seq_pool_bwd_f32(g.data_ptr(), _f32_rows("g", g, d, n), _idx_ptr("seg_len", seg_len, torch.int32),
                                             n, P, d, dx.data_ptr(), d, _stream()))
    return dx


# ---- a query per prefix of the sequence (seq_attn.hip; --seqTargets all) ------------------------------------------
def seq_prefix_query(x: torch.Tensor, U: torch.Tensor, seg_len: torch.Tensor, pos_length: int, leaky: float):
    """Q[b * P + j] = max(leaky * pre, pre) + U[b], pre = the sum of slot b's token rows 0..j of x [n_slots * P, d]
    (sagnn_seq_prefix_query_f32) -> [n_slots * P, d], zero rows in the padding. U [n_slots, d]. The slot's last real row
    has the bits of leaky_add(seq_pool(x), U, leaky)."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(x.shape[1])
    _one_device(x, U=U, seg_len=seg_len)
    Q = torch.empty((n * P, d), dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_seq_prefix_query_f32(x.data_ptr(), _f32_rows("x", x, d, n * P),
                                                 _idx_ptr("seg_len", seg_len, torch.int32), U.data_ptr(),
                                                 _f32_rows("U", U, d, n), n, P, d, float(leaky), Q.data_ptr(), d, _stream()))
    return Q


def seq_prefix_query_bwd(x: torch.Tensor, dQ: torch.Tensor, seg_len: torch.Tensor, pos_length: int, leaky: float):
    """Gradients of seq_prefix_query (sagnn_seq_prefix_query_bwd_f32): (dx [n_slots * P, d] with zero rows in the padding,
    dU [n_slots, d]); no atomics, bit-identical between runs."""
    n, P, d = int(seg_len.numel()), int(pos_length), int(x.shape[1])
    _one_device(x, dQ=dQ, seg_len=seg_len)
    dx = torch.empty((n * P, d), dtype=torch.float32, device=x.device)
    dU = torch.empty((n, d), dtype=torch.float32, device=x.device)
    check(_lib.load().sagnn_seq_prefix_query_bwd_f32(x.data_ptr(), _f32_rows("x", x, d, n * P),
                                                     _idx_ptr("seg_len", seg_len, torch.int32), dQ.data_ptr(),
                                                     _f32_rows("dQ", dQ, d, n * P), n, P, d, float(leaky), dx.data_ptr(), d,
                                                     dU.data_ptr(), d, _stream()))
    return dx, dU


def seq_targets(seq_items: torch.Tensor, seg_begin: torch.Tensor, seg_len: torch.Tensor, slot_user: torch.Tensor,
                slot_target: torch.Tensor, pos_length: int, n_items: int):
    """The next-item target of every slab row (sagnn_seq_targets_i32): target[b * P + j] = the item after token j of slot
    b, slot_target[b] after its last token, -1 in the padding, in a slot with slot_target[b] < 0 and for an id outside
    [0, n_items); excl_row[b * P + j] = slot_user[b]. All int32 device tensors; returns (target, excl_row), [n_slots * P]."""
    n, P = int(seg_len.numel()), int(pos_length)
    items, n_flat, _, beg, ln, _ = _seq_tokens(seq_items, None, seg_begin, seg_len)
    _one_device(seq_items, seg_begin=seg_begin, seg_len=seg_len, slot_user=slot_user, slot_target=slot_target)
    target, excl_row = _out(n * P, torch.int32, seg_len.device), _out(n * P, torch.int32, seg_len.device)
    check(_lib.load().sagnn_seq_targets_i32(items, n_flat, beg, ln, _idx_ptr("slot_user", slot_user, torch.int32, n),
                                            _idx_ptr("slot_target", slot_target, torch.int32, n), n, P, int(n_items),
                                            target.data_ptr(), excl_row.data_ptr(), _stream()))
    return target, excl_row


# ---- additive-attention pooling of the sequence head (seq_attn.hip; --seqPool additive) ----------------------------
def seq_addpool_supported(d: int, q: int, pos_length: int) -> str | None:
    """None when sagnn_seq_addpool_f32 / _bwd_f32 take the shape (sagnn_seq_addpool_supported), else the library's reason."""
    return None if _lib.load().sagnn_seq_addpool_supported(int(d), int(q), int(pos_length)) == 0 else _lib.last_error()


def seq_addpool(x: torch.Tensor, u: torch.Tensor, v: torch.Tensor, seg_len: torch.Tensor, pos_length: int,
                want_weights: bool = False):
    """out[b] = sum_j w_j x[b * P + j], w the softmax over slot b's real tokens of <tanh(u[b * P + j]), v>
    (sagnn_seq_addpool_f32): x [n_slots * P, d], u [n_slots * P, q], v [q] -> [n_slots, d]; with want_weights also
    w [n_slots * P] (zeros in the padding)."""
    n, P, d, q = int(seg_len.numel()), int(pos_length), int(x.shape[1]), int(u.shape[1])
    out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    w = torch.empty(n * P, dtype=torch.float32, device=x.device) if want_weights else None
    check(_lib.load().sagnn_seq_addpool_f32(_ptr_or_empty(x), _f32_rows("x", x, d, n * P), _ptr_or_empty(u), _f32_rows("u", u, q, n * P),
                                            _vec("v", v, q), _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, q,
                                            _ptr_or_empty(out), d, None if w is None else _ptr_or_empty(w), _stream()))
    return (out, w) if want_weights else out


def seq_addpool_bwd(x: torch.Tensor, u: torch.Tensor, v: torch.Tensor, g: torch.Tensor, seg_len: torch.Tensor,
                    pos_length: int):
    """(x, u, v, g [n_slots, d]) -> (dx [n_slots * P, d], the direct part w_j g; du [n_slots * P, q]; dv [q])
    (sagnn_seq_addpool_bwd_f32): zeros in the padding, bit-identical between runs."""
    n, P, d, q = int(seg_len.numel()), int(pos_length), int(x.shape[1]), int(u.shape[1])
    dev = x.device
    dx = torch.empty((n * P, d), dtype=torch.float32, device=dev)
    du = torch.empty((n * P, q), dtype=torch.float32, device=dev)
    dv_part = torch.empty((max(n, 1), q), dtype=torch.float32, device=dev)
    dv = torch.empty(q, dtype=torch.float32, device=dev)
    check(_lib.load().sagnn_seq_addpool_bwd_f32(
        _ptr_or_empty(x), _f32_rows("x", x, d, n * P), _ptr_or_empty(u), _f32_rows("u", u, q, n * P), _vec("v", v, q),
        _ptr_or_empty(g), _f32_rows("g", g, d, n), _idx_ptr("seg_len", seg_len, torch.int32), n, P, d, q, _ptr_or_empty(dx), d,
        _ptr_or_empty(du), q,
        dv_part.data_ptr(), dv.data_ptr(), _stream()))
    return dx, du, dv
