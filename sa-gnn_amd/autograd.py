"""torch.autograd bindings for the hot path (reference: the gradients tf.train.AdamOptimizer
.minimize builds for model.py:118-129, model.py:250). Forward and backward both run in
libsagnn.so, through the checked wrappers of ops.py (the only caller of the library); torch only
carries the graph."""
from __future__ import annotations

import torch

from . import ops

# Host-side A/B switches (tests flip them): False routes the backward through the per-step / per-product entries
# that the fused entries (attention-backward front + tail, one-launch BPTT) replaced.
FUSED_ATTN_BWD = True
FUSED_BPTT = True
DEFERRED_DW_LIMIT = 32 << 30   # bytes of gate gradients ([t, n, 4d]) a BPTT may keep for the separate weight-gradient pass
SPLIT_DW = True                # one-launch BPTT (d = 32 / 64): weight gradient as a second pass on the f16 x 2 engine ...
# Feature widths the fusion's backward runs at: multiples of 32 (the dense products) with 64 % d == 0 or d % 64 == 0
# (ops.attn_bwd, ops.layernorm_td_bwd). The forward alone also runs at d = 96, 160, 224.
TRAINABLE_D = (32, 64, 128, 192, 256)
SPLIT_DW_MIN_T = 4              # ... from this many steps on (measured: T = 16 -13 %, T = 6 -8 %, T = 2 / 3 nothing: the gate gradients' HBM round trip)


class GnnStackFn(torch.autograd.Function):
    """(uEmbed [T, U, d], iEmbed [T, I, d]) -> (user slab [T, U, d], item slab [T, I, d]): the whole loop of
    model.py:118-129 as ONE autograd node. Interval outputs are written straight into the slabs the fusion reads
    as [N, T, d] views (no torch.stack copy). With an ops.SpmmBatch the loop over k happens INSIDE the launches
    (one per layer, ops.gnn_stack / gnn_stack_bwd); with plan lists every interval takes its own 2 L launches
    (ops.gnn_interval: graphs whose T-fold scratch would not fit).
    TE: None, or the time-aware messages of DESIGN.md §20 as one more input [T, L, 2, M, d] — TE[k, l, dir] is added, row
    bucket[e], to what edge e of product (interval k, layer l, direction dir) gathers — with its gradient dTE. The
    gradients into the embeddings are the same either way: the adjoint chain does not see the time term. The plans carry
    the buckets (ops.SpmmPlan(buckets=)); not with `drop`."""

    @staticmethod
    def forward(ctx, u_embed, i_embed, plans_user, plans_item, n_layers, leaky, drop=None, TE=None):
        T, U, d = u_embed.shape
        I = i_embed.shape[1]
        dev = u_embed.device
        ue, ie = (x if x.stride(2) == 1 else x.contiguous() for x in (u_embed.detach(), i_embed.detach()))
        te = None if TE is None else TE.detach().contiguous()
        out_u = torch.empty((T, U, d), dtype=torch.float32, device=dev)
        out_i = torch.empty((T, I, d), dtype=torch.float32, device=dev)
        mask_u = torch.empty((T, n_layers, U, d // 4), dtype=torch.uint8, device=dev)
        mask_i = torch.empty((T, n_layers, I, d // 4), dtype=torch.uint8, device=dev)
        if isinstance(plans_user, ops.SpmmBatch):
            ops.gnn_stack(plans_user, ue, ie, n_layers, leaky, out_u, out_i, mask_u=mask_u, mask_i=mask_i, drop=drop, time=te)
        else:
            scr_u = torch.empty((2, U, d), dtype=torch.float32, device=dev) if n_layers > 1 else None
            scr_i = torch.empty((2, I, d), dtype=torch.float32, device=dev) if n_layers > 1 else None
            for k in range(T):
                ops.gnn_interval(plans_user[k], plans_item[k], ue[k], ie[k], n_layers, leaky, out_u[k], out_i[k], scr_u, scr_i,
                                 mask_u=mask_u[k], mask_i=mask_i[k], drop=drop, interval=k, time=None if te is None else te[k])
        ctx.save_for_backward(mask_u, mask_i, *(() if te is None else (te,)))
        ctx.plans = (plans_user, plans_item)
        ctx.drop = drop       # the backward drops the edges the forward dropped: the same ops.EdgeDrop
        ctx.cfg = (n_layers, leaky)
        return out_u, out_i

    @staticmethod
    def backward(ctx, g_user, g_item):
        mask_u, mask_i, *te = ctx.saved_tensors
        te = te[0] if te else None
        plans_user, plans_item = ctx.plans
        n_layers, leaky = ctx.cfg
        T, _, U, dq = mask_u.shape
        I, d, dev = mask_i.shape[2], dq * 4, mask_u.device
        if g_user is None:
            g_user = torch.zeros((T, U, d), dtype=torch.float32, device=dev)
        if g_item is None:
            g_item = torch.zeros((T, I, d), dtype=torch.float32, device=dev)
        if g_user.stride(2) != 1:
            g_user = g_user.contiguous()
        if g_item.stride(2) != 1:
            g_item = g_item.contiguous()
        du = torch.empty((T, U, d), dtype=torch.float32, device=dev)
        di = torch.empty((T, I, d), dtype=torch.float32, device=dev)
        dte = None if te is None else torch.empty_like(te)
        if isinstance(plans_user, ops.SpmmBatch):
            ops.gnn_stack_bwd(plans_user, g_user, g_item, n_layers, leaky, mask_u, mask_i, du, di, drop=ctx.drop, time=te,
                              grad_time=dte)
            return du, di, None, None, None, None, None, dte
        scr_u = torch.empty((4, U, d), dtype=torch.float32, device=dev)
        scr_i = torch.empty((4, I, d), dtype=torch.float32, device=dev)
        for k in range(T):
            ops.gnn_interval_bwd(plans_user[k], plans_item[k], g_user[k], g_item[k], n_layers, leaky, mask_u[k], mask_i[k],
                                 grad_u0=du[k], grad_i0=di[k], scratch_u=scr_u, scratch_i=scr_i, drop=ctx.drop, interval=k,
                                 time=None if te is None else te[k], grad_time=None if te is None else dte[k])
        return du, di, None, None, None, None, None, dte


def gnn_stack(u_embed, i_embed, plans_user, plans_item, n_layers: int, leaky: float, drop=None, TE=None):
    """plans_user: a list of T ops.SpmmPlan (with plans_item the matching list) or an ops.SpmmBatch (plans_item None).
    drop: an ops.EdgeDrop for edge dropout in the forward and, identically, in the backward; None = no dropout.
    TE: None (the node without time), or the time tables [T, L, 2, M, d] in the registration order of their weights
    (k, l, user call, item call); the node then also returns dTE. Not with `drop`."""
    if TE is not None and drop is not None:
        raise ValueError("edge dropout and time-aware messages do not combine (--edgeKeepRate < 1 with --edgeTime slot)")
    return GnnStackFn.apply(u_embed, i_embed, plans_user, plans_item, n_layers, leaky, drop, TE)


def gnn_interval(u0, i0, plan_user, plan_item, n_layers: int, leaky: float):
    """(uEmbed[k], iEmbed[k]) -> (user_k, item_k): the stack of one interval, on its own plans."""
    user_out, item_out = gnn_stack(u0.unsqueeze(0), i0.unsqueeze(0), [plan_user], [plan_item], n_layers, leaky)
    return user_out[0], item_out[0]


def _check_trainable(x):
    """Refuses a width the backward has no kernels for BEFORE the forward runs (the library would return SAGNN_ERR_DIM
    halfway through the backward pass, after the LSTM and the attention forward have been paid for)."""
    d = int(x.shape[-1])
    if d not in TRAINABLE_D:
        raise ValueError(f"d = {d}: the interval fusion trains at d in {TRAINABLE_D} (inference: any multiple of 32 up to 256)")


def _split_qkv_grads(dWqkv, dbqkv, d):
    """[d, 3d] / [3d] -> (dWq, dbq, dWk, dbk, dWv, dbv)."""
    out = ()
    for i in range(3):
        out += (dWqkv[:, i * d:(i + 1) * d].contiguous(), dbqkv[i * d:(i + 1) * d].contiguous())
    return out


_attn_bwd_front = ops.attn_bwd_front      # the fused front under the name it had while it lived in this file


def _attn_bwd_qkv(x, gamma, beta, Wqkv, Wq, bq, Wk, bk, Wv, bv, heads, g_out):
    """Recompute y = LN(x) (gamma None: y = x) and Q|K|V of x [n, t, d] dense, attention backward for g_out [n, d]
    contiguous -> (y [n*t, d], dQ|dK|dV [n*t, 3d]): the fused front where it covers the shape and FUSED_ATTN_BWD is
    set, otherwise [layernorm_td ->] dense_nn -> attn_bwd. Wqkv: [Wq | Wk | Wv], detached."""
    n, t, d = x.shape
    if ops.attn_bwd_front_supported(d, t, heads) and FUSED_ATTN_BWD:
        y, qkv = ops.attn_bwd_front(x, gamma, beta, *(w.detach() for w in (Wq, bq, Wk, bk, Wv, bv)), heads, g_out)
        return (x.view(n * t, d) if y is None else y), qkv
    y = x if gamma is None else ops.layernorm_td(x, gamma, beta)                     # [n, t, d]
    bqkv = torch.cat([bq, bk, bv]).detach().contiguous()
    y2 = y.view(n * t, d)
    qkv = ops.dense_nn(y2, Wqkv, bqkv)                                               # [n*t, 3d]
    return y2, ops.attn_bwd(qkv, g_out, n, t, heads)


def _qkv_grads(y2, dqkv, Wqkv, fused_tail: bool, in_place: bool):
    """The gradients behind Q|K|V = y W + b for y2 [rows, d] and dqkv [rows, 3d]: dW = y2^T dqkv, db = colsum dqkv and
    dy = dqkv W^T -> (dy [rows, d], dWqkv [d, 3d], dbqkv [3d]). fused_tail: all three in one pass over dqkv
    (ops.attn_bwd_tail, which writes dy over y2) instead of two products; in_place: dy reuses y2's storage (always
    with the fused tail), so y2 must be the caller's to overwrite."""
    d = y2.shape[1]
    dWqkv = torch.zeros((d, 3 * d), dtype=torch.float32, device=y2.device)
    dbqkv = torch.zeros(3 * d, dtype=torch.float32, device=y2.device)
    if fused_tail:
        assert in_place
        return ops.attn_bwd_tail(y2, dqkv, Wqkv, dWqkv, dbqkv), dWqkv, dbqkv
    ops.dense_tn(y2, dqkv, dWqkv, dbqkv)
    return ops.dense_nn(dqkv, Wqkv.t().contiguous(), None, out=y2 if in_place else None), dWqkv, dbqkv


def lstm_bwd(x, h, gates, cell, dh, drop, W):
    """Whole BPTT in one launch (ops.lstm_bwd, d in {32, 64}): x [n, t, d] (any strides), h / gates / cell as the
    training forward stored them, dh [n, t, d] dense = gradient at the emitted h -> (dx [n, t, d], dW [2d, 4d],
    db [4d]). Decides here whether the weight gradient is deferred to a second pass over the stored gate gradients
    (SPLIT_DW, from SPLIT_DW_MIN_T steps on, while they fit DEFERRED_DW_LIMIT)."""
    n, t, d = x.shape
    need = ops.lstm_bwd_workspace_bytes(n, t, d)
    return ops.lstm_bwd(x, h, gates, cell, dh, drop, W,
                        deferred_dw=SPLIT_DW and t >= SPLIT_DW_MIN_T and 0 < need <= DEFERRED_DW_LIMIT)


def _emit_and_attend(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale):
    """The stages behind the recurrent cell, shared by both cells: the DropoutWrapper scaling of the emitted h (h itself is
    stored un-dropped: it is also the recurrent operand of the backward pass), layer norm + attention + mean -> out [n, d]."""
    h_emit = h if drop_scale is None else ops.mul(h, drop_scale.contiguous())
    return ops.ln_mhsa_mean(h_emit, ln_gamma.detach(), ln_beta.detach(), Wq.detach(), bq.detach(), Wk.detach(),
                            bk.detach(), Wv.detach(), bv.detach(), heads)


def _fusion_forward(x, lstm_W, lstm_b, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale):
    """The training forward of the interval fusion on x [n, t, d] (any node/interval strides): returns
    (out [n, d], h, gates, cell), the last three as the backward reads them."""
    h, gates, cell = ops.lstm_fwd_train(x, lstm_W.detach(), lstm_b.detach())
    return _emit_and_attend(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale), h, gates, cell


def _fusion_forward_gru(x, gru, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale):
    """_fusion_forward under --rnnCell gru; gru = (Wg, bg, Wc, bc): returns (out [n, d], h, gates [n, t, 2d], cand)."""
    h, gates, cand = ops.gru_fwd_train(x, *(w.detach() for w in gru))
    return _emit_and_attend(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale), h, gates, cand


def _attention_backward(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, drop, heads, g_out):
    """The backward of _emit_and_attend for g_out [n, d], shared by both cells: returns (dh [n, t, d], the gradient at the
    EMITTED h, then dgamma, dbeta, dWqkv [d, 3d], dbqkv [3d])."""
    n, t, d = h.shape
    g_out = g_out.contiguous()
    # ---- recompute y and Q|K|V, attention backward -> dQ|dK|dV -----------------------------
    h_emit = h if drop is None else ops.mul(h, drop.contiguous())
    Wqkv = torch.cat([Wq, Wk, Wv], dim=1).detach().contiguous()                      # [d, 3d]
    y2, qkv = _attn_bwd_qkv(h_emit, ln_gamma.detach(), ln_beta.detach(), Wqkv, Wq, bq, Wk, bk, Wv, bv, heads, g_out)
    # y2 is this function's own recompute: dy goes over it, by the one-pass tail where that runs at d
    dy, dWqkv, dbqkv = _qkv_grads(y2, qkv, Wqkv, fused_tail=ops.attn_bwd_tail_supported(d) and FUSED_ATTN_BWD, in_place=True)
    # ---- layer norm backward (in place on dy) ----------------------------------------------
    dy = dy.view(n, t, d)
    dh, dgamma, dbeta = ops.layernorm_td_bwd(h_emit, dy, ln_gamma.detach(), out=dy)
    return dh, dgamma, dbeta, dWqkv, dbqkv


def _fusion_backward(x, lstm_W, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, h, gates, cell, drop, heads, g_out):
    """The backward of _fusion_forward for g_out [n, d]: returns (dx [n, t, d], then the gradients of lstm_W, lstm_b,
    ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv)."""
    n, t, d = x.shape
    dev = x.device
    dh, dgamma, dbeta, dWqkv, dbqkv = _attention_backward(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, drop, heads, g_out)
    # ---- BPTT ----------------------------------------------------------------------------------
    if ops.lstm_bwd_supported(d) and FUSED_BPTT:
        dx, dW, db = lstm_bwd(x, h, gates, cell, dh, drop, lstm_W.detach())
        return (dx, dW, db, dgamma, dbeta) + _split_qkv_grads(dWqkv, dbqkv, d)
    # generic BPTT (the widths of TRAINABLE_D beyond 32 / 64; d = 128 is BASELINE config 3). Per step: the element-wise gate
    # backward and ONE product d[x_t | h_{t-1}] = dG_t W^T written where the next step reads it. The gate gradients of
    # all steps stay in HBM ([t, n, 4d]) and the weight gradient is two segmented products after the loop instead of
    # 2 t small ones (each of those a split-K launch ending in 64 K float atomics per block).
    WT = lstm_W.detach().t().contiguous()                                            # [4d, 2d]
    dW = torch.zeros((2 * d, 4 * d), dtype=torch.float32, device=dev)
    db = torch.zeros(4 * d, dtype=torch.float32, device=dev)
    defer = n * t * 4 * d * 4 <= DEFERRED_DW_LIMIT
    dG = torch.empty((t if defer else 1, n, 4 * d), dtype=torch.float32, device=dev)
    dc = [torch.empty((n, d), dtype=torch.float32, device=dev) for _ in range(2)]
    dxh = torch.empty((n, t, 2 * d), dtype=torch.float32, device=dev)                # [dx_t | dh_{t-1}] per step
    for ts in range(t - 1, -1, -1):
        last = ts == t - 1
        dgates = dG[ts if defer else 0]
        ops.lstm_bwd_step(gates, cell, dh, drop, None if last else dxh[:, ts + 1, d:], None if last else dc[(ts + 1) & 1],
                          dgates, dc[ts & 1], ts)
        if not defer:
            ops.dense_tn(x[:, ts, :], dgates, dW[:d], db)
            if ts > 0:
                ops.dense_tn(h[:, ts - 1, :], dgates, dW[d:], None)                  # h un-dropped: the recurrent operand
        ops.dense_nn(dgates, WT, None, out=dxh[:, ts, :])
    if defer:
        ops.dense_tn_seg(x.permute(1, 0, 2), dG, dW[:d], db)
        if t > 1:
            ops.dense_tn_seg(h.permute(1, 0, 2)[:t - 1], dG[1:], dW[d:], None)
    return (dxh[:, :, :d].contiguous(), dW, db, dgamma, dbeta) + _split_qkv_grads(dWqkv, dbqkv, d)


def _fusion_backward_gru(x, Wg, Wc, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, h, gates, cand, drop, heads, g_out):
    """The backward of _fusion_forward_gru: returns (dx [n, t, d], then the gradients of Wg, bg, Wc, bc, ln_gamma, ln_beta,
    Wq, bq, Wk, bk, Wv, bv). The BPTT is the per-step loop at every width, shaped like the LSTM's generic
    one: per step two element-wise launches around [dx_s | d(r.h)] = da_c Wc^T and [dx_s | dh_{s-1}] += da_g Wg^T; the
    pre-activation gradients of all steps and r.h_{s-1} stay in HBM ([t, n, 4d] in all) and the weight gradients are four
    segmented products after the loop, or per-step products where that would pass DEFERRED_DW_LIMIT."""
    n, t, d = x.shape
    dev = x.device
    dh, dgamma, dbeta, dWqkv, dbqkv = _attention_backward(h, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, drop, heads, g_out)

    def new(*shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=dev)

    WgT, WcT = Wg.detach().t().contiguous(), Wc.detach().t().contiguous()            # [2d, 2d], [d, 2d]
    dWg, dbg, dWc, dbc = new(2 * d, 2 * d, zero=True), new(2 * d, zero=True), new(2 * d, d, zero=True), new(d, zero=True)
    defer = n * t * 4 * d * 4 <= DEFERRED_DW_LIMIT
    k = t if defer else 1
    dAg, dAc, RH = new(k, n, 2 * d), new(k, n, d), new(k, n, d)                      # da_g, da_c and r.h_{s-1} per step
    du, dhu = new(n, d), new(n, d)
    dxh = new(n, t, 2 * d)                                                           # [dx_s | dh_{s-1}] per step
    for ts in range(t - 1, -1, -1):
        j = ts if defer else 0
        ops.gru_bwd_cand(gates, cand, h, dh, drop, None if ts == t - 1 else dxh[:, ts + 1, d:], dAc[j], du, dhu, ts)
        ops.dense_nn(dAc[j], WcT, None, out=dxh[:, ts, :])                           # [dx_s | d(r.h)]
        ops.gru_bwd_gates(gates, h, du, dhu, dxh[:, ts, d:], dAg[j], RH[j], ts)      # d(r.h) -> dh_u + d(r.h) r
        ops.dense_nn(dAg[j], WgT, None, out=dxh[:, ts, :], accumulate=True)
        if not defer:
            ops.dense_tn(x[:, ts, :], dAg[j], dWg[:d], dbg)
            ops.dense_tn(x[:, ts, :], dAc[j], dWc[:d], dbc)
            if ts > 0:                                                               # h_{-1} = 0: no recurrent term at step 0
                ops.dense_tn(h[:, ts - 1, :], dAg[j], dWg[d:], None)
                ops.dense_tn(RH[j], dAc[j], dWc[d:], None)
    if defer:
        xt = x.permute(1, 0, 2)
        ops.dense_tn_seg(xt, dAg, dWg[:d], dbg)
        ops.dense_tn_seg(xt, dAc, dWc[:d], dbc)
        if t > 1:
            ops.dense_tn_seg(h.permute(1, 0, 2)[:t - 1], dAg[1:], dWg[d:], None)
            ops.dense_tn_seg(RH[1:], dAc[1:], dWc[d:], None)
    return (dxh[:, :, :d].contiguous(), dWg, dbg, dWc, dbc, dgamma, dbeta) + _split_qkv_grads(dWqkv, dbqkv, d)


def _cell_args(p: dict):
    """The cell's parameters as the fusion nodes take them, from a parameter dict as ops.interval_fusion reads it:
    (lstm_W, lstm_b) and no GRU tail, or (None, None) and the tail (gru_Wg, gru_bg, gru_Wc, gru_bc)."""
    if ops.fusion_cell(p) == "gru":
        return (None, None), (p["gru_Wg"], p["gru_bg"], p["gru_Wc"], p["gru_bc"])
    return (p["lstm_W"], p["lstm_b"]), ()


def _cell_forward(x, lstm_W, lstm_b, gru, attn, heads, drop_scale):
    """(out, h, gates, cell or cand) under whichever cell is given: gru = () or (Wg, bg, Wc, bc); attn = the eight
    layer-norm / attention parameters."""
    if gru:
        return _fusion_forward_gru(x, gru, *attn, heads, drop_scale)
    return _fusion_forward(x, lstm_W, lstm_b, *attn, heads, drop_scale)


def _cell_backward(x, cell_w, attn, h, gates, cell, drop, heads, g_out):
    """cell_w: (lstm_W,) or (Wg, Wc), as saved. Returns (dx, (dlstm_W, dlstm_b), (the GRU tail's four gradients or ()),
    the eight gradients of attn)."""
    if len(cell_w) == 2:
        grads = _fusion_backward_gru(x, *cell_w, *attn, h, gates, cell, drop, heads, g_out)
        return grads[0], (None, None), grads[1:5], grads[5:]
    grads = _fusion_backward(x, *cell_w, *attn, h, gates, cell, drop, heads, g_out)
    return grads[0], grads[1:3], (), grads[3:]


class IntervalFusionFn(torch.autograd.Function):
    """x [n, t, d] (any node/interval strides) + fusion parameters -> out [n, d]
    (reference model.py:135-155), differentiable in x and every parameter.

    Forward = LSTM (saving gate activations and cell states) + fused layer-norm/attention kernel.
    Backward recomputes y = LN(h) and Q|K|V with the forward kernels, then:
      attention backward (per node) -> dQ|dK|dV -> dW_qkv / db_qkv (dense tn) and dy (dense nn)
      -> layer-norm backward -> BPTT: per step an element-wise gate backward, dW_lstm += [x_t|h_{t-1}]^T
      dgates (dense tn) and d[x_t | h_{t-1}] = dgates @ W^T (dense nn).
    Parameter order: lstm_W, lstm_b, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv.
    --rnnCell gru: lstm_W and lstm_b are None and the cell's Wg, bg, Wc, bc follow drop_scale (the GRU tail); the
    recurrence and its BPTT are then _fusion_forward_gru / _fusion_backward_gru."""

    @staticmethod
    def forward(ctx, x, lstm_W, lstm_b, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale, *gru):
        attn = (ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv)
        out, h, gates, cell = _cell_forward(x, lstm_W, lstm_b, gru, attn, heads, drop_scale)
        ctx.save_for_backward(x, *((gru[0], gru[2]) if gru else (lstm_W,)), *attn, h, gates, cell,
                              drop_scale if drop_scale is not None else torch.empty(0, device=x.device))
        ctx.heads = heads
        ctx.has_drop = drop_scale is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, *cell_w, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, h, gates, cell, drop = ctx.saved_tensors
        drop = drop if ctx.has_drop else None
        dx, d_lstm, d_gru, d_attn = _cell_backward(x, cell_w, (ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv), h, gates, cell, drop,
                                                   ctx.heads, g_out)
        return (dx,) + d_lstm + d_attn + (None, None) + d_gru


def interval_fusion(x, p: dict, heads: int, drop_scale=None):
    """Differentiable interval fusion; p as in ops.interval_fusion (either cell). d must be one of TRAINABLE_D."""
    _check_trainable(x)
    lstm, gru = _cell_args(p)
    return IntervalFusionFn.apply(x, *lstm, p["ln_gamma"], p["ln_beta"], p["Wq"], p["bq"],
                                  p["Wk"], p["bk"], p["Wv"], p["bv"], heads, drop_scale, *gru)


class IntervalFusionRowsFn(torch.autograd.Function):
    """The interval fusion of the rows a training step reads: x [N, t, d] (any node/interval strides, the GNN slab's
    view), rows int32 [cap] ascending and distinct in their first `count` slots (ops.rows_compact), count int32 [1] on
    the device -> out [N, d], the fusion of x[rows[j]] in row rows[j] for j < count and exact zeros elsewhere.
    Forward: gather the rows into a dense [cap, t, d] block, _fusion_forward on it, scatter. Backward: gather the
    upstream gradient's rows (zeros in the padding slots j >= count), _fusion_backward, scatter dx into a zero
    [N, t, d] gradient. The fusion is independent per node, so an untouched row has no gradient to give.
    drop_scale: None, a full-size [N, t, d] mask (gathered with the rows) or a [cap, t, d] mask for the slots
    (cap != N). The cell's parameters as in IntervalFusionFn (the GRU tail follows drop_scale)."""

    @staticmethod
    def forward(ctx, x, rows, count, lstm_W, lstm_b, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, heads, drop_scale, *gru):
        N, t, d = (int(v) for v in x.shape)
        cap = int(rows.numel())
        dev = x.device
        attn = (ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv)
        ctx.heads, ctx.shape, ctx.x_layout = heads, (N, t, d), x.stride(1) == N * d and x.stride(0) == d
        out = torch.zeros((N, d), dtype=torch.float32, device=dev)
        ctx.has_drop = drop_scale is not None
        if cap == 0:
            ctx.empty = True
            ctx.save_for_backward(*(gru or (lstm_W,)), *attn)
            return out
        ctx.empty = False
        xs = ops.rows_gather(x.detach(), rows)                                           # [cap, t, d] dense
        drop = None
        if drop_scale is not None:
            if tuple(drop_scale.shape) == (N, t, d):
                drop = ops.rows_gather(drop_scale, rows)
            elif tuple(drop_scale.shape) == (cap, t, d):
                drop = drop_scale.contiguous()
            else:
                raise ValueError(f"drop_scale: expected [{N}, {t}, {d}] or [{cap}, {t}, {d}], got {tuple(drop_scale.shape)}")
        fused, h, gates, cell = _cell_forward(xs, lstm_W, lstm_b, gru, attn, heads, drop)
        ops.rows_scatter(fused, rows, count, out)
        ctx.save_for_backward(xs, rows, count, *((gru[0], gru[2]) if gru else (lstm_W,)), *attn, h, gates, cell,
                              drop if drop is not None else torch.empty(0, device=dev))
        return out

    @staticmethod
    def backward(ctx, g_out):
        N, t, d = ctx.shape
        if ctx.empty:
            *cell_w, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv = ctx.saved_tensors
            dev = Wq.device
            d_attn = tuple(torch.zeros_like(p) for p in (ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv))
            if len(cell_w) == 4:
                d_lstm, d_gru = (None, None), tuple(torch.zeros_like(p) for p in cell_w)
            else:
                d_lstm, d_gru = (torch.zeros_like(cell_w[0]), torch.zeros(4 * d, dtype=torch.float32, device=dev)), ()
            return (torch.zeros((N, t, d), dtype=torch.float32, device=dev), None, None) + d_lstm + d_attn + (None, None) + d_gru
        xs, rows, count, *cell_w, ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv, h, gates, cell, drop = ctx.saved_tensors
        drop = drop if ctx.has_drop else None
        g = ops.rows_gather(g_out if g_out.stride(1) == 1 else g_out.contiguous(), rows, count)   # [cap, d]
        dxs, d_lstm, d_gru, d_attn = _cell_backward(xs, cell_w, (ln_gamma, ln_beta, Wq, bq, Wk, bk, Wv, bv), h, gates, cell,
                                                    drop, ctx.heads, g)
        dev = xs.device
        # in the slab's own layout ([t, N, d] storage seen as [N, t, d]) when x is that view
        dx = torch.zeros((t, N, d), dtype=torch.float32, device=dev).permute(1, 0, 2) if ctx.x_layout else \
            torch.zeros((N, t, d), dtype=torch.float32, device=dev)
        ops.rows_scatter(dxs.contiguous(), rows, count, dx)
        return (dx, None, None) + d_lstm + d_attn + (None, None) + d_gru


def interval_fusion_rows(x, rows, count, cap: int, p: dict, heads: int, drop_scale=None):
    """Differentiable interval fusion of rows[:cap] of x (IntervalFusionRowsFn): [N, d] with exact zeros in every row
    not among the first `count` slots. rows / count as ops.rows_compact returns them (count on the device; cap, the
    number of slots to run, from the host, at least the count); p as in ops.interval_fusion (either cell)."""
    _check_trainable(x)
    if int(cap) > rows.numel():
        raise ValueError(f"cap = {int(cap)} > {rows.numel()} row slots")
    lstm, gru = _cell_args(p)
    return IntervalFusionRowsFn.apply(x, rows[:int(cap)], count, *lstm, p["ln_gamma"], p["ln_beta"],
                                      p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], heads, drop_scale, *gru)


# ----------------------------------------------------------------------------------------------
# Stand-alone differentiable pieces (prediction head, SSL branch): model.py:156-205, 241-250
# ----------------------------------------------------------------------------------------------


def _mhsa_mean_backward(y, Wq, bq, Wk, bk, Wv, bv, heads, g_out):
    """y [n, t, d] dense, g_out [n, d] -> (dy [n, t, d], dWq, dbq, dWk, dbk, dWv, dbv). y is the saved input of the
    forward: it is never overwritten, so the in-place tail of _fusion_backward is not taken."""
    n, t, d = y.shape
    Wqkv = torch.cat([Wq, Wk, Wv], dim=1).detach().contiguous()
    y2, qkv = _attn_bwd_qkv(y.contiguous(), None, None, Wqkv, Wq, bq, Wk, bk, Wv, bv, heads, g_out.contiguous())
    dy, dWqkv, dbqkv = _qkv_grads(y2, qkv, Wqkv, fused_tail=False, in_place=False)
    return (dy.view(n, t, d),) + _split_qkv_grads(dWqkv, dbqkv, d)


class SpmmFn(torch.autograd.Function):
    """y = A·x (pattern sum, no activation): the masked sums of model.py:161-162 on a per-batch
    CSR. Backward is the same kernel on the transposed CSR."""

    @staticmethod
    def forward(ctx, x, plan, plan_t):
        ctx.plan_t = plan_t
        return ops.spmm(plan, x.detach().contiguous(), 1.0)

    @staticmethod
    def backward(ctx, g):
        return ops.spmm(ctx.plan_t, g.contiguous(), 1.0), None, None


class SeqSumFn(torch.autograd.Function):
    """(fi, posEmbed) -> (seq_tok, pos_tok): the masked sums of model.py:161-162 read from a device-sampled batch's
    sequence segments (seq_items[seg_begin[b]:][:seg_len[b]], right-aligned) instead of two per-batch CSRs."""

    @staticmethod
    def forward(ctx, fi, pos_embed, seq_items, seg_begin, seg_len):
        ctx.save_for_backward(seq_items, seg_begin, seg_len)
        ctx.shape = (int(fi.shape[0]), int(pos_embed.shape[0]))
        return ops.seq_sum(fi.detach(), pos_embed.detach(), seq_items, seg_begin, seg_len)

    @staticmethod
    def backward(ctx, g_seq, g_pos):
        seq_items, seg_begin, seg_len = ctx.saved_tensors
        n_items, P = ctx.shape
        ref = g_seq if g_seq is not None else g_pos
        g_seq = torch.zeros_like(ref) if g_seq is None else g_seq.contiguous()
        g_pos = torch.zeros_like(ref) if g_pos is None else g_pos.contiguous()
        d_fi, d_pos = ops.seq_sum_bwd(g_seq, g_pos, seq_items, seg_begin, seg_len, n_items, P)
        return d_fi, d_pos, None, None, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta):
        x = x.detach().contiguous()
        ctx.save_for_backward(x, gamma)
        return ops.layernorm_td(x, gamma.detach(), beta.detach())

    @staticmethod
    def backward(ctx, g):
        x, gamma = ctx.saved_tensors
        return ops.layernorm_td_bwd(x, g.contiguous(), gamma.detach())


class MhsaMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Wq, bq, Wk, bk, Wv, bv, heads):
        x = x.detach().contiguous()
        ctx.save_for_backward(x, Wq, bq, Wk, bk, Wv, bv)
        ctx.heads = heads
        return ops.mhsa_mean(x, Wq.detach(), bq.detach(), Wk.detach(), bk.detach(), Wv.detach(), bv.detach(), heads)

    @staticmethod
    def backward(ctx, g):
        x, Wq, bq, Wk, bk, Wv, bv = ctx.saved_tensors
        return _mhsa_mean_backward(x, Wq, bq, Wk, bk, Wv, bv, ctx.heads, g.contiguous()) + (None,)


class LeakyAddFn(torch.autograd.Function):
    """out = max(leaky*a, a) + b (model.py:166)."""

    @staticmethod
    def forward(ctx, a, b, leaky):
        a = a.detach().contiguous()
        ctx.save_for_backward(a)
        ctx.leaky = leaky
        return ops.leaky_add(a, b.detach().contiguous(), leaky)

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        g = g.contiguous()
        return ops.leaky_bwd(a, g, ctx.leaky), g, None


class PairScoreFn(torch.autograd.Function):
    """preds[e] = <U[u], I[i]> + <leaky(S[l]), I[i]> (model.py:169-173; iEmbed_att IS final_item_vector)."""

    @staticmethod
    def forward(ctx, U, I, S, uids, iids, locs, leaky):
        U, I, S = U.detach().contiguous(), I.detach().contiguous(), S.detach().contiguous()
        ctx.save_for_backward(U, I, S, uids, iids, locs)
        ctx.leaky = leaky
        return ops.pair_score(U, I, uids, iids, S=S, A=I, locs=locs, leaky=leaky)

    @staticmethod
    def backward(ctx, g):
        U, I, S, uids, iids, locs = ctx.saved_tensors
        # A is I (iEmbed_att IS final_item_vector): dA is dI, both sums land in it
        dU, dI, dS, _ = ops.pair_score_bwd(U, I, uids, iids, g.contiguous(), S=S, A=I, locs=locs, leaky=ctx.leaky)
        return dU, dI, dS, None, None, None, None


class SoftmaxLossFn(torch.autograd.Function):
    """Full-catalogue softmax cross-entropy of ops.softmax_loss as a 1-element loss (--predLoss softmax). Saves lse;
    the backward recomputes the logits in two kernels (dQ by item chunk, dI by item tile) and never stores them."""

    @staticmethod
    def forward(ctx, Q, I, target, inv_temp, scale, excl, excl_row):
        Q, I = Q.detach().contiguous(), I.detach().contiguous()
        loss, lse, _ = ops.softmax_loss(Q, I, target, inv_temp, scale, excl, excl_row)
        ctx.save_for_backward(Q, I, target, lse)
        ctx.args = (inv_temp, scale, excl, excl_row)
        return loss

    @staticmethod
    def backward(ctx, g):
        Q, I, target, lse = ctx.saved_tensors
        dQ, dI = ops.softmax_loss_bwd(Q, I, target, lse, g.detach().reshape(1).float().contiguous(), *ctx.args)
        return dQ, dI, None, None, None, None, None


class SoftmaxLossCandFn(torch.autograd.Function):
    """SoftmaxLossFn over a candidate list (ops.softmax_loss_cand, --softmaxNegs). The backward returns a full-size dI:
    zeros, the candidates' rows copied to rows `cand` (distinct ids), then every slot's target row added at its target
    by ops.softmax_target_add, which orders the slots that share a target: bit-identical between runs.
    With bias (--softmaxNegDist pop: the offsets of ops.sample_strata_weighted, whose list repeats ids) the rows of the
    live positions alone are scattered (ops.softmax_cand_scatter): their ids are distinct, so no row has two writers.
    scatter_targets (--seqTargets all: a row per sequence token, far more than the batch softmax_target_add is meant
    for): the target rows go through ops.softmax_target_scatter, float atomics, equal up to the order of summation."""

    @staticmethod
    def forward(ctx, Q, I, cand, target, inv_temp, scale, excl, excl_row, bias=None, scatter_targets=False):
        Q, I = Q.detach().contiguous(), I.detach().contiguous()
        loss, lse, _ = ops.softmax_loss_cand(Q, I, cand, target, inv_temp, scale, excl, excl_row, bias)
        ctx.save_for_backward(Q, I, cand, target, lse, *(() if bias is None else (bias,)))
        ctx.args = (inv_temp, scale, excl, excl_row)
        ctx.scatter_targets = bool(scatter_targets)
        return loss

    @staticmethod
    def backward(ctx, g):
        Q, I, cand, target, lse, *bias = ctx.saved_tensors
        bias = bias[0] if bias else None
        dQ, dIc, dT = ops.softmax_loss_cand_bwd(Q, I, cand, target, lse, g.detach().reshape(1).float().contiguous(),
                                                *ctx.args, bias)
        dI = torch.zeros_like(I)
        if cand.numel():
            if bias is None:
                dI.index_copy_(0, cand.long(), dIc)
            else:
                ops.softmax_cand_scatter(dI, dIc, cand, bias)
        if ctx.scatter_targets:
            ops.softmax_target_scatter(dI, dT, target)
        else:
            ops.softmax_target_add(dI, dT, target)
        return dQ, dI, None, None, None, None, None, None, None, None


class ProdLeakySumFn(torch.autograd.Function):
    """s[e] = sum_j leaky(X[u][j] * Y[i][j]) (model.py:191, :199)."""

    @staticmethod
    def forward(ctx, X, Y, uids, iids, leaky):
        X, Y = X.detach().contiguous(), Y.detach().contiguous()
        ctx.save_for_backward(X, Y, uids, iids)
        ctx.leaky = leaky
        return ops.prod_leaky_sum(X, Y, uids, iids, leaky)

    @staticmethod
    def backward(ctx, g):
        X, Y, uids, iids = ctx.saved_tensors
        dX, dY = ops.prod_leaky_sum_bwd(X, Y, uids, iids, ctx.leaky, g.contiguous())
        return dX, dY, None, None, None


def _pad_cols(W, kp):
    out = torch.zeros(W.shape[:-1] + (kp,), dtype=W.dtype, device=W.device)
    out[..., : W.shape[-1]] = W
    return out


class MetaWeightFn(torch.autograd.Function):
    """w[e] = sigmoid(FC(leaky(FC([F*V | F | V][u_e])))) (model.py:179-182), evaluated for the sampled
    users only (the reference computes it for every user and gathers afterwards: same values).
    W2 [3d, k], b2 [k], W3 [k, 1], b3 [1]; k = ssldim is padded to a multiple of 32 for the MFMA
    product."""

    @staticmethod
    def forward(ctx, F, V, uids, W2, b2, W3, b3, leaky):
        F, V = F.detach().contiguous(), V.detach().contiguous()
        k = W2.shape[1]
        kp = (k + 31) // 32 * 32
        m1 = ops.meta_features(F, V, uids)
        W2p = _pad_cols(W2.detach(), kp).contiguous()
        z1 = ops.dense_nn(m1, W2p, _pad_cols(b2.detach(), kp).contiguous())
        a1 = ops.leaky(z1, leaky)
        w3 = W3.detach().reshape(-1).contiguous()
        w = ops.rowdot_sigmoid(a1, w3, b3.detach(), k)
        ctx.save_for_backward(F, V, uids, m1, z1, a1, w, W2p, w3)
        ctx.cfg = (leaky, k, kp)
        return w

    @staticmethod
    def backward(ctx, dw):
        F, V, uids, m1, z1, a1, w, W2p, w3 = ctx.saved_tensors
        leaky, k, kp = ctx.cfg
        d = F.shape[1]
        dev = F.device
        dA, dw3, db3 = ops.rowdot_sigmoid_bwd(a1, w3, w, dw.contiguous(), k)
        dz1 = ops.leaky_bwd(z1, dA, leaky)
        dW2p = torch.zeros((3 * d, kp), dtype=torch.float32, device=dev)
        db2p = torch.zeros(kp, dtype=torch.float32, device=dev)
        ops.dense_tn(m1, dz1, dW2p, db2p)
        dm1 = ops.dense_nn(dz1, W2p.t().contiguous(), None)
        dF, dV = ops.meta_features_bwd(F, V, uids, dm1)
        return dF, dV, None, dW2p[:, :k].contiguous(), db2p[:k].contiguous(), dw3.view(k, 1), db3, None


class HingeFn(torch.autograd.Function):
    """scale * sum max(0, 1 - S*(pos - neg)), S = wp*sp - wn*sn or 1 (model.py:202, :244). sp/sn are
    constants (tf.stop_gradient, model.py:192-193)."""

    @staticmethod
    def forward(ctx, pos, neg, wp, wn, sp, sn, scale):
        weighted = wp is not None
        pos, neg, wp, wn, sp, sn = (None if v is None else v.detach().contiguous() for v in (pos, neg, wp, wn, sp, sn))
        loss, dpos, dneg, dwp, dwn = ops.hinge(pos, neg, wp, wn, sp, sn, scale)
        ctx.weighted = weighted
        ctx.save_for_backward(dpos, dneg, *((dwp, dwn) if weighted else ()))
        return loss

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        dpos, dneg = saved[0] * g, saved[1] * g
        if ctx.weighted:
            return dpos, dneg, saved[2] * g, saved[3] * g, None, None, None
        return dpos, dneg, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# Self-attention over the item sequence (--seqAtt full; seq_attn.hip). Activations
# are padded slabs [n_slots * P, d]; seg_len (int32 [n_slots], on the device) holds the lengths.
# ----------------------------------------------------------------------------------------------


class SeqGatherFn(torch.autograd.Function):
    """(fi, posEmbed) -> (item token slab, position token slab), both [n_slots * P, d] with zeros in the padding
    (ops.seq_gather). Slot b's token j is item seq_items[seg_begin[b] + j] at position seq_pos[seg_begin[b] + j],
    or right-aligned (P - n_b + j) with seq_pos None."""

    @staticmethod
    def forward(ctx, fi, pos_embed, seq_items, seq_pos, seg_begin, seg_len):
        ctx.tokens = (seq_items, seq_pos, seg_begin, seg_len)
        ctx.shape = (int(fi.shape[0]), int(pos_embed.shape[0]))
        return ops.seq_gather(fi.detach(), pos_embed.detach(), seq_items, seq_pos, seg_begin, seg_len)

    @staticmethod
    def backward(ctx, g_seq, g_pos):
        n_items, P = ctx.shape
        ref = g_seq if g_seq is not None else g_pos
        g_seq = torch.zeros_like(ref) if g_seq is None else g_seq.contiguous()
        g_pos = torch.zeros_like(ref) if g_pos is None else g_pos.contiguous()
        d_fi, d_pos = ops.seq_gather_bwd(g_seq, g_pos, *ctx.tokens, n_items, P)
        return d_fi, d_pos, None, None, None, None


class SeqAttnFn(torch.autograd.Function):
    """One sequence-attention layer on a slab: x [n_slots * P, d] -> leaky(ctx) + x with y = LN(x) per token,
    q|k|v = y [Wq|Wk|Wv] + b and ctx the ragged attention over each slot's real tokens (ops.seq_attn).
    Saved for the backward: x and q|k|v. The backward recomputes ctx (for the slope of leaky) and y, then
    ops.seq_attn_bwd -> dW, db (dense_tn) and dy (dense_nn) -> layer-norm backward. Padded rows of the incoming gradient must be zero (SeqPoolFn's and this class's are); the returned
    gradient's are."""

    @staticmethod
    def forward(ctx, x, gamma, beta, Wq, bq, Wk, bk, Wv, bv, seg_len, P, heads, leaky, causal=False):
        x = x.detach().contiguous()
        R, d = x.shape
        y = ops.layernorm_td(x.view(R, 1, d), gamma.detach(), beta.detach()).view(R, d)
        Wqkv = torch.cat([Wq, Wk, Wv], dim=1).detach().contiguous()
        bqkv = torch.cat([bq, bk, bv]).detach().contiguous()
        qkv = ops.dense_nn(y, Wqkv, bqkv)
        causal = bool(causal)
        if d // int(heads) >= 16:                     # --seqHeads: few wide heads, on the matrix cores
            att = ops.seq_attn_wide(qkv, seg_len, P, heads, causal)
        else:
            att = ops.seq_attn(qkv, seg_len, P, heads, causal) if causal else ops.seq_attn(qkv, seg_len, P, heads)
        ctx.save_for_backward(x, qkv, gamma, beta, Wqkv, seg_len)
        ctx.cfg = (int(P), int(heads), float(leaky))
        ctx.causal = causal
        return ops.leaky_add(att, x, leaky)

    @staticmethod
    def backward(ctx, g):
        x, qkv, gamma, beta, Wqkv, seg_len = ctx.saved_tensors
        P, heads, leaky = ctx.cfg
        R, d = x.shape
        g = g.contiguous()
        wide = d // heads >= 16
        mask = (True,) if ctx.causal else ()          # the default path's calls stay what they were
        att = ops.seq_attn_wide(qkv, seg_len, P, heads, ctx.causal) if wide else ops.seq_attn(qkv, seg_len, P, heads, *mask)
        g_att = ops.leaky_bwd(att, g, leaky)
        dqkv = (ops.seq_attn_wide_bwd(qkv, g_att, seg_len, P, heads, ctx.causal) if wide
                else ops.seq_attn_bwd(qkv, g_att, seg_len, P, heads, *mask))
        y = ops.layernorm_td(x.view(R, 1, d), gamma.detach(), beta.detach()).view(R, d)     # not saved: recomputed
        # dW, db and dy as two products, not the fused tail (ops.attn_bwd_tail). This layer was written while the tail
        # returned NaN bias gradients for a workgroup whose first chunk held only zero rows (a slab's padding: any slot
        # shorter than P - 32). The tail now gives a zero gradient row the factor 0
        # (tests/test_gpu_zero_grad_rows.py); moving this layer onto it is a performance change that has not been measured
        dy, dWqkv, dbqkv = _qkv_grads(y, dqkv, Wqkv, fused_tail=False, in_place=True)
        dy = dy.view(R, 1, d)
        dy, dgamma, dbeta = ops.layernorm_td_bwd(x.view(R, 1, d), dy, gamma.detach(), out=dy)
        dx = ops.leaky_add(dy.view(R, d), g, 1.0)                                     # slope 1: dy + g, the residual's share
        return (dx, dgamma, dbeta) + _split_qkv_grads(dWqkv, dbqkv, d) + (None, None, None, None, None)


class SeqFfnFn(torch.autograd.Function):
    """The position-wise feed-forward block after a sequence-attention layer (--seqFFN): x [n_slots * P,
    d] -> x + act(LN(x) W1 + b1) W2 + b2 on the real token rows, zero rows in the padding (ops.seq_ffn). Saved for the
    backward: x and the parameters; the backward is one ops.seq_ffn_bwd call, which recomputes the hidden activations.
    Padded rows of the incoming gradient must be zero (SeqPoolFn's and SeqAttnFn's are); the returned gradient's are."""

    @staticmethod
    def forward(ctx, x, gamma, beta, W1, b1, W2, b2, seg_len, P, leaky):
        x = x.detach().contiguous()
        params = tuple(p.detach().contiguous() for p in (gamma, beta, W1, b1, W2, b2))
        ctx.save_for_backward(x, *params, seg_len)
        ctx.cfg = (int(P), float(leaky))
        return ops.seq_ffn(x, *params, seg_len, P, leaky)

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta, W1, b1, W2, b2, seg_len = ctx.saved_tensors
        return ops.seq_ffn_bwd(x, g.contiguous(), gamma, beta, W1, b1, W2, b2, seg_len, *ctx.cfg) + (None, None, None)


class SeqPoolFn(torch.autograd.Function):
    """x [n_slots * P, d] -> [n_slots, d]: the sum over each slot's real tokens (ops.seq_pool); the backward
    broadcasts, with zeros into the padding."""

    @staticmethod
    def forward(ctx, x, seg_len, P):
        ctx.save_for_backward(seg_len)
        ctx.P = int(P)
        return ops.seq_pool(x.detach().contiguous(), seg_len, P)

    @staticmethod
    def backward(ctx, g):
        (seg_len,) = ctx.saved_tensors
        return ops.seq_pool_bwd(g.contiguous(), seg_len, ctx.P), None, None


class SeqPrefixQueryFn(torch.autograd.Function):
    """(x [n_slots * P, d], U [n_slots, d]) -> Q [n_slots * P, d]: a query per prefix of each slot's sequence
    (--seqTargets all), Q[b, j] = leaky(sum_{i <= j} x[b, i]) + U[b] with zero rows in the padding
    (ops.seq_prefix_query). Saved for the backward: x; the prefix sums are recomputed (ops.seq_prefix_query_bwd)."""

    @staticmethod
    def forward(ctx, x, U, seg_len, P, leaky):
        x = x.detach().contiguous()
        ctx.save_for_backward(x, seg_len)
        ctx.cfg = (int(P), float(leaky))
        return ops.seq_prefix_query(x, U.detach().contiguous(), seg_len, P, leaky)

    @staticmethod
    def backward(ctx, g):
        x, seg_len = ctx.saved_tensors
        dx, dU = ops.seq_prefix_query_bwd(x, g.contiguous(), seg_len, *ctx.cfg)
        return dx, dU, None, None, None


class SeqAddPoolFn(torch.autograd.Function):
    """x [n_slots * P, d] -> [n_slots, d]: additive-attention pooling over each slot's real tokens (--seqPool additive,
    DESIGN.md §21): u = x Wa + ba over the slab (ops.dense_nn), out[b] = sum_j w_j x_j with w the softmax of
    <tanh(u_j), v> (ops.seq_addpool). Saved for the backward: x and u. The backward is ops.seq_addpool_bwd (w_j g, du,
    dv) -> dWa, dba (dense_tn) and dx += du Wa^T (dense_nn, accumulating); zeros into the padding."""

    @staticmethod
    def forward(ctx, x, Wa, ba, v, seg_len, P):
        x = x.detach().contiguous()
        Wa, v = Wa.detach().contiguous(), v.detach().contiguous()
        u = ops.dense_nn(x, Wa, ba.detach().contiguous())
        ctx.save_for_backward(x, u, Wa, v, seg_len)
        ctx.P = int(P)
        return ops.seq_addpool(x, u, v, seg_len, P)

    @staticmethod
    def backward(ctx, g):
        x, u, Wa, v, seg_len = ctx.saved_tensors
        dx, du, dv = ops.seq_addpool_bwd(x, u, v, g.contiguous(), seg_len, ctx.P)
        dWa, dba = torch.zeros_like(Wa), torch.zeros(Wa.shape[1], dtype=torch.float32, device=Wa.device)
        ops.dense_tn(x, du, dWa, dba)
        ops.dense_nn(du, Wa.t().contiguous(), None, out=dx, accumulate=True)
        return dx, dWa, dba, dv, None, None
