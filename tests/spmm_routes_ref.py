"""What tests/test_gpu_spmm_routes.py stands on, none of it touching a device:

  selection   the Python restatement of which instantiation of the SpMM row kernels a launch takes (spmm.hip lines cited);
  pattern     the graph with many rows and little work: every row empty except three windows of a few hundred rows whose
              degrees are laid out by position in the 16-row block of a wave;
  reference   the stack, its one product and its adjoint in float64 torch, edge by edge, over the window rows alone.

The ABI does not say which instantiation ran, so the selection is restated here and tests/test_spmm_routes_host.py holds
it against the case table; the reference is held against a dense restatement there."""
import itertools

import numpy as np
import torch

import edge_drop_ref as D

# ---- the selection (sa-gnn_amd/csrc) -----------------------------------------------------------------------------------
K_WAVE = 64                  # spmm.hip:42 kWave
WAVES_PER_BLOCK = 4          # spmm.hip:43-44 kBlock / kWave
ROWS_PER_WAVE = 16           # spmm.hip:45 kRowsPerWave
K_SMALL_ROWS = 262144        # spmm.hip:49 kSmallRows
UNROLL = 8                   # spmm.hip:50 kUnroll
DEFAULT_TUNING = (16, 256, 256)   # spmm.hip:685-689 kDefaultShort / kDefaultLong / kDefaultChunk

WIDTHS = (4, 32, 48, 64, 128, 256)
FORMS = ("plain", "weights", "drop", "drop+weights", "time", "time+weights")
ENTRIES = ("per-plan", "batched")
VARIANTS = ("small", "large")
BWD_WIDTHS = (32, 64, 128, 256)       # one width per lane-group class


def lpr(d):
    """common.h:27-32 lanes_per_row: 8, 16, 32 or 64 lanes of one float4 each for d <= 32, 64, 128, 256."""
    need, lanes = (d + 3) // 4, 8
    while lanes < need:
        lanes <<= 1
    return lanes


def group(d):
    """G = kWave / LPR: the feature rows one gather instruction of a wave covers (spmm.hip:395)."""
    return K_WAVE // lpr(d)


def variant(n_rows):
    """spmm.hip:878 launch_spmm: small = n_rows < kSmallRows."""
    return "small" if n_rows < K_SMALL_ROWS else "large"


def batch_variant(U, I):
    """spmm.hip:1257 launch_batch: small = max(U, I) < kSmallRows, for the user AND the item segments."""
    return "small" if max(U, I) < K_SMALL_ROWS else "large"


def rpw(var, d):
    """Rows per wave: RPW_SMALL = max(G, 4) (spmm.hip:877, :1256) or kRowsPerWave."""
    return max(group(d), 4) if var == "small" else ROWS_PER_WAVE


def short_iters(var, d):
    """Iterations of the short-row loop of rows_wave, RPW / G (spmm.hip:423)."""
    return rpw(var, d) // group(d)


FORM_FLAGS = {                 # form: (weights, drop, time)
    "plain": (False, False, False), "weights": (True, False, False),
    "drop": (False, True, False), "drop+weights": (True, True, False),
    "time": (False, False, True), "time+weights": (True, False, True),
}


def form_name(weights, drop, time):
    """The form of a launch from the plan (weights; the buckets a time call needs) and the call (drop, time)."""
    if drop and time:
        raise ValueError(REFUSED["drop+time"])
    return {flags: name for name, flags in FORM_FLAGS.items()}[bool(weights), bool(drop), bool(time)]


def form_flags(form):
    """(weights, drop, time) of a form name."""
    return FORM_FLAGS[form]


# The neighbours of the table the library refuses, each with its refusal; none of WIDTHS x FORMS is among them.
REFUSED = {
    "drop+time": "edge dropout and time do not combine",                             # spmm.hip:1503 check_time (:973 one product), ops._gnn_args
    "d=2": "need a multiple of 4 in [4, 256]",                                       # spmm.hip:933-936 check_d
    "d=6": "need a multiple of 4 in [4, 256]",
    "d=260": "need a multiple of 4 in [4, 256]",
}


def check_d(d):
    """spmm.hip:933-936: the widths the SpMM takes."""
    return not (d < 4 or d > 256 or d & 3)


def all_cells():
    """variant x d x form x entry; the library refuses none of them (REFUSED lies outside)."""
    assert all(check_d(d) for d in WIDTHS)
    return set(itertools.product(VARIANTS, WIDTHS, FORMS, ENTRIES))


# ---- the pattern -------------------------------------------------------------------------------------------------------
def tuning_for(d, wide=False):
    """(short_thresh, long_thresh, chunk_edges) of a width's cases. d = 32 keeps the library's defaults (16 > LPR = 8). The
    others lower the long threshold to 129, the largest medium degree the issue names, and the chunk to 192 so that a long
    row of ONE chunk exists; their short threshold is LPR + 5, past a lane group. At LPR = 64 the medium degrees 63, 64
    and 65 and a short threshold past 64 cannot share one tuning, so d = 256 has two: 40 (those medium degrees, no short
    row past the lane group) and, with wide=True, 70 (short rows of up to 70 edges, the reload of a row's second slice;
    63, 64 and 65 are short rows there)."""
    assert not wide or d in WIDE_WIDTHS
    if d == 32:
        return DEFAULT_TUNING
    lanes = lpr(d)
    return (lanes + 5 if lanes < 64 else 70 if wide else 40, 129, 192)


WIDE_WIDTHS = (256,)          # the widths that run a second, `wide` tuning


def chunks_of(deg, chunk):
    """spmm.hip:747-755: the balanced cut of a long row, chunk lengths in order."""
    nck = (deg + chunk - 1) // chunk
    ln = (deg + nck - 1) // nck
    ln = (ln + K_WAVE - 1) // K_WAVE * K_WAVE
    return [min(deg, s + ln) - s for s in range(0, deg, ln)]


def row_class(deg, tuning):
    st, lt, _ = tuning
    return "empty" if deg == 0 else "short" if deg <= st else "medium" if deg <= lt else "long"


def degree_pools(d, wide=False):
    """(medium, long) degrees of a width: the 64-edge slice boundaries of wave_row_sum and one degree per remainder modulo
    G * kUnroll; a long row of one chunk (where the tuning has one), one of three or more chunks whose last holds a single
    edge, and two plain ones."""
    st, lt, ch = tuning_for(d, wide)
    step = group(d) * UNROLL
    base = (st // step + 1) * step
    medium = [x for x in (63, 64, 65, 129) if x > st] + [base + r for r in range(step)]
    assert all(st < x <= lt for x in medium), (d, medium)
    one_chunk = [x for x in (lt + 1, ch) if x > lt and len(chunks_of(x, ch)) == 1]
    single = next(x for x in range(lt + 1, 8 * ch) if len(chunks_of(x, ch)) >= 3 and chunks_of(x, ch)[-1] == 1)
    long_ = one_chunk + [single, lt + 2, ch + 1]
    assert all(x > lt for x in long_)
    return medium, long_


def window_blocks(d, wide=False):
    """[(label, 16 degrees)]: the blocks of one window, each the row block of one wave of the large variant."""
    st, lt, ch = tuning_for(d, wide)
    lanes, G = lpr(d), group(d)
    medium, long_ = degree_pools(d, wide)
    med, lng = itertools.cycle(medium), itertools.cycle(long_)
    blocks = [("ramp_up", [round(i * st / 15) for i in range(16)]),
              ("ramp_down", [round((15 - i) * st / 15) for i in range(16)]),
              ("alt_row", [0, st] * 8),
              ("alt_iter", [st * ((i // G) % 2) for i in range(16)]),
              ("alt_iter_inv", [st * (1 - (i // G) % 2) for i in range(16)])]
    if st > lanes:      # short rows wider than a lane group next to narrower ones (G >= 2: in the same iteration)
        half = [st, 1, lanes + 1, lanes, st - 1, 0, lanes + 1, 2]
        # G = 1: an iteration is one row; the second half brings the slice boundaries 63, 64, 65 in as short rows
        blocks.append(("wide_short", half + ([lanes - 1, st, 3, lanes + 2, lanes, 7, st - 2, lanes + 1] if G == 1 else half)))
    for s in range(4):  # every class at every position modulo G (G <= 8): position p of block s holds class (p + s) % 4
        degs = []
        for i in range(16):
            c = (i + s) % 4
            degs.append(0 if c == 0 else (3 * i + s) % st + 1 if c == 1 else next(med) if c == 2 else next(lng))
        blocks.append((f"mixed_{s}", degs))
    pool = list(medium)
    while len(pool) % 16:
        pool.append(next(med))
    blocks += [(f"all_medium_{j}", pool[16 * j:16 * j + 16]) for j in range(len(pool) // 16)]
    blocks.append(("all_long", [next(lng) for _ in range(16)]))
    blocks.append(("tail_mix", dict(blocks)["mixed_1"]))       # mixed_1 again (short, medium, long, empty, ...): what the last, cut wave holds
    return blocks


def window_degrees(d, wide=False):
    return np.array([x for _, b in window_blocks(d, wide) for x in b], np.int64)


def large_rows(k, r):
    """n_rows = 262144 + 64 k + r."""
    return K_SMALL_ROWS + 64 * k + r


class Pattern:
    """One interval's stored pattern, rows = users: rowptr / colidx (int32), and per edge, in colidx order, its row, a
    weight (negative ones and exact zeros among them) and a bucket id below 3 and below 300. win: the global ids of the
    window rows (ascending), windows: their (start, length); every other row is empty."""

    def transposed(self):
        """(rowptr, colidx, order): the exact transpose with multiplicities, rows = items, users ascending within an
        item; order permutes the per-edge arrays alongside."""
        order = np.lexsort((self.rows, self.colidx))
        rp = np.zeros(self.n_src + 1, np.int64)
        np.cumsum(np.bincount(self.colidx, minlength=self.n_src), out=rp[1:])
        return rp.astype(np.int32), self.rows[order].astype(np.int32), order


def pattern(d, n_rows, n_src, seed=0, mid_start=None, tail_start=None, tail_len=None, wide=False):
    """The windows of width d at rows 0, mid_start (default: 32 rows ahead of a 64-row block boundary near the middle) and
    tail_start (default: the last rows, so that the cut last wave holds the head of `tail_mix`). A window's edges depend
    on (seed, d, window) alone, so two patterns of different row counts hold the same windows."""
    degs = window_degrees(d, wide)
    W = len(degs)
    if mid_start is None:
        mid_start = (n_rows // 2) // 64 * 64 - 32
    if tail_start is None:
        tail_start = -(-(n_rows - W) // 16) * 16
    if tail_len is None:
        tail_len = n_rows - tail_start
    assert mid_start % 16 == 0 and tail_start % 16 == 0 and W <= mid_start and mid_start + W <= tail_start
    assert 0 < tail_len <= W and tail_start + tail_len == n_rows
    p = Pattern()
    p.d, p.n_rows, p.n_src, p.tuning, p.seed, p.wide = d, n_rows, n_src, tuning_for(d, wide), seed, wide
    p.windows = [(0, W), (mid_start, W), (tail_start, tail_len)]
    deg = np.zeros(n_rows, np.int64)
    cols, wts, b3, b300 = [], [], [], []
    st, lt, _ = p.tuning
    for w, (start, length) in enumerate(p.windows):
        rng = np.random.default_rng([seed, d, w, int(wide)])
        c = rng.integers(0, n_src, int(degs.sum())).astype(np.int32)
        e0 = np.concatenate([[0], np.cumsum(degs)])
        for lo, hi in ((2, st), (st + 1, lt)):      # a duplicated stored entry inside a short and inside a medium row
            r = int(np.flatnonzero((degs >= lo) & (degs <= hi))[0])
            c[e0[r] + 1] = c[e0[r]]
        x = rng.standard_normal(c.size).astype(np.float32)
        x[rng.random(c.size) < 0.1] = 0.0
        n = int(e0[length])
        deg[start:start + length] = degs[:length]
        cols.append(c[:n]), wts.append(x[:n])
        b3.append(rng.integers(0, 3, c.size).astype(np.uint16)[:n]), b300.append(rng.integers(0, 300, c.size).astype(np.uint16)[:n])
    p.rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    p.colidx, p.weights = np.concatenate(cols), np.concatenate(wts)
    p.buckets = {3: np.concatenate(b3), 300: np.concatenate(b300)}
    p.rows = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    p.win = np.concatenate([np.arange(s, s + n) for s, n in p.windows])
    p.deg = deg
    return p


def phantom(n_rows, n_src, d, wide=False):
    """The empty interval as the model stores it: the single edge (0, 0), bucket 0."""
    p = Pattern()
    p.d, p.n_rows, p.n_src, p.tuning = d, n_rows, n_src, tuning_for(d, wide)
    p.rowptr = np.concatenate([[0], np.ones(n_rows, np.int32)]).astype(np.int32)
    p.colidx, p.weights = np.zeros(1, np.int32), np.array([-0.75], np.float32)
    p.buckets = {3: np.zeros(1, np.uint16), 300: np.zeros(1, np.uint16)}
    p.rows, p.deg = np.zeros(1, np.int64), np.diff(p.rowptr).astype(np.int64)
    p.windows, p.win = [], np.zeros(0, np.int64)
    return p


def small_twin(big):
    """The small-variant pattern of the same windows: the first two at their own rows (so a drop decides their edges alike),
    the last right behind the second; fewer than 262,144 rows."""
    (_, W), (mid, _), (_, tail_len) = big.windows
    tail = mid + W
    assert tail % 16 == 0
    small = pattern(big.d, tail + tail_len, big.n_src, big.seed, mid, tail, tail_len, big.wide)
    assert variant(small.n_rows) == "small"
    return small


# ---- the float64 reference, edge by edge --------------------------------------------------------------------------------
def f64(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64)


def edge_list(pat, rows_local, form, drop, k, M, L):
    """One interval's edges for the reference: local user row, item, bucket, and per layer the coefficient of the edge in
    the user-side product (direction 0) and in the item-side one (direction 1): its weight (1 without weights), times the
    drop's scale where edge_drop_ref keeps it and 0 where it does not. rows_local maps a global user id to its reference
    row. drop: (seed, step, threshold, scale) or None."""
    weights, dropped, timed = form_flags(form)
    w = pat.weights.astype(np.float64) if weights else np.ones(pat.colidx.size)
    coef = []
    for l in range(L):
        pair = []
        for direction in (0, 1):
            c = w
            if dropped:
                seed, step, thresh, scale = drop
                kept = D.keep_mask(seed, step, k, l, direction, pat.rows, pat.colidx, thresh=thresh)
                c = w * kept * float(np.float32(scale))
            pair.append(f64(c))
        coef.append(pair)
    return {"u": torch.as_tensor(rows_local[pat.rows]), "i": torch.as_tensor(pat.colidx.astype(np.int64)),
            "b": torch.as_tensor(pat.buckets[M].astype(np.int64)) if timed else None, "coef": coef}


def product(n_out, out_idx, src_idx, coef, x, te=None, b=None):
    """s[out_idx[e]] += coef[e] * (x[src_idx[e]] + te[b[e]])."""
    v = x[src_idx]
    if te is not None:
        v = v + te[b]
    return torch.zeros((n_out, x.shape[1]), dtype=torch.float64).index_add(0, out_idx, coef[:, None] * v)


def stack(edges, u0, i0, te, L, leaky, slopes=None, terms=False):
    """e^{l+1} = act(A e_other^l + C TE[k, l, dir]) + e^l on the reference rows; outputs sum_l e^l. u0 [T, W, d], i0
    [T, I, d], te [T, L, 2, M, d] or None. slopes: None (act = max(leaky s, s), ties to the leaky side as the kernels'
    masks do) or [k][l][side] bool tensors that say where the slope is 1. Returns a dict: out_u, out_i, and sums[k][l] =
    (s_u, s_i), the row sums ahead of the activation.
    terms: also the abs_terms of assert_sum_close by the recurrence of _sparse_stack_reference (test_gpu_edge_drop.py):
    t^0 = 0, t^{l+1} = |A| (|e_other^l| + t_other^l) + |C| |TE| + |e^l| + t^l, an output collecting sum_l (|e^l| + t^l), as
    terms_u / terms_i; and sum_terms[k][l], the |A| ... + |C| |TE| part alone, which bounds the rounding of a row sum."""
    res = {"out_u": [], "out_i": [], "sums": [], "terms_u": [], "terms_i": [], "sum_terms": []}
    for k, e in enumerate(edges):
        eu, ei, sk, tk = [u0[k]], [i0[k]], [], []
        tu, ti = torch.zeros_like(u0[k]), torch.zeros_like(i0[k])
        term_u, term_i = u0[k].abs(), i0[k].abs()
        for l in range(L):
            cu, ci = e["coef"][l]
            te_u, te_i = (None, None) if te is None else (te[k, l, 0], te[k, l, 1])
            su = product(u0.shape[1], e["u"], e["i"], cu, ei[-1], te_u, e["b"])
            si = product(i0.shape[1], e["i"], e["u"], ci, eu[-1], te_i, e["b"])
            if terms:
                with torch.no_grad():
                    au, ai = (None, None) if te is None else (te_u.abs(), te_i.abs())
                    tsu = product(u0.shape[1], e["u"], e["i"], cu.abs(), ei[-1].abs() + ti, au, e["b"])
                    tsi = product(i0.shape[1], e["i"], e["u"], ci.abs(), eu[-1].abs() + tu, ai, e["b"])
                    tu, ti = tsu + eu[-1].abs() + tu, tsi + ei[-1].abs() + ti
                    tk.append((tsu, tsi))
            pu, pi = (su > 0, si > 0) if slopes is None else slopes[k][l]
            eu.append(torch.where(pu, su, leaky * su) + eu[-1])
            ei.append(torch.where(pi, si, leaky * si) + ei[-1])
            sk.append((su, si))
            if terms:
                with torch.no_grad():
                    term_u, term_i = term_u + eu[-1].abs() + tu, term_i + ei[-1].abs() + ti
        res["out_u"].append(sum(eu[1:], eu[0])), res["out_i"].append(sum(ei[1:], ei[0]))
        res["sums"].append(sk), res["sum_terms"].append(tk)
        res["terms_u"].append(term_u), res["terms_i"].append(term_i)
    for key in ("out_u", "out_i", "terms_u", "terms_i"):
        res[key] = torch.stack(res[key])
    return res


def abs_edges(edges):
    """The same edges with |coefficient|: the stack over them with leaky = 1 is linear, and its autograd under |G| sums
    the absolute values of what the adjoint adds up, the abs_terms of a gradient."""
    return [{**e, "coef": [[c.abs() for c in pair] for pair in e["coef"]]} for e in edges]


def stack_grads(edges, u0, i0, te, gu, gi, L, leaky, slopes):
    """float64 autograd of `stack` under L = <out_u, gu> + <out_i, gi>: (du0, di0, dte or None), and their abs_terms."""
    def run(edges, leaky, slopes, gu, gi, te):
        tu, ti = u0.clone().requires_grad_(True), i0.clone().requires_grad_(True)
        tt = None if te is None else te.clone().requires_grad_(True)
        r = stack(edges, tu, ti, tt, L, leaky, slopes)
        ((r["out_u"] * gu).sum() + (r["out_i"] * gi).sum()).backward()
        return tu.grad, ti.grad, None if tt is None else tt.grad
    ones = [[(torch.ones_like(u0[0], dtype=torch.bool), torch.ones_like(i0[0], dtype=torch.bool))] * L] * len(edges)
    return run(edges, leaky, slopes, gu, gi, te), run(abs_edges(edges), 1.0, ones, gu.abs(), gi.abs(), None if te is None else te.abs())


def one_product(e, l, direction, x, te, leaky, res, acc):
    """One product on the user rows (direction 0) with the epilogue: (out, acc_out, abs_terms of out)."""
    assert direction == 0
    c = e["coef"][l][0]
    s = product(res.shape[0], e["u"], e["i"], c, x, te, e["b"])
    t = product(res.shape[0], e["u"], e["i"], c.abs(), x.abs(), None if te is None else te.abs(), e["b"])
    y = torch.maximum(leaky * s, s) + res
    return y, y + acc, t + res.abs()


def dense_stack(edges, u0, i0, te, L, leaky):
    """`stack` restated on dense matrices, A[k][l][dir] and C[k][l][dir] accumulated entry by entry: the check of the
    sparse form (tests/test_spmm_routes_host.py)."""
    W, I = u0.shape[1], i0.shape[1]
    outs_u, outs_i = [], []
    for k, e in enumerate(edges):
        eu, ei = [u0[k].numpy()], [i0[k].numpy()]
        for l in range(L):
            s = []
            for direction, (n_out, n_src, oi, sidx, x) in enumerate(((W, I, e["u"], e["i"], ei[-1]), (I, W, e["i"], e["u"], eu[-1]))):
                a = np.zeros((n_out, n_src))
                np.add.at(a, (oi.numpy(), sidx.numpy()), e["coef"][l][direction].numpy())
                v = a @ x
                if te is not None:
                    c = np.zeros((n_out, te.shape[3]))
                    np.add.at(c, (oi.numpy(), e["b"].numpy()), e["coef"][l][direction].numpy())
                    v = v + c @ te[k, l, direction].numpy()
                s.append(v)
            eu.append(np.maximum(leaky * s[0], s[0]) + eu[-1])
            ei.append(np.maximum(leaky * s[1], s[1]) + ei[-1])
        outs_u.append(sum(eu[1:], eu[0])), outs_i.append(sum(ei[1:], ei[0]))
    return np.stack(outs_u), np.stack(outs_i)
