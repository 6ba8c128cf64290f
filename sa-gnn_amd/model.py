"""Recommender with the reference's entry points (reference model.py:18-250) over libsagnn.so.

What is kept: `Recommender(sess, handler)`, `.prepareModel()`, `.ours()`,
`.messagePropagate(srclats, mat, type)`, `.edgeDropout(mat)`, the parameter names/shapes and the
L2 registry. `sess` is the device context (a torch.device or its string); the TF graph/session
split disappears, so `ours()` runs the hot path eagerly on the current HIP stream.

Scope: the per-interval propagation stack and the interval fusion — everything
that produces `final_user_vector` / `final_item_vector` (reference model.py:104-155). The
prediction head, SSL loss, samplers and optimiser around it are §8(f) "next" rows.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import autograd as ag
from . import ops
from .Params import args
from .Utils import NNLayers as NNs
from .Utils.attention import MultiHeadSelfAttention
from .graph import NORMS, interval_pair


SEQ_ATT = ("sum", "full", "causal")   # args.seqAtt: the reference's collapsed head, attention over every sequence item, or
                                      # that attention under a causal mask (--seqAtt full --seqMask causal, Params.parse_args)
SEQ_TOKEN_MODES = ("full", "causal")  # the modes in which every sequence item is a token (causal: a token sees no later one)
SEQ_TARGETS = ("last", "all")  # --seqTargets: one loss term per slot, or one per sequence token (every prefix a query)
SEQ_POOL = ("sum", "additive")  # --seqPool: the reference's sum over the tokens, or its dead AdditiveAttention applied
EDGE_TIME = ("none", "slot")   # --edgeTime: the reference's graph, or messages that add their edge's time-bucket row
RNN_CELL = ("lstm", "gru")      # --rnnCell: the reference's BasicLSTMCell, or the GRU its gru_cell() is named after
PRED_LOSS = ("hinge", "softmax")   # --predLoss: the reference's sampled hinge loss, or softmax over the whole catalogue
NEG_DIST = ("uniform", "pop")      # --softmaxNegDist: the uniform strata of --softmaxNegs, or a popularity-weighted draw


def seq_heads() -> int:
    """The head count of the sequence head's attention over tokens (_seq_att_full): --seqHeads, or --num_attention_heads
    when it is 0. Nothing else reads --seqHeads: the interval fusion and the collapsed head keep num_attention_heads."""
    return args.seqHeads or args.num_attention_heads


def random_fusion_params(d: int, device, seed: int = 0, cell: str = "lstm") -> dict:
    """Random-init fusion parameters with the shapes TF creates (BasicLSTMCell kernel [2d, 4d] and
    bias [4d]; layer_norm gamma/beta [d]; three dense kernels [d, d] with bias [d]). Kernels are
    xavier-uniform; biases/beta get small random values so benchmarks and tests exercise them.
    cell="gru": GRUCell's gate kernel [2d, 2d] / bias [2d] and candidate kernel [2d, d] / bias [d] in the LSTM's place."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)

    def xavier(r, c):
        lim = (6.0 / (r + c)) ** 0.5
        return (torch.rand((r, c), generator=g) * 2 * lim - lim).to(device)

    def small(n, mean=0.0):
        return (mean + 0.1 * torch.randn(n, generator=g)).to(device)

    if cell not in RNN_CELL:
        raise ValueError(f"cell {cell!r}: one of {RNN_CELL}")
    rnn = {"lstm_W": xavier(2 * d, 4 * d), "lstm_b": small(4 * d)} if cell == "lstm" else \
        {"gru_Wg": xavier(2 * d, 2 * d), "gru_bg": small(2 * d, 1.0), "gru_Wc": xavier(2 * d, d), "gru_bc": small(d)}
    return {**rnn, "ln_gamma": small(d, 1.0),
            "ln_beta": small(d), "Wq": xavier(d, d), "bq": small(d), "Wk": xavier(d, d), "bk": small(d),
            "Wv": xavier(d, d), "bv": small(d)}


def _flatten_sequences(seqs):
    """handler.sequence (one array per user) as one flat int64 array + int64 offsets [U + 1]."""
    lens = np.fromiter((len(q) for q in seqs), dtype=np.int64, count=len(seqs))
    ptr = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.asarray(q, dtype=np.int64).reshape(-1) for q in seqs]) if len(seqs) else np.zeros(0, np.int64)
    return flat, ptr


def _tst_as_int64(tstInt):
    """handler.tstInt (an item id or None per user) as int64, -1 for None."""
    return np.array([-1 if t is None else t for t in tstInt], dtype=np.int64)


def _right_aligned(flat, end, n, rows, P):
    """sequence int64 / mask float32 [rows, P]: row r holds the last min(n[r], P) of the n[r] items that end before
    flat[end[r]], right-aligned (the head's input layout, reference model.py:284-290 and :399-405)."""
    k = np.minimum(n, P)
    sequence = np.zeros((rows, P), dtype=np.int64)
    mask = np.zeros((rows, P), dtype=np.float32)
    r = np.repeat(np.arange(len(k), dtype=np.int64), k)
    within = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k)
    sequence[r, P - k[r] + within] = flat[end[r] - k[r] + within]
    mask[r, P - k[r] + within] = 1
    return sequence, mask


def _exclusions(flat, start, seq_end):
    """The full-ranking exclusion CSR: row r lists flat[start[r]:seq_end[r]] (the sequence the head reads), sorted.
    Returns rowptr int64 [n + 1] and the items (int64)."""
    rowptr = np.zeros(len(start) + 1, dtype=np.int64)
    np.cumsum(seq_end - start, out=rowptr[1:])
    items = np.concatenate([np.sort(flat[a:e]) for a, e in zip(start, seq_end)]) if len(start) else np.zeros(0, np.int64)
    return rowptr, items


def _rank_sums(rank, shoot):
    """One batch's HR / NDCG sums at shoot, 5 and 20 from its target ranks (-1 = a miss), as six floats."""
    res = []
    for k in (shoot, 5, 20):
        hit = (rank >= 0) & (rank < k)
        res += [float(hit.sum()), float((1.0 / np.log2(rank[hit] + 2)).sum())]
    return tuple(res)


def _metrics(tot, num):
    """The test epoch's dict from the float64 totals of _rank_sums over its num users."""
    return {"HR": tot[0] / num, "NDCG": tot[1] / num, "HR5": tot[2] / num, "NDCG5": tot[3] / num,
            "HR20": tot[4] / num, "NDCG20": tot[5] / num}


def _check_sequence_ids(flat, ptr, n_items: int):
    """ValueError for the first sequence id outside [0, n_items)."""
    bad = np.flatnonzero((flat < 0) | (flat >= n_items))
    if bad.size:
        u = int(np.searchsorted(ptr, bad[0], side="right") - 1)
        raise ValueError(f"sequence of user {u} holds item {int(flat[bad[0]])}, outside [0, {n_items})")


def banned_table(handler, n_items: int, flat=None, ptr=None):
    """The banned CSR of every user as host arrays (ban_ptr int64 [U + 1], ban_items int32): per user the sorted
    distinct items of its trnMat row (non-zero values), its last item and its test item, i.e. what the reference's
    negSamp never returns (DataHandler.py:28-41). The device sampler draws its negatives outside these lists and the
    full-catalogue softmax loss leaves them out of its sum. flat / ptr: _flatten_sequences(handler.sequence) when the
    caller holds it already."""
    if flat is None:
        flat, ptr = _flatten_sequences(handler.sequence)
    U, I = len(ptr) - 1, int(n_items)
    _check_sequence_ids(flat, ptr, I)
    lens = np.diff(ptr)
    # banned (user, item) keys: trnMat's non-zero entries, the last item, the test item
    trn = sp.csr_matrix(handler.trnMat, copy=True)
    trn.sum_duplicates()
    trn.eliminate_zeros()
    rows = [np.repeat(np.arange(trn.shape[0], dtype=np.int64), np.diff(trn.indptr))]
    cols = [trn.indices.astype(np.int64)]
    has = np.flatnonzero(lens > 0)
    rows.append(has)
    cols.append(flat[ptr[has + 1] - 1])
    tst = _tst_as_int64(handler.tstInt)
    tu = np.flatnonzero((tst >= 0) & (tst < I))
    rows.append(tu)
    cols.append(tst[tu])
    keys = np.unique(np.concatenate(rows) * I + np.concatenate(cols))
    ban_ptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // I, minlength=U)[:U], out=ban_ptr[1:])
    return ban_ptr, (keys % I).astype(np.int32)


def item_degrees(trn_mat, n_items: int) -> np.ndarray:
    """int64 [n_items]: the stored non-zero entries per column of trnMat (duplicates summed, explicit zeros dropped)."""
    trn = sp.csc_matrix(trn_mat, copy=True)
    trn.sum_duplicates()
    trn.eliminate_zeros()
    deg = np.zeros(int(n_items), dtype=np.int64)
    n = min(int(n_items), trn.shape[1])
    deg[:n] = np.diff(trn.indptr)[:n]
    return deg


def pop_cum(deg, a: float):
    """The integer mass of --softmaxNegDist pop: w_i = max(1, rint(2^20 (deg_i + 1)^a)) in float64 as int64, returned as
    (cum int64 [n_items], the inclusive prefix sum; W = cum[-1] as a Python int). Integer mass makes the stratified draw
    exact in 64-bit arithmetic, on the device and in its numpy restatement alike. Raises ValueError for an exponent
    outside [0, 1] and for W >= 2^62 (the draw's products j * (W / n_cand) must stay inside int64)."""
    a = float(a)
    if not np.isfinite(a) or not 0.0 <= a <= 1.0:
        raise ValueError(f"--softmaxNegPow {a}: need a finite exponent in [0, 1]")
    deg = np.asarray(deg, dtype=np.int64)
    if deg.ndim != 1 or deg.size < 1 or (deg < 0).any():
        raise ValueError("pop_cum: need one non-negative degree per item")
    w = np.maximum(1.0, np.rint(2.0 ** 20 * (deg.astype(np.float64) + 1.0) ** a))
    total = sum(int(v) for v in w) if float(w.sum()) >= 2.0 ** 61 else int(w.astype(np.int64).sum())
    if total >= 2 ** 62:
        raise ValueError(f"--softmaxNegDist pop: the total weight {total} reaches 2^62; lower --softmaxNegPow")
    return np.cumsum(w.astype(np.int64)), total


class DeviceSampler:
    """The per-dataset tables of the device sampler (sagnn_sample_train_i32 / sagnn_sample_ssl_i32), built and
    checked once on the host and kept on the device:
      - the flat sequences (seq_ptr int64 [U + 1] into seq_items int32);
      - the banned CSR (ban_ptr / ban_items): per user the sorted distinct items of its trnMat row (non-zero values),
        its last item and its test item, i.e. what the reference's negSamp never returns (DataHandler.py:28-41);
      - the canonical subMat rows (sub_ptr int64 [T, U + 1] into sub_items): distinct items with a non-zero value,
        the set the reference draws SSL pairs from (model.py:315, `toarray() != 0`);
      - per user `samp` (pairs of sampleTrainBatch) and per interval `npair` (pairs of sampleSslBatch).
    Raises ValueError for a sequence id outside [0, n_items) and for a user with pairs to draw but no allowed negative
    (the reference's rejection loop would never end there)."""

    def __init__(self, handler, device, n_items: int, train_sample_num: int, ssl_num: int):
        flat, ptr = _flatten_sequences(handler.sequence)
        U, I = len(ptr) - 1, int(n_items)
        lens = np.diff(ptr)
        _check_sequence_ids(flat, ptr, I)
        self.samp = np.clip(np.minimum(train_sample_num, lens - 1), 0, None)
        ban_ptr, ban_items = banned_table(handler, I, flat, ptr)
        full = np.flatnonzero((self.samp > 0) & (np.diff(ban_ptr) >= I))
        if full.size:
            raise ValueError(f"user {int(full[0])} has training pairs to draw but every item is banned for negatives")
        # canonical interval rows
        T = len(handler.subMat)
        sub_ptr = np.zeros((T, U + 1), dtype=np.int64)
        sub_items, base = [], 0
        self.npair = np.zeros((T, U), dtype=np.int64)
        for k, m in enumerate(handler.subMat):
            c = sp.csr_matrix(m, copy=True)
            c.sum_duplicates()
            c.eliminate_zeros()
            c.sort_indices()
            if c.shape[0] != U:
                raise ValueError(f"subMat[{k}] has {c.shape[0]} rows, {U} users")
            sub_ptr[k] = base + c.indptr.astype(np.int64)
            sub_items.append(c.indices.astype(np.int32))
            base += c.nnz
            self.npair[k] = np.minimum(ssl_num, np.diff(c.indptr) // 2)
        as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.n_users, self.n_items, self.train_sample_num, self.ssl_num = U, I, int(train_sample_num), int(ssl_num)
        self.seq_ptr, self.seq_items = as_dev(ptr), as_dev(flat.astype(np.int32))
        self.ban_ptr, self.ban_items = as_dev(ban_ptr), as_dev(ban_items)
        self.sub_ptr = as_dev(sub_ptr)
        self.sub_items = as_dev(np.concatenate(sub_items) if sub_items else np.zeros(0, np.int32))


class DeviceEvaluator:
    """The fixed inputs of a test epoch (testEpoch / testEpochFull) as tables, built once from the host path's own
    helpers (Recommender._test_batch, _masked_sum_csr, _exclusions) and kept on the device:
      - users int64 / uids int32 [n]: handler.tstUsrs, in order;
      - cand int32 [n, testSize]: the testSize - 1 negatives of test_dict, then the target LAST (sampleTestBatch);
      - target int32 [n]: tstInt (args.test) or the sequence's last item (validation);
      - chunks: per args.batch users (testEpoch's batches, same order) the start row, the user count and the head's
        masked-sum CSRs over args.batch slots (rowptr, item ids, positions), exactly what _masked_sum_plans uploads
        for that batch; on the device they become static SpmmPlans (plans) or, under --seqAtt full, the token arrays
        of the sequence attention (tokens, Recommender._csr_tokens);
      - the full-ranking exclusion CSR (excl_rowptr int64 / excl_items int32: each user's sequence items as the head
        reads them, sorted), checked once and uploaded once as an ops.ExclusionCSR (excl).
    Raises ValueError for a test_dict row shorter than testSize - 1 (as the host does), for candidate or target ids
    outside [0, n_items) (the host would read outside the item table), for a validation user with an empty sequence
    (the host would read the next user's first item as the target) and for testSize above the kernel's limit.
    With device=None only the host tables are built."""

    MAX_CANDIDATES = 8192      # sagnn_candidate_rank_f32's limit on C

    def __init__(self, rec, device=None):
        I, B = int(args.item), int(args.batch)
        if not 1 <= args.testSize <= self.MAX_CANDIDATES:
            raise ValueError(f"testSize = {args.testSize}: the device evaluator takes 1 .. {self.MAX_CANDIDATES}")
        users = np.asarray(rec.handler.tstUsrs, dtype=np.int64).reshape(-1)
        n = len(users)
        flat, ptr = rec._flat_sequences()
        rec._test_candidates()                   # a short test_dict row is reported first
        if not args.test:
            empty = np.flatnonzero(ptr[users + 1] == ptr[users])
            if empty.size:
                raise ValueError(f"user {int(users[empty[0]])} has an empty sequence: no validation target")
        self.chunks, parts = [], []
        for st in range(0, n, B):
            sequence, mask, start, seq_end, target, cand = rec._test_batch(users[st:st + B])
            self.chunks.append((st, len(target)) + Recommender._masked_sum_csr(sequence, mask))
            parts.append((start, seq_end, target, cand.astype(np.int32)))    # the negatives are int32 (test_dict table)
        start, seq_end, target, cand = ([np.concatenate(c) for c in zip(*parts)] if parts else
                                        [np.zeros(0, np.int64)] * 3 + [np.zeros((0, args.testSize), np.int32)])
        bad = np.flatnonzero((target < 0) | (target >= I))
        if bad.size:
            raise ValueError(f"target of test user {int(users[bad[0]])} is {int(target[bad[0]])}, outside [0, {I})")
        bad = np.argwhere((cand[:, :-1] < 0) | (cand[:, :-1] >= I))
        if bad.size:
            r, j = bad[0]
            raise ValueError(f"test_dict candidate {int(cand[r, j]) + 1} of user {int(users[r]) + 1} is outside [1, {I}]")
        self.n, self.n_items, self.batch = n, I, B
        self.users = users
        self.target = target.astype(np.int32)
        self.cand = cand
        self.excl_rowptr, excl = _exclusions(flat, start, seq_end)
        self.excl_items = excl.astype(np.int32)
        self.device = None
        if device is not None:
            self._upload(device)

    def _upload(self, device):
        as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        P = int(args.pos_length)
        self.device = device
        self.uids_d, self.users_d = as_dev(self.users.astype(np.int32)), as_dev(self.users)
        self.cand_d, self.target_d = as_dev(self.cand), as_dev(self.target)
        self.plans = self.tokens = None
        if args.seqAtt in SEQ_TOKEN_MODES:
            self.tokens = [Recommender._csr_tokens(rp, it, pos, device) for _, _, rp, it, pos in self.chunks]
        else:
            self.plans = [(ops.SpmmPlan(rp, it, self.batch, self.n_items, device=device, validate=False),
                           ops.SpmmPlan(rp, pos, self.batch, P, device=device, validate=False))
                          for _, _, rp, it, pos in self.chunks]
        self.excl = ops.ExclusionCSR(self.excl_rowptr, self.excl_items, self.n, self.n_items, device)


class Recommender:
    def __init__(self, sess, handler):
        self.sess = sess
        self.device = torch.device(sess if sess is not None else "cuda:0")
        self.handler = handler
        print("USER", args.user, "ITEM", args.item)
        self.metrics = dict()
        for met in ["Loss", "preLoss", "HR", "NDCG"]:
            self.metrics["Train" + met] = list()
            self.metrics["Test" + met] = list()

    # ------------------------------------------------------------------ hot-path pieces
    def messagePropagate(self, srclats, mat, type="user"):
        """reference model.py:80-92. `mat` is an IntervalAdj whose rows are the target nodes;
        `type` selected the row count in the reference (self.users / self.items) and is implied
        by mat.dense_shape[0] here. Registers the same dead, L2-regularised [d, d] weight the
        reference creates per call (FC(self.timeEmbed, latdim, reg=True), model.py:81)."""
        NNs.defineRandomNameParam([args.latdim, args.latdim], reg=True)
        expect = args.user if type == "user" else args.item
        if mat.dense_shape[0] != expect:
            raise ValueError(f"type={type!r} expects {expect} target rows, adjacency has {mat.dense_shape[0]}")
        return ops.spmm(mat.plan, srclats.detach(), NNs.leaky)

    def edgeDropout(self, mat):
        """reference model.py:93-102 rewrites edge VALUES only; messagePropagate never reads them
        (model.py:84-86), so the forward result is independent of keepRate and TF prunes the op.
        Identity here. Dropout that does reach the graph is opt-in and lives inside the SpMM kernels:
        --edgeKeepRate below 1 makes train_loss drop edges (ops.EdgeDrop); this method
        stays what the reference computes."""
        return mat

    def _define_fusion_params(self):
        d = args.latdim
        # tf.contrib.rnn.BasicLSTMCell(d) shared by users and items (model.py:135-144):
        # kernel [2d, 4d] glorot-uniform (TF's default initializer), bias zeros.
        if args.rnnCell == "gru":
            # --rnnCell gru: TF 1.14 GRUCell's four variables in the LSTM's place: both kernels
            # glorot-uniform, the gate bias 1.0 (GRUCell's bias_initializer default for r | u), the candidate bias zeros
            self.rnn_cell = {"gru_Wg": NNs.defineParam("rnn_gru_gates_kernel", [2 * d, 2 * d]),
                             "gru_bg": NNs.defineParam("rnn_gru_gates_bias", [2 * d], initializer="ones"),
                             "gru_Wc": NNs.defineParam("rnn_gru_candidate_kernel", [2 * d, d]),
                             "gru_bc": NNs.defineParam("rnn_gru_candidate_bias", [d], initializer="zeros")}
        else:
            self.lstm_kernel = NNs.defineParam("rnn_lstm_kernel", [2 * d, 4 * d])
            self.lstm_bias = NNs.defineParam("rnn_lstm_bias", [4 * d], initializer="zeros")
            self.rnn_cell = {"lstm_W": self.lstm_kernel, "lstm_b": self.lstm_bias}   # as ops.interval_fusion's p names them
        # two layer_norm calls -> separate gamma/beta (model.py:152-153)
        self.ln = []
        for tag in ("LayerNorm", "LayerNorm_1"):
            self.ln.append((NNs.defineParam(tag + "_gamma", [d], initializer="ones"),
                            NNs.defineParam(tag + "_beta", [d], initializer="zeros")))
        self.multihead_self_attention0 = MultiHeadSelfAttention(d, args.num_attention_heads)
        self.multihead_self_attention1 = MultiHeadSelfAttention(d, args.num_attention_heads)

    # T-fold layer scratch and masks of the batched stack stay below this many bytes (dataset-sized graphs: Gowalla's
    # scratch is 78 MB); above it every interval takes its own launches, which are long enough to hide their dispatch
    BATCH_SCRATCH_LIMIT = 8 << 30

    def _interval_batch(self):
        """ops.SpmmBatch over the T interval plans, or None when the T-fold scratch would be too large."""
        if self._batch is None and self._batch_ok is None:
            T, d = args.graphNum, args.latdim
            self._batch_ok = 2 * T * (args.user + args.item) * d * 4 <= self.BATCH_SCRATCH_LIMIT and T >= 1
            if self._batch_ok:
                self._batch = ops.SpmmBatch([a.plan for a in self.subAdj], [a.plan for a in self.subTpAdj])
        return self._batch

    def _stack_plans(self):
        """The (plans_user, plans_item) that ag.gnn_stack takes for this model: (the ops.SpmmBatch, None), or the two
        lists of T interval plans when the batch is off (_interval_batch)."""
        batch = self._interval_batch()
        if batch is not None:
            return batch, None
        return [a.plan for a in self.subAdj], [a.plan for a in self.subTpAdj]

    def time_tables(self):
        """TE [T, L, 2, M, d] = timeEmbed @ W of every messagePropagate call, in the registration order of the weights
        (interval, layer, user call, item call), as ONE batched matmul; None under --edgeTime none or
        without GNN layers. Differentiable: dTE reaches timeEmbed and the 2 T L weights through torch."""
        T, L, d = args.graphNum, args.gnn_layer, args.latdim
        if args.edgeTime != "slot" or L == 0:
            return None
        return torch.matmul(self.timeEmbed, torch.stack(self.time_weights).view(T, L, 2, d, d))

    def propagate_intervals(self, intervals=None):
        """reference model.py:118-134: for every interval k the L-layer stack with residuals and
        add_n, written straight into [N, T, d] slabs (no stack/transpose pass). `intervals`
        restricts the loop to a rank's shard (parallel.py); other columns are left untouched."""
        T, d, L = args.graphNum, args.latdim, args.gnn_layer
        if self.user_vector_tensor is None:
            self.user_vector_tensor = torch.empty((args.user, T, d), dtype=torch.float32, device=self.device)
            self.item_vector_tensor = torch.empty((args.item, T, d), dtype=torch.float32, device=self.device)
        batch = self._interval_batch() if (intervals is None and L > 0) else None
        te = self.time_tables()
        te = None if te is None else te.detach()
        if batch is not None:
            # every interval in one launch per layer (sagnn_gnn_stack_f32): the reference's loop over k is independent
            # per interval, and on dataset-sized graphs its 2 T L SpMMs are bound by their launches
            if L > 1 and (self._scratch_bu is None):
                self._scratch_bu = torch.empty((2, T, args.user, d), dtype=torch.float32, device=self.device)
                self._scratch_bi = torch.empty((2, T, args.item, d), dtype=torch.float32, device=self.device)
            ops.gnn_stack(batch, self.uEmbed.detach(), self.iEmbed.detach(), L, NNs.leaky,
                          self.user_vector_tensor.permute(1, 0, 2), self.item_vector_tensor.permute(1, 0, 2),
                          self._scratch_bu, self._scratch_bi, time=te)
            return self.user_vector_tensor, self.item_vector_tensor
        if L > 1 and self._scratch_u is None:
            self._scratch_u = torch.empty((2, args.user, d), dtype=torch.float32, device=self.device)
            self._scratch_i = torch.empty((2, args.item, d), dtype=torch.float32, device=self.device)
        for k in (range(T) if intervals is None else intervals):
            if L == 0:
                self.user_vector_tensor[:, k, :].copy_(self.uEmbed[k].detach())
                self.item_vector_tensor[:, k, :].copy_(self.iEmbed[k].detach())
                continue
            ops.gnn_interval(self.subAdj[k].plan, self.subTpAdj[k].plan, self.uEmbed[k].detach(),
                             self.iEmbed[k].detach(), L, NNs.leaky,
                             self.user_vector_tensor[:, k, :], self.item_vector_tensor[:, k, :],
                             self._scratch_u, self._scratch_i, time=None if te is None else te[k])
        return self.user_vector_tensor, self.item_vector_tensor

    def fuse_intervals(self, user_vector_tensor, item_vector_tensor):
        """reference model.py:135-155: shared LSTM, per-type layer_norm + MHSA, mean over T."""
        heads = args.num_attention_heads
        outs = []
        for x, (gamma, beta), att in ((user_vector_tensor, self.ln[0], self.multihead_self_attention0),
                                      (item_vector_tensor, self.ln[1], self.multihead_self_attention1)):
            p = {**{k: v.detach() for k, v in self.rnn_cell.items()}, "ln_gamma": gamma.detach(), "ln_beta": beta.detach()}
            p.update({k: v.detach() for k, v in att.weights().items()})
            outs.append(ops.interval_fusion(x, p, heads))
        return outs[0], outs[1]

    def ours(self):
        """The hot path of reference model.py:104-155. Returns (final_user_vector [U, d],
        final_item_vector [I, d]); the reference's (preds, sslloss) are built on top of these by
        the head / SSL branch (model.py:156-205), outside this build's scope."""
        T, d = args.graphNum, args.latdim
        self.uEmbed = NNs.defineParam("uEmbed", [T, args.user, d], reg=True)
        self.iEmbed = NNs.defineParam("iEmbed", [T, args.item, d], reg=True)
        self.posEmbed = NNs.defineParam("posEmbed", [args.pos_length, d], reg=True)
        self.timeEmbed = NNs.defineParam("timeEmbed", [self.maxTime + 1, d], reg=True)
        # one [d, d] weight per messagePropagate call: 2*T*L of them (model.py:81, :122-123), in the order (interval,
        # layer, user call, item call). Dead in the reference and under --edgeTime none; --edgeTime slot reads them
        self.time_weights = [NNs.defineRandomNameParam([d, d], reg=True) for _ in range(2 * T * args.gnn_layer)]
        self._define_fusion_params()
        self._define_head_params()
        self._define_ssl_params()
        self._define_seq_pool_params()
        self._define_seq_ffn_params()
        return self.forward()

    def _define_seq_ffn_params(self):
        """The position-wise feed-forward blocks of --seqFFN F, one per attention layer of the token head:
        a layer norm (gamma ones, beta zeros), W1 [d, F] and W2 [F, d] with the default initialiser and zero biases; none
        L2-regularised, like the MHSA kernels. Defined after every other variable, so those start where they start under
        --seqFFN 0; nothing is defined at 0."""
        self.seq_ffn = []
        if args.seqFFN <= 0:
            return
        d, F = args.latdim, args.seqFFN
        for i in range(args.att_layer):
            n = f"seq_ffn{i}_"
            self.seq_ffn.append((NNs.defineParam(n + "ln_gamma", [d], initializer="ones"),
                                 NNs.defineParam(n + "ln_beta", [d], initializer="zeros"),
                                 NNs.defineParam(n + "W1", [d, F]), NNs.defineParam(n + "b1", [F], initializer="zeros"),
                                 NNs.defineParam(n + "W2", [F, d]), NNs.defineParam(n + "b2", [d], initializer="zeros")))

    def _define_seq_pool_params(self):
        """The additive-attention pooling of --seqPool additive (the reference's additive_attention0, model.py:147, whose
        call model.py:168 comments out): a tf.layers.dense kernel and bias, not L2-regularised like the MHSA
        kernels, and the query vector, here a trained variable (Utils/attention.py:9 re-draws a tensor per run). Defined
        after every other variable, so those start where they start under --seqPool sum; nothing is defined under sum."""
        self.additive_attention0 = None
        if args.seqPool != "additive":
            return
        d, q = args.latdim, args.query_vector_dim
        Wa = NNs.defineParam("additive_attention0_kernel", [d, q])
        ba = NNs.defineParam("additive_attention0_bias", [q], initializer="zeros")
        query = torch.rand(q, generator=NNs._generator, dtype=torch.float32) * 0.2 - 0.1
        self.additive_attention0 = (Wa, ba, NNs.defineParam("additive_attention0_query", [q], initializer=query))

    def _define_ssl_params(self):
        """The SSL meta-net (model.py:179-182): FC(3d -> ssldim, bias, leakyRelu, reg) named 'meta2'
        and FC(ssldim -> 1, bias, sigmoid, reg) named 'meta3', shared by all intervals; biases are
        zeros and not L2-regularised (Utils/NNLayers.py:117-124)."""
        d = args.latdim
        self.meta2_W = NNs.defineParam("meta2", [3 * d, args.ssldim], reg=True)
        self.meta2_b = NNs.defineParam("meta2Bias", [args.ssldim], initializer="zeros")
        self.meta3_W = NNs.defineParam("meta3", [args.ssldim, 1], reg=True)
        self.meta3_b = NNs.defineParam("meta3Bias", [1], initializer="zeros")

    def _define_head_params(self):
        """Variables of the prediction head in the reference's creation order (model.py:158-166):
        att_layer MHSA instances, then layer_norm gamma/beta pairs LayerNorm_2 (item-sequence
        token), LayerNorm_3 (position token), LayerNorm_4.. (one per attention layer)."""
        d = args.latdim
        self.multihead_self_attention_sequence = [MultiHeadSelfAttention(d, args.num_attention_heads)
                                                  for _ in range(args.att_layer)]
        self.head_ln = []
        for i in range(2 + args.att_layer):
            tag = "LayerNorm_%d" % (2 + i)
            self.head_ln.append((NNs.defineParam(tag + "_gamma", [d], initializer="ones"),
                                 NNs.defineParam(tag + "_beta", [d], initializer="zeros")))

    def forward(self):
        """Re-runs the hot path with the current parameters (what every sess.run recomputes)."""
        uvt, ivt = self.propagate_intervals()
        self.final_user_vector, self.final_item_vector = self.fuse_intervals(uvt, ivt)
        return self.final_user_vector, self.final_item_vector

    def capture_forward(self, warmup: int = 2):
        """Captures forward() into a hipGraph (torch.cuda.CUDAGraph) and returns a replay callable.
        Real datasets are launch-bound on MI355X (each SpMM is tens of microseconds): one graph
        launch replaces 2*T*L + 4 kernel launches. Outputs land in the same tensors every replay
        (self.final_user_vector / self.final_item_vector); parameters are read in place."""
        for _ in range(max(warmup, 1)):      # first call configures kernels / allocates workspaces
            self.forward()
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.forward()

        def replay():
            graph.replay()
            return self.final_user_vector, self.final_item_vector

        self._graph = graph
        return replay

    # ------------------------------------------------------------------ prediction head
    @staticmethod
    def _masked_sum_csr(sequence, mask):
        """The CSRs of the masked sums of model.py:161-162: row b lists the unmasked entries of the batch slot's
        sequence. Returns rowptr int32 [B + 1], their item ids and their positions (int32)."""
        sequence = np.asarray(sequence, dtype=np.int64)
        keep = np.asarray(mask) != 0
        B, L = keep.shape
        rowptr = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(keep.sum(1), out=rowptr[1:])
        items = sequence[keep].astype(np.int32)
        pos = np.ascontiguousarray(np.broadcast_to(np.arange(L, dtype=np.int32), (B, L))[keep])
        return rowptr, items, pos

    def _masked_sum_plans(self, sequence, mask):
        """Per-batch plans for the masked sums of model.py:161-162 (item ids, and positions)."""
        rowptr, items, pos = self._masked_sum_csr(sequence, mask)
        B, L = np.asarray(mask).shape
        pi = ops.SpmmPlan(rowptr, items, B, args.item, device=self.device, validate=False)
        pp = ops.SpmmPlan(rowptr, pos, B, L, device=self.device, validate=False)
        return pi, pp

    def predict(self, uids, iids, sequence, mask, uLocs_seq):
        """self.preds of the reference (model.py:156-173) for one batch, on the cached
        final_user_vector / final_item_vector. sequence/mask: [args.batch, pos_length]."""
        fu, fi = self.final_user_vector, self.final_item_vector
        att = self._head_att(sequence, mask)
        return ops.pair_score(fu, fi, self._i32(uids), self._i32(iids), S=att, A=fi, locs=self._i32(uLocs_seq),
                              leaky=NNs.leaky)

    def _head_att(self, sequence, mask):
        """The head's sequence representation att [args.batch, d] (model.py:158-168) on the cached final vectors."""
        if args.seqAtt in SEQ_TOKEN_MODES:
            return self._head_att_tokens(*self._csr_tokens(*self._masked_sum_csr(sequence, mask), self.device))
        return self._head_att_plans(*self._masked_sum_plans(sequence, mask))

    @staticmethod
    def _csr_tokens(rowptr, items, pos, device):
        """_masked_sum_csr's arrays as the token description of the sequence attention, on the device: (item ids
        int32, positions int32, seg_begin int64 [B] = rowptr[:-1], seg_len int32 [B] = diff(rowptr))."""
        as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return (as_dev(items), as_dev(pos), as_dev(rowptr[:-1].astype(np.int64)), as_dev(np.diff(rowptr).astype(np.int32)))

    def _seq_att_full(self, fi, seq_items, seq_pos, seg_begin, seg_len, pooled=True):
        """--seqAtt full / causal (not in the reference's graph): att [args.batch, d] with every item of a slot's
        sequence a token and the att_layer attention layers run over the slot's real tokens, as the attn_mask of
        Utils/attention.py:35-45 would have it. Token j of slot b is item seq_items[seg_begin[b] + j] at position
        seq_pos[...] (None: right-aligned); activations are padded slabs [args.batch * pos_length, d]. The one place
        that builds it: differentiable in fi and the head's parameters (train_loss), and called without a graph by the
        inference paths. Same variables as the collapsed head. Under causal a token attends to itself and the tokens
        before it. pooled=False returns the last layer's slab [args.batch * pos_length, d] instead of the pooled rows
        (--seqTargets all)."""
        heads, leaky, P = seq_heads(), NNs.leaky, args.pos_length
        mask = (True,) if args.seqAtt == "causal" else ()     # full: SeqAttnFn's call stays what it was
        seq, pos = ag.SeqGatherFn.apply(fi, self.posEmbed, seq_items, seq_pos, seg_begin, seg_len)
        R, d = seq.shape
        ln = lambda x, gb: ag.LayerNormFn.apply(x.view(R, 1, d), gb[0], gb[1]).view(R, d)
        x = ag.LeakyAddFn.apply(ln(seq, self.head_ln[0]), ln(pos, self.head_ln[1]), 1.0)
        for i, mh in enumerate(self.multihead_self_attention_sequence):
            w = mh.weights()
            x = ag.SeqAttnFn.apply(x, *self.head_ln[2 + i], w["Wq"], w["bq"], w["Wk"], w["bk"], w["Wv"], w["bv"], seg_len, P,
                                   heads, leaky, *mask)
            if args.seqFFN > 0:                               # --seqFFN: the block's second half
                x = ag.SeqFfnFn.apply(x, *self.seq_ffn[i], seg_len, P, leaky)
        if not pooled:
            return x
        if args.seqPool == "additive":
            return ag.SeqAddPoolFn.apply(x, *self.additive_attention0, seg_len, P)
        return ag.SeqPoolFn.apply(x, seg_len, P)

    def _head_att_tokens(self, seq_items, seq_pos, seg_begin, seg_len):
        """_head_att under --seqAtt full, on the batch's token arrays (_csr_tokens): _seq_att_full without a graph."""
        with torch.no_grad():
            return self._seq_att_full(self.final_item_vector, seq_items, seq_pos, seg_begin, seg_len)

    def _head_att_plans(self, pi, pp):
        """_head_att on the masked-sum plans of the batch (item ids pi, positions pp)."""
        heads, leaky = args.num_attention_heads, NNs.leaky
        fi = self.final_item_vector
        seq_tok = ops.spmm(pi, fi, 1.0)                                   # [B, d] masked item sum
        pos_tok = ops.spmm(pp, self.posEmbed.detach(), 1.0)               # [B, d] masked position sum
        B, d = seq_tok.shape
        ln = lambda x, gb: ops.layernorm_td(x.view(B, 1, d), gb[0].detach(), gb[1].detach()).view(B, d)
        att = ops.leaky_add(ln(seq_tok, self.head_ln[0]), ln(pos_tok, self.head_ln[1]), 1.0)
        for i, mh in enumerate(self.multihead_self_attention_sequence):
            a1 = mh.attention_mean(ln(att, self.head_ln[2 + i]).view(B, 1, d))      # length-1 sequence
            att = ops.leaky_add(a1, att, leaky)
        return att

    def _query_rows(self, uids, sequence, mask):
        """The head's user-side row q[b] = leaky(att[b]) + fu[uids[b]]: the head score of (uids[b], i) is
        <fu[u], fi[i]> + <leaky(att[b]), fi[i]> = <q[b], fi[i]> (model.py:169-170), so ranking the whole catalogue
        is one product of these rows with final_item_vector."""
        uids = torch.as_tensor(np.asarray(uids, dtype=np.int64), device=self.device)
        att = self._head_att(sequence, mask)[:uids.numel()]
        return ops.leaky_add(att, self.final_user_vector.index_select(0, uids), NNs.leaky)

    def _test_sequences(self, batIds):
        """The sequences sampleTestBatch feeds the head: the user's whole sequence (args.test) or all but its last
        item (validation), the last min(len, pos_length) items right-aligned. Returns sequence, mask [args.batch,
        pos_length], and per user the flat range [start, seq_end) the sequence was cut from."""
        batIds = np.asarray(batIds, dtype=np.int64)
        flat, ptr = self._flat_sequences()
        start, end = ptr[batIds], ptr[batIds + 1]
        seq_end = end if args.test else np.maximum(end - 1, start)
        sequence, mask = _right_aligned(flat, seq_end, seq_end - start, args.batch, args.pos_length)
        return sequence, mask, start, seq_end

    def _test_batch(self, batIds):
        """The inputs of a test batch for both evaluators: _test_sequences' four arrays, the target int64 [n] (tstInt, -1
        for None; in validation the held-out item flat[seq_end]) and the candidates int64 [n, testSize]: test_dict's
        testSize - 1 negatives (users outside tstUsrs read the dict itself), then the target LAST."""
        batIds = np.asarray(batIds, dtype=np.int64)
        sequence, mask, start, seq_end = self._test_sequences(batIds)
        target = self._tst_ids()[batIds] if args.test else self._flat_sequences()[0][seq_end]
        neg_all, row_of = self._test_candidates()
        rows = row_of[batIds]
        if (rows < 0).any():                                      # not a test user: fall back to the dict
            neg = np.stack([np.asarray(self.handler.test_dict[int(u) + 1][:args.testSize - 1], dtype=np.int64) - 1
                            for u in batIds])
        else:
            neg = neg_all[rows].astype(np.int64)
        return sequence, mask, start, seq_end, target, np.concatenate([neg, target[:, None]], axis=1)

    def _cached(self, name, key, build):
        """build()'s value, kept in attribute `name` as (signature, value, key) until `key` changes: objects compare by
        identity (the entry holds them, so ids are not reused), flags by value. The old value goes before build() runs."""
        sig = tuple(k if isinstance(k, (bool, int, float, str)) else id(k) for k in key)
        entry = getattr(self, name, None)
        if entry is None or entry[0] != sig:
            setattr(self, name, None)
            entry = (sig, build(), key)
            setattr(self, name, entry)
        return entry[1]

    def _flat_sequences(self):
        """_flatten_sequences(handler.sequence), built once."""
        return self._cached("_seq_cache", (self.handler.sequence,), lambda: _flatten_sequences(self.handler.sequence))

    def _tst_ids(self):
        """_tst_as_int64(handler.tstInt), built once."""
        return self._cached("_tst_ids_cache", (self.handler.tstInt,), lambda: _tst_as_int64(self.handler.tstInt))

    def _test_candidates(self):
        """test_dict (1-indexed user -> 1-indexed candidate items, preprocess_to_sequence.ipynb cell 11) as one int32
        matrix [test users, testSize - 1] of 0-indexed negatives + the row of every user in it; built once (the
        reference re-reads the dict per user and batch: 25 ms of list -> array conversions per 512-user batch)."""
        h = self.handler

        def build():
            users = np.asarray(h.tstUsrs, dtype=np.int64)
            row_of = np.full(args.user, -1, dtype=np.int64)
            row_of[users] = np.arange(len(users))
            k = args.testSize - 1
            neg = np.empty((len(users), k), dtype=np.int32)
            for r, u in enumerate(users):
                cand = h.test_dict[int(u) + 1][:k]
                if len(cand) != k:
                    raise ValueError(f"test_dict[{int(u) + 1}] holds {len(cand)} candidates, testSize - 1 = {k} needed")
                neg[r] = cand
            neg -= 1
            return neg, row_of
        return self._cached("_tst_cache", (h.test_dict, h.tstUsrs, args.user, args.testSize), build)

    def sampleTestBatch(self, batIds, labelMat=None):
        """reference model.py:384-428: args.testSize-1 pre-drawn negatives from test_dict
        (1-indexed user keys and item ids) plus the held-out positive LAST; the user's whole
        sequence, right-aligned into pos_length slots (_test_batch)."""
        batIds = np.asarray(batIds, dtype=np.int64)
        temTst = self.handler.tstInt[batIds]
        sequence, mask, _, _, target, locs = self._test_batch(batIds)
        val_list = [None] * args.batch
        if not args.test:
            for i, t in enumerate(target.tolist()):              # last item held out for validation
                val_list[i] = t
        C = locs.shape[1]
        uLocs = np.repeat(batIds, C)
        uLocs_seq = np.repeat(np.arange(len(batIds), dtype=np.int64), C)
        return uLocs, locs.reshape(-1), temTst, list(locs), sequence, mask, uLocs_seq, val_list

    @staticmethod
    def calcRes(preds, temTst, tstLocs, shoot=None):
        """reference model.py:484-510 without the sort. The reference ranks the candidates by a stable
        descending sort (ties keep candidate order; the positive is the LAST candidate, so it loses them) and
        takes `list.index(target)` in the top k, i.e. the best-ranked copy of the target item (a pre-drawn
        negative may be the same item). That rank is  #(pred > p) + #(earlier candidates with pred == p)  for
        p = the copies' highest score, j = its first copy — counted directly, O(candidates) per user instead of
        an argsort of [batch, testSize] (15 ms per batch: 80 % of a test epoch)."""
        shoot = args.shoot if shoot is None else shoot
        # a NaN score never outranks anything: under the reference's sort a NaN positive (the LAST candidate) stays
        # last, i.e. a miss — left as NaN, p_best would compare False everywhere and count as rank 0 (a diverged
        # model would report HR = 1)
        preds = np.where(np.isnan(preds), -np.inf, preds)
        locs = np.stack([np.asarray(t) for t in tstLocs])                      # [B, C]
        B, C = locs.shape
        target = np.asarray([(-1 if t is None else t) for t in temTst[:B]])[:, None]
        copies = locs == target
        has = copies.any(1)
        p_best = np.where(copies, preds, -np.inf).max(1)                       # highest score among the copies
        first = (copies & (preds == p_best[:, None])).argmax(1)                 # its first candidate index
        ahead = (preds > p_best[:, None]).sum(1) + ((preds == p_best[:, None]) & (np.arange(C)[None, :] < first[:, None])).sum(1)
        return _rank_sums(np.where(has, ahead, -1), shoot)

    def testEpoch(self):
        """reference model.py:430-482. The hot path is evaluated ONCE (parameters are frozen and
        keepRate = 1 during testing, model.py:458) instead of once per batch. args.evaluator = "device" runs
        _test_epoch_device (the same dict)."""
        if args.evaluator == "device":
            return self._test_epoch_device(full=False)
        self.forward()
        ids = self.handler.tstUsrs
        num = len(ids)
        tot = np.zeros(6)
        for st in range(0, num, args.batch):
            batIds = ids[st:st + args.batch]
            uLocs, iLocs, temTst, tstLocs, sequence, mask, uLocs_seq, val_list = self.sampleTestBatch(batIds)
            preds = self.predict(uLocs, iLocs, sequence, mask, uLocs_seq).cpu().numpy()
            target = temTst if args.test else val_list
            tot += np.array(self.calcRes(preds.reshape(len(batIds), -1), target, tstLocs))
        return _metrics(tot, num)

    def recommend(self, uids, k=None, exclude_seen=True):
        """The k best items of the whole catalogue for each user (sagnn_score_topk_f32 on _query_rows), on the cached
        final vectors (run forward() first). The head reads each user's sequence as sampleTestBatch builds it;
        exclude_seen leaves out the user's training items (handler.trnMat row). Returns numpy (items int32,
        scores float32), both [len(uids), k], best first; -1 / -inf where fewer than k items are eligible."""
        k = args.shoot if k is None else int(k)
        uids = np.asarray(uids, dtype=np.int64).reshape(-1)
        items, scores = [], []
        for st in range(0, len(uids), args.batch):
            bat = uids[st:st + args.batch]
            sequence, mask, _, _ = self._test_sequences(bat)
            excl = None
            if exclude_seen:
                rows = self.handler.trnMat[bat].tocsr()
                rows.sort_indices()
                excl = (rows.indptr, rows.indices)
            it, sc, _ = ops.score_topk(self._query_rows(bat, sequence, mask), self.final_item_vector, k, excl=excl)
            items.append(it.cpu().numpy())
            scores.append(sc.cpu().numpy())
        if not items:
            return np.zeros((0, k), np.int32), np.zeros((0, k), np.float32)
        return np.concatenate(items), np.concatenate(scores)

    def testEpochFull(self):
        """Full-catalogue HR / NDCG at shoot, 5 and 20: testEpoch()'s users, targets and batches, with the target
        ranked against every item instead of testSize - 1 sampled ones. A user's exclusions are the items of the
        sequence its head reads (the target stays eligible: sagnn_score_topk_f32 never excludes it). Same keys and
        normalisation as testEpoch(); forward() runs once. args.evaluator = "device" runs _test_epoch_device."""
        if args.evaluator == "device":
            return self._test_epoch_device(full=True)
        self.forward()
        ids = self.handler.tstUsrs
        num = len(ids)
        flat, _ = self._flat_sequences()
        tot = np.zeros(6)
        for st in range(0, num, args.batch):
            batIds = np.asarray(ids[st:st + args.batch], dtype=np.int64)
            sequence, mask, start, seq_end, target, _ = self._test_batch(batIds)
            _, _, rank = ops.score_topk(self._query_rows(batIds, sequence, mask), self.final_item_vector, 1,
                                        excl=_exclusions(flat, start, seq_end), target=target.astype(np.int32))
            tot += np.array(_rank_sums(rank.cpu().numpy(), args.shoot))
        return _metrics(tot, num)

    def _device_evaluator(self) -> DeviceEvaluator:
        """The device evaluator's tables for the current handler and flags, built once."""
        h = self.handler
        key = (h.sequence, h.test_dict, h.tstInt, h.tstUsrs, bool(args.test), args.testSize, args.pos_length, args.batch,
               args.item, str(self.device), args.seqAtt)
        return self._cached("_dev_eval", key, lambda: DeviceEvaluator(self, self.device))

    def _test_epoch_device(self, full: bool):
        """testEpoch (full=False) or testEpochFull (full=True) on the device evaluator's tables: forward() once, then
        per batch of testEpoch the head on the static plans and one ranking launch (sagnn_candidate_rank_f32 on the
        sampled candidates, or sagnn_score_topk_f32 over the catalogue); the ranks come back in one copy."""
        E = self._device_evaluator()
        self.forward()
        fu, fi, leaky = self.final_user_vector, self.final_item_vector, NNs.leaky
        ranks = []
        for c, (st, nb, _, _, _) in enumerate(E.chunks):
            att = (self._head_att_tokens(*E.tokens[c]) if E.tokens is not None else self._head_att_plans(*E.plans[c]))[:nb]
            if full:
                q = ops.leaky_add(att, fu.index_select(0, E.users_d[st:st + nb]), leaky)
                _, _, r = ops.score_topk(q, fi, 1, excl=E.excl.rows(st, st + nb), target=E.target_d[st:st + nb])
            else:
                r, _ = ops.candidate_rank(fu, fi, E.uids_d[st:st + nb], E.cand_d[st:st + nb], E.target_d[st:st + nb],
                                          S=att, A=fi, leaky=leaky)
            ranks.append(r)
        rank = torch.cat(ranks).cpu().numpy() if ranks else np.zeros(0, np.int64)
        return self._rank_metrics(rank, E.batch)

    @staticmethod
    def _rank_metrics(rank, batch):
        """HR / NDCG at shoot, 5 and 20 from the target ranks of every test user (-1 = a miss), summed per batch of
        `batch` users in float64 with the helpers of testEpoch and testEpochFull, so the dict equals theirs."""
        tot = np.zeros(6)
        for st in range(0, len(rank), batch):
            tot += np.array(_rank_sums(rank[st:st + batch], args.shoot))
        return _metrics(tot, len(rank))

    # ------------------------------------------------------------------ training
    def _i32(self, v):
        if isinstance(v, torch.Tensor):          # a device-sampled batch: int32 on the device already
            return v.to(self.device, torch.int32)
        return torch.as_tensor(np.asarray(v, dtype=np.int32), device=self.device)

    def train_loss(self, batch, keep_rate=None, edge_keep=None):
        """The reference's loss for one step (model.py:104-205, 241-246) as a torch autograd graph
        whose nodes are HIP operators (sa_gnn_amd.autograd). batch: dict with uids, iids,
        uLocs_seq, sequence [args.batch, pos_length], mask, suids[k], siids[k]; a device-sampled batch
        (sample_batch_device) carries seq_seg = (seg_begin, seg_len) instead of sequence / mask. Returns
        (preLoss, sslloss) as 1-element tensors; total loss = preLoss + ssl_reg*sslloss (+ the L2
        term, applied inside the optimiser step). Under --fusion_rows batch the interval fusion runs on the rows the
        loss reads only (_touched_rows, autograd.interval_fusion_rows); fu / fi stay full-size with zero rows elsewhere.
        With an edge keep rate below 1 (edge_keep, default args.edgeKeepRate) the GNN stack drops edges, forward and
        backward alike, keyed by batch["edge_seed"] = (seed, step) (default (0, 0)); every other entry point of the
        model (forward, evaluators, recommend, parallel) never drops.
        Under --predLoss softmax preLoss is the full-catalogue softmax cross-entropy of every active slot's positive
        (_softmax_pre_loss) and the batch's sampled negatives are not read. The flag is not part of the model: the
        variables are the same, and checkpoints neither store nor check it. With --softmaxNegs N > 0 the softmax runs
        over N candidates shared by the batch, drawn on the device at the top of the step (ops.sample_strata keyed by
        batch["cand_seed"] = (seed, step), default (0, 0)) under either sampler, plus each slot's own target; under
        --fusion_rows batch the candidates are marked as touched item rows. Under --softmaxNegDist pop the N candidates are
        a popularity-weighted draw with repeats (ops.sample_strata_weighted over _pop_cum_device) and batch["cand_bias"]
        carries their logQ offsets; nothing else in the step differs.
        Under --seqTargets all (with --seqAtt causal) the softmax loss runs on every real token of every
        active slot instead of the slot's pooled row (_softmax_pre_loss_all); like the loss flags it is not part of the model."""
        T, L, d, heads, leaky = args.graphNum, args.gnn_layer, args.latdim, args.num_attention_heads, NNs.leaky
        keep = args.keepRate if keep_rate is None else keep_rate
        subset = args.fusion_rows == "batch"
        if args.predLoss == "softmax" and args.softmaxNegs > 0:
            if args.softmaxNegDist == "pop":     # the same seed, the same place in the step
                cand, bias = ops.sample_strata_weighted(*self._pop_cum_device(), args.softmaxNegs,
                                                        *batch.get("cand_seed", (0, 0)))
                batch = dict(batch, cand=cand, cand_bias=bias)
            else:
                batch = dict(batch, cand=ops.sample_strata(args.item, args.softmaxNegs, *batch.get("cand_seed", (0, 0)),
                                                           self.device))
        if subset:        # the rows the loss reads, compacted on the device before the GNN stack is queued
            batch = dict(batch, uids=self._i32(batch["uids"]), iids=self._i32(batch["iids"]),
                         suids=[self._i32(v) for v in batch["suids"]], siids=[self._i32(v) for v in batch["siids"]])
            touched = self._touched_rows(batch)
        # one autograd node for the whole interval loop; uv / iv are [T, N, d] slabs written in place
        edge_keep = args.edgeKeepRate if edge_keep is None else edge_keep
        edge_drop = ops.EdgeDrop(*batch.get("edge_seed", (0, 0)), edge_keep) if edge_keep < 1.0 else None
        if edge_drop is not None and args.edgeTime != "none":
            raise ValueError("an edge keep rate below 1 does not combine with --edgeTime slot")
        uv, iv = ag.gnn_stack(self.uEmbed, self.iEmbed, *self._stack_plans(), L, leaky, drop=edge_drop, TE=self.time_tables())
        finals = []
        if subset:        # the one read-back of the step: the two counts, copied while the stack's launches queue
            touched["done"].synchronize()
            counts = [int(v) for v in touched["host"]]
            for side, n, c in zip(("users", "items"), counts, touched["caps"]):
                if n > c:
                    raise RuntimeError(f"fusion_rows: {n} touched {side} exceed the capacity {c}")
            self.fusion_rows_counts = tuple(counts)
        for side, (xs, (gamma, beta), att, key) in enumerate(((uv, self.ln[0], self.multihead_self_attention0, "drop_u"),
                                                              (iv, self.ln[1], self.multihead_self_attention1, "drop_i"))):
            x = xs.permute(1, 0, 2)                                       # [N, T, d] view of [T, N, d]: no copy
            drop = batch.get(key)
            if drop is not None and drop.device != x.device:              # the kernels take its pointer as it is
                raise ValueError(f'batch["{key}"] is on {drop.device}, the model on {x.device}')
            # the slots the fusion runs on: at least one, so that an empty set still runs (on padding, to zeros)
            n_run = max(counts[side], 1) if subset else x.shape[0]
            if drop is None and keep < 1.0:                               # DropoutWrapper(output_keep_prob)
                drop = (torch.rand((n_run, T, d), device=self.device) < keep).float() / keep
            p = {**self.rnn_cell, "ln_gamma": gamma, "ln_beta": beta}
            p.update(att.weights())
            if subset:
                rows, count = touched["rows"][side]
                finals.append(ag.interval_fusion_rows(x, rows, count, n_run, p, heads, drop_scale=drop))
            else:
                finals.append(ag.interval_fusion(x, p, heads, drop_scale=drop))
        fu, fi = finals
        # ---- head (model.py:156-173)
        tokens = None
        if args.seqAtt in SEQ_TOKEN_MODES:                                # every sequence item a token (_seq_att_full)
            if "seq_seg" in batch:
                tokens = (self._device_sampler().seq_items, None) + tuple(batch["seq_seg"])
            else:
                tokens = self._csr_tokens(*self._masked_sum_csr(batch["sequence"], batch["mask"]), self.device)
            att = self._seq_att_full(fi, *tokens, pooled=args.seqTargets != "all")       # all: the slab before pooling
        else:
            att = self._head_att_sum_train(fi, batch)
        if args.predLoss == "softmax" and args.seqTargets == "all":
            pre_loss = self._softmax_pre_loss_all(fu, fi, att, batch, tokens)
        elif args.predLoss == "softmax":
            pre_loss = self._softmax_pre_loss(fu, fi, att, batch)
        else:
            preds = ag.PairScoreFn.apply(fu, fi, att, self._i32(batch["uids"]), self._i32(batch["iids"]),
                                         self._i32(batch["uLocs_seq"]), leaky)
            n = preds.shape[0] // 2
            pre_loss = ag.HingeFn.apply(preds[:n], preds[n:], None, None, None, None, 1.0 / max(n, 1))
        # ---- SSL (model.py:174-205)
        ssl = torch.zeros(1, dtype=torch.float32, device=self.device)
        for k in range(T):
            if len(batch["suids"][k]) < 2:
                continue
            su, si = self._i32(batch["suids"][k]), self._i32(batch["siids"][k])
            ns = su.numel() // 2
            w = ag.MetaWeightFn.apply(fu, uv[k], su, self.meta2_W, self.meta2_b, self.meta3_W, self.meta3_b, leaky)
            s_final = ag.ProdLeakySumFn.apply(fu.detach(), fi.detach(), su, si, leaky)      # stop_gradient
            p1 = ag.ProdLeakySumFn.apply(uv[k], iv[k], su, si, leaky)
            ssl = ssl + ag.HingeFn.apply(p1[:ns], p1[ns:], w[:ns], w[ns:], s_final[:ns], s_final[ns:], 1.0)
        return pre_loss, ssl

    def _banned_device(self):
        """banned_table of the current handler as device tensors (ptr int64, items int32), built once."""
        h = self.handler

        def build():
            ptr, items = banned_table(h, args.item)
            items = items if items.size else np.zeros(1, np.int32)       # an empty table still needs a valid pointer
            return torch.from_numpy(ptr).to(self.device), torch.from_numpy(items).to(self.device)
        return self._cached("_banned_dev", (h.sequence, h.trnMat, h.tstInt, args.item, str(self.device)), build)

    def _pop_cum_device(self):
        """--softmaxNegDist pop: (cum int64 [items] on the device, W) of pop_cum over the stored non-zero entries per
        column of the handler's trnMat, built and uploaded once."""
        h = self.handler

        def build():
            cum, total = pop_cum(item_degrees(h.trnMat, args.item), args.softmaxNegPow)
            return torch.from_numpy(cum).to(self.device), total
        return self._cached("_pop_cum_dev", (h.trnMat, args.item, float(args.softmaxNegPow), str(self.device)), build)

    def _active_slots(self, batch):
        """The (slot, user, target) triples of the positive half of a batch, without a read-back: device tensors (slots
        int64, users int32, targets int32), one entry per active slot in ascending slot order, from the first pair of each
        slot (host batch) or the pair at the slot's pair offset (device batch: batch["active"] = (slots, offsets), host
        tables of sample_batch_device). None when no slot holds a pair."""
        if "active" in batch:
            slots, first = batch["active"]
        else:
            locs = batch["uLocs_seq"]
            locs = locs.cpu().numpy() if isinstance(locs, torch.Tensor) else np.asarray(locs)
            slots, first = np.unique(locs[:len(locs) // 2], return_index=True)
        if len(slots) == 0:
            return None
        first = torch.as_tensor(np.asarray(first, dtype=np.int64), device=self.device)
        slots = torch.as_tensor(np.asarray(slots, dtype=np.int64), device=self.device)
        return slots, self._i32(batch["uids"]).index_select(0, first), self._i32(batch["iids"]).index_select(0, first)

    def _slot_users_targets(self, slots, users, targets):
        """_active_slots' triples spread over the batch's slots, as ops.seq_targets reads them: (slot_user, slot_target)
        int32 [args.batch]; an inactive slot keeps user 0 (a valid exclusion list) and target -1 (no loss term)."""
        slot_user = torch.zeros(args.batch, dtype=torch.int32, device=self.device)
        slot_target = torch.full((args.batch,), -1, dtype=torch.int32, device=self.device)
        slot_user.index_copy_(0, slots, users)
        slot_target.index_copy_(0, slots, targets)
        return slot_user, slot_target

    def _softmax_pre_loss(self, fu, fi, att, batch):
        """--predLoss softmax: (1 / max(n_active, 1)) * sum over the active slots b of ln sum_{i in E_b} exp(z_bi) - z_{b,t_b}
        with z_bi = <leaky(att[b]) + fu[u_b], fi[i]> / softmaxTemp and E_b = every item outside user u_b's banned list
        (the items negSamp never draws), plus the target t_b. One (slot, user, target) triple per active slot, from the
        positive half of the batch without a read-back: the first pair of each slot (host batch) or the pair at the
        slot's pair offset (device batch: batch["active"] = (slots, offsets), host tables of sample_batch_device).
        With batch["cand"] (--softmaxNegs, drawn by train_loss) E_b is the candidates outside the banned list plus t_b;
        with batch["cand_bias"] (--softmaxNegDist pop) candidate position j adds cand_bias[j] to its logit, which makes
        the sum an estimator of the full-catalogue one, and a position at -inf does not count."""
        active = self._active_slots(batch)
        if active is None:
            return att.sum().reshape(1) * 0.0
        slots, u, t = active
        q = ag.LeakyAddFn.apply(att.index_select(0, slots), fu.index_select(0, u.long()), NNs.leaky)
        scale = 1.0 / max(int(slots.numel()), 1)
        if "cand" in batch:     # --softmaxNegs: E_b = the step's candidates outside the banned list, plus the target
            return ag.SoftmaxLossCandFn.apply(q, fi, batch["cand"], t, 1.0 / args.softmaxTemp, scale,
                                              self._banned_device(), u, batch.get("cand_bias"))
        return ag.SoftmaxLossFn.apply(q, fi, t, 1.0 / args.softmaxTemp, scale, self._banned_device(), u)

    def _softmax_pre_loss_all(self, fu, fi, x, batch, tokens):
        """--seqTargets all: _softmax_pre_loss with every real token of every active slot a query. x is
        the last attention layer's slab [args.batch * pos_length, d] under --seqAtt causal, tokens the batch's token arrays.
        Row (b, j) is q = leaky(sum_{i <= j} x[b, i]) + fu[u_b] (ag.SeqPrefixQueryFn) against the item after token j, the
        slot's sampled positive after the last token (ops.seq_targets); its eligible set is user u_b's, as under last.
        preLoss = the sum of the rows' terms over their count. The count stays on the device: the loss entries run with
        scale 1 and the sum is divided by a device scalar, which the backward hands them as their upstream gradient. A
        slot with a positive and no tokens has no row."""
        P = args.pos_length
        active = self._active_slots(batch)
        if active is None:
            return x.sum().reshape(1) * 0.0
        slot_user, slot_target = self._slot_users_targets(*active)
        seq_items, _, seg_begin, seg_len = tokens
        target, excl_row = ops.seq_targets(seq_items, seg_begin, seg_len, slot_user, slot_target, P, args.item)
        q = ag.SeqPrefixQueryFn.apply(x, fu.index_select(0, slot_user.long()), seg_len, P, NNs.leaky)
        count = (target >= 0).sum().clamp(min=1).to(torch.float32)
        if "cand" in batch:
            total = ag.SoftmaxLossCandFn.apply(q, fi, batch["cand"], target, 1.0 / args.softmaxTemp, 1.0, self._banned_device(),
                                               excl_row, batch.get("cand_bias"), True)
        else:
            total = ag.SoftmaxLossFn.apply(q, fi, target, 1.0 / args.softmaxTemp, 1.0, self._banned_device(), excl_row)
        return total / count

    def _head_att_sum_train(self, fi, batch):
        """The reference's collapsed head (--seqAtt sum) as autograd nodes: the masked sums make ONE token per slot and
        the attention layers run on length-1 sequences (model.py:158-168)."""
        d, heads, leaky = args.latdim, args.num_attention_heads, NNs.leaky
        if "seq_seg" in batch:                                            # device-sampled: segments, no CSRs
            seg_begin, seg_len = batch["seq_seg"]
            seq_tok, pos_tok = ag.SeqSumFn.apply(fi, self.posEmbed, self._device_sampler().seq_items, seg_begin, seg_len)
        else:
            pi, pp = self._masked_sum_plans(batch["sequence"], batch["mask"])
            pit, ppt = self._masked_sum_plans_t(batch["sequence"], batch["mask"])
            seq_tok = ag.SpmmFn.apply(fi, pi, pit)
            pos_tok = ag.SpmmFn.apply(self.posEmbed, pp, ppt)
        B = seq_tok.shape[0]
        ln = lambda x, gb: ag.LayerNormFn.apply(x.view(B, 1, d), gb[0], gb[1]).view(B, d)
        att = ag.LeakyAddFn.apply(ln(seq_tok, self.head_ln[0]), ln(pos_tok, self.head_ln[1]), 1.0)
        for i, mh in enumerate(self.multihead_self_attention_sequence):
            w = mh.weights()
            a1 = ag.MhsaMeanFn.apply(ln(att, self.head_ln[2 + i]).view(B, 1, d), w["Wq"], w["bq"], w["Wk"], w["bk"],
                                     w["Wv"], w["bv"], heads)
            att = ag.LeakyAddFn.apply(a1, att, leaky)
        return att

    def _touched_rows(self, batch) -> dict:
        """--fusion_rows batch: the user rows (uids, suids[k]) and item rows (iids, siids[k], the head's sequence items)
        the loss reads (with --softmaxNegs also the step's candidates), marked and compacted on the device
        (ops.rows_mark / rows_compact) into capacities known on the host, and the two counts copied to pinned host
        memory without waiting. Returns {"rows": [(rows, count)] * 2, "caps", "host": the pinned counts, "done": the
        event after their copy}."""
        U, I, dev = args.user, args.item, self.device
        flags_u, flags_i, host = self._cached(
            "_rows_bufs", (U, I, str(dev)), lambda: (torch.zeros(U, dtype=torch.uint8, device=dev),
                                                     torch.zeros(I, dtype=torch.uint8, device=dev),
                                                     torch.zeros(2, dtype=torch.int32, pin_memory=True)))
        cand = batch.get("cand")                                          # --softmaxNegs: the step's candidate rows
        for ids in [batch["iids"]] + list(batch["siids"]) + ([] if cand is None else [cand]):
            ops.rows_mark(ids, flags_i)
        if "seq_seg" in batch:
            seg_begin, seg_len = batch["seq_seg"]
            ops.rows_mark_segments(self._device_sampler().seq_items, seg_begin, seg_len, args.pos_length, flags_i)
            n_seq = int(seg_len.numel()) * args.pos_length
        else:
            _, items, _ = self._masked_sum_csr(batch["sequence"], batch["mask"])
            n_seq = len(items)
            ops.rows_mark(torch.from_numpy(items).to(dev), flags_i)
        for ids in [batch["uids"]] + list(batch["suids"]):
            ops.rows_mark(ids, flags_u)
        cap_u = min(U, int(batch["uids"].numel()) + sum(int(v.numel()) for v in batch["suids"]))
        cap_i = min(I, int(batch["iids"].numel()) + sum(int(v.numel()) for v in batch["siids"]) + n_seq
                    + (0 if cand is None else int(cand.numel())))
        rows_u, count_u = ops.rows_compact(flags_u, max(cap_u, 1) if U else 0)
        rows_i, count_i = ops.rows_compact(flags_i, max(cap_i, 1) if I else 0)
        host[0:1].copy_(count_u, non_blocking=True)
        host[1:2].copy_(count_i, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return {"rows": [(rows_u, count_u), (rows_i, count_i)], "caps": (max(cap_u, 1), max(cap_i, 1)), "host": host,
                "done": done}

    def _masked_sum_plans_t(self, sequence, mask):
        """Transposed per-batch CSRs (rows = items / positions, columns = batch slots) for the
        backward of the masked sums. scipy's CSR -> CSC conversion is a counting sort that keeps
        duplicated entries (an item twice in a sequence counts twice), 4x cheaper than an argsort."""
        rowptr, items, pos = self._masked_sum_csr(sequence, mask)
        B, L = np.asarray(mask).shape
        out = []
        for cols, n_rows in ((items, args.item), (pos, L)):
            csc = sp.csr_matrix((np.ones(len(cols), dtype=np.int8), cols, rowptr), shape=(B, n_rows)).tocsc()
            out.append(ops.SpmmPlan(csc.indptr.astype(np.int32), csc.indices.astype(np.int32), n_rows, B, device=self.device,
                                    validate=False))
        return out

    TRAIN_SAMPLE_NUM = 40      # the train_sample_num trainEpoch passes (sample_num_list, reference model.py:345-356)

    def sampleTrainBatch(self, batIds, labelMat, timeMat=None, train_sample_num=TRAIN_SAMPLE_NUM, as_arrays=False):
        """reference model.py:252-302: per user ONE positive (one of the last pred_num+1 items before
        the held-out one, repeated sampNum times) against sampNum uniform negatives the user has
        not interacted with (and != the last item / the test item); the sequence fed to the head
        stops before the chosen positive. Same distribution as the reference's per-user Python
        loops (its rejection sampler negSamp, DataHandler.py:28-41), drawn in bulk for the whole
        batch (one sorted (slot, item) key table of everything a user may not draw, one searchsorted
        per rejection round): the loops cost ~75 ms per 512-user batch on the host, 10x the device
        time of the step."""
        rng = np.random
        batIds = np.asarray(batIds, dtype=np.int64)
        B, P, I = len(batIds), args.pos_length, args.item
        flat, ptr = self._flat_sequences()
        start, end = ptr[batIds], ptr[batIds + 1]
        n_pos = end - start - 1                                      # len(posset) = len(full) - 1
        samp = np.minimum(train_sample_num, np.maximum(n_pos, 0))    # negatives (= positive copies) per user
        act = samp > 0
        hi = np.maximum(np.minimum(args.pred_num + 1, n_pos - 3), 1)
        choose = np.where(act, (rng.random_sample(B) * hi).astype(np.int64) + 1, 1)
        pos_item = flat[np.where(act, end - 1 - choose, 0)]          # posset[-choose] = full[-1 - choose]
        # ---- negatives: bulk rejection against seen items, the last item and the held-out item -----
        lab = labelMat[batIds]                                       # CSR rows, no densification
        slot_seen = np.repeat(np.arange(B, dtype=np.int64), np.diff(lab.indptr))
        tst_item = self._tst_ids()[batIds]
        has_tst = tst_item >= 0
        last_item = flat[np.maximum(end - 1, start)]
        banned = np.concatenate([slot_seen * I + lab.indices.astype(np.int64),
                                 np.flatnonzero(act) * I + last_item[act],
                                 np.flatnonzero(has_tst) * I + tst_item[has_tst]])
        banned.sort()
        slot = np.repeat(np.arange(B, dtype=np.int64), samp)         # batch slot of every (pos, neg) pair
        negs = rng.randint(0, I, size=slot.size).astype(np.int64)
        bad = np.arange(slot.size)
        while bad.size:
            keys = slot[bad] * I + negs[bad]
            loc = np.searchsorted(banned, keys)
            hit = banned[np.minimum(loc, banned.size - 1)] == keys
            bad = bad[hit]
            negs[bad] = rng.randint(0, I, size=bad.size)
        half_u, half_i, half_l = batIds[slot], pos_item[slot], slot
        # ---- the sequence fed to the head: the items before the chosen positive, right-aligned -------
        m = np.maximum(n_pos - choose, 0)                            # len(posset[:-choose])
        sequence, mask = _right_aligned(flat, start + m, m, args.batch, P)
        uL, iL, uLs = np.concatenate([half_u, half_u]), np.concatenate([half_i, negs]), np.concatenate([half_l, half_l])
        if as_arrays:      # the epoch loop keeps int32 arrays end to end (the list round trip cost 2 ms per step)
            return uL.astype(np.int32), iL.astype(np.int32), sequence, mask, uLs.astype(np.int32)
        return uL.tolist(), iL.tolist(), sequence, mask, uLs.tolist()       # the reference's feed_dict lists

    def sampleSslBatch(self, batIds, labelMat, use_epsilon=True, as_arrays=False):
        """reference model.py:304-339: per interval and user up to sslNum (item, item) pairs drawn
        with replacement from the user's items of that interval, written INTERLEAVED
        (pair j at 2j, 2j+1) — the loss later splits the vector by halves (model.py:192-201).
        Vectorised over the batch on the CSR rows (the reference densifies [batch, I] per interval)."""
        rng = np.random
        batIds = np.asarray(batIds)
        uLocs, iLocs, uLocs_seq = [], [], []
        for k in range(args.graphNum):
            lab = labelMat[k][batIds]
            deg = np.diff(lab.indptr)
            npair = np.minimum(args.sslNum, deg // 2)                # pairs per user
            total = int(npair.sum())
            if total == 0:
                empty = np.zeros(0, np.int32)
                uLocs.append(empty); iLocs.append(empty); uLocs_seq.append(empty)
                continue
            slot = np.repeat(np.arange(len(batIds)), npair)          # batch slot of every pair
            base = lab.indptr[:-1][slot]
            first = lab.indices[base + (rng.random_sample(total) * deg[slot]).astype(np.int64)]
            second = lab.indices[base + (rng.random_sample(total) * deg[slot]).astype(np.int64)]
            its = np.empty(2 * total, dtype=np.int32)
            its[0::2], its[1::2] = first, second
            uLocs.append(np.repeat(batIds[slot], 2).astype(np.int32))
            iLocs.append(its)
            uLocs_seq.append(np.repeat(slot, 2).astype(np.int32))
        if as_arrays:      # the epoch loop keeps int32 arrays; the reference's feed_dict takes lists
            return uLocs, iLocs, uLocs_seq
        return tuple([a.tolist() for a in x] for x in (uLocs, iLocs, uLocs_seq))

    def _host_train_batch(self, batIds) -> dict:
        """trainEpoch's host-sampled batch for train_loss: sampleTrainBatch and sampleSslBatch as int32 arrays."""
        h = self.handler
        uLocs, iLocs, sequence, mask, uLocs_seq = self.sampleTrainBatch(batIds, h.trnMat, h.timeMat, self.TRAIN_SAMPLE_NUM,
                                                                        as_arrays=True)
        suLocs, siLocs, _ = self.sampleSslBatch(batIds, h.subMat, False, as_arrays=True)
        return {"uids": uLocs, "iids": iLocs, "uLocs_seq": uLocs_seq, "sequence": sequence, "mask": mask,
                "suids": suLocs, "siids": siLocs}

    def _device_sampler(self) -> DeviceSampler:
        """The device sampler's tables for the current handler and flags, built once."""
        h = self.handler
        return self._cached("_dev_sampler", (h.sequence, h.trnMat, h.subMat, h.tstInt, args.item, args.sslNum, str(self.device)),
                            lambda: DeviceSampler(h, self.device, args.item, self.TRAIN_SAMPLE_NUM, args.sslNum))

    def sample_batch_device(self, batIds, seed: int, step: int) -> dict:
        """One training batch drawn on the device: sampleTrainBatch's and sampleSslBatch's distributions (with the SSL
        pairs drawn from each row's distinct items), as a pure function of (seed, step, user id) per user. Returns
        device int32 tensors uids, iids, uLocs_seq, suids[k], siids[k], seq_seg = (seg_begin int64, seg_len int32)
        [args.batch], the head's sequence segments, and active = (slots, offsets): the slots that hold pairs and the
        index of each one's first pair (host int64 arrays). Every count comes from host tables: nothing is copied back."""
        S = self._device_sampler()
        bat = np.asarray(batIds, dtype=np.int64).reshape(-1)
        B, T = len(bat), len(S.npair)
        if B > args.batch:
            raise ValueError(f"{B} users in a batch of {args.batch} slots")
        if B and (bat.min() < 0 or bat.max() >= S.n_users):
            raise ValueError(f"batIds outside [0, {S.n_users})")
        samp = S.samp[bat]
        npair2 = 2 * S.npair[:, bat]                                      # [T, B] SSL entries per slot
        offs = np.zeros(B + T * B + 1, dtype=np.int64)                    # pair_off [B] | ssl_off [T, B] | n_out
        np.cumsum(samp[:-1], out=offs[1:B])
        np.cumsum(npair2.reshape(-1), out=offs[B + 1:])
        n_pairs = int(samp.sum())
        dev = self.device
        bat_d = torch.from_numpy(bat.astype(np.int32)).to(dev)
        offs_d = torch.from_numpy(offs).to(dev)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        uids, iids, locs, seg_begin, seg_len = ops.sample_train(
            bat_d, args.batch, S.seq_ptr, S.seq_items, S.ban_ptr, S.ban_items, S.n_items, S.train_sample_num,
            args.pred_num, args.pos_length, offs_d[:B], n_pairs, seed, step)
        su, si, _ = ops.sample_ssl(bat_d, S.sub_ptr, S.sub_items, S.ssl_num, offs_d[B:B + T * B], int(offs[-1]), seed, step)
        ends = np.concatenate([[0], np.cumsum(npair2.sum(1))]).astype(np.int64)
        act = np.flatnonzero(samp > 0)                                    # the slots that hold pairs, and their first pair
        return {"uids": uids, "iids": iids, "uLocs_seq": locs, "seq_seg": (seg_begin, seg_len),
                "active": (act.astype(np.int64), offs[:B][act]),
                "suids": [su[ends[k]:ends[k + 1]] for k in range(T)], "siids": [si[ends[k]:ends[k + 1]] for k in range(T)]}

    def _trainable(self):
        return {k: v for k, v in NNs.params.items() if v.requires_grad}

    def trainEpoch(self):
        """reference model.py:341-382: trnNum users per epoch in batches of args.batch."""
        if getattr(self, "optimizer", None) is None:
            self.optimizer = self._make_optimizer()
        sfIds = np.random.permutation(args.user)[:args.trnNum]
        steps = int(np.ceil(len(sfIds) / args.batch))
        device = args.sampler == "device"
        if device:        # one seed per epoch from numpy's global stream: np.random.seed still reproduces a run
            seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
        edge_drop = args.edgeKeepRate < 1.0
        if edge_drop:     # its own seed per epoch, drawn only when the flag is on: a seeded run without it sees the
            edge_seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))      # np.random stream it always saw
        cand_draw = args.predLoss == "softmax" and args.softmaxNegs > 0
        if cand_draw:     # likewise, and after the edge-drop seed
            cand_seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
        # losses stay on the device until the epoch ends: a float() per step would make the host wait for the
        # step's kernels before it samples the next batch (host sampling and device work overlap this way)
        loss_sum = torch.zeros(1, dtype=torch.float32, device=self.device)
        pre_sum = torch.zeros(1, dtype=torch.float32, device=self.device)
        for i in range(steps):
            batIds = sfIds[i * args.batch:(i + 1) * args.batch]
            batch = self.sample_batch_device(batIds, seed, i) if device else self._host_train_batch(batIds)
            if edge_drop:
                batch["edge_seed"] = (edge_seed, i)
            if cand_draw:
                batch["cand_seed"] = (cand_seed, i)
            params = self._trainable()
            for p in params.values():
                p.grad = None
            pre, ssl = self.train_loss(batch)
            (pre + args.ssl_reg * ssl).backward()
            with torch.no_grad():
                pre_sum += pre.detach()
                loss_sum += pre.detach() + args.reg * NNs.Regularize() + args.ssl_reg * ssl.detach()
            self.optimizer.step({k: p.grad for k, p in params.items()})
        return {"Loss": float(loss_sum) / steps, "preLoss": float(pre_sum) / steps}

    def _make_optimizer(self):
        return ops.Adam(self._trainable(), lr=args.lr, decay=args.decay, decay_step=args.decay_step,
                        reg=args.reg, reg_names=set(NNs.regParams))

    def saveHistory(self, directory="."):
        """reference model.py:512-520: metric history + variables (torch.save instead of a TF
        checkpoint; same file stems History/<save_path>.his and Models/<save_path>). tf.train.Saver()
        saves every global variable, i.e. also Adam's slots and globalStep — kept here under
        "optimizer" so a resumed run continues the lr staircase and the moments."""
        import os
        import pickle
        if args.epoch == 0:
            return
        os.makedirs(os.path.join(directory, "History"), exist_ok=True)
        os.makedirs(os.path.join(directory, "Models"), exist_ok=True)
        with open(os.path.join(directory, "History", args.save_path + ".his"), "wb") as fs:
            pickle.dump(self.metrics, fs)
        state = {"params": {k: v.detach().cpu() for k, v in NNs.params.items()}, "adjNorm": args.adjNorm,
                 "seqAtt": args.seqAtt, "seqPool": args.seqPool, "edgeTime": self._edge_time_state(), "rnnCell": args.rnnCell}
        if args.seqAtt in SEQ_TOKEN_MODES:
            state["seqHeads"] = seq_heads()        # the effective head count of the attention over tokens
            state["seqFFN"] = int(args.seqFFN)     # the hidden width of the feed-forward blocks, 0 = none
        if getattr(self, "optimizer", None) is not None:
            state["optimizer"] = self.optimizer.state_dict()
        torch.save(state, os.path.join(directory, "Models", args.save_path))

    def _edge_time_state(self) -> dict:
        """What a checkpoint records of --edgeTime: the flag and, under slot, what fixes every edge's bucket."""
        if args.edgeTime == "none":
            return {"mode": "none"}
        return {"mode": args.edgeTime, "slot": float(args.slot), "mi": int(self.handler.timeMin), "M": int(self.maxTime) + 1}

    def loadModel(self, directory="."):
        """reference model.py:522-526. The variable set and every shape must match the model that
        prepareModel() built (tf.train.Saver.restore raises on a missing or mis-shaped variable)."""
        import os
        import pickle
        state = torch.load(os.path.join(directory, "Models", args.load_model), weights_only=True)
        stored_norm = state.get("adjNorm", "none")       # a checkpoint from before --adjNorm is an unnormalised model
        if stored_norm != args.adjNorm:
            raise ValueError(f"checkpoint was trained with --adjNorm {stored_norm}, this run has --adjNorm {args.adjNorm}: "
                             "the normalisation is part of the model")
        stored_att = state.get("seqAtt", "sum")          # a checkpoint from before --seqAtt is a collapsed-head model
        if stored_att != args.seqAtt:
            raise ValueError(f"checkpoint was trained with --seqAtt {stored_att}, this run has --seqAtt {args.seqAtt}: "
                             "the head's attention is part of the model")
        stored_heads = state.get("seqHeads")             # a checkpoint from before --seqHeads is not checked
        if stored_heads is not None and args.seqAtt in SEQ_TOKEN_MODES and stored_heads != seq_heads():
            raise ValueError(f"checkpoint was trained with {stored_heads} heads in the sequence attention, this run has "
                             f"{seq_heads()} (--seqHeads {args.seqHeads}, --num_attention_heads {args.num_attention_heads}): "
                             "the head count is part of the model")
        stored_ffn = state.get("seqFFN", 0)              # a checkpoint from before --seqFFN has no feed-forward blocks
        if stored_ffn != args.seqFFN:
            raise ValueError(f"checkpoint was trained with --seqFFN {stored_ffn}, this run has --seqFFN {args.seqFFN}: "
                             "the feed-forward blocks are part of the model")
        stored_pool = state.get("seqPool", "sum")        # a checkpoint from before --seqPool pools with the plain sum
        if stored_pool != args.seqPool:
            raise ValueError(f"checkpoint was trained with --seqPool {stored_pool}, this run has --seqPool {args.seqPool}: "
                             "the head's pooling is part of the model")
        stored_cell = state.get("rnnCell", "lstm")       # a checkpoint from before --rnnCell is an LSTM model
        if stored_cell != args.rnnCell:
            raise ValueError(f"checkpoint was trained with --rnnCell {stored_cell}, this run has --rnnCell {args.rnnCell}: "
                             "the recurrent cell is part of the model")
        stored_time = state.get("edgeTime", {"mode": "none"})      # a checkpoint from before --edgeTime has no time term
        if stored_time != self._edge_time_state():
            raise ValueError(f"checkpoint was trained with --edgeTime {stored_time}, this run has {self._edge_time_state()}: "
                             "the time term, --slot, the earliest timestamp and the table size are part of the model")
        saved = state["params"]
        if set(saved) != set(NNs.params):
            raise KeyError(f"checkpoint variables differ from the model's: missing {sorted(set(NNs.params) - set(saved))[:4]}, "
                           f"unexpected {sorted(set(saved) - set(NNs.params))[:4]}")
        for k, v in saved.items():
            if tuple(v.shape) != tuple(NNs.params[k].shape):
                raise ValueError(f"checkpoint variable {k!r}: shape {tuple(v.shape)} != {tuple(NNs.params[k].shape)}")
        with torch.no_grad():
            for k, v in saved.items():
                NNs.params[k].copy_(v)
        if "optimizer" in state:
            self.optimizer = self._make_optimizer()
            self.optimizer.load_state_dict(state["optimizer"])
        with open(os.path.join(directory, "History", args.load_model + ".his"), "rb") as fs:
            self.metrics = pickle.load(fs)
        print("Model Loaded")

    # ------------------------------------------------------------------ model construction
    def prepareModel(self):
        """reference model.py:207-240 up to the call of ours(): adjacency constants for every
        interval and both directions, leaky slope, then the hot path."""
        if not 0.0 < args.edgeKeepRate <= 1.0:
            raise ValueError(f"--edgeKeepRate {args.edgeKeepRate}: need a rate in (0, 1]")
        if args.adjNorm not in NORMS:
            raise ValueError(f"--adjNorm {args.adjNorm}: one of {NORMS}")
        if args.seqAtt not in SEQ_ATT:
            raise ValueError(f"--seqAtt {args.seqAtt}: one of {SEQ_ATT}")
        if args.seqPool not in SEQ_POOL:
            raise ValueError(f"--seqPool {args.seqPool}: one of {SEQ_POOL}")
        if args.seqTargets not in SEQ_TARGETS:
            raise ValueError(f"--seqTargets {args.seqTargets}: one of {SEQ_TARGETS}")
        if args.seqTargets == "all":       # refused before any forward, naming the flag that is missing
            if args.seqAtt != "causal":
                raise ValueError(f"--seqTargets all needs --seqAtt causal (--seqAtt full --seqMask causal on the command line; "
                                 f"got --seqAtt {args.seqAtt}): under bidirectional "
                                 "attention a prefix's row has seen its own target")
            if args.seqPool != "sum":
                raise ValueError(f"--seqTargets all needs --seqPool sum (got --seqPool {args.seqPool}): the prefix queries "
                                 "are running sums of the token rows")
            if args.predLoss != "softmax":
                raise ValueError(f"--seqTargets all needs --predLoss softmax (got --predLoss {args.predLoss}): the prefixes "
                                 "have no sampled negatives for the hinge loss")
        if args.predLoss not in PRED_LOSS:
            raise ValueError(f"--predLoss {args.predLoss}: one of {PRED_LOSS}")
        if args.rnnCell not in RNN_CELL:
            raise ValueError(f"--rnnCell {args.rnnCell}: one of {RNN_CELL}")
        if args.rnnCell == "gru" and (args.latdim % 32 or not 32 <= args.latdim <= 256):   # the GRU entries' widths
            raise ValueError(f"--rnnCell gru needs latdim to be a multiple of 32 up to 256, got {args.latdim}")
        if args.edgeTime not in EDGE_TIME:
            raise ValueError(f"--edgeTime {args.edgeTime}: one of {EDGE_TIME}")
        time = None
        if args.edgeTime == "slot":
            if args.edgeKeepRate < 1.0:
                raise ValueError("--edgeTime slot does not combine with --edgeKeepRate < 1: the bucket-sorted reduction of "
                                 "the time tables' gradient cannot evaluate the (user, item)-keyed drop")
            # (a handler prepared before the flag was set has not run it yet)
            self.handler.timeMin, self.handler.maxTime = self.handler.timeProcess(self.handler.subMat)
            time = (self.handler.timeMin, args.slot, ops.check_n_buckets(self.handler.maxTime + 1))
        if not args.softmaxTemp > 0.0 or not np.isfinite(args.softmaxTemp):
            raise ValueError(f"--softmaxTemp {args.softmaxTemp}: need a finite temperature > 0")
        if args.softmaxNegs < 0:
            raise ValueError(f"--softmaxNegs {args.softmaxNegs}: need a count >= 0 (0 = the whole catalogue)")
        if args.softmaxNegs > 0 and args.predLoss != "softmax":
            raise ValueError(f"--softmaxNegs {args.softmaxNegs} needs --predLoss softmax: --predLoss {args.predLoss} "
                             "draws its own negatives")
        if args.softmaxNegs > args.item:
            raise ValueError(f"--softmaxNegs {args.softmaxNegs} exceeds the {args.item} items of the catalogue")
        if args.softmaxNegDist not in NEG_DIST:
            raise ValueError(f"--softmaxNegDist {args.softmaxNegDist}: one of {NEG_DIST}")
        if args.softmaxNegDist == "pop":
            if args.predLoss != "softmax" or args.softmaxNegs <= 0:
                raise ValueError(f"--softmaxNegDist pop needs --predLoss softmax and --softmaxNegs > 0: it weights the "
                                 f"draw of the shared candidates (got --predLoss {args.predLoss}, --softmaxNegs "
                                 f"{args.softmaxNegs})")
            if not np.isfinite(args.softmaxNegPow) or not 0.0 <= args.softmaxNegPow <= 1.0:
                raise ValueError(f"--softmaxNegPow {args.softmaxNegPow}: need a finite exponent in [0, 1]")
        if args.predLoss == "softmax":
            if args.fusion_rows == "batch" and args.softmaxNegs == 0:
                raise ValueError("--predLoss softmax does not combine with --fusion_rows batch: the loss reads every item "
                                 "row of the fused table, so there is no row subset to fuse")
            if args.latdim not in (32, 64, 128):
                raise ValueError(f"--predLoss softmax needs latdim in (32, 64, 128), got {args.latdim}")
        if args.seqPool == "additive":     # refused before any forward; ahead of --seqAtt full, whose limits it shares
            if args.seqAtt not in SEQ_TOKEN_MODES:
                raise ValueError("--seqPool additive needs --seqAtt full or causal: under --seqAtt sum a slot holds one token, the "
                                 "softmax over it is 1 and the pooling is the identity")
            why = ops.seq_addpool_supported(args.latdim, args.query_vector_dim, args.pos_length)
            if why is not None:
                raise ValueError(f"--seqPool additive is not available for this configuration: {why}")
            if args.latdim % 32 or args.query_vector_dim % 32:       # the projection and its gradients: the dense entries
                raise ValueError(f"--seqPool additive needs latdim and query_vector_dim to be multiples of 32, got "
                                 f"{args.latdim} and {args.query_vector_dim}")
        if args.seqHeads < 0:
            raise ValueError(f"--seqHeads {args.seqHeads}: need a count >= 0 (0 = follow --num_attention_heads)")
        if args.seqHeads > 0 and args.seqAtt not in SEQ_TOKEN_MODES:
            raise ValueError(f"--seqHeads {args.seqHeads} needs --seqAtt full (with or without --seqMask causal; got --seqAtt "
                             f"{args.seqAtt}): it is the head count of the attention over the sequence's tokens")
        if args.seqFFN < 0:
            raise ValueError(f"--seqFFN {args.seqFFN}: need a hidden width >= 0 (0 = no feed-forward blocks)")
        if args.seqFFN > 0:                 # refused before any forward, with the library's reason
            if args.seqAtt not in SEQ_TOKEN_MODES:
                raise ValueError(f"--seqFFN {args.seqFFN} needs --seqAtt full (with or without --seqMask causal; got --seqAtt "
                                 f"{args.seqAtt}): the blocks follow the attention layers over the sequence's tokens")
            why = ops.seq_ffn_supported(args.latdim, args.seqFFN, args.pos_length)
            if why is not None:
                raise ValueError(f"--seqFFN {args.seqFFN} is not available for this configuration: {why}")
        if args.seqAtt in SEQ_TOKEN_MODES:  # refused before any forward: the attention kernels take these shapes only
            heads = seq_heads()
            why = ops.seq_attn_supported(args.latdim, heads, args.pos_length)
            if why is not None and args.seqHeads > 0:        # few wide heads: the matrix-core entries
                wide = ops.seq_attn_wide_supported(args.latdim, heads, args.pos_length)
                why = None if wide is None else (f"--seqHeads {args.seqHeads} needs latdim / seqHeads in (2, 4, 8, 16, 32, 64) "
                                                 f"and pos_length <= 256 ({why}; {wide})")
            if why is not None:
                raise ValueError(f"--seqAtt {args.seqAtt} is not available for this configuration: {why}")
        NNs.reset(self.device)
        NNs.leaky = args.leaky
        self.actFunc = "leakyRelu"
        self.subAdj, self.subTpAdj = [], []
        for i in range(args.graphNum):
            adj, tp = interval_pair(self.handler.subMat[i], self.device, norm=args.adjNorm, time=time)
            self.subAdj.append(adj)
            self.subTpAdj.append(tp)
        self.maxTime = self.handler.maxTime
        self.user_vector_tensor = self.item_vector_tensor = None
        self._scratch_u = self._scratch_i = self._scratch_bu = self._scratch_bi = None
        self._batch, self._batch_ok = None, None
        self.final_user_vector, self.final_item_vector = self.ours()

    def makePrint(self, name, ep, reses, save):
        ret = "Epoch %d/%d, %s: " % (ep, args.epoch, name)
        for metric, val in reses.items():
            ret += "%s = %.4f, " % (metric, val)
            tem = name + metric
            if save and tem in self.metrics:
                self.metrics[tem].append(val)
        return ret[:-2] + "  "

    def run(self):
        """reference model.py:41-70: train args.epoch epochs, test every tstEpoch, keep the best NDCG."""
        self.prepareModel()
        if args.load_model is not None:
            self.loadModel()
            stloc = len(self.metrics["TrainLoss"]) * args.tstEpoch - (args.tstEpoch - 1)
        else:
            stloc = 0
        maxndcg, maxres, maxepoch = 0.0, dict(), 0
        for ep in range(stloc, args.epoch):
            test = ep % args.tstEpoch == 0
            print(self.makePrint("Train", ep, self.trainEpoch(), test))
            if test:
                reses = self.testEpoch()
                print(self.makePrint("Test", ep, reses, test))
                if args.full_rank:
                    print(self.makePrint("TestFull", ep, self.testEpochFull(), False))
                if reses["NDCG"] > maxndcg:
                    self.saveHistory()
                    maxndcg, maxres, maxepoch = reses["NDCG"], reses, ep
        reses = self.testEpoch()
        print(self.makePrint("Test", args.epoch, reses, True))
        if args.full_rank:
            print(self.makePrint("TestFull", args.epoch, self.testEpochFull(), False))
        print(self.makePrint("max", maxepoch, maxres, True))
        return reses
