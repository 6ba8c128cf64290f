/*
 * sagnn.h — C ABI of libsagnn.so: SelfGNN's per-time-interval graph propagation and
 * interval fusion as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference (LIU-YUXI/SA-GNN, TF1 graph mode) has no FFI: its seam is the Python
 * method Recommender.messagePropagate (model.py:80-92) and the loop around it in
 * Recommender.ours (model.py:118-155). Each entry point below names the reference
 * lines it replaces. The Python host in sa-gnn_amd/ binds these with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - Plain C: pointers, sizes, strides in ELEMENTS. No torch / HIP types.
 *     `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Every `d_*` / unprefixed tensor pointer is DEVICE memory owned by the caller.
 *     `h_*` pointers are HOST memory. The library never frees or retains caller memory
 *     except the two CSR device pointers kept inside a plan object.
 *   - All floating point is fp32, all indices int32 (reference: fp32 / int32 throughout).
 *   - Calls are asynchronous on `stream`; the library never synchronises except in
 *     sagnn_spmm_plan_create (one-off upload of plan metadata).
 *   - Return value: 0 = OK; negative = argument error (SAGNN_ERR_*); positive = hipError_t.
 *     No C++ exception crosses the ABI. sagnn_last_error() gives a thread-local message.
 *   - Feature rows must be 16-byte aligned: base pointers 16-B aligned, every ld a
 *     multiple of 4, d a multiple of 4 with 4 <= d <= 256.
 */
#ifndef SAGNN_H
#define SAGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGNN_VERSION 10500 /* 1.5.0 */

enum {
  SAGNN_OK = 0,
  SAGNN_ERR_NULL = -1,      /* a required pointer is NULL */
  SAGNN_ERR_DIM = -2,       /* d / t / heads unsupported */
  SAGNN_ERR_ALIGN = -3,     /* pointer or leading dimension not 16-byte aligned */
  SAGNN_ERR_CSR = -4,       /* rowptr not monotone, rowptr[n]!=nnz, colidx out of range */
  SAGNN_ERR_ARG = -5,       /* any other inconsistent argument */
  SAGNN_ERR_WORKSPACE = -6, /* workspace missing or too small */
  SAGNN_ERR_NOMEM = -7      /* host allocation failed */
};

int sagnn_version(void);

/* Arithmetic engine of the GEMM-shaped fusion stages (LSTM gate product, the three dense layers of the
 * attention, their backward products), selected PER CALLING THREAD — there is no environment switch and no
 * process-wide state: a thread that never calls sagnn_set_engine runs SAGNN_ENGINE_F16X2.
 *   SAGNN_ENGINE_F16X2  the default: 16-bit matrix cores over two-piece split fp32 operands (see ARITHMETIC below)
 *   SAGNN_ENGINE_F32    v_mfma_f32_32x32x2_f32 kernels: an fp32 fmaf chain bit for bit (the exact-fp32 reference the
 *                       default engine is measured against)
 *   SAGNN_ENGINE_VALU   the plain VALU formulations
 * Which kernel a fusion call runs, per engine, shape and alignment: the table in sa-gnn_amd/csrc/engine.cpp.
 * sagnn_set_engine returns SAGNN_OK or SAGNN_ERR_ARG; sagnn_get_engine the calling thread's engine. The SpMM is
 * plain fp32 under every engine. */
enum { SAGNN_ENGINE_F16X2 = 0, SAGNN_ENGINE_F32 = 1, SAGNN_ENGINE_VALU = 2 };
int sagnn_set_engine(int engine);
int sagnn_get_engine(void);
/* Number of tiles / chunks the default engine has re-evaluated in fp32 on the current device since the last reset,
 * because an operand left the window of the split (ARITHMETIC below): 0 on ordinary data. Synchronises the device
 * (a diagnostic: tests use it to pin which path produced a result). */
int sagnn_range_redo_count(int64_t* count, int reset);

/* Copies the calling thread's last error text (NUL-terminated, truncated to cap) and
 * returns its full length. */
size_t sagnn_last_error(char* buf, size_t cap);

/* ------------------------------------------------------------------------------------
 * Per-launch timing with HIP events recorded on the launch stream (bench.py's roofline
 * figure). sagnn_profile_enable(capacity) pre-creates `capacity` event pairs and turns
 * recording on (capacity 0 turns it off and frees them); every kernel launch the library
 * issues then takes one slot until they run out. sagnn_profile_read synchronises on the
 * recorded events, returns up to `cap` records in issue order and clears the log.
 * kind: 0 = SpMM row/chunk kernel (units_a = nnz, units_b = n_rows), 1 = SpMM fix-up,
 *       2 = LSTM (or the GRU forward of sagnn_gru_fwd_f32), 3 = layer-norm, 4 = MHSA+mean (units_a = n, units_b = t),
 *       5 = an entry of the sequence attention (seq_attn.hip: gather, attention, pool, additive pool and
 *       their backwards; units_a = n_slots, units_b = pos_length),
 *       6 = sagnn_softmax_loss_f32 or its backward in SAGNN_SOFTMAX_FULL (units_a = n_queries, units_b = n_items),
 *       7 = the same entries in a candidate mode (units_a = n_queries, units_b = n_cand).
 * -------------------------------------------------------------------------------- */
int sagnn_profile_enable(int capacity);
int sagnn_profile_read(float* ms, int32_t* kind, int64_t* units_a, int64_t* units_b, int cap,
                       int* n_out);

/* ------------------------------------------------------------------------------------
 * CSR validation (host). Replaces nothing in the reference: TF-CPU raised
 * InvalidArgument from GatherV2 on an out-of-range index (model.py:86); the kernels do
 * not bounds-check, so the host wrapper calls this once per adjacency at load time.
 * -------------------------------------------------------------------------------- */
int sagnn_csr_check_host(const int32_t* h_rowptr, const int32_t* h_colidx,
                         int64_t n_rows, int64_t n_src, int64_t nnz);

/* ------------------------------------------------------------------------------------
 * SpMM plan: per-adjacency metadata, built once (the reference bakes each adjacency into
 * the TF graph as a constant SparseTensor once, model.py:227-237).
 *
 * Rows are handled by degree class:
 *   deg <= short_thresh            one lane-group (d/4 lanes) per row, several rows per wave
 *   short < deg <= long_thresh     one whole wavefront per row
 *   deg > long_thresh              split into chunks of <= chunk_edges edges, one wavefront
 *                                  per chunk into a partial-sum workspace, then a fix-up
 *                                  pass adds the partials in chunk order (deterministic,
 *                                  no atomics)
 * Only the third class needs stored metadata (the chunk list).
 * -------------------------------------------------------------------------------- */
typedef struct sagnn_spmm_plan sagnn_spmm_plan;

typedef struct sagnn_spmm_tuning {
  int32_t short_thresh;  /* 0 = default */
  int32_t long_thresh;   /* 0 = default */
  int32_t chunk_edges;   /* 0 = default; rounded up to a multiple of 64 */
  int32_t reserved;
} sagnn_spmm_tuning;

typedef struct sagnn_spmm_plan_info {
  int64_t n_rows, n_src, nnz;
  int64_t n_long_rows;   /* rows with deg > long_thresh */
  int64_t n_chunks;      /* total chunks over all long rows */
  int32_t short_thresh, long_thresh, chunk_edges;
  int32_t max_degree;
  int32_t on_device;     /* 1 if chunk metadata was uploaded (d_rowptr given) */
  int32_t weighted;      /* 1 if edge weights are set (sagnn_spmm_plan_set_weights); was `reserved`, always 0 before */
} sagnn_spmm_plan_info;

/* h_rowptr: host copy of rowptr [n_rows+1] (read during the call only).
 * d_rowptr/d_colidx: device CSR, must outlive the plan. Pass both NULL to build a
 * host-only plan (no GPU touched) — used by the CPU test-suite to check the chunking. */
int sagnn_spmm_plan_create(const int32_t* h_rowptr, const int32_t* d_rowptr,
                           const int32_t* d_colidx, int64_t n_rows, int64_t n_src,
                           int64_t nnz, const sagnn_spmm_tuning* tuning /* nullable */,
                           sagnn_spmm_plan** plan_out);
int sagnn_spmm_plan_destroy(sagnn_spmm_plan* plan);
int sagnn_spmm_plan_get_info(const sagnn_spmm_plan* plan, sagnn_spmm_plan_info* info);
/* Copies the chunk list to host arrays of capacity `cap` entries each (cap >= n_chunks).
 * chunk i covers edges [e_begin[i], e_end[i]) of row rows[i]; chunks of one row are
 * consecutive and in edge order. */
int sagnn_spmm_plan_copy_chunks(const sagnn_spmm_plan* plan, int32_t* rows, int32_t* e_begin,
                                int32_t* e_end, int64_t cap);
/* Edge weights (opt-in; not in the reference, whose normalised edge values are cast to int32 and never read:
 * DataHandler.py:53-59, model.py:84-86). d_weights: device array of nnz floats in colidx order, BORROWED: it must
 * outlive the plan or be cleared first; NULL clears the weights. Refused for a NULL plan and for a host-only plan.
 *
 * With weights set, every entry that takes the plan computes
 *     s[r,:] = sum over the row's stored edges e, in order, of w[e] * X[colidx[e],:]
 * accumulated as acc = fmaf(w[e], x, acc) (one rounding per edge and element), and everything after s (activation,
 * mask_out, residual, running sums, out2) is unchanged: sagnn_spmm_f32, _ex_f32, _drop_f32, sagnn_gnn_interval_* and
 * their backwards. Under edge dropout a dropped edge is still a gather that is never issued, its weight is ignored, and
 * scale = 1/keep multiplies the finished weighted sum. The weights are not checked on the device: NaN or Inf values are
 * the caller's to keep out. A plan without weights runs exactly the kernels it ran before this entry existed.
 *
 * sagnn_spmm_batch_create reads the weight pointers of its 2 T plans at creation (later changes to a plan do not reach
 * the batch) and fails when some plans have weights and others do not; sagnn_gnn_stack_* and their backwards follow
 * the batch.
 *
 * ADJOINT CONTRACT with weights: the backward entries run the same kernels on the adjoint plans (below). For a correct
 * gradient the adjoint plan must carry the SAME weight for the same (user, item) edge as the forward plan it
 * transposes. The library does not check this; the Python layer guarantees it (graph.interval_pair(norm="sym")). */
int sagnn_spmm_plan_set_weights(sagnn_spmm_plan* plan, const float* d_weights);
/* Bytes of device workspace sagnn_spmm_f32 needs for feature width d (0 if no long rows). */
size_t sagnn_spmm_workspace_bytes(const sagnn_spmm_plan* plan, int d);

/* ------------------------------------------------------------------------------------
 * sagnn_spmm_f32 — replaces Recommender.messagePropagate (model.py:80-92) together with
 * the residual add (model.py:124-125) and the running tf.add_n (model.py:126-127):
 *
 *     s[r,:]   = sum over edges (r,c) of X[c,:]          GatherV2 + SegmentSum (:86-87);
 *                                                        rows without edges give 0 (:87-91)
 *     y[r,:]   = max(leaky*s, s) + residual[r,:]         Activate 'leakyRelu' (NNLayers.py:136)
 *                                                        + embs[-1]          (model.py:124)
 *     out[r,:]     = y            (if out     != NULL)
 *     acc_out[r,:] = acc_in + y   (if acc_out != NULL; acc_in NULL means 0)
 *
 * Edge values are ignored, as in the reference (model.py:84, :86), unless the plan carries weights
 * (sagnn_spmm_plan_set_weights above: s[r,:] = sum of w[e] * X[c,:]). residual may be NULL.
 * acc_in may alias residual and may alias acc_out (in-place running sum). out/acc_out
 * must not alias X. At least one of out/acc_out is required.
 * -------------------------------------------------------------------------------- */
int sagnn_spmm_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                   const float* residual, int64_t ldr, float leaky, float* out, int64_t ldo,
                   const float* acc_in, int64_t ld_acc_in, float* acc_out, int64_t ld_acc_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Extended epilogue for training (sagnn_spmm_ex_f32); zero-initialise and fill what is used.
 *   s = A·X;  y = max(leaky*s, s) + residual;  out = y;  acc_out = acc_in + y
 *   mask_out [n_rows, d/4] bytes: bit j of byte l is 1 iff the activation passed s[4l+j] through
 *       with slope 1 (tf.maximum(leaky*x, x) sends the gradient to its FIRST argument on ties,
 *       so x = 0 counts as slope `leaky`: reference Utils/NNLayers.py:136)
 *   out2 = v * (mask_in bit ? 1 : slope2), v = the accumulated value if acc_out is given, else y
 *       (what the next backward step gathers). */
typedef struct sagnn_spmm_epilogue {
  float leaky;
  const float* residual; int64_t ldr;
  float* out; int64_t ldo;
  const float* acc_in; int64_t ld_acc_in;
  float* acc_out; int64_t ld_acc_out;
  uint8_t* mask_out;
  const uint8_t* mask_in;
  float* out2; int64_t ldo2; float slope2;
  const float* acc_in2; int64_t ld_acc_in2;   /* optional second addend: acc_out = acc_in + acc_in2 + y */
} sagnn_spmm_epilogue;

int sagnn_spmm_ex_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                      const sagnn_spmm_epilogue* epilogue, void* workspace, size_t workspace_bytes,
                      void* stream);
/* out[r, :] = g[r, :] * (mask bit ? 1 : slope), mask [n_rows, d/4] bytes as sagnn_spmm_ex_f32 records them: the seed of the
 * backward chain of the interval stack, for hosts that run the chain on row slices themselves (T < world sharding). */
int sagnn_mask_scale_f32(const float* g, int64_t ldg, const uint8_t* mask, float slope, float* out, int64_t ldo,
                         int64_t n_rows, int d, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch over the T intervals. The loop body of model.py:118-129 is independent per interval, so a layer of the stack
 * is 2 T independent SpMMs (T with rows = users, T with rows = items); on dataset-sized graphs (tens of thousands of
 * rows) each is a launch of a few microseconds and the stack is bound by its 2 T L launches (+ as many fix-ups). A
 * batch object ties the T interval plans together: a block of the batched kernel finds (direction, interval, row block)
 * by division, every per-interval operand is a SLAB — interval k's [N, d] matrix starts `slab` elements after interval
 * k-1's, rows `ld` apart — so u0 [T, U, d] is (ld = d, slab = U d) and a column of the [N, T, d] tensor the fusion reads
 * is (ld = T d, slab = d). One row launch and (if any interval has long rows) ONE fix-up launch per layer:
 * Amazon-shaped T = 5, L = 3: 60 launches -> 6.
 *
 * sagnn_spmm_batch_create keeps the plans' device CSR pointers: the plans must outlive the batch. Every interval must
 * have the same user / item counts. Workspace: sagnn_spmm_batch_workspace_bytes (partial sums of all long-row chunks).
 * -------------------------------------------------------------------------------- */
typedef struct sagnn_spmm_batch sagnn_spmm_batch;
int sagnn_spmm_batch_create(const sagnn_spmm_plan* const* plans_user, const sagnn_spmm_plan* const* plans_item,
                            int n_intervals, sagnn_spmm_batch** batch_out);
int sagnn_spmm_batch_destroy(sagnn_spmm_batch* batch);
size_t sagnn_spmm_batch_workspace_bytes(const sagnn_spmm_batch* batch, int d);

/* ------------------------------------------------------------------------------------
 * Edge dropout of the interval graphs (opt-in, training only; not in the reference, whose edgeDropout rewrites edge
 * VALUES that messagePropagate never reads: model.py:93-102 vs :84-86). The same kernels with one more step: the lane
 * that loads an edge's column index decides whether the edge takes part.
 *
 *   keep(edge) = word 0 of Philox4x32-10(key = seed (low word first), counter = (user id, item id, tag, step))
 *                < keep_threshold
 *   tag        = (interval k << 8) | (layer l << 1) | dir    dir 0: the user-side product A e_i^l,
 *                                                            dir 1: the item-side product A^T e_u^l
 *   s[r,:]     = scale * sum over KEPT edges (r,c) of X[c,:]  then the epilogue of sagnn_spmm_ex_f32
 *
 * The decision depends on the edge's (user id, item id) only: not on its position in a CSR, not on the plan that
 * stores it, not on the degree class that processes it. Duplicated stored entries share one decision. Hence the masked
 * pattern of a product and the masked pattern of its exact transpose are transposes of each other, and the ADJOINT
 * CONTRACT (below) carries over: the backward of layer l's user-side product runs on rows = items with the USER-side
 * tag, the backward of the item-side product on rows = users with the item-side tag (the stack entries do this).
 * keep_threshold = min(floor(keep * 2^32), 2^32 - 1) and scale = 1 / keep are computed by the host, once. Draws of
 * different (k, l, dir, step) are independent. No atomics: a row's result is a deterministic function of its inputs.
 *
 * An entry that drops checks the sagnn_edge_drop before anything else: NULL, keep_threshold = 0, scale not finite or
 * <= 0, n_layers > 127, an interval index >= 2^23 are refused with no device work done.
 * -------------------------------------------------------------------------------- */
typedef struct sagnn_edge_drop {
  uint64_t seed;
  uint32_t step;
  uint32_t keep_threshold;
  float scale;
} sagnn_edge_drop;

/* sagnn_spmm_ex_f32 as ONE masked product: `tag` as given, rows_are_users != 0 when the plan's rows are users (its
 * column indices items), 0 when its rows are items. The same tag on the transposed plan with the flag swapped gives
 * the exact transpose of the mask. */
int sagnn_spmm_drop_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                        const sagnn_spmm_epilogue* epilogue, const sagnn_edge_drop* drop, uint32_t tag,
                        int rows_are_users, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------
 * Time-aware messages (the term the reference comments out at model.py:86). Every stored edge of a plan
 * carries a bucket id (sagnn_spmm_plan_set_buckets) and every product of the stack (interval k, layer l, direction dir;
 * dir 0: rows are users, 1: rows are items) has a table TE[k,l,dir] of n_buckets rows of d floats:
 *
 *   s[r,:] = sum over the edges e of row r of  w[e] * ( X[col[e],:] + TE[k,l,dir][bucket[e],:] )     (w = 1: unweighted)
 *
 * then the epilogue of sagnn_spmm_ex_f32. X + TE is rounded once, then accumulated as the plan's kernels accumulate.
 * The gradient into X is that of the product without time; the backward entries add
 *
 *   dTE[k,l,dir][b,:] = sum over the edges e with bucket[e] = b of  w[e] * gm[row[e],:]
 *
 * with gm the masked gradient at that product's rows: an SpMM whose rows are buckets, run on the "time adjoint" plans
 * the caller builds (n_rows = n_buckets, n_src = the product's row count, colidx = the row of each edge in stable
 * bucket order, the weights permuted alongside). No atomics: dTE is a deterministic function of its inputs.
 *
 * An entry with time refuses (SAGNN_ERR_ARG, before any launch) a plan or batch without buckets, a bucket count that
 * differs from time->n_buckets, and a non-NULL `drop`: edge dropout and time do not combine.
 * -------------------------------------------------------------------------------- */
/* d_buckets: [nnz] uint16 in colidx order, every value < n_buckets <= 65535 (checked by the caller), borrowed like the
 * weights. NULL clears them. Set before sagnn_spmm_batch_create, which copies the pointer. */
int sagnn_spmm_plan_set_buckets(sagnn_spmm_plan* plan, const uint16_t* d_buckets, int32_t n_buckets);

typedef struct sagnn_edge_time {
  const float* te;          /* TE[0,0,0]; a table is [n_buckets, d], rows d apart, 16-byte aligned */
  int64_t stride_interval;  /* elements from TE[k,l,dir] to TE[k+1,l,dir] */
  int64_t stride_layer;     /*                          to TE[k,l+1,dir] */
  int64_t stride_dir;       /*                          to TE[k,l,1] from TE[k,l,0] */
  int32_t n_buckets;
  /* the backward entries only */
  float* dte;                         /* written: dTE, laid out like te */
  const sagnn_spmm_plan* adj_user;    /* interval entries: the time-adjoint plans of the user-side (dir 0) product */
  const sagnn_spmm_plan* adj_item;    /*                   and of the item-side (dir 1) product */
  const sagnn_spmm_batch* adj_batch;  /* stack entries: sagnn_spmm_time_batch_create of the 2 T time-adjoint plans */
  void* adj_workspace;                /* sagnn_spmm[_batch]_workspace_bytes of the adjoint plans (the larger) / batch */
  size_t adj_workspace_bytes;
} sagnn_edge_time;

/* The 2 T time-adjoint plans of a model as one batch: every plan has n_buckets rows; the user-side ones gather from U
 * rows, the item-side ones from I rows. (sagnn_spmm_batch_create insists on transposed pairs; these are not.) */
int sagnn_spmm_time_batch_create(const sagnn_spmm_plan* const* adj_user, const sagnn_spmm_plan* const* adj_item,
                                 int n_intervals, sagnn_spmm_batch** batch_out);

/* One product with the table time->te (the strides are not read). `drop` must be NULL. */
int sagnn_spmm_time_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                        const sagnn_spmm_epilogue* epilogue, const sagnn_edge_drop* drop, const sagnn_edge_time* time,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * The GNN stack — the loop model.py:118-129 (L layers, both directions, simultaneous update, residuals, add_n), issued
 * from C. Four entries: forward or backward, of ONE interval k (2 L SpMM launches on its plan pair) or of a BATCH of T
 * intervals (one launch per layer, above). Per interval:
 *
 *   e_u^0 = u0, e_i^0 = i0
 *   e_u^{l+1} = leaky(A   e_i^l) + e_u^l        plan_user: rows = users, cols = items
 *   e_i^{l+1} = leaky(A^T e_u^l) + e_i^l        plan_item: rows = items, cols = users
 *   user_out = sum_{l=0..L} e_u^l ;  item_out = sum_{l=0..L} e_i^l
 *
 * The outputs are written with row strides ld_out, so an interval entry can target row k of an [N, T, d] slab directly
 * (replaces tf.stack + tf.transpose, model.py:131-134). The backward (what tf.gradients builds for the loop): given
 * G_u = dL/d user_out, G_i = dL/d item_out and the masks the forward recorded, writes dL/d u0 and dL/d i0 — the same
 * SpMM kernel with the roles of the two adjacencies swapped (the reference already holds both, model.py:234-236).
 *
 * ADJOINT CONTRACT: the backward's plan_user (rows = users) must be the exact transpose, multiplicities included,
 * of the item-side pattern the forward pass used, and plan_item that of the user-side pattern; the backward's `batch`
 * must tie such plans, per interval. For matrices without duplicated stored entries these are the forward plans
 * themselves; with duplicates (forward counts one twice, DataHandler.transpose merges it: DataHandler.py:9-11) the
 * caller passes plans of the exact transposes — the library cannot tell the two cases apart from the handles, so the
 * host side checks it (sa-gnn_amd/graph.py interval_pair, ops._adjoint_pair).
 *
 * `edges` names the form of every product; it is not inferred from which pointer is set:
 *   SAGNN_EDGES_PLAIN  drop and time must be NULL.
 *   SAGNN_EDGES_DROP   edge dropout (above) under `drop`. An interval entry drops with the tags of interval
 *                      `interval`, interval k of a batch with those of k. The backward takes the sagnn_edge_drop (and
 *                      interval) of its forward call.
 *   SAGNN_EDGES_TIME   time-aware messages (above) under `time`; drop must be NULL. An interval entry works on
 *                      TE[interval,:,:], a stack entry on all of it. The forward's plans / batch carry the buckets; the
 *                      backward's need none, it reduces dTE through time->adj_*.
 * A NULL args, an `edges` outside these three and PLAIN with a drop or time set are refused before any launch.
 * -------------------------------------------------------------------------------- */
typedef struct sagnn_gnn_side {     /* the operands of one node type (users or items), N rows */
  const float* in;   int64_t ld_in,  slab_in;    /* forward: e^0 (u0 / i0); backward: G = dL/d out */
  float*       out;  int64_t ld_out, slab_out;   /* forward: sum of the layers; backward: dL/d e^0 */
  float*       scratch;                          /* forward [2,T,N,d] (NULL if n_layers <= 1); backward [4,T,N,d] */
  uint8_t*     mask;                             /* [T, n_layers, N, d/4]; forward writes (both sides or neither), backward reads */
} sagnn_gnn_side;

enum { SAGNN_EDGES_PLAIN = 0, SAGNN_EDGES_DROP = 1, SAGNN_EDGES_TIME = 2 };

typedef struct sagnn_gnn_args {
  sagnn_gnn_side user, item;
  int d, n_layers;
  float leaky;
  int edges;                       /* SAGNN_EDGES_* */
  const sagnn_edge_drop* drop;     /* SAGNN_EDGES_DROP */
  const sagnn_edge_time* time;     /* SAGNN_EDGES_TIME */
  int interval;                    /* interval entries: the k of the drop tags / of TE[k]; stack entries do not read it */
  void* workspace; size_t workspace_bytes;   /* sagnn_spmm_workspace_bytes (the larger of the two plans) / _batch_ */
} sagnn_gnn_args;

/* The interval entries take T = 1 and do not read slab_in / slab_out. */
int sagnn_gnn_interval_f32(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item, const sagnn_gnn_args* args,
                           void* stream);
int sagnn_gnn_interval_bwd_f32(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item,
                               const sagnn_gnn_args* args, void* stream);
int sagnn_gnn_stack_f32(const sagnn_spmm_batch* batch, const sagnn_gnn_args* args, void* stream);
int sagnn_gnn_stack_bwd_f32(const sagnn_spmm_batch* batch, const sagnn_gnn_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * Interval fusion (model.py:135-155). x[node, interval, :] is read at
 * x + node*ld_n + interval*ld_t (elements): [n, t, d] storage is ld_t = d, ld_n >= t*d (what
 * tf.stack + tf.transpose produce, model.py:131-134); [t, n, d] storage is ld_n = d,
 * ld_t >= n*d (what the interval-sharded exchange delivers). Outputs h / y are [n, t, d] with
 * node stride ld_h / ld_y and the t*d block of a node dense.
 *
 * sagnn_lstm_fwd_f32 — dynamic_rnn(MultiRNNCell([DropoutWrapper(BasicLSTMCell(d))]))
 *   (model.py:135-146) at keep probability 1: TF 1.14 BasicLSTMCell, kernel W [2d, 4d]
 *   row-major (rows 0..d-1 multiply x_t, rows d..2d-1 multiply h), bias b [4d], gate
 *   order i, j, f, o;  c' = c*sigmoid(f + forget_bias) + sigmoid(i)*tanh(j);
 *   h' = tanh(c')*sigmoid(o); zero initial state. Writes h for every step: [n, t, d].
 *   drop_scale (nullable) [n, t, d] multiplies the EMITTED h only (DropoutWrapper's
 *   output_keep_prob; the recurrent state is not dropped).
 *
 * sagnn_layernorm_td_f32 — tf.contrib.layers.layer_norm defaults (model.py:152-153):
 *   mean/variance over (t, d) jointly per node, gamma/beta [d], eps = 1e-12 inside rsqrt.
 *
 * sagnn_mhsa_mean_f32 — MultiHeadSelfAttention.attention (Utils/attention.py:55-78) with
 *   ScaledDotProductAttention (:35-45), then tf.reduce_mean(axis=1) (model.py:154-155):
 *   Q/K/V = x@W+b (W [d, d] row-major, in x out), heads of d_k = d/heads,
 *   scores = exp(Q K^T / sqrt(d_k)) (no max subtraction), attn = scores/(rowsum + 1e-8),
 *   context = attn V, mean over the t query positions -> out [n, d].
 *
 * sagnn_interval_fusion_f32 — the three stages back to back on `stream` with the LSTM
 *   output kept in a caller-provided workspace (sagnn_interval_fusion_workspace_bytes) and
 *   normalised in place; only out [n, d] is a result.
 *
 * ARITHMETIC of the GEMM-shaped stages (the gate product [x_t | h] W and the three dense layers)
 *   where the default engine takes its f16 x 2 kernels (csrc/engine.cpp): fp32 in, fp32 out, evaluated on the 16-bit
 *   matrix cores over SPLIT operands: two round-to-nearest f16 pieces per value (v = v1 + v2'/4096), three piece
 *   products, fp32 accumulation. The split represents v to 2^-23 |v| inside a window — |v| < 32768 at the top, and an
 *   ABSOLUTE floor of 2^-37 at the bottom — so what is guaranteed is:
 *     - every operand goes through a range check on its way to the matrix cores: a tile that holds |v| >= 32768, or
 *       an aligned 4-element segment that is non-zero but below 2^-18 as a whole (an input row of 1e-9), is
 *       re-evaluated in the kernel with fp32 fmaf chains. Such inputs get exactly an fp32 evaluation.
 *     - on the fast path each operand element is within max(2^-23 |v|, 2^-37) of its fp32 value, i.e. within
 *       2^-19 of its segment's largest element at worst and 2^-23 for segments above 2^-14 (every layer-normed row,
 *       every embedding sum): as close to the float64 product as an fp32 fmaf chain for such rows, not bit-identical
 *       to one.
 *     - gradients have no natural scale, so the attention-backward tail (sagnn_attn_bwd_tail_f32) scales every row
 *       of dQ|dK|dV by an exact power of two before the split: dy is accurate per ROW (relative to that row's own
 *       largest gradient, from 1e-38 to 1e38), dW / db relative to the sum of the magnitudes of their terms.
 *   sagnn_set_engine(SAGNN_ENGINE_F32) selects the exact-fp32 kernels instead. Results are deterministic run to run
 *   under every engine.
 *
 * STRIDE LIMITS of the LSTM forward entries (sagnn_lstm_fwd_f32, _state_f32, _train_f32, and sagnn_interval_fusion_f32
 *   through its LSTM). n, and with it every offset n * ld, is 64-bit everywhere; what is limited is the ROW STRIDE where
 *   a kernel takes a 64-bit base per tile of rows and addresses inside the tile with 32-bit byte offsets:
 *     - the f16 x 2 kernel (d = 32, 64 under SAGNN_ENGINE_F16X2; 96-row tiles) takes ld_h < 2^22 and t * d < 2^18. This
 *       limit REROUTES: from ld_h = 2^22 on the same call runs the fp32 matrix-core kernel, results to the same bounds.
 *       ld_n and ld_t are not limited on this kernel.
 *     - the fp32 matrix-core kernel (d = 32, 64; 32-row tiles) takes ld_n < 2^24, ld_h < 2^24 and t * d < 2^20. This
 *       limit REFUSES: SAGNN_ERR_ARG before any device work, under both matrix engines.
 *   The d = 128 and VALU kernels, h_init (ld_hi), every attention entry (ld_n, ld_t, ld_out, ld_g), the dense products,
 *   the SpMM and the row gather / scatter address with 64-bit offsets and have no such limit. The GRU's and the BPTT's
 *   limits are stated at their entries below. tests/test_gpu_far_offsets.py runs each kernel at the last stride admitted.
 * -------------------------------------------------------------------------------- */
int sagnn_lstm_fwd_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, const float* W,
                       const float* b, float forget_bias, const float* drop_scale, float* h,
                       int64_t ld_h, void* stream);
/* The same recurrence continued from a given state: h_init [n, d] (row stride ld_hi) and c_init
 * [n, d] (both NULL = zero state, i.e. sagnn_lstm_fwd_f32), c_final [n, d] receives the cell state
 * after the last step (NULL = not wanted). A sequence cut into consecutive calls is bit-identical
 * to one call; the multi-GPU pipeline uses this to run the steps of the intervals that have
 * already arrived while the last exchange round is still in flight. */
int sagnn_lstm_fwd_state_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                             const float* W, const float* b, float forget_bias, const float* drop_scale,
                             const float* h_init, int64_t ld_hi, const float* c_init, float* h, int64_t ld_h,
                             float* c_final, void* stream);
int sagnn_layernorm_td_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                           const float* gamma, const float* beta, float eps, float* y,
                           int64_t ld_y, void* stream);
int sagnn_mhsa_mean_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                        const float* Wq, const float* bq, const float* Wk, const float* bk,
                        const float* Wv, const float* bv, float* out, int64_t ld_out,
                        void* stream);
/* "Wide" attention for any d that is a multiple of 32 (e.g. the MovieLens configuration, d = 128,
 * whose three [d, d] weights and Q|K|V tiles do not fit LDS together): Q|K|V by MFMA products
 * (sagnn_dense_nn_f32's kernel) into caller scratch [n, t, 3d], then a per-node attention kernel.
 * sagnn_interval_fusion_f32 and the Python wrappers route here for d other than 32 / 64 / 128 (d = 128, 16 heads
 * runs the split-operand kernels: attention over two column halves, the LSTM as one launch per step). */
size_t sagnn_mhsa_wide_workspace_bytes(int64_t n, int t, int d);
int sagnn_mhsa_mean_wide_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                             const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                             const float* bv, float* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                             void* stream);
/* layer_norm over (T, d) + attention + mean without the LSTM (model.py:152-155): what the
 * training forward calls after sagnn_lstm_fwd_train_f32. Workspace (bytes from
 * sagnn_ln_mhsa_mean_workspace_bytes, 0 on the fused matrix-core path) holds the normalised
 * tensor where the normalisation cannot ride on the attention kernel's operand. The query assumes
 * aligned x (base 16-byte aligned, ld_n and ld_t multiples of 4). An unaligned x never runs fused: its caller
 * reserves n*t*d*4 + sagnn_mhsa_wide_workspace_bytes(n, t, d) bytes, enough for either unfused kernel
 * (SAGNN_ERR_WORKSPACE with less than the kernel taken needs). */
size_t sagnn_ln_mhsa_mean_workspace_bytes(int64_t n, int t, int d, int heads);
int sagnn_ln_mhsa_mean_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                           const float* ln_gamma, const float* ln_beta, float ln_eps, const float* Wq,
                           const float* bq, const float* Wk, const float* bk, const float* Wv, const float* bv,
                           float* out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);
int sagnn_interval_fusion_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                              const float* lstm_W, const float* lstm_b, float forget_bias,
                              const float* ln_gamma, const float* ln_beta, float ln_eps,
                              const float* Wq, const float* bq, const float* Wk, const float* bk,
                              const float* Wv, const float* bv, float* out, int64_t ld_out,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t sagnn_interval_fusion_workspace_bytes(int64_t n, int t, int d);

/* ------------------------------------------------------------------------------------
 * Backward of the interval fusion: the gradients tf.gradients derives for
 * model.py:135-155. The host (sa-gnn_amd/autograd.py) sequences these entries with the dense
 * products below. Training needs d in {32, 64, 128, 192, 256}: the dense products take multiples of 32, and
 * sagnn_attn_bwd_f32 / sagnn_layernorm_td_bwd_f32 need 64 % d == 0 or d % 64 == 0 (SAGNN_ERR_DIM otherwise, so
 * d = 96, 160 and 224 run the forward only). Each of the five is checked against the float64 oracle; the fused
 * entries — attention-backward front and tail, the one-launch BPTT — say which shapes they cover through their
 * *_supported queries. sagnn_attn_bwd_f32 takes any d_k = d / heads (the fused fronts: powers of two).
 *
 * sagnn_lstm_fwd_train_f32 — sagnn_lstm_fwd_f32 that also stores the gate activations
 *   gates [n, t, 4d] = sigmoid(i) | tanh(j) | sigmoid(f + forget_bias) | sigmoid(o) and the cell
 *   state cell [n, t, d].
 * sagnn_attn_bwd_f32 — qkv [n, t, 3d] (Q | K | V rows, as x@W+b produced them) is overwritten
 *   with dQ | dK | dV given g_out = dL/d(mean-over-queries context) [n, d].
 * sagnn_layernorm_td_bwd_f32 — dy -> dh (may alias dy), dgamma/dbeta accumulated with atomics
 *   (zero them first).
 * sagnn_lstm_bwd_step_f32 — step ts of BPTT: dh_ext [n, t, d] (gradient arriving at the emitted
 *   h, scaled by drop_scale if given), dh_rec [n, d] (recurrent gradient, NULL at the last step),
 *   dc_in [n, d] (NULL at the last step) -> dgates [n, 4d] (pre-activation gradients, i|j|f|o)
 *   and dc_out [n, d].
 * sagnn_lstm_bwd_f32 — the whole BPTT in one launch (d in {32, 64}; sagnn_lstm_bwd_supported):
 *   x as given to the forward, h/gates/cell as sagnn_lstm_fwd_train_f32 stored them (h un-dropped,
 *   [n, t, d] dense), dh_ext [n, t, d] with row stride ld_dhe -> dx [n, t, d] dense, and
 *   dW [2d, 4d] / db [4d] ACCUMULATED with float atomics (zero them first). Gate gradients stay
 *   on chip: per 32-row chunk and step, d[x|h] = dG W^T and dW += [x|h]^T dG run as MFMA tiles.
 *   STRIDE LIMIT (sagnn_lstm_bwd_f32 and sagnn_lstm_bwd_ws_f32, both forms): ld_n < 2^25, ld_dhe < 2^25 and
 *   t * d < 2^20; a 32-row chunk is addressed with 32-bit element offsets from a 64-bit base. This limit REFUSES:
 *   SAGNN_ERR_ARG before any device work. n, and the contiguous h / gates / cell / dx with it, is not limited.
 * -------------------------------------------------------------------------------- */
int sagnn_lstm_fwd_train_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                             const float* W, const float* b, float forget_bias, const float* drop_scale,
                             float* h, int64_t ld_h, float* gates, float* cell, void* stream);
int sagnn_attn_bwd_f32(float* qkv, const float* g_out, int64_t ld_g, int64_t n, int t, int d, int heads,
                       void* stream);
int sagnn_layernorm_td_bwd_f32(const float* h, int64_t ld_h, const float* dy, int64_t ld_dy, int64_t n, int t,
                               int d, const float* gamma, float eps, float* dh, int64_t ld_dh, float* dgamma,
                               float* dbeta, void* stream);
int sagnn_lstm_bwd_step_f32(const float* gates, const float* cell, const float* dh_ext, int64_t ld_dhe,
                            const float* drop_scale, const float* dh_rec, int64_t ld_dhr, const float* dc_in,
                            float* dgates, float* dc_out, int64_t n, int t, int d, int ts, void* stream);
/* Front of the attention backward pass in one launch (shapes: sagnn_attn_bwd_front_supported, csrc/engine.cpp):
 * y = layer_norm(x) when apply_ln (else x), Q|K|V = y W + b, attention
 * backward given g_out = dL/d(mean context) [n, d] -> dqkv [n*t, 3d] (dQ | dK | dV rows) and, when
 * y_out is not NULL, y [n*t, d]. Replaces layernorm_td + dense_nn + attn_bwd of the recompute path. */
int sagnn_attn_bwd_front_supported(int d, int t, int heads);
int sagnn_attn_bwd_front_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                             const float* ln_gamma, const float* ln_beta, float ln_eps, int apply_ln,
                             const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                             const float* bv, const float* g_out, int64_t ld_g, float* dqkv, float* y_out,
                             void* stream);
/* Tail of the attention backward pass in one pass over dQ|dK|dV (d in {32, 64}): y [rows, d] is
 * OVERWRITTEN with dy = dqkv Wqkv^T; dWqkv [d, 3d] += y^T dqkv and dbqkv [3d] += column sums of dqkv
 * are accumulated with float atomics (zero them first). Wqkv = [Wq | Wk | Wv] as [d, 3d]. Replaces
 * sagnn_dense_tn_f32 + sagnn_dense_nn_f32 on the same operands (dqkv read once instead of twice). */
int sagnn_attn_bwd_tail_supported(int d);
int sagnn_attn_bwd_tail_f32(float* y, const float* dqkv, int64_t rows, int d, const float* Wqkv, float* dWqkv,
                            float* dbqkv, void* stream);
int sagnn_lstm_bwd_supported(int d);
int sagnn_lstm_bwd_f32(const float* x, int64_t ld_n, int64_t ld_t, const float* h, const float* gates,
                       const float* cell, const float* dh_ext, int64_t ld_dhe, const float* drop_scale,
                       const float* W, float* dx, float* dW, float* db, int64_t n, int t, int d, void* stream);
/* sagnn_lstm_bwd_f32 with the weight gradient as a SECOND PASS on the default engine: the BPTT launch leaves out its
 * dW product (fp32 MFMA: the larger part of its time) and stores the gate gradients time-major into the caller's
 * scratch ([t, n, 4d] floats = sagnn_lstm_bwd_workspace_bytes, 16-byte aligned); one pass over them then takes
 * dW += [x_s | h_{s-1}]^T dG_s on the 16-bit matrix cores over split operands, gate-gradient rows scaled by exact
 * powers of two as in the attention tail (ARITHMETIC above). Same arguments and results otherwise; where
 * csrc/engine.cpp does not select this form (no workspace, another engine), the call IS sagnn_lstm_bwd_f32. */
size_t sagnn_lstm_bwd_workspace_bytes(int64_t n, int t, int d);
int sagnn_lstm_bwd_ws_f32(const float* x, int64_t ld_n, int64_t ld_t, const float* h, const float* gates,
                          const float* cell, const float* dh_ext, int64_t ld_dhe, const float* drop_scale,
                          const float* W, float* dx, float* dW, float* db, int64_t n, int t, int d, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * GRU cell of the interval fusion (opt-in, --rnnCell gru). The reference builds its recurrent cell in a
 * function it names gru_cell() (model.py:135-136) that returns BasicLSTMCell; these entries run TF 1.14 GRUCell in its
 * place, with the same strides, outputs and dropout meaning as the LSTM block above. Per row, zero initial state,
 * s = 0 .. t-1:
 *     [r | u] = sigmoid([x_s | h] Wg + bg)       Wg [2d, 2d], bg [2d]; block order r, u
 *     c       = tanh([x_s | r.h] Wc + bc)        Wc [2d, d],  bc [d]
 *     h'      = u.h + (1 - u).c
 *   Wg / Wc row-major; rows 0..d-1 multiply x_s, rows d..2d-1 the state (the layout of the LSTM's W). drop_scale
 *   (nullable) [n, t, d] multiplies the EMITTED h only. d: a multiple of 32 up to 256 (SAGNN_ERR_DIM otherwise); x, h,
 *   the weights and every optional tensor 16-byte aligned with ld_n, ld_t, ld_h multiples of 4 (SAGNN_ERR_ALIGN).
 *   TensorFlow cannot be run beside this library: like the LSTM's, the floating-point side of this cell restates TF's
 *   documented source and is pinned by no reference run.
 *
 * ARITHMETIC: exact fp32 (v_mfma_f32_32x32x2_f32, an fmaf chain) under EVERY engine: sagnn_set_engine does not reach
 *   these entries, there is no f16 x 2 form of the GRU. Results are deterministic run to run, and a row's result does
 *   not depend on which other rows the call holds.
 *
 * sagnn_gru_fused_supported — 1 where sagnn_gru_fwd_f32 runs as ONE launch persistent over t (d = 32, 64), else 0:
 *   there the call runs one step at a time (two products by sagnn_dense_nn_f32's kernels and two element-wise launches
 *   per step; the counterpart of the LSTM's generic route, not built for speed) in a caller workspace of
 *   sagnn_gru_workspace_bytes = n * 3d floats, 16-byte aligned (0 where the fused kernel runs; SAGNN_ERR_WORKSPACE).
 *   STRIDE LIMIT of the one-launch form (d = 32, 64): ld_n < 2^24, ld_h < 2^24 and t * d < 2^19 (32-row tiles addressed
 *   with 32-bit byte offsets from a 64-bit base). This limit REFUSES: SAGNN_ERR_ARG before any device work. The per-step
 *   route and the two backward entries address with 64-bit offsets and have no such limit.
 * sagnn_gru_fwd_f32 — h [n, t, d] (node stride ld_h) for every step. gates / cand (both or neither): the training
 *   form, which also stores gates [n, t, 2d] = r | u after the sigmoid and cand [n, t, d] = c after the tanh, and h
 *   un-dropped as the backward reads it: drop_scale must then be NULL (SAGNN_ERR_ARG).
 *
 * Backward: per step, for every supported d (a one-launch BPTT is not built). For s = t-1 .. 0, the host runs
 *   sagnn_gru_bwd_cand_f32   dh = dh_ext[:, s] (. drop_scale) + dh_rec (NULL at the last step; row stride ld_dhr)
 *                            -> da_c = dh (1-u)(1-c^2), du = dh (h_{s-1} - c), dh_u = dh u, each [n, d] dense
 *   sagnn_dense_nn_f32       [dx_s | d(r.h)] = da_c Wc^T
 *   sagnn_gru_bwd_gates_f32  d_rh [n, d] (row stride ld_drh) holds d(r.h) on entry; -> da_g [n, 2d] =
 *                            [d(r.h) h_{s-1} r(1-r) | du u(1-u)], d_rh = dh_rec' = dh_u + d(r.h) r, and, when rh is not
 *                            NULL, rh [n, d] = r.h_{s-1} (the operand of Wc's recurrent weight gradient)
 *   sagnn_dense_nn_f32       [dx_s | dh_rec'] += da_g Wg^T (accumulate)
 *   with gates / cand / h as the training form stored them and h_{-1} = 0. The weight and bias gradients are
 *   sagnn_dense_tn(_seg)_f32 products of da_g / da_c against x_s, h_{s-1} and r.h_{s-1}.
 * -------------------------------------------------------------------------------- */
int sagnn_gru_fused_supported(int d);
size_t sagnn_gru_workspace_bytes(int64_t n, int t, int d);
int sagnn_gru_fwd_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, const float* Wg,
                      const float* bg, const float* Wc, const float* bc, const float* drop_scale, float* h,
                      int64_t ld_h, float* gates, float* cand, void* workspace, size_t workspace_bytes, void* stream);
int sagnn_gru_bwd_cand_f32(const float* gates, const float* cand, const float* h, const float* dh_ext, int64_t ld_dhe,
                           const float* drop_scale, const float* dh_rec, int64_t ld_dhr, float* da_c, float* du,
                           float* dh_u, int64_t n, int t, int d, int ts, void* stream);
int sagnn_gru_bwd_gates_f32(const float* gates, const float* h, const float* du, const float* dh_u, float* d_rh,
                            int64_t ld_drh, float* da_g, float* rh, int64_t n, int t, int d, int ts, void* stream);

/* ------------------------------------------------------------------------------------
 * Prediction head (reference model.py:156-173). The masked sum of item /
 * position embeddings (model.py:161-162) is sagnn_spmm_f32 on a per-batch CSR (row = batch slot,
 * columns = the unmasked sequence entries, leaky = 1); layer_norm and the length-1 MHSA are
 * sagnn_layernorm_td_f32 / sagnn_mhsa_mean_f32 with t = 1; what is left:
 *   sagnn_leaky_add_f32:  out = max(leaky*a, a) + b      (model.py:166; b nullable)
 *   sagnn_pair_score_f32: preds[e] = <U[uids[e]], I[iids[e]]> + <leaky(S[locs[e]]), A[iids[e]]>
 *                         (model.py:169-173; S/A/locs NULL drops the second term)
 * -------------------------------------------------------------------------------- */
int sagnn_leaky_add_f32(const float* a, const float* b, float* out, float leaky, int64_t count, void* stream);
int sagnn_pair_score_f32(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* S, int64_t lds,
                         const float* A, int64_t lda, const int32_t* uids, const int32_t* iids,
                         const int32_t* locs, float leaky, float* out, int64_t n_pairs, int d, void* stream);

/* ------------------------------------------------------------------------------------
 * Training-side operators (reference model.py:169-205, 241-250). All scatter
 * outputs (dU, dI, dS, dA, dX, dY, dF, dV, dw3, db3, loss) ACCUMULATE with float atomics: zero
 * them first. Dense gradient rows are [rows, d] contiguous. The slope of max(leaky*x, x) is `leaky` wherever
 * x <= leaky*x (tf.maximum sends the gradient to its first argument on ties: x = 0, a product of exactly 0).
 *   sagnn_pair_score_bwd_f32      backward of sagnn_pair_score_f32 given g [n_pairs]
 *   sagnn_prod_leaky_sum_f32      s[e] = sum_j leaky(X[uids[e]][j] * Y[iids[e]][j])   (model.py:191,199)
 *   sagnn_prod_leaky_sum_bwd_f32  its backward
 *   sagnn_meta_features_f32       m[e] = [F[u]*V[u] | F[u] | V[u]], u = uids[e]      (model.py:179)
 *   sagnn_meta_features_bwd_f32   its backward
 *   sagnn_leaky_f32               backward == 0: out = max(leaky*a, a); else out = g * slope(a)
 *   sagnn_rowdot_sigmoid_f32      w[e] = sigmoid(<A[e, :k], w3> + b3)                 (model.py:182)
 *   sagnn_rowdot_sigmoid_bwd_f32  dA[e, :k] = dz*w3, dw3 += sum dz*A[e], db3 += sum dz, dz = dw*w*(1-w)
 *   sagnn_hinge_f32               loss += scale * sum max(0, 1 - S*(pos - neg)), S = wp*sp - wn*sn
 *                                 (S = 1 when wp is NULL: model.py:244; weighted: model.py:196,202);
 *                                 writes d(loss)/d pos, neg, wp, wn; a row with 1 - S*(pos - neg) <= 0 has no term
 *                                 and zero gradients. The gradient outputs are optional IN PAIRS: dpos with dneg,
 *                                 dwp with dwn (both or neither; dwp / dwn only with wp); wp, wn, sp, sn all or none
 * Limits: pair entries (pair_score_bwd, prod_leaky_sum*) d = 4 * a power of two, <= 256; meta_features* d a multiple
 *   of 4 in [4, 256]; U, I, S, A, X, Y, F, V, the meta-feature block (out / dm, [n, 3d] dense) 16-byte aligned with
 *   strides that are multiples of 4 and >= d; S, A, locs, dS, dA all or none (none drops the second term);
 *   1 <= k <= 8192, lda >= k, ldda >= k (no alignment: the row-dot reads scalars; dA columns >= k are not written);
 *   counts >= 0 (0 returns SAGNN_OK at once) and small enough for one launch (SAGNN_ERR_ARG "grid too large").
 *   Ids are the caller's responsibility (never checked here). Every argument is checked before any device work.
 * -------------------------------------------------------------------------------- */
int sagnn_pair_score_bwd_f32(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* S, int64_t lds,
                             const float* A, int64_t lda, const int32_t* uids, const int32_t* iids,
                             const int32_t* locs, float leaky, const float* g, float* dU, float* dI, float* dS,
                             float* dA, int64_t n_pairs, int d, void* stream);
int sagnn_prod_leaky_sum_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, const int32_t* uids,
                             const int32_t* iids, float leaky, float* out, int64_t n_pairs, int d, void* stream);
int sagnn_prod_leaky_sum_bwd_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, const int32_t* uids,
                                 const int32_t* iids, float leaky, const float* g, float* dX, float* dY,
                                 int64_t n_pairs, int d, void* stream);
int sagnn_meta_features_f32(const float* F, int64_t ldf, const float* V, int64_t ldv, const int32_t* uids,
                            float* out, int64_t n, int d, void* stream);
int sagnn_meta_features_bwd_f32(const float* F, int64_t ldf, const float* V, int64_t ldv, const int32_t* uids,
                                const float* dm, float* dF, float* dV, int64_t n, int d, void* stream);
int sagnn_leaky_f32(const float* a, const float* g, float* out, float leaky, int64_t count, int backward,
                    void* stream);
int sagnn_rowdot_sigmoid_f32(const float* A, int64_t lda, const float* w3, const float* b3, float* out, int64_t n,
                             int k, void* stream);
int sagnn_rowdot_sigmoid_bwd_f32(const float* A, int64_t lda, const float* w3, const float* w, const float* dw,
                                 float* dA, int64_t ldda, float* dw3, float* db3, int64_t n, int k, void* stream);
int sagnn_hinge_f32(const float* pos, const float* neg, const float* wp, const float* wn, const float* sp,
                    const float* sn, float scale, float* loss, float* dpos, float* dneg, float* dwp, float* dwn,
                    int64_t n, void* stream);

/* out[i] = a[i] * b[i] (dropout scaling of the emitted LSTM output, model.py:139). */
int sagnn_mul_f32(const float* a, const float* b, float* out, int64_t count, void* stream);

/* One tf.train.AdamOptimizer step (model.py:248-250) with the L2 term of regLoss
 * (args.reg * Regularize(), model.py:245, Utils/NNLayers.py:159-175) folded into the gradient:
 *   g' = g + 2*l2*p;  m = b1*m + (1-b1)*g';  v = b2*v + (1-b2)*g'^2
 *   p -= lr*sqrt(1 - b2^step)/(1 - b1^step) * m / (sqrt(v) + eps)        (step counts from 1)
 * The caller applies the staircase decay lr = lr0 * decay^floor(step/decay_step) (model.py:249). */
int sagnn_adam_step_f32(float* param, const float* grad, float* m, float* v, int64_t count, float lr,
                        float beta1, float beta2, float eps, float l2, int64_t step, void* stream);

/* The same step for n_tensors parameter tensors in ONE launch (one per 48 tensors): host arrays of
 * device pointers / element counts / per-tensor l2. grads[i] == NULL means a zero gradient: TF's
 * minimize() differentiates loss + reg*Regularize() (model.py:245-250), so a registered tensor that
 * no forward op reads (timeEmbed, the dead [d,d] weights of model.py:81) still receives 2*l2*p and
 * decays under Adam. All pointers 16-byte aligned. */
int sagnn_adam_multi_f32(int n_tensors, float* const* params, const float* const* grads, float* const* m,
                         float* const* v, const int64_t* counts, const float* l2, float lr, float beta1,
                         float beta2, float eps, int64_t step, void* stream);

/* ------------------------------------------------------------------------------------
 * Dense products on the matrix cores (exact fp32), n rows huge, W small:
 *   sagnn_dense_nn_f32:  Y[n, dout] (+)= X[n, din] @ W[din, dout] + bias      (bias nullable;
 *       accumulate != 0 adds into Y). Replaces `inp @ W` of NNLayers.FC (Utils/NNLayers.py:108)
 *       and tf.layers.dense (Utils/attention.py:66-72) outside the fused kernels, and the
 *       input-gradient products of the backward pass.
 *   sagnn_dense_tn_f32:  dW[din, dout] += X[n, din]^T @ G[n, dout];  db[dout] += column sums of G
 *       (db nullable). The weight-gradient products; accumulates with float atomics, so zero
 *       dW/db first and expect run-to-run differences in the last bits.
 *   sagnn_dense_tn_seg_f32: the same sums over n_seg row SEGMENTS of seg_rows rows each, row i of segment s
 *       at X + s * x_seg + i * ldx and G + s * g_seg + i * ldg (strides in floats, multiples of 4;
 *       seg_rows * n_seg < 2^31): the weight gradient of a whole BPTT in one launch — x [n, t, d] in any
 *       node / interval strides against the stored gate gradients [t, n, 4d] — instead of one product per step.
 * din, dout: any multiples of 32. A W block that fits LDS stays resident there and the tall operand streams
 * past it; larger blocks (the d = 128 LSTM: [512, 256]) and the segmented form run a tiled GEMM
 * (dense_gemm.hip: 128 x 128 / 64 x 128 block tiles, split-K with atomics for the transposed form).
 * -------------------------------------------------------------------------------- */
int sagnn_dense_nn_f32(const float* X, int64_t ldx, int64_t n, int din, int dout, const float* W,
                       const float* bias, float* Y, int64_t ldy, int accumulate, void* stream);
int sagnn_dense_tn_f32(const float* X, int64_t ldx, const float* G, int64_t ldg, int64_t n, int din,
                       int dout, float* dW, float* db, void* stream);
int sagnn_dense_tn_seg_f32(const float* X, int64_t ldx, int64_t x_seg, const float* G, int64_t ldg, int64_t g_seg,
                           int64_t seg_rows, int n_seg, int din, int dout, float* dW, float* db, void* stream);

/* ------------------------------------------------------------------------------------
 * Full-catalogue retrieval (retrieval.hip): the best k items of every query row over the whole item table.
 *   score(b, i) = <Q[b], I[i]> in fp32 on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): every score is
 *   a fixed fmaf chain over k, a function of the query row and the item row alone. sagnn_set_engine does NOT
 *   apply to this entry. The model's head score <fu[u], fi[i]> + <leaky(att[b]), fi[i]> is this product with
 *   Q[b] = leaky(att[b]) + fu[u] (sagnn_leaky_add_f32) and I = fi.
 * Order (strict, total): higher score first; equal scores go to the lower item id (-0.0 == +0.0); a NaN score
 *   ranks below every number and is never returned.
 * Eligible items: every item of [0, n_items) except row b's exclusions. The optional exclusion list is a CSR
 *   (excl_rowptr [n_queries + 1], excl_items) of ascending ids per row, duplicates allowed; the ids are only
 *   compared, never used as addresses. target[b] is always eligible, even when its row excludes it.
 * Outputs: topk_items / topk_scores [n_queries, k] (contiguous), best first; slots past the number of eligible
 *   non-NaN items hold id -1 and score -inf. target_rank[b] (with target only) = the number of eligible items
 *   that come before target[b], from the same score values as the top k, so rank < k <=> topk_items[b, rank] ==
 *   target[b]; a NaN target score gives the number of eligible items (a miss); a target outside [0, n_items)
 *   gives -1.
 * A row's outputs depend on that row's inputs only (not on n_queries or its place in the batch) and are
 *   bit-identical between runs.
 * Limits: d in {32, 64, 128}; 1 <= k <= 128; 1 <= n_items < 2^31; ldq, ldi multiples of 4 and >= d; Q, I and
 *   workspace 16-byte aligned; workspace_bytes >= sagnn_score_topk_workspace_bytes(...). Every argument is
 *   checked before any device work. Two launches on `stream`, no allocation, no synchronisation (capturable).
 * -------------------------------------------------------------------------------- */
size_t sagnn_score_topk_workspace_bytes(int64_t n_queries, int64_t n_items, int d, int k);
int sagnn_score_topk_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries, int64_t n_items,
                         int d, int k, const int32_t* excl_rowptr, const int32_t* excl_items, const int32_t* target,
                         int32_t* topk_items, float* topk_scores, int64_t* target_rank, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Sampled-candidate evaluation (evaluate.hip): the reference's test epoch (model.py:430-510) scores testSize
 * candidates per user with the head and ranks the held-out target among them.
 *   scores[b, j] = <U[uids[b]], I[c]> + <leaky(S[b]), A[c]>, c = cand[b * ldc + j] (S / A NULL drops the second
 *   term): bit-identical to sagnn_pair_score_f32 for (uids[b], c, locs = b) — both run the same per-lane arithmetic
 *   and lane reduction (d / 4 lanes per pair).
 *   rank[b]: NaN scores count as -inf; with copies = {j : cand[b, j] == target[b]}, p = the highest score over the
 *   copies and f = the first copy scoring p, rank = #{j : s_j > p} + #{j < f : s_j == p} (the reference's stable
 *   descending sort, best-ranked copy; at p = -inf every NaN / -inf candidate before f counts). No copy, or
 *   target[b] < 0, gives -1 (a miss).
 * uids / target int32 [n_rows]; cand int32 [n_rows, C] at row stride ldc; rank int64 [n_rows]; scores (nullable)
 *   [n_rows, C] at ld_scores. Candidate and user ids are the caller's responsibility (never checked here).
 * A row's outputs depend on that row's inputs only (not on n_rows or its position) and are bit-identical between runs.
 * Limits: d a multiple of 4 in [4, 256] with d / 4 a power of two; 1 <= C <= 8192; ldc >= C; ld_scores >= C;
 *   strides multiples of 4 and >= d; U, I, S, A 16-byte aligned. Every argument is checked before any device work.
 *   One launch on `stream`, no allocation, no synchronisation (capturable).
 * -------------------------------------------------------------------------------- */
int sagnn_candidate_rank_f32(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* S, int64_t lds,
                             const float* A, int64_t lda, const int32_t* uids, const int32_t* cand, int64_t ldc,
                             const int32_t* target, float leaky, int64_t n_rows, int C, int d, int64_t* rank,
                             float* scores, int64_t ld_scores, void* stream);

/* ------------------------------------------------------------------------------------
 * Device sampling of the training batch (sampler.hip): the reference's sampleTrainBatch / negSamp /
 * sampleSslBatch (model.py:252-339, DataHandler.py:28-41) drawn by HIP kernels, and the head's masked sums
 * (model.py:161-162) read straight from the sampled sequence segments.
 * Random numbers: Philox4x32-10, key = seed (low word first), counter = (user id, draw index j, step, stream);
 *   a uniform integer on [0, n) is the high 64 bits of ((w0 << 32) | w1) * n from the first two output words
 *   (bias <= n / 2^64). Streams: 0 = the positive's `choose` (j = 0), 1 = negative j, 2 + k = SSL draw j of interval k
 *   (pair p is draws 2p and 2p + 1). A user's draws are a pure function of (seed, step, user id).
 * Sequences: seq_ptr [n_users + 1] (int64) into seq_items (every id in [0, n_items)). Banned lists: ban_ptr
 *   [n_users + 1] (int64) into ban_items, each row sorted and unique (the items a user may not draw as negatives).
 *
 * sagnn_sample_train_i32, per batch slot b < n_batch with u = bat_ids[b], n_pos = len(seq[u]) - 1:
 *   samp = clamp(min(train_sample_num, n_pos), 0), hi = max(min(pred_num + 1, n_pos - 3), 1), choose uniform on [1, hi];
 *   samp pairs at off = pair_off[b] + j (j < samp, off < n_pairs): uids[off] = uids[n_pairs + off] = u,
 *   iids[off] = seq[u][n_pos - choose], iids[n_pairs + off] = the r-th item outside the banned row (r uniform on
 *   [0, n_items - banned count); -1 if the row bans every item), uLocs_seq[off] = uLocs_seq[n_pairs + off] = b.
 *   Outputs are [2 n_pairs]; the caller sizes pair_off from the per-user samp, so nothing is copied back.
 *   The head's sequence per slot b < n_slots: seg_begin[b] (index into seq_items), seg_len[b] =
 *   min(max(n_pos - choose, 0), pos_length), the last seg_len items before the positive; slots >= n_batch get 0, 0.
 * sagnn_sample_ssl_i32, per interval k < n_intervals, slot b < n_batch: sub_ptr [n_intervals, n_users + 1] (int64)
 *   into sub_items (the user's distinct items of interval k), npair = min(ssl_num, n_k(u) / 2) pairs, pair p at
 *   off = ssl_off[k * n_batch + b] + 2p and off + 1 (< n_out): iids two uniform draws with replacement from the row,
 *   uids = u, uLocs_seq = b at both.
 * sagnn_seq_sum_f32: seq_tok[b] = sum_{j < seg_len[b]} fi[seq_items[seg_begin[b] + j]] and pos_tok[b] =
 *   sum_{p = P - seg_len[b]}^{P - 1} pos_embed[p], both summed in ascending j / p from 0.0f (the order the SpMM sums a
 *   row of at most 16 entries, so equal bit for bit to the per-batch CSR form there); outputs [n_slots, d] at ldo.
 * sagnn_seq_sum_bwd_f32: d_fi[seq_items[seg_begin[b] + j]] += g_seq[b] (ACCUMULATES; float atomics on whole rows, so
 *   the last bits may differ from run to run) and d_pos[p] = sum over b in ascending order with seg_len[b] >= P - p
 *   of g_pos[b] (WRITTEN; deterministic).
 * Limits: d a multiple of 4 in [4, 256]; feature pointers 16-byte aligned, strides multiples of 4 and >= d;
 *   pos_length > 0; 0 < n_items < 2^31; 0 <= step < 2^32. Every argument is checked before any device work. One or two
 *   launches on `stream`, no allocation, no synchronisation.
 * -------------------------------------------------------------------------------- */
int sagnn_sample_train_i32(const int32_t* bat_ids, int64_t n_batch, int64_t n_slots, const int64_t* seq_ptr,
                           const int32_t* seq_items, const int64_t* ban_ptr, const int32_t* ban_items, int64_t n_users,
                           int64_t n_items, int train_sample_num, int pred_num, int pos_length, const int64_t* pair_off,
                           int64_t n_pairs, uint64_t seed, int64_t step, int32_t* uids, int32_t* iids,
                           int32_t* uLocs_seq, int64_t* seg_begin, int32_t* seg_len, void* stream);
int sagnn_sample_ssl_i32(const int32_t* bat_ids, int64_t n_batch, int n_intervals, const int64_t* sub_ptr,
                         const int32_t* sub_items, int64_t n_users, int ssl_num, const int64_t* ssl_off, int64_t n_out,
                         uint64_t seed, int64_t step, int32_t* uids, int32_t* iids, int32_t* uLocs_seq, void* stream);
int sagnn_seq_sum_f32(const float* fi, int64_t ldf, int64_t n_items, const float* pos_embed, int64_t ldp,
                      int pos_length, const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin,
                      const int32_t* seg_len, int64_t n_slots, int d, float* seq_tok, float* pos_tok, int64_t ldo,
                      void* stream);
int sagnn_seq_sum_bwd_f32(const float* g_seq, const float* g_pos, int64_t ldg, const int32_t* seq_items, int64_t n_flat,
                          const int64_t* seg_begin, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                          float* d_fi, int64_t ld_dfi, int64_t n_items, float* d_pos, int64_t ld_dpos, void* stream);

/* ------------------------------------------------------------------------------------
 * Row subsets of the interval fusion for training (fusion_rows.hip). The fusion is independent per node and the loss
 * reads few rows of its outputs, so a training step may fuse only the rows a batch reads: mark them, compact the
 * marks into ascending row ids, gather those rows into a dense [cap, t, d] block for the fusion entries above, and
 * scatter the results back.
 * sagnn_rows_mark_i32: flags[ids[i]] = 1 for every i < n_ids with 0 <= ids[i] < n_rows (other ids are skipped).
 * sagnn_rows_mark_seg_i32: the same for seq_items[seg_begin[b] + j], b < n_slots, j < min(seg_len[b], max_len), entries
 *   outside [0, n_flat) skipped (the device sampler's sequence segments, read as sagnn_seq_sum_f32 reads them).
 *   Several marks may go into one flag buffer (uint8 [n_rows], zero before the first mark).
 * sagnn_rows_compact_i32: rows[0 .. count) = the flagged row ids in ascending order, *count (device int32) = how many
 *   were flagged, slots [count, cap) = 0 (a valid id); ids past cap are dropped (*count still tells the total). Clears
 *   every flag it read, so the buffer is zero again afterwards. Three launches; the workspace holds
 *   sagnn_rows_compact_workspace_bytes(n_rows) bytes of tile offsets.
 * sagnn_rows_gather_f32: out[j, s, :] = x[rows[j], s, :] for j < cap, s < t, x at strides ld_n (row) / ld_t
 *   (interval), out dense [cap, t, d]. count non-NULL: slots j >= min(*count, cap) are written as zeros.
 * sagnn_rows_scatter_f32: dst[rows[j], s, :] = src[j, s, :] for j < min(*count, cap), src dense [cap, t, d], dst at
 *   strides ld_n / ld_t; no other element of dst is written. Rows must be distinct (a compaction's are).
 * Row ids read on the device outside [0, n_rows) are skipped (gather writes zeros). Limits: 0 <= n_rows < 2^31;
 *   0 <= cap <= n_rows, cap >= 1 for a compaction over n_rows > 0; d a multiple of 4 in [4, 256]; t >= 1; feature
 *   pointers and the flag buffer 16-byte aligned, strides multiples of 4, ld_n >= d. Every argument is checked before
 *   any device work. No allocation, no synchronisation.
 * -------------------------------------------------------------------------------- */
int sagnn_rows_mark_i32(const int32_t* ids, int64_t n_ids, int64_t n_rows, uint8_t* flags, void* stream);
int sagnn_rows_mark_seg_i32(const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin, const int32_t* seg_len,
                            int64_t n_slots, int max_len, int64_t n_rows, uint8_t* flags, void* stream);
size_t sagnn_rows_compact_workspace_bytes(int64_t n_rows);
int sagnn_rows_compact_i32(uint8_t* flags, int64_t n_rows, int32_t* rows, int64_t cap, int32_t* count, void* workspace,
                           size_t workspace_bytes, void* stream);
int sagnn_rows_gather_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n_rows, int t, int d, const int32_t* rows,
                          int64_t cap, const int32_t* count, float* out, void* stream);
int sagnn_rows_scatter_f32(const float* src, const int32_t* rows, int64_t cap, const int32_t* count, int t, int d,
                           float* dst, int64_t ld_n, int64_t ld_t, int64_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------
 * Self-attention over the user's item sequence (seq_attn.hip; --seqAtt full, not in the reference's graph: the
 * reference multiplies the mask into the tokens before its attention layers, model.py:161-162, so they run on
 * length-1 sequences and the attn_mask of Utils/attention.py:35-45 is never passed).
 * Layout: a padded slab [n_slots * P, d], P = pos_length; token j of slot b is row b * P + j, j < n_b =
 *   clamp(seg_len[b], 0, P) (seg_len int32 [n_slots] on the device). Padding rule: rows j >= n_b hold finite values in
 *   every activation and exact zeros in every gradient these entries write, so the row-wise entries
 *   (sagnn_layernorm_td_f32 with t = 1, sagnn_dense_nn_f32, sagnn_dense_tn_f32, sagnn_leaky_add_f32) run over all
 *   n_slots * P rows and dW = y^T dQKV stays correct. sagnn_attn_bwd_tail_f32 is not among them: a workgroup of it whose
 *   first chunk of 32 gradient rows is all zero, which is what such padding produces, returns NaN bias gradients.
 * Tokens: slot b's token j is item seq_items[seg_begin[b] + j] (seg_begin int64 [n_slots], seq_items int32 [n_flat])
 *   at position seq_pos[seg_begin[b] + j], or, with seq_pos NULL, right-aligned at P - n_b + j. An explicit seq_pos
 *   ascends strictly within a slot (a mask's positions do). Entries outside [0, n_flat), items outside [0, n_items)
 *   and positions outside [0, P) read as zero rows and receive no gradient.
 * sagnn_seq_gather_f32: seq_slab[b * P + j] = fi[item], pos_slab[b * P + j] = pos_embed[position]; zeros in the padding.
 * sagnn_seq_gather_bwd_f32: d_fi[item] += g_seq[b * P + j] (ACCUMULATES; float atomics on whole rows, an item twice
 *   in a sequence counts twice; the last bits may differ from run to run) and d_pos[p] = the sum over slots in
 *   ascending b of the g_pos row of the token at position p (WRITTEN; deterministic).
 * sagnn_seq_attn_f32: qkv [n_slots * P, 3d] dense (q | k | v per row, head h in columns h * d_k .. of each third,
 *   d_k = d / heads) -> ctx [n_slots * P, d] dense: over slot b's n_b tokens only,
 *   e[j, s] = exp(<q_j, k_s> / sqrt(d_k)) with no max subtraction, a = e / (sum_s e + 1e-8), ctx_j = sum_s a[j, s] v_s
 *   (s ascending). Padded rows of ctx are zero. The quotient is evaluated with numerator and denominator scaled by
 *   exp(-max_s score) per row, which leaves it what it is and keeps scores beyond fp32's exp range (88) from
 *   overflowing into inf / inf (forward and backward alike); results are finite for any finite q|k|v.
 * sagnn_seq_attn_bwd_f32: (qkv, g_ctx [n_slots * P, d]) -> dqkv [n_slots * P, 3d], every row WRITTEN, padded rows zero.
 *   e is recomputed from qkv (nothing else is saved by the forward); no atomics, bit-identical between runs. Padded
 *   rows of g_ctx are not read.
 * sagnn_seq_pool_f32: out[b] = sum_{j < n_b} x[b * P + j] (j ascending from 0.0f; an empty slot gives a zero row).
 * sagnn_seq_pool_bwd_f32: dx[b * P + j] = g[b] for j < n_b, zeros in the padding (every row WRITTEN).
 * sagnn_seq_attn_supported(d, heads, pos_length): SAGNN_OK when the two attention entries take the shape,
 *   SAGNN_ERR_DIM otherwise (the reason in sagnn_last_error): d a multiple of 4, d % heads == 0, d / heads in
 *   {2, 4, 8}, 1 <= pos_length <= 256 (one workgroup per (slot, head) with a thread per token; K, V and, backward, q
 *   and g of the head in LDS). Never touches the device.
 * fp32 VALU under every engine (sagnn_set_engine does not change these kernels). Profile kind 5.
 * Limits: gather / pool: d a multiple of 4 in [4, 256], 1 <= pos_length <= 256 (SAGNN_ERR_DIM otherwise); feature
 *   pointers 16-byte aligned, strides multiples of 4 and >= d; n_items > 0; counts >= 0 (n_slots = 0 returns SAGNN_OK
 *   at once, except that sagnn_seq_gather_bwd_f32 still writes its zero d_pos). Every argument is checked before any device work. One launch each (two for sagnn_seq_gather_bwd_f32)
 *   on `stream`, no allocation, no synchronisation (capturable).
 * -------------------------------------------------------------------------------- */
int sagnn_seq_attn_supported(int d, int heads, int pos_length);
int sagnn_seq_gather_f32(const float* fi, int64_t ldf, int64_t n_items, const float* pos_embed, int64_t ldp,
                         int pos_length, const int32_t* seq_items, int64_t n_flat, const int32_t* seq_pos,
                         const int64_t* seg_begin, const int32_t* seg_len, int64_t n_slots, int d, float* seq_slab,
                         float* pos_slab, int64_t ldo, void* stream);
int sagnn_seq_gather_bwd_f32(const float* g_seq, const float* g_pos, int64_t ldg, const int32_t* seq_items,
                             int64_t n_flat, const int32_t* seq_pos, const int64_t* seg_begin, const int32_t* seg_len,
                             int64_t n_slots, int pos_length, int d, float* d_fi, int64_t ld_dfi, int64_t n_items,
                             float* d_pos, int64_t ld_dpos, void* stream);
int sagnn_seq_attn_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d, int heads,
                       float* ctx, void* stream);
int sagnn_seq_attn_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                           int pos_length, int d, int heads, float* dqkv, void* stream);
int sagnn_seq_pool_f32(const float* x, int64_t ldx, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                       float* out, int64_t ldo, void* stream);
int sagnn_seq_pool_bwd_f32(const float* g, int64_t ldg, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                           float* dx, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------
 * Causal sequence attention and a query per prefix (seq_attn.hip; --seqAtt causal, --seqTargets all; neither is in the
 * reference, whose head collapses the sequence into one token trained against one target, model.py:161-168). The slab
 * layout, the padding rule, the token description and the limits are those of the block above.
 * sagnn_seq_attn_masked_f32 / sagnn_seq_attn_masked_bwd_f32: sagnn_seq_attn_f32 / sagnn_seq_attn_bwd_f32 with a mask
 *   choice. causal = 0: those two entries, bit for bit (they forward here). causal = 1: token j attends to tokens
 *   0..j of its slot only: e[j, s] is defined for s <= j, a = e / (sum_{s <= j} e + 1e-8) with the row's largest score
 *   among s <= j as the shift, ctx_j = sum_{s <= j} a[j, s] v_s (s ascending); backward dq_j over s <= j, dk_s and dv_s
 *   over the queries j = s .. n_b - 1 (j ascending). ctx_j does not depend on any token after j, and a gradient that is
 *   non-zero in row j alone gives exact zeros in dk_s, dv_s for s > j. No atomics, bit-identical between runs. On a
 *   slot of one token both choices give the same bits. Any other value of causal: SAGNN_ERR_ARG.
 * sagnn_seq_prefix_query_f32: Q[b * P + j] = max(leaky * pre, pre) + U[b] for j < n_b, pre = sum_{i <= j} x[b * P + i]
 *   (i ascending from 0.0f: the partial sums of sagnn_seq_pool_f32, so that row n_b - 1 has the bits of
 *   sagnn_leaky_add_f32 on that entry's output and U[b]); exact zeros in the padding, every row WRITTEN. U [n_slots, d].
 * sagnn_seq_prefix_query_bwd_f32: dx[b * P + i] = sum_{j >= i} dQ[b * P + j] slope(pre[b, j]) (j descending from
 *   n_b - 1), zeros in the padding, and dU[b] = sum_{j < n_b} dQ[b * P + j] (j ascending; an empty slot: zeros); both
 *   WRITTEN. pre is recomputed by the forward's additions, slope is sagnn_leaky_f32's (leaky on ties). Padded rows of dQ
 *   are not read. No atomics, bit-identical between runs. dx must not alias dQ.
 * sagnn_seq_targets_i32: target[b * P + j] = seq_items[seg_begin[b] + j + 1] for j < n_b - 1, slot_target[b] for
 *   j = n_b - 1, and -1 in the padding, in every row of a slot with slot_target[b] < 0, and for an id outside
 *   [0, n_items) or an entry outside [0, n_flat). excl_row[b * P + j] = slot_user[b] in every row. All int32, on the
 *   device; what sagnn_softmax_loss_f32 takes as target / excl_row for the slab as its query rows.
 * Limits as above (d a multiple of 4 in [4, 256], 1 <= pos_length <= 256, 16-byte aligned rows, strides multiples of 4
 *   and >= d); n_slots = 0 returns SAGNN_OK at once. One launch each on `stream`, no allocation, no synchronisation
 *   (capturable). Profile kind 5.
 * -------------------------------------------------------------------------------- */
int sagnn_seq_attn_masked_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d, int heads,
                              int causal, float* ctx, void* stream);
int sagnn_seq_attn_masked_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                  int pos_length, int d, int heads, int causal, float* dqkv, void* stream);
int sagnn_seq_prefix_query_f32(const float* x, int64_t ldx, const int32_t* seg_len, const float* U, int64_t ldu,
                               int64_t n_slots, int pos_length, int d, float leaky, float* Q, int64_t ldq, void* stream);
int sagnn_seq_prefix_query_bwd_f32(const float* x, int64_t ldx, const int32_t* seg_len, const float* dQ, int64_t lddq,
                                   int64_t n_slots, int pos_length, int d, float leaky, float* dx, int64_t ld_dx, float* dU,
                                   int64_t ld_du, void* stream);
int sagnn_seq_targets_i32(const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin, const int32_t* seg_len,
                          const int32_t* slot_user, const int32_t* slot_target, int64_t n_slots, int pos_length,
                          int64_t n_items, int32_t* target, int32_t* excl_row, void* stream);

/* ------------------------------------------------------------------------------------
 * Sequence attention at head widths 16, 32 and 64 (seq_attn_wide.hip; --seqHeads, not in the reference): the layout and
 * the contract of sagnn_seq_attn_masked_f32 / sagnn_seq_attn_masked_bwd_f32 above for few wide heads, with every
 * product (Q K^T, P V; backward G V^T, dS K, dS^T Q, P^T G) on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).
 * sagnn_seq_attn_wide_f32: qkv [n_slots * P, 3d] dense (q | k | v per row, head h in columns h * d_k .. of each third,
 *   d_k = d / heads) -> ctx [n_slots * P, d] dense. Over slot b's n_b = clamp(seg_len[b], 0, P) tokens only (s <= j under
 *   causal = 1): e[j, s] = exp(<q_j, k_s> / sqrt(d_k)), a = e / (sum_s e + 1e-8), ctx_j = sum_s a[j, s] v_s. The quotient
 *   is evaluated as e' / (sum e' + 1e-8 * 2^-m), shifted by the row's largest score m (a running maximum over tiles of 16
 *   keys in ascending order, the partial sums rescaled when it moves), so results are finite for any finite q|k|v. Padded
 *   rows of ctx are exact zeros; padded rows of qkv are never read, and a tile row at or beyond n_b is loaded as zeros,
 *   so the rows past the end of the buffer that a tile of the last slot covers when P % 16 != 0 are not touched. A masked
 *   score is removed by a select, not by a product with 0. ctx_j does not depend on any token after j under causal = 1.
 * sagnn_seq_attn_wide_bwd_f32: (qkv, g_ctx [n_slots * P, d]) -> dqkv [n_slots * P, 3d], every row WRITTEN, padded rows
 *   exact zeros; e is recomputed from qkv. dk_s and dv_s are summed over the query tiles in ascending order inside the
 *   one workgroup that owns the (slot, head): no atomics, bit-identical between runs, forward and backward. Padded rows
 *   of g_ctx are not read. Under causal = 1 a gradient that is non-zero in rows <= j only gives exact zeros in dk_s, dv_s
 *   for s > j.
 * sagnn_seq_attn_wide_supported(d, heads, pos_length): SAGNN_OK iff d > 0, d % 4 == 0, heads > 0, d % heads == 0,
 *   d / heads in {16, 32, 64} and 1 <= pos_length <= 256; SAGNN_ERR_DIM otherwise (the reason in sagnn_last_error).
 *   Never touches the device. The widths 2, 4 and 8 stay with sagnn_seq_attn_supported's entries; the two sets are disjoint.
 * causal outside {0, 1}: SAGNN_ERR_ARG. qkv, g_ctx, ctx, dqkv 16-byte aligned and dense. n_slots >= 0 (0 returns SAGNN_OK
 *   at once), n_slots < 2^31. Every argument is checked before any device work. One workgroup of 256 threads per (slot,
 *   head); dynamic LDS 2 * ceil16(P) * (d_k + 4) floats (K and V of the head; backward 3 * ceil16(P) floats more and the
 *   same buffer re-used for q and g): 136 KB (139 KB backward) at d_k = 64, P = 256. Exact fp32 under every engine
 *   (sagnn_set_engine does not change these kernels). One launch each on `stream`, no allocation, no synchronisation
 *   (capturable). Profile kind 5.
 * -------------------------------------------------------------------------------- */
int sagnn_seq_attn_wide_supported(int d, int heads, int pos_length);
int sagnn_seq_attn_wide_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d, int heads,
                            int causal, float* ctx, void* stream);
int sagnn_seq_attn_wide_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                int pos_length, int d, int heads, int causal, float* dqkv, void* stream);

/* ------------------------------------------------------------------------------------
 * Position-wise feed-forward block of the sequence head (seq_ffn.hip; --seqFFN, not in the reference): the second half
 * of a self-attentive block, on the slab layout above. For every real token row x_j of every slot
 *   z = LN(x_j; gamma, beta, ln_eps)   (per token over d: z = (x - mean) * rsqrt(var + ln_eps) * gamma + beta, the
 *                                       function sagnn_layernorm_td_f32 evaluates at t = 1)
 *   a = z W1 + b1 [f],  h = act(a) with act(a) = leaky * a where leaky * a >= a, else a (sagnn_leaky_f32's convention),
 *   out = x_j + h W2 + b2.
 * The operands are the fields of sagnn_seq_ffn_args: x [n_slots * P, d] with row stride ldx, seg_len [n_slots] (clamped
 * to [0, P]), W1 [d, f] and W2 [f, d] dense, gamma, beta, b2 [d], b1 [f].
 * sagnn_seq_ffn_f32: every row of out [n_slots * P, d] (row stride ld_out) is WRITTEN, exact zeros in the padding; padded
 *   rows of x are never read. One launch: a persistent grid whose workgroups hold W1 and W2 in LDS; a wave takes tiles
 *   of 16 tokens of one slot and skips (zero-fills) those at or beyond n_b; h stays in registers.
 * sagnn_seq_ffn_bwd_f32: given x and the upstream g [n_slots * P, d] (z, a and h are recomputed; the forward saves
 *   nothing else): dx = g + LN^T((g W2^T . act'(a)) W1^T), every row WRITTEN with exact zeros in the padding, and the six
 *   parameter gradients dgamma, dbeta [d], dW1 [d, f], db1 [f], dW2 [f, d], db2 [d], WRITTEN, not accumulated. Padded rows
 *   of x and g are never read. Three launches: the data path (which stores h | da of the real rows in the workspace,
 *   slab-addressed [n_slots * P, 2f], and per-wave partial sums of dgamma | dbeta), the weight gradients (tokens as the
 *   matrix cores' k index; one partial of dW1 | dW2 | db1 | db2 per workgroup, the grid a function of the shape only) and
 *   the sum of the partials in one fixed order. workspace: sagnn_seq_ffn_bwd_workspace_bytes(n_slots, P, d, f) bytes,
 *   16-byte aligned; SAGNN_ERR_WORKSPACE when missing or smaller (0 from the query: a shape the entries refuse).
 * No atomics: every output, the six parameter gradients included, has the same bits in every run. A row's out and dx do
 *   not depend on its position in a tile or on any other row. Exact fp32 under every engine: all products are chains of
 *   v_mfma_f32_16x16x4_f32, and sagnn_set_engine does not reach them. Every offset is 64-bit.
 * sagnn_seq_ffn_supported(d, f, pos_length): SAGNN_OK iff d in {32, 64, 128}, f % 16 == 0, 16 <= f <= 256,
 *   d * f <= 16384 and 1 <= pos_length <= 256; SAGNN_ERR_DIM otherwise (the reason in sagnn_last_error). d * f bounds the
 *   LDS the two weight matrices take: (d (f + 4) + f (d + 4) + f) floats, 134 KB at (64, 256) of the compute unit's
 *   160 KB; (128, 256) is refused. Never touches the device.
 * Every argument is checked before any device work: NULL (args and every pointer; SAGNN_ERR_NULL), 16-byte alignment of
 *   every float pointer, row strides multiples of 4 and >= d (SAGNN_ERR_ALIGN), leaky in [0, 1), ln_eps in (0, 1],
 *   n_slots >= 0 (SAGNN_ERR_ARG). n_slots = 0 returns SAGNN_OK at once, except that the backward still writes its zero
 *   parameter gradients. No allocation, no synchronisation (capturable). Profile kind 5.
 * -------------------------------------------------------------------------------- */
typedef struct sagnn_seq_ffn_args {
  const float* x;
  int64_t ldx;
  const int32_t* seg_len;
  int64_t n_slots;
  int pos_length, d, f;
  const float *gamma, *beta;
  float ln_eps;
  const float *W1, *b1, *W2, *b2;
  float leaky;
} sagnn_seq_ffn_args;

int sagnn_seq_ffn_supported(int d, int f, int pos_length);
int sagnn_seq_ffn_f32(const sagnn_seq_ffn_args* args, float* out, int64_t ld_out, void* stream);
size_t sagnn_seq_ffn_bwd_workspace_bytes(int64_t n_slots, int pos_length, int d, int f);
int sagnn_seq_ffn_bwd_f32(const sagnn_seq_ffn_args* args, const float* g, int64_t ldg, float* dx, int64_t ld_dx, float* dgamma,
                          float* dbeta, float* dW1, float* db1, float* dW2, float* db2, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Additive-attention pooling of the sequence head (seq_attn.hip; --seqPool additive, not in the reference's graph: it
 * constructs AdditiveAttention(query_vector_dim, latdim), model.py:147, and comments its call out, model.py:168).
 * On the slab layout above, with u = x Wa + ba [n_slots * P, q] computed by the caller (sagnn_dense_nn_f32 over all
 * rows) and v [q] the query vector, for slot b over its n_b real tokens only:
 *   s_j = sum_c tanh(u[b * P + j, c]) v[c],  w = softmax_j(s) (evaluated with the slot's largest s subtracted),
 *   out[b] = sum_j w_j x[b * P + j].
 * sagnn_seq_addpool_f32: out [n_slots, d] is WRITTEN, a zero row for an empty slot. w (nullable, [n_slots * P]) is
 *   WRITTEN for every row, zeros in the padding: the weight the head gives each item. Padded rows of x and u are never
 *   read. Finite for any finite x, u, v: tanh saturates to +-1, and the shift keeps scores beyond fp32's exp range (88)
 *   from overflowing.
 * sagnn_seq_addpool_bwd_f32: given x, u, v and the upstream g [n_slots, d] (t, s and w are recomputed; the forward saves
 *   nothing else), with a_j = <g[b], x_j>, abar = sum_j w_j a_j and ds_j = w_j (a_j - abar):
 *   dx[b * P + j] = w_j g[b] (the direct part only: the caller adds du Wa^T with sagnn_dense_nn_f32, accumulate = 1),
 *   du[b * P + j, c] = ds_j v[c] (1 - t_j[c]^2),  dv_part[b, c] = sum_j ds_j t_j[c],  dv[c] = sum_b dv_part[b, c] (b
 *   ascending; a second launch). Every row of dx, du and dv_part ([n_slots, q] dense workspace) and dv [q] is WRITTEN:
 *   exact zeros in the padding and for an empty slot. dWa = x^T du and dba = colsum(du) are the caller's
 *   sagnn_dense_tn_f32 over the slab. Padded rows of x and u and the rows of g of empty slots are never read.
 * No atomics: every sum across lanes, token groups and slots has one fixed order, so out, w, dx, du and dv are
 *   bit-identical between runs.
 * sagnn_seq_addpool_supported(d, q, pos_length): SAGNN_OK when the two entries take the shape, SAGNN_ERR_DIM otherwise
 *   (the reason in sagnn_last_error). Never touches the device.
 * fp32 VALU under every engine. Profile kind 5.
 * Limits: d and q multiples of 4 in [4, 256], 1 <= pos_length <= 256 (one workgroup per slot); x, u, g, out, dx, du, v and
 *   dv_part 16-byte aligned, strides multiples of 4 and >= the row width; n_slots >= 0 (n_slots = 0 returns SAGNN_OK at
 *   once, except that sagnn_seq_addpool_bwd_f32 still writes its zero dv). Every argument is checked before any device
 *   work. One launch (two for the backward) on `stream`, no allocation, no synchronisation (capturable).
 * -------------------------------------------------------------------------------- */
int sagnn_seq_addpool_supported(int d, int q, int pos_length);
int sagnn_seq_addpool_f32(const float* x, int64_t ldx, const float* u, int64_t ldu, const float* v, const int32_t* seg_len,
                          int64_t n_slots, int pos_length, int d, int q, float* out, int64_t ldo, float* w, void* stream);
int sagnn_seq_addpool_bwd_f32(const float* x, int64_t ldx, const float* u, int64_t ldu, const float* v, const float* g,
                              int64_t ldg, const int32_t* seg_len, int64_t n_slots, int pos_length, int d, int q, float* dx,
                              int64_t ld_dx, float* du, int64_t ld_du, float* dv_part, float* dv, void* stream);

/* ------------------------------------------------------------------------------------
 * Full-catalogue softmax cross-entropy (softmax_loss.hip; --predLoss softmax, not in the reference, which trains the
 * head with a sampled hinge loss only: model.py:241-246): sagnn_softmax_loss_f32 and sagnn_softmax_loss_bwd_f32 with
 * mode = SAGNN_SOFTMAX_FULL. The operands are the fields of sagnn_softmax_args, declared with the two entries below the
 * three blocks that state what each mode computes.
 *   z(b, i) = <Q[b], I[i]> * inv_temp, the product in fp32 on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): a
 *   fixed fmaf chain over k, a function of the query row and the item row alone. sagnn_set_engine does NOT apply.
 *   loss[0] = scale * sum over rows b with a target of ( lse[b] - z(b, target[b]) ),
 *   lse[b]  = ln sum_{i eligible for b} exp(z(b, i)),  tscore[b] = <Q[b], I[target[b]]> (the product, before inv_temp).
 * Eligible items: every item of [0, n_items) except row b's exclusion list; target[b] is always eligible, even when
 *   the list holds it. Row b uses list excl_row[b] (int32 [n_queries]) of the CSR (excl_ptr int64 [n_lists + 1] into
 *   excl_items int32), or list b when excl_row is NULL (then n_lists >= n_queries): a per-user table plus the batch's
 *   user ids serve as they are. Lists are ascending, duplicates allowed; the ids are only compared, never used as
 *   addresses. An excl_row value outside [0, n_lists) means an empty list. All three pointers NULL: no exclusions
 *   (excl_ptr and excl_items go together, excl_row needs them).
 * A target outside [0, n_items) (the model passes -1) skips the row: its loss term, lse[b] and tscore[b] are 0, its dQ
 *   row is 0 and it adds nothing to dI. The row's Q values must still be FINITE (any finite value, +-FLT_MAX included,
 *   gives the bits of a zero row in every output): the backward's dI product takes the row against a zero factor, and
 *   an infinity or a NaN there makes every dI row NaN, in all three modes. The model's slab meets this by construction:
 *   sagnn_seq_prefix_query_f32 writes exact zeros into the padding, and an inactive slot's rows are finite queries.
 * sagnn_softmax_loss_bwd_f32: given lse as the forward wrote it and the upstream scalar g (DEVICE float [1]), with
 *   g(b, i) = g * scale * inv_temp * (p(b, i) - [i == target[b]]), p = exp(z - lse[b]) on eligible items and 0 elsewhere,
 *   dQ[b] = sum_i g(b, i) I[i] and dI[i] = sum_b g(b, i) Q[b]. The logits are recomputed, never stored. Every row of
 *   dQ [n_queries, d] and dI [n_items, d] is WRITTEN (zeros where nothing contributes); nothing is accumulated.
 * lse[b], tscore[b] and dQ[b] depend on row b's inputs only: not on n_queries, the row's position or the strides. All
 *   outputs are bit-identical between runs (no atomics: chunk partials are merged in a fixed order).
 * Logits beyond fp32's exp range are fine (running maximum); a side without eligible items merges as empty.
 * Limits, on the struct's fields: d in {32, 64, 128}; n_queries >= 0; 1 <= n_items < 2^31; ldq, ldi, lddq, lddi multiples
 *   of 4 and >= d; Q, I, dQ, dI and workspace 16-byte aligned; inv_temp > 0 and finite, scale finite; workspace_bytes >=
 *   sagnn_softmax_loss_workspace_bytes(n_queries, n_items, d) (one size serves both entries; it grows with each
 *   argument). Every field is checked before any device work. Three launches each on `stream`, no allocation, no
 *   synchronisation (capturable). Profile kind 6.
 * -------------------------------------------------------------------------------- */
size_t sagnn_softmax_loss_workspace_bytes(int64_t n_queries, int64_t n_items, int d);

/* ------------------------------------------------------------------------------------
 * Sampled-candidate softmax cross-entropy (softmax_loss.hip, sampler.hip; --softmaxNegs, not in the reference): the
 * loss above over a candidate list shared by the batch, so that a step reads n_cand + n_queries item rows only.
 * sagnn_sample_strata_i32: a stratified draw of n_cand ids from [0, n_items). Candidate j is one uniform draw from
 *   the stratum [lo_j, lo_{j+1}), lo_j = floor(j * n_items / n_cand) in 64-bit arithmetic: cand[j] = lo_j + the high half
 *   of ((w0 << 32) | w1) * (lo_{j+1} - lo_j), with (w0, w1, ..) = philox4x32_10(counter = (j, 0, step, 0xFFFFFFFF),
 *   key = seed); the batch samplers use the stream words 0, 1 and 2 + k. The list has exactly n_cand ids, strictly
 *   ascending and distinct, and is a pure function of (seed, step, j); every item is drawn with probability 1 / (its
 *   stratum's size), and the sizes differ by at most one. n_cand == n_items gives 0, 1, .., n_items - 1.
 *   Refused before any launch: n_items < 1 or >= 2^31, n_cand < 0 or > n_items, a NULL cand with n_cand > 0. One launch
 *   on `stream` (none when n_cand == 0).
 * sagnn_softmax_loss_f32 with mode = SAGNN_SOFTMAX_CAND: I is the full [n_items, d] table, cand int32 [n_cand] (DEVICE)
 *   strictly ascending ids in [0, n_items); its contents are the caller's responsibility, they are used as row
 *   addresses. z, lse, tscore, loss, the exclusion lists and the skipped rows are those of SAGNN_SOFTMAX_FULL, with the
 *   eligible set
 *     E_b = { c in cand : c not on row b's list, c != target[b] } + { target[b] }:
 *   the target enters exactly once, through its own term, whether or not it is a candidate or on the list.
 *   n_cand == 0 is legal: lse[b] = z(b, target[b]), no loss, no gradient.
 * sagnn_softmax_loss_bwd_f32 with mode = SAGNN_SOFTMAX_CAND: with g(b, i) as above over E_b,
 *   dQ[b]  = sum_{i in E_b} g(b, i) I[i], the target's term included;
 *   dIc[j] = sum over rows b with cand[j] in E_b and cand[j] != target[b] of g(b, cand[j]) Q[b]: row j of
 *            dIc [n_cand, d] belongs to item cand[j]. dIc and its stride lddic are the struct's dI and lddi;
 *   dT[b]  = g(b, target[b]) Q[b], [n_queries, d]: the target's share of dI, one row per query (several rows may share
 *            a target; adding them into dI is the caller's).
 *   Every row of dQ, dIc and dT is WRITTEN (zeros where nothing contributes, skipped rows included).
 * lse[b], tscore[b], dQ[b] and dT[b] depend on row b's inputs only; chunks depend on n_cand only; no atomics, all
 *   outputs are bit-identical between runs.
 * Limits, on the struct's fields: those of SAGNN_SOFTMAX_FULL, and 0 <= n_cand <= n_items, cand non-NULL when n_cand > 0,
 *   lddi (lddic) and lddt multiples of 4 and >= d, dI (dIc) and dT 16-byte aligned, workspace_bytes >=
 *   sagnn_softmax_loss_cand_workspace_bytes(n_queries, n_cand, d) (grows with each argument). Every field is checked
 *   before any device work. At most three launches each on `stream`, no allocation, no synchronisation (capturable).
 *   Profile kind 7 (units_a = n_queries, units_b = n_cand).
 * sagnn_softmax_target_add_f32: dI[target[b]] += dT[b] for every row b with a target in [0, n_items), the rows that
 *   share a target added in ascending b by one thread per element (no atomics: bit-identical between runs). Meant
 *   for a batch: a thread compares its target with all n_queries. Same limits on d, n_queries, n_items, strides and
 *   alignment; one launch on `stream`, not recorded by the profile.
 * sagnn_softmax_target_scatter_f32: the same sum, dI[target[r]] += dT[r] for every row r with a target in [0, n_items),
 *   for row counts far beyond a batch (--seqTargets all: a row per sequence token): one thread per (row, float4 column)
 *   and float atomics, so rows that share a target are added in no fixed order and dI is equal between runs up to the
 *   order of summation, as sagnn_seq_gather_bwd_f32's d_fi is. Same limits (n_rows <= INT32_MAX); one launch on
 *   `stream`, not recorded by the profile. The full-catalogue mode needs neither entry: it writes dI itself.
 * -------------------------------------------------------------------------------- */
int sagnn_softmax_target_add_f32(const float* dT, int64_t lddt, const int32_t* target, int64_t n_queries, int64_t n_items,
                                 int d, float* dI, int64_t lddi, void* stream);
int sagnn_softmax_target_scatter_f32(const float* dT, int64_t lddt, const int32_t* target, int64_t n_rows, int64_t n_items,
                                     int d, float* dI, int64_t lddi, void* stream);
int sagnn_sample_strata_i32(int64_t n_items, int64_t n_cand, uint64_t seed, uint32_t step, int32_t* cand, void* stream);
size_t sagnn_softmax_loss_cand_workspace_bytes(int64_t n_queries, int64_t n_cand, int d);

/* ------------------------------------------------------------------------------------
 * Popularity-weighted candidates with the logQ correction (sampler.hip, softmax_loss.hip; --softmaxNegDist pop, not in
 * the reference): the sampled softmax of word2vec and two-tower retrieval over the candidate mode above.
 * sagnn_sample_strata_w_i32: a stratified draw of n_cand ids with replacement, item i drawn in proportion to its
 *   integer weight w_i. cum int64 [n_items] (DEVICE) is the inclusive prefix sum of the weights, non-decreasing with
 *   cum[0] >= 1; total = cum[n_items - 1] = W is the caller's HOST copy of its last entry (the entry reads nothing
 *   back). The mass [0, W) is cut into n_cand strata [lo_j, lo_{j+1}), lo_j = j * (W / n_cand) + (j * (W % n_cand)) /
 *   n_cand in 64-bit arithmetic (no 128-bit division; every product is below 2^62), and
 *     r_j = lo_j + the high half of ((w0 << 32) | w1) * (lo_{j+1} - lo_j),
 *     (w0, w1, ..) = philox4x32_10(counter = (j, 1, step, 0xFFFFFFFF), key = seed):
 *   the strata stream of sagnn_sample_strata_i32 with counter word 1 set, so none of its blocks is reused.
 *   cand[j] = #{ i : cum[i] <= r_j }, the item whose mass holds r_j. The list is non-decreasing, repeats are adjacent,
 *   and it is a pure function of (cum, n_cand, seed, step, j). The run of id c is the positions [lb, ub) that hold it:
 *   position lb is LIVE with bias[lb] = ln(m) - ln(e), m = ub - lb, e = n_cand * w_c / W the expected number of draws
 *   of c (w_c = cum[c] - cum[c - 1]), the logs in double, rounded once to float, and exactly 0.0f when
 *   m * W == n_cand * w_c as integers; the other positions of the run are DEAD, bias = -inf. Then
 *     sum_{live j} exp(z(cand[j]) + bias[j]) = sum_{draws} exp(z(c)) / e_c,
 *   whose expectation is the sum of exp(z(i)) over the whole catalogue, e_c within a relative n_cand / W of the exact
 *   expected count. Equal weights and n_cand == n_items give 0, 1, .., n_items - 1 with every bias exactly 0.
 *   Refused before any launch: n_items < 1 or >= 2^31, total < 1 or >= 2^62, n_cand < 0, >= 2^31 or > total, a NULL cum,
 *   a NULL cand or bias with n_cand > 0. Two launches on `stream` (none when n_cand == 0), no allocation, no
 *   synchronisation (capturable). A cum that breaks the contract still yields ids inside [0, n_items).
 * sagnn_softmax_loss_f32 / sagnn_softmax_loss_bwd_f32 with mode = SAGNN_SOFTMAX_CAND_BIAS: SAGNN_SOFTMAX_CAND with a
 *   per-position offset bias float [n_cand] (DEVICE) and a NON-DECREASING cand whose repeats are adjacent. Position j
 *   is eligible for row b when cand[j] is (above) AND bias[j] > -inf, and its logit is z(b, cand[j]) + bias[j], one
 *   fp32 add; the target's own term takes no offset and tscore is unchanged. With the first position of each run the
 *   only one above -inf (what the draw writes) an id enters a row's sum once. The dIc rows of dead positions are exact
 *   zeros. A zero bias on a strictly ascending list gives the bits of SAGNN_SOFTMAX_CAND. The same limits,
 *   workspace (sagnn_softmax_loss_cand_workspace_bytes), launches and profile kind; a NULL bias with n_cand > 0 is
 *   refused.
 * sagnn_softmax_cand_scatter_f32: dI[cand[j]] = dIc[j] for every position j with bias[j] > -inf and cand[j] inside
 *   [0, n_items): the live rows into a full-size dI. The live ids are distinct, so every row has one writer and the
 *   result does not depend on the order of execution. Limits on d, n_items, n_cand, strides and alignment as above;
 *   one launch on `stream` (none when n_cand == 0), not recorded by the profile.
 * -------------------------------------------------------------------------------- */
int sagnn_sample_strata_w_i32(const int64_t* cum, int64_t n_items, int64_t total, int64_t n_cand, uint64_t seed,
                              uint32_t step, int32_t* cand, float* bias, void* stream);
int sagnn_softmax_cand_scatter_f32(const float* dIc, int64_t lddic, const int32_t* cand, const float* bias, int64_t n_cand,
                                   int64_t n_items, int d, float* dI, int64_t lddi, void* stream);

/* ------------------------------------------------------------------------------------
 * The two softmax-loss entries and their operands. `mode` names the form; it is not inferred from which pointer is set:
 *   SAGNN_SOFTMAX_FULL       the whole catalogue; cand and bias must be NULL and n_cand 0.
 *   SAGNN_SOFTMAX_CAND       the candidate list cand [n_cand]; bias must be NULL.
 *   SAGNN_SOFTMAX_CAND_BIAS  the list with the offsets bias [n_cand]; a NULL bias with n_cand > 0 is refused.
 * A NULL args (SAGNN_ERR_NULL), a `mode` outside these three and a field that contradicts the mode (SAGNN_ERR_ARG) are
 * refused before anything else is looked at; then the shared fields, the candidate fields, the entry's own pointers and
 * the workspace are checked in that order, all of it before any launch. A field that an entry or a mode does not read
 * may hold anything, the ones the mode rules name excepted. The messages in sagnn_last_error start with softmax_loss,
 * softmax_loss_cand or softmax_loss_candb by the mode, with _bwd appended by the backward.
 * -------------------------------------------------------------------------------- */
enum { SAGNN_SOFTMAX_FULL = 0, SAGNN_SOFTMAX_CAND = 1, SAGNN_SOFTMAX_CAND_BIAS = 2 };

typedef struct sagnn_softmax_args {
  /* both entries, every mode */
  const float* Q;  int64_t ldq;               /* [n_queries, d] */
  const float* I;  int64_t ldi;               /* [n_items, d], the full table in every mode */
  int64_t n_queries, n_items;
  int d;
  const int32_t* target;                      /* [n_queries] */
  float inv_temp, scale;
  const int64_t* excl_ptr;                    /* [n_lists + 1], or the three NULL */
  const int32_t* excl_items;
  const int32_t* excl_row;                    /* [n_queries], or NULL: row b uses list b */
  int64_t n_lists;
  int mode;                                   /* SAGNN_SOFTMAX_* */
  /* both entries, the candidate modes */
  const int32_t* cand;  int64_t n_cand;       /* SAGNN_SOFTMAX_CAND and _CAND_BIAS */
  const float* bias;                          /* SAGNN_SOFTMAX_CAND_BIAS: [n_cand] */
  /* the forward writes these; the backward reads lse alone */
  float* loss;                                /* [1] */
  float* lse;                                 /* [n_queries] */
  float* tscore;                              /* [n_queries] */
  /* the backward alone */
  const float* g;                             /* the upstream scalar, DEVICE [1] */
  float* dQ;  int64_t lddq;                   /* [n_queries, d] */
  float* dI;  int64_t lddi;                   /* SAGNN_SOFTMAX_FULL: dI [n_items, d]; candidate modes: dIc [n_cand, d] */
  float* dT;  int64_t lddt;                   /* candidate modes: [n_queries, d]; SAGNN_SOFTMAX_FULL does not read them */
  /* both entries: sagnn_softmax_loss_workspace_bytes in SAGNN_SOFTMAX_FULL, _cand_workspace_bytes in the candidate modes */
  void* workspace;  size_t workspace_bytes;
} sagnn_softmax_args;

int sagnn_softmax_loss_f32(const sagnn_softmax_args* args, void* stream);
int sagnn_softmax_loss_bwd_f32(const sagnn_softmax_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAGNN_H */
