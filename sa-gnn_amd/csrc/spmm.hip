// Interval SpMM for gfx950: out = leaky(A·X) + residual, with the running add_n fused.
//
// Replaces the GatherV2 -> SegmentSum -> Pad -> GatherV2 -> Maximum chain of
// Recommender.messagePropagate (reference model.py:80-92) plus the residual add and add_n of
// model.py:124-127. The adjacency is a binary pattern (edge values are dropped by the
// reference, model.py:84-86), so the kernel reads rowptr + colidx only.
//
// Mapping (wave64): a feature row of d floats is covered by LPR = d/4 lanes holding one float4
// each, so one `global_load_dwordx4` wave-instruction gathers G = 64/LPR neighbour rows
// (1 KiB at d = 64). Rows are processed in three degree classes:
//   short  (deg <= short_thresh) one lane-group per row, G rows of the wave's row block at once,
//          a single accumulator added in edge order;
//   medium (<= long_thresh)      the whole wave on one row, G neighbours per instruction, UN
//          instructions in flight, then a cross-group shuffle reduction;
//   long   (> long_thresh)       pre-cut into chunks (plan), one wave per chunk writing a raw
//          partial sum, then a fix-up wave per row adds the partials in chunk order.
// Column indices are fetched coalesced (one per lane) and broadcast with ds_bpermute.
//
// Edge dropout (the *_drop_* entries): the lane that loaded an edge's column index decides whether the
// edge is kept — one Philox block per edge, a pure function of (seed, step, tag, user id, item id) — and replaces a
// dropped index by -1 before the broadcast, so a dropped edge is a gather that is never issued. Every kernel is one
// template whose drop-only arguments are a pack: with the pack empty it compiles to what it was without dropout.
//
// Edge weights (sagnn_spmm_plan_set_weights): s[r] = sum_e w[e] * X[col[e], :]. The lane that loads
// colidx[e] loads w[e] from the same coalesced non-temporal stream and both are broadcast together; the gather
// accumulates acc = fmaf(w, x, acc), one rounding per edge and element, in edge order. A dropped or absent edge has
// index -1, gathers nothing and adds fmaf(w, 0, acc) = acc. The weights travel in the same trailing pack (none; drop;
// weights; drop + weights): WEIGHTED is a compile-time property of an instantiation. The fix-ups add raw partial sums,
// which the chunk waves have weighted already, so a weighted launch runs the fix-up kernels it would run unweighted.
#include <float.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "common.h"
#include "philox.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;              // 4 waves
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kRowsPerWave = 16;         // row block per wavefront (rowptr slice fits one lane each)
// Dataset-sized graphs (tens of thousands of rows: Gowalla, Amazon, MovieLens) give 16-row blocks only a dozen
// waves per CU and every launch is a chain of three dependent L2 round trips: below kSmallRows rows a wave takes
// ONE row per lane group (4 rows at d = 64), four times the waves in flight.
constexpr int64_t kSmallRows = 262144;
constexpr int kUnroll = 8;               // gather instructions in flight per wave

struct Epilogue {
  const float* residual;
  int64_t ldr;
  const float* acc_in;
  int64_t ld_acc_in;
  float* out;
  int64_t ldo;
  float* acc_out;
  int64_t ld_acc_out;
  float leaky;
  // training extras (sagnn_spmm_ex_f32)
  uint8_t* mask_out;       // [n_rows, d/4]: bit j of byte l = 1 iff the activation passed s[4l+j] through
  const uint8_t* mask_in;  // same layout, for out2
  float* out2;             // out2 = v * (mask_in bit ? 1 : slope2), v = acc value if acc_out else y
  int64_t ldo2;
  float slope2;
  int mask_stride;         // bytes per mask row (= lanes per row)
  const float* acc_in2;    // second addend of the running sum (acc_out = acc_in + acc_in2 + y)
  int64_t ld_acc_in2;
};

__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// Streaming accesses (each byte touched once per launch: row outputs, residual / running-sum
// reads, column indices) are marked non-temporal so they do not push gathered rows out of the
// caches: -3 % per launch (4.25 -> 4.10 ms at the roofline config). The gathers themselves stay
// plain loads: making the cold ones non-temporal (hot/cold split by column degree) was 17 %
// SLOWER. -DSAGNN_PLAIN_STREAMS restores plain accesses for A/B runs.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4s(const float* p) {
#ifndef SAGNN_PLAIN_STREAMS
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return ld4(p);
#endif
}
__device__ __forceinline__ void st4s(float* p, float4 v) {
#ifndef SAGNN_PLAIN_STREAMS
  const f32x4_t w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<f32x4_t*>(p));
#else
  st4(p, v);
#endif
}
__device__ __forceinline__ int ldi_s(const int32_t* p) {
#ifndef SAGNN_PLAIN_STREAMS
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
__device__ __forceinline__ float ldf_s(const float* p) {
#ifndef SAGNN_PLAIN_STREAMS
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
__device__ __forceinline__ int ldb_s(const uint16_t* p) {
#ifndef SAGNN_PLAIN_STREAMS
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
__device__ __forceinline__ void add4(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// Edge dropout of one product: the decision of edge (user, item) is word 0 of Philox4x32-10(key = seed, counter =
// (user, item, tag, step)) < thresh. rows_users says which of (row, column index) is the user.
struct RowDrop {
  uint32_t k0, k1, step, thresh, tag;
  int rows_users;
  float scale;             // 1 / keep: multiplies the finished row sum
};
// Both directions of a batched launch: r.tag is the tag of the segments whose rows are users, tag_i that of the
// item-row segments, both without the interval (seg_drop adds k << 8).
struct BatchDrop {
  RowDrop r;
  uint32_t tag_i;
};

__device__ __forceinline__ RowDrop seg_drop(const BatchDrop& b, int dir, int k) {
  RowDrop r = b.r;
  r.tag = (dir ? b.tag_i : r.tag) | ((uint32_t)k << 8);
  r.rows_users = !dir;
  return r;
}

// acc += w * v (WEIGHTED: one fused multiply-add per element) or acc += v
template <bool WEIGHTED>
__device__ __forceinline__ void acc4(float4& a, float w, const float4& v) {
  if constexpr (WEIGHTED) {
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
  } else {
    add4(a, v);
  }
}

// The loading lane's filter: idx if edge (row, idx) is kept, else -1 (an index of -1 stays -1).
template <bool DROP>
__device__ __forceinline__ int keep_edge(const RowDrop& dr, int row, int idx) {
  if constexpr (DROP) {
    const uint32_t u = dr.rows_users ? (uint32_t)row : (uint32_t)idx;
    const uint32_t i = dr.rows_users ? (uint32_t)idx : (uint32_t)row;
    const sagnn::Word4 w = sagnn::philox4x32_10(sagnn::Word4{u, i, dr.tag, dr.step}, dr.k0, dr.k1);
    return w.x < dr.thresh ? idx : -1;
  } else {
    return idx;
  }
}

template <bool DROP>
__device__ __forceinline__ float4 drop_scale(const RowDrop& dr, float4 s) {
  if constexpr (DROP) return make_float4(dr.scale * s.x, dr.scale * s.y, dr.scale * s.z, dr.scale * s.w);
  else return s;
}

// Time-aware messages (sagnn_spmm_plan_set_buckets): edge e adds TE[bucket[e], :] to the row it gathers,
// v = X[col[e]] + TE[bucket[e]], before the accumulation. RowTime is one product's bucket stream and table (rows d
// apart); BatchTime the 2T segments' bucket pointers, parallel to SegMeta, and the layer's TE base with the element
// strides of interval and direction.
struct RowTime {
  const uint16_t* bucket;
  const float* te;
};
struct BatchTime {
  const uint16_t* const* buckets;
  const float* te;
  int64_t s_k, s_dir;
};
__device__ __forceinline__ RowTime seg_time(const BatchTime& t, int seg, int dir, int k) {
  return RowTime{t.buckets[seg], t.te + (int64_t)k * t.s_k + (int64_t)dir * t.s_dir};
}
__device__ __forceinline__ RowTime seg_time(const RowTime& t, int, int, int) { return t; }

// What only some kernels are passed comes after the arguments every kernel has, as a pack that is empty for the default
// kernels (their argument list stays what it was). The forms are told apart by the TYPES in the pack:
//   const int32_t*, RowDrop / BatchDrop   the row of each long-row chunk and the launch's drop (the fix-ups take the
//                                         scale alone: their partial sums arrive unscaled);
//   const float* / const float* const*    the edge weights of the plan, or for the batched kernels a device table of the
//                                         2T segments' weight pointers, parallel to SegMeta;
//   RowTime / BatchTime                   the time term, above.
// Instantiated: none; (chunk_row, drop); (weights); (chunk_row, drop, weights); (time); (time, weights). A pointer among
// them is __restrict__ like the pointers ahead of it (KernelArg).
template <class T>
struct KernelArg { using type = T; };
template <class T>
struct KernelArg<T*> { using type = T* __restrict__; };
template <class Want, class... A>
constexpr bool kHas = (std::is_same_v<Want, A> || ...);
template <class... A>
struct Pack {
  static constexpr bool DROP = kHas<RowDrop, A...> || kHas<BatchDrop, A...>;
  static constexpr bool WEIGHTED = kHas<const float*, A...> || kHas<const float* const*, A...>;
  static constexpr bool TIME = kHas<RowTime, A...> || kHas<BatchTime, A...>;
  static_assert(DROP == kHas<const int32_t*, A...>, "a drop comes with the rows of the chunks");
  static_assert(!(DROP && TIME), "there are no drop + time kernels");
  static_assert(sizeof...(A) == 2 * DROP + WEIGHTED + TIME, "trailing arguments: a drop, weights, a time term");
};
// the pack's argument of type Want, or Want{} when the pack has none
template <class Want>
__device__ __forceinline__ Want arg_of() { return Want{}; }
template <class Want, class A0, class... A>
__device__ __forceinline__ Want arg_of(A0 a0, A... rest) {
  if constexpr (std::is_same_v<Want, A0>) return a0;
  else return arg_of<Want, A...>(rest...);
}
template <class... A>
__device__ __forceinline__ int chunk_row_of(int64_t ci, A... da) {
  if constexpr (Pack<A...>::DROP) return arg_of<const int32_t*, A...>(da...)[ci];
  else return 0;
}
// the weights of the launch's plan, or of segment `seg` of a batch
template <class... A>
__device__ __forceinline__ const float* weights_of(int seg, A... da) {
  if constexpr (kHas<const float* const*, A...>) return arg_of<const float* const*, A...>(da...)[seg];
  else return arg_of<const float*, A...>(da...);
}
__device__ __forceinline__ float4 scaled(float4 s) { return s; }
__device__ __forceinline__ float4 scaled(float4 s, float scale) {
  return make_float4(scale * s.x, scale * s.y, scale * s.z, scale * s.w);
}

// y = max(leaky*s, s) + residual ; out = y ; acc_out = acc_in + y (+ acc_in2) ; training extras as above.
__device__ __forceinline__ void finish_row(const Epilogue& ep, int64_t row, int col, float4 s) {
  float4 y;
  y.x = fmaxf(ep.leaky * s.x, s.x);
  y.y = fmaxf(ep.leaky * s.y, s.y);
  y.z = fmaxf(ep.leaky * s.z, s.z);
  y.w = fmaxf(ep.leaky * s.w, s.w);
  if (ep.mask_out) {
    // tf.maximum(leaky*x, x) routes the gradient to its FIRST argument on ties (x = 0), so the
    // slope is 1 only where x is strictly the larger one
    const unsigned bits = (s.x > ep.leaky * s.x ? 1u : 0u) | (s.y > ep.leaky * s.y ? 2u : 0u) |
                          (s.z > ep.leaky * s.z ? 4u : 0u) | (s.w > ep.leaky * s.w ? 8u : 0u);
    ep.mask_out[row * ep.mask_stride + (col >> 2)] = (uint8_t)bits;
  }
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ep.residual) {
    r = ld4s(ep.residual + row * ep.ldr + col);
    add4(y, r);
  }
  if (ep.out) st4s(ep.out + row * ep.ldo + col, y);
  if (ep.acc_out) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ep.acc_in) {
      a = (ep.acc_in == ep.residual && ep.ld_acc_in == ep.ldr)
              ? r
              : ld4s(ep.acc_in + row * ep.ld_acc_in + col);
    }
    add4(a, y);
    if (ep.acc_in2) add4(a, ld4s(ep.acc_in2 + row * ep.ld_acc_in2 + col));
    st4s(ep.acc_out + row * ep.ld_acc_out + col, a);
    y = a;
  }
  if (ep.out2) {
    const unsigned bits = ep.mask_in ? ep.mask_in[row * ep.mask_stride + (col >> 2)] : 15u;
    float4 z;
    z.x = (bits & 1u) ? y.x : ep.slope2 * y.x;
    z.y = (bits & 2u) ? y.y : ep.slope2 * y.y;
    z.z = (bits & 4u) ? y.z : ep.slope2 * y.z;
    z.w = (bits & 8u) ? y.w : ep.slope2 * y.w;
    st4s(ep.out2 + row * ep.ldo2 + col, z);
  }
}

// gm[r, :] = g[r, :] * (mask bit ? 1 : slope) for interval blockIdx.y of a slab (one matrix: grid.y = 1, the slab
// strides unused): seeds the backward chain of the GNN stack.
__global__ void mask_scale_kernel(const float* __restrict__ g, int64_t ldg, int64_t s_g, const uint8_t* __restrict__ mask,
                                  int64_t s_mask, int mask_stride, float slope, float* __restrict__ gm, int64_t ldgm,
                                  int64_t s_gm, int64_t n_rows, int d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lpr = d >> 2;
  if (i >= n_rows * lpr) return;
  const int64_t k = blockIdx.y;
  const int64_t row = i / lpr;
  const int l = (int)(i - row * lpr);
  const float4 v = ld4(g + k * s_g + row * ldg + 4 * l);
  const unsigned bits = mask[k * s_mask + row * mask_stride + l];
  float4 z;
  z.x = (bits & 1u) ? v.x : slope * v.x;
  z.y = (bits & 2u) ? v.y : slope * v.y;
  z.z = (bits & 4u) ? v.z : slope * v.z;
  z.w = (bits & 8u) ? v.w : slope * v.w;
  st4(gm + k * s_gm + row * ldgm + 4 * l, z);
}

// Whole wave sums X[idx[e], :] for e in [e0, e1): G neighbour rows per load instruction.
// IDENT: the "index" of edge e is e itself (fix-up pass over the partial-sum workspace).
// Returns the total in every lane-group (cross-group xor reduction).
// DROP: the edges belong to row `row`; each lane filters the 64-edge slice it loaded when the slice is taken up, so
// the load of the next slice still overlaps this slice's gathers.
// WEIGHTED: edge e counts w[e] times; a slice's weights are requested with its indices and broadcast with them.
// TIME: edge e gathers TE[bucket[e], :] (rows ldte apart) next to X[idx[e], :]; a slice's buckets travel like its weights, the
// table row is a plain cached load by the lanes that gather X, and it is added into its X row before the accumulation.
template <int LPR, bool IDENT, bool DROP = false, bool WEIGHTED = false, bool TIME = false>
__device__ __forceinline__ float4 wave_row_sum(const int32_t* __restrict__ colidx, int e0, int e1,
                                               const float* __restrict__ X, int64_t ldx,
                                               int lane, int grp, int col, bool lane_on, const RowDrop& dr = RowDrop{},
                                               int row = 0, const float* __restrict__ w = nullptr,
                                               const RowTime& tm = RowTime{}, int ldte = 0) {
  static_assert(!(IDENT && (WEIGHTED || TIME)), "the fix-up pass adds partial sums that carry the weights and the time term already");
  constexpr int G = kWave / LPR;
  constexpr int STEP = G * kUnroll;  // divides 64 for every LPR in {8,16,32,64}
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int idx_next = -1;
  float w_next = 0.f;
  int b_next = 0;
  if (e0 + lane < e1) {
    idx_next = IDENT ? (e0 + lane) : ldi_s(colidx + e0 + lane);
    if constexpr (WEIGHTED) w_next = ldf_s(w + e0 + lane);
    if constexpr (TIME) b_next = ldb_s(tm.bucket + e0 + lane);
  }
  for (int e = e0; e < e1; e += kWave) {
    const int idx = keep_edge<DROP>(dr, row, idx_next);
    const float wt = w_next;
    const int bk = b_next;
    const int en = e + kWave;
    idx_next = -1;
    if constexpr (WEIGHTED) w_next = 0.f;
    if constexpr (TIME) b_next = 0;
    if (en + lane < e1) {
      idx_next = IDENT ? (en + lane) : ldi_s(colidx + en + lane);
      if constexpr (WEIGHTED) w_next = ldf_s(w + en + lane);
      if constexpr (TIME) b_next = ldb_s(tm.bucket + en + lane);
    }
    const int cnt = min(kWave, e1 - e);
    for (int j = 0; j < cnt; j += STEP) {
      float4 v[kUnroll];
      int c[kUnroll];
      float cw[kUnroll];
      int cb[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        c[u] = __shfl(idx, j + u * G + grp);
        if constexpr (WEIGHTED) cw[u] = __shfl(wt, j + u * G + grp);
        else cw[u] = 1.f;
        if constexpr (TIME) cb[u] = __shfl(bk, j + u * G + grp);
        else cb[u] = 0;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c[u] >= 0 && lane_on) v[u] = ld4(X + (int64_t)c[u] * ldx + col);
      }
      if constexpr (TIME) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
          if (c[u] >= 0 && lane_on) add4(v[u], ld4(tm.te + cb[u] * ldte + col));
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) acc4<WEIGHTED>(acc, cw[u], v[u]);
    }
  }
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off);
    acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off);
    acc.w += __shfl_xor(acc.w, off);
  }
  return acc;
}

// A wave's share of the row blocks: RPW consecutive rows starting at row0 (short rows by lane groups, medium rows by
// the whole wave; long rows belong to the chunk waves + fix-up).
template <int LPR, int RPW, bool DROP, bool WEIGHTED, bool TIME = false>
__device__ __forceinline__ void rows_wave(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                          const float* __restrict__ X, int64_t ldx, int d, int64_t n_rows, int64_t row0,
                                          int short_t, int long_t, const Epilogue& ep, int lane,
                                          const RowDrop& dr, const float* __restrict__ w,
                                          const RowTime& tm = RowTime{}) {
  constexpr int G = kWave / LPR;
  const int grp = lane / LPR;
  const int sub = lane % LPR;
  const int col = 4 * sub;
  const bool lane_on = col < d;
  const int nr = (int)min((int64_t)RPW, n_rows - row0);
  // lane l (l <= nr) holds rowptr[row0 + l]; lanes beyond replicate the last entry (degree 0).
  const int rp = rowptr[row0 + min(lane, nr)];
  // the shuffle must run with every lane active: a lane masked off by the select below would
  // read 0 from ds_bpermute instead of its neighbour's rowptr entry
  const int rp_up = __shfl_down(rp, 1);
  const int deg_l = (lane < nr) ? (rp_up - rp) : 0;
  unsigned long long medium = __ballot(deg_l > short_t && deg_l <= long_t);

  // ---- short rows: one lane-group per row, G rows per iteration -------------------------
  // The column-index slice of the next iteration is requested before this iteration's
  // gathers so the two dependent HBM round trips overlap.
  int e0_n = __shfl(rp, grp);
  int dg_n = __shfl(deg_l, grp);
  int idx_n = -1;
  float w_n = 0.f;           // WEIGHTED: the weight travels with its index, from the same lane
  int b_n = 0;               // TIME: so does the bucket
  if (dg_n <= short_t && sub < dg_n) {
    idx_n = ldi_s(colidx + e0_n + sub);
    if constexpr (WEIGHTED) w_n = ldf_s(w + e0_n + sub);
    if constexpr (TIME) b_n = ldb_s(tm.bucket + e0_n + sub);
  }
#pragma unroll 1
  for (int it = 0; it < RPW / G; ++it) {
    const int lr = it * G + grp;
    const int e0 = e0_n;
    const int dg = dg_n;
    // DROP: the prefetched slice is filtered here, not where it was requested, so its load stays in flight
    int idx = keep_edge<DROP>(dr, (int)row0 + lr, idx_n);
    float wt = w_n;
    int bk = b_n;
    const bool mine = (lr < nr) && (dg <= short_t);
    const int my_deg = mine ? dg : 0;
    if (it + 1 < RPW / G) {
      e0_n = __shfl(rp, lr + G);
      dg_n = __shfl(deg_l, lr + G);
      idx_n = -1;
      if constexpr (WEIGHTED) w_n = 0.f;
      if constexpr (TIME) b_n = 0;
      if (dg_n <= short_t && sub < dg_n) {
        idx_n = ldi_s(colidx + e0_n + sub);
        if constexpr (WEIGHTED) w_n = ldf_s(w + e0_n + sub);
        if constexpr (TIME) b_n = ldb_s(tm.bucket + e0_n + sub);
      }
    }
    int maxdeg = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int x = __builtin_amdgcn_readlane(deg_l, it * G + g);
      maxdeg = max(maxdeg, x <= short_t ? x : 0);
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int eo = 0; eo < maxdeg; eo += LPR) {
      if (eo > 0) {
        const int k = eo + sub;
        idx = (k < my_deg) ? keep_edge<DROP>(dr, (int)row0 + lr, ldi_s(colidx + e0 + k)) : -1;
        if constexpr (WEIGHTED) wt = (k < my_deg) ? ldf_s(w + e0 + k) : 0.f;
        if constexpr (TIME) bk = (k < my_deg) ? ldb_s(tm.bucket + e0 + k) : 0;
      }
      const int lim = min(LPR, maxdeg - eo);
      for (int j = 0; j < lim; j += kUnroll) {
        float4 v[kUnroll];
        int c[kUnroll];
        float cw[kUnroll];
        int cb[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          c[u] = __shfl(idx, grp * LPR + j + u);
          if constexpr (WEIGHTED) cw[u] = __shfl(wt, grp * LPR + j + u);
          else cw[u] = 1.f;
          if constexpr (TIME) cb[u] = __shfl(bk, grp * LPR + j + u);
          else cb[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c[u] >= 0 && lane_on) v[u] = ld4(X + (int64_t)c[u] * ldx + col);
        }
        if constexpr (TIME) {
#pragma unroll
          for (int u = 0; u < kUnroll; ++u)
            if (c[u] >= 0 && lane_on) add4(v[u], ld4(tm.te + cb[u] * d + col));
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) acc4<WEIGHTED>(acc, cw[u], v[u]);
      }
    }
    if (mine && lane_on) finish_row(ep, row0 + lr, col, drop_scale<DROP>(dr, acc));
  }

  // ---- medium rows: the whole wave per row ----------------------------------------------
  while (medium) {
    const int lr = __builtin_ctzll(medium);
    medium &= medium - 1;
    const int e0 = __builtin_amdgcn_readlane(rp, lr);
    const int dg = __builtin_amdgcn_readlane(deg_l, lr);
    const float4 s =
        wave_row_sum<LPR, false, DROP, WEIGHTED, TIME>(colidx, e0, e0 + dg, X, ldx, lane, grp, col, lane_on, dr, (int)row0 + lr, w,
                                                       tm, d);
    if (grp == 0 && lane_on) finish_row(ep, row0 + lr, col, drop_scale<DROP>(dr, s));
  }
}

// One launch covers the long-row chunks (first `chunk_blocks` blocks, heaviest work first)
// and the row blocks (remaining blocks).
template <int LPR, int RPW, class... DropArgs>   // none; (chunk_row, RowDrop); (weights); (chunk_row, RowDrop, weights); (RowTime); (RowTime, weights)
__global__ __launch_bounds__(kBlock) void spmm_rows_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const float* __restrict__ X, int64_t ldx, int d, int64_t n_rows, int short_t, int long_t,
    const int32_t* __restrict__ chunk_e0, const int32_t* __restrict__ chunk_e1, int64_t n_chunks,
    int chunk_blocks, float* __restrict__ partial, Epilogue ep, typename KernelArg<DropArgs>::type... da) {
  constexpr bool DROP = Pack<DropArgs...>::DROP, WEIGHTED = Pack<DropArgs...>::WEIGHTED, TIME = Pack<DropArgs...>::TIME;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;

  if ((int)blockIdx.x < chunk_blocks) {
    const int grp = lane / LPR;
    const int col = 4 * (lane % LPR);
    const bool lane_on = col < d;
    const int64_t ci = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (ci >= n_chunks) return;
    const float4 s = wave_row_sum<LPR, false, DROP, WEIGHTED, TIME>(
        colidx, chunk_e0[ci], chunk_e1[ci], X, ldx, lane, grp, col, lane_on, arg_of<RowDrop, DropArgs...>(da...),
        chunk_row_of<DropArgs...>(ci, da...), weights_of<DropArgs...>(0, da...), arg_of<RowTime, DropArgs...>(da...), d);
    if (grp == 0 && lane_on) st4(partial + ci * (int64_t)d + col, s);
    return;
  }

  const int64_t row0 = ((int64_t)(blockIdx.x - chunk_blocks) * kWavesPerBlock + wave) * RPW;
  if (row0 >= n_rows) return;
  rows_wave<LPR, RPW, DROP, WEIGHTED, TIME>(rowptr, colidx, X, ldx, d, n_rows, row0, short_t, long_t, ep, lane,
                                            arg_of<RowDrop, DropArgs...>(da...), weights_of<DropArgs...>(0, da...),
                                            arg_of<RowTime, DropArgs...>(da...));
}

// Fix-up for long rows: add the partial sums of a row in chunk order (a drop launch: and scale the finished sum once),
// then the epilogue.
template <int LPR, class... Scale>   // none, or (float)
__global__ __launch_bounds__(kBlock) void spmm_fixup_kernel(const int32_t* __restrict__ long_row,
                                                           const int32_t* __restrict__ long_slot,
                                                           int64_t n_long,
                                                           const float* __restrict__ partial, int d,
                                                           Epilogue ep, Scale... scale) {
  static_assert(sizeof...(Scale) <= 1, "drop-only argument: none, or the scale");
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int grp = lane / LPR;
  const int col = 4 * (lane % LPR);
  const bool lane_on = col < d;
  const int64_t li = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (li >= n_long) return;
  const float4 s = wave_row_sum<LPR, true>(nullptr, long_slot[li], long_slot[li + 1], partial, d,
                                           lane, grp, col, lane_on);
  if (grp == 0 && lane_on) finish_row(ep, long_row[li], col, scaled(s, scale...));
}

// ---- all T intervals of a layer, both directions, in ONE launch (dataset-sized graphs) ----------------------------
// The reference's loop over k (model.py:118-129) is independent per interval, so a layer of the stack is 2 T
// independent SpMMs: T with rows = users, T with rows = items. Segment s of a batch is (direction s / T, interval
// s % T); all segments of a direction have the same row count, so a row block finds its segment by division. The
// per-interval operands are slabs of [T, N, d] tensors (or columns of [N, T, d] ones): every pointer of the epilogue
// carries a slab stride, and segment (dir, k) works on base + k * stride — nothing per-call lives in device memory.
struct SegMeta {
  const int32_t* rowptr;
  const int32_t* colidx;
  int32_t short_t, long_t;
};
struct DirArgs {
  const float* X;
  int64_t ldx, s_X;
  Epilogue ep;
  // slab strides (elements; bytes for the masks) of ep's pointers
  int64_t s_res, s_acc_in, s_out, s_acc_out, s_mask_out, s_mask_in, s_out2, s_acc_in2;
};
struct BatchGeom {
  int32_t T;
  int32_t chunk_blocks;          // blocks [0, chunk_blocks): long-row chunks of every segment
  int32_t blocks_u, blocks_i;    // row blocks per user / item segment
  int32_t rows_u, rows_i;
};

__device__ __forceinline__ Epilogue seg_epilogue(const DirArgs& a, int k) {
  Epilogue e = a.ep;
  if (e.residual) e.residual += (int64_t)k * a.s_res;
  if (e.acc_in) e.acc_in += (int64_t)k * a.s_acc_in;
  if (e.out) e.out += (int64_t)k * a.s_out;
  if (e.acc_out) e.acc_out += (int64_t)k * a.s_acc_out;
  if (e.mask_out) e.mask_out += (int64_t)k * a.s_mask_out;
  if (e.mask_in) e.mask_in += (int64_t)k * a.s_mask_in;
  if (e.out2) e.out2 += (int64_t)k * a.s_out2;
  if (e.acc_in2) e.acc_in2 += (int64_t)k * a.s_acc_in2;
  return e;
}

// A drop launch: a segment's tag and orientation come from its (direction, interval). A weighted launch: a segment's
// weights come from the table of 2T pointers, indexed like SegMeta.
template <int LPR, int RPW, class... DropArgs>   // none; (chunk_row, BatchDrop); (weight table); all three; (BatchTime); (BatchTime, weight table)
__global__ __launch_bounds__(kBlock) void spmm_rows_batch_kernel(const SegMeta* __restrict__ meta, BatchGeom g,
                                                                const int32_t* __restrict__ chunk_e0,
                                                                const int32_t* __restrict__ chunk_e1,
                                                                const int32_t* __restrict__ chunk_seg, int64_t n_chunks,
                                                                float* __restrict__ partial, int d, DirArgs au, DirArgs ai,
                                                                typename KernelArg<DropArgs>::type... da) {
  constexpr bool DROP = Pack<DropArgs...>::DROP, WEIGHTED = Pack<DropArgs...>::WEIGHTED, TIME = Pack<DropArgs...>::TIME;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  if ((int)blockIdx.x < g.chunk_blocks) {
    const int grp = lane / LPR;
    const int col = 4 * (lane % LPR);
    const bool lane_on = col < d;
    const int64_t ci = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (ci >= n_chunks) return;
    const int seg = __builtin_amdgcn_readfirstlane(chunk_seg[ci]);
    const int dir = seg >= g.T, k = seg - dir * g.T;
    const DirArgs& a = dir ? ai : au;
    RowTime tm{};
    if constexpr (TIME) tm = seg_time(arg_of<BatchTime, DropArgs...>(da...), seg, dir, k);
    const float4 s = wave_row_sum<LPR, false, DROP, WEIGHTED, TIME>(
        meta[seg].colidx, chunk_e0[ci], chunk_e1[ci], a.X + (int64_t)k * a.s_X, a.ldx, lane, grp, col, lane_on,
        seg_drop(arg_of<BatchDrop, DropArgs...>(da...), dir, k), chunk_row_of<DropArgs...>(ci, da...),
        weights_of<DropArgs...>(seg, da...), tm, d);
    if (grp == 0 && lane_on) st4(partial + ci * (int64_t)d + col, s);
    return;
  }
  int rb = (int)blockIdx.x - g.chunk_blocks;
  const int dir = rb >= g.T * g.blocks_u;
  if (dir) rb -= g.T * g.blocks_u;
  const int per = dir ? g.blocks_i : g.blocks_u;
  const int k = rb / per;
  const int64_t n_rows = dir ? g.rows_i : g.rows_u;
  const int64_t row0 = ((int64_t)(rb - k * per) * kWavesPerBlock + wave) * RPW;
  if (row0 >= n_rows) return;
  const SegMeta m = meta[dir * g.T + k];
  const DirArgs& a = dir ? ai : au;
  const Epilogue ep = seg_epilogue(a, k);
  RowTime tm{};
  if constexpr (TIME) tm = seg_time(arg_of<BatchTime, DropArgs...>(da...), dir * g.T + k, dir, k);
  rows_wave<LPR, RPW, DROP, WEIGHTED, TIME>(m.rowptr, m.colidx, a.X + (int64_t)k * a.s_X, a.ldx, d, n_rows, row0, m.short_t,
                                            m.long_t, ep, lane, seg_drop(arg_of<BatchDrop, DropArgs...>(da...), dir, k),
                                            weights_of<DropArgs...>(dir * g.T + k, da...), tm);
}

template <int LPR, class... Scale>
__global__ __launch_bounds__(kBlock) void spmm_fixup_batch_kernel(const int32_t* __restrict__ long_row,
                                                                 const int32_t* __restrict__ long_slot,
                                                                 const int32_t* __restrict__ long_seg, int64_t n_long,
                                                                 const float* __restrict__ partial, int d, int T,
                                                                 DirArgs au, DirArgs ai, Scale... scale) {
  static_assert(sizeof...(Scale) <= 1, "drop-only argument: none, or the scale");
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int grp = lane / LPR;
  const int col = 4 * (lane % LPR);
  const bool lane_on = col < d;
  const int64_t li = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (li >= n_long) return;
  const int seg = __builtin_amdgcn_readfirstlane(long_seg[li]);
  const int dir = seg >= T, k = seg - dir * T;
  const Epilogue ep = seg_epilogue(dir ? ai : au, k);
  const float4 s = wave_row_sum<LPR, true>(nullptr, long_slot[li], long_slot[li + 1], partial, d, lane, grp, col, lane_on);
  if (grp == 0 && lane_on) finish_row(ep, long_row[li], col, scaled(s, scale...));
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Plan
// ------------------------------------------------------------------------------------------
struct sagnn_spmm_plan {
  sagnn_spmm_plan_info info{};
  const int32_t* d_rowptr = nullptr;
  const int32_t* d_colidx = nullptr;
  // host copies of the chunk metadata (kept for tests / introspection)
  std::vector<int32_t> chunk_row, chunk_e0, chunk_e1;
  std::vector<int32_t> long_row, long_slot;  // long_slot has n_long+1 entries
  // device copies: one allocation [chunk_e0 | chunk_e1 | long_row | long_slot | chunk_row]
  int32_t* d_meta = nullptr;
  const int32_t *d_chunk_e0 = nullptr, *d_chunk_e1 = nullptr, *d_long_row = nullptr,
                *d_long_slot = nullptr, *d_chunk_row = nullptr;   // chunk_row: read by the drop kernels only
  const float* d_weights = nullptr;   // borrowed, [nnz] in colidx order (sagnn_spmm_plan_set_weights); NULL = unweighted
  const uint16_t* d_buckets = nullptr;   // borrowed, [nnz] in colidx order (sagnn_spmm_plan_set_buckets); NULL = no time term
  int32_t n_buckets = 0;
};

namespace {
constexpr int kDefaultShort = 16;
// measured on MI355X: 256/256 beats 2048/1024 on small graphs (a 2k-edge row is
// a 60-100 us serial chain for one wave) and is on par at 100M edges
constexpr int kDefaultLong = 256;
constexpr int kDefaultChunk = 256;

int check_rowptr(const int32_t* rp, int64_t n_rows, int64_t nnz) {
  if (rp[0] != 0) return sagnn::fail(SAGNN_ERR_CSR, "rowptr[0] = %d, expected 0", rp[0]);
  for (int64_t r = 0; r < n_rows; ++r)
    if (rp[r + 1] < rp[r])
      return sagnn::fail(SAGNN_ERR_CSR, "rowptr decreases at row %lld", (long long)r);
  if (rp[n_rows] != nnz)
    return sagnn::fail(SAGNN_ERR_CSR, "rowptr[n_rows] = %d but nnz = %lld", rp[n_rows],
                       (long long)nnz);
  return SAGNN_OK;
}
}  // namespace

extern "C" int sagnn_csr_check_host(const int32_t* h_rowptr, const int32_t* h_colidx,
                                    int64_t n_rows, int64_t n_src, int64_t nnz) {
  if (!h_rowptr || (nnz > 0 && !h_colidx)) return sagnn::fail(SAGNN_ERR_NULL, "null CSR array");
  if (n_rows < 0 || n_src < 0 || nnz < 0 || nnz > INT32_MAX || n_rows >= INT32_MAX ||
      n_src > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "CSR sizes out of int32 range");
  if (int rc = check_rowptr(h_rowptr, n_rows, nnz)) return rc;
  for (int64_t e = 0; e < nnz; ++e)
    if (h_colidx[e] < 0 || h_colidx[e] >= n_src)
      return sagnn::fail(SAGNN_ERR_CSR, "colidx[%lld] = %d outside [0, %lld)", (long long)e,
                         h_colidx[e], (long long)n_src);
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_create(const int32_t* h_rowptr, const int32_t* d_rowptr,
                                      const int32_t* d_colidx, int64_t n_rows, int64_t n_src,
                                      int64_t nnz, const sagnn_spmm_tuning* tuning,
                                      sagnn_spmm_plan** plan_out) {
  if (!plan_out) return sagnn::fail(SAGNN_ERR_NULL, "plan_out is NULL");
  *plan_out = nullptr;
  if (!h_rowptr) return sagnn::fail(SAGNN_ERR_NULL, "h_rowptr is NULL");
  if ((d_rowptr == nullptr) != (d_colidx == nullptr) && nnz > 0)
    return sagnn::fail(SAGNN_ERR_NULL, "d_rowptr and d_colidx must both be given or both NULL");
  // edge cursors advance in steps of 64 past the last edge, so keep that much int32 headroom
  if (n_rows < 0 || n_src < 0 || nnz < 0 || nnz > INT32_MAX - 256 || n_rows >= INT32_MAX - 256 ||
      n_src > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "CSR sizes out of int32 range");
  if (int rc = check_rowptr(h_rowptr, n_rows, nnz)) return rc;

  sagnn_spmm_plan* p = new (std::nothrow) sagnn_spmm_plan();
  if (!p) return sagnn::fail(SAGNN_ERR_NOMEM, "out of host memory");
  int short_t = tuning && tuning->short_thresh > 0 ? tuning->short_thresh : kDefaultShort;
  int long_t = tuning && tuning->long_thresh > 0 ? tuning->long_thresh : kDefaultLong;
  int chunk = tuning && tuning->chunk_edges > 0 ? tuning->chunk_edges : kDefaultChunk;
  chunk = (chunk + kWave - 1) / kWave * kWave;
  if (long_t < short_t) long_t = short_t;

  int32_t max_deg = 0;
  try {
    p->long_slot.push_back(0);
    for (int64_t r = 0; r < n_rows; ++r) {
      const int32_t b = h_rowptr[r], e = h_rowptr[r + 1], deg = e - b;
      max_deg = std::max(max_deg, deg);
      if (deg <= long_t) continue;
      // balanced cut: nck chunks of equal length (multiple of 64, <= chunk)
      const int32_t nck = (deg + chunk - 1) / chunk;
      int32_t len = (deg + nck - 1) / nck;
      len = (len + kWave - 1) / kWave * kWave;
      for (int32_t s = b; s < e; s += len) {
        p->chunk_row.push_back((int32_t)r);
        p->chunk_e0.push_back(s);
        p->chunk_e1.push_back(std::min(e, s + len));
      }
      p->long_row.push_back((int32_t)r);
      p->long_slot.push_back((int32_t)p->chunk_row.size());
    }
  } catch (const std::bad_alloc&) {
    delete p;
    return sagnn::fail(SAGNN_ERR_NOMEM, "out of host memory building chunk list");
  }

  p->info.n_rows = n_rows;
  p->info.n_src = n_src;
  p->info.nnz = nnz;
  p->info.n_long_rows = (int64_t)p->long_row.size();
  p->info.n_chunks = (int64_t)p->chunk_row.size();
  p->info.short_thresh = short_t;
  p->info.long_thresh = long_t;
  p->info.chunk_edges = chunk;
  p->info.max_degree = max_deg;
  p->info.on_device = 0;
  p->d_rowptr = d_rowptr;
  p->d_colidx = d_colidx;

  if (d_rowptr) {
    const size_t nck = p->chunk_row.size(), nl = p->long_row.size();
    if (nck > 0) {
      const size_t words = 3 * nck + nl + (nl + 1);
      hipError_t e = hipMalloc((void**)&p->d_meta, words * sizeof(int32_t));
      if (e != hipSuccess) {
        delete p;
        return sagnn::hip_fail(e, "hipMalloc(plan metadata)");
      }
      std::vector<int32_t> host(words);
      std::copy(p->chunk_e0.begin(), p->chunk_e0.end(), host.begin());
      std::copy(p->chunk_e1.begin(), p->chunk_e1.end(), host.begin() + nck);
      std::copy(p->long_row.begin(), p->long_row.end(), host.begin() + 2 * nck);
      std::copy(p->long_slot.begin(), p->long_slot.end(), host.begin() + 2 * nck + nl);
      std::copy(p->chunk_row.begin(), p->chunk_row.end(), host.begin() + 2 * nck + 2 * nl + 1);
      e = hipMemcpy(p->d_meta, host.data(), words * sizeof(int32_t), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(p->d_meta);
        delete p;
        return sagnn::hip_fail(e, "hipMemcpy(plan metadata)");
      }
      p->d_chunk_e0 = p->d_meta;
      p->d_chunk_e1 = p->d_meta + nck;
      p->d_long_row = p->d_meta + 2 * nck;
      p->d_long_slot = p->d_meta + 2 * nck + nl;
      p->d_chunk_row = p->d_meta + 2 * nck + 2 * nl + 1;
    }
    p->info.on_device = 1;
  }
  *plan_out = p;
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_destroy(sagnn_spmm_plan* plan) {
  if (!plan) return SAGNN_OK;
  if (plan->d_meta) (void)hipFree(plan->d_meta);
  delete plan;
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_set_weights(sagnn_spmm_plan* plan, const float* d_weights) {
  if (!plan) return sagnn::fail(SAGNN_ERR_NULL, "plan is NULL");
  if (!plan->info.on_device) return sagnn::fail(SAGNN_ERR_ARG, "plan was built host-only (no device CSR): it takes no weights");
  if (d_weights && (reinterpret_cast<uintptr_t>(d_weights) & 3))
    return sagnn::fail(SAGNN_ERR_ALIGN, "weights: pointer must be 4-byte aligned");
  plan->d_weights = d_weights;
  plan->info.weighted = d_weights ? 1 : 0;
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_set_buckets(sagnn_spmm_plan* plan, const uint16_t* d_buckets, int32_t n_buckets) {
  if (!plan) return sagnn::fail(SAGNN_ERR_NULL, "plan is NULL");
  if (!plan->info.on_device) return sagnn::fail(SAGNN_ERR_ARG, "plan was built host-only (no device CSR): it takes no buckets");
  if (d_buckets && (n_buckets < 1 || n_buckets > 65535))
    return sagnn::fail(SAGNN_ERR_ARG, "buckets: n_buckets = %d, need 1 <= n_buckets <= 65535 (uint16 ids)", n_buckets);
  if (d_buckets && (reinterpret_cast<uintptr_t>(d_buckets) & 1))
    return sagnn::fail(SAGNN_ERR_ALIGN, "buckets: pointer must be 2-byte aligned");
  plan->d_buckets = d_buckets;
  plan->n_buckets = d_buckets ? n_buckets : 0;
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_get_info(const sagnn_spmm_plan* plan, sagnn_spmm_plan_info* info) {
  if (!plan || !info) return sagnn::fail(SAGNN_ERR_NULL, "plan/info is NULL");
  *info = plan->info;
  return SAGNN_OK;
}

extern "C" int sagnn_spmm_plan_copy_chunks(const sagnn_spmm_plan* plan, int32_t* rows,
                                           int32_t* e_begin, int32_t* e_end, int64_t cap) {
  if (!plan) return sagnn::fail(SAGNN_ERR_NULL, "plan is NULL");
  const int64_t n = plan->info.n_chunks;
  if (cap < n) return sagnn::fail(SAGNN_ERR_ARG, "cap %lld < n_chunks %lld", (long long)cap, (long long)n);
  if (n > 0 && (!rows || !e_begin || !e_end)) return sagnn::fail(SAGNN_ERR_NULL, "null output array");
  std::copy(plan->chunk_row.begin(), plan->chunk_row.end(), rows);
  std::copy(plan->chunk_e0.begin(), plan->chunk_e0.end(), e_begin);
  std::copy(plan->chunk_e1.begin(), plan->chunk_e1.end(), e_end);
  return SAGNN_OK;
}

extern "C" size_t sagnn_spmm_workspace_bytes(const sagnn_spmm_plan* plan, int d) {
  if (!plan || d <= 0) return 0;
  return (size_t)plan->info.n_chunks * (size_t)d * sizeof(float);
}

// ------------------------------------------------------------------------------------------
// Launch
// ------------------------------------------------------------------------------------------
namespace {

// drop = nullptr, te = nullptr and a plan without weights: the default kernels. The row block of a wave (small) and the
// trailing arguments (the drop's, the plan's weights, the time term's) name the instantiation of a kernel; its launch is
// stated once. te: the product's TE table (the plan's buckets index it); never with a drop.
template <int LPR>
int launch_spmm(const sagnn_spmm_plan* p, const float* X, int64_t ldx, int d, const Epilogue& ep,
                float* partial, hipStream_t stream, const RowDrop* drop = nullptr, const float* te = nullptr) {
  const int64_t n_rows = p->info.n_rows;
  const int64_t n_chunks = p->info.n_chunks;
  const int64_t chunk_blocks = (n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
  constexpr int G = kWave / LPR;
  constexpr int RPW_SMALL = G > 4 ? G : 4;        // one row per lane group (at least 4 rows)
  const bool small = n_rows < kSmallRows;
  const int64_t rows_per_block = (int64_t)kWavesPerBlock * (small ? RPW_SMALL : kRowsPerWave);
  const int64_t row_blocks = (n_rows + rows_per_block - 1) / rows_per_block;
  const int64_t blocks = chunk_blocks + row_blocks;
  if (blocks > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "grid too large");
  if (blocks > 0) {
    sagnn::ProfileScope prof(sagnn::kProfSpmmRows, stream, p->info.nnz, n_rows);
    const auto rows = [&](auto kernel, auto... da) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, p->d_rowptr, p->d_colidx, X, ldx, d, n_rows,
                         p->info.short_thresh, p->info.long_thresh, p->d_chunk_e0, p->d_chunk_e1, n_chunks,
                         (int)chunk_blocks, partial, ep, da...);
    };
    const float* w = p->d_weights;
    const RowTime tm{p->d_buckets, te};
    if (te && w)
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL, RowTime, const float*> : spmm_rows_kernel<LPR, kRowsPerWave, RowTime, const float*>,
           tm, w);
    else if (te)
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL, RowTime> : spmm_rows_kernel<LPR, kRowsPerWave, RowTime>, tm);
    else if (drop && w)
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL, const int32_t*, RowDrop, const float*>
                 : spmm_rows_kernel<LPR, kRowsPerWave, const int32_t*, RowDrop, const float*>,
           p->d_chunk_row, *drop, w);
    else if (drop)
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL, const int32_t*, RowDrop> : spmm_rows_kernel<LPR, kRowsPerWave, const int32_t*, RowDrop>,
           p->d_chunk_row, *drop);
    else if (w)
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL, const float*> : spmm_rows_kernel<LPR, kRowsPerWave, const float*>, w);
    else
      rows(small ? spmm_rows_kernel<LPR, RPW_SMALL> : spmm_rows_kernel<LPR, kRowsPerWave>);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  const int64_t n_long = p->info.n_long_rows;
  if (n_long > 0) {
    sagnn::ProfileScope prof(sagnn::kProfSpmmFixup, stream, n_chunks, n_long);
    const int64_t fb = (n_long + kWavesPerBlock - 1) / kWavesPerBlock;
    const auto fixup = [&](auto kernel, auto... scale) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)fb), dim3(kBlock), 0, stream,
                         p->d_long_row, p->d_long_slot, n_long, partial, d, ep, scale...);
    };
    if (drop) fixup(spmm_fixup_kernel<LPR, float>, drop->scale);
    else fixup(spmm_fixup_kernel<LPR>);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  return SAGNN_OK;
}

int check_mat(const char* name, const void* ptr, int64_t ld, int d, bool required) {
  if (!ptr) return required ? sagnn::fail(SAGNN_ERR_NULL, "%s is NULL", name) : SAGNN_OK;
  if (!sagnn::aligned16(ptr) || (ld & 3) != 0)
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: pointer must be 16-byte aligned and ld a multiple of 4", name);
  if (ld < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: ld %lld < d %d", name, (long long)ld, d);
  return SAGNN_OK;
}

int check_d(int d) {
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "d = %d: need a multiple of 4 in [4, 256]", d);
  return SAGNN_OK;
}

struct Slab {           // a [T, N, d]-like operand: interval k's matrix starts at p + k * slab, rows ld apart
  float* p;
  int64_t ld, slab;
};

int check_slab(const char* name, const Slab& x, int d) {
  if (int rc = check_mat(name, x.p, x.ld, d, true)) return rc;
  if (x.slab & 3) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: slab stride must be a multiple of 4", name);
  return SAGNN_OK;
}

// out = g * (mask bit ? 1 : slope) on the T matrices of a slab; mask slabs s_mask bytes apart, d/4 bytes per row
int launch_mask_scale(const Slab& g, const uint8_t* mask, int64_t s_mask, float slope, const Slab& out, int64_t n_rows,
                      int d, int64_t T, hipStream_t stream) {
  const int64_t n = n_rows * (d / 4);
  if (n == 0) return SAGNN_OK;
  hipLaunchKernelGGL(mask_scale_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, stream, g.p, g.ld,
                     g.slab, mask, s_mask, d / 4, slope, out.p, out.ld, out.slab, n_rows, d);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

// The kernels' epilogue of the caller's (masks: d / 4 bytes per row)
Epilogue kernel_epilogue(const sagnn_spmm_epilogue& e, int d) {
  return Epilogue{e.residual, e.ldr,      e.acc_in,  e.ld_acc_in, e.out,  e.ldo,    e.acc_out, e.ld_acc_out,
                  e.leaky,    e.mask_out, e.mask_in, e.out2,      e.ldo2, e.slope2, d / 4,     e.acc_in2,
                  e.ld_acc_in2};
}

// sagnn_spmm_ex_f32 on the kernels' own epilogue: every per-call check, then the launch(es) of one plan
int spmm_ex(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d, const Epilogue& e, void* workspace,
            size_t workspace_bytes, void* stream, const RowDrop* drop = nullptr, const float* te = nullptr) {
  if (!plan->info.on_device) return sagnn::fail(SAGNN_ERR_ARG, "plan was built host-only (no device CSR)");
  if (int rc = check_d(d)) return rc;
  if (te) {
    if (drop) return sagnn::fail(SAGNN_ERR_ARG, "edge time: no product takes a drop and a time term");
    if (!plan->d_buckets) return sagnn::fail(SAGNN_ERR_ARG, "edge time: the plan has no buckets (sagnn_spmm_plan_set_buckets)");
    if (!sagnn::aligned16(te)) return sagnn::fail(SAGNN_ERR_ALIGN, "edge time: TE must be 16-byte aligned");
  }
  if (!e.out && !e.acc_out && !e.out2) return sagnn::fail(SAGNN_ERR_NULL, "no output given");
  if (int rc = check_mat("X", X, ldx, d, plan->info.nnz > 0)) return rc;
  if (int rc = check_mat("residual", e.residual, e.ldr, d, false)) return rc;
  if (int rc = check_mat("out", e.out, e.ldo, d, false)) return rc;
  if (int rc = check_mat("acc_in", e.acc_in, e.ld_acc_in, d, false)) return rc;
  if (int rc = check_mat("acc_out", e.acc_out, e.ld_acc_out, d, false)) return rc;
  if (int rc = check_mat("acc_in2", e.acc_in2, e.ld_acc_in2, d, false)) return rc;
  if (e.acc_in2 && !e.acc_out) return sagnn::fail(SAGNN_ERR_ARG, "acc_in2 given without acc_out");
  if (int rc = check_mat("out2", e.out2, e.ldo2, d, false)) return rc;
  if ((e.out && e.out == X) || (e.acc_out && e.acc_out == X) || (e.out2 && e.out2 == X))
    return sagnn::fail(SAGNN_ERR_ARG, "outputs must not alias X");
  if (e.mask_in && !e.out2) return sagnn::fail(SAGNN_ERR_ARG, "mask_in given without out2");
  const size_t need = sagnn_spmm_workspace_bytes(plan, d);
  if (need > 0) {
    if (!workspace || workspace_bytes < need)
      return sagnn::fail(SAGNN_ERR_WORKSPACE, "workspace needs %zu bytes, got %zu", need,
                         workspace ? workspace_bytes : (size_t)0);
    if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "workspace not 16-byte aligned");
  }
  if (plan->info.n_rows == 0) return SAGNN_OK;

  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  switch (sagnn::lanes_per_row(d)) {
    case 8: return launch_spmm<8>(plan, X, ldx, d, e, partial, s, drop, te);
    case 16: return launch_spmm<16>(plan, X, ldx, d, e, partial, s, drop, te);
    case 32: return launch_spmm<32>(plan, X, ldx, d, e, partial, s, drop, te);
    default: return launch_spmm<64>(plan, X, ldx, d, e, partial, s, drop, te);
  }
}

}  // namespace

extern "C" int sagnn_spmm_ex_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                                 const sagnn_spmm_epilogue* e, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!plan || !e) return sagnn::fail(SAGNN_ERR_NULL, "plan/epilogue is NULL");
  return spmm_ex(plan, X, ldx, d, kernel_epilogue(*e, d), workspace, workspace_bytes, stream);
}

namespace {
constexpr int kDropMaxLayers = 127;          // tag = (k << 8) | (l << 1) | dir: seven bits of layer
constexpr int64_t kDropMaxIntervals = 1 << 23;

// The caller's sagnn_edge_drop, checked ahead of everything else of a drop entry (no device work before it passes)
int check_drop(const sagnn_edge_drop* drop, int n_layers, int64_t last_interval) {
  if (!drop) return sagnn::fail(SAGNN_ERR_NULL, "edge drop: the sagnn_edge_drop is NULL");
  if (drop->keep_threshold == 0) return sagnn::fail(SAGNN_ERR_ARG, "edge drop: keep_threshold = 0 keeps no edge");
  if (!(drop->scale > 0.f) || !(drop->scale <= FLT_MAX))
    return sagnn::fail(SAGNN_ERR_ARG, "edge drop: scale = %g, need a finite value > 0", (double)drop->scale);
  if (n_layers > kDropMaxLayers)
    return sagnn::fail(SAGNN_ERR_ARG, "edge drop: n_layers = %d, the tag holds %d", n_layers, kDropMaxLayers);
  if (last_interval < 0 || last_interval >= kDropMaxIntervals)
    return sagnn::fail(SAGNN_ERR_ARG, "edge drop: interval %lld outside [0, 2^23)", (long long)last_interval);
  return SAGNN_OK;
}

RowDrop row_drop(const sagnn_edge_drop& e, uint32_t tag, bool rows_users) {
  return RowDrop{(uint32_t)e.seed, (uint32_t)(e.seed >> 32), e.step, e.keep_threshold, tag, rows_users ? 1 : 0, e.scale};
}
}  // namespace

extern "C" int sagnn_spmm_drop_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                                   const sagnn_spmm_epilogue* e, const sagnn_edge_drop* drop, uint32_t tag,
                                   int rows_are_users, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_drop(drop, 0, 0)) return rc;
  if (!plan || !e) return sagnn::fail(SAGNN_ERR_NULL, "plan/epilogue is NULL");
  const RowDrop dr = row_drop(*drop, tag, rows_are_users != 0);
  return spmm_ex(plan, X, ldx, d, kernel_epilogue(*e, d), workspace, workspace_bytes, stream, &dr);
}

extern "C" int sagnn_spmm_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                              const float* residual, int64_t ldr, float leaky, float* out,
                              int64_t ldo, const float* acc_in, int64_t ld_acc_in, float* acc_out,
                              int64_t ld_acc_out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  sagnn_spmm_epilogue e{};
  e.leaky = leaky;
  e.residual = residual;
  e.ldr = ldr;
  e.out = out;
  e.ldo = ldo;
  e.acc_in = acc_in;
  e.ld_acc_in = ld_acc_in;
  e.acc_out = acc_out;
  e.ld_acc_out = ld_acc_out;
  return sagnn_spmm_ex_f32(plan, X, ldx, d, &e, workspace, workspace_bytes, stream);
}

// out[r, :] = g[r, :] * (mask bit ? 1 : slope): the seed of the backward chain (what run_backward does first),
// exposed for hosts that run the chain themselves on row slices (parallel.FractionalRunner.run_backward).
extern "C" int sagnn_mask_scale_f32(const float* g, int64_t ldg, const uint8_t* mask, float slope, float* out, int64_t ldo,
                                    int64_t n_rows, int d, void* stream) {
  if (!g || !mask || !out) return sagnn::fail(SAGNN_ERR_NULL, "null pointer");
  if (int rc = check_d(d)) return rc;
  if (n_rows < 0) return sagnn::fail(SAGNN_ERR_ARG, "n_rows = %lld", (long long)n_rows);
  if (int rc = check_mat("g", g, ldg, d, true)) return rc;
  if (int rc = check_mat("out", out, ldo, d, true)) return rc;
  return launch_mask_scale(Slab{const_cast<float*>(g), ldg, 0}, mask, 0, slope, Slab{out, ldo, 0}, n_rows, d, 1,
                           static_cast<hipStream_t>(stream));
}

namespace {
int check_interval_plans(const sagnn_spmm_plan* pu, const sagnn_spmm_plan* pi) {
  if (!pu || !pi) return sagnn::fail(SAGNN_ERR_NULL, "plan is NULL");
  if (pu->info.n_src != pi->info.n_rows || pi->info.n_src != pu->info.n_rows)
    return sagnn::fail(SAGNN_ERR_ARG, "plans are not a transposed pair: user %lldx%lld, item %lldx%lld",
                       (long long)pu->info.n_rows, (long long)pu->info.n_src, (long long)pi->info.n_rows,
                       (long long)pi->info.n_src);
  return SAGNN_OK;
}
}  // namespace

// ------------------------------------------------------------------------------------------
// Batch over the T intervals: one launch per LAYER of the stack (+ one fix-up launch)
// ------------------------------------------------------------------------------------------
struct sagnn_spmm_batch {
  int T = 0;
  int64_t U = 0, I = 0;
  int64_t n_chunks = 0, n_long = 0, nnz = 0;
  // device: [SegMeta x 2T] and [chunk_e0 | chunk_e1 | chunk_seg | long_row | long_seg | long_slot (+1) | chunk_row]
  SegMeta* d_meta = nullptr;
  const float** d_weights = nullptr;   // [2T] the segments' weight pointers as the plans held them at creation; NULL = unweighted
  const uint16_t** d_buckets = nullptr;   // [2T] likewise the bucket pointers; NULL = the plans have none
  int32_t n_buckets = 0;
  int32_t* d_ints = nullptr;
  const int32_t *d_chunk_e0 = nullptr, *d_chunk_e1 = nullptr, *d_chunk_seg = nullptr, *d_long_row = nullptr,
                *d_long_seg = nullptr, *d_long_slot = nullptr, *d_chunk_row = nullptr;
};

namespace {
// The tables of a batch; `paired`: the plans of an interval must be a transposed pair (sagnn_spmm_batch_create). The time
// batch (sagnn_spmm_time_batch_create) gathers from U rows on one side and I rows on the other into n_buckets rows each.
int batch_create(const sagnn_spmm_plan* const* plans_user, const sagnn_spmm_plan* const* plans_item, int n_intervals,
                 bool paired, sagnn_spmm_batch** batch_out) {
  if (!batch_out) return sagnn::fail(SAGNN_ERR_NULL, "batch_out is NULL");
  *batch_out = nullptr;
  if (!plans_user || !plans_item) return sagnn::fail(SAGNN_ERR_NULL, "plan table is NULL");
  if (n_intervals < 1 || n_intervals > 4096) return sagnn::fail(SAGNN_ERR_ARG, "n_intervals = %d", n_intervals);
  const int T = n_intervals;
  for (int k = 0; k < T; ++k) {
    if (paired) {
      if (int rc = check_interval_plans(plans_user[k], plans_item[k])) return rc;
    } else {
      if (!plans_user[k] || !plans_item[k]) return sagnn::fail(SAGNN_ERR_NULL, "plan is NULL");
      if (plans_user[k]->info.n_rows != plans_item[k]->info.n_rows || plans_user[k]->info.n_src != plans_user[0]->info.n_src ||
          plans_item[k]->info.n_src != plans_item[0]->info.n_src)
        return sagnn::fail(SAGNN_ERR_ARG, "interval %d: time-adjoint plans need one bucket count and one source row count per side", k);
    }
    if (!plans_user[k]->info.on_device || !plans_item[k]->info.on_device)
      return sagnn::fail(SAGNN_ERR_ARG, "interval %d: plan was built host-only", k);
    if (plans_user[k]->info.n_rows != plans_user[0]->info.n_rows || plans_item[k]->info.n_rows != plans_item[0]->info.n_rows)
      return sagnn::fail(SAGNN_ERR_ARG, "interval %d: every interval must have the same user / item counts", k);
  }
  const bool weighted = plans_user[0]->d_weights != nullptr;
  // a batch carries buckets when all its plans do, with one bucket count; otherwise it has none and the time entries
  // refuse it (the adjoint batch of a model mixes forward plans with exact adjoints that need no buckets)
  int32_t n_buckets = plans_user[0]->n_buckets;
  for (int k = 0; k < T; ++k)
    for (const sagnn_spmm_plan* p : {plans_user[k], plans_item[k]}) {
      if ((p->d_weights != nullptr) != weighted)
        return sagnn::fail(SAGNN_ERR_ARG, "interval %d: some plans of the batch carry edge weights and others do not "
                           "(sagnn_spmm_plan_set_weights): give all 2 T plans weights or none", k);
      if (p->n_buckets != n_buckets) n_buckets = 0;
    }
  sagnn_spmm_batch* b = new (std::nothrow) sagnn_spmm_batch();
  if (!b) return sagnn::fail(SAGNN_ERR_NOMEM, "out of host memory");
  b->T = T;
  b->U = plans_user[0]->info.n_rows;
  b->I = plans_item[0]->info.n_rows;
  std::vector<SegMeta> meta(2 * (size_t)T);
  std::vector<const float*> wtab(2 * (size_t)T);
  std::vector<const uint16_t*> btab(2 * (size_t)T);
  b->n_buckets = n_buckets;
  std::vector<int32_t> ce0, ce1, cseg, crow, lrow, lseg, lslot;
  try {
    for (int s = 0; s < 2 * T; ++s) {
      const sagnn_spmm_plan* p = s < T ? plans_user[s] : plans_item[s - T];
      meta[s] = SegMeta{p->d_rowptr, p->d_colidx, p->info.short_thresh, p->info.long_thresh};
      wtab[s] = p->d_weights;
      btab[s] = p->d_buckets;
      const int32_t coff = (int32_t)ce0.size();
      ce0.insert(ce0.end(), p->chunk_e0.begin(), p->chunk_e0.end());
      ce1.insert(ce1.end(), p->chunk_e1.begin(), p->chunk_e1.end());
      cseg.insert(cseg.end(), p->chunk_e0.size(), (int32_t)s);
      crow.insert(crow.end(), p->chunk_row.begin(), p->chunk_row.end());
      for (size_t j = 0; j < p->long_row.size(); ++j) {
        lrow.push_back(p->long_row[j]);
        lseg.push_back((int32_t)s);
        lslot.push_back(coff + p->long_slot[j]);
      }
      b->nnz += p->info.nnz;
    }
    lslot.push_back((int32_t)ce0.size());
  } catch (const std::bad_alloc&) {
    delete b;
    return sagnn::fail(SAGNN_ERR_NOMEM, "out of host memory building the batch tables");
  }
  if (ce0.size() > (size_t)INT32_MAX - 256) {
    delete b;
    return sagnn::fail(SAGNN_ERR_ARG, "too many long-row chunks for one batch");
  }
  b->n_chunks = (int64_t)ce0.size();
  b->n_long = (int64_t)lrow.size();
  hipError_t e = hipMalloc((void**)&b->d_meta, meta.size() * sizeof(SegMeta));
  if (e == hipSuccess) e = hipMemcpy(b->d_meta, meta.data(), meta.size() * sizeof(SegMeta), hipMemcpyHostToDevice);
  if (e == hipSuccess && weighted) {
    e = hipMalloc((void**)&b->d_weights, wtab.size() * sizeof(const float*));
    if (e == hipSuccess) e = hipMemcpy(b->d_weights, wtab.data(), wtab.size() * sizeof(const float*), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && n_buckets > 0) {
    e = hipMalloc((void**)&b->d_buckets, btab.size() * sizeof(const uint16_t*));
    if (e == hipSuccess) e = hipMemcpy(b->d_buckets, btab.data(), btab.size() * sizeof(const uint16_t*), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && b->n_chunks > 0) {
    const size_t nck = ce0.size(), nl = lrow.size();
    std::vector<int32_t> host;
    host.reserve(4 * nck + 3 * nl + 1);
    host.insert(host.end(), ce0.begin(), ce0.end());
    host.insert(host.end(), ce1.begin(), ce1.end());
    host.insert(host.end(), cseg.begin(), cseg.end());
    host.insert(host.end(), lrow.begin(), lrow.end());
    host.insert(host.end(), lseg.begin(), lseg.end());
    host.insert(host.end(), lslot.begin(), lslot.end());
    host.insert(host.end(), crow.begin(), crow.end());
    e = hipMalloc((void**)&b->d_ints, host.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(b->d_ints, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    b->d_chunk_e0 = b->d_ints;
    b->d_chunk_e1 = b->d_ints + nck;
    b->d_chunk_seg = b->d_ints + 2 * nck;
    b->d_long_row = b->d_ints + 3 * nck;
    b->d_long_seg = b->d_ints + 3 * nck + nl;
    b->d_long_slot = b->d_ints + 3 * nck + 2 * nl;
    b->d_chunk_row = b->d_ints + 3 * nck + 3 * nl + 1;
  }
  if (e != hipSuccess) {
    if (b->d_meta) (void)hipFree(b->d_meta);
    if (b->d_weights) (void)hipFree(b->d_weights);
    if (b->d_buckets) (void)hipFree(b->d_buckets);
    if (b->d_ints) (void)hipFree(b->d_ints);
    delete b;
    return sagnn::hip_fail(e, "batch tables (hipMalloc / hipMemcpy)");
  }
  *batch_out = b;
  return SAGNN_OK;
}
}  // namespace

extern "C" int sagnn_spmm_batch_create(const sagnn_spmm_plan* const* plans_user, const sagnn_spmm_plan* const* plans_item,
                                       int n_intervals, sagnn_spmm_batch** batch_out) {
  return batch_create(plans_user, plans_item, n_intervals, true, batch_out);
}

extern "C" int sagnn_spmm_time_batch_create(const sagnn_spmm_plan* const* adj_user, const sagnn_spmm_plan* const* adj_item,
                                            int n_intervals, sagnn_spmm_batch** batch_out) {
  return batch_create(adj_user, adj_item, n_intervals, false, batch_out);
}

extern "C" int sagnn_spmm_batch_destroy(sagnn_spmm_batch* b) {
  if (!b) return SAGNN_OK;
  if (b->d_meta) (void)hipFree(b->d_meta);
  if (b->d_weights) (void)hipFree(b->d_weights);
  if (b->d_buckets) (void)hipFree(b->d_buckets);
  if (b->d_ints) (void)hipFree(b->d_ints);
  delete b;
  return SAGNN_OK;
}

extern "C" size_t sagnn_spmm_batch_workspace_bytes(const sagnn_spmm_batch* b, int d) {
  if (!b || d <= 0) return 0;
  return (size_t)b->n_chunks * (size_t)d * sizeof(float);
}

namespace {

template <int LPR>
int launch_batch(const sagnn_spmm_batch* b, int d, const DirArgs& au, const DirArgs& ai, float* partial, hipStream_t stream,
                 const BatchDrop* drop, const BatchTime* time) {
  constexpr int G = kWave / LPR;
  constexpr int RPW_SMALL = G > 4 ? G : 4;
  const bool small = (b->U > b->I ? b->U : b->I) < kSmallRows;
  const int64_t rpb = (int64_t)kWavesPerBlock * (small ? RPW_SMALL : kRowsPerWave);
  const int64_t chunk_blocks = (b->n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t bu = (b->U + rpb - 1) / rpb, bi = (b->I + rpb - 1) / rpb;
  const int64_t blocks = chunk_blocks + (int64_t)b->T * (bu + bi);
  if (blocks > INT32_MAX || b->U > INT32_MAX || b->I > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "grid too large");
  const BatchGeom g{b->T, (int32_t)chunk_blocks, (int32_t)bu, (int32_t)bi, (int32_t)b->U, (int32_t)b->I};
  if (blocks > 0) {
    sagnn::ProfileScope prof(sagnn::kProfSpmmRows, stream, b->nnz, (int64_t)b->T * (b->U + b->I));
    const auto rows = [&](auto kernel, auto... da) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, b->d_meta, g, b->d_chunk_e0, b->d_chunk_e1,
                         b->d_chunk_seg, b->n_chunks, partial, d, au, ai, da...);
    };
    const float* const* w = b->d_weights;
    if (time && w)
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL, BatchTime, const float* const*>
                 : spmm_rows_batch_kernel<LPR, kRowsPerWave, BatchTime, const float* const*>, *time, w);
    else if (time)
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL, BatchTime> : spmm_rows_batch_kernel<LPR, kRowsPerWave, BatchTime>, *time);
    else if (drop && w)
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL, const int32_t*, BatchDrop, const float* const*>
                 : spmm_rows_batch_kernel<LPR, kRowsPerWave, const int32_t*, BatchDrop, const float* const*>,
           b->d_chunk_row, *drop, w);
    else if (drop)
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL, const int32_t*, BatchDrop>
                 : spmm_rows_batch_kernel<LPR, kRowsPerWave, const int32_t*, BatchDrop>,
           b->d_chunk_row, *drop);
    else if (w)
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL, const float* const*>
                 : spmm_rows_batch_kernel<LPR, kRowsPerWave, const float* const*>, w);
    else
      rows(small ? spmm_rows_batch_kernel<LPR, RPW_SMALL> : spmm_rows_batch_kernel<LPR, kRowsPerWave>);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  if (b->n_long > 0) {
    sagnn::ProfileScope prof(sagnn::kProfSpmmFixup, stream, b->n_chunks, b->n_long);
    const int64_t fb = (b->n_long + kWavesPerBlock - 1) / kWavesPerBlock;
    const auto fixup = [&](auto kernel, auto... scale) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)fb), dim3(kBlock), 0, stream,
                         b->d_long_row, b->d_long_slot, b->d_long_seg, b->n_long, partial, d, b->T, au, ai, scale...);
    };
    if (drop) fixup(spmm_fixup_batch_kernel<LPR, float>, drop->r.scale);
    else fixup(spmm_fixup_batch_kernel<LPR>);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  return SAGNN_OK;
}

int launch_batch_d(const sagnn_spmm_batch* b, int d, const DirArgs& au, const DirArgs& ai, float* partial, hipStream_t s,
                   const BatchDrop* drop = nullptr, const BatchTime* time = nullptr) {
  switch (sagnn::lanes_per_row(d)) {
    case 8: return launch_batch<8>(b, d, au, ai, partial, s, drop, time);
    case 16: return launch_batch<16>(b, d, au, ai, partial, s, drop, time);
    case 32: return launch_batch<32>(b, d, au, ai, partial, s, drop, time);
    default: return launch_batch<64>(b, d, au, ai, partial, s, drop, time);
  }
}


int check_batch_ws(const sagnn_spmm_batch* b, int d, const void* workspace, size_t workspace_bytes) {
  const size_t need = sagnn_spmm_batch_workspace_bytes(b, d);
  if (need == 0) return SAGNN_OK;
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "workspace needs %zu bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
  if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "workspace not 16-byte aligned");
  return SAGNN_OK;
}

// ------------------------------------------------------------------------------------------
// The layer schedule of the GNN stack (model.py:118-129), forward and backward, stated once for one interval
// (sagnn_gnn_interval_*: T = 1, slab strides unused) and for a batch of T (sagnn_gnn_stack_*)
// ------------------------------------------------------------------------------------------
struct Side {           // the operands of one node type
  Slab in, out;         // forward: e^0 and sum_l e^l; backward: G = dL/d(sum_l e^l) and dL/d e^0
  float* scratch;       // [2][T][rows][d] forward (unused for one layer), [4][T][rows][d] backward
  uint8_t* mask;        // [T][n_layers][rows][d/4] activation masks: written forward (optional), read backward
  int64_t rows;
};
struct Stack {
  Side u, i;
  int64_t T;
  int d, n_layers;
  float leaky;
};

Slab scratch_slot(const Stack& st, const Side& s, int slot) {
  return Slab{s.scratch + slot * st.T * s.rows * st.d, (int64_t)st.d, s.rows * st.d};
}

// Alignment of a stack's operands, ahead of any launch (the scratch only where the schedule uses it)
int check_stack(const Stack& st, bool scratch_used, const char* in_u, const char* in_i, const char* out_u, const char* out_i) {
  if (int rc = check_slab(in_u, st.u.in, st.d)) return rc;
  if (int rc = check_slab(in_i, st.i.in, st.d)) return rc;
  if (int rc = check_slab(out_u, st.u.out, st.d)) return rc;
  if (int rc = check_slab(out_i, st.i.out, st.d)) return rc;
  if (scratch_used && (!sagnn::aligned16(st.u.scratch) || !sagnn::aligned16(st.i.scratch)))
    return sagnn::fail(SAGNN_ERR_ALIGN, "scratch buffers must be 16-byte aligned");
  return SAGNN_OK;
}

// Forward layer l on the rows of `self`, gathering the rows of `other`:  e^{l+1} = leaky(A e_other^l) + e^l.
DirArgs forward_layer(const Stack& st, const Side& self, const Side& other, int l) {
  const bool last = (l + 1 == st.n_layers);
  const int64_t mrow = st.d / 4;
  // e^0 is the caller's table; layer l writes e^{l+1} into half l & 1 of the ping-pong scratch
  // (skipped for the last layer, whose only consumer is the running sum).
  const Slab cur = l == 0 ? self.in : scratch_slot(st, self, (l - 1) & 1);
  const Slab x = l == 0 ? other.in : scratch_slot(st, other, (l - 1) & 1);
  DirArgs a{};
  a.ep.leaky = st.leaky;
  a.ep.mask_stride = (int)mrow;
  a.X = x.p, a.ldx = x.ld, a.s_X = x.slab;
  a.ep.residual = cur.p, a.ep.ldr = cur.ld, a.s_res = cur.slab;
  if (!last) {
    const Slab next = scratch_slot(st, self, l & 1);
    a.ep.out = next.p, a.ep.ldo = next.ld, a.s_out = next.slab;
  }
  // Running sum sum_l e^l without a write that is only read back: layer 0 of a deeper stack
  // writes e^1 alone; layer 1 starts the sum from e^1 (its residual, already in registers);
  // the LAST layer adds e^0 on the way out (acc_in2). One layer: acc_out = e^0 + e^1 directly.
  if (last || l >= 1) {
    const Slab acc = l <= 1 ? cur : self.out;
    a.ep.acc_in = acc.p, a.ep.ld_acc_in = acc.ld, a.s_acc_in = acc.slab;
    a.ep.acc_out = self.out.p, a.ep.ld_acc_out = self.out.ld, a.s_acc_out = self.out.slab;
    if (last && l >= 1) a.ep.acc_in2 = self.in.p, a.ep.ld_acc_in2 = self.in.ld, a.s_acc_in2 = self.in.slab;
  }
  if (self.mask) {
    a.ep.mask_out = self.mask + (int64_t)l * self.rows * mrow;
    a.s_mask_out = (int64_t)st.n_layers * self.rows * mrow;
  }
  return a;
}

// Backward of the stack. With g^l = dL/de^l (l = 0..L), G = dL/d(sum_l e^l):
//   g_u^L = G_u,  g_i^L = G_i
//   g_u^l = G_u + g_u^{l+1} + A   (g_i^{l+1} * m_i^{l+1})     (rows = users)
//   g_i^l = G_i + g_i^{l+1} + A^T (g_u^{l+1} * m_u^{l+1})     (rows = items)
// m^{l+1} = slope mask of the forward layer that produced e^{l+1} (1 where the activation passed
// the sum through, leaky elsewhere). Each step is the forward kernel with slope 1, residual =
// g^{l+1}, acc_in = G, and the masked copy for the next step written by the same epilogue.
// Scratch slots 0/1 ping-pong the full gradients g^l, slots 2/3 the masked copies; the seed g^L * m^L is in slot 2.
DirArgs backward_step(const Stack& st, const Side& self, const Side& other, int l) {
  const int L = st.n_layers;
  const int64_t mrow = st.d / 4;
  const int cur = (L - 1 - l) & 1;   // which masked copy holds g^{l+1} * m^{l+1}
  const Slab x = scratch_slot(st, other, 2 + cur);
  const Slab g_next = (l == L - 1) ? self.in : scratch_slot(st, self, (l + 1) & 1);
  const Slab g = (l == 0) ? self.out : scratch_slot(st, self, l & 1);
  DirArgs a{};
  a.ep.leaky = 1.f;
  a.ep.mask_stride = (int)mrow;
  a.X = x.p, a.ldx = x.ld, a.s_X = x.slab;
  a.ep.residual = g_next.p, a.ep.ldr = g_next.ld, a.s_res = g_next.slab;
  a.ep.acc_in = self.in.p, a.ep.ld_acc_in = self.in.ld, a.s_acc_in = self.in.slab;
  a.ep.acc_out = g.p, a.ep.ld_acc_out = g.ld, a.s_acc_out = g.slab;
  if (l > 0) {
    const Slab gm = scratch_slot(st, self, 2 + (cur ^ 1));
    a.ep.mask_in = self.mask + (int64_t)(l - 1) * self.rows * mrow;
    a.s_mask_in = (int64_t)L * self.rows * mrow;
    a.ep.out2 = gm.p, a.ep.ldo2 = gm.ld, a.s_out2 = gm.slab;
    a.ep.slope2 = st.leaky;
  }
  return a;
}

// The edge-dropout tags of one launch pair (without the interval): tag_u for the launch whose rows are users, tag_i for
// the one whose rows are items. dir 0 = the forward's user-side product A e_i, dir 1 = its item-side product A^T e_u.
struct LayerTags {
  uint32_t tag_u, tag_i;
  int layer;              // read by the time forms: which TE[:, l, :] the launch pair adds
};

// The drivers: `launch(au, ai, tags)` runs one layer, rows = users and rows = items (batched() or per_plan() below;
// only the drop forms read the tags).
template <class Launch>
int run_forward(const Stack& st, Launch launch) {
  for (int l = 0; l < st.n_layers; ++l)
    if (int rc = launch(forward_layer(st, st.u, st.i, l), forward_layer(st, st.i, st.u, l),
                        LayerTags{(uint32_t)l << 1, (uint32_t)l << 1 | 1u, l}))
      return rc;
  return SAGNN_OK;
}

// before_step(l, gm_u, gm_i) runs ahead of step l with the masked gradients g^{l+1} * m^{l+1} of both sides, which are
// the gradients at the row sums of layer l's two products (the time forms reduce them into dTE[:, l, :]).
struct NoBeforeStep {
  int operator()(int, const Slab&, const Slab&) const { return SAGNN_OK; }
};
template <class Launch, class BeforeStep = NoBeforeStep>
int run_backward(const Stack& st, Launch launch, void* stream, BeforeStep before_step = BeforeStep{}) {
  for (const Side* s : {&st.u, &st.i}) {   // seed: g^L * m^L of every interval (one launch per node type)
    const int64_t mrow = st.d / 4;
    if (int rc = launch_mask_scale(s->in, s->mask + (int64_t)(st.n_layers - 1) * s->rows * mrow, st.n_layers * s->rows * mrow,
                                   st.leaky, scratch_slot(st, *s, 2), s->rows, st.d, st.T, static_cast<hipStream_t>(stream)))
      return rc;
  }
  // Step l's rows = users launch is the adjoint of layer l's ITEM-side product (it carries g_i^{l+1} back to the users
  // through the transpose of the pattern that product gathered through), so it drops with that product's tag (dir 1)
  // on rows that are users; the rows = items launch mirrors it with the user-side tag (dir 0).
  for (int l = st.n_layers - 1; l >= 0; --l) {
    const int cur = (st.n_layers - 1 - l) & 1;
    if (int rc = before_step(l, scratch_slot(st, st.u, 2 + cur), scratch_slot(st, st.i, 2 + cur))) return rc;
    if (int rc = launch(backward_step(st, st.u, st.i, l), backward_step(st, st.i, st.u, l),
                        LayerTags{(uint32_t)l << 1 | 1u, (uint32_t)l << 1, l}))
      return rc;
  }
  return SAGNN_OK;
}

// One launch per layer for all T intervals and both directions (+ one fix-up launch when the batch has long rows)
auto batched(const sagnn_spmm_batch* b, int d, void* workspace, void* stream) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags&) {
    return launch_batch_d(b, d, au, ai, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
  };
}

auto batched_drop(const sagnn_spmm_batch* b, int d, void* workspace, void* stream, const sagnn_edge_drop& drop) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags& t) {
    const BatchDrop bd{row_drop(drop, t.tag_u, true), t.tag_i};
    return launch_batch_d(b, d, au, ai, static_cast<float*>(workspace), static_cast<hipStream_t>(stream), &bd);
  };
}

// One interval: the user-side launch, then the item-side launch, each with the per-call checks of sagnn_spmm_ex_f32
auto per_plan(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item, int d, void* workspace,
              size_t workspace_bytes, void* stream) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags&) {
    if (int rc = spmm_ex(plan_user, au.X, au.ldx, d, au.ep, workspace, workspace_bytes, stream)) return rc;
    return spmm_ex(plan_item, ai.X, ai.ldx, d, ai.ep, workspace, workspace_bytes, stream);
  };
}

// per_plan with edge dropout; `interval` is the k of the tags
auto per_plan_drop(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item, int d, void* workspace,
                   size_t workspace_bytes, void* stream, const sagnn_edge_drop& drop, int interval) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags& t) {
    const uint32_t k = (uint32_t)interval << 8;
    const RowDrop du = row_drop(drop, t.tag_u | k, true), di = row_drop(drop, t.tag_i | k, false);
    if (int rc = spmm_ex(plan_user, au.X, au.ldx, d, au.ep, workspace, workspace_bytes, stream, &du)) return rc;
    return spmm_ex(plan_item, ai.X, ai.ldx, d, ai.ep, workspace, workspace_bytes, stream, &di);
  };
}

// ---- the time forms (sagnn_edge_time) ----
// The caller's sagnn_edge_time, checked ahead of every launch of a time entry; n_buckets: that of the plans / the batch
int check_time(const sagnn_edge_time* t, const sagnn_edge_drop* drop, int32_t n_buckets, int d) {
  if (drop) return sagnn::fail(SAGNN_ERR_ARG, "edge time: edge dropout and time do not combine (drop must be NULL)");
  if (!t || !t->te) return sagnn::fail(SAGNN_ERR_NULL, "edge time: the sagnn_edge_time or its te is NULL");
  if (n_buckets == 0) return sagnn::fail(SAGNN_ERR_ARG, "edge time: the plans carry no buckets (sagnn_spmm_plan_set_buckets)");
  if (t->n_buckets != n_buckets)
    return sagnn::fail(SAGNN_ERR_ARG, "edge time: n_buckets = %d but the plans were given %d", t->n_buckets, n_buckets);
  if (!sagnn::aligned16(t->te) || ((t->stride_interval | t->stride_layer | t->stride_dir) & 3) || (d & 3))
    return sagnn::fail(SAGNN_ERR_ALIGN, "edge time: te must be 16-byte aligned and its strides multiples of 4");
  return SAGNN_OK;
}

// what the backward entries need on top: where dTE goes and the time-adjoint plans (interval) or batch (stack)
int check_time_bwd(const sagnn_edge_time* t, bool stack, int64_t U, int64_t I, int T) {
  if (!t->dte) return sagnn::fail(SAGNN_ERR_NULL, "edge time: dte is NULL");
  if (!sagnn::aligned16(t->dte)) return sagnn::fail(SAGNN_ERR_ALIGN, "edge time: dte must be 16-byte aligned");
  if (stack) {
    const sagnn_spmm_batch* b = t->adj_batch;
    if (!b) return sagnn::fail(SAGNN_ERR_NULL, "edge time: adj_batch is NULL");
    if (b->T != T || b->U != t->n_buckets || b->I != t->n_buckets)
      return sagnn::fail(SAGNN_ERR_ARG, "edge time: adj_batch is not the time batch of %d intervals and %d buckets", T, t->n_buckets);
    return SAGNN_OK;
  }
  if (!t->adj_user || !t->adj_item) return sagnn::fail(SAGNN_ERR_NULL, "edge time: adj_user / adj_item is NULL");
  if (t->adj_user->info.n_rows != t->n_buckets || t->adj_item->info.n_rows != t->n_buckets || t->adj_user->info.n_src != U ||
      t->adj_item->info.n_src != I)
    return sagnn::fail(SAGNN_ERR_ARG, "edge time: adj_user / adj_item are not %d x %lld and %d x %lld", t->n_buckets,
                       (long long)U, t->n_buckets, (long long)I);
  return SAGNN_OK;
}

// per_plan / batched with the time term of layer t.layer; `interval`: the k of a per-plan pair
auto per_plan_time(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item, int d, void* workspace,
                   size_t workspace_bytes, void* stream, const sagnn_edge_time& tm, int interval) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags& t) {
    const float* te = tm.te + interval * tm.stride_interval + t.layer * tm.stride_layer;
    if (int rc = spmm_ex(plan_user, au.X, au.ldx, d, au.ep, workspace, workspace_bytes, stream, nullptr, te)) return rc;
    return spmm_ex(plan_item, ai.X, ai.ldx, d, ai.ep, workspace, workspace_bytes, stream, nullptr, te + tm.stride_dir);
  };
}

auto batched_time(const sagnn_spmm_batch* b, int d, void* workspace, void* stream, const sagnn_edge_time& tm) {
  return [=](const DirArgs& au, const DirArgs& ai, const LayerTags& t) {
    const BatchTime bt{b->d_buckets, tm.te + t.layer * tm.stride_layer, tm.stride_interval, tm.stride_dir};
    return launch_batch_d(b, d, au, ai, static_cast<float*>(workspace), static_cast<hipStream_t>(stream), nullptr, &bt);
  };
}

// dTE[:, l, dir] = (time adjoint of that product) . gm: a plain product (slope 1, no residual) whose rows are buckets
DirArgs dte_args(const Slab& gm, float* out, int d, int64_t s_out) {
  DirArgs a{};
  a.ep.leaky = 1.f;
  a.ep.mask_stride = d / 4;
  a.X = gm.p, a.ldx = gm.ld, a.s_X = gm.slab;
  a.ep.out = out, a.ep.ldo = d, a.s_out = s_out;
  return a;
}

auto dte_per_plan(const sagnn_edge_time& tm, int d, int interval, void* stream) {
  return [=](int l, const Slab& gm_u, const Slab& gm_i) {
    float* dte = tm.dte + interval * tm.stride_interval + l * tm.stride_layer;
    if (int rc = spmm_ex(tm.adj_user, gm_u.p, gm_u.ld, d, dte_args(gm_u, dte, d, 0).ep, tm.adj_workspace,
                         tm.adj_workspace_bytes, stream))
      return rc;
    return spmm_ex(tm.adj_item, gm_i.p, gm_i.ld, d, dte_args(gm_i, dte + tm.stride_dir, d, 0).ep, tm.adj_workspace,
                   tm.adj_workspace_bytes, stream);
  };
}

auto dte_batched(const sagnn_edge_time& tm, int d, void* stream) {
  return [=](int l, const Slab& gm_u, const Slab& gm_i) {
    float* dte = tm.dte + l * tm.stride_layer;
    return launch_batch_d(tm.adj_batch, d, dte_args(gm_u, dte, d, tm.stride_interval),
                          dte_args(gm_i, dte + tm.stride_dir, d, tm.stride_interval), static_cast<float*>(tm.adj_workspace),
                          static_cast<hipStream_t>(stream));
  };
}

Slab slab(const float* p, int64_t ld, int64_t stride) { return Slab{const_cast<float*>(p), ld, stride}; }

// ---- the four entries (include/sagnn.h, "The GNN stack") ----
// What an entry runs on: the plan pair of one interval (T = 1, slab strides unused) or a batch of T intervals. Apart from
// this geometry and the launcher it selects, the interval and the stack entries are the same code.
struct Graphs {
  const sagnn_spmm_plan *plan_user, *plan_item;   // the interval entries
  const sagnn_spmm_batch* batch;                  // the stack entries
  bool stack;
  bool given() const { return stack ? batch != nullptr : plan_user && plan_item; }
  int64_t T() const { return stack ? batch->T : 1; }
  int64_t U() const { return stack ? batch->U : plan_user->info.n_rows; }
  int64_t I() const { return stack ? batch->I : plan_item->info.n_rows; }
};

int check_graphs(const Graphs& g) {
  if (g.stack) return g.batch ? SAGNN_OK : sagnn::fail(SAGNN_ERR_NULL, "batch is NULL");
  return check_interval_plans(g.plan_user, g.plan_item);
}

// What the form named by args->edges checks ahead of the shared body. DROP looks at its struct before anything else,
// the graphs included; TIME at the graphs first, because it compares their bucket count with the struct's.
int check_form(const Graphs& g, const sagnn_gnn_args* a, bool backward) {
  if (!a) return sagnn::fail(SAGNN_ERR_NULL, "the sagnn_gnn_args is NULL");
  switch (a->edges) {
    case SAGNN_EDGES_PLAIN:
      if (a->drop || a->time) return sagnn::fail(SAGNN_ERR_ARG, "edges = SAGNN_EDGES_PLAIN with a drop or time struct");
      return SAGNN_OK;
    case SAGNN_EDGES_DROP:
      return check_drop(a->drop, a->n_layers, !g.stack ? a->interval : g.batch ? g.batch->T - 1 : 0);
    case SAGNN_EDGES_TIME: {
      if (!g.given()) return sagnn::fail(SAGNN_ERR_NULL, g.stack ? "batch is NULL" : "plan is NULL");
      // The forward's graphs carry the buckets. The backward's are the adjoint patterns, which need none (the chain
      // does not see the time term): there the buckets are in time->adj_user / adj_item / adj_batch.
      int32_t n_buckets = a->time ? a->time->n_buckets : 0;
      if (!backward) {
        if (!g.stack && g.plan_user->n_buckets != g.plan_item->n_buckets)
          return sagnn::fail(SAGNN_ERR_ARG, "edge time: the two plans carry different bucket counts (or only one carries buckets)");
        n_buckets = g.stack ? g.batch->n_buckets : g.plan_user->n_buckets;
      }
      if (int rc = check_time(a->time, a->drop, n_buckets, a->d)) return rc;
      if (!g.stack && a->interval < 0) return sagnn::fail(SAGNN_ERR_ARG, "edge time: interval = %d", a->interval);
      return backward ? check_time_bwd(a->time, g.stack, g.U(), g.I(), (int)g.T()) : SAGNN_OK;
    }
  }
  return sagnn::fail(SAGNN_ERR_ARG, "edges = %d: not a SAGNN_EDGES_* value", a->edges);
}

Stack make_stack(const Graphs& g, const sagnn_gnn_args& a) {
  const auto side = [&](const sagnn_gnn_side& s, int64_t rows) {
    return Side{slab(s.in, s.ld_in, g.stack ? s.slab_in : 0), slab(s.out, s.ld_out, g.stack ? s.slab_out : 0), s.scratch,
                s.mask, rows};
  };
  return Stack{side(a.user, g.U()), side(a.item, g.I()), g.T(), a.d, a.n_layers, a.leaky};
}

// run(launcher): the launcher of one layer for these graphs and edge form
template <class Run>
int with_launcher(const Graphs& g, const sagnn_gnn_args& a, void* stream, Run run) {
  void* const ws = a.workspace;
  const size_t n = a.workspace_bytes;
  switch (a.edges) {
    case SAGNN_EDGES_DROP:
      return g.stack ? run(batched_drop(g.batch, a.d, ws, stream, *a.drop))
                     : run(per_plan_drop(g.plan_user, g.plan_item, a.d, ws, n, stream, *a.drop, a.interval));
    case SAGNN_EDGES_TIME:
      return g.stack ? run(batched_time(g.batch, a.d, ws, stream, *a.time))
                     : run(per_plan_time(g.plan_user, g.plan_item, a.d, ws, n, stream, *a.time, a.interval));
    default:
      return g.stack ? run(batched(g.batch, a.d, ws, stream)) : run(per_plan(g.plan_user, g.plan_item, a.d, ws, n, stream));
  }
}

int gnn_forward(const Graphs& g, const sagnn_gnn_args* a, void* stream) {
  if (int rc = check_form(g, a, false)) return rc;
  if (int rc = check_graphs(g)) return rc;
  const sagnn_gnn_side &u = a->user, &i = a->item;
  if (!u.in || !i.in || !u.out || !i.out) return sagnn::fail(SAGNN_ERR_NULL, "null embedding pointer");
  if (g.stack)   // a batch is on the device, so d comes first; an interval looks at d after its plan (below)
    if (int rc = check_d(a->d)) return rc;
  if (a->n_layers < 1) return sagnn::fail(SAGNN_ERR_ARG, "n_layers = %d: need >= 1", a->n_layers);
  if ((u.mask == nullptr) != (i.mask == nullptr)) return sagnn::fail(SAGNN_ERR_NULL, "give both masks or neither");
  if (a->n_layers > 1 && (!u.scratch || !i.scratch))
    return sagnn::fail(SAGNN_ERR_NULL, "scratch buffers required for n_layers > 1");
  if (!g.stack) {
    // the first launch refuses a host-only plan before it looks at d: keep that order
    if (!g.plan_user->info.on_device) return sagnn::fail(SAGNN_ERR_ARG, "plan was built host-only (no device CSR)");
    if (int rc = check_d(a->d)) return rc;
  }
  const Stack st = make_stack(g, *a);
  if (int rc = check_stack(st, a->n_layers > 1, "u0", "i0", "user_out", "item_out")) return rc;
  if (g.stack)   // (the per-plan launches check the workspace themselves, as sagnn_spmm_ex_f32 does)
    if (int rc = check_batch_ws(g.batch, a->d, a->workspace, a->workspace_bytes)) return rc;
  return with_launcher(g, *a, stream, [&](auto launch) { return run_forward(st, launch); });
}

int gnn_backward(const Graphs& g, const sagnn_gnn_args* a, void* stream) {
  if (int rc = check_form(g, a, true)) return rc;
  if (int rc = check_graphs(g)) return rc;
  const sagnn_gnn_side &u = a->user, &i = a->item;
  if (!u.in || !i.in || !u.out || !i.out || !u.mask || !i.mask || !u.scratch || !i.scratch)
    return sagnn::fail(SAGNN_ERR_NULL, "null pointer");
  if (a->n_layers < 1) return sagnn::fail(SAGNN_ERR_ARG, "n_layers = %d: need >= 1", a->n_layers);
  if (int rc = check_d(a->d)) return rc;
  const Stack st = make_stack(g, *a);
  if (int rc = check_stack(st, true, "G_u", "G_i", "grad_u0", "grad_i0")) return rc;
  if (g.stack)
    if (int rc = check_batch_ws(g.batch, a->d, a->workspace, a->workspace_bytes)) return rc;
  if (a->edges != SAGNN_EDGES_TIME)
    return with_launcher(g, *a, stream, [&](auto launch) { return run_backward(st, launch, stream); });
  // the adjoint chain does not see the time term: the plain launches, and dTE ahead of each step
  const sagnn_edge_time& tm = *a->time;
  if (!g.stack)
    return run_backward(st, per_plan(g.plan_user, g.plan_item, a->d, a->workspace, a->workspace_bytes, stream), stream,
                        dte_per_plan(tm, a->d, a->interval, stream));
  if (int rc = check_batch_ws(tm.adj_batch, a->d, tm.adj_workspace, tm.adj_workspace_bytes)) return rc;
  return run_backward(st, batched(g.batch, a->d, a->workspace, stream), stream, dte_batched(tm, a->d, stream));
}
}  // namespace

// One interval k of the loop of model.py:118-129: 2 L launches through the per-call checks of sagnn_spmm_ex_f32.
extern "C" int sagnn_gnn_interval_f32(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item,
                                      const sagnn_gnn_args* args, void* stream) {
  return gnn_forward(Graphs{plan_user, plan_item, nullptr, false}, args, stream);
}

// plan_user / plan_item: the ADJOINT plans (for canonical matrices the forward plans themselves).
extern "C" int sagnn_gnn_interval_bwd_f32(const sagnn_spmm_plan* plan_user, const sagnn_spmm_plan* plan_item,
                                          const sagnn_gnn_args* args, void* stream) {
  return gnn_backward(Graphs{plan_user, plan_item, nullptr, false}, args, stream);
}

// The whole loop — every interval, every layer — in L row launches (+ L fix-up launches when the graphs have long rows).
extern "C" int sagnn_gnn_stack_f32(const sagnn_spmm_batch* batch, const sagnn_gnn_args* args, void* stream) {
  return gnn_forward(Graphs{nullptr, nullptr, batch, true}, args, stream);
}

// batch: the batch of the ADJOINT patterns (for canonical matrices the same batch).
extern "C" int sagnn_gnn_stack_bwd_f32(const sagnn_spmm_batch* batch, const sagnn_gnn_args* args, void* stream) {
  return gnn_backward(Graphs{nullptr, nullptr, batch, true}, args, stream);
}

// One product with a time table (include/sagnn.h, "Time-aware messages")
extern "C" int sagnn_spmm_time_f32(const sagnn_spmm_plan* plan, const float* X, int64_t ldx, int d,
                                   const sagnn_spmm_epilogue* e, const sagnn_edge_drop* drop, const sagnn_edge_time* time,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!plan || !e) return sagnn::fail(SAGNN_ERR_NULL, "plan/epilogue is NULL");
  if (int rc = check_time(time, drop, plan->n_buckets, d)) return rc;
  return spmm_ex(plan, X, ldx, d, kernel_epilogue(*e, d), workspace, workspace_bytes, stream, nullptr, time->te);
}
