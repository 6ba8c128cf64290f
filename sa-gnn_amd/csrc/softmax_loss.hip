// Full-catalogue softmax cross-entropy (sagnn_softmax_loss_f32 / _bwd_f32): z(b, i) = <Q[b], I[i]> * inv_temp on the
// exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32), loss = scale * sum_b (ln sum_{i eligible} exp z(b, i) - z(b, t_b)).
// The [queries x items] logits are never stored: the forward streams a log-sum-exp, the backward recomputes them.
//
// Forward pass 1 (lse_chunk_kernel): one wavefront per (kNT query tiles of 16 rows, item chunk), laid out as
// retrieval.hip's topk_chunk_kernel: item rows are the A operand, the Q fragments stay in registers, acc[r] is the
// score of item 4 * (lane >> 4) + r for query lane & 15. One item fragment feeds kNT query tiles. A lane keeps a running
// (max, sum) over its items; the four lanes of a query are combined by shuffles and one (max, sum) per (query, chunk)
// goes to the workspace. An empty side has max = -inf and sum = 0 and is never passed through exp(-inf - (-inf)).
// Pass 2 (lse_row_kernel): one wavefront per query merges the chunk partials (a fixed tree over the chunk index) into
// lse[b], takes the target's score from the same tile arithmetic and writes the row's loss term.
// Pass 3 (loss_sum_kernel): one workgroup adds the row terms in a fixed order into loss[0]. No atomics anywhere.
//
// Backward, g(b, i) = (g * scale * inv_temp) * (p(b, i) - [i == t_b]), p = exp(z - lse[b]) on eligible items:
// dq_chunk_kernel: the forward's grid and layout. The accumulator, turned into g in place, is the B operand of
//   dQ^T[16 features x 16 queries] += I^T[features x items] . G[items x queries]: MFMA r contracts over the items
//   4 * (lane >> 4) + r, so its A operand is element (item 4 * (lane >> 4) + r, feature f0 + (lane & 15)). A lane ends
//   with four contiguous features of one query. Per-chunk partials go to the workspace; dq_merge_kernel adds them in
//   chunk order.
// di_kernel: one wavefront per kNI item tiles loops over all query tiles with the QUERIES on the accumulator rows
//   (queries as A, items as B), so the accumulator is the B operand of dI^T[16 features x 16 items] += Q^T . G and a
//   lane ends with four contiguous features of one item row. 64 lanes look up the exclusions of 64 queries at once
//   (lower bound at the span's first item, then a walk into a bit mask) and hand the masks over by shuffle.
// Chunks depend on n_items only and every sum has a fixed order, so lse / tscore / dQ of a row depend on that row alone
// and all outputs are bit-identical between runs.
//
// The same loss over a candidate list shared by the batch (sagnn_softmax_loss_cand_f32 / _bwd_f32, --softmaxNegs) runs
// sibling kernels over the list's positions; they follow the full-catalogue kernels below.
#include "common.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNT = 2;            // query tiles per wavefront in the chunk kernels
constexpr int kMinChunk = 128;    // items per chunk at least (a multiple of 16)
constexpr int kMaxChunks = 256;
constexpr int kSmallSpans = 256;   // di_cand_kernel: fewer spans than this run at 16 positions per wavefront instead

struct Problem {
  const float* Q;
  int64_t ldq;
  const float* I;
  int64_t ldi;
  int64_t n_queries, n_items;
  const int32_t* target;
  float inv_temp, scale;
  const int64_t* excl_ptr;
  const int32_t* excl_items;
  const int32_t* excl_row;
  int64_t n_lists;
  int64_t chunk, n_chunks;
};

// Chunks from n_items alone: at most kMaxChunks of them, at least kMinChunk items each, a multiple of 16.
__host__ __device__ inline int64_t chunk_items(int64_t n_items) {
  int64_t c = (n_items + kMaxChunks - 1) / kMaxChunks;
  if (c < kMinChunk) c = kMinChunk;
  return (c + 15) / 16 * 16;
}

// (m, s) += (om, os) for sums s * exp(m); an empty side is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mx = fmaxf(m, om);
  if (mx == -INFINITY) return;
  s = s * __expf(m - mx) + os * __expf(om - mx);
  m = mx;
}

// The exclusion list of query row b as [lo, hi) into excl_items; empty when there is none.
__device__ __forceinline__ void excl_range(const Problem& p, int64_t b, int64_t& lo, int64_t& hi) {
  lo = hi = 0;
  if (!p.excl_ptr) return;
  const int64_t L = p.excl_row ? (int64_t)p.excl_row[b] : b;
  if (L < 0 || L >= p.n_lists) return;
  lo = p.excl_ptr[L];
  hi = p.excl_ptr[L + 1];
}

__device__ __forceinline__ int64_t excl_lower_bound(const int32_t* __restrict__ items, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)items[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// A lane's walk over its row's exclusions as the chunk advances
struct Walk {
  int64_t ep, ee;
  int nxt;                                               // excl_items[ep] while ep < ee
};

__device__ __forceinline__ void walk_init(const Problem& p, int64_t b, bool ok, int64_t c0, Walk& w) {
  w.ep = w.ee = 0;
  w.nxt = 0;
  if (!ok) return;
  int64_t lo, hi;
  excl_range(p, b, lo, hi);
  w.ee = hi;
  w.ep = excl_lower_bound(p.excl_items, lo, hi, c0);
  if (w.ep < w.ee) w.nxt = p.excl_items[w.ep];
}

// bit r: item s0 + 4g + r is on the list (the walk passes every entry below s0 + 16)
__device__ __forceinline__ unsigned walk_bits(const Problem& p, Walk& w, int64_t s0, int g) {
  unsigned xm = 0;
  while (w.ep < w.ee && (int64_t)w.nxt < s0 + 16) {
    const int64_t off = (int64_t)w.nxt - s0;
    if (off >= 0 && (off >> 2) == g) xm |= 1u << (off & 3);
    if (++w.ep < w.ee) w.nxt = p.excl_items[w.ep];
  }
  return xm;
}

// acc[r] = <row 4 * (lane >> 4) + r of the A side, row lane & 15 of the B side>; a[t] / b[t] are the lane's float4 of
// its A / B row at columns 16t + 4 * (lane >> 4). A fixed fmaf chain over the columns.
template <int D>
__device__ __forceinline__ f32x4 tile_scores(const float4 (&a)[D / 16], const float4 (&b)[D / 16]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[t].w, acc, 0, 0, 0);
  }
  return acc;
}

template <int D>
__device__ __forceinline__ void load_frag(const float* __restrict__ row, int g, float4 (&f)[D / 16]) {
#pragma unroll
  for (int t = 0; t < D / 16; ++t) f[t] = *reinterpret_cast<const float4*>(row + 16 * t + 4 * g);
}

// What a lane of the chunk kernels knows about the query lane & 15 of one of its tiles
template <int D>
struct QueryLane {
  float4 qf[D / 16];
  int64_t b;
  bool in, ok;                                           // row exists; row exists and has a target
  int ti;                                                // the target, -1 without one
  Walk w;
};

template <int D>
__device__ __forceinline__ void query_init(const Problem& p, int64_t b, int64_t c0, int g, QueryLane<D>& ql) {
  ql.b = b;
  ql.in = b < p.n_queries;
  const int64_t bq = ql.in ? b : p.n_queries - 1;
  const int32_t tv = p.target[bq];
  ql.ok = ql.in && tv >= 0 && (int64_t)tv < p.n_items;
  ql.ti = ql.ok ? tv : -1;
  load_frag<D>(p.Q + bq * p.ldq, g, ql.qf);
  walk_init(p, bq, ql.ok, c0, ql.w);
}

template <int D>
__global__ __launch_bounds__(64) void lse_chunk_kernel(Problem p, float2* __restrict__ part) {
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < p.n_items ? c0 + p.chunk : p.n_items;
  QueryLane<D> ql[kNT];
  float m[kNT], s[kNT];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, c0, g, ql[u]);
    m[u] = -INFINITY;
    s[u] = 0.f;
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    int64_t it = s0 + q;
    if (it >= p.n_items) it = p.n_items - 1;
    float4 a[D / 16];
    load_frag<D>(p.I + it * p.ldi, g, a);
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = walk_bits(p, ql[u].w, s0, g);
      float z[4];
      bool e[4];
      float mx = m[u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t item = s0 + 4 * g + r;
        e[r] = ql[u].ok && item < c1 && (!((xm >> r) & 1) || item == ql[u].ti);
        z[r] = acc[r] * p.inv_temp;
        if (e[r]) mx = fmaxf(mx, z[r]);
      }
      if (mx > -INFINITY) {
        float sum = s[u] * __expf(m[u] - mx);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e[r]) sum += __expf(z[r] - mx);
        s[u] = sum;
        m[u] = mx;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    lse_merge(m[u], s[u], __shfl_xor(m[u], 16), __shfl_xor(s[u], 16));
    lse_merge(m[u], s[u], __shfl_xor(m[u], 32), __shfl_xor(s[u], 32));
    if (ql[u].in && g == 0) part[ql[u].b * p.n_chunks + blockIdx.y] = make_float2(m[u], s[u]);
  }
}

template <int D>
__global__ __launch_bounds__(64) void lse_row_kernel(Problem p, const float2* __restrict__ part, float* __restrict__ lse,
                                                     float* __restrict__ tscore, float* __restrict__ terms) {
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int64_t b = blockIdx.x;
  const int32_t tv = p.target[b];
  const bool ok = tv >= 0 && (int64_t)tv < p.n_items;
  float m = -INFINITY, s = 0.f;
  for (int64_t j = lane; j < p.n_chunks; j += 64) {
    const float2 v = part[b * p.n_chunks + j];
    lse_merge(m, s, v.x, v.y);
  }
  for (int off = 1; off < 64; off <<= 1) lse_merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
  // the target's score: every row of the A side is the target, every row of the B side the query
  float4 a[D / 16], qf[D / 16];
  load_frag<D>(p.I + (int64_t)(ok ? tv : 0) * p.ldi, g, a);
  load_frag<D>(p.Q + b * p.ldq, g, qf);
  const f32x4 acc = tile_scores<D>(a, qf);
  if (lane == 0) {
    const float l = ok ? m + logf(s) : 0.f;
    const float ts = ok ? acc[0] : 0.f;
    lse[b] = l;
    tscore[b] = ts;
    terms[b] = ok ? l - ts * p.inv_temp : 0.f;
  }
}

__global__ __launch_bounds__(256) void loss_sum_kernel(const float* __restrict__ terms, int64_t n, float scale,
                                                       float* __restrict__ loss) {
  __shared__ float sh[256];
  float v = 0.f;
  for (int64_t b = threadIdx.x; b < n; b += 256) v += terms[b];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = scale * sh[0];
}

// g(b, i) of one accumulator element: z = acc * inv_temp
__device__ __forceinline__ float grad_elem(float acc, float inv_temp, float lse, float coef, bool elig, bool is_target) {
  const float pr = elig ? __expf(acc * inv_temp - lse) : 0.f;
  return coef * (pr - (is_target ? 1.f : 0.f));
}

template <int D>
__global__ __launch_bounds__(64) void dq_chunk_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                      float* __restrict__ part) {
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < p.n_items ? c0 + p.chunk : p.n_items;
  const float coef = gup[0] * p.scale * p.inv_temp;
  QueryLane<D> ql[kNT];
  float row_lse[kNT];
  f32x4 dq[kNT][D / 16];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, c0, g, ql[u]);
    row_lse[u] = lse[ql[u].in ? ql[u].b : p.n_queries - 1];
#pragma unroll
    for (int f = 0; f < D / 16; ++f) dq[u][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    int64_t it = s0 + q;
    if (it >= p.n_items) it = p.n_items - 1;
    float4 a[D / 16];
    load_frag<D>(p.I + it * p.ldi, g, a);
    f32x4 G[kNT];
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = walk_bits(p, ql[u].w, s0, g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t item = s0 + 4 * g + r;
        const bool tgt = ql[u].ok && item == ql[u].ti;
        const bool e = ql[u].ok && item < c1 && (!((xm >> r) & 1) || tgt);
        G[u][r] = ql[u].ok ? grad_elem(acc[r], p.inv_temp, row_lse[u], coef, e, tgt) : 0.f;
      }
    }
    // dQ^T += I^T G: MFMA r contracts over items s0 + 4g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int64_t ir = s0 + 4 * g + r;
      if (ir >= p.n_items) ir = p.n_items - 1;
      const float* row = p.I + ir * p.ldi + q;
#pragma unroll
      for (int f = 0; f < D / 16; ++f) {
        const float av = row[16 * f];
#pragma unroll
        for (int u = 0; u < kNT; ++u) dq[u][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, G[u][r], dq[u][f], 0, 0, 0);
      }
    }
  }
  // lane (g, q) holds features 16f + 4g .. + 3 of query q
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    if (!ql[u].in) continue;
    float* out = part + ((int64_t)blockIdx.y * p.n_queries + ql[u].b) * D + 4 * g;
#pragma unroll
    for (int f = 0; f < D / 16; ++f)
      *reinterpret_cast<float4*>(out + 16 * f) = make_float4(dq[u][f][0], dq[u][f][1], dq[u][f][2], dq[u][f][3]);
  }
}

// dQ[b, 4c .. 4c + 3] = the chunk partials added in chunk order
__global__ __launch_bounds__(256) void dq_merge_kernel(const float* __restrict__ part, int64_t n_queries, int d,
                                                       int64_t n_chunks, float* __restrict__ dQ, int64_t lddq) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = d / 4;
  if (e >= n_queries * per_row) return;
  const int64_t b = e / per_row;
  const int c = (int)(e % per_row);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t j = 0; j < n_chunks; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(part + (j * n_queries + b) * d + 4 * c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<float4*>(dQ + b * lddq + 4 * c) = acc;
}

template <int D, int NI>
__global__ __launch_bounds__(64) void di_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                float* __restrict__ dI, int64_t lddi) {
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * (16 * NI);
  const float coef = gup[0] * p.scale * p.inv_temp;
  float4 ib[NI][D / 16];                                 // item rows as the B side of the scores
  f32x4 di[NI][D / 16];
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    int64_t it = i0 + 16 * v + c;
    if (it >= p.n_items) it = p.n_items - 1;
    load_frag<D>(p.I + it * p.ldi, g, ib[v]);
#pragma unroll
    for (int f = 0; f < D / 16; ++f) di[v][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t qg = 0; qg < p.n_queries; qg += 64) {
    // lane l: the exclusions of query qg + l inside [i0, i1) as a bit mask
    unsigned mask_lo = 0, mask_hi = 0;
    if (p.excl_ptr && qg + lane < p.n_queries) {
      int64_t lo, hi;
      excl_range(p, qg + lane, lo, hi);
      int64_t ep = excl_lower_bound(p.excl_items, lo, hi, i0);
      while (ep < hi) {
        const int64_t off = (int64_t)p.excl_items[ep] - i0;
        if (off >= 16 * NI) break;
        if (off >= 0) {
          if (off < 32) mask_lo |= 1u << off; else mask_hi |= 1u << (off - 32);
        }
        ++ep;
      }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int64_t qb = qg + 16 * j;
      if (qb >= p.n_queries) break;                      // uniform over the wavefront
      int64_t ra = qb + c;                               // the A row of the scores
      if (ra >= p.n_queries) ra = p.n_queries - 1;
      float4 qa[D / 16];
      load_frag<D>(p.Q + ra * p.ldq, g, qa);
      // the four queries qb + 4g + r of this lane's accumulator rows
      float row_lse[4];
      int ti[4];
      unsigned xl[4], xh[4];
      int64_t rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = qb + 4 * g + r;
        const bool in = b < p.n_queries;
        rq[r] = in ? b : p.n_queries - 1;
        const int32_t tv = p.target[rq[r]];
        ti[r] = (in && tv >= 0 && (int64_t)tv < p.n_items) ? tv : -1;
        row_lse[r] = lse[rq[r]];
        xl[r] = __shfl(mask_lo, 16 * j + 4 * g + r);
        xh[r] = __shfl(mask_hi, 16 * j + 4 * g + r);
      }
      f32x4 G[NI];
#pragma unroll
      for (int v = 0; v < NI; ++v) {
        const f32x4 acc = tile_scores<D>(qa, ib[v]);     // acc[r] = score(query qb + 4g + r, item i0 + 16v + c)
        const int off = 16 * v + c;
        const int64_t item = i0 + off;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = ti[r] >= 0 && item < p.n_items;
          const bool tgt = ok && item == ti[r];
          const bool ex = ((off < 32 ? xl[r] >> off : xh[r] >> (off - 32)) & 1) != 0;
          G[v][r] = ok ? grad_elem(acc[r], p.inv_temp, row_lse[r], coef, !ex || tgt, tgt) : 0.f;
        }
      }
      // dI^T += Q^T G: MFMA r contracts over queries qb + 4g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = p.Q + rq[r] * p.ldq + c;
#pragma unroll
        for (int f = 0; f < D / 16; ++f) {
          const float av = row[16 * f];
#pragma unroll
          for (int v = 0; v < NI; ++v) di[v][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, G[v][r], di[v][f], 0, 0, 0);
        }
      }
    }
  }
  // lane (g, c) holds features 16f + 4g .. + 3 of item i0 + 16v + c
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    const int64_t item = i0 + 16 * v + c;
    if (item >= p.n_items) continue;
    float* out = dI + item * lddi + 4 * g;
#pragma unroll
    for (int f = 0; f < D / 16; ++f)
      *reinterpret_cast<float4*>(out + 16 * f) = make_float4(di[v][f][0], di[v][f][1], di[v][f][2], di[v][f][3]);
  }
}

// ---- The same loss over a candidate list (sagnn_softmax_loss_cand_f32 / _bwd_f32) ------------------------------------
// Siblings of the kernels above over the POSITIONS [0, n_cand) of an ascending id list: the item row of position j is
// I[cand[j]], chunks and spans cut the positions, and an exclusion is matched by the global id. The target never
// enters through a candidate position: lse_row_cand_kernel merges its term once, dq_row_cand_kernel adds its gradient
// once. A position >= n_cand reads the last candidate's row and is never eligible.
struct CandProblem {
  Problem p;                                             // p.chunk / p.n_chunks cut [0, n_cand)
  const int32_t* cand;
  int64_t n_cand;
};

__device__ __forceinline__ int cand_id(const CandProblem& cp, int64_t pos) {
  return cp.cand[pos < cp.n_cand ? pos : cp.n_cand - 1];
}

// bit r: id[r] is on the list (the walk passes every entry up to `last`, the tile's last id)
__device__ __forceinline__ unsigned walk_bits_cand(const Problem& p, Walk& w, const int (&id)[4], int last) {
  unsigned xm = 0;
  while (w.ep < w.ee && w.nxt <= last) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (w.nxt == id[r]) xm |= 1u << r;
    if (++w.ep < w.ee) w.nxt = p.excl_items[w.ep];
  }
  return xm;
}

template <int D>
__global__ __launch_bounds__(64) void lse_chunk_cand_kernel(CandProblem cp, float2* __restrict__ part) {
  const Problem& p = cp.p;
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < cp.n_cand ? c0 + p.chunk : cp.n_cand;
  QueryLane<D> ql[kNT];
  float m[kNT], s[kNT];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, (int64_t)cp.cand[c0], g, ql[u]);
    m[u] = -INFINITY;
    s[u] = 0.f;
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    const int idq = cand_id(cp, s0 + q);
    float4 a[D / 16];
    load_frag<D>(p.I + (int64_t)idq * p.ldi, g, a);
    int id[4];                                           // the ids of the accumulator rows s0 + 4g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) id[r] = __shfl(idq, 4 * g + r);
    const int last = __shfl(idq, 15);
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = walk_bits_cand(p, ql[u].w, id, last);
      float z[4];
      bool e[4];
      float mx = m[u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = ql[u].ok && s0 + 4 * g + r < c1 && !((xm >> r) & 1) && id[r] != ql[u].ti;
        z[r] = acc[r] * p.inv_temp;
        if (e[r]) mx = fmaxf(mx, z[r]);
      }
      if (mx > -INFINITY) {
        float sum = s[u] * __expf(m[u] - mx);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e[r]) sum += __expf(z[r] - mx);
        s[u] = sum;
        m[u] = mx;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    lse_merge(m[u], s[u], __shfl_xor(m[u], 16), __shfl_xor(s[u], 16));
    lse_merge(m[u], s[u], __shfl_xor(m[u], 32), __shfl_xor(s[u], 32));
    if (ql[u].in && g == 0) part[ql[u].b * p.n_chunks + blockIdx.y] = make_float2(m[u], s[u]);
  }
}

// lse_row_kernel plus the target's own term, merged after the chunk partials
template <int D>
__global__ __launch_bounds__(64) void lse_row_cand_kernel(Problem p, const float2* __restrict__ part, float* __restrict__ lse,
                                                          float* __restrict__ tscore, float* __restrict__ terms) {
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int64_t b = blockIdx.x;
  const int32_t tv = p.target[b];
  const bool ok = tv >= 0 && (int64_t)tv < p.n_items;
  float m = -INFINITY, s = 0.f;
  for (int64_t j = lane; j < p.n_chunks; j += 64) {
    const float2 v = part[b * p.n_chunks + j];
    lse_merge(m, s, v.x, v.y);
  }
  for (int off = 1; off < 64; off <<= 1) lse_merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
  float4 a[D / 16], qf[D / 16];
  load_frag<D>(p.I + (int64_t)(ok ? tv : 0) * p.ldi, g, a);
  load_frag<D>(p.Q + b * p.ldq, g, qf);
  const f32x4 acc = tile_scores<D>(a, qf);
  if (lane == 0) {
    if (ok) lse_merge(m, s, acc[0] * p.inv_temp, 1.f);
    const float l = ok ? m + logf(s) : 0.f;
    const float ts = ok ? acc[0] : 0.f;
    lse[b] = l;
    tscore[b] = ts;
    terms[b] = ok ? l - ts * p.inv_temp : 0.f;
  }
}

template <int D>
__global__ __launch_bounds__(64) void dq_chunk_cand_kernel(CandProblem cp, const float* __restrict__ lse,
                                                           const float* __restrict__ gup, float* __restrict__ part) {
  const Problem& p = cp.p;
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < cp.n_cand ? c0 + p.chunk : cp.n_cand;
  const float coef = gup[0] * p.scale * p.inv_temp;
  QueryLane<D> ql[kNT];
  float row_lse[kNT];
  f32x4 dq[kNT][D / 16];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, (int64_t)cp.cand[c0], g, ql[u]);
    row_lse[u] = lse[ql[u].in ? ql[u].b : p.n_queries - 1];
#pragma unroll
    for (int f = 0; f < D / 16; ++f) dq[u][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    const int idq = cand_id(cp, s0 + q);
    float4 a[D / 16];
    load_frag<D>(p.I + (int64_t)idq * p.ldi, g, a);
    int id[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) id[r] = __shfl(idq, 4 * g + r);
    const int last = __shfl(idq, 15);
    f32x4 G[kNT];
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = walk_bits_cand(p, ql[u].w, id, last);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool e = ql[u].ok && s0 + 4 * g + r < c1 && !((xm >> r) & 1) && id[r] != ql[u].ti;
        G[u][r] = grad_elem(acc[r], p.inv_temp, row_lse[u], coef, e, false);
      }
    }
    // dQ^T += I^T G: MFMA r contracts over the items id[r]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = p.I + (int64_t)id[r] * p.ldi + q;
#pragma unroll
      for (int f = 0; f < D / 16; ++f) {
        const float av = row[16 * f];
#pragma unroll
        for (int u = 0; u < kNT; ++u) dq[u][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, G[u][r], dq[u][f], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    if (!ql[u].in) continue;
    float* out = part + ((int64_t)blockIdx.y * p.n_queries + ql[u].b) * D + 4 * g;
#pragma unroll
    for (int f = 0; f < D / 16; ++f)
      *reinterpret_cast<float4*>(out + 16 * f) = make_float4(dq[u][f][0], dq[u][f][1], dq[u][f][2], dq[u][f][3]);
  }
}

// One wavefront per query: dQ[b] = the chunk partials added in chunk order, then the target's g(b, t_b) I[t_b];
// dT[b] = g(b, t_b) Q[b]. The target's score is the forward's tile arithmetic.
template <int D>
__global__ __launch_bounds__(64) void dq_row_cand_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                         const float* __restrict__ part, float* __restrict__ dQ, int64_t lddq,
                                                         float* __restrict__ dT, int64_t lddt) {
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int64_t b = blockIdx.x;
  const int32_t tv = p.target[b];
  const bool ok = tv >= 0 && (int64_t)tv < p.n_items;
  const float* irow = p.I + (int64_t)(ok ? tv : 0) * p.ldi;
  const float* qrow = p.Q + b * p.ldq;
  float4 a[D / 16], qf[D / 16];
  load_frag<D>(irow, g, a);
  load_frag<D>(qrow, g, qf);
  const f32x4 acc = tile_scores<D>(a, qf);
  const float gt = ok ? grad_elem(acc[0], p.inv_temp, lse[b], gup[0] * p.scale * p.inv_temp, true, true) : 0.f;
  if (lane >= D / 4) return;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f), dt = sum;
  for (int64_t j = 0; j < p.n_chunks; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(part + (j * p.n_queries + b) * D + 4 * lane);
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  if (ok) {
    const float4 iv = *reinterpret_cast<const float4*>(irow + 4 * lane);
    const float4 qv = *reinterpret_cast<const float4*>(qrow + 4 * lane);
    sum.x += gt * iv.x; sum.y += gt * iv.y; sum.z += gt * iv.z; sum.w += gt * iv.w;
    dt = make_float4(gt * qv.x, gt * qv.y, gt * qv.z, gt * qv.w);
  }
  *reinterpret_cast<float4*>(dQ + b * lddq + 4 * lane) = sum;
  *reinterpret_cast<float4*>(dT + b * lddt + 4 * lane) = dt;
}

// di_kernel over 16 * NI candidate positions. The span's ids sit in LDS; lane l walks the list of query qg + l over
// [first id, last id] of the span and finds each entry among the ids by lower bound.
template <int D, int NI>
__global__ __launch_bounds__(64) void di_cand_kernel(CandProblem cp, const float* __restrict__ lse, const float* __restrict__ gup,
                                                     float* __restrict__ dIc, int64_t lddic) {
  const Problem& p = cp.p;
  __shared__ int sid[16 * NI];
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * (16 * NI);
  const int n_span = (int)(cp.n_cand - i0 < 16 * NI ? cp.n_cand - i0 : 16 * NI);
  const float coef = gup[0] * p.scale * p.inv_temp;
  if (lane < 16 * NI) sid[lane] = cand_id(cp, i0 + lane);
  __syncthreads();
  const int first = sid[0], last = sid[n_span - 1];
  int idv[NI];
  float4 ib[NI][D / 16];
  f32x4 di[NI][D / 16];
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    idv[v] = sid[16 * v + c];
    load_frag<D>(p.I + (int64_t)idv[v] * p.ldi, g, ib[v]);
#pragma unroll
    for (int f = 0; f < D / 16; ++f) di[v][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t qg = 0; qg < p.n_queries; qg += 64) {
    // lane l: the exclusions of query qg + l among the span's ids as a bit mask over the positions
    unsigned mask_lo = 0, mask_hi = 0;
    if (p.excl_ptr && qg + lane < p.n_queries) {
      int64_t lo, hi;
      excl_range(p, qg + lane, lo, hi);
      int64_t ep = excl_lower_bound(p.excl_items, lo, hi, first);
      while (ep < hi) {
        const int e = p.excl_items[ep];
        if (e > last) break;
        int x = 0, y = n_span;
        while (x < y) {
          const int mid = (x + y) >> 1;
          if (sid[mid] < e) x = mid + 1; else y = mid;
        }
        if (x < n_span && sid[x] == e) {
          if (x < 32) mask_lo |= 1u << x; else mask_hi |= 1u << (x - 32);
        }
        ++ep;
      }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int64_t qb = qg + 16 * j;
      if (qb >= p.n_queries) break;                      // uniform over the wavefront
      int64_t ra = qb + c;
      if (ra >= p.n_queries) ra = p.n_queries - 1;
      float4 qa[D / 16];
      load_frag<D>(p.Q + ra * p.ldq, g, qa);
      float row_lse[4];
      int ti[4];
      unsigned xl[4], xh[4];
      int64_t rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = qb + 4 * g + r;
        const bool in = b < p.n_queries;
        rq[r] = in ? b : p.n_queries - 1;
        const int32_t tv = p.target[rq[r]];
        ti[r] = (in && tv >= 0 && (int64_t)tv < p.n_items) ? tv : -1;
        row_lse[r] = lse[rq[r]];
        xl[r] = __shfl(mask_lo, 16 * j + 4 * g + r);
        xh[r] = __shfl(mask_hi, 16 * j + 4 * g + r);
      }
      f32x4 G[NI];
#pragma unroll
      for (int v = 0; v < NI; ++v) {
        const f32x4 acc = tile_scores<D>(qa, ib[v]);     // acc[r] = score(query qb + 4g + r, item idv[v])
        const int off = 16 * v + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = ti[r] >= 0 && off < n_span;
          const bool ex = ((off < 32 ? xl[r] >> off : xh[r] >> (off - 32)) & 1) != 0;
          G[v][r] = grad_elem(acc[r], p.inv_temp, row_lse[r], coef, ok && !ex && idv[v] != ti[r], false);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = p.Q + rq[r] * p.ldq + c;
#pragma unroll
        for (int f = 0; f < D / 16; ++f) {
          const float av = row[16 * f];
#pragma unroll
          for (int v = 0; v < NI; ++v) di[v][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, G[v][r], di[v][f], 0, 0, 0);
        }
      }
    }
  }
  // lane (g, c) holds features 16f + 4g .. + 3 of position i0 + 16v + c
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    if (16 * v + c >= n_span) continue;
    float* out = dIc + (i0 + 16 * v + c) * lddic + 4 * g;
#pragma unroll
    for (int f = 0; f < D / 16; ++f)
      *reinterpret_cast<float4*>(out + 16 * f) = make_float4(di[v][f][0], di[v][f][1], di[v][f][2], di[v][f][3]);
  }
}

// dI[t] += the dT rows of the queries whose target is t, in ascending query order, by the first such query: one
// wavefront per query. 64 lanes compare 64 targets at a time (a ballot); the owner then walks the set bits upwards, its
// first d / 4 lanes holding one float4 column each, so every dI element has one writer and the sum one order.
__global__ __launch_bounds__(64) void target_add_kernel(const float* __restrict__ dT, int64_t lddt,
                                                        const int32_t* __restrict__ target, int64_t n_queries,
                                                        int64_t n_items, int d, float* __restrict__ dI, int64_t lddi) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int32_t t = target[b];
  if (t < 0 || (int64_t)t >= n_items) return;            // uniform over the wavefront, as every branch below
  for (int64_t o0 = 0; o0 < b; o0 += 64) {
    const int64_t o = o0 + lane;
    if (__ballot(o < b && target[o] == t)) return;       // an earlier query owns the row
  }
  const bool col = lane < d / 4;
  float* out = dI + (int64_t)t * lddi + 4 * lane;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col) acc = *reinterpret_cast<const float4*>(out);
  for (int64_t o0 = b & ~(int64_t)63; o0 < n_queries; o0 += 64) {
    const int64_t o = o0 + lane;
    unsigned long long m = __ballot(o >= b && o < n_queries && target[o] == t);
    while (m) {
      const int k = __ffsll(m) - 1;
      m &= m - 1;
      if (col) {
        const float4 v = *reinterpret_cast<const float4*>(dT + (o0 + k) * lddt + 4 * lane);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  }
  if (col) *reinterpret_cast<float4*>(out) = acc;
}

// Workspace: forward = (max, sum) per (query, chunk) then one loss term per query; backward = dQ partials per chunk.
struct Layout {
  int64_t chunk, n_chunks;
  size_t terms_off, bytes;
};

inline Layout layout(int64_t n_queries, int64_t n_items, int d) {
  Layout L;
  L.chunk = chunk_items(n_items);
  L.n_chunks = (n_items + L.chunk - 1) / L.chunk;
  // sized by a bound on n_chunks that grows with n_items (n_chunks itself dips where the chunk size steps up)
  int64_t bound = (n_items + kMinChunk - 1) / kMinChunk;
  if (bound > kMaxChunks) bound = kMaxChunks;
  L.terms_off = ((size_t)n_queries * bound * sizeof(float2) + 255) & ~(size_t)255;
  const size_t fwd = L.terms_off + (((size_t)n_queries * sizeof(float) + 255) & ~(size_t)255);
  const size_t bwd = ((size_t)bound * n_queries * d * sizeof(float) + 255) & ~(size_t)255;
  L.bytes = fwd > bwd ? fwd : bwd;
  return L;
}

Problem problem(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries, int64_t n_items,
                const int32_t* target, float inv_temp, float scale, const int64_t* excl_ptr, const int32_t* excl_items,
                const int32_t* excl_row, int64_t n_lists, const Layout& L) {
  return Problem{Q, ldq, I, ldi, n_queries, n_items, target, inv_temp, scale, excl_ptr, excl_items, excl_row, n_lists,
                 L.chunk, L.n_chunks};
}

template <int D>
int launch_fwd(const Problem& p, const Layout& L, float* loss, float* lse, float* tscore, void* workspace, hipStream_t s) {
  float2* part = reinterpret_cast<float2*>(workspace);
  float* terms = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + L.terms_off);
  if (p.n_queries > 0) {
    const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
    hipLaunchKernelGGL(lse_chunk_kernel<D>, grid1, dim3(64), 0, s, p, part);
    SAGNN_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lse_row_kernel<D>, dim3((unsigned)p.n_queries), dim3(64), 0, s, p, part, lse, tscore, terms);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, terms, p.n_queries, p.scale, loss);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

template <int D>
int launch_bwd(const Problem& p, const Layout& L, const float* lse, const float* g, float* dQ, int64_t lddq, float* dI,
               int64_t lddi, void* workspace, hipStream_t s) {
  constexpr int NI = D == 128 ? 2 : 4;
  float* part = reinterpret_cast<float*>(workspace);
  if (p.n_queries > 0) {
    const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
    hipLaunchKernelGGL(dq_chunk_kernel<D>, grid1, dim3(64), 0, s, p, lse, g, part);
    SAGNN_HIP_TRY(hipGetLastError());
    const int64_t vecs = p.n_queries * (D / 4);
    hipLaunchKernelGGL(dq_merge_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, s, part, p.n_queries, D, L.n_chunks,
                       dQ, lddq);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  const int64_t spans = (p.n_items + 16 * NI - 1) / (16 * NI);
  hipLaunchKernelGGL((di_kernel<D, NI>), dim3((unsigned)spans), dim3(64), 0, s, p, lse, g, dI, lddi);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

template <int D>
int launch_cand_fwd(const CandProblem& cp, const Layout& L, float* loss, float* lse, float* tscore, void* workspace,
                    hipStream_t s) {
  const Problem& p = cp.p;
  float2* part = reinterpret_cast<float2*>(workspace);
  float* terms = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + L.terms_off);
  if (p.n_queries > 0) {
    if (L.n_chunks > 0) {
      const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
      hipLaunchKernelGGL(lse_chunk_cand_kernel<D>, grid1, dim3(64), 0, s, cp, part);
      SAGNN_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lse_row_cand_kernel<D>, dim3((unsigned)p.n_queries), dim3(64), 0, s, p, part, lse, tscore, terms);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, terms, p.n_queries, p.scale, loss);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

template <int D>
int launch_cand_bwd(const CandProblem& cp, const Layout& L, const float* lse, const float* g, float* dQ, int64_t lddq,
                    float* dIc, int64_t lddic, float* dT, int64_t lddt, void* workspace, hipStream_t s) {
  constexpr int NI = D == 128 ? 2 : 4;
  const Problem& p = cp.p;
  float* part = reinterpret_cast<float*>(workspace);
  if (p.n_queries > 0) {
    if (L.n_chunks > 0) {
      const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
      hipLaunchKernelGGL(dq_chunk_cand_kernel<D>, grid1, dim3(64), 0, s, cp, lse, g, part);
      SAGNN_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(dq_row_cand_kernel<D>, dim3((unsigned)p.n_queries), dim3(64), 0, s, p, lse, g, part, dQ, lddq, dT, lddt);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  if (cp.n_cand > 0) {
    // a short list at 16 positions per wavefront, so that it still fills the part; an item's sum over the queries has
    // the same order in both forms
    const int64_t spans = (cp.n_cand + 16 * NI - 1) / (16 * NI);
    if (spans < kSmallSpans)
      hipLaunchKernelGGL((di_cand_kernel<D, 1>), dim3((unsigned)((cp.n_cand + 15) / 16)), dim3(64), 0, s, cp, lse, g, dIc, lddic);
    else
      hipLaunchKernelGGL((di_cand_kernel<D, NI>), dim3((unsigned)spans), dim3(64), 0, s, cp, lse, g, dIc, lddic);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  return SAGNN_OK;
}

// The checks both entries share; `who` prefixes the message.
int check_common(const char* who, const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                 int64_t n_items, int d, const int32_t* target, float inv_temp, float scale, const int64_t* excl_ptr,
                 const int32_t* excl_items, const int32_t* excl_row, int64_t n_lists) {
  if (!Q || !I) return sagnn::fail(SAGNN_ERR_NULL, "%s: null Q or I", who);
  if (!target) return sagnn::fail(SAGNN_ERR_NULL, "%s: null target", who);
  if ((excl_ptr == nullptr) != (excl_items == nullptr))
    return sagnn::fail(SAGNN_ERR_NULL, "%s: excl_ptr and excl_items go together", who);
  if (excl_row && !excl_ptr) return sagnn::fail(SAGNN_ERR_NULL, "%s: excl_row without excl_ptr / excl_items", who);
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (n_queries < 0 || n_queries > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_queries = %lld", who, (long long)n_queries);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)n_items);
  if (!(inv_temp > 0.f) || !isfinite(inv_temp))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: inv_temp = %g, need a finite value > 0", who, (double)inv_temp);
  if (!isfinite(scale)) return sagnn::fail(SAGNN_ERR_ARG, "%s: scale = %g is not finite", who, (double)scale);
  if (excl_ptr && n_lists < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_lists = %lld", who, (long long)n_lists);
  if (excl_ptr && !excl_row && n_lists < n_queries)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: %lld exclusion lists for %lld rows and no excl_row", who, (long long)n_lists,
                       (long long)n_queries);
  if ((ldq & 3) || (ldi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides ldq / ldi must be multiples of 4", who);
  if (ldq < d || ldi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides ldq / ldi must be >= d", who);
  if (!sagnn::aligned16(Q) || !sagnn::aligned16(I))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: Q and I must be 16-byte aligned", who);
  return SAGNN_OK;
}

int check_workspace(const char* who, int64_t n_queries, int64_t n_items, int d, const void* workspace, size_t workspace_bytes) {
  const size_t need = sagnn_softmax_loss_workspace_bytes(n_queries, n_items, d);
  if (need == 0) return SAGNN_OK;
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  return SAGNN_OK;
}

int check_cand(const char* who, int64_t n_items, const int32_t* cand, int64_t n_cand) {
  if (n_cand < 0 || n_cand > n_items)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_cand = %lld, need 0 <= n_cand <= n_items = %lld", who, (long long)n_cand,
                       (long long)n_items);
  if (n_cand > 0 && !cand) return sagnn::fail(SAGNN_ERR_NULL, "%s: null cand", who);
  return SAGNN_OK;
}

int check_cand_workspace(const char* who, int64_t n_queries, int64_t n_cand, int d, const void* workspace,
                         size_t workspace_bytes) {
  const size_t need = sagnn_softmax_loss_cand_workspace_bytes(n_queries, n_cand, d);
  if (need == 0) return SAGNN_OK;
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  return SAGNN_OK;
}

}  // namespace

extern "C" size_t sagnn_softmax_loss_workspace_bytes(int64_t n_queries, int64_t n_items, int d) {
  if (n_queries < 0 || n_items <= 0 || d <= 0) return 0;
  return layout(n_queries, n_items, d).bytes;
}

extern "C" int sagnn_softmax_loss_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                                      int64_t n_items, int d, const int32_t* target, float inv_temp, float scale,
                                      const int64_t* excl_ptr, const int32_t* excl_items, const int32_t* excl_row,
                                      int64_t n_lists, float* loss, float* lse, float* tscore, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* who = "softmax_loss";
  if (int rc = check_common(who, Q, ldq, I, ldi, n_queries, n_items, d, target, inv_temp, scale, excl_ptr, excl_items,
                            excl_row, n_lists))
    return rc;
  if (!loss || !lse || !tscore) return sagnn::fail(SAGNN_ERR_NULL, "%s: null loss, lse or tscore", who);
  if (int rc = check_workspace(who, n_queries, n_items, d, workspace, workspace_bytes)) return rc;
  const Layout L = layout(n_queries, n_items, d);
  const Problem p = problem(Q, ldq, I, ldi, n_queries, n_items, target, inv_temp, scale, excl_ptr, excl_items, excl_row, n_lists, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSoftmaxLoss, s, n_queries, n_items);
  switch (d) {
    case 32: return launch_fwd<32>(p, L, loss, lse, tscore, workspace, s);
    case 64: return launch_fwd<64>(p, L, loss, lse, tscore, workspace, s);
    default: return launch_fwd<128>(p, L, loss, lse, tscore, workspace, s);
  }
}

extern "C" int sagnn_softmax_loss_bwd_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                                          int64_t n_items, int d, const int32_t* target, float inv_temp, float scale,
                                          const int64_t* excl_ptr, const int32_t* excl_items, const int32_t* excl_row,
                                          int64_t n_lists, const float* lse, const float* g, float* dQ, int64_t lddq,
                                          float* dI, int64_t lddi, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "softmax_loss_bwd";
  if (int rc = check_common(who, Q, ldq, I, ldi, n_queries, n_items, d, target, inv_temp, scale, excl_ptr, excl_items,
                            excl_row, n_lists))
    return rc;
  if (!lse || !g) return sagnn::fail(SAGNN_ERR_NULL, "%s: null lse or g", who);
  if (!dQ || !dI) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dQ or dI", who);
  if ((lddq & 3) || (lddi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddq / lddi must be multiples of 4", who);
  if (lddq < d || lddi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddq / lddi must be >= d", who);
  if (!sagnn::aligned16(dQ) || !sagnn::aligned16(dI))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dQ and dI must be 16-byte aligned", who);
  if (int rc = check_workspace(who, n_queries, n_items, d, workspace, workspace_bytes)) return rc;
  const Layout L = layout(n_queries, n_items, d);
  const Problem p = problem(Q, ldq, I, ldi, n_queries, n_items, target, inv_temp, scale, excl_ptr, excl_items, excl_row, n_lists, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSoftmaxLoss, s, n_queries, n_items);
  switch (d) {
    case 32: return launch_bwd<32>(p, L, lse, g, dQ, lddq, dI, lddi, workspace, s);
    case 64: return launch_bwd<64>(p, L, lse, g, dQ, lddq, dI, lddi, workspace, s);
    default: return launch_bwd<128>(p, L, lse, g, dQ, lddq, dI, lddi, workspace, s);
  }
}

extern "C" size_t sagnn_softmax_loss_cand_workspace_bytes(int64_t n_queries, int64_t n_cand, int d) {
  if (n_queries < 0 || n_cand < 0 || d <= 0) return 0;
  return layout(n_queries, n_cand, d).bytes;
}

extern "C" int sagnn_softmax_loss_cand_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                                           int64_t n_items, int d, const int32_t* cand, int64_t n_cand,
                                           const int32_t* target, float inv_temp, float scale, const int64_t* excl_ptr,
                                           const int32_t* excl_items, const int32_t* excl_row, int64_t n_lists, float* loss,
                                           float* lse, float* tscore, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "softmax_loss_cand";
  if (int rc = check_common(who, Q, ldq, I, ldi, n_queries, n_items, d, target, inv_temp, scale, excl_ptr, excl_items,
                            excl_row, n_lists))
    return rc;
  if (int rc = check_cand(who, n_items, cand, n_cand)) return rc;
  if (!loss || !lse || !tscore) return sagnn::fail(SAGNN_ERR_NULL, "%s: null loss, lse or tscore", who);
  if (int rc = check_cand_workspace(who, n_queries, n_cand, d, workspace, workspace_bytes)) return rc;
  const Layout L = layout(n_queries, n_cand, d);
  const CandProblem cp{problem(Q, ldq, I, ldi, n_queries, n_items, target, inv_temp, scale, excl_ptr, excl_items, excl_row,
                               n_lists, L), cand, n_cand};
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSoftmaxLossCand, s, n_queries, n_cand);
  switch (d) {
    case 32: return launch_cand_fwd<32>(cp, L, loss, lse, tscore, workspace, s);
    case 64: return launch_cand_fwd<64>(cp, L, loss, lse, tscore, workspace, s);
    default: return launch_cand_fwd<128>(cp, L, loss, lse, tscore, workspace, s);
  }
}

extern "C" int sagnn_softmax_loss_cand_bwd_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                                               int64_t n_items, int d, const int32_t* cand, int64_t n_cand,
                                               const int32_t* target, float inv_temp, float scale, const int64_t* excl_ptr,
                                               const int32_t* excl_items, const int32_t* excl_row, int64_t n_lists,
                                               const float* lse, const float* g, float* dQ, int64_t lddq, float* dIc,
                                               int64_t lddic, float* dT, int64_t lddt, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  const char* who = "softmax_loss_cand_bwd";
  if (int rc = check_common(who, Q, ldq, I, ldi, n_queries, n_items, d, target, inv_temp, scale, excl_ptr, excl_items,
                            excl_row, n_lists))
    return rc;
  if (int rc = check_cand(who, n_items, cand, n_cand)) return rc;
  if (!lse || !g) return sagnn::fail(SAGNN_ERR_NULL, "%s: null lse or g", who);
  if (!dQ || !dIc || !dT) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dQ, dIc or dT", who);
  if ((lddq & 3) || (lddic & 3) || (lddt & 3))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddq / lddic / lddt must be multiples of 4", who);
  if (lddq < d || lddic < d || lddt < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddq / lddic / lddt must be >= d", who);
  if (!sagnn::aligned16(dQ) || !sagnn::aligned16(dIc) || !sagnn::aligned16(dT))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dQ, dIc and dT must be 16-byte aligned", who);
  if (int rc = check_cand_workspace(who, n_queries, n_cand, d, workspace, workspace_bytes)) return rc;
  const Layout L = layout(n_queries, n_cand, d);
  const CandProblem cp{problem(Q, ldq, I, ldi, n_queries, n_items, target, inv_temp, scale, excl_ptr, excl_items, excl_row,
                               n_lists, L), cand, n_cand};
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSoftmaxLossCand, s, n_queries, n_cand);
  switch (d) {
    case 32: return launch_cand_bwd<32>(cp, L, lse, g, dQ, lddq, dIc, lddic, dT, lddt, workspace, s);
    case 64: return launch_cand_bwd<64>(cp, L, lse, g, dQ, lddq, dIc, lddic, dT, lddt, workspace, s);
    default: return launch_cand_bwd<128>(cp, L, lse, g, dQ, lddq, dIc, lddic, dT, lddt, workspace, s);
  }
}

extern "C" int sagnn_softmax_target_add_f32(const float* dT, int64_t lddt, const int32_t* target, int64_t n_queries,
                                            int64_t n_items, int d, float* dI, int64_t lddi, void* stream) {
  const char* who = "softmax_target_add";
  if (!dT || !target || !dI) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dT, target or dI", who);
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (n_queries < 0 || n_queries > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_queries = %lld", who, (long long)n_queries);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)n_items);
  if ((lddt & 3) || (lddi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddt / lddi must be multiples of 4", who);
  if (lddt < d || lddi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddt / lddi must be >= d", who);
  if (!sagnn::aligned16(dT) || !sagnn::aligned16(dI))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dT and dI must be 16-byte aligned", who);
  if (n_queries == 0) return SAGNN_OK;
  hipLaunchKernelGGL(target_add_kernel, dim3((unsigned)n_queries), dim3(64), 0, static_cast<hipStream_t>(stream), dT, lddt,
                     target, n_queries, n_items, d, dI, lddi);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
