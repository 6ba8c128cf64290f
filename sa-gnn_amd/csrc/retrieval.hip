// Full-catalogue top-K retrieval (sagnn_score_topk_f32): s(b, i) = <Q[b], I[i]> on the exact-fp32 matrix cores,
// the best K eligible items of every query row in a strict total order, and the rank of an optional target item.
//
// Order: higher score first; equal scores go to the lower item id (-0.0 == +0.0); NaN is never eligible.
//
// Pass 1 (topk_chunk_kernel): one wavefront per (16 query rows, item chunk). Scores come from
// v_mfma_f32_16x16x4_f32 with the item rows as A (16 items x 4 k) and the query rows as B (4 k x 16 queries), so
// a lane holds 4 scores of ONE query (column lane & 15) for items 4 * (lane >> 4) + r of the tile. Every score is
// a fixed fmaf chain over k (the MFMA's numerics), so an item's score depends on the item and the query only.
// Per query the wave keeps a sorted top-K list in LDS and its K-th entry as a threshold in registers: most scores
// cost one compare. Scores that beat the threshold are appended to a per-query pending buffer; when a buffer may
// overflow, list + pending are merged by rank (index / binary search in the list + a count over pending). The
// chunk's list is written sorted to the workspace with the number of eligible items that beat the target.
// Pass 2 (topk_merge_kernel): one wavefront per query merges the chunk lists (K steps of a wave-wide arg-best
// over the list heads) and sums the integer rank counts.
// Chunk sizes depend on n_items only, and the merge is exact in the total order, so a row's output depends on that
// row's inputs only (not on n_queries, its position in the batch or the chunking).
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kQ = 16;            // query rows per wavefront (the MFMA's N)
constexpr int kStep = 32;         // items per step: two 16-item MFMA tiles
constexpr int kPend = 64;         // pending candidates per query between merges
constexpr int kMaxChunks = 1024;  // pass 2 keeps one head per chunk in LDS
constexpr int kSentinelId = INT_MAX;

struct Cand {
  float s;
  int i;
};

// a beats b in the total order (neither is NaN)
__device__ __forceinline__ bool beats(float as, int ai, float bs, int bi) {
  return as > bs || (as == bs && ai < bi);
}

// Scores of 16 items (row `it` of lane & 15, already clamped into the table) against the wave's 16 query rows.
// acc[r] = s(item of row 4 * (lane >> 4) + r, query lane & 15). Q fragment q[t] = Q[query lane & 15][16t + 4g .. +3].
template <int D>
__device__ __forceinline__ f32x4 tile_scores(const float* __restrict__ I, int64_t ldi, int64_t it, const float4 (&q)[D / 16],
                                             int g) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* row = I + it * ldi + 4 * g;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(row + 16 * t);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, q[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, q[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, q[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, q[t].w, acc, 0, 0, 0);
  }
  return acc;
}

// Workspace layout (shared by the host size function and the kernels).
struct Layout {
  int64_t chunk, n_chunks;
  size_t cand_off, cnt_off, bytes;
};

__host__ __device__ inline Layout layout(int64_t n_queries, int64_t n_items, int k) {
  Layout L;
  // chunks from n_items alone: ~256 of them on a large table, at least 512 items each (a multiple of kStep)
  int64_t c = (n_items + 255) / 256;
  if (c < 512) c = 512;
  const int64_t floor_c = (n_items + kMaxChunks - 1) / kMaxChunks;
  if (c < floor_c) c = floor_c;
  c = (c + kStep - 1) / kStep * kStep;
  L.chunk = c;
  L.n_chunks = (n_items + c - 1) / c;
  L.cand_off = 0;
  L.cnt_off = ((size_t)n_queries * L.n_chunks * k * sizeof(Cand) + 255) & ~(size_t)255;
  L.bytes = L.cnt_off + (size_t)n_queries * L.n_chunks * sizeof(int64_t);
  return L;
}

// Merges the pending candidates of every query into its sorted list (cur -> nxt), by rank. Lane (q, g) takes elements
// g, g + 4, ... of the list and of the pending buffer of query q. A list element's rank is its index plus the pending
// elements that beat it; a pending element's is the list elements that beat it (a prefix of the sorted list: binary
// search) plus the pending elements that beat it. Pending ids are distinct real items, so the ranks are a
// permutation (the sentinels at the list's tail keep their order) and ranks < k fill nxt exactly.
__device__ __forceinline__ void merge_pending(Cand* cur, Cand* nxt, Cand* pend, int* n_pend, int k, int q, int g) {
  __syncthreads();
  const int np = n_pend[q];
  const Cand* L = cur + q * k;
  const Cand* P = pend + q * kPend;
  for (int e = g; e < k; e += 4) {
    const Cand c = L[e];
    int rank = e;
    for (int f = 0; f < np && rank < k; ++f) rank += beats(P[f].s, P[f].i, c.s, c.i);
    if (rank < k) nxt[q * k + rank] = c;
  }
  for (int e = g; e < np; e += 4) {
    const Cand c = P[e];
    int lo = 0, hi = k;                        // list elements that beat c: [0, lo)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (beats(L[mid].s, L[mid].i, c.s, c.i)) lo = mid + 1; else hi = mid;
    }
    int rank = lo;
    for (int f = 0; f < np && rank < k; ++f) rank += beats(P[f].s, P[f].i, c.s, c.i);
    if (rank < k) nxt[q * k + rank] = c;
  }
  __syncthreads();
  if (g == 0) n_pend[q] = 0;
  __syncthreads();
}

template <int D>
__global__ __launch_bounds__(64) void topk_chunk_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ I,
                                                        int64_t ldi, int64_t n_queries, int64_t n_items, int k,
                                                        const int32_t* __restrict__ excl_rowptr,
                                                        const int32_t* __restrict__ excl_items,
                                                        const int32_t* __restrict__ target, Cand* __restrict__ cand_out,
                                                        int64_t* __restrict__ cnt_out, int64_t chunk, int64_t n_chunks) {
  extern __shared__ unsigned char smem[];
  Cand* bufA = reinterpret_cast<Cand*>(smem);
  Cand* bufB = bufA + kQ * k;
  Cand* pend = bufB + kQ * k;
  int* n_pend = reinterpret_cast<int*>(pend + kQ * kPend);
  float* tgt_s = reinterpret_cast<float*>(n_pend + kQ);

  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * kQ + q;        // query row of this lane
  const bool row_ok = b < n_queries;
  const int64_t bq = row_ok ? b : n_queries - 1;
  const int64_t c0 = (int64_t)blockIdx.y * chunk;
  const int64_t c1 = c0 + chunk < n_items ? c0 + chunk : n_items;

  float4 qf[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) qf[t] = *reinterpret_cast<const float4*>(Q + bq * ldq + 16 * t + 4 * g);

  for (int e = lane; e < kQ * k; e += 64) bufA[e] = Cand{-INFINITY, kSentinelId};
  if (lane < kQ) n_pend[lane] = 0;

  // target: its score from the same tile routine (row lane & 15 = the target of query lane & 15; the diagonal of the
  // tile is bit-identical to the score the item gets in its own chunk)
  int ti = -1;
  if (target) {
    const int32_t tv = target[bq];
    ti = (row_ok && tv >= 0 && (int64_t)tv < n_items) ? tv : -1;
    const f32x4 acc = tile_scores<D>(I, ldi, ti >= 0 ? ti : 0, qf, g);
    // lane (q, g) holds rows 4g .. 4g+3 of column q: the diagonal element sits at g == q >> 2, r == q & 3
    if (g == (q >> 2)) tgt_s[q] = acc[q & 3];
  }
  __syncthreads();
  const float ts = target ? tgt_s[q] : 0.f;
  const bool ts_nan = ts != ts;

  // exclusions of this lane's row at or after c0: lower bound, then a pointer walk as the chunk advances
  int64_t ep = 0, ee = 0;
  int nxt_ex = 0;                                        // excl_items[ep] while ep < ee
  if (excl_rowptr && row_ok) {
    int64_t lo = excl_rowptr[b], hi = excl_rowptr[b + 1];
    ee = hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)excl_items[mid] < c0) lo = mid + 1; else hi = mid;
    }
    ep = lo;
    if (ep < ee) nxt_ex = excl_items[ep];
  }

  Cand* cur = bufA;
  Cand* nxt = bufB;
  float thr_s = -INFINITY;
  int thr_i = kSentinelId;
  int64_t cnt = 0;                                       // eligible items of this lane that beat the target
  for (int64_t s0 = c0; s0 < c1; s0 += kStep) {
    int64_t it0 = s0 + q, it1 = s0 + 16 + q;             // A-operand rows of this lane for the two tiles
    if (it0 >= n_items) it0 = n_items - 1;
    if (it1 >= n_items) it1 = n_items - 1;
    const f32x4 a0 = tile_scores<D>(I, ldi, it0, qf, g);
    const f32x4 a1 = tile_scores<D>(I, ldi, it1, qf, g);
    // exclusion bits of this lane's 8 items (s0 + 16h + 4g + r -> bit 4h + r)
    unsigned xm = 0;
    while (ep < ee && (int64_t)nxt_ex < s0 + kStep) {
      const int64_t off = (int64_t)nxt_ex - s0;
      if (off >= 0 && ((off >> 2) & 3) == g) xm |= 1u << ((off >> 4) * 4 + (off & 3));
      if (++ep < ee) nxt_ex = excl_items[ep];
    }
    unsigned pass = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t item = s0 + 16 * h + 4 * g + r;
        const float s = h ? a1[r] : a0[r];
        const bool elig = item < c1 && (!((xm >> (4 * h + r)) & 1) || item == ti) && row_ok;
        if (elig && beats(s, (int)item, thr_s, thr_i)) pass |= 1u << (4 * h + r);
        if (target && elig && (ts_nan || (s == s && beats(s, (int)item, ts, ti)))) ++cnt;
      }
    }
    if (__any(pass != 0)) {
      for (int j = 0; j < 8; ++j) {
        if ((pass >> j) & 1) {
          const int pos = atomicAdd(&n_pend[q], 1);
          pend[q * kPend + pos] = Cand{(j >> 2) ? a1[j & 3] : a0[j & 3], (int)(s0 + 16 * (j >> 2) + 4 * g + (j & 3))};
        }
      }
      __syncthreads();
      if (__any(n_pend[q] > kPend - kStep)) {
        merge_pending(cur, nxt, pend, n_pend, k, q, g);
        Cand* tmp = cur; cur = nxt; nxt = tmp;
        const Cand w = cur[q * k + k - 1];
        thr_s = w.s;
        thr_i = w.i;
      }
    }
  }
  merge_pending(cur, nxt, pend, n_pend, k, q, g);
  cur = nxt;

  // the 4 lanes of a query hold partial counts
  cnt += __shfl_xor(cnt, 16);
  cnt += __shfl_xor(cnt, 32);
  if (!row_ok) return;
  const int64_t slot = b * n_chunks + blockIdx.y;
  for (int e = g; e < k; e += 4) cand_out[slot * k + e] = cur[q * k + e];
  if (g == 0) cnt_out[slot] = cnt;
}

// One wavefront per query: merges the n_chunks sorted lists (sentinel-padded) and sums the rank counts.
__global__ __launch_bounds__(64) void topk_merge_kernel(const Cand* __restrict__ cand, const int64_t* __restrict__ cnt,
                                                        int64_t n_chunks, int k, int64_t n_items,
                                                        const int32_t* __restrict__ target,
                                                        int32_t* __restrict__ items, float* __restrict__ scores,
                                                        int64_t* __restrict__ rank) {
  __shared__ int head[kMaxChunks];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const Cand* L = cand + b * n_chunks * k;
  for (int j = lane; j < n_chunks; j += 64) head[j] = 0;
  __syncthreads();
  // the best head among this lane's lists j = lane, lane + 64, ...
  auto local_best = [&](float& bs, int& bi, int& bj) {
    bs = -INFINITY; bi = kSentinelId; bj = INT_MAX;
    for (int j = lane; j < n_chunks; j += 64) {
      const int h = head[j];
      if (h >= k) continue;
      const Cand c = L[(int64_t)j * k + h];
      if (bj == INT_MAX || beats(c.s, c.i, bs, bi)) { bs = c.s; bi = c.i; bj = j; }
    }
  };
  float bs; int bi, bj;
  local_best(bs, bi, bj);
  for (int r = 0; r < k; ++r) {
    float ws = bs; int wi = bi, wj = bj;
    for (int off = 1; off < 64; off <<= 1) {
      const float os = __shfl_xor(ws, off);
      const int oi = __shfl_xor(wi, off), oj = __shfl_xor(wj, off);
      if (beats(os, oi, ws, wi) || (os == ws && oi == wi && oj < wj)) { ws = os; wi = oi; wj = oj; }
    }
    const bool real = wi != kSentinelId;
    if (lane == 0) {
      items[b * k + r] = real ? wi : -1;
      scores[b * k + r] = real ? ws : -INFINITY;
    }
    if (!real) continue;                     // every remaining head is a sentinel: the rest is padding
    if (wj != INT_MAX && (wj & 63) == lane) {
      ++head[wj];
      local_best(bs, bi, bj);
    }
  }
  if (rank) {
    int64_t s = 0;
    for (int j = lane; j < n_chunks; j += 64) s += cnt[b * n_chunks + j];
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
    const int32_t tv = target[b];
    if (lane == 0) rank[b] = (tv >= 0 && (int64_t)tv < n_items) ? s : -1;
  }
}

template <int D>
int launch(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries, int64_t n_items, int k,
           const int32_t* excl_rowptr, const int32_t* excl_items, const int32_t* target, int32_t* topk_items,
           float* topk_scores, int64_t* target_rank, void* workspace, hipStream_t s) {
  const Layout L = layout(n_queries, n_items, k);
  Cand* cand = reinterpret_cast<Cand*>(static_cast<unsigned char*>(workspace) + L.cand_off);
  int64_t* cnt = reinterpret_cast<int64_t*>(static_cast<unsigned char*>(workspace) + L.cnt_off);
  const size_t lds = (size_t)kQ * (2 * k + kPend) * sizeof(Cand) + kQ * sizeof(int) + kQ * sizeof(float);
  const dim3 grid1((unsigned)((n_queries + kQ - 1) / kQ), (unsigned)L.n_chunks);
  hipLaunchKernelGGL(topk_chunk_kernel<D>, grid1, dim3(64), lds, s, Q, ldq, I, ldi, n_queries, n_items, k, excl_rowptr,
                     excl_items, target, cand, cnt, L.chunk, L.n_chunks);
  SAGNN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_queries), dim3(64), 0, s, cand, cnt, L.n_chunks, k, n_items, target,
                     topk_items, topk_scores, target_rank);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

}  // namespace

extern "C" size_t sagnn_score_topk_workspace_bytes(int64_t n_queries, int64_t n_items, int d, int k) {
  (void)d;
  if (n_queries <= 0 || n_items <= 0 || k <= 0) return 0;
  return layout(n_queries, n_items, k).bytes;
}

extern "C" int sagnn_score_topk_f32(const float* Q, int64_t ldq, const float* I, int64_t ldi, int64_t n_queries,
                                    int64_t n_items, int d, int k, const int32_t* excl_rowptr,
                                    const int32_t* excl_items, const int32_t* target, int32_t* topk_items,
                                    float* topk_scores, int64_t* target_rank, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!Q || !I) return sagnn::fail(SAGNN_ERR_NULL, "score_topk: null Q or I");
  if (!topk_items || !topk_scores) return sagnn::fail(SAGNN_ERR_NULL, "score_topk: null topk_items or topk_scores");
  if ((excl_rowptr == nullptr) != (excl_items == nullptr))
    return sagnn::fail(SAGNN_ERR_NULL, "score_topk: excl_rowptr and excl_items go together");
  if ((target == nullptr) != (target_rank == nullptr))
    return sagnn::fail(SAGNN_ERR_NULL, "score_topk: target and target_rank go together");
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "score_topk: d = %d, need 32, 64 or 128", d);
  if (k < 1 || k > 128) return sagnn::fail(SAGNN_ERR_ARG, "score_topk: k = %d, need 1 <= k <= 128", k);
  if (n_queries < 0 || n_queries > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "score_topk: n_queries = %lld", (long long)n_queries);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "score_topk: n_items = %lld, need 1 <= n_items < 2^31", (long long)n_items);
  if ((ldq & 3) || (ldi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "score_topk: strides ldq / ldi must be multiples of 4");
  if (ldq < d || ldi < d) return sagnn::fail(SAGNN_ERR_ARG, "score_topk: strides ldq / ldi must be >= d");
  if (!sagnn::aligned16(Q) || !sagnn::aligned16(I))
    return sagnn::fail(SAGNN_ERR_ALIGN, "score_topk: Q and I must be 16-byte aligned");
  if (n_queries == 0) return SAGNN_OK;
  const size_t need = sagnn_score_topk_workspace_bytes(n_queries, n_items, d, k);
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "score_topk: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "score_topk: workspace must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (d) {
    case 32: return launch<32>(Q, ldq, I, ldi, n_queries, n_items, k, excl_rowptr, excl_items, target, topk_items, topk_scores, target_rank, workspace, s);
    case 64: return launch<64>(Q, ldq, I, ldi, n_queries, n_items, k, excl_rowptr, excl_items, target, topk_items, topk_scores, target_rank, workspace, s);
    default: return launch<128>(Q, ldq, I, ldi, n_queries, n_items, k, excl_rowptr, excl_items, target, topk_items, topk_scores, target_rank, workspace, s);
  }
}
