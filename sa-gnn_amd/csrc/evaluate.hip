// Sampled-candidate evaluation (sagnn_candidate_rank_f32): the head score of every candidate of a query row and the
// rank of the row's target among them, under the rule Recommender.calcRes implements (reference model.py:484-510).
//
// One workgroup of 256 threads per row. The four wavefronts score the row's candidates with the lane layout of
// sagnn_pair_score_f32 (d / 4 lanes per candidate, pair_score.h), so every score is bit-identical to that entry's
// for (uids[b], cand[b, j], locs = b). The scores stay in LDS (C floats); then
//   p = the highest score over the target's copies (NaN read as -inf), f = the first copy with that score,
//   rank = #{j : s_j > p} + #{j < f : s_j == p},
// with a block-wide (p, f) arg-max and a block-wide count. Both reductions are exact, and a row reads only its own
// inputs, so its outputs depend neither on B nor on its position.
#include "common.h"
#include "pair_score.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kRankBlock = 256;
constexpr int kRankWaves = kRankBlock / 64;
constexpr int kMaxCandidates = 8192;   // 32 KB of LDS per workgroup

__device__ __forceinline__ float nan_low(float v) { return v != v ? -INFINITY : v; }

__global__ void __launch_bounds__(kRankBlock)
candidate_rank_kernel(const float* __restrict__ U, int64_t ldu, const float* __restrict__ I, int64_t ldi,
                      const float* __restrict__ S, int64_t lds_, const float* __restrict__ A, int64_t lda,
                      const int32_t* __restrict__ uids, const int32_t* __restrict__ cand, int64_t ldc,
                      const int32_t* __restrict__ target, float leaky, int C, int d, int64_t* __restrict__ rank,
                      float* __restrict__ scores, int64_t ld_scores) {
  extern __shared__ float sc[];                  // the row's C scores
  __shared__ float red_p[kRankWaves];
  __shared__ int red_f[kRankWaves];
  __shared__ int red_n[kRankWaves];
  const int64_t b = blockIdx.x;
  const int lpr = d >> 2, ppw = 64 / lpr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (lane % lpr) * 4;
  const int32_t* __restrict__ row = cand + b * ldc;
  const float* __restrict__ ur = U + (int64_t)uids[b] * ldu;
  const float* __restrict__ sr = S ? S + b * lds_ : nullptr;
  const int step = kRankWaves * ppw;
  for (int j0 = 0; j0 < C; j0 += step) {         // block-uniform trip count: every lane reaches the shuffles
    const int j = j0 + wave * ppw + lane / lpr;
    const float acc = sagnn::pair_score_lanes(
        j < C, S != nullptr,
        [&](const float*& u_, const float*& i_, const float*& s_, const float*& a_) {
          const int64_t it = row[j];
          u_ = ur;
          i_ = I + it * ldi;
          if (S) {
            s_ = sr;
            a_ = A + it * lda;
          }
        },
        leaky, col, lpr);
    if (j < C && (lane % lpr) == 0) {
      sc[j] = acc;
      if (scores) scores[b * ld_scores + j] = acc;
    }
  }
  __syncthreads();
  // (p, f): the best copy, the earliest among equal scores
  const int32_t t = target[b];
  float p = -INFINITY;
  int f = INT_MAX;
  for (int j = threadIdx.x; j < C; j += kRankBlock) {
    if (row[j] != t) continue;
    const float v = nan_low(sc[j]);
    if (v > p || (v == p && j < f)) {
      p = v;
      f = j;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float po = __shfl_xor(p, off);
    const int fo = __shfl_xor(f, off);
    if (po > p || (po == p && fo < f)) {
      p = po;
      f = fo;
    }
  }
  if (lane == 0) {
    red_p[wave] = p;
    red_f[wave] = f;
  }
  __syncthreads();
  p = red_p[0];
  f = red_f[0];
  for (int w = 1; w < kRankWaves; ++w)
    if (red_p[w] > p || (red_p[w] == p && red_f[w] < f)) {
      p = red_p[w];
      f = red_f[w];
    }
  if (t < 0 || f == INT_MAX) {                   // no copy of the target: a miss (block-uniform)
    if (threadIdx.x == 0) rank[b] = -1;
    return;
  }
  int n = 0;
  for (int j = threadIdx.x; j < C; j += kRankBlock) {
    const float v = nan_low(sc[j]);
    n += (v > p) || (v == p && j < f);
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
  if (lane == 0) red_n[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t total = 0;
    for (int w = 0; w < kRankWaves; ++w) total += red_n[w];
    rank[b] = total;
  }
}

}  // namespace

extern "C" int sagnn_candidate_rank_f32(const float* U, int64_t ldu, const float* I, int64_t ldi, const float* S,
                                        int64_t lds, const float* A, int64_t lda, const int32_t* uids,
                                        const int32_t* cand, int64_t ldc, const int32_t* target, float leaky,
                                        int64_t n_rows, int C, int d, int64_t* rank, float* scores, int64_t ld_scores,
                                        void* stream) {
  if (!U || !I || !uids || !cand || !target || !rank)
    return sagnn::fail(SAGNN_ERR_NULL, "candidate_rank: null U, I, uids, cand, target or rank");
  if ((S == nullptr) != (A == nullptr)) return sagnn::fail(SAGNN_ERR_NULL, "candidate_rank: S and A go together");
  const int lpr = d / 4;
  if (d < 4 || d > 256 || (d & 3) || (lpr & (lpr - 1)))
    return sagnn::fail(SAGNN_ERR_DIM, "candidate_rank: d = %d, need 4 * a power of two, <= 256", d);
  if (C < 1 || C > kMaxCandidates)
    return sagnn::fail(SAGNN_ERR_ARG, "candidate_rank: C = %d, need 1 <= C <= %d", C, kMaxCandidates);
  if (n_rows < 0 || n_rows > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "candidate_rank: n_rows = %lld", (long long)n_rows);
  if (ldc < C) return sagnn::fail(SAGNN_ERR_ARG, "candidate_rank: ldc = %lld < C = %d", (long long)ldc, C);
  if (scores && ld_scores < C)
    return sagnn::fail(SAGNN_ERR_ARG, "candidate_rank: ld_scores = %lld < C = %d", (long long)ld_scores, C);
  if ((ldu & 3) || (ldi & 3) || (S && ((lds & 3) || (lda & 3))))
    return sagnn::fail(SAGNN_ERR_ALIGN, "candidate_rank: strides ldu / ldi / lds / lda must be multiples of 4");
  if (ldu < d || ldi < d || (S && (lds < d || lda < d)))
    return sagnn::fail(SAGNN_ERR_ARG, "candidate_rank: strides ldu / ldi / lds / lda must be >= d");
  if (!sagnn::aligned16(U) || !sagnn::aligned16(I) || !sagnn::aligned16(S) || !sagnn::aligned16(A))
    return sagnn::fail(SAGNN_ERR_ALIGN, "candidate_rank: U, I, S and A must be 16-byte aligned");
  if (n_rows == 0) return SAGNN_OK;
  hipLaunchKernelGGL(candidate_rank_kernel, dim3((unsigned)n_rows), dim3(kRankBlock), (size_t)C * sizeof(float),
                     static_cast<hipStream_t>(stream), U, ldu, I, ldi, S, lds, A, lda, uids, cand, ldc, target, leaky, C,
                     d, rank, scores, ld_scores);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
