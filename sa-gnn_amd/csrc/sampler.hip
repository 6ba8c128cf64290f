// Device samplers of the training batch and the head's sequence sums over their segments (include/sagnn.h,
// "Device sampling of the training batch").
//
// Every draw is one Philox4x32-10 block: key = the 64-bit seed, counter = (user id, draw index, step, stream).
// A uniform integer on [0, n) is the high half of the 128-bit product ((w0 << 32) | w1) * n. A user's draws are
// therefore a pure function of (seed, step, user id): they depend neither on the other users of the batch nor on the
// user's slot in it, and no generator state or thread order is involved.
//
// These kernels move a few kilobytes per batch (512 slots x at most 40 draws): one thread per draw, no LDS.
#include "common.h"
#include "philox.h"

#include <limits.h>

namespace {

constexpr int kBlock = 256;

using sagnn::Word4;
using sagnn::philox4x32_10;

// uniform on [0, n), n >= 1; bias at most n / 2^64
__device__ __forceinline__ uint32_t draw(uint64_t seed, uint32_t user, uint32_t j, uint32_t step, uint32_t stream,
                                         uint32_t n) {
  const Word4 w = philox4x32_10(Word4{user, j, step, stream}, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint32_t)__umul64hi(((uint64_t)w.x << 32) | w.y, (uint64_t)n);
}

// One thread per (slot b, draw j). Thread j = 0 of a slot also writes the slot's sequence segment; every thread of a
// slot re-derives the slot's `choose` (stream 0, draw 0), so no thread waits for another.
__global__ void sample_train_kernel(const int32_t* __restrict__ bat, int64_t n_batch, int64_t n_slots, int draws,
                                    const int64_t* __restrict__ seq_ptr, const int32_t* __restrict__ seq_items,
                                    const int64_t* __restrict__ ban_ptr, const int32_t* __restrict__ ban,
                                    int64_t n_users, int64_t n_items, int tsn, int pred_num, int P,
                                    const int64_t* __restrict__ pair_off, int64_t n_pairs, uint64_t seed, uint32_t step,
                                    int32_t* __restrict__ uids, int32_t* __restrict__ iids, int32_t* __restrict__ locs,
                                    int64_t* __restrict__ seg_begin, int32_t* __restrict__ seg_len) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * draws) return;
  const int64_t b = t / draws;
  const int j = (int)(t - b * draws);
  const int64_t u = b < n_batch ? (int64_t)bat[b] : -1;
  if (u < 0 || u >= n_users) {              // padding slot (or an id outside the tables): an empty sequence
    if (j == 0) {
      seg_begin[b] = 0;
      seg_len[b] = 0;
    }
    return;
  }
  const int64_t s0 = seq_ptr[u];
  const int64_t n_pos = seq_ptr[u + 1] - s0 - 1;                       // len(sequence[u][:-1])
  const int64_t samp = max(min((int64_t)tsn, n_pos), (int64_t)0);
  const int64_t hi = max(min((int64_t)pred_num + 1, n_pos - 3), (int64_t)1);
  const int64_t choose = 1 + draw(seed, (uint32_t)u, 0, step, 0, (uint32_t)hi);
  const int64_t m = max(n_pos - choose, (int64_t)0);                    // len(posset[:-choose])
  if (j == 0) {
    const int64_t len = min(m, (int64_t)P);
    seg_begin[b] = s0 + m - len;
    seg_len[b] = (int32_t)len;
  }
  if (j >= samp) return;
  const int64_t off = pair_off[b] + j;
  if (off < 0 || off >= n_pairs) return;
  // the r-th item not in the sorted banned list: r + #{k : ban[k] - k <= r}
  const int64_t b0 = ban_ptr[u];
  const int64_t nb = ban_ptr[u + 1] - b0;
  int32_t neg = -1;
  if (n_items > nb) {
    const int64_t r = draw(seed, (uint32_t)u, (uint32_t)j, step, 1, (uint32_t)(n_items - nb));
    int64_t lo = 0, up = nb;
    while (lo < up) {
      const int64_t mid = (lo + up) >> 1;
      if ((int64_t)ban[b0 + mid] - mid <= r) lo = mid + 1;
      else up = mid;
    }
    neg = (int32_t)(r + lo);
  }
  uids[off] = uids[n_pairs + off] = (int32_t)u;
  iids[off] = seq_items[s0 + n_pos - choose];                          // posset[-choose]
  iids[n_pairs + off] = neg;
  locs[off] = locs[n_pairs + off] = (int32_t)b;
}

// One thread per (interval k, slot b, pair j); pair j of a slot goes to 2j and 2j + 1 of the slot's range.
__global__ void sample_ssl_kernel(const int32_t* __restrict__ bat, int64_t n_batch, int n_int,
                                  const int64_t* __restrict__ sub_ptr, const int32_t* __restrict__ sub_items,
                                  int64_t n_users, int ssl_num, const int64_t* __restrict__ ssl_off, int64_t n_out,
                                  uint64_t seed, uint32_t step, int32_t* __restrict__ uids, int32_t* __restrict__ iids,
                                  int32_t* __restrict__ locs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_int * n_batch * ssl_num) return;
  const int64_t kb = t / ssl_num;
  const int j = (int)(t - kb * ssl_num);
  const int k = (int)(kb / n_batch);
  const int64_t b = kb - (int64_t)k * n_batch;
  const int64_t u = bat[b];
  if (u < 0 || u >= n_users) return;
  const int64_t* ptr = sub_ptr + (int64_t)k * (n_users + 1);
  const int64_t a0 = ptr[u];
  const int64_t deg = ptr[u + 1] - a0;
  if (j >= min((int64_t)ssl_num, deg / 2)) return;
  const int64_t off = ssl_off[kb] + 2 * j;
  if (off < 0 || off + 1 >= n_out) return;
  const uint32_t stream = 2u + (uint32_t)k;
  iids[off] = sub_items[a0 + draw(seed, (uint32_t)u, 2u * j, step, stream, (uint32_t)deg)];
  iids[off + 1] = sub_items[a0 + draw(seed, (uint32_t)u, 2u * j + 1, step, stream, (uint32_t)deg)];
  uids[off] = uids[off + 1] = (int32_t)u;
  locs[off] = locs[off + 1] = (int32_t)b;
}

// cand[j] = lo_j + one uniform draw on [0, lo_{j+1} - lo_j), lo_j = floor(j * n_items / n_cand): one thread per
// candidate, stream word 0xFFFFFFFF (the batch samplers use 0, 1 and 2 + k). Ascending and distinct by construction.
__global__ void sample_strata_kernel(int64_t n_items, int64_t n_cand, uint64_t seed, uint32_t step,
                                     int32_t* __restrict__ cand) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cand) return;
  const int64_t lo = j * n_items / n_cand;
  const int64_t up = (j + 1) * n_items / n_cand;
  cand[j] = (int32_t)(lo + draw(seed, (uint32_t)j, 0, step, 0xFFFFFFFFu, (uint32_t)(up - lo)));
}

// The weighted draw (sagnn_sample_strata_w_i32) over the integer mass [0, W), W = cum[n_items - 1]: stratum j is
// [lo_j, lo_{j+1}), lo_j = j * (W / n_cand) + j * (W % n_cand) / n_cand, every product below 2^62.
__device__ __forceinline__ int64_t stratum_lo(int64_t j, int64_t q, int64_t rem, int64_t n_cand) {
  return j * q + j * rem / n_cand;
}

// cand[j] = #{i : cum[i] <= r_j}, r_j = lo_j + one uniform draw on [0, lo_{j+1} - lo_j) from the strata stream's block
// with counter word 1 set: one thread per candidate. r_j < W, so the count is below n_items for the cum of the
// contract; it is clamped there, so that a cum which breaks the contract still yields row addresses inside the table.
__global__ void sample_strata_w_kernel(const int64_t* __restrict__ cum, int64_t n_items, int64_t W, int64_t n_cand,
                                       uint64_t seed, uint32_t step, int32_t* __restrict__ cand) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cand) return;
  const int64_t q = W / n_cand, rem = W % n_cand;
  const int64_t lo = stratum_lo(j, q, rem, n_cand);
  const int64_t up = stratum_lo(j + 1, q, rem, n_cand);
  const Word4 w = philox4x32_10(Word4{(uint32_t)j, 1u, step, 0xFFFFFFFFu}, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int64_t r = lo + (int64_t)__umul64hi(((uint64_t)w.x << 32) | w.y, (uint64_t)(up - lo));
  int64_t a = 0, b = n_items;                                        // the first i with cum[i] > r
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (cum[mid] <= r) a = mid + 1;
    else b = mid;
  }
  cand[j] = (int32_t)min(a, n_items - 1);
}

// The runs of the drawn list and their offsets, one thread per position. The run of id c is [lb, ub): position lb is
// live, bias = ln(m) - ln(n_cand * w_c / W) with m = ub - lb and w_c = cum[c] - cum[c - 1], the logs in double and one
// rounding to float, exactly 0 when m * W == n_cand * w_c (compared as 128-bit products); the others are dead, -inf.
__global__ void strata_w_bias_kernel(const int64_t* __restrict__ cum, int64_t W, int64_t n_cand,
                                     const int32_t* __restrict__ cand, float* __restrict__ bias) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cand) return;
  const int32_t c = cand[j];
  if (j > 0 && cand[j - 1] == c) {
    bias[j] = -INFINITY;
    return;
  }
  int64_t a = j + 1, b = n_cand;                                     // ub: the first position past j with another id
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (cand[mid] <= c) a = mid + 1;
    else b = mid;
  }
  const uint64_t m = (uint64_t)(a - j);
  const uint64_t wc = (uint64_t)(cum[c] - (c > 0 ? cum[c - 1] : 0));
  const bool even = m * (uint64_t)W == (uint64_t)n_cand * wc && __umul64hi(m, (uint64_t)W) == __umul64hi((uint64_t)n_cand, wc);
  if (wc == 0) {                                                     // an item without mass is never drawn under the contract
    bias[j] = -INFINITY;
    return;
  }
  bias[j] = even ? 0.f : (float)(log((double)m) - log((double)n_cand * (double)wc / (double)W));
}

__device__ __forceinline__ void add4(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

__device__ __forceinline__ int clamp_len(const int32_t* seg_len, int64_t b, int P) { return min(max(seg_len[b], 0), P); }

// seq_tok[b] = sum_j fi[items[seg_begin[b] + j]], pos_tok[b] = sum of the last seg_len[b] position rows, both in
// ascending j from 0.0f: one thread per (slot, float4 column)
__global__ void seq_sum_kernel(const float* __restrict__ fi, int64_t ldf, int64_t n_items, const float* __restrict__ pe,
                               int64_t ldp, int P, const int32_t* __restrict__ items, int64_t n_flat,
                               const int64_t* __restrict__ seg_begin, const int32_t* __restrict__ seg_len, int64_t n_slots,
                               int d, float* __restrict__ seq_tok, float* __restrict__ pos_tok, int64_t ldo) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * lpr) return;
  const int64_t b = t / lpr;
  const int col = (int)(t - b * lpr) * 4;
  const int len = clamp_len(seg_len, b, P);
  const int64_t beg = seg_begin[b];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), p = s;
  for (int j = 0; j < len; ++j) {
    const int64_t e = beg + j;
    const int64_t it = (e >= 0 && e < n_flat) ? (int64_t)items[e] : -1;
    if (it >= 0 && it < n_items) add4(s, *reinterpret_cast<const float4*>(fi + it * ldf + col));
  }
  for (int q = P - len; q < P; ++q) add4(p, *reinterpret_cast<const float4*>(pe + (int64_t)q * ldp + col));
  *reinterpret_cast<float4*>(seq_tok + b * ldo + col) = s;
  *reinterpret_cast<float4*>(pos_tok + b * ldo + col) = p;
}

// d_fi[items[seg_begin[b] + j]] += g_seq[b]: one thread per (slot, j, float4 column), a wave's atomics on whole
// contiguous row segments
__global__ void seq_scatter_kernel(const float* __restrict__ g, int64_t ldg, const int32_t* __restrict__ items,
                                   int64_t n_flat, const int64_t* __restrict__ seg_begin,
                                   const int32_t* __restrict__ seg_len, int64_t n_slots, int P, int d,
                                   float* __restrict__ dfi, int64_t ld_dfi, int64_t n_items) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * P * lpr) return;
  const int64_t bj = t / lpr;
  const int col = (int)(t - bj * lpr) * 4;
  const int64_t b = bj / P;
  const int j = (int)(bj - b * P);
  if (j >= clamp_len(seg_len, b, P)) return;
  const int64_t e = seg_begin[b] + j;
  if (e < 0 || e >= n_flat) return;
  const int64_t it = items[e];
  if (it < 0 || it >= n_items) return;
  const float4 v = *reinterpret_cast<const float4*>(g + b * ldg + col);
  float* o = dfi + it * ld_dfi + col;
  atomicAdd(o + 0, v.x);
  atomicAdd(o + 1, v.y);
  atomicAdd(o + 2, v.z);
  atomicAdd(o + 3, v.w);
}

// d_pos[p] = sum over b (ascending) with seg_len[b] >= P - p of g_pos[b]: one thread per (position, float4 column),
// no atomics, so the result is the same in every run
__global__ void pos_grad_kernel(const float* __restrict__ g, int64_t ldg, const int32_t* __restrict__ seg_len,
                                int64_t n_slots, int P, int d, float* __restrict__ dpos, int64_t ld_dpos) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)P * lpr) return;
  const int p = (int)(t / lpr);
  const int col = (int)(t - (int64_t)p * lpr) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int64_t b = 0; b < n_slots; ++b) {
    if (clamp_len(seg_len, b, P) >= P - p) add4(acc, *reinterpret_cast<const float4*>(g + b * ldg + col));
  }
  *reinterpret_cast<float4*>(dpos + (int64_t)p * ld_dpos + col) = acc;
}

int blocks_for(int64_t threads, unsigned* out) {
  const int64_t n = (threads + kBlock - 1) / kBlock;
  if (n > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "sampler: %lld threads exceed one launch", (long long)threads);
  *out = (unsigned)n;
  return SAGNN_OK;
}

int check_rows(const char* who, int d, int64_t ld, const void* p, const char* name) {
  if ((ld & 3) || !sagnn::aligned16(p))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned with a stride that is a multiple of 4", who, name);
  if (ld < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: stride of %s = %lld < d = %d", who, name, (long long)ld, d);
  return SAGNN_OK;
}

int check_seq_dims(const char* who, int d, int P, int64_t n_slots, int64_t n_flat, int64_t n_items) {
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a multiple of 4 in [4, 256]", who, d);
  if (P <= 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: pos_length = %d, need > 0", who, P);
  if (n_slots < 0 || n_flat < 0)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld, n_flat = %lld)", who, (long long)n_slots,
                       (long long)n_flat);
  if (n_items <= 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need > 0", who, (long long)n_items);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_sample_train_i32(const int32_t* bat_ids, int64_t n_batch, int64_t n_slots, const int64_t* seq_ptr,
                                      const int32_t* seq_items, const int64_t* ban_ptr, const int32_t* ban_items,
                                      int64_t n_users, int64_t n_items, int train_sample_num, int pred_num,
                                      int pos_length, const int64_t* pair_off, int64_t n_pairs, uint64_t seed,
                                      int64_t step, int32_t* uids, int32_t* iids, int32_t* uLocs_seq,
                                      int64_t* seg_begin, int32_t* seg_len, void* stream) {
  if (!bat_ids || !seq_ptr || !seq_items || !ban_ptr || !ban_items || !pair_off)
    return sagnn::fail(SAGNN_ERR_NULL, "sample_train: null input (bat_ids, seq_ptr, seq_items, ban_ptr, ban_items, pair_off)");
  if (!uids || !iids || !uLocs_seq || !seg_begin || !seg_len)
    return sagnn::fail(SAGNN_ERR_NULL, "sample_train: null output (uids, iids, uLocs_seq, seg_begin, seg_len)");
  if (n_batch < 0 || n_slots < 0 || n_users < 0 || n_pairs < 0 || train_sample_num < 0 || pred_num < 0)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_train: negative count (n_batch %lld, n_slots %lld, n_users %lld, n_pairs %lld, "
                       "train_sample_num %d, pred_num %d)", (long long)n_batch, (long long)n_slots, (long long)n_users,
                       (long long)n_pairs, train_sample_num, pred_num);
  if (n_batch > n_slots)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_train: n_batch = %lld > n_slots = %lld", (long long)n_batch, (long long)n_slots);
  if (n_items <= 0 || n_items > INT32_MAX || n_users > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_train: n_items = %lld, n_users = %lld, need 0 < n_items < 2^31, n_users < 2^31",
                       (long long)n_items, (long long)n_users);
  if (pos_length <= 0) return sagnn::fail(SAGNN_ERR_ARG, "sample_train: pos_length = %d, need > 0", pos_length);
  if (step < 0 || step > (int64_t)UINT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_train: step = %lld, need 0 <= step < 2^32", (long long)step);
  const int draws = train_sample_num > 0 ? train_sample_num : 1;
  unsigned blocks = 0;
  if (int rc = blocks_for(n_slots * draws, &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(sample_train_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), bat_ids,
                     n_batch, n_slots, draws, seq_ptr, seq_items, ban_ptr, ban_items, n_users, n_items, train_sample_num,
                     pred_num, pos_length, pair_off, n_pairs, seed, (uint32_t)step, uids, iids, uLocs_seq, seg_begin,
                     seg_len);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_sample_ssl_i32(const int32_t* bat_ids, int64_t n_batch, int n_intervals, const int64_t* sub_ptr,
                                    const int32_t* sub_items, int64_t n_users, int ssl_num, const int64_t* ssl_off,
                                    int64_t n_out, uint64_t seed, int64_t step, int32_t* uids, int32_t* iids,
                                    int32_t* uLocs_seq, void* stream) {
  if (!bat_ids || !sub_ptr || !sub_items || !ssl_off)
    return sagnn::fail(SAGNN_ERR_NULL, "sample_ssl: null input (bat_ids, sub_ptr, sub_items, ssl_off)");
  if (!uids || !iids || !uLocs_seq) return sagnn::fail(SAGNN_ERR_NULL, "sample_ssl: null output (uids, iids, uLocs_seq)");
  if (n_batch < 0 || n_intervals < 0 || n_users < 0 || ssl_num < 0 || n_out < 0)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_ssl: negative count (n_batch %lld, n_intervals %d, n_users %lld, ssl_num %d, "
                       "n_out %lld)", (long long)n_batch, n_intervals, (long long)n_users, ssl_num, (long long)n_out);
  if (n_users > INT32_MAX || n_intervals > 65536)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_ssl: n_users = %lld, n_intervals = %d out of range", (long long)n_users,
                       n_intervals);
  if (step < 0 || step > (int64_t)UINT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_ssl: step = %lld, need 0 <= step < 2^32", (long long)step);
  unsigned blocks = 0;
  if (int rc = blocks_for((int64_t)n_intervals * n_batch * ssl_num, &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(sample_ssl_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), bat_ids,
                     n_batch, n_intervals, sub_ptr, sub_items, n_users, ssl_num, ssl_off, n_out, seed, (uint32_t)step,
                     uids, iids, uLocs_seq);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_sum_f32(const float* fi, int64_t ldf, int64_t n_items, const float* pos_embed, int64_t ldp,
                                 int pos_length, const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin,
                                 const int32_t* seg_len, int64_t n_slots, int d, float* seq_tok, float* pos_tok,
                                 int64_t ldo, void* stream) {
  if (!fi || !pos_embed || !seq_items || !seg_begin || !seg_len || !seq_tok || !pos_tok)
    return sagnn::fail(SAGNN_ERR_NULL, "seq_sum: null pointer (fi, pos_embed, seq_items, seg_begin, seg_len, seq_tok, pos_tok)");
  if (int rc = check_seq_dims("seq_sum", d, pos_length, n_slots, n_flat, n_items)) return rc;
  if (int rc = check_rows("seq_sum", d, ldf, fi, "fi")) return rc;
  if (int rc = check_rows("seq_sum", d, ldp, pos_embed, "pos_embed")) return rc;
  if (int rc = check_rows("seq_sum", d, ldo, seq_tok, "seq_tok")) return rc;
  if (int rc = check_rows("seq_sum", d, ldo, pos_tok, "pos_tok")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(n_slots * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(seq_sum_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), fi, ldf, n_items,
                     pos_embed, ldp, pos_length, seq_items, n_flat, seg_begin, seg_len, n_slots, d, seq_tok, pos_tok, ldo);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_sum_bwd_f32(const float* g_seq, const float* g_pos, int64_t ldg, const int32_t* seq_items,
                                     int64_t n_flat, const int64_t* seg_begin, const int32_t* seg_len, int64_t n_slots,
                                     int pos_length, int d, float* d_fi, int64_t ld_dfi, int64_t n_items, float* d_pos,
                                     int64_t ld_dpos, void* stream) {
  if (!g_seq || !g_pos || !seq_items || !seg_begin || !seg_len || !d_fi || !d_pos)
    return sagnn::fail(SAGNN_ERR_NULL, "seq_sum_bwd: null pointer (g_seq, g_pos, seq_items, seg_begin, seg_len, d_fi, d_pos)");
  if (int rc = check_seq_dims("seq_sum_bwd", d, pos_length, n_slots, n_flat, n_items)) return rc;
  if (int rc = check_rows("seq_sum_bwd", d, ldg, g_seq, "g_seq")) return rc;
  if (int rc = check_rows("seq_sum_bwd", d, ldg, g_pos, "g_pos")) return rc;
  if (int rc = check_rows("seq_sum_bwd", d, ld_dfi, d_fi, "d_fi")) return rc;
  if (int rc = check_rows("seq_sum_bwd", d, ld_dpos, d_pos, "d_pos")) return rc;
  unsigned b_scatter = 0, b_pos = 0;
  if (int rc = blocks_for(n_slots * pos_length * (d / 4), &b_scatter)) return rc;
  if (int rc = blocks_for((int64_t)pos_length * (d / 4), &b_pos)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b_scatter)
    hipLaunchKernelGGL(seq_scatter_kernel, dim3(b_scatter), dim3(kBlock), 0, s, g_seq, ldg, seq_items, n_flat, seg_begin,
                       seg_len, n_slots, pos_length, d, d_fi, ld_dfi, n_items);
  hipLaunchKernelGGL(pos_grad_kernel, dim3(b_pos), dim3(kBlock), 0, s, g_pos, ldg, seg_len, n_slots, pos_length, d, d_pos,
                     ld_dpos);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_sample_strata_i32(int64_t n_items, int64_t n_cand, uint64_t seed, uint32_t step, int32_t* cand,
                                       void* stream) {
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "sample_strata: n_items = %lld, need 1 <= n_items < 2^31", (long long)n_items);
  if (n_cand < 0 || n_cand > n_items)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_strata: n_cand = %lld, need 0 <= n_cand <= n_items = %lld", (long long)n_cand,
                       (long long)n_items);
  if (n_cand > 0 && !cand) return sagnn::fail(SAGNN_ERR_NULL, "sample_strata: null cand");
  unsigned blocks = 0;
  if (int rc = blocks_for(n_cand, &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(sample_strata_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), n_items, n_cand,
                     seed, step, cand);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_sample_strata_w_i32(const int64_t* cum, int64_t n_items, int64_t total, int64_t n_cand, uint64_t seed,
                                         uint32_t step, int32_t* cand, float* bias, void* stream) {
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "sample_strata_w: n_items = %lld, need 1 <= n_items < 2^31", (long long)n_items);
  if (total < 1 || total >= ((int64_t)1 << 62))
    return sagnn::fail(SAGNN_ERR_ARG, "sample_strata_w: total = %lld, need 1 <= total < 2^62", (long long)total);
  if (n_cand < 0 || n_cand >= ((int64_t)1 << 31) || n_cand > total)
    return sagnn::fail(SAGNN_ERR_ARG, "sample_strata_w: n_cand = %lld, need 0 <= n_cand <= total = %lld and n_cand < 2^31",
                       (long long)n_cand, (long long)total);
  if (!cum) return sagnn::fail(SAGNN_ERR_NULL, "sample_strata_w: null cum");
  if (n_cand > 0 && (!cand || !bias)) return sagnn::fail(SAGNN_ERR_NULL, "sample_strata_w: null cand or bias");
  unsigned blocks = 0;
  if (int rc = blocks_for(n_cand, &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sample_strata_w_kernel, dim3(blocks), dim3(kBlock), 0, s, cum, n_items, total, n_cand, seed, step, cand);
  SAGNN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(strata_w_bias_kernel, dim3(blocks), dim3(kBlock), 0, s, cum, total, n_cand, cand, bias);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
