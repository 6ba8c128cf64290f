// Self-attention over the user's item sequence (--seqAtt full): the head's opt-in form in which every
// item of a batch slot's sequence is a token and the attention layers run over the slot's real tokens only.
// Activations live in a padded slab [n_slots * P, d] (token j of slot b at row b * P + j, P = pos_length) with the
// per-slot lengths on the device. Three kernels and their backwards: the token gather, the ragged attention on a
// q|k|v slab and the pooling sum. Layer norm, the q|k|v projection and the weight gradients between them go through
// the row-wise entries of fusion.hip / dense.hip / attn_bwd_tail.hip on all n_slots * P rows; for that, padded rows
// hold finite values in every activation and exact zeros in every gradient written here.
// Reference for the arithmetic: Utils/attention.py:35-45 with the attn_mask the reference never passes; fp32 VALU
// under every engine.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxP = 256;          // one thread per token of a slot: a workgroup holds the whole sequence
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ int clamp_len(const int32_t* seg_len, int64_t b, int P) { return min(max(seg_len[b], 0), P); }

__device__ __forceinline__ void add4(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// ---- gather: slab rows from fi / pos_embed, zeros in the padding ---------------------------------------------------
// one thread per (slot, token, float4 column)
__global__ void seq_gather_kernel(const float* __restrict__ fi, int64_t ldf, int64_t n_items, const float* __restrict__ pe,
                                  int64_t ldp, int P, const int32_t* __restrict__ items, int64_t n_flat,
                                  const int32_t* __restrict__ pos, const int64_t* __restrict__ seg_begin,
                                  const int32_t* __restrict__ seg_len, int64_t n_slots, int d, float* __restrict__ seq_slab,
                                  float* __restrict__ pos_slab, int64_t ldo) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * P * lpr) return;
  const int64_t row = t / lpr;
  const int col = (int)(t - row * lpr) * 4;
  const int64_t b = row / P;
  const int j = (int)(row - b * P);
  const int len = clamp_len(seg_len, b, P);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), p = s;
  if (j < len) {
    const int64_t e = seg_begin[b] + j;
    const bool in = e >= 0 && e < n_flat;
    const int64_t it = in ? (int64_t)items[e] : -1;
    if (it >= 0 && it < n_items) s = *reinterpret_cast<const float4*>(fi + it * ldf + col);
    const int q = pos ? (in ? pos[e] : -1) : P - len + j;
    if (q >= 0 && q < P) p = *reinterpret_cast<const float4*>(pe + (int64_t)q * ldp + col);
  }
  *reinterpret_cast<float4*>(seq_slab + row * ldo + col) = s;
  *reinterpret_cast<float4*>(pos_slab + row * ldo + col) = p;
}

// d_fi[items[seg_begin[b] + j]] += g_seq[b * P + j]: a wave's atomics on whole contiguous row segments
__global__ void seq_gather_scatter_kernel(const float* __restrict__ g, int64_t ldg, const int32_t* __restrict__ items,
                                          int64_t n_flat, const int64_t* __restrict__ seg_begin,
                                          const int32_t* __restrict__ seg_len, int64_t n_slots, int P, int d,
                                          float* __restrict__ dfi, int64_t ld_dfi, int64_t n_items) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * P * lpr) return;
  const int64_t row = t / lpr;
  const int col = (int)(t - row * lpr) * 4;
  const int64_t b = row / P;
  const int j = (int)(row - b * P);
  if (j >= clamp_len(seg_len, b, P)) return;
  const int64_t e = seg_begin[b] + j;
  if (e < 0 || e >= n_flat) return;
  const int64_t it = items[e];
  if (it < 0 || it >= n_items) return;
  const float4 v = *reinterpret_cast<const float4*>(g + row * ldg + col);
  float* o = dfi + it * ld_dfi + col;
  atomicAdd(o + 0, v.x);
  atomicAdd(o + 1, v.y);
  atomicAdd(o + 2, v.z);
  atomicAdd(o + 3, v.w);
}

// d_pos[p] = sum over slots b (ascending) of the token of b that sits at position p: one thread per (position, float4
// column), no atomics. Right-aligned (pos NULL): token j = p - (P - len). Explicit positions ascend strictly within a
// slot (a mask's do), so the token is found by bisection.
__global__ void seq_gather_pos_grad_kernel(const float* __restrict__ g, int64_t ldg, const int32_t* __restrict__ pos,
                                           int64_t n_flat, const int64_t* __restrict__ seg_begin,
                                           const int32_t* __restrict__ seg_len, int64_t n_slots, int P, int d,
                                           float* __restrict__ dpos, int64_t ld_dpos) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)P * lpr) return;
  const int p = (int)(t / lpr);
  const int col = (int)(t - (int64_t)p * lpr) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = 0; b < n_slots; ++b) {
    const int len = clamp_len(seg_len, b, P);
    int j = -1;
    if (!pos) {
      j = p - (P - len);
    } else {
      const int64_t beg = seg_begin[b];
      int lo = 0, hi = len;                       // first token whose position is >= p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int64_t e = beg + mid;
        const int q = (e >= 0 && e < n_flat) ? pos[e] : INT_MAX;
        if (q < p) lo = mid + 1; else hi = mid;
      }
      const int64_t e = beg + lo;
      if (lo < len && e >= 0 && e < n_flat && pos[e] == p) j = lo;
    }
    if (j >= 0 && j < len) add4(acc, *reinterpret_cast<const float4*>(g + (b * P + j) * ldg + col));
  }
  *reinterpret_cast<float4*>(dpos + (int64_t)p * ld_dpos + col) = acc;
}

// ---- ragged attention on the q|k|v slab ---------------------------------------------------------------------------
// The largest folded score of a query's row. The kernels evaluate a = e / (sum e + 1e-8) as
// e' / (sum e' + 1e-8 * 2^-m) with e' = e * 2^-m: the same quotient, term by term, but no e' exceeds 1, so scores
// that trained weights push past fp32's exp range (88) neither overflow nor turn a into inf / inf. A row whose scores
// are all below -126 gets 2^-m = inf and a = 0, the limit of the quotient.
template <int DK>
__device__ __forceinline__ float row_max(const float (&q)[DK], const float* __restrict__ Ks, int len) {
  float m = -INFINITY;
  for (int s = 0; s < len; ++s) {
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < DK; ++c) dot = fmaf(q[c], Ks[s * DK + c], dot);
    m = fmaxf(m, dot);
  }
  return m;
}

// One workgroup per (slot, head), one query per thread. The head's K and V columns of the slot's real tokens sit in
// LDS (every lane reads the same key: broadcast reads); q, the row sum and ctx stay in registers. e = exp2 of the
// score with log2(e) / sqrt(d_k) folded into q; the contract has no max subtraction (Utils/attention.py:38-39) and
// the shift by the row's largest score (row_max) leaves its quotient what it is.
template <int DK>
__global__ void __launch_bounds__(kBlock) seq_attn_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ seg_len,
                                                          int P, int d, float* __restrict__ ctx) {
  __shared__ __attribute__((aligned(16))) float Ks[kMaxP * DK];
  __shared__ __attribute__((aligned(16))) float Vs[kMaxP * DK];
  const int64_t b = blockIdx.x;
  const int h = blockIdx.y, j = threadIdx.x;
  const int len = clamp_len(seg_len, b, P);
  const int64_t ld = 3 * (int64_t)d;
  const int hc = h * DK;
  const float* row = qkv + (b * P + j) * ld + hc;       // dereferenced for j < len <= P only
  if (j < len) {
#pragma unroll
    for (int c = 0; c < DK; ++c) {
      Ks[j * DK + c] = row[d + c];
      Vs[j * DK + c] = row[2 * d + c];
    }
  }
  __syncthreads();
  if (j >= P) return;
  float* out = ctx + (b * P + j) * (int64_t)d + hc;
  if (j >= len) {
#pragma unroll
    for (int c = 0; c < DK; ++c) out[c] = 0.f;
    return;
  }
  const float fold = kLog2e * rsqrtf((float)DK);
  float q[DK], acc[DK];
#pragma unroll
  for (int c = 0; c < DK; ++c) {
    q[c] = row[c] * fold;
    acc[c] = 0.f;
  }
  const float m = row_max<DK>(q, Ks, len);
  float z = 0.f;
  for (int s = 0; s < len; ++s) {
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < DK; ++c) dot = fmaf(q[c], Ks[s * DK + c], dot);
    const float e = exp2f(dot - m);
    z += e;
#pragma unroll
    for (int c = 0; c < DK; ++c) acc[c] = fmaf(e, Vs[s * DK + c], acc[c]);
  }
  const float rz = 1.f / (z + 1e-8f * exp2f(-m));
#pragma unroll
  for (int c = 0; c < DK; ++c) out[c] = acc[c] * rz;
}

// Backward: e is recomputed from q|k|v (neither a nor Z is stored). With rz_j = 1 / (Z_j + 1e-8), a = e rz,
// D_j = <g_j, ctx_j> and p_js = a_js (<g_j, v_s> - D_j):
//   dq_j = sum_s p_js k_s / sqrt(d_k),  dk_s = sum_j p_js q_j / sqrt(d_k),  dv_s = sum_j a_js g_j.
// Pass 1, a thread per query: Z_j and ctx_j, then dq_j; the folded q, g, rz, D and the row's shift go to LDS. Pass 2, a thread per
// key: dk_s and dv_s over the queries in ascending j. No atomics: the same bits in every run.
template <int DK>
__global__ void __launch_bounds__(kBlock) seq_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ g,
                                                              const int32_t* __restrict__ seg_len, int P, int d,
                                                              float* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) float Ks[kMaxP * DK];
  __shared__ __attribute__((aligned(16))) float Vs[kMaxP * DK];
  __shared__ __attribute__((aligned(16))) float Qs[kMaxP * DK];   // q * log2(e) / sqrt(d_k)
  __shared__ __attribute__((aligned(16))) float Gs[kMaxP * DK];
  __shared__ float Rz[kMaxP], Ds[kMaxP], Ms[kMaxP];   // per query: 1 / (Z' + 1e-8 2^-m), D, the row's shift m
  const int64_t b = blockIdx.x;
  const int h = blockIdx.y, j = threadIdx.x;
  const int len = clamp_len(seg_len, b, P);
  const int64_t ld = 3 * (int64_t)d;
  const int hc = h * DK;
  const float* row = qkv + (b * P + j) * ld + hc;       // dereferenced for j < len <= P only
  float* drow = dqkv + (b * P + j) * ld + hc;           // written for j < P only
  const float scale = rsqrtf((float)DK);
  float k[DK], v[DK];
  if (j < len) {
    const float* grow = g + (b * P + j) * (int64_t)d + hc;
#pragma unroll
    for (int c = 0; c < DK; ++c) {
      k[c] = row[d + c];
      v[c] = row[2 * d + c];
      Ks[j * DK + c] = k[c];
      Vs[j * DK + c] = v[c];
      Qs[j * DK + c] = row[c] * (kLog2e * scale);
      Gs[j * DK + c] = grow[c];
    }
  }
  __syncthreads();
  if (j < len) {
    float q[DK], gj[DK], acc[DK];
#pragma unroll
    for (int c = 0; c < DK; ++c) {
      q[c] = Qs[j * DK + c];
      gj[c] = Gs[j * DK + c];
      acc[c] = 0.f;
    }
    const float m = row_max<DK>(q, Ks, len);
    float z = 0.f;
    for (int s = 0; s < len; ++s) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < DK; ++c) dot = fmaf(q[c], Ks[s * DK + c], dot);
      const float e = exp2f(dot - m);
      z += e;
#pragma unroll
      for (int c = 0; c < DK; ++c) acc[c] = fmaf(e, Vs[s * DK + c], acc[c]);
    }
    const float rz = 1.f / (z + 1e-8f * exp2f(-m));
    float D = 0.f;
#pragma unroll
    for (int c = 0; c < DK; ++c) D = fmaf(gj[c], acc[c] * rz, D);
    float dq[DK];
#pragma unroll
    for (int c = 0; c < DK; ++c) dq[c] = 0.f;
    for (int s = 0; s < len; ++s) {
      float dot = 0.f, gv = 0.f;
#pragma unroll
      for (int c = 0; c < DK; ++c) {
        dot = fmaf(q[c], Ks[s * DK + c], dot);
        gv = fmaf(gj[c], Vs[s * DK + c], gv);
      }
      const float p = exp2f(dot - m) * rz * (gv - D);
#pragma unroll
      for (int c = 0; c < DK; ++c) dq[c] = fmaf(p, Ks[s * DK + c], dq[c]);
    }
#pragma unroll
    for (int c = 0; c < DK; ++c) drow[c] = dq[c] * scale;
    Rz[j] = rz;
    Ds[j] = D;
    Ms[j] = m;
  }
  __syncthreads();
  if (j >= P) return;
  if (j >= len) {
#pragma unroll
    for (int c = 0; c < DK; ++c) drow[c] = drow[d + c] = drow[2 * d + c] = 0.f;
    return;
  }
  float dk[DK], dv[DK];
#pragma unroll
  for (int c = 0; c < DK; ++c) dk[c] = dv[c] = 0.f;
  for (int i = 0; i < len; ++i) {                        // queries in ascending order
    float dot = 0.f, gv = 0.f;
#pragma unroll
    for (int c = 0; c < DK; ++c) {
      dot = fmaf(Qs[i * DK + c], k[c], dot);
      gv = fmaf(Gs[i * DK + c], v[c], gv);
    }
    const float a = exp2f(dot - Ms[i]) * Rz[i];
    const float p = a * (gv - Ds[i]);
#pragma unroll
    for (int c = 0; c < DK; ++c) {
      dk[c] = fmaf(p, Qs[i * DK + c], dk[c]);
      dv[c] = fmaf(a, Gs[i * DK + c], dv[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < DK; ++c) {
    drow[d + c] = dk[c] * kLn2;                          // Qs carries log2(e) / sqrt(d_k): times ln 2 leaves 1 / sqrt(d_k)
    drow[2 * d + c] = dv[c];
  }
}

// ---- pooling: the sum over a slot's real tokens, and its broadcast -------------------------------------------------
__global__ void seq_pool_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seg_len,
                                int64_t n_slots, int P, int d, float* __restrict__ out, int64_t ldo) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * lpr) return;
  const int64_t b = t / lpr;
  const int col = (int)(t - b * lpr) * 4;
  const int len = clamp_len(seg_len, b, P);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < len; ++j) add4(acc, *reinterpret_cast<const float4*>(x + (b * P + j) * ldx + col));
  *reinterpret_cast<float4*>(out + b * ldo + col) = acc;
}

__global__ void seq_pool_bwd_kernel(const float* __restrict__ g, int64_t ldg, const int32_t* __restrict__ seg_len,
                                    int64_t n_slots, int P, int d, float* __restrict__ dx, int64_t ldx) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * P * lpr) return;
  const int64_t row = t / lpr;
  const int col = (int)(t - row * lpr) * 4;
  const int64_t b = row / P;
  const int j = (int)(row - b * P);
  const float4 v = j < clamp_len(seg_len, b, P) ? *reinterpret_cast<const float4*>(g + b * ldg + col)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
  *reinterpret_cast<float4*>(dx + row * ldx + col) = v;
}

// ---- host-side argument checks: every entry rejects a bad call before any device work ------------------------------
int check_slab_dims(const char* who, int d, int P, int64_t n_slots) {
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a multiple of 4 in [4, 256]", who, d);
  if (P < 1 || P > kMaxP) return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, P, kMaxP);
  if (n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)n_slots);
  return SAGNN_OK;
}

int check_rows(const char* who, int d, int64_t ld, const void* p, const char* name) {
  if ((ld & 3) || !sagnn::aligned16(p))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned with a stride that is a multiple of 4", who, name);
  if (ld < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: stride of %s = %lld < d = %d", who, name, (long long)ld, d);
  return SAGNN_OK;
}

int check_tables(const char* who, int64_t n_flat, int64_t n_items) {
  if (n_flat < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_flat = %lld)", who, (long long)n_flat);
  if (n_items <= 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need > 0", who, (long long)n_items);
  return SAGNN_OK;
}

int blocks_for(const char* who, int64_t threads, unsigned* out) {
  const int64_t n = (threads + kBlock - 1) / kBlock;
  if (n > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: %lld threads exceed one launch", who, (long long)threads);
  *out = (unsigned)n;
  return SAGNN_OK;
}

int attn_shape(const char* who, int d, int heads, int P) {
  if (d < 4 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a positive multiple of 4", who, d);
  if (heads < 1 || d % heads) return sagnn::fail(SAGNN_ERR_DIM, "%s: heads = %d does not divide d = %d", who, heads, d);
  const int dk = d / heads;
  if (dk != 2 && dk != 4 && dk != 8)
    return sagnn::fail(SAGNN_ERR_DIM, "%s: d / heads = %d, need 2, 4 or 8", who, dk);
  if (P < 1 || P > kMaxP) return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, P, kMaxP);
  return SAGNN_OK;
}

int check_attn(const char* who, int d, int heads, int P, int64_t n_slots, unsigned* threads) {
  if (int rc = attn_shape(who, d, heads, P)) return rc;
  if (n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)n_slots);
  if (n_slots > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: grid too large (%lld slots)", who, (long long)n_slots);
  *threads = (unsigned)((P + 63) / 64 * 64);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_seq_attn_supported(int d, int heads, int pos_length) {
  return attn_shape("seq_attn", d, heads, pos_length);
}

extern "C" int sagnn_seq_gather_f32(const float* fi, int64_t ldf, int64_t n_items, const float* pos_embed, int64_t ldp,
                                    int pos_length, const int32_t* seq_items, int64_t n_flat, const int32_t* seq_pos,
                                    const int64_t* seg_begin, const int32_t* seg_len, int64_t n_slots, int d,
                                    float* seq_slab, float* pos_slab, int64_t ldo, void* stream) {
  const char* who = "seq_gather";
  if (!fi || !pos_embed || !seq_items || !seg_begin || !seg_len || !seq_slab || !pos_slab)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (fi, pos_embed, seq_items, seg_begin, seg_len, seq_slab, pos_slab)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_tables(who, n_flat, n_items)) return rc;
  if (int rc = check_rows(who, d, ldf, fi, "fi")) return rc;
  if (int rc = check_rows(who, d, ldp, pos_embed, "pos_embed")) return rc;
  if (int rc = check_rows(who, d, ldo, seq_slab, "seq_slab")) return rc;
  if (int rc = check_rows(who, d, ldo, pos_slab, "pos_slab")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * pos_length * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_gather_kernel, dim3(blocks), dim3(kBlock), 0, s, fi, ldf, n_items, pos_embed, ldp, pos_length,
                     seq_items, n_flat, seq_pos, seg_begin, seg_len, n_slots, d, seq_slab, pos_slab, ldo);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_gather_bwd_f32(const float* g_seq, const float* g_pos, int64_t ldg, const int32_t* seq_items,
                                        int64_t n_flat, const int32_t* seq_pos, const int64_t* seg_begin,
                                        const int32_t* seg_len, int64_t n_slots, int pos_length, int d, float* d_fi,
                                        int64_t ld_dfi, int64_t n_items, float* d_pos, int64_t ld_dpos, void* stream) {
  const char* who = "seq_gather_bwd";
  if (!g_seq || !g_pos || !seq_items || !seg_begin || !seg_len || !d_fi || !d_pos)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (g_seq, g_pos, seq_items, seg_begin, seg_len, d_fi, d_pos)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_tables(who, n_flat, n_items)) return rc;
  if (int rc = check_rows(who, d, ldg, g_seq, "g_seq")) return rc;
  if (int rc = check_rows(who, d, ldg, g_pos, "g_pos")) return rc;
  if (int rc = check_rows(who, d, ld_dfi, d_fi, "d_fi")) return rc;
  if (int rc = check_rows(who, d, ld_dpos, d_pos, "d_pos")) return rc;
  unsigned b_scatter = 0, b_pos = 0;
  if (int rc = blocks_for(who, n_slots * pos_length * (d / 4), &b_scatter)) return rc;
  if (int rc = blocks_for(who, (int64_t)pos_length * (d / 4), &b_pos)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (b_scatter)
    hipLaunchKernelGGL(seq_gather_scatter_kernel, dim3(b_scatter), dim3(kBlock), 0, s, g_seq, ldg, seq_items, n_flat,
                       seg_begin, seg_len, n_slots, pos_length, d, d_fi, ld_dfi, n_items);
  hipLaunchKernelGGL(seq_gather_pos_grad_kernel, dim3(b_pos), dim3(kBlock), 0, s, g_pos, ldg, seq_pos, n_flat, seg_begin,
                     seg_len, n_slots, pos_length, d, d_pos, ld_dpos);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_attn_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                                  int heads, float* ctx, void* stream) {
  const char* who = "seq_attn";
  if (!qkv || !seg_len || !ctx) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, seg_len, ctx)", who);
  unsigned threads = 0;
  if (int rc = check_attn(who, d, heads, pos_length, n_slots, &threads)) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, qkv, "qkv")) return rc;
  if (int rc = check_rows(who, d, d, ctx, "ctx")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  switch (d / heads) {
    case 2: hipLaunchKernelGGL(seq_attn_kernel<2>, grid, dim3(threads), 0, s, qkv, seg_len, pos_length, d, ctx); break;
    case 4: hipLaunchKernelGGL(seq_attn_kernel<4>, grid, dim3(threads), 0, s, qkv, seg_len, pos_length, d, ctx); break;
    default: hipLaunchKernelGGL(seq_attn_kernel<8>, grid, dim3(threads), 0, s, qkv, seg_len, pos_length, d, ctx); break;
  }
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_attn_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                      int pos_length, int d, int heads, float* dqkv, void* stream) {
  const char* who = "seq_attn_bwd";
  if (!qkv || !g_ctx || !seg_len || !dqkv) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, g_ctx, seg_len, dqkv)", who);
  unsigned threads = 0;
  if (int rc = check_attn(who, d, heads, pos_length, n_slots, &threads)) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, qkv, "qkv")) return rc;
  if (int rc = check_rows(who, d, d, g_ctx, "g_ctx")) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, dqkv, "dqkv")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  switch (d / heads) {
    case 2: hipLaunchKernelGGL(seq_attn_bwd_kernel<2>, grid, dim3(threads), 0, s, qkv, g_ctx, seg_len, pos_length, d, dqkv); break;
    case 4: hipLaunchKernelGGL(seq_attn_bwd_kernel<4>, grid, dim3(threads), 0, s, qkv, g_ctx, seg_len, pos_length, d, dqkv); break;
    default: hipLaunchKernelGGL(seq_attn_bwd_kernel<8>, grid, dim3(threads), 0, s, qkv, g_ctx, seg_len, pos_length, d, dqkv); break;
  }
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_pool_f32(const float* x, int64_t ldx, const int32_t* seg_len, int64_t n_slots, int pos_length,
                                  int d, float* out, int64_t ldo, void* stream) {
  const char* who = "seq_pool";
  if (!x || !seg_len || !out) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, seg_len, out)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldx, x, "x")) return rc;
  if (int rc = check_rows(who, d, ldo, out, "out")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_pool_kernel, dim3(blocks), dim3(kBlock), 0, s, x, ldx, seg_len, n_slots, pos_length, d, out, ldo);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_pool_bwd_f32(const float* g, int64_t ldg, const int32_t* seg_len, int64_t n_slots, int pos_length,
                                      int d, float* dx, int64_t ldx, void* stream) {
  const char* who = "seq_pool_bwd";
  if (!g || !seg_len || !dx) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (g, seg_len, dx)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldg, g, "g")) return rc;
  if (int rc = check_rows(who, d, ldx, dx, "dx")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * pos_length * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_pool_bwd_kernel, dim3(blocks), dim3(kBlock), 0, s, g, ldg, seg_len, n_slots, pos_length, d, dx, ldx);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
