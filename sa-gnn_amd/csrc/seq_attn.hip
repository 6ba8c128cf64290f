// Self-attention over the user's item sequence (--seqAtt full): the head's opt-in form in which every
// item of a batch slot's sequence is a token and the attention layers run over the slot's real tokens only.
// Activations live in a padded slab [n_slots * P, d] (token j of slot b at row b * P + j, P = pos_length) with the
// per-slot lengths on the device. Three kernels and their backwards: the token gather, the ragged attention on a
// q|k|v slab and the pooling sum, plus the opt-in additive-attention pooling (--seqPool additive, §21). Layer norm, the q|k|v projection and the weight gradients between them go through
// the row-wise entries of fusion.hip / dense.hip / attn_bwd_tail.hip on all n_slots * P rows; for that, padded rows
// hold finite values in every activation and exact zeros in every gradient written here.
// The attention also runs causally (--seqAtt causal: a CAUSAL template flag on its two kernels), and every prefix of a
// slot can be a query (--seqTargets all: the prefix-query and target kernels); DESIGN.md §26.
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
// CAUSAL (--seqAtt causal): query j sees keys 0..j only, so the trip counts differ per lane; the barrier
// stays ahead of every lane-dependent branch.
template <int DK, bool CAUSAL>
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
  const int keys = CAUSAL ? j + 1 : len;                 // j < len here
  const float m = row_max<DK>(q, Ks, keys);
  float z = 0.f;
  for (int s = 0; s < keys; ++s) {
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
// CAUSAL: pass 1 runs over the keys s <= j, pass 2 over the queries i = s .. len - 1 (the ones that see key s).
template <int DK, bool CAUSAL>
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
    const int keys = CAUSAL ? j + 1 : len;
    const float m = row_max<DK>(q, Ks, keys);
    float z = 0.f;
    for (int s = 0; s < keys; ++s) {
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
    for (int s = 0; s < keys; ++s) {
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
  for (int i = CAUSAL ? j : 0; i < len; ++i) {           // queries in ascending order
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

// ---- every prefix a query (--seqTargets all) --------------------------------------------------------
// Q[b, j] = leaky(pre[b, j]) + U[b], pre[b, j] = sum_{i <= j} x[b, i] (i ascending from 0.0f: seq_pool_kernel's sum,
// kept at every step), exact zeros in the padding. One thread per (slot, float4 column), walking j upwards.
__global__ void seq_prefix_query_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seg_len,
                                        const float* __restrict__ U, int64_t ldu, int64_t n_slots, int P, int d, float leaky,
                                        float* __restrict__ Q, int64_t ldq) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * lpr) return;
  const int64_t b = t / lpr;
  const int col = (int)(t - b * lpr) * 4;
  const int len = clamp_len(seg_len, b, P);
  const float4 u = *reinterpret_cast<const float4*>(U + b * ldu + col);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < len; ++j) {
    add4(acc, *reinterpret_cast<const float4*>(x + (b * P + j) * ldx + col));
    *reinterpret_cast<float4*>(Q + (b * P + j) * ldq + col) =
        make_float4(sagnn::leaky_addf(acc.x, u.x, leaky), sagnn::leaky_addf(acc.y, u.y, leaky),
                    sagnn::leaky_addf(acc.z, u.z, leaky), sagnn::leaky_addf(acc.w, u.w, leaky));
  }
  for (int j = len; j < P; ++j) *reinterpret_cast<float4*>(Q + (b * P + j) * ldq + col) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the slope of max(leaky * a, a) at a, as sagnn_leaky_f32's backward form takes it: the gradient goes to leaky * a on ties
__device__ __forceinline__ float leaky_slope(float a, float leaky) { return (a > leaky * a) ? 1.f : leaky; }

// dx[b, i] = sum_{j >= i} dQ[b, j] slope(pre[b, j]), dU[b] = sum_{j < n_b} dQ[b, j]. The same thread layout. Upwards:
// pre is rebuilt by the forward's own additions (never by subtraction, so every slope is the forward's), the term
// dQ slope goes to dx[b, j] and dU sums in ascending j. Downwards from n_b - 1: the running suffix sum replaces the
// terms, each read back by the thread that wrote it. One fixed order each, no atomics, zeros in the padding.
__global__ void seq_prefix_query_bwd_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seg_len,
                                            const float* __restrict__ dQ, int64_t lddq, int64_t n_slots, int P, int d,
                                            float leaky, float* __restrict__ dx, int64_t ld_dx, float* __restrict__ dU,
                                            int64_t ld_du) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * lpr) return;
  const int64_t b = t / lpr;
  const int col = (int)(t - b * lpr) * 4;
  const int len = clamp_len(seg_len, b, P);
  float4 pre = make_float4(0.f, 0.f, 0.f, 0.f), du = pre;
  for (int j = 0; j < len; ++j) {
    add4(pre, *reinterpret_cast<const float4*>(x + (b * P + j) * ldx + col));
    const float4 g = *reinterpret_cast<const float4*>(dQ + (b * P + j) * lddq + col);
    add4(du, g);
    *reinterpret_cast<float4*>(dx + (b * P + j) * ld_dx + col) =
        make_float4(g.x * leaky_slope(pre.x, leaky), g.y * leaky_slope(pre.y, leaky), g.z * leaky_slope(pre.z, leaky),
                    g.w * leaky_slope(pre.w, leaky));
  }
  *reinterpret_cast<float4*>(dU + b * ld_du + col) = du;
  float4 suf = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = len - 1; j >= 0; --j) {
    float4* o = reinterpret_cast<float4*>(dx + (b * P + j) * ld_dx + col);
    add4(suf, *o);
    *o = suf;
  }
  for (int j = len; j < P; ++j) *reinterpret_cast<float4*>(dx + (b * P + j) * ld_dx + col) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// target[b * P + j] = the item after token j of slot b (the slot's sampled positive after its last token), -1 in the
// padding, in a slot without a positive and for an id outside [0, n_items); excl_row = the slot's user. One thread per
// slab row.
__global__ void seq_targets_kernel(const int32_t* __restrict__ items, int64_t n_flat, const int64_t* __restrict__ seg_begin,
                                   const int32_t* __restrict__ seg_len, const int32_t* __restrict__ slot_user,
                                   const int32_t* __restrict__ slot_target, int64_t n_slots, int P, int64_t n_items,
                                   int32_t* __restrict__ target, int32_t* __restrict__ excl_row) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_slots * P) return;
  const int64_t b = row / P;
  const int j = (int)(row - b * P);
  const int len = clamp_len(seg_len, b, P);
  const int32_t last = slot_target[b];
  int64_t tgt = -1;
  if (j < len && last >= 0) {
    if (j == len - 1) {
      tgt = last;
    } else {
      const int64_t e = seg_begin[b] + j + 1;
      if (e >= 0 && e < n_flat) tgt = items[e];
    }
  }
  target[row] = (tgt >= 0 && tgt < n_items) ? (int32_t)tgt : -1;
  excl_row[row] = slot_user[b];
}

// ---- additive-attention pooling (--seqPool additive) ------------------------------------------------
// att_user[b] = sum_j w_j x_j, w = softmax over the slot's real tokens of s_j = <tanh(u_j), v>, u = x Wa + ba (the
// projection is a dense_nn over the slab). One workgroup per slot; every loop runs over n_b. Rows are read by
// sub-groups of G lanes (G the power of two >= row width / 4, a float4 per lane: whole rows, coalesced), 64 / G tokens
// per wave; sums across lanes are xor butterflies and sums across token groups go through LDS in ascending group
// order, so every reduction has one fixed order and the kernels have no atomics.
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ int lanes_for(int n4) {    // n4 <= 64
  int g = 1;
  while (g < n4) g <<= 1;
  return g;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ float4 tanh4(const float4& u) { return make_float4(tanhf(u.x), tanhf(u.y), tanhf(u.z), tanhf(u.w)); }

// S[j] = sum_c f(row_j[c]) * vec[c] for j < len: rows of n floats at `rows + j * ld`; f = tanh or the identity
template <bool TANH>
__device__ __forceinline__ void row_dots(const float* __restrict__ rows, int64_t ld, const float* __restrict__ vec, int n,
                                         int len, float* S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n4 = n >> 2, G = lanes_for(n4), per = 64 / G, sub = lane & (G - 1), tok = lane / G;
  const float4 vv = sub < n4 ? ld4(vec + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j0 = 0; j0 < len; j0 += kWaves * per) {       // a block-uniform trip count: every lane reaches the shuffles
    const int j = j0 + wave * per + tok;
    float p = 0.f;
    if (j < len && sub < n4) {
      float4 r = ld4(rows + j * ld + sub * 4);
      if (TANH) r = tanh4(r);
      p = fmaf(r.w, vv.w, fmaf(r.z, vv.z, fmaf(r.y, vv.y, r.x * vv.x)));
    }
    for (int off = G >> 1; off; off >>= 1) p += __shfl_xor(p, off);
    if (j < len && sub == 0) S[j] = p;
  }
}

// W[j] = softmax over j < len of S (the largest score subtracted), zeros for len <= j < P. Every wave evaluates the
// two reductions alike, so no wave waits for another's result. Ends with a barrier; S must be complete on entry.
__device__ __forceinline__ void slot_softmax(const float* S, int len, int P, float* W) {
  const int lane = threadIdx.x & 63;
  float m = -INFINITY, z = 0.f;
  for (int j = lane; j < len; j += 64) m = fmaxf(m, S[j]);
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  for (int j = lane; j < len; j += 64) z += expf(S[j] - m);
  for (int off = 32; off; off >>= 1) z += __shfl_xor(z, off);
  const int j = threadIdx.x;
  if (j < P) W[j] = j < len ? expf(S[j] - m) / z : 0.f;       // z >= 1: the largest score's term
  __syncthreads();
}

// partial sums of token groups, merged in ascending group order: thread t < n4 returns float4 column t of the sum
__device__ __forceinline__ float4 merge_groups(float4 acc, int n4, float4* Part) {
  __syncthreads();                                       // Part may still be read from an earlier merge
  Part[threadIdx.x] = acc;
  __syncthreads();
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (threadIdx.x < n4)
    for (int g = 0; g < kBlock / n4; ++g) add4(o, Part[g * n4 + threadIdx.x]);
  return o;
}

__global__ void __launch_bounds__(kBlock) seq_addpool_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u,
                                                             int64_t ldu, const float* __restrict__ v,
                                                             const int32_t* __restrict__ seg_len, int P, int d, int q,
                                                             float* __restrict__ out, int64_t ldo, float* __restrict__ w) {
  __shared__ float S[kMaxP], W[kMaxP];
  __shared__ __attribute__((aligned(16))) float4 Part[kBlock];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int len = clamp_len(seg_len, b, P);
  row_dots<true>(u + b * P * ldu, ldu, v, q, len, S);
  __syncthreads();
  slot_softmax(S, len, P, W);
  if (w && tid < P) w[b * P + tid] = W[tid];
  const int d4 = d >> 2, groups = kBlock / d4, col = tid % d4, grp = tid / d4;
  const float* xs = x + b * P * ldx + col * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (grp < groups)
    for (int j = grp; j < len; j += groups) {
      const float4 r = ld4(xs + j * ldx);
      const float wj = W[j];
      acc.x = fmaf(wj, r.x, acc.x);
      acc.y = fmaf(wj, r.y, acc.y);
      acc.z = fmaf(wj, r.z, acc.z);
      acc.w = fmaf(wj, r.w, acc.w);
    }
  const float4 o = merge_groups(acc, d4, Part);
  if (tid < d4) st4(out + b * ldo + tid * 4, o);
}

// Backward: t, s and w are recomputed from x and u. a_j = <g, x_j>, abar = sum_j w_j a_j, ds_j = w_j (a_j - abar);
// dx_j = w_j g (the direct part; du Wa^T is the caller's product), du_j = ds_j v (1 - t_j^2), dv_part[b] = sum_j ds_j t_j.
__global__ void __launch_bounds__(kBlock) seq_addpool_bwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ u, int64_t ldu,
                                                                 const float* __restrict__ v, const float* __restrict__ g,
                                                                 int64_t ldg, const int32_t* __restrict__ seg_len, int P, int d,
                                                                 int q, float* __restrict__ dx, int64_t ld_dx,
                                                                 float* __restrict__ du, int64_t ld_du,
                                                                 float* __restrict__ dv_part) {
  __shared__ float S[kMaxP], W[kMaxP], A[kMaxP], Ds[kMaxP];
  __shared__ __attribute__((aligned(16))) float4 Part[kBlock];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int len = clamp_len(seg_len, b, P);
  const float* us = u + b * P * ldu;
  const float* gb = g + b * ldg;
  row_dots<true>(us, ldu, v, q, len, S);
  row_dots<false>(x + b * P * ldx, ldx, gb, d, len, A);
  __syncthreads();
  slot_softmax(S, len, P, W);
  float abar = 0.f;
  for (int j = lane; j < len; j += 64) abar = fmaf(W[j], A[j], abar);
  for (int off = 32; off; off >>= 1) abar += __shfl_xor(abar, off);
  if (tid < P) Ds[tid] = tid < len ? W[tid] * (A[tid] - abar) : 0.f;
  __syncthreads();
  const int d4 = d >> 2, q4 = q >> 2;
  float* dxs = dx + b * P * ld_dx;
  for (int i = tid; i < P * d4; i += kBlock) {            // every row of dx: w_j g, zeros in the padding (W is 0 there)
    const int j = i / d4, c = (i - j * d4) * 4;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < len) {
      const float4 gg = ld4(gb + c);
      const float wj = W[j];
      r = make_float4(wj * gg.x, wj * gg.y, wj * gg.z, wj * gg.w);
    }
    st4(dxs + j * ld_dx + c, r);
  }
  float* dus = du + b * P * ld_du;
  const int groups = kBlock / q4, col = tid % q4, grp = tid / q4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (grp < groups) {
    const float4 vv = ld4(v + col * 4);
    for (int j = grp; j < len; j += groups) {
      const float4 t = tanh4(ld4(us + j * ldu + col * 4));
      const float ds = Ds[j];
      acc.x = fmaf(ds, t.x, acc.x);
      acc.y = fmaf(ds, t.y, acc.y);
      acc.z = fmaf(ds, t.z, acc.z);
      acc.w = fmaf(ds, t.w, acc.w);
      st4(dus + j * ld_du + col * 4, make_float4(ds * vv.x * (1.f - t.x * t.x), ds * vv.y * (1.f - t.y * t.y),
                                                 ds * vv.z * (1.f - t.z * t.z), ds * vv.w * (1.f - t.w * t.w)));
    }
  }
  for (int i = tid; i < (P - len) * q4; i += kBlock) {    // the padding of du
    const int j = len + i / q4, c = (i % q4) * 4;
    st4(dus + j * ld_du + c, make_float4(0.f, 0.f, 0.f, 0.f));
  }
  const float4 o = merge_groups(acc, q4, Part);
  if (tid < q4) st4(dv_part + b * q + tid * 4, o);
}

// dv[c] = sum over slots b (ascending) of dv_part[b, c]: one thread per column, no atomics
__global__ void seq_addpool_dv_kernel(const float* __restrict__ dv_part, int64_t n_slots, int q, float* __restrict__ dv) {
  const int c = threadIdx.x;
  if (c >= q) return;
  float acc = 0.f;
#pragma unroll 16
  for (int64_t b = 0; b < n_slots; ++b) acc += dv_part[b * q + c];
  dv[c] = acc;
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

namespace {

template <bool CAUSAL>
void launch_attn(int dk, dim3 grid, unsigned threads, hipStream_t s, const float* qkv, const int32_t* seg_len, int P, int d,
                 float* ctx) {
  switch (dk) {
    case 2: hipLaunchKernelGGL((seq_attn_kernel<2, CAUSAL>), grid, dim3(threads), 0, s, qkv, seg_len, P, d, ctx); break;
    case 4: hipLaunchKernelGGL((seq_attn_kernel<4, CAUSAL>), grid, dim3(threads), 0, s, qkv, seg_len, P, d, ctx); break;
    default: hipLaunchKernelGGL((seq_attn_kernel<8, CAUSAL>), grid, dim3(threads), 0, s, qkv, seg_len, P, d, ctx); break;
  }
}

template <bool CAUSAL>
void launch_attn_bwd(int dk, dim3 grid, unsigned threads, hipStream_t s, const float* qkv, const float* g,
                     const int32_t* seg_len, int P, int d, float* dqkv) {
  switch (dk) {
    case 2: hipLaunchKernelGGL((seq_attn_bwd_kernel<2, CAUSAL>), grid, dim3(threads), 0, s, qkv, g, seg_len, P, d, dqkv); break;
    case 4: hipLaunchKernelGGL((seq_attn_bwd_kernel<4, CAUSAL>), grid, dim3(threads), 0, s, qkv, g, seg_len, P, d, dqkv); break;
    default: hipLaunchKernelGGL((seq_attn_bwd_kernel<8, CAUSAL>), grid, dim3(threads), 0, s, qkv, g, seg_len, P, d, dqkv); break;
  }
}

int check_causal(const char* who, int causal) {
  if (causal != 0 && causal != 1) return sagnn::fail(SAGNN_ERR_ARG, "%s: causal = %d, need 0 or 1", who, causal);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_seq_attn_masked_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                                         int heads, int causal, float* ctx, void* stream) {
  const char* who = "seq_attn";
  if (!qkv || !seg_len || !ctx) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, seg_len, ctx)", who);
  if (int rc = check_causal(who, causal)) return rc;
  unsigned threads = 0;
  if (int rc = check_attn(who, d, heads, pos_length, n_slots, &threads)) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, qkv, "qkv")) return rc;
  if (int rc = check_rows(who, d, d, ctx, "ctx")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (causal)
    launch_attn<true>(d / heads, grid, threads, s, qkv, seg_len, pos_length, d, ctx);
  else
    launch_attn<false>(d / heads, grid, threads, s, qkv, seg_len, pos_length, d, ctx);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_attn_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                                  int heads, float* ctx, void* stream) {
  return sagnn_seq_attn_masked_f32(qkv, seg_len, n_slots, pos_length, d, heads, 0, ctx, stream);
}

extern "C" int sagnn_seq_attn_masked_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                             int pos_length, int d, int heads, int causal, float* dqkv, void* stream) {
  const char* who = "seq_attn_bwd";
  if (!qkv || !g_ctx || !seg_len || !dqkv) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, g_ctx, seg_len, dqkv)", who);
  if (int rc = check_causal(who, causal)) return rc;
  unsigned threads = 0;
  if (int rc = check_attn(who, d, heads, pos_length, n_slots, &threads)) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, qkv, "qkv")) return rc;
  if (int rc = check_rows(who, d, d, g_ctx, "g_ctx")) return rc;
  if (int rc = check_rows(who, 3 * d, 3 * (int64_t)d, dqkv, "dqkv")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (causal)
    launch_attn_bwd<true>(d / heads, grid, threads, s, qkv, g_ctx, seg_len, pos_length, d, dqkv);
  else
    launch_attn_bwd<false>(d / heads, grid, threads, s, qkv, g_ctx, seg_len, pos_length, d, dqkv);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_attn_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                      int pos_length, int d, int heads, float* dqkv, void* stream) {
  return sagnn_seq_attn_masked_bwd_f32(qkv, g_ctx, seg_len, n_slots, pos_length, d, heads, 0, dqkv, stream);
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

extern "C" int sagnn_seq_prefix_query_f32(const float* x, int64_t ldx, const int32_t* seg_len, const float* U, int64_t ldu,
                                          int64_t n_slots, int pos_length, int d, float leaky, float* Q, int64_t ldq,
                                          void* stream) {
  const char* who = "seq_prefix_query";
  if (!x || !seg_len || !U || !Q) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, seg_len, U, Q)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldx, x, "x")) return rc;
  if (int rc = check_rows(who, d, ldu, U, "U")) return rc;
  if (int rc = check_rows(who, d, ldq, Q, "Q")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_prefix_query_kernel, dim3(blocks), dim3(kBlock), 0, s, x, ldx, seg_len, U, ldu, n_slots, pos_length, d,
                     leaky, Q, ldq);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_prefix_query_bwd_f32(const float* x, int64_t ldx, const int32_t* seg_len, const float* dQ,
                                              int64_t lddq, int64_t n_slots, int pos_length, int d, float leaky, float* dx,
                                              int64_t ld_dx, float* dU, int64_t ld_du, void* stream) {
  const char* who = "seq_prefix_query_bwd";
  if (!x || !seg_len || !dQ || !dx || !dU) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, seg_len, dQ, dx, dU)", who);
  if (int rc = check_slab_dims(who, d, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldx, x, "x")) return rc;
  if (int rc = check_rows(who, d, lddq, dQ, "dQ")) return rc;
  if (int rc = check_rows(who, d, ld_dx, dx, "dx")) return rc;
  if (int rc = check_rows(who, d, ld_du, dU, "dU")) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_prefix_query_bwd_kernel, dim3(blocks), dim3(kBlock), 0, s, x, ldx, seg_len, dQ, lddq, n_slots,
                     pos_length, d, leaky, dx, ld_dx, dU, ld_du);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_targets_i32(const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin, const int32_t* seg_len,
                                     const int32_t* slot_user, const int32_t* slot_target, int64_t n_slots, int pos_length,
                                     int64_t n_items, int32_t* target, int32_t* excl_row, void* stream) {
  const char* who = "seq_targets";
  if (!seq_items || !seg_begin || !seg_len || !slot_user || !slot_target || !target || !excl_row)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (seq_items, seg_begin, seg_len, slot_user, slot_target, target, excl_row)",
                       who);
  if (pos_length < 1 || pos_length > kMaxP)
    return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, pos_length, kMaxP);
  if (n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)n_slots);
  if (int rc = check_tables(who, n_flat, n_items)) return rc;
  if (n_items >= ((int64_t)1 << 31)) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need < 2^31", who, (long long)n_items);
  unsigned blocks = 0;
  if (int rc = blocks_for(who, n_slots * pos_length, &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_targets_kernel, dim3(blocks), dim3(kBlock), 0, s, seq_items, n_flat, seg_begin, seg_len, slot_user,
                     slot_target, n_slots, pos_length, n_items, target, excl_row);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

namespace {

int addpool_shape(const char* who, int d, int q, int P) {
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a multiple of 4 in [4, 256]", who, d);
  if (q < 4 || q > 256 || (q & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: q = %d, need a multiple of 4 in [4, 256]", who, q);
  if (P < 1 || P > kMaxP) return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, P, kMaxP);
  return SAGNN_OK;
}

int check_addpool(const char* who, int d, int q, int P, int64_t n_slots) {
  if (int rc = addpool_shape(who, d, q, P)) return rc;
  if (n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)n_slots);
  if (n_slots > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: grid too large (%lld slots)", who, (long long)n_slots);
  return SAGNN_OK;
}

int check_vec16(const char* who, const void* p, const char* name) {
  if (!sagnn::aligned16(p)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned", who, name);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_seq_addpool_supported(int d, int q, int pos_length) {
  return addpool_shape("seq_addpool", d, q, pos_length);
}

extern "C" int sagnn_seq_addpool_f32(const float* x, int64_t ldx, const float* u, int64_t ldu, const float* v,
                                     const int32_t* seg_len, int64_t n_slots, int pos_length, int d, int q, float* out,
                                     int64_t ldo, float* w, void* stream) {
  const char* who = "seq_addpool";
  if (!x || !u || !v || !seg_len || !out) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, u, v, seg_len, out)", who);
  if (int rc = check_addpool(who, d, q, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldx, x, "x")) return rc;
  if (int rc = check_rows(who, q, ldu, u, "u")) return rc;
  if (int rc = check_rows(who, d, ldo, out, "out")) return rc;
  if (int rc = check_vec16(who, v, "v")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  hipLaunchKernelGGL(seq_addpool_kernel, dim3((unsigned)n_slots), dim3(kBlock), 0, s, x, ldx, u, ldu, v, seg_len, pos_length,
                     d, q, out, ldo, w);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_addpool_bwd_f32(const float* x, int64_t ldx, const float* u, int64_t ldu, const float* v,
                                         const float* g, int64_t ldg, const int32_t* seg_len, int64_t n_slots,
                                         int pos_length, int d, int q, float* dx, int64_t ld_dx, float* du, int64_t ld_du,
                                         float* dv_part, float* dv, void* stream) {
  const char* who = "seq_addpool_bwd";
  if (!x || !u || !v || !g || !seg_len || !dx || !du || !dv_part || !dv)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, u, v, g, seg_len, dx, du, dv_part, dv)", who);
  if (int rc = check_addpool(who, d, q, pos_length, n_slots)) return rc;
  if (int rc = check_rows(who, d, ldx, x, "x")) return rc;
  if (int rc = check_rows(who, q, ldu, u, "u")) return rc;
  if (int rc = check_rows(who, d, ldg, g, "g")) return rc;
  if (int rc = check_rows(who, d, ld_dx, dx, "dx")) return rc;
  if (int rc = check_rows(who, q, ld_du, du, "du")) return rc;
  if (int rc = check_vec16(who, v, "v")) return rc;
  if (int rc = check_vec16(who, dv_part, "dv_part")) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (n_slots)
    hipLaunchKernelGGL(seq_addpool_bwd_kernel, dim3((unsigned)n_slots), dim3(kBlock), 0, s, x, ldx, u, ldu, v, g, ldg, seg_len,
                       pos_length, d, q, dx, ld_dx, du, ld_du, dv_part);
  hipLaunchKernelGGL(seq_addpool_dv_kernel, dim3(1), dim3((unsigned)((q + 63) / 64 * 64)), 0, s, dv_part, n_slots, q, dv);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
