// Position-wise feed-forward block of the sequence head (--seqFFN), on the slab layout of seq_attn.hip:
//   z = LN(x_j), a = z W1 + b1, h = act(a), out = x_j + h W2 + b2     for every real token row j of every slot,
// exact zeros in the padding. Ragged: only real tokens are read and computed; every product is a chain of
// v_mfma_f32_16x16x4_f32 (exact fp32, the same under every engine); no atomics, so every output has the same bits in
// every run.
// Forward and the backward's data path: a persistent grid, W1 [d, F] and W2 [F, d] staged once per workgroup into LDS
// at row strides of F + 4 and d + 4 floats. The work unit is a tile of 16 tokens of one slot, a wave strides over the
// n_slots * ceil(P / 16) units and only zero-fills those at or beyond n_b. A lane (g = lane >> 4, q = lane & 15) holds
// columns 16t + 4g .. + 3 of token q: the layer-norm moments are a sum over its own values and the 4 lanes that share q.
// a^T = W1^T z^T is computed with the hidden units on the accumulator rows (seq_attn_wide.hip's transposition), so the
// 4 accumulator values of a lane, hidden units 16f + 4g + r of token q, are already the B operand of out^T = W2^T h^T
// when the MFMA's k index g is dealt to hidden unit 16f + 4g + r at step r: h never leaves registers, and out^T lands in
// the layout x was loaded in. The backward's dh^T = W2 g^T and dz^T = W1 da^T use the same deal with the weights read
// along their rows (one 16-byte LDS read per 4 steps).
// The weight gradients (dW1 = z^T da, dW2 = h^T g, db1, db2) take the token as the MFMA's k index: a workgroup stages a
// tile's z, da, h and g row-major in LDS, keeps its whole dW1 and dW2 in accumulators over all its tiles (the four waves
// own disjoint 16 x 16 output tiles) and writes one partial; a last launch sums the partials in one fixed order.
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxP = 256;
constexpr int kMaxF = 256;
constexpr int kMaxDF = 16384;             // d * F: both weight matrices stay resident in LDS
constexpr int kCUs = 256;                 // grids are sized for the MI355X's compute units, as a function of the shape only
constexpr size_t kLdsPerCU = 160 * 1024;

__device__ __forceinline__ int clamp_len(const int32_t* seg_len, int64_t b, int P) { return min(max(seg_len[b], 0), P); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// the sum over the 4 lanes that share lane & 15, in one order for all four
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}
// the sum over the 16 lanes that share lane >> 4, in one order for all sixteen
__device__ __forceinline__ float row_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v + __shfl_xor(v, 8);
}

__device__ __forceinline__ f32x4 mfma4(const float4& a, const float4& b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

struct Shape {
  int64_t n_slots;
  int P, F;
  float eps, leaky;
};

// W1 [D, F] -> LDS at a row stride of F + 4, W2 [F, D] -> at D + 4, b1 [F] behind them
template <int D>
__device__ __forceinline__ void stage_weights(const float* __restrict__ W1, const float* __restrict__ W2,
                                              const float* __restrict__ b1, int F, float* W1s, float* W2s, float* b1s) {
  const int f4 = F / 4;
  for (int i = threadIdx.x; i < D * f4; i += kBlock) {
    const int r = i / f4, c = (i - r * f4) * 4;
    st4(W1s + r * (F + 4) + c, ld4(W1 + r * F + c));
  }
  constexpr int d4 = D / 4;
  for (int i = threadIdx.x; i < F * d4; i += kBlock) {
    const int r = i / d4, c = (i - r * d4) * 4;
    st4(W2s + r * (D + 4) + c, ld4(W2 + r * D + c));
  }
  for (int i = threadIdx.x; i < f4; i += kBlock) st4(b1s + 4 * i, ld4(b1 + 4 * i));
}

// a lane's columns 16t + 4g .. + 3 of a [D] vector
template <int D>
__device__ __forceinline__ void vec_frag(const float* __restrict__ v, int g, float4 (&f)[D / 16]) {
#pragma unroll
  for (int t = 0; t < D / 16; ++t) f[t] = ld4(v + 16 * t + 4 * g);
}

// a lane's fragment of one row (row points at column 4g); zeros when the row is padding, which is not read
template <int D>
__device__ __forceinline__ void load_frag(const float* __restrict__ row, bool ok, float4 (&f)[D / 16]) {
#pragma unroll
  for (int t = 0; t < D / 16; ++t) f[t] = ok ? ld4(row + 16 * t) : zero4();
}

// layer norm of the token whose columns the 4 lanes sharing lane & 15 hold: xh = (x - mean) * rstd in place of x, and
// z = xh * gamma + beta; returns rstd
template <int D>
__device__ __forceinline__ float layer_norm(float4 (&x)[D / 16], const float4 (&gam)[D / 16], const float4 (&bet)[D / 16],
                                            float eps, float4 (&z)[D / 16]) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) s += sum4(x[t]);
  const float mean = group_sum(s) * (1.f / D);
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    x[t] = make_float4(x[t].x - mean, x[t].y - mean, x[t].z - mean, x[t].w - mean);
    v += (x[t].x * x[t].x + x[t].y * x[t].y) + (x[t].z * x[t].z + x[t].w * x[t].w);
  }
  const float rstd = rsqrtf(group_sum(v) * (1.f / D) + eps);
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    x[t] = make_float4(x[t].x * rstd, x[t].y * rstd, x[t].z * rstd, x[t].w * rstd);
    z[t] = make_float4(fmaf(x[t].x, gam[t].x, bet[t].x), fmaf(x[t].y, gam[t].y, bet[t].y), fmaf(x[t].z, gam[t].z, bet[t].z),
                       fmaf(x[t].w, gam[t].w, bet[t].w));
  }
  return rstd;
}

// a^T of hidden units 16hf .. + 15: acc[r] = a[token q][16hf + 4g + r] = b1 + sum_k z[token q][k] W1[k][16hf + 4g + r]
template <int D>
__device__ __forceinline__ f32x4 hidden_pre(const float* W1s, const float* b1s, int F, int hf, int g, int q,
                                            const float4 (&z)[D / 16]) {
  const float4 b = ld4(b1s + 16 * hf + 4 * g);
  f32x4 a = {b.x, b.y, b.z, b.w};
  const float* w = W1s + (4 * g) * (F + 4) + 16 * hf + q;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    const float* wt = w + 16 * t * (F + 4);
    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[0], z[t].x, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[F + 4], z[t].y, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[2 * (F + 4)], z[t].z, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[3 * (F + 4)], z[t].w, a, 0, 0, 0);
  }
  return a;
}

// rows [row0, row0 + 16) of one slot's [P, D] block of `out` that are padding: zeros (a lane stores its own columns)
template <int D>
__device__ __forceinline__ void store_rows(float* __restrict__ row, bool in_slot, bool real, const float4 (&v)[D / 16]) {
  if (!in_slot) return;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) st4(row + 16 * t, real ? v[t] : zero4());
}

template <int D>
__global__ void __launch_bounds__(kBlock) seq_ffn_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seg_len,
                                                         Shape sh, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ W2, const float* __restrict__ b2,
                                                         float* __restrict__ out, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NF = D / 16, LD2 = D + 4;
  const int F = sh.F, P = sh.P, LD1 = F + 4;
  float* W1s = lds;
  float* W2s = W1s + D * LD1;
  float* b1s = W2s + F * LD2;
  stage_weights<D>(W1, W2, b1, F, W1s, W2s, b1s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 15, g = lane >> 4;
  float4 gam[NF], bet[NF], b2f[NF];
  vec_frag<D>(gamma, g, gam);
  vec_frag<D>(beta, g, bet);
  vec_frag<D>(b2, g, b2f);
  const int tiles = (P + 15) >> 4;
  const int64_t units = sh.n_slots * tiles, stride = (int64_t)gridDim.x * kWaves;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < units; u += stride) {
    const int64_t b = u / tiles;
    const int j = (int)(u - b * tiles) * 16 + q;
    const int len = clamp_len(seg_len, b, P);
    const int64_t r = b * P + j;
    float* orow = out + r * ldo + 4 * g;
    float4 xf[NF], zf[NF];
    if (j - q >= len) {                                   // the whole tile is padding: wave-uniform
      store_rows<D>(orow, j < P, false, xf);
      continue;
    }
    const bool ok = j < len;
    load_frag<D>(x + r * ldx + 4 * g, ok, xf);
    float4 res[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) res[t] = xf[t];
    layer_norm<D>(xf, gam, bet, sh.eps, zf);
    f32x4 o[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) o[t] = f32x4{b2f[t].x, b2f[t].y, b2f[t].z, b2f[t].w};
    for (int hf = 0; hf < F / 16; ++hf) {
      const f32x4 a = hidden_pre<D>(W1s, b1s, F, hf, g, q, zf);
      const float* w = W2s + (16 * hf + 4 * g) * LD2 + q;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float lk = sh.leaky * a[i];
        const float h = lk >= a[i] ? lk : a[i];
#pragma unroll
        for (int t = 0; t < NF; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i * LD2 + 16 * t], h, o[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < NF; ++t)
      res[t] = make_float4(res[t].x + o[t][0], res[t].y + o[t][1], res[t].z + o[t][2], res[t].w + o[t][3]);
    store_rows<D>(orow, j < P, ok, res);
  }
}

// Backward, data path: dx = g + LN^T((g W2^T . act'(a)) W1^T); h and da of the real rows to hda [n_slots * P, 2F]; the
// wave's sums of dz . xh (dgamma) and dz (dbeta) over its tokens to ln_part [gridDim.x * kWaves, 2D].
template <int D>
__global__ void __launch_bounds__(kBlock) seq_ffn_bwd_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seg_len,
                                                             Shape sh, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ gout, int64_t ldg,
                                                             float* __restrict__ dx, int64_t ld_dx, float* __restrict__ hda,
                                                             float* __restrict__ ln_part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NF = D / 16, LD2 = D + 4;
  const int F = sh.F, P = sh.P, LD1 = F + 4;
  float* W1s = lds;
  float* W2s = W1s + D * LD1;
  float* b1s = W2s + F * LD2;
  stage_weights<D>(W1, W2, b1, F, W1s, W2s, b1s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 15, g = lane >> 4;
  float4 gam[NF], bet[NF], dgam[NF], dbet[NF];
  vec_frag<D>(gamma, g, gam);
  vec_frag<D>(beta, g, bet);
#pragma unroll
  for (int t = 0; t < NF; ++t) dgam[t] = dbet[t] = zero4();
  const int tiles = (P + 15) >> 4;
  const int64_t units = sh.n_slots * tiles, stride = (int64_t)gridDim.x * kWaves;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < units; u += stride) {
    const int64_t b = u / tiles;
    const int j = (int)(u - b * tiles) * 16 + q;
    const int len = clamp_len(seg_len, b, P);
    const int64_t r = b * P + j;
    float* drow = dx + r * ld_dx + 4 * g;
    float4 xh[NF], zf[NF], gf[NF];
    if (j - q >= len) {
      store_rows<D>(drow, j < P, false, xh);
      continue;
    }
    const bool ok = j < len;
    load_frag<D>(x + r * ldx + 4 * g, ok, xh);
    load_frag<D>(gout + r * ldg + 4 * g, ok, gf);         // a padded token: g = 0, so dh = da = dz = 0 below
    const float rstd = layer_norm<D>(xh, gam, bet, sh.eps, zf);
    f32x4 dz[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) dz[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* wrow = hda + r * (2 * (int64_t)F) + 4 * g;
    for (int hf = 0; hf < F / 16; ++hf) {
      const f32x4 a = hidden_pre<D>(W1s, b1s, F, hf, g, q, zf);
      f32x4 dh = {0.f, 0.f, 0.f, 0.f};
      const float* w2 = W2s + (16 * hf + q) * LD2 + 4 * g;
#pragma unroll
      for (int t = 0; t < NF; ++t) dh = mfma4(ld4(w2 + 16 * t), gf[t], dh);
      float h[4], da[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float lk = sh.leaky * a[i];
        const bool low = lk >= a[i];
        h[i] = low ? lk : a[i];
        da[i] = low ? sh.leaky * dh[i] : dh[i];
      }
      if (ok) {
        st4(wrow + 16 * hf, make_float4(h[0], h[1], h[2], h[3]));
        st4(wrow + F + 16 * hf, make_float4(da[0], da[1], da[2], da[3]));
      }
      const float4 da4 = make_float4(da[0], da[1], da[2], da[3]);
      const float* w1 = W1s + q * LD1 + 16 * hf + 4 * g;
#pragma unroll
      for (int t = 0; t < NF; ++t) dz[t] = mfma4(ld4(w1 + 16 * t * LD1), da4, dz[t]);
    }
    // layer-norm backward: dxh = dz * gamma, dx = g + rstd * (dxh - mean(dxh) - xh * mean(dxh * xh))
    float s1 = 0.f, s2 = 0.f;
    float4 dxh[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) {
      const float4 v = make_float4(dz[t][0], dz[t][1], dz[t][2], dz[t][3]);
      dgam[t] = make_float4(fmaf(v.x, xh[t].x, dgam[t].x), fmaf(v.y, xh[t].y, dgam[t].y), fmaf(v.z, xh[t].z, dgam[t].z),
                            fmaf(v.w, xh[t].w, dgam[t].w));
      dbet[t] = make_float4(dbet[t].x + v.x, dbet[t].y + v.y, dbet[t].z + v.z, dbet[t].w + v.w);
      dxh[t] = make_float4(v.x * gam[t].x, v.y * gam[t].y, v.z * gam[t].z, v.w * gam[t].w);
      s1 += sum4(dxh[t]);
      s2 += (dxh[t].x * xh[t].x + dxh[t].y * xh[t].y) + (dxh[t].z * xh[t].z + dxh[t].w * xh[t].w);
    }
    const float m1 = group_sum(s1) * (1.f / D), m2 = group_sum(s2) * (1.f / D);
#pragma unroll
    for (int t = 0; t < NF; ++t)
      dxh[t] = make_float4(fmaf(rstd, dxh[t].x - m1 - xh[t].x * m2, gf[t].x), fmaf(rstd, dxh[t].y - m1 - xh[t].y * m2, gf[t].y),
                           fmaf(rstd, dxh[t].z - m1 - xh[t].z * m2, gf[t].z), fmaf(rstd, dxh[t].w - m1 - xh[t].w * m2, gf[t].w));
    store_rows<D>(drow, j < P, ok, dxh);
  }
  // the wave's partial of dgamma | dbeta: over its 16 token lanes in one order, then one row of ln_part
  float* part = ln_part + ((int64_t)blockIdx.x * kWaves + wave) * (2 * D) + 4 * g;
#pragma unroll
  for (int t = 0; t < NF; ++t) {
    const float4 a = make_float4(row_sum(dgam[t].x), row_sum(dgam[t].y), row_sum(dgam[t].z), row_sum(dgam[t].w));
    const float4 c = make_float4(row_sum(dbet[t].x), row_sum(dbet[t].y), row_sum(dbet[t].z), row_sum(dbet[t].w));
    if (q == 0) {
      st4(part + 16 * t, a);
      st4(part + D + 16 * t, c);
    }
  }
}

// Backward, weight gradients: block-wide tiles of 16 tokens, staged row-major (z recomputed from x; h and da from hda;
// g), rows at or beyond n_b as zeros. Wave w owns the hidden blocks n = w, w + 4, ..: the output tiles (m, n) of dW1
// (rows 16m .., columns 16n ..) for every m < D / 16 and the tiles of dW2 at the transposed places, kept in accumulators
// over all the block's tiles; an operand read serves D / 16 (or up to 4) products. One partial [dW1 | dW2 | db1 | db2]
// per block.
template <int D>
__global__ void __launch_bounds__(kBlock) seq_ffn_wgrad_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const int32_t* __restrict__ seg_len, Shape sh,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ gout, int64_t ldg,
                                                               const float* __restrict__ hda, float* __restrict__ w_part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int LDD = D + 4, NX = (D / 4 + 15) / 16, ND = D / 16;
  constexpr int JN = ((kMaxDF / D < kMaxF ? kMaxDF / D : kMaxF) / 16 + kWaves - 1) / kWaves;   // hidden blocks a wave owns at most
  const int F = sh.F, P = sh.P, LDF = F + 4;
  float* zs = lds;
  float* gs = zs + 16 * LDD;
  float* hs = gs + 16 * LDD;
  float* das = hs + 16 * LDF;
  const int tid = threadIdx.x, lane = tid & 63, q = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // scalar: the tile ownership tests below are uniform
  const int srow = tid >> 4, sub = tid & 15;              // staging: 16 threads per token row
  const int nfb = F / 16;
  f32x4 acc1[JN][ND], acc2[JN][ND];
#pragma unroll
  for (int i = 0; i < JN; ++i)
#pragma unroll
    for (int m = 0; m < ND; ++m) acc1[i][m] = acc2[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;
  float4 gam[NX], bet[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    const int c4 = sub + 16 * k;
    gam[k] = c4 < D / 4 ? ld4(gamma + 4 * c4) : zero4();
    bet[k] = c4 < D / 4 ? ld4(beta + 4 * c4) : zero4();
  }
  const int tiles = (P + 15) >> 4;
  const int64_t units = sh.n_slots * tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t b = u / tiles;
    const int row0 = (int)(u - b * tiles) * 16;
    const int len = clamp_len(seg_len, b, P);
    if (row0 >= len) continue;                            // block-uniform
    {
      const bool ok = row0 + srow < len;
      const int64_t r = b * P + row0 + srow;
      float4 xv[NX];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int c4 = sub + 16 * k;
        xv[k] = ok && c4 < D / 4 ? ld4(x + r * ldx + 4 * c4) : zero4();
        s += sum4(xv[k]);
      }
      const float mean = row_sum(s) * (1.f / D);
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int c4 = sub + 16 * k;
        if (c4 < D / 4) {
          xv[k] = make_float4(xv[k].x - mean, xv[k].y - mean, xv[k].z - mean, xv[k].w - mean);
          v += (xv[k].x * xv[k].x + xv[k].y * xv[k].y) + (xv[k].z * xv[k].z + xv[k].w * xv[k].w);
        }
      }
      const float rstd = rsqrtf(row_sum(v) * (1.f / D) + sh.eps);
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int c4 = sub + 16 * k;
        if (c4 < D / 4) {
          float4 z = zero4();
          if (ok)
            z = make_float4(fmaf(xv[k].x * rstd, gam[k].x, bet[k].x), fmaf(xv[k].y * rstd, gam[k].y, bet[k].y),
                            fmaf(xv[k].z * rstd, gam[k].z, bet[k].z), fmaf(xv[k].w * rstd, gam[k].w, bet[k].w));
          st4(zs + srow * LDD + 4 * c4, z);
          st4(gs + srow * LDD + 4 * c4, ok ? ld4(gout + r * ldg + 4 * c4) : zero4());
        }
      }
      const float* wr = hda + r * (2 * (int64_t)F);
      for (int c4 = sub; c4 < F / 4; c4 += 16) {
        st4(hs + srow * LDF + 4 * c4, ok ? ld4(wr + 4 * c4) : zero4());
        st4(das + srow * LDF + 4 * c4, ok ? ld4(wr + F + 4 * c4) : zero4());
      }
    }
    __syncthreads();
    if (tid < F) {
#pragma unroll
      for (int i = 0; i < 16; ++i) db1 += das[i * LDF + tid];
    }
    if (tid < D) {
#pragma unroll
      for (int i = 0; i < 16; ++i) db2 += gs[i * LDD + tid];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                         // the MFMA's k index g at step k: token 4g + k of the tile
      const float* zr = zs + (4 * g + k) * LDD + q;
      const float* gr = gs + (4 * g + k) * LDD + q;
      const float* hr = hs + (4 * g + k) * LDF + q;
      const float* dr = das + (4 * g + k) * LDF + q;
      float za[ND], gb[ND];
#pragma unroll
      for (int m = 0; m < ND; ++m) {
        za[m] = zr[16 * m];
        gb[m] = gr[16 * m];
      }
#pragma unroll
      for (int i = 0; i < JN; ++i) {
        const int n = wave + kWaves * i;
        if (n < nfb) {                                    // wave-uniform
          const float dv = dr[16 * n], hv = hr[16 * n];
#pragma unroll
          for (int m = 0; m < ND; ++m) {
            acc1[i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[m], dv, acc1[i][m], 0, 0, 0);
            acc2[i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv, gb[m], acc2[i][m], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  const int64_t DF = (int64_t)D * F;
  float* part = w_part + (int64_t)blockIdx.x * (2 * DF + F + D);
#pragma unroll
  for (int i = 0; i < JN; ++i) {
    const int n = wave + kWaves * i;
    if (n < nfb) {
#pragma unroll
      for (int m = 0; m < ND; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          part[(int64_t)(16 * m + 4 * g + r) * F + 16 * n + q] = acc1[i][m][r];
          part[DF + (int64_t)(16 * n + 4 * g + r) * D + 16 * m + q] = acc2[i][m][r];
        }
    }
  }
  if (tid < F) part[2 * DF + tid] = db1;
  if (tid < D) part[2 * DF + F + tid] = db2;
}

// The sum of the partials, in one fixed order. Blocks [0, nb_w): 16 elements of [dW1 | dW2 | db1 | db2] each, 16 threads
// per element; thread `sl` of an element sums the blocks' partials sl, sl + 16, .. in ascending order, thread 0 then adds
// the 16 sums in ascending order. Blocks from nb_w on: 4 elements of dgamma | dbeta each, 64 threads per element, over
// the n_ln waves' partials in the same way.
__global__ void __launch_bounds__(kBlock) seq_ffn_reduce_kernel(const float* __restrict__ w_part, int n_w,
                                                                const float* __restrict__ ln_part, int n_ln, int D, int F,
                                                                int nb_w, float* __restrict__ dW1, float* __restrict__ dW2,
                                                                float* __restrict__ db1, float* __restrict__ db2,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[kBlock];
  const int DF = D * F, tid = threadIdx.x;
  const bool w = (int)blockIdx.x < nb_w;
  const float* part = w ? w_part : ln_part;
  const int n = w ? n_w : n_ln, width = w ? 2 * DF + F + D : 2 * D, ne = w ? 16 : 4, nsl = kBlock / ne;
  const int el = tid & (ne - 1), sl = tid / ne;
  const int e = (w ? (int)blockIdx.x : (int)blockIdx.x - nb_w) * ne + el;
  float s = 0.f;
  if (e < width)
    for (int p = sl; p < n; p += nsl) s += part[(int64_t)p * width + e];
  red[tid] = s;
  __syncthreads();
  if (sl != 0 || e >= width) return;
  float t = 0.f;
  for (int k = 0; k < nsl; ++k) t += red[k * ne + el];
  if (!w) {
    if (e < D) dgamma[e] = t;
    else dbeta[e - D] = t;
  } else if (e < DF) {
    dW1[e] = t;
  } else if (e < 2 * DF) {
    dW2[e - DF] = t;
  } else if (e < 2 * DF + F) {
    db1[e - 2 * DF] = t;
  } else {
    db2[e - 2 * DF - F] = t;
  }
}

// ---- host side: every entry rejects a bad call before any device work ----------------------------------------------
int ffn_shape(const char* who, int d, int f, int P) {
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (f < 16 || f > kMaxF || f % 16)
    return sagnn::fail(SAGNN_ERR_DIM, "%s: f = %d, need a multiple of 16 with 16 <= f <= %d", who, f, kMaxF);
  if (d * f > kMaxDF)
    return sagnn::fail(SAGNN_ERR_DIM, "%s: d * f = %d * %d, need d * f <= %d (both weight matrices stay in LDS)", who, d, f, kMaxDF);
  if (P < 1 || P > kMaxP) return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, P, kMaxP);
  return SAGNN_OK;
}

size_t weights_lds(int d, int f) { return ((size_t)d * (f + 4) + (size_t)f * (d + 4) + f) * sizeof(float); }
size_t wgrad_lds(int d, int f) { return (size_t)32 * (d + 4 + f + 4) * sizeof(float); }

int64_t units_of(int64_t n_slots, int P) { return n_slots * ((P + 15) / 16); }

// workgroups of the persistent kernels: what a compute unit holds at once, by LDS and by the registers of the data-path
// backward (148, 228 and 396 per lane at d = 32, 64 and 128: 3, 2 and 1 waves per SIMD), times the compute units
int data_blocks(int64_t n_slots, int P, int d, int f) {
  const int64_t by_regs = d == 32 ? 3 : d == 64 ? 2 : 1;
  const int64_t per_cu = std::min<int64_t>(by_regs, std::max<int64_t>(1, (int64_t)(kLdsPerCU / weights_lds(d, f))));
  const int64_t need = (units_of(n_slots, P) + kWaves - 1) / kWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, per_cu * kCUs));
}
int wgrad_blocks(int64_t n_slots, int P) { return (int)std::max<int64_t>(1, std::min<int64_t>(units_of(n_slots, P), kCUs)); }

int64_t w_part_floats(int d, int f) { return 2 * (int64_t)d * f + f + d; }

struct Workspace {
  int64_t hda, w_part, ln_part, total;    // offsets and the total, in floats
};
Workspace workspace_of(int64_t n_slots, int P, int d, int f) {
  Workspace w;
  w.hda = 0;
  w.w_part = n_slots * P * 2 * f;
  w.ln_part = w.w_part + (int64_t)wgrad_blocks(n_slots, P) * w_part_floats(d, f);
  w.total = w.ln_part + (int64_t)data_blocks(n_slots, P, d, f) * kWaves * 2 * d;
  return w;
}

int check_args(const char* who, const sagnn_seq_ffn_args* a) {
  if (!a) return sagnn::fail(SAGNN_ERR_NULL, "%s: null args", who);
  if (!a->x || !a->seg_len || !a->gamma || !a->beta || !a->W1 || !a->b1 || !a->W2 || !a->b2)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (x, seg_len, gamma, beta, W1, b1, W2, b2)", who);
  if (int rc = ffn_shape(who, a->d, a->f, a->pos_length)) return rc;
  if (a->n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)a->n_slots);
  if (a->n_slots > INT64_MAX / ((int64_t)kMaxP * 2 * kMaxF * (int64_t)sizeof(float)))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_slots = %lld is too large", who, (long long)a->n_slots);
  if (!(a->leaky >= 0.f && a->leaky < 1.f)) return sagnn::fail(SAGNN_ERR_ARG, "%s: leaky = %g, need 0 <= leaky < 1", who, a->leaky);
  if (!(a->ln_eps > 0.f) || a->ln_eps > 1.f) return sagnn::fail(SAGNN_ERR_ARG, "%s: ln_eps = %g, need 0 < ln_eps <= 1", who, a->ln_eps);
  if (a->ldx < a->d || (a->ldx & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: ldx = %lld, need a multiple of 4 >= d", who, (long long)a->ldx);
  const void* ptrs[] = {a->x, a->gamma, a->beta, a->W1, a->b1, a->W2, a->b2};
  for (const void* p : ptrs)
    if (!sagnn::aligned16(p)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: x, gamma, beta, W1, b1, W2 and b2 must be 16-byte aligned", who);
  return SAGNN_OK;
}

int check_rows(const char* who, const char* name, const void* p, int64_t ld, int d) {
  if (!p) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (%s)", who, name);
  if (!sagnn::aligned16(p)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned", who, name);
  if (ld < d || (ld & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: the row stride of %s is %lld, need a multiple of 4 >= d", who, name, (long long)ld);
  return SAGNN_OK;
}

Shape shape_of(const sagnn_seq_ffn_args* a) { return Shape{a->n_slots, a->pos_length, a->f, a->ln_eps, a->leaky}; }

template <int D>
int launch_fwd(const sagnn_seq_ffn_args* a, float* out, int64_t ldo, hipStream_t s) {
  const size_t lds = weights_lds(D, a->f);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&seq_ffn_kernel<D>), lds)) return rc;
  hipLaunchKernelGGL((seq_ffn_kernel<D>), dim3(data_blocks(a->n_slots, a->pos_length, D, a->f)), dim3(kBlock), lds, s, a->x, a->ldx,
                     a->seg_len, shape_of(a), a->gamma, a->beta, a->W1, a->b1, a->W2, a->b2, out, ldo);
  return SAGNN_OK;
}

template <int D>
int launch_bwd(const sagnn_seq_ffn_args* a, const float* g, int64_t ldg, float* dx, int64_t ld_dx, float* ws, const Workspace& w,
               hipStream_t s) {
  const size_t lds = weights_lds(D, a->f), lds_w = wgrad_lds(D, a->f);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&seq_ffn_bwd_kernel<D>), lds)) return rc;
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&seq_ffn_wgrad_kernel<D>), lds_w)) return rc;
  hipLaunchKernelGGL((seq_ffn_bwd_kernel<D>), dim3(data_blocks(a->n_slots, a->pos_length, D, a->f)), dim3(kBlock), lds, s, a->x,
                     a->ldx, a->seg_len, shape_of(a), a->gamma, a->beta, a->W1, a->b1, a->W2, g, ldg, dx, ld_dx, ws + w.hda,
                     ws + w.ln_part);
  hipLaunchKernelGGL((seq_ffn_wgrad_kernel<D>), dim3(wgrad_blocks(a->n_slots, a->pos_length)), dim3(kBlock), lds_w, s, a->x, a->ldx,
                     a->seg_len, shape_of(a), a->gamma, a->beta, g, ldg, ws + w.hda, ws + w.w_part);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_seq_ffn_supported(int d, int f, int pos_length) { return ffn_shape("seq_ffn", d, f, pos_length); }

extern "C" int sagnn_seq_ffn_f32(const sagnn_seq_ffn_args* args, float* out, int64_t ld_out, void* stream) {
  const char* who = "seq_ffn";
  if (int rc = check_args(who, args)) return rc;
  if (int rc = check_rows(who, "out", out, ld_out, args->d)) return rc;
  if (args->n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, args->n_slots, args->pos_length);
  int rc;
  switch (args->d) {
    case 32: rc = launch_fwd<32>(args, out, ld_out, s); break;
    case 64: rc = launch_fwd<64>(args, out, ld_out, s); break;
    default: rc = launch_fwd<128>(args, out, ld_out, s); break;
  }
  if (rc) return rc;
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" size_t sagnn_seq_ffn_bwd_workspace_bytes(int64_t n_slots, int pos_length, int d, int f) {
  if (n_slots < 0 || ffn_shape("seq_ffn_bwd_workspace_bytes", d, f, pos_length)) return 0;
  return (size_t)workspace_of(n_slots, pos_length, d, f).total * sizeof(float);
}

extern "C" int sagnn_seq_ffn_bwd_f32(const sagnn_seq_ffn_args* args, const float* g, int64_t ldg, float* dx, int64_t ld_dx,
                                     float* dgamma, float* dbeta, float* dW1, float* db1, float* dW2, float* db2,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "seq_ffn_bwd";
  if (int rc = check_args(who, args)) return rc;
  if (int rc = check_rows(who, "g", g, ldg, args->d)) return rc;
  if (int rc = check_rows(who, "dx", dx, ld_dx, args->d)) return rc;
  if (!dgamma || !dbeta || !dW1 || !db1 || !dW2 || !db2)
    return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (dgamma, dbeta, dW1, db1, dW2, db2)", who);
  const int d = args->d, f = args->f;
  const Workspace w = workspace_of(args->n_slots, args->pos_length, d, f);
  if (!workspace || !sagnn::aligned16(workspace) || workspace_bytes < (size_t)w.total * sizeof(float))
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "%s: workspace needs %zu bytes, 16-byte aligned (sagnn_seq_ffn_bwd_workspace_bytes)", who,
                       (size_t)w.total * sizeof(float));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, args->n_slots, args->pos_length);
  int n_w = 0, n_ln = 0;
  if (args->n_slots > 0) {
    int rc;
    switch (d) {
      case 32: rc = launch_bwd<32>(args, g, ldg, dx, ld_dx, ws, w, s); break;
      case 64: rc = launch_bwd<64>(args, g, ldg, dx, ld_dx, ws, w, s); break;
      default: rc = launch_bwd<128>(args, g, ldg, dx, ld_dx, ws, w, s); break;
    }
    if (rc) return rc;
    n_w = wgrad_blocks(args->n_slots, args->pos_length);
    n_ln = data_blocks(args->n_slots, args->pos_length, d, f) * kWaves;
  }
  const int nb_w = ((int)w_part_floats(d, f) + 15) / 16, nb_ln = (2 * d + 3) / 4;
  hipLaunchKernelGGL(seq_ffn_reduce_kernel, dim3(nb_w + nb_ln), dim3(kBlock), 0, s, ws + w.w_part, n_w, ws + w.ln_part, n_ln, d, f,
                     nb_w, dW1, dW2, db1, db2, dgamma, dbeta);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
