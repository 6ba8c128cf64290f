// Sequence attention at head widths 16, 32 and 64 (--seqHeads): the contract of seq_attn.hip's ragged
// attention (sagnn_seq_attn_masked_f32 / _bwd_f32) on the fp32 matrix cores. seq_attn.hip keeps a query's d_k floats
// of q, acc and dq in a thread's registers and walks the keys on the VALU, which stops at d_k = 8; here every product
// (Q K^T, P V and, backward, G V^T, dS K, dS^T Q, P^T G) is a chain of v_mfma_f32_16x16x4_f32: exact fp32, the same
// under every engine.
// One workgroup of four waves per (slot, head). Tiles of 16 tokens; every loop runs over the slot's ceil(n_b / 16)
// tiles, never over P. A score tile is computed transposed (keys as the A rows, queries as the B columns), so a lane
// holds 4 keys of one query in its accumulator: row maximum and row sum are reductions over the 4 lanes that share
// lane & 15, and the 4 values are already the B operand of the second product (ctx^T = V^T P^T, with the MFMA's k index
// g = lane >> 4 dealt to key 4g + i at step i), so P never goes through LDS. The A operand of that product is one float
// of V per lane, read from LDS at a row stride of d_k + 4 floats (rows 4g + i of the four lane groups fall into four
// different bank groups).
// Rows at or beyond n_b are zeroed on load by a predicate on the row index (a tile of the last slot reaches past the
// end of the buffer when P % 16 != 0), and a masked score becomes e = 0 through a compare and select, never through a
// product with 0.
#include <limits.h>

#include "common.h"

namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxP = 256;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ int clamp_len(const int32_t* seg_len, int64_t b, int P) { return min(max(seg_len[b], 0), P); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 scaled(const float4& v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }

__host__ __device__ constexpr int tile_rows(int P) { return (P + 15) / 16 * 16; }

// rows [0, rows) of one head's DK columns (src points at row 0, column 0 of them; row stride ld) times `scale` into
// LDS at a row stride of DK + 4; rows >= len are zeros and are not read
template <int DK>
__device__ __forceinline__ void stage(const float* __restrict__ src, int64_t ld, int len, int rows, float scale, float* dst) {
  constexpr int C4 = DK / 4, LD = DK + 4;
  for (int i = threadIdx.x; i < rows * C4; i += kBlock) {
    const int r = i / C4, c = (i - r * C4) * 4;
    float4 v = zero4();
    if (r < len) v = scaled(ld4(src + r * ld + c), scale);
    st4(dst + r * LD + c, v);
  }
}

// a lane's fragment of one row: columns 16t + 4g .. + 3 (row points at column 4g); zeros when the row is padding
template <int DK>
__device__ __forceinline__ void load_frag(const float* __restrict__ row, bool ok, float scale, float4 (&f)[DK / 16]) {
#pragma unroll
  for (int t = 0; t < DK / 16; ++t) f[t] = ok ? scaled(ld4(row + 16 * t), scale) : zero4();
}

template <int DK>
__device__ __forceinline__ void lds_frag(const float* row, float4 (&f)[DK / 16]) {
#pragma unroll
  for (int t = 0; t < DK / 16; ++t) f[t] = ld4(row + 16 * t);
}

// acc[r] = <row 4 * (lane >> 4) + r of the A side, row lane & 15 of the B side>: a fixed fmaf chain over the columns
// (softmax_loss.hip's tile_scores)
template <int DK>
__device__ __forceinline__ f32x4 tile_scores(const float4 (&a)[DK / 16], const float4 (&b)[DK / 16]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < DK / 16; ++t) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[t].w, acc, 0, 0, 0);
  }
  return acc;
}

// out^T[16f + 4g + r][lane & 15] += sum over the tile's 16 rows of rows[4g' + i][16f + c] * w(row 4g' + i, lane & 15):
// `rows` points at LDS row 4g, column lane & 15 of the tile; w[i] is the lane's weight of row 4g + i
template <int DK>
__device__ __forceinline__ void contract(const float* rows, const float (&w)[4], f32x4 (&out)[DK / 16]) {
  constexpr int LD = DK + 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int f = 0; f < DK / 16; ++f) out[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(rows[i * LD + 16 * f], w[i], out[f], 0, 0, 0);
}

// the sum / the maximum over the 4 lanes that share lane & 15, in one order for all four
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

template <int DK>
__device__ __forceinline__ void store_frag(float* row, const f32x4 (&acc)[DK / 16], float s) {
#pragma unroll
  for (int f = 0; f < DK / 16; ++f) st4(row + 16 * f, make_float4(acc[f][0] * s, acc[f][1] * s, acc[f][2] * s, acc[f][3] * s));
}

// zeros in rows [len, P) of the head's DK columns of `thirds` column blocks d apart (row stride ld)
template <int DK>
__device__ __forceinline__ void zero_padding(float* base, int64_t ld, int d, int thirds, int len, int P) {
  constexpr int C4 = DK / 4;
  for (int i = threadIdx.x; i < (P - len) * C4; i += kBlock) {
    const int r = len + i / C4, c = (i % C4) * 4;
    for (int t = 0; t < thirds; ++t) st4(base + r * ld + t * d + c, zero4());
  }
}

// Forward. K and V of the head sit in LDS (2 * tile_rows(P) * (DK + 4) floats); a wave owns the query tiles
// wave, wave + 4, ... and walks the key tiles in ascending order with the running maximum m, sum z and ctx^T, rescaled
// by 2^(m_old - m_new) when the maximum moves: e' / (sum e' + 1e-8 * 2^-m) with m the row's largest folded score.
// CAUSAL: the key tiles above the diagonal are skipped, the diagonal one is masked per element.
template <int DK, bool CAUSAL>
__global__ void __launch_bounds__(kBlock) seq_attn_wide_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ seg_len,
                                                               int P, int d, float* __restrict__ ctx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int LD = DK + 4, NF = DK / 16;
  const int64_t b = blockIdx.x;
  const int hc = blockIdx.y * DK;
  const int len = clamp_len(seg_len, b, P);
  const int64_t ld = 3 * (int64_t)d;
  const float* base = qkv + b * P * ld + hc;
  float* out = ctx + b * P * (int64_t)d + hc;
  zero_padding<DK>(out, d, d, 1, len, P);
  if (len == 0) return;
  const int nt = (len + 15) >> 4;
  float* Ks = lds;
  float* Vs = lds + tile_rows(P) * LD;
  stage<DK>(base + d, ld, len, nt * 16, 1.f, Ks);
  stage<DK>(base + 2 * d, ld, len, nt * 16, 1.f, Vs);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 15, g = lane >> 4;
  const float fold = kLog2e * rsqrtf((float)DK);
  for (int qt = wave; qt < nt; qt += kWaves) {
    const int j = qt * 16 + q;
    float4 qf[NF];
    load_frag<DK>(base + j * ld + 4 * g, j < len, fold, qf);
    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, z = 0.f;
    const int nkt = CAUSAL ? qt + 1 : nt;
    for (int kt = 0; kt < nkt; ++kt) {
      float4 kf[NF];
      lds_frag<DK>(Ks + (kt * 16 + q) * LD + 4 * g, kf);
      const f32x4 s = tile_scores<DK>(kf, qf);
      const int s0 = kt * 16 + 4 * g;
      bool ok[4];
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = s0 + r < len && (!CAUSAL || s0 + r <= j);
        tm = fmaxf(tm, ok[r] ? s[r] : -INFINITY);
      }
      const float mn = fmaxf(m, group_max(tm));           // finite from the first tile on: key 0 is visible to every query
      const float corr = exp2f(m - mn);
      float e[4], zs = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = ok[r] ? exp2f(s[r] - mn) : 0.f;
        zs += e[r];
      }
      z = fmaf(z, corr, group_sum(zs));
      m = mn;
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] *= corr;
      contract<DK>(Vs + s0 * LD + q, e, acc);
    }
    const float rz = 1.f / (z + 1e-8f * exp2f(-m));
    if (j < len) store_frag<DK>(out + j * (int64_t)d + 4 * g, acc, rz);
  }
}

// Backward: e is recomputed from q|k|v. With a = e rz, dP_js = <g_j, v_s>, D_j = sum_s a_js dP_js (= <g_j, ctx_j>) and
// p_js = a_js (dP_js - D_j):  dq_j = sum_s p_js k_s / sqrt(d_k),  dk_s = sum_j p_js q_j / sqrt(d_k),  dv_s = sum_j a_js g_j.
// Phase 1, K and V in LDS, a wave per query tile: m, rz and D of its 16 queries in one walk over the key tiles (the
// forward's running rescale, on z and on sum e' dP), then dq in a second walk; m, rz, D go to LDS.
// Phase 2, the same LDS re-used for q * log2(e) / sqrt(d_k) and g, a wave per key tile: the score tile the other way
// round (queries as the A rows), so a lane holds 4 queries of one key, and dk^T, dv^T accumulate over the query tiles in
// ascending order in the one wave that owns the key tile. No atomics: the same bits in every run.
// CAUSAL: phase 1 walks the key tiles 0 .. qt, phase 2 the query tiles kt .. nt - 1.
template <int DK, bool CAUSAL>
__global__ void __launch_bounds__(kBlock) seq_attn_wide_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ gctx,
                                                                   const int32_t* __restrict__ seg_len, int P, int d,
                                                                   float* __restrict__ dqkv) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int LD = DK + 4, NF = DK / 16;
  const int64_t b = blockIdx.x;
  const int hc = blockIdx.y * DK;
  const int len = clamp_len(seg_len, b, P);
  const int64_t ld = 3 * (int64_t)d;
  const float* base = qkv + b * P * ld + hc;
  const float* gbase = gctx + b * P * (int64_t)d + hc;
  float* dbase = dqkv + b * P * ld + hc;
  zero_padding<DK>(dbase, ld, d, 3, len, P);
  if (len == 0) return;
  const int nt = (len + 15) >> 4, R = tile_rows(P);
  float* A = lds;                    // K, then q * log2(e) / sqrt(d_k)
  float* B = lds + R * LD;           // V, then g
  float* Ms = B + R * LD;            // per query: the row's shift m, 1 / (Z' + 1e-8 2^-m), D
  float* Rz = Ms + R;
  float* Ds = Rz + R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 15, g = lane >> 4;
  const float scale = rsqrtf((float)DK), fold = kLog2e * scale;

  stage<DK>(base + d, ld, len, nt * 16, 1.f, A);
  stage<DK>(base + 2 * d, ld, len, nt * 16, 1.f, B);
  __syncthreads();
  for (int qt = wave; qt < nt; qt += kWaves) {
    const int j = qt * 16 + q;
    float4 qf[NF], gf[NF];
    load_frag<DK>(base + j * ld + 4 * g, j < len, fold, qf);
    load_frag<DK>(gbase + j * (int64_t)d + 4 * g, j < len, 1.f, gf);
    const int nkt = CAUSAL ? qt + 1 : nt;
    float m = -INFINITY, z = 0.f, da = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
      float4 kf[NF], vf[NF];
      lds_frag<DK>(A + (kt * 16 + q) * LD + 4 * g, kf);
      lds_frag<DK>(B + (kt * 16 + q) * LD + 4 * g, vf);
      const f32x4 s = tile_scores<DK>(kf, qf), dp = tile_scores<DK>(vf, gf);
      const int s0 = kt * 16 + 4 * g;
      bool ok[4];
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = s0 + r < len && (!CAUSAL || s0 + r <= j);
        tm = fmaxf(tm, ok[r] ? s[r] : -INFINITY);
      }
      const float mn = fmaxf(m, group_max(tm));
      const float corr = exp2f(m - mn);
      float zs = 0.f, ds = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = ok[r] ? exp2f(s[r] - mn) : 0.f;
        zs += e;
        ds = fmaf(e, ok[r] ? dp[r] : 0.f, ds);
      }
      z = fmaf(z, corr, group_sum(zs));
      da = fmaf(da, corr, group_sum(ds));
      m = mn;
    }
    const float rz = 1.f / (z + 1e-8f * exp2f(-m));
    const float D = da * rz;
    f32x4 dq[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) dq[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nkt; ++kt) {
      float4 kf[NF], vf[NF];
      lds_frag<DK>(A + (kt * 16 + q) * LD + 4 * g, kf);
      lds_frag<DK>(B + (kt * 16 + q) * LD + 4 * g, vf);
      const f32x4 s = tile_scores<DK>(kf, qf), dp = tile_scores<DK>(vf, gf);
      const int s0 = kt * 16 + 4 * g;
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = s0 + r < len && (!CAUSAL || s0 + r <= j);
        p[r] = ok ? exp2f(s[r] - m) * rz * (dp[r] - D) : 0.f;
      }
      contract<DK>(A + s0 * LD + q, p, dq);
    }
    if (j < len) store_frag<DK>(dbase + j * ld + 4 * g, dq, scale);
    if (g == 0) {                                           // j < nt * 16 <= R
      Ms[j] = m;
      Rz[j] = rz;
      Ds[j] = D;
    }
  }
  __syncthreads();
  stage<DK>(base, ld, len, nt * 16, fold, A);
  stage<DK>(gbase, d, len, nt * 16, 1.f, B);
  __syncthreads();
  for (int kt = wave; kt < nt; kt += kWaves) {
    const int sk = kt * 16 + q;
    float4 kf[NF], vf[NF];
    load_frag<DK>(base + sk * ld + d + 4 * g, sk < len, 1.f, kf);
    load_frag<DK>(base + sk * ld + 2 * d + 4 * g, sk < len, 1.f, vf);
    f32x4 dk[NF], dv[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) dk[f] = dv[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = CAUSAL ? kt : 0; qt < nt; ++qt) {         // query tiles in ascending order
      float4 aq[NF], ag[NF];
      lds_frag<DK>(A + (qt * 16 + q) * LD + 4 * g, aq);
      lds_frag<DK>(B + (qt * 16 + q) * LD + 4 * g, ag);
      const f32x4 s = tile_scores<DK>(aq, kf), dp = tile_scores<DK>(ag, vf);
      const int j0 = qt * 16 + 4 * g;
      const float4 m4 = ld4(Ms + j0), r4 = ld4(Rz + j0), d4 = ld4(Ds + j0);
      const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
      float a[4], p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = j0 + r < len && sk < len && (!CAUSAL || sk <= j0 + r);
        a[r] = ok ? exp2f(s[r] - mm[r]) * rr[r] : 0.f;
        p[r] = ok ? a[r] * (dp[r] - dd[r]) : 0.f;
      }
      contract<DK>(A + j0 * LD + q, p, dk);
      contract<DK>(B + j0 * LD + q, a, dv);
    }
    if (sk < len) {
      store_frag<DK>(dbase + sk * ld + d + 4 * g, dk, kLn2);   // A carries log2(e) / sqrt(d_k): times ln 2 leaves 1 / sqrt(d_k)
      store_frag<DK>(dbase + sk * ld + 2 * d + 4 * g, dv, 1.f);
    }
  }
}

// ---- host side: every entry rejects a bad call before any device work ----------------------------------------------
int wide_shape(const char* who, int d, int heads, int P) {
  if (d < 4 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a positive multiple of 4", who, d);
  if (heads < 1 || d % heads) return sagnn::fail(SAGNN_ERR_DIM, "%s: heads = %d does not divide d = %d", who, heads, d);
  const int dk = d / heads;
  if (dk != 16 && dk != 32 && dk != 64) return sagnn::fail(SAGNN_ERR_DIM, "%s: d / heads = %d, need 16, 32 or 64", who, dk);
  if (P < 1 || P > kMaxP) return sagnn::fail(SAGNN_ERR_DIM, "%s: pos_length = %d, need 1 <= pos_length <= %d", who, P, kMaxP);
  return SAGNN_OK;
}

int check_call(const char* who, int d, int heads, int P, int64_t n_slots, int causal) {
  if (causal != 0 && causal != 1) return sagnn::fail(SAGNN_ERR_ARG, "%s: causal = %d, need 0 or 1", who, causal);
  if (int rc = wide_shape(who, d, heads, P)) return rc;
  if (n_slots < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (n_slots = %lld)", who, (long long)n_slots);
  if (n_slots > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: grid too large (%lld slots)", who, (long long)n_slots);
  return SAGNN_OK;
}

int check_dense(const char* who, const void* p, const char* name) {
  if (!sagnn::aligned16(p)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned", who, name);
  return SAGNN_OK;
}

size_t lds_bytes(int dk, int P, bool bwd) {
  return ((size_t)2 * tile_rows(P) * (dk + 4) + (bwd ? 3 * tile_rows(P) : 0)) * sizeof(float);
}

template <int DK, bool CAUSAL>
int launch_fwd(dim3 grid, size_t lds, hipStream_t s, const float* qkv, const int32_t* seg_len, int P, int d, float* ctx) {
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&seq_attn_wide_kernel<DK, CAUSAL>), lds)) return rc;
  hipLaunchKernelGGL((seq_attn_wide_kernel<DK, CAUSAL>), grid, dim3(kBlock), lds, s, qkv, seg_len, P, d, ctx);
  return SAGNN_OK;
}

template <int DK, bool CAUSAL>
int launch_bwd(dim3 grid, size_t lds, hipStream_t s, const float* qkv, const float* g, const int32_t* seg_len, int P, int d,
               float* dqkv) {
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&seq_attn_wide_bwd_kernel<DK, CAUSAL>), lds)) return rc;
  hipLaunchKernelGGL((seq_attn_wide_bwd_kernel<DK, CAUSAL>), grid, dim3(kBlock), lds, s, qkv, g, seg_len, P, d, dqkv);
  return SAGNN_OK;
}

template <bool CAUSAL>
int launch_fwd_dk(int dk, dim3 grid, size_t lds, hipStream_t s, const float* qkv, const int32_t* seg_len, int P, int d, float* ctx) {
  switch (dk) {
    case 16: return launch_fwd<16, CAUSAL>(grid, lds, s, qkv, seg_len, P, d, ctx);
    case 32: return launch_fwd<32, CAUSAL>(grid, lds, s, qkv, seg_len, P, d, ctx);
    default: return launch_fwd<64, CAUSAL>(grid, lds, s, qkv, seg_len, P, d, ctx);
  }
}

template <bool CAUSAL>
int launch_bwd_dk(int dk, dim3 grid, size_t lds, hipStream_t s, const float* qkv, const float* g, const int32_t* seg_len, int P,
                  int d, float* dqkv) {
  switch (dk) {
    case 16: return launch_bwd<16, CAUSAL>(grid, lds, s, qkv, g, seg_len, P, d, dqkv);
    case 32: return launch_bwd<32, CAUSAL>(grid, lds, s, qkv, g, seg_len, P, d, dqkv);
    default: return launch_bwd<64, CAUSAL>(grid, lds, s, qkv, g, seg_len, P, d, dqkv);
  }
}

}  // namespace

extern "C" int sagnn_seq_attn_wide_supported(int d, int heads, int pos_length) {
  return wide_shape("seq_attn_wide", d, heads, pos_length);
}

extern "C" int sagnn_seq_attn_wide_f32(const float* qkv, const int32_t* seg_len, int64_t n_slots, int pos_length, int d,
                                       int heads, int causal, float* ctx, void* stream) {
  const char* who = "seq_attn_wide";
  if (!qkv || !seg_len || !ctx) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, seg_len, ctx)", who);
  if (int rc = check_call(who, d, heads, pos_length, n_slots, causal)) return rc;
  if (int rc = check_dense(who, qkv, "qkv")) return rc;
  if (int rc = check_dense(who, ctx, "ctx")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int dk = d / heads;
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  const size_t lds = lds_bytes(dk, pos_length, false);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (int rc = causal ? launch_fwd_dk<true>(dk, grid, lds, s, qkv, seg_len, pos_length, d, ctx)
                      : launch_fwd_dk<false>(dk, grid, lds, s, qkv, seg_len, pos_length, d, ctx))
    return rc;
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_seq_attn_wide_bwd_f32(const float* qkv, const float* g_ctx, const int32_t* seg_len, int64_t n_slots,
                                           int pos_length, int d, int heads, int causal, float* dqkv, void* stream) {
  const char* who = "seq_attn_wide_bwd";
  if (!qkv || !g_ctx || !seg_len || !dqkv) return sagnn::fail(SAGNN_ERR_NULL, "%s: null pointer (qkv, g_ctx, seg_len, dqkv)", who);
  if (int rc = check_call(who, d, heads, pos_length, n_slots, causal)) return rc;
  if (int rc = check_dense(who, qkv, "qkv")) return rc;
  if (int rc = check_dense(who, g_ctx, "g_ctx")) return rc;
  if (int rc = check_dense(who, dqkv, "dqkv")) return rc;
  if (n_slots == 0) return SAGNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int dk = d / heads;
  const dim3 grid((unsigned)n_slots, (unsigned)heads);
  const size_t lds = lds_bytes(dk, pos_length, true);
  sagnn::ProfileScope prof(sagnn::kProfSeqAtt, s, n_slots, pos_length);
  if (int rc = causal ? launch_bwd_dk<true>(dk, grid, lds, s, qkv, g_ctx, seg_len, pos_length, d, dqkv)
                      : launch_bwd_dk<false>(dk, grid, lds, s, qkv, g_ctx, seg_len, pos_length, d, dqkv))
    return rc;
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
