// GRU cell of the interval fusion (--rnnCell gru): TF 1.14 GRUCell over T steps, zero initial state,
// beside the BasicLSTMCell of fusion_mfma.hip. Per row and step
//     [r | u] = sigmoid([x | h] Wg + bg)      Wg [2d, 2d]
//     c       = tanh([x | r.h] Wc + bc)       Wc [2d, d]
//     h'      = u.h + (1 - u).c
// Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) under every engine: there is no f16 x 2 form of this cell.
//
// Fused kernel (d = 32 / 64), modelled on lstm_fwd_mfma_kernel: persistent over T, one wave per SIMD, a wave owns 32
// rows, both weights copied once into LDS in fragment order, no block barrier in the step loop. A step holds TWO
// dependent products: r must exist before r.h can enter the candidate product, so r.h goes from the C layout through
// the wave's staging tile back into the A layout, the way h does at the end of a step. The x half of the candidate
// product does not depend on r and is issued with the gate product.
//
//   Fragment order of a weight W [2D][NC], NT = NC / 32 column tiles (4, 2 or 1): for k-step kk, lane l, tile ct
//       Wf[(kk*64 + l)*NT + ct] = W[kcol(kk, l>>5)][ct*32 + (l&31)]
//   so the B operands of all NT tiles of a k-step arrive with one ds_read_b{32 NT} per lane, consecutive lanes at
//   consecutive addresses. (fusion_mfma.hip's order groups four tiles per read and needs NC % 128 == 0.)
//
// Any other d (multiples of 32 up to 256): one step at a time on the stream, the two products through dense.hip's
// kernels and two element-wise kernels of this file. The counterpart of the LSTM's generic route: not built for speed.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 waves = one per SIMD
constexpr int kRowsPerWave = 32;
constexpr int kRowsPerBlock = 128;
constexpr float kL2E = 1.44269504088896340736f;

// sigmoid(z) = 1 / (1 + 2^(-z log2e)), tanh(z) = 1 - 2 / (1 + 2^(2 z log2e)), z = acc + bias with the bias pre-scaled
// (kb = k * bias) so that it rides on the fma. Both saturate cleanly: 2^+big = inf -> rcp 0, 2^-big = 0 -> rcp 1.
__device__ __forceinline__ float sigmoid_kb(float acc, float kb) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc, -kL2E, kb)));
}
__device__ __forceinline__ float tanh_kb(float acc, float kb) {
  return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc, 2.f * kL2E, kb))), 1.f);
}

// row of C/D register r in lane half rh for a 32x32 MFMA tile
__device__ __forceinline__ int crow(int r, int rh) { return (r & 3) + 8 * (r >> 2) + 4 * rh; }

// ---- the per-wave [32][D] staging tile: the layout of fusion_mfma.hip ---------------------------
// Filled row-major (float4 from global, or element-wise from the C layout), read back in the A layout (lane = row) as
// float4: lane (row, kh) takes columns 8q + 4kh .. + 3, so k-step m = 4q + e multiplies column kcol(m, kh). The 16-byte
// slots of a row are XOR-swizzled with the row: both access patterns are bank-conflict free.
__device__ __forceinline__ int kcol(int m, int kh) { return 8 * (m >> 2) + 4 * kh + (m & 3); }
template <int D>
__device__ __forceinline__ int tile_slot(int row, int slot) {
  constexpr int SL = D / 4;
  constexpr int RPB = SL >= 16 ? 1 : 16 / SL;
  return slot ^ ((row / RPB) & (SL - 1));
}
template <int D>
__device__ __forceinline__ float4* tile_vec(float* tile, int row, int slot) {
  return reinterpret_cast<float4*>(tile + row * D) + tile_slot<D>(row, slot);
}
template <int D>
__device__ __forceinline__ float* tile_elem(float* tile, int row, int col) {
  return tile + row * D + (tile_slot<D>(row, col >> 2) << 2) + (col & 3);
}
template <int D>
__device__ __forceinline__ void read_a_operand(float* tile, int row, int kh, float (&a)[D / 2]) {
#pragma unroll
  for (int q = 0; q < D / 8; ++q) {
    const float4 v = *tile_vec<D>(tile, row, 2 * q + kh);
    a[4 * q + 0] = v.x;
    a[4 * q + 1] = v.y;
    a[4 * q + 2] = v.z;
    a[4 * q + 3] = v.w;
  }
}

// W [K][32 NT] row-major -> fragment order (K a multiple of 8)
template <int NT>
__device__ __forceinline__ void load_fragments(float* __restrict__ Wf, const float* __restrict__ W, int K) {
  constexpr int NC = 32 * NT;
  const int total = K / 2 * 64 * NT;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int ct = idx % NT;
    const int l = (idx / NT) & 63;
    const int kk = idx / (NT * 64);
    Wf[idx] = W[(size_t)kcol(kk, l >> 5) * NC + ct * 32 + (l & 31)];
  }
}

template <int NT>
__device__ __forceinline__ void read_fragment(const float* __restrict__ Wf, int kk, int lane, float (&b)[NT]) {
  const float* p = Wf + (kk * 64 + lane) * NT;
  if constexpr (NT == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
  } else if constexpr (NT == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    b[0] = v.x, b[1] = v.y;
  } else {
    b[0] = *p;
  }
}

// acc[NT tiles] += A[32 x 2 KS] @ Wf[k-steps kbase .. kbase + KS). As fusion_mfma.hip's mfma_half: the fragments of
// k-step kk + 1 are requested before the MFMAs of kk and a scheduling barrier closes every k-step, so two fragment
// sets are live (left alone the scheduler hoists every read and spills).
template <int KS, int NT>
__device__ __forceinline__ void mfma_part(f32x16 (&acc)[NT], const float (&a)[KS], const float* __restrict__ Wf, int kbase,
                                          int lane) {
  float cur[NT], nxt[NT];
  read_fragment<NT>(Wf, kbase, lane, cur);
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    if (kk + 1 < KS) read_fragment<NT>(Wf, kbase + kk + 1, lane, nxt);
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], cur[ct], acc[ct], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) cur[ct] = nxt[ct];
  }
}

__device__ __forceinline__ void wave_release_acquire() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// SAVE: training forward — also stores gates [n, t, 2D] (r | u after the sigmoid) and cand [n, t, D] (c after the tanh).
template <int D, bool SAVE>
__global__ __launch_bounds__(kBlock, 1) void gru_fwd_kernel(
    const float* __restrict__ x, int64_t ld_n, int64_t ld_t, int64_t n, int t, const float* __restrict__ Wg,
    const float* __restrict__ bg, const float* __restrict__ Wc, const float* __restrict__ bc,
    const float* __restrict__ drop, float* __restrict__ h_out, int64_t ld_h, float* __restrict__ gates_out,
    float* __restrict__ cand_out, int64_t n_tiles) {
  constexpr int HT = D / 32;        // hidden-unit tiles = column tiles of the candidate product
  constexpr int GT = 2 * HT;        // column tiles of the gate product (r | u)
  constexpr int KS = D / 2;         // k-steps per operand half
  constexpr int LPR = D / 4;        // lanes per row in the coalesced fill
  constexpr int RPI = kWave / LPR;  // rows per fill instruction
  constexpr int NFILL = kRowsPerWave / RPI;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Wgf = lds;                    // 2D x 2D floats
  float* Wcf = lds + 2 * D * 2 * D;    // 2D x D floats
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // ONE private [32][D] tile per wave, used in turn by x_s, r.h and h': every read of it lands in registers before the
  // next writer is reached in program order (x_s is read ahead of the products, whose results the r.h writes need), so a
  // second tile would remove no wait.
  float* stage = lds + 2 * D * 3 * D + wave * (kRowsPerWave * D);
  const int ai = lane & 31, kh = lane >> 5;   // A layout: row, k parity
  const int cj = lane & 31, rh = lane >> 5;   // C layout: column, row half

  load_fragments<GT>(Wgf, Wg, 2 * D);
  load_fragments<HT>(Wcf, Wc, 2 * D);
  __syncthreads();

  float bgk[GT], bck[HT];
#pragma unroll
  for (int ct = 0; ct < GT; ++ct) bgk[ct] = -kL2E * bg[ct * 32 + cj];
#pragma unroll
  for (int ct = 0; ct < HT; ++ct) bck[ct] = 2.f * kL2E * bc[ct * 32 + cj];
  const int fr = lane / LPR, fc4 = (lane % LPR) * 4;   // fill: row-in-group, column

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRowsPerBlock + (int64_t)wave * kRowsPerWave;
    if (row0 >= n) continue;  // wave-uniform
    float hc[HT][16];         // the state in the C layout (the blend reads it); a_h is the same state in the A layout
    float a_h[KS];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht)
#pragma unroll
      for (int r = 0; r < 16; ++r) hc[ht][r] = 0.f;

    // Stores and the drop mask go through buffer descriptors: a wave-uniform base, 32-bit lane offsets, rows past n
    // dropped by the hardware range check.
    const int rows_valid = (int)(n - row0 < kRowsPerWave ? n - row0 : kRowsPerWave);
    const auto rs_h = __builtin_amdgcn_make_buffer_rsrc(h_out + row0 * ld_h, 0, rows_valid * (int)ld_h * 4, 0x00020000);
    const auto rs_g = __builtin_amdgcn_make_buffer_rsrc(SAVE ? gates_out + row0 * t * 2 * D : h_out, 0,
                                                        SAVE ? rows_valid * t * 2 * D * 4 : 0, 0x00020000);
    const auto rs_c = __builtin_amdgcn_make_buffer_rsrc(SAVE ? cand_out + row0 * t * D : h_out, 0,
                                                        SAVE ? rows_valid * t * D * 4 : 0, 0x00020000);
    const auto rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(drop ? drop + row0 * t * D : x), 0,
                                                        drop ? rows_valid * t * D * 4 : 0, 0x00020000);
    float4 xr[NFILL];
    auto fetch_x = [&](int ts) {
#pragma unroll
      for (int q = 0; q < NFILL; ++q) {
        const int64_t row = row0 + q * RPI + fr;
        xr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) xr[q] = *reinterpret_cast<const float4*>(x + row * ld_n + (int64_t)ts * ld_t + fc4);
      }
    };
    fetch_x(0);

    for (int ts = 0; ts < t; ++ts) {
      // lane-derived LDS offsets are recomputed every step (see lstm_fwd_mfma_kernel: hoisted, they spill)
      int ai_ = ai, kh_ = kh, cj_ = cj, rh_ = rh, fr_ = fr, fc4_ = fc4;
      asm volatile("" : "+v"(ai_), "+v"(kh_), "+v"(cj_), "+v"(rh_), "+v"(fr_), "+v"(fc4_));

      // ---- x_s through the tile into the A layout ---------------------------------------------
      float a_x[KS];
#pragma unroll
      for (int q = 0; q < NFILL; ++q) *tile_vec<D>(stage, q * RPI + fr_, fc4_ >> 2) = xr[q];
      wave_release_acquire();
      read_a_operand<D>(stage, ai_, kh_, a_x);
      if (ts + 1 < t) fetch_x(ts + 1);  // in flight under the MFMAs below

      // ---- x_s Wc[0:D] (needs no r), then [x_s | h] Wg ------------------------------------------
      f32x16 acc_c[HT], acc_g[GT];
#pragma unroll
      for (int ct = 0; ct < HT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_c[ct][r] = 0.f;
#pragma unroll
      for (int ct = 0; ct < GT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_g[ct][r] = 0.f;
      mfma_part<KS, HT>(acc_c, a_x, Wcf, 0, lane);
      mfma_part<KS, GT>(acc_g, a_x, Wgf, 0, lane);
      if (ts > 0) mfma_part<KS, GT>(acc_g, a_h, Wgf, KS, lane);   // zero state: both recurrent halves contribute nothing

      // ---- r, u in the C layout; r.h back into the tile -------------------------------------------
      __builtin_amdgcn_wave_barrier();
      float u[HT][16];
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float sr = sigmoid_kb(acc_g[ht][r], bgk[ht]);
          u[ht][r] = sigmoid_kb(acc_g[HT + ht][r], bgk[HT + ht]);
          const int row = crow(r, rh_);
          const int col = ht * 32 + cj_;
          if (ts > 0) *tile_elem<D>(stage, row, col) = sr * hc[ht][r];
          if (SAVE) {
            const int go = (row * t + ts) * 2 * D + col;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, sr), rs_g, go * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, u[ht][r]), rs_g, (go + D) * 4, 0, 0);
          }
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (ts > 0) {
        float a_rh[KS];
        wave_release_acquire();
        read_a_operand<D>(stage, ai_, kh_, a_rh);
        mfma_part<KS, HT>(acc_c, a_rh, Wcf, KS, lane);
        __builtin_amdgcn_wave_barrier();
      }

      // ---- c, the blend, h' into the tile for the next step --------------------------------------
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float cv = tanh_kb(acc_c[ht][r], bck[ht]);
          const float hn = fmaf(u[ht][r], hc[ht][r] - cv, cv);   // u h + (1 - u) c
          hc[ht][r] = hn;
          const int row = crow(r, rh_);
          const int col = ht * 32 + cj_;
          *tile_elem<D>(stage, row, col) = hn;
          const int e_td = (row * t + ts) * D + col;   // element (row, ts, col) of an [n, t, D] tensor from the tile's first row
          if (SAVE) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, cv), rs_c, e_td * 4, 0, 0);
          float hv = hn;
          if (drop) hv *= __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_d, e_td * 4, 0, 0));
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, hv), rs_h, (row * (int)ld_h + ts * D + col) * 4, 0, 0);
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
      wave_release_acquire();
      if (ts + 1 < t) read_a_operand<D>(stage, ai_, kh_, a_h);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- the per-step route: element-wise halves of a step around dense.hip's products ---------------
// scratch [n, 3d]: columns [0, 2d) hold the gate pre-activations (bias added by the product).
// -> r | u = sigmoid: u stays in [d, 2d), r.h_prev goes to [0, d) (the candidate product's operand; h_prev NULL at
// step 0: nothing written), both go to gates_s (row stride ld_g) when that is given.
__global__ __launch_bounds__(kBlock) void gru_gate_step_kernel(float* __restrict__ scratch, const float* __restrict__ h_prev,
                                                               int64_t ld_h, float* __restrict__ gates_s, int64_t ld_g,
                                                               int64_t n, int d) {
  const int d4 = d / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * d4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / d4;
    const int c = (int)(i % d4) * 4;
    float* s = scratch + row * 3 * d + c;
    const float4 pr = *reinterpret_cast<const float4*>(s), pu = *reinterpret_cast<const float4*>(s + d);
    const float4 r = make_float4(sigmoid_kb(pr.x, 0.f), sigmoid_kb(pr.y, 0.f), sigmoid_kb(pr.z, 0.f), sigmoid_kb(pr.w, 0.f));
    const float4 u = make_float4(sigmoid_kb(pu.x, 0.f), sigmoid_kb(pu.y, 0.f), sigmoid_kb(pu.z, 0.f), sigmoid_kb(pu.w, 0.f));
    *reinterpret_cast<float4*>(s + d) = u;
    if (h_prev) {
      const float4 hp = *reinterpret_cast<const float4*>(h_prev + row * ld_h + c);
      *reinterpret_cast<float4*>(s) = make_float4(r.x * hp.x, r.y * hp.y, r.z * hp.z, r.w * hp.w);
    }
    if (gates_s) {
      *reinterpret_cast<float4*>(gates_s + row * ld_g + c) = r;
      *reinterpret_cast<float4*>(gates_s + row * ld_g + d + c) = u;
    }
  }
}

// scratch columns [2d, 3d) hold the candidate pre-activations, [d, 2d) u. c = tanh, h' = u h_prev + (1 - u) c.
// h is [n, t, d] with node stride ld_h: h' goes to step ts UN-dropped, because step ts + 1 reads it as its state;
// this launch therefore scales the previous step's h by its mask (drop [n, t, d] dense), which no later launch reads,
// and the last step scales its own.
__global__ __launch_bounds__(kBlock) void gru_blend_step_kernel(const float* __restrict__ scratch, float* __restrict__ h,
                                                                int64_t ld_h, const float* __restrict__ drop,
                                                                float* __restrict__ cand, int64_t n, int t, int d, int ts) {
  const int d4 = d / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * d4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / d4;
    const int c = (int)(i % d4) * 4;
    const float* s = scratch + row * 3 * d + c;
    const float4 u = *reinterpret_cast<const float4*>(s + d), pc = *reinterpret_cast<const float4*>(s + 2 * d);
    const float4 cv = make_float4(tanh_kb(pc.x, 0.f), tanh_kb(pc.y, 0.f), tanh_kb(pc.z, 0.f), tanh_kb(pc.w, 0.f));
    float* hs = h + row * ld_h + (int64_t)ts * d + c;
    const int64_t e_td = (row * t + ts) * d + c;
    float4 hp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ts > 0) {
      hp = *reinterpret_cast<const float4*>(hs - d);
      if (drop) {
        const float4 m = *reinterpret_cast<const float4*>(drop + e_td - d);
        *reinterpret_cast<float4*>(hs - d) = make_float4(hp.x * m.x, hp.y * m.y, hp.z * m.z, hp.w * m.w);
      }
    }
    float4 hn = make_float4(fmaf(u.x, hp.x - cv.x, cv.x), fmaf(u.y, hp.y - cv.y, cv.y), fmaf(u.z, hp.z - cv.z, cv.z),
                            fmaf(u.w, hp.w - cv.w, cv.w));
    if (cand) *reinterpret_cast<float4*>(cand + e_td) = cv;
    if (drop && ts == t - 1) {
      const float4 m = *reinterpret_cast<const float4*>(drop + e_td);
      hn = make_float4(hn.x * m.x, hn.y * m.y, hn.z * m.z, hn.w * m.w);
    }
    *reinterpret_cast<float4*>(hs) = hn;
  }
}

// ---- backward, step ts: the element-wise halves around the two dense products -------
// dh = dh_ext[:, ts] (. drop) + dh_rec -> da_c = dh (1 - u)(1 - c^2), du = dh (h_prev - c), dh_u = dh u
__global__ __launch_bounds__(kBlock) void gru_bwd_cand_kernel(const float* __restrict__ gates, const float* __restrict__ cand,
                                                              const float* __restrict__ h, const float* __restrict__ dh_ext,
                                                              int64_t ld_dhe, const float* __restrict__ drop,
                                                              const float* __restrict__ dh_rec, int64_t ld_dhr,
                                                              float* __restrict__ da_c, float* __restrict__ du,
                                                              float* __restrict__ dh_u, int64_t n, int t, int d, int ts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * d; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / d;
    const int c = (int)(i % d);
    const int64_t e_td = (row * t + ts) * d + c;
    float dh = dh_ext[row * ld_dhe + (int64_t)ts * d + c];
    if (drop) dh *= drop[e_td];
    if (dh_rec) dh += dh_rec[row * ld_dhr + c];
    const float u = gates[(row * t + ts) * 2 * d + d + c];
    const float cv = cand[e_td];
    const float hp = ts > 0 ? h[e_td - d] : 0.f;
    da_c[i] = dh * (1.f - u) * (1.f - cv * cv);
    du[i] = dh * (hp - cv);
    dh_u[i] = dh * u;
  }
}

// d_rh [n, d] (row stride ld_drh) holds d(r.h_prev) on entry and dh_rec' = dh_u + d(r.h_prev) r on return;
// da_g [n, 2d] = [d(r.h_prev) h_prev r (1 - r) | du u (1 - u)]; rh [n, d] (nullable) = r.h_prev, the operand of the
// candidate kernel's recurrent weight gradient.
__global__ __launch_bounds__(kBlock) void gru_bwd_gates_kernel(const float* __restrict__ gates, const float* __restrict__ h,
                                                               const float* __restrict__ du, const float* __restrict__ dh_u,
                                                               float* __restrict__ d_rh, int64_t ld_drh,
                                                               float* __restrict__ da_g, float* __restrict__ rh, int64_t n,
                                                               int t, int d, int ts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * d; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / d;
    const int c = (int)(i % d);
    const float* g = gates + (row * t + ts) * 2 * d + c;
    const float r = g[0], u = g[d];
    const float hp = ts > 0 ? h[(row * t + ts - 1) * d + c] : 0.f;
    const float drh = d_rh[row * ld_drh + c];
    da_g[row * 2 * d + c] = drh * hp * r * (1.f - r);
    da_g[row * 2 * d + d + c] = du[i] * u * (1.f - u);
    d_rh[row * ld_drh + c] = fmaf(drh, r, dh_u[i]);
    if (rh) rh[i] = r * hp;
  }
}

int grid_for(int64_t work) {
  const int64_t blocks = (work + kBlock - 1) / kBlock;
  return (int)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

struct GruArgs {
  sagnn::SeqView x;
  const float *Wg, *bg, *Wc, *bc, *drop;
  float* h;
  int64_t ld_h;
  float *gates, *cand;
};

template <int D, bool SAVE>
int launch_gru_fused(const GruArgs& a, hipStream_t s) {
  const sagnn::SeqView& v = a.x;
  const size_t lds = (size_t)(2 * D * 3 * D + 4 * kRowsPerWave * D) * sizeof(float);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&gru_fwd_kernel<D, SAVE>), lds)) return rc;
  const int cus = sagnn::cu_count_current();
  const int64_t n_tiles = (v.n + kRowsPerBlock - 1) / kRowsPerBlock;
  const int64_t blocks = n_tiles < cus ? n_tiles : cus;
  sagnn::ProfileScope prof(sagnn::kProfLstm, s, v.n, v.t);
  hipLaunchKernelGGL((gru_fwd_kernel<D, SAVE>), dim3((unsigned)blocks), dim3(kBlock), lds, s, v.x, v.ld_n, v.ld_t, v.n, v.t, a.Wg,
                     a.bg, a.Wc, a.bc, a.drop, a.h, a.ld_h, a.gates, a.cand, n_tiles);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

int gru_fwd_fused(const GruArgs& a, hipStream_t s) {
  const bool save = a.gates != nullptr;
  // 32-row tiles are addressed with 32-bit byte offsets from a per-tile base
  if (a.x.ld_n >= (1 << 24) || a.ld_h >= (1 << 24) || (int64_t)a.x.t * a.x.d >= (1 << 19))
    return sagnn::fail(SAGNN_ERR_ARG, "fused GRU: row strides must stay below 2^24 floats");
  if (a.x.d == 64) return save ? launch_gru_fused<64, true>(a, s) : launch_gru_fused<64, false>(a, s);
  return save ? launch_gru_fused<32, true>(a, s) : launch_gru_fused<32, false>(a, s);
}

int gru_fwd_steps(const GruArgs& a, float* scratch, hipStream_t s) {
  const sagnn::SeqView& v = a.x;
  const int d = v.d;
  const int64_t n = v.n, lds = 3 * (int64_t)d;
  sagnn::ProfileScope prof(sagnn::kProfLstm, s, n, v.t);
  const int grid = grid_for(n * (d / 4));
  for (int ts = 0; ts < v.t; ++ts) {
    const float* xs = v.x + (int64_t)ts * v.ld_t;
    const float* hp = ts > 0 ? a.h + (int64_t)(ts - 1) * d : nullptr;   // un-dropped until this step's blend has read it
    if (int rc = sagnn::dense_nn_any(xs, v.ld_n, n, d, 2 * d, a.Wg, 2 * d, a.bg, scratch, lds, 0, s)) return rc;
    if (hp)
      if (int rc = sagnn::dense_nn_any(hp, a.ld_h, n, d, 2 * d, a.Wg + (size_t)d * 2 * d, 2 * d, nullptr, scratch, lds, 1, s)) return rc;
    hipLaunchKernelGGL(gru_gate_step_kernel, dim3(grid), dim3(kBlock), 0, s, scratch, hp, a.ld_h,
                       a.gates ? a.gates + (int64_t)ts * 2 * d : nullptr, (int64_t)v.t * 2 * d, n, d);
    SAGNN_HIP_TRY(hipGetLastError());
    if (int rc = sagnn::dense_nn_any(xs, v.ld_n, n, d, d, a.Wc, d, a.bc, scratch + 2 * d, lds, 0, s)) return rc;
    if (hp)
      if (int rc = sagnn::dense_nn_any(scratch, lds, n, d, d, a.Wc + (size_t)d * d, d, nullptr, scratch + 2 * d, lds, 1, s)) return rc;
    hipLaunchKernelGGL(gru_blend_step_kernel, dim3(grid), dim3(kBlock), 0, s, scratch, a.h, a.ld_h, a.drop, a.cand, n, v.t, d, ts);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  return SAGNN_OK;
}

bool fused_d(int d) { return d == 32 || d == 64; }

int check_gru_dims(int64_t n, int t, int d) {
  if (n < 0) return sagnn::fail(SAGNN_ERR_ARG, "negative count n = %lld", (long long)n);
  if (t < 1 || t > 64) return sagnn::fail(SAGNN_ERR_DIM, "gru: t = %d, need 1 <= t <= 64", t);
  if (d < 32 || d > 256 || (d & 31)) return sagnn::fail(SAGNN_ERR_DIM, "gru: d = %d, need a multiple of 32 with 32 <= d <= 256", d);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_gru_fused_supported(int d) { return fused_d(d) ? 1 : 0; }

extern "C" size_t sagnn_gru_workspace_bytes(int64_t n, int t, int d) {
  if (n <= 0 || t <= 0 || d <= 0 || fused_d(d)) return 0;
  return (size_t)n * 3 * (size_t)d * sizeof(float);
}

extern "C" int sagnn_gru_fwd_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, const float* Wg,
                                 const float* bg, const float* Wc, const float* bc, const float* drop_scale, float* h,
                                 int64_t ld_h, float* gates, float* cand, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (int rc = check_gru_dims(n, t, d)) return rc;
  if (!x || !Wg || !bg || !Wc || !bc || !h) return sagnn::fail(SAGNN_ERR_NULL, "gru_fwd: null pointer");
  if ((gates == nullptr) != (cand == nullptr)) return sagnn::fail(SAGNN_ERR_NULL, "gru_fwd: null pointer (give both gates and cand or neither)");
  if (gates && drop_scale) return sagnn::fail(SAGNN_ERR_ARG, "gru_fwd: the training form stores h un-dropped, drop_scale must be NULL");
  const sagnn::SeqView v{x, ld_n, ld_t, n, t, d};
  if (!v.vec() || !sagnn::aligned16(h) || (ld_h & 3) || !sagnn::aligned16(Wg) || !sagnn::aligned16(Wc) ||
      (drop_scale && !sagnn::aligned16(drop_scale)) || (gates && (!sagnn::aligned16(gates) || !sagnn::aligned16(cand))))
    return sagnn::fail(SAGNN_ERR_ALIGN, "gru_fwd: pointers and strides must be 16-byte aligned");
  if (ld_n < d || ld_t < d) return sagnn::fail(SAGNN_ERR_ARG, "gru_fwd: ld_n / ld_t smaller than d = %d", d);
  if (ld_h < (int64_t)t * d) return sagnn::fail(SAGNN_ERR_ARG, "gru_fwd: ld_h smaller than t*d");
  if (n == 0) return SAGNN_OK;
  const GruArgs a{v, Wg, bg, Wc, bc, drop_scale, h, ld_h, gates, cand};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (fused_d(d)) return gru_fwd_fused(a, s);
  const size_t need = sagnn_gru_workspace_bytes(n, t, d);
  if (!workspace || workspace_bytes < need) return sagnn::fail(SAGNN_ERR_WORKSPACE, "gru_fwd workspace needs %zu bytes", need);
  if (!sagnn::aligned16(workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "gru_fwd: workspace must be 16-byte aligned");
  return gru_fwd_steps(a, static_cast<float*>(workspace), s);
}

static int check_bwd_step(const char* who, int64_t n, int t, int d, int ts) {
  if (n < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count n = %lld", who, (long long)n);
  if (t < 1 || d < 4 || d > 256 || (d & 3) || ts < 0 || ts >= t)
    return sagnn::fail(SAGNN_ERR_DIM, "%s: bad t = %d / d = %d / ts = %d", who, t, d, ts);
  return SAGNN_OK;
}

extern "C" int sagnn_gru_bwd_cand_f32(const float* gates, const float* cand, const float* h, const float* dh_ext,
                                      int64_t ld_dhe, const float* drop_scale, const float* dh_rec, int64_t ld_dhr,
                                      float* da_c, float* du, float* dh_u, int64_t n, int t, int d, int ts, void* stream) {
  if (int rc = check_bwd_step("gru_bwd_cand", n, t, d, ts)) return rc;
  if (!gates || !cand || !h || !dh_ext || !da_c || !du || !dh_u) return sagnn::fail(SAGNN_ERR_NULL, "gru_bwd_cand: null pointer");
  if (ld_dhe < (int64_t)t * d) return sagnn::fail(SAGNN_ERR_ARG, "gru_bwd_cand: ld_dhe smaller than t*d");
  if (dh_rec && ld_dhr < d) return sagnn::fail(SAGNN_ERR_ARG, "gru_bwd_cand: ld_dhr smaller than d");
  if (n == 0) return SAGNN_OK;
  hipLaunchKernelGGL(gru_bwd_cand_kernel, dim3(grid_for(n * d)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), gates, cand,
                     h, dh_ext, ld_dhe, drop_scale, dh_rec, ld_dhr, da_c, du, dh_u, n, t, d, ts);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_gru_bwd_gates_f32(const float* gates, const float* h, const float* du, const float* dh_u, float* d_rh,
                                       int64_t ld_drh, float* da_g, float* rh, int64_t n, int t, int d, int ts,
                                       void* stream) {
  if (int rc = check_bwd_step("gru_bwd_gates", n, t, d, ts)) return rc;
  if (!gates || !h || !du || !dh_u || !d_rh || !da_g) return sagnn::fail(SAGNN_ERR_NULL, "gru_bwd_gates: null pointer");
  if (ld_drh < d) return sagnn::fail(SAGNN_ERR_ARG, "gru_bwd_gates: ld_drh smaller than d");
  if (n == 0) return SAGNN_OK;
  hipLaunchKernelGGL(gru_bwd_gates_kernel, dim3(grid_for(n * d)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), gates, h, du,
                     dh_u, d_rh, ld_drh, da_g, rh, n, t, d, ts);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
