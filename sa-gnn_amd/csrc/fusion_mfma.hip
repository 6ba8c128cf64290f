// Interval fusion on the matrix cores (gfx950, exact-fp32 MFMA v_mfma_f32_32x32x2_f32).
//
// The two GEMM-shaped stages of reference model.py:135-155 — the BasicLSTMCell gate product
// [x_t | h] @ W[2d,4d] and the three dense layers of MultiHeadSelfAttention — run on MFMA tiles;
// fp32 in / fp32 accumulate is bit-for-bit an fmaf chain, so the 1e-4 parity bar holds (bf16
// would not). Each wavefront owns 32 rows and is independent of the others after the one-off
// weight load: one wave per SIMD, the whole 512-register budget, no block barriers in the loop.
//
//   LDS image of a weight matrix ("fragment order"): for k-step kk, half hf, lane l, e in 0..3:
//       Wf[((kk*HF + hf)*64 + l)*4 + e] = W[kcol(kk, l>>5)][(4hf + e)*32 + (l&31)]
//   so the B operands of 4 column tiles arrive with ONE conflict-free ds_read_b128 per lane.
//   A operands (x_t, h, layer-norm input) are staged per wave in a [32][D] tile whose column is
//   XOR-swizzled with the row, which makes both the row-major fill and the column-strided
//   A-layout read (lane = row) bank-conflict free.
#include "common.h"

// Diagnostic build only (-DSAGNN_STAMPS): per-section cycle sums of the attention kernel, read back
// with sagnn_debug_read_stamps(). Never compiled into the shipped library.
#ifdef SAGNN_STAMPS
__device__ unsigned long long g_stamps[8];
#define STAMP_DECL unsigned long long st_prev = stamp_now(), st_acc[6] = {0, 0, 0, 0, 0, 0}
#define STAMP(i)                         \
  do {                                   \
    const unsigned long long _t = stamp_now(); \
    st_acc[i] += _t - st_prev;           \
    st_prev = _t;                        \
  } while (0)
#define STAMP_FLUSH                                                        \
  do {                                                                     \
    if ((threadIdx.x & 63) == 0)                                           \
      for (int _i = 0; _i < 6; ++_i) atomicAdd(&g_stamps[_i], st_acc[_i]); \
  } while (0)
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#endif

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 waves = one per SIMD
constexpr int kRowsPerWave = 32;
constexpr int kRowsPerBlock = 128;

__device__ __forceinline__ float fast_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-x));
}
__device__ __forceinline__ float fast_tanh(float x) {
  // tanh(x) = 1 - 2/(1 + exp(2x)); saturates cleanly (exp -> inf gives 1, exp -> 0 gives -1)
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x));
}

// row of C/D register r in lane half rh for a 32x32 MFMA tile (cdna_hip_programming.md §3)
__device__ __forceinline__ int crow(int r, int rh) { return (r & 3) + 8 * (r >> 2) + 4 * rh; }

// ---- the per-wave [32][D] staging tile -------------------------------------------------------
// Rows are filled row-major (coalesced float4 from global, or element-wise from the MFMA C layout)
// and read back in the A layout, lane = row, as float4: lane (row, kh) takes columns
// 8q + 4kh .. + 3, the operands of k-steps 4q .. 4q+3. K-STEP ORDER: k-step m = 4q + e therefore
// multiplies column kcol(m, kh) = 8q + 4kh + e; the weight fragments are laid out to match. The
// 16-byte slots of a row are XOR-swizzled with the row so that the 16-lane groups of a
// ds_read_b128 (one row each) and the 32 consecutive columns of an element-wise write all fall
// on distinct banks.
__device__ __forceinline__ int kcol(int m, int kh) { return 8 * (m >> 2) + 4 * kh + (m & 3); }
template <int D>
__device__ __forceinline__ int tile_slot(int row, int slot) {
  constexpr int SL = D / 4;                      // slots per row
  constexpr int RPB = SL >= 16 ? 1 : 16 / SL;    // rows per 256-byte bank row
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
// A operand of all D/2 k-steps for lane (row, kh)
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

// Copies W [K][NC] (row-major, K a multiple of 8, NC a multiple of 128) into fragment order.
template <int NC>
__device__ __forceinline__ void load_weight_fragments(float* __restrict__ Wf,
                                                      const float* __restrict__ W, int K) {
  constexpr int HF = NC / 128;
  const int total = K * NC;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int e = idx & 3;
    const int l = (idx >> 2) & 63;
    const int rest = idx >> 8;
    const int hf = rest % HF;
    const int kk = rest / HF;
    Wf[idx] = W[(size_t)kcol(kk, l >> 5) * NC + (4 * hf + e) * 32 + (l & 31)];
  }
}

// acc[4*HF tiles] += A[32 x 2*KS] @ Wf[k-steps kbase .. kbase+KS), one 32x32x2 MFMA per tile and
// k-step. The B fragments of k-step kk+1 are requested before the MFMAs of k-step kk and a
// scheduling barrier closes every k-step, so exactly two fragment sets are live (left alone the
// scheduler hoists all 2*KS ds_read_b128 and spills).
template <int KS, int HF>
__device__ __forceinline__ void mfma_half(f32x16 (&acc)[4 * HF], const float (&a)[KS],
                                          const float* __restrict__ Wf, int kbase, int lane) {
  float4 cur[HF], nxt[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf)
    cur[hf] = *reinterpret_cast<const float4*>(Wf + ((kbase * HF + hf) * 64 + lane) * 4);
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    if (kk + 1 < KS) {
#pragma unroll
      for (int hf = 0; hf < HF; ++hf)
        nxt[hf] = *reinterpret_cast<const float4*>(Wf + (((kbase + kk + 1) * HF + hf) * 64 + lane) * 4);
    }
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      acc[4 * hf + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], cur[hf].x, acc[4 * hf + 0], 0, 0, 0);
      acc[4 * hf + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], cur[hf].y, acc[4 * hf + 1], 0, 0, 0);
      acc[4 * hf + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], cur[hf].z, acc[4 * hf + 2], 0, 0, 0);
      acc[4 * hf + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], cur[hf].w, acc[4 * hf + 3], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) cur[hf] = nxt[hf];
  }
}

// ---------------------------------------------------------------------------------------------
// LSTM: TF 1.14 BasicLSTMCell over T steps, zero initial state (reference model.py:135-146).
// ---------------------------------------------------------------------------------------------
// SAVE: training forward — additionally stores the gate activations (i | j | f | o after their
// non-linearities) [n, t, 4D] and the cell state [n, t, D] for the backward pass.
template <int D, bool SAVE>
__global__ __launch_bounds__(kBlock, 1) void lstm_fwd_mfma_kernel(
    const float* __restrict__ x, int64_t ld_n, int64_t ld_t, int64_t n, int t,
    const float* __restrict__ W, const float* __restrict__ bias, float forget_bias,
    const float* __restrict__ drop, float* __restrict__ h_out, int64_t ld_h,
    float* __restrict__ gates_out, float* __restrict__ c_out, int64_t n_tiles,
    const float* __restrict__ h_init, int64_t ld_hi, const float* __restrict__ c_init,
    float* __restrict__ c_final) {
  // h_init [n, D] (row stride ld_hi) / c_init [n, D]: state to continue from (NULL = zero state);
  // c_final [n, D]: cell state after the last step (NULL = not wanted). A sequence cut into
  // consecutive calls gives bit-identical results to one call.
  constexpr int NC = 4 * D;        // gate columns
  constexpr int CT = NC / 32;      // column tiles (8 at D=64)
  constexpr int HF = CT / 4;       // b128 reads per k-step
  constexpr int KS = D / 2;        // k-steps per operand half (x or h)
  constexpr int HT = D / 32;       // hidden-unit tiles
  constexpr int LPR = D / 4;       // lanes per row in the coalesced fill
  constexpr int RPI = kWave / LPR; // rows per fill instruction
  constexpr int NFILL = kRowsPerWave / RPI;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Wf = lds;                                            // 2D x 4D floats
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: tile bases stay on the SALU
  float* stage = lds + 2 * D * NC + wave * (kRowsPerWave * D);  // private [32][D]
  const int ai = lane & 31, kh = lane >> 5;                   // A layout: row, k parity
  const int cj = lane & 31, rh = lane >> 5;                   // C layout: column, row half

  load_weight_fragments<NC>(Wf, W, 2 * D);
  __syncthreads();
  STAMP_DECL;

  // Gate non-linearities as exp2(fma(acc, k, k*bias)): the bias add, the forget bias and the
  // log2(e) scaling ride on one fma (VALU work is paid on top of the fp32 MFMAs, not under them).
  // sigmoid(x) = 1 / (1 + 2^(-x log2e)); tanh(x) = 1 - 2 / (1 + 2^(2x log2e)).
  constexpr float kL2E = 1.44269504088896340736f;
  float bcol[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const float b = bias[ct * 32 + cj] + ((ct / HT) == 2 ? forget_bias : 0.f);
    bcol[ct] = ((ct / HT) == 1 ? 2.f * kL2E : -kL2E) * b;   // j gate: tanh; i, f, o: sigmoid
  }
  const int fr = lane / LPR, fc4 = (lane % LPR) * 4;           // fill: row-in-group, column

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kRowsPerBlock + (int64_t)wave * kRowsPerWave;
    if (row0 >= n) continue;  // wave-uniform
    float c[HT][16];
    float a_h[KS];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht)
#pragma unroll
      for (int r = 0; r < 16; ++r) c[ht][r] = 0.f;
    if (h_init) {  // continue from a given state: h through the staging tile into the A layout, c in the C layout
      const int rows_v = (int)(n - row0 < kRowsPerWave ? n - row0 : kRowsPerWave);
#pragma unroll
      for (int q = 0; q < NFILL; ++q) {
        const int r = q * RPI + fr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows_v) v = *reinterpret_cast<const float4*>(h_init + (row0 + r) * ld_hi + fc4);
        *tile_vec<D>(stage, r, fc4 >> 2) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      read_a_operand<D>(stage, ai, kh, a_h);
      __builtin_amdgcn_wave_barrier();
      const auto rs_ci = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(c_init + row0 * D), 0, rows_v * D * 4, 0x00020000);
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          c[ht][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_ci, (crow(r, rh) * D + ht * 32 + cj) * 4, 0, 0));
    }

    // Global traffic of the tile goes through buffer descriptors: a wave-uniform base (SALU), 32-bit
    // lane offsets, and rows past n dropped by the hardware range check — the 64-bit per-element
    // address arithmetic and row predicates this replaces were a third of the gate phase (VALU work
    // is not hidden by the fp32 MFMAs).
    const int rows_valid = (int)(n - row0 < kRowsPerWave ? n - row0 : kRowsPerWave);
    const auto rs_h = __builtin_amdgcn_make_buffer_rsrc(h_out + row0 * ld_h, 0, rows_valid * (int)ld_h * 4, 0x00020000);
    const auto rs_g = __builtin_amdgcn_make_buffer_rsrc(SAVE ? gates_out + row0 * t * NC : h_out, 0,
                                                        SAVE ? rows_valid * t * NC * 4 : 0, 0x00020000);
    const auto rs_c = __builtin_amdgcn_make_buffer_rsrc(SAVE ? c_out + row0 * t * D : h_out, 0,
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

    STAMP(5);
    for (int ts = 0; ts < t; ++ts) {
      // Lane-derived LDS offsets are recomputed every step (a handful of VALU ops against 256+
      // MFMAs): left loop-invariant, the compiler hoists ~100 swizzled addresses out of the
      // step loop and spills them.
      int ai_ = ai, kh_ = kh, cj_ = cj, rh_ = rh, fr_ = fr, fc4_ = fc4;
      asm volatile("" : "+v"(ai_), "+v"(kh_), "+v"(cj_), "+v"(rh_), "+v"(fr_), "+v"(fc4_));

      // ---- stage x_t through LDS into the A layout --------------------------------------
      float a_x[KS];
#pragma unroll
      for (int q = 0; q < NFILL; ++q) *tile_vec<D>(stage, q * RPI + fr_, fc4_ >> 2) = xr[q];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      read_a_operand<D>(stage, ai_, kh_, a_x);
      if (ts + 1 < t) fetch_x(ts + 1);  // in flight under the MFMAs below
      STAMP(0);

      // ---- gates = x_t @ W[0:D] + h @ W[D:2D]  (bias joins in the gate math) -------------
      f32x16 acc[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
      mfma_half<KS, HF>(acc, a_x, Wf, 0, lane);
      STAMP(1);
      if (ts > 0 || h_init)  // zero initial state: the recurrent half contributes nothing at the first step
        mfma_half<KS, HF>(acc, a_h, Wf, KS, lane);
      STAMP(2);

      // ---- gate math in the C layout (columns i | j | f | o, each D wide) ----------------
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float si = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc[ht][r], -kL2E, bcol[ht])));
          const float tj = fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc[HT + ht][r], 2.f * kL2E, bcol[HT + ht]))), 1.f);
          const float sf = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc[2 * HT + ht][r], -kL2E, bcol[2 * HT + ht])));
          const float so = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(acc[3 * HT + ht][r], -kL2E, bcol[3 * HT + ht])));
          const float cn = fmaf(c[ht][r], sf, si * tj);
          const float hn = fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(cn * (2.f * kL2E))), 1.f) * so;
          c[ht][r] = cn;
          const int row = crow(r, rh_);
          const int col = ht * 32 + cj_;
          *tile_elem<D>(stage, row, col) = hn;  // for the next step's A operand
          // element (row, ts, col) of an [n, t, D] tensor, in floats from the tile's first row
          const int e_td = (row * t + ts) * D + col;
          if (SAVE) {
            const int go = (row * t + ts) * NC + col;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, si), rs_g, go * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, tj), rs_g, (go + D) * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, sf), rs_g, (go + 2 * D) * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, so), rs_g, (go + 3 * D) * 4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, cn), rs_c, e_td * 4, 0, 0);
          }
          float hv = hn;
          if (drop) hv *= __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_d, e_td * 4, 0, 0));
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, hv), rs_h, (row * (int)ld_h + ts * D + col) * 4, 0, 0);
          // keep the scheduler from interleaving all 16*HT chains (register pressure)
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
      STAMP(3);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (ts + 1 < t) read_a_operand<D>(stage, ai_, kh_, a_h);
      __builtin_amdgcn_wave_barrier();
      STAMP(4);
    }
    if (c_final) {
      const auto rs_cf = __builtin_amdgcn_make_buffer_rsrc(c_final + row0 * D, 0, rows_valid * D * 4, 0x00020000);
#pragma unroll
      for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, c[ht][r]), rs_cf, (crow(r, rh) * D + ht * 32 + cj) * 4, 0, 0);
    }
  }
  STAMP_FLUSH;
}


// ---------------------------------------------------------------------------------------------
// layer_norm over (T, d) -> Q/K/V dense -> exp attention -> mean over queries
// (reference model.py:152-155, Utils/attention.py:35-45, 55-78), one pass over h.
//
// A wavefront owns NB = 32 / T nodes = NB*T GEMM rows (row m = nb*T + t). The normalisation is
// applied to the A operand in registers (each lane holds half of one row), the three [d, d]
// products run as MFMAs against fragment-ordered weights in LDS, Q/K/V go to a per-wave LDS
// tile, and the T x T attention of each head is evaluated with lane = feature column
// (scores are reduced across the d_k adjacent lanes of a head).
// ---------------------------------------------------------------------------------------------
// Sum over the dk adjacent lanes of a head (dk a power of two). dk <= 4 stays on DPP quad
// permutes; wider heads fall back to ds_bpermute shuffles.
__device__ __forceinline__ float head_sum(float p, int dk) {
  if (dk >= 2) p += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0xB1, 0xF, 0xF, true));
  if (dk >= 4) p += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0x4E, 0xF, 0xF, true));
  for (int off = 4; off < dk; off <<= 1) p += __shfl_xor(p, off);
  return p;
}

// Attention + mean over queries from the per-wave Q|K|V tile (row m = nb*t + ts, row stride QS,
// Q at +0, K at +D, V at +2D). Generic form: lane = feature column; every (tq, s) score is
// reduced across the dk lanes of the head, so each head's exp/normalise work is repeated dk times.
template <int D, int QS>
__device__ __forceinline__ void attention_columns(const float* __restrict__ qkv, int t, int dk,
                                                  int nb_per_wave, int lane, float scale, float inv_t,
                                                  int64_t node0, int64_t n, float* __restrict__ out,
                                                  int64_t ld_out) {
  constexpr int NPP = kWave / D;
  constexpr int NPAR = 4;
  const int col = lane % D;
  const int sub = lane / D;
  for (int nb0 = 0; nb0 < nb_per_wave; nb0 += NPP * NPAR) {
    const float* base[NPAR];
    float o[NPAR];
    bool live[NPAR];
#pragma unroll
    for (int u = 0; u < NPAR; ++u) {
      const int nb = nb0 + u * NPP + sub;
      live[u] = nb < nb_per_wave;
      base[u] = qkv + (live[u] ? nb : 0) * t * QS + col;
      o[u] = 0.f;
    }
    for (int tq = 0; tq < t; ++tq) {
      float qv[NPAR], rs[NPAR], ctx[NPAR];
#pragma unroll
      for (int u = 0; u < NPAR; ++u) {
        qv[u] = base[u][tq * QS];
        rs[u] = 0.f;
        ctx[u] = 0.f;
      }
      for (int s = 0; s < t; ++s) {
        float p[NPAR], vv[NPAR];
#pragma unroll
        for (int u = 0; u < NPAR; ++u) {
          p[u] = qv[u] * base[u][s * QS + D];
          vv[u] = base[u][s * QS + 2 * D];
        }
#pragma unroll
        for (int u = 0; u < NPAR; ++u) p[u] = head_sum(p[u], dk);
#pragma unroll
        for (int u = 0; u < NPAR; ++u) {
          const float e = __expf(p[u] * scale);
          rs[u] += e;
          ctx[u] = fmaf(e, vv[u], ctx[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < NPAR; ++u) o[u] = fmaf(ctx[u], __builtin_amdgcn_rcpf(rs[u] + 1e-8f), o[u]);
    }
#pragma unroll
    for (int u = 0; u < NPAR; ++u) {
      const int64_t node = node0 + nb0 + u * NPP + sub;
      if (live[u] && node < n) out[node * ld_out + col] = o[u] * inv_t;
    }
  }
}

// Head form for d_k = DK in {2, 4}: the DK lanes of a head split the KEY positions (lane c takes
// s = c, c+DK, ...), each computing whole d_k-wide dot products and context vectors from vector
// LDS reads; one DPP reduction of the row sum per query and one of the context per node. Per
// node this is ~T^2/DK score evaluations per lane instead of T^2.
template <int D, int DK, int QS, int NPAR>
__device__ __forceinline__ void attention_heads(const float* __restrict__ qkv, int t, int nb_per_wave,
                                                int lane, float scale, float inv_t, int64_t node0,
                                                int64_t n, float* __restrict__ out, int64_t ld_out) {
  constexpr int NPP = kWave / D;
  typedef float vec __attribute__((ext_vector_type(DK)));
  const int col = lane % D;
  const int sub = lane / D;
  const int c = col % DK;
  const int h0 = col - c;
  for (int nb0 = 0; nb0 < nb_per_wave; nb0 += NPP * NPAR) {
    const float* base[NPAR];
    bool live[NPAR];
    vec o[NPAR];
#pragma unroll
    for (int u = 0; u < NPAR; ++u) {
      const int nb = nb0 + u * NPP + sub;
      live[u] = nb < nb_per_wave;
      base[u] = qkv + (live[u] ? nb : 0) * t * QS + h0;
      o[u] = (vec)(0.f);
    }
    for (int tq = 0; tq < t; ++tq) {
      vec qv[NPAR], ctx[NPAR];
      float rs[NPAR];
#pragma unroll
      for (int u = 0; u < NPAR; ++u) {
        qv[u] = *reinterpret_cast<const vec*>(base[u] + tq * QS) * scale;
        ctx[u] = (vec)(0.f);
        rs[u] = 0.f;
      }
      for (int s = c; s < t; s += DK) {
#pragma unroll
        for (int u = 0; u < NPAR; ++u) {
          const vec kv = *reinterpret_cast<const vec*>(base[u] + s * QS + D);
          const vec vv = *reinterpret_cast<const vec*>(base[u] + s * QS + 2 * D);
          float p = qv[u][0] * kv[0];
#pragma unroll
          for (int k = 1; k < DK; ++k) p = fmaf(qv[u][k], kv[k], p);
          const float e = __expf(p);
          rs[u] += e;
          ctx[u] += e * vv;
        }
      }
#pragma unroll
      for (int u = 0; u < NPAR; ++u) {
        const float inv = __builtin_amdgcn_rcpf(head_sum(rs[u], DK) + 1e-8f);
        o[u] += ctx[u] * inv;
      }
    }
#pragma unroll
    for (int u = 0; u < NPAR; ++u) {
      float r = 0.f;
#pragma unroll
      for (int k = 0; k < DK; ++k) {
        const float tot = head_sum(o[u][k], DK);
        r = (c == k) ? tot : r;
      }
      const int64_t node = node0 + nb0 + u * NPP + sub;
      if (live[u] && node < n) out[node * ld_out + col] = r * inv_t;
    }
  }
}

// Pair form for a compile-time T <= 8: one lane owns one (node, head) pair outright — Q, K, V of
// the pair (T d_k-vectors each) are read once with vector LDS loads, the T x T scores, their
// normalisers and the context run with no cross-lane traffic, and the d_k outputs leave as one
// vector store. With few intervals the head-split form above leaves lanes idle (T = 2, d_k = 4:
// half of them) and serialises on LDS round trips; this form costs ~T^2 (d_k + 2) VALU per pair.
template <int D, int DK, int QS, int T>
__device__ __forceinline__ void attention_pairs(const float* __restrict__ qkv, int nb_per_wave, int lane,
                                                float scale, float inv_t, int64_t node0, int64_t n,
                                                float* __restrict__ out, int64_t ld_out) {
  constexpr int H = D / DK;
  typedef float vec __attribute__((ext_vector_type(DK)));
  const int pairs = nb_per_wave * H;
  for (int p = lane; p < pairs; p += kWave) {
    const int nb = p / H, hd = p - nb * H;
    const float* base = qkv + nb * T * QS + hd * DK;
    vec q[T], k[T], v[T];
#pragma unroll
    for (int ts = 0; ts < T; ++ts) {
      q[ts] = *reinterpret_cast<const vec*>(base + ts * QS) * scale;
      k[ts] = *reinterpret_cast<const vec*>(base + ts * QS + D);
      v[ts] = *reinterpret_cast<const vec*>(base + ts * QS + 2 * D);
    }
    vec o = (vec)(0.f);
#pragma unroll
    for (int tq = 0; tq < T; ++tq) {
      vec ctx = (vec)(0.f);
      float rs = 0.f;
#pragma unroll
      for (int s = 0; s < T; ++s) {
        float pd = q[tq][0] * k[s][0];
#pragma unroll
        for (int c = 1; c < DK; ++c) pd = fmaf(q[tq][c], k[s][c], pd);
        const float e = __expf(pd);
        rs += e;
        ctx += e * v[s];
      }
      o += ctx * __builtin_amdgcn_rcpf(rs + 1e-8f);
    }
    const int64_t node = node0 + nb;
    if (node < n) *reinterpret_cast<vec*>(out + node * ld_out + hd * DK) = o * inv_t;
  }
}

// Backward of the pair form, in place on the wave's Q|K|V tile: each lane turns the Q, K, V rows of
// its (node, head) pair into dQ, dK, dV given g = dL/d(mean context) / T (Utils/attention.py:35-45
// differentiated; same formulas as attn_bwd_kernel in fusion_bwd.hip):
//   a_qs = e_qs / (R_q + 1e-8), p_s = g . V[s], dz_qs = a_qs (p_s - sum_s' a_qs' p_s'),
//   dQ[q] = scale sum_s dz_qs K[s], dK[s] = scale sum_q dz_qs Q[q], dV[s] = g sum_q a_qs.
template <int D, int DK, int QS, int T>
__device__ __forceinline__ void attention_pairs_bwd(float* __restrict__ qkv, int nb_per_wave, int lane, float scale,
                                                    float inv_t, int64_t node0, int64_t n,
                                                    const float* __restrict__ g_out, int64_t ld_g) {
  constexpr int H = D / DK;
  constexpr int PPL = ((kRowsPerWave / T) * H + kWave - 1) / kWave;   // pairs per lane, at most
  typedef float vec __attribute__((ext_vector_type(DK)));
  const int pairs = nb_per_wave * H;
  // the upstream gradients of ALL my pairs are requested up front: one exposed memory latency per
  // tile instead of one per pair
  vec gpre[PPL];
#pragma unroll
  for (int it = 0; it < PPL; ++it) {
    const int p = lane + it * kWave;
    const int nb = p / H, hd = p - nb * H;
    const int64_t node = node0 + nb;
    gpre[it] = (vec)(0.f);
    if (p < pairs && node < n) gpre[it] = *reinterpret_cast<const vec*>(g_out + node * ld_g + hd * DK);
  }
#pragma unroll 1
  for (int it = 0; it < PPL; ++it) {   // rolled (the body holds 4T vectors); gpre[it] by selects, not scratch
    const int p = lane + it * kWave;
    if (p >= pairs) break;
    const int nb = p / H, hd = p - nb * H;
    float* base = qkv + nb * T * QS + hd * DK;
    vec q[T], k[T], v[T], dk[T];
    float ps[T], asum[T];
    vec g = gpre[0];
#pragma unroll
    for (int c = 1; c < PPL; ++c) g = (it == c) ? gpre[c] : g;
    g *= inv_t;
#pragma unroll
    for (int ts = 0; ts < T; ++ts) {
      q[ts] = *reinterpret_cast<const vec*>(base + ts * QS);
      k[ts] = *reinterpret_cast<const vec*>(base + ts * QS + D);
      v[ts] = *reinterpret_cast<const vec*>(base + ts * QS + 2 * D);
      dk[ts] = (vec)(0.f);
      asum[ts] = 0.f;
      float pd = g[0] * v[ts][0];
#pragma unroll
      for (int c = 1; c < DK; ++c) pd = fmaf(g[c], v[ts][c], pd);
      ps[ts] = pd;
    }
#pragma unroll
    for (int tq = 0; tq < T; ++tq) {
      float a[T];
      float rs = 0.f;
#pragma unroll
      for (int s = 0; s < T; ++s) {
        float z = q[tq][0] * k[s][0];
#pragma unroll
        for (int c = 1; c < DK; ++c) z = fmaf(q[tq][c], k[s][c], z);
        a[s] = __expf(z * scale);
        rs += a[s];
      }
      const float inv = __builtin_amdgcn_rcpf(rs + 1e-8f);
      float dot = 0.f;
#pragma unroll
      for (int s = 0; s < T; ++s) {
        a[s] *= inv;
        dot = fmaf(a[s], ps[s], dot);
      }
      vec dq = (vec)(0.f);
#pragma unroll
      for (int s = 0; s < T; ++s) {
        const float dz = a[s] * (ps[s] - dot);
        dq += dz * k[s];
        dk[s] += dz * q[tq];
        asum[s] += a[s];
      }
      *reinterpret_cast<vec*>(base + tq * QS) = dq * scale;
    }
#pragma unroll
    for (int ts = 0; ts < T; ++ts) {
      *reinterpret_cast<vec*>(base + ts * QS + D) = dk[ts] * scale;
      *reinterpret_cast<vec*>(base + ts * QS + 2 * D) = g * asum[ts];
    }
  }
}

// Head-split form with a compile-time T (a multiple of DK): as attention_heads, but the key and
// value vectors of a lane's positions are read once per node instead of once per query, and every
// loop has a constant trip count.
template <int D, int DK, int QS, int T>
__device__ __forceinline__ void attention_heads_ct(const float* __restrict__ qkv, int nb_per_wave, int lane,
                                                   float scale, float inv_t, int64_t node0, int64_t n,
                                                   float* __restrict__ out, int64_t ld_out) {
  static_assert(T % DK == 0, "T must be a multiple of d_k");
  constexpr int NPP = kWave / D;   // nodes per pass
  constexpr int SPL = T / DK;      // key positions per lane
  typedef float vec __attribute__((ext_vector_type(DK)));
  const int col = lane % D, sub = lane / D;
  const int c = col % DK, h0 = col - c;
  for (int nb0 = 0; nb0 < nb_per_wave; nb0 += NPP) {
    const int nb = nb0 + sub;
    const bool live = nb < nb_per_wave;
    const float* base = qkv + (live ? nb : 0) * T * QS + h0;
    vec kv[SPL], vv[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      kv[i] = *reinterpret_cast<const vec*>(base + (c + i * DK) * QS + D);
      vv[i] = *reinterpret_cast<const vec*>(base + (c + i * DK) * QS + 2 * D);
    }
    vec o = (vec)(0.f);
#pragma unroll 4
    for (int tq = 0; tq < T; ++tq) {
      const vec qv = *reinterpret_cast<const vec*>(base + tq * QS) * scale;
      vec ctx = (vec)(0.f);
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
        float pd = qv[0] * kv[i][0];
#pragma unroll
        for (int k = 1; k < DK; ++k) pd = fmaf(qv[k], kv[i][k], pd);
        const float e = __expf(pd);
        rs += e;
        ctx += e * vv[i];
      }
      o += ctx * __builtin_amdgcn_rcpf(head_sum(rs, DK) + 1e-8f);
    }
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < DK; ++k) {
      const float tot = head_sum(o[k], DK);
      r = (c == k) ? tot : r;
    }
    const int64_t node = node0 + nb;
    if (live && node < n) out[node * ld_out + col] = r * inv_t;
  }
}

template <int TM>
__device__ __forceinline__ void load_square_fragments(float* __restrict__ Wf,
                                                      const float* __restrict__ W, int D) {
  // Wf[(kk*64 + l)*TM + e] = W[kcol(kk, l>>5)][e*32 + (l&31)],  kk < D/2
  const int total = D * D;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int e = idx % TM;
    const int l = (idx / TM) & 63;
    const int kk = idx / (TM * 64);
    Wf[idx] = W[(size_t)kcol(kk, l >> 5) * D + e * 32 + (l & 31)];
  }
}

// TT: number of intervals known at compile time (0 = run-time t): picks the attention form and lets
// the row loops of the normalisation unroll.
// BWD (needs 1 <= TT <= 8): the front of the backward pass instead of the forward tail — the same
// normalisation and Q|K|V tile, then the pair-form attention backward in place on the tile; writes
// dQ|dK|dV [n*t, 3D] (dqkv_out) and the normalised rows y [n*t, D] (y_out, operand of dW = y^T dQKV)
// given g_out = dL/d(out) [n, D] (row stride ld_out); `out` is not written.
template <int D, int TT, bool BWD>
__global__ __launch_bounds__(kBlock, 1) void ln_mhsa_mean_mfma_kernel(
    const float* __restrict__ x, int64_t ld_n, int64_t ld_t, int64_t n, int t_rt, int heads,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int apply_ln,
    const float* __restrict__ Wq, const float* __restrict__ bq, const float* __restrict__ Wk,
    const float* __restrict__ bk, const float* __restrict__ Wv, const float* __restrict__ bv,
    float* __restrict__ out, int64_t ld_out, int64_t n_tiles, const float* __restrict__ g_out,
    float* __restrict__ dqkv_out, float* __restrict__ y_out) {
  static_assert(!BWD || (TT >= 1 && TT <= 8), "backward front needs the pair form");
  constexpr int TM = D / 32;       // 32-column tiles per weight matrix
  constexpr int KS = D / 2;        // k-steps
  constexpr int LPR = D / 4;
  constexpr int RPI = kWave / LPR;
  constexpr int NFILL = kRowsPerWave / RPI;
  // Row stride of the per-wave Q|K|V tile. Head-split forms: +16 B so the rows of one head fall on
  // distinct banks. Pair forms at D = 64: exactly 3D, so that node strides are multiples of a bank
  // row and the 16-lane groups of a ds_read_b128 (lanes {0-3, 12-15, 20-27}, ... = heads of two
  // neighbouring nodes) never meet on a bank (17 % of the LDS cycles were conflicts with 3D + 4).
  constexpr int QS = (D == 64 && TT >= 1 && TT <= 8) ? 3 * D : 3 * D + 4;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Wqf = lds;
  float* Wkf = lds + D * D;
  float* Wvf = lds + 2 * D * D;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* qkv = lds + 3 * D * D + wave * (kRowsPerWave * QS);  // private [32][3D]; its head
  float* stage = qkv;                                         // doubles as the [32][D] fill tile
  const int ai = lane & 31, kh = lane >> 5;
  const int cj = lane & 31, rh = lane >> 5;
  const int fr = lane / LPR, fc4 = (lane % LPR) * 4;

  load_square_fragments<TM>(Wqf, Wq, D);
  load_square_fragments<TM>(Wkf, Wk, D);
  load_square_fragments<TM>(Wvf, Wv, D);
  __syncthreads();

  const int t = TT > 0 ? TT : t_rt;
  const int nb_per_wave = kRowsPerWave / t;      // nodes per wave tile (t <= 32)
  const int rows_used = nb_per_wave * t;
  const int dk = D / heads;
  const float scale = 1.f / sqrtf((float)dk);
  const float inv_td = 1.f / (float)(t * D);
  const float inv_t = 1.f / (float)t;

  float gam[KS], bet[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    gam[kk] = apply_ln ? gamma[kcol(kk, kh)] : 1.f;   // a[kk] is column kcol(kk, kh) of the lane's row
    bet[kk] = apply_ln ? beta[kcol(kk, kh)] : 0.f;
  }
  float bqc[TM], bkc[TM], bvc[TM];
#pragma unroll
  for (int e = 0; e < TM; ++e) {
    bqc[e] = bq[e * 32 + cj];
    bkc[e] = bk[e * 32 + cj];
    bvc[e] = bv[e * 32 + cj];
  }

  float4 xr[NFILL];
  auto fetch_tile = [&](int64_t tile) {
    const int64_t node0 = (tile * 4 + wave) * nb_per_wave;
#pragma unroll
    for (int q = 0; q < NFILL; ++q) {
      const int m = q * RPI + fr;
      const int nb = m / t, ts = m - nb * t;
      const int64_t node = node0 + nb;
      xr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (tile < n_tiles && m < rows_used && node < n)
        xr[q] = *reinterpret_cast<const float4*>(x + node * ld_n + (int64_t)ts * ld_t + fc4);
    }
  };
  fetch_tile(blockIdx.x);

  STAMP_DECL;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t node0 = (tile * 4 + wave) * nb_per_wave;
    if (node0 >= n) {  // wave-uniform; keep the prefetch chain going for later tiles
      fetch_tile(tile + gridDim.x);
      continue;
    }
    STAMP(5);
    int ai_ = ai, kh_ = kh, cj_ = cj, rh_ = rh, fr_ = fr, fc4_ = fc4;
    asm volatile("" : "+v"(ai_), "+v"(kh_), "+v"(cj_), "+v"(rh_), "+v"(fr_), "+v"(fc4_));

    // ---- fill the [32][D] tile: row m = nb*t + ts. xr was fetched one tile ahead -----------
#pragma unroll
    for (int q = 0; q < NFILL; ++q) *tile_vec<D>(stage, q * RPI + fr_, fc4_ >> 2) = xr[q];
    fetch_tile(tile + gridDim.x);  // next tile's rows, in flight under this tile's work
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float a[KS];
    read_a_operand<D>(stage, ai_, kh_, a);
    __builtin_amdgcn_wave_barrier();

    STAMP(0);
    // ---- layer norm on the A operand: moments over the node's t rows x D columns ----------
    if (apply_ln) {
      const int base = (ai_ / t) * t;               // first row of this lane's node
      float ps = 0.f;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) ps += a[kk];
      ps += __shfl_xor(ps, 32);
      float tot = 0.f;
      for (int ts = 0; ts < t; ++ts) tot += __shfl(ps, (base + ts) & 31);
      const float mean = tot * inv_td;
      float pv = 0.f;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const float dl = a[kk] - mean;
        pv = fmaf(dl, dl, pv);
      }
      pv += __shfl_xor(pv, 32);
      float var = 0.f;
      for (int ts = 0; ts < t; ++ts) var += __shfl(pv, (base + ts) & 31);
      const float rstd = rsqrtf(var * inv_td + eps);
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const float inv = rstd * gam[kk];
        a[kk] = a[kk] * inv + (bet[kk] - mean * inv);
      }
    }

    STAMP(1);
    if (BWD && y_out) {
      // normalised rows back through the (now free) fill tile, then out as whole rows: tile row m is
      // global row node0*t + m
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < KS / 4; ++q)
        *tile_vec<D>(stage, ai_, 2 * q + kh_) = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int64_t left = (n - node0) * t;
      const int rows_ok = (int)(left < rows_used ? left : rows_used);
      const auto rs_y = __builtin_amdgcn_make_buffer_rsrc(y_out + node0 * t * D, 0, rows_ok * D * 4, 0x00020000);
#pragma unroll
      for (int q = 0; q < NFILL; ++q) {
        const int m = q * RPI + fr_;
        const float4 yv = *tile_vec<D>(stage, m, fc4_ >> 2);
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 pk = {__builtin_bit_cast(int, yv.x), __builtin_bit_cast(int, yv.y), __builtin_bit_cast(int, yv.z),
                          __builtin_bit_cast(int, yv.w)};
        __builtin_amdgcn_raw_buffer_store_b128(pk, rs_y, (m * D + fc4_) * 4, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();  // tile reads done before the Q|K|V tile overwrites it
    }
    // ---- Q | K | V = A @ W + b ---------------------------------------------------------------
    f32x16 aq[TM], ak[TM], av[TM];
#pragma unroll
    for (int e = 0; e < TM; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // accumulators start at the bias (column = lane in the C layout)
        aq[e][r] = bqc[e];
        ak[e][r] = bkc[e];
        av[e][r] = bvc[e];
      }
    {
      float wq[TM], wk[TM], wv[TM], nq[TM], nk[TM], nv[TM];
#pragma unroll
      for (int e = 0; e < TM; ++e) {
        wq[e] = Wqf[lane * TM + e];
        wk[e] = Wkf[lane * TM + e];
        wv[e] = Wvf[lane * TM + e];
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        if (kk + 1 < KS) {
#pragma unroll
          for (int e = 0; e < TM; ++e) {
            nq[e] = Wqf[((kk + 1) * 64 + lane) * TM + e];
            nk[e] = Wkf[((kk + 1) * 64 + lane) * TM + e];
            nv[e] = Wvf[((kk + 1) * 64 + lane) * TM + e];
          }
        }
#pragma unroll
        for (int e = 0; e < TM; ++e) {
          aq[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], wq[e], aq[e], 0, 0, 0);
          ak[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], wk[e], ak[e], 0, 0, 0);
          av[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], wv[e], av[e], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < TM; ++e) {
          wq[e] = nq[e];
          wk[e] = nk[e];
          wv[e] = nv[e];
        }
      }
    }

    STAMP(2);
    // ---- Q | K | V tile to LDS (C layout -> row major) --------------------------------------
#pragma unroll
    for (int e = 0; e < TM; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* dst = qkv + crow(r, rh_) * QS + e * 32 + cj_;
        dst[0] = aq[e][r];
        dst[D] = ak[e][r];
        dst[2 * D] = av[e][r];
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    STAMP(3);
    // ---- attention per node and head ---------------------------------------------------------
    // NPAR nodes are interleaved for ILP; with few nodes per wave (large t) extra slots are waste
    const bool wide = nb_per_wave >= 4 * (kWave / D);
    if (BWD) {
      constexpr int TB = (TT >= 1 && TT <= 8) ? TT : 1;
      if (dk == 4) attention_pairs_bwd<D, 4, QS, TB>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, g_out, ld_out);
      else attention_pairs_bwd<D, 2, QS, TB>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, g_out, ld_out);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // dQ|dK|dV tile out as whole rows (3D floats each)
      const int64_t left = (n - node0) * t;
      const int rows_ok = (int)(left < rows_used ? left : rows_used);
      const auto rs_q = __builtin_amdgcn_make_buffer_rsrc(dqkv_out + node0 * t * 3 * D, 0, rows_ok * 3 * D * 4, 0x00020000);
      constexpr int V4 = 3 * D / 4;  // float4 per row
      // all 32 tile rows, unrolled (reads batch ahead of the stores); rows past rows_ok fall outside
      // the descriptor and are dropped
#pragma unroll
      for (int k = 0; k < kRowsPerWave * V4 / kWave; ++k) {
        const int i = lane + k * kWave;
        const int m = i / V4, c4 = (i - m * V4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(qkv + m * QS + c4);
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 pk = {__builtin_bit_cast(int, v.x), __builtin_bit_cast(int, v.y), __builtin_bit_cast(int, v.z),
                          __builtin_bit_cast(int, v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(pk, rs_q, (m * 3 * D + c4) * 4, 0, 0);
      }
    } else if (TT >= 1 && TT <= 8 && (dk == 4 || dk == 2)) {
      if (dk == 4) attention_pairs<D, 4, QS, (TT >= 1 && TT <= 8) ? TT : 1>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
      else attention_pairs<D, 2, QS, (TT >= 1 && TT <= 8) ? TT : 1>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    } else if (TT > 8 && dk == 4 && TT % 4 == 0) {
      attention_heads_ct<D, 4, QS, (TT > 8 && TT % 4 == 0) ? TT : 4>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    } else if (TT > 8 && dk == 2 && TT % 2 == 0) {
      attention_heads_ct<D, 2, QS, (TT > 8 && TT % 2 == 0) ? TT : 2>(qkv, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    } else if (dk == 4) {
      if (wide) attention_heads<D, 4, QS, 4>(qkv, t, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
      else attention_heads<D, 4, QS, 2>(qkv, t, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    } else if (dk == 2) {
      if (wide) attention_heads<D, 2, QS, 4>(qkv, t, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
      else attention_heads<D, 2, QS, 2>(qkv, t, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    } else {
      attention_columns<D, QS>(qkv, t, dk, nb_per_wave, lane, scale, inv_t, node0, n, out, ld_out);
    }
    __builtin_amdgcn_wave_barrier();
    STAMP(4);
  }
  STAMP_FLUSH;
}

}  // namespace

namespace sagnn {

template <int D, bool SAVE>
static int launch_lstm_mfma(const LstmArgs& a, hipStream_t s) {
  const SeqView& v = a.x;
  const size_t lds = (size_t)(2 * D * 4 * D + 4 * kRowsPerWave * D) * sizeof(float);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&lstm_fwd_mfma_kernel<D, SAVE>), lds)) return rc;
  const int cus = cu_count_current();
  const int64_t n_tiles = (v.n + kRowsPerBlock - 1) / kRowsPerBlock;
  const int64_t blocks = n_tiles < cus ? n_tiles : cus;
  ProfileScope prof(kProfLstm, s, v.n, v.t);
  hipLaunchKernelGGL((lstm_fwd_mfma_kernel<D, SAVE>), dim3((unsigned)blocks), dim3(kBlock), lds, s, v.x, v.ld_n, v.ld_t, v.n, v.t,
                     a.W, a.b, a.forget_bias, a.drop, a.h, a.ld_h, a.gates, a.cell, n_tiles, a.h_init, a.ld_hi, a.c_init, a.c_final);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

int lstm_fwd_mfma(const LstmArgs& a, hipStream_t s) {
  const bool save = a.gates != nullptr;
  const int d = a.x.d;
  // 32-row tiles are addressed with 32-bit byte offsets from a per-tile base
  if (a.x.ld_n >= (1 << 24) || a.ld_h >= (1 << 24) || (int64_t)a.x.t * d >= (1 << 20))
    return fail(SAGNN_ERR_ARG, "MFMA LSTM: row strides must stay below 2^24 floats");
  if (d == 64) return save ? launch_lstm_mfma<64, true>(a, s) : launch_lstm_mfma<64, false>(a, s);
  if (d == 32) return save ? launch_lstm_mfma<32, true>(a, s) : launch_lstm_mfma<32, false>(a, s);
  return fail(SAGNN_ERR_DIM, "MFMA LSTM supports d = 32 or 64, got %d", d);
}

// Forward (TT = 0: the run-time-t form): writes out [n, d], b is empty. BWD: the front of the backward pass, out NULL.
template <int D, int TT, bool BWD>
static int launch_ln_mhsa_t(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, const AttnBwdOut& b, hipStream_t s) {
  const size_t lds = (size_t)(3 * D * D + 4 * kRowsPerWave * (3 * D + 4)) * sizeof(float);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&ln_mhsa_mean_mfma_kernel<D, TT, BWD>), lds)) return rc;
  const int cus = cu_count_current();
  const int64_t nodes_per_tile = 4 * (kRowsPerWave / v.t);
  const int64_t n_tiles = (v.n + nodes_per_tile - 1) / nodes_per_tile;
  const int64_t blocks = n_tiles < cus ? n_tiles : cus;
  ProfileScope prof(kProfMhsa, s, v.n, v.t);
  // the backward front takes g_out's row stride through the kernel's `ld_out` parameter
  hipLaunchKernelGGL((ln_mhsa_mean_mfma_kernel<D, TT, BWD>), dim3((unsigned)blocks), dim3(kBlock), lds, s, v.x, v.ld_n, v.ld_t,
                     v.n, v.t, a.heads, a.gamma, a.beta, a.eps, a.apply_ln, a.Wq, a.bq, a.Wk, a.bk, a.Wv, a.bv, out,
                     BWD ? b.ld_g : ld_out, n_tiles, b.g_out, b.dqkv, b.y);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

template <int D>
static int ln_mhsa_mean_mfma_d(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, hipStream_t s) {
  int rc;
  const auto launch = [&](auto T) { return launch_ln_mhsa_t<D, decltype(T)::value, false>(v, a, out, ld_out, AttnBwdOut{}, s); };
  if (dispatch_t(v.t, SpecialisedT{}, launch, rc)) return rc;
  return launch(std::integral_constant<int, 0>{});   // any other t: the run-time form
}

// apply_ln = 0: plain MHSA + mean (gamma/beta ignored); 1: layer_norm over (t, d) first.
int ln_mhsa_mean_mfma(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, hipStream_t s) {
  if (v.d == 64) return ln_mhsa_mean_mfma_d<64>(v, a, out, ld_out, s);
  if (v.d == 32) return ln_mhsa_mean_mfma_d<32>(v, a, out, ld_out, s);
  return fail(SAGNN_ERR_DIM, "MFMA attention supports d = 32 or 64, got %d", v.d);
}

// Which calls of sagnn_attn_bwd_front_f32 reach this kernel (select_attn_bwd_front, engine.cpp; tests/test_gpu_bwd_routes.py
// restates the selector and runs every row): d in {32, 64}, t in MfmaBwdFrontT, d_k = d / heads in {2, 4}, behind the
// Split row, which takes 16 heads under every engine but f32.
//
// engine        d    heads   d_k    runs
// ---------------------------------------------------------------------------------------------------------------------
// f32           32   16      2      ln_mhsa_mean_mfma_kernel<32, T, true>, attention_pairs_bwd<32, 2, QS, T>
// f32           64   16      4      ln_mhsa_mean_mfma_kernel<64, T, true>, attention_pairs_bwd<64, 4, QS, T>
// any           32   8       4      ln_mhsa_mean_mfma_kernel<32, T, true>, attention_pairs_bwd<32, 4, QS, T>
// any           64   32      2      ln_mhsa_mean_mfma_kernel<64, T, true>, attention_pairs_bwd<64, 2, QS, T>
// f16x2, valu   32, 64   16         the Split row (attn_split.hip), not this kernel
//
// T in {1, 2, 3, 4, 5, 6, 8}: 2 x 7 x 2 = 28 kernel / branch combinations. min(ceil(n / tile), CUs) blocks, a tile =
// 4 waves x (32 / T) nodes; a wave's (32 / T) * heads (node, head) pairs go over its 64 lanes, so above 64 pairs a lane
// takes its upstream gradient from gpre[1 ..] (every shape at d = 64 / d_k = 2; d_k = 4 at d = 32 up to T = 3; the
// 16-head shapes up to T = 6).
template <int D>
static int attn_bwd_front_mfma_d(const SeqView& v, const AttnParams& a, const AttnBwdOut& b, hipStream_t s) {
  int rc;
  const auto launch = [&](auto T) { return launch_ln_mhsa_t<D, decltype(T)::value, true>(v, a, nullptr, 0, b, s); };
  if (dispatch_t(v.t, MfmaBwdFrontT{}, launch, rc)) return rc;
  return fail(SAGNN_ERR_DIM, "attention backward front: t = %d has no specialised kernel", v.t);
}

// Front of the attention backward pass: y = LN(x) (or x), Q|K|V, attention backward -> dqkv [n*t, 3d], y [n*t, d].
int attn_bwd_front_mfma(const SeqView& v, const AttnParams& a, const AttnBwdOut& b, hipStream_t s) {
  if (v.d == 64) return attn_bwd_front_mfma_d<64>(v, a, b, s);
  if (v.d == 32) return attn_bwd_front_mfma_d<32>(v, a, b, s);
  return fail(SAGNN_ERR_DIM, "attention backward front supports d = 32 or 64, got %d", v.d);
}

}  // namespace sagnn

#ifdef SAGNN_STAMPS
extern "C" int sagnn_debug_read_stamps(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif
