// Interval fusion for gfx950 (reference model.py:135-155): BasicLSTMCell over the T interval
// embeddings of every node, layer-norm over (T, d), multi-head self-attention over T with the
// reference's exp/(sum + 1e-8) normalisation, mean over T.
//
// This file holds the VALU (fp32 FMA) formulation: one thread per (node, hidden unit), weights
// streamed through L2, activations staged in LDS. fusion_mfma.hip holds the MFMA formulation
// of the two GEMM-shaped stages; both are checked against the same oracle.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLstmRowsPerThread = 4;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// TF 1.14 BasicLSTMCell.call (rnn_cell_impl.py): gate_inputs = [x, h] @ W + b;
// i, j, f, o = split(gate_inputs, 4); c' = c*sigmoid(f + forget_bias) + sigmoid(i)*tanh(j);
// h' = tanh(c')*sigmoid(o).
__global__ void lstm_fwd_valu_kernel(const float* __restrict__ x, int64_t ld_n, int64_t ld_t,
                                     int64_t n, int t, int d, const float* __restrict__ W,
                                     const float* __restrict__ b, float forget_bias,
                                     const float* __restrict__ drop, float* __restrict__ h_out,
                                     int64_t ld_h, float* __restrict__ gates_out,
                                     float* __restrict__ c_out, const float* __restrict__ h_init, int64_t ld_hi,
                                     const float* __restrict__ c_init, float* __restrict__ c_final) {
  extern __shared__ float sm[];  // [rows_per_block][2d]: x_t | h
  constexpr int RPT = kLstmRowsPerThread;
  const int j = threadIdx.x % d;
  const int rs = threadIdx.x / d;
  const int slots = blockDim.x / d;
  const int rows_pb = slots * RPT;
  const int64_t row_base = (int64_t)blockIdx.x * rows_pb;
  const int d2 = 2 * d, d4 = 4 * d;

  float c[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int64_t row = row_base + rs * RPT + r;
    c[r] = (c_init && row < n) ? c_init[row * d + j] : 0.f;   // state to continue from (NULL = zero)
  }
  for (int i = threadIdx.x; i < rows_pb * d; i += blockDim.x) {
    const int64_t row = row_base + i / d;
    sm[(i / d) * d2 + d + (i % d)] = (h_init && row < n) ? h_init[row * ld_hi + (i % d)] : 0.f;
  }

  const float b_i = b[j], b_j = b[d + j], b_f = b[2 * d + j], b_o = b[3 * d + j];
  for (int ts = 0; ts < t; ++ts) {
    for (int i = threadIdx.x; i < rows_pb * d; i += blockDim.x) {
      const int r = i / d, k = i % d;
      const int64_t row = row_base + r;
      sm[r * d2 + k] = row < n ? x[row * ld_n + (int64_t)ts * ld_t + k] : 0.f;
    }
    __syncthreads();
    float gi[RPT], gj[RPT], gf[RPT], go[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      gi[r] = 0.f;
      gj[r] = 0.f;
      gf[r] = 0.f;
      go[r] = 0.f;
    }
    for (int k = 0; k < d2; ++k) {
      const float* wr = W + (int64_t)k * d4 + j;
      const float wi = wr[0], wj = wr[d], wf = wr[2 * d], wo = wr[3 * d];
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const float a = sm[(rs * RPT + r) * d2 + k];
        gi[r] = fmaf(a, wi, gi[r]);
        gj[r] = fmaf(a, wj, gj[r]);
        gf[r] = fmaf(a, wf, gf[r]);
        go[r] = fmaf(a, wo, go[r]);
      }
    }
    __syncthreads();  // every thread has finished reading x_t | h
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int lr = rs * RPT + r;
      const int64_t row = row_base + lr;
      const float si = sigmoidf_(gi[r] + b_i), tj = tanhf(gj[r] + b_j);
      const float sf = sigmoidf_(gf[r] + b_f + forget_bias), so = sigmoidf_(go[r] + b_o);
      const float cn = c[r] * sf + si * tj;
      const float hn = tanhf(cn) * so;
      c[r] = cn;
      sm[lr * d2 + d + j] = hn;
      if (gates_out && row < n) {  // training forward: activations + cell state for the backward pass
        float* gp = gates_out + (row * t + ts) * (int64_t)d4 + j;
        gp[0] = si;
        gp[d] = tj;
        gp[2 * d] = sf;
        gp[3 * d] = so;
        c_out[(row * t + ts) * (int64_t)d + j] = cn;
      }
      if (row < n) {
        const int64_t o = row * ld_h + (int64_t)ts * d + j;
        h_out[o] = drop ? hn * drop[row * (int64_t)t * d + (int64_t)ts * d + j] : hn;
      }
    }
  }
  if (c_final) {
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t row = row_base + rs * RPT + r;
      if (row < n) c_final[row * d + j] = c[r];
    }
  }
}

// tf.contrib.layers.layer_norm(begin_norm_axis=1, begin_params_axis=-1): moments over (t, d),
// then tf.nn.batch_normalization: inv = rsqrt(var + eps) * gamma; y = x*inv + (beta - mean*inv).
// One wavefront per node.
// x and y may alias (in-place): each element is read and written by the same lane.
__global__ void layernorm_td_kernel(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                    const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float eps, float* y,
                                    int64_t ld_y) {
  const int lane = threadIdx.x & 63;
  const int64_t node = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (node >= n) return;
  const int td = t * d;
  const float* xr = x + node * ld_n;
  // element i = (ts, k) of the node sits at ts*ld_t + k in x and at i in the dense output
  float s = 0.f;
  for (int i = lane; i < td; i += 64) s += xr[(int64_t)(i / d) * ld_t + (i % d)];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float mean = s / (float)td;
  float v = 0.f;
  for (int i = lane; i < td; i += 64) {
    const float dlt = xr[(int64_t)(i / d) * ld_t + (i % d)] - mean;
    v = fmaf(dlt, dlt, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const float rstd = rsqrtf(v / (float)td + eps);
  float* yr = y + node * ld_y;
  for (int i = lane; i < td; i += 64) {
    const int k = i % d;
    const float inv = rstd * gamma[k];
    yr[i] = xr[(int64_t)(i / d) * ld_t + k] * inv + (beta[k] - mean * inv);
  }
}

// MultiHeadSelfAttention.attention + reduce_mean over the query axis. d threads per node.
__global__ void mhsa_mean_valu_kernel(const float* __restrict__ x, int64_t ld_n, int64_t ld_t,
                                      int64_t n, int t, int d, int heads,
                                      const float* __restrict__ Wq,
                                      const float* __restrict__ bq, const float* __restrict__ Wk,
                                      const float* __restrict__ bk, const float* __restrict__ Wv,
                                      const float* __restrict__ bv, float* __restrict__ out,
                                      int64_t ld_out) {
  extern __shared__ float sm[];  // per slot: y | q | k | v, each [t][d]
  const int j = threadIdx.x % d;
  const int slot = threadIdx.x / d;
  const int slots = blockDim.x / d;
  const int td = t * d;
  float* ys = sm + (size_t)slot * 4 * td;
  float* qs = ys + td;
  float* ks = qs + td;
  float* vs = ks + td;
  const int dk = d / heads;
  const int hoff = (j / dk) * dk;
  const float scale = 1.f / sqrtf((float)dk);

  for (int64_t node0 = (int64_t)blockIdx.x * slots; node0 < n; node0 += (int64_t)gridDim.x * slots) {
    const int64_t node = node0 + slot;
    const bool valid = node < n;
    for (int ts = 0; ts < t; ++ts) ys[ts * d + j] = valid ? x[node * ld_n + (int64_t)ts * ld_t + j] : 0.f;
    __syncthreads();
    for (int ts = 0; ts < t; ++ts) {
      float q = 0.f, k = 0.f, v = 0.f;
      for (int kk = 0; kk < d; ++kk) {
        const float a = ys[ts * d + kk];
        q = fmaf(a, Wq[kk * d + j], q);
        k = fmaf(a, Wk[kk * d + j], k);
        v = fmaf(a, Wv[kk * d + j], v);
      }
      qs[ts * d + j] = q + bq[j];
      ks[ts * d + j] = k + bk[j];
      vs[ts * d + j] = v + bv[j];
    }
    __syncthreads();
    float o = 0.f;
    for (int tq = 0; tq < t; ++tq) {
      float rowsum = 0.f, ctx = 0.f;
      for (int s = 0; s < t; ++s) {
        float dot = 0.f;
        for (int c = 0; c < dk; ++c) dot = fmaf(qs[tq * d + hoff + c], ks[s * d + hoff + c], dot);
        const float e = expf(dot * scale);
        rowsum += e;
        ctx = fmaf(e, vs[s * d + j], ctx);
      }
      o += ctx / (rowsum + 1e-8f);
    }
    if (valid) out[node * ld_out + j] = o / (float)t;
    __syncthreads();
  }
}


// ---- "wide" attention: any d that is a multiple of 32 (e.g. 128): Q|K|V by the MFMA dense products
// of dense.hip into a [n, t, 3d] buffer, then this per-node kernel. (The LSTM keeps its VALU form
// for such d: an un-fused MFMA composition measured no faster, 37.5 vs 37.2 ms at n = 1M, d = 128,
// T = 6 — the gate round trip through HBM eats the MFMA gain.) ---------------------------------------

// Attention + mean over queries from a Q|K|V buffer [n, t, 3d] (rows as x@W+b produced them).
__global__ void attn_mean_from_qkv_kernel(const float* __restrict__ qkv, int64_t n, int t, int d, int heads,
                                          float* __restrict__ out, int64_t ld_out) {
  extern __shared__ float sm[];
  const int j = threadIdx.x % d;
  const int slot = threadIdx.x / d;
  const int slots = blockDim.x / d;
  const int td = t * d;
  float* qs = sm + (size_t)slot * 3 * td;
  float* ks = qs + td;
  float* vs = ks + td;
  const int dk = d / heads;
  const int hoff = (j / dk) * dk;
  const float scale = 1.f / sqrtf((float)dk);
  for (int64_t node0 = (int64_t)blockIdx.x * slots; node0 < n; node0 += (int64_t)gridDim.x * slots) {
    const int64_t node = node0 + slot;
    const bool valid = node < n;
    const float* row = qkv + (valid ? node : 0) * (int64_t)(3 * td);
    for (int ts = 0; ts < t; ++ts) {
      qs[ts * d + j] = row[ts * 3 * d + j];
      ks[ts * d + j] = row[ts * 3 * d + d + j];
      vs[ts * d + j] = row[ts * 3 * d + 2 * d + j];
    }
    __syncthreads();
    float o = 0.f;
    for (int tq = 0; tq < t; ++tq) {
      float rowsum = 0.f, ctx = 0.f;
      for (int s2 = 0; s2 < t; ++s2) {
        float dot = 0.f;
        for (int c = 0; c < dk; ++c) dot = fmaf(qs[tq * d + hoff + c], ks[s2 * d + hoff + c], dot);
        const float e = expf(dot * scale);
        rowsum += e;
        ctx = fmaf(e, vs[s2 * d + j], ctx);
      }
      o += ctx / (rowsum + 1e-8f);
    }
    if (valid) out[node * ld_out + j] = o / (float)t;
    __syncthreads();
  }
}

int check_dims(int64_t n, int t, int d) {
  if (n < 0) return sagnn::fail(SAGNN_ERR_ARG, "n = %lld < 0", (long long)n);
  if (t < 1 || t > 64) return sagnn::fail(SAGNN_ERR_DIM, "t = %d: need 1..64", t);
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "d = %d: need a multiple of 4 in [4, 256]", d);
  return SAGNN_OK;
}

// x[node, ts, :] lives at node*ld_n + ts*ld_t: either [n, t, d] (ld_t = d, ld_n >= t*d) or
// [t, n, d] (ld_n = d, ld_t >= n*d) or any other non-overlapping pair of strides.
int check_strides(int64_t ld_n, int64_t ld_t, int64_t n, int t, int d) {
  if (ld_n < d || ld_t < d) return sagnn::fail(SAGNN_ERR_ARG, "ld_n / ld_t smaller than d");
  const bool node_major = ld_n >= (int64_t)(t - 1) * ld_t + d;
  const bool time_major = ld_t >= (n - 1) * ld_n + d;
  if (!node_major && !time_major && n > 1 && t > 1)
    return sagnn::fail(SAGNN_ERR_ARG, "ld_n = %lld, ld_t = %lld overlap for n = %lld, t = %d",
                       (long long)ld_n, (long long)ld_t, (long long)n, t);
  return SAGNN_OK;
}

using sagnn::AttnParams;
using sagnn::LstmArgs;
using sagnn::SeqView;

int check_heads(int heads, int d) {
  if (heads < 1 || d % heads) return sagnn::fail(SAGNN_ERR_DIM, "heads = %d does not divide d = %d", heads, d);
  return SAGNN_OK;
}

// a weight of the three dense layers is missing, or a layer-norm parameter that apply_ln asks for
bool missing(const AttnParams& a) {
  return !a.Wq || !a.bq || !a.Wk || !a.bk || !a.Wv || !a.bv || (a.apply_ln && (!a.gamma || !a.beta));
}

// The checks of an attention forward entry, in the order its callers rely on: dimensions, heads | d, pointers, strides,
// ld_out. The entries with an order of their own (interval_fusion: workspace before heads; the backward front: shape
// before pointers) call the pieces. rows_out = false: the wide entry, which has never looked at ld_out.
int check_attn_call(const SeqView& v, const AttnParams& a, const float* out, int64_t ld_out, bool rows_out = true) {
  if (int rc = check_dims(v.n, v.t, v.d)) return rc;
  if (int rc = check_heads(a.heads, v.d)) return rc;
  if (!v.x || missing(a) || !out) return sagnn::fail(SAGNN_ERR_NULL, "null tensor pointer");
  if (int rc = check_strides(v.ld_n, v.ld_t, v.n, v.t, v.d)) return rc;
  if (rows_out && ld_out < v.d) return sagnn::fail(SAGNN_ERR_ARG, "ld_out smaller than d");
  return SAGNN_OK;
}

}  // namespace

namespace sagnn {

int lstm_fwd_valu(const LstmArgs& a, hipStream_t s) {
  const SeqView& v = a.x;
  const int d = v.d;
  const int slots = kBlock / d > 0 ? kBlock / d : 1;
  const int threads = slots * d;
  const int rows_pb = slots * kLstmRowsPerThread;
  const int64_t blocks = (v.n + rows_pb - 1) / rows_pb;
  if (blocks > INT32_MAX) return fail(SAGNN_ERR_ARG, "grid too large");
  const size_t lds = (size_t)rows_pb * 2 * d * sizeof(float);
  ProfileScope prof(kProfLstm, s, v.n, v.t);
  hipLaunchKernelGGL(lstm_fwd_valu_kernel, dim3((unsigned)blocks), dim3(threads), lds, s, v.x, v.ld_n, v.ld_t, v.n, v.t, d, a.W,
                     a.b, a.forget_bias, a.drop, a.h, a.ld_h, a.gates, a.cell, a.h_init, a.ld_hi, a.c_init, a.c_final);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

int mhsa_mean_valu(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, hipStream_t s) {
  const int t = v.t, d = v.d;
  int slots = kBlock / d > 0 ? kBlock / d : 1;
  while (slots > 1 && (size_t)slots * 4 * t * d * sizeof(float) > 64 * 1024) slots >>= 1;
  const size_t lds = (size_t)slots * 4 * t * d * sizeof(float);
  if (lds > 160 * 1024) return fail(SAGNN_ERR_DIM, "t*d = %d too large for LDS", t * d);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&mhsa_mean_valu_kernel), lds)) return rc;
  int64_t blocks = (v.n + slots - 1) / slots;
  if (blocks > 8192) blocks = 8192;
  ProfileScope prof(kProfMhsa, s, v.n, t);
  hipLaunchKernelGGL(mhsa_mean_valu_kernel, dim3((unsigned)blocks), dim3(slots * d), lds, s, v.x, v.ld_n, v.ld_t, v.n, t, d,
                     a.heads, a.Wq, a.bq, a.Wk, a.bk, a.Wv, a.bv, out, ld_out);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

// MHSA + mean for any d % 32 == 0: Q|K|V by three MFMA products per interval into ws [n, t, 3d],
// then the per-node attention kernel.
int mhsa_mean_wide(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, float* ws, hipStream_t s) {
  const int64_t n = v.n;
  const int t = v.t, d = v.d;
  ProfileScope prof(kProfMhsa, s, n, t);
  const int64_t ldq = (int64_t)t * 3 * d;
  for (int ts = 0; ts < t; ++ts) {
    const float* xt = v.x + (int64_t)ts * v.ld_t;
    float* qt = ws + (int64_t)ts * 3 * d;
    if (int rc = dense_nn_any(xt, v.ld_n, n, d, d, a.Wq, d, a.bq, qt, ldq, 0, s)) return rc;
    if (int rc = dense_nn_any(xt, v.ld_n, n, d, d, a.Wk, d, a.bk, qt + d, ldq, 0, s)) return rc;
    if (int rc = dense_nn_any(xt, v.ld_n, n, d, d, a.Wv, d, a.bv, qt + 2 * d, ldq, 0, s)) return rc;
  }
  int slots = kBlock / d > 0 ? kBlock / d : 1;
  while (slots > 1 && (size_t)slots * 3 * t * d * sizeof(float) > 64 * 1024) slots >>= 1;
  const size_t lds = (size_t)slots * 3 * t * d * sizeof(float);
  if (lds > 160 * 1024) return fail(SAGNN_ERR_DIM, "t*d = %d too large for LDS", t * d);
  if (int rc = sagnn::ensure_dynamic_lds(reinterpret_cast<const void*>(&attn_mean_from_qkv_kernel), lds)) return rc;
  int64_t blocks = (n + slots - 1) / slots;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(attn_mean_from_qkv_kernel, dim3((unsigned)blocks), dim3(slots * d), lds, s, ws, n, t, d, a.heads,
                     out, ld_out);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

}  // namespace sagnn

extern "C" size_t sagnn_mhsa_wide_workspace_bytes(int64_t n, int t, int d) {
  return (n <= 0 || d <= 0 || t <= 0) ? 0 : (size_t)n * (size_t)t * 3 * (size_t)d * sizeof(float);
}

// sagnn_mhsa_mean_wide_f32 on the structs: interval_fusion and ln_mhsa_mean come here with their normalised rows
static int mhsa_mean_wide_call(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (int rc = check_dims(v.n, v.t, v.d)) return rc;
  if (!sagnn::wide_supported(v.d)) return sagnn::fail(SAGNN_ERR_DIM, "d = %d: the wide path needs a multiple of 32", v.d);
  if (int rc = check_attn_call(v, a, out, ld_out, false)) return rc;
  if (!v.vec()) return sagnn::fail(SAGNN_ERR_ALIGN, "x rows must be 16-byte aligned");
  if (v.n == 0) return SAGNN_OK;
  const size_t need = sagnn_mhsa_wide_workspace_bytes(v.n, v.t, v.d);
  if (!workspace || workspace_bytes < need) return sagnn::fail(SAGNN_ERR_WORKSPACE, "mhsa wide workspace needs %zu bytes", need);
  return sagnn::mhsa_mean_wide(v, a, out, ld_out, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int sagnn_mhsa_mean_wide_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                        int heads, const float* Wq, const float* bq, const float* Wk,
                                        const float* bk, const float* Wv, const float* bv, float* out,
                                        int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream) {
  return mhsa_mean_wide_call({x, ld_n, ld_t, n, t, d}, {heads, nullptr, nullptr, 0.f, 0, Wq, bq, Wk, bk, Wv, bv}, out, ld_out,
                             workspace, workspace_bytes, stream);
}

// The three LSTM forward entries: inference (h_init / c_init / c_final optional) and training (gates / cell saved).
static int lstm_fwd(const LstmArgs& a, bool train, void* stream) {
  const SeqView& v = a.x;
  if (int rc = check_dims(v.n, v.t, v.d)) return rc;
  if (!v.x || !a.W || !a.b || !a.h || (train && (!a.gates || !a.cell))) return sagnn::fail(SAGNN_ERR_NULL, "null tensor pointer");
  if ((a.h_init == nullptr) != (a.c_init == nullptr)) return sagnn::fail(SAGNN_ERR_NULL, "give both h_init and c_init or neither");
  if (int rc = check_strides(v.ld_n, v.ld_t, v.n, v.t, v.d)) return rc;
  if (a.ld_h < (int64_t)v.t * v.d) return sagnn::fail(SAGNN_ERR_ARG, "ld_h smaller than t*d");
  if (a.h_init && a.ld_hi < v.d) return sagnn::fail(SAGNN_ERR_ARG, "ld_hi smaller than d");
  if (v.n == 0) return SAGNN_OK;
  const bool vec = v.vec() && (!a.h_init || (sagnn::aligned16(a.h_init) && (a.ld_hi & 3) == 0));
  const bool h_vec = (a.ld_h & 3) == 0 && sagnn::aligned16(a.h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (sagnn::select_lstm_fwd(sagnn::calling_engine(), v.d, v.t, vec, a.ld_h, h_vec, train, a.drop != nullptr,
                                 !a.drop || sagnn::aligned16(a.drop))) {
    case sagnn::LstmFwd::F16x2: return sagnn::lstm_fwd_f16(a, s);
    case sagnn::LstmFwd::F32Mfma: return sagnn::lstm_fwd_mfma(a, s);
    case sagnn::LstmFwd::Split128: return sagnn::lstm_fwd_split128(a, s);
    default: return sagnn::lstm_fwd_valu(a, s);
  }
}

extern "C" int sagnn_lstm_fwd_state_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                        const float* W, const float* b, float forget_bias,
                                        const float* drop_scale, const float* h_init, int64_t ld_hi,
                                        const float* c_init, float* h, int64_t ld_h, float* c_final, void* stream) {
  return lstm_fwd({{x, ld_n, ld_t, n, t, d}, W, b, forget_bias, drop_scale, h, ld_h, nullptr, nullptr, h_init, ld_hi, c_init,
                   c_final}, false, stream);
}

extern "C" int sagnn_lstm_fwd_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                  const float* W, const float* b, float forget_bias,
                                  const float* drop_scale, float* h, int64_t ld_h, void* stream) {
  return lstm_fwd({{x, ld_n, ld_t, n, t, d}, W, b, forget_bias, drop_scale, h, ld_h, nullptr, nullptr, nullptr, 0, nullptr,
                   nullptr}, false, stream);
}

extern "C" int sagnn_lstm_fwd_train_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                        const float* W, const float* b, float forget_bias,
                                        const float* drop_scale, float* h, int64_t ld_h, float* gates,
                                        float* cell, void* stream) {
  return lstm_fwd({{x, ld_n, ld_t, n, t, d}, W, b, forget_bias, drop_scale, h, ld_h, gates, cell, nullptr, 0, nullptr, nullptr},
                  true, stream);
}

extern "C" int sagnn_layernorm_td_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d,
                                      const float* gamma, const float* beta, float eps, float* y,
                                      int64_t ld_y, void* stream) {
  if (int rc = check_dims(n, t, d)) return rc;
  if (!x || !gamma || !beta || !y) return sagnn::fail(SAGNN_ERR_NULL, "null tensor pointer");
  if (int rc = check_strides(ld_n, ld_t, n, t, d)) return rc;
  if (ld_y < (int64_t)t * d) return sagnn::fail(SAGNN_ERR_ARG, "ld_y smaller than t*d");
  if (n == 0) return SAGNN_OK;
  const int64_t blocks = (n + 3) / 4;
  if (blocks > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "grid too large");
  sagnn::ProfileScope prof(sagnn::kProfLayerNorm, static_cast<hipStream_t>(stream), n, t);
  hipLaunchKernelGGL(layernorm_td_kernel, dim3((unsigned)blocks), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), x, ld_n, ld_t, n, t, d, gamma, beta, eps, y, ld_y);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

// layer norm + Q|K|V + attention + mean in ONE kernel: AttnFwd::Split or AttnFwd::F32Mfma
static bool fused(sagnn::AttnFwd k) { return k == sagnn::AttnFwd::Split || k == sagnn::AttnFwd::F32Mfma; }

static int fused_attention(sagnn::AttnFwd k, const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, void* stream) {
  const auto launch = k == sagnn::AttnFwd::Split ? sagnn::ln_mhsa_mean_split : sagnn::ln_mhsa_mean_mfma;
  return launch(v, a, out, ld_out, static_cast<hipStream_t>(stream));
}

// sagnn_mhsa_mean_f32 on the structs (a.apply_ln = 0)
static int mhsa_mean_call(const SeqView& v, const AttnParams& a, float* out, int64_t ld_out, void* stream) {
  if (int rc = check_attn_call(v, a, out, ld_out)) return rc;
  if (v.n == 0) return SAGNN_OK;
  const sagnn::AttnFwd k = sagnn::select_attn_fwd(sagnn::calling_engine(), v.d, v.t, a.heads, v.vec());
  if (fused(k)) return fused_attention(k, v, a, out, ld_out, stream);
  return sagnn::mhsa_mean_valu(v, a, out, ld_out, static_cast<hipStream_t>(stream));   // Wide too: no workspace
}

extern "C" int sagnn_mhsa_mean_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                                   const float* Wq, const float* bq, const float* Wk,
                                   const float* bk, const float* Wv, const float* bv, float* out,
                                   int64_t ld_out, void* stream) {
  return mhsa_mean_call({x, ld_n, ld_t, n, t, d}, {heads, nullptr, nullptr, 0.f, 0, Wq, bq, Wk, bk, Wv, bv}, out, ld_out, stream);
}

// Attention over rows y [n, t, d] that a layer-norm launch has normalised in the workspace; `rest` follows them there.
static int attention_after_layernorm(sagnn::AttnFwd k, float* y, int64_t n, int t, int d, AttnParams a, float* out,
                                     int64_t ld_out, size_t rest, void* stream) {
  const int64_t ldw = (int64_t)t * d;
  const SeqView yv{y, ldw, d, n, t, d};
  a.gamma = a.beta = nullptr, a.eps = 0.f, a.apply_ln = 0;   // already applied
  if (k == sagnn::AttnFwd::Wide)   // d = 96, 160, ...: MFMA products + per-node kernel
    return mhsa_mean_wide_call(yv, a, out, ld_out, y + n * ldw, rest, stream);
  return mhsa_mean_call(yv, a, out, ld_out, stream);
}

extern "C" size_t sagnn_interval_fusion_workspace_bytes(int64_t n, int t, int d) {
  if (n <= 0 || t <= 0 || d <= 0) return 0;
  size_t bytes = (size_t)n * (size_t)t * (size_t)d * sizeof(float);  // h, normalised in place
  // Q|K|V wherever the wide attention is the fall-back (no heads here: also where a fused kernel is taken)
  if (sagnn::select_attn_fwd(sagnn::calling_engine(), d, t, 1, false) == sagnn::AttnFwd::Wide)
    bytes += sagnn_mhsa_wide_workspace_bytes(n, t, d);
  return bytes;
}

extern "C" int sagnn_interval_fusion_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t,
                                         int d, int heads, const float* lstm_W, const float* lstm_b,
                                         float forget_bias, const float* ln_gamma,
                                         const float* ln_beta, float ln_eps, const float* Wq,
                                         const float* bq, const float* Wk, const float* bk,
                                         const float* Wv, const float* bv, float* out,
                                         int64_t ld_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  const AttnParams a{heads, ln_gamma, ln_beta, ln_eps, 1, Wq, bq, Wk, bk, Wv, bv};
  if (int rc = check_dims(n, t, d)) return rc;
  const size_t need = sagnn_interval_fusion_workspace_bytes(n, t, d);
  if (n > 0 && (!workspace || workspace_bytes < need))
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "fusion workspace needs %zu bytes", need);
  float* h = static_cast<float*>(workspace);
  const int64_t ldw = (int64_t)t * d;
  if (int rc = check_heads(heads, d)) return rc;
  if (missing(a) || !out) return sagnn::fail(SAGNN_ERR_NULL, "null tensor pointer");
  if (n == 0) return SAGNN_OK;
  const sagnn::AttnFwd k = sagnn::select_attn_fwd(sagnn::calling_engine(), d, t, heads, true);   // h: workspace rows
  if (int rc = sagnn_lstm_fwd_f32(x, ld_n, ld_t, n, t, d, lstm_W, lstm_b, forget_bias, nullptr, h, ldw, stream)) return rc;
  // layer norm rides on the fused kernel's A operand: h is read once and never rewritten
  if (fused(k)) return fused_attention(k, {h, ldw, d, n, t, d}, a, out, ld_out, stream);
  if (int rc = sagnn_layernorm_td_f32(h, ldw, d, n, t, d, ln_gamma, ln_beta, ln_eps, h, ldw, stream)) return rc;
  return attention_after_layernorm(k, h, n, t, d, a, out, ld_out, workspace_bytes - (size_t)n * ldw * sizeof(float), stream);
}


// layer_norm over (T, d) + attention + mean (model.py:152-155) without the LSTM: the training
// forward runs the LSTM separately (it stores gates / cell) and comes here with the emitted h.
extern "C" size_t sagnn_ln_mhsa_mean_workspace_bytes(int64_t n, int t, int d, int heads) {
  if (n <= 0 || t <= 0 || d <= 0) return 0;
  const sagnn::AttnFwd k = sagnn::select_attn_fwd(sagnn::calling_engine(), d, t, heads, true);
  if (fused(k)) return 0;  // normalised on the way into the product
  size_t bytes = (size_t)n * (size_t)t * (size_t)d * sizeof(float);
  if (k == sagnn::AttnFwd::Wide) bytes += sagnn_mhsa_wide_workspace_bytes(n, t, d);
  return bytes;
}

extern "C" int sagnn_ln_mhsa_mean_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                                      const float* ln_gamma, const float* ln_beta, float ln_eps, const float* Wq,
                                      const float* bq, const float* Wk, const float* bk, const float* Wv,
                                      const float* bv, float* out, int64_t ld_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const SeqView v{x, ld_n, ld_t, n, t, d};
  const AttnParams a{heads, ln_gamma, ln_beta, ln_eps, 1, Wq, bq, Wk, bk, Wv, bv};
  if (int rc = check_attn_call(v, a, out, ld_out)) return rc;
  if (n == 0) return SAGNN_OK;
  const sagnn::AttnFwd k = sagnn::select_attn_fwd(sagnn::calling_engine(), d, t, heads, v.vec());
  if (fused(k)) return fused_attention(k, v, a, out, ld_out, stream);
  const size_t ybytes = (size_t)n * t * d * sizeof(float);
  size_t need = ybytes + (k == sagnn::AttnFwd::Wide ? sagnn_mhsa_wide_workspace_bytes(n, t, d) : 0);
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "ln_mhsa_mean workspace needs %zu bytes", need);
  float* y = static_cast<float*>(workspace);
  if (int rc = sagnn_layernorm_td_f32(x, ld_n, ld_t, n, t, d, ln_gamma, ln_beta, ln_eps, y, (int64_t)t * d, stream)) return rc;
  return attention_after_layernorm(k, y, n, t, d, a, out, ld_out, workspace_bytes - ybytes, stream);
}

// Front of the attention backward pass in one launch (shapes: engine.cpp): y = LN(x) (apply_ln) or x, Q|K|V = y W + b on
// the matrix cores, attention backward per (node, head) in registers -> dqkv [n*t, 3d]; y [n*t, d] is written when y_out
// is given (operand of dW = y^T dQKV).
extern "C" int sagnn_attn_bwd_front_supported(int d, int t, int heads) {
  const sagnn::Engine e = sagnn::calling_engine();
  return e != sagnn::Engine::Valu && sagnn::select_attn_bwd_front(e, d, t, heads) != sagnn::AttnBwdFront::None;
}

extern "C" int sagnn_attn_bwd_front_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n, int t, int d, int heads,
                                        const float* ln_gamma, const float* ln_beta, float ln_eps, int apply_ln,
                                        const float* Wq, const float* bq, const float* Wk, const float* bk,
                                        const float* Wv, const float* bv, const float* g_out, int64_t ld_g,
                                        float* dqkv, float* y_out, void* stream) {
  const SeqView v{x, ld_n, ld_t, n, t, d};
  const AttnParams a{heads, ln_gamma, ln_beta, ln_eps, apply_ln, Wq, bq, Wk, bk, Wv, bv};
  if (int rc = check_dims(n, t, d)) return rc;
  const sagnn::AttnBwdFront k = sagnn::select_attn_bwd_front(sagnn::calling_engine(), d, t, heads);
  if (k == sagnn::AttnBwdFront::None)
    return sagnn::fail(SAGNN_ERR_DIM, "attn_bwd_front: unsupported d = %d, t = %d, heads = %d", d, t, heads);
  if (!x || missing(a) || !g_out || !dqkv) return sagnn::fail(SAGNN_ERR_NULL, "null tensor pointer");
  if (int rc = check_strides(ld_n, ld_t, n, t, d)) return rc;
  if (ld_g < d) return sagnn::fail(SAGNN_ERR_ARG, "ld_g smaller than d");
  if (!v.vec() || !sagnn::aligned16(g_out) || (ld_g & 3) || !sagnn::aligned16(dqkv) || (y_out && !sagnn::aligned16(y_out)))
    return sagnn::fail(SAGNN_ERR_ALIGN, "attn_bwd_front: need 16-byte aligned rows");
  if (n == 0) return SAGNN_OK;
  const auto launch = k == sagnn::AttnBwdFront::Split ? sagnn::attn_bwd_front_split : sagnn::attn_bwd_front_mfma;
  return launch(v, a, {g_out, ld_g, dqkv, y_out}, static_cast<hipStream_t>(stream));
}
