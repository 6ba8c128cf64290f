// Row subsets of the interval fusion for training (include/sagnn.h, "Row subsets of the interval fusion"): mark the
// rows a batch reads in a byte flag per row, compact the flags into ascending row ids, gather those rows of the GNN
// slab into a dense [cap, t, d] block for the existing fusion kernels, and scatter the results back.
//
// Compaction is three launches over tiles of kTile rows: count the flags per tile, one workgroup scans the tile counts
// (and writes the total to the caller's device count), then every tile writes its ids at its offset, in row order,
// and clears the flags it read. Gather and scatter move one float4 per thread.
#include "common.h"

#include <limits.h>

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 16;                       // flags per thread: one 16-byte load
constexpr int64_t kTile = (int64_t)kBlock * kPerThread;
constexpr int kScanBlock = 1024;

__global__ void mark_kernel(const int32_t* __restrict__ ids, int64_t n_ids, int64_t n_rows, uint8_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ids) return;
  const int64_t v = ids[i];
  if (v >= 0 && v < n_rows) flags[v] = 1;
}

// one thread per (slot b, entry j < max_len); entry j of slot b is seq_items[seg_begin[b] + j] for j < seg_len[b]
__global__ void mark_seg_kernel(const int32_t* __restrict__ items, int64_t n_flat, const int64_t* __restrict__ seg_begin,
                                const int32_t* __restrict__ seg_len, int64_t n_slots, int max_len, int64_t n_rows,
                                uint8_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * max_len) return;
  const int64_t b = t / max_len;
  const int j = (int)(t - b * max_len);
  if (j >= min(seg_len[b], max_len)) return;
  const int64_t e = seg_begin[b] + j;
  if (e < 0 || e >= n_flat) return;
  const int64_t v = items[e];
  if (v >= 0 && v < n_rows) flags[v] = 1;
}

// the kPerThread flags thread `tid` of tile `blk` owns, as a 16-bit set mask (bit q = row base + q)
__device__ __forceinline__ uint32_t load_flags(const uint8_t* flags, int64_t n_rows, int64_t base) {
  uint32_t m = 0;
  if (base + kPerThread <= n_rows) {
    const uint4 v = *reinterpret_cast<const uint4*>(flags + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((w[k] >> (8 * q)) & 0xFFu) m |= 1u << (4 * k + q);
  } else {
    for (int q = 0; q < kPerThread && base + q < n_rows; ++q)
      if (flags[base + q]) m |= 1u << q;
  }
  return m;
}

// exclusive scan of one int per thread over the workgroup (NT threads, NT / 64 waves); *total = the sum
template <int NT>
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < NT / 64; ++i) {
      const int c = lds[i];
      lds[i] = s;
      s += c;
    }
    lds[NT / 64] = s;
  }
  __syncthreads();
  const int r = x - v + lds[w];
  *total = lds[NT / 64];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kBlock) tile_count_kernel(const uint8_t* __restrict__ flags, int64_t n_rows,
                                                            int32_t* __restrict__ tile_count) {
  __shared__ int lds[kBlock / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
  const int c = base < n_rows ? __popc(load_flags(flags, n_rows, base)) : 0;
  int total;
  block_exclusive_scan<kBlock>(c, lds, &total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: tile_off[i] = sum of tile_count[< i] (in place), tile_off[n_tiles] = *count = the total
__global__ void __launch_bounds__(kScanBlock) tile_scan_kernel(int32_t* __restrict__ tile, int64_t n_tiles,
                                                               int32_t* __restrict__ count) {
  __shared__ int lds[kScanBlock / 64 + 1];
  int carry = 0;
  for (int64_t i0 = 0; i0 < n_tiles; i0 += kScanBlock) {
    const int64_t i = i0 + threadIdx.x;
    const int v = i < n_tiles ? tile[i] : 0;
    int total;
    const int r = block_exclusive_scan<kScanBlock>(v, lds, &total);
    if (i < n_tiles) tile[i] = carry + r;
    carry += total;
  }
  if (threadIdx.x == 0) {
    tile[n_tiles] = carry;
    *count = carry;
  }
}

__global__ void __launch_bounds__(kBlock) tile_write_kernel(uint8_t* __restrict__ flags, int64_t n_rows,
                                                            const int32_t* __restrict__ tile_off, int64_t n_tiles,
                                                            int32_t* __restrict__ rows, int64_t cap) {
  __shared__ int lds[kBlock / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
  const uint32_t m = base < n_rows ? load_flags(flags, n_rows, base) : 0u;
  int total;
  const int r = block_exclusive_scan<kBlock>(__popc(m), lds, &total);
  if (m) {
    int64_t pos = (int64_t)tile_off[blockIdx.x] + r;
    for (int q = 0; q < kPerThread; ++q) {
      if (!((m >> q) & 1u)) continue;
      if (pos < cap) rows[pos] = (int32_t)(base + q);
      ++pos;
    }
    // clear what was read: the next mark starts from a zero buffer without a memset
    if (base + kPerThread <= n_rows) {
      *reinterpret_cast<uint4*>(flags + base) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (int q = 0; q < kPerThread && base + q < n_rows; ++q) flags[base + q] = 0;
    }
  }
  // slots [count, cap) get row 0, a valid id, so that kernels run over cap rows read finite data
  const int64_t n = tile_off[n_tiles];
  for (int64_t j = n + (int64_t)blockIdx.x * kBlock + threadIdx.x; j < cap; j += (int64_t)gridDim.x * kBlock) rows[j] = 0;
}

__device__ __forceinline__ int64_t live_count(const int32_t* count, int64_t cap) {
  return count ? min(max((int64_t)*count, (int64_t)0), cap) : cap;
}

// out[j, s, :] = x[rows[j], s, :] (x at strides ld_n / ld_t); zeros for j >= *count when count is given
__global__ void gather_kernel(const float* __restrict__ x, int64_t ld_n, int64_t ld_t, int64_t n_rows, int t, int d,
                              const int32_t* __restrict__ rows, int64_t cap, const int32_t* __restrict__ count,
                              float* __restrict__ out) {
  const int lpr = d >> 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap * t * lpr) return;
  const int64_t js = i / lpr;
  const int col = (int)(i - js * lpr) * 4;
  const int64_t j = js / t;
  const int s = (int)(js - j * t);
  const int64_t r = rows[j];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < live_count(count, cap) && r >= 0 && r < n_rows) v = *reinterpret_cast<const float4*>(x + r * ld_n + s * ld_t + col);
  *reinterpret_cast<float4*>(out + js * d + col) = v;
}

// dst[rows[j], s, :] = src[j, s, :] for j < *count (dst at strides ld_n / ld_t); nothing else is written
__global__ void scatter_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows, int64_t cap,
                               const int32_t* __restrict__ count, int t, int d, float* __restrict__ dst, int64_t ld_n,
                               int64_t ld_t, int64_t n_rows) {
  const int lpr = d >> 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap * t * lpr) return;
  const int64_t js = i / lpr;
  const int col = (int)(i - js * lpr) * 4;
  const int64_t j = js / t;
  const int s = (int)(js - j * t);
  if (j >= live_count(count, cap)) return;
  const int64_t r = rows[j];
  if (r < 0 || r >= n_rows) return;
  *reinterpret_cast<float4*>(dst + r * ld_n + s * ld_t + col) = *reinterpret_cast<const float4*>(src + js * d + col);
}

int blocks_for(int64_t threads, unsigned* out) {
  const int64_t n = (threads + kBlock - 1) / kBlock;
  if (n > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "fusion_rows: %lld threads exceed one launch", (long long)threads);
  *out = (unsigned)n;
  return SAGNN_OK;
}

int64_t n_tiles_for(int64_t n_rows) { return (n_rows + kTile - 1) / kTile; }

int check_n_rows(const char* who, int64_t n_rows) {
  if (n_rows < 0 || n_rows > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_rows = %lld, need 0 <= n_rows < 2^31", who, (long long)n_rows);
  return SAGNN_OK;
}

// shared checks of gather / scatter: the strided side (ld_n, ld_t, pointer) and the dense side
int check_move(const char* who, const void* strided, int64_t ld_n, int64_t ld_t, int64_t n_rows, int t, int d,
               int64_t cap, const void* dense) {
  if (d < 4 || d > 256 || (d & 3)) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need a multiple of 4 in [4, 256]", who, d);
  if (t < 1) return sagnn::fail(SAGNN_ERR_DIM, "%s: t = %d, need >= 1", who, t);
  if (int rc = check_n_rows(who, n_rows)) return rc;
  if (cap < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: negative count (cap = %lld)", who, (long long)cap);
  if (cap > n_rows)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: cap = %lld > n_rows = %lld", who, (long long)cap, (long long)n_rows);
  if (ld_n < d || ld_t < 0)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: strides ld_n = %lld, ld_t = %lld, need ld_n >= d and ld_t >= 0", who,
                       (long long)ld_n, (long long)ld_t);
  if ((ld_n & 3) || (ld_t & 3) || !sagnn::aligned16(strided) || !sagnn::aligned16(dense))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: pointers must be 16-byte aligned with strides that are multiples of 4", who);
  return SAGNN_OK;
}

}  // namespace

extern "C" int sagnn_rows_mark_i32(const int32_t* ids, int64_t n_ids, int64_t n_rows, uint8_t* flags, void* stream) {
  if (!ids || !flags) return sagnn::fail(SAGNN_ERR_NULL, "rows_mark: null pointer (ids, flags)");
  if (n_ids < 0) return sagnn::fail(SAGNN_ERR_ARG, "rows_mark: negative count (n_ids = %lld)", (long long)n_ids);
  if (int rc = check_n_rows("rows_mark", n_rows)) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(n_ids, &blocks)) return rc;
  if (blocks == 0 || n_rows == 0) return SAGNN_OK;
  hipLaunchKernelGGL(mark_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), ids, n_ids, n_rows, flags);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_rows_mark_seg_i32(const int32_t* seq_items, int64_t n_flat, const int64_t* seg_begin,
                                       const int32_t* seg_len, int64_t n_slots, int max_len, int64_t n_rows,
                                       uint8_t* flags, void* stream) {
  if (!seq_items || !seg_begin || !seg_len || !flags)
    return sagnn::fail(SAGNN_ERR_NULL, "rows_mark_seg: null pointer (seq_items, seg_begin, seg_len, flags)");
  if (n_flat < 0 || n_slots < 0 || max_len < 0)
    return sagnn::fail(SAGNN_ERR_ARG, "rows_mark_seg: negative count (n_flat = %lld, n_slots = %lld, max_len = %d)",
                       (long long)n_flat, (long long)n_slots, max_len);
  if (int rc = check_n_rows("rows_mark_seg", n_rows)) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(n_slots * max_len, &blocks)) return rc;
  if (blocks == 0 || n_rows == 0) return SAGNN_OK;
  hipLaunchKernelGGL(mark_seg_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), seq_items, n_flat,
                     seg_begin, seg_len, n_slots, max_len, n_rows, flags);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" size_t sagnn_rows_compact_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0) return 0;
  return (size_t)(n_tiles_for(n_rows) + 1) * sizeof(int32_t);
}

extern "C" int sagnn_rows_compact_i32(uint8_t* flags, int64_t n_rows, int32_t* rows, int64_t cap, int32_t* count,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!flags || !rows || !count) return sagnn::fail(SAGNN_ERR_NULL, "rows_compact: null pointer (flags, rows, count)");
  if (int rc = check_n_rows("rows_compact", n_rows)) return rc;
  if (cap < 0) return sagnn::fail(SAGNN_ERR_ARG, "rows_compact: negative count (cap = %lld)", (long long)cap);
  if (cap < 1 && n_rows > 0) return sagnn::fail(SAGNN_ERR_ARG, "rows_compact: cap = %lld, need >= 1 with rows to mark", (long long)cap);
  if (cap > n_rows)
    return sagnn::fail(SAGNN_ERR_ARG, "rows_compact: cap = %lld > n_rows = %lld", (long long)cap, (long long)n_rows);
  if (!sagnn::aligned16(flags)) return sagnn::fail(SAGNN_ERR_ALIGN, "rows_compact: flags must be 16-byte aligned");
  const size_t need = sagnn_rows_compact_workspace_bytes(n_rows);
  if (!workspace || workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "rows_compact: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const int64_t n_tiles = n_tiles_for(n_rows);
  if (n_tiles > INT_MAX) return sagnn::fail(SAGNN_ERR_ARG, "rows_compact: %lld tiles exceed one launch", (long long)n_tiles);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* tile = static_cast<int32_t*>(workspace);
  if (n_tiles == 0) {
    SAGNN_HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), s));
    return SAGNN_OK;
  }
  hipLaunchKernelGGL(tile_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, flags, n_rows, tile);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, tile, n_tiles, count);
  hipLaunchKernelGGL(tile_write_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, s, flags, n_rows, tile, n_tiles, rows, cap);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_rows_gather_f32(const float* x, int64_t ld_n, int64_t ld_t, int64_t n_rows, int t, int d,
                                     const int32_t* rows, int64_t cap, const int32_t* count, float* out, void* stream) {
  if (!x || !rows || !out) return sagnn::fail(SAGNN_ERR_NULL, "rows_gather: null pointer (x, rows, out)");
  if (int rc = check_move("rows_gather", x, ld_n, ld_t, n_rows, t, d, cap, out)) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(cap * t * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(gather_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), x, ld_n, ld_t, n_rows,
                     t, d, rows, cap, count, out);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_rows_scatter_f32(const float* src, const int32_t* rows, int64_t cap, const int32_t* count, int t,
                                      int d, float* dst, int64_t ld_n, int64_t ld_t, int64_t n_rows, void* stream) {
  if (!src || !rows || !count || !dst) return sagnn::fail(SAGNN_ERR_NULL, "rows_scatter: null pointer (src, rows, count, dst)");
  if (int rc = check_move("rows_scatter", dst, ld_n, ld_t, n_rows, t, d, cap, src)) return rc;
  unsigned blocks = 0;
  if (int rc = blocks_for(cap * t * (d / 4), &blocks)) return rc;
  if (blocks == 0) return SAGNN_OK;
  hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), src, rows, cap, count,
                     t, d, dst, ld_n, ld_t, n_rows);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
