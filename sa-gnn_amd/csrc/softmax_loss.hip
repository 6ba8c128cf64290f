// Softmax cross-entropy over the catalogue, one kernel family in two modes. z(b, i) = <Q[b], I[i]> * inv_temp on the
// exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32), loss = scale * sum_b (ln sum_{i eligible} exp z(b, i) - z(b, t_b)).
// The [queries x items] logits are never stored: the forward streams a log-sum-exp, the backward recomputes them.
//
// The kernels run over POSITIONS. Full mode (SAGNN_SOFTMAX_FULL of sagnn_softmax_loss_f32 / _bwd_f32): position j is item
// j, there are n_items of them. Candidate mode (SAGNN_SOFTMAX_CAND, --softmaxNegs): position j is item cand[j] of an
// ascending id list shared by the batch, there are n_cand of them, and a position past the list reads the last
// candidate's row and is never eligible. The mode is a template argument, never a runtime branch, and all it decides
// is stated once, in Mode<CAND> and Tile<CAND> below:
//   1. what a position is (its id, the row of I it reads, how many there are);
//   2. how the exclusion walk matches: by offset into the tile in full mode, by id in candidate mode;
//   3. how the target enters: in full mode through its own position (eligible even when listed, grad_elem takes
//      is_target); in candidate mode never through a position but once per row, in lse_row_kernel and dq_row_kernel;
//   4. the launch shape (launch_fwd / launch_bwd): candidate mode may have no chunk at all, runs a short list at
//      NI = 1 in di_kernel, and has dq_row_kernel where full mode has dq_merge_kernel.
// A full instantiation loads no cand, shuffles no ids and uses no LDS.
//
// Candidate mode has one more compile-time property, the per-position logit offset (SAGNN_SOFTMAX_CAND_BIAS,
// --softmaxNegDist pop), stated once in Offset<BIAS> below: position j adds bias[j] to its logit, and a
// position with bias[j] = -inf is dead, never eligible. The list may then repeat ids (non-decreasing, repeats adjacent,
// the first position of a run the only live one), and the id matching above stays right for these reasons alone:
//   - the chunk kernels' walk passes every list entry <= the tile's last id, so a run that goes on into the next tile
//     (or chunk: the next chunk's walk starts at its first id again) may be matched there or not: those positions are
//     dead, and eligibility is all the match decides;
//   - di_kernel finds a list entry's first occurrence among the span's ids: the run's live position when the run
//     starts in the span, a dead one when it started before it;
//   - a tile, span or chunk without a live position merges as the empty (-inf, 0): a dead position's -inf is never added
//     to a score, its accumulator row gets g = 0 and its dIc row is written as zeros;
//   - the target's own term (lse_row_kernel, dq_row_kernel) takes no offset.
// An instantiation without the offset loads no bias and is the code it was.
//
// Forward pass 1 (lse_chunk_kernel): one wavefront per (kNT query tiles of 16 rows, chunk of positions), laid out as
// retrieval.hip's topk_chunk_kernel: item rows are the A operand, the Q fragments stay in registers, acc[r] is the
// score of position s0 + 4 * (lane >> 4) + r for query lane & 15. One item fragment feeds kNT query tiles. A lane keeps
// a running (max, sum) over its positions; the four lanes of a query are combined by shuffles and one (max, sum) per
// (query, chunk) goes to the workspace. An empty side has max = -inf and sum = 0 and is never passed through
// exp(-inf - (-inf)).
// Pass 2 (lse_row_kernel): one wavefront per query merges the chunk partials (a fixed tree over the chunk index) into
// lse[b], takes the target's score from the same tile arithmetic and writes the row's loss term; candidate mode merges
// the target's own (z_t, 1) after the partials.
// Pass 3 (loss_sum_kernel): one workgroup adds the row terms in a fixed order into loss[0]. No atomics anywhere.
//
// Backward, g(b, i) = (g * scale * inv_temp) * (p(b, i) - [i == t_b]), p = exp(z - lse[b]) on eligible items:
// dq_chunk_kernel: the forward's grid and layout. The accumulator, turned into g in place, is the B operand of
//   dQ^T[16 features x 16 queries] += I^T[features x items] . G[items x queries]: MFMA r contracts over the positions
//   s0 + 4 * (lane >> 4) + r, so its A operand is element (that position's item, feature f0 + (lane & 15)). A lane ends
//   with four contiguous features of one query. Per-chunk partials go to the workspace; dq_merge_kernel (full) adds
//   them in chunk order, dq_row_kernel (candidate) does the same, adds the target's g(b, t_b) I[t_b] and writes dT.
// di_kernel: one wavefront per NI tiles of positions loops over all query tiles with the QUERIES on the accumulator
//   rows (queries as A, items as B), so the accumulator is the B operand of dI^T[16 features x 16 items] += Q^T . G and
//   a lane ends with four contiguous features of one position's row. 64 lanes look up the exclusions of 64 queries at
//   once into a bit mask over the span's positions and hand the masks over by shuffle.
// Chunks depend on the position count only and every sum has a fixed order, so lse / tscore / dQ / dT of a row depend
// on that row alone and all outputs are bit-identical between runs.
#include "common.h"

#include <math.h>

#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNT = 2;            // query tiles per wavefront in the chunk kernels
constexpr int kMinChunk = 128;    // positions per chunk at least (a multiple of 16)
constexpr int kMaxChunks = 256;
constexpr int kSmallSpans = 256;   // di_kernel, candidate mode: fewer spans than this run at 16 positions per wavefront

struct Problem {
  const float* Q;
  int64_t ldq;
  const float* I;
  int64_t ldi;
  int64_t n_queries, n_items;
  const int32_t* target;
  float inv_temp, scale;
  const int64_t* excl_ptr;
  const int32_t* excl_items;
  const int32_t* excl_row;
  int64_t n_lists;
  int64_t chunk, n_chunks;                               // cut the positions
  const int32_t* cand;                                   // candidate mode only: the positions' ids and their count
  int64_t n_cand;
};

// Chunks from the position count alone: at most kMaxChunks of them, at least kMinChunk positions each, a multiple of 16.
__host__ __device__ inline int64_t chunk_items(int64_t n_items) {
  int64_t c = (n_items + kMaxChunks - 1) / kMaxChunks;
  if (c < kMinChunk) c = kMinChunk;
  return (c + 15) / 16 * 16;
}

// (m, s) += (om, os) for sums s * exp(m); an empty side is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float mx = fmaxf(m, om);
  if (mx == -INFINITY) return;
  s = s * __expf(m - mx) + os * __expf(om - mx);
  m = mx;
}

// The exclusion list of query row b as [lo, hi) into excl_items; empty when there is none.
__device__ __forceinline__ void excl_range(const Problem& p, int64_t b, int64_t& lo, int64_t& hi) {
  lo = hi = 0;
  if (!p.excl_ptr) return;
  const int64_t L = p.excl_row ? (int64_t)p.excl_row[b] : b;
  if (L < 0 || L >= p.n_lists) return;
  lo = p.excl_ptr[L];
  hi = p.excl_ptr[L + 1];
}

__device__ __forceinline__ int64_t excl_lower_bound(const int32_t* __restrict__ items, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)items[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// A lane's walk over its row's exclusions as the chunk advances
struct Walk {
  int64_t ep, ee;
  int nxt;                                               // excl_items[ep] while ep < ee
};

__device__ __forceinline__ void walk_init(const Problem& p, int64_t b, bool ok, int64_t c0, Walk& w) {
  w.ep = w.ee = 0;
  w.nxt = 0;
  if (!ok) return;
  int64_t lo, hi;
  excl_range(p, b, lo, hi);
  w.ee = hi;
  w.ep = excl_lower_bound(p.excl_items, lo, hi, c0);
  if (w.ep < w.ee) w.nxt = p.excl_items[w.ep];
}

// bit r: item s0 + 4g + r is on the list (the walk passes every entry below s0 + 16)
__device__ __forceinline__ unsigned walk_bits(const Problem& p, Walk& w, int64_t s0, int g) {
  unsigned xm = 0;
  while (w.ep < w.ee && (int64_t)w.nxt < s0 + 16) {
    const int64_t off = (int64_t)w.nxt - s0;
    if (off >= 0 && (off >> 2) == g) xm |= 1u << (off & 3);
    if (++w.ep < w.ee) w.nxt = p.excl_items[w.ep];
  }
  return xm;
}

// bit r: id[r] is on the list (the walk passes every entry up to `last`, the tile's last id)
__device__ __forceinline__ unsigned walk_bits(const Problem& p, Walk& w, const int (&id)[4], int last) {
  unsigned xm = 0;
  while (w.ep < w.ee && w.nxt <= last) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (w.nxt == id[r]) xm |= 1u << r;
    if (++w.ep < w.ee) w.nxt = p.excl_items[w.ep];
  }
  return xm;
}

// ---- The two modes ---------------------------------------------------------------------------------------------------
// What a position is: how many there are, the id of one, the row of I an id reads (full mode clamps a position past the
// end to the last row, id_at of candidate mode clamps the position), the key a chunk's exclusion walk starts at, and
// whether position i0 + off of a span of n_span exists (each mode in the form its dI kernel compares in: a 64-bit id
// in full mode, the offset in candidate mode). And when one (query, position) element counts. `ok`: the query has a
// target; `inside`: the position exists; `ex`: its id is on the query's list; `ti`: the query's target, -1 without one.
template <bool CAND>
struct Mode;

template <>
struct Mode<false> {
  typedef int64_t id_t;
  static __device__ __forceinline__ int64_t count(const Problem& p) { return p.n_items; }
  static __device__ __forceinline__ int64_t id_at(const Problem&, int64_t pos) { return pos; }
  static __device__ __forceinline__ int64_t row(const Problem& p, int64_t id) { return id < p.n_items ? id : p.n_items - 1; }
  static __device__ __forceinline__ int64_t walk_key(const Problem&, int64_t c0) { return c0; }
  static __device__ __forceinline__ bool in_span(const Problem& p, int64_t i0, int off, int) { return i0 + off < p.n_items; }
  // the target is a position like any other, eligible even when listed
  static __device__ __forceinline__ bool is_target(bool ok, int64_t id, int ti) { return ok && id == ti; }
  static __device__ __forceinline__ bool eligible(bool ok, bool inside, bool ex, int64_t id, int ti) {
    return ok && inside && (!ex || id == ti);
  }
};

template <>
struct Mode<true> {
  typedef int id_t;
  static __device__ __forceinline__ int64_t count(const Problem& p) { return p.n_cand; }
  static __device__ __forceinline__ int id_at(const Problem& p, int64_t pos) {
    return p.cand[pos < p.n_cand ? pos : p.n_cand - 1];
  }
  static __device__ __forceinline__ int64_t row(const Problem&, int id) { return id; }
  static __device__ __forceinline__ int64_t walk_key(const Problem& p, int64_t c0) { return p.cand[c0]; }
  static __device__ __forceinline__ bool in_span(const Problem&, int64_t, int off, int n_span) { return off < n_span; }
  // the target never enters through a position: the row kernels add its term once
  static __device__ __forceinline__ bool is_target(bool, int, int) { return false; }
  static __device__ __forceinline__ bool eligible(bool ok, bool inside, bool ex, int id, int ti) {
    return ok && inside && !ex && id != ti;
  }
};

// The 16 positions [s0, s0 + 16) as lane (g, q) of a chunk kernel sees them: lane_id is the id of position s0 + q, whose
// row the lane loads, id(r) the id of position s0 + 4g + r, its accumulator row r. excl_bits advances the lane's walk
// over the tile: bit r says that id(r) is on the list.
template <bool CAND>
struct Tile;

template <>
struct Tile<false> {
  int64_t s0;
  int g;
  int64_t lane_id;
  __device__ __forceinline__ Tile(const Problem&, int64_t s0_, int q, int g_) : s0(s0_), g(g_), lane_id(s0_ + q) {}
  __device__ __forceinline__ int64_t id(int r) const { return s0 + 4 * g + r; }
  __device__ __forceinline__ unsigned excl_bits(const Problem& p, Walk& w) const { return walk_bits(p, w, s0, g); }
};

template <>
struct Tile<true> {
  int lane_id, ids[4], last;                             // ids and the tile's last id come from the neighbours' lane_id
  __device__ __forceinline__ Tile(const Problem& p, int64_t s0, int q, int g) : lane_id(Mode<true>::id_at(p, s0 + q)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ids[r] = __shfl(lane_id, 4 * g + r);
    last = __shfl(lane_id, 15);
  }
  __device__ __forceinline__ int id(int r) const { return ids[r]; }
  __device__ __forceinline__ unsigned excl_bits(const Problem& p, Walk& w) const { return walk_bits(p, w, ids, last); }
};

// Candidate mode's logit offset, the LAST argument of the three kernels that take it: empty without the offset, so
// that those instantiations keep their arguments and their code. at(): the offset of one position, -inf past the list
// (never read out of bounds). live(): the position may be eligible. add(): x + the offset, for x = a logit or a logit
// minus a maximum / the row's lse: written with the offset last, so that a zero offset gives the bits of the
// instantiation without one whichever way the compiler contracts the multiply by inv_temp into the subtraction.
template <bool BIAS>
struct Offset;

template <>
struct Offset<false> {
  __device__ __forceinline__ float at(const Problem&, int64_t) const { return 0.f; }
  static __device__ __forceinline__ bool live(float) { return true; }
  static __device__ __forceinline__ float add(float x, float) { return x; }
};

template <>
struct Offset<true> {
  const float* bias;                                     // one per position
  __device__ __forceinline__ float at(const Problem& p, int64_t pos) const { return pos < p.n_cand ? bias[pos] : -INFINITY; }
  static __device__ __forceinline__ bool live(float b) { return b > -INFINITY; }
  static __device__ __forceinline__ float add(float x, float b) { return x + b; }
};

// The offsets of a chunk kernel's tile, as Tile<true> holds its ids: lane q loads position s0 + q's, b[r] is that of
// position s0 + 4g + r. Empty without the offset.
template <bool BIAS>
struct TileOffset {
  __device__ __forceinline__ TileOffset(const Problem&, const Offset<BIAS>&, int64_t, int, int) {}
  __device__ __forceinline__ float operator[](int) const { return 0.f; }
};

template <>
struct TileOffset<true> {
  float b[4];
  __device__ __forceinline__ TileOffset(const Problem& p, const Offset<true>& ob, int64_t s0, int q, int g) {
    const float mine = ob.at(p, s0 + q);
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = __shfl(mine, 4 * g + r);
  }
  __device__ __forceinline__ float operator[](int r) const { return b[r]; }
};

// acc[r] = <row 4 * (lane >> 4) + r of the A side, row lane & 15 of the B side>; a[t] / b[t] are the lane's float4 of
// its A / B row at columns 16t + 4 * (lane >> 4). A fixed fmaf chain over the columns.
template <int D>
__device__ __forceinline__ f32x4 tile_scores(const float4 (&a)[D / 16], const float4 (&b)[D / 16]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[t].w, acc, 0, 0, 0);
  }
  return acc;
}

template <int D>
__device__ __forceinline__ void load_frag(const float* __restrict__ row, int g, float4 (&f)[D / 16]) {
#pragma unroll
  for (int t = 0; t < D / 16; ++t) f[t] = *reinterpret_cast<const float4*>(row + 16 * t + 4 * g);
}

// What a lane of the chunk kernels knows about the query lane & 15 of one of its tiles
template <int D>
struct QueryLane {
  float4 qf[D / 16];
  int64_t b;
  bool in, ok;                                           // row exists; row exists and has a target
  int ti;                                                // the target, -1 without one
  Walk w;
};

template <int D>
__device__ __forceinline__ void query_init(const Problem& p, int64_t b, int64_t c0, int g, QueryLane<D>& ql) {
  ql.b = b;
  ql.in = b < p.n_queries;
  const int64_t bq = ql.in ? b : p.n_queries - 1;
  const int32_t tv = p.target[bq];
  ql.ok = ql.in && tv >= 0 && (int64_t)tv < p.n_items;
  ql.ti = ql.ok ? tv : -1;
  load_frag<D>(p.Q + bq * p.ldq, g, ql.qf);
  walk_init(p, bq, ql.ok, c0, ql.w);
}

// One tile into a lane's running (m, s): the tile's maximum first, then one exp per eligible element and one for the
// rescale. Nothing eligible so far and nothing here leaves (-inf, 0) alone. With the offset the logit of element r is
// z[r] + off[r]; an eligible element's offset is finite.
template <bool BIAS, class Off>
__device__ __forceinline__ void lse_update(float& m, float& s, const float (&z)[4], const bool (&e)[4], const Off& off) {
  typedef Offset<BIAS> B;
  float mx = m;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (e[r]) mx = fmaxf(mx, B::add(z[r], off[r]));
  if (mx > -INFINITY) {
    float sum = s * __expf(m - mx);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (e[r]) sum += __expf(B::add(z[r] - mx, off[r]));
    s = sum;
    m = mx;
  }
}

// g(b, i) of one accumulator element: z = acc * inv_temp (+ off with the offset, finite where elig)
template <bool BIAS = false>
__device__ __forceinline__ float grad_elem(float acc, float inv_temp, float lse, float coef, bool elig, bool is_target,
                                           float off = 0.f) {
  const float pr = elig ? __expf(Offset<BIAS>::add(acc * inv_temp - lse, off)) : 0.f;
  return coef * (pr - (is_target ? 1.f : 0.f));
}

// grad_elem under the mode's rules. Full mode writes an exact zero for a query without a target; candidate mode's
// coef * 0 there keeps what its kernels always wrote.
// `off`: the position's offset (BIAS only), which also decides whether it is live.
template <bool CAND, bool BIAS>
__device__ __forceinline__ float grad_at(float acc, const Problem& p, float lse, float coef, bool ok, bool inside, bool ex,
                                         typename Mode<CAND>::id_t id, int ti, float off) {
  typedef Mode<CAND> M;
  if constexpr (!CAND)
    if (!ok) return 0.f;
  return grad_elem<BIAS>(acc, p.inv_temp, lse, coef, M::eligible(ok, inside && Offset<BIAS>::live(off), ex, id, ti),
                         M::is_target(ok, id, ti), off);
}

// out[n][f] += row x G[n][r] over the features 16f .. 16f + 15: one MFMA of the second product per (f, n), which
// contracts over the lane groups' rows r. Its A operand is one float of `row` at feature 16f + (lane & 15): `row`
// points at the lane's feature of f = 0.
template <int D, int N>
__device__ __forceinline__ void contract_row(const float* __restrict__ row, int r, const f32x4 (&G)[N], f32x4 (&out)[N][D / 16]) {
#pragma unroll
  for (int f = 0; f < D / 16; ++f) {
    const float av = row[16 * f];
#pragma unroll
    for (int n = 0; n < N; ++n) out[n][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, G[n][r], out[n][f], 0, 0, 0);
  }
}

// A lane's accumulator row to memory: features 16f + 4g .. + 3, `out` points at feature 4g
template <int D>
__device__ __forceinline__ void store_row(float* __restrict__ out, const f32x4 (&acc)[D / 16]) {
#pragma unroll
  for (int f = 0; f < D / 16; ++f)
    *reinterpret_cast<float4*>(out + 16 * f) = make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
}

template <int D, bool CAND, bool BIAS>
__global__ __launch_bounds__(64) void lse_chunk_kernel(Problem p, float2* __restrict__ part, Offset<BIAS> ob) {
  static_assert(CAND || !BIAS, "the offset is a property of candidate mode");
  typedef Mode<CAND> M;
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < M::count(p) ? c0 + p.chunk : M::count(p);
  QueryLane<D> ql[kNT];
  float m[kNT], s[kNT];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, M::walk_key(p, c0), g, ql[u]);
    m[u] = -INFINITY;
    s[u] = 0.f;
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    const Tile<CAND> t(p, s0, q, g);
    const TileOffset<BIAS> off(p, ob, s0, q, g);
    float4 a[D / 16];
    load_frag<D>(p.I + M::row(p, t.lane_id) * p.ldi, g, a);
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = t.excl_bits(p, ql[u].w);
      float z[4];
      bool e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = M::eligible(ql[u].ok, s0 + 4 * g + r < c1 && Offset<BIAS>::live(off[r]), (xm >> r) & 1, t.id(r), ql[u].ti);
        z[r] = acc[r] * p.inv_temp;
      }
      lse_update<BIAS>(m[u], s[u], z, e, off);
    }
  }
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    lse_merge(m[u], s[u], __shfl_xor(m[u], 16), __shfl_xor(s[u], 16));
    lse_merge(m[u], s[u], __shfl_xor(m[u], 32), __shfl_xor(s[u], 32));
    if (ql[u].in && g == 0) part[ql[u].b * p.n_chunks + blockIdx.y] = make_float2(m[u], s[u]);
  }
}

template <int D, bool CAND>
__global__ __launch_bounds__(64) void lse_row_kernel(Problem p, const float2* __restrict__ part, float* __restrict__ lse,
                                                     float* __restrict__ tscore, float* __restrict__ terms) {
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int64_t b = blockIdx.x;
  const int32_t tv = p.target[b];
  const bool ok = tv >= 0 && (int64_t)tv < p.n_items;
  float m = -INFINITY, s = 0.f;
  for (int64_t j = lane; j < p.n_chunks; j += 64) {
    const float2 v = part[b * p.n_chunks + j];
    lse_merge(m, s, v.x, v.y);
  }
  for (int off = 1; off < 64; off <<= 1) lse_merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
  // the target's score: every row of the A side is the target, every row of the B side the query
  float4 a[D / 16], qf[D / 16];
  load_frag<D>(p.I + (int64_t)(ok ? tv : 0) * p.ldi, g, a);
  load_frag<D>(p.Q + b * p.ldq, g, qf);
  const f32x4 acc = tile_scores<D>(a, qf);
  if (lane == 0) {
    if constexpr (CAND)                                  // the target's own term, after the chunk partials
      if (ok) lse_merge(m, s, acc[0] * p.inv_temp, 1.f);
    const float l = ok ? m + logf(s) : 0.f;
    const float ts = ok ? acc[0] : 0.f;
    lse[b] = l;
    tscore[b] = ts;
    terms[b] = ok ? l - ts * p.inv_temp : 0.f;
  }
}

__global__ __launch_bounds__(256) void loss_sum_kernel(const float* __restrict__ terms, int64_t n, float scale,
                                                       float* __restrict__ loss) {
  __shared__ float sh[256];
  float v = 0.f;
  for (int64_t b = threadIdx.x; b < n; b += 256) v += terms[b];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = scale * sh[0];
}

template <int D, bool CAND, bool BIAS>
__global__ __launch_bounds__(64) void dq_chunk_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                      float* __restrict__ part, Offset<BIAS> ob) {
  typedef Mode<CAND> M;
  const int lane = threadIdx.x;
  const int q = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * p.chunk;
  const int64_t c1 = c0 + p.chunk < M::count(p) ? c0 + p.chunk : M::count(p);
  const float coef = gup[0] * p.scale * p.inv_temp;
  QueryLane<D> ql[kNT];
  float row_lse[kNT];
  f32x4 dq[kNT][D / 16];
#pragma unroll
  for (int u = 0; u < kNT; ++u) {
    query_init<D>(p, ((int64_t)blockIdx.x * kNT + u) * 16 + q, M::walk_key(p, c0), g, ql[u]);
    row_lse[u] = lse[ql[u].in ? ql[u].b : p.n_queries - 1];
#pragma unroll
    for (int f = 0; f < D / 16; ++f) dq[u][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t s0 = c0; s0 < c1; s0 += 16) {
    const Tile<CAND> t(p, s0, q, g);
    const TileOffset<BIAS> off(p, ob, s0, q, g);
    float4 a[D / 16];
    load_frag<D>(p.I + M::row(p, t.lane_id) * p.ldi, g, a);
    f32x4 G[kNT];
#pragma unroll
    for (int u = 0; u < kNT; ++u) {
      const f32x4 acc = tile_scores<D>(a, ql[u].qf);
      const unsigned xm = t.excl_bits(p, ql[u].w);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        G[u][r] = grad_at<CAND, BIAS>(acc[r], p, row_lse[u], coef, ql[u].ok, s0 + 4 * g + r < c1, (xm >> r) & 1, t.id(r),
                                      ql[u].ti, off[r]);
    }
    // dQ^T += I^T G: MFMA r contracts over the positions s0 + 4g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) contract_row<D, kNT>(p.I + M::row(p, t.id(r)) * p.ldi + q, r, G, dq);
  }
  // lane (g, q) holds features 16f + 4g .. + 3 of query q
#pragma unroll
  for (int u = 0; u < kNT; ++u)
    if (ql[u].in) store_row<D>(part + ((int64_t)blockIdx.y * p.n_queries + ql[u].b) * D + 4 * g, dq[u]);
}

// Full mode: dQ[b, 4c .. 4c + 3] = the chunk partials added in chunk order
__global__ __launch_bounds__(256) void dq_merge_kernel(const float* __restrict__ part, int64_t n_queries, int d,
                                                       int64_t n_chunks, float* __restrict__ dQ, int64_t lddq) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = d / 4;
  if (e >= n_queries * per_row) return;
  const int64_t b = e / per_row;
  const int c = (int)(e % per_row);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t j = 0; j < n_chunks; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(part + (j * n_queries + b) * d + 4 * c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<float4*>(dQ + b * lddq + 4 * c) = acc;
}

// Candidate mode, one wavefront per query: dQ[b] = the chunk partials added in chunk order, then the target's
// g(b, t_b) I[t_b]; dT[b] = g(b, t_b) Q[b]. The target's score is the forward's tile arithmetic.
template <int D>
__global__ __launch_bounds__(64) void dq_row_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                    const float* __restrict__ part, float* __restrict__ dQ, int64_t lddq,
                                                    float* __restrict__ dT, int64_t lddt) {
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int64_t b = blockIdx.x;
  const int32_t tv = p.target[b];
  const bool ok = tv >= 0 && (int64_t)tv < p.n_items;
  const float* irow = p.I + (int64_t)(ok ? tv : 0) * p.ldi;
  const float* qrow = p.Q + b * p.ldq;
  float4 a[D / 16], qf[D / 16];
  load_frag<D>(irow, g, a);
  load_frag<D>(qrow, g, qf);
  const f32x4 acc = tile_scores<D>(a, qf);
  const float gt = ok ? grad_elem(acc[0], p.inv_temp, lse[b], gup[0] * p.scale * p.inv_temp, true, true) : 0.f;
  if (lane >= D / 4) return;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f), dt = sum;
  for (int64_t j = 0; j < p.n_chunks; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(part + (j * p.n_queries + b) * D + 4 * lane);
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  if (ok) {
    const float4 iv = *reinterpret_cast<const float4*>(irow + 4 * lane);
    const float4 qv = *reinterpret_cast<const float4*>(qrow + 4 * lane);
    sum.x += gt * iv.x; sum.y += gt * iv.y; sum.z += gt * iv.z; sum.w += gt * iv.w;
    dt = make_float4(gt * qv.x, gt * qv.y, gt * qv.z, gt * qv.w);
  }
  *reinterpret_cast<float4*>(dQ + b * lddq + 4 * lane) = sum;
  *reinterpret_cast<float4*>(dT + b * lddt + 4 * lane) = dt;
}

// One wavefront per span of 16 * NI positions from i0; row j of dI belongs to position j. Lane l finds the exclusions
// of query qg + l inside the span as a bit mask over its positions: in full mode by the entries' offsets from i0, in
// candidate mode by a lower bound of each entry among the span's ids, which sit in LDS for that.
template <int D, int NI, bool CAND, bool BIAS>
__global__ __launch_bounds__(64) void di_kernel(Problem p, const float* __restrict__ lse, const float* __restrict__ gup,
                                                float* __restrict__ dI, int64_t lddi, Offset<BIAS> ob) {
  typedef Mode<CAND> M;
  __shared__ int sid[16 * NI];                           // touched, and so allocated, in candidate mode only
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * (16 * NI);
  const float coef = gup[0] * p.scale * p.inv_temp;
  const int n_span = (int)(M::count(p) - i0 < 16 * NI ? M::count(p) - i0 : 16 * NI);
  [[maybe_unused]] int first = 0, last = 0;              // candidate mode: the span's first and last id
  typename M::id_t idv[NI];                              // the id of position i0 + 16v + c
  if constexpr (CAND) {
    if (lane < 16 * NI) sid[lane] = M::id_at(p, i0 + lane);
    __syncthreads();
    first = sid[0];
    last = sid[n_span - 1];
#pragma unroll
    for (int v = 0; v < NI; ++v) idv[v] = sid[16 * v + c];
  } else {
#pragma unroll
    for (int v = 0; v < NI; ++v) idv[v] = M::id_at(p, i0 + 16 * v + c);
  }
  float4 ib[NI][D / 16];                                 // item rows as the B side of the scores
  f32x4 di[NI][D / 16];
  [[maybe_unused]] float offv[NI];                       // the offset of position i0 + 16v + c, -inf past the span
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    offv[v] = ob.at(p, i0 + 16 * v + c);
    load_frag<D>(p.I + M::row(p, idv[v]) * p.ldi, g, ib[v]);
#pragma unroll
    for (int f = 0; f < D / 16; ++f) di[v][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t qg = 0; qg < p.n_queries; qg += 64) {
    unsigned mask_lo = 0, mask_hi = 0;
    if (p.excl_ptr && qg + lane < p.n_queries) {
      int64_t lo, hi;
      excl_range(p, qg + lane, lo, hi);
      if constexpr (CAND) {
        int64_t ep = excl_lower_bound(p.excl_items, lo, hi, first);
        while (ep < hi) {
          const int e = p.excl_items[ep];
          if (e > last) break;
          int x = 0, y = n_span;
          while (x < y) {
            const int mid = (x + y) >> 1;
            if (sid[mid] < e) x = mid + 1; else y = mid;
          }
          if (x < n_span && sid[x] == e) {
            if (x < 32) mask_lo |= 1u << x; else mask_hi |= 1u << (x - 32);
          }
          ++ep;
        }
      } else {
        int64_t ep = excl_lower_bound(p.excl_items, lo, hi, i0);
        while (ep < hi) {
          const int64_t off = (int64_t)p.excl_items[ep] - i0;
          if (off >= 16 * NI) break;
          if (off >= 0) {
            if (off < 32) mask_lo |= 1u << off; else mask_hi |= 1u << (off - 32);
          }
          ++ep;
        }
      }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int64_t qb = qg + 16 * j;
      if (qb >= p.n_queries) break;                      // uniform over the wavefront
      int64_t ra = qb + c;                               // the A row of the scores
      if (ra >= p.n_queries) ra = p.n_queries - 1;
      float4 qa[D / 16];
      load_frag<D>(p.Q + ra * p.ldq, g, qa);
      // the four queries qb + 4g + r of this lane's accumulator rows
      float row_lse[4];
      int ti[4];
      unsigned xl[4], xh[4];
      int64_t rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = qb + 4 * g + r;
        const bool in = b < p.n_queries;
        rq[r] = in ? b : p.n_queries - 1;
        const int32_t tv = p.target[rq[r]];
        ti[r] = (in && tv >= 0 && (int64_t)tv < p.n_items) ? tv : -1;
        row_lse[r] = lse[rq[r]];
        xl[r] = __shfl(mask_lo, 16 * j + 4 * g + r);
        xh[r] = __shfl(mask_hi, 16 * j + 4 * g + r);
      }
      f32x4 G[NI];
#pragma unroll
      for (int v = 0; v < NI; ++v) {
        const f32x4 acc = tile_scores<D>(qa, ib[v]);     // acc[r] = score(query qb + 4g + r, position i0 + 16v + c)
        const int off = 16 * v + c;
        const bool inside = M::in_span(p, i0, off, n_span);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ex = ((off < 32 ? xl[r] >> off : xh[r] >> (off - 32)) & 1) != 0;
          G[v][r] = grad_at<CAND, BIAS>(acc[r], p, row_lse[r], coef, ti[r] >= 0 && inside, true, ex, idv[v], ti[r], offv[v]);
        }
      }
      // dI^T += Q^T G: MFMA r contracts over queries qb + 4g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) contract_row<D, NI>(p.Q + rq[r] * p.ldq + c, r, G, di);
    }
  }
  // lane (g, c) holds features 16f + 4g .. + 3 of position i0 + 16v + c
#pragma unroll
  for (int v = 0; v < NI; ++v) {
    if (M::in_span(p, i0, 16 * v + c, n_span)) store_row<D>(dI + (i0 + 16 * v + c) * lddi + 4 * g, di[v]);
  }
}

// Candidate mode's dT into a full-size dI (sagnn_softmax_target_add_f32).
// dI[t] +=the dT rows of the queries whose target is t, in ascending query order, by the first such query: one
// wavefront per query. 64 lanes compare 64 targets at a time (a ballot); the owner then walks the set bits upwards, its
// first d / 4 lanes holding one float4 column each, so every dI element has one writer and the sum one order.
__global__ __launch_bounds__(64) void target_add_kernel(const float* __restrict__ dT, int64_t lddt,
                                                        const int32_t* __restrict__ target, int64_t n_queries,
                                                        int64_t n_items, int d, float* __restrict__ dI, int64_t lddi) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int32_t t = target[b];
  if (t < 0 || (int64_t)t >= n_items) return;            // uniform over the wavefront, as every branch below
  for (int64_t o0 = 0; o0 < b; o0 += 64) {
    const int64_t o = o0 + lane;
    if (__ballot(o < b && target[o] == t)) return;       // an earlier query owns the row
  }
  const bool col = lane < d / 4;
  float* out = dI + (int64_t)t * lddi + 4 * lane;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col) acc = *reinterpret_cast<const float4*>(out);
  for (int64_t o0 = b & ~(int64_t)63; o0 < n_queries; o0 += 64) {
    const int64_t o = o0 + lane;
    unsigned long long m = __ballot(o >= b && o < n_queries && target[o] == t);
    while (m) {
      const int k = __ffsll(m) - 1;
      m &= m - 1;
      if (col) {
        const float4 v = *reinterpret_cast<const float4*>(dT + (o0 + k) * lddt + 4 * lane);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  }
  if (col) *reinterpret_cast<float4*>(out) = acc;
}

// The dIc rows of the live positions into a full-size dI (sagnn_softmax_cand_scatter_f32): dI[cand[j]] = dIc[j] where
// bias[j] > -inf. One thread per (position, float4 column); the live positions' ids are distinct, so a dI row has one
// writer at most and the result does not depend on the order of the threads.
__global__ __launch_bounds__(256) void cand_scatter_kernel(const float* __restrict__ dIc, int64_t lddic,
                                                           const int32_t* __restrict__ cand, const float* __restrict__ bias,
                                                           int64_t n_cand, int64_t n_items, int d, float* __restrict__ dI,
                                                           int64_t lddi) {
  const int per_row = d / 4;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_cand * per_row) return;
  const int64_t j = e / per_row;
  const int c = (int)(e - j * per_row);
  const int64_t id = cand[j];
  if (!(bias[j] > -INFINITY) || id < 0 || id >= n_items) return;
  *reinterpret_cast<float4*>(dI + id * lddi + 4 * c) = *reinterpret_cast<const float4*>(dIc + j * lddic + 4 * c);
}

// dT into a full-size dI where the rows number far more than a batch (sagnn_softmax_target_scatter_f32, --seqTargets
// all: every token of the slab is a row): dI[target[r]] += dT[r] with float atomics, one thread per (row, float4
// column), the scatter of seq_gather_scatter_kernel. target_add_kernel compares every row's target with every other's.
__global__ __launch_bounds__(256) void target_scatter_kernel(const float* __restrict__ dT, int64_t lddt,
                                                             const int32_t* __restrict__ target, int64_t n_rows,
                                                             int64_t n_items, int d, float* __restrict__ dI, int64_t lddi) {
  const int per_row = d / 4;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_rows * per_row) return;
  const int64_t r = e / per_row;
  const int c = (int)(e - r * per_row);
  const int64_t t = target[r];
  if (t < 0 || t >= n_items) return;
  const float4 v = *reinterpret_cast<const float4*>(dT + r * lddt + 4 * c);
  float* o = dI + t * lddi + 4 * c;
  atomicAdd(o + 0, v.x);
  atomicAdd(o + 1, v.y);
  atomicAdd(o + 2, v.z);
  atomicAdd(o + 3, v.w);
}

// Workspace: forward = (max, sum) per (query, chunk) then one loss term per query; backward = dQ partials per chunk.
struct Layout {
  int64_t chunk, n_chunks;
  size_t terms_off, bytes;
};

inline Layout layout(int64_t n_queries, int64_t n_items, int d) {
  Layout L;
  L.chunk = chunk_items(n_items);
  L.n_chunks = (n_items + L.chunk - 1) / L.chunk;
  // sized by a bound on n_chunks that grows with n_items (n_chunks itself dips where the chunk size steps up)
  int64_t bound = (n_items + kMinChunk - 1) / kMinChunk;
  if (bound > kMaxChunks) bound = kMaxChunks;
  L.terms_off = ((size_t)n_queries * bound * sizeof(float2) + 255) & ~(size_t)255;
  const size_t fwd = L.terms_off + (((size_t)n_queries * sizeof(float) + 255) & ~(size_t)255);
  const size_t bwd = ((size_t)bound * n_queries * d * sizeof(float) + 255) & ~(size_t)255;
  L.bytes = fwd > bwd ? fwd : bwd;
  return L;
}

template <int D, bool CAND, bool BIAS>
int launch_fwd(const Problem& p, const Offset<BIAS>& ob, const Layout& L, float* loss, float* lse, float* tscore,
               void* workspace, hipStream_t s) {
  float2* part = reinterpret_cast<float2*>(workspace);
  float* terms = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + L.terms_off);
  if (p.n_queries > 0) {
    if (L.n_chunks > 0) {                                // an empty candidate list has no chunk
      const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
      hipLaunchKernelGGL((lse_chunk_kernel<D, CAND, BIAS>), grid1, dim3(64), 0, s, p, part, ob);
      SAGNN_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((lse_row_kernel<D, CAND>), dim3((unsigned)p.n_queries), dim3(64), 0, s, p, part, lse, tscore, terms);
    SAGNN_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, terms, p.n_queries, p.scale, loss);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

// dI has one row per position; dT is candidate mode's
template <int D, bool CAND, bool BIAS>
int launch_bwd(const Problem& p, const Offset<BIAS>& ob, const Layout& L, const float* lse, const float* g, float* dQ,
               int64_t lddq, float* dI, int64_t lddi, float* dT, int64_t lddt, void* workspace, hipStream_t s) {
  constexpr int NI = D == 128 ? 2 : 4;
  float* part = reinterpret_cast<float*>(workspace);
  if (p.n_queries > 0) {
    if (L.n_chunks > 0) {
      const dim3 grid1((unsigned)((p.n_queries + 16 * kNT - 1) / (16 * kNT)), (unsigned)L.n_chunks);
      hipLaunchKernelGGL((dq_chunk_kernel<D, CAND, BIAS>), grid1, dim3(64), 0, s, p, lse, g, part, ob);
      SAGNN_HIP_TRY(hipGetLastError());
    }
    if constexpr (CAND) {
      hipLaunchKernelGGL(dq_row_kernel<D>, dim3((unsigned)p.n_queries), dim3(64), 0, s, p, lse, g, part, dQ, lddq, dT, lddt);
    } else {
      const int64_t vecs = p.n_queries * (D / 4);
      hipLaunchKernelGGL(dq_merge_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, s, part, p.n_queries, D,
                         L.n_chunks, dQ, lddq);
    }
    SAGNN_HIP_TRY(hipGetLastError());
  }
  const int64_t n = CAND ? p.n_cand : p.n_items;
  if (n > 0) {
    const int64_t spans = (n + 16 * NI - 1) / (16 * NI);
    if constexpr (CAND) {
      // a short list at 16 positions per wavefront, so that it still fills the part; an item's sum over the queries has
      // the same order in both forms
      if (spans < kSmallSpans)
        hipLaunchKernelGGL((di_kernel<D, 1, true, BIAS>), dim3((unsigned)((n + 15) / 16)), dim3(64), 0, s, p, lse, g, dI, lddi, ob);
      else
        hipLaunchKernelGGL((di_kernel<D, NI, true, BIAS>), dim3((unsigned)spans), dim3(64), 0, s, p, lse, g, dI, lddi, ob);
    } else {
      hipLaunchKernelGGL((di_kernel<D, NI, false, false>), dim3((unsigned)spans), dim3(64), 0, s, p, lse, g, dI, lddi, ob);
    }
    SAGNN_HIP_TRY(hipGetLastError());
  }
  return SAGNN_OK;
}

// f(std::integral_constant<int, d>()) for a d that check_common let through
template <class F>
int dispatch_d(int d, F f) {
  switch (d) {
    case 32: return f(std::integral_constant<int, 32>());
    case 64: return f(std::integral_constant<int, 64>());
    default: return f(std::integral_constant<int, 128>());
  }
}

// f(CAND, BIAS) as std::bool_constant for a mode that check_mode let through
template <class F>
int dispatch_mode(int mode, F f) {
  switch (mode) {
    case SAGNN_SOFTMAX_FULL: return f(std::false_type(), std::false_type());
    case SAGNN_SOFTMAX_CAND: return f(std::true_type(), std::false_type());
    default: return f(std::true_type(), std::true_type());
  }
}

// The struct itself and the form args->mode names, ahead of everything else: the mode decides the name in the messages.
int check_mode(const sagnn_softmax_args* a) {
  if (!a) return sagnn::fail(SAGNN_ERR_NULL, "the sagnn_softmax_args is NULL");
  switch (a->mode) {
    case SAGNN_SOFTMAX_FULL:
      if (a->cand) return sagnn::fail(SAGNN_ERR_ARG, "mode = SAGNN_SOFTMAX_FULL with a cand");
      if (a->bias) return sagnn::fail(SAGNN_ERR_ARG, "mode = SAGNN_SOFTMAX_FULL with a bias");
      if (a->n_cand != 0) return sagnn::fail(SAGNN_ERR_ARG, "mode = SAGNN_SOFTMAX_FULL with n_cand = %lld", (long long)a->n_cand);
      return SAGNN_OK;
    case SAGNN_SOFTMAX_CAND:
      if (a->bias) return sagnn::fail(SAGNN_ERR_ARG, "mode = SAGNN_SOFTMAX_CAND with a bias");
      return SAGNN_OK;
    case SAGNN_SOFTMAX_CAND_BIAS: return SAGNN_OK;
  }
  return sagnn::fail(SAGNN_ERR_ARG, "mode = %d: not a SAGNN_SOFTMAX_* value", a->mode);
}

// The checks both entries share in every mode; `who` prefixes the message.
int check_common(const char* who, const sagnn_softmax_args& a) {
  if (!a.Q || !a.I) return sagnn::fail(SAGNN_ERR_NULL, "%s: null Q or I", who);
  if (!a.target) return sagnn::fail(SAGNN_ERR_NULL, "%s: null target", who);
  if ((a.excl_ptr == nullptr) != (a.excl_items == nullptr))
    return sagnn::fail(SAGNN_ERR_NULL, "%s: excl_ptr and excl_items go together", who);
  if (a.excl_row && !a.excl_ptr) return sagnn::fail(SAGNN_ERR_NULL, "%s: excl_row without excl_ptr / excl_items", who);
  if (a.d != 32 && a.d != 64 && a.d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, a.d);
  if (a.n_queries < 0 || a.n_queries > INT32_MAX)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_queries = %lld", who, (long long)a.n_queries);
  if (a.n_items < 1 || a.n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)a.n_items);
  if (!(a.inv_temp > 0.f) || !isfinite(a.inv_temp))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: inv_temp = %g, need a finite value > 0", who, (double)a.inv_temp);
  if (!isfinite(a.scale)) return sagnn::fail(SAGNN_ERR_ARG, "%s: scale = %g is not finite", who, (double)a.scale);
  if (a.excl_ptr && a.n_lists < 0) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_lists = %lld", who, (long long)a.n_lists);
  if (a.excl_ptr && !a.excl_row && a.n_lists < a.n_queries)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: %lld exclusion lists for %lld rows and no excl_row", who, (long long)a.n_lists,
                       (long long)a.n_queries);
  if ((a.ldq & 3) || (a.ldi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides ldq / ldi must be multiples of 4", who);
  if (a.ldq < a.d || a.ldi < a.d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides ldq / ldi must be >= d", who);
  if (!sagnn::aligned16(a.Q) || !sagnn::aligned16(a.I))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: Q and I must be 16-byte aligned", who);
  return SAGNN_OK;
}

// The candidate modes' own checks.
int check_cand(const char* who, const sagnn_softmax_args& a) {
  if (a.n_cand < 0 || a.n_cand > a.n_items)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_cand = %lld, need 0 <= n_cand <= n_items = %lld", who, (long long)a.n_cand,
                       (long long)a.n_items);
  if (a.n_cand > 0 && !a.cand) return sagnn::fail(SAGNN_ERR_NULL, "%s: null cand", who);
  if (a.mode == SAGNN_SOFTMAX_CAND_BIAS && a.n_cand > 0 && !a.bias) return sagnn::fail(SAGNN_ERR_NULL, "%s: null bias", who);
  return SAGNN_OK;
}

int check_workspace(const char* who, size_t need, const sagnn_softmax_args& a) {
  if (need == 0) return SAGNN_OK;
  if (!a.workspace || a.workspace_bytes < need)
    return sagnn::fail(SAGNN_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, a.workspace_bytes, need);
  if (!sagnn::aligned16(a.workspace)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: workspace must be 16-byte aligned", who);
  return SAGNN_OK;
}

int check_fwd_outputs(const char* who, const sagnn_softmax_args& a) {
  if (!a.loss || !a.lse || !a.tscore) return sagnn::fail(SAGNN_ERR_NULL, "%s: null loss, lse or tscore", who);
  return SAGNN_OK;
}

// The backward's inputs and its output matrices of d columns: dQ and dI, and in the candidate modes, where dI is the
// [n_cand, d] dIc, dT as well. The messages name them.
int check_bwd_outputs(const char* who, const sagnn_softmax_args& a) {
  const bool cand = a.mode != SAGNN_SOFTMAX_FULL;
  const int n = cand ? 3 : 2;
  const char* any = cand ? "dQ, dIc or dT" : "dQ or dI";
  const char* strides = cand ? "lddq / lddic / lddt" : "lddq / lddi";
  const char* all = cand ? "dQ, dIc and dT" : "dQ and dI";
  float* const out[] = {a.dQ, a.dI, a.dT};
  const int64_t ld[] = {a.lddq, a.lddi, a.lddt};
  if (!a.lse || !a.g) return sagnn::fail(SAGNN_ERR_NULL, "%s: null lse or g", who);
  for (int k = 0; k < n; ++k)
    if (!out[k]) return sagnn::fail(SAGNN_ERR_NULL, "%s: null %s", who, any);
  for (int k = 0; k < n; ++k)
    if (ld[k] & 3) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides %s must be multiples of 4", who, strides);
  for (int k = 0; k < n; ++k)
    if (ld[k] < a.d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides %s must be >= d", who, strides);
  for (int k = 0; k < n; ++k)
    if (!sagnn::aligned16(out[k])) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: %s must be 16-byte aligned", who, all);
  return SAGNN_OK;
}

// Both entries: the checks in the order of their messages (the mode, the shared ones, the candidates, the entry's own
// pointers, the workspace), the problem, then the launches of the mode and of d.
int run(const sagnn_softmax_args* args, bool backward, void* stream) {
  static const char* const names[3][2] = {{"softmax_loss", "softmax_loss_bwd"},
                                          {"softmax_loss_cand", "softmax_loss_cand_bwd"},
                                          {"softmax_loss_candb", "softmax_loss_candb_bwd"}};
  if (int rc = check_mode(args)) return rc;
  const sagnn_softmax_args& a = *args;
  const char* who = names[a.mode][backward];
  const bool cand = a.mode != SAGNN_SOFTMAX_FULL;
  if (int rc = check_common(who, a)) return rc;
  if (cand)
    if (int rc = check_cand(who, a)) return rc;
  if (int rc = backward ? check_bwd_outputs(who, a) : check_fwd_outputs(who, a)) return rc;
  const int64_t n_pos = cand ? a.n_cand : a.n_items;
  const Layout L = layout(a.n_queries, n_pos, a.d);
  if (int rc = check_workspace(who, L.bytes, a)) return rc;
  const Problem p{a.Q, a.ldq, a.I, a.ldi, a.n_queries, a.n_items, a.target, a.inv_temp, a.scale, a.excl_ptr, a.excl_items,
                  a.excl_row, a.n_lists, L.chunk, L.n_chunks, a.cand, a.n_cand};
  hipStream_t s = static_cast<hipStream_t>(stream);
  sagnn::ProfileScope prof(cand ? sagnn::kProfSoftmaxLossCand : sagnn::kProfSoftmaxLoss, s, a.n_queries, n_pos);
  return dispatch_mode(a.mode, [&](auto C, auto B) {
    constexpr bool CAND = decltype(C)::value, BIAS = decltype(B)::value;
    Offset<BIAS> ob;
    if constexpr (BIAS) ob.bias = a.bias;
    // a mode's three forwards are named before its three backwards: that is the kernels' order in the code object
    if (!backward)
      return dispatch_d(a.d, [&](auto D) {
        return launch_fwd<decltype(D)::value, CAND, BIAS>(p, ob, L, a.loss, a.lse, a.tscore, a.workspace, s);
      });
    return dispatch_d(a.d, [&](auto D) {
      return launch_bwd<decltype(D)::value, CAND, BIAS>(p, ob, L, a.lse, a.g, a.dQ, a.lddq, a.dI, a.lddi, a.dT, a.lddt,
                                                        a.workspace, s);
    });
  });
}

}  // namespace

extern "C" size_t sagnn_softmax_loss_workspace_bytes(int64_t n_queries, int64_t n_items, int d) {
  if (n_queries < 0 || n_items <= 0 || d <= 0) return 0;
  return layout(n_queries, n_items, d).bytes;
}

extern "C" size_t sagnn_softmax_loss_cand_workspace_bytes(int64_t n_queries, int64_t n_cand, int d) {
  if (n_queries < 0 || n_cand < 0 || d <= 0) return 0;
  return layout(n_queries, n_cand, d).bytes;
}

extern "C" int sagnn_softmax_loss_f32(const sagnn_softmax_args* args, void* stream) { return run(args, false, stream); }

extern "C" int sagnn_softmax_loss_bwd_f32(const sagnn_softmax_args* args, void* stream) { return run(args, true, stream); }

extern "C" int sagnn_softmax_target_add_f32(const float* dT, int64_t lddt, const int32_t* target, int64_t n_queries,
                                            int64_t n_items, int d, float* dI, int64_t lddi, void* stream) {
  const char* who = "softmax_target_add";
  if (!dT || !target || !dI) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dT, target or dI", who);
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (n_queries < 0 || n_queries > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_queries = %lld", who, (long long)n_queries);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)n_items);
  if ((lddt & 3) || (lddi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddt / lddi must be multiples of 4", who);
  if (lddt < d || lddi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddt / lddi must be >= d", who);
  if (!sagnn::aligned16(dT) || !sagnn::aligned16(dI))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dT and dI must be 16-byte aligned", who);
  if (n_queries == 0) return SAGNN_OK;
  hipLaunchKernelGGL(target_add_kernel, dim3((unsigned)n_queries), dim3(64), 0, static_cast<hipStream_t>(stream), dT, lddt,
                     target, n_queries, n_items, d, dI, lddi);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_softmax_target_scatter_f32(const float* dT, int64_t lddt, const int32_t* target, int64_t n_rows,
                                                int64_t n_items, int d, float* dI, int64_t lddi, void* stream) {
  const char* who = "softmax_target_scatter";
  if (!dT || !target || !dI) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dT, target or dI", who);
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (n_rows < 0 || n_rows > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: n_rows = %lld", who, (long long)n_rows);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)n_items);
  if ((lddt & 3) || (lddi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddt / lddi must be multiples of 4", who);
  if (lddt < d || lddi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddt / lddi must be >= d", who);
  if (!sagnn::aligned16(dT) || !sagnn::aligned16(dI))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dT and dI must be 16-byte aligned", who);
  if (n_rows == 0) return SAGNN_OK;
  const int64_t blocks = (n_rows * (d / 4) + 255) / 256;
  if (blocks > INT32_MAX) return sagnn::fail(SAGNN_ERR_ARG, "%s: %lld rows exceed one launch", who, (long long)n_rows);
  hipLaunchKernelGGL(target_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), dT, lddt,
                     target, n_rows, n_items, d, dI, lddi);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}

extern "C" int sagnn_softmax_cand_scatter_f32(const float* dIc, int64_t lddic, const int32_t* cand, const float* bias,
                                              int64_t n_cand, int64_t n_items, int d, float* dI, int64_t lddi, void* stream) {
  const char* who = "softmax_cand_scatter";
  if (d != 32 && d != 64 && d != 128) return sagnn::fail(SAGNN_ERR_DIM, "%s: d = %d, need 32, 64 or 128", who, d);
  if (n_items < 1 || n_items >= ((int64_t)1 << 31))
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_items = %lld, need 1 <= n_items < 2^31", who, (long long)n_items);
  if (n_cand < 0 || n_cand > n_items)
    return sagnn::fail(SAGNN_ERR_ARG, "%s: n_cand = %lld, need 0 <= n_cand <= n_items = %lld", who, (long long)n_cand,
                       (long long)n_items);
  if (!dI || (n_cand > 0 && (!dIc || !cand || !bias))) return sagnn::fail(SAGNN_ERR_NULL, "%s: null dIc, cand, bias or dI", who);
  if ((lddic & 3) || (lddi & 3)) return sagnn::fail(SAGNN_ERR_ALIGN, "%s: strides lddic / lddi must be multiples of 4", who);
  if (lddic < d || lddi < d) return sagnn::fail(SAGNN_ERR_ARG, "%s: strides lddic / lddi must be >= d", who);
  if (!sagnn::aligned16(dI) || (n_cand > 0 && !sagnn::aligned16(dIc)))
    return sagnn::fail(SAGNN_ERR_ALIGN, "%s: dIc and dI must be 16-byte aligned", who);
  if (n_cand == 0) return SAGNN_OK;
  const int64_t vecs = n_cand * (d / 4);
  hipLaunchKernelGGL(cand_scatter_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     dIc, lddic, cand, bias, n_cand, n_items, d, dI, lddi);
  SAGNN_HIP_TRY(hipGetLastError());
  return SAGNN_OK;
}
