// The head score <U[u], I[i]> + <leaky(S[b]), A[i]> (reference model.py:169-173), shared by sagnn_pair_score_f32
// (fusion_bwd.hip) and sagnn_candidate_rank_f32 (evaluate.hip) so that both return the same bits for a triple.
// Lane layout: lpr = d / 4 lanes per pair (a power of two <= 64), lane (lane % lpr) holds columns col .. col + 3 with
// col = (lane % lpr) * 4. The per-lane arithmetic and the __shfl_xor reduction order are fixed here: any change moves
// the last bit of both entries at once.
#pragma once

#include <hip/hip_runtime.h>

namespace sagnn {

// One lane's share of the score, reduced over the lpr lanes of its pair. `rows(u, i, s, a)` sets the row pointers of
// the lane's pair (U, I, S, A rows; s and a only read with `head`) and runs only when `active`; an inactive lane
// contributes 0. Every lane of the wavefront must call it (the shuffles). Returns the pair's score in every lane of
// the pair.
template <class Rows>
__device__ __forceinline__ float pair_score_lanes(bool active, bool head, Rows rows, float leaky, int col, int lpr) {
  float acc = 0.f;
  if (active) {
    const float *ur, *ir, *sr = nullptr, *ar = nullptr;
    rows(ur, ir, sr, ar);
    const float4 a = *reinterpret_cast<const float4*>(ur + col);
    const float4 b = *reinterpret_cast<const float4*>(ir + col);
    acc = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    if (head) {
      const float4 s = *reinterpret_cast<const float4*>(sr + col);
      const float4 c = *reinterpret_cast<const float4*>(ar + col);
      acc += fmaxf(leaky * s.x, s.x) * c.x + fmaxf(leaky * s.y, s.y) * c.y + fmaxf(leaky * s.z, s.z) * c.z +
             fmaxf(leaky * s.w, s.w) * c.w;
    }
  }
  for (int off = 1; off < lpr; off <<= 1) acc += __shfl_xor(acc, off);
  return acc;
}

}  // namespace sagnn
