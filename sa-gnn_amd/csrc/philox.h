// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the one counter-based generator of
// the library. The device sampler (sampler.hip) and the edge dropout of the interval SpMM (spmm.hip) both draw from
// this copy; tests/device_sampler_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sagnn {

struct Word4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ Word4 philox4x32_10(Word4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = Word4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
  }
  return c;
}

}  // namespace sagnn
