// philox_device.h — the counter-based generator the augmentation (augment.hip) and the 3-D pose sampler (pose3d.hip) share:
// Philox4x64-10 with np.random.Philox's constants. One definition: tests/test_gpu_augment.py pins its words against numpy's.
#pragma once

#include "pcnn_device.h"

namespace pcnn {

__device__ __forceinline__ void mulhilo(unsigned long long a, unsigned long long b, unsigned long long& hi,
                                        unsigned long long& lo)
{
  hi = __umul64hi(a, b);
  lo = a * b;
}

// Philox4x64-10, np.random.Philox's constants: the block of counter (c0, c1, c2, 0) under key (k0, k1)
__device__ __forceinline__ void philox4x64(unsigned long long c0, unsigned long long c1, unsigned long long c2,
                                           unsigned long long k0, unsigned long long k1, unsigned long long out[4])
{
  unsigned long long c3 = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    unsigned long long hi0, lo0, hi1, lo1;
    mulhilo(0xD2E7470EE14C6C93ull, c0, hi0, lo0);
    mulhilo(0xCA5A826395121157ull, c2, hi1, lo1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B97F4A7C15ull;
    k1 += 0xBB67AE8584CAA73Bull;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

}  // namespace pcnn
