// sl1_device.h — what the two forms of the vertex loss share (losses.hip: pred / target / weight tensors;
// vertex_targets.hip: label map + object table): the element arithmetic of smooth_l1_loss_vertex
// (lib/fcn/train.py:564-573), the number of partial sums and the kernel that folds them. One definition, so the two
// forward kernels cannot drift apart: they are held to each other bit for bit (tests/test_gpu_vertex_targets.py).
#pragma once

#include "reduce_device.h"

namespace {

using namespace pcnn;

constexpr int SL1_BLOCKS = 1024;

__device__ __forceinline__ void sl1_elem(float p, float t, float w, float sigma2, float& in_loss,
                                         float& dpred)
{
  const float diff = w * (p - t);
  const float ad = fabsf(diff);
  const float inv = div_rn(1.0f, sigma2);
  if (ad < inv) {
    in_loss = (diff * diff) * div_rn(sigma2, 2.0f);
    dpred = w * (sigma2 * diff);
  } else {
    in_loss = ad - div_rn(0.5f, sigma2);
    dpred = w * (diff > 0.f ? 1.0f : (diff < 0.f ? -1.0f : 0.0f));
  }
}

__global__ __launch_bounds__(SL1_BLOCKS / 2) void sl1_final_kernel(const float* __restrict__ partial,
                                                                   float* __restrict__ out)
{
  __shared__ float sl[SL1_BLOCKS], sw[SL1_BLOCKS];
  const int t = threadIdx.x;
  sl[t] = partial[t];
  sl[t + SL1_BLOCKS / 2] = partial[t + SL1_BLOCKS / 2];
  sw[t] = partial[SL1_BLOCKS + t];
  sw[t + SL1_BLOCKS / 2] = partial[SL1_BLOCKS + t + SL1_BLOCKS / 2];
  block_tree_sum<SL1_BLOCKS>(sl, sw, t);
  if (t == 0) {
    const float denom = sw[0] + 1e-10f;
    out[0] = div_rn(sl[0], denom);
    out[1] = sl[0];
    out[2] = sw[0];
  }
}

}  // namespace
