// sl1_gt_device.h — what the two target-free forms of the vertex loss share (vertex_targets.hip: the prediction is a
// [B,H,W,3C] tensor; vertex_head_loss.hip: it is interpolated from the 1/8-resolution field where it is needed): the row
// match of include/posecnn_hip_train.h and the forward's partial kernel, templated on where an element's prediction comes
// from. One definition, so the two forwards cannot drift apart: they are held to each other bit for bit
// (tests/test_gpu_vertex_head.py).
#pragma once

#include "sl1_device.h"

namespace {

constexpr int SL1_GT_UNROLL = 8;   // labels in flight per thread (4 waves per SIMD: the loads need the ILP)

// The highest-index row of `tab` ([M,6]: cls, mask_id, cx, cy, log_z, w) that matches label l / instance inst at
// pixel (x, y) -> its targets and weight. No early exit: the M row reads are independent of each other.
__device__ __forceinline__ bool vt_match(const float* tab, int M, int l, int inst, int x, int y, float& tx,
                                         float& ty, float& tz, float& w)
{
  const float lf = (float)l, instf = (float)inst;
  int sel = -1;
  for (int j = 0; j < M; ++j) {
    const float cls = tab[6 * j], mid = tab[6 * j + 1];
    if (cls == lf && (mid == 0.f || mid == instf)) sel = j;
  }
  if (sel < 0) return false;
  const double dx = (double)tab[6 * sel + 2] - (double)x;
  const double dy = (double)tab[6 * sel + 3] - (double)y;
  const double n = __builtin_sqrt(dx * dx + dy * dy) + 1e-10;
  tx = (float)(dx / n);
  ty = (float)(dy / n);
  tz = tab[6 * sel + 4];
  w = tab[6 * sel + 5];
  return true;
}

// Where element i = channel ch of pixel (x, y) of frame f finds its prediction: the [B,H,W,3C] tensor itself.
struct PredTensor {
  const float* pred;
  __device__ __forceinline__ float operator()(long long i, int, int, int, int) const { return pred[i]; }
};

// Thread (blk, t) takes elements blk*256 + t + m*SL1_BLOCKS*256, m ascending (the order of sl1_partial_kernel); the
// prediction is fetched only under a matching row. qs / rs: quotient and remainder of the element stride
// SL1_BLOCKS * 256 by 3C.
template <class Pred>
__global__ __launch_bounds__(256) void sl1_gt_partial_kernel(const Pred pred, const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ instance,
                                                             const float* __restrict__ objects, long long n,
                                                             int HW, int W, int C, int M, float sigma2, int qs,
                                                             int rs, float* __restrict__ partial)
{
  __shared__ float sl[256], sw[256];
  const int t = threadIdx.x;
  const int C3 = 3 * C;
  constexpr long long STRIDE = (long long)SL1_BLOCKS * 256;
  float al = 0.f, aw = 0.f;
  int pix = (blockIdx.x * 256 + t) / C3, ch = (blockIdx.x * 256 + t) - pix * C3;
  for (long long i = (long long)blockIdx.x * 256 + t; i < n; i += STRIDE * SL1_GT_UNROLL) {
    int lab[SL1_GT_UNROLL], px[SL1_GT_UNROLL], cc[SL1_GT_UNROLL];
#pragma unroll
    for (int k = 0; k < SL1_GT_UNROLL; ++k) {
      px[k] = pix;
      cc[k] = ch;
      lab[k] = i + k * STRIDE < n ? label[pix] : 0;   // past the end: background, adds nothing
      pix += qs;
      ch += rs;
      if (ch >= C3) {
        ch -= C3;
        ++pix;
      }
    }
#pragma unroll
    for (int k = 0; k < SL1_GT_UNROLL; ++k) {   // m ascending: the accumulation order of sl1_partial_kernel
      const int l = lab[k];
      const int d = cc[k] - 3 * l;
      if (l > 0 && l < C && (unsigned)d < 3u) {
        const int f = px[k] / HW, rem = px[k] - f * HW;
        const int y = rem / W, x = rem - y * W;
        const int inst = instance ? instance[px[k]] : 0;
        float tx, ty, tz, w;
        if (vt_match(objects + (long long)f * M * 6, M, l, inst, x, y, tx, ty, tz, w)) {
          float il, dp;
          sl1_elem(pred(i + k * STRIDE, f, y, x, cc[k]), d == 0 ? tx : (d == 1 ? ty : tz), w, sigma2, il, dp);
          al = al + il;
          aw = aw + w;
        }
      }
    }
  }
  sl[t] = al;
  sw[t] = aw;
  block_tree_sum<256>(sl, sw, t);
  if (t == 0) {
    partial[blockIdx.x] = sl[0];
    partial[SL1_BLOCKS + blockIdx.x] = sw[0];
  }
}

}  // namespace
