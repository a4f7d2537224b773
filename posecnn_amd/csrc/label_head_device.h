// label_head_device.h — what the label-head epilogue (upscore.hip) and its training twin (label_loss.hip) share: the
// 128-pixel segment a workgroup owns and the copy of its low-resolution cells into LDS, the per-pixel arithmetic
// (interpolate -> bias -> ReLU, then softmax -> first argmax), and the host-side tile plan. One definition, so label and
// prob of the two entries cannot drift apart: they are held to each other bit for bit (tests/test_gpu_label_loss.py).
#pragma once

#include "bilinear.h"

namespace pcnn {

constexpr int LH_SEG = 128;   // pixels (= threads) per workgroup

// ---- the segment --------------------------------------------------------------------------------------------------------
// Workgroup blockIdx.x owns pixels ox0 .. ox0 + npx - 1 of output row oy of frame b; they read input rows ty.i0 ..,
// input columns cx0 .. cx0 + ncx - 1.
struct Segment {
  int b, oy, ox0, npx, cx0, ncx;
  Taps ty;
};

// The segment's geometry, the k tap weights in s_tab (evaluated once per workgroup, in double like make_deconv_filter;
// everything after is integer arithmetic + lookups) and its ty.n rows of ncx cells x C channels in s_z as [ty.n][ncx][C].
// A row is one contiguous run of z: FOUR loads per thread issued before the first LDS write (a row-by-row copy loop is a
// load, a wait and a store per trip — four trips to memory in sequence in front of every workgroup's first barrier).
// Must be called by every thread of the workgroup; ends in a barrier. upscore_softmax_argmax_fixed_kernel keeps its own
// float2 form of this: routed through here its instruction stream changes (upscore.hip).
__device__ __forceinline__ Segment load_segment(const float* __restrict__ z, float* s_z, float* s_tab, int H, int W, int C,
                                                int k, int s, int nseg)
{
  const int pad = (k - s) / 2;
  const int Ho = H * s, Wo = W * s;
  const int seg = blockIdx.x % nseg;
  const int oy = (blockIdx.x / nseg) % Ho;
  const int b = blockIdx.x / (nseg * Ho);
  const int ox0 = seg * LH_SEG;
  const int npx = min(LH_SEG, Wo - ox0);
  const int tid = threadIdx.x;
  if (tid < k) s_tab[tid] = bilinear_tap(tid, k);
  __syncthreads();
  const Taps ty = make_taps_tab(oy, k, s, pad, H, s_tab);
  const Taps tfirst = make_taps_tab(ox0, k, s, pad, W, s_tab);
  const Taps tlast = make_taps_tab(ox0 + npx - 1, k, s, pad, W, s_tab);
  const int cx0 = tfirst.i0;
  const int ncx = tlast.i0 + (tlast.n > 0 ? tlast.n : 1) - cx0;
  const int rowlen = ncx * C;
  const int tot = ty.n * rowlen;
  const float* src0 = z + (((long long)b * H + ty.i0) * W + cx0) * C;
  for (int e0 = tid; e0 < tot; e0 += 4 * LH_SEG) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int e = min(e0 + j * LH_SEG, tot - 1);
      const int ry = e / rowlen, i = e - ry * rowlen;
      v[j] = src0[(long long)ry * W * C + i];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (e0 + j * LH_SEG < tot) s_z[e0 + j * LH_SEG] = v[j];
  }
  __syncthreads();
  return Segment{b, oy, ox0, npx, cx0, ncx, ty};
}

// ---- one pixel, scalar form -----------------------------------------------------------------------------------------------
// CT > 0: the class count at compile time (everything unrolls, scores stay in registers); CT == 0: C at run time, every
// channel operation guarded by c < C. The tap loops are unrolled with guards either way: runtime bounds would index the
// tap arrays dynamically and put them in scratch memory (upscore.hip). The packed-f32 form of the same expression trees
// for an even compile-time C is upscore_softmax_argmax_fixed_kernel.

// e[c] = [ReLU](deconv(z)[c] + bias[c]) of the pixel with column taps tx; *pos (optional): bit c set where e[c] > 0.
// The sums start from +0. ZERO = false: the caller has cleared e[] itself. Where that happens changes no bit but the
// register allocation, by up to a wave of occupancy either way (VGPRs, clear here / at e[]'s declaration in the kernel):
// upscore_softmax_argmax_kernel<24> 70 / 58, label_loss_bwd_kernel<22, 22> 93 / 98 — so each kernel says which.
template <int CT, int CMAX, bool ZERO = true>
__device__ __forceinline__ void interp_scores(const float* s_z, const float* __restrict__ bias, const Taps& ty, const Taps& tx,
                                              int ncx, int cx0, int Crt, int relu, float (&e)[CMAX],
                                              unsigned long long* pos = nullptr)
{
  const int C = CT > 0 ? CT : Crt;
  if (ZERO) {
#pragma unroll
    for (int c = 0; c < CMAX; c++) e[c] = 0.f;
  }
#pragma unroll
  for (int jy = 0; jy < 4; jy++)
    if (jy < ty.n) {
#pragma unroll
      for (int jx = 0; jx < 4; jx++)
        if (jx < tx.n) {
          const float w = ty.w[jy] * tx.w[jx];
          const float* zc = s_z + (jy * ncx + (tx.i0 + jx - cx0)) * C;
#pragma unroll
          for (int c = 0; c < CMAX; c++)
            if (c < C) e[c] = e[c] + w * zc[c];
        }
    }
  unsigned long long mask = 0ull;
#pragma unroll
  for (int c = 0; c < CMAX; c++)
    if (c < C) {
      float v = e[c] + bias[c];
      if (relu) v = v > 0.f ? v : 0.f;
      if (v > 0.f) mask |= 1ull << c;
      e[c] = v;
    }
  if (pos) *pos = mask;
}

struct Softmax {
  float sum, dg, pg;   // the denominator; score[g] - max and prob[g] of class g (0 when g is no class)
  int best;            // first argmax of the probabilities
};

// softmax_high_dimension (network.py:474-488) + argmax_2d (:432-434): e[] enters as the scores, leaves as the probabilities
template <int CT, int CMAX>
__device__ __forceinline__ Softmax softmax_argmax(float (&e)[CMAX], int Crt, int g = -1)
{
  const int C = CT > 0 ? CT : Crt;
  Softmax P;
  float m = e[0];
#pragma unroll
  for (int c = 0; c < CMAX; c++)
    if (c < C) m = fmaxf(m, e[c]);
  float sum = 0.f;
  P.dg = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; c++)
    if (c < C) {
      const float d = e[c] - m;
      if (c == g) P.dg = d;
      e[c] = exp_softmax_f32(d);
      sum += e[c];
    }
  float bestp = div_rn(e[0], sum);
  P.best = 0;
  P.pg = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; c++)
    if (c < C) {
      const float p = div_rn(e[c], sum);
      e[c] = p;
      if (c == g) P.pg = p;
      if (p > bestp) { bestp = p; P.best = c; }
    }
  P.sum = sum;
  return P;
}

// ---- the tile, host side ------------------------------------------------------------------------------------------------
// Dynamic LDS: the staged cells [rows][ncx_max][C] from float 0, then (where the kernel parks a row of C floats per pixel)
// [LH_SEG][C] from float s_out_off. The caller has checked its arguments: 1 <= s <= k <= 4 s, C <= PCNN_MAX_CLASSES.
struct LabelHeadPlan {
  int nseg, s_out_off;
  long long blocks;
  size_t sh_in, sh_all;   // LDS bytes without / with the per-pixel rows
};

static inline LabelHeadPlan label_head_plan(int B, int H, int W, int C, int k, int s)
{
  LabelHeadPlan p;
  const int Wo = W * s, Ho = H * s;
  p.nseg = (Wo + LH_SEG - 1) / LH_SEG;
  p.blocks = (long long)B * Ho * p.nseg;
  const int rows = (k + s - 1) / s;                      // input rows per output row
  const int ncx_max = (LH_SEG - 1) / s + rows + 1;       // input columns per segment
  p.s_out_off = (rows * ncx_max * C + 3) / 4 * 4;
  p.sh_in = sizeof(float) * (size_t)p.s_out_off;
  p.sh_all = sizeof(float) * ((size_t)p.s_out_off + (size_t)LH_SEG * C);
  return p;
}

}  // namespace pcnn
