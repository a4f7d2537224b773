// label_loss.hip — the training twin of the label-head epilogue (upscore.hip): the same pass, ending in the hard-label
// cross-entropy loss instead of the probabilities, and its backward (include/posecnn_hip_loss.h).
//
// The reference's training graph (lib/networks/vgg16_convs.py:128-149, lib/fcn/train.py:41-44) upsamples 64 channels to
// full resolution, contracts them to C classes there, and walks ReLU -> log_softmax -> Hardlabel -> multiply -> two sums,
// forward and back, over [B,480,640,C] tensors. The 1x1 `score` conv and the fixed bilinear deconv commute, so here as in
// inference the contraction has happened at 1/8 resolution and one kernel per direction does the rest from z [B,H,W,C]:
//
//   pcnn_label_head_loss_fwd   label, optional per-pixel terms, loss = S / (count + 1e-10); no [B,Ho,Wo,C] tensor written
//   pcnn_label_head_loss_bwd   dscore [B,Ho,Wo,C] (the one such tensor of the pair) and dbias; dz is pcnn_deconv_bilinear_bwd
//
// Segment, per-pixel arithmetic and tile plan are the label head's own (label_head_device.h) — same bits for label and
// prob (the CPU checker builds the expected terms from the oracle's probabilities). Reductions: f64, fixed order, no
// atomics (see the header; reduce_device.h).
#include "../../include/posecnn_hip_loss.h"
#include "label_head_device.h"
#include "reduce_device.h"

namespace {

using namespace pcnn;

constexpr int LL_RUNS = 4;    // dbias: runs of LH_SEG / LL_RUNS consecutive pixels per workgroup
constexpr int LL_FIN = 256;   // threads of the forward's final kernel

// log of a softmax denominator, x in [1, 64]: a fixed sequence of IEEE f32 operations like exp_softmax_f32, restated by
// tests/label_loss_ref.py one numpy operation per line. x = 2^n t with t in [sqrt(1/2), sqrt(2)); log t = 2 atanh(q),
// q = (t - 1) / (t + 1), |q| <= 0.1716: the odd series through q^9 (the q^11 term is 2e-9 of the result); t - 1 is exact,
// n ln2_hi is exact (15 significant bits). Measured error: DESIGN.md.
__device__ __forceinline__ float log_sum_f32(float x)
{
  if (x != x) return x;
  const int bits = __float_as_int(x);
  int n = (bits >> 23) - 127;
  float t = __int_as_float((bits & 0x007fffff) | 0x3f800000);
  if (t > 1.41421354f) {
    t = t * 0.5f;
    n = n + 1;
  }
  const float f = t - 1.0f;
  const float q = div_rn(f, 2.0f + f);
  const float y = q * q;
  float p = 0.222222224f;
  p = p * y + 0.285714298f;
  p = p * y + 0.4f;
  p = p * y + 0.666666687f;
  p = p * y;
  const float l = (q + q) + q * p;
  const float nf = (float)n;
  return nf * 0.693145752f + (l + nf * 1.42860677e-06f);
}

__device__ __forceinline__ bool hot_class(int g, float pg, float threshold)
{
  // hard_label_op_gpu.cu.cc:17-29; g < 0 here also stands for a label outside [0, C), ignored as in up_hard_label_rows
  return g >= 0 && (g > 0 || pg < threshold);
}

template <int CT, int CMAX>
__global__ __launch_bounds__(LH_SEG) void label_loss_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ bias, const int* __restrict__ gt, int* __restrict__ label,
    float* __restrict__ terms, double* __restrict__ part_s, long long* __restrict__ part_n, int H, int W, int Crt, int k,
    int s, int relu, int nseg, float threshold)
{
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_tab[64];
  __shared__ double s_sum[LH_SEG];
  __shared__ int s_cnt[LH_SEG];
  const int C = CT > 0 ? CT : Crt;
  const int tid = threadIdx.x;
  const Segment S = load_segment(z, smem, s_tab, H, W, C, k, s, nseg);
  float term = 0.f;
  int hot = 0;
  if (tid < S.npx) {
    const int Wo = W * s;
    const long long pix = ((long long)S.b * H * s + S.oy) * Wo + S.ox0 + tid;
    int g = gt[pix];
    if (g < 0 || g >= C) g = -1;
    const Taps tx = make_taps_tab(S.ox0 + tid, k, s, (k - s) / 2, W, s_tab);
    float e[CMAX];
    interp_scores<CT, CMAX>(smem, bias, S.ty, tx, S.ncx, S.cx0, C, relu, e);
    const Softmax P = softmax_argmax<CT, CMAX>(e, C, g);
    label[pix] = P.best;
    if (hot_class(g, P.pg, threshold)) {
      hot = 1;
      term = log_sum_f32(P.sum) - P.dg;
    }
    if (terms) terms[pix] = term;
  }
  s_sum[tid] = (double)term;
  s_cnt[tid] = hot;
  block_tree_sum<LH_SEG>(s_sum, s_cnt, tid);
  if (tid == 0) {
    part_s[blockIdx.x] = s_sum[0];
    part_n[blockIdx.x] = (long long)s_cnt[0];
  }
}

__global__ __launch_bounds__(LL_FIN) void label_loss_fwd_final_kernel(const double* __restrict__ part_s,
                                                                      const long long* __restrict__ part_n, int nblk,
                                                                      float* __restrict__ loss, double* __restrict__ sums)
{
  __shared__ double s_sum[LL_FIN];
  __shared__ long long s_cnt[LL_FIN];
  const int t = threadIdx.x;
  double a = 0.0;
  long long n = 0;
  for (int i = t; i < nblk; i += LL_FIN) {
    a = a + part_s[i];
    n = n + part_n[i];
  }
  s_sum[t] = a;
  s_cnt[t] = n;
  block_tree_sum<LL_FIN>(s_sum, s_cnt, t);
  if (t == 0) {
    sums[0] = s_sum[0];
    sums[1] = (double)s_cnt[0];
    loss[0] = (float)(s_sum[0] / ((double)s_cnt[0] + 1e-10));   // train.py:41-44
  }
}

template <int CT, int CMAX>
__global__ __launch_bounds__(LH_SEG) void label_loss_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ bias, const int* __restrict__ gt,
    const double* __restrict__ sums, const float* __restrict__ upstream, float* __restrict__ dscore,
    double* __restrict__ part_b, int H, int W, int Crt, int k, int s, int relu, int nseg, int s_out_off, float threshold)
{
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_tab[64];
  __shared__ double s_run[LL_RUNS * PCNN_MAX_CLASSES];
  const int C = CT > 0 ? CT : Crt;
  const int tid = threadIdx.x;
  const Segment S = load_segment(z, smem, s_tab, H, W, C, k, s, nseg);
  float* s_out = smem + s_out_off;   // [LH_SEG][C]
  const int Wo = W * s;
  const long long pix0 = ((long long)S.b * H * s + S.oy) * Wo + S.ox0;
  if (tid < S.npx) {
    const float coef = div_rn(upstream ? upstream[0] : 1.0f, (float)sums[1] + 1e-10f);
    int g = gt[pix0 + tid];
    if (g < 0 || g >= C) g = -1;
    const Taps tx = make_taps_tab(S.ox0 + tid, k, s, (k - s) / 2, W, s_tab);
    float e[CMAX];
    unsigned long long pos;   // bit c: score[c] > 0
    interp_scores<CT, CMAX>(smem, bias, S.ty, tx, S.ncx, S.cx0, C, relu, e, &pos);
    const Softmax P = softmax_argmax<CT, CMAX>(e, C, g);
    const bool hot = hot_class(g, P.pg, threshold);
#pragma unroll
    for (int c = 0; c < CMAX; c++)
      if (c < C) {
        float d = coef * (e[c] - (c == g ? 1.0f : 0.0f));
        if (!hot || (relu && !((pos >> c) & 1ull))) d = 0.f;   // the ReLU's gradient at score == 0 is zero
        s_out[tid * C + c] = d;
      }
  }
  __syncthreads();
  {
    // the segment's npx * C floats are one contiguous run of dscore; the deconv gradient reads them next: ordinary stores
    float* o = dscore + pix0 * C;
    const int nfl = S.npx * C;
    if ((nfl & 3) == 0 && (s_out_off & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
      for (int i = tid * 4; i < nfl; i += LH_SEG * 4) *reinterpret_cast<v4f*>(o + i) = *reinterpret_cast<const v4f*>(s_out + i);
    } else {
      for (int i = tid; i < nfl; i += LH_SEG) o[i] = s_out[i];
    }
  }
  // dbias partials: LL_RUNS runs of consecutive pixels per class, ascending inside a run, then the runs ascending
  constexpr int RUN = LH_SEG / LL_RUNS;
  for (int idx = tid; idx < C * LL_RUNS; idx += LH_SEG) {
    const int c = idx % C, q = idx / C;
    const int p1 = min((q + 1) * RUN, S.npx);
    double a = 0.0;
    for (int p = q * RUN; p < p1; p++) a = a + (double)s_out[p * C + c];
    s_run[q * PCNN_MAX_CLASSES + c] = a;
  }
  __syncthreads();
  if (tid < C) {
    double a = s_run[tid];
#pragma unroll
    for (int q = 1; q < LL_RUNS; q++) a = a + s_run[q * PCNN_MAX_CLASSES + tid];
    part_b[(size_t)tid * gridDim.x + blockIdx.x] = a;
  }
}

// the label head's tile (the forward stages the cells only: sh_in; the backward parks dscore rows as well: sh_all)
struct Plan : LabelHeadPlan {
  size_t ws_bytes;
};

int make_plan(const char* who, int B, int H, int W, int C, int k, int s, Plan* p)
{
  PCNN_REQUIRE(B >= 1 && H >= 1 && W >= 1, PCNN_EINVAL, "%s: bad shape: batch %d, height %d, width %d", who, B, H, W);
  PCNN_REQUIRE(C >= 2 && C <= PCNN_MAX_CLASSES, PCNN_EINVAL, "%s: num_classes must be in [2, %d] (got %d)", who,
               PCNN_MAX_CLASSES, C);
  PCNN_REQUIRE(s >= 1 && k >= s && (k - s) % 2 == 0 && k <= 4 * s && k <= 64, PCNN_EINVAL,
               "%s: need stride >= 1, stride <= kernel <= min(4*stride, 64) and (kernel - stride) even (got kernel=%d stride=%d)",
               who, k, s);
  PCNN_REQUIRE((long long)B * H * s * W * s < (1ll << 31), PCNN_EINVAL, "%s: batch*height*width*stride^2 must be < 2^31", who);
  static_cast<LabelHeadPlan&>(*p) = label_head_plan(B, H, W, C, k, s);
  // + 4096: the static arrays of the two kernels (tap table, reduction leaves, dbias runs) share the 160 KB
  PCNN_REQUIRE(p->sh_all + 4096 <= 160 * 1024, PCNN_EINVAL, "%s: tile does not fit LDS (kernel=%d stride=%d num_classes=%d)", who, k, s, C);
  p->ws_bytes = sizeof(double) * (size_t)p->blocks * (size_t)C;   // fwd: 2 x blocks words; bwd: C x blocks (C >= 2)
  return PCNN_OK;
}

}  // namespace

extern "C" int pcnn_label_head_loss_workspace_bytes(int B, int H, int W, int C, int k, int s, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "label_head_loss_workspace_bytes: NULL bytes");
  Plan p;
  int st = make_plan("label_head_loss_workspace_bytes", B, H, W, C, k, s, &p);
  if (st != PCNN_OK) return st;
  *bytes = p.ws_bytes;
  return PCNN_OK;
}

extern "C" int pcnn_label_head_loss_fwd(const float* z, const float* bias, const int32_t* gt, int B, int H, int W, int C,
                                        int k, int s, int relu, float threshold, float* loss, double* sums, int32_t* label,
                                        float* terms, void* workspace, size_t workspace_bytes, void* stream_)
{
  const char* who = "label_head_loss_fwd";
  Plan p;
  int st = make_plan(who, B, H, W, C, k, s, &p);
  if (st != PCNN_OK) return st;
  // attribute check of the Hardlabel op, hard_label_op.cc:150-155
  PCNN_REQUIRE(threshold > 0, PCNN_EINVAL, "%s: Need threshold > 0, got %g", who, (double)threshold);
  PCNN_REQUIRE(z, PCNN_ENULL, "%s: NULL z", who);
  PCNN_REQUIRE(bias, PCNN_ENULL, "%s: NULL bias", who);
  PCNN_REQUIRE(gt, PCNN_ENULL, "%s: NULL gt_label", who);
  PCNN_REQUIRE(loss, PCNN_ENULL, "%s: NULL loss", who);
  PCNN_REQUIRE(sums, PCNN_ENULL, "%s: NULL sums", who);
  PCNN_REQUIRE(label, PCNN_ENULL, "%s: NULL label", who);
  PCNN_REQUIRE(aligned16(sums), PCNN_EINVAL, "%s: sums must be 16-byte aligned", who);
  PCNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, p.ws_bytes);
  hipStream_t stream = (hipStream_t)stream_;
  double* part_s = (double*)workspace;
  long long* part_n = (long long*)workspace + p.blocks;
#define LL_FWD(CT, CMAX)                                                                                              \
  PCNN_LAUNCH((label_loss_fwd_kernel<CT, CMAX>), dim3((unsigned)p.blocks), dim3(LH_SEG), p.sh_in, stream, z, bias, gt, label, \
              terms, part_s, part_n, H, W, C, k, s, relu, p.nseg, threshold)
  if (C == 22) LL_FWD(22, 22);
  else if (C == 16) LL_FWD(16, 16);
  else if (C == 14) LL_FWD(14, 14);
  else if (C <= 24) LL_FWD(0, 24);
  else LL_FWD(0, 64);
#undef LL_FWD
  PCNN_LAUNCH(label_loss_fwd_final_kernel, dim3(1), dim3(LL_FIN), 0, stream, part_s, part_n, (int)p.blocks, loss, sums);
  return check_launch(who);
}

extern "C" int pcnn_label_head_loss_bwd(const float* z, const float* bias, const int32_t* gt, const double* sums,
                                        const float* upstream, int B, int H, int W, int C, int k, int s, int relu,
                                        float threshold, float* dscore, float* dbias, void* workspace,
                                        size_t workspace_bytes, void* stream_)
{
  const char* who = "label_head_loss_bwd";
  Plan p;
  int st = make_plan(who, B, H, W, C, k, s, &p);
  if (st != PCNN_OK) return st;
  PCNN_REQUIRE(threshold > 0, PCNN_EINVAL, "%s: Need threshold > 0, got %g", who, (double)threshold);
  PCNN_REQUIRE(z, PCNN_ENULL, "%s: NULL z", who);
  PCNN_REQUIRE(bias, PCNN_ENULL, "%s: NULL bias", who);
  PCNN_REQUIRE(gt, PCNN_ENULL, "%s: NULL gt_label", who);
  PCNN_REQUIRE(sums, PCNN_ENULL, "%s: NULL sums", who);
  PCNN_REQUIRE(dscore, PCNN_ENULL, "%s: NULL dscore", who);
  PCNN_REQUIRE(dbias, PCNN_ENULL, "%s: NULL dbias", who);
  PCNN_REQUIRE(aligned16(sums), PCNN_EINVAL, "%s: sums must be 16-byte aligned", who);
  PCNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, p.ws_bytes);
  hipStream_t stream = (hipStream_t)stream_;
  double* part_b = (double*)workspace;
#define LL_BWD(CT, CMAX)                                                                                              \
  PCNN_LAUNCH((label_loss_bwd_kernel<CT, CMAX>), dim3((unsigned)p.blocks), dim3(LH_SEG), p.sh_all, stream, z, bias, gt, sums, \
              upstream, dscore, part_b, H, W, C, k, s, relu, p.nseg, p.s_out_off, threshold)
  if (C == 22) LL_BWD(22, 22);
  else if (C == 16) LL_BWD(16, 16);
  else if (C == 14) LL_BWD(14, 14);
  else if (C <= 24) LL_BWD(0, 24);
  else LL_BWD(0, 64);
#undef LL_BWD
  PCNN_LAUNCH(channel_partials_final_kernel<CPF_THREADS>, dim3((unsigned)C), dim3(CPF_THREADS), 0, stream, part_b, (int)p.blocks, dbias);
  return check_launch(who);
}
