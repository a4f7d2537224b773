// pose3d.hip — the pose stage of the 3-D vertex route: Synthesizer::estimatePose3D (lib/synthesize/synthesize.cpp:1769-1966)
// as three launches per batch with nothing returning to the host in between. Arithmetic, orders and the deviations from the
// reference: include/posecnn_hip_pose3d.h; the numpy restatement is tests/pose3d_ref.py (bit for bit). The bodies of the
// prepare and ransac kernels, the fit and the box gate live in pose_device.h, shared with the colour route (pose2d.hip).
//
//   p3d_prepare_kernel   one workgroup of 1024 threads per frame; each of its 16 waves owns one contiguous run of the raster.
//                        Pass 1 counts the class pixels per wave (LDS integer atomics: a count has no order), one scan over
//                        (class, wave) turns the counts into the place where each wave's run of a class starts, pass 2 has
//                        no barrier: a wave scatters its run 64 pixels at a time, rank by ballot per class present, against
//                        its own running bases. Of a pixel's 12 C bytes of vertex_pred only the 12 of its class are read.
//   p3d_sample_kernel    one thread per (frame, hypothesis): at most max_attempts Philox blocks, each a 3-point Horn fit.
//   p3d_ransac_kernel    one workgroup of 8 waves per (frame, class): gathers its hypotheses in index order, then runs the
//                        whole preemptive loop with barriers only — a wave per hypothesis over the round's subset, integer
//                        butterfly for the count, an all-pairs rank in LDS for the halving, ballot prefix for the inlier
//                        ranks of the refit. At most floor(log2 hypotheses) + ref_it + 1 rounds, no spin-wait.
// Which side bounds them (reasoning, no counters collected): prepare reads the label map twice and 2 + 12 bytes per class
// pixel, but only 16 workgroups exist at batch 16 (one wave per SIMD-quarter of a CU): load latency, not bandwidth; sample is one divergent thread per hypothesis and
// bound by the ~2000 dependent f64 operations of a fit; ransac re-reads a class's 24-byte records from L2 once per
// (hypothesis, round) and spends ~25 f64 operations on each: f64 ALU bound.
#include "philox_device.h"
#include "pose_device.h"

namespace {

using namespace pcnn;
using namespace pcnn::pose;

// RESIDUAL of the header
__device__ __forceinline__ double residual(const double* P, const Rec& r)
{
  const double ox = (double)r.o[0], oy = (double)r.o[1], oz = (double)r.o[2];
  const double d0 = (double)r.e[0] - (((P[0] * ox + P[1] * oy) + P[2] * oz) + P[3]);
  const double d1 = (double)r.e[1] - (((P[4] * ox + P[5] * oy) + P[6] * oz) + P[7]);
  const double d2 = (double)r.e[2] - (((P[8] * ox + P[9] * oy) + P[10] * oz) + P[11]);
  return __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// the depth route's inlier test and refit for the shared loop (pose_device.h)
struct Route3D {
  double thr;
  __device__ void frame(int) {}
  __device__ bool inlier(const double* P, const Rec& r) const { return r.e[2] != 0.f && residual(P, r) < thr; }
  __device__ void refit(double* P, const float* __restrict__ rec, int n, int m, int cnt, int max_pixels, int lane) const
  {
    Sums s;
    sums_zero(s);
    visit_selected(*this, P, rec, n, m, cnt, max_pixels, lane, [&](const Rec& r) { sums_add(s, r); });
#pragma unroll
    for (int k = 0; k < 3; ++k) s.a[k] = wave_fold(s.a[k]), s.b[k] = wave_fold(s.b[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) s.ab[k] = wave_fold(s.ab[k]);
    fit_pose(s, cnt < max_pixels ? cnt : max_pixels, P);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void p3d_prepare_kernel(const int32_t* __restrict__ label,
                                                                   const uint16_t* __restrict__ depth,
                                                                   const float* __restrict__ vertex_pred,
                                                                   const float* __restrict__ extents,
                                                                   const float* __restrict__ intrinsics, float factor, int H,
                                                                   int W, int C, float* __restrict__ records,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ offsets)
{
  prepare_body<true>(label, depth, vertex_pred, extents, intrinsics, factor, H, W, C, records, counts, offsets);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAMPLE_THREADS) void p3d_sample_kernel(
    const float* __restrict__ records, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    const float* __restrict__ extents, const float* __restrict__ intrinsics, const unsigned long long* __restrict__ streams,
    unsigned long long k0, unsigned long long k1, int H, int W, int C, int Hyp, int max_attempts, int min_area, double thr,
    double min_dist, double* __restrict__ hyp_pose, int32_t* __restrict__ hyp_class, int32_t* __restrict__ hyp_attempt,
    int32_t* __restrict__ hyp_rec)
{
  __shared__ int s_live[PCNN_MAX_CLASSES], s_cnt[PCNN_MAX_CLASSES], s_off[PCNN_MAX_CLASSES];
  __shared__ int s_nlive;
  const int b = blockIdx.y, h = blockIdx.x * SAMPLE_THREADS + threadIdx.x, HW = H * W;
  if (threadIdx.x == 0) {
    int nl = 0;
    for (int c = 0; c < C; ++c) {
      const int n = clampi(counts[b * C + c], 0, HW);
      s_cnt[c] = n;
      s_off[c] = clampi(offsets[b * C + c], 0, HW - n);
      if (c >= 1 && n > min_area) s_live[nl++] = c;
    }
    s_nlive = nl;
  }
  __syncthreads();
  if (h >= Hyp) return;
  const int nlive = s_nlive;
  const unsigned long long stream = streams[b];
  const float* K = intrinsics + b * 4;
  const size_t slot = (size_t)b * Hyp + h;

  for (int att = 0; att < max_attempts && nlive > 0; ++att) {
    unsigned long long w[4];
    philox4x64((unsigned long long)att, stream, (unsigned long long)h, k0, k1, w);
    const int c = s_live[(int)(((w[0] >> 32) * (unsigned long long)nlive) >> 32)];
    const unsigned long long n = (unsigned long long)s_cnt[c];   // > min_area >= 0
    const float* base = records + ((size_t)b * HW + s_off[c]) * REC;
    int j[3];
    Rec r[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      j[i] = (int)(((w[1 + i] >> 32) * n) >> 32);   // < n
      r[i] = load_rec(base + (size_t)j[i] * REC);
      ok = ok && r[i].e[2] != 0.f && !(r[i].o[0] == 0.f && r[i].o[1] == 0.f && r[i].o[2] == 0.f);
#pragma unroll
      for (int k = 0; k < i; ++k) ok = ok && !(dist3(r[k].e, r[i].e) < min_dist) && !(dist3(r[k].o, r[i].o) < min_dist);
    }
    if (!ok) continue;
    Sums s;
    sums_zero(s);
#pragma unroll
    for (int i = 0; i < 3; ++i) sums_add(s, r[i]);
    double P[12];
    fit_pose(s, 3, P);
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && residual(P, r[i]) < thr;
    if (!ok) continue;
    if (!box_ok(P, extents + c * 3, K, H, W, min_area)) continue;
#pragma unroll
    for (int i = 0; i < 12; ++i) hyp_pose[slot * 12 + i] = P[i];
    hyp_class[slot] = c;
    hyp_attempt[slot] = att;
#pragma unroll
    for (int i = 0; i < 3; ++i) hyp_rec[slot * 3 + i] = j[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) hyp_pose[slot * 12 + i] = 0.0;
  hyp_class[slot] = 0;
  hyp_attempt[slot] = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i) hyp_rec[slot * 3 + i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// single != 0: one round (`first_round`) on caller-given hypotheses, per-slot outputs (wpose IS pose_out);
// single == 0: the whole loop, per-class outputs.
__global__ __launch_bounds__(RANSAC_THREADS) void p3d_ransac_kernel(
    const float* __restrict__ records, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    const double* hyp_pose, const int32_t* __restrict__ hyp_class, int HW, int C, int Hyp, int first_round,
    int single, int pixel_batch, int max_pixels, int ref_it, double thr, double* wpose,
    int32_t* __restrict__ class_out, int32_t* __restrict__ inl_out, double* __restrict__ poses64,
    float* __restrict__ poses32, int32_t* __restrict__ inliers, int32_t* __restrict__ ref_steps_out,
    int32_t* __restrict__ num_hyps)
{
  ransac_body(Route3D{thr}, records, counts, offsets, hyp_pose, hyp_class, HW, C, Hyp, first_round, single, pixel_batch, max_pixels,
              ref_it, wpose, class_out, inl_out, poses64, poses32, inliers, ref_steps_out, num_hyps);
}

// ---------------------------------------------------------------------------------------------------------------------
int check_sample_args(const char* who, int max_attempts, int min_area, float thr, float min_dist)
{
  PCNN_REQUIRE(max_attempts >= 1, PCNN_EINVAL, "%s: max_attempts must be at least 1 (got %d)", who, max_attempts);
  PCNN_REQUIRE(min_area >= 0, PCNN_EINVAL, "%s: min_area must not be negative (got %d)", who, min_area);
  PCNN_REQUIRE(finite(thr) && finite(min_dist), PCNN_EINVAL, "%s: inlier_threshold and min_dist must be finite", who);
  return PCNN_OK;
}

void launch_prepare(const int32_t* label, const uint16_t* depth, const float* vertex_pred, const float* extents,
                    const float* intrinsics, float factor_depth, int B, int H, int W, int C, float* records, int32_t* counts,
                    int32_t* offsets, hipStream_t stream)
{
  PCNN_LAUNCH(p3d_prepare_kernel, dim3(B), dim3(PREP_THREADS), 0, stream, label, depth, vertex_pred, extents, intrinsics,
              factor_depth, H, W, C, records, counts, offsets);
}

void launch_sample(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                   const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                   int Hyp, int max_attempts, int min_area, float thr, float min_dist, double* hyp_pose, int32_t* hyp_class,
                   int32_t* hyp_attempt, int32_t* hyp_rec, hipStream_t stream)
{
  PCNN_LAUNCH(p3d_sample_kernel, dim3((Hyp + SAMPLE_THREADS - 1) / SAMPLE_THREADS, B), dim3(SAMPLE_THREADS), 0, stream, records,
              counts, offsets, extents, intrinsics, reinterpret_cast<const unsigned long long*>(streams),
              (unsigned long long)seed0, (unsigned long long)seed1, H, W, C, Hyp, max_attempts, min_area, (double)thr,
              (double)min_dist, hyp_pose, hyp_class, hyp_attempt, hyp_rec);
}

}  // namespace

extern "C" int pcnn_pose3d_workspace_bytes(int B, int H, int W, int C, int hypotheses, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "pose3d_workspace_bytes: bytes is NULL");
  if (int st = check_shape("pose3d_workspace_bytes", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_workspace_bytes", hypotheses)) return st;
  *bytes = carve(B, H, W, C, hypotheses, 3).total;
  return PCNN_OK;
}

extern "C" int pcnn_pose3d_prepare_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred,
                                       const float* extents, const float* intrinsics, float factor_depth, int B, int H, int W,
                                       int C, float* records, int32_t* counts, int32_t* offsets, void* stream)
{
  if (int st = check_shape("pose3d_prepare", B, H, W, C)) return st;
  PCNN_REQUIRE(finite(factor_depth) && factor_depth != 0.f, PCNN_EINVAL, "pose3d_prepare: factor_depth must be finite and not 0");
  PCNN_REQUIRE(label && depth && vertex_pred && extents && intrinsics, PCNN_ENULL, "pose3d_prepare: an input is NULL");
  PCNN_REQUIRE(records && counts && offsets, PCNN_ENULL, "pose3d_prepare: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose3d_prepare: records must be 8-byte aligned");
  launch_prepare(label, depth, vertex_pred, extents, intrinsics, factor_depth, B, H, W, C, records, counts, offsets,
                 (hipStream_t)stream);
  return check_launch("pose3d_prepare_fwd");
}

extern "C" int pcnn_pose3d_sample_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                                      const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B,
                                      int H, int W, int C, int hypotheses, int max_attempts, int min_area,
                                      float inlier_threshold, float min_dist, double* hyp_pose, int32_t* hyp_class,
                                      int32_t* hyp_attempt, int32_t* hyp_rec, void* stream)
{
  if (int st = check_shape("pose3d_sample", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_sample", hypotheses)) return st;
  if (int st = check_sample_args("pose3d_sample", max_attempts, min_area, inlier_threshold, min_dist)) return st;
  PCNN_REQUIRE(records && counts && offsets && extents && intrinsics && streams, PCNN_ENULL, "pose3d_sample: an input is NULL");
  PCNN_REQUIRE(hyp_pose && hyp_class && hyp_attempt && hyp_rec, PCNN_ENULL, "pose3d_sample: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose3d_sample: records must be 8-byte aligned");
  launch_sample(records, counts, offsets, extents, intrinsics, streams, seed0, seed1, B, H, W, C, hypotheses, max_attempts,
                min_area, inlier_threshold, min_dist, hyp_pose, hyp_class, hyp_attempt, hyp_rec, (hipStream_t)stream);
  return check_launch("pose3d_sample_fwd");
}

extern "C" int pcnn_pose3d_round_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const double* hyp_pose,
                                     const int32_t* hyp_class, int B, int H, int W, int C, int hypotheses, int round,
                                     int pixel_batch, int max_pixels, float inlier_threshold, double* pose_out,
                                     int32_t* class_out, int32_t* inliers_out, void* stream)
{
  if (int st = check_shape("pose3d_round", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_round", hypotheses)) return st;
  if (int st = check_round_args("pose3d_round", round, pixel_batch, max_pixels, inlier_threshold)) return st;
  PCNN_REQUIRE(records && counts && offsets && hyp_pose && hyp_class, PCNN_ENULL, "pose3d_round: an input is NULL");
  PCNN_REQUIRE(pose_out && class_out && inliers_out, PCNN_ENULL, "pose3d_round: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose3d_round: records must be 8-byte aligned");
  PCNN_REQUIRE(pose_out != hyp_pose, PCNN_EINVAL, "pose3d_round: pose_out must not be hyp_pose");
  PCNN_LAUNCH(p3d_ransac_kernel, dim3(C, B), dim3(RANSAC_THREADS), 0, (hipStream_t)stream, records, counts, offsets, hyp_pose,
              hyp_class, H * W, C, hypotheses, round, 1, pixel_batch, max_pixels, 0, (double)inlier_threshold, pose_out,
              class_out, inliers_out, (double*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
              (int32_t*)nullptr);
  return check_launch("pose3d_round_fwd");
}

extern "C" int pcnn_pose3d_estimate_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred,
                                        const float* extents, const float* intrinsics, const uint64_t* streams,
                                        float factor_depth, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                                        int hypotheses, int pixel_batch, int max_pixels, int ref_it, int min_area,
                                        float inlier_threshold, float min_dist, int max_attempts, double* poses64,
                                        float* poses32, int32_t* inliers, int32_t* ref_steps, int32_t* num_hyps,
                                        void* workspace, size_t workspace_bytes, void* stream_)
{
  if (int st = check_shape("pose3d_estimate", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_estimate", hypotheses)) return st;
  if (int st = check_sample_args("pose3d_estimate", max_attempts, min_area, inlier_threshold, min_dist)) return st;
  PCNN_REQUIRE(ref_it >= 0 && ref_it <= (1 << 20), PCNN_EINVAL, "pose3d_estimate: ref_it must be in [0, 2^20] (got %d)", ref_it);
  if (int st = check_round_args("pose3d_estimate", 32 + ref_it, pixel_batch, max_pixels, inlier_threshold)) return st;
  PCNN_REQUIRE(finite(factor_depth) && factor_depth != 0.f, PCNN_EINVAL, "pose3d_estimate: factor_depth must be finite and not 0");
  PCNN_REQUIRE(label && depth && vertex_pred && extents && intrinsics && streams, PCNN_ENULL, "pose3d_estimate: an input is NULL");
  PCNN_REQUIRE(poses64 && poses32 && inliers && ref_steps && num_hyps, PCNN_ENULL, "pose3d_estimate: an output is NULL");
  const Carve cv = carve(B, H, W, C, hypotheses, 3);
  PCNN_REQUIRE_WORKSPACE("pose3d_estimate", workspace, workspace_bytes, cv.total);

  hipStream_t stream = (hipStream_t)stream_;
  char* ws = static_cast<char*>(workspace);
  float* records = reinterpret_cast<float*>(ws + cv.records);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + cv.counts);
  int32_t* offsets = reinterpret_cast<int32_t*>(ws + cv.offsets);
  double* hyp_pose = reinterpret_cast<double*>(ws + cv.hyp_pose);
  int32_t* hyp_class = reinterpret_cast<int32_t*>(ws + cv.hyp_class);
  int32_t* hyp_attempt = reinterpret_cast<int32_t*>(ws + cv.hyp_attempt);
  int32_t* hyp_rec = reinterpret_cast<int32_t*>(ws + cv.hyp_rec);
  double* wpose = reinterpret_cast<double*>(ws + cv.wpose);
  launch_prepare(label, depth, vertex_pred, extents, intrinsics, factor_depth, B, H, W, C, records, counts, offsets, stream);
  launch_sample(records, counts, offsets, extents, intrinsics, streams, seed0, seed1, B, H, W, C, hypotheses, max_attempts,
                min_area, inlier_threshold, min_dist, hyp_pose, hyp_class, hyp_attempt, hyp_rec, stream);
  PCNN_LAUNCH(p3d_ransac_kernel, dim3(C, B), dim3(RANSAC_THREADS), 0, stream, records, counts, offsets, hyp_pose, hyp_class,
              H * W, C, hypotheses, 1, 0, pixel_batch, max_pixels, ref_it, (double)inlier_threshold, wpose, (int32_t*)nullptr,
              (int32_t*)nullptr, poses64, poses32, inliers, ref_steps, num_hyps);
  return check_launch("pose3d_estimate_fwd");
}
