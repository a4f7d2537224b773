// pose_polish.hip — the last step of both pose routes of the 3-D vertex route: refineWithOpt (lib/synthesize/synthesize.cpp
// :1510-1567) as one launch per batch. Arithmetic, orders, the optimiser's rules and the deviation from the reference:
// include/posecnn_hip/pose_polish.h; the numpy restatement is tests/pose_polish_ref.py (bit for bit).
//
//   pose_polish_kernel   one wave per (frame, class), no barrier. Two sweeps over the class's records build the list (count,
//                        then compaction by ballot rank with the thinning of pose_device.h) into LDS — 24 KB at
//                        PCNN_POSE_POLISH_LDS_RECORDS — or, for a larger max_pixels, into the workspace. An evaluation is
//                        the retraction (every lane, same bits), ceil(L / 64) records per lane and one xor butterfly.
//                        The simplex (7 x 6 f64) and its values live in LDS because lo / hi / nh index them dynamically (a
//                        private array would go to scratch): every lane writes the same bits to the same address and
//                        reads them back in its own program order.
// The simplex rules are a second copy of the ~60 lines icp.hip's icp_polish_kernel states for N = 7: that one is
// workgroup-wide with thread 0 writing between barriers, this one is wave-wide and barrier-free, and its bits are pinned by
// its own tests — one copy per execution shape.
// Which side bounds it (reasoning, no counters collected): at 100 evaluations and L = 1000 a lane walks 100 x 16 records of
// ~40 dependent f64 operations each plus ~150 uniform ones per evaluation; with one wave per (frame, class) a CU holds at
// most a few waves: f64 latency, not throughput or memory.
#include "pose_device.h"

#include "../../include/posecnn_hip/pose_polish.h"
#include "../../include/posecnn_hip_pose2d.h"

namespace {

using namespace pcnn;
using namespace pcnn::pose;

constexpr int NM_N = 6;
constexpr int LDS_RECORDS = PCNN_POSE_POLISH_LDS_RECORDS;

// RESIDUAL of posecnn_hip_pose3d.h (pose3d.hip holds the route's own copy in its unnamed namespace)
__device__ __forceinline__ double polish_residual(const double* P, const Rec& r)
{
  const double ox = (double)r.o[0], oy = (double)r.o[1], oz = (double)r.o[2];
  const double d0 = (double)r.e[0] - (((P[0] * ox + P[1] * oy) + P[2] * oz) + P[3]);
  const double d1 = (double)r.e[1] - (((P[4] * ox + P[5] * oy) + P[6] * oz) + P[7]);
  const double d2 = (double)r.e[2] - (((P[8] * ox + P[9] * oy) + P[10] * oz) + P[11]);
  return __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// REPROJ of posecnn_hip_pose2d.h: the distance; `front` = q.z > 0
__device__ __forceinline__ double polish_reproj(const double* P, const Rec& r, const double* K, bool& front)
{
  const double ox = (double)r.o[0], oy = (double)r.o[1], oz = (double)r.o[2];
  const double qx = ((P[0] * ox + P[1] * oy) + P[2] * oz) + P[3];
  const double qy = ((P[4] * ox + P[5] * oy) + P[6] * oz) + P[7];
  const double qz = ((P[8] * ox + P[9] * oy) + P[10] * oz) + P[11];
  front = qz > 0.0;
  const double du = (K[0] * qx / qz + K[2]) - (double)r.e[0];
  const double dv = (K[1] * qy / qz + K[3]) - (double)r.e[1];
  return __builtin_sqrt(du * du + dv * dv);
}

// the route's distance and inlier test: ROUTE 0 depth, 1 colour (K = fx, fy, px, py widened)
template <int ROUTE>
struct PolishRoute {
  double thr;
  double K[4];
  __device__ double distance(const double* P, const Rec& r, bool& valid) const
  {
    if (ROUTE == 0) {
      valid = true;
      return polish_residual(P, r);
    }
    return polish_reproj(P, r, K, valid);
  }
  __device__ bool inlier(const double* P, const Rec& r) const
  {
    bool valid;
    const double d = distance(P, r, valid);
    return (ROUTE == 0 ? r.e[2] != 0.f : valid) && d < thr;
  }
};

// P(x) of the header: the colour route's retraction applied to P0
__device__ __forceinline__ void pose_of(const double* P0, const double* x, double* P)
{
  const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
  const double nrm = __builtin_sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double w = 1.0 / nrm, xq = hx / nrm, yq = hy / nrm, zq = hz / nrm;
  const double xx = xq * xq, yy = yq * yq, zz = zq * zq, xy = xq * yq, xz = xq * zq, yz = yq * zq, wx = w * xq, wy = w * yq,
               wz = w * zq;
  const double Q[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                          {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                          {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) P[4 * i + j] = (Q[i][0] * P0[j] + Q[i][1] * P0[4 + j]) + Q[i][2] * P0[8 + j];
    P[4 * i + 3] = P0[4 * i + 3] + x[3 + i];
  }
}

// E(x) of the header over the compacted list (LDS or workspace); every lane returns the same bits
template <int ROUTE>
__device__ __forceinline__ double energy_of(const PolishRoute<ROUTE>& route, const double* P0, const double* x, const float* list,
                                            int L, int lane)
{
  double P[12];
  pose_of(P0, x, P);
  double acc = 0.0;
  bool bad = false;
  for (int j = lane; j < L; j += PCNN_WAVE) {
    bool valid;
    const double d = route.distance(P, load_rec(list + (size_t)j * REC), valid);
    bad = bad || !valid;
    acc = acc + d;
  }
  const double e = wave_fold(acc) / (double)L;
  return (__ballot(bad) != 0ull || !(e - e == 0.0)) ? __builtin_inf() : e;
}

struct Simplex {
  double v[NM_N + 1][NM_N], f[NM_N + 1], c[NM_N], xr[NM_N], xe[NM_N];
};

// IN_LDS: the list fits the LDS buffer (max_pixels <= LDS_RECORDS); otherwise `ws_list` holds `cap` records per (frame, class)
template <int ROUTE, bool IN_LDS>
__global__ __launch_bounds__(PCNN_WAVE) void pose_polish_kernel(
    const float* __restrict__ records, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    const float* __restrict__ intrinsics, const double* poses_in, const int32_t* __restrict__ gate, int HW, int C, int max_pixels,
    int min_pixels, int evaluations, double thr, double* poses64, float* __restrict__ poses32, double* __restrict__ energy,
    int32_t* __restrict__ evals_out, int32_t* __restrict__ listed, float* __restrict__ ws_list, long long cap)
{
  __shared__ float s_list[IN_LDS ? LDS_RECORDS * REC : REC];
  __shared__ Simplex s;
  const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const size_t cls = (size_t)b * C + c;
  double P0[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P0[k] = poses_in[cls * 12 + k];

  PolishRoute<ROUTE> route;
  route.thr = thr;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    route.K[k] = 0.0;
    if (ROUTE != 0) route.K[k] = (double)intrinsics[b * 4 + k];
  }

  // the list: count, then compact (uniform over the wave)
  int L = 0;
  float* list = IN_LDS ? s_list : ws_list + (size_t)cls * (size_t)cap * REC;
  if (c >= 1 && evaluations >= NM_N + 1 && gate[cls] > min_pixels) {
    const int n = clampi(counts[cls], 0, HW);
    const float* rec = records + ((size_t)b * HW + clampi(offsets[cls], 0, HW - n)) * REC;
    int cnt = 0;
    for (int k = lane; k < n; k += PCNN_WAVE) cnt += route.inlier(P0, load_rec(rec + (size_t)k * REC)) ? 1 : 0;
    cnt = wave_sum(cnt);
    L = cnt < max_pixels ? cnt : max_pixels;
    visit_listed(route, P0, rec, n, cnt, max_pixels, lane, [&](int j, const Rec& r) {   // j < L <= LDS_RECORDS or cap
      float* dst = list + (size_t)j * REC;
      *reinterpret_cast<float2*>(dst) = make_float2(r.e[0], r.e[1]);
      *reinterpret_cast<float2*>(dst + 2) = make_float2(r.e[2], r.o[0]);
      *reinterpret_cast<float2*>(dst + 4) = make_float2(r.o[1], r.o[2]);
    });
  }
  if (L == 0) {
    if (lane < 12) {
      const double v = poses_in[cls * 12 + lane];
      poses64[cls * 12 + lane] = v;
      poses32[cls * 12 + lane] = (float)v;
    }
    if (lane < 2) energy[cls * 2 + lane] = 0.0;
    if (lane == 0) evals_out[cls] = 0, listed[cls] = 0;
    return;
  }
  // the list is written by other lanes of this wave: through LDS, or through global memory
  if (IN_LDS) __threadfence_block(); else __threadfence();

  const double range[NM_N] = {PCNN_POSE_POLISH_BOX_ROT, PCNN_POSE_POLISH_BOX_ROT, PCNN_POSE_POLISH_BOX_ROT,
                              PCNN_POSE_POLISH_BOX_XY,  PCNN_POSE_POLISH_BOX_XY,  PCNN_POSE_POLISH_BOX_Z};
#define NM_EVAL(X) energy_of(route, P0, (X), list, L, lane)
  int evals = 0;
  for (int k = 0; k <= NM_N; ++k) {
    for (int i = 0; i < NM_N; ++i) s.v[k][i] = 0.0;
    if (k > 0) s.v[k][k - 1] = 0.0 + (range[k - 1] - (-range[k - 1])) * 0.25;
    s.f[k] = NM_EVAL(s.v[k]);
    evals++;
  }
  const double f_start = s.f[0];
  while (evals < evaluations) {
    int lo = 0, hi = 0, nh = -1;
    for (int k = 1; k <= NM_N; ++k) {
      if (s.f[k] < s.f[lo]) lo = k;
      if (s.f[k] >= s.f[hi]) hi = k;
    }
    for (int k = 0; k <= NM_N; ++k)
      if (k != hi && (nh < 0 || s.f[k] >= s.f[nh])) nh = k;
    const double flo = s.f[lo], fhi = s.f[hi], fnh = s.f[nh];
    for (int i = 0; i < NM_N; ++i) {
      double sacc = 0.0;
      for (int k = 0; k <= NM_N; ++k)
        if (k != hi) sacc = sacc + s.v[k][i];
      s.c[i] = sacc / (double)NM_N;
    }
#define NM_POINT(DST, COEF)                                    \
    for (int i = 0; i < NM_N; ++i) {                           \
      double v_ = s.c[i] + (COEF) * (s.c[i] - s.v[hi][i]);     \
      if (v_ < -range[i]) v_ = -range[i];                      \
      if (v_ > range[i]) v_ = range[i];                        \
      (DST)[i] = v_;                                           \
    }
#define NM_TAKE(SRC, FV)                                       \
    do {                                                       \
      for (int i = 0; i < NM_N; ++i) s.v[hi][i] = (SRC)[i];    \
      s.f[hi] = (FV);                                          \
    } while (0)
    NM_POINT(s.xr, 1.0);
    const double fr = NM_EVAL(s.xr);
    evals++;
    if (fr < flo) {
      if (evals < evaluations) {
        NM_POINT(s.xe, 2.0);
        const double fe = NM_EVAL(s.xe);
        evals++;
        if (fe < fr) NM_TAKE(s.xe, fe); else NM_TAKE(s.xr, fr);
      } else {
        NM_TAKE(s.xr, fr);
      }
    } else if (fr < fnh) {
      NM_TAKE(s.xr, fr);
    } else {
      if (evals >= evaluations) {
        if (fr < fhi) NM_TAKE(s.xr, fr);
        break;
      }
      const double coef = fr < fhi ? 0.5 : -0.5;
      NM_POINT(s.xe, coef);
      const double fc = NM_EVAL(s.xe);
      evals++;
      const double fref = fr < fhi ? fr : fhi;
      if (fc < fref) {
        NM_TAKE(s.xe, fc);
      } else {
        for (int k = 0; k <= NM_N && evals < evaluations; ++k) {
          if (k == lo) continue;
          for (int i = 0; i < NM_N; ++i) s.v[k][i] = s.v[lo][i] + 0.5 * (s.v[k][i] - s.v[lo][i]);
          s.f[k] = NM_EVAL(s.v[k]);
          evals++;
        }
      }
    }
  }
#undef NM_EVAL
#undef NM_POINT
#undef NM_TAKE
  int lo = 0;
  for (int k = 1; k <= NM_N; ++k)
    if (s.f[k] < s.f[lo]) lo = k;
  double P[12];
  pose_of(P0, s.v[lo], P);
  const double f_end = s.f[lo];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) poses64[cls * 12 + k] = P[k], poses32[cls * 12 + k] = (float)P[k];
    energy[cls * 2] = f_start;
    energy[cls * 2 + 1] = f_end;
    evals_out[cls] = evals;
    listed[cls] = L;
  }
}

size_t list_cap(int max_pixels) { return (size_t)(max_pixels < (1 << 24) ? max_pixels : (1 << 24)); }   // L <= n <= H W <= 2^24

size_t polish_ws_bytes(int B, int C, int max_pixels)
{
  if (max_pixels <= LDS_RECORDS) return 16;
  return align_up((size_t)B * C * list_cap(max_pixels) * REC * sizeof(float), 16);
}

int check_polish_args(const char* who, int max_pixels, int min_pixels, int evaluations, float thr)
{
  PCNN_REQUIRE(evaluations == 0 || (evaluations >= NM_N + 1 && evaluations <= PCNN_POSE_POLISH_MAX_EVALUATIONS), PCNN_EINVAL,
               "%s: evaluations must be 0 or in [%d, %d] — the initial simplex alone takes %d (got %d)", who, NM_N + 1,
               PCNN_POSE_POLISH_MAX_EVALUATIONS, NM_N + 1, evaluations);
  PCNN_REQUIRE(max_pixels >= 1, PCNN_EINVAL, "%s: max_pixels must be at least 1 (got %d)", who, max_pixels);
  PCNN_REQUIRE(min_pixels >= 0, PCNN_EINVAL, "%s: min_pixels must not be negative (got %d)", who, min_pixels);
  PCNN_REQUIRE(finite(thr), PCNN_EINVAL, "%s: inlier_threshold must be finite", who);
  return PCNN_OK;
}

// arguments checked by the caller
void launch_polish(int route, const float* records, const int32_t* counts, const int32_t* offsets, const float* intrinsics,
                   const double* poses_in, const int32_t* gate, int B, int H, int W, int C, int max_pixels, int min_pixels,
                   int evaluations, float thr, double* poses64, float* poses32, double* energy, int32_t* evals, int32_t* listed,
                   void* workspace, hipStream_t stream)
{
  const bool in_lds = max_pixels <= LDS_RECORDS;
  float* ws_list = static_cast<float*>(workspace);
  const long long cap = (long long)list_cap(max_pixels);
#define POLISH_LAUNCH(R, LDS)                                                                                                  \
  PCNN_LAUNCH((pose_polish_kernel<R, LDS>), dim3(C, B), dim3(PCNN_WAVE), 0, stream, records, counts, offsets, intrinsics,        \
              poses_in, gate, H * W, C, max_pixels, min_pixels, evaluations, (double)thr, poses64, poses32, energy, evals, listed, \
              ws_list, cap)
  if (route == 0) {
    if (in_lds) POLISH_LAUNCH(0, true); else POLISH_LAUNCH(0, false);
  } else {
    if (in_lds) POLISH_LAUNCH(1, true); else POLISH_LAUNCH(1, false);
  }
#undef POLISH_LAUNCH
}

}  // namespace

extern "C" int pcnn_pose_polish_workspace_bytes(int B, int C, int max_pixels, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "pose_polish_workspace_bytes: bytes is NULL");
  if (int st = check_shape("pose_polish_workspace_bytes", B, 1, 1, C)) return st;
  PCNN_REQUIRE(max_pixels >= 1, PCNN_EINVAL, "pose_polish_workspace_bytes: max_pixels must be at least 1 (got %d)", max_pixels);
  *bytes = polish_ws_bytes(B, C, max_pixels);
  return PCNN_OK;
}

extern "C" int pcnn_pose_polish_fwd(int route, const float* records, const int32_t* counts, const int32_t* offsets,
                                    const float* intrinsics, const double* poses_in, const int32_t* gate, int B, int H, int W,
                                    int C, int max_pixels, int min_pixels, int evaluations, float inlier_threshold,
                                    double* poses64, float* poses32, double* energy, int32_t* evals, int32_t* listed,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
  PCNN_REQUIRE(route == 0 || route == 1, PCNN_EINVAL, "pose_polish: route must be 0 (depth) or 1 (colour) (got %d)", route);
  if (int st = check_shape("pose_polish", B, H, W, C)) return st;
  if (int st = check_polish_args("pose_polish", max_pixels, min_pixels, evaluations, inlier_threshold)) return st;
  PCNN_REQUIRE(records && counts && offsets && poses_in && gate && (route == 0 || intrinsics), PCNN_ENULL,
               "pose_polish: an input is NULL");
  PCNN_REQUIRE(poses64 && poses32 && energy && evals && listed, PCNN_ENULL, "pose_polish: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose_polish: records must be 8-byte aligned");
  PCNN_REQUIRE_WORKSPACE("pose_polish", workspace, workspace_bytes, polish_ws_bytes(B, C, max_pixels));
  launch_polish(route, records, counts, offsets, intrinsics, poses_in, gate, B, H, W, C, max_pixels, min_pixels, evaluations,
                inlier_threshold, poses64, poses32, energy, evals, listed, workspace, (hipStream_t)stream);
  return check_launch("pose_polish_fwd");
}

extern "C" int pcnn_pose3d_estimate_polished_workspace_bytes(int B, int H, int W, int C, int hypotheses, int max_pixels,
                                                             size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "pose3d_estimate_polished_workspace_bytes: bytes is NULL");
  if (int st = check_shape("pose3d_estimate_polished_workspace_bytes", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_estimate_polished_workspace_bytes", hypotheses)) return st;
  PCNN_REQUIRE(max_pixels >= 1, PCNN_EINVAL, "pose3d_estimate_polished_workspace_bytes: max_pixels must be at least 1 (got %d)",
               max_pixels);
  *bytes = carve(B, H, W, C, hypotheses, 3).total + polish_ws_bytes(B, C, max_pixels);
  return PCNN_OK;
}

extern "C" int pcnn_pose2d_estimate_polished_workspace_bytes(int B, int H, int W, int C, int hypotheses, int max_pixels,
                                                             size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "pose2d_estimate_polished_workspace_bytes: bytes is NULL");
  if (int st = check_shape("pose2d_estimate_polished_workspace_bytes", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_estimate_polished_workspace_bytes", hypotheses)) return st;
  PCNN_REQUIRE(max_pixels >= 1, PCNN_EINVAL, "pose2d_estimate_polished_workspace_bytes: max_pixels must be at least 1 (got %d)",
               max_pixels);
  *bytes = carve(B, H, W, C, hypotheses, 4).total + polish_ws_bytes(B, C, max_pixels);
  return PCNN_OK;
}

// The drivers: the existing estimate entry on the front of the workspace (its own checks and three launches), then the
// polish in place on its poses, on the records it left at the workspace's carve — the same stream, nothing in between.
extern "C" int pcnn_pose3d_estimate_polished_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred,
                                                 const float* extents, const float* intrinsics, const uint64_t* streams,
                                                 float factor_depth, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                                                 int hypotheses, int pixel_batch, int max_pixels, int ref_it, int min_area,
                                                 float inlier_threshold, float min_dist, int max_attempts, int min_pixels,
                                                 int evaluations, double* poses64, float* poses32, int32_t* inliers,
                                                 int32_t* ref_steps, int32_t* num_hyps, double* energy, int32_t* evals,
                                                 int32_t* listed, void* workspace, size_t workspace_bytes, void* stream)
{
  if (int st = check_shape("pose3d_estimate_polished", B, H, W, C)) return st;
  if (int st = check_hyp("pose3d_estimate_polished", hypotheses)) return st;
  if (int st = check_polish_args("pose3d_estimate_polished", max_pixels, min_pixels, evaluations, inlier_threshold)) return st;
  PCNN_REQUIRE(evaluations == 0 || (energy && evals && listed), PCNN_ENULL, "pose3d_estimate_polished: a polish output is NULL");
  const Carve cv = carve(B, H, W, C, hypotheses, 3);
  const size_t extra = evaluations ? polish_ws_bytes(B, C, max_pixels) : 0;
  PCNN_REQUIRE_WORKSPACE("pose3d_estimate_polished", workspace, workspace_bytes, cv.total + extra);
  if (int st = pcnn_pose3d_estimate_fwd(label, depth, vertex_pred, extents, intrinsics, streams, factor_depth, seed0, seed1, B, H, W,
                                        C, hypotheses, pixel_batch, max_pixels, ref_it, min_area, inlier_threshold, min_dist,
                                        max_attempts, poses64, poses32, inliers, ref_steps, num_hyps, workspace, cv.total, stream))
    return st;
  if (evaluations == 0) return PCNN_OK;
  char* ws = static_cast<char*>(workspace);
  launch_polish(0, reinterpret_cast<const float*>(ws + cv.records), reinterpret_cast<const int32_t*>(ws + cv.counts),
                reinterpret_cast<const int32_t*>(ws + cv.offsets), intrinsics, poses64, inliers, B, H, W, C, max_pixels, min_pixels,
                evaluations, inlier_threshold, poses64, poses32, energy, evals, listed, ws + cv.total, (hipStream_t)stream);
  return check_launch("pose3d_estimate_polished_fwd");
}

extern "C" int pcnn_pose2d_estimate_polished_fwd(const int32_t* label, const float* vertex_pred, const float* extents,
                                                 const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1,
                                                 int B, int H, int W, int C, int hypotheses, int pixel_batch, int max_pixels,
                                                 int ref_it, int min_area, float inlier_threshold, float min_dist2d,
                                                 float min_dist3d, int max_attempts, int min_pixels, int evaluations,
                                                 double* poses64, float* poses32, int32_t* inliers, int32_t* ref_steps,
                                                 int32_t* num_hyps, double* energy, int32_t* evals, int32_t* listed,
                                                 void* workspace, size_t workspace_bytes, void* stream)
{
  if (int st = check_shape("pose2d_estimate_polished", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_estimate_polished", hypotheses)) return st;
  if (int st = check_polish_args("pose2d_estimate_polished", max_pixels, min_pixels, evaluations, inlier_threshold)) return st;
  PCNN_REQUIRE(evaluations == 0 || (energy && evals && listed), PCNN_ENULL, "pose2d_estimate_polished: a polish output is NULL");
  const Carve cv = carve(B, H, W, C, hypotheses, 4);
  const size_t extra = evaluations ? polish_ws_bytes(B, C, max_pixels) : 0;
  PCNN_REQUIRE_WORKSPACE("pose2d_estimate_polished", workspace, workspace_bytes, cv.total + extra);
  if (int st = pcnn_pose2d_estimate_fwd(label, vertex_pred, extents, intrinsics, streams, seed0, seed1, B, H, W, C, hypotheses,
                                        pixel_batch, max_pixels, ref_it, min_area, inlier_threshold, min_dist2d, min_dist3d,
                                        max_attempts, poses64, poses32, inliers, ref_steps, num_hyps, workspace, cv.total, stream))
    return st;
  if (evaluations == 0) return PCNN_OK;
  char* ws = static_cast<char*>(workspace);
  launch_polish(1, reinterpret_cast<const float*>(ws + cv.records), reinterpret_cast<const int32_t*>(ws + cv.counts),
                reinterpret_cast<const int32_t*>(ws + cv.offsets), intrinsics, poses64, inliers, B, H, W, C, max_pixels, min_pixels,
                evaluations, inlier_threshold, poses64, poses32, energy, evals, listed, ws + cv.total, (hipStream_t)stream);
  return check_launch("pose2d_estimate_polished_fwd");
}
