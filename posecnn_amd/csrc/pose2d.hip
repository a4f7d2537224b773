// pose2d.hip — the colour-only pose stage of the 3-D vertex route: Synthesizer::estimatePose2D
// (lib/synthesize/synthesize.cpp:1571-1767) as three launches per batch with nothing returning to the host in between.
// Arithmetic, orders and the deviations from the reference: include/posecnn_hip_pose2d.h; the numpy restatement is
// tests/pose2d_ref.py (bit for bit). The class compaction, the preemptive loop, Horn's fit and the box gate are the depth
// route's own code (pose_device.h); this file adds what 2-D - 3-D pairs need:
//
//   p2d_prepare_kernel   prepare_body<false>: records (x, y, 0, obj xyz), no depth read.
//   p2d_sample_kernel    one thread per (frame, hypothesis): at most max_attempts Philox blocks, each four records, Grunert's
//                        quartic on the first three by Ferrari's factorisation in + - x / sqrt (80 Newton steps on the
//                        resolvent cubic, 4 polish steps per root), a 3-point Horn fit per root with positive ranges, the
//                        fourth pair chooses.
//   p2d_ransac_kernel    ransac_body<Route2D>: the inlier test is the reprojection distance, the refit PCNN_POSE2D_GN_STEPS
//                        Gauss-Newton steps — 27 wave-folded sums, a 6 x 6 Cholesky solve every lane repeats on the same
//                        bits, a quaternion retraction.
// Which side bounds them (reasoning, no counters collected): sample is one divergent thread per hypothesis and bound by
// the dependent f64 chain of an attempt (~80 x 12 operations of the cubic, up to four fits of ~2000); ransac spends ~35 f64
// operations on a record per (hypothesis, round) in the count and ~250 per selected record and Gauss-Newton step in the
// refit: f64 ALU bound.
#include "philox_device.h"
#include "pose_device.h"

#include "../../include/posecnn_hip_pose2d.h"

namespace {

using namespace pcnn;
using namespace pcnn::pose;

static_assert(PCNN_POSE2D_RECORD == REC && PCNN_POSE2D_MAX_HYPOTHESES == MAX_HYP, "the two routes share record and loop");

struct Camera {
  double fx, fy, px, py;
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ K)
{
  return Camera{(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
}

// q = R o + t, the header's order
__device__ __forceinline__ void transform(const double* P, const float* o, double* q)
{
  const double ox = (double)o[0], oy = (double)o[1], oz = (double)o[2];
  q[0] = ((P[0] * ox + P[1] * oy) + P[2] * oz) + P[3];
  q[1] = ((P[4] * ox + P[5] * oy) + P[6] * oz) + P[7];
  q[2] = ((P[8] * ox + P[9] * oy) + P[10] * oz) + P[11];
}

// REPROJ of the header: the distance; `front` = q.z > 0
__device__ __forceinline__ double reproj(const double* P, const Rec& r, const Camera& K, bool& front)
{
  double q[3];
  transform(P, r.o, q);
  front = q[2] > 0.0;
  const double du = (K.fx * q[0] / q[2] + K.px) - (double)r.e[0];
  const double dv = (K.fy * q[1] / q[2] + K.py) - (double)r.e[1];
  return __builtin_sqrt(du * du + dv * dv);
}

__device__ __forceinline__ bool all_finite(const double* P)
{
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && (P[i] - P[i] == 0.0);
  return ok;
}

// QUARTIC of the header: v[0..3], NaN where Ferrari's factorisation has no real root for the slot
__device__ __forceinline__ void quartic_roots(double A4, double A3, double A2, double A1, double A0, double* v)
{
  const double B = A3 / A4, C = A2 / A4, Dd = A1 / A4, E = A0 / A4;
  const double B2 = B * B;
  const double p = C - 0.375 * B2;
  const double q = (Dd - 0.5 * B * C) + 0.125 * B2 * B;
  const double r = ((E - 0.25 * B * Dd) + 0.0625 * B2 * C) - 0.01171875 * B2 * B2;
  const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
  double mx = __builtin_fabs(c2);
  mx = __builtin_fabs(c1) > mx ? __builtin_fabs(c1) : mx;
  mx = __builtin_fabs(c0) > mx ? __builtin_fabs(c0) : mx;
  double m = 1.0 + mx;
  for (int i = 0; i < PCNN_POSE2D_CUBIC_STEPS; ++i) {
    const double g = ((m + c2) * m + c1) * m + c0;
    const double dg = (3.0 * m + 2.0 * c2) * m + c1;
    m = m - g / dg;
  }
  double y[4];
  if (m > 0.0) {
    const double s = __builtin_sqrt(2.0 * m);
    const double h = 0.5 * p + m;
    const double t = q / (2.0 * s);
    const double sd1 = __builtin_sqrt(s * s - 4.0 * (h + t));
    const double sd2 = __builtin_sqrt(s * s - 4.0 * (h - t));
    y[0] = 0.5 * (s + sd1), y[1] = 0.5 * (s - sd1), y[2] = 0.5 * (sd2 - s), y[3] = 0.5 * ((-s) - sd2);
  } else {   // the biquadratic (also for a NaN)
    const double sd = __builtin_sqrt(p * p - 4.0 * r);
    const double z1 = __builtin_sqrt(0.5 * (sd - p)), z2 = __builtin_sqrt(0.5 * ((-p) - sd));
    y[0] = z1, y[1] = -z1, y[2] = z2, y[3] = -z2;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double x = y[k] - 0.25 * B;
    for (int i = 0; i < PCNN_POSE2D_POLISH_STEPS; ++i) {
      const double f = (((x + B) * x + C) * x + Dd) * x + E;
      const double df = ((4.0 * x + 3.0 * B) * x + 2.0 * C) * x + Dd;
      x = x - f / df;
    }
    v[k] = x;
  }
}

// P3P of the header on r[0..2], r[3] chooses: false without a solution
__device__ __forceinline__ bool p3p(const Rec* r, const Camera& K, double* Pbest)
{
  double f[3][3], o[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double bx = ((double)r[i].e[0] - K.px) / K.fx, by = ((double)r[i].e[1] - K.py) / K.fy;
    const double nrm = __builtin_sqrt((bx * bx + by * by) + 1.0);
    f[i][0] = bx / nrm, f[i][1] = by / nrm, f[i][2] = 1.0 / nrm;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[i][k] = (double)r[i].o[k];
  }
  auto d2 = [&](int i, int j) {
    const double dx = o[i][0] - o[j][0], dy = o[i][1] - o[j][1], dz = o[i][2] - o[j][2];
    return (dx * dx + dy * dy) + dz * dz;
  };
  auto dot = [&](int i, int j) { return (f[i][0] * f[j][0] + f[i][1] * f[j][1]) + f[i][2] * f[j][2]; };
  const double a2 = d2(1, 2), b2 = d2(0, 2), c2 = d2(0, 1);
  const double ca = dot(1, 2), cb = dot(0, 2), cg = dot(0, 1);
  const double q = (a2 - c2) / b2, rr = (a2 + c2) / b2, cob = c2 / b2, aob = a2 / b2;
  const double qm = q - 1.0, ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
  const double A4 = qm * qm - 4.0 * cob * ca2;
  const double A3 = 4.0 * ((q * (1.0 - q) * cb - (1.0 - rr) * ca * cg) + 2.0 * cob * ca2 * cb);
  const double A2 = 2.0 * (((((q * q - 1.0) + 2.0 * q * q * cb2) + 2.0 * ((b2 - c2) / b2) * ca2) - 4.0 * rr * ca * cb * cg) +
                           2.0 * ((b2 - a2) / b2) * cg2);
  const double A1 = 4.0 * ((-q * (1.0 + q) * cb + 2.0 * aob * cg2 * cb) - (1.0 - rr) * ca * cg);
  const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * aob * cg2;
  const double b = __builtin_sqrt(b2);
  double v4[4];
  quartic_roots(A4, A3, A2, A1, A0, v4);

  double best = __builtin_inf();
  bool found = false;
  for (int k = 0; k < 4; ++k) {
    const double v = v4[k];
    const double u = (((qm * v * v - 2.0 * q * cb * v) + 1.0) + q) / (2.0 * (cg - v * ca));
    const double s1 = b / __builtin_sqrt((1.0 + v * v) - 2.0 * v * cb);
    const double s2 = u * s1, s3 = v * s1;
    if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
    const double sc[3] = {s1, s2, s3};
    Sums s;
    sums_zero(s);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double e[3] = {sc[i] * f[i][0], sc[i] * f[i][1], sc[i] * f[i][2]};
      sums_add(s, o[i], e);
    }
    double P[12];
    fit_pose(s, 3, P);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double qq[3];
      transform(P, r[i].o, qq);
      ok = ok && qq[2] > 0.0;
    }
    bool front;
    const double d4 = reproj(P, r[3], K, front);
    if (ok && d4 < best) {
      best = d4;
      found = true;
#pragma unroll
      for (int i = 0; i < 12; ++i) Pbest[i] = P[i];
    }
  }
  return found;
}

__device__ __forceinline__ double dist2(const float* a, const float* b)
{
  const double dx = (double)(a[0] - b[0]), dy = (double)(a[1] - b[1]);
  return __builtin_sqrt(dx * dx + dy * dy);
}

// pointLineDistance (synthesize.cpp:1075): f32 differences, widened; |(p2 - p1) x (p3 - p1)| / |p2 - p1|
__device__ __forceinline__ double point_line(const float* p1, const float* p2, const float* p3)
{
  const double a0 = (double)(p2[0] - p1[0]), a1 = (double)(p2[1] - p1[1]), a2 = (double)(p2[2] - p1[2]);
  const double b0 = (double)(p3[0] - p1[0]), b1 = (double)(p3[1] - p1[1]), b2 = (double)(p3[2] - p1[2]);
  const double cx = a1 * b2 - a2 * b1, cy = a2 * b0 - a0 * b2, cz = a0 * b1 - a1 * b0;
  return __builtin_sqrt((cx * cx + cy * cy) + cz * cz) / __builtin_sqrt((a0 * a0 + a1 * a1) + a2 * a2);
}

constexpr int tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }   // (i, j), i <= j, of the 6 x 6 upper triangle
static_assert(tri(0, 0) == 0 && tri(0, 5) == 5 && tri(1, 1) == 6 && tri(5, 5) == 20, "21 entries, row by row");

// the colour route's inlier test and refit for the shared loop (pose_device.h)
struct Route2D {
  double thr;
  const float* intrinsics;
  Camera K;
  __device__ void frame(int b) { K = load_camera(intrinsics + b * 4); }
  __device__ bool inlier(const double* P, const Rec& r) const
  {
    bool front;
    const double d = reproj(P, r, K, front);
    return front && d < thr;
  }

  // REFIT of the header: `P` holds the pose the inlier list is taken under; it leaves as it came when a solve fails
  __device__ void refit(double* P, const float* __restrict__ rec, int n, int m, int cnt, int max_pixels, int lane) const
  {
    double P0[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P0[i] = P[i];
    bool good = true;
    const Camera cam = K;
#pragma unroll 1
    for (int step = 0; step < PCNN_POSE2D_GN_STEPS; ++step) {
      double Hs[21], g[6];
#pragma unroll
      for (int i = 0; i < 21; ++i) Hs[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) g[i] = 0.0;
      visit_selected(*this, P0, rec, n, m, cnt, max_pixels, lane, [&](const Rec& r) {
        const double ox = (double)r.o[0], oy = (double)r.o[1], oz = (double)r.o[2];
        const double y0 = (P[0] * ox + P[1] * oy) + P[2] * oz;
        const double y1 = (P[4] * ox + P[5] * oy) + P[6] * oz;
        const double y2 = (P[8] * ox + P[9] * oy) + P[10] * oz;
        const double qx = y0 + P[3], qy = y1 + P[7], qz = y2 + P[11];
        const double ru = (cam.fx * qx / qz + cam.px) - (double)r.e[0];
        const double rv = (cam.fy * qy / qz + cam.py) - (double)r.e[1];
        const double iz = 1.0 / qz;
        const double a = cam.fx * iz, b = cam.fy * iz;
        const double c = -(cam.fx * qx * iz * iz), d = -(cam.fy * qy * iz * iz);
        const double Ju[6] = {c * y1, a * y2 - c * y0, -(a * y1), a, 0.0, c};
        const double Jv[6] = {d * y1 - b * y2, -(d * y0), b * y0, 0.0, b, d};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = i; j < 6; ++j) Hs[tri(i, j)] = Hs[tri(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
          g[i] = g[i] + (Ju[i] * ru + Jv[i] * rv);
        }
      });
#pragma unroll
      for (int i = 0; i < 21; ++i) Hs[i] = wave_fold(Hs[i]);
#pragma unroll
      for (int i = 0; i < 6; ++i) g[i] = wave_fold(g[i]);

      // H x = -g by Cholesky, the header's order, in place: L_ij (i >= j) takes the register of H_ji, x that of z; every
      // lane holds the same bits
      double x[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = Hs[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - Hs[tri(k, j)] * Hs[tri(k, j)];
        good = good && d > 0.0 && (d - d == 0.0);
        Hs[tri(j, j)] = __builtin_sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double t = Hs[tri(j, i)];
#pragma unroll
          for (int k = 0; k < j; ++k) t = t - Hs[tri(k, i)] * Hs[tri(k, j)];
          Hs[tri(j, i)] = t / Hs[tri(j, j)];
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double t = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = t - Hs[tri(k, i)] * x[k];
        x[i] = t / Hs[tri(i, i)];
      }
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double t = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t = t - Hs[tri(i, k)] * x[k];
        x[i] = t / Hs[tri(i, i)];
      }

      // t <- t + dt, R <- Q(dq) R, dq = (1, omega / 2) normalised
      const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
      const double nrm = __builtin_sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
      const double w = 1.0 / nrm, xq = hx / nrm, yq = hy / nrm, zq = hz / nrm;
      const double xx = xq * xq, yy = yq * yq, zz = zq * zq, xy = xq * yq, xz = xq * zq, yz = yq * zq, wx = w * xq, wy = w * yq,
                   wz = w * zq;
      const double Q[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                              {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                              {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
      double N[12];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) N[4 * i + j] = (Q[i][0] * P[j] + Q[i][1] * P[4 + j]) + Q[i][2] * P[8 + j];
        N[4 * i + 3] = P[4 * i + 3] + x[3 + i];
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) P[i] = N[i];
      good = good && all_finite(P);
    }
    if (!good) {
#pragma unroll
      for (int i = 0; i < 12; ++i) P[i] = P0[i];
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void p2d_prepare_kernel(const int32_t* __restrict__ label,
                                                                   const float* __restrict__ vertex_pred,
                                                                   const float* __restrict__ extents, int H, int W, int C,
                                                                   float* __restrict__ records, int32_t* __restrict__ counts,
                                                                   int32_t* __restrict__ offsets)
{
  prepare_body<false>(label, nullptr, vertex_pred, extents, nullptr, 1.f, H, W, C, records, counts, offsets);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAMPLE_THREADS) void p2d_sample_kernel(
    const float* __restrict__ records, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    const float* __restrict__ extents, const float* __restrict__ intrinsics, const unsigned long long* __restrict__ streams,
    unsigned long long k0, unsigned long long k1, int H, int W, int C, int Hyp, int max_attempts, int min_area, double thr,
    double min_dist2d, double min_dist3d, double* __restrict__ hyp_pose, int32_t* __restrict__ hyp_class,
    int32_t* __restrict__ hyp_attempt, int32_t* __restrict__ hyp_rec)
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
  const float* Kf = intrinsics + b * 4;
  const Camera K = load_camera(Kf);
  const size_t slot = (size_t)b * Hyp + h;

  for (int att = 0; att < max_attempts && nlive > 0; ++att) {
    unsigned long long w[4];
    philox4x64((unsigned long long)att, stream, (unsigned long long)h, k0, k1, w);
    const int c = s_live[(int)(((w[0] >> 32) * (unsigned long long)nlive) >> 32)];
    const unsigned long long n = (unsigned long long)s_cnt[c];   // > min_area >= 0
    const float* base = records + ((size_t)b * HW + s_off[c]) * REC;
    int j[4];
    Rec r[4];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long word = i < 3 ? w[1 + i] >> 32 : w[0] & 0xFFFFFFFFull;   // the fourth: the class word's low half
      j[i] = (int)((word * n) >> 32);                                                  // < n
      r[i] = load_rec(base + (size_t)j[i] * REC);
      ok = ok && !(r[i].o[0] == 0.f && r[i].o[1] == 0.f && r[i].o[2] == 0.f);
#pragma unroll
      for (int k = 0; k < i; ++k) ok = ok && !(dist2(r[k].e, r[i].e) < min_dist2d) && !(dist3(r[k].o, r[i].o) < min_dist3d);
    }
    ok = ok && !(point_line(r[0].o, r[1].o, r[2].o) < min_dist3d) && !(point_line(r[0].o, r[1].o, r[3].o) < min_dist3d) &&
         !(point_line(r[0].o, r[2].o, r[3].o) < min_dist3d) && !(point_line(r[1].o, r[2].o, r[3].o) < min_dist3d);
    if (!ok) continue;
    double P[12];
    if (!p3p(r, K, P)) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool front;
      const double d = reproj(P, r[i], K, front);
      ok = ok && front && d < thr;
    }
    if (!ok || !all_finite(P)) continue;
    if (!box_ok(P, extents + c * 3, Kf, H, W, min_area)) continue;
#pragma unroll
    for (int i = 0; i < 12; ++i) hyp_pose[slot * 12 + i] = P[i];
    hyp_class[slot] = c;
    hyp_attempt[slot] = att;
#pragma unroll
    for (int i = 0; i < 4; ++i) hyp_rec[slot * 4 + i] = j[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) hyp_pose[slot * 12 + i] = 0.0;
  hyp_class[slot] = 0;
  hyp_attempt[slot] = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i) hyp_rec[slot * 4 + i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// single != 0: one round (`first_round`) on caller-given hypotheses, per-slot outputs (wpose IS pose_out);
// single == 0: the whole loop, per-class outputs.
__global__ __launch_bounds__(RANSAC_THREADS) void p2d_ransac_kernel(
    const float* __restrict__ records, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    const float* __restrict__ intrinsics, const double* hyp_pose, const int32_t* __restrict__ hyp_class, int HW, int C, int Hyp,
    int first_round, int single, int pixel_batch, int max_pixels, int ref_it, double thr, double* wpose,
    int32_t* __restrict__ class_out, int32_t* __restrict__ inl_out, double* __restrict__ poses64,
    float* __restrict__ poses32, int32_t* __restrict__ inliers, int32_t* __restrict__ ref_steps_out,
    int32_t* __restrict__ num_hyps)
{
  ransac_body(Route2D{thr, intrinsics, Camera{}}, records, counts, offsets, hyp_pose, hyp_class, HW, C, Hyp, first_round, single,
              pixel_batch, max_pixels, ref_it, wpose, class_out, inl_out, poses64, poses32, inliers, ref_steps_out, num_hyps);
}

// ---------------------------------------------------------------------------------------------------------------------
int check_sample_args(const char* who, int max_attempts, int min_area, float thr, float min_dist2d, float min_dist3d)
{
  PCNN_REQUIRE(max_attempts >= 1, PCNN_EINVAL, "%s: max_attempts must be at least 1 (got %d)", who, max_attempts);
  PCNN_REQUIRE(min_area >= 0, PCNN_EINVAL, "%s: min_area must not be negative (got %d)", who, min_area);
  PCNN_REQUIRE(finite(thr) && finite(min_dist2d) && finite(min_dist3d), PCNN_EINVAL,
               "%s: inlier_threshold, min_dist2d and min_dist3d must be finite", who);
  return PCNN_OK;
}

void launch_prepare(const int32_t* label, const float* vertex_pred, const float* extents, int B, int H, int W, int C,
                    float* records, int32_t* counts, int32_t* offsets, hipStream_t stream)
{
  PCNN_LAUNCH(p2d_prepare_kernel, dim3(B), dim3(PREP_THREADS), 0, stream, label, vertex_pred, extents, H, W, C, records, counts,
              offsets);
}

void launch_sample(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                   const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                   int Hyp, int max_attempts, int min_area, float thr, float min_dist2d, float min_dist3d, double* hyp_pose,
                   int32_t* hyp_class, int32_t* hyp_attempt, int32_t* hyp_rec, hipStream_t stream)
{
  PCNN_LAUNCH(p2d_sample_kernel, dim3((Hyp + SAMPLE_THREADS - 1) / SAMPLE_THREADS, B), dim3(SAMPLE_THREADS), 0, stream, records,
              counts, offsets, extents, intrinsics, reinterpret_cast<const unsigned long long*>(streams),
              (unsigned long long)seed0, (unsigned long long)seed1, H, W, C, Hyp, max_attempts, min_area, (double)thr,
              (double)min_dist2d, (double)min_dist3d, hyp_pose, hyp_class, hyp_attempt, hyp_rec);
}

}  // namespace

extern "C" int pcnn_pose2d_workspace_bytes(int B, int H, int W, int C, int hypotheses, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "pose2d_workspace_bytes: bytes is NULL");
  if (int st = check_shape("pose2d_workspace_bytes", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_workspace_bytes", hypotheses)) return st;
  *bytes = carve(B, H, W, C, hypotheses, 4).total;
  return PCNN_OK;
}

extern "C" int pcnn_pose2d_prepare_fwd(const int32_t* label, const float* vertex_pred, const float* extents, int B, int H, int W,
                                       int C, float* records, int32_t* counts, int32_t* offsets, void* stream)
{
  if (int st = check_shape("pose2d_prepare", B, H, W, C)) return st;
  PCNN_REQUIRE(label && vertex_pred && extents, PCNN_ENULL, "pose2d_prepare: an input is NULL");
  PCNN_REQUIRE(records && counts && offsets, PCNN_ENULL, "pose2d_prepare: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose2d_prepare: records must be 8-byte aligned");
  launch_prepare(label, vertex_pred, extents, B, H, W, C, records, counts, offsets, (hipStream_t)stream);
  return check_launch("pose2d_prepare_fwd");
}

extern "C" int pcnn_pose2d_sample_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                                      const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B,
                                      int H, int W, int C, int hypotheses, int max_attempts, int min_area,
                                      float inlier_threshold, float min_dist2d, float min_dist3d, double* hyp_pose,
                                      int32_t* hyp_class, int32_t* hyp_attempt, int32_t* hyp_rec, void* stream)
{
  if (int st = check_shape("pose2d_sample", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_sample", hypotheses)) return st;
  if (int st = check_sample_args("pose2d_sample", max_attempts, min_area, inlier_threshold, min_dist2d, min_dist3d)) return st;
  PCNN_REQUIRE(records && counts && offsets && extents && intrinsics && streams, PCNN_ENULL, "pose2d_sample: an input is NULL");
  PCNN_REQUIRE(hyp_pose && hyp_class && hyp_attempt && hyp_rec, PCNN_ENULL, "pose2d_sample: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose2d_sample: records must be 8-byte aligned");
  launch_sample(records, counts, offsets, extents, intrinsics, streams, seed0, seed1, B, H, W, C, hypotheses, max_attempts,
                min_area, inlier_threshold, min_dist2d, min_dist3d, hyp_pose, hyp_class, hyp_attempt, hyp_rec,
                (hipStream_t)stream);
  return check_launch("pose2d_sample_fwd");
}

extern "C" int pcnn_pose2d_round_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* intrinsics,
                                     const double* hyp_pose, const int32_t* hyp_class, int B, int H, int W, int C, int hypotheses,
                                     int round, int pixel_batch, int max_pixels, float inlier_threshold, double* pose_out,
                                     int32_t* class_out, int32_t* inliers_out, void* stream)
{
  if (int st = check_shape("pose2d_round", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_round", hypotheses)) return st;
  if (int st = check_round_args("pose2d_round", round, pixel_batch, max_pixels, inlier_threshold)) return st;
  PCNN_REQUIRE(records && counts && offsets && intrinsics && hyp_pose && hyp_class, PCNN_ENULL, "pose2d_round: an input is NULL");
  PCNN_REQUIRE(pose_out && class_out && inliers_out, PCNN_ENULL, "pose2d_round: an output is NULL");
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7u) == 0, PCNN_EINVAL, "pose2d_round: records must be 8-byte aligned");
  PCNN_REQUIRE(pose_out != hyp_pose, PCNN_EINVAL, "pose2d_round: pose_out must not be hyp_pose");
  PCNN_LAUNCH(p2d_ransac_kernel, dim3(C, B), dim3(RANSAC_THREADS), 0, (hipStream_t)stream, records, counts, offsets, intrinsics,
              hyp_pose, hyp_class, H * W, C, hypotheses, round, 1, pixel_batch, max_pixels, 0, (double)inlier_threshold, pose_out,
              class_out, inliers_out, (double*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
              (int32_t*)nullptr);
  return check_launch("pose2d_round_fwd");
}

extern "C" int pcnn_pose2d_estimate_fwd(const int32_t* label, const float* vertex_pred, const float* extents,
                                        const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B,
                                        int H, int W, int C, int hypotheses, int pixel_batch, int max_pixels, int ref_it,
                                        int min_area, float inlier_threshold, float min_dist2d, float min_dist3d,
                                        int max_attempts, double* poses64, float* poses32, int32_t* inliers, int32_t* ref_steps,
                                        int32_t* num_hyps, void* workspace, size_t workspace_bytes, void* stream_)
{
  if (int st = check_shape("pose2d_estimate", B, H, W, C)) return st;
  if (int st = check_hyp("pose2d_estimate", hypotheses)) return st;
  if (int st = check_sample_args("pose2d_estimate", max_attempts, min_area, inlier_threshold, min_dist2d, min_dist3d)) return st;
  PCNN_REQUIRE(ref_it >= 0 && ref_it <= (1 << 20), PCNN_EINVAL, "pose2d_estimate: ref_it must be in [0, 2^20] (got %d)", ref_it);
  if (int st = check_round_args("pose2d_estimate", 32 + ref_it, pixel_batch, max_pixels, inlier_threshold)) return st;
  PCNN_REQUIRE(label && vertex_pred && extents && intrinsics && streams, PCNN_ENULL, "pose2d_estimate: an input is NULL");
  PCNN_REQUIRE(poses64 && poses32 && inliers && ref_steps && num_hyps, PCNN_ENULL, "pose2d_estimate: an output is NULL");
  const Carve cv = carve(B, H, W, C, hypotheses, 4);
  PCNN_REQUIRE_WORKSPACE("pose2d_estimate", workspace, workspace_bytes, cv.total);

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
  launch_prepare(label, vertex_pred, extents, B, H, W, C, records, counts, offsets, stream);
  launch_sample(records, counts, offsets, extents, intrinsics, streams, seed0, seed1, B, H, W, C, hypotheses, max_attempts,
                min_area, inlier_threshold, min_dist2d, min_dist3d, hyp_pose, hyp_class, hyp_attempt, hyp_rec, stream);
  PCNN_LAUNCH(p2d_ransac_kernel, dim3(C, B), dim3(RANSAC_THREADS), 0, stream, records, counts, offsets, intrinsics, hyp_pose,
              hyp_class, H * W, C, hypotheses, 1, 0, pixel_batch, max_pixels, ref_it, (double)inlier_threshold, wpose,
              (int32_t*)nullptr, (int32_t*)nullptr, poses64, poses32, inliers, ref_steps, num_hyps);
  return check_launch("pose2d_estimate_fwd");
}
