// pose_device.h — what the two pose stages of the 3-D vertex route share: pose3d.hip (depth: object point against camera
// point, include/posecnn_hip_pose3d.h) and pose2d.hip (colour only: object point against pixel, include/posecnn_hip_pose2d.h).
// One copy of the six-float record and its load, the Sums and their fold order, Horn's fit, the projected-box gate, the
// subset index, the class compaction (`prepare_body`) and the preemptive loop (`ransac_body`). A route plugs its inlier test
// and its refit into the loop:
//     struct Route { __device__ void frame(int b);                                  // per-frame state (intrinsics)
//                    __device__ bool inlier(const double* P, const Rec& r) const;
//                    __device__ void refit(double* P, const float* rec, int n, int m, int cnt, int max_pixels, int lane) const; };
// Arithmetic, orders and the loop's steps are stated in the two public headers; nothing here fuses or reorders.
// `visit_listed` is the list of the routes' final polish (pose_polish.hip, include/posecnn_hip/pose_polish.h).
#pragma once
#include "pcnn_device.h"

#include "../../include/posecnn_hip_pose3d.h"

namespace pcnn {
namespace pose {

constexpr int PREP_THREADS = 1024, PREP_WAVES = PREP_THREADS / PCNN_WAVE;
constexpr int SAMPLE_THREADS = 64;
constexpr int RANSAC_THREADS = 512, RANSAC_WAVES = RANSAC_THREADS / PCNN_WAVE;
constexpr int MAX_HYP = PCNN_POSE3D_MAX_HYPOTHESES;
constexpr int REC = PCNN_POSE3D_RECORD;

// e: the camera point (depth route) or (pixel x, pixel y, 0) (colour route); o: the object point
struct Rec {
  float e[3], o[3];
};

struct Sums {
  double a[3], b[3], ab[9];
};

__device__ __forceinline__ Rec load_rec(const float* __restrict__ r)
{
  Rec v;
  const float2 p0 = *reinterpret_cast<const float2*>(r), p1 = *reinterpret_cast<const float2*>(r + 2),
               p2 = *reinterpret_cast<const float2*>(r + 4);
  v.e[0] = p0.x, v.e[1] = p0.y, v.e[2] = p1.x;
  v.o[0] = p1.y, v.o[1] = p2.x, v.o[2] = p2.y;
  return v;
}

__device__ __forceinline__ void sums_zero(Sums& s)
{
#pragma unroll
  for (int i = 0; i < 3; ++i) s.a[i] = 0.0, s.b[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s.ab[i] = 0.0;
}

// one pair onto the sums: a = the object point, b = the camera point
__device__ __forceinline__ void sums_add(Sums& s, const double* a, const double* b)
{
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.a[i] = s.a[i] + a[i];
    s.b[i] = s.b[i] + b[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s.ab[i * 3 + j] = s.ab[i * 3 + j] + a[i] * b[j];
}

__device__ __forceinline__ void sums_add(Sums& s, const Rec& r)
{
  const double a[3] = {(double)r.o[0], (double)r.o[1], (double)r.o[2]}, b[3] = {(double)r.e[0], (double)r.e[1], (double)r.e[2]};
  sums_add(s, a, b);
}

// FIT of posecnn_hip_pose3d.h: Horn's quaternion form, the 4 x 4 eigenproblem by a fixed number of cyclic Jacobi sweeps
__device__ __forceinline__ void fit_pose(const Sums& s, int n, double* P)
{
  const double dn = (double)n;
  double cA[3], cB[3], M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) cA[i] = s.a[i] / dn, cB[i] = s.b[i] / dn;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = s.ab[i * 3 + j] - s.a[i] * cB[j];
  const double Mxx = M[0], Mxy = M[1], Mxz = M[2], Myx = M[3], Myy = M[4], Myz = M[5], Mzx = M[6], Mzy = M[7], Mzz = M[8];
  double A[4][4], V[4][4];
  A[0][0] = (Mxx + Myy) + Mzz;
  A[1][1] = (Mxx - Myy) - Mzz;
  A[2][2] = (Myy - Mxx) - Mzz;
  A[3][3] = (Mzz - Mxx) - Myy;
  A[0][1] = A[1][0] = Myz - Mzy;
  A[0][2] = A[2][0] = Mzx - Mxz;
  A[0][3] = A[3][0] = Mxy - Myx;
  A[1][2] = A[2][1] = Mxy + Myx;
  A[1][3] = A[3][1] = Mzx + Mxz;
  A[2][3] = A[3][2] = Myz + Mzy;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;

  for (int sweep = 0; sweep < PCNN_POSE3D_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        double t = 0.0;
        if (apq != 0.0) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
        }
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double x = A[k][p], y = A[k][q];
          A[k][p] = c * x - sn * y;
          A[k][q] = sn * x + c * y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double x = A[p][k], y = A[q][k];
          A[p][k] = c * x - sn * y;
          A[q][k] = sn * x + c * y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double x = V[k][p], y = V[k][q];
          V[k][p] = c * x - sn * y;
          V[k][q] = sn * x + c * y;
        }
      }
  }
  double best = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > best) best = A[i][i], qw = V[0][i], qx = V[1][i], qy = V[2][i], qz = V[3][i];
  const double nrm = __builtin_sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  const double w = qw / nrm, x = qx / nrm, y = qy / nrm, z = qz / nrm;
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  P[0] = 1.0 - 2.0 * (yy + zz), P[1] = 2.0 * (xy - wz), P[2] = 2.0 * (xz + wy);
  P[4] = 2.0 * (xy + wz), P[5] = 1.0 - 2.0 * (xx + zz), P[6] = 2.0 * (yz - wx);
  P[8] = 2.0 * (xz - wy), P[9] = 2.0 * (yz + wx), P[10] = 1.0 - 2.0 * (xx + yy);
#pragma unroll
  for (int i = 0; i < 3; ++i) P[4 * i + 3] = cB[i] - ((P[4 * i] * cA[0] + P[4 * i + 1] * cA[1]) + P[4 * i + 2] * cA[2]);
}

__device__ __forceinline__ double dist3(const float* a, const float* b)
{
  const double dx = (double)(a[0] - b[0]), dy = (double)(a[1] - b[1]), dz = (double)(a[2] - b[2]);
  return __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
}

// the projected box of posecnn_hip_pose3d.h: false when a corner is not in front of the camera or the clamped area is below min_area
__device__ __forceinline__ bool box_ok(const double* P, const float* ext, const float* K, int H, int W, int min_area)
{
  const double hx = (double)(ext[0] * 0.5f), hy = (double)(ext[1] * 0.5f), hz = (double)(ext[2] * 0.5f);
  const double fx = (double)K[0], fy = (double)K[1], px = (double)K[2], py = (double)K[3];
  int minX = W - 1, maxX = 0, minY = H - 1, maxY = 0;
  for (int j = 0; j < 8; ++j) {
    const double cx = (j & 1) ? -hx : hx, cy = (j & 2) ? -hy : hy, cz = (j & 4) ? -hz : hz;
    const double qx = ((P[0] * cx + P[1] * cy) + P[2] * cz) + P[3];
    const double qy = ((P[4] * cx + P[5] * cy) + P[6] * cz) + P[7];
    const double qz = ((P[8] * cx + P[9] * cy) + P[10] * cz) + P[11];
    if (!(qz > 0.0)) return false;
    double u = fx * qx / qz + px, v = fy * qy / qz + py;
    u = u >= 0.0 ? u : 0.0;   // a NaN goes to 0 too
    v = v >= 0.0 ? v : 0.0;
    u = u <= (double)(W - 1) ? u : (double)(W - 1);
    v = v <= (double)(H - 1) ? v : (double)(H - 1);
    const int iu = (int)u, iv = (int)v;
    minX = iu < minX ? iu : minX;
    maxX = iu > maxX ? iu : maxX;
    minY = iv < minY ? iv : minY;
    maxY = iv > maxY ? iv : maxY;
  }
  return (long long)(maxX - minX + 1) * (maxY - minY + 1) >= (long long)min_area;
}

// floor(k n / m), the round's subset: from round ceil(n / pixel_batch) on m == n and the index is k itself — no 64-bit divide
__device__ __forceinline__ int subset_index(int k, int n, int m)
{
  return m == n ? k : (int)((long long)k * n / m);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// the fold of the 64 lane sums: v_l <- v_l + v_(l xor s), s = 32 .. 1; every lane ends with the same bits
__device__ __forceinline__ double wave_fold(double v)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s);
  return v;
}

// The refit's list: the round's subset records that are inliers under P0, in subset order, thinned when there are
// cnt >= max_pixels of them to the ranks floor(j cnt / max_pixels). Subset position k belongs to lane k mod 64 and a lane
// meets its records in ascending k: `visit(r)` adds onto the lane's own sums. Uniform over the wave (ballots inside).
template <class Route, class Visit>
__device__ __forceinline__ void visit_selected(const Route& route, const double* P0, const float* __restrict__ rec, int n, int m,
                                               int cnt, int max_pixels, int lane, Visit visit)
{
  int seen = 0;
  for (int k0 = 0; k0 < m; k0 += PCNN_WAVE) {
    const int k = k0 + lane;
    bool in = false;
    Rec r;
    if (k < m) {
      r = load_rec(rec + (size_t)subset_index(k, n, m) * REC);
      in = route.inlier(P0, r);
    }
    const unsigned long long mask = __ballot(in);
    if (in) {
      const long long rk = seen + __popcll(mask & lanemask_lt());
      bool sel = cnt < max_pixels;
      if (!sel) {   // rank floor(j cnt / max_pixels) for a j < max_pixels? j is increasing in the rank: at most one fits
        const long long j = (rk * max_pixels + cnt - 1) / cnt;
        sel = j < max_pixels && j * cnt / max_pixels == rk;
      }
      if (sel) visit(r);
    }
    seen += __popcll(mask);
  }
}

// The polish's list (include/posecnn_hip/pose_polish.h): `visit_selected` over ALL n records of the class (m == n), telling
// the visitor where the record stands in the list: `visit(j, r)`, j = its rank among the inliers, or the j with
// floor(j cnt / max_pixels) == rank when the list is thinned. j < min(cnt, max_pixels). Uniform over the wave.
template <class Route, class Visit>
__device__ __forceinline__ void visit_listed(const Route& route, const double* P0, const float* __restrict__ rec, int n, int cnt,
                                             int max_pixels, int lane, Visit visit)
{
  int seen = 0;
  for (int k0 = 0; k0 < n; k0 += PCNN_WAVE) {
    const int k = k0 + lane;
    bool in = false;
    Rec r;
    if (k < n) {
      r = load_rec(rec + (size_t)k * REC);
      in = route.inlier(P0, r);
    }
    const unsigned long long mask = __ballot(in);
    if (in) {
      const long long rk = seen + __popcll(mask & lanemask_lt());
      long long j = rk;
      bool sel = cnt < max_pixels;
      if (!sel) {
        j = (rk * max_pixels + cnt - 1) / cnt;
        sel = j < max_pixels && j * cnt / max_pixels == rk;
      }
      if (sel) visit((int)j, r);
    }
    seen += __popcll(mask);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// PREPARE of both headers, the body of a kernel of PREP_THREADS threads, one workgroup per frame. DEPTH: e = the camera
// point of the depth frame; otherwise e = ((float)x, (float)y, 0) and `depth`, `intrinsics`, `factor` are not read.
template <bool DEPTH>
__device__ __forceinline__ void prepare_body(const int32_t* __restrict__ label, const uint16_t* __restrict__ depth,
                                             const float* __restrict__ vertex_pred, const float* __restrict__ extents,
                                             const float* __restrict__ intrinsics, float factor, int H, int W, int C,
                                             float* __restrict__ records, int32_t* __restrict__ counts,
                                             int32_t* __restrict__ offsets)
{
  __shared__ int s_cnt[PCNN_MAX_CLASSES], s_base[PCNN_MAX_CLASSES];
  __shared__ int s_wc[PREP_WAVES][PCNN_MAX_CLASSES];
  const int t = threadIdx.x, b = blockIdx.x, HW = H * W, lane = t & 63, wave = t >> 6;
  const int32_t* lab = label + (size_t)b * HW;
  const uint16_t* dep = DEPTH ? depth + (size_t)b * HW : nullptr;
  const float* vp = vertex_pred + (size_t)b * HW * 3 * C;
  float* rec = records + (size_t)b * HW * REC;
  float fx = 1.f, fy = 1.f, px = 0.f, py = 0.f;
  if (DEPTH) fx = intrinsics[b * 4], fy = intrinsics[b * 4 + 1], px = intrinsics[b * 4 + 2], py = intrinsics[b * 4 + 3];

  // every wave owns one contiguous run of the raster: its records of a class follow those of the waves before it
  const int per = (HW + PREP_WAVES - 1) / PREP_WAVES;
  const int lo = wave * per < HW ? wave * per : HW, hi = lo + per < HW ? lo + per : HW;
  static_assert(PREP_WAVES * PCNN_MAX_CLASSES == PREP_THREADS, "one thread clears one entry of s_wc");
  (&s_wc[0][0])[t] = 0;
  __syncthreads();
  for (int p = lo + lane; p < hi; p += PCNN_WAVE) {
    const int c = lab[p];
    if (c >= 1 && c < C) atomicAdd(&s_wc[wave][c], 1);   // a count has no order
  }
  __syncthreads();
  if (t < C) {
    int tot = 0;
    for (int w = 0; w < PREP_WAVES; ++w) tot += s_wc[w][t];
    s_cnt[t] = tot;
  }
  __syncthreads();
  if (t == 0) {
    int off = 0;
    for (int c = 0; c < C; ++c) {
      s_base[c] = off;
      offsets[b * C + c] = off;
      counts[b * C + c] = s_cnt[c];
      off += s_cnt[c];
    }
  }
  __syncthreads();
  if (t < C) {                 // counts -> where each wave's run of the class starts
    int run = s_base[t];
    for (int w = 0; w < PREP_WAVES; ++w) {
      const int n = s_wc[w][t];
      s_wc[w][t] = run;
      run += n;
    }
  }
  __syncthreads();

  // no barrier from here on: a wave scatters its own run, 64 pixels at a time, against its own running bases
  volatile int* next = s_wc[wave];
  for (int p0 = lo; p0 < hi; p0 += PCNN_WAVE) {
    const int p = p0 + lane;
    int c = 0;
    if (p < hi) {
      c = lab[p];
      if (c < 1 || c >= C) c = 0;
    }
    int dst = 0;
    unsigned long long todo = __ballot(c > 0);
    while (todo) {          // one turn per class present in the wave (uniform: `todo` is the same in every lane)
      const int leader = __ffsll((long long)todo) - 1;
      const int lc = __shfl(c, leader);
      const unsigned long long same = __ballot(c == lc);
      const int base = next[lc];                      // read by every lane before the leader moves it on
      if (c == lc) dst = base + __popcll(same & lanemask_lt());   // < HW: the bases are the scan of this frame's own counts
      if (lane == leader) next[lc] = base + __popcll(same);
      todo &= ~same;
    }
    if (c > 0) {
      const int x = p % W, y = p / W;
      float ex = (float)x, ey = (float)y, ez = 0.f;
      if (DEPTH) {
        const unsigned d = dep[p];
        ex = 0.f, ey = 0.f;
        if (d != 0) {
          const float df = (float)d;
          ex = div_rn(div_rn(((float)x - px) * df, fx), factor);
          ey = div_rn(div_rn(((float)y - py) * df, fy), factor);
          ez = div_rn(df, factor);
        }
      }
      float o[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float e = extents[c * 3 + i];
        const float vmin = div_rn(-e, 2.f), vmax = div_rn(e, 2.f), span = vmax - vmin;
        const float a = (float)(1.0 / (double)span);
        const float bb = (float)(-1.0 * (double)vmin / (double)span);
        o[i] = div_rn(vp[(size_t)p * 3 * C + 3 * c + i] - bb, a);
      }
      float* r = rec + (size_t)dst * REC;
      *reinterpret_cast<float2*>(r) = make_float2(ex, ey);
      *reinterpret_cast<float2*>(r + 2) = make_float2(ez, o[0]);
      *reinterpret_cast<float2*>(r + 4) = make_float2(o[1], o[2]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// RANSAC of both headers, the body of a kernel of RANSAC_THREADS threads, one workgroup per (frame, class), barriers only.
// single != 0: one round (`first_round`) on caller-given hypotheses, per-slot outputs (wpose IS pose_out);
// single == 0: the whole loop, per-class outputs.
template <class Route>
__device__ __forceinline__ void ransac_body(Route route, const float* __restrict__ records, const int32_t* __restrict__ counts,
                                            const int32_t* __restrict__ offsets, const double* hyp_pose,
                                            const int32_t* __restrict__ hyp_class, int HW, int C, int Hyp, int first_round,
                                            int single, int pixel_batch, int max_pixels, int ref_it, double* wpose,
                                            int32_t* __restrict__ class_out, int32_t* __restrict__ inl_out,
                                            double* __restrict__ poses64, float* __restrict__ poses32,
                                            int32_t* __restrict__ inliers, int32_t* __restrict__ ref_steps_out,
                                            int32_t* __restrict__ num_hyps)
{
  __shared__ int s_id[2][MAX_HYP], s_inl[2][MAX_HYP];
  __shared__ int s_size;
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t* hc = hyp_class + (size_t)b * Hyp;
  double* wp = wpose + (size_t)b * Hyp * 12;
  const double* hp = hyp_pose + (size_t)b * Hyp * 12;
  route.frame(b);

  // the class's hypotheses in ascending index (class 0's workgroup takes, in a single round, the slots that hold none)
  if (wave == 0) {
    int base = 0;
    for (int h0 = 0; h0 < Hyp; h0 += PCNN_WAVE) {
      const int h = h0 + lane;
      bool mine = false;
      if (h < Hyp) {
        const int v = hc[h];
        mine = c == 0 ? (v < 1 || v >= C) : v == c;
      }
      const unsigned long long m = __ballot(mine);
      if (mine) s_id[0][base + __popcll(m & lanemask_lt())] = h;
      base += __popcll(m);
    }
    if (lane == 0) s_size = base;
  }
  __syncthreads();
  int size = s_size;
  const int size0 = size;

  if (c == 0) {
    if (single) {
      for (int i = t; i < size; i += RANSAC_THREADS) {
        const int id = s_id[0][i];
        class_out[(size_t)b * Hyp + id] = 0;
        inl_out[(size_t)b * Hyp + id] = 0;
        for (int k = 0; k < 12; ++k) wp[(size_t)id * 12 + k] = hp[(size_t)id * 12 + k];
      }
      return;
    }
    size = 0;
  }
  const size_t cls = (size_t)b * C + c;
  if (size == 0) {
    if (!single) {
      if (t < 12) poses64[cls * 12 + t] = 0.0, poses32[cls * 12 + t] = 0.f;
      if (t == 0) inliers[cls] = 0, ref_steps_out[cls] = 0, num_hyps[cls] = 0;
    }
    return;
  }

  for (int i = t; i < size * 12; i += RANSAC_THREADS) {
    const size_t at = (size_t)s_id[0][i / 12] * 12 + i % 12;
    wp[at] = hp[at];
  }
  if (single)
    for (int i = t; i < size; i += RANSAC_THREADS) s_inl[0][i] = 0;
  const int n = clampi(counts[cls], 0, HW);
  const float* rec = records + ((size_t)b * HW + clampi(offsets[cls], 0, HW - n)) * REC;
  __syncthreads();

  int cur = 0, ref_steps = 0, round = single ? first_round - 1 : 0;
  const int max_rounds = round + (single ? 1 : 32 + ref_it);   // size halves every round it is above 1: never reached
  while ((single || size > 1 || ref_steps < ref_it) && round < max_rounds) {
    round += 1;
    const long long want = (long long)pixel_batch * round;
    const int m = want < (long long)n ? (int)want : n;

    // 2. inliers of every hypothesis over the round's subset
    for (int i = wave; i < size; i += RANSAC_WAVES) {
      double P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = wp[(size_t)s_id[cur][i] * 12 + k];
      int cnt = 0;
      for (int k = lane; k < m; k += PCNN_WAVE) {
        const Rec r = load_rec(rec + (size_t)subset_index(k, n, m) * REC);
        cnt += route.inlier(P, r) ? 1 : 0;
      }
      cnt = wave_sum(cnt);
      if (lane == 0) s_inl[cur][i] = cnt;
    }
    __syncthreads();

    // 3. inliers descending, then index ascending; the first size / 2 stay
    if (size > 1) {
      const int keep = size / 2;
      for (int i = t; i < size; i += RANSAC_THREADS) {
        const int my = s_inl[cur][i], id = s_id[cur][i];
        int rank = 0;
        for (int k = 0; k < size; ++k) {
          const int o = s_inl[cur][k];
          rank += (o > my || (o == my && s_id[cur][k] < id)) ? 1 : 0;
        }
        if (rank < keep) {
          s_id[cur ^ 1][rank] = id;
          s_inl[cur ^ 1][rank] = my;
        } else if (single) {
          class_out[(size_t)b * Hyp + id] = 0;
          inl_out[(size_t)b * Hyp + id] = my;
        }
      }
      __syncthreads();
      cur ^= 1;
      size = keep;
    }

    // 4. refit of every survivor on its (thinned) inlier list
    for (int i = wave; i < size; i += RANSAC_WAVES) {
      const int cnt = s_inl[cur][i];
      if (cnt < 4) continue;                         // uniform over the wave
      const int id = s_id[cur][i];
      double P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = wp[(size_t)id * 12 + k];
      route.refit(P, rec, n, m, cnt, max_pixels, lane);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) wp[(size_t)id * 12 + k] = P[k];
      }
    }
    ref_steps += 1;
    __syncthreads();
  }

  if (single) {
    for (int i = t; i < size; i += RANSAC_THREADS) {
      class_out[(size_t)b * Hyp + s_id[cur][i]] = c;
      inl_out[(size_t)b * Hyp + s_id[cur][i]] = s_inl[cur][i];
    }
    return;
  }
  const int id = s_id[cur][0];
  if (t < 12) {
    const double v = wp[(size_t)id * 12 + t];
    poses64[cls * 12 + t] = v;
    poses32[cls * 12 + t] = (float)v;
  }
  if (t == 0) {
    inliers[cls] = round > 0 ? s_inl[cur][0] : 0;
    ref_steps_out[cls] = ref_steps;
    num_hyps[cls] = size0;
  }
}

// ---- host: the validation and the workspace layout of both routes -------------------------------------------------------
inline int check_shape(const char* who, int B, int H, int W, int C)
{
  PCNN_REQUIRE(B >= 1 && B <= 65535, PCNN_EINVAL, "%s: batch must be in [1, 65535] (got %d)", who, B);
  PCNN_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= (1ll << 24), PCNN_EINVAL,
               "%s: height and width must be at least 1 and height * width at most 2^24 (got %d x %d)", who, H, W);
  PCNN_REQUIRE(C >= 2 && C <= PCNN_MAX_CLASSES, PCNN_EINVAL, "%s: num_classes must be in [2, %d] (got %d)", who,
               PCNN_MAX_CLASSES, C);
  return PCNN_OK;
}

inline int check_hyp(const char* who, int hypotheses)
{
  PCNN_REQUIRE(hypotheses >= 1 && hypotheses <= MAX_HYP, PCNN_EINVAL, "%s: hypotheses must be in [1, %d] (got %d)", who, MAX_HYP,
               hypotheses);
  return PCNN_OK;
}

inline bool finite(float v) { return v - v == 0.f; }

inline int check_round_args(const char* who, int rounds, int pixel_batch, int max_pixels, float thr)
{
  PCNN_REQUIRE(pixel_batch >= 1 && max_pixels >= 1, PCNN_EINVAL, "%s: pixel_batch and max_pixels must be at least 1 (got %d, %d)",
               who, pixel_batch, max_pixels);
  PCNN_REQUIRE(rounds >= 1 && (long long)pixel_batch * rounds < (1ll << 31), PCNN_EINVAL,
               "%s: round must be at least 1 and pixel_batch * round below 2^31 (got %d, %d)", who, rounds, pixel_batch);
  PCNN_REQUIRE(finite(thr), PCNN_EINVAL, "%s: inlier_threshold must be finite", who);
  return PCNN_OK;
}

struct Carve {
  size_t records, counts, offsets, hyp_pose, hyp_class, hyp_attempt, hyp_rec, wpose, total;
};

// `points`: the records of one hypothesis (3 in the depth route, 4 in the colour route)
inline Carve carve(int B, int H, int W, int C, int Hyp, int points)
{
  Carve v;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += align_up(bytes, 16);
    return here;
  };
  v.records = take((size_t)B * H * W * REC * sizeof(float));
  v.counts = take((size_t)B * C * sizeof(int32_t));
  v.offsets = take((size_t)B * C * sizeof(int32_t));
  v.hyp_pose = take((size_t)B * Hyp * 12 * sizeof(double));
  v.hyp_class = take((size_t)B * Hyp * sizeof(int32_t));
  v.hyp_attempt = take((size_t)B * Hyp * sizeof(int32_t));
  v.hyp_rec = take((size_t)B * Hyp * points * sizeof(int32_t));
  v.wpose = take((size_t)B * Hyp * 12 * sizeof(double));
  v.total = at;
  return v;
}

}  // namespace pose
}  // namespace pcnn
