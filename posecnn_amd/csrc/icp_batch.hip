// icp_batch.hip — Synthesizer::solveICP (lib/synthesize/synthesize.cpp:2052-2380) for every detection row of a batch of
// frames in ONE call with no host round trip: the stages of icp.hip / render.hip (their device bodies, icp_device.h and
// render_device.h — one copy) with a job dimension, a job table built on the device and the arithmetic between the stages,
// which posecnn_amd/icp.py's per-frame path does in numpy on the host, in small glue kernels.
//
// Launch sequence (J = max_jobs job slots, P = H W pixels, every launch sized by J — the host never learns how many rows
// are live; the workgroups of a dead slot return at once):
//   icpb_count_kernel      grid R: row -> status (dead / background / no model / under min_pixels / refinable); a refinable
//                          row's label pixels are counted by its workgroup (integer tree, no atomics)
//   icpb_plan_kernel       1 workgroup: refinable rows, in row order, take the job slots (block prefix sum); rows past the
//                          capacity get status 5; job table = (row, frame, class, mesh ranges, live); zero output rows
//   icpb_pose_kernel       T = pose34(row)                                                      [glue, thread per job]
//   clear / raster / resolve   render at T: vertices, normals, canonical                        [grid.y = J]
//   icpb_backproject_kernel, icpb_center_kernel, icpb_center_sum_kernel                         [grid.y = J]
//   icpb_translate_kernel  agree, pairs; Tz = f32(sum dz) / f32(agree); t = (rx Tz, ry Tz, Tz)  [glue]
//   clear / raster / resolve   re-render the vertices (jobs with agree > 0)                     [grid.y = J]
//   icpb_polish_kernel     Nelder-Mead, one workgroup per job                                   [grid J]
//   icpb_hyps_kernel       T <- pose34(x) o T; poses_new row; the 8 depth hypotheses            [glue]
//   clear / raster / resolve   vertices + normals of the 8 hypotheses                           [grid.y = 8 J]
//   icpb_init_kernel, iterations x (icpb_terms_kernel, icpb_solve_kernel)                       [grid.y = 8 J; the live
//                          map is read by job index, not expanded eight times]
//   icpb_compose_kernel    hypothesis <- update o hypothesis                                    [glue, thread per (job, h)]
//   icpb_score_kernel      SegICP hits (jobs with pairs > 0)                                    [grid.y = 8 J]
//   icpb_output_kernel     first maximum, poses_icp row, info row                               [glue]
//
// Glue arithmetic: f64, + - x / sqrt only, each expression in the one order written below (3-term sums left to right:
// (a + b) + c); tests/icp_batch_ref.py restates the same expressions, and the outputs agree with it bit for bit.
#include <algorithm>

#include "icp_device.h"
#include "pcnn_device.h"
#include "render_device.h"

namespace {

using namespace pcnn;

constexpr int NHYP = 8;
constexpr int JOB_INTS = 8;      // row, frame, class, first vertex, vertices, first face, faces, live
constexpr int JF_INTS = 4;       // agree, pairs, polish ran, -
constexpr int MISC = 16;         // Tz, sums[5], polish x[7], polish info[2]
constexpr int INFO_COLS = 12;    // status, agree, pairs, choose, hits[8]

enum { ST_DEAD = 0, ST_REFINED = 1, ST_BACKGROUND = 2, ST_FEW_PIXELS = 3, ST_NO_MODEL = 4, ST_CAPACITY = 5 };

struct Ws {          // the caller's workspace, carved (every part 256-byte aligned)
  unsigned long long* zbuf;            // [8 J][P]
  float *v0, *n0, *c0, *live;          // [J][P][4], [J][P][4], [J][P][3], [J][P][3]
  unsigned char* mask;                 // [J][P]
  float *hv, *hn;                      // [8 J][P][4] each (slot 8 j also holds the re-render before the polish)
  float* partial;                      // [8 J][nblocks][29] (the center stage uses [J][nblocks][5] of it)
  unsigned* flags;                     // [8 J][nwords]
  double *T, *misc, *hyps, *upd;       // [J][12], [J][MISC], [8 J][12], [8 J][12]
  float* rp;                           // [8 J][12]: the f32 poses handed to the renderer / the score
  int *hits, *jobs, *jf;               // [8 J], [J][JOB_INTS], [J][JF_INTS]
  size_t bytes;
};

Ws carve(void* base, int J, int H, int W)
{
  const size_t P = (size_t)H * W, nb = (P + ICP_BLOCK - 1) / ICP_BLOCK, nw = (P + 31) / 32, j = (size_t)J;
  size_t off = 0;
  char* const b0 = static_cast<char*>(base);      // NULL: only the size is wanted
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return b0 ? b0 + o : nullptr; };
  Ws w;
  w.zbuf = (unsigned long long*)take(8 * NHYP * j * P);
  w.v0 = (float*)take(16 * j * P);
  w.n0 = (float*)take(16 * j * P);
  w.c0 = (float*)take(12 * j * P);
  w.live = (float*)take(12 * j * P);
  w.mask = (unsigned char*)take(j * P);
  w.hv = (float*)take(16 * NHYP * j * P);
  w.hn = (float*)take(16 * NHYP * j * P);
  w.partial = (float*)take(4 * NHYP * j * nb * ICP_NSUM);
  w.flags = (unsigned*)take(4 * NHYP * j * nw);
  w.T = (double*)take(8 * j * 12);
  w.misc = (double*)take(8 * j * MISC);
  w.hyps = (double*)take(8 * NHYP * j * 12);
  w.upd = (double*)take(8 * NHYP * j * 12);
  w.rp = (float*)take(4 * NHYP * j * 12);
  w.hits = (int*)take(4 * NHYP * j);
  w.jobs = (int*)take(4 * j * JOB_INTS);
  w.jf = (int*)take(4 * j * JF_INTS);
  w.bytes = off;
  return w;
}

// ---- rows -> jobs ----------------------------------------------------------------------------------------------------------
// class id = int(roi[1]) as icp_python reads it (truncation); NaN and anything below 1 is background
__device__ __forceinline__ int icpb_decode(const float* __restrict__ roi, int B, int C, int& frame, int& cls)
{
  const float f = roi[0], c = roi[1];
  if (!(c >= 1.f)) return ST_BACKGROUND;
  if (!(c < (float)(C + 1))) return ST_NO_MODEL;
  if (!(f >= 0.f) || !(f < (float)B)) return ST_BACKGROUND;      // no such frame: nothing to refine
  frame = (int)f;
  cls = (int)c;
  return ST_REFINED;
}

__device__ __forceinline__ int icpb_live_rows(const int* __restrict__ count, int R)
{
  return count ? min(max(count[0], 0), R) : R;
}

__global__ __launch_bounds__(256) void icpb_count_kernel(
    const int* __restrict__ labels, const float* __restrict__ rois, int roi_cols, const int* __restrict__ count, int R, int B,
    long long P, int C, int min_pixels, int* __restrict__ info)
{
  __shared__ int red[256];
  const int r = blockIdx.x, t = threadIdx.x;
  int st = ST_DEAD, frame = 0, cls = 0;
  if (r < icpb_live_rows(count, R)) st = icpb_decode(rois + (size_t)r * roi_cols, B, C, frame, cls);
  if (st == ST_REFINED) {          // (uniform over the workgroup)
    const int* lab = labels + (size_t)frame * P;
    int c = 0;
    for (long long p = t; p < P; p += 256) c += lab[p] == cls;
    red[t] = c;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (t < s) red[t] = red[t] + red[t + s];
      __syncthreads();
    }
    if (red[0] < min_pixels) st = ST_FEW_PIXELS;
  }
  if (t == 0) info[(size_t)r * INFO_COLS] = st;
}

__global__ __launch_bounds__(256) void icpb_plan_kernel(
    const float* __restrict__ rois, int roi_cols, int R, int B, int C, const int* __restrict__ v_off, const int* __restrict__ f_off,
    int J, int* __restrict__ jobs, int* __restrict__ info, float* __restrict__ poses_new, float* __restrict__ poses_icp)
{
  __shared__ int s_flag[256];
  __shared__ int s_base;
  const int t = threadIdx.x;
  if (t == 0) s_base = 0;
  for (int j = t; j < J; j += 256)
    for (int k = 0; k < JOB_INTS; k++) jobs[j * JOB_INTS + k] = 0;
  __syncthreads();
  for (int r0 = 0; r0 < R; r0 += 256) {
    const int r = r0 + t;
    const int st = r < R ? info[(size_t)r * INFO_COLS] : ST_DEAD;
    s_flag[t] = st == ST_REFINED;
    __syncthreads();
    int before = s_base;
    for (int k = 0; k < t; k++) before += s_flag[k];
    if (r < R) {
      int out = st;
      if (st == ST_REFINED) {
        if (before < J) {
          int frame = 0, cls = 0;
          icpb_decode(rois + (size_t)r * roi_cols, B, C, frame, cls);
          int* job = jobs + before * JOB_INTS;
          job[0] = r; job[1] = frame; job[2] = cls;
          job[3] = v_off[cls - 1]; job[4] = v_off[cls] - v_off[cls - 1];
          job[5] = f_off[cls - 1]; job[6] = f_off[cls] - f_off[cls - 1];
          job[7] = 1;
        } else {
          out = ST_CAPACITY;
        }
      }
      info[(size_t)r * INFO_COLS] = out;
      for (int k = 1; k < INFO_COLS; k++) info[(size_t)r * INFO_COLS + k] = 0;
      for (int k = 0; k < 7; k++) { poses_new[(size_t)r * 7 + k] = 0.f; poses_icp[(size_t)r * 7 + k] = 0.f; }
    }
    __syncthreads();
    if (t == 255) s_base = before + s_flag[255];
    __syncthreads();
  }
}

// ---- glue: f64, one written order ---------------------------------------------------------------------------------------------
// pose_error.quat2mat + the translation: T 3x4 row-major
__device__ __forceinline__ void glue_pose34(const double* q, double* T)
{
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double n = ((w * w + x * x) + y * y) + z * z;
  if (n < 1e-16) {
    T[0] = 1.0; T[1] = 0.0; T[2] = 0.0; T[4] = 0.0; T[5] = 1.0; T[6] = 0.0; T[8] = 0.0; T[9] = 0.0; T[10] = 1.0;
  } else {
    const double s = 2.0 / n;
    T[0] = 1.0 - s * (y * y + z * z); T[1] = s * (x * y - z * w);       T[2] = s * (x * z + y * w);
    T[4] = s * (x * y + z * w);       T[5] = 1.0 - s * (x * x + z * z); T[6] = s * (y * z - x * w);
    T[8] = s * (x * z - y * w);       T[9] = s * (y * z + x * w);       T[10] = 1.0 - s * (x * x + y * y);
  }
  T[3] = q[4]; T[7] = q[5]; T[11] = q[6];
}

// U o T (Sophus: update * T_co); `out` may not alias an input
__device__ __forceinline__ void glue_compose(const double* U, const double* T, double* out)
{
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out[4 * i + j] = (U[4 * i] * T[j] + U[4 * i + 1] * T[4 + j]) + U[4 * i + 2] * T[8 + j];
    out[4 * i + 3] = ((U[4 * i] * T[3] + U[4 * i + 1] * T[7]) + U[4 * i + 2] * T[11]) + U[4 * i + 3];
  }
}

// icp.mat2quat: unit quaternion wxyz with w >= 0, then the f32 output row (quaternion, translation)
__device__ __forceinline__ void glue_pose_row(const double* T, float* row)
{
  const double R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  double q[4];
  const double tr = (R[0][0] + R[1][1]) + R[2][2];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s;
    q[1] = (R[2][1] - R[1][2]) / s;
    q[2] = (R[0][2] - R[2][0]) / s;
    q[3] = (R[1][0] - R[0][1]) / s;
  } else {
    int i = 0;                                   // first maximum of the diagonal
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const double s = sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0) * 2.0;
    q[1 + i] = 0.25 * s;
    q[0] = (R[k][j] - R[j][k]) / s;
    q[1 + j] = (R[j][i] + R[i][j]) / s;
    q[1 + k] = (R[k][i] + R[i][k]) / s;
  }
  const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int c = 0; c < 4; c++) q[c] = q[c] / nrm;
  if (!(q[0] >= 0.0))
    for (int c = 0; c < 4; c++) q[c] = -q[c];
  for (int c = 0; c < 4; c++) row[c] = (float)q[c];
  row[4] = (float)T[3]; row[5] = (float)T[7]; row[6] = (float)T[11];
}

__global__ __launch_bounds__(64) void icpb_pose_kernel(const int* __restrict__ jobs, int J, const float* __restrict__ poses,
                                                       double* __restrict__ T, double* __restrict__ misc, float* __restrict__ rp)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J || !jobs[j * JOB_INTS + 7]) return;
  const float* row = poses + (size_t)jobs[j * JOB_INTS] * 7;
  double q[7], Tj[12];
  for (int c = 0; c < 7; c++) q[c] = (double)row[c];
  glue_pose34(q, Tj);
  for (int c = 0; c < 12; c++) { T[12 * j + c] = Tj[c]; rp[12 * NHYP * j + c] = (float)Tj[c]; }
  misc[MISC * j] = Tj[11];
}

// synthesize.cpp:2209-2225
__global__ __launch_bounds__(64) void icpb_translate_kernel(const int* __restrict__ jobs, int J, const float* __restrict__ poses,
                                                            int polish_evaluations, double* __restrict__ T,
                                                            double* __restrict__ misc, float* __restrict__ rp, int* __restrict__ jf)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J || !jobs[j * JOB_INTS + 7]) return;
  const double* sums = misc + MISC * j + 1;
  const int agree = (int)sums[3], pairs = (int)sums[4];
  jf[j * JF_INTS] = agree;
  jf[j * JF_INTS + 1] = pairs;
  jf[j * JF_INTS + 2] = agree > 0 && polish_evaluations > 0;
  jf[j * JF_INTS + 3] = 0;
  if (agree > 0) {
    const float* row = poses + (size_t)jobs[j * JOB_INTS] * 7;
    const double Tz = (double)((float)sums[2] / (float)agree);
    const double tx = (double)row[4], ty = (double)row[5], tz = (double)row[6];
    const double rx = tz != 0.0 ? tx / tz : 0.0, ry = tz != 0.0 ? ty / tz : 0.0;
    double* Tj = T + 12 * j;
    Tj[3] = rx * Tz; Tj[7] = ry * Tz; Tj[11] = Tz;
    misc[MISC * j] = Tz;
    for (int c = 0; c < 12; c++) rp[12 * NHYP * j + c] = (float)Tj[c];
  }
}

__constant__ double HYPOTHESIS_DZ[NHYP] = {0.0, -0.02, -0.01, 0.01, 0.02, 0.03, 0.04, 0.05};    // synthesize.cpp:2252-2270

// :2226-2270: the polish's update, the first output row, the 8 depth hypotheses
__global__ __launch_bounds__(64) void icpb_hyps_kernel(const int* __restrict__ jobs, int J, const int* __restrict__ jf,
                                                       double* __restrict__ T, double* __restrict__ misc, double* __restrict__ hyps,
                                                       float* __restrict__ rp, float* __restrict__ poses_new)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J || !jobs[j * JOB_INTS + 7]) return;
  double Tj[12];
  for (int c = 0; c < 12; c++) Tj[c] = T[12 * j + c];
  double Tz = misc[MISC * j];
  if (jf[j * JF_INTS + 2]) {
    double U[12], N[12];
    glue_pose34(misc + MISC * j + 6, U);
    glue_compose(U, Tj, N);
    for (int c = 0; c < 12; c++) { Tj[c] = N[c]; T[12 * j + c] = N[c]; }
    Tz = Tj[11];
    misc[MISC * j] = Tz;
  }
  glue_pose_row(Tj, poses_new + (size_t)jobs[j * JOB_INTS] * 7);
  for (int h = 0; h < NHYP; h++)
    for (int c = 0; c < 12; c++) {
      const double v = c == 11 ? Tz + HYPOTHESIS_DZ[h] : Tj[c];
      hyps[12 * (NHYP * j + h) + c] = v;
      rp[12 * (NHYP * j + h) + c] = (float)v;
    }
}

__global__ __launch_bounds__(64) void icpb_compose_kernel(const int* __restrict__ jobs, int J, const double* __restrict__ upd,
                                                          double* __restrict__ hyps, float* __restrict__ rp)
{
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= NHYP * J || !jobs[(n / NHYP) * JOB_INTS + 7]) return;
  double Tn[12], N[12];
  for (int c = 0; c < 12; c++) Tn[c] = hyps[12 * n + c];
  glue_compose(upd + 12 * n, Tn, N);
  for (int c = 0; c < 12; c++) { hyps[12 * n + c] = N[c]; rp[12 * n + c] = (float)N[c]; }
}

// :2336-2375: first maximum of the scores (hypothesis 0 without pairs), the second output row, the diagnostics
__global__ __launch_bounds__(64) void icpb_output_kernel(const int* __restrict__ jobs, int J, const int* __restrict__ jf,
                                                         const double* __restrict__ hyps, const int* __restrict__ hits,
                                                         float* __restrict__ poses_icp, int* __restrict__ info)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J || !jobs[j * JOB_INTS + 7]) return;
  const int row = jobs[j * JOB_INTS], pairs = jf[j * JF_INTS + 1];
  int* out = info + (size_t)row * INFO_COLS;
  int choose = 0;
  if (pairs > 0)
    for (int h = 1; h < NHYP; h++)
      if (hits[NHYP * j + h] > hits[NHYP * j + choose]) choose = h;
  out[1] = jf[j * JF_INTS];
  out[2] = pairs;
  out[3] = choose;
  for (int h = 0; h < NHYP; h++) out[4 + h] = pairs > 0 ? hits[NHYP * j + h] : -1;
  glue_pose_row(hyps + 12 * (NHYP * j + choose), poses_icp + (size_t)row * 7);
}

// ---- the stages with a job dimension -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void icpb_clear_kernel(unsigned long long* __restrict__ zbuf, long long n)
{
  rd_clear_body(zbuf, n);
}

// grid (face blocks of the largest mesh, np J): pose n = np j + h of job j; only_polish: jobs whose polish runs
__global__ __launch_bounds__(256) void icpb_raster_kernel(
    const int* __restrict__ jobs, const int* __restrict__ jf, int only_polish, int np, const float* __restrict__ vtx,
    const int* __restrict__ faces, const float* __restrict__ rp, const float* __restrict__ intr, int H, int W, float znear,
    float zfar, unsigned long long* __restrict__ zbuf)
{
  const int n = blockIdx.y, j = n / np, h = n % np;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7] || (only_polish && !jf[j * JF_INTS + 2]) || (int)blockIdx.x * 256 >= job[6]) return;
  const float* k = intr + 4 * job[1];
  rd_raster_body(vtx + 3 * (size_t)job[3], faces + 3 * (size_t)job[5], job[6], rp + 12 * (size_t)(NHYP * j + h), H, W, k[0], k[1], k[2],
                 k[3], znear, zfar, zbuf + (size_t)n * H * W);
}

// outputs per pose n; `stride` poses per job in the output maps (8 for the hypothesis maps, 1 for a job's own maps)
__global__ __launch_bounds__(256) void icpb_resolve_kernel(
    const int* __restrict__ jobs, const int* __restrict__ jf, int only_polish, int np, int stride, const float* __restrict__ vtx,
    const float* __restrict__ nrm, const int* __restrict__ faces, const float* __restrict__ rp, const float* __restrict__ intr,
    int H, int W, float znear, int with_model_index, const unsigned long long* __restrict__ zbuf, float* __restrict__ out_v,
    float* __restrict__ out_n, float* __restrict__ out_c)
{
  const int n = blockIdx.y, j = n / np, h = n % np;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7] || (only_polish && !jf[j * JF_INTS + 2])) return;
  const float* k = intr + 4 * job[1];
  const size_t P = (size_t)H * W, o = ((size_t)stride * j + h) * P;
  rd_resolve_body(vtx + 3 * (size_t)job[3], nrm + 3 * (size_t)job[3], faces + 3 * (size_t)job[5], rp + 12 * (size_t)(NHYP * j + h), H, W,
                  k[0], k[1], k[2], k[3], znear, with_model_index ? (float)(job[2] - 1) : 0.f, zbuf + (size_t)n * P,
                  out_v ? out_v + 4 * o : nullptr, out_n ? out_n + 4 * o : nullptr, out_c ? out_c + 3 * o : nullptr);
}

__global__ __launch_bounds__(256) void icpb_backproject_kernel(
    const int* __restrict__ jobs, const uint16_t* __restrict__ depth, const int* __restrict__ labels, const float* __restrict__ intr,
    long long P, int W, float factor, float* __restrict__ live)
{
  const int j = blockIdx.y;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7]) return;
  const float* k = intr + 4 * job[1];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256)
    icp_backproject_pixel(depth + (size_t)job[1] * P, labels + (size_t)job[1] * P, i, W, job[2], factor, k[0], k[1], k[2], k[3],
                          live + 3 * (size_t)j * P);
}

__global__ __launch_bounds__(ICP_BLOCK) void icpb_center_kernel(
    const int* __restrict__ jobs, const int* __restrict__ labels, const float* __restrict__ live, const float* __restrict__ c0,
    const float* __restrict__ v0, const float* __restrict__ n0, long long P, float max_error, unsigned char* __restrict__ mask,
    float* __restrict__ partial, int nblocks)
{
  const int j = blockIdx.y;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7]) return;
  icp_center_body(labels + (size_t)job[1] * P, live + 3 * (size_t)j * P, c0 + 3 * (size_t)j * P, v0 + 4 * (size_t)j * P,
                  n0 + 4 * (size_t)j * P, 4, P, job[2], max_error, mask + (size_t)j * P, partial + (size_t)j * nblocks * ICP_NCEN);
}

__global__ __launch_bounds__(256) void icpb_center_sum_kernel(const int* __restrict__ jobs, const float* __restrict__ partial,
                                                              int nblocks, double* __restrict__ misc)
{
  const int j = blockIdx.x;
  if (!jobs[j * JOB_INTS + 7]) return;
  icp_center_sum_body(partial + (size_t)j * nblocks * ICP_NCEN, nblocks, misc + MISC * j + 1);
}

__global__ __launch_bounds__(NM_LANES) void icpb_polish_kernel(
    const int* __restrict__ jobs, const int* __restrict__ jf, const int* __restrict__ labels, const float* __restrict__ live,
    const float* __restrict__ hv, int H, int W, float znear, float zfar, int maxeval, double* __restrict__ misc)
{
  const int j = blockIdx.x;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7] || !jf[j * JF_INTS + 2]) return;
  const size_t P = (size_t)H * W;
  icp_polish_body(labels + (size_t)job[1] * P, live + 3 * (size_t)j * P, hv + 4 * (size_t)NHYP * j * P, 4, H, W, job[2], znear, zfar,
                  maxeval, misc + MISC * j + 6, misc + MISC * j + 13);
}

__global__ __launch_bounds__(64) void icpb_init_kernel(const int* __restrict__ jobs, double* __restrict__ upd, int N)
{
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < 12 * N && jobs[(i / (12 * NHYP)) * JOB_INTS + 7]) {
    const int e = i % 12;
    upd[i] = (e == 0 || e == 5 || e == 10) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(ICP_BLOCK) void icpb_terms_kernel(
    const int* __restrict__ jobs, const float* __restrict__ live, const float* __restrict__ hv, const float* __restrict__ hn,
    const double* __restrict__ upd, const float* __restrict__ intr, long long P, int H, int W, float znear, float zfar,
    float max_error, float* __restrict__ partial, int nblocks)
{
  const int n = blockIdx.y, j = n / NHYP;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7]) return;
  const float* k = intr + 4 * job[1];
  icp_terms_body(live + 3 * (size_t)j * P, hv + 4 * (size_t)n * P, hn + 4 * (size_t)n * P, upd + 12 * n, P, H, W, 4, k[0], k[1], k[2], k[3],
                 znear, zfar, max_error, partial + ((size_t)n * nblocks + blockIdx.x) * ICP_NSUM);
}

__global__ __launch_bounds__(256) void icpb_solve_kernel(const int* __restrict__ jobs, const float* __restrict__ partial, int nblocks,
                                                         double* __restrict__ upd)
{
  const int n = blockIdx.x;
  if (!jobs[(n / NHYP) * JOB_INTS + 7]) return;
  icp_solve_body(partial + (size_t)n * nblocks * ICP_NSUM, nblocks, upd + 12 * n, nullptr);
}

__global__ __launch_bounds__(256) void icpb_score_kernel(
    const int* __restrict__ jobs, const int* __restrict__ jf, const float* __restrict__ live, const float* __restrict__ c0,
    const unsigned char* __restrict__ mask, int H, int W, const float* __restrict__ rp, const float* __restrict__ intr, float radius,
    unsigned* __restrict__ flags, int nwords, int* __restrict__ hits)
{
  const int n = blockIdx.y, j = n / NHYP;
  const int* job = jobs + j * JOB_INTS;
  if (!job[7] || jf[j * JF_INTS + 1] <= 0) return;
  const float* k = intr + 4 * job[1];
  const size_t P = (size_t)H * W;
  icp_score_body(live + 3 * (size_t)j * P, c0 + 3 * (size_t)j * P, mask + (size_t)j * P, H, W, rp + 12 * (size_t)n, k[0], k[1], k[2], k[3],
                 radius, flags + (size_t)n * nwords, hits + n);
}

}  // namespace

extern "C" int pcnn_icp_batch_workspace_bytes(int max_jobs, int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "icp_batch_workspace_bytes: NULL output");
  PCNN_REQUIRE(max_jobs >= 0 && max_jobs <= 8191 && height >= 1 && width >= 1, PCNN_EINVAL, "icp_batch_workspace_bytes: bad shape");
  *bytes = carve(nullptr, max_jobs, height, width).bytes;
  return PCNN_OK;
}

extern "C" int pcnn_icp_batch_fwd(const int32_t* labels, const uint16_t* depth, const float* intrinsics, int batch, int height,
                                  int width, float factor_depth, const float* rois, int roi_cols, const float* poses,
                                  const int32_t* count, int num_rows, const float* bank_vertices, const float* bank_normals,
                                  const int32_t* bank_faces, const int32_t* bank_vertex_offsets, const int32_t* bank_face_offsets,
                                  int num_classes, int max_faces, int max_jobs, float max_error, int iterations,
                                  int polish_evaluations, int min_pixels, float radius, float z_near, float z_far, float* poses_new,
                                  float* poses_icp, int32_t* info, void* workspace, size_t workspace_bytes, void* stream_)
{
  PCNN_REQUIRE(batch >= 1 && height >= 8 && width >= 8 && num_rows >= 0 && roi_cols >= 2, PCNN_EINVAL,
               "icp_batch: bad shape (B=%d %dx%d, %d rows of %d columns)", batch, height, width, num_rows, roi_cols);
  PCNN_REQUIRE(num_classes >= 0 && max_faces >= 0 && max_jobs >= 0 && max_jobs <= 8191, PCNN_EINVAL,
               "icp_batch: bad bank or capacity (%d classes, %d faces at most, %d jobs)", num_classes, max_faces, max_jobs);
  PCNN_REQUIRE(num_rows <= 65535, PCNN_EINVAL, "icp_batch: at most 65535 rows per call");
  PCNN_REQUIRE(iterations >= 0 && max_error >= 0, PCNN_EINVAL, "icp_batch: iterations and max_error must be non-negative");
  PCNN_REQUIRE(polish_evaluations == 0 || polish_evaluations >= 8, PCNN_EINVAL,
               "icp_batch: the polish's initial simplex alone takes 8 evaluations (got polish_evaluations = %d; 0 skips it)", polish_evaluations);
  PCNN_REQUIRE(factor_depth > 0 && radius > 0 && z_near > 0 && z_far >= z_near, PCNN_EINVAL,
               "icp_batch: factor_depth and radius must be positive, 0 < z_near <= z_far");
  if (num_rows == 0) return PCNN_OK;
  PCNN_REQUIRE(labels && depth && intrinsics && rois && poses && poses_new && poses_icp && info, PCNN_ENULL, "icp_batch: NULL pointer");
  PCNN_REQUIRE(bank_vertex_offsets && bank_face_offsets && (max_faces == 0 || (bank_vertices && bank_normals && bank_faces)), PCNN_ENULL,
               "icp_batch: NULL mesh bank");
  const Ws w = carve(workspace, max_jobs, height, width);
  PCNN_REQUIRE_WORKSPACE("icp_batch", workspace, workspace_bytes, w.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  const int J = max_jobs;
  const long long P = (long long)height * width;
  const int nblocks = (int)((P + ICP_BLOCK - 1) / ICP_BLOCK), nwords = (int)((P + 31) / 32);
  const unsigned pix_blocks = (unsigned)((P + 255) / 256), face_blocks = (unsigned)((max_faces + 255) / 256);
  const dim3 per_job((J + 63) / 64);

  PCNN_LAUNCH(icpb_count_kernel, dim3(num_rows), dim3(256), 0, stream, labels, rois, roi_cols, count, num_rows, batch, P, num_classes,
              min_pixels, info);
  PCNN_LAUNCH(icpb_plan_kernel, dim3(1), dim3(256), 0, stream, rois, roi_cols, num_rows, batch, num_classes, bank_vertex_offsets,
              bank_face_offsets, J, w.jobs, info, poses_new, poses_icp);
  if (J == 0) return check_launch("icp_batch_fwd");

  auto render = [&](int np, int stride, int only_polish, int with_model_index, float* ov, float* on, float* oc) {
    const long long nz = P * np * J;
    PCNN_LAUNCH(icpb_clear_kernel, dim3((unsigned)std::min<long long>((nz + 255) / 256, 8192)), dim3(256), 0, stream, w.zbuf, nz);
    if (face_blocks)
      PCNN_LAUNCH(icpb_raster_kernel, dim3(face_blocks, np * J), dim3(256), 0, stream, w.jobs, w.jf, only_polish, np, bank_vertices,
                  bank_faces, w.rp, intrinsics, height, width, z_near, z_far, w.zbuf);
    PCNN_LAUNCH(icpb_resolve_kernel, dim3(pix_blocks, np * J), dim3(256), 0, stream, w.jobs, w.jf, only_polish, np, stride, bank_vertices,
                bank_normals, bank_faces, w.rp, intrinsics, height, width, z_near, with_model_index, w.zbuf, ov, on, oc);
  };

  PCNN_LAUNCH(icpb_pose_kernel, per_job, dim3(64), 0, stream, w.jobs, J, poses, w.T, w.misc, w.rp);
  render(1, 1, 0, 1, w.v0, w.n0, w.c0);
  PCNN_LAUNCH(icpb_backproject_kernel, dim3(std::min(pix_blocks, 4096u), J), dim3(256), 0, stream, w.jobs, depth, labels, intrinsics, P,
              width, factor_depth, w.live);
  PCNN_LAUNCH(icpb_center_kernel, dim3(nblocks, J), dim3(ICP_BLOCK), 0, stream, w.jobs, labels, w.live, w.c0, w.v0, w.n0, P, max_error,
              w.mask, w.partial, nblocks);
  PCNN_LAUNCH(icpb_center_sum_kernel, dim3(J), dim3(256), 0, stream, w.jobs, w.partial, nblocks, w.misc);
  PCNN_LAUNCH(icpb_translate_kernel, per_job, dim3(64), 0, stream, w.jobs, J, poses, polish_evaluations, w.T, w.misc, w.rp, w.jf);
  if (polish_evaluations > 0) {
    render(1, NHYP, 1, 0, w.hv, nullptr, nullptr);
    PCNN_LAUNCH(icpb_polish_kernel, dim3(J), dim3(NM_LANES), 0, stream, w.jobs, w.jf, labels, w.live, w.hv, height, width, z_near, z_far,
                polish_evaluations, w.misc);
  }
  PCNN_LAUNCH(icpb_hyps_kernel, per_job, dim3(64), 0, stream, w.jobs, J, w.jf, w.T, w.misc, w.hyps, w.rp, poses_new);
  render(NHYP, NHYP, 0, 0, w.hv, w.hn, nullptr);
  PCNN_LAUNCH(icpb_init_kernel, dim3((12 * NHYP * J + 63) / 64), dim3(64), 0, stream, w.jobs, w.upd, NHYP * J);
  for (int it = 0; it < iterations; it++) {
    PCNN_LAUNCH(icpb_terms_kernel, dim3(nblocks, NHYP * J), dim3(ICP_BLOCK), 0, stream, w.jobs, w.live, w.hv, w.hn, w.upd, intrinsics, P,
                height, width, z_near, z_far, max_error, w.partial, nblocks);
    PCNN_LAUNCH(icpb_solve_kernel, dim3(NHYP * J), dim3(256), 0, stream, w.jobs, w.partial, nblocks, w.upd);
  }
  PCNN_LAUNCH(icpb_compose_kernel, dim3((NHYP * J + 63) / 64), dim3(64), 0, stream, w.jobs, J, w.upd, w.hyps, w.rp);
  int st = zero_async(w.flags, sizeof(unsigned) * (size_t)NHYP * J * nwords, stream, "icp_batch");
  if (st == PCNN_OK) st = zero_async(w.hits, sizeof(int) * (size_t)NHYP * J, stream, "icp_batch");
  if (st != PCNN_OK) return st;
  PCNN_LAUNCH(icpb_score_kernel, dim3(pix_blocks, NHYP * J), dim3(256), 0, stream, w.jobs, w.jf, w.live, w.c0, w.mask, height, width, w.rp,
              intrinsics, radius, w.flags, nwords, w.hits);
  PCNN_LAUNCH(icpb_output_kernel, per_job, dim3(64), 0, stream, w.jobs, J, w.jf, w.hyps, w.hits, poses_icp, info);
  return check_launch("icp_batch_fwd");
}
