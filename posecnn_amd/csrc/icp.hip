// icp.hip — depth-based pose refinement, first slice: the projective point-to-plane ICP core
// behind Synthesizer::refinePose / solveICP (lib/synthesize/synthesize.cpp:2020-2026, :2052-2380; called from
// lib/fcn/test.py:1925-1933), i.e. df::icp (lib/kinect_fusion/src/optimization/icp.cpp:20-106) with its per-pixel
// kernel (src/optimization/icp.cu:25-136) and the masked depth -> vertex map step (synthesize.cpp:2139-2155 +
// src/image/backprojection.cu:10-27), plus the two host-side steps of solveICP around the iterations — the translation
// estimate (synthesize.cpp:2157-2225) and the SegICP scoring of the refined hypotheses (:2302-2343, PCL kd-tree in the
// reference) — as kernels. The predicted maps come from csrc/render.hip (OpenGL in the reference); the nlopt polish
// (poseWithOpt) is not reproduced.
//
// The reference runs, per iteration and per object: one kernel writing a 28-byte Jacobian/residual record for EVERY
// pixel of the frame (8.6 MB), cudaDeviceSynchronize, a thrust::transform_reduce over all of them, a second
// synchronise, a 6x6 solve on the host, and an H2D of the new pose — 8 to 50 times per object.
// Here an iteration is two launches and nothing leaves the device until the last one is done:
//   icp_terms_kernel   one thread per pixel of the predicted maps, all N objects of a frame in one grid (grid.y);
//                      the 29 sums a pixel contributes to (21 J^T J, 6 J^T r, inlier count, sum r^2) are reduced
//                      in LDS by a halving tree per 256-pixel block (blocks without a single contributing pixel —
//                      ~95 % of a frame — skip the tree) into one partial row per block;
//   icp_solve_kernel   one workgroup per object: partial rows added in f64 in a fixed order (8 segments x 29 columns),
//                      LDL^T solve, update = exp(solution), accumulated = update * accumulated — all in f64 by lane 0;
//                      the state stays in the workspace, the next iteration's terms kernel reads it from there.
// Arithmetic follows the canonical statement the CPU checker implements as well (same expression trees, same reduction
// order, sin/cos replaced by fixed Taylor polynomials), so the result is bit-identical to it (tests/test_gpu_icp.py).
// The device bodies live in icp_device.h (icp_batch.hip runs the same ones with a job dimension); the kernels below hand
// each workgroup its problem from the kernel arguments.
#include <algorithm>

#include "icp_device.h"
#include "pcnn_device.h"

// The tunables the edge cases of tests/icp_cases.py are built around, as icp_device.h defines them for every kernel that
// runs its bodies: a retune there has to be repeated here (or this file does not compile), and tests/test_icp_edges_cpu.py,
// which reads these lines, then asks for the cases to move with it.
namespace icp_tunables {
constexpr int ICP_BLOCK = 256, ICP_NSEG = 8, ICP_CH = 8, NM_LANES = 1024;
static_assert(ICP_BLOCK == pcnn::ICP_BLOCK && ICP_NSEG == pcnn::ICP_NSEG && ICP_CH == pcnn::ICP_CH && NM_LANES == pcnn::NM_LANES,
              "icp.hip restates the tunables of icp_device.h");
}  // namespace icp_tunables

namespace {

using namespace pcnn;

__global__ __launch_bounds__(256) void icp_backproject_kernel(
    const uint16_t* __restrict__ depth, const int* __restrict__ label, long long P, int W, int obj_id, float factor,
    float fx, float fy, float px, float py, float* __restrict__ vertex_map)
{
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256)
    icp_backproject_pixel(depth, label, i, W, obj_id, factor, fx, fy, px, py, vertex_map);
}

__global__ __launch_bounds__(64) void icp_init_kernel(double* __restrict__ state, int N)
{
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < 12 * N) {
    const int e = i % 12;
    state[i] = (e == 0 || e == 5 || e == 10) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_terms_kernel(
    const float* __restrict__ live, const float* __restrict__ pred_v, const float* __restrict__ pred_n,
    const double* __restrict__ state, long long P, int H, int W, int pc, float fx, float fy, float px, float py,
    float znear, float zfar, float max_error, float* __restrict__ partial, int nblocks)
{
  const int n = blockIdx.y;
  icp_terms_body(live + (long long)n * P * 3, pred_v + (long long)n * P * pc, pred_n + (long long)n * P * pc, state + 12 * n, P, H, W,
                 pc, fx, fy, px, py, znear, zfar, max_error, partial + ((long long)n * nblocks + blockIdx.x) * ICP_NSUM);
}

__global__ __launch_bounds__(256) void icp_solve_kernel(
    const float* __restrict__ partial, int nblocks, double* __restrict__ state, float* __restrict__ stats, int it, int iterations)
{
  const int n = blockIdx.x;
  icp_solve_body(partial + (long long)n * nblocks * ICP_NSUM, nblocks, state + 12 * n,
                 stats ? stats + ((long long)n * iterations + it) * 2 : nullptr);
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_center_kernel(
    const int* __restrict__ label, const float* __restrict__ live, const float* __restrict__ canon,
    const float* __restrict__ pred_v, const float* __restrict__ pred_n, int pc, long long P, int obj_id, float max_error,
    unsigned char* __restrict__ mask, float* __restrict__ partial)
{
  icp_center_body(label, live, canon, pred_v, pred_n, pc, P, obj_id, max_error, mask, partial);
}

__global__ __launch_bounds__(256) void icp_center_sum_kernel(const float* __restrict__ partial, int nblocks, double* __restrict__ sums)
{
  icp_center_sum_body(partial, nblocks, sums);
}

__global__ __launch_bounds__(256) void icp_score_kernel(
    const float* __restrict__ live, const float* __restrict__ canon, const unsigned char* __restrict__ mask, int H, int W,
    const float* __restrict__ hyps, float fx, float fy, float px, float py, float radius, unsigned* __restrict__ flags,
    int nwords, int* __restrict__ hits)
{
  const int m = blockIdx.y;
  icp_score_body(live, canon, mask, H, W, hyps + 12 * (size_t)m, fx, fy, px, py, radius, flags + (size_t)m * nwords, hits + m);
}

__global__ __launch_bounds__(NM_LANES) void icp_polish_kernel(
    const int* __restrict__ label, const float* __restrict__ live, const float* __restrict__ pred_v, int pc, int H, int W,
    int obj, float znear, float zfar, int maxeval, double* __restrict__ x_out, double* __restrict__ info)
{
  icp_polish_body(label, live, pred_v, pc, H, W, obj, znear, zfar, maxeval, x_out, info);
}

}  // namespace

extern "C" int pcnn_icp_backproject_fwd(const uint16_t* depth, const int32_t* label, int height, int width, int obj_id,
                                        float factor_depth, float fx, float fy, float px, float py, float* vertex_map,
                                        void* stream_)
{
  PCNN_REQUIRE(height >= 1 && width >= 1, PCNN_EINVAL, "icp_backproject: bad shape %dx%d", height, width);
  PCNN_REQUIRE(factor_depth > 0 && fx != 0 && fy != 0, PCNN_EINVAL, "icp_backproject: factor_depth must be positive, focal lengths non-zero");
  PCNN_REQUIRE(depth && vertex_map, PCNN_ENULL, "icp_backproject: NULL pointer");
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)height * width;
  const unsigned grid = (unsigned)std::min<long long>((P + 255) / 256, 4096);
  PCNN_LAUNCH(icp_backproject_kernel, dim3(grid), dim3(256), 0, stream, depth, label, P, width, obj_id, factor_depth, fx, fy, px, py, vertex_map);
  return check_launch("icp_backproject_fwd");
}

extern "C" int pcnn_icp_refine_workspace_bytes(int num_objects, int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "icp_refine_workspace_bytes: NULL output");
  PCNN_REQUIRE(num_objects >= 0 && height >= 1 && width >= 1, PCNN_EINVAL, "icp_refine_workspace_bytes: bad shape");
  *bytes = icp_ws_bytes(num_objects, height, width);
  return PCNN_OK;
}

extern "C" int pcnn_icp_refine_fwd(const float* live_vertices, const float* pred_vertices, const float* pred_normals,
                                   int num_objects, int height, int width, int pred_channels, float fx, float fy, float px,
                                   float py, float z_near, float z_far, float max_error, int iterations, double* update,
                                   float* stats, void* workspace, size_t workspace_bytes, void* stream_)
{
  PCNN_REQUIRE(num_objects >= 0 && height >= 8 && width >= 8, PCNN_EINVAL, "icp_refine: bad shape N=%d %dx%d", num_objects, height, width);
  PCNN_REQUIRE(pred_channels == 3 || pred_channels == 4, PCNN_EINVAL, "icp_refine: predicted maps carry 3 or 4 floats per pixel (got %d)", pred_channels);
  PCNN_REQUIRE(iterations >= 0 && max_error >= 0, PCNN_EINVAL, "icp_refine: iterations and max_error must be non-negative");
  PCNN_REQUIRE(num_objects <= 65535, PCNN_EINVAL, "icp_refine: at most 65535 objects per call");
  if (num_objects == 0) return PCNN_OK;
  PCNN_REQUIRE(live_vertices && pred_vertices && pred_normals && update, PCNN_ENULL, "icp_refine: NULL pointer");
  PCNN_REQUIRE(workspace && workspace_bytes >= icp_ws_bytes(num_objects, height, width), PCNN_EWORKSPACE,
               "icp_refine: workspace too small (%zu < %zu)", workspace_bytes, icp_ws_bytes(num_objects, height, width));
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)height * width;
  const int nblocks = (int)((P + ICP_BLOCK - 1) / ICP_BLOCK);
  float* partial = static_cast<float*>(workspace);
  PCNN_LAUNCH(icp_init_kernel, dim3((12 * num_objects + 63) / 64), dim3(64), 0, stream, update, num_objects);
  for (int it = 0; it < iterations; it++) {
    PCNN_LAUNCH(icp_terms_kernel, dim3(nblocks, num_objects), dim3(ICP_BLOCK), 0, stream, live_vertices, pred_vertices, pred_normals,
                update, P, height, width, pred_channels, fx, fy, px, py, z_near, z_far, max_error, partial, nblocks);
    PCNN_LAUNCH(icp_solve_kernel, dim3(num_objects), dim3(256), 0, stream, partial, nblocks, update, stats, it, iterations);
  }
  return check_launch("icp_refine_fwd");
}

extern "C" int pcnn_icp_center_workspace_bytes(int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "icp_center_workspace_bytes: NULL output");
  PCNN_REQUIRE(height >= 1 && width >= 1, PCNN_EINVAL, "icp_center_workspace_bytes: bad shape");
  *bytes = align_up(sizeof(float) * (size_t)(((long long)height * width + ICP_BLOCK - 1) / ICP_BLOCK) * ICP_NCEN, 256);
  return PCNN_OK;
}

extern "C" int pcnn_icp_center_fwd(const int32_t* label, const float* live_vertices, const float* canonical,
                                   const float* pred_vertices, const float* pred_normals, int pred_channels, int height,
                                   int width, int obj_id, float max_error, double* sums, uint8_t* mask, void* workspace,
                                   size_t workspace_bytes, void* stream_)
{
  PCNN_REQUIRE(height >= 1 && width >= 1, PCNN_EINVAL, "icp_center: bad shape %dx%d", height, width);
  PCNN_REQUIRE(pred_channels == 3 || pred_channels == 4, PCNN_EINVAL, "icp_center: predicted maps carry 3 or 4 floats per pixel (got %d)", pred_channels);
  PCNN_REQUIRE(label && live_vertices && canonical && pred_vertices && pred_normals && sums && mask && workspace, PCNN_ENULL, "icp_center: NULL pointer");
  size_t need = 0;
  pcnn_icp_center_workspace_bytes(height, width, &need);
  PCNN_REQUIRE(workspace_bytes >= need, PCNN_EWORKSPACE, "icp_center: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)height * width;
  const int nblocks = (int)((P + ICP_BLOCK - 1) / ICP_BLOCK);
  float* partial = static_cast<float*>(workspace);
  PCNN_LAUNCH(icp_center_kernel, dim3(nblocks), dim3(ICP_BLOCK), 0, stream, label, live_vertices, canonical, pred_vertices,
              pred_normals, pred_channels, P, obj_id, max_error, mask, partial);
  PCNN_LAUNCH(icp_center_sum_kernel, dim3(1), dim3(256), 0, stream, partial, nblocks, sums);
  return check_launch("icp_center_fwd");
}

extern "C" int pcnn_icp_score_workspace_bytes(int num_hypotheses, int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "icp_score_workspace_bytes: NULL output");
  PCNN_REQUIRE(num_hypotheses >= 0 && height >= 1 && width >= 1, PCNN_EINVAL, "icp_score_workspace_bytes: bad shape");
  *bytes = sizeof(unsigned) * (size_t)num_hypotheses * (size_t)(((long long)height * width + 31) / 32);
  return PCNN_OK;
}

extern "C" int pcnn_icp_score_fwd(const float* live_vertices, const float* canonical, const uint8_t* mask, int height, int width,
                                  const float* hypotheses, int num_hypotheses, float fx, float fy, float px, float py,
                                  float radius, int32_t* hits, void* workspace, size_t workspace_bytes, void* stream_)
{
  PCNN_REQUIRE(height >= 1 && width >= 1 && num_hypotheses >= 0, PCNN_EINVAL, "icp_score: bad shape %dx%d, %d hypotheses", height, width, num_hypotheses);
  PCNN_REQUIRE(num_hypotheses <= 65535, PCNN_EINVAL, "icp_score: at most 65535 hypotheses per call");
  PCNN_REQUIRE(radius > 0 && fx != 0 && fy != 0, PCNN_EINVAL, "icp_score: radius must be positive, focal lengths non-zero");
  if (num_hypotheses == 0) return PCNN_OK;
  PCNN_REQUIRE(live_vertices && canonical && mask && hypotheses && hits && workspace, PCNN_ENULL, "icp_score: NULL pointer");
  size_t need = 0;
  pcnn_icp_score_workspace_bytes(num_hypotheses, height, width, &need);
  PCNN_REQUIRE(workspace_bytes >= need, PCNN_EWORKSPACE, "icp_score: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t stream = (hipStream_t)stream_;
  const long long P = (long long)height * width;
  const int nwords = (int)((P + 31) / 32);
  int st = zero_async(workspace, need, stream, "icp_score");
  if (st == PCNN_OK) st = zero_async(hits, sizeof(int32_t) * (size_t)num_hypotheses, stream, "icp_score");
  if (st != PCNN_OK) return st;
  PCNN_LAUNCH(icp_score_kernel, dim3((unsigned)((P + 255) / 256), num_hypotheses), dim3(256), 0, stream, live_vertices, canonical, mask,
              height, width, hypotheses, fx, fy, px, py, radius, static_cast<unsigned*>(workspace), nwords, hits);
  return check_launch("icp_score_fwd");
}

extern "C" int pcnn_icp_polish_fwd(const int32_t* label, const float* live_vertices, const float* pred_vertices, int pred_channels,
                                   int height, int width, int obj_id, float z_near, float z_far, int max_evaluations, double* update,
                                   double* info, void* stream_)
{
  PCNN_REQUIRE(height >= 1 && width >= 1, PCNN_EINVAL, "icp_polish: bad shape %dx%d", height, width);
  PCNN_REQUIRE(pred_channels == 3 || pred_channels == 4, PCNN_EINVAL, "icp_polish: predicted maps carry 3 or 4 floats per pixel (got %d)", pred_channels);
  PCNN_REQUIRE(max_evaluations >= 8, PCNN_EINVAL, "icp_polish: the initial simplex alone takes 8 evaluations (got max_evaluations = %d)", max_evaluations);
  PCNN_REQUIRE(label && live_vertices && pred_vertices && update && info, PCNN_ENULL, "icp_polish: NULL pointer");
  hipStream_t stream = (hipStream_t)stream_;
  PCNN_LAUNCH(icp_polish_kernel, dim3(1), dim3(NM_LANES), 0, stream, label, live_vertices, pred_vertices, pred_channels, height, width,
              obj_id, z_near, z_far, max_evaluations, update, info);
  return check_launch("icp_polish_fwd");
}
