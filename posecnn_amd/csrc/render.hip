// render.hip — the predicted maps of the pose-refinement step: what Synthesizer::refinePose / solveICP obtain from
// OpenGL before every ICP call (lib/synthesize/synthesize.cpp:1972-1991, :2104-2136):
//   * renderer_vn_ (df::GLRenderer<VertAndNormalRenderType>, shaders lib/kinect_fusion/shaders/vertsAndNorms.{vert,frag}):
//       texture 0 = camera-frame position of the surface point behind each pixel, texture 1 = the per-vertex normal
//       (rotated into the camera frame and normalised PER VERTEX, then interpolated — not re-normalised per pixel);
//   * renderer_ (CanonicalVertRenderType, shaders canonicalVerts.{vert,frag}): the object-frame ("canonical") vertex,
//       x shifted by the model index (synthesize.cpp:266-271), background = the NaN clear colour (:2113).
// Camera convention: pangolin::ProjectionMatrixRDF_TopLeft(w, h, fx, -fy, px + 0.5, h - (py + 0.5), ...) (:2088) puts
// pixel CENTRES at integer (u, v) of u = fx X / Z + px — the convention of df's Poly3 camera model that the ICP kernel
// projects with — so the sample point of pixel (x, y) is (x, y) itself.
//
// There is no GL on this path. A frame's refinement renders one mesh at 8 hypothesis poses, a few objects per frame
// (synthesize.cpp:2272-2300): small triangles (YCB meshes: 10^4-10^5 faces over ~10^4 pixels), many poses. So:
//   render_raster_kernel   grid (faces / 256, poses): one thread per triangle sets it up (3 vertex transforms,
//                          projection, canonical edge functions) and walks its bounding box when that is small
//                          (<= 64 pixels, the common case); triangles with a larger box are queued in LDS and
//                          walked by the whole workgroup afterwards. Visibility = atomicMin on a 64-bit key
//                          (depth bits << 32 | face index): order-independent, ties broken by the face index,
//                          hence deterministic.
//   render_resolve_kernel  one thread per pixel and pose: re-derives the winning triangle's weights and writes the
//                          perspective-correct attributes (NaN where nothing was hit).
// Watertightness: the edge function of an edge is always evaluated from its lower-numbered vertex to the higher one
// (and negated for the triangle that runs it the other way), so two triangles sharing an edge see the SAME float on
// it; coverage is inclusive on both sides — a pixel exactly on a shared edge is claimed twice and the key decides.
// Triangles with a vertex in front of z_near are dropped, not clipped (objects under refinement lie wholly inside the
// depth range, synthesize.cpp passes z_near = 0.25 m).
//
// GL's own rasterisation (fixed-point snapping, top-left rule, vendor interpolation) is not reproducible bit for bit;
// the CPU checker restates THIS file's arithmetic (same expression trees, all IEEE f32, no contraction) and the tests
// pin both to an analytic ray-caster.
#include <algorithm>

#include "pcnn_device.h"
#include "render_device.h"

// The box size up to which a triangle's own thread walks it, as render_device.h defines it for every kernel that runs
// rd_raster_body: a retune there has to be repeated here (or this file does not compile), and tests/test_thresholds_cpu.py,
// which reads this line, then asks for the cases on either side of it to move.
namespace render_tunables {
constexpr int RD_SMALL = 64;
static_assert(RD_SMALL == pcnn::RD_SMALL, "render.hip restates the tunable of render_device.h");
}  // namespace render_tunables

namespace {

using namespace pcnn;

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* __restrict__ zbuf, long long n)
{
  rd_clear_body(zbuf, n);
}

__global__ __launch_bounds__(256) void render_raster_kernel(
    const float* __restrict__ vtx, const int* __restrict__ faces, int nfaces, const float* __restrict__ poses, int H, int W,
    float fx, float fy, float px, float py, float znear, float zfar, unsigned long long* __restrict__ zbuf)
{
  const int n = blockIdx.y;
  rd_raster_body(vtx, faces, nfaces, poses + 12 * (size_t)n, H, W, fx, fy, px, py, znear, zfar, zbuf + (size_t)n * H * W);
}

__global__ __launch_bounds__(256) void render_resolve_kernel(
    const float* __restrict__ vtx, const float* __restrict__ nrm, const int* __restrict__ faces, const float* __restrict__ poses,
    int H, int W, float fx, float fy, float px, float py, float znear, float canon_x_offset,
    const unsigned long long* __restrict__ zbuf, float* __restrict__ out_v, float* __restrict__ out_n, float* __restrict__ out_c)
{
  const size_t o = (size_t)blockIdx.y * H * W;
  rd_resolve_body(vtx, nrm, faces, poses + 12 * (size_t)blockIdx.y, H, W, fx, fy, px, py, znear, canon_x_offset, zbuf + o,
                  out_v ? out_v + 4 * o : nullptr, out_n ? out_n + 4 * o : nullptr, out_c ? out_c + 3 * o : nullptr);
}

}  // namespace

extern "C" int pcnn_render_mesh_workspace_bytes(int num_poses, int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "render_mesh_workspace_bytes: NULL output");
  PCNN_REQUIRE(num_poses >= 0 && height >= 1 && width >= 1, PCNN_EINVAL, "render_mesh_workspace_bytes: bad shape");
  *bytes = sizeof(unsigned long long) * (size_t)num_poses * height * width;
  return PCNN_OK;
}

extern "C" int pcnn_render_mesh_fwd(const float* vertices, const float* normals, const int32_t* faces, int num_vertices,
                                    int num_faces, const float* poses, int num_poses, int height, int width, float fx,
                                    float fy, float px, float py, float z_near, float z_far, float canon_x_offset,
                                    float* out_vertices, float* out_normals, float* out_canonical, void* workspace,
                                    size_t workspace_bytes, void* stream_)
{
  PCNN_REQUIRE(num_poses >= 0 && height >= 1 && width >= 1 && num_vertices >= 0 && num_faces >= 0, PCNN_EINVAL,
               "render_mesh: bad shape (%d poses, %dx%d, %d vertices, %d faces)", num_poses, height, width, num_vertices, num_faces);
  PCNN_REQUIRE(num_poses <= 65535, PCNN_EINVAL, "render_mesh: at most 65535 poses per call");
  PCNN_REQUIRE(z_near > 0 && z_far >= z_near && fx != 0 && fy != 0, PCNN_EINVAL, "render_mesh: need 0 < z_near <= z_far and non-zero focal lengths");
  if (num_poses == 0) return PCNN_OK;
  PCNN_REQUIRE(poses && workspace && (num_faces == 0 || (vertices && faces)), PCNN_ENULL, "render_mesh: NULL pointer");
  PCNN_REQUIRE(!out_normals || normals || num_faces == 0, PCNN_ENULL, "render_mesh: a normal map needs per-vertex normals");
  const size_t need = sizeof(unsigned long long) * (size_t)num_poses * height * width;
  PCNN_REQUIRE(workspace_bytes >= need, PCNN_EWORKSPACE, "render_mesh: workspace too small (%zu < %zu)", workspace_bytes, need);
  PCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, PCNN_EINVAL, "render_mesh: workspace must be 8-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  unsigned long long* zbuf = static_cast<unsigned long long*>(workspace);
  const long long P = (long long)height * width;
  const long long nz = P * num_poses;
  PCNN_LAUNCH(render_clear_kernel, dim3((unsigned)std::min<long long>((nz + 255) / 256, 8192)), dim3(256), 0, stream, zbuf, nz);
  if (num_faces > 0)
    PCNN_LAUNCH(render_raster_kernel, dim3((num_faces + 255) / 256, num_poses), dim3(256), 0, stream, vertices, faces, num_faces,
                poses, height, width, fx, fy, px, py, z_near, z_far, zbuf);
  PCNN_LAUNCH(render_resolve_kernel, dim3((unsigned)((P + 255) / 256), num_poses), dim3(256), 0, stream, vertices, normals, faces,
              poses, height, width, fx, fy, px, py, z_near, canon_x_offset, zbuf, out_vertices, out_normals, out_canonical);
  return check_launch("render_mesh_fwd");
}
