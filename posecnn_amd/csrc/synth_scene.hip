// synth_scene.hip — synthetic training scenes: what the reference's render thread (tools/train_net.py:155-258) obtains from
// Synthesizer::render (lib/synthesize/synthesize.cpp:345-609, OpenGL) and lib/gt_synthesize_layer/minibatch.py:113-154
// pastes a background under: S scenes of several lit, coloured or textured meshes each, rendered in one launch sequence
// into a BGRA colour frame, a uint16 depth frame, a label map, an object-frame vertex map, the pixel count of every
// instance and the scene's `valid` flag (the 800-pixel rule of train_net.py:220-228). Declared in
// include/posecnn_hip_synth.h, which documents the arguments.
//
// Geometry is render.hip's, from the same header (render_device.h): the same vertex transform and projection with pixel
// centres at integer (u, v), lower-to-higher edge functions, inclusive coverage, triangles with a vertex in front of z_near
// dropped (not clipped), depth kept inside [z_near, z_far], perspective-correct weights. Visibility across the objects of a
// scene: one 64-bit depth buffer per scene, atomicMin on (depth bits << 32) | (slot << 27 | face) — a tie goes to the lower
// slot, then to the lower face; order-independent, hence deterministic.
//
// Shading is ApplyLight of lib/kinect_fusion/shaders/canonicalVertsAndColor.frag / canonicalVertsAndTexture.frag:27-57,71-83
// with one point light given in the camera frame, attenuation 0.01, ambient coefficient 0.5, white specular colour
// (glRender.h:246).
//
// What is NOT the reference's bits, and cannot be:
//   1. GL's rasteriser and its texture filter are fixed-point and vendor-defined;
//   2. GLSL `pow` has no specified bits;
//   3. the shader rotates the INTERPOLATED object-frame normal, this file interpolates normals that were rotated and
//      normalised per vertex (as render.hip's out_normals) and normalises the result per pixel.
// So this file defines the arithmetic, and tests/synth_ref.py restates it in numpy byte for byte: all IEEE f32 with one
// rounding per operation (-ffp-contract=off), dot products summed left to right, correctly rounded divide and square root
// (pcnn_device.h), the specular power taken with an INTEGER shininess by left-to-right binary powering (a fixed sequence of
// f32 multiplies). Also not reproduced: the reference carries the depth through gl_FragCoord.z and back
// (train_net.py:203-205) before `.astype(np.uint16)` (:257); here depth = trunc(min(65535, factor_depth * z)) of the f32
// camera depth z that won the depth test.
//
//   per pixel with a hit (w0..w2, s: the weights of render_device.h; A_j: attribute of the triangle's vertex j)
//     interp(A)  = ((w0 A_0 + w1 A_1) + w2 A_2) / s
//     pos        = interp(camera-frame vertex)          vertmap = interp(object-frame vertex)
//     n          = interp(R normal_j, normalised per vertex when its length is > 0); n /= |n| when |n| > 0
//     colour     = interp(vertex colour RGB) | bilinear texture sample at interp(uv) | (1, 1, 1) without either
//     d = light - pos; dist = |d|; L = d / dist (dist > 0); att = 1 / (1 + 0.01 (dist dist))
//     V = -pos / |pos| (|pos| > 0);  diff = max(0, n.L);  spec = 0
//     if diff > 0:  I = -L;  r = I - (2 (n.I)) n;  spec = powi(max(0, V.r), shininess)
//     lin_k = (0.5 colour_k) I_light + att ((diff colour_k) I_light + spec I_light)
//     byte_k = trunc(min(max(255 lin_k, 0), 255))       stored B, G, R, 255
//   texture sample (h x w texels, RGB uint8): fu = u w - 0.5, fv = (1 - v) h - 0.5, both clamped to [-1, size];
//     x0 = floor(fu), ax = fu - x0, x1 = x0 + 1, indices clamped to the edge; texel / 255;
//     (t00 (1 - ax) + t10 ax) (1 - ay) + (t01 (1 - ax) + t11 ax) ay
//
// Launch sequence (nothing synchronises with the host, allocates or reads a count back):
//   synth_upload_kernel   the few host tables (one 96-byte row per instance, scene ranges, lights) travel as kernel
//                         ARGUMENTS, 3840 bytes per launch, and are stored to the workspace — no host staging buffer whose
//                         lifetime would have to outlast the call, and safe under stream capture;
//   synth_clear_kernel    depth buffers (8 bytes per pixel and scene) and pixel_counts;
//   synth_raster_kernel   a flat list of (instance, 256-face chunk): workgroup b finds its instance by bisection of the
//                         rows' chunk prefix, so no workgroup is empty whatever the mix of mesh sizes. One thread per
//                         triangle walks a bounding box of up to 64 pixels; larger ones are queued in LDS and walked by the
//                         workgroup;
//   synth_resolve_kernel  one thread per pixel: re-derives the winner's weights, shades, composites, writes every output
//                         once; pixel_counts by integer atomics, one per wave and slot present (ballot + popcount);
//   synth_valid_kernel    one thread per scene.
#include <algorithm>
#include <string.h>

#include "pcnn_device.h"
#include "render_device.h"
#include "../../include/posecnn_hip_synth.h"

namespace {

using namespace pcnn;

constexpr int SY_ROW = 24;            // words of an instance row
constexpr int SY_SMALL = 64;          // bounding boxes up to this many pixels are walked by the triangle's own thread (as render.hip)
constexpr int SY_SLOT_SHIFT = 27;
constexpr unsigned SY_FACE_MASK = (1u << SY_SLOT_SHIFT) - 1u;
constexpr int SY_BLOB_WORDS = 960;    // 3840 bytes of kernel arguments per upload launch

// instance row (32-bit words): the instance's scene, slot and class, the first chunk of its faces in the flat work list, its
// mesh's ranges in the pooled arrays, its texture, shininess and pose
enum { R_SCENE = 0, R_SLOT, R_CLS, R_CHUNK, R_VOFF, R_NV, R_FOFF, R_NF, R_TOFF, R_TH, R_TW, R_SHIN, R_POSE };

struct SyBlob { uint32_t w[SY_BLOB_WORDS]; };

__global__ __launch_bounds__(256) void synth_upload_kernel(SyBlob blob, uint32_t* __restrict__ dst, int nwords)
{
  for (int i = threadIdx.x; i < nwords; i += 256) dst[i] = blob.w[i];
}

__global__ __launch_bounds__(256) void synth_clear_kernel(unsigned long long* __restrict__ zbuf, long long n,
                                                          int* __restrict__ counts, int ncounts)
{
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  for (long long i = t0; i < n; i += step) zbuf[i] = RD_EMPTY;
  for (long long i = t0; i < ncounts; i += step) counts[i] = 0;
}

__device__ __forceinline__ bool sy_face_ok(const int* __restrict__ face, int nv)
{
  return (unsigned)face[0] < (unsigned)nv && (unsigned)face[1] < (unsigned)nv && (unsigned)face[2] < (unsigned)nv;
}

__device__ __forceinline__ void sy_pixel(const RdTri& t, int x, int y, int W, float znear, float zfar, unsigned low,
                                         unsigned long long* __restrict__ zbuf)
{
  float w[3], s;
  if (!rd_weights(t, (float)x, (float)y, w, s)) return;
  const float z = ((w[0] * t.z[0] + w[1] * t.z[1]) + w[2] * t.z[2]) / s;
  if (!(z >= znear) || !(z <= zfar)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | low;
  atomicMin(&zbuf[(size_t)y * W + x], key);
}

__global__ __launch_bounds__(256) void synth_raster_kernel(
    const float* __restrict__ vtx, const int* __restrict__ faces, const int* __restrict__ rows, int ninst, int H, int W,
    float fx, float fy, float px, float py, float znear, float zfar, unsigned long long* __restrict__ zbuf)
{
  __shared__ RdTri s_big[256];
  __shared__ unsigned s_bigid[256];
  __shared__ int s_nbig;
  const int tid = threadIdx.x;
  if (tid == 0) s_nbig = 0;
  __syncthreads();
  // the last instance whose first chunk is <= this workgroup's (instances without faces share their successor's)
  const int b = (int)blockIdx.x;
  int lo = 0, hi = ninst - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[SY_ROW * mid + R_CHUNK] <= b) lo = mid; else hi = mid - 1;
  }
  const int* row = rows + SY_ROW * lo;
  const int f = (b - row[R_CHUNK]) * 256 + tid;
  const int nf = row[R_NF], nv = row[R_NV];
  const float* T = reinterpret_cast<const float*>(row + R_POSE);
  const float* v0 = vtx + 3 * (size_t)row[R_VOFF];
  const unsigned slotbits = (unsigned)row[R_SLOT] << SY_SLOT_SHIFT;
  unsigned long long* zb = zbuf + (size_t)row[R_SCENE] * H * W;
  if (f < nf) {
    const int* face = faces + 3 * ((size_t)row[R_FOFF] + f);
    RdTri t;
    float cam[3][3];
    if (sy_face_ok(face, nv) && rd_setup(T, v0, face, W, H, fx, fy, px, py, znear, t, cam)) {
      const long long box = (long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1);
      if (box <= SY_SMALL) {
        for (int y = t.y0; y <= t.y1; y++)
          for (int x = t.x0; x <= t.x1; x++) sy_pixel(t, x, y, W, znear, zfar, slotbits | (unsigned)f, zb);
      } else {
        const int q = atomicAdd(&s_nbig, 1);
        s_big[q] = t;
        s_bigid[q] = slotbits | (unsigned)f;
      }
    }
  }
  __syncthreads();
  const int nbig = s_nbig;
  for (int q = 0; q < nbig; q++) {
    const RdTri& t = s_big[q];
    const int bw = t.x1 - t.x0 + 1;
    const long long box = (long long)bw * (t.y1 - t.y0 + 1);
    for (long long i = tid; i < box; i += 256) {
      const int y = t.y0 + (int)(i / bw), x = t.x0 + (int)(i % bw);
      sy_pixel(t, x, y, W, znear, zfar, s_bigid[q], zb);
    }
  }
}

__device__ __forceinline__ float sy_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void sy_normalize(float* a)
{
  const float len = sqrt_rn(sy_dot(a, a));
  if (len > 0.f) { a[0] = a[0] / len; a[1] = a[1] / len; a[2] = a[2] / len; }
}

// x^n, n >= 1: left-to-right binary powering
__device__ __forceinline__ float sy_powi(float x, int n)
{
  float r = x;
  for (int bit = 30 - __clz(n); bit >= 0; bit--) {
    r = r * r;
    if ((n >> bit) & 1) r = r * x;
  }
  return r;
}

__device__ __forceinline__ float sy_texel(const uint8_t* __restrict__ tex, int tw, int x, int y, int k)
{
  return (float)tex[3 * ((size_t)y * tw + x) + k] / 255.f;
}

__device__ __forceinline__ uint8_t sy_byte(float lin)
{
  return (uint8_t)(int)fminf(fmaxf(255.f * lin, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void synth_resolve_kernel(
    const float* __restrict__ vtx, const float* __restrict__ nrm, const float* __restrict__ colors, const float* __restrict__ uvs,
    const int* __restrict__ faces, const uint8_t* __restrict__ textures, const int* __restrict__ rows,
    const int* __restrict__ scene_first, const float* __restrict__ lights, const uint8_t* __restrict__ background, int H, int W,
    float fx, float fy, float px, float py, float znear, float factor_depth, const unsigned long long* __restrict__ zbuf,
    uint8_t* __restrict__ color, uint16_t* __restrict__ depth, int* __restrict__ label, float* __restrict__ vertmap,
    int* __restrict__ counts)
{
  const long long P = (long long)H * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int sc = blockIdx.y;
  const bool live = i < P;
  const int first = scene_first[sc];
  int slot = -1;
  if (live) {
    const size_t o = (size_t)sc * P + i;
    const unsigned long long key = zbuf[o];
    int lab = 0;
    unsigned dep = 0;
    float obj[3] = {0.f, 0.f, 0.f};
    uint8_t bgra[4] = {0, 0, 0, 0};
    if (background) { bgra[0] = background[3 * o]; bgra[1] = background[3 * o + 1]; bgra[2] = background[3 * o + 2]; }
    if (key != RD_EMPTY) {
      const unsigned low = (unsigned)(key & 0xffffffffu);
      const int sl = (int)(low >> SY_SLOT_SHIFT);
      const int* row = rows + SY_ROW * (size_t)(first + sl);
      const int* face = faces + 3 * ((size_t)row[R_FOFF] + (low & SY_FACE_MASK));
      const float* T = reinterpret_cast<const float*>(row + R_POSE);
      const size_t voff = (size_t)row[R_VOFF];
      const float* v0 = vtx + 3 * voff;
      RdTri t;
      float cam[3][3], w[3], s;
      rd_setup(T, v0, face, W, H, fx, fy, px, py, znear, t, cam);
      const int x = (int)(i % W), y = (int)(i / W);
      if (rd_weights(t, (float)x, (float)y, w, s)) {
        slot = sl;
        lab = row[R_CLS];
        const float z = __uint_as_float((unsigned)(key >> 32));
        dep = (unsigned)(int)fminf(65535.f, factor_depth * z);
        float pos[3], n[3], col[3] = {1.f, 1.f, 1.f};
#pragma unroll
        for (int k = 0; k < 3; k++) {
          pos[k] = ((w[0] * cam[0][k] + w[1] * cam[1][k]) + w[2] * cam[2][k]) / s;
          obj[k] = ((w[0] * v0[3 * (size_t)face[0] + k] + w[1] * v0[3 * (size_t)face[1] + k]) + w[2] * v0[3 * (size_t)face[2] + k]) / s;
        }
        float vn[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const float* p = nrm + 3 * (voff + face[j]);
          const float a = p[0], b = p[1], c = p[2];
          vn[j][0] = (T[0] * a + T[1] * b) + T[2] * c;
          vn[j][1] = (T[4] * a + T[5] * b) + T[6] * c;
          vn[j][2] = (T[8] * a + T[9] * b) + T[10] * c;
          sy_normalize(vn[j]);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = ((w[0] * vn[0][k] + w[1] * vn[1][k]) + w[2] * vn[2][k]) / s;
        sy_normalize(n);
        const int tw = row[R_TW], th = row[R_TH];
        if (tw > 0) {
          float uv[2];
#pragma unroll
          for (int k = 0; k < 2; k++)
            uv[k] = ((w[0] * uvs[2 * (voff + face[0]) + k] + w[1] * uvs[2 * (voff + face[1]) + k]) + w[2] * uvs[2 * (voff + face[2]) + k]) / s;
          const float fu = fminf(fmaxf(uv[0] * (float)tw - 0.5f, -1.f), (float)tw);
          const float fv = fminf(fmaxf((1.f - uv[1]) * (float)th - 0.5f, -1.f), (float)th);
          const float xf = floorf(fu), yf = floorf(fv);
          const float ax = fu - xf, ay = fv - yf;
          const int x0 = min(max((int)xf, 0), tw - 1), x1 = min(max((int)xf + 1, 0), tw - 1);
          const int y0 = min(max((int)yf, 0), th - 1), y1 = min(max((int)yf + 1, 0), th - 1);
          const uint8_t* tex = textures + (size_t)row[R_TOFF];
          const float bx = 1.f - ax, by = 1.f - ay;
#pragma unroll
          for (int k = 0; k < 3; k++)
            col[k] = (sy_texel(tex, tw, x0, y0, k) * bx + sy_texel(tex, tw, x1, y0, k) * ax) * by +
                     (sy_texel(tex, tw, x0, y1, k) * bx + sy_texel(tex, tw, x1, y1, k) * ax) * ay;
        } else if (colors) {
#pragma unroll
          for (int k = 0; k < 3; k++)
            col[k] = ((w[0] * colors[3 * (voff + face[0]) + k] + w[1] * colors[3 * (voff + face[1]) + k]) + w[2] * colors[3 * (voff + face[2]) + k]) / s;
        }
        const float* lt = lights + 4 * (size_t)sc;
        const float li = lt[3];
        float L[3] = {lt[0] - pos[0], lt[1] - pos[1], lt[2] - pos[2]};
        const float dist = sqrt_rn(sy_dot(L, L));
        if (dist > 0.f) { L[0] = L[0] / dist; L[1] = L[1] / dist; L[2] = L[2] / dist; }
        const float att = 1.f / (1.f + 0.01f * (dist * dist));
        float V[3] = {-pos[0], -pos[1], -pos[2]};
        sy_normalize(V);
        const float diff = fmaxf(0.f, sy_dot(n, L));
        float spec = 0.f;
        if (diff > 0.f) {
          const float I[3] = {-L[0], -L[1], -L[2]};
          const float two = 2.f * sy_dot(n, I);
          const float r[3] = {I[0] - two * n[0], I[1] - two * n[1], I[2] - two * n[2]};
          spec = sy_powi(fmaxf(0.f, sy_dot(V, r)), row[R_SHIN]);
        }
        const float sp = spec * li;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float lin = (0.5f * col[k]) * li + att * ((diff * col[k]) * li + sp);
          bgra[2 - k] = sy_byte(lin);
        }
        bgra[3] = 255;
      }
    }
    label[o] = lab;
    depth[o] = (uint16_t)dep;
    reinterpret_cast<uint32_t*>(color)[o] = (uint32_t)bgra[0] | ((uint32_t)bgra[1] << 8) | ((uint32_t)bgra[2] << 16) | ((uint32_t)bgra[3] << 24);
    if (vertmap) { vertmap[3 * o] = obj[0]; vertmap[3 * o + 1] = obj[1]; vertmap[3 * o + 2] = obj[2]; }
  }
  // pixel_counts: one integer atomic per wave and slot present in it (every lane of the wave takes part in the ballots)
  unsigned long long todo = __ballot(slot >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int s0 = __shfl(slot, leader);
    const unsigned long long same = __ballot(slot == s0);
    if (lane_id() == leader) atomicAdd(&counts[first + s0], __popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(64) void synth_valid_kernel(const int* __restrict__ scene_first, const int* __restrict__ counts,
                                                         int num_scenes, int min_pixels, int* __restrict__ valid)
{
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= num_scenes) return;
  int ok = 1;
  for (int i = scene_first[s]; i < scene_first[s + 1]; i++) ok &= counts[i] >= min_pixels;
  valid[s] = ok;
}

// the host tables reach the workspace as kernel arguments, SY_BLOB_WORDS at a time
struct Uploader {
  SyBlob blob;
  uint32_t* dst;
  int fill = 0;
  hipStream_t stream;
  void flush()
  {
    if (!fill) return;
    PCNN_LAUNCH(synth_upload_kernel, dim3(1), dim3(256), 0, stream, blob, dst, fill);
    dst += fill;
    fill = 0;
  }
  void put(const void* words, int n)
  {
    const uint32_t* p = static_cast<const uint32_t*>(words);
    while (n > 0) {
      const int take = std::min(n, SY_BLOB_WORDS - fill);
      memcpy(blob.w + fill, p, 4 * (size_t)take);
      fill += take; p += take; n -= take;
      if (fill == SY_BLOB_WORDS) flush();
    }
  }
};

size_t zbuf_bytes(int S, int H, int W) { return align_up(sizeof(unsigned long long) * (size_t)S * H * W, 16); }
size_t rows_bytes(int S) { return (size_t)PCNN_SYNTH_MAX_INSTANCES * S * SY_ROW * 4; }
size_t first_bytes(int S) { return align_up(4 * ((size_t)S + 1), 16); }

}  // namespace

extern "C" int pcnn_synth_scene_workspace_bytes(int num_scenes, int height, int width, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "synth_scene_workspace_bytes: NULL output");
  PCNN_REQUIRE(num_scenes >= 0 && num_scenes <= 65535 && height >= 1 && width >= 1, PCNN_EINVAL, "synth_scene_workspace_bytes: bad shape");
  *bytes = zbuf_bytes(num_scenes, height, width) + rows_bytes(num_scenes) + first_bytes(num_scenes) + 16 * (size_t)num_scenes;
  return PCNN_OK;
}

extern "C" int pcnn_synth_scene_fwd(const float* vertices, const float* normals, const float* colors, const float* uvs,
                                    const int32_t* faces, int num_vertices, int num_faces, const int32_t* mesh_table,
                                    int num_meshes, const uint8_t* textures, size_t texture_bytes, const int32_t* texture_table,
                                    const int32_t* instance_ids, const float* instance_params, int num_instances,
                                    const float* lights, const uint8_t* background, int num_scenes, int height, int width,
                                    float fx, float fy, float px, float py, float z_near, float z_far, float factor_depth,
                                    int min_pixels, uint8_t* color, uint16_t* depth, int32_t* label, float* vertmap,
                                    int32_t* pixel_counts, int32_t* valid, void* workspace, size_t workspace_bytes, void* stream_)
{
  const int S = num_scenes, N = num_instances;
  PCNN_REQUIRE(S >= 0 && S <= 65535 && N >= 0 && height >= 1 && width >= 1 && num_vertices >= 0 && num_faces >= 0 && num_meshes >= 0,
               PCNN_EINVAL, "synth_scene: bad shape (%d scenes, %d instances, %dx%d, %d vertices, %d faces, %d meshes)", S, N, height,
               width, num_vertices, num_faces, num_meshes);
  PCNN_REQUIRE(z_near > 0 && z_far >= z_near && fx != 0 && fy != 0, PCNN_EINVAL, "synth_scene: need 0 < z_near <= z_far and non-zero focal lengths");
  PCNN_REQUIRE(factor_depth > 0, PCNN_EINVAL, "synth_scene: factor_depth must be positive");
  PCNN_REQUIRE(texture_bytes < ((size_t)1 << 31), PCNN_EINVAL, "synth_scene: at most 2^31 - 1 bytes of pooled textures");
  PCNN_REQUIRE((long long)N <= (long long)PCNN_SYNTH_MAX_INSTANCES * S, PCNN_EINVAL, "synth_scene: %d instances in %d scenes (at most %d per scene)", N, S, PCNN_SYNTH_MAX_INSTANCES);
  if (S == 0) return PCNN_OK;
  PCNN_REQUIRE(color && depth && label && valid && workspace && lights, PCNN_ENULL, "synth_scene: NULL pointer");
  PCNN_REQUIRE(N == 0 || (instance_ids && instance_params && pixel_counts && mesh_table), PCNN_ENULL, "synth_scene: NULL instance or mesh table");
  PCNN_REQUIRE(num_faces == 0 || (vertices && normals && faces), PCNN_ENULL, "synth_scene: NULL vertices / normals / faces");
  // ---- the tables, on the host, before the device is touched ----
  for (int m = 0; m < num_meshes && N > 0; m++) {
    const int32_t* mt = mesh_table + 4 * (size_t)m;
    PCNN_REQUIRE(mt[0] >= 0 && mt[1] >= 0 && (long long)mt[0] + mt[1] <= num_vertices && mt[2] >= 0 && mt[3] >= 0 && (long long)mt[2] + mt[3] <= num_faces,
                 PCNN_EINVAL, "synth_scene: mesh %d lies outside the pooled arrays", m);
    PCNN_REQUIRE(mt[3] <= (1 << SY_SLOT_SHIFT), PCNN_EINVAL, "synth_scene: mesh %d has %d faces (at most 2^27)", m, mt[3]);
    if (texture_table) {
      const int32_t* tt = texture_table + 3 * (size_t)m;
      PCNN_REQUIRE(tt[2] >= 0 && (tt[2] == 0 || (tt[0] >= 0 && tt[1] >= 1 && (unsigned long long)tt[0] + 3ull * tt[1] * tt[2] <= texture_bytes)),
                   PCNN_EINVAL, "synth_scene: the texture of mesh %d lies outside the pooled textures", m);
      PCNN_REQUIRE(tt[2] == 0 || (uvs && textures), PCNN_ENULL, "synth_scene: mesh %d is textured but uvs / textures is NULL", m);
    }
  }
  long long chunks = 0;
  int prev_scene = 0, in_scene = 0;
  for (int i = 0; i < N; i++) {
    const int32_t* id = instance_ids + 3 * (size_t)i;
    PCNN_REQUIRE(id[0] >= 0 && id[0] < S, PCNN_EINVAL, "synth_scene: instance %d names scene %d of %d", i, id[0], S);
    PCNN_REQUIRE(id[0] >= prev_scene, PCNN_EINVAL, "synth_scene: instances must be sorted by scene (instance %d)", i);
    in_scene = id[0] == prev_scene ? in_scene + 1 : 1;
    prev_scene = id[0];
    PCNN_REQUIRE(in_scene <= PCNN_SYNTH_MAX_INSTANCES, PCNN_EINVAL, "synth_scene: scene %d has more than %d instances", id[0], PCNN_SYNTH_MAX_INSTANCES);
    PCNN_REQUIRE(id[1] >= 0 && id[1] < num_meshes, PCNN_EINVAL, "synth_scene: instance %d names mesh %d of %d", i, id[1], num_meshes);
    PCNN_REQUIRE(id[2] >= 1 && id[2] < PCNN_MAX_CLASSES, PCNN_EINVAL, "synth_scene: instance %d has class id %d (1..%d)", i, id[2], PCNN_MAX_CLASSES - 1);
    const float sh = instance_params[13 * (size_t)i + 12];
    PCNN_REQUIRE(sh >= 1.f && sh <= 255.f && sh == (float)(int)sh, PCNN_EINVAL, "synth_scene: instance %d: shininess must be an integer 1..255", i);
    chunks += (mesh_table[4 * (size_t)id[1] + 3] + 255) / 256;
  }
  PCNN_REQUIRE(chunks <= 0x7fffffffLL, PCNN_EINVAL, "synth_scene: too many faces in one call");
  size_t need = 0;
  pcnn_synth_scene_workspace_bytes(S, height, width, &need);
  PCNN_REQUIRE(workspace_bytes >= need, PCNN_EWORKSPACE, "synth_scene: workspace too small (%zu < %zu)", workspace_bytes, need);
  PCNN_REQUIRE(aligned16(workspace), PCNN_EINVAL, "synth_scene: workspace must be 16-byte aligned");

  hipStream_t stream = (hipStream_t)stream_;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(ws);
  int* d_rows = reinterpret_cast<int*>(ws + zbuf_bytes(S, height, width));
  int* d_first = reinterpret_cast<int*>(reinterpret_cast<char*>(d_rows) + rows_bytes(S));
  float* d_lights = reinterpret_cast<float*>(reinterpret_cast<char*>(d_first) + first_bytes(S));

  Uploader up;
  up.stream = stream;
  up.dst = reinterpret_cast<uint32_t*>(d_rows);
  long long chunk = 0;
  for (int i = 0, slot = 0; i < N; i++) {
    const int32_t* id = instance_ids + 3 * (size_t)i;
    const float* prm = instance_params + 13 * (size_t)i;
    const int32_t* mt = mesh_table + 4 * (size_t)id[1];
    slot = (i > 0 && id[0] == instance_ids[3 * (size_t)(i - 1)]) ? slot + 1 : 0;
    int32_t row[SY_ROW];
    row[R_SCENE] = id[0]; row[R_SLOT] = slot; row[R_CLS] = id[2]; row[R_CHUNK] = (int32_t)chunk;
    row[R_VOFF] = mt[0]; row[R_NV] = mt[1]; row[R_FOFF] = mt[2]; row[R_NF] = mt[3];
    row[R_TOFF] = row[R_TH] = row[R_TW] = 0;
    if (texture_table && texture_table[3 * (size_t)id[1] + 2] > 0) {
      row[R_TOFF] = texture_table[3 * (size_t)id[1]]; row[R_TH] = texture_table[3 * (size_t)id[1] + 1]; row[R_TW] = texture_table[3 * (size_t)id[1] + 2];
    }
    row[R_SHIN] = (int)prm[12];
    memcpy(row + R_POSE, prm, 48);
    up.put(row, SY_ROW);
    chunk += (mt[3] + 255) / 256;
  }
  up.flush();
  up.dst = reinterpret_cast<uint32_t*>(d_first);
  for (int s = 0, i = 0; s <= S; s++) {      // scene_first[s] = the first instance of scene s; [S] = N
    while (s < S && i < N && instance_ids[3 * (size_t)i] < s) i++;
    const int32_t v = s < S ? i : N;
    up.put(&v, 1);
  }
  up.flush();
  up.dst = reinterpret_cast<uint32_t*>(d_lights);
  up.put(lights, 4 * S);
  up.flush();

  const long long P = (long long)height * width;
  const long long nz = P * S;
  PCNN_LAUNCH(synth_clear_kernel, dim3((unsigned)std::min<long long>((nz + 255) / 256, 8192)), dim3(256), 0, stream, zbuf, nz, pixel_counts, N);
  if (chunks > 0)
    PCNN_LAUNCH(synth_raster_kernel, dim3((unsigned)chunks), dim3(256), 0, stream, vertices, faces, d_rows, N, height, width, fx, fy, px,
                py, z_near, z_far, zbuf);
  PCNN_LAUNCH(synth_resolve_kernel, dim3((unsigned)((P + 255) / 256), S), dim3(256), 0, stream, vertices, normals, colors, uvs, faces,
              textures, d_rows, d_first, d_lights, background, height, width, fx, fy, px, py, z_near, factor_depth, zbuf, color, depth,
              label, vertmap, pixel_counts);
  PCNN_LAUNCH(synth_valid_kernel, dim3((S + 63) / 64), dim3(64), 0, stream, d_first, pixel_counts, S, min_pixels, valid);
  return check_launch("synth_scene_fwd");
}
