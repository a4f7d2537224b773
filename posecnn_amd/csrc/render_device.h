// render_device.h — the triangle set-up, edge functions and perspective-correct weights shared by the two rasterisers of this
// library (render.hip: one mesh at many poses; synth_scene.hip: many lit meshes per scene). One definition, so both files
// compute the same coverage, depth and weights bit for bit (the library is built -ffp-contract=off: every expression below
// is one IEEE f32 operation per operator). The conventions are documented at the top of render.hip.
#pragma once

#include "pcnn_device.h"

namespace pcnn {

constexpr unsigned long long RD_EMPTY = ~0ull;

struct RdTri {
  float u[3], v[3], z[3];   // projected vertices and their camera depths
  int flip[3];              // edge i (opposite vertex i) runs from the higher-numbered vertex to the lower one
  int x0, x1, y0, y1;       // clipped bounding box (inclusive); empty when x0 > x1
};

__device__ __forceinline__ void rd_transform(const float* __restrict__ T, const float* __restrict__ p, float* c)
{
  const float x = p[0], y = p[1], z = p[2];
  c[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  c[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  c[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// edge function from a (lower vertex number) to b at (x, y)
__device__ __forceinline__ float rd_edge(float au, float av, float bu, float bv, float x, float y)
{
  return (bu - au) * (y - av) - (bv - av) * (x - au);
}

__device__ __forceinline__ bool rd_setup(const float* __restrict__ T, const float* __restrict__ vtx, const int* __restrict__ face,
                                         int W, int H, float fx, float fy, float px, float py, float znear, RdTri& t, float cam[3][3])
{
  const int i0 = face[0], i1 = face[1], i2 = face[2];
  const int idx[3] = {i0, i1, i2};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    rd_transform(T, vtx + 3 * (size_t)idx[k], cam[k]);
    t.z[k] = cam[k][2];
    t.u[k] = cam[k][0] / cam[k][2] * fx + px;
    t.v[k] = cam[k][1] / cam[k][2] * fy + py;
  }
  t.x0 = 1; t.x1 = 0; t.y0 = 1; t.y1 = 0;
  if (i0 == i1 || i1 == i2 || i0 == i2) return false;
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (!(t.z[k] >= znear) || !(fabsf(t.u[k]) < 1e7f) || !(fabsf(t.v[k]) < 1e7f)) return false;
  t.flip[0] = i1 > i2;
  t.flip[1] = i2 > i0;
  t.flip[2] = i0 > i1;
  const float umin = fminf(fminf(t.u[0], t.u[1]), t.u[2]), umax = fmaxf(fmaxf(t.u[0], t.u[1]), t.u[2]);
  const float vmin = fminf(fminf(t.v[0], t.v[1]), t.v[2]), vmax = fmaxf(fmaxf(t.v[0], t.v[1]), t.v[2]);
  t.x0 = max(0, (int)ceilf(umin));
  t.x1 = min(W - 1, (int)floorf(umax));
  t.y0 = max(0, (int)ceilf(vmin));
  t.y1 = min(H - 1, (int)floorf(vmax));
  return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// screen-space weights of pixel (x, y): e[i] = edge function opposite vertex i; false when the pixel is outside
__device__ __forceinline__ bool rd_weights(const RdTri& t, float x, float y, float* w, float& s)
{
  float e[3];
  // edge 0: vertices 1 -> 2, edge 1: 2 -> 0, edge 2: 0 -> 1
  e[0] = t.flip[0] ? -rd_edge(t.u[2], t.v[2], t.u[1], t.v[1], x, y) : rd_edge(t.u[1], t.v[1], t.u[2], t.v[2], x, y);
  e[1] = t.flip[1] ? -rd_edge(t.u[0], t.v[0], t.u[2], t.v[2], x, y) : rd_edge(t.u[2], t.v[2], t.u[0], t.v[0], x, y);
  e[2] = t.flip[2] ? -rd_edge(t.u[1], t.v[1], t.u[0], t.v[0], x, y) : rd_edge(t.u[0], t.v[0], t.u[1], t.v[1], x, y);
  const bool pos = e[0] >= 0.f && e[1] >= 0.f && e[2] >= 0.f;
  const bool neg = e[0] <= 0.f && e[1] <= 0.f && e[2] <= 0.f;
  if (!(pos || neg)) return false;
  const float area = (e[0] + e[1]) + e[2];
  if (area == 0.f) return false;
  // perspective-correct: weight_i = (e_i / area) / z_i, normalised by their sum
  w[0] = e[0] / area / t.z[0];
  w[1] = e[1] / area / t.z[1];
  w[2] = e[2] / area / t.z[2];
  s = (w[0] + w[1]) + w[2];
  return s > 0.f;
}

// ---- the mesh renderer's kernel bodies (render.hip: one mesh, poses in grid.y; icp_batch.hip: a job table) --------------
constexpr int RD_SMALL = 64;     // bounding boxes up to this many pixels are walked by the triangle's own thread

__device__ __forceinline__ void rd_pixel(const RdTri& t, int x, int y, int W, float znear, float zfar, unsigned tri,
                                         unsigned long long* __restrict__ zbuf)
{
  float w[3], s;
  if (!rd_weights(t, (float)x, (float)y, w, s)) return;
  const float z = ((w[0] * t.z[0] + w[1] * t.z[1]) + w[2] * t.z[2]) / s;
  if (!(z >= znear) || !(z <= zfar)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | tri;
  atomicMin(&zbuf[(size_t)y * W + x], key);
}

// n z-buffer entries to "nothing hit", grid-stride over blockIdx.x
__device__ __forceinline__ void rd_clear_body(unsigned long long* __restrict__ zbuf, long long n)
{
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) zbuf[i] = RD_EMPTY;
}

// One pose T f32 [12] of one mesh into its z-buffer zb [H][W]: block blockIdx.x of 256 faces
__device__ __forceinline__ void rd_raster_body(
    const float* __restrict__ vtx, const int* __restrict__ faces, int nfaces, const float* __restrict__ T, int H, int W,
    float fx, float fy, float px, float py, float znear, float zfar, unsigned long long* __restrict__ zb)
{
  __shared__ RdTri s_big[256];
  __shared__ unsigned s_bigid[256];
  __shared__ int s_nbig;
  const int tid = threadIdx.x;
  const int f = blockIdx.x * 256 + tid;
  if (tid == 0) s_nbig = 0;
  __syncthreads();
  if (f < nfaces) {
    RdTri t;
    float cam[3][3];
    if (rd_setup(T, vtx, faces + 3 * (size_t)f, W, H, fx, fy, px, py, znear, t, cam)) {
      const long long box = (long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1);
      if (box <= RD_SMALL) {
        for (int y = t.y0; y <= t.y1; y++)
          for (int x = t.x0; x <= t.x1; x++) rd_pixel(t, x, y, W, znear, zfar, (unsigned)f, zb);
      } else {
        const int slot = atomicAdd(&s_nbig, 1);
        s_big[slot] = t;
        s_bigid[slot] = (unsigned)f;
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
      rd_pixel(t, x, y, W, znear, zfar, s_bigid[q], zb);
    }
  }
}

// One pose T of one mesh: pixel blockIdx.x * 256 + threadIdx.x of its z-buffer -> its maps (each may be NULL)
__device__ __forceinline__ void rd_resolve_body(
    const float* __restrict__ vtx, const float* __restrict__ nrm, const int* __restrict__ faces, const float* __restrict__ T,
    int H, int W, float fx, float fy, float px, float py, float znear, float canon_x_offset,
    const unsigned long long* __restrict__ zbuf, float* __restrict__ out_v, float* __restrict__ out_n, float* __restrict__ out_c)
{
  const long long P = (long long)H * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const unsigned long long key = zbuf[i];
  const float qnan = __uint_as_float(0x7fc00000u);
  float ov[3] = {qnan, qnan, qnan}, on[3] = {qnan, qnan, qnan}, oc[3] = {qnan, qnan, qnan};
  if (key != RD_EMPTY) {
    const unsigned f = (unsigned)(key & 0xffffffffu);
    const int* face = faces + 3 * (size_t)f;
    RdTri t;
    float cam[3][3], w[3], s;
    rd_setup(T, vtx, face, W, H, fx, fy, px, py, znear, t, cam);
    const int x = (int)(i % W), y = (int)(i / W);
    if (rd_weights(t, (float)x, (float)y, w, s)) {
#pragma unroll
      for (int k = 0; k < 3; k++) ov[k] = ((w[0] * cam[0][k] + w[1] * cam[1][k]) + w[2] * cam[2][k]) / s;
      if (out_n) {
        float vn[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const float* p = nrm + 3 * (size_t)face[j];
          const float a = p[0], b = p[1], c = p[2];
          const float rx = (T[0] * a + T[1] * b) + T[2] * c;
          const float ry = (T[4] * a + T[5] * b) + T[6] * c;
          const float rz = (T[8] * a + T[9] * b) + T[10] * c;
          const float len = sqrt_rn((rx * rx + ry * ry) + rz * rz);
          const bool ok = len > 0.f;      // vertsAndNorms.vert: normalised only when the length is positive
          vn[j][0] = ok ? rx / len : rx;
          vn[j][1] = ok ? ry / len : ry;
          vn[j][2] = ok ? rz / len : rz;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) on[k] = ((w[0] * vn[0][k] + w[1] * vn[1][k]) + w[2] * vn[2][k]) / s;
      }
      if (out_c) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float a0 = vtx[3 * (size_t)face[0] + k] + (k == 0 ? canon_x_offset : 0.f);
          const float a1 = vtx[3 * (size_t)face[1] + k] + (k == 0 ? canon_x_offset : 0.f);
          const float a2 = vtx[3 * (size_t)face[2] + k] + (k == 0 ? canon_x_offset : 0.f);
          oc[k] = ((w[0] * a0 + w[1] * a1) + w[2] * a2) / s;
        }
      }
    }
  }
  const size_t o = (size_t)i;
  if (out_v) { out_v[4 * o] = ov[0]; out_v[4 * o + 1] = ov[1]; out_v[4 * o + 2] = ov[2]; out_v[4 * o + 3] = key != RD_EMPTY ? 1.f : qnan; }
  if (out_n) { out_n[4 * o] = on[0]; out_n[4 * o + 1] = on[1]; out_n[4 * o + 2] = on[2]; out_n[4 * o + 3] = key != RD_EMPTY ? 0.f : qnan; }
  if (out_c) { out_c[3 * o] = oc[0]; out_c[3 * o + 1] = oc[1]; out_c[3 * o + 2] = oc[2]; }
}

}  // namespace pcnn
