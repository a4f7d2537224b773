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

}  // namespace pcnn
