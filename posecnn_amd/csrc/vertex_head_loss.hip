// vertex_head_loss.hip — the training twin of the fused vertex head: smooth_l1_loss_vertex (lib/fcn/train.py:564-573) and its
// backward straight from the 1/stride-resolution field z [B,H,W,3C], the label map and the object table
// (include/posecnn_hip_vertex_loss.h). The unfused route materialises vertex_pred = deconv(z) + bias [B,H s,W s,3C], runs
// the loss over it, writes a gradient of the same size and gathers it back to z's resolution; only 3 of a foreground
// pixel's 3C channels ever carry weight, so here neither tensor exists:
//
//   forward    sl1_gt_partial_kernel (sl1_gt_device.h) with its pred[i] load replaced by the interpolation: same order,
//              same bits as pcnn_smooth_l1_vertex_gt_fwd on the materialised tensor
//   backward   vertex_head_bwd_kernel: a workgroup owns a tile of cells of one frame. Phase 1, one footprint pixel per
//              thread: label -> row -> interpolated triple -> gradient triple + class, left in LDS. Phase 2, one work item
//              per (cell, class present in the footprint): the k x k gather of pcnn_deconv_bilinear_bwd out of LDS,
//              taking only the pixels of its class (the others would add +-0: the header has the argument); classes
//              absent from the footprint are written as zeros without a walk. dbias: f64 partials of the tile's own pixels
//              in a fixed order, then channel_partials_final_kernel (reduce_device.h). No floating-point atomics.
//
// Measured times and what bounds them (reasoning, no counters): DESIGN.md §3.6v.
#include "sl1_gt_device.h"

#include "../../include/posecnn_hip_vertex_loss.h"
#include "bilinear.h"

namespace {

constexpr int VH_THREADS = 256;
constexpr int VH_MAX_OBJECTS = 64;   // rows of a frame's table, as vertex_targets.hip
constexpr int VH_FOOTPRINT = 3072;   // pixels of a tile's footprint kept in LDS (13 bytes each)

// element (f, y, x, ch) of deconv(z) + bias, the bits of deconv_bilinear_kernel (bilinear.h)
struct PredLowres {
  const float* z;
  const float* bias;
  int H, W, C3, k, s;
  __device__ __forceinline__ float operator()(long long, int f, int y, int x, int ch) const
  {
    const int pad = (k - s) / 2;
    const Taps ty = make_taps(y, k, s, pad, H);
    const Taps tx = make_taps(x, k, s, pad, W);
    return bilinear_at(z + (size_t)f * H * W * C3, ty, tx, W, C3, ch) + bias[ch];
  }
};

// grid: one workgroup per tile, numbered (b * tiles_y + tile_y) * tiles_x + tile_x. Dynamic LDS: gx, gy, gz [FP] floats
// and cl [FP] bytes, FP = fph * fpw the footprint of th x tw cells.
__global__ __launch_bounds__(VH_THREADS) void vertex_head_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ bias, const int32_t* __restrict__ label,
    const int32_t* __restrict__ instance, const float* __restrict__ objects, const float* __restrict__ sums,
    const float* __restrict__ upstream, int H, int W, int C, int M, int k, int s, float sigma2, int th, int tw, int tiles_y,
    int tiles_x, float* __restrict__ dz, double* __restrict__ part)
{
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float tab[VH_MAX_OBJECTS * 6];
  __shared__ float s_tap[64];
  __shared__ double s_row[3 * 64];
  __shared__ unsigned long long s_mask;
  __shared__ int s_list[PCNN_MAX_CLASSES];
  __shared__ int s_np;
  const int t = threadIdx.x;
  const int C3 = 3 * C;
  const int pad = (k - s) / 2;
  const int Ho = H * s, Wo = W * s;
  const int fph = th * s + k - s, fpw = tw * s + k - s, FP = fph * fpw;
  float* gx = smem;
  float* gy = gx + FP;
  float* gz = gy + FP;
  unsigned char* cl = reinterpret_cast<unsigned char*>(gz + FP);
  const int blk = blockIdx.x;
  const int b = blk / (tiles_x * tiles_y);
  const int i0 = ((blk / tiles_x) % tiles_y) * th, j0 = (blk % tiles_x) * tw;
  const int nth = min(th, H - i0), ntw = min(tw, W - j0);
  const int oy0 = s * i0 - pad, ox0 = s * j0 - pad;   // the footprint's first pixel; may lie outside the image
  for (int q = t; q < 6 * M; q += VH_THREADS) tab[q] = objects[(long long)b * M * 6 + q];
  if (t < k) s_tap[t] = bilinear_tap(t, k);
  if (t == 0) s_mask = 0ull;
  __syncthreads();

  // ---- phase 1: one footprint pixel per thread
  {
    const float denom = sums[2] + 1e-10f;
    const float up = upstream ? upstream[0] : 1.0f;
    const float* zb = z + (size_t)b * H * W * C3;
    const int uh = nth * s + k - s, uw = ntw * s + k - s;   // the part of the footprint this tile's cells reach
    for (int p = t; p < FP; p += VH_THREADS) {
      const int ly = p / fpw, lx = p - ly * fpw;
      const int y = oy0 + ly, x = ox0 + lx;
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
      int cls = 0;
      if (ly < uh && lx < uw && y >= 0 && y < Ho && x >= 0 && x < Wo) {
        const long long pix = ((long long)b * Ho + y) * Wo + x;
        const int l = label[pix];
        if (l > 0 && l < C) {
          const int inst = instance ? instance[pix] : 0;
          float tx, ty, tz, w;
          if (vt_match(tab, M, l, inst, x, y, tx, ty, tz, w)) {
            const Taps Ty = make_taps_tab(y, k, s, pad, H, s_tap);
            const Taps Tx = make_taps_tab(x, k, s, pad, W, s_tap);
            float p0, p1, p2, il, dp;
            bilinear_at3(zb, Ty, Tx, W, C3, 3 * l, p0, p1, p2);
            sl1_elem(p0 + bias[3 * l], tx, w, sigma2, il, dp);
            g0 = div_rn(dp, denom) * up;
            sl1_elem(p1 + bias[3 * l + 1], ty, w, sigma2, il, dp);
            g1 = div_rn(dp, denom) * up;
            sl1_elem(p2 + bias[3 * l + 2], tz, w, sigma2, il, dp);
            g2 = div_rn(dp, denom) * up;
            cls = l;
            atomicOr(&s_mask, 1ull << l);
          }
        }
      }
      gx[p] = g0;
      gy[p] = g1;
      gz[p] = g2;
      cl[p] = (unsigned char)cls;
    }
  }
  __syncthreads();
  const unsigned long long mask = s_mask;
  if (t == 0) {
    int n = 0;
    for (int l = 1; l < C; ++l)
      if ((mask >> l) & 1ull) s_list[n++] = l;
    s_np = n;
  }
  __syncthreads();
  const int np = s_np;
  const int ncell = nth * ntw;

  // ---- phase 2a: the channels of classes nobody in the footprint carries
  for (int idx = t; idx < ncell * C; idx += VH_THREADS) {
    const int cell = idx / C, l = idx - cell * C;
    if (!((mask >> l) & 1ull)) {
      const int ci = cell / ntw, cj = cell - ci * ntw;
      float* o = dz + (((size_t)b * H + i0 + ci) * W + j0 + cj) * C3 + 3 * l;
      o[0] = 0.f;
      o[1] = 0.f;
      o[2] = 0.f;
    }
  }
  // ---- phase 2b: (cell, present class): output rows ascending, output columns ascending, acc = acc + (wy * wx) * g
  for (int idx = t; idx < ncell * np; idx += VH_THREADS) {
    const int q = idx / ncell, cell = idx - q * ncell;
    const int l = s_list[q];
    const int ci = cell / ntw, cj = cell - ci * ntw;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int ty = 0; ty < k; ++ty) {
      const int ly = s * ci + ty;
      if (oy0 + ly < 0 || oy0 + ly >= Ho) continue;
      const float wy = s_tap[ty];
      for (int tx = 0; tx < k; ++tx) {
        const int lx = s * cj + tx;
        if (ox0 + lx < 0 || ox0 + lx >= Wo) continue;
        const int p = ly * fpw + lx;
        if (cl[p] == l) {
          const float w = wy * s_tap[tx];
          a0 = a0 + w * gx[p];
          a1 = a1 + w * gy[p];
          a2 = a2 + w * gz[p];
        }
      }
    }
    float* o = dz + (((size_t)b * H + i0 + ci) * W + j0 + cj) * C3 + 3 * l;
    o[0] = a0;
    o[1] = a1;
    o[2] = a2;
  }

  // ---- dbias partials of the tile's own pixels (footprint rows / columns pad .. pad + n s - 1): rows ascending in x, then
  //      the row sums ascending in y
  const size_t nblk = gridDim.x;
  const int nr = nth * s, nc = ntw * s;   // nr <= 64 for every tile shape the host picks
  for (int q = 0; q < np; ++q) {
    const int l = s_list[q];
    if (t < 3 * nr) {
      const int d = t / nr, r = t - d * nr;
      const float* g = d == 0 ? gx : (d == 1 ? gy : gz);
      const int p0 = (pad + r) * fpw + pad;
      double a = 0.0;
      for (int c = 0; c < nc; ++c)
        if (cl[p0 + c] == l) a = a + (double)g[p0 + c];
      s_row[t] = a;
    }
    __syncthreads();
    if (t < 3) {
      double a = 0.0;
      for (int r = 0; r < nr; ++r) a = a + s_row[t * nr + r];
      part[(size_t)(3 * l + t) * nblk + blk] = a;
    }
    __syncthreads();
  }
  for (int c = t; c < C3; c += VH_THREADS)
    if (!((mask >> (c / 3)) & 1ull)) part[(size_t)c * nblk + blk] = 0.0;
}

struct Plan {
  int th, tw, tiles_y, tiles_x;
  long long pixels, blocks;
  size_t shmem, ws_bytes;
};

int make_plan(const char* who, int B, int H, int W, int C, int M, int k, int s, Plan* p)
{
  PCNN_REQUIRE(s >= 1 && k >= s && k <= 2 * s && k <= 64 && (k - s) % 2 == 0, PCNN_EINVAL,
               "%s: need stride >= 1, stride <= kernel <= min(2*stride, 64) and (kernel - stride) even (got kernel=%d stride=%d)",
               who, k, s);
  // the shape limits of the target-free loss entries (vt_check_shape, vertex_targets.hip) on the full-resolution map
  PCNN_REQUIRE(B >= 0 && H >= 0 && W >= 0, PCNN_EINVAL, "%s: negative size", who);
  PCNN_REQUIRE(C >= 2 && C <= PCNN_MAX_CLASSES, PCNN_EINVAL, "%s: 2 <= num_classes <= %d", who, PCNN_MAX_CLASSES);
  PCNN_REQUIRE(M >= 0 && M <= VH_MAX_OBJECTS, PCNN_EINVAL, "%s: 0 <= num_objects <= %d", who, VH_MAX_OBJECTS);
  PCNN_REQUIRE(B <= 65535, PCNN_EINVAL, "%s: batch > 65535", who);
  PCNN_REQUIRE(H <= (1 << 30) / s && W <= (1 << 30) / s, PCNN_EINVAL, "%s: more than 2^30 pixels", who);
  p->pixels = (long long)B * (H * s) * (W * s);
  PCNN_REQUIRE(p->pixels <= (1ll << 30), PCNN_EINVAL, "%s: more than 2^30 pixels", who);   // pixel indices are ints
  static const int ladder[6][2] = {{4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}};
  p->th = 1;
  p->tw = 1;
  for (int i = 0; i < 6; ++i)
    if ((ladder[i][0] * s + k - s) * (ladder[i][1] * s + k - s) <= VH_FOOTPRINT) {
      p->th = ladder[i][0];
      p->tw = ladder[i][1];
      break;
    }
  p->tiles_y = (H + p->th - 1) / p->th;
  p->tiles_x = (W + p->tw - 1) / p->tw;
  p->blocks = (long long)B * p->tiles_y * p->tiles_x;
  const size_t fp = (size_t)(p->th * s + k - s) * (size_t)(p->tw * s + k - s);   // <= 64 * 64
  p->shmem = align_up(fp * 13, 16);
  const size_t bwd = sizeof(double) * (size_t)p->blocks * 3 * (size_t)C, fwd = sizeof(float) * 2 * SL1_BLOCKS;
  p->ws_bytes = bwd > fwd ? bwd : fwd;
  return PCNN_OK;
}

}  // namespace

extern "C" int pcnn_vertex_head_loss_workspace_bytes(int B, int H, int W, int C, int k, int s, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "vertex_head_loss_workspace_bytes: NULL bytes");
  Plan p;
  if (int st = make_plan("vertex_head_loss_workspace_bytes", B, H, W, C, 0, k, s, &p)) return st;
  *bytes = p.ws_bytes;
  return PCNN_OK;
}

extern "C" int pcnn_vertex_head_loss_fwd(const float* z, const float* bias, const int32_t* label, const int32_t* instance,
                                         const float* objects, int B, int H, int W, int C, int M, int k, int s, float sigma,
                                         float* out, void* workspace, size_t workspace_bytes, void* stream_)
{
  const char* who = "vertex_head_loss_fwd";
  Plan p;
  if (int st = make_plan(who, B, H, W, C, M, k, s, &p)) return st;
  PCNN_REQUIRE(sigma > 0.f, PCNN_EINVAL, "%s: sigma must be positive", who);
  PCNN_REQUIRE(out, PCNN_ENULL, "%s: NULL out", who);
  PCNN_REQUIRE(bias, PCNN_ENULL, "%s: NULL bias", who);
  if (p.pixels > 0) {
    PCNN_REQUIRE(z, PCNN_ENULL, "%s: NULL z", who);
    PCNN_REQUIRE(label, PCNN_ENULL, "%s: NULL label", who);
    PCNN_REQUIRE(objects || M == 0, PCNN_ENULL, "%s: NULL objects", who);
  }
  PCNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, p.ws_bytes);
  hipStream_t stream = (hipStream_t)stream_;
  float* partial = (float*)workspace;
  const int C3 = 3 * C, stride = SL1_BLOCKS * 256;
  const PredLowres pred{z, bias, H, W, C3, k, s};
  PCNN_LAUNCH(sl1_gt_partial_kernel<PredLowres>, dim3(SL1_BLOCKS), dim3(256), 0, stream, pred, label, instance, objects,
              p.pixels * C3, H * s * W * s, W * s, C, M, sigma * sigma, stride / C3, stride % C3, partial);
  PCNN_LAUNCH(sl1_final_kernel, dim3(1), dim3(SL1_BLOCKS / 2), 0, stream, partial, out);
  return check_launch(who);
}

extern "C" int pcnn_vertex_head_loss_bwd(const float* z, const float* bias, const int32_t* label, const int32_t* instance,
                                         const float* objects, const float* out, const float* upstream, int B, int H, int W,
                                         int C, int M, int k, int s, float sigma, float* dz, float* dbias, void* workspace,
                                         size_t workspace_bytes, void* stream_)
{
  const char* who = "vertex_head_loss_bwd";
  Plan p;
  if (int st = make_plan(who, B, H, W, C, M, k, s, &p)) return st;
  PCNN_REQUIRE(sigma > 0.f, PCNN_EINVAL, "%s: sigma must be positive", who);
  PCNN_REQUIRE(dbias, PCNN_ENULL, "%s: NULL dbias", who);
  PCNN_REQUIRE(bias, PCNN_ENULL, "%s: NULL bias", who);
  if (p.pixels > 0) {
    PCNN_REQUIRE(z, PCNN_ENULL, "%s: NULL z", who);
    PCNN_REQUIRE(label, PCNN_ENULL, "%s: NULL label", who);
    PCNN_REQUIRE(objects || M == 0, PCNN_ENULL, "%s: NULL objects", who);
    PCNN_REQUIRE(out, PCNN_ENULL, "%s: NULL out", who);
    PCNN_REQUIRE(dz, PCNN_ENULL, "%s: NULL dz", who);
    PCNN_REQUIRE(aligned16(dz), PCNN_EINVAL, "%s: dz must be 16-byte aligned", who);
  }
  PCNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, p.ws_bytes);
  PCNN_REQUIRE(p.blocks < (1ll << 31), PCNN_EINVAL, "%s: grid too large", who);
  hipStream_t stream = (hipStream_t)stream_;
  double* part = (double*)workspace;
  if (p.blocks > 0)
    PCNN_LAUNCH(vertex_head_bwd_kernel, dim3((unsigned)p.blocks), dim3(VH_THREADS), p.shmem, stream, z, bias, label, instance,
                objects, out, upstream, H, W, C, M, k, s, sigma * sigma, p.th, p.tw, p.tiles_y, p.tiles_x, dz, part);
  PCNN_LAUNCH(channel_partials_final_kernel<CPF_THREADS>, dim3((unsigned)(3 * C)), dim3(CPF_THREADS), 0, stream, part, (int)p.blocks, dbias);
  return check_launch(who);
}
