// vertex_targets.hip — the training feed's vertex regression targets (lib/gt_synthesize_layer/minibatch.py:543-602,
// _generate_vertex_targets) on the device, and the vertex loss (lib/fcn/train.py:564-573) evaluated straight from what
// they are made of. Both [B,H,W,3C] tensors (1.3 GB each at B=16, 640x480, C=22) follow from a label map and a table
// of at most 64 objects per frame; only 3 of a foreground pixel's 3C channels carry weight.
//
//   vt_tile_kernel<VT_TARGETS>   writes targets + weights        (the generator: API completeness, the yardstick)
//   sl1_gt_partial_kernel        loss forward without them       (sl1_gt_device.h; + sl1_final_kernel of sl1_device.h)
//   vt_tile_kernel<VT_GRAD>      loss backward without them      (writes the full grad_pred)
//
// Arithmetic of a matched pixel: include/posecnn_hip_train.h. Float64, one rounding per operation (-ffp-contract=off;
// f64 sqrt and divide are correctly rounded on gfx950), so it equals numpy's bits.
//
// The tile kernels are store-bound. A block owns 256 consecutive pixels of one frame: every thread reads ONE label,
// matches it against the frame's table (in LDS: all lanes walk the same rows, a broadcast read) and leaves the pixel's
// three values in LDS — the float64 work runs once per matched pixel; then the block streams the tile's 256*3C floats
// out as 128-bit stores, each lane looking up the one or two pixels its four elements belong to.
//
// The forward keeps sl1_partial_kernel's reduction order exactly (thread (blk, t) takes elements
// blk*256 + t + m*SL1_BLOCKS*256, m ascending). An element without a matching row has weight +0 and in_loss +0 there,
// and a + (+0) == a bitwise for every value the accumulators can hold (they start at +0 and never become -0), so
// skipping it changes nothing: pred is loaded only under a matching row. Precondition: pred finite where the weight
// is 0 (the unfused kernel would make 0 * inf = NaN of it).
#include "sl1_gt_device.h"

#include "../../include/posecnn_hip_train.h"

namespace {

constexpr int VT_MAX_OBJECTS = 64;
constexpr int VT_TILE = 256;       // pixels per block = threads per block
constexpr int VT_TARGETS = 0, VT_GRAD = 1;

// element `ch` of tile pixel `pix`: its pixel's value if ch is one of the three live channels, else +0
template <int MODE>
__device__ __forceinline__ void vt_value(const float4* rec, const int* rch, int pix, int ch, float& a, float& b)
{
  a = 0.f;
  b = 0.f;
  const int d = ch - rch[pix];   // rch = -4 without a match: d >= 4
  if ((unsigned)d < 3u) {
    const float4 r = rec[pix];
    a = d == 0 ? r.x : (d == 1 ? r.y : r.z);
    if (MODE == VT_TARGETS) b = r.w;
  }
}

// grid (ceil(HW / 256), B). MODE VT_TARGETS: out0 = targets, out1 = weights. VT_GRAD: out0 = grad_pred.
// q4 / r4: quotient and remainder of 4 * 256 (the element stride of a thread's 128-bit stores) by 3C.
template <int MODE>
__global__ __launch_bounds__(VT_TILE) void vt_tile_kernel(const int32_t* __restrict__ label,
                                                           const int32_t* __restrict__ instance,
                                                           const float* __restrict__ objects,
                                                           const float* __restrict__ pred,
                                                           const float* __restrict__ sums,
                                                           const float* __restrict__ upstream, int HW, int W, int C,
                                                           int M, float sigma2, int q4, int r4,
                                                           float* __restrict__ out0, float* __restrict__ out1)
{
  __shared__ float tab[VT_MAX_OBJECTS * 6];
  __shared__ float4 rec[VT_TILE];
  __shared__ int rch[VT_TILE];
  const int t = threadIdx.x;
  const int C3 = 3 * C;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * VT_TILE;             // first pixel of the tile inside its frame
  const int npix = min(VT_TILE, HW - p0);
  const long long pix0 = (long long)b * HW + p0;   // ... inside the batch
  for (int k = t; k < 6 * M; k += VT_TILE) tab[k] = objects[(long long)b * M * 6 + k];
  __syncthreads();

  // ---- one pixel per thread: label -> row -> three values
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  int ch0 = -4;
  if (t < npix) {
    const int l = label[pix0 + t];
    if (l > 0 && l < C) {
      const int inst = instance ? instance[pix0 + t] : 0;
      const int y = (p0 + t) / W, x = (p0 + t) - y * W;
      float tx, ty, tz, w;
      if (vt_match(tab, M, l, inst, x, y, tx, ty, tz, w)) {
        ch0 = 3 * l;
        if (MODE == VT_TARGETS) {
          r = make_float4(tx, ty, tz, w);
        } else {
          const float denom = sums[2] + 1e-10f;
          const float g = upstream ? upstream[0] : 1.0f;
          const float* p = pred + (pix0 + t) * C3 + ch0;
          float il, dp;
          sl1_elem(p[0], tx, w, sigma2, il, dp);
          r.x = div_rn(dp, denom) * g;
          sl1_elem(p[1], ty, w, sigma2, il, dp);
          r.y = div_rn(dp, denom) * g;
          sl1_elem(p[2], tz, w, sigma2, il, dp);
          r.z = div_rn(dp, denom) * g;
        }
      }
    }
  }
  rec[t] = r;
  rch[t] = ch0;
  __syncthreads();

  // ---- stream the tile out: elements [e0, e0 + cnt) of the flat tensor; 128-bit stores on its 16-byte aligned part
  const long long e0 = pix0 * C3;
  const int cnt = npix * C3;
  const int head = min((int)((4 - (e0 & 3)) & 3), cnt);
  const int nquad = (cnt - head) >> 2;
  const int tail0 = head + 4 * nquad;
  if (t < head || tail0 + t < cnt) {               // at most 3 + 3 scalar elements per tile
    const int rel = t < head ? t : tail0 + t;
    float a, w;
    vt_value<MODE>(rec, rch, rel / C3, rel % C3, a, w);
    out0[e0 + rel] = a;
    if (MODE == VT_TARGETS) out1[e0 + rel] = w;
    if (t < head && tail0 + t < cnt) {             // a thread can own one of each
      const int rel2 = tail0 + t;
      vt_value<MODE>(rec, rch, rel2 / C3, rel2 % C3, a, w);
      out0[e0 + rel2] = a;
      if (MODE == VT_TARGETS) out1[e0 + rel2] = w;
    }
  }
  float4* o0 = reinterpret_cast<float4*>(out0 + e0 + head);
  float4* o1 = MODE == VT_TARGETS ? reinterpret_cast<float4*>(out1 + e0 + head) : nullptr;
  int pix = (head + 4 * t) / C3, ch = (head + 4 * t) - pix * C3;
  for (int q = t; q < nquad; q += VT_TILE) {
    float a[4], w[4];
    int pp = pix, cc = ch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      vt_value<MODE>(rec, rch, pp, cc, a[k], w[k]);
      if (++cc == C3) {
        cc = 0;
        ++pp;   // never read past the tile: the quad's last element is inside it
      }
    }
    o0[q] = make_float4(a[0], a[1], a[2], a[3]);
    if (MODE == VT_TARGETS) o1[q] = make_float4(w[0], w[1], w[2], w[3]);
    pix += q4;
    ch += r4;
    if (ch >= C3) {
      ch -= C3;
      ++pix;
    }
  }
}

// shape checks shared by the three entries; *pixels = B*H*W
int vt_check_shape(const char* who, int B, int H, int W, int C, int M, long long* pixels)
{
  PCNN_REQUIRE(B >= 0 && H >= 0 && W >= 0, PCNN_EINVAL, "%s: negative size", who);
  PCNN_REQUIRE(C >= 2 && C <= PCNN_MAX_CLASSES, PCNN_EINVAL, "%s: 2 <= num_classes <= %d", who, PCNN_MAX_CLASSES);
  PCNN_REQUIRE(M >= 0 && M <= VT_MAX_OBJECTS, PCNN_EINVAL, "%s: 0 <= num_objects <= %d", who, VT_MAX_OBJECTS);
  PCNN_REQUIRE(B <= 65535, PCNN_EINVAL, "%s: batch > 65535", who);
  *pixels = (long long)B * H * W;
  PCNN_REQUIRE(*pixels <= (1ll << 30), PCNN_EINVAL, "%s: more than 2^30 pixels", who);   // pixel indices are ints
  return PCNN_OK;
}

}  // namespace

extern "C" int pcnn_vertex_targets_fwd(const int32_t* label, const int32_t* instance, const float* objects, int B,
                                       int H, int W, int C, int M, float* targets, float* weights, void* stream_)
{
  long long pixels;
  if (int st = vt_check_shape("vertex_targets", B, H, W, C, M, &pixels)) return st;
  if (pixels == 0) return PCNN_OK;
  PCNN_REQUIRE(label && targets && weights && (objects || M == 0), PCNN_ENULL, "vertex_targets: NULL pointer");
  PCNN_REQUIRE(aligned16(targets) && aligned16(weights), PCNN_EINVAL, "vertex_targets: outputs need 16-byte alignment");
  hipStream_t stream = (hipStream_t)stream_;
  const int HW = H * W, C3 = 3 * C;
  PCNN_LAUNCH(vt_tile_kernel<VT_TARGETS>, dim3((HW + VT_TILE - 1) / VT_TILE, B), dim3(VT_TILE), 0, stream, label,
              instance, objects, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, HW, W, C, M,
              0.f, 4 * VT_TILE / C3, 4 * VT_TILE % C3, targets, weights);
  return check_launch("vertex_targets_fwd");
}

extern "C" int pcnn_smooth_l1_vertex_gt_fwd(const float* pred, const int32_t* label, const int32_t* instance,
                                            const float* objects, int B, int H, int W, int C, int M, float sigma,
                                            float* out, void* workspace, size_t workspace_bytes, void* stream_)
{
  long long pixels;
  if (int st = vt_check_shape("smooth_l1_vertex_gt", B, H, W, C, M, &pixels)) return st;
  PCNN_REQUIRE(sigma > 0.f, PCNN_EINVAL, "smooth_l1_vertex_gt: sigma must be positive");
  PCNN_REQUIRE(out && (pixels == 0 || (pred && label && (objects || M == 0))), PCNN_ENULL,
               "smooth_l1_vertex_gt: NULL pointer");
  PCNN_REQUIRE(workspace && workspace_bytes >= sizeof(float) * 2 * SL1_BLOCKS, PCNN_EWORKSPACE,
               "smooth_l1_vertex_gt: workspace NULL or too small");
  hipStream_t stream = (hipStream_t)stream_;
  float* partial = (float*)workspace;
  const int C3 = 3 * C, stride = SL1_BLOCKS * 256;
  PCNN_LAUNCH(sl1_gt_partial_kernel<PredTensor>, dim3(SL1_BLOCKS), dim3(256), 0, stream, PredTensor{pred}, label, instance,
              objects, pixels * C3, H * W, W, C, M, sigma * sigma, stride / C3, stride % C3, partial);
  PCNN_LAUNCH(sl1_final_kernel, dim3(1), dim3(SL1_BLOCKS / 2), 0, stream, partial, out);
  return check_launch("smooth_l1_vertex_gt_fwd");
}

extern "C" int pcnn_smooth_l1_vertex_gt_bwd(const float* pred, const int32_t* label, const int32_t* instance,
                                            const float* objects, const float* out, const float* upstream, int B,
                                            int H, int W, int C, int M, float sigma, float* grad_pred,
                                            void* stream_)
{
  long long pixels;
  if (int st = vt_check_shape("smooth_l1_vertex_gt_bwd", B, H, W, C, M, &pixels)) return st;
  PCNN_REQUIRE(sigma > 0.f, PCNN_EINVAL, "smooth_l1_vertex_gt_bwd: sigma must be positive");
  if (pixels == 0) return PCNN_OK;
  PCNN_REQUIRE(pred && label && out && grad_pred && (objects || M == 0), PCNN_ENULL,
               "smooth_l1_vertex_gt_bwd: NULL pointer");
  PCNN_REQUIRE(aligned16(grad_pred), PCNN_EINVAL, "smooth_l1_vertex_gt_bwd: grad_pred needs 16-byte alignment");
  hipStream_t stream = (hipStream_t)stream_;
  const int HW = H * W, C3 = 3 * C;
  PCNN_LAUNCH(vt_tile_kernel<VT_GRAD>, dim3((HW + VT_TILE - 1) / VT_TILE, B), dim3(VT_TILE), 0, stream, label,
              instance, objects, pred, out, upstream, HW, W, C, M, sigma * sigma, 4 * VT_TILE / C3,
              4 * VT_TILE % C3, grad_pred, (float*)nullptr);
  return check_launch("smooth_l1_vertex_gt_bwd");
}
