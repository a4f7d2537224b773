// trunk_epilogue.hip — the training twins of the trunk's epilogue kernels (upscore.hip: bias_act_kernel,
// bias_relu_pool2_kernel), forward and backward (include/posecnn_hip_trunk_train.h).
//
// Under autograd the trunk's bias_add -> ReLU -> max_pool (network.py:181-187,303-310) is three framework kernels each way,
// an activated full-resolution tensor kept for the ReLU's backward and an int64 index tensor kept for the pool's. Here:
//
//   pcnn_bias_relu_pool2_train_fwd   pooled (+ the activated tensor when somebody else reads it) and one byte per pooled
//                                    element: which of the window's four values won, or that the ReLU closed the window
//   pcnn_bias_relu_pool2_train_bwd   dy from dpooled and that byte (+ the gated dact of the dual form), and dbias
//   pcnn_bias_relu_train_bwd         dy = gate(da) and dbias for the layers without a pool (forward: pcnn_bias_act_fwd, in place)
//
// All three are streams: every byte is read or written once. The bias gradient rides in the pass that writes dy: f64, fixed
// order, no atomics — per-run partials here, then channel_partials_final_kernel (reduce_device.h) as in label_loss.hip; the
// order is stated in the header and restated in numpy by tests/trunk_epilogue_ref.py. load_v / store_v: pcnn_device.h.
#include "../../include/posecnn_hip_trunk_train.h"
#include "reduce_device.h"

namespace {

using namespace pcnn;

constexpr int TE_RUN = 128;     // pixels per workgroup: the unit of the dbias partition
constexpr int TE_SLOTS = 16;    // pixel p of a run is summed in slot p % TE_SLOTS
constexpr int TE_LANES = 16;    // threads across a workgroup's channels
constexpr int TE_CHUNK = 64;    // channels per workgroup: TE_LANES threads x 4
constexpr int TE_THREADS = TE_SLOTS * TE_LANES;

// The window's byte: V of them as one word on the vector path. Written once here and read once by the backward pass, a whole
// forward and backward of the rest of the network later: kept out of the cache lines the feature maps live in (the
// non-temporal note of upscore.hip's up_copy_out).
template <int V>
__device__ __forceinline__ void store_sel(uint8_t* p, const unsigned* s)
{
  if (V == 4)
    __builtin_nontemporal_store(s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24), reinterpret_cast<unsigned*>(p));
  else
    p[0] = (uint8_t)s[0];
}
template <int V>
__device__ __forceinline__ void load_sel(const uint8_t* p, unsigned* s)
{
  if (V == 4) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = (w >> (8 * i)) & 255u;
  } else {
    s[0] = p[0];
  }
}

// One thread per pooled pixel x V channels, as bias_relu_pool2_kernel. y and act may be the same tensor: a thread reads its
// window before it writes it and nobody else touches it (so neither is __restrict__).
template <int V>
__global__ __launch_bounds__(256) void bias_relu_pool2_train_fwd_kernel(const float* y, const float* __restrict__ bias,
                                                                        float* act, float* __restrict__ pooled,
                                                                        uint8_t* __restrict__ sel, long long total, int Wo,
                                                                        int C, int relu)
{
  const int cv = C / V;
  const long long rowstride = (long long)2 * Wo * C;   // one input row
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % cv) * V;
    const long long p = idx / cv;            // pooled pixel (b, oy, ox)
    const int ox = (int)(p % Wo);
    const long long bo = p / Wo;             // b * Ho + oy
    const long long f0 = (bo * 2) * rowstride + (long long)(2 * ox) * C + c;
    const long long off[4] = {f0, f0 + C, f0 + rowstride, f0 + rowstride + C};
    float t[4][V];
#pragma unroll
    for (int k = 0; k < 4; k++) load_v<V>(y + off[k], t[k]);
    float best[V];
    unsigned s[V];
#pragma unroll
    for (int i = 0; i < V; i++) {
      const float b = bias[c + i];
#pragma unroll
      for (int k = 0; k < 4; k++) t[k][i] = t[k][i] + b;
      best[i] = t[0][i];
      s[i] = 0u;
#pragma unroll
      for (int k = 1; k < 4; k++)
        if (t[k][i] > best[i]) {
          best[i] = t[k][i];
          s[i] = (unsigned)k;
        }
      if (relu) {
        if (!(best[i] > 0.f)) s[i] = 4u;
        best[i] = best[i] > 0.f ? best[i] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) t[k][i] = t[k][i] > 0.f ? t[k][i] : 0.f;
      }
    }
    store_v<V>(pooled + idx * V, best);
    store_sel<V>(sel + idx * V, s);
    if (act) {
#pragma unroll
      for (int k = 0; k < 4; k++) store_v<V>(act + off[k], t[k]);
    }
  }
}

// ---- the backward passes: a workgroup owns TE_RUN pixels x TE_CHUNK channels -----------------------------------------------
// Thread (lane, slot) = (tid % 16, tid / 16) owns four channels of the chunk — V = 4: 4 lane .. 4 lane + 3 (one 16-byte access),
// V = 1: lane, lane + 16, lane + 32, lane + 48 — and the pixels slot, slot + 16, ... of the run. Which channels a thread owns
// differs between the two load paths; which pixels a slot sums, and in what order, does not.
template <int V>
__device__ __forceinline__ int te_channel(int lane, int i)
{
  return V == 4 ? 4 * lane + i : lane + TE_LANES * i;
}

// slot sums -> the run's partial per channel; every thread of the workgroup calls it
template <int V>
__device__ __forceinline__ void te_reduce_run(double (*s_acc)[TE_CHUNK], const double* acc, double* __restrict__ part, int c0,
                                              int C, int lane, int slot)
{
#pragma unroll
  for (int i = 0; i < 4; i++) s_acc[slot][te_channel<V>(lane, i)] = acc[i];
  __syncthreads();
  for (int st = TE_SLOTS / 2; st >= 1; st >>= 1) {
    if (slot < st) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int cl = te_channel<V>(lane, i);
        s_acc[slot][cl] = s_acc[slot][cl] + s_acc[slot + st][cl];
      }
    }
    __syncthreads();
  }
  if (slot == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int cl = te_channel<V>(lane, i);
      if (c0 + cl < C) part[(size_t)(c0 + cl) * gridDim.x + blockIdx.x] = s_acc[0][cl];
    }
  }
}

template <int V>
__global__ __launch_bounds__(TE_THREADS) void bias_relu_train_bwd_kernel(const float* __restrict__ da,
                                                                         const float* __restrict__ a, float* __restrict__ dy,
                                                                         double* __restrict__ part, long long rows, int C,
                                                                         int relu)
{
  __shared__ double s_acc[TE_SLOTS][TE_CHUNK];
  const int lane = threadIdx.x % TE_LANES, slot = threadIdx.x / TE_LANES;
  const int c0 = blockIdx.y * TE_CHUNK;
  const long long p0 = (long long)blockIdx.x * TE_RUN;
  const int npx = (int)(rows - p0 < TE_RUN ? rows - p0 : TE_RUN);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = slot; p < npx; p += TE_SLOTS) {
    const long long base = (p0 + p) * C + c0;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (V == 4) {
      const int cl = 4 * lane;
      if (c0 + cl < C) {
        load_v<4>(da + base + cl, g);
        if (relu) {
          float v[4];
          load_v<4>(a + base + cl, v);
#pragma unroll
          for (int i = 0; i < 4; i++) g[i] = v[i] > 0.f ? g[i] : 0.f;
        }
        store_v<4>(dy + base + cl, g);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int cl = lane + TE_LANES * i;
        if (c0 + cl < C) {
          g[i] = da[base + cl];
          if (relu) g[i] = a[base + cl] > 0.f ? g[i] : 0.f;
          dy[base + cl] = g[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = acc[i] + (double)g[i];
  }
  if (part) te_reduce_run<V>(s_acc, acc, part, c0, C, lane, slot);
}

// dact and dy may not overlap; dact == nullptr: the pooled-only form
template <int V>
__global__ __launch_bounds__(TE_THREADS) void bias_relu_pool2_train_bwd_kernel(
    const float* __restrict__ dpooled, const uint8_t* __restrict__ sel, const float* __restrict__ dact,
    const float* __restrict__ act, float* __restrict__ dy, double* __restrict__ part, long long windows, int Wo, int C)
{
  __shared__ double s_acc[TE_SLOTS][TE_CHUNK];
  const int lane = threadIdx.x % TE_LANES, slot = threadIdx.x / TE_LANES;
  const int c0 = blockIdx.y * TE_CHUNK;
  const long long p0 = (long long)blockIdx.x * TE_RUN;
  const int npx = (int)(windows - p0 < TE_RUN ? windows - p0 : TE_RUN);
  const long long rowstride = (long long)2 * Wo * C;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = slot; p < npx; p += TE_SLOTS) {
    const long long q = p0 + p;              // pooled pixel (b, oy, ox)
    const int ox = (int)(q % Wo);
    const long long bo = q / Wo;
    const long long f0 = (bo * 2) * rowstride + (long long)(2 * ox) * C + c0;
    const long long off[4] = {f0, f0 + C, f0 + rowstride, f0 + rowstride + C};
    const long long pbase = q * C + c0;
    float g[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int i = 0; i < 4; i++) g[k][i] = 0.f;
    if (V == 4) {
      const int cl = 4 * lane;
      if (c0 + cl < C) {
        float dp[4];
        unsigned s[4];
        load_v<4>(dpooled + pbase + cl, dp);
        load_sel<4>(sel + pbase + cl, s);
        float da4[4][4], a4[4][4];
        if (dact) {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            load_v<4>(dact + off[k] + cl, da4[k]);
            load_v<4>(act + off[k] + cl, a4[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float r = s[i] == (unsigned)k ? dp[i] : 0.f;
            g[k][i] = dact ? (a4[k][i] > 0.f ? da4[k][i] : 0.f) + r : r;
          }
          store_v<4>(dy + off[k] + cl, g[k]);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int cl = lane + TE_LANES * i;
        if (c0 + cl < C) {
          const float dp = dpooled[pbase + cl];
          const unsigned s = sel[pbase + cl];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const float r = s == (unsigned)k ? dp : 0.f;
            g[k][i] = dact ? (act[off[k] + cl] > 0.f ? dact[off[k] + cl] : 0.f) + r : r;
            dy[off[k] + cl] = g[k][i];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int k = 0; k < 4; k++) acc[i] = acc[i] + (double)g[k][i];
    }
  }
  if (part) te_reduce_run<V>(s_acc, acc, part, c0, C, lane, slot);
}

struct Plan {
  long long pixels;   // rows, or windows
  int nruns, nchunks;
  size_t ws_bytes;
};

int make_plan(const char* who, long long pixels, long long per_pixel, int C, Plan* p)
{
  PCNN_REQUIRE(pixels >= 1 && C >= 1, PCNN_EINVAL, "%s: bad shape: %lld pixels, %d channels", who, pixels, C);
  PCNN_REQUIRE(pixels < (1ll << 31) && pixels * per_pixel <= ((1ll << 31) - 1) / C, PCNN_EINVAL,
               "%s: the tensor must have fewer than 2^31 elements", who);
  p->pixels = pixels;
  p->nruns = (int)((pixels + TE_RUN - 1) / TE_RUN);
  p->nchunks = (C + TE_CHUNK - 1) / TE_CHUNK;
  p->ws_bytes = sizeof(double) * (size_t)p->nruns * (size_t)C;
  return PCNN_OK;
}

int pool_plan(const char* who, int B, int H, int W, int C, Plan* p)
{
  PCNN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, PCNN_EINVAL, "%s: bad shape %dx%dx%dx%d", who, B, H, W, C);
  PCNN_REQUIRE(H % 2 == 0 && W % 2 == 0, PCNN_EINVAL, "%s: need even height/width (got %dx%dx%dx%d)", who, B, H, W, C);
  PCNN_REQUIRE((long long)B * H < (1ll << 31) && (long long)B * H * W < (1ll << 31), PCNN_EINVAL,
               "%s: the tensor must have fewer than 2^31 elements", who);
  return make_plan(who, (long long)B * (H / 2) * (W / 2), 4, C, p);
}

int check_workspace(const char* who, const Plan& p, const float* dbias, const void* workspace, size_t workspace_bytes)
{
  if (!dbias) return PCNN_OK;
  PCNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, p.ws_bytes);
  return PCNN_OK;
}

}  // namespace

extern "C" int pcnn_bias_relu_pool2_train_workspace_bytes(int B, int H, int W, int C, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "bias_relu_pool2_train_workspace_bytes: NULL bytes");
  Plan p;
  int st = pool_plan("bias_relu_pool2_train_workspace_bytes", B, H, W, C, &p);
  if (st != PCNN_OK) return st;
  *bytes = p.ws_bytes;
  return PCNN_OK;
}

extern "C" int pcnn_bias_relu_train_workspace_bytes(int64_t rows, int C, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "bias_relu_train_workspace_bytes: NULL bytes");
  Plan p;
  int st = make_plan("bias_relu_train_workspace_bytes", (long long)rows, 1, C, &p);
  if (st != PCNN_OK) return st;
  *bytes = p.ws_bytes;
  return PCNN_OK;
}

extern "C" int pcnn_bias_relu_pool2_train_fwd(const float* y, const float* bias, int B, int H, int W, int C, int relu,
                                              float* act, float* pooled, uint8_t* sel, void* stream_)
{
  const char* who = "bias_relu_pool2_train_fwd";
  Plan p;
  int st = pool_plan(who, B, H, W, C, &p);
  if (st != PCNN_OK) return st;
  PCNN_REQUIRE(relu == 0 || relu == 1, PCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", who, relu);
  PCNN_REQUIRE(y, PCNN_ENULL, "%s: NULL y", who);
  PCNN_REQUIRE(bias, PCNN_ENULL, "%s: NULL bias", who);
  PCNN_REQUIRE(pooled, PCNN_ENULL, "%s: NULL pooled", who);
  PCNN_REQUIRE(sel, PCNN_ENULL, "%s: NULL sel", who);
  hipStream_t stream = (hipStream_t)stream_;
  auto grid = [](long long total) { long long b = (total + 255) / 256; return (unsigned)(b < 256 * 32 ? b : 256 * 32); };
  const long long n = p.pixels * C;
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(pooled) && (!act || aligned16(act)) &&
                   (reinterpret_cast<uintptr_t>(sel) & 3u) == 0;
  if (vec)
    PCNN_LAUNCH(bias_relu_pool2_train_fwd_kernel<4>, dim3(grid(n / 4)), dim3(256), 0, stream, y, bias, act, pooled, sel, n / 4,
                W / 2, C, relu);
  else
    PCNN_LAUNCH(bias_relu_pool2_train_fwd_kernel<1>, dim3(grid(n)), dim3(256), 0, stream, y, bias, act, pooled, sel, n, W / 2,
                C, relu);
  return check_launch(who);
}

extern "C" int pcnn_bias_relu_pool2_train_bwd(const float* dpooled, const uint8_t* sel, const float* dact, const float* act,
                                              int B, int H, int W, int C, float* dy, float* dbias, void* workspace,
                                              size_t workspace_bytes, void* stream_)
{
  const char* who = "bias_relu_pool2_train_bwd";
  Plan p;
  int st = pool_plan(who, B, H, W, C, &p);
  if (st != PCNN_OK) return st;
  PCNN_REQUIRE((dact == nullptr) == (act == nullptr), PCNN_EINVAL, "%s: dact and act are both NULL or both given", who);
  PCNN_REQUIRE(dpooled, PCNN_ENULL, "%s: NULL dpooled", who);
  PCNN_REQUIRE(sel, PCNN_ENULL, "%s: NULL sel", who);
  PCNN_REQUIRE(dy, PCNN_ENULL, "%s: NULL dy", who);
  st = check_workspace(who, p, dbias, workspace, workspace_bytes);
  if (st != PCNN_OK) return st;
  hipStream_t stream = (hipStream_t)stream_;
  double* part = dbias ? (double*)workspace : nullptr;
  const dim3 grid((unsigned)p.nruns, (unsigned)p.nchunks);
  const bool vec = C % 4 == 0 && aligned16(dpooled) && aligned16(dy) && (!dact || (aligned16(dact) && aligned16(act))) &&
                   (reinterpret_cast<uintptr_t>(sel) & 3u) == 0;
  if (vec)
    PCNN_LAUNCH(bias_relu_pool2_train_bwd_kernel<4>, grid, dim3(TE_THREADS), 0, stream, dpooled, sel, dact, act, dy, part,
                p.pixels, W / 2, C);
  else
    PCNN_LAUNCH(bias_relu_pool2_train_bwd_kernel<1>, grid, dim3(TE_THREADS), 0, stream, dpooled, sel, dact, act, dy, part,
                p.pixels, W / 2, C);
  if (dbias) PCNN_LAUNCH(channel_partials_final_kernel<CPF_THREADS>, dim3((unsigned)C), dim3(CPF_THREADS), 0, stream, part, p.nruns, dbias);
  return check_launch(who);
}

extern "C" int pcnn_bias_relu_train_bwd(const float* da, const float* a, int64_t rows, int C, int relu, float* dy,
                                        float* dbias, void* workspace, size_t workspace_bytes, void* stream_)
{
  const char* who = "bias_relu_train_bwd";
  Plan p;
  int st = make_plan(who, (long long)rows, 1, C, &p);
  if (st != PCNN_OK) return st;
  PCNN_REQUIRE(relu == 0 || relu == 1, PCNN_EINVAL, "%s: relu must be 0 or 1 (got %d)", who, relu);
  PCNN_REQUIRE(da, PCNN_ENULL, "%s: NULL da", who);
  PCNN_REQUIRE(a || !relu, PCNN_ENULL, "%s: NULL a", who);
  PCNN_REQUIRE(dy, PCNN_ENULL, "%s: NULL dy", who);
  st = check_workspace(who, p, dbias, workspace, workspace_bytes);
  if (st != PCNN_OK) return st;
  hipStream_t stream = (hipStream_t)stream_;
  double* part = dbias ? (double*)workspace : nullptr;
  const dim3 grid((unsigned)p.nruns, (unsigned)p.nchunks);
  const bool vec = C % 4 == 0 && aligned16(da) && aligned16(dy) && (!relu || aligned16(a));
  if (vec)
    PCNN_LAUNCH(bias_relu_train_bwd_kernel<4>, grid, dim3(TE_THREADS), 0, stream, da, a, dy, part, (long long)rows, C, relu);
  else
    PCNN_LAUNCH(bias_relu_train_bwd_kernel<1>, grid, dim3(TE_THREADS), 0, stream, da, a, dy, part, (long long)rows, C, relu);
  if (dbias) PCNN_LAUNCH(channel_partials_final_kernel<CPF_THREADS>, dim3((unsigned)C), dim3(CPF_THREADS), 0, stream, part, p.nruns, dbias);
  return check_launch(who);
}
