// augment.hip — the training augmentation of lib/utils/blob.py:74-129 (`chromatic_transform`, `add_noise`) in the order of
// lib/gt_synthesize_layer/minibatch.py:170-201, fused with the blob formation: raw uint8 colour (and uint16 depth) frames
// in, the network's f32 `data` (`data_p`) blobs out. Arithmetic of every step: include/posecnn_hip_augment.h. One IEEE
// rounding per operation (-ffp-contract=off, correctly rounded divide and sqrt), so the numpy restatement
// (tests/augment_ref.py) agrees bit for bit everywhere but in the Gaussian's log and cos, which are the device library's.
//
//   augment_depth_max_kernel   per-frame maximum of the depth frame (depth_norm = 0 only): one workgroup per frame, 16-byte
//                              loads, one plain store — no atomics, nothing to zero first
//   augment_frames_kernel      everything else. A workgroup of 256 threads owns a 64 x 16 tile of one frame, a thread 4
//                              consecutive pixels of a row; blockIdx.z is the frame, whose row of parameters (a kernel
//                              argument) makes the mode uniform over the workgroup. The colour plane, then the depth plane:
//       modes 0, 1   a thread loads its own 4 pixels (16 bytes of BGRA, 12 of BGR, 8 of depth), no LDS staging; the
//                    Gaussian draws ONE Philox block per thread when W % 4 == 0 (a block is 4 pixels);
//       modes 2, 3   the tile's transformed pixels plus a halo of size / 2 along the blur's axis are staged in LDS (packed
//                    (b, g, r, 0) dwords; f32 depth values), reflect-101 coordinates, so the HLS round trip of a pixel is
//                    computed once per tile however long the line is;
//       store        the 12 floats of a thread go through LDS so that the global stores are consecutive float4s along the
//                    tile's 768-byte row segments (W % 4 == 0; scalar stores otherwise).
// Which side bounds it (reasoning, no counters collected yet): 16 bytes move per colour pixel (4 in, 12 out) against
// roughly 300 vector-ALU operations in mode 1 (a quarter of a Philox block's twenty 64 x 64 -> 128-bit multiplies, log, cos,
// the HLS pair with its four divisions, nine f64 operations) — at 16 x 480 x 640 about 40 us of ALU against 16 us of HBM
// traffic: ALU bound by 2-3 x, as per-element transcendentals make a streaming kernel (DESIGN.md 3.6t has the timings).
#include "pcnn_device.h"
#include "philox_device.h"

#include "../../include/posecnn_hip_augment.h"

namespace {

using namespace pcnn;

constexpr int TW = 64, TH = 16;               // tile
constexpr int NTHREADS = 256;
constexpr int MAX_R = 7;
constexpr int STAGE_WORDS = (TW * (TH + 2 * MAX_R) > (TW + 2 * MAX_R) * TH) ? TW * (TH + 2 * MAX_R) : (TW + 2 * MAX_R) * TH;
constexpr int ROW_FLOATS = TW * 3;
constexpr int MODE_NONE = 0, MODE_GAUSS = 1, MODE_HBLUR = 2, MODE_VBLUR = 3;
constexpr int MAX_THREADS_MAX = 1024;

struct PlaneRow {
  unsigned long long stream;
  float sigma;
  int mode, size, pad;
};

struct FrameRow {                             // 80 bytes: 32 of them are 2560 bytes of kernel arguments
  double dh, dl, ds;
  PlaneRow color, depth;
  int chroma, pad;
};

struct Rows {
  FrameRow r[PCNN_AUGMENT_LAUNCH_FRAMES];
};

struct Means {
  double m[3];
};

__device__ __forceinline__ int reflect101(int p, int n)
{
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

__device__ __forceinline__ uint32_t to_byte(float v)          // rint, held in [0, 255]
{
  return (uint32_t)(int)fminf(fmaxf(__builtin_rintf(v), 0.f), 255.f);
}

// steps 1-3 of the header on a packed (b, g, r, x) pixel -> packed (b, g, r, 0)
__device__ __forceinline__ uint32_t chromatic(uint32_t q, double dh, double dl, double ds)
{
  const float k255 = (float)(1.0 / 255.0);
  const float b = (float)(q & 0xffu) * k255, g = (float)((q >> 8) & 0xffu) * k255, r = (float)((q >> 16) & 0xffu) * k255;
  const float vmax = fmaxf(fmaxf(b, g), r), vmin = fminf(fminf(b, g), r);
  const float sum = vmax + vmin, l = sum * 0.5f, diff = vmax - vmin;
  float h = 0.f, s = 0.f;
  if (diff != 0.f) {
    s = div_rn(diff, l < 0.5f ? sum : (2.f - vmax) - vmin);
    const float qq = div_rn(60.f, diff);
    if (vmax == r) h = (g - b) * qq;
    else if (vmax == g) h = (b - r) * qq + 120.f;
    else h = (r - g) * qq + 240.f;
    if (h < 0.f) h = h + 360.f;
  }
  const uint32_t H8 = to_byte(h * 0.5f), L8 = to_byte(l * 255.f), S8 = to_byte(s * 255.f);

  double x = (double)H8 + dh;
  if (x >= 180.0) x = x - 180.0;
  else if (x < 0.0) x = x + 180.0;
  const double y = fmin(fmax((double)L8 + dl, 0.0), 255.0), z = fmin(fmax((double)S8 + ds, 0.0), 255.0);
  const int Hn = (int)x, Ln = (int)y, Sn = (int)z;

  const float l2 = (float)Ln * k255, s2 = (float)Sn * k255;
  float ob = l2, og = l2, orr = l2;
  if (Sn != 0) {
    const float p2 = l2 <= 0.5f ? l2 * (1.f + s2) : (l2 + s2) - l2 * s2;
    const float p1 = 2.f * l2 - p2, d = p2 - p1;
    int sector = Hn / 30;
    const float f = (float)(Hn - 30 * sector) * (float)(1.0 / 30.0);
    if (sector >= 6) sector -= 6;
    const float up = p1 + d * f, down = p1 + d * (1.f - f);
    orr = sector == 0 || sector == 5 ? p2 : sector == 1 ? down : sector == 4 ? up : p1;
    og = sector == 1 || sector == 2 ? p2 : sector == 0 ? up : sector == 3 ? down : p1;
    ob = sector == 3 || sector == 4 ? p2 : sector == 2 ? up : sector == 5 ? down : p1;
  }
  return to_byte(ob * 255.f) | (to_byte(og * 255.f) << 8) | (to_byte(orr * 255.f) << 16);
}

// philox4x64(counter, key): philox_device.h

__device__ __forceinline__ float gauss_of(unsigned long long w)
{
  const uint32_t hi = (uint32_t)(w >> 32), lo = (uint32_t)w;
  const float u1 = (float)((hi >> 8) + 1u) * 5.9604644775390625e-08f;     // 2^-24
  const float u2 = (float)(lo >> 8) * 5.9604644775390625e-08f;
  const float rad = sqrt_rn(-2.f * logf(u1));
  return rad * cosf(6.2831853071795864769f * u2);
}

// the normal deviates of the 4 pixels p0 .. p0 + 3 of a frame
__device__ __forceinline__ void gauss4(int p0, const PlaneRow& row, int plane, unsigned long long k0, unsigned long long k1,
                                       float g[4])
{
  unsigned long long blk[4];
  int cur = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + j;
    if ((p >> 2) != cur) {
      cur = p >> 2;
      philox4x64((unsigned long long)cur, row.stream, (unsigned long long)plane, k0, k1, blk);
    }
    const int w = p & 3;
    g[j] = gauss_of(w == 0 ? blk[0] : w == 1 ? blk[1] : w == 2 ? blk[2] : blk[3]);
  }
}

__device__ __forceinline__ float clip255(float v) { return v < 0.f ? 0.f : v > 255.f ? 255.f : v; }

__device__ __forceinline__ float depth_value(uint32_t d, int depth_norm, float fmax_)
{
  if (depth_norm == 0) return div_rn((float)d, fmax_) * 255.f;
  return fminf(fmaxf(div_rn((float)d, 2000.f), 0.f), 1.f) * 255.f;
}

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ color, long long pix, int C)
{
  if (C == 4) return *reinterpret_cast<const uint32_t*>(color + pix * 4);
  const uint8_t* s = color + pix * 3;
  return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
}

// grid (B); block 1024. ws[b] = the frame's largest depth value
__global__ __launch_bounds__(MAX_THREADS_MAX) void augment_depth_max_kernel(const uint16_t* __restrict__ depth, int HW,
                                                                            int* __restrict__ ws)
{
  __shared__ uint32_t part[MAX_THREADS_MAX / PCNN_WAVE];
  const int t = threadIdx.x;
  const uint16_t* f = depth + (long long)blockIdx.x * HW;
  uint32_t m = 0;
  // the frame's first element is 2-byte aligned only: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
  const int head = min(HW, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(f) & 15u)) & 15u) >> 1));
  const int body = (HW - head) >> 3;
  if (t < head) m = f[t];
  const uint4* v = reinterpret_cast<const uint4*>(f + head);
  for (int i = t; i < body; i += MAX_THREADS_MAX) {
    const uint4 q = v[i];
    m = max(m, max(max(q.x & 0xffffu, q.x >> 16), max(q.y & 0xffffu, q.y >> 16)));
    m = max(m, max(max(q.z & 0xffffu, q.z >> 16), max(q.w & 0xffffu, q.w >> 16)));
  }
  for (int i = head + 8 * body + t; i < HW; i += MAX_THREADS_MAX) m = max(m, (uint32_t)f[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((t & 63) == 0) part[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < MAX_THREADS_MAX / PCNN_WAVE; ++i) m = max(m, part[i]);
    ws[blockIdx.x] = (int)m;
  }
}

// grid (ceil(W / 64), ceil(H / 16), frames of this launch); color, depth, dmax, data, data_p point at the launch's first frame
__global__ __launch_bounds__(NTHREADS) void augment_frames_kernel(Rows rows, const uint8_t* __restrict__ color, int C,
                                                                   const uint16_t* __restrict__ depth,
                                                                   const int* __restrict__ dmax, int depth_norm,
                                                                   Means means, unsigned long long k0,
                                                                   unsigned long long k1, int H, int W,
                                                                   float* __restrict__ data, float* __restrict__ data_p)
{
  __shared__ uint32_t stage[STAGE_WORDS];
  __shared__ __attribute__((aligned(16))) float outf[TH * ROW_FLOATS];
  const int t = threadIdx.x;
  const int fr = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int th = min(TH, H - y0), tw = min(TW, W - x0);
  const int ty = t >> 4, tx = (t & 15) * 4;
  const int y = y0 + ty, x = x0 + tx;
  const long long frame = (long long)fr * H * W;
  const FrameRow row = rows.r[fr];
  const bool w4 = (W & 3) == 0;
  const bool mine = y < H && x < W;            // the thread's first pixel is in the frame (all four are when W % 4 == 0)
  const int p0 = y * W + x;

  for (int plane = 0; plane < (depth ? 2 : 1); ++plane) {
    const PlaneRow pr = plane == 0 ? row.color : row.depth;
    const int mode = pr.mode;
    float fmax_ = 0.f;
    if (plane == 1 && depth_norm == 0) fmax_ = (float)dmax[fr];
    float v[4][3];                             // the plane's values before the means are subtracted

    if (mode == MODE_HBLUR || mode == MODE_VBLUR) {
      // ---- stage the tile's transformed pixels + halo along the blur's axis
      const int r = pr.size >> 1;
      const int rx = mode == MODE_HBLUR ? r : 0, ry = mode == MODE_VBLUR ? r : 0;
      const int sw = TW + 2 * rx, count = sw * (th + 2 * ry);
      for (int k = t; k < count; k += NTHREADS) {
        const int ly = k / sw, lx = k - ly * sw;
        const int gy = reflect101(y0 - ry + ly, H), gx = reflect101(x0 - rx + lx, W);
        const long long pix = frame + (long long)gy * W + gx;
        if (plane == 0) {
          uint32_t q = load_pixel(color, pix, C) & 0xffffffu;
          if (row.chroma) q = chromatic(q, row.dh, row.dl, row.ds);
          stage[k] = q;
        } else {
          stage[k] = __float_as_uint(depth_value(depth[pix], depth_norm, fmax_));
        }
      }
      __syncthreads();
      const float kf = (float)(1.0 / (double)pr.size);
      const int step = mode == MODE_HBLUR ? 1 : sw;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t* base = stage + ty * sw + tx + j;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (plane == 0) {
          for (int i = 0; i < pr.size; ++i) {
            const uint32_t q = base[i * step];
            a0 = a0 + (float)(q & 0xffu) * kf;
            a1 = a1 + (float)((q >> 8) & 0xffu) * kf;
            a2 = a2 + (float)((q >> 16) & 0xffu) * kf;
          }
          v[j][0] = (float)to_byte(a0);
          v[j][1] = (float)to_byte(a1);
          v[j][2] = (float)to_byte(a2);
        } else {
          for (int i = 0; i < pr.size; ++i) a0 = a0 + __uint_as_float(base[i * step]) * kf;
          v[j][0] = v[j][1] = v[j][2] = a0;
        }
      }
    } else {
      // ---- the thread's own 4 pixels
      uint32_t q[4] = {0u, 0u, 0u, 0u};
      float dv[4] = {0.f, 0.f, 0.f, 0.f};
      if (mine) {
        const long long pix = frame + p0;
        if (plane == 0) {
          if (w4 && C == 4) {
            const uint4 u = *reinterpret_cast<const uint4*>(color + pix * 4);
            q[0] = u.x; q[1] = u.y; q[2] = u.z; q[3] = u.w;
          } else if (w4) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(color + pix * 3);
            const uint32_t a = s[0], b = s[1], c = s[2];
            q[0] = a; q[1] = (a >> 24) | (b << 8); q[2] = (b >> 16) | (c << 16); q[3] = c >> 8;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (x + j < W) q[j] = load_pixel(color, pix + j, C);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q[j] &= 0xffffffu;
            if (row.chroma) q[j] = chromatic(q[j], row.dh, row.dl, row.ds);
          }
        } else {
          uint32_t d[4] = {0u, 0u, 0u, 0u};
          if (w4) {
            const uint2 u = *reinterpret_cast<const uint2*>(depth + pix);
            d[0] = u.x & 0xffffu; d[1] = u.x >> 16; d[2] = u.y & 0xffffu; d[3] = u.y >> 16;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (x + j < W) d[j] = depth[pix + j];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) dv[j] = depth_value(d[j], depth_norm, fmax_);
        }
      }
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if (mode == MODE_GAUSS) gauss4(p0, pr, plane, k0, k1, g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (plane == 0) {
          v[j][0] = (float)(q[j] & 0xffu);
          v[j][1] = (float)((q[j] >> 8) & 0xffu);
          v[j][2] = (float)((q[j] >> 16) & 0xffu);
        } else {
          v[j][0] = v[j][1] = v[j][2] = dv[j];
        }
        if (mode == MODE_GAUSS) {
          const float n = pr.sigma * g[j];
#pragma unroll
          for (int c = 0; c < 3; ++c) v[j][c] = clip255(v[j][c] + n);
        }
      }
    }

    // ---- minus the means, through LDS to the plane's blob
    float* o = outf + ty * ROW_FLOATS + tx * 3;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * j + c] = (float)((double)v[j][c] - means.m[c]);
    __syncthreads();
    float* dst = (plane == 0 ? data : data_p) + (frame + (long long)y0 * W + x0) * 3;
    if (w4) {
      const int row4 = tw * 3 / 4;             // float4s of a row segment (tw is a multiple of 4)
      for (int k = t; k < th * (ROW_FLOATS / 4); k += NTHREADS) {
        const int ly = k / (ROW_FLOATS / 4), c4 = k - ly * (ROW_FLOATS / 4);
        if (c4 < row4)
          *reinterpret_cast<float4*>(dst + (long long)ly * W * 3 + c4 * 4) =
              *reinterpret_cast<const float4*>(outf + ly * ROW_FLOATS + c4 * 4);
      }
    } else {
      const int rowf = tw * 3;
      for (int k = t; k < th * ROW_FLOATS; k += NTHREADS) {
        const int ly = k / ROW_FLOATS, c = k - ly * ROW_FLOATS;
        if (c < rowf) dst[(long long)ly * W * 3 + c] = outf[ly * ROW_FLOATS + c];
      }
    }
    __syncthreads();                           // outf and stage are reused by the depth plane
  }
}

bool blur_size_ok(int s) { return s == 3 || s == 5 || s == 7 || s == 9 || s == 11 || s == 15; }

// one plane's columns (mode, sigma or size, stream id) of frame b -> PlaneRow
int pack_plane(const char* what, int b, const double* col, PlaneRow* out)
{
  const double mode = col[0], arg = col[1], stream = col[2];
  PCNN_REQUIRE(mode == 0.0 || mode == 1.0 || mode == 2.0 || mode == 3.0, PCNN_EINVAL,
               "augment_frames: params row %d: %s mode must be 0, 1, 2 or 3 (got %g)", b, what, mode);
  PCNN_REQUIRE(stream >= 0.0 && stream < 9007199254740992.0 && stream == (double)(unsigned long long)stream, PCNN_EINVAL,
               "augment_frames: params row %d: %s stream id must be an integer in [0, 2^53) (got %g)", b, what, stream);
  out->mode = (int)mode;
  out->stream = (unsigned long long)stream;
  out->sigma = 0.f;
  out->size = 0;
  out->pad = 0;
  if (out->mode == MODE_GAUSS) {
    PCNN_REQUIRE(arg >= 0.0 && arg <= 3.0e38, PCNN_EINVAL, "augment_frames: params row %d: %s sigma must be finite and >= 0 (got %g)",
                 b, what, arg);
    out->sigma = (float)arg;
  } else if (out->mode != MODE_NONE) {
    PCNN_REQUIRE(arg >= 3.0 && arg <= 15.0 && arg == (double)(int)arg && blur_size_ok((int)arg), PCNN_EINVAL,
                 "augment_frames: params row %d: %s blur size must be one of 3 5 7 9 11 15 (got %g)", b, what, arg);
    out->size = (int)arg;
  }
  return PCNN_OK;
}

int check_shape(int B, int H, int W)
{
  PCNN_REQUIRE(B >= 1 && B <= 65535 * PCNN_AUGMENT_LAUNCH_FRAMES, PCNN_EINVAL, "augment_frames: batch must be at least 1 (got %d)", B);
  PCNN_REQUIRE(H >= 8 && W >= 8, PCNN_EINVAL, "augment_frames: height and width must be at least 8 (got %d x %d)", H, W);
  PCNN_REQUIRE(H <= 65535 * TH, PCNN_EINVAL, "augment_frames: height > %d (one grid row per %d image rows)", 65535 * TH, TH);
  PCNN_REQUIRE((long long)B * H * W <= (1ll << 30), PCNN_EINVAL, "augment_frames: batch * height * width is more than 2^30 pixels");
  return PCNN_OK;
}

}  // namespace

extern "C" int pcnn_augment_frames_workspace_bytes(int B, int has_depth, int depth_norm, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "augment_frames_workspace_bytes: bytes is NULL");
  PCNN_REQUIRE(B >= 1, PCNN_EINVAL, "augment_frames_workspace_bytes: batch must be at least 1 (got %d)", B);
  PCNN_REQUIRE(depth_norm == 0 || depth_norm == 1, PCNN_EINVAL, "augment_frames_workspace_bytes: depth_norm must be 0 or 1 (got %d)",
               depth_norm);
  *bytes = has_depth && depth_norm == 0 ? align_up((size_t)B * sizeof(int), 16) : 0;
  return PCNN_OK;
}

extern "C" int pcnn_augment_frames_fwd(const uint8_t* color, int C, const uint16_t* depth, const double* params,
                                       const double* pixel_means, uint64_t seed0, uint64_t seed1, int depth_norm, int B,
                                       int H, int W, float* data, float* data_p, void* workspace, size_t workspace_bytes,
                                       void* stream_)
{
  if (int st = check_shape(B, H, W)) return st;
  PCNN_REQUIRE(C == 3 || C == 4, PCNN_EINVAL, "augment_frames: channels must be 3 or 4 (got %d)", C);
  PCNN_REQUIRE(depth_norm == 0 || depth_norm == 1, PCNN_EINVAL, "augment_frames: depth_norm must be 0 or 1 (got %d)", depth_norm);
  PCNN_REQUIRE(color, PCNN_ENULL, "augment_frames: color is NULL");
  PCNN_REQUIRE(params, PCNN_ENULL, "augment_frames: params is NULL");
  PCNN_REQUIRE(pixel_means, PCNN_ENULL, "augment_frames: pixel_means is NULL");
  PCNN_REQUIRE(data, PCNN_ENULL, "augment_frames: data is NULL");
  PCNN_REQUIRE(!depth || data_p, PCNN_ENULL, "augment_frames: data_p is NULL and depth is given");
  PCNN_REQUIRE(aligned16(color) && aligned16(depth) && aligned16(data) && aligned16(data_p), PCNN_EINVAL,
               "augment_frames: color, depth, data and data_p must be 16-byte aligned");
  for (int c = 0; c < 3; ++c)
    PCNN_REQUIRE(pixel_means[c] - pixel_means[c] == 0.0, PCNN_EINVAL, "augment_frames: pixel_means[%d] is not finite", c);
  size_t need = 0;
  if (int st = pcnn_augment_frames_workspace_bytes(B, depth != nullptr, depth_norm, &need)) return st;
  PCNN_REQUIRE(need == 0 || workspace, PCNN_ENULL, "augment_frames: workspace is NULL (%zu bytes needed)", need);
  PCNN_REQUIRE(workspace_bytes >= need, PCNN_EWORKSPACE, "augment_frames: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  PCNN_REQUIRE(need == 0 || aligned16(workspace), PCNN_EINVAL, "augment_frames: workspace must be 16-byte aligned");

  // every row is checked before the first launch
  for (int b = 0; b < B; ++b) {
    const double* p = params + (size_t)b * PCNN_AUGMENT_ROW;
    FrameRow tmp;
    PCNN_REQUIRE(p[0] >= -90.0 && p[0] <= 90.0, PCNN_EINVAL, "augment_frames: params row %d: d_h must be in [-90, 90] (got %g)", b, p[0]);
    PCNN_REQUIRE(p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0, PCNN_EINVAL, "augment_frames: params row %d: d_l and d_s must be finite", b);
    PCNN_REQUIRE(p[6] == 0.0 || p[6] == 1.0, PCNN_EINVAL, "augment_frames: params row %d: chromatic must be 0 or 1 (got %g)", b, p[6]);
    if (int st = pack_plane("colour", b, p + 3, &tmp.color)) return st;
    if (depth)
      if (int st = pack_plane("depth", b, p + 7, &tmp.depth)) return st;
  }

  hipStream_t stream = (hipStream_t)stream_;
  int* dmax = nullptr;
  if (need) {
    dmax = static_cast<int*>(workspace);
    PCNN_LAUNCH(augment_depth_max_kernel, dim3(B), dim3(MAX_THREADS_MAX), 0, stream, depth, H * W, dmax);
  }
  Means means = {{pixel_means[0], pixel_means[1], pixel_means[2]}};
  const long long HW = (long long)H * W;
  for (int b0 = 0; b0 < B; b0 += PCNN_AUGMENT_LAUNCH_FRAMES) {
    const int nb = B - b0 < PCNN_AUGMENT_LAUNCH_FRAMES ? B - b0 : PCNN_AUGMENT_LAUNCH_FRAMES;
    Rows rows = {};
    for (int i = 0; i < nb; ++i) {
      const double* p = params + (size_t)(b0 + i) * PCNN_AUGMENT_ROW;
      FrameRow& r = rows.r[i];
      r.dh = p[0];
      r.dl = p[1];
      r.ds = p[2];
      r.chroma = (int)p[6];
      pack_plane("colour", b0 + i, p + 3, &r.color);
      if (depth) pack_plane("depth", b0 + i, p + 7, &r.depth);
    }
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, nb);
    PCNN_LAUNCH(augment_frames_kernel, grid, dim3(NTHREADS), 0, stream, rows, color + b0 * HW * C,
                C, depth ? depth + b0 * HW : nullptr, dmax ? dmax + b0 : nullptr, depth_norm, means,
                (unsigned long long)seed0, (unsigned long long)seed1, H, W, data + b0 * HW * 3,
                data_p ? data_p + b0 * HW * 3 : nullptr);
  }
  return check_launch("augment_frames_fwd");
}
