// normals.hip — the network input of cfg.INPUT = 'NORMAL' (lib/fcn/test.py:80-101) formed on the device: the normal map
// of lib/normals/compute_normals.cu:30-101 (computeVmapKernel + computeNmapKernel), its uint8 image, and the 8-bit
// 3-channel bilateral filter the reference runs over it (cv2.bilateralFilter(im, 9, 75, 75)). Arithmetic of every
// stage: include/posecnn_hip_frontend.h. One IEEE f32 rounding per operation (-ffp-contract=off, correctly rounded
// divide and sqrt), so the numpy restatement (tests/normals_ref.py) agrees bit for bit.
//
//   depth_normals_kernel          nmap f32 [B,H,W,3]                       (API completeness, the yardstick)
//   tile_kernel<SRC_IMAGE, D>     bilateral filter of a uint8 image        (likewise)
//   tile_kernel<SRC_DEPTH, D>     depth -> filtered normal image           (the hot path: nothing between in memory)
//
// tile_kernel: a workgroup of 256 threads owns a 32 x 32 tile of the output. LDS holds the tile's source pixels plus a
// halo of r = d / 2, one packed dword (b, g, r, 0) each; SRC_DEPTH computes them from the depth with reflect-101
// coordinates (the quantised normal of the reflected pixel is what the filter's border sees), 1.56 x the tile's own
// pixels at d = 9. A lane reads consecutive dwords of a row (no bank conflict); the 768-entry colour table sits in LDS
// and is indexed by one v_sad_u8 of the two packed pixels. D = 9 unrolls the 49 taps with immediate LDS offsets and the
// space weights in scalar registers; D = 0 is the loop for any other d. The 3-byte results go through LDS so that the
// global stores are dwords wherever a row segment covers a whole one (3 W need not be a multiple of 4: the segment's
// first and last bytes are stored singly).
#include "pcnn_device.h"

#include "../../include/posecnn_hip_frontend.h"

namespace {

using namespace pcnn;

constexpr int NT = 32;                       // tile side
constexpr int NTHREADS = 256;
constexpr int MAX_D = 15;
constexpr int MAX_R = MAX_D / 2;
constexpr int MAX_SIDE = NT + 2 * MAX_R;
constexpr int ROW_SLOTS = NT * 3 / 4 + 1;    // dwords a 96-byte row segment can touch at any alignment
constexpr int SRC_DEPTH = 0, SRC_IMAGE = 1;

struct DepthArgs {
  const float* f32;        // [B,H,W] metres, or
  const uint16_t* u16;     // [B,H,W] raw / factor
  float factor;
  const float* intrinsics; // [B,4] fx, fy, cx, cy
  float cutoff;
};

struct Camera {
  float fx_inv, fy_inv, cx, cy;
};

__device__ __forceinline__ Camera camera_of(const DepthArgs& a, int b)
{
  const float* k = a.intrinsics + 4 * b;
  Camera c;
  c.fx_inv = div_rn(1.f, k[0]);
  c.fy_inv = div_rn(1.f, k[1]);
  c.cx = k[2];
  c.cy = k[3];
  return c;
}

__device__ __forceinline__ float nan_f() { return __int_as_float(0x7fffffff); }

__device__ __forceinline__ float depth_at(const DepthArgs& a, long long i)
{
  return a.f32 ? a.f32[i] : div_rn((float)a.u16[i], a.factor);
}

// computeVmapKernel's value at row u, column v
__device__ __forceinline__ void vertex_at(float z, int u, int v, const Camera& c, float cutoff, float p[3])
{
  if (z != 0.f && z < cutoff) {
    p[0] = (z * ((float)u - c.cx)) * c.fx_inv;
    p[1] = (z * ((float)v - c.cy)) * c.fy_inv;
    p[2] = z;
  } else {
    p[0] = p[1] = p[2] = nan_f();
  }
}

// computeNmapKernel's value at row u, column v of the frame that starts at pixel `frame`
__device__ __forceinline__ void normal_at(const DepthArgs& a, long long frame, int u, int v, int H, int W,
                                          const Camera& c, float n[3])
{
  n[0] = n[1] = n[2] = nan_f();
  if (u == H - 1 || v == W - 1) return;
  const long long i = frame + (long long)u * W + v;
  float p00[3], p01[3], p10[3];
  vertex_at(depth_at(a, i), u, v, c, a.cutoff, p00);
  vertex_at(depth_at(a, i + W), u + 1, v, c, a.cutoff, p01);
  vertex_at(depth_at(a, i + 1), u, v + 1, c, a.cutoff, p10);
  if (p00[0] != p00[0] || p01[0] != p01[0] || p10[0] != p10[0]) return;
  const float a0 = p01[0] - p00[0], a1 = p01[1] - p00[1], a2 = p01[2] - p00[2];
  const float b0 = p10[0] - p00[0], b1 = p10[1] - p00[1], b2 = p10[2] - p00[2];
  const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
  const float s2 = c0 * c0 + (c1 * c1 + c2 * c2);
  n[0] = c0;
  n[1] = c1;
  n[2] = c2;
  if (s2 > 0.f) {
    const float s = sqrt_rn(s2);
    n[0] = div_rn(c0, s);
    n[1] = div_rn(c1, s);
    n[2] = div_rn(c2, s);
  }
}

// (127.5 n + 127.5).astype(uint8): NaN -> 0, truncation toward zero
__device__ __forceinline__ uint32_t quantise(float n)
{
  float t = 127.5f * n;
  t = t + 127.5f;
  if (t != t) return 0u;
  return (uint32_t)(int)fminf(fmaxf(t, 0.f), 255.f);
}

// OpenCV's BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), any distance
__device__ __forceinline__ int reflect101(int p, int n)
{
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// grid ceil(B H W / 256)
__global__ __launch_bounds__(NTHREADS) void depth_normals_kernel(DepthArgs a, int H, int W, long long pixels,
                                                                  float* __restrict__ nmap)
{
  __shared__ float s[NTHREADS * 3];
  const int t = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * NTHREADS;
  const long long p = p0 + t;
  if (p < pixels) {
    const int HW = H * W;
    const int b = (int)(p / HW), rem = (int)(p - (long long)b * HW);
    const int u = rem / W, v = rem - u * W;
    float n[3];
    normal_at(a, (long long)b * HW, u, v, H, W, camera_of(a, b), n);
    s[3 * t] = n[0];
    s[3 * t + 1] = n[1];
    s[3 * t + 2] = n[2];
  }
  __syncthreads();
  const long long left = (pixels - p0) * 3;
  const int cnt = left < NTHREADS * 3 ? (int)left : NTHREADS * 3;
  for (int k = t; k < cnt; k += NTHREADS) nmap[p0 * 3 + k] = s[k];
}

struct Acc {
  float b, g, r, w;
};

__device__ __forceinline__ void tap(Acc& s, uint32_t q, uint32_t centre, float space, const float* cw)
{
  const float w = space * cw[__builtin_amdgcn_sad_u8(q, centre, 0u)];
  s.b = s.b + (float)(q & 0xffu) * w;
  s.g = s.g + (float)((q >> 8) & 0xffu) * w;
  s.r = s.r + (float)((q >> 16) & 0xffu) * w;
  s.w = s.w + w;
}

// grid (ceil(W / 32), ceil(H / 32), B). D: the filter's diameter when it is known at compile time, 0: `d` (0 = no filter)
template <int SRC, int D>
__global__ __launch_bounds__(NTHREADS) void tile_kernel(DepthArgs da, const uint8_t* __restrict__ src, int H, int W,
                                                         int d, const float* __restrict__ color_weight,
                                                         const float* __restrict__ space_weight,
                                                         uint8_t* __restrict__ dst)
{
  __shared__ uint32_t pix[MAX_SIDE * MAX_SIDE];
  __shared__ float cw[768];
  __shared__ float sw[MAX_D * MAX_D];
  __shared__ unsigned char outb[NT][NT * 3];
  const int t = threadIdx.x;
  const int r = D ? D / 2 : d / 2;
  const int side = NT + 2 * r;
  const int b = blockIdx.z, y0 = blockIdx.y * NT, x0 = blockIdx.x * NT;
  const int th = min(NT, H - y0), tw = min(NT, W - x0);
  const long long frame = (long long)b * H * W;

  if (D || d) {
    for (int k = t; k < 768; k += NTHREADS) cw[k] = color_weight[k];
    if (!D) {
      int taps = 0;
      for (int i = -r; i <= r; ++i)
        for (int j = -r; j <= r; ++j) taps += i * i + j * j <= r * r;
      for (int k = t; k < taps; k += NTHREADS) sw[k] = space_weight[k];
    }
  }

  // ---- the tile's source pixels + halo, packed (b, g, r, 0); only what the tile's live outputs read
  {
    Camera cam;
    if (SRC == SRC_DEPTH) cam = camera_of(da, b);
    const int fw = tw + 2 * r, fcount = (th + 2 * r) * fw;
    for (int k = t; k < fcount; k += NTHREADS) {
      const int ly = k / fw, lx = k - ly * fw;
      const int gy = reflect101(y0 - r + ly, H), gx = reflect101(x0 - r + lx, W);
      uint32_t q;
      if (SRC == SRC_DEPTH) {
        float n[3];
        normal_at(da, frame, gy, gx, H, W, cam, n);
        q = quantise(n[2]) | (quantise(n[1]) << 8) | (quantise(n[0]) << 16);   // channels (2, 1, 0)
      } else {
        const uint8_t* s = src + (frame + (long long)gy * W + gx) * 3;
        q = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
      }
      pix[ly * side + lx] = q;
    }
  }
  __syncthreads();

  // ---- filter: thread (ty, lx) owns the pixels (ty + 8 p, lx)
  const int lx = t & (NT - 1), ty = t / NT;
  for (int p = 0; p < NT / (NTHREADS / NT); ++p) {
    const int ly = ty + p * (NTHREADS / NT);
    if (ly >= th || lx >= tw) continue;
    const uint32_t* base = pix + (ly + r) * side + lx + r;
    const uint32_t centre = base[0];
    uint32_t ob = centre & 0xffu, og = (centre >> 8) & 0xffu, orr = (centre >> 16) & 0xffu;
    if (D || d) {
      Acc s = {0.f, 0.f, 0.f, 0.f};
      int k = 0;
      if (D) {
        constexpr int R = D / 2, S = NT + 2 * R;
#pragma unroll
        for (int i = -R; i <= R; ++i) {
#pragma unroll
          for (int j = -R; j <= R; ++j) {
            if (i * i + j * j <= R * R) {
              tap(s, base[i * S + j], centre, space_weight[k], cw);
              ++k;
            }
          }
        }
      } else {
        for (int i = -r; i <= r; ++i) {
          for (int j = -r; j <= r; ++j) {
            if (i * i + j * j <= r * r) {
              tap(s, base[i * side + j], centre, sw[k], cw);
              ++k;
            }
          }
        }
      }
      const float inv = div_rn(1.f, s.w);
      ob = (uint32_t)(int)__builtin_rintf(s.b * inv);
      og = (uint32_t)(int)__builtin_rintf(s.g * inv);
      orr = (uint32_t)(int)__builtin_rintf(s.r * inv);
    }
    outb[ly][3 * lx] = (unsigned char)ob;
    outb[ly][3 * lx + 1] = (unsigned char)og;
    outb[ly][3 * lx + 2] = (unsigned char)orr;
  }
  __syncthreads();

  // ---- store: per tile row the bytes [0, 3 tw) of its segment; slot k is the k-th aligned dword the segment touches
  const int rowbytes = 3 * tw;
  for (int s = t; s < th * ROW_SLOTS; s += NTHREADS) {
    const int ly = s / ROW_SLOTS, k = s - ly * ROW_SLOTS;
    uint8_t* g = dst + (frame + (long long)(y0 + ly) * W + x0) * 3;
    const int o = 4 * k - (int)(reinterpret_cast<uintptr_t>(g) & 3u);
    if (o >= rowbytes) continue;
    const unsigned char* ob = outb[ly];
    if (o >= 0 && o + 4 <= rowbytes) {
      *reinterpret_cast<uint32_t*>(g + o) =
          (uint32_t)ob[o] | ((uint32_t)ob[o + 1] << 8) | ((uint32_t)ob[o + 2] << 16) | ((uint32_t)ob[o + 3] << 24);
    } else {
      for (int q = 0; q < 4; ++q)
        if (o + q >= 0 && o + q < rowbytes) g[o + q] = ob[o + q];
    }
  }
}

int count_taps(int d)
{
  const int r = d / 2;
  int n = 0;
  for (int i = -r; i <= r; ++i)
    for (int j = -r; j <= r; ++j) n += i * i + j * j <= r * r;
  return n;
}

int check_frames(const char* who, int B, int H, int W)
{
  PCNN_REQUIRE(B >= 1 && B <= 65535, PCNN_EINVAL, "%s: 1 <= batch <= 65535", who);
  PCNN_REQUIRE(H >= 5 && W >= 5, PCNN_EINVAL, "%s: height and width must be at least 5 (got %d x %d)", who, H, W);
  PCNN_REQUIRE(H <= 65535 * NT, PCNN_EINVAL, "%s: height > %d (one grid row per %d image rows)", who, 65535 * NT, NT);
  PCNN_REQUIRE((long long)B * H * W <= (1ll << 30), PCNN_EINVAL, "%s: more than 2^30 pixels", who);
  return PCNN_OK;
}

int check_depth(const char* who, const float* f32, const uint16_t* u16, float factor, const float* intrinsics)
{
  PCNN_REQUIRE((f32 != nullptr) != (u16 != nullptr), PCNN_EINVAL, "%s: exactly one of depth_f32 and depth_u16 must be set",
               who);
  PCNN_REQUIRE(!u16 || factor > 0.f, PCNN_EINVAL, "%s: factor_depth must be positive", who);
  PCNN_REQUIRE(intrinsics, PCNN_ENULL, "%s: intrinsics is NULL", who);
  return PCNN_OK;
}

int check_filter(const char* who, int d, const float* color_weight, const float* space_weight, int num_taps)
{
  PCNN_REQUIRE(d >= 3 && d <= MAX_D && (d & 1), PCNN_EINVAL, "%s: d must be odd, 3 <= d <= %d (got %d)", who, MAX_D, d);
  PCNN_REQUIRE(num_taps == count_taps(d), PCNN_EINVAL, "%s: d = %d has %d taps (got num_taps = %d)", who, d,
               count_taps(d), num_taps);
  PCNN_REQUIRE(color_weight && space_weight, PCNN_ENULL, "%s: NULL weight table", who);
  return PCNN_OK;
}

template <int SRC>
void launch_tiles(const DepthArgs& da, const uint8_t* src, int B, int H, int W, int d, const float* color_weight,
                  const float* space_weight, uint8_t* dst, hipStream_t stream)
{
  const dim3 grid((W + NT - 1) / NT, (H + NT - 1) / NT, B);
  if (d == 9) {
    PCNN_LAUNCH((tile_kernel<SRC, 9>), grid, dim3(NTHREADS), 0, stream, da, src, H, W, d, color_weight, space_weight,
                dst);
  } else {
    PCNN_LAUNCH((tile_kernel<SRC, 0>), grid, dim3(NTHREADS), 0, stream, da, src, H, W, d, color_weight, space_weight,
                dst);
  }
}

}  // namespace

extern "C" int pcnn_depth_normals_fwd(const float* depth_f32, const uint16_t* depth_u16, float factor_depth,
                                      const float* intrinsics, int B, int H, int W, float depth_cutoff, float* nmap,
                                      void* stream_)
{
  if (int st = check_frames("depth_normals", B, H, W)) return st;
  if (int st = check_depth("depth_normals", depth_f32, depth_u16, factor_depth, intrinsics)) return st;
  PCNN_REQUIRE(nmap, PCNN_ENULL, "depth_normals: nmap is NULL");
  const DepthArgs da = {depth_f32, depth_u16, factor_depth, intrinsics, depth_cutoff};
  const long long pixels = (long long)B * H * W;
  PCNN_LAUNCH(depth_normals_kernel, dim3((unsigned)((pixels + NTHREADS - 1) / NTHREADS)), dim3(NTHREADS), 0,
              (hipStream_t)stream_, da, H, W, pixels, nmap);
  return check_launch("depth_normals_fwd");
}

extern "C" int pcnn_bilateral_u8c3_fwd(const uint8_t* src, int B, int H, int W, int d, const float* color_weight,
                                       const float* space_weight, int num_taps, uint8_t* dst, void* stream_)
{
  if (int st = check_frames("bilateral_u8c3", B, H, W)) return st;
  if (int st = check_filter("bilateral_u8c3", d, color_weight, space_weight, num_taps)) return st;
  PCNN_REQUIRE(src && dst, PCNN_ENULL, "bilateral_u8c3: NULL image");
  PCNN_REQUIRE(src != dst, PCNN_EINVAL, "bilateral_u8c3: dst must not alias src");
  const DepthArgs none = {nullptr, nullptr, 0.f, nullptr, 0.f};
  launch_tiles<SRC_IMAGE>(none, src, B, H, W, d, color_weight, space_weight, dst, (hipStream_t)stream_);
  return check_launch("bilateral_u8c3_fwd");
}

extern "C" int pcnn_normal_image_fwd(const float* depth_f32, const uint16_t* depth_u16, float factor_depth,
                                     const float* intrinsics, int B, int H, int W, float depth_cutoff, int d,
                                     const float* color_weight, const float* space_weight, int num_taps,
                                     uint8_t* image, void* stream_)
{
  if (int st = check_frames("normal_image", B, H, W)) return st;
  if (int st = check_depth("normal_image", depth_f32, depth_u16, factor_depth, intrinsics)) return st;
  if (d != 0) {
    if (int st = check_filter("normal_image", d, color_weight, space_weight, num_taps)) return st;
  }
  PCNN_REQUIRE(image, PCNN_ENULL, "normal_image: image is NULL");
  const DepthArgs da = {depth_f32, depth_u16, factor_depth, intrinsics, depth_cutoff};
  launch_tiles<SRC_DEPTH>(da, nullptr, B, H, W, d, color_weight, space_weight, image, (hipStream_t)stream_);
  return check_launch("normal_image_fwd");
}
