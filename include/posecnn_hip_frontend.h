/*
 * posecnn_hip_frontend.h — input front-end entries of libposecnn_hip.so: the surface-normal image the reference feeds
 * the network under cfg.INPUT = 'NORMAL' (lib/fcn/test.py:80-101) formed on the device from the depth frame:
 *     depth / factor_depth -> gpu_normals (lib/normals/compute_normals.cu:30-101) -> 127.5 n + 127.5 as uint8 ->
 *     channels (2, 1, 0) -> cv2.bilateralFilter(im, 9, 75, 75)
 * Status codes and conventions are those of posecnn_hip.h; the ABI version is that header's.
 *
 * Inputs common to the entries that take a depth frame
 *   depth_f32   f32    [B,H,W]  metres                          \  exactly one of the two is non-NULL
 *   depth_u16   uint16 [B,H,W]  raw; z = (float)d / factor_depth /  (one f32 division: numpy's astype(f32) / float(f))
 *   intrinsics  f32    [B,4]    rows (fx, fy, cx, cy), on the device; 1.f / fx and 1.f / fy are formed by the kernel
 *   depth_cutoff                the reference passes 20.0
 *   B >= 1, H >= 5, W >= 5; anything else is PCNN_EINVAL before any launch.
 *
 * Normal map (u = row, v = column; every operation one IEEE f32 rounding, divide and sqrt correctly rounded):
 *   vertex(u, v) = ((z (u - cx)) fx_inv, (z (v - cy)) fy_inv, z) if z != 0 && z < cutoff, else NaN — the row goes with
 *   cx and the column with cy, the reference's own pairing. The last row and the last column are NaN; elsewhere NaN
 *   unless the x components of the pixel's vertex, of its lower neighbour's (u+1, v) and of its right neighbour's
 *   (u, v+1) are all numbers. Otherwise a = lower - centre, b = right - centre,
 *   c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), s2 = c0 c0 + (c1 c1 + c2 c2), n = c / sqrt(s2) per component
 *   if s2 > 0, else c. A NaN output carries the bits 0x7fffffff.
 *
 * Quantised image: per component t = 127.5f n, t = t + 127.5f; NaN -> 0, otherwise truncated toward zero (and held in
 * [0, 255]); byte order (n_z, n_y, n_x).
 *
 * Bilateral filter (the published scalar 8-bit 3-channel algorithm of OpenCV's bilateralFilter): d odd, 3 <= d <= 15,
 * r = d / 2, border reflect-101. Taps (i, j) in [-r, r]^2, i outer, j inner, kept when i i + j j <= r r (49 at d = 9).
 *   color_weight f32 [768]  entry i = (float)exp(i i (-0.5 / sigma_color^2)), evaluated in float64, on the device
 *   space_weight f32 [K]    entry k = (float)exp(rho rho (-0.5 / sigma_space^2)), rho = sqrt((double)(i i + j j)) of tap k
 * Per pixel, taps in that order, all f32: w = space_weight[k] * color_weight[|b-b0| + |g-g0| + |r-r0|];
 * sum_c = sum_c + (float)c_k * w; wsum = wsum + w; then inv = 1.f / wsum, out_c = sum_c * inv rounded half to even.
 * num_taps must be the K of d (PCNN_EINVAL otherwise).
 */
#ifndef POSECNN_HIP_FRONTEND_H_
#define POSECNN_HIP_FRONTEND_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nmap f32 [B,H,W,3]: every element is written. The vertex map never exists in memory. */
int pcnn_depth_normals_fwd(const float* depth_f32, const uint16_t* depth_u16, float factor_depth,
                           const float* intrinsics, int batch, int height, int width, float depth_cutoff,
                           float* nmap, void* stream);

/* src, dst uint8 [B,H,W,3] (dst must not alias src): every byte of dst is written. */
int pcnn_bilateral_u8c3_fwd(const uint8_t* src, int batch, int height, int width, int d, const float* color_weight,
                            const float* space_weight, int num_taps, uint8_t* dst, void* stream);

/* image uint8 [B,H,W,3] = bilateral(quantise(normals(depth))) in one kernel: neither the normal map nor the
 * unfiltered image is stored. d = 0: no filter (the tables may be NULL, num_taps 0), image = the quantised image. */
int pcnn_normal_image_fwd(const float* depth_f32, const uint16_t* depth_u16, float factor_depth,
                          const float* intrinsics, int batch, int height, int width, float depth_cutoff, int d,
                          const float* color_weight, const float* space_weight, int num_taps, uint8_t* image,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_FRONTEND_H_ */
