/*
 * posecnn_hip_augment.h — training augmentation entries of libposecnn_hip.so: `chromatic_transform` and `add_noise`
 * (lib/utils/blob.py:74-129) in the order of lib/gt_synthesize_layer/minibatch.py:170-201, as one kernel that turns a
 * batch's raw frames into the network's `data` / `data_p` input blobs. The random flip is not here (the followed
 * configuration, experiments/cfgs/lov_color_2d.yml:19-21, turns it off), nor is chromatic_transform's `label` mask (no
 * caller passes it). Status codes and conventions are those of posecnn_hip.h; the ABI version is that header's.
 *
 * Inputs
 *   color        uint8  [B,H,W,C]  BGR, C = 3 or 4; with C = 4 the fourth byte is ignored          (DEVICE, 16-byte aligned)
 *   depth        uint16 [B,H,W]    raw, or NULL: no depth plane, data_p is not touched               (DEVICE, 16-byte aligned)
 *   params       double [B][PCNN_AUGMENT_ROW]  one HOST row per frame; it travels as kernel arguments, PCNN_AUGMENT_LAUNCH_FRAMES
 *                frames per launch, so no host buffer has to outlast the call and the call is safe under stream capture:
 *                  [0] d_h  [1] d_l  [2] d_s      the frame's jitter, finite, |d_h| <= 90
 *                  [3] colour mode                 0 none, 1 Gaussian, 2 horizontal blur, 3 vertical blur
 *                  [4] sigma (mode 1, >= 0, used as (float)sigma) or size (modes 2, 3: one of 3 5 7 9 11 15); ignored in mode 0
 *                  [5] colour stream id            an integer in [0, 2^53)
 *                  [6] chromatic                   0: the bytes pass through untouched; 1: the HLS round trip below, which
 *                                                  is NOT the identity at zero jitter
 *                  [7] depth mode  [8] depth sigma or size  [9] depth stream id      (read only when depth is given)
 *   pixel_means  double [3]        HOST; subtracted per channel, as the raw-frame entries of posecnn_hip.h take it
 *   seed0, seed1                   the 128-bit Philox key
 *   depth_norm   0: the frame's own maximum (minibatch.py:189), found on the device by one small kernel (one workgroup per
 *                   frame) without a host synchronisation; an all-zero frame divides 0 by 0 and every element of its
 *                   data_p is NaN, as numpy's is (the NaN's sign and payload are not specified)
 *                1: clip(d / 2000, 0, 1) 255, what the raw-frame kernels of posecnn_hip.h form
 * Outputs (DEVICE, 16-byte aligned, every element written)
 *   data         f32 [B,H,W,3]
 *   data_p       f32 [B,H,W,3]     when depth is given
 * Workspace: pcnn_augment_frames_workspace_bytes (4 bytes per frame with a depth plane and depth_norm = 0, else 0 — then
 * `workspace` may be NULL); 16-byte aligned.
 *
 * Validation, all on the host before any launch: B >= 1, H >= 8, W >= 8 (a blur's radius of up to 7 stays inside
 * reflect-101), B H W <= 2^30, C in {3, 4}, depth_norm in {0, 1}, the row conditions above -> PCNN_EINVAL; a NULL
 * color, params, pixel_means, data, or data_p with a depth plane -> PCNN_ENULL; a short workspace -> PCNN_EWORKSPACE.
 *
 * Arithmetic. One IEEE rounding per operation, no fused multiply-add, divide and sqrt correctly rounded; "f32" and "f64"
 * name the format every operand and result of a step has. tests/augment_ref.py restates it in numpy.
 *
 * 1. BGR -> 8-bit HLS (the published 8-bit algorithm of OpenCV's cvtColor documentation), f32:
 *      c = (float)byte * k255, k255 = (float)(1.0 / 255.0), for b, g, r;  vmax, vmin = the largest and smallest of the three;
 *      sum = vmax + vmin;  l = sum * 0.5f;  diff = vmax - vmin;
 *      diff == 0: h = s = 0; otherwise
 *        s = diff / (l < 0.5f ? sum : (2.f - vmax) - vmin);  q = 60.f / diff;
 *        h = (g - b) q            if vmax == r, else
 *            (b - r) q + 120.f    if vmax == g, else
 *            (r - g) q + 240.f;   h = h + 360.f if h < 0;
 *      H8 = rint(h * 0.5f), L8 = rint(l * 255.f), S8 = rint(s * 255.f): half to even, held in [0, 255]. H8 is in [0, 180].
 * 2. Jitter, f64, as numpy does it: x = (double)H8 + d_h; x = x - 180 if x >= 180, x = x + 180 if x < 0 (np.mod(x, 180)
 *    for |d_h| <= 90; a tiny negative x gives exactly 180); y = min(max((double)L8 + d_l, 0), 255), z likewise with S8 and
 *    d_s; the three are truncated toward zero to bytes H', L', S'.
 * 3. 8-bit HLS -> BGR (the two-parameter sector form), f32: l = (float)L' * k255, s = (float)S' * k255;
 *      S' == 0: b = g = r = l; otherwise
 *        p2 = l <= 0.5f ? l * (1.f + s) : (l + s) - l * s;  p1 = 2.f * l - p2;  d = p2 - p1;
 *        sector = H' / 30 (integer; 6 counts as 0), f = (float)(H' - 30 sector) * (float)(1.0 / 30.0);
 *        up = p1 + d * f;  down = p1 + d * (1.f - f);
 *        (r, g, b) = (p2, up, p1), (down, p2, p1), (p1, p2, up), (p1, down, p2), (up, p1, p2), (p2, p1, down) for sector 0..5;
 *      byte = rint(c * 255.f), half to even, held in [0, 255].
 *    OpenCV's own bytes are not pinned: its 8-bit HLS code is a fixed-point / vectorised variant of the same formulas.
 * 4. Depth value, f32: depth_norm 0: ((float)d / (float)max) * 255.f; depth_norm 1: t = (float)d / 2000.f held in [0, 1],
 *    t * 255.f. One value per pixel stands for the three tiled channels.
 * 5. Noise, per plane (plane 0 = colour on the bytes of step 3 or, chromatic off, the input bytes; plane 1 = depth on the
 *    value of step 4):
 *    mode 0: v = (float)byte, or the depth value.
 *    mode 1: generator Philox4x64-10 with the constants of np.random.Philox (multipliers 0xD2E7470EE14C6C93,
 *      0xCA5A826395121157; key increments 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B). Pixel p = y W + x of a frame uses the
 *      64-bit output word p & 3 of the block with counter (p >> 2, stream id, plane, 0) and key (seed0, seed1). (numpy
 *      increments the counter before it generates: np.random.Philox(counter=c, key=k).random_raw(4) is the block of
 *      counter c + 1.) With hi = word >> 32, lo = word & 0xffffffff:
 *        u1 = (float)((hi >> 8) + 1) * 2^-24 in (0, 1];  u2 = (float)(lo >> 8) * 2^-24 in [0, 1), both exact;
 *        g = sqrt(-2.f * log(u1)) * cos((float)(2 pi) * u2), every step f32 (log and cos are the device library's);
 *        v = (float)byte + sigma * g per channel with the one g (or depth value + sigma * g), held in [0, 255] by
 *        v < 0 ? 0 : v > 255 ? 255 : v, which keeps a NaN. |g| <= sqrt(48 ln 2) = 5.77.
 *      The stream id comes from the row, never from the frame's position in the batch.
 *    modes 2, 3: k = (float)(1.0 / size), r = size / 2; acc = 0.f; for i = -r .. r in ascending order
 *      acc = acc + value(x + i, y) * k (mode 2) or value(x, y + i) * k (mode 3), coordinates reflected (reflect-101:
 *      -1 -> 1, n -> n - 2). Colour: value = (float)byte per channel and v = rint(acc), half to even, held in [0, 255];
 *      depth: v = acc, not rounded.
 * 6. out_c = (float)((double)v - pixel_means[c]).
 */
#ifndef POSECNN_HIP_AUGMENT_H_
#define POSECNN_HIP_AUGMENT_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_AUGMENT_ROW 10
#define PCNN_AUGMENT_LAUNCH_FRAMES 32

int pcnn_augment_frames_workspace_bytes(int batch, int has_depth, int depth_norm, size_t* bytes);

int pcnn_augment_frames_fwd(const uint8_t* color, int channels, const uint16_t* depth, const double* params,
                            const double* pixel_means, uint64_t seed0, uint64_t seed1, int depth_norm, int batch,
                            int height, int width, float* data, float* data_p, void* workspace, size_t workspace_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_AUGMENT_H_ */
