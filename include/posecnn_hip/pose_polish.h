/*
 * posecnn_hip/pose_polish.h — the last step of both pose routes of the 3-D vertex route in libposecnn_hip.so: the
 * Nelder-Mead polish `refineWithOpt` (lib/synthesize/synthesize.cpp:1510-1567, objectives optEnergy3D / optEnergy2D
 * :1427-1507, called at :1737-1745 and :1936-1944) as ONE launch per batch, one problem per (frame, class). Status codes
 * and conventions are those of posecnn_hip.h; the ABI version is that header's. The record layout, RESIDUAL, the fold order
 * and the thinning rule are those of posecnn_hip_pose3d.h, REPROJ and the retraction those of posecnn_hip_pose2d.h; they
 * are not repeated here. tests/pose_polish_ref.py restates every step in numpy, bit for bit.
 *
 * Arithmetic. One IEEE rounding per operation, no fused multiply-add, divide and sqrt correctly rounded; sums and products
 * are written left to right unless parenthesised; f64 throughout, only + - x / sqrt and comparisons.
 *
 * LIST. n = counts[b][c], the class's records in record order. With P0 = poses_in[b][c] the inliers are, route 0 (depth):
 * eye.z != 0 and RESIDUAL(P0, record) < (double)inlier_threshold; route 1 (colour): q.z > 0 and REPROJ(P0, record) <
 * (double)inlier_threshold. cnt of them; the list is all of them when cnt < max_pixels, else those of rank
 * floor(j cnt / max_pixels), j = 0 .. max_pixels - 1; L = min(cnt, max_pixels) its length, position j its order. The list
 * is fixed for the whole polish.
 *
 * GATE. The class is polished when c >= 1, evaluations >= 7, gate[b][c] > min_pixels and L > 0. Otherwise
 * poses64 = poses_in (copied), poses32 the same rounded, energy = (0, 0), evals = 0, listed = 0.
 *
 * UNKNOWNS. x = (w0, w1, w2, t0, t1, t2). P(x): h = 0.5 (x0, x1, x2), n = sqrt(((1 + hx hx) + hy hy) + hz hz),
 * (w, x, y, z) = (1 / n, hx / n, hy / n, hz / n), Q the rotation of FIT's quaternion formula, R_ij = (Q_i0 R0_0j + Q_i1 R0_1j)
 * + Q_i2 R0_2j, t_i = t0_i + x_(3+i): the retraction of the colour route's refit applied to P0. Box: lb = -r, ub = r with
 * r = (PCNN_POSE_POLISH_BOX_ROT x 3, PCNN_POSE_POLISH_BOX_XY x 2, PCNN_POSE_POLISH_BOX_Z); start x0 = 0.
 *
 * ENERGY E(x). P = P(x); d_j = RESIDUAL(P, list_j) (route 0) or the distance of REPROJ(P, list_j) (route 1); list position
 * j belongs to lane j mod 64, a lane adds its d_j in ascending j onto +0, the 64 lane sums are folded by the xor butterfly
 * 32 .. 1, the sum is divided by (double)L. Route 1: +inf when a listed point has q.z <= 0 under P. +inf when the value is
 * not finite.
 *
 * OPTIMISER: the published Nelder-Mead of nlopt's nldrmd (Box's bound handling by clamping; alpha 1, beta 0.5, gamma 2,
 * delta 0.5), N = 6, restated — not its code, not its bits.
 *   vertex 0 = x0, vertex k = x0 with coordinate k - 1 replaced by x0_(k-1) + (ub_(k-1) - lb_(k-1)) 0.25, k = 1 .. 6;
 *   f_k = E(vertex k) in that order: 7 evaluations. While evals < evaluations:
 *     lo = hi = 0; for k = 1 .. 6: f_k < f_lo -> lo = k; f_k >= f_hi -> hi = k. nh: over k = 0 .. 6, k != hi, the first k,
 *     replaced by every later k with f_k >= f_nh.
 *     c_i = (sum over k != hi, ascending, onto +0, of vertex_k,i) / 6;
 *     point(coef)_i = c_i + coef (c_i - vertex_hi,i), then raised to lb_i when below it, then lowered to ub_i when above;
 *     xr = point(1), fr = E(xr).
 *     fr < f_lo:   when evals < evaluations: xe = point(2), fe = E(xe); hi <- (xe, fe) when fe < fr, else (xr, fr);
 *                  otherwise hi <- (xr, fr).
 *     else fr < f_nh:  hi <- (xr, fr).
 *     else: when evals >= evaluations: hi <- (xr, fr) when fr < f_hi; stop. xc = point(0.5) when fr < f_hi, else
 *                  point(-0.5); fc = E(xc); hi <- (xc, fc) when fc < min(fr, f_hi) (fr when fr < f_hi, else f_hi); otherwise
 *                  shrink: for k = 0 .. 6, k != lo, while evals < evaluations:
 *                  vertex_k,i <- vertex_lo,i + 0.5 (vertex_k,i - vertex_lo,i), f_k = E(vertex k).
 *   Every E() counts one evaluation; the loop ends at exactly `evaluations` of them, there is no tolerance.
 *   Result: the vertex xb with the smallest f (the first on a tie): poses64 = P(xb), poses32 the same rounded,
 *   energy = (f_0 of the initial simplex = E(x0), f of xb), evals = the evaluations made, listed = L.
 *   x0 is a vertex of the initial simplex and `<` never takes a worse point: energy[1] <= energy[0].
 *
 * Deviation from the reference: it bounds an absolute Rodrigues vector and translation around their
 * start, which needs sin / cos; here the unknowns are a local update of the start pose in + - x / sqrt only.
 *
 * EXECUTION. One wave of 64 lanes per (frame, class), no barrier, no communication between waves; every loop bound is
 * computable from the arguments. The list is compacted once by ballot rank: into LDS when
 * max_pixels <= PCNN_POSE_POLISH_LDS_RECORDS, else into the workspace (pcnn_pose_polish_workspace_bytes; 16 bytes, unused,
 * in the first case). Every lane repeats the simplex bookkeeping on identical bits.
 *
 * pcnn_pose_polish_fwd polishes caller-given poses on caller-given prepared records (pcnn_pose3d_prepare_fwd /
 * pcnn_pose2d_prepare_fwd); poses64 may be poses_in (in place). `gate` is the `inliers` output of an estimate entry.
 * pcnn_pose3d_estimate_polished_fwd / pcnn_pose2d_estimate_polished_fwd take the arguments of pcnn_pose3d_estimate_fwd /
 * pcnn_pose2d_estimate_fwd plus min_pixels, evaluations and the three polish outputs: prepare, sample, ransac and polish
 * (in place on poses64, gate = inliers, the estimate's max_pixels and inlier_threshold) on one stream with no host
 * synchronisation. With evaluations == 0 they are the existing drivers: no fourth launch, energy / evals / listed are not
 * written and may be NULL.
 *
 * All pointers are DEVICE pointers: records f32 [B,H W,6] (8-byte aligned), counts, offsets int32 [B,C], intrinsics f32
 * [B,4] (route 1; may be NULL for route 0), poses_in f64 [B,C,3,4], gate int32 [B,C], poses64 f64 [B,C,3,4], poses32 f32
 * [B,C,3,4], energy f64 [B,C,2], evals, listed int32 [B,C].
 * Validation, on the host before any launch: route in {0, 1}; evaluations == 0 or 7 <= evaluations <=
 * PCNN_POSE_POLISH_MAX_EVALUATIONS; max_pixels >= 1; min_pixels >= 0; inlier_threshold finite; B, H, W, C as in
 * posecnn_hip_pose3d.h -> PCNN_EINVAL; NULL pointer -> PCNN_ENULL; short workspace -> PCNN_EWORKSPACE.
 */
#ifndef POSECNN_HIP_POSE_POLISH_H
#define POSECNN_HIP_POSE_POLISH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_POSE_POLISH_MAX_EVALUATIONS 4096
#define PCNN_POSE_POLISH_LDS_RECORDS 1024
#define PCNN_POSE_POLISH_BOX_ROT 0.17453292519943295 /* 10 pi / 180 */
#define PCNN_POSE_POLISH_BOX_XY 0.1
#define PCNN_POSE_POLISH_BOX_Z 0.5

int pcnn_pose_polish_workspace_bytes(int B, int C, int max_pixels, size_t* bytes);

int pcnn_pose_polish_fwd(int route, const float* records, const int32_t* counts, const int32_t* offsets,
                         const float* intrinsics, const double* poses_in, const int32_t* gate, int B, int H, int W, int C,
                         int max_pixels, int min_pixels, int evaluations, float inlier_threshold, double* poses64,
                         float* poses32, double* energy, int32_t* evals, int32_t* listed, void* workspace,
                         size_t workspace_bytes, void* stream);

int pcnn_pose3d_estimate_polished_workspace_bytes(int B, int H, int W, int C, int hypotheses, int max_pixels, size_t* bytes);

int pcnn_pose3d_estimate_polished_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred,
                                      const float* extents, const float* intrinsics, const uint64_t* streams,
                                      float factor_depth, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                                      int hypotheses, int pixel_batch, int max_pixels, int ref_it, int min_area,
                                      float inlier_threshold, float min_dist, int max_attempts, int min_pixels,
                                      int evaluations, double* poses64, float* poses32, int32_t* inliers, int32_t* ref_steps,
                                      int32_t* num_hyps, double* energy, int32_t* evals, int32_t* listed, void* workspace,
                                      size_t workspace_bytes, void* stream);

int pcnn_pose2d_estimate_polished_workspace_bytes(int B, int H, int W, int C, int hypotheses, int max_pixels, size_t* bytes);

int pcnn_pose2d_estimate_polished_fwd(const int32_t* label, const float* vertex_pred, const float* extents,
                                      const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B,
                                      int H, int W, int C, int hypotheses, int pixel_batch, int max_pixels, int ref_it,
                                      int min_area, float inlier_threshold, float min_dist2d, float min_dist3d,
                                      int max_attempts, int min_pixels, int evaluations, double* poses64, float* poses32,
                                      int32_t* inliers, int32_t* ref_steps, int32_t* num_hyps, double* energy, int32_t* evals,
                                      int32_t* listed, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
