/*
 * posecnn_hip_pose3d.h — the 3-D vertex route's pose stage in libposecnn_hip.so: `Synthesizer::estimatePose3D`
 * (lib/synthesize/synthesize.cpp:1769-1966) as three launches per batch — preemptive RANSAC with a Kabsch fit over
 * (object point, camera point) pairs, one rigid pose per (frame, class). Status codes and conventions are those of
 * posecnn_hip.h; the ABI version is that header's. tests/pose3d_ref.py restates every step in numpy, bit for bit.
 *
 * Arithmetic. One IEEE rounding per operation, no fused multiply-add, divide and sqrt correctly rounded; sums are written
 * left to right unless parenthesised.
 *
 * PREPARE (p3d_prepare, one workgroup per frame). For every pixel p = y W + x whose label c is in [1, C) one record
 * (eye xyz, obj xyz), six f32:
 *     eye = (0, 0, 0) when depth d == 0, else  ((float)x - px) (float)d / fx / factor,  ((float)y - py) (float)d / fy / factor,
 *           (float)d / factor                                                                                        (f32)
 *     obj_i = (v_i - b_i) / a_i,  v_i = vertex_pred[p][3c + i],  vmax = extent_i / 2, vmin = -extent_i / 2 (f32),
 *           a_i = (float)(1.0 / (double)(vmax - vmin)),  b_i = (float)(-1.0 (double)vmin / (double)(vmax - vmin))
 * Records are compacted per (frame, class) in ascending p: class c of frame b owns records[b][offsets[b][c] ..
 * + counts[b][c]); offsets is the exclusive scan of counts in class order, counts[b][0] = 0. Labels outside [0, C) are
 * background. records beyond the frame's total are not touched.
 *
 * SAMPLE (p3d_sample, one thread per (frame, h)). live = the classes with counts > min_area, ascending. Attempt
 * a = 0 .. max_attempts - 1 draws the Philox4x64-10 block of counter (a, streams[b], h, 0) under key (seed0, seed1);
 * idx(w, n) = ((w >> 32) n) >> 32. c = live[idx(w0, |live|)], records j_i = idx(w_{1+i}, counts[c]), i = 0, 1, 2.
 * The attempt is refused when, for some i: eye_i.z == 0; or dist(eye_i, eye_k) < (double)min_dist for a k < i; or
 * obj_i == (0, 0, 0); or dist(obj_i, obj_k) < (double)min_dist for a k < i, where dist takes the f32 differences, widens
 * them and forms sqrt(dx dx + dy dy + dz dz) in f64. Then FIT over the three pairs (sums in the order 0, 1, 2); refused
 * when a pair's RESIDUAL is not < (double)inlier_threshold; then the box: corners (sx hx, sy hy, sz hz), h = extent 0.5f
 * widened, q = R corner + t; refused when a q.z <= 0; u = (double)fx q.x / q.z + (double)px, v likewise, each held in
 * [0, W - 1] / [0, H - 1] and truncated; with min starting at W - 1 (H - 1) and max at 0 the area
 * (maxX - minX + 1)(maxY - minY + 1) must be >= min_area. The first attempt not refused is the hypothesis:
 * hyp_pose = R|t (row-major 3 x 4, f64), hyp_class = c, hyp_attempt = a, hyp_rec = (j_0, j_1, j_2). Without one (or with
 * no live class): zeros, class 0, attempt -1, records -1.
 *
 * RESIDUAL(P, record), f64: q_i = P_i0 ox + P_i1 oy + P_i2 oz + P_i3;  d_i = e_i - q_i;  sqrt(d_0 d_0 + d_1 d_1 + d_2 d_2).
 *
 * FIT(n; Sa, Sb, Sab) (a = obj, b = eye; Sa_i = sum a_i, Sb_j = sum b_j, Sab_ij = sum a_i b_j, f64), Horn's closed form:
 *     cA = Sa / n, cB = Sb / n, M_ij = Sab_ij - Sa_i cB_j;
 *     N = [ (Mxx + Myy) + Mzz, Myz - Mzy, Mzx - Mxz, Mxy - Myx;  . , (Mxx - Myy) - Mzz, Mxy + Myx, Mzx + Mxz;
 *           . , . , (Myy - Mxx) - Mzz, Myz + Mzy;  . , . , . , (Mzz - Mxx) - Myy ], symmetric;
 *     PCNN_POSE3D_JACOBI_SWEEPS cyclic Jacobi sweeps over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) on A = N, V = I:
 *       t = 0 when A_pq == 0, else theta = (A_qq - A_pp) / (2 A_pq), t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1));
 *       c = 1 / sqrt(t t + 1), s = t c; then for k = 0..3 the columns (A_kp, A_kq) <- (c A_kp - s A_kq, s A_kp + c A_kq), then
 *       for k = 0..3 the rows (A_pk, A_qk) likewise, then V's columns likewise;
 *     (w, x, y, z) = the column of V under the largest A_ii (the first such), divided by sqrt(w w + x x + y y + z z);
 *     R = [1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy);  2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx);
 *          2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)];   t_i = cB_i - (R_i0 cA_0 + R_i1 cA_1 + R_i2 cA_2).
 *
 * RANSAC (p3d_ransac, one workgroup per (frame, class), no communication between workgroups). The class's hypotheses in
 * ascending h, size of them, n = counts. round = 0, ref_steps = 0; while size > 1 or ref_steps < ref_it:
 *   1. round += 1, m = min(n, pixel_batch round); the subset is records floor(k n / m), k = 0 .. m - 1;
 *   2. inliers(h) = the subset records with eye.z != 0 and RESIDUAL(pose_h) < (double)inlier_threshold;
 *   3. when size > 1: order by inliers descending, then h ascending; keep the first size / 2;
 *   4. every survivor with >= 4 inliers is refitted on its inlier list (subset order), thinned when it has
 *      cnt >= max_pixels entries to those of rank floor(j cnt / max_pixels), j = 0 .. max_pixels - 1. Sum order of the fit:
 *      subset position k belongs to lane k mod 64, a lane adds its chosen pairs in ascending k onto +0, and the 64 lane sums
 *      are folded by v_l <- v_l + v_(l xor s), s = 32, 16, 8, 4, 2, 1; ref_steps += 1 (also without a refit).
 * Per (frame, class): poses64 = the last survivor's R|t, poses32 the same rounded to f32, inliers = its last count,
 * ref_steps, num_hyps = the hypotheses the class received. Everything is zero for class 0 and a class without hypothesis.
 *
 * pcnn_pose3d_round_fwd runs steps 1-4 ONCE, for the given `round`, on caller-given hypotheses (hyp_class outside
 * [1, C): not a hypothesis) and writes every slot: pose_out (the refitted or unchanged pose), class_out (the class, 0 when
 * dropped in step 3 or not a hypothesis), inliers_out. pcnn_pose3d_estimate_fwd is prepare, sample, ransac on one stream
 * with no host synchronisation.
 *
 * All pointers are DEVICE pointers; label int32 [B,H,W], depth uint16 [B,H,W], vertex_pred f32 [B,H,W,3C] (4-byte
 * aligned is enough), extents f32 [C,3], intrinsics f32 [B,4] rows (fx, fy, px, py), streams uint64 [B].
 * Validation, on the host before any launch: 1 <= B <= 65535, H, W >= 1, H W <= 2^24, 2 <= C <= 64,
 * 1 <= hypotheses <= PCNN_POSE3D_MAX_HYPOTHESES, max_attempts, pixel_batch, max_pixels, round >= 1 (pixel_batch round
 * < 2^31), ref_it, min_area >= 0, factor_depth, inlier_threshold, min_dist finite (factor_depth != 0) -> PCNN_EINVAL;
 * NULL pointer -> PCNN_ENULL; short workspace -> PCNN_EWORKSPACE. Only the driver needs a workspace.
 */
#ifndef POSECNN_HIP_POSE3D_H
#define POSECNN_HIP_POSE3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_POSE3D_MAX_HYPOTHESES 1024
#define PCNN_POSE3D_JACOBI_SWEEPS 8
#define PCNN_POSE3D_RECORD 6

int pcnn_pose3d_workspace_bytes(int B, int H, int W, int C, int hypotheses, size_t* bytes);

int pcnn_pose3d_prepare_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred, const float* extents,
                            const float* intrinsics, float factor_depth, int B, int H, int W, int C, float* records,
                            int32_t* counts, int32_t* offsets, void* stream);

int pcnn_pose3d_sample_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                           const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B, int H,
                           int W, int C, int hypotheses, int max_attempts, int min_area, float inlier_threshold,
                           float min_dist, double* hyp_pose, int32_t* hyp_class, int32_t* hyp_attempt, int32_t* hyp_rec,
                           void* stream);

int pcnn_pose3d_round_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const double* hyp_pose,
                          const int32_t* hyp_class, int B, int H, int W, int C, int hypotheses, int round, int pixel_batch,
                          int max_pixels, float inlier_threshold, double* pose_out, int32_t* class_out,
                          int32_t* inliers_out, void* stream);

int pcnn_pose3d_estimate_fwd(const int32_t* label, const uint16_t* depth, const float* vertex_pred, const float* extents,
                             const float* intrinsics, const uint64_t* streams, float factor_depth, uint64_t seed0,
                             uint64_t seed1, int B, int H, int W, int C, int hypotheses, int pixel_batch, int max_pixels,
                             int ref_it, int min_area, float inlier_threshold, float min_dist, int max_attempts,
                             double* poses64, float* poses32, int32_t* inliers, int32_t* ref_steps, int32_t* num_hyps,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
