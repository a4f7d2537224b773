/*
 * posecnn_hip_pose2d.h — the colour-only pose stage of the 3-D vertex route in libposecnn_hip.so:
 * `Synthesizer::estimatePose2D` (lib/synthesize/synthesize.cpp:1571-1767) as three launches per batch — preemptive RANSAC
 * over (object point, pixel) pairs with a closed-form P3P sampler and a Gauss-Newton refit, one rigid pose per
 * (frame, class), no depth frame. Status codes and conventions are those of posecnn_hip.h; the ABI version is that
 * header's. The record layout, Philox block, idx(), FIT, the projected box, the loop of RANSAC and the fold order are
 * those of posecnn_hip_pose3d.h and are not repeated here. tests/pose2d_ref.py restates every step in numpy, bit for bit.
 *
 * Arithmetic. One IEEE rounding per operation, no fused multiply-add, divide and sqrt correctly rounded; sums and products
 * are written left to right unless parenthesised. In f64 only + - x / sqrt, comparisons and fixed iteration counts: no
 * transcendental function anywhere. f32 inputs are widened before use unless said otherwise.
 *
 * PREPARE (one workgroup per frame). For every pixel p = y W + x whose label c is in [1, C) one record of
 * PCNN_POSE2D_RECORD f32: ((float)x, (float)y, 0, obj xyz), obj_i = (v_i - b_i) / a_i with a_i, b_i exactly as in the depth
 * route. Compaction per (frame, class) in ascending p, counts, offsets and the background rule as there. No depth is read.
 *
 * SAMPLE (one thread per (frame, h)). live, the block of counter (a, streams[b], h, 0) and idx() as in the depth route.
 * c = live[idx(w0, |live|)]; records j_i = idx(w_{1+i}, counts[c]) for i = 0, 1, 2 and j_3 = ((w0 & 0xFFFFFFFF) counts[c]) >> 32.
 * The attempt is refused when, for some i: obj_i == (0, 0, 0); or dist2(pix_i, pix_k) < (double)min_dist2d for a k < i; or
 * dist(obj_i, obj_k) < (double)min_dist3d for a k < i (dist, dist2: f32 differences, widened, sqrt(dx dx + dy dy [+ dz dz]));
 * or LINE(obj_i, obj_j, obj_k) < (double)min_dist3d for (i, j, k) in (0,1,2) (0,1,3) (0,2,3) (1,2,3), where with the f32
 * differences a = p_j - p_i, b = p_k - p_i widened, c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
 * LINE = sqrt((c0 c0 + c1 c1) + c2 c2) / sqrt((a0 a0 + a1 a1) + a2 a2). A NaN never refuses here; it is refused below.
 *
 * P3P on pairs 0, 1, 2 (Grunert's form; 1-based in the formulas: pair i - 1). Bearings: bx = (x - px) / fx, by = (y - py) / fy,
 * n = sqrt((bx bx + by by) + 1), f = (bx / n, by / n, 1 / n). With P_i = obj_i: a2 = |P2 - P3|^2, b2 = |P1 - P3|^2,
 * c2 = |P1 - P2|^2 (each (dx dx + dy dy) + dz dz of f64 differences), ca = f2.f3, cb = f1.f3, cg = f1.f2 (each
 * (x x + y y) + z z), q = (a2 - c2) / b2, r = (a2 + c2) / b2, cob = c2 / b2, aob = a2 / b2, qm = q - 1,
 * ca2 = ca ca, cb2 = cb cb, cg2 = cg cg:
 *     A4 = qm qm - 4 cob ca2
 *     A3 = 4 ((q (1 - q) cb - (1 - r) ca cg) + 2 cob ca2 cb)
 *     A2 = 2 (((((q q - 1) + 2 q q cb2) + 2 ((b2 - c2) / b2) ca2) - 4 r ca cb cg) + 2 ((b2 - a2) / b2) cg2)
 *     A1 = 4 ((-q (1 + q) cb + 2 aob cg2 cb) - (1 - r) ca cg)
 *     A0 = (1 + q) (1 + q) - 4 aob cg2
 * QUARTIC, the roots v of A4 v^4 + .. + A0 by Ferrari's factorisation: B, C, D, E = A3, A2, A1, A0 / A4; B2 = B B;
 *     p = C - 0.375 B2;  qq = (D - 0.5 B C) + 0.125 B2 B;  rr = ((E - 0.25 B D) + 0.0625 B2 C) - 0.01171875 B2 B2;
 *     the resolvent cubic m^3 + c2 m^2 + c1 m + c0 with c2 = p, c1 = 0.25 p p - rr, c0 = -0.125 qq qq: from
 *     m = 1 + max(|c2|, |c1|, |c0|) (a later one replaces an earlier one when greater) PCNN_POSE2D_CUBIC_STEPS Newton steps
 *     m <- m - (((m + c2) m + c1) m + c0) / ((3 m + 2 c2) m + c1);
 *     when m > 0: s = sqrt(2 m), h = 0.5 p + m, t = qq / (2 s), sd1 = sqrt(s s - 4 (h + t)), sd2 = sqrt(s s - 4 (h - t)),
 *       y = 0.5 (s + sd1), 0.5 (s - sd1), 0.5 (sd2 - s), 0.5 ((-s) - sd2);
 *     otherwise the biquadratic: sd = sqrt(p p - 4 rr), z1 = sqrt(0.5 (sd - p)), z2 = sqrt(0.5 ((-p) - sd)), y = z1, -z1, z2, -z2;
 *     each v = y - 0.25 B, then PCNN_POSE2D_POLISH_STEPS steps v <- v - ((((v + B) v + C) v + D) v + E) / (((4 v + 3 B) v + 2 C) v + D).
 *   The sqrt of a negative number is a NaN and a NaN slot is no root. This is adequate for the O(1) coefficients of P3P and
 *   is NOT a general quartic solver (on random quartics over six decades of coefficients it misses real roots); nothing
 *   trusts it: every root goes through the four-pair gate below.
 * For the slots k = 0 .. 3 in order: u = (((qm v v - 2 q cb v) + 1) + q) / (2 (cg - v ca)),
 * s1 = sqrt(b2) / sqrt((1 + v v) - 2 v cb), s2 = u s1, s3 = v s1; skipped unless s1 > 0, s2 > 0 and s3 > 0; FIT over the
 * pairs (a = P_i, b = s_i f_i), sums in the order 1, 2, 3, n = 3; skipped when one of the FOUR points has q.z <= 0 under it
 * (q = R o + t, q_i = ((P_i0 ox + P_i1 oy) + P_i2 oz) + P_i3); the solution with the smallest REPROJ distance d4 of pair
 * 3 is taken (d4 < the best so far, which starts at +inf: the first on a tie). The attempt is refused without a solution;
 * when REPROJ of one of the four pairs is not an inlier under (double)inlier_threshold; when the box of the depth route
 * fails; when a pose entry is not finite. The first attempt not refused is the hypothesis: hyp_pose, hyp_class,
 * hyp_attempt as in the depth route, hyp_rec = (j_0, j_1, j_2, j_3). Without one: zeros, class 0, attempt -1, records -1.
 *
 * REPROJ(P, record), f64: q = R o + t as above; u = fx q.x / q.z + px, v = fy q.y / q.z + py; du = u - x, dv = v - y;
 * distance = sqrt(du du + dv dv); an inlier when q.z > 0 and distance < (double)inlier_threshold.
 *
 * RANSAC. Steps 1 - 4 of the depth route with REPROJ as the inlier test of step 2 and this refit in step 4: the list
 * (subset order, thinned) is taken under the pose P0 the survivor has before the refit and is fixed; then
 * PCNN_POSE2D_GN_STEPS times, P = R|t being the current pose:
 *   for every listed record: y_i = (P_i0 ox + P_i1 oy) + P_i2 oz, q = (y_0 + P_03, y_1 + P_13, y_2 + P_23);
 *     ru = (fx q.x / q.z + px) - x, rv = (fy q.y / q.z + py) - y; iz = 1 / q.z, a = fx iz, b = fy iz,
 *     c = -(fx q.x iz iz), d = -(fy q.y iz iz);
 *     Ju = (c y_1, a y_2 - c y_0, -(a y_1), a, 0, c),  Jv = (d y_1 - b y_2, -(d y_0), b y_0, 0, b, d)
 *     (the derivatives of (u, v) by a rotation vector applied on the left and by the translation);
 *     H_ij += Ju_i Ju_j + Jv_i Jv_j for i <= j (21 sums), g_i += Ju_i ru + Jv_i rv (6 sums): subset position k on lane
 *     k mod 64, ascending onto +0, the 64 lane sums folded by the xor butterfly 32 .. 1;
 *   H x = -g by Cholesky: for j = 0 .. 5: d = H_jj, d <- d - L_jk L_jk for k = 0 .. j - 1; FAIL unless d > 0 and finite;
 *     L_jj = sqrt(d); for i = j + 1 .. 5: s = H_ji, s <- s - L_ik L_jk for k = 0 .. j - 1, L_ij = s / L_jj. Then for
 *     i = 0 .. 5: s = -g_i, s <- s - L_ik z_k for k = 0 .. i - 1, z_i = s / L_ii; then for i = 5 .. 0: s = z_i,
 *     s <- s - L_ki x_k for k = i + 1 .. 5, x_i = s / L_ii;
 *   h = 0.5 (x_0, x_1, x_2), n = sqrt(((1 + hx hx) + hy hy) + hz hz), (w, x, y, z) = (1 / n, hx / n, hy / n, hz / n), Q the
 *     rotation of FIT's quaternion formula; R <- Q R with R'_ij = (Q_i0 R_0j + Q_i1 R_1j) + Q_i2 R_2j; t_i <- t_i + x_(3+i);
 *     FAIL when an entry of the new pose is not finite.
 * After a FAIL in any step the survivor keeps P0 for the round. ref_steps += 1 either way.
 * Outputs per (frame, class) as in the depth route.
 *
 * pcnn_pose2d_round_fwd runs steps 1-4 ONCE on caller-given hypotheses, pcnn_pose2d_estimate_fwd is prepare, sample,
 * ransac on one stream with no host synchronisation — both as in the depth route. Every loop has a bound known before the
 * launch; no workgroup waits on another.
 *
 * All pointers are DEVICE pointers; label int32 [B,H,W], vertex_pred f32 [B,H,W,3C] (4-byte aligned is enough), extents
 * f32 [C,3], intrinsics f32 [B,4] rows (fx, fy, px, py), streams uint64 [B], records f32 [B,H W,6] (8-byte aligned).
 * Validation, on the host before any launch: 1 <= B <= 65535, H, W >= 1, H W <= 2^24, 2 <= C <= 64,
 * 1 <= hypotheses <= PCNN_POSE2D_MAX_HYPOTHESES, max_attempts, pixel_batch, max_pixels, round >= 1 (pixel_batch round
 * < 2^31), ref_it, min_area >= 0, inlier_threshold, min_dist2d, min_dist3d finite -> PCNN_EINVAL; NULL pointer ->
 * PCNN_ENULL; short workspace -> PCNN_EWORKSPACE. Only the driver needs a workspace.
 */
#ifndef POSECNN_HIP_POSE2D_H
#define POSECNN_HIP_POSE2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_POSE2D_MAX_HYPOTHESES 1024
#define PCNN_POSE2D_RECORD 6
#define PCNN_POSE2D_GN_STEPS 2
#define PCNN_POSE2D_CUBIC_STEPS 80
#define PCNN_POSE2D_POLISH_STEPS 4

int pcnn_pose2d_workspace_bytes(int B, int H, int W, int C, int hypotheses, size_t* bytes);

int pcnn_pose2d_prepare_fwd(const int32_t* label, const float* vertex_pred, const float* extents, int B, int H, int W, int C,
                            float* records, int32_t* counts, int32_t* offsets, void* stream);

int pcnn_pose2d_sample_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* extents,
                           const float* intrinsics, const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B, int H,
                           int W, int C, int hypotheses, int max_attempts, int min_area, float inlier_threshold,
                           float min_dist2d, float min_dist3d, double* hyp_pose, int32_t* hyp_class, int32_t* hyp_attempt,
                           int32_t* hyp_rec, void* stream);

int pcnn_pose2d_round_fwd(const float* records, const int32_t* counts, const int32_t* offsets, const float* intrinsics,
                          const double* hyp_pose, const int32_t* hyp_class, int B, int H, int W, int C, int hypotheses,
                          int round, int pixel_batch, int max_pixels, float inlier_threshold, double* pose_out,
                          int32_t* class_out, int32_t* inliers_out, void* stream);

int pcnn_pose2d_estimate_fwd(const int32_t* label, const float* vertex_pred, const float* extents, const float* intrinsics,
                             const uint64_t* streams, uint64_t seed0, uint64_t seed1, int B, int H, int W, int C,
                             int hypotheses, int pixel_batch, int max_pixels, int ref_it, int min_area,
                             float inlier_threshold, float min_dist2d, float min_dist3d, int max_attempts, double* poses64,
                             float* poses32, int32_t* inliers, int32_t* ref_steps, int32_t* num_hyps, void* workspace,
                             size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
