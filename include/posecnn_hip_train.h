/*
 * posecnn_hip_train.h — training-side entries of libposecnn_hip.so that have no counterpart among the reference's
 * custom ops: the vertex regression targets the reference builds on the host
 * (lib/gt_synthesize_layer/minibatch.py:543-602, _generate_vertex_targets) generated on the device, and the vertex loss
 * (lib/fcn/train.py:564-573) evaluated from what those targets are made of, a label map and a table of objects, without
 * the two [B,H,W,3C] tensors ever existing. Status codes and conventions are those of posecnn_hip.h; the ABI version is
 * that header's.
 *
 * Inputs common to the three entries
 *   label     int32 [B,H,W]     gt_label_2d
 *   instance  int32 [B,H,W]     instance mask (the reference's `mask` image, multi-instance path); NULL = all zero
 *   objects   f32   [B,M,6]     rows (cls, mask_id, cx, cy, log_z, w); cls >= 1 live, cls <= 0 empty; mask_id = 0: no
 *                               instance test; 0 <= M <= 64 (NULL allowed iff M == 0); 2 <= C <= 64
 *
 * Arithmetic. For pixel (y, x) of frame b with label l: if l <= 0 or l >= C, or no row matches, its 3C targets and
 * weights are +0. The matching row is the HIGHEST-index row j with cls_j == l and (mask_id_j == 0 or
 * (float)instance[b,y,x] == mask_id_j) — the overwrite order of the reference's loops. With a match, in float64 with one
 * rounding per operation (correctly rounded sqrt and divide):
 *     dx = (double)cx - x;  dy = (double)cy - y;  n = sqrt(dx*dx + dy*dy) + 1e-10
 *     targets[3l .. 3l+2] = (float)(dx/n), (float)(dy/n), log_z        weights[3l .. 3l+2] = w, w, w
 * which is bit for bit what numpy computes at minibatch.py:586-594 from cx, cy = float32(im_scale * center) and
 * log_z = float32(log(poses[2,3,j])). No logarithm runs on the device.
 */
#ifndef POSECNN_HIP_TRAIN_H_
#define POSECNN_HIP_TRAIN_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* targets, weights f32 [B,H,W,3C]: every element is written. */
int pcnn_vertex_targets_fwd(const int32_t* label, const int32_t* instance, const float* objects, int batch,
                            int height, int width, int num_classes, int num_objects, float* targets,
                            float* weights, void* stream);

/* pcnn_smooth_l1_vertex_fwd(pred, targets, weights, ...) of the tensors above, without them: out f32 [3] = loss,
 * sum(in), sum(w), bit-identical — the same reduction order, and an element without a matching row adds +0 to both
 * sums, which changes neither. pred f32 [B,H,W,3C] is read only where a row matches, so:
 *   PRECONDITION  pred must be finite wherever the weight is 0. pcnn_smooth_l1_vertex_fwd turns an infinite or NaN
 *   prediction under a zero weight into NaN (0 * inf); these entries give it no influence at all.
 * workspace: pcnn_smooth_l1_vertex_workspace_bytes. */
int pcnn_smooth_l1_vertex_gt_fwd(const float* pred, const int32_t* label, const int32_t* instance,
                                 const float* objects, int batch, int height, int width, int num_classes,
                                 int num_objects, float sigma, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* pcnn_smooth_l1_vertex_bwd likewise: grad_pred f32 [B,H,W,3C], every element written; `out` is the forward's,
 * upstream f32 [1] on the device (NULL = 1). Bit-identical wherever a row matches; elsewhere +0 (the unfused entry may
 * give -0 there). Same precondition on pred. */
int pcnn_smooth_l1_vertex_gt_bwd(const float* pred, const int32_t* label, const int32_t* instance,
                                 const float* objects, const float* out, const float* upstream, int batch,
                                 int height, int width, int num_classes, int num_objects, float sigma,
                                 float* grad_pred, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_TRAIN_H_ */
