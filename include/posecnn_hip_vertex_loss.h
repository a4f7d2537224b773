/*
 * posecnn_hip_vertex_loss.h — the training twin of the fused vertex head of libposecnn_hip.so: the vertex loss of
 * lib/fcn/train.py:564-573 and its backward evaluated from the 1/stride-resolution field, the label map and the object
 * table, so that neither `vertex_pred` [B,H s,W s,3C] nor its gradient is ever written. Status codes and conventions are
 * those of posecnn_hip.h; the ABI version is that header's.
 *
 * Inputs (DEVICE)
 *   z          f32   [B,H,W,3C]      low-resolution vertex field without bias
 *   bias       f32   [3C]
 *   label      int32 [B,H s,W s]     gt_label_2d
 *   instance   int32 [B,H s,W s]     instance mask, or NULL = all zero
 *   objects    f32   [B,M,6]         rows (cls, mask_id, cx, cy, log_z, w) exactly as in posecnn_hip_train.h; NULL iff M == 0
 *   upstream   f32   [1]             (backward) d L / d loss, or NULL for 1
 *   out        f32   [3]             {loss, sum(in_loss), sum(w)}: written by the forward, read by the backward
 * Outputs (DEVICE, every element written)
 *   out        f32   [3]             (forward)
 *   dz         f32   [B,H,W,3C]      (backward) 16-byte aligned
 *   dbias      f32   [3C]            (backward)
 * Workspace: pcnn_vertex_head_loss_workspace_bytes, 16-byte aligned, one size for both passes; its prior contents do not
 * matter and every call overwrites what it reads.
 *
 * Arithmetic, one IEEE f32 rounding per operation, no fused multiply-add. With
 *   pred[p, c] = (sum over the <= 2 x 2 taps, rows then columns ascending, acc = acc + (w_y w_x) z) + bias[c]
 * — the bits of pcnn_deconv_bilinear_fwd(z, kernel, stride, bias) — evaluated only for the three channels 3l .. 3l+2 of a
 * pixel whose label l matches a row of the table (posecnn_hip_train.h):
 *   forward   out is bit for bit pcnn_smooth_l1_vertex_gt_fwd(pred, ...): the same partial kernel and reduction order
 *             (thread (blk, t) of 1024 x 256 takes elements blk 256 + t + m 1024 256, m ascending; two halving trees).
 *   backward  g[p, c] = (dpred / (sum(w) + 1e-10f)) * upstream, the element of pcnn_smooth_l1_vertex_gt_bwd; dz is bit
 *             for bit pcnn_deconv_bilinear_bwd of it: for cell (b, i, j) and channel c a gather over its kernel x kernel
 *             window, output rows ascending, then output columns ascending, acc = acc + (tap(ty) tap(tx)) g. A pixel
 *             whose matched label does not own channel c has g = +-0 there; the taps are positive and the accumulator
 *             starts at +0 and can never become -0, so acc + w (+-0) == acc bitwise and such pixels are skipped.
 *   PRECONDITION (as posecnn_hip_train.h): z and bias finite.
 * The backward's kernel: a workgroup owns a tile of TH x TW cells of one frame, (TH, TW) the first of (4,8), (4,4), (2,4),
 * (2,2), (1,2), (1,1) whose pixel footprint (TH s + k - s)(TW s + k - s) is at most 3072, else (1,1); tiles are numbered
 * (b tiles_y + tile_y) tiles_x + tile_x with tiles_y = ceil(H / TH), tiles_x = ceil(W / TW).
 *   dbias[c] = (float)(f64 sum over all pixels p of g[p, c]), free of atomics: a workgroup sums the pixels of its own
 *   cells (rows s i0 .. s (i0 + th) - 1, columns s j0 .. s (j0 + tw) - 1: every pixel once, no halo), converted to f64,
 *   each pixel row from +0 in ascending x, the row sums then from +0 in ascending y; a second kernel, one workgroup per
 *   channel, adds the tiles' partials: thread t of 256 takes partials t, t + 256, ... in ascending order from +0, then a
 *   halving tree (lane i + lane i + stride, stride = 128 .. 1).
 *
 * Validation, all on the host before any launch: B, H, W >= 0, B <= 65535, B H s W s <= 2^30, 2 <= C <= 64, 0 <= M <= 64,
 * stride >= 1, stride <= kernel <= 2 stride, kernel <= 64, (kernel - stride) even, sigma > 0 -> PCNN_EINVAL; a NULL z,
 * bias, label, objects (M > 0), out, dz, dbias or bytes -> PCNN_ENULL; a NULL or short workspace -> PCNN_EWORKSPACE; a dz or
 * workspace that is not 16-byte aligned -> PCNN_EINVAL. The calls are asynchronous on `stream`, allocate nothing, read
 * nothing back and may be captured into a graph.
 */
#ifndef POSECNN_HIP_VERTEX_LOSS_H_
#define POSECNN_HIP_VERTEX_LOSS_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcnn_vertex_head_loss_workspace_bytes(int batch, int height, int width, int num_classes, int kernel, int stride,
                                          size_t* bytes);

int pcnn_vertex_head_loss_fwd(const float* z, const float* bias, const int32_t* label, const int32_t* instance,
                              const float* objects, int batch, int height, int width, int num_classes, int num_objects,
                              int kernel, int stride, float sigma, float* out, void* workspace, size_t workspace_bytes,
                              void* stream);

int pcnn_vertex_head_loss_bwd(const float* z, const float* bias, const int32_t* label, const int32_t* instance,
                              const float* objects, const float* out, const float* upstream, int batch, int height,
                              int width, int num_classes, int num_objects, int kernel, int stride, float sigma, float* dz,
                              float* dbias, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_VERTEX_LOSS_H_ */
