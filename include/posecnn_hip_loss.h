/*
 * posecnn_hip_loss.h — the training twin of the label-head epilogue of libposecnn_hip.so: the pass of
 * pcnn_upscore_softmax_argmax_hard_fwd (posecnn_hip.h) ending in the hard-label cross-entropy loss of lib/fcn/train.py:41-44
 * (loss_cross_entropy_single_frame over the Hardlabel weights of vgg16_convs.py:148-149), and its backward. Nothing of size
 * [B,H s,W s,C] is written by the forward. Status codes and conventions are those of posecnn_hip.h; the ABI version is
 * that header's.
 *
 * Inputs (DEVICE)
 *   z          f32   [B,H,W,C]       low-resolution class scores without bias
 *   bias       f32   [C]
 *   gt_label   int32 [B,H s,W s]     ground-truth labels; values outside [0, C) have no hot class
 *   threshold                        the Hardlabel op's attribute, > 0
 *   relu                             0 / 1: score = deconv(z) + bias, or its ReLU
 *   upstream   f32   [1]             (backward) d L / d loss, or NULL for 1
 *   sums       f64   [2]             {S, count}: written by the forward, read by the backward; 16-byte aligned
 * Outputs (DEVICE, every element written)
 *   loss       f32   [1]
 *   label      int32 [B,H s,W s]     first argmax of the probabilities
 *   terms      f32   [B,H s,W s]     per-pixel loss terms, or NULL: not written
 *   dscore     f32   [B,H s,W s,C]   (backward) d L / d score; d L / d z is pcnn_deconv_bilinear_bwd of it
 *   dbias      f32   [C]             (backward)
 * Workspace: pcnn_label_head_loss_workspace_bytes, 16-byte aligned, one size for both passes; its prior contents do not
 * matter and every call overwrites what it reads.
 *
 * Per output pixel p, one IEEE f32 rounding per operation, no fused multiply-add, divide correctly rounded — the
 * expression trees and operation order of pcnn_upscore_softmax_argmax_fwd, so that label and probabilities have its bits:
 *   score[c] = [relu](sum over taps (w_y w_x) z + bias[c]);  m = max_c score[c];
 *   e[c] = exp_softmax_f32(score[c] - m);  sum = e[0] + e[1] + ... (c ascending);  prob[c] = e[c] / sum;
 *   label[p] = first maximum of prob;
 *   g = gt_label[p];  hot = 0 <= g < C and (g > 0 or prob[g] < threshold);
 *   terms[p] = hot ? log_sum_f32(sum) - (score[g] - m) : 0            (-log_softmax(score)[g])
 * log_sum_f32(x), x in [1, 64], all f32:  x = 2^n t, t in [1, 2);  if t > 1.41421354f: t = t * 0.5f, n = n + 1;
 *   f = t - 1.f;  q = f / (2.f + f);  y = q * q;
 *   P = 0.222222224f;  P = P * y + 0.285714298f;  P = P * y + 0.4f;  P = P * y + 0.666666687f;  P = P * y;
 *   L = (q + q) + q * P;  result = (float)n * 0.693145752f + (L + (float)n * 1.42860677e-06f).  A NaN is passed through.
 * Reductions, free of atomics, so the result is a pure function of the inputs:
 *   a workgroup owns 128 consecutive pixels of one output row; its terms, converted to f64, are summed by a halving tree
 *   (lane i + lane i + stride, stride = 64 .. 1), its hot pixels counted in integers; a second one-workgroup kernel adds
 *   the partials: thread t of 256 takes partials t, t + 256, ... in ascending order, then the same halving tree.
 *   S = the f64 sum, count = the integer sum;  loss = (float)(S / ((double)count + 1e-10)).  count = 0 gives loss 0.
 * Backward:  coef = upstream / ((float)count + 1e-10f) in f32;  the pixel is recomputed;
 *   dscore[p,c] = hot ? coef * (prob[c] - (c == g ? 1.f : 0.f)) : 0, and 0 where relu is set and score[c] <= 0;
 *   dbias[c] = (float)(f64 sum over p of dscore[p,c]): per workgroup, the 128 pixels in four runs of 32 consecutive
 *   pixels summed in ascending order, the runs then added in ascending order; the partials as above, one workgroup per class.
 *
 * Validation, all on the host before any launch: B, H, W >= 1, 2 <= C <= 64, B H s W s < 2^31, stride >= 1,
 * stride <= kernel <= 4 stride, kernel <= 64, (kernel - stride) even, a tile that fits the LDS (every kernel <= 2 stride
 * does), threshold > 0 -> PCNN_EINVAL; sums or workspace not 16-byte aligned -> PCNN_EINVAL; a NULL z, bias, gt_label, loss, sums, label, dscore, dbias or bytes -> PCNN_ENULL; a
 * NULL or short workspace -> PCNN_EWORKSPACE. The calls are asynchronous on `stream`, allocate nothing, read nothing
 * back and may be captured into a graph.
 */
#ifndef POSECNN_HIP_LOSS_H_
#define POSECNN_HIP_LOSS_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcnn_label_head_loss_workspace_bytes(int batch, int height, int width, int num_classes, int kernel, int stride,
                                         size_t* bytes);

int pcnn_label_head_loss_fwd(const float* z, const float* bias, const int32_t* gt_label, int batch, int height, int width,
                             int num_classes, int kernel, int stride, int relu, float threshold, float* loss,
                             double* sums, int32_t* label, float* terms, void* workspace, size_t workspace_bytes,
                             void* stream);

int pcnn_label_head_loss_bwd(const float* z, const float* bias, const int32_t* gt_label, const double* sums,
                             const float* upstream, int batch, int height, int width, int num_classes, int kernel,
                             int stride, int relu, float threshold, float* dscore, float* dbias, void* workspace,
                             size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_LOSS_H_ */
