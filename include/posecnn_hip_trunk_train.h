/*
 * posecnn_hip_trunk_train.h — the training twins of the trunk's epilogue kernels of libposecnn_hip.so: bias + ReLU
 * (pcnn_bias_act_fwd) and bias + ReLU + 2x2 max-pool (pcnn_bias_relu_pool2_fwd) with what a backward pass needs, and the
 * backward passes themselves, each with the bias gradient from the same pass. Status codes and conventions are those of
 * posecnn_hip.h; the ABI version is that header's.
 *
 * Tensors (DEVICE, NHWC, f32 unless said otherwise; every output element is written, nothing is presumed zeroed)
 *   y        [B,H,W,C]       raw convolution output, H and W even
 *   bias     [C]
 *   act      [B,H,W,C]       [ReLU](y + bias): the bits of pcnn_bias_act_fwd; NULL: not written; may be y itself
 *   pooled   [B,H/2,W/2,C]   the bits of pcnn_bias_relu_pool2_fwd
 *   sel      u8 [B,H/2,W/2,C]  which element of the window the pooled value came from: 0..3, or 4 ("closed")
 *   dpooled, dact, dy, da    gradients with the shapes of pooled, act, y, a
 *   a        [rows,C]        the output of pcnn_bias_act_fwd (the un-pooled layers' forward stays that in-place call)
 *   dbias    [C]             or NULL: not computed, and no workspace is needed
 * Workspace: pcnn_bias_relu_pool2_train_workspace_bytes / pcnn_bias_relu_train_workspace_bytes, 16-byte aligned; its prior
 * contents do not matter and every call overwrites what it reads.
 *
 * Forward, per window and channel, window order k = 0..3: (y,x), (y,x+1), (y+1,x), (y+1,x+1); one IEEE f32 rounding per
 * operation:
 *   t_k = y_k + bias[c];   best = t_0, s = 0;   for k = 1..3: if t_k > best: best = t_k, s = k
 *   pooled = relu ? (best > 0 ? best : 0) : best;      act_k = relu ? (t_k > 0 ? t_k : 0) : t_k
 *   sel = (relu and not best > 0) ? 4 : s
 * s is the FIRST maximum of the BIASED values: two raw values that differ can round to the same biased value, and then the
 * earlier one wins, as it does in max_pool(relu(y + bias)).
 * NaN: every comparison with a NaN is false. A NaN t_0 stays `best` (s = 0) whatever follows; a NaN t_k, k >= 1, is never
 * selected. With relu set a NaN `best` gives pooled = 0 and sel = 4, and a NaN t_k gives act_k = 0, as pcnn_bias_act_fwd does.
 *
 * Backward of the pooled form (the gate `act_k > 0` is the ReLU's: the dual form presumes the forward ran with relu = 1):
 *   dy_k = (sel == k ? dpooled : 0)                                        when dact is NULL
 *   dy_k = (act_k > 0 ? dact_k : 0) + (sel == k ? dpooled : 0)             one f32 add, in this order, otherwise
 * Backward of the un-pooled form:   dy = relu ? (a > 0 ? da : 0) : da      (a may be NULL when relu is 0)
 *
 * dbias[c] = (float)(f64 sum over pixels of dy[., c]), accumulated in the pass that writes dy, free of atomics, in an order
 * that is a function of the shape alone (never of the launch or of which load path the pointers allow):
 *   "pixels" are the rows of [rows,C] for the un-pooled form and the windows, in (b, y/2, x/2) order, for the pooled form;
 *   a window contributes its four dy_k in the order k = 0..3.
 *   A workgroup owns a run of 128 consecutive pixels (the last run may be short). Pixel p of the run belongs to slot p mod 16;
 *   a slot adds its pixels' values, converted to f64, in ascending order to 0.0 (a window: k = 0, 1, 2, 3, then the next
 *   window). The 16 slot sums are combined by a halving tree: slot i + slot i + stride, stride = 8, 4, 2, 1.
 *   A second kernel, one workgroup per channel, adds the runs' partials: thread t of 256 takes partials t, t + 256, ... in
 *   ascending order starting from 0.0, then a halving tree, stride = 128 .. 1; the result is rounded once to f32.
 *
 * Validation, all on the host before any launch: B, H, W, C >= 1 (rows >= 1), H and W even for the pooled entries,
 * B H W C < 2^31 (rows C < 2^31), relu 0 or 1, exactly one of dact / act given, a workspace that is not 16-byte aligned
 * -> PCNN_EINVAL; a NULL y, bias, pooled, sel, dpooled, da, dy, bytes, or a NULL a with relu = 1 -> PCNN_ENULL; with dbias
 * given, a NULL or short workspace -> PCNN_EWORKSPACE. 16-byte loads and stores are used when C % 4 == 0 and every f32
 * pointer is 16-byte (sel: 4-byte) aligned, scalar ones otherwise; the results do not depend on which. The calls are
 * asynchronous on `stream`, allocate nothing, read nothing back and may be captured into a graph.
 */
#ifndef POSECNN_HIP_TRUNK_TRAIN_H_
#define POSECNN_HIP_TRUNK_TRAIN_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcnn_bias_relu_pool2_train_workspace_bytes(int batch, int height, int width, int channels, size_t* bytes);
int pcnn_bias_relu_train_workspace_bytes(int64_t rows, int channels, size_t* bytes);

int pcnn_bias_relu_pool2_train_fwd(const float* y, const float* bias, int batch, int height, int width, int channels,
                                   int relu, float* act, float* pooled, uint8_t* sel, void* stream);

int pcnn_bias_relu_pool2_train_bwd(const float* dpooled, const uint8_t* sel, const float* dact, const float* act, int batch,
                                   int height, int width, int channels, float* dy, float* dbias, void* workspace,
                                   size_t workspace_bytes, void* stream);

int pcnn_bias_relu_train_bwd(const float* da, const float* a, int64_t rows, int channels, int relu, float* dy, float* dbias,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_TRUNK_TRAIN_H_ */
