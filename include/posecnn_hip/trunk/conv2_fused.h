/*
 * posecnn_hip/trunk/conv2_fused.h — a 3x3 / stride 1 / SAME convolution with 64 or 128 input and 128 output channels
 * (conv2_1, conv2_2 of the VGG16 trunk) as ONE kernel of libposecnn_hip.so (csrc/conv2_fused.hip): the Winograd F(4x4,3x3)
 * input transform, the 36 contractions and the output transform, with the transformed input kept on the CU. Status codes and
 * conventions are those of posecnn_hip.h; the ABI version is that header's.
 *
 *   pcnn_winograd43_conv_fused_fwd: x f32 [B,H,W,Cin], utp the fragment-major filter bank of
 *       pcnn_winograd43_pack_filters_fwd (posecnn_hip_wino_packed.h) f32 [groups][36][Cout/16][Cin/64][4][64][4], bias f32
 *       [groups,Cout]; image b uses filter set b / (B / groups).
 *       pool 0: y f32 [B,H,W,128] = [ReLU](conv(x) + bias); pool 1: y f32 [B,H/2,W/2,128], its 2x2 max-pool.
 *       Bit-identical to pcnn_winograd43_input_fwd followed by pcnn_winograd43_conv_packed_fwd on the same tensors as long
 *       as that entry does not split Cin: with Cin = 64, with a NULL workspace, and in every launch of at least 128 blocks
 *       of 16 x 16 pixels (a split sums two partial outputs: another rounding order).
 *       H x W x Cin of one image must stay below 2^30 elements (32-bit byte offsets inside an image).
 *       PCNN_EINVAL, nothing written, unless H and W are multiples of 16, Cin is 64 or 128, Cout == 128, pool is 0 or 1,
 *       groups >= 1 and B % groups == 0, and x, utp, bias, y are 16-byte aligned; PCNN_ENULL for a NULL pointer.
 */
#ifndef POSECNN_HIP_TRUNK_CONV2_FUSED_H
#define POSECNN_HIP_TRUNK_CONV2_FUSED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pcnn_winograd43_conv_fused_fwd(const float* x, const float* utp, const float* bias, int batch, int height, int width,
                                   int in_channels, int out_channels, int groups, int relu, int pool, float* y,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif
