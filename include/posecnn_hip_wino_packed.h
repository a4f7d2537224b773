/*
 * posecnn_hip_wino_packed.h — the packed-filter route of the Winograd trunk kernel in libposecnn_hip.so
 * (csrc/wino_mfma.hip). Status codes and conventions are those of posecnn_hip.h; the ABI version is that header's.
 *
 * pcnn_winograd43_conv_fwd (posecnn_hip.h) stages both operands of its 36 contractions through an LDS ring. The filter
 * operand does not need it: a wave reads only the 16 filter rows of its own output channels. Here the kernel takes those
 * rows straight from global memory into registers — 2 instead of 6 DMA instructions and 8 instead of 12 LDS reads per wave
 * and 64-deep K stage, 64 instead of 72 KB of LDS — from a bank laid out in the order its lanes consume it. Same products,
 * same K order, same fold: the same bits as pcnn_winograd43_conv_fwd on the row-major bank.
 *
 *   pcnn_winograd43_pack_filters_fwd: ut f32 [groups][36][Cout][Cin] (what pcnn_winograd43_conv_fwd takes) -> utp f32
 *       [groups][36][Cout/16][Cin/64][4][64][4], as many floats as ut, not in place:
 *         utp[g][k][n16][kc][j][16 lk + lr][e] = ut[g][k][16 n16 + lr][64 kc + 16 j + 4 lk + e]
 *       One wave-wide 16-byte load is one contiguous KB, a stage's four loads 4 KB. A plain permutation, once per filter.
 *       Cin, Cout multiples of 64, groups >= 1 (PCNN_EINVAL), ut / utp non-NULL (PCNN_ENULL), 16-byte aligned, distinct.
 *   pcnn_winograd43_conv_packed_fwd: the arguments, checks, outputs and workspace rule
 *       (pcnn_winograd43_conv_workspace_bytes) of pcnn_winograd43_conv_fwd, with utp (16-byte aligned) in place of ut.
 */
#ifndef POSECNN_HIP_WINO_PACKED_H
#define POSECNN_HIP_WINO_PACKED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pcnn_winograd43_pack_filters_fwd(const float* ut, int in_channels, int out_channels, int groups, float* utp,
                                     void* stream);

int pcnn_winograd43_conv_packed_fwd(const float* v, const float* utp, const float* bias, int batch, int height,
                                    int width, int in_channels, int out_channels, int groups, int relu,
                                    int pool, float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                                    void* stream);

#ifdef __cplusplus
}
#endif

#endif
