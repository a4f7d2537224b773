// wino_mfma.hip — the Winograd-domain contractions of the VGG16 trunk on the gfx950 matrix cores,
// with the output transform fused in (`Network.conv` for every 3x3 / stride 1 / SAME layer with
// Cin, Cout multiples of 64: lib/networks/network.py:159-187, lib/networks/vgg16_convs.py:37-52 and
// the depth tower :54-67). Replaces the library batched GEMM + wino43_output_kernel pair of round 1
// and its Cin = 64-only fused kernel.
//
//   y = [ReLU](A^T (sum_ci V[k][t][ci] U[k][ci][co]) A + bias[co])   [2x2 max-pooled]
//
// F(4x4,3x3): 36 planes k = 6 xi + nu, each a GEMM [T x Cin] . [Cin x Cout] in exact f32 on
// v_mfma_f32_16x16x4_f32 (no xf32/TF32 on gfx950; 157 TFLOP/s peak). Design for the chip, not for a
// generic GEMM:
//
//  * Workgroup = 32 tiles x 64 output channels, 4 waves, TWO workgroups per CU (one wave of each per
//    SIMD, so that one workgroup's LDS / global / VALU work, barrier waits and epilogue hide under the
//    other's MFMAs). Wave w owns the block's 32 tiles x channels [16 w, 16 w + 16): two 16x16
//    accumulator blocks. This is the only shape; what else was measured is listed at the kernel.
//  * The transform-domain product M NEVER exists, not even in registers as a whole: planes are
//    processed column by column (nu outer, xi inner). Once the 6 planes of column nu are summed
//    over all of Cin, t = A^T M[:, nu] (4 values) is folded into the 16 outputs Y += t (x) A[nu, :]
//    and the 6 accumulators are recycled. 22 live values per (tile, channel) instead of 36 is what
//    lets 64 x 64 elements per CU (two 32 x 64 blocks) fit the register file (360 KB of the CU's
//    512 KB) — 4x the tile of the round-1 kernel.
//  * Operands go global -> LDS directly (global_load_lds_dwordx4: no staging registers, no
//    ds_write pass) through a ring of 3 stage buffers, ONE barrier per 64-deep K stage: the 6 DMA
//    instructions a wave issues for stage s+2 (2 of V rows, 4 of U^T rows) fly under the MFMAs of
//    stages s and s+1 (a stage of a Cin = 64 layer is a fresh HBM miss per plane: one stage of cover
//    is not enough). The barrier is a raw s_barrier behind a COUNTED s_waitcnt vmcnt(6) — the wave's
//    own DMAs of stage s have landed, the 6 of stage s+1 stay in flight; __syncthreads() would drain
//    the DMA queue (vmcnt(0)) every stage. The LDS image, its XOR swizzle and the rules of the ring
//    are those of csrc/mfma_ring.h, shared with csrc/fc_mfma.hip. One b128 read feeds 4 MFMAs. A
//    lane's 8 read addresses are loop invariants: the ring position travels in the reads' offset field
//    (three copies of a half stage's six reads behind a scalar branch), so a stage has NO vector-ALU
//    instruction between its 32 MFMAs.
//  * The packed route (BSRC = 1, pcnn_winograd43_conv_packed_fwd): wave w is the only reader of U^T rows 16 w ... 16 w + 15
//    (it issues exactly the DMAs of the rows it later reads), so the filter operand needs neither LDS nor the barrier. It
//    comes by global_load_dwordx4 straight into registers, one stage ahead, from a fragment-major bank built once per
//    filter (wino43_pack_filters_kernel: one wave-wide load = one contiguous KB). Per wave and stage 2 DMA instructions
//    instead of 6, 8 ds_read_b128 instead of 12, a ring of 24 KB instead of 72 (the kernel's 64 KB are the epilogue's
//    staging buffers); four B register sets whose roles alternate from stage to stage, statically (the K loop walks
//    stage pairs). Same products, same K order, same fold — the same bits; BSRC = 0 is the kernel as it was.
//  * Epilogue: bias + ReLU (+ 2x2 max-pool of the 4x4 tile) in registers, then through LDS (two staging
//    buffers, one barrier per pass) so that every store instruction writes whole 256-byte channel rows
//    (the C/D layout alone would give 64-byte segments).
//  * Launches too small to fill the chip (batch-1 conv4_x / conv5_x) split Cin over grid.y; a reduction
//    kernel sums the raw partial outputs in a fixed order and applies bias / ReLU / pooling.
//  * blockIdx -> (tile block, channel block) is XCD-aware: a tile block's V rows are shared by the
//    Cout / 64 workgroups that run back to back on ONE XCD (same L2), tile blocks are dealt round
//    robin to the 8 XCDs.
//  * `groups`: G independent filter sets over G equal slices of the tile range — the colour and the
//    depth tower of an RGB-D network (identical shapes, different weights) run as ONE launch with
//    twice the workgroups.
#include <cstdlib>

#include "pcnn_device.h"
#include "mfma_ring.h"
#include "../../include/posecnn_hip_wino_packed.h"

namespace {

using namespace pcnn;

constexpr int WM_BC = 64;     // output channels per workgroup
constexpr int WM_KC = 64;     // K (input channels) per pipeline stage
constexpr int WM_LD = 64;     // LDS row (floats): unpadded, XOR-swizzled 16-byte chunks
constexpr int WM_NBUF = 3;    // stage buffers in the LDS ring (prefetch distance 2)
constexpr int WM_BT = 32;     // tiles per workgroup
constexpr int WM_NW = 4;      // waves per workgroup
constexpr int WM_UB = WM_BC / 4 / WM_NW;   // U^T DMA instructions (4 rows each) per wave and stage: 4, next to 2 of V rows

// The bits of the kernel's ABL parameter (tools/wino_ablate.hip only; the library instantiates 0): each leaves one
// ingredient out to see what it costs. Timing only — the results are wrong by design.
enum : int {
  ABL_NO_BARRIER = 1,       // the stage's counted wait without its s_barrier
  ABL_NO_DMA = 2,           // no operand DMA
  ABL_NO_LDS_READS = 4,     // no ds_read_b128 (the operand registers stay what they are)
  ABL_NO_MFMA = 8,          // no MFMAs
  ABL_NO_FOLD = 16,         // no column fold
  ABL_NO_EPILOGUE = 32,     // no epilogue: one value per lane keeps the accumulators alive
  ABL_L2_OPERANDS = 64,     // every workgroup on the operands of block (0, 0): all L2-resident, i.e. what the fabric costs
  ABL_NO_STORES = 128,      // unpooled output (POOL 0 / 2): the staged rows are read back but not stored
  ABL_EPI_REGS_ONLY = 256,  // epilogue = bias + ReLU on the registers, nothing staged or stored
  ABL_NT_STORES = 512,      // unpooled output: non-temporal stores
  ABL_NO_B_LOADS = 1024,    // BSRC = 1: no filter loads into registers (the operand registers stay what they are)
};

// POOL: 0 = y [.,H,W,Cout]; 1 = only max_pool_2x2(y) (written to y); 2 = both (y and ypool)
// BSRC: where the filter operand B (the wave's 16 U^T rows) comes from. 0 = through the LDS ring like A, from the row-major
// bank ut [group][36][Cout][Cin]. 1 = straight from global memory into registers, from the fragment-major bank utp of
// wino43_pack_filters_kernel below: no wave reads a B row that another wave brought in, so B needs neither LDS nor the
// stage barrier. The ring then holds A alone (24 KB; the 64 KB of the kernel are the epilogue's staging buffers), a wave
// issues 2 DMA instructions per stage instead of 6 and 8 ds_read_b128 instead of 12. Same products, same K order
// (k = 16 j + 4 lk + i), same accumulator chains: the same bits.
// ODD (BSRC = 1 only): the parity of the K stages per plane, NK — the launcher's business; see the plane loops.
// ABL: see above.
// `mode` bit 0: XCD x owns channel block x (launches with ncb == 8 whose filter bank outweighs their transformed input,
// i.e. the deep layers of a single frame: every XCD then streams ITS eighth of U once instead of all of U).
// The first MFMA pair into a plane's accumulators takes C = 0 as an inline constant, so a column fold leaves them as they are.
// Measured and dropped — what was tried and what it measured (12-layer totals are at 2 x 16 frames). The code of the
// template switches WR, ZC and EPI was last in the tree at commit 73cff15; the two round-4 schedules left it in round 5:
//   * WR = 2 (round 2): 64 tiles x 64 channels, 8 waves, ONE workgroup per CU, 2/3 of the operand bytes per flop: conv3_2
//     1.87 ms against 1.75 for the pairs, conv3_1 1.02 / 0.95, conv4_2 1.79 / 1.78, 12 layers 16.25 / 15.86 ms.
//   * ZC = 0 (round 3): a v_mov zeroing the accumulators after every column fold (48 VALU per fold) instead of the inline
//     constant: same bits (0 + a b either way), 12 layers 14.56-14.64 ms against 14.62.
//   * s_setprio 3 / 0 by the workgroup's slot on the CU (HW_ID.TG_ID), so that one of the two co-resident workgroups runs
//     as if alone and the other fills the gaps: 14.62 -> 14.71 / 14.90 ms for the two polarities.
//   * persistent workgroups (a grid of the 512 resident slots, each walking its block pairs): 14.62 -> 15.07 ms (conv4_2
//     1.61 -> 1.73, conv2_2 1.74 -> 1.83) — the hardware's hand-out of blocks to whichever slot frees first balances better
//     than a static walk, and the loop's 8 extra live registers cost the kernel its last slack.
//   * EPI = 1 (round 5): MFMA operand roles swapped (same products, same K order, same bits), so that a lane holds four
//     consecutive channels of one tile and stores 16-byte pieces straight from registers — no LDS staging, no barriers. The
//     ablation had priced the staging at 7 / 5 / 4 % of conv2_1 / conv2_2 / conv3_2; the direct form gives it back in
//     64-byte partial-line stores: 12 layers 14.136 against 14.169 ms alone, inside the step 1107 / 1118 against 1098 /
//     1098 us per launch, the step 796 / 794 against 764 / 808 frames/s. No gain: the staged epilogue stays.
template <int POOL, int BSRC = 0, int ABL = 0, int ODD = 0>
__global__ __launch_bounds__(64 * WM_NW, 2) void wino43_mfma_kernel(
    const float* __restrict__ v, const float* __restrict__ ut, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ ypool, int H, int W, int Cin, int Cout, int Ht, int Wt,
    long long T, long long tiles_per_group, int relu, int nbt, int ncb, int ksplit, long long ysplit_stride, int mode)
{
  constexpr int RING = WM_NBUF * (WM_BT + (BSRC == 0 ? 64 : 0)) * WM_LD, STAGE2 = 2 * WM_BT * 4 * 64;
  __shared__ __attribute__((aligned(16))) float smem[RING > STAGE2 ? RING : STAGE2];   // sA[3][WM_BT][64] | BSRC 0: sB[3][64][64]; epilogue: 2 x [WM_BT][4][64]

  // XCD-aware block map: XCD x = blockIdx % 8 takes tile blocks tb == x (mod 8); on an XCD the
  // channel blocks of a tile block are consecutive
  const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
  const bool cbmajor = (mode & 1) != 0;          // (ncb == 8, checked by the launcher)
  const int cb = cbmajor ? x : q % ncb;
  const int tb = cbmajor ? q : (q / ncb) * 8 + x;
  if (tb >= nbt) return;
  const int tb_data = (ABL & ABL_L2_OPERANDS) ? 0 : tb, cb_data = (ABL & ABL_L2_OPERANDS) ? 0 : cb;
  y += (long long)blockIdx.y * ysplit_stride;    // `ksplit` > 1: this Cin slice's partial output (see below)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: everything derived from it (LDS bases, M0) stays on the SALU
  const int lr = lane & 15, lk = lane >> 4;
  // tile blocks never straddle a group: group g owns tiles [g tpg, (g+1) tpg) in nbg blocks of WM_BT
  const int nbg = (int)((tiles_per_group + WM_BT - 1) / WM_BT);
  const int grp = tb / nbg;
  const long long t0 = (long long)grp * tiles_per_group + (long long)(tb_data - (ABL & ABL_L2_OPERANDS ? 0 : grp * nbg)) * WM_BT;
  const long long tend = (long long)(grp + 1) * tiles_per_group;   // first tile that is not this block's business
  const float* utg = ut + (size_t)grp * 36 * Cout * Cin;
  // `ksplit` > 1 (small launches, see the launcher): workgroup blockIdx.y contracts only its slice of Cin and
  // writes a raw partial output (the host passes no bias, no ReLU, POOL = 0); a reduction kernel finishes
  const int ks = blockIdx.y;
  const int NK = Cin / WM_KC / ksplit;

  // staging: a stage = WM_BT rows x 256 B of V and 64 rows of U^T = WM_BT/4 + 16 DMA instructions of 4 rows
  // each; wave w issues V instructions 2w, 2w + 1 and U^T instructions WM_UB w ... WM_UB w + WM_UB - 1. Lane l of
  // instruction ii lands at row 4 ii + (l >> 4), physical chunk l & 15, and therefore fetches logical
  // chunk (l & 15) ^ (row & 15).
  const int dr0 = 8 * wave + lk, dr1 = dr0 + 4;                 // the lane's V rows in its two instructions
  const int dc0 = ring_src_col(lr, dr0), dc1 = ring_src_col(lr, dr1);
  const int ur0 = 4 * WM_UB * wave + lk;                           // first U^T row; instruction i adds 4 i
  const long long tlast = tend - 1;
  const long long ta0 = t0 + dr0 < tend ? t0 + dr0 : tlast, ta1 = t0 + dr1 < tend ? t0 + dr1 : tlast;   // rows past the end: any finite data, never stored
  // per-lane BYTE offsets (32 bit) from wave-uniform bases: the DMA then addresses as SGPR base + VGPR
  // offset and the per-stage pointer arithmetic stays on the scalar unit
  const unsigned va0 = (unsigned)((ta0 * Cin + dc0) * 4), va1 = (unsigned)((ta1 * Cin + dc1) * 4);
  unsigned ub[WM_UB];
#pragma unroll
  for (int i = 0; i < WM_UB; i++) ub[i] = (unsigned)((((size_t)(cb_data * WM_BC + ur0 + 4 * i)) * Cin + ring_src_col(lr, ur0 + 4 * i)) * 4);
  const char* vbase = reinterpret_cast<const char*>(v);
  const char* ubase = reinterpret_cast<const char*>(utg);
  const long long vplane = T * Cin;
  const long long uplane = (long long)Cout * Cin;
  const int ldsw = 8 * wave * WM_LD;                            // this wave's first V row (floats) inside a stage buffer
  const int ldsu = 4 * WM_UB * wave * WM_LD;                       // ... and its first U^T row
  // LDS byte addresses of those rows in stage buffer 0 (wave-uniform: M0 of the DMA)
  const unsigned lds_base_ = (unsigned)(unsigned long long)(__attribute__((address_space(3))) float*)smem;
  const unsigned lds_a0 = lds_base_ + (unsigned)ldsw * 4u;
  const unsigned lds_b0 = lds_base_ + (unsigned)(WM_NBUF * WM_BT * WM_LD + ldsu) * 4u;

  // the lane's bias value, requested HERE: issued where it is first used (the epilogue, round 4) it was a bare global
  // round trip between the last MFMA and the first staged row of every workgroup (~1 us of a 15-us conv2_1 workgroup)
  const float bv = bias ? bias[(size_t)grp * Cout + cb * WM_BC + 16 * wave + lr] : 0.f;   // (no bias: the raw partial output of a Cin split)
  v4f acc[6][2];
#pragma unroll
  for (int i = 0; i < 6; i++) acc[i][0] = acc[i][1] = (v4f){0.f, 0.f, 0.f, 0.f};
  // outputs of the lane's elements: [block][pair of C/D rows i][4 a + e][i & 1] — rows i, i + 1 side by side, so that the fold
  // (PKF) can work on register PAIRS as the MFMA delivers them (acc[x][b] = rows 0..3 in four consecutive registers)
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f yo2[2][2][16];
#define YO(B_, I_, O_) yo2[B_][(I_) >> 1][O_][(I_) & 1]
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int o = 0; o < 16; o++) yo2[b][i][o] = (v2f){0.f, 0.f};

#define WM_DMA(BUF, VO, UO)                                                  \
  if constexpr (!(ABL & ABL_NO_DMA)) {                                       \
    const char* vs_ = vbase + (VO) * 4;                                      \
    const char* us_ = ubase + (UO) * 4;                                      \
    const unsigned la_ = lds_a0 + (unsigned)(BUF) * (WM_BT * WM_LD * 4);       \
    const unsigned lb_ = lds_b0 + (unsigned)(BUF) * (64 * WM_LD * 4);          \
    glds16_s(vs_, va0, la_);                                                 \
    glds16_s(vs_, va1, la_ + 4 * WM_LD * 4);                                 \
    if constexpr (BSRC == 0) {                                               \
      _Pragma("unroll") for (int i_ = 0; i_ < WM_UB; i_++)                    \
        glds16_s(us_, ub[i_], lb_ + 4 * i_ * WM_LD * 4);                      \
    }                                                                        \
  }

  // Stage order: nu outer, xi, then kc fastest; (pnu, pxi, pkc) is the prefetch pointer, two stages
  // ahead of the compute pointer. Prologue: stages 0 and 1 in flight.
  // The prefetch offsets (floats) advance incrementally on the scalar unit: next K slice +64; next
  // plane of the column k += 6; next column k: 30 + nu -> nu + 1.
  int pnu = 0, pxi = 0, pkc = 0;
  // BSRC = 1: a stage of the packed bank is the wave's own 4 KB [4 (K group j)][64 lanes][4] at
  // ((16-channel block) * Cin / 64 + K slice) * 1024 floats of its plane; planes are Cout * Cin floats apart as in ut
  constexpr int WM_USTEP = BSRC == 0 ? WM_KC : 16 * WM_KC;   // floats from one K slice of B to the next
  long long pvo = (long long)ks * NK * WM_KC;   // this split's first input channel
  long long puo = BSRC == 0 ? pvo : ((long long)(cb_data * (WM_BC / 16) + wave) * (Cin / WM_KC) + (long long)ks * NK) * WM_USTEP;
  const long long kback = (long long)(NK - 1) * WM_KC, ukback = (long long)(NK - 1) * WM_USTEP;
  // uniform branches on the scalar unit (3-4 SALU instructions on the common path; a select-only
  // version cost ~40 per stage and measured 1.2 % slower over the 12 layers); past the last stage the
  // pointer parks on it (the two extra prefetches re-load the last stage into a free buffer and are
  // drained before the epilogue)
  const long long dvx = 6 * vplane - kback, dux = 6 * uplane - ukback;       // next plane of the column
  const long long dvn = -29 * vplane - kback, dun = -29 * uplane - ukback;   // next column
#define WM_PF_ADVANCE()                                                                          \
  do {                                                                                           \
    if (pkc + 1 < NK) { pkc++; pvo += WM_KC; puo += WM_USTEP; }         /* next K slice */        \
    else if (pxi < 5) { pkc = 0; pxi++; pvo += dvx; puo += dux; }       /* next plane of the column */ \
    else if (pnu < 5) { pkc = 0; pxi = 0; pnu++; pvo += dvn; puo += dun; }   /* next column */     \
  } while (0)   /* past the last stage the pointer parks on it */
  // BSRC = 1: the filter operand lives in four register sets of two K groups each. A stage uses a pair (groups 0, 1 |
  // groups 2, 3) while the other pair receives the NEXT stage's — B runs one stage ahead, A two —, and the pairs swap
  // roles every stage — statically: the stage's parity is a macro argument and the K loop walks stage pairs (see the
  // stage below; a register copy instead would be 16 VALU instructions between the stage's MFMAs).
  // The loads are inline asm like the DMAs, whose vmcnt they share: a compiler-visible load among DMAs it cannot see
  // would get a wait that is too lax. SGPR base (advanced like pvo) + one loop-invariant lane offset; the K group
  // travels in the offset field.
  v4f bq[4][2];
  if constexpr (BSRC == 1 && (ABL & ABL_NO_B_LOADS)) {
#pragma unroll
    for (int i = 0; i < 4; i++) bq[i][0] = bq[i][1] = (v4f){1.f, 1.f, 1.f, 1.f};
  }
  const unsigned vbo = 16u * (unsigned)lane;
  long long pub = 0;   // B's own prefetch offset: the stage behind (pvo, puo)
#define WM_BLOAD(S, UO, J0)                                                  \
  if constexpr (!(ABL & ABL_NO_B_LOADS)) {                                   \
    const char* us_ = ubase + (UO) * 4;                                      \
    RING_GLOAD_B128(S[0], us_, vbo, (J0) * 1024);                            \
    RING_GLOAD_B128(S[1], us_, vbo, (J0) * 1024 + 1024);                     \
  }
  if constexpr (BSRC == 0) {
    { WM_DMA(0, pvo, puo); WM_PF_ADVANCE(); }
    { WM_DMA(1, pvo, puo); WM_PF_ADVANCE(); }
  } else {
    // B of stage 0, then A of stages 0 and 1: at every stage barrier the two youngest entries of the wave's vmcnt queue
    // are the A DMAs of the stage after, everything older (this stage's A and B) has landed behind vmcnt(2)
    WM_BLOAD(bq[0], puo, 0);
    WM_BLOAD(bq[1], puo, 2);
    { WM_DMA(0, pvo, puo); WM_PF_ADVANCE(); }
    { WM_DMA(1, pvo, puo); pub = puo; WM_PF_ADVANCE(); }
  }
  int cur = 0;

  // ds_read side of the swizzle: row R = (..) + lr, logical chunk 4 j + lk -> physical (4 j + lk) ^ lr
  const int ra0 = lr * WM_LD, rb = (16 * wave + lr) * WM_LD;   // (+ 16 rows for the second block)

  // The K loop is software pipelined by half a stage: the 16 MFMAs of K groups 2, 3 of stage s-1 are
  // issued AFTER the barrier of stage s, behind the LDS reads of groups 0, 1 of stage s — so the LDS
  // latency that follows every barrier (all waves would otherwise wait for their first operands at
  // the same moment, with the matrix pipe idle) and the latency of the mid-stage reads are both
  // covered by MFMAs that are already queued. Two operand register sets: X (groups 0, 1), Y (2, 3).
  v4f xa0[2], xa1[2], xb[2], ya0[2], ya1[2], yb[2];
  // The LDS reads are inline asm: hipcc's own s_waitcnt insertion collapses to lgkmcnt(0) across the
  // loop back edge (it would wait for reads issued a moment ago), so the reads are invisible to it
  // and the waits are placed by hand: lgkmcnt(0) inside the stage barrier retires the Y reads, one
  // lgkmcnt(0) after Y's MFMAs retires the X reads. sched_barrier(0) pins the order around them.
  const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) float*)smem;
  unsigned adA[4], adB[4];   // byte addresses of this lane's operand chunks in stage buffer 0, per K group
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const unsigned chb = ring_chunk_bytes(j, lk, lr);
    adA[j] = lds0 + (unsigned)ra0 * 4u + chb;
    adB[j] = lds0 + (unsigned)(WM_NBUF * WM_BT * WM_LD + rb) * 4u + chb;
  }
// The ring position is part of the INSTRUCTION, not of the address: buffer `cur` of the A operand starts
// cur * 8192 bytes behind buffer 0 (second row block + 4096), of the B operand cur * 16384 — at most 32 768, inside
// ds_read_b128's 16-bit offset field — so the lane's 8 chunk addresses adA / adB are loop invariants and a stage
// reads with no vector arithmetic at all (the 8 v_add_u32 per stage of rounds 2-6 each cost ~3.5 cycles of matrix
// time: a VALU instruction never hides behind an MFMA of its SIMD). The six reads of a half stage exist once per ring
// position and `cur` (wave-uniform, on the scalar unit) picks the copy with a scalar branch; everything else of the stage
// exists once.
#define WM_DSREAD(DST, ADDR, OFF)                                                                     \
  if constexpr (!(ABL & ABL_NO_LDS_READS)) RING_DSREAD_B128(DST, ADDR, OFF);                          \
  else asm volatile("" : "+v"(DST) : "v"(ADDR))
#define WM_READ_AT(SA0, SA1, SB, G0, CUR)                                                             \
  _Pragma("unroll") for (int g_ = 0; g_ < 2; g_++) {                                                  \
    WM_DSREAD(SB[g_], adB[(G0) + g_], (CUR) * (64 * WM_LD * 4));                                      \
    WM_DSREAD(SA0[g_], adA[(G0) + g_], (CUR) * (WM_BT * WM_LD * 4));                                  \
    WM_DSREAD(SA1[g_], adA[(G0) + g_], (CUR) * (WM_BT * WM_LD * 4) + 4096);   /* 16 rows further */    \
  }
#define WM_READ(SA0, SA1, SB, G0)                                                                     \
  if constexpr (ABL & ABL_NO_LDS_READS) { WM_READ_AT(SA0, SA1, SB, G0, 0); }   /* (nothing to dispatch) */ \
  else if (cur == 0) { WM_READ_AT(SA0, SA1, SB, G0, 0); }                                             \
  else if (cur == 1) { WM_READ_AT(SA0, SA1, SB, G0, 1); }                                             \
  else { WM_READ_AT(SA0, SA1, SB, G0, 2); }
  // BSRC = 1: the A reads alone (four per half stage)
#define WM_READA_AT(SA0, SA1, G0, CUR)                                                                \
  _Pragma("unroll") for (int g_ = 0; g_ < 2; g_++) {                                                  \
    WM_DSREAD(SA0[g_], adA[(G0) + g_], (CUR) * (WM_BT * WM_LD * 4));                                  \
    WM_DSREAD(SA1[g_], adA[(G0) + g_], (CUR) * (WM_BT * WM_LD * 4) + 4096);                           \
  }
#define WM_READA(SA0, SA1, G0)                                                                        \
  if constexpr (ABL & ABL_NO_LDS_READS) { WM_READA_AT(SA0, SA1, G0, 0); }                             \
  else if (cur == 0) { WM_READA_AT(SA0, SA1, G0, 0); }                                                \
  else if (cur == 1) { WM_READA_AT(SA0, SA1, G0, 1); }                                                \
  else { WM_READA_AT(SA0, SA1, G0, 2); }
  static_assert(WM_NBUF == 3, "WM_READ dispatches over a ring of three buffers");
#define WM_MFMA1(SA0, SA1, SB, G, ACC)                                                                \
  if constexpr (ABL & ABL_NO_MFMA) { asm volatile("" :: "v"(SA0[G]), "v"(SA1[G]), "v"(SB[G])); } else \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) {                                                  \
    ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA0[G][i_], SB[G][i_], ACC[0], 0, 0, 0);            \
    ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA1[G][i_], SB[G][i_], ACC[1], 0, 0, 0);            \
  }
#define WM_MFMA(SA0, SA1, SB, ACC)                                                                    \
  WM_MFMA1(SA0, SA1, SB, 0, ACC) WM_MFMA1(SA0, SA1, SB, 1, ACC)
  /* the same K group, but the first pair starts the accumulators from the constant 0 (first MFMAs of a plane) */
#define WM_MFMA1_Z(SA0, SA1, SB, G, ACC)                                                              \
  if constexpr (ABL & ABL_NO_MFMA) { asm volatile("" :: "v"(SA0[G]), "v"(SA1[G]), "v"(SB[G])); } else { \
    const v4f z_ = (v4f){0.f, 0.f, 0.f, 0.f};                                                         \
    ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA0[G][0], SB[G][0], z_, 0, 0, 0);                  \
    ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA1[G][0], SB[G][0], z_, 0, 0, 0);                  \
    _Pragma("unroll") for (int i_ = 1; i_ < 4; i_++) {                                                \
      ACC[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA0[G][i_], SB[G][i_], ACC[0], 0, 0, 0);          \
      ACC[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(SA1[G][i_], SB[G][i_], ACC[1], 0, 0, 0);          \
    }                                                                                                 \
  }
  // column NU of the transform domain is complete: t = A^T M[:, NU]; Y[a][e] += t[a] * A[NU][e]
  // with A[NU][:] = (1,0,0,0) (1,1,1,1) (1,-1,1,-1) (1,2,4,8) (1,-2,4,-8) (0,0,0,1); accumulators recycled
#define WM_FOLD(NU)                                                                                   \
  if constexpr (!(ABL & ABL_NO_FOLD)) {                                                               \
    const int n_ = (NU);                                                                              \
    const float c0 = n_ == 5 ? 0.f : 1.f;                                                             \
    const float c1 = n_ == 1 ? 1.f : n_ == 2 ? -1.f : n_ == 3 ? 2.f : n_ == 4 ? -2.f : 0.f;           \
    const float c2 = (n_ == 1 || n_ == 2) ? 1.f : (n_ == 3 || n_ == 4) ? 4.f : 0.f;                   \
    const float c3 = n_ == 1 ? 1.f : n_ == 2 ? -1.f : n_ == 3 ? 8.f : n_ == 4 ? -8.f : n_ == 5 ? 1.f : 0.f; \
    /* two C/D rows at a time on packed f32 (round 5): v_pk_add / v_pk_fma on the register pairs as the MFMA delivers them,  */ \
    /* element for element t = A^T m of rounds 2-4, A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1], and   */ \
    /* their 16 rank-1 FMAs (same bits; 12 layers 14.5 vs 14.7 ms alone, the step unchanged: 793 / 796 vs 792 / 794         */ \
    /* frames/s). Explicit FMAs: this file is built -ffp-contract=off; one instruction per term instead of two buys 1.7 %   */ \
    /* of the 12-layer trunk (the fold is 12 % of a Cin = 64 layer)                                                         */ \
    _Pragma("unroll") for (int b_ = 0; b_ < 2; b_++)                                                \
      _Pragma("unroll") for (int h_ = 0; h_ < 2; h_++) {                                            \
        v2f m_[6], t_[4];                                                                           \
        _Pragma("unroll") for (int x_ = 0; x_ < 6; x_++) m_[x_] = (v2f){acc[x_][b_][2 * h_], acc[x_][b_][2 * h_ + 1]}; \
        const v2f s_ = m_[1] + m_[2], d_ = m_[1] - m_[2], S_ = m_[3] + m_[4], D_ = m_[3] - m_[4];   \
        t_[0] = (m_[0] + s_) + S_;                                                                  \
        t_[1] = __builtin_elementwise_fma((v2f){2.f, 2.f}, D_, d_);                                 \
        t_[2] = __builtin_elementwise_fma((v2f){4.f, 4.f}, S_, s_);                                 \
        t_[3] = __builtin_elementwise_fma((v2f){8.f, 8.f}, D_, d_) + m_[5];                         \
        _Pragma("unroll") for (int a_ = 0; a_ < 4; a_++) {                                          \
          yo2[b_][h_][4 * a_ + 0] = __builtin_elementwise_fma(t_[a_], (v2f){c0, c0}, yo2[b_][h_][4 * a_ + 0]); \
          yo2[b_][h_][4 * a_ + 1] = __builtin_elementwise_fma(t_[a_], (v2f){c1, c1}, yo2[b_][h_][4 * a_ + 1]); \
          yo2[b_][h_][4 * a_ + 2] = __builtin_elementwise_fma(t_[a_], (v2f){c2, c2}, yo2[b_][h_][4 * a_ + 2]); \
          yo2[b_][h_][4 * a_ + 3] = __builtin_elementwise_fma(t_[a_], (v2f){c3, c3}, yo2[b_][h_][4 * a_ + 3]); \
        }                                                                                           \
      }                                                                                             \
  }

  // One stage on accumulator set XI (XP = the set of the stage before when that was another plane):
  //   own DMAs of this stage landed (counted wait: the next stage's stay in flight) -> barrier
  //   (everybody's landed, everybody done reading the previous stage) -> DMA of stage s+2 into the
  //   buffer the previous stage just freed -> reads X(s) -> MFMAs Y(s-1) -> reads Y(s) -> MFMAs X(s)
  // vmcnt(6): the 2 + WM_UB DMA instructions of the NEXT stage are what may still be in flight. (ABL_NO_BARRIER waits
  // on a stricter vmcnt(4): every record of that ablation was measured with it.)
#define WM_STAGE0(XI, XP)                                                                             \
  do {                                                                                                \
    if constexpr (ABL & ABL_NO_BARRIER) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");   \
    else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");                     \
    WM_READ(xa0, xa1, xb, 0);                                                                         \
    __builtin_amdgcn_sched_barrier(0);   /* the X reads go out first: their latency hides under Y's MFMAs */ \
    if (kc > 0) { WM_MFMA(ya0, ya1, yb, acc[XI]); }                                                   \
    else if ((XI) > 0) { WM_MFMA(ya0, ya1, yb, acc[XP]); }                                            \
    else if (nu > 0) { WM_MFMA(ya0, ya1, yb, acc[5]); WM_FOLD(nup); }                                 \
    {                                                                                                 \
      const int nb = cur >= 1 ? cur - 1 : 2;   /* (cur + 2) % 3: the previous stage's buffer */         \
      WM_DMA(nb, pvo, puo);                                                                           \
      WM_PF_ADVANCE();                                                                                \
    }                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   /* the X reads (issued 16 MFMAs ago) */        \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    if (kc == 0) { WM_MFMA1_Z(xa0, xa1, xb, 0, acc[XI]); }   /* a plane's first MFMAs: C = 0 */        \
    else { WM_MFMA1(xa0, xa1, xb, 0, acc[XI]); }                                                      \
    __builtin_amdgcn_sched_barrier(0);   /* the Y reads go out between X's MFMA groups: nothing waits for them before the next barrier */ \
    WM_READ(ya0, ya1, yb, 2);                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    WM_MFMA1(xa0, xa1, xb, 1, acc[XI]);                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   /* Y landed before the compiler may touch its registers (loop-carried) */ \
    cur = cur == 2 ? 0 : cur + 1;                                                                     \
  } while (0)
  static_assert(2 + WM_UB == 6, "the stage barrier's vmcnt(6) counts the 2 + WM_UB DMA instructions a wave issues per stage");

  // The same stage with B in registers (BSRC = 1), at stage parity P: this stage's K groups 0, 1 are in bq[2 P], its groups
  // 2, 3 in bq[2 P + 1] (the NEXT stage reads them, behind its barrier); the next stage's B goes to bq[2 - 2 P] and
  // bq[3 - 2 P]. The latter still holds groups 2, 3 of the stage before and is free once the MFMAs of Y(s-1) have been
  // issued; the former has been free since the end of the stage before, so its loads go out first, right behind the barrier.
  // Every stage — a plane's or a column's first, and the parked ones past the last — issues, in this order, 4 B loads of
  // stage s+1 and then 2 A DMAs of stage s+2. At the barrier of stage s the wave's queue therefore holds, oldest first,
  // A(s) (issued in s-2), B(s) and A(s+1) (both in s-1): vmcnt(2) leaves the two A DMAs of the next stage in flight and
  // retires everything older, this stage's B included. Loads and DMAs return in issue order.
  constexpr int WM_VM1 = WM_BT / 4 / WM_NW;   // A DMA instructions per wave and stage
  // The roles of the four register sets are STATIC: stage parity P (0: this stage's B in bq[0] | bq[1], the next stage's
  // into bq[2] | bq[3]; 1: the other way round) is a macro argument, and the K loop of a plane walks its stages in pairs.
  // A column has 6 NK stages, an even number, so every column starts at parity 0; a plane starts at parity 0 when NK is
  // even or the plane index is, at parity 1 otherwise — two forms of the column loop, chosen by the template parameter ODD
  // (both in one kernel behind a test of NK's low bit cost the register allocator 4 registers more than there are).
  // (Parity as a run-time value — two copies of the stage, or of every statement that names a B register, behind a scalar
  // branch — made the compiler hoist the fold in front of the branch or sink it behind the loads and copy register sets
  // where the copies meet: 200-400 registers spilled.)
#define WM_YMFMA_R(SB, ACC)                                                                           \
  __builtin_amdgcn_sched_barrier(0); WM_MFMA(ya0, ya1, SB, ACC); __builtin_amdgcn_sched_barrier(0)
#define WM_STAGE1(XI, XP, P, KC)                                                                      \
  do {                                                                                                \
    if constexpr (ABL & ABL_NO_BARRIER) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");   \
    else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");                     \
    WM_READA(xa0, xa1, 0);                                                                            \
    WM_BLOAD(bq[2 - 2 * (P)], pub, 0);   /* free since the stage before: out first */                  \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    if ((KC) > 0) { WM_YMFMA_R(bq[3 - 2 * (P)], acc[XI]); }                                           \
    else if ((XI) > 0) { WM_YMFMA_R(bq[3 - 2 * (P)], acc[XP]); }                                      \
    else if (nu > 0) { WM_YMFMA_R(bq[3 - 2 * (P)], acc[5]); WM_FOLD(nup); }                           \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    /* the next stage's B, behind Y(s-1), which read the registers its groups 2, 3 go to */           \
    WM_BLOAD(bq[3 - 2 * (P)], pub, 2);                                                                \
    {                                                                                                 \
      const int nb = cur >= 1 ? cur - 1 : 2;   /* (cur + 2) % 3: the previous stage's buffer */         \
      WM_DMA(nb, pvo, puo);                                                                           \
      pub = puo;                                                                                      \
      WM_PF_ADVANCE();                                                                                \
    }                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   /* the X reads (issued 16 MFMAs ago) */        \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    if ((KC) == 0) { WM_MFMA1_Z(xa0, xa1, bq[2 * (P)], 0, acc[XI]); }   /* a plane's first MFMAs: C = 0 */ \
    else { WM_MFMA1(xa0, xa1, bq[2 * (P)], 0, acc[XI]); }                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    WM_READA(ya0, ya1, 2);                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    WM_MFMA1(xa0, xa1, bq[2 * (P)], 1, acc[XI]);                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                \
    cur = cur == 2 ? 0 : cur + 1;                                                                     \
  } while (0)
  static_assert(WM_VM1 == 2, "the stage barrier's vmcnt(2) of BSRC = 1 counts the A DMA instructions a wave issues per stage");
  /* a plane of an even number of stages: pairs from parity 0 */
#define WM_PLANE_E(XI, XP) for (int kc = 0; kc < NK; kc += 2) { WM_STAGE1(XI, XP, 0, kc); WM_STAGE1(XI, XP, 1, kc + 1); }
  /* a plane of an odd number of stages starting at parity P0: one stage, then pairs from the other parity */
#define WM_PLANE_O(XI, XP, P0)                                                                        \
  WM_STAGE1(XI, XP, P0, 0);                                                                           \
  for (int kc = 1; kc < NK; kc += 2) { WM_STAGE1(XI, XP, 1 - (P0), kc); WM_STAGE1(XI, XP, P0, kc + 1); }

  // nu - 1 as a scalar loop variable of its own: written `nu - 1` next to the `nu > 0` test the compiler fuses the two into one
  // VECTOR subtract-with-borrow, whose result now outlives the X reads of the stage (one VGPR more than the kernel had)
  int nup = -1;
  if constexpr (BSRC == 0) {
    for (int nu = 0; nu < 6; nu++) {
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(0, 5);
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(1, 0);
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(2, 1);
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(3, 2);
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(4, 3);
      for (int kc = 0; kc < NK; kc++) WM_STAGE0(5, 4);
      nup = nu;
    }
  } else if constexpr (ODD == 0) {
    for (int nu = 0; nu < 6; nu++) {
      WM_PLANE_E(0, 5) WM_PLANE_E(1, 0) WM_PLANE_E(2, 1) WM_PLANE_E(3, 2) WM_PLANE_E(4, 3) WM_PLANE_E(5, 4)
      nup = nu;
    }
  } else {
    for (int nu = 0; nu < 6; nu++) {
      WM_PLANE_O(0, 5, 0) WM_PLANE_O(1, 0, 1) WM_PLANE_O(2, 1, 0) WM_PLANE_O(3, 2, 1) WM_PLANE_O(4, 3, 0) WM_PLANE_O(5, 4, 1)
      nup = nu;
    }
  }
  // drain: K groups 2, 3 of the last stage, the last column, and every LDS read before the buffers
  // are recycled for the epilogue
  if constexpr (BSRC == 0) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    WM_MFMA(ya0, ya1, yb, acc[5]);
  } else {
    // The last stage's parked B loads went into bq[0], bq[1], which nothing reads any more: they have landed (vmcnt(2):
    // only the last stage's two A DMAs may still fly) before the compiler may give those registers to the fold. The
    // number of stages, 36 NK, is even: the last stage's K groups 2, 3 are in bq[3].
    asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    WM_MFMA(ya0, ya1, bq[3], acc[5]);
  }
  WM_FOLD(5);
  // all waves' parked prefetch DMAs have landed before the ring becomes the epilogue's staging buffer: the DMAs are
  // inline asm, so the compiler's __syncthreads() is a bare s_barrier without the vmcnt(0) it would need (see
  // csrc/fc_mfma.hip: the same omission corrupted output rows there)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#undef WM_STAGE0
#undef WM_STAGE1
#undef WM_YMFMA_R
#undef WM_PLANE_E
#undef WM_PLANE_O
#undef WM_BLOAD
#undef WM_READA
#undef WM_READA_AT
#undef WM_READ
#undef WM_READ_AT
#undef WM_DSREAD
#undef WM_MFMA
#undef WM_MFMA1
#undef WM_MFMA1_Z
#undef WM_FOLD
#undef WM_DMA
#undef WM_PF_ADVANCE

  if constexpr (ABL & ABL_EPI_REGS_ONLY) {
    const float bv_ = bv;
    float k_ = 0.f;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int o = 0; o < 16; o++) { float val = YO(b, i, o) + bv_; if (relu) val = val > 0.f ? val : 0.f; k_ += val; }
    if (k_ == 12345.678f) y[tid] = k_;
    return;
  }
  if constexpr (ABL & ABL_NO_EPILOGUE) {
    float k_ = 0.f;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int o = 0; o < 16; o++) k_ += YO(b, i, o);
#pragma unroll
    for (int x_ = 0; x_ < 6; x_++) k_ += acc[x_][0][0] + acc[x_][1][1];
    if (k_ == 12345.678f) y[tid] = k_;
    return;
  }
  // ---- epilogue -------------------------------------------------------------------------------
  // lane holds, per block b, tiles 16 b + 4 lk + i (i = 0..3) x channel 16 wave + lr
  const int col = 16 * wave + lr;
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int o = 0; o < 16; o++) {
        float val = YO(b, i, o) + bv;
        if (relu) val = val > 0.f ? val : 0.f;
        YO(b, i, o) = val;
      }

  // Staging through LDS: [WM_BT tiles][4][64 channels] floats per pass, two buffers (the ring is free
  // now) so that a pass needs ONE barrier: pass a+1 writes the buffer whose readers all arrived at
  // barrier a. Writer lanes (lr, lk) hit rows 4 lk tiles apart = the same banks, so the 16-channel
  // group is XORed with lk (reader: same XOR, wave-uniform, float4 alignment kept).
  constexpr int SYF = WM_BT * 4 * 64;
  const int wcol = col ^ (16 * lk);
  // The thread's 8 store slots: tile wave + WM_NW r, pixel column re, channels rc4..rc4+3. Tile
  // coordinates by carries from the block's first tile (one 64-bit division per thread, not per store).
  const int HtWt = Ht * Wt;
  const int bimg0 = (int)(t0 / HtWt);
  const int rem0 = (int)(t0 - (long long)bimg0 * HtWt);
  const int ty0 = rem0 / Wt, tx0 = rem0 - ty0 * Wt;
  const int re = (tid >> 4) & 3, rc4 = (tid & 15) * 4;
  int s_img[8], s_tyx[8];   // image; ty | tx << 16 (ty = 0xffff: not this block's tile)
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int tl = wave + WM_NW * r;
    const unsigned n = (unsigned)(tx0 + tl), q = n / (unsigned)Wt, tx = n - q * (unsigned)Wt;
    const unsigned m = (unsigned)ty0 + q, q2 = m / (unsigned)Ht, ty = m - q2 * (unsigned)Ht;
    s_img[r] = bimg0 + (int)q2;
    s_tyx[r] = t0 + tl < tend ? (int)(ty | (tx << 16)) : 0xffff;
  }
  if (POOL != 1) {
    // four passes, one output row a of the 4x4 tiles each: [tile][e][channel]
#pragma unroll
    for (int a = 0; a < 4; a++) {
      float* sY = smem + (a & 1) * SYF;
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int tl = 16 * b + 4 * lk + i;
#pragma unroll
          for (int e = 0; e < 4; e++) sY[(tl * 4 + e) * 64 + wcol] = YO(b, i, 4 * a + e);
        }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const int tl = wave + WM_NW * r;
        const int ty = s_tyx[r] & 0xffff, tx = s_tyx[r] >> 16;
        const int oy = 4 * ty + a, ox = 4 * tx + re;
        if (oy < H && ox < W) {   // ty = 0xffff fails here
          const v4f o4 = *reinterpret_cast<const v4f*>(&sY[(tl * 4 + re) * 64 + (rc4 ^ (16 * ((tl >> 2) & 3)))]);
          if constexpr (ABL & ABL_NO_STORES) { if (o4[0] == 12345.678f) y[tid] = o4[1]; }
          else if constexpr (ABL & ABL_NT_STORES) __builtin_nontemporal_store(o4, reinterpret_cast<v4f*>(y + (((long long)s_img[r] * H + oy) * W + ox) * Cout + cb * WM_BC + rc4));
          else *reinterpret_cast<v4f*>(y + (((long long)s_img[r] * H + oy) * W + ox) * Cout + cb * WM_BC + rc4) = o4;
        }
      }
    }
  }
  if (POOL != 0) {
    // pooled 2x2 windows of the 4x4 tile: [tile][2 a' + e'][channel]
    float* yp = POOL == 1 ? y : ypool;
    float* sY = smem;   // pass "4": buffer 0 again (its readers of pass 2 are behind barrier 3)
    const int Hp = H / 2, Wp = W / 2;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int tl = 16 * b + 4 * lk + i;
#pragma unroll
        for (int a2 = 0; a2 < 2; a2++)
#pragma unroll
          for (int e2 = 0; e2 < 2; e2++) {
            float p = YO(b, i, 4 * (2 * a2) + 2 * e2);
            const float p1 = YO(b, i, 4 * (2 * a2) + 2 * e2 + 1), p2 = YO(b, i, 4 * (2 * a2 + 1) + 2 * e2),
                        p3 = YO(b, i, 4 * (2 * a2 + 1) + 2 * e2 + 1);
            p = p1 > p ? p1 : p;
            p = p2 > p ? p2 : p;
            p = p3 > p ? p3 : p;
            sY[(tl * 4 + 2 * a2 + e2) * 64 + wcol] = p;
          }
      }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int tl = wave + WM_NW * r;
      const int ty = s_tyx[r] & 0xffff, tx = s_tyx[r] >> 16;
      const int py = 2 * ty + (re >> 1), px = 2 * tx + (re & 1);
      if (py < Hp && px < Wp)
        *reinterpret_cast<v4f*>(yp + (((long long)s_img[r] * Hp + py) * Wp + px) * Cout + cb * WM_BC + rc4) =
            *reinterpret_cast<const v4f*>(&sY[(tl * 4 + re) * 64 + (rc4 ^ (16 * ((tl >> 2) & 3)))]);
    }
  }
}

#undef YO

// Split-Cin reduction: y = [ReLU](sum_s part[s] + bias) [2x2 max-pooled], partials in ascending order.
// POOL as in the main kernel. One thread per float4 of the (pooled, for POOL != 0) output.
template <int POOL>
__global__ __launch_bounds__(256) void wino43_splitk_reduce_kernel(
    const float* __restrict__ part, int S, long long stride, const float* __restrict__ bias, int relu,
    float* __restrict__ y, float* __restrict__ ypool, int B, int H, int W, int C, int imgs_per_group)
{
  const int c4n = C >> 2;
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  const long long total = (long long)B * Ho * Wo * c4n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % c4n) * 4;
    long long r = i / c4n;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const v4f bv = *reinterpret_cast<const v4f*>(bias + (size_t)(b / imgs_per_group) * C + c4);
    v4f best = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < (POOL ? 4 : 1); q++) {
      const int yy = POOL ? 2 * oy + (q >> 1) : oy, xx = POOL ? 2 * ox + (q & 1) : ox;
      const long long o = (((long long)b * H + yy) * W + xx) * C + c4;
      v4f v = *reinterpret_cast<const v4f*>(part + o);
      for (int s2 = 1; s2 < S; s2++) v += *reinterpret_cast<const v4f*>(part + s2 * stride + o);
      v += bv;
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
      if (POOL != 1) *reinterpret_cast<v4f*>(y + o) = v;
      if (q == 0) best = v;
      else {
#pragma unroll
        for (int e = 0; e < 4; e++) best[e] = v[e] > best[e] ? v[e] : best[e];
      }
    }
    if (POOL != 0) {
      float* yp = POOL == 1 ? y : ypool;
      *reinterpret_cast<v4f*>(yp + (((long long)b * Ho + oy) * Wo + ox) * C + c4) = best;
    }
  }
}

// Cin split of a launch too small to fill the chip (batch-1 conv4_x / conv5_x: 80 / 24 workgroups of 288
// stages each for 512 slots — pure per-workgroup latency): double while the grid stays within the slots
int wino43_cin_split(long long nbt, int ncb, int Cin)
{
  const int NK = Cin / WM_KC;
  int S = 1;
  // Measured round 3 on one frame (tools/bench_wino_mfma.py --batch 1 --groups 1, conv4_2: 80 workgroups of 288 stages):
  // S = 1 186 us, 2 111, 4 107, 8 129 (the reduction reads S partial outputs); conv3_x (152 workgroups) 104 us split or
  // not. A 6-deep LDS ring (prefetch distance 5, one workgroup per CU) made every small launch SLOWER (conv4_2 107 -> 126,
  // conv5_x 66 -> 82), and with one workgroup per CU ring depths 3 / 4 / 5 time the same (conv4_2, S = 1: 184 / 186 / 188 us;
  // S = 2: 111 / 114 / 113): a lone workgroup keeps its MFMA pipe ~65 % busy whatever the prefetch depth — what a small
  // launch lacks is a second workgroup per CU, not operand cover.
  // Round 4: 16-tile workgroups for these launches (the kernel above with one A block per wave: twice the workgroups, half
  // the matrix work each, 176 VGPRs; bit-identical) — conv3_2 at one frame 102 -> 97 us, conv4_x 103 -> 103, conv5_x 42 -> 44,
  // the one-frame trunk 0.893 -> 0.888 ms: a half-size workgroup waits as long for its operands as a full one. Dropped.
  if (nbt * ncb >= 128) return 1;   // (152 workgroups — batch-1 conv3_x — measured slower split in two: the partials cost more than they buy)
  while (S < 8 && nbt * ncb * S * 2 <= 512 && NK % (2 * S) == 0) S *= 2;
  return S;
}

}  // namespace

extern "C" int pcnn_winograd43_conv_workspace_bytes(int B, int H, int W, int Cin, int Cout, int groups, size_t* bytes)
{
  PCNN_REQUIRE(bytes, PCNN_ENULL, "winograd43_conv_workspace_bytes: NULL output");
  PCNN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 64 && Cout >= 64 && groups >= 1 && B % groups == 0, PCNN_EINVAL,
               "winograd43_conv_workspace_bytes: bad shape");
  const long long tpg = (long long)B * ((H + 3) / 4) * ((W + 3) / 4) / groups;
  const int S = wino43_cin_split((long long)groups * ((tpg + WM_BT - 1) / WM_BT), Cout / WM_BC, Cin);
  *bytes = S > 1 ? sizeof(float) * ((size_t)S * B * H * W * Cout + (size_t)groups * Cout) : 0;
  return PCNN_OK;
}

// Both entries of the kernel: `packed` = the filter bank is the fragment-major one of pcnn_winograd43_pack_filters_fwd
// and the kernel takes it straight into registers (BSRC = 1).
static int wino43_conv_launch(bool packed, const float* v, const float* ut, const float* bias, int B, int H,
                              int W, int Cin, int Cout, int groups, int relu, int pool,
                              float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                              void* stream_)
{
  PCNN_REQUIRE(B >= 1 && H >= 1 && W >= 1, PCNN_EINVAL, "winograd43_conv: bad shape %dx%dx%d", B, H, W);
  PCNN_REQUIRE(Cin >= 64 && Cin % 64 == 0, PCNN_EINVAL, "winograd43_conv: input channels must be a multiple of 64 (got %d)", Cin);
  PCNN_REQUIRE(Cout >= 64 && Cout % 64 == 0, PCNN_EINVAL, "winograd43_conv: output channels must be a multiple of 64 (got %d)", Cout);
  PCNN_REQUIRE(pool >= 0 && pool <= 2, PCNN_EINVAL, "winograd43_conv: pool must be 0 (none), 1 (pooled only) or 2 (both)");
  PCNN_REQUIRE(!pool || (H % 2 == 0 && W % 2 == 0), PCNN_EINVAL, "winograd43_conv: pooling needs even height/width");
  PCNN_REQUIRE(groups >= 1 && B % groups == 0, PCNN_EINVAL, "winograd43_conv: batch %d is not a multiple of groups %d", B, groups);
  PCNN_REQUIRE(v && ut && bias && y && (pool != 2 || y_pool), PCNN_ENULL, "winograd43_conv: NULL pointer");
  PCNN_REQUIRE(aligned16(v) && aligned16(ut) && aligned16(bias) && aligned16(y) && (pool != 2 || aligned16(y_pool)), PCNN_EINVAL,
               "winograd43_conv: pointers (v, ut, bias, y, y_pool) must be 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  const int Ht = (H + 3) / 4, Wt = (W + 3) / 4;
  const long long T = (long long)B * Ht * Wt;
  const long long tpg = T / groups;
  const int ncb = Cout / WM_BC;
  // 32-tile blocks, two independent 4-wave workgroups per CU, for every layer: the pair drifts out of phase,
  // so one workgroup's barrier waits, column folds, epilogue stores and block turnover run under the other's
  // MFMAs (the numbers against 64-tile blocks, one 8-wave workgroup per CU, are at the kernel).
  const long long nbt = (long long)groups * ((tpg + WM_BT - 1) / WM_BT);
  const long long blocks = ((nbt + 7) / 8) * 8 * ncb;
  PCNN_REQUIRE(blocks < (1ll << 31), PCNN_EINVAL, "winograd43_conv: grid too large");
  // the kernel addresses a plane of V and of U^T with 32-bit byte offsets from 64-bit plane bases (the packed bank's plane
  // is as large as the row-major one's, Cout * Cin floats; there the lane's offset is 16 * lane and the rest rides in the base)
  PCNN_REQUIRE(T * Cin < (1ll << 30) && (long long)Cout * Cin < (1ll << 30), PCNN_EINVAL,
               "winograd43_conv: a transform plane of %lld x %d (or %d x %d) floats exceeds the kernel's 32-bit byte offsets", T, Cin, Cout, Cin);
  // optional Cin split for launches that cannot fill the chip (needs the caller's workspace)
  int S = wino43_cin_split(nbt, ncb, Cin);
  const size_t out_elems = (size_t)B * H * W * Cout;
  if (S > 1 && !(workspace && aligned16(workspace) && workspace_bytes >= sizeof(float) * (S * out_elems + (size_t)groups * Cout))) S = 1;
  // Block map (see the kernel). cb-major: every XCD owns one channel block and streams its eighth of the filter bank
  // once; pays when U outweighs V — the deep layers of a single frame (conv4_2: U 37.7 MB, V 22 MB: fabric traffic
  // 8 U + V = 324 MB tile-block-major, U + 8 V = 215 MB channel-block-major; conv5_x 307 -> 85 MB: 64 -> 42 us).
  // PCNN_WINO_MODE overrides the map for experiments and the variant-equality test: 1 = cb-major wherever ncb == 8,
  // 0 = never; unset = the library's choice. (The round-4 kernel variants this switch also selected — the one-wave-per-
  // SIMD 32x32x2 kernel, the round-3 zeroing v_movs — left the library in round 5: tools/variants/)
  static const int env_mode = [] { const char* e = getenv("PCNN_WINO_MODE"); return e ? atoi(e) : -1; }();
  const double u_bytes = 36.0 * Cout * (double)Cin * 4.0 * groups, v_bytes = 36.0 * (double)T * Cin * 4.0;
  int mode = (ncb == 8 && u_bytes > v_bytes) ? 1 : 0;
  if (env_mode >= 0) mode = ((env_mode & 1) && ncb == 8) ? 1 : 0;
  const long long nblocks = (mode & 1) ? 8 * nbt : blocks;
#define WM_GO_(K, Y, BIAS, RELU, KS, STRIDE) PCNN_LAUNCH(K, dim3((unsigned)nblocks, KS), dim3(64 * WM_NW), 0, stream, v, ut, BIAS, Y, y_pool, \
                             H, W, Cin, Cout, Ht, Wt, T, tpg, RELU, (int)nbt, ncb, KS, (long long)(STRIDE), mode)
#define WM_GO(P, Y, BIAS, RELU, KS, STRIDE)                                      \
  do {                                                                           \
    if (packed && ((Cin / WM_KC / (KS)) & 1)) WM_GO_((wino43_mfma_kernel<P, 1, 0, 1>), Y, BIAS, RELU, KS, STRIDE); \
    else if (packed) WM_GO_((wino43_mfma_kernel<P, 1>), Y, BIAS, RELU, KS, STRIDE);   \
    else WM_GO_((wino43_mfma_kernel<P>), Y, BIAS, RELU, KS, STRIDE);             \
  } while (0)
  if (S == 1) {
    if (pool == 0) WM_GO(0, y, bias, relu, 1, 0); else if (pool == 1) WM_GO(1, y, bias, relu, 1, 0); else WM_GO(2, y, bias, relu, 1, 0);
  } else {
    float* part = static_cast<float*>(workspace);
    WM_GO(0, part, (const float*)nullptr, 0, S, out_elems);
    const long long items = (long long)B * (pool ? (H / 2) * (W / 2) : H * W) * (Cout / 4);
    const unsigned rgrid = (unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536);
    if (pool == 0)
      PCNN_LAUNCH(wino43_splitk_reduce_kernel<0>, dim3(rgrid), dim3(256), 0, stream, part, S, (long long)out_elems, bias, relu, y, y_pool, B, H, W, Cout, B / groups);
    else if (pool == 1)
      PCNN_LAUNCH(wino43_splitk_reduce_kernel<1>, dim3(rgrid), dim3(256), 0, stream, part, S, (long long)out_elems, bias, relu, y, y_pool, B, H, W, Cout, B / groups);
    else
      PCNN_LAUNCH(wino43_splitk_reduce_kernel<2>, dim3(rgrid), dim3(256), 0, stream, part, S, (long long)out_elems, bias, relu, y, y_pool, B, H, W, Cout, B / groups);
  }
  return check_launch(packed ? "winograd43_conv_packed_fwd" : "winograd43_conv_fwd");
}

extern "C" int pcnn_winograd43_conv_fwd(const float* v, const float* ut, const float* bias, int B, int H,
                                        int W, int Cin, int Cout, int groups, int relu, int pool,
                                        float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                                        void* stream_)
{
  return wino43_conv_launch(false, v, ut, bias, B, H, W, Cin, Cout, groups, relu, pool, y, y_pool, workspace, workspace_bytes, stream_);
}

extern "C" int pcnn_winograd43_conv_packed_fwd(const float* v, const float* utp, const float* bias, int B, int H,
                                               int W, int Cin, int Cout, int groups, int relu, int pool,
                                               float* y, float* y_pool, void* workspace, size_t workspace_bytes,
                                               void* stream_)
{
  return wino43_conv_launch(true, v, utp, bias, B, H, W, Cin, Cout, groups, relu, pool, y, y_pool, workspace, workspace_bytes, stream_);
}

namespace {

// ut [group][36][Cout][Cin] -> utp [group][36][Cout/16][Cin/64][4 (K group j)][64 (lane = 16 lk + lr)][4]:
//   utp[g][k][n16][kc][j][16 lk + lr][e] = ut[g][k][16 n16 + lr][64 kc + 16 j + 4 lk + e]
// — the order in which a wave of wino43_mfma_kernel<., 1> consumes its B operand: one wave-wide 16-byte load is one
// contiguous KB, a stage's four loads 4 KB. A plain permutation, one float4 per thread, run once per filter.
__global__ __launch_bounds__(256) void wino43_pack_filters_kernel(const float* __restrict__ ut, float* __restrict__ utp,
                                                                  int Cin, int Cout, long long total4)
{
  const int nkc = Cin / WM_KC, n16n = Cout / 16;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total4; o += (long long)gridDim.x * 256) {
    const int l = (int)(o & 63), j = (int)((o >> 6) & 3);
    long long r = o >> 8;
    const int kc = (int)(r % nkc); r /= nkc;
    const int n16 = (int)(r % n16n);
    const long long gk = r / n16n;   // 36 g + k
    const int lr = l & 15, lk = l >> 4;
    const long long src = (gk * Cout + 16 * n16 + lr) * Cin + 64 * kc + 16 * j + 4 * lk;
    *reinterpret_cast<v4f*>(utp + 4 * o) = *reinterpret_cast<const v4f*>(ut + src);
  }
}

}  // namespace

extern "C" int pcnn_winograd43_pack_filters_fwd(const float* ut, int Cin, int Cout, int groups, float* utp, void* stream_)
{
  PCNN_REQUIRE(Cin >= 64 && Cin % 64 == 0, PCNN_EINVAL, "winograd43_pack_filters: input channels must be a multiple of 64 (got %d)", Cin);
  PCNN_REQUIRE(Cout >= 64 && Cout % 64 == 0, PCNN_EINVAL, "winograd43_pack_filters: output channels must be a multiple of 64 (got %d)", Cout);
  PCNN_REQUIRE(groups >= 1, PCNN_EINVAL, "winograd43_pack_filters: groups must be positive (got %d)", groups);
  PCNN_REQUIRE(ut && utp, PCNN_ENULL, "winograd43_pack_filters: NULL pointer");
  PCNN_REQUIRE(ut != utp, PCNN_EINVAL, "winograd43_pack_filters: not an in-place permutation");
  PCNN_REQUIRE(aligned16(ut) && aligned16(utp), PCNN_EINVAL, "winograd43_pack_filters: pointers (ut, utp) must be 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  const long long total4 = (long long)groups * 36 * Cout * Cin / 4;
  const unsigned grid = (unsigned)((total4 + 255) / 256 < 65536 ? (total4 + 255) / 256 : 65536);
  PCNN_LAUNCH(wino43_pack_filters_kernel, dim3(grid), dim3(256), 0, stream, ut, utp, Cin, Cout, total4);
  return check_launch("winograd43_pack_filters_fwd");
}
