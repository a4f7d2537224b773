// mfma_ring.h — what the two dense fp32-MFMA kernels (csrc/wino_mfma.hip: the trunk, csrc/fc_mfma.hip: fc6 / fc7 and the
// 1x1 heads) share: operands go global -> LDS by DMA into a ring of stage buffers and come back with ds_read_b128.
//
// The LDS image of a stage is the DMA's lane-linear one: rows of 64 floats (16 chunks of 16 bytes), unpadded, four rows per
// DMA instruction (lane l lands at row l >> 4, physical chunk l & 15). Bank conflicts are avoided by an XOR swizzle of the
// chunk index with the row — logical chunk c of row r lives at physical chunk c ^ (r & 15) — applied to the SOURCE address
// of the DMA (ring_src_col) and to the address of the read (ring_chunk_bytes): the same involution on both sides.
//
// Ring protocol (the stage bodies differ and stay in the two files; the rules do not):
//   * One rendezvous per 64-deep K stage, a raw s_barrier behind a COUNTED s_waitcnt vmcnt(N): N = the DMA instructions a
//     wave issues per stage, so the wave's DMAs of THIS stage have landed while those of the next stay in flight
//     (__syncthreads() would drain the queue). The two-buffer ring of fc_mfma.hip has no stage in flight there: N = 0.
//   * The DMAs and the LDS reads are inline asm, invisible to the compiler's own s_waitcnt insertion (which collapses to
//     lgkmcnt(0) across a loop back edge). Every wait is placed by hand: lgkmcnt(0) inside the stage barrier retires the
//     second half stage's reads, one lgkmcnt(0) after its MFMAs retires the first half's; sched_barrier(0) pins the order.
//   * For the same reason the __syncthreads() that hands the ring to the epilogue as its staging buffer is a bare
//     s_barrier: an explicit s_waitcnt vmcnt(0) must stand IN FRONT of it, or another wave's parked prefetch lands on
//     staged output rows. The comment at that wait in fc_mfma.hip has the story of the bug.
//   * The ring position travels in the offset field of the reads (one copy of a half stage's six reads per buffer behind
//     a scalar branch): a lane's chunk addresses are loop invariants and a stage has no vector-ALU instruction between its
//     MFMAs — on gfx950 a VALU instruction is never hidden behind an MFMA of its SIMD.
//   * An operand that only its own wave reads need not pass through the ring at all (wino_mfma.hip, BSRC = 1: a wave's 16
//     filter rows). It comes by RING_GLOAD_B128 straight into registers, one stage ahead, and its loads sit in the SAME vmcnt
//     queue as the DMAs, in issue order. So the order of issue inside a stage is part of the protocol: the register loads
//     of stage s+1 go out BEFORE the DMAs of stage s+2, and N of the counted wait stays the DMA instructions per stage —
//     everything older than the youngest stage's DMAs, this stage's registers included, has then landed. A register with
//     a load in flight is not read, moved or reused before that wait: the compiler does not know the load is pending, so
//     this is checked in the ISA (roles of the register sets fixed at compile time; no copy of them in the loop).
#pragma once

namespace pcnn {

typedef float v4f __attribute__((ext_vector_type(4)));

// 16 bytes per lane, global -> LDS, no register round trip: SGPR base + 32-bit VGPR byte offset, LDS destination =
// wave-uniform base (M0) + 16 * lane. Spelled out in asm because through __builtin_amdgcn_global_load_lds the compiler turned
// most of these into 64-bit VGPR addresses (a v_mov_b64 + v_lshl_add_u64 pair per load, ~20 VALU instructions per stage next to
// 32 MFMAs); here the per-stage pointer arithmetic stays on the scalar unit. Completion: the hand-placed vmcnt waits above.
__device__ __forceinline__ void glds16_s(const char* sbase, unsigned voff, unsigned lds_addr)
{
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1"
               :: "v"(voff), "s"(sbase), "s"(lds_addr) : "memory", "m0");
}

// DMA side of the swizzle: the source column (floats) that lane (lr = lane & 15) fetches for stage row `row`
__device__ __forceinline__ int ring_src_col(int lr, int row) { return (lr ^ (row & 15)) * 4; }
// read side: byte offset inside its row of the chunk that lane (lr, lk = lane >> 4) reads for K group j — the lane's row is
// (a multiple of 16) + lr, and K is consumed in the order 16 j + 4 lk + i for both operands (one b128 read feeds 4 MFMAs)
__device__ __forceinline__ unsigned ring_chunk_bytes(int j, int lk, int lr) { return (unsigned)(((4 * j + lk) ^ lr) * 16); }

}  // namespace pcnn

// the ring position OFF (a compile-time constant) is part of the instruction, not of the address
#define RING_DSREAD_B128(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "i"(OFF))

// 16 bytes per lane, global -> registers, beside the DMAs and in their vmcnt queue: SGPR base + 32-bit VGPR byte offset
// + a compile-time offset (13 bits, signed). DST must not be read, moved or reused before the hand-placed vmcnt wait
// that covers it.
#define RING_GLOAD_B128(DST, SBASE, VOFF, OFF) \
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(DST) : "v"(VOFF), "s"(SBASE), "i"(OFF) : "memory")
