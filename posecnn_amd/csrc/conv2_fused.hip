// conv2_fused.hip — conv2_1 / conv2_2 (3x3, stride 1, SAME, Cin = 64 | 128 -> Cout = 128, vgg16_convs.py:40-42 and the depth
// tower :57-59) as ONE kernel per layer: Winograd F(4x4,3x3) input transform, the 36 contractions and the output transform
// (+ bias, ReLU, 2 x 2 max-pool) without the transformed input V ever leaving the CU. The unfused pair writes V (2.25 x the
// layer's input) with wino43_input_kernel and reads it back with wino43_mfma_kernel.
//
// Modelled on phase 2 and the epilogue of conv12_wino43_fused_kernel (csrc/conv_first.hip). A workgroup owns a 4 x 4 block of
// tiles (16 x 16 output pixels) of one image; 512 threads, one workgroup per CU (LDS 137 KB). Wave w owns output channels
// 16 w .. 16 w + 15 and the 36 accumulators of its 16 tiles (144 VGPRs). With Cout = 128 all eight waves carry matrix work,
// so every wave is producer and consumer in turn: in step s all produce plane group s (row xi = s of B^T d B) into one of two
// LDS buffers and then contract group s - 1 out of the other, one barrier per step.
//   per 64-channel half h of Cin:
//     patch    the 18 x 18 x 64 input patch of the block into LDS (zeros outside the image: SAME padding), 68 floats per
//              pixel; a thread's (up to) 11 float4 are requested together. The second half's patch is requested under the
//              last contraction of the first (in three batches, to stay inside the register file).
//     produce  thread = (tile, channel pair) builds the six planes of row xi with the expression trees of fw_bt6 /
//              wino43_input_kernel on float2 and parks them XOR-swizzled (16-byte chunks) as the A operand;
//     consume  v_mfma_f32_16x16x4_f32, two planes interleaved, B straight from the fragment-major bank of
//              pcnn_winograd43_pack_filters_fwd ([groups][36][Cout/16][Cin/64][4][64][4]) into registers, two planes ahead.
//   Half 1 continues the accumulators of half 0: every accumulator sees k = 64 h + 16 j + 4 (lane >> 4) + i ascending with
//   C = 0 first — the chain of wino43_mfma_kernel.
//   epilogue the column-by-column fold of wino43_mfma_kernel (t = A^T M[:, nu], Y += t (x) A[nu, :]), bias, ReLU, 2 x 2 max,
//            staged through LDS so that stores are whole 512-byte pixel rows.
// Bit-identical to pcnn_winograd43_input_fwd + pcnn_winograd43_conv_packed_fwd wherever that entry does not split Cin
// (tests/test_gpu_conv2_fused.py; the header has the rule).
#include "pcnn_device.h"
#include "../../include/posecnn_hip/trunk/conv2_fused.h"

namespace {

using namespace pcnn;

constexpr int C2_P = 18;                          // patch rows / columns of a 4 x 4 tile block
constexpr int C2_YS = 68;                         // floats per patch pixel (64 channels + 4 of padding)
constexpr int C2_PATCH = C2_P * C2_P * C2_YS;     // 22 032 floats
constexpr int C2_GRP = 6 * 16 * 64;               // a group buffer: 6 planes x 16 tiles x 64 channels
constexpr int C2_SMEM = C2_PATCH + 2 * C2_GRP;    // 34 320 floats = 137 280 B; the epilogue stages 16 x 16 x 128 = 32 768 in it
constexpr int C2_NPV = (C2_P * C2_P * 16 + 511) / 512;   // float4 of the patch per thread: 11, the last one on one wave only

typedef float c2v4 __attribute__((ext_vector_type(4)));

// A wave-uniform pointer, opaque to the optimiser: what is added to it afterwards is the lane's part, so the load addresses
// as SGPR base + 32-bit VGPR offset. (Left alone, the compiler folds the lane's offset into the base first and then adds
// every plane's constant — too large for the offset field — with two VALU instructions per load and a register pair each.)
typedef const __attribute__((address_space(1))) float* c2gptr;   // (a pointer rebuilt from integers is a flat one unless it says so)
typedef const __attribute__((address_space(1))) c2v4* c2gptr4;
__device__ __forceinline__ c2gptr c2_uniform(const float* p)
{
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return (c2gptr)(((unsigned long long)hi << 32) | lo);
}

template <int KH, int POOL>
__global__ __launch_bounds__(512, 1) void conv2_wino43_fused_kernel(
    const float* __restrict__ x, const float* __restrict__ utp, const float* __restrict__ bias, float* __restrict__ y,
    int H, int W, int nbx, int nby, int imgs_per_group, int relu)
{
  constexpr int CIN = 64 * KH;
  __shared__ __attribute__((aligned(16))) float smem[C2_SMEM];
  float* const s_y = smem;
  float* const s_v = smem + C2_PATCH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (readfirstlane: an integer division by a run-time value goes through the vector ALU, and everything derived from its
  //  result — the filter set's base, every plane's address — would follow it there)
  const int b = __builtin_amdgcn_readfirstlane(blockIdx.x / (nbx * nby));
  const int by = __builtin_amdgcn_readfirstlane((blockIdx.x / nbx) % nby), bx = __builtin_amdgcn_readfirstlane(blockIdx.x % nbx);
  const int py0 = 16 * by - 1, px0 = 16 * bx - 1;   // image coordinates of patch pixel (0, 0)
  const int grp = __builtin_amdgcn_readfirstlane(b / imgs_per_group);
  utp += (size_t)grp * 36 * 128 * CIN;
  const float bv = bias[(size_t)grp * 128 + 16 * wave + (lane & 15)];   // requested here, used in the epilogue

  // ---- the patch of half HH: elements E0 .. E1 - 1 of the thread's C2_NPV float4 (pixel i >> 4, channel quad i & 15) ----
  c2v4 pv[C2_NPV];
  const float* xb = x + (size_t)b * H * W * CIN;
#define C2_LOADP(E0, E1, HH, TID)                                                                                  \
  _Pragma("unroll") for (int e = (E0); e < (E1); e++) {                                                         \
    const int i = (TID) + 512 * e;                                                                              \
    const int p = i >> 4, q = i & 15;                                                                           \
    const int r = p / C2_P, c = p - C2_P * r;                                                                   \
    const int iy = py0 + r, ix = px0 + c;                                                                       \
    const bool ok = i < C2_P * C2_P * 16 && iy >= 0 && iy < H && ix >= 0 && ix < W;                             \
    const unsigned pix = ok ? (unsigned)(iy * W + ix) : 0u;   /* (outside: any valid address, value dropped) */ \
    c2v4 val = *reinterpret_cast<const c2v4*>(xb + (pix * CIN + 64 * (HH) + 4 * q));                            \
    if (!ok) val = (c2v4){0.f, 0.f, 0.f, 0.f};                                                                  \
    pv[e] = val;                                                                                                \
  }
#define C2_STOREP(E0, E1, TID)                                                                                  \
  _Pragma("unroll") for (int e = (E0); e < (E1); e++) {                                                         \
    const int i = (TID) + 512 * e;                                                                              \
    if (i < C2_P * C2_P * 16) *reinterpret_cast<c2v4*>(&s_y[(i >> 4) * C2_YS + 4 * (i & 15)]) = pv[e];          \
  }
  C2_LOADP(0, C2_NPV, 0, tid)
  C2_STOREP(0, C2_NPV, tid)

  const int lr = lane & 15, lk = lane >> 4;
  const int tile = tid >> 5, cp = tid & 31;            // producer item: (tile, channel pair)
  const int tyy = tile >> 2, txx = tile & 3;
  // every LDS access of the lane = one of these bases + a compile-time offset (the offset field of the instruction): written
  // out per access, the compiler keeps one address register for each of them
  const float* const yb = s_y + ((4 * tyy) * C2_P + 4 * txx) * C2_YS + 2 * cp;                 // the tile's patch corner
  float* const vb = s_v + tile * 64 + (((cp >> 1) ^ tile) * 4) + 2 * (cp & 1);                 // the producer's slot in a plane
  const float* ab[4];                                                                          // the A operand's K groups
#pragma unroll
  for (int g = 0; g < 4; g++) ab[g] = s_v + lr * 64 + (((4 * g + lk) ^ lr) * 4);
  v4f acc[36];
  c2v4 a0[4], a1[4], q0[4], q1[4];
  // fragment-major bank: [plane][wave][half][K group][lane][4]; the wave's corner of plane 0 as a scalar
  const float* const utw = (const float*)c2_uniform(utp + wave * KH * 1024);
  const unsigned foff = (unsigned)(lane * 4);
  // B operands (K group G of half HH) of planes K, K + 1
#define C2_LOADB(D0, D1, K, HH, G)                                                                              \
  { const c2gptr pk0_ = c2_uniform(utw + (size_t)(K) * (128 * CIN) + 1024 * (HH));                              \
    const c2gptr pk1_ = c2_uniform(utw + (size_t)((K) + 1) * (128 * CIN) + 1024 * (HH));                        \
    D0 = *(c2gptr4)(pk0_ + (foff + 256 * (G)));                                                                 \
    D1 = *(c2gptr4)(pk1_ + (foff + 256 * (G))); }
#define C2_LOADA(D0, D1, BUF, J, G)                                                                             \
  { D0 = *reinterpret_cast<const c2v4*>(ab[G] + ((BUF) * C2_GRP + (J) * 1024));                                 \
    D1 = *reinterpret_cast<const c2v4*>(ab[G] + ((BUF) * C2_GRP + ((J) + 1) * 1024)); }
  // row XI of B^T d B for the thread's (tile, channel pair): the trees of fw_bt6 / wino43_input_kernel on float2
#define C2_PRODUCE(XI, BUF)                                                                                     \
  {                                                                                                             \
    f2 ta[6];                                                                                                   \
    _Pragma("unroll") for (int hh = 0; hh < 2; hh++) {                                                          \
      f2 d[3][6];                                                                                               \
      _Pragma("unroll") for (int s3 = 0; s3 < 3; s3++)                                                          \
        _Pragma("unroll") for (int r = 0; r < 6; r++)                                                           \
          if (((XI) == 0 && (r == 0 || r == 2 || r == 4)) || ((XI) == 5 && (r == 1 || r == 3 || r == 5)) ||     \
              ((XI) >= 1 && (XI) <= 4 && r >= 1 && r <= 4))                                                     \
            d[s3][r] = *reinterpret_cast<const f2*>(yb + (r * C2_P + 3 * hh + s3) * C2_YS);                     \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
      _Pragma("unroll") for (int s3 = 0; s3 < 3; s3++) {                                                        \
        const int s2 = 3 * hh + s3;                                                                             \
        if ((XI) == 0) ta[s2] = (4.f * d[s3][0] - 5.f * d[s3][2]) + d[s3][4];                                   \
        else if ((XI) == 5) ta[s2] = (4.f * d[s3][1] - 5.f * d[s3][3]) + d[s3][5];                              \
        else if ((XI) == 1 || (XI) == 2) {                                                                      \
          const f2 a = d[s3][4] - 4.f * d[s3][2], b_ = d[s3][3] - 4.f * d[s3][1];                               \
          ta[s2] = (XI) == 1 ? a + b_ : a - b_;                                                                 \
        } else {                                                                                                \
          const f2 c = d[s3][4] - d[s3][2], e = 2.f * (d[s3][3] - d[s3][1]);                                    \
          ta[s2] = (XI) == 3 ? c + e : c - e;                                                                   \
        }                                                                                                       \
      }                                                                                                         \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
    }                                                                                                           \
    f2 oa[6];                                                                                                   \
    oa[0] = (4.f * ta[0] - 5.f * ta[2]) + ta[4];                                                                \
    { const f2 a = ta[4] - 4.f * ta[2], b_ = ta[3] - 4.f * ta[1]; oa[1] = a + b_; oa[2] = a - b_; }             \
    { const f2 c = ta[4] - ta[2], e = 2.f * (ta[3] - ta[1]); oa[3] = c + e; oa[4] = c - e; }                    \
    oa[5] = (4.f * ta[1] - 5.f * ta[3]) + ta[5];                                                                \
    _Pragma("unroll") for (int j = 0; j < 6; j++)                                                               \
      *reinterpret_cast<f2*>(vb + ((BUF) * C2_GRP + j * 1024)) = oa[j];                                         \
  }
  // planes 6 XI + J, 6 XI + J + 1 of half HH out of buffer BUF, their MFMAs interleaved (back-to-back MFMAs into one
  // accumulator issue at half rate). On entry q0 / q1 hold their B operands, a0 / a1 their A operands unless J == 0 (first
  // pair behind the step's barrier: fetched here). Behind the MFMAs of a K group the next pair's operands are requested into
  // the registers just read: A of the same group, B of planes NK, NK + 1 of half NH (NK < 0: none).
#define C2_PAIR(XI, J, BUF, HH, NK, NH)                                                                         \
  {                                                                                                             \
    if ((J) == 0) { _Pragma("unroll") for (int g_ = 0; g_ < 4; g_++) C2_LOADA(a0[g_], a1[g_], BUF, 0, g_) }     \
    v4f ca_, cb_;                                                                                               \
    if ((HH) == 0) { ca_ = (v4f){0.f, 0.f, 0.f, 0.f}; cb_ = ca_; }                                              \
    else { ca_ = acc[6 * (XI) + (J)]; cb_ = acc[6 * (XI) + (J) + 1]; }                                          \
    _Pragma("unroll") for (int g_ = 0; g_ < 4; g_++) {                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) {                                                        \
        ca_ = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[g_][i_], q0[g_][i_], ca_, 0, 0, 0);                       \
        cb_ = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[g_][i_], q1[g_][i_], cb_, 0, 0, 0);                       \
      }                                                                                                         \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
      if ((J) < 4) { C2_LOADA(a0[g_], a1[g_], BUF, (J) + 2, g_) }                                               \
      if ((NK) >= 0) { C2_LOADB(q0[g_], q1[g_], (NK), (NH), g_) }                                               \
    }                                                                                                           \
    acc[6 * (XI) + (J)] = ca_;                                                                                  \
    acc[6 * (XI) + (J) + 1] = cb_;                                                                              \
  }
  // the B operands behind the last pair of group XI: the next group's first pair, or the next half's
#define C2_NEXTK(XI, HH) ((XI) < 5 ? 6 * (XI) + 6 : (HH) + 1 < KH ? 0 : -1)
#define C2_NEXTH(XI, HH) ((XI) < 5 ? (HH) : (HH) + 1)
#define C2_CONSUME(XI, BUF, HH)                                                                                 \
  C2_PAIR(XI, 0, BUF, HH, 6 * (XI) + 2, HH) C2_PAIR(XI, 2, BUF, HH, 6 * (XI) + 4, HH)                           \
  C2_PAIR(XI, 4, BUF, HH, C2_NEXTK(XI, HH), C2_NEXTH(XI, HH))
#define C2_STEP(S, HH)                                                                                          \
  C2_PRODUCE(S, (S) & 1)                                                                                        \
  __builtin_amdgcn_sched_barrier(0);   /* the group's operand reads stay behind the transform: registers */     \
  C2_CONSUME((S) - 1, ((S) - 1) & 1, HH)                                                                        \
  __syncthreads();

  {
#pragma unroll
    for (int g = 0; g < 4; g++) C2_LOADB(q0[g], q1[g], 0, 0, g)
  }
  __syncthreads();   // the patch of half 0 is in LDS
#pragma unroll
  for (int h = 0; h < KH; h++) {
    C2_PRODUCE(0, 0)
    __syncthreads();
    C2_STEP(1, h) C2_STEP(2, h) C2_STEP(3, h) C2_STEP(4, h) C2_STEP(5, h)
    // step 6: the last group's contraction. Nobody reads the patch any more (group 5 was produced before the barrier of
    // step 5), so the next half's patch replaces it here: requested in front of a plane pair, parked behind it.
    if (h + 1 < KH) {
      // (the thread index through an empty asm: the addresses are computed again here. Recognised as the first patch's, they
      //  would stay in 30 registers through the whole first half, which the 144 accumulators leave no room for)
      int tid2 = tid;
      asm volatile("" : "+v"(tid2));
      C2_LOADP(0, 4, h + 1, tid2)
      C2_PAIR(5, 0, 1, h, 32, h)
      C2_STOREP(0, 4, tid2)
      C2_LOADP(4, 8, h + 1, tid2)
      C2_PAIR(5, 2, 1, h, 34, h)
      C2_STOREP(4, 8, tid2)
      C2_LOADP(8, C2_NPV, h + 1, tid2)
      C2_PAIR(5, 4, 1, h, 0, h + 1)
      C2_STOREP(8, C2_NPV, tid2)
    } else {
      C2_CONSUME(5, 1, h)
    }
    __syncthreads();
  }
#undef C2_STEP
#undef C2_CONSUME
#undef C2_NEXTK
#undef C2_NEXTH
#undef C2_PAIR
#undef C2_PRODUCE
#undef C2_LOADA
#undef C2_LOADB
#undef C2_STOREP
#undef C2_LOADP

  // ---- epilogue: output transform (the MFMA kernel's fold, column by column), bias, ReLU, 2 x 2 max -------------------
  // a lane holds tiles 4 lk + i (i = 0..3: tile row lk, tile column i) x channel 16 wave + lr. Staged through LDS (all of it is
  // free behind the last barrier): [pixel row][pixel column][128], the 16-channel group XORed with lk — the writer lanes of a
  // wave sit whole pixel rows apart, i.e. on the same banks.
  float* const s_o = smem;
  {
    typedef float f2e __attribute__((ext_vector_type(2)));
    const int wcol = (16 * wave + lr) ^ (16 * lk);
#pragma unroll
    for (int ih = 0; ih < 2; ih++) {
      // tiles i = 2 ih, 2 ih + 1 on packed f32: element for element the scalar sequence of wino43_mfma_kernel's fold
      f2e yo[16];
#pragma unroll
      for (int o = 0; o < 16; o++) yo[o] = (f2e){0.f, 0.f};
#pragma unroll
      for (int nu = 0; nu < 6; nu++) {
        const float c0 = nu == 5 ? 0.f : 1.f;
        const float c1 = nu == 1 ? 1.f : nu == 2 ? -1.f : nu == 3 ? 2.f : nu == 4 ? -2.f : 0.f;
        const float c2 = (nu == 1 || nu == 2) ? 1.f : (nu == 3 || nu == 4) ? 4.f : 0.f;
        const float c3 = nu == 1 ? 1.f : nu == 2 ? -1.f : nu == 3 ? 8.f : nu == 4 ? -8.f : nu == 5 ? 1.f : 0.f;
        f2e m_[6], t_[4];
#pragma unroll
        for (int x_ = 0; x_ < 6; x_++) m_[x_] = (f2e){acc[6 * x_ + nu][2 * ih], acc[6 * x_ + nu][2 * ih + 1]};
        {
          const f2e s = m_[1] + m_[2], d = m_[1] - m_[2], S = m_[3] + m_[4], D = m_[3] - m_[4];
          t_[0] = (m_[0] + s) + S;
          t_[1] = __builtin_elementwise_fma((f2e){2.f, 2.f}, D, d);
          t_[2] = __builtin_elementwise_fma((f2e){4.f, 4.f}, S, s);
          t_[3] = __builtin_elementwise_fma((f2e){8.f, 8.f}, D, d) + m_[5];
        }
#pragma unroll
        for (int a_ = 0; a_ < 4; a_++) {
          yo[4 * a_ + 0] = __builtin_elementwise_fma(t_[a_], (f2e){c0, c0}, yo[4 * a_ + 0]);
          yo[4 * a_ + 1] = __builtin_elementwise_fma(t_[a_], (f2e){c1, c1}, yo[4 * a_ + 1]);
          yo[4 * a_ + 2] = __builtin_elementwise_fma(t_[a_], (f2e){c2, c2}, yo[4 * a_ + 2]);
          yo[4 * a_ + 3] = __builtin_elementwise_fma(t_[a_], (f2e){c3, c3}, yo[4 * a_ + 3]);
        }
      }
#pragma unroll
      for (int o = 0; o < 16; o++) {
        f2e val = yo[o] + (f2e){bv, bv};
        if (relu) { val.x = val.x > 0.f ? val.x : 0.f; val.y = val.y > 0.f ? val.y : 0.f; }
        yo[o] = val;
      }
      if (POOL == 0) {
        // tile (row lk, column i), output (a, e) -> pixel (4 lk + a, 4 i + e)
#pragma unroll
        for (int a_ = 0; a_ < 4; a_++)
#pragma unroll
          for (int e_ = 0; e_ < 4; e_++) {
            s_o[((4 * lk + a_) * 16 + 4 * (2 * ih) + e_) * 128 + wcol] = yo[4 * a_ + e_].x;
            s_o[((4 * lk + a_) * 16 + 4 * (2 * ih + 1) + e_) * 128 + wcol] = yo[4 * a_ + e_].y;
          }
      } else {
#pragma unroll
        for (int a2 = 0; a2 < 2; a2++)
#pragma unroll
          for (int e2 = 0; e2 < 2; e2++) {
            f2e p = yo[4 * (2 * a2) + 2 * e2];
            const f2e p1 = yo[4 * (2 * a2) + 2 * e2 + 1], p2 = yo[4 * (2 * a2 + 1) + 2 * e2], p3 = yo[4 * (2 * a2 + 1) + 2 * e2 + 1];
            p.x = p1.x > p.x ? p1.x : p.x; p.y = p1.y > p.y ? p1.y : p.y;
            p.x = p2.x > p.x ? p2.x : p.x; p.y = p2.y > p.y ? p2.y : p.y;
            p.x = p3.x > p.x ? p3.x : p.x; p.y = p3.y > p.y ? p3.y : p.y;
            s_o[((2 * lk + a2) * 8 + (2 * (2 * ih) + e2)) * 128 + wcol] = p.x;       // -> pooled (2 lk + a2, 2 i + e2)
            s_o[((2 * lk + a2) * 8 + (2 * (2 * ih + 1) + e2)) * 128 + wcol] = p.y;
          }
      }
    }
  }
  __syncthreads();
  if (POOL == 0) {
#pragma unroll 4
    for (int i = tid; i < 16 * 16 * 32; i += 512) {
      const int c4 = (i & 31) * 4, pxl = (i >> 5) & 15, pyl = i >> 9;
      *reinterpret_cast<c2v4*>(y + (((size_t)b * H + 16 * by + pyl) * W + 16 * bx + pxl) * 128 + c4) =
          *reinterpret_cast<const c2v4*>(&s_o[(pyl * 16 + pxl) * 128 + (c4 ^ (16 * (pyl >> 2)))]);
    }
  } else {
    const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
    for (int i = tid; i < 8 * 8 * 32; i += 512) {
      const int c4 = (i & 31) * 4, pxl = (i >> 5) & 7, pyl = i >> 8;
      *reinterpret_cast<c2v4*>(y + (((size_t)b * Hp + 8 * by + pyl) * Wp + 8 * bx + pxl) * 128 + c4) =
          *reinterpret_cast<const c2v4*>(&s_o[(pyl * 8 + pxl) * 128 + (c4 ^ (16 * (pyl >> 1)))]);
    }
  }
}

}  // namespace

extern "C" int pcnn_winograd43_conv_fused_fwd(const float* x, const float* utp, const float* bias, int B, int H, int W,
                                              int Cin, int Cout, int groups, int relu, int pool, float* y, void* stream_)
{
  PCNN_REQUIRE(B >= 1 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0, PCNN_EINVAL,
               "winograd43_conv_fused: the frame must be a multiple of 16 in both directions (got %dx%dx%d)", B, H, W);
  PCNN_REQUIRE(Cin == 64 || Cin == 128, PCNN_EINVAL, "winograd43_conv_fused: input channels must be 64 or 128 (got %d)", Cin);
  PCNN_REQUIRE(Cout == 128, PCNN_EINVAL, "winograd43_conv_fused: output channels must be 128 (got %d)", Cout);
  PCNN_REQUIRE(pool == 0 || pool == 1, PCNN_EINVAL, "winograd43_conv_fused: pool must be 0 (none) or 1 (pooled only)");
  PCNN_REQUIRE(groups >= 1 && B % groups == 0, PCNN_EINVAL, "winograd43_conv_fused: batch %d is not a multiple of groups %d", B, groups);
  PCNN_REQUIRE(x && utp && bias && y, PCNN_ENULL, "winograd43_conv_fused: NULL pointer");
  PCNN_REQUIRE(aligned16(x) && aligned16(utp) && aligned16(bias) && aligned16(y), PCNN_EINVAL,
               "winograd43_conv_fused: pointers (x, utp, bias, y) must be 16-byte aligned");
  const long long blocks = (long long)B * (H / 16) * (W / 16);
  PCNN_REQUIRE(blocks < (1ll << 31), PCNN_EINVAL, "winograd43_conv_fused: grid too large");
  // the kernel addresses the pixels of one image with 32-bit element offsets from the image's 64-bit base
  PCNN_REQUIRE((long long)H * W * Cin < (1ll << 30), PCNN_EINVAL,
               "winograd43_conv_fused: an image of %dx%dx%d floats exceeds the kernel's 32-bit offsets", H, W, Cin);
  hipStream_t stream = (hipStream_t)stream_;
#define C2_GO(KH, P)                                                                                              \
  PCNN_LAUNCH((conv2_wino43_fused_kernel<KH, P>), dim3((unsigned)blocks), dim3(512), 0, stream, x, utp, bias, y, H, W, W / 16, \
              H / 16, B / groups, relu)
  if (Cin == 64) { if (pool) C2_GO(1, 1); else C2_GO(1, 0); }
  else { if (pool) C2_GO(2, 1); else C2_GO(2, 0); }
#undef C2_GO
  return check_launch("winograd43_conv_fused_fwd");
}
