// tools/wino_ablate.hip — "ablate before optimizing" (cdna_hip_programming.md §5.4): the fused Winograd
// MFMA kernel of csrc/wino_mfma.hip with one ingredient of its K loop removed per variant, timed with HIP
// events on synthetic buffers at a trunk layer's shape (the ABL_* bits are documented at their enum in csrc/wino_mfma.hip).
// Not part of the library. Build + run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iposecnn_amd/csrc -Iinclude \
//         tools/wino_ablate.hip posecnn_amd/csrc/common.hip -o tools/wino_ablate && tools/wino_ablate 32 60 80 512 512     (B H W Cin Cout)
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "../posecnn_amd/csrc/wino_mfma.hip"

// BSRC = 1: `ut` is read as the fragment-major bank (timing only: synthetic data either way); ODD = the parity of Cin / 64
template <int ABL, int BSRC = 0, int ODD = 0>
static float run(const float* v, const float* ut, const float* bias, float* y, int H, int W, int Cin, int Cout, long long T, int iters)
{
  const int Ht = (H + 3) / 4, Wt = (W + 3) / 4;
  const long long nbt = (T + WM_BT - 1) / WM_BT;
  const int ncb = Cout / 64;
  const long long blocks = ((nbt + 7) / 8) * 8 * ncb;
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 2; i++)
    hipLaunchKernelGGL((wino43_mfma_kernel<0, BSRC, ABL, ODD>), dim3((unsigned)blocks), dim3(64 * WM_NW), 0, 0, v, ut, bias, y, (float*)nullptr, H, W, Cin, Cout, Ht, Wt, T, T, 1, (int)nbt, ncb, 1, 0, 0);
  hipEventRecord(e0, 0);
  for (int i = 0; i < iters; i++)
    hipLaunchKernelGGL((wino43_mfma_kernel<0, BSRC, ABL, ODD>), dim3((unsigned)blocks), dim3(64 * WM_NW), 0, 0, v, ut, bias, y, (float*)nullptr, H, W, Cin, Cout, Ht, Wt, T, T, 1, (int)nbt, ncb, 1, 0, 0);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  return ms / iters;
}

int main(int argc, char** argv)
{
  // image geometry: B images of H x W with T = B * (H/4) * (W/4) tiles
  const int B = argc > 1 ? atoi(argv[1]) : 32, H = argc > 2 ? atoi(argv[2]) : 60, W = argc > 3 ? atoi(argv[3]) : 80;
  const int Cin = argc > 4 ? atoi(argv[4]) : 512, Cout = argc > 5 ? atoi(argv[5]) : 512;
  const long long T = (long long)B * ((H + 3) / 4) * ((W + 3) / 4);
  float *v, *ut, *bias, *y;
  hipMalloc(&v, sizeof(float) * 36 * ((T + 63) / 64 * 64) * Cin);
  hipMalloc(&ut, sizeof(float) * 36 * (size_t)Cout * Cin);
  hipMalloc(&bias, sizeof(float) * Cout);
  hipMalloc(&y, sizeof(float) * (size_t)B * H * W * Cout);
  std::vector<float> h(1 << 20);
  for (auto& f : h) f = (float)rand() / RAND_MAX - 0.5f;
  for (size_t o = 0; o < 36ull * T * Cin; o += h.size()) hipMemcpy(v + o, h.data(), sizeof(float) * std::min<size_t>(h.size(), (size_t)(36ull * T * Cin - o)), hipMemcpyHostToDevice);
  for (size_t o = 0; o < 36ull * Cout * Cin; o += h.size()) hipMemcpy(ut + o, h.data(), sizeof(float) * std::min<size_t>(h.size(), (size_t)(36ull * Cout * Cin - o)), hipMemcpyHostToDevice);
  hipMemcpy(bias, h.data(), sizeof(float) * Cout, hipMemcpyHostToDevice);
  const double fl = 2.0 * 36 * T * Cin * Cout;
  const int it = 10;
#define R(ABL, WHAT) { float ms = run<ABL>(v, ut, bias, y, H, W, Cin, Cout, T, it); printf("%-44s %8.3f ms  %6.1f TFLOP/s-equivalent\n", WHAT, ms, fl / ms / 1e9); }
  printf("T=%lld Cin=%d Cout=%d\n", T, Cin, Cout);
  for (int w = 0; w < 250; w++) run<0>(v, ut, bias, y, H, W, Cin, Cout, T, 5);   // clocks up (they ramp for seconds)
  R(0, "full kernel");
  R(ABL_L2_OPERANDS, "full kernel, every operand L2-resident");
  R(0, "full kernel (again)");
  R(ABL_NO_EPILOGUE, "no epilogue");
  R(ABL_NO_EPILOGUE | ABL_NO_FOLD, "no epilogue, no column fold");
  R(ABL_NO_EPILOGUE | ABL_NO_BARRIER, "no epilogue, no barrier");
  R(ABL_NO_EPILOGUE | ABL_NO_DMA, "no epilogue, no DMA");
  R(ABL_NO_EPILOGUE | ABL_NO_LDS_READS, "no epilogue, no LDS reads");
  R(ABL_NO_EPILOGUE | ABL_NO_DMA | ABL_NO_LDS_READS, "no epilogue, no DMA, no LDS reads");
  R(ABL_NO_EPILOGUE | ABL_NO_BARRIER | ABL_NO_DMA | ABL_NO_LDS_READS | ABL_NO_FOLD, "MFMAs + loop control only");
  R(ABL_NO_EPILOGUE | ABL_NO_MFMA, "no epilogue, no MFMAs");
  R(ABL_NO_EPILOGUE | ABL_NO_MFMA | ABL_NO_LDS_READS, "no epilogue, no MFMAs, no LDS reads (DMA only)");
  R(ABL_NO_EPILOGUE | ABL_L2_OPERANDS, "no epilogue, every operand L2-resident");
  R(ABL_NT_STORES, "full kernel, non-temporal output stores");
  R(0, "full kernel (again 3)");
  R(ABL_NT_STORES, "full kernel, non-temporal output stores (again)");
  R(ABL_NO_STORES, "epilogue without its global stores");
  R(ABL_EPI_REGS_ONLY, "epilogue = bias + ReLU only (no staging, no stores)");
  R(0, "full kernel (again 2)");
  // the packed-filter route (B operand from global memory into registers); Cin / 64 even and odd take different instances
#define RB(ABL, WHAT) { float ms = (Cin / 64) & 1 ? run<ABL, 1, 1>(v, ut, bias, y, H, W, Cin, Cout, T, it) : run<ABL, 1, 0>(v, ut, bias, y, H, W, Cin, Cout, T, it); \
                        printf("%-44s %8.3f ms  %6.1f TFLOP/s-equivalent\n", WHAT, ms, fl / ms / 1e9); }
  RB(0, "packed: full kernel");
  RB(ABL_NO_EPILOGUE, "packed: no epilogue");
  RB(ABL_NO_EPILOGUE | ABL_NO_B_LOADS, "packed: no epilogue, no B loads");
  RB(ABL_NO_EPILOGUE | ABL_NO_DMA, "packed: no epilogue, no A DMA");
  RB(ABL_NO_EPILOGUE | ABL_NO_LDS_READS, "packed: no epilogue, no LDS reads");
  RB(ABL_NO_EPILOGUE | ABL_NO_BARRIER, "packed: no epilogue, no barrier");
  RB(0, "packed: full kernel (again)");
  R(0, "full kernel (last)");
  return 0;
}
