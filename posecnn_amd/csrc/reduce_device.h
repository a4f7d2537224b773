// reduce_device.h — the fixed-order reductions the loss and gradient kernels share: the halving tree in LDS and the kernel
// that folds per-workgroup partials into one value per channel. One definition, because the order IS the result: the CPU
// checkers (tests/label_loss_ref.py, tests/vertex_head_ref.py, tests/trunk_epilogue_ref.py, oracle) restate exactly it.
#pragma once

#include "pcnn_device.h"

namespace pcnn {

// s[0 .. N) -> s[0]: N/2, N/4, ... 1 threads add the upper half onto the lower, s[t] = s[t] + s[t + st]. Every thread of
// the workgroup calls it with its index t, after writing its leaves (the leading barrier is here); s[0] is valid for all
// threads on return.
template <int N, class T>
__device__ __forceinline__ void block_tree_sum(T* s, int t)
{
  __syncthreads();
  for (int st = N / 2; st >= 1; st >>= 1) {
    if (t < st) s[t] = s[t] + s[t + st];
    __syncthreads();
  }
}

// two arrays in step: the (sum, count) and (loss, weight) pairs
template <int N, class T, class U>
__device__ __forceinline__ void block_tree_sum(T* a, U* b, int t)
{
  __syncthreads();
  for (int st = N / 2; st >= 1; st >>= 1) {
    if (t < st) {
      a[t] = a[t] + a[t + st];
      b[t] = b[t] + b[t + st];
    }
    __syncthreads();
  }
}

// out[c] = (float) sum of part[c * nblk .. (c + 1) * nblk): one workgroup of NT threads per channel; thread t adds partials
// t, t + NT, ... ascending in f64, then the NT-leaf tree. The second stage of every dbias in the library, all of them at
// NT = CPF_THREADS: the order is part of the result. (A template, so that only the files that launch it carry a copy.)
constexpr int CPF_THREADS = 256;

template <int NT>
static __global__ __launch_bounds__(NT) void channel_partials_final_kernel(const double* __restrict__ part, int nblk,
                                                                           float* __restrict__ out)
{
  __shared__ double s_sum[NT];
  const int t = threadIdx.x;
  const double* p = part + (size_t)blockIdx.x * nblk;
  double a = 0.0;
  for (int i = t; i < nblk; i += NT) a = a + p[i];
  s_sum[t] = a;
  block_tree_sum<NT>(s_sum, t);
  if (t == 0) out[blockIdx.x] = (float)s_sum[0];
}

}  // namespace pcnn
