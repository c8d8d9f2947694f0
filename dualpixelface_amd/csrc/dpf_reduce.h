// The two-phase fp64 reduction of the loss, fit, metric and norm kernels (metrics.hip, loss_bank.hip, affine_fit.hip, grad_ctl.hip):
// every block of a pass leaves one row of partial results in the workspace, one block per result then folds the rows.  No floating-point
// atomics and every association order fixed, so the bits repeat run to run.  How many rows a pass writes and how many elements a block
// walks decide which element lands in which partial: they are part of a kernel's numerical identity and stay with the kernel.
//
// The host part is plain C++ (metrics_plan.h includes it and is built without HIP); the device part needs __HIPCC__.
#pragma once
#include <stdint.h>

// rows (= blocks) of a pass over n elements at elems_per_block each, clamped to [1, max_rows]
inline int dpf_red_rows(long long n, long long elems_per_block, int max_rows) {
  long long g = (n + elems_per_block - 1) / elems_per_block;
  if (g > max_rows) g = max_rows;
  if (g < 1) g = 1;
  return (int)g;
}

// a workspace of `have` bytes serves a request of `need` (negative: the shape was refused); align: a power of two
inline bool dpf_ws_ok(const void* ws, long long have, long long need, int align) {
  return ws && need > 0 && have >= need && ((uintptr_t)ws & (uintptr_t)(align - 1)) == 0;
}

#ifdef __HIPCC__

constexpr int kDpfRedBlock = 256;        // threads per block of every kernel that calls into here (4 waves)
constexpr int kDpfRedWaves = 4;

__device__ __forceinline__ double dpf_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double dpf_wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ bool dpf_finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Block-wide sums of acc[0 .. NSUM) and maxima of acc[NSUM .. NSUM + NMAX) (blockDim.x == 256): thread k < NSUM + NMAX writes value k to
// out[k], the four wave results joined as ((s0 + s1) + s2) + s3 and fmax(fmax(s0, s1), fmax(s2, s3)).  The leading barrier lets a kernel
// call this twice: the second call may not overwrite sm under a reader of the first.
template <int NSUM, int NMAX = 0>
__device__ __forceinline__ void dpf_block_reduce_d(const double (&acc)[NSUM + NMAX], double* __restrict__ out) {
  constexpr int NV = NSUM + NMAX;
  __shared__ double sm[NV][kDpfRedWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double v = k < NSUM ? dpf_wave_sum_d(acc[k]) : dpf_wave_max_d(acc[k]);
    if (lane == 0) sm[k][w] = v;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < NSUM) out[k] = ((sm[k][0] + sm[k][1]) + sm[k][2]) + sm[k][3];
  else if (k < NV) out[k] = fmax(fmax(sm[k][0], sm[k][1]), fmax(sm[k][2], sm[k][3]));
}

// One block folds `rows` partial rows, row_stride doubles apart, of which the first NSUM + NMAX are taken: thread t joins the rows
// t, t + 256, ... in that order, then the block reduce.  tot_shared (NSUM + NMAX doubles of LDS) is valid in every thread afterwards.
// A maximum starts from 0: the kernels here take maxima of positive values only, and "nothing seen" reads 0.
template <int NSUM, int NMAX = 0>
__device__ __forceinline__ void dpf_fold_rows_d(const double* __restrict__ part, long long rows, int row_stride, double* tot_shared) {
  constexpr int NV = NSUM + NMAX;
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  for (long long r = threadIdx.x; r < rows; r += kDpfRedBlock) {
    const double* __restrict__ row = part + r * row_stride;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] += row[k];
#pragma unroll
    for (int k = NSUM; k < NV; ++k) acc[k] = fmax(acc[k], row[k]);
  }
  dpf_block_reduce_d<NSUM, NMAX>(acc, tot_shared);
  __syncthreads();
}

#endif  // __HIPCC__
