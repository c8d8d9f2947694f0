// Gradient accumulation and global-norm clipping over the flat arenas, the device side of the option keys
// accumulate_grad_batches, gradient_clip_val and track_grad_norm:
//
//   dpf_grad_fold     acc[i] = first ? g[i] : acc[i] + g[i] in fp32 (bitwise the left-to-right sum of a group's gradients) and, when the
//                     control record says that this micro-step ends the group, the per-workgroup sums of squares of the new acc[] in the
//                     same pass
//   dpf_grad_sumsq    the per-workgroup sums of squares of an arena on their own (no accumulation arena at N = 1; after the all-reduce
//                     between ranks)
//   dpf_grad_finish   one workgroup: total = gscale * sqrt(sum), coef = min(1, clip / (total + 1e-6)) (torch's clip_grad_norm_, norm type 2)
//                     -> ctl[GMUL] = float(gscale * coef), ctl[NORM] = float(total)
//
// Every element is squared and summed in fp64 (this file is built with -ffp-contract=off).  An arena is walked in quads of four
// consecutive elements, quad q by thread q mod (grid * 256) whatever the alignment: with all pointers 16-byte aligned a whole quad is one
// 16-byte access, otherwise four scalar ones, and the sums are formed in the same order, so both forms return the same bits.  Wave sums
// by __shfl_xor on doubles, wave results through LDS in a fixed order, one row per workgroup, rows added in a fixed stride order by the
// finish kernel; no floating-point atomics, nothing waits on the host, nothing allocates.
//
// The control record (DPF_GRAD_CTL_FLOATS floats of device memory) is what a captured train step reads instead of kernel arguments:
//   [0], [1]  the optimiser's per-step scalars (Adam: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t); SGD / RMSprop: lr, unused)   host
//   [2]       first: non-zero = this micro-step opens a group (the fold overwrites)                                            host
//   [3]       apply: non-zero = this micro-step ends a group (partials, finish and the optimiser run; otherwise they return)   host
//   [4]       gmul: what the optimiser multiplies every gradient element by                                                    finish
//   [5]       grad_norm: the global 2-norm of the scaled gradient before clipping                                              finish
#include "dpf_common.h"
#include "dpf_reduce.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;              // threads per block of every kernel here (4 waves)
constexpr int kItems = 4;                // quads per thread before the grid stops growing
constexpr int kMaxBlocks = 1024;         // = rows of partial sums
constexpr int kWsAlign = 8;              // the workspace holds doubles
enum { C_FIRST = 2, C_APPLY = 3, C_GMUL = 4, C_NORM = 5 };

__device__ __forceinline__ double square(float x) { return (double)x * (double)x; }

// FOLD: acc is updated from g as above; otherwise acc is only read.  PART: part[blockIdx.x] receives the block's sum of squares -- under
// FOLD only when ctl[C_APPLY] is set.  V == 4: acc and g are 16-byte aligned.
template <bool FOLD, bool PART, int V>
__global__ __launch_bounds__(256) void grad_pass_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n,
                                                        const float* __restrict__ ctl, double* __restrict__ part) {
  bool first = false, sums = PART;
  if (FOLD) {
    first = ctl[C_FIRST] != 0.f;
    sums = PART && ctl[C_APPLY] != 0.f;                  // (uniform over the grid)
  }
  const long long nquads = (n + 3) / 4;
  double s[1] = {0.0};
  for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < nquads; q += (long long)gridDim.x * kBlock) {
    const long long i = 4 * q;
    if (V == 4 && i + 4 <= n) {
      f32x4 a = *reinterpret_cast<const f32x4*>(acc + i);
      if (FOLD) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = first ? gv[k] : a[k] + gv[k];
        *reinterpret_cast<f32x4*>(acc + i) = a;
      }
      if (sums) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[0] += square(a[k]);
      }
    } else {
      const int m = n - i < 4 ? (int)(n - i) : 4;
      for (int k = 0; k < m; ++k) {
        float a = acc[i + k];
        if (FOLD) {
          a = first ? g[i + k] : a + g[i + k];
          acc[i + k] = a;
        }
        if (sums) s[0] += square(a);
      }
    }
  }
  if (PART) {
    if (!sums) return;
    dpf_block_reduce_d<1>(s, part + blockIdx.x);
  }
}

// one workgroup folds the rows (dpf_reduce.h)
__global__ __launch_bounds__(256) void grad_finish_kernel(const double* __restrict__ part, int rows, double gscale, double clip,
                                                          float* __restrict__ ctl) {
  if (ctl[C_APPLY] == 0.f) return;
  __shared__ double tot[1];
  dpf_fold_rows_d<1>(part, rows, 1, tot);
  if (threadIdx.x != 0) return;
  const double total = gscale * sqrt(tot[0]);
  double coef = 1.0;
  if (clip > 0.0) {
    const double r = clip / (total + 1e-6);
    coef = r < 1.0 || r != r ? r : 1.0;                  // clamp(max = 1), a NaN ratio stays NaN as in torch
  }
  ctl[C_GMUL] = (float)(gscale * coef);
  ctl[C_NORM] = (float)total;
}

int rows_of(long long n) { return dpf_red_rows(n, (long long)kBlock * 4 * kItems, kMaxBlocks); }

bool ws_ok(const void* ws, long long ws_bytes, long long n) {
  return dpf_ws_ok(ws, ws_bytes, (long long)rows_of(n) * (long long)sizeof(double), kWsAlign);
}

template <bool FOLD, bool PART>
void launch_pass(bool v4, float* acc, const float* g, long long n, const float* ctl, double* part, hipStream_t st) {
  const dim3 grid(rows_of(n)), block(kBlock);
  if (v4) hipLaunchKernelGGL((grad_pass_kernel<FOLD, PART, 4>), grid, block, 0, st, acc, g, n, ctl, part);
  else hipLaunchKernelGGL((grad_pass_kernel<FOLD, PART, 1>), grid, block, 0, st, acc, g, n, ctl, part);
}

}  // namespace

extern "C" {

long long dpf_grad_ctl_workspace_bytes(long long n) {
  if (n <= 0) return -1;
  return (long long)rows_of(n) * (long long)sizeof(double);
}

int dpf_grad_fold(float* acc, const float* grad, long long n, const float* ctl, void* ws, long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!acc || !grad || !ctl || n <= 0 || (ws && !ws_ok(ws, ws_bytes, n))) return DPF_ERR_INVALID_ARG;
  const bool v4 = dpf_aligned16(acc) && dpf_aligned16(grad);
  if (ws) launch_pass<true, true>(v4, acc, grad, n, ctl, (double*)ws, (hipStream_t)stream);
  else launch_pass<true, false>(v4, acc, grad, n, ctl, nullptr, (hipStream_t)stream);
  return dpf_check_launch();
}

int dpf_grad_sumsq(const float* grad, long long n, void* ws, long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!grad || n <= 0 || !ws_ok(ws, ws_bytes, n)) return DPF_ERR_INVALID_ARG;
  // (the arena is only read: the FOLD = false instantiation never stores through acc)
  launch_pass<false, true>(dpf_aligned16(grad), const_cast<float*>(grad), nullptr, n, nullptr, (double*)ws, (hipStream_t)stream);
  return dpf_check_launch();
}

int dpf_grad_finish(const void* ws, long long ws_bytes, long long n, double gscale, double clip, float* ctl, void* stream) {
  dpf_clear_error();
  if (!ctl || n <= 0 || !ws_ok(ws, ws_bytes, n) || !(clip >= 0.0)) return DPF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)ws, rows_of(n), gscale, clip, ctl);
  return dpf_check_launch();
}

}  // extern "C"
