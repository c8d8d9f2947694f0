// The robust affine fit of the 'least_square' disparity conversion (src/utils/geometry.py::regress_affine; dualpixelface_amd/losses.py):
// per sample, the line y = A x + B between x = idepth and y = the first prediction head that minimises scipy's soft_l1 cost
//   sum over the pixels with x > 0 of  f^2 * 2 (sqrt(1 + (r / f)^2) - 1),  r = A x + B - y,
// by iteratively reweighted least squares from the ordinary least-squares line.
//
//   dpf_affine_fit   (pass, fold) x (1 + max_iters), then one objective pass and the kernel that writes ab [B, 2] and info [B, 6]
//
// Per pixel, in fp64 and in this order (this file is built with -ffp-contract=off; x is about 1e-3 and A about -2.7e4):
//   r = (A * x + B) - y,  s = sqrt(1 + (r / f) * (r / f)),  w = 1 / s  (w = 1 in pass 0),  objective term 2 (s - 1)
//   sums of w, w x, w y, (w x) x, (w x) y, the term, and in pass 0 the valid count and max x
// A pass writes per-workgroup partials; the fold of one sample (one workgroup) adds them in a fixed order, solves the 2x2 normal equations
// (|det| < 1e-30: A = 0, B = sum w y / sum w, or 0 without a valid pixel -- metrics._weighted_affine_fit's rule) and marks the sample done
// once |dA| * max x + |dB| < tol; every later pass and fold of that sample returns at once.  Kernel boundaries are the only hand-off
// between workgroups, no floating-point atomics: the bits repeat run to run.  Nothing here waits on the host.
#include "dpf_common.h"
#include "dpf_reduce.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;              // threads per block of every kernel here (4 waves)
constexpr int kItems = 4;                // loads of 4 pixels per thread before the grid stops growing
constexpr int kMaxBlocks = 1024;         // blocks per sample
constexpr int kMaxB = 65535;             // samples ride on gridDim.y
constexpr int kSums = 7;                 // partial row: sum w, w x, w y, w x x, w x y, objective term, count; then max x
constexpr int kRow = 8;
constexpr int kWsAlign = 8;              // the workspace holds doubles
constexpr int kState = 8;                // per sample: A, B, done, iterations, count, max x, objective at the start (-1: not yet), spare
constexpr int kInfo = 6;                 // as include/dpf_hip.h
constexpr double kDetMin = 1e-30;

enum { S_A = 0, S_B, S_DONE, S_ITERS, S_COUNT, S_XMAX, S_OBJ0 };
enum { PASS_FIRST = 0, PASS_REWEIGHT = 1, PASS_OBJECTIVE = 2 };

template <int MODE>
__device__ __forceinline__ void pixel(float xf, float yf, double A, double B, double f, double (&acc)[kRow]) {
  if (!(xf > 0.f)) return;               // NaN is not valid; whatever y holds there stays out of the sums
  const double x = (double)xf, y = (double)yf;
  double w = 1.0;
  if (MODE != PASS_FIRST) {
    const double r = (A * x + B) - y, z = r / f;
    const double s = sqrt(1.0 + z * z);
    w = 1.0 / s;
    acc[5] += 2.0 * (s - 1.0);
    if (MODE == PASS_OBJECTIVE) return;
  }
  const double wx = w * x;
  acc[0] += w;
  acc[1] += wx;
  acc[2] += w * y;
  acc[3] += wx * x;
  acc[4] += wx * y;
  if (MODE == PASS_FIRST) {
    acc[6] += 1.0;
    acc[7] = fmax(acc[7], x);
  }
}

// grid (blocks per sample, B).  y: head 0 of pred, a contiguous plane of HW floats per sample, ystride floats apart; x: idepth [B][HW].
// V == 4: HW % 4 == 0, ystride % 4 == 0 and both bases 16-byte aligned, so a load never straddles a plane.  part: [B][gridDim.x][kRow].
template <int MODE, int V>
__global__ __launch_bounds__(256) void fit_pass_kernel(const float* __restrict__ y, long long ystride, const float* __restrict__ x, long long HW,
                                                       double f, const double* __restrict__ state, double* __restrict__ part) {
  const long long b = blockIdx.y;
  double A = 0.0, B = 0.0;
  if (MODE != PASS_FIRST) {              // (pass 0 reads no state: its fold is what initialises the record)
    const double* st = state + b * kState;
    if (MODE == PASS_REWEIGHT && st[S_DONE] != 0.0) return;
    A = st[S_A];
    B = st[S_B];
  }
  const float* __restrict__ yb = y + (size_t)b * (size_t)ystride;
  const float* __restrict__ xb = x + (size_t)b * (size_t)HW;
  double acc[kRow];
#pragma unroll
  for (int k = 0; k < kRow; ++k) acc[k] = 0.0;
  for (long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) * V; i < HW; i += (long long)gridDim.x * kBlock * V) {
    if constexpr (V == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + i);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(yb + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) pixel<MODE>(xv[j], yv[j], A, B, f, acc);
    } else {
      pixel<MODE>(xb[i], yb[i], A, B, f, acc);
    }
  }
  dpf_block_reduce_d<kSums, 1>(acc, part + ((size_t)b * gridDim.x + blockIdx.x) * kRow);
}

// grid (B).  first: the fold of pass 0 (writes the whole state record); it: the number of this reweighted solve otherwise
__global__ __launch_bounds__(256) void fit_fold_kernel(const double* __restrict__ part, int rows, int first, int it, double f, double tol,
                                                       double* __restrict__ state) {
  double* st = state + (size_t)blockIdx.x * kState;
  if (!first && st[S_DONE] != 0.0) return;
  __shared__ double tot[kRow];
  dpf_fold_rows_d<kSums, 1>(part + (size_t)blockIdx.x * rows * kRow, rows, kRow, tot);
  if (threadIdx.x != 0) return;
  const double sw = tot[0], sx = tot[1], sy = tot[2], sxx = tot[3], sxy = tot[4];
  const double det = sw * sxx - sx * sx;
  double A = 0.0, B = 0.0;
  if (fabs(det) >= kDetMin) {            // (false for a NaN determinant, like the rule's other side)
    A = (sw * sxy - sx * sy) / det;
    B = (sxx * sy - sx * sxy) / det;
  } else if (sw > 0.0) {
    B = sy / sw;
  }
  if (first) {
    st[S_DONE] = tot[6] > 0.0 ? 0.0 : 1.0;             // nothing valid: (0, 0), and nothing to iterate on
    st[S_ITERS] = 0.0;
    st[S_COUNT] = tot[6];
    st[S_XMAX] = tot[7];
    st[S_OBJ0] = -1.0;
    st[7] = 0.0;
  } else {
    if (it == 1) st[S_OBJ0] = (f * f) * tot[5];         // the objective at the least-squares start
    const double step = fabs(A - st[S_A]) * st[S_XMAX] + fabs(B - st[S_B]);
    st[S_ITERS] = (double)it;
    if (step < tol) st[S_DONE] = 1.0;
  }
  st[S_A] = A;
  st[S_B] = B;
}

// grid (B): folds the objective pass and writes ab = [b, a] as float32 and the info record
__global__ __launch_bounds__(256) void fit_finish_kernel(const double* __restrict__ part, int rows, double f, const double* __restrict__ state,
                                                         float* __restrict__ ab, double* __restrict__ info) {
  const double* st = state + (size_t)blockIdx.x * kState;
  __shared__ double tot[kRow];
  dpf_fold_rows_d<kSums, 1>(part + (size_t)blockIdx.x * rows * kRow, rows, kRow, tot);
  if (threadIdx.x != 0) return;
  const double obj = (f * f) * tot[5];
  ab[2 * blockIdx.x] = (float)st[S_B];
  ab[2 * blockIdx.x + 1] = (float)st[S_A];
  double* o = info + (size_t)blockIdx.x * kInfo;
  o[0] = st[S_A];
  o[1] = st[S_B];
  o[2] = st[S_ITERS];
  o[3] = st[S_COUNT];
  o[4] = obj;
  o[5] = st[S_OBJ0] < 0.0 ? obj : st[S_OBJ0];          // no reweighted solve ran: the result is the start
}

int blocks_per_sample(long long HW) { return dpf_red_rows(HW, (long long)kBlock * 4 * kItems, kMaxBlocks); }

template <int MODE>
void launch_pass(bool v4, dim3 grid, hipStream_t st, const float* y, long long ystride, const float* x, long long HW, double f,
                 const double* state, double* part) {
  if (v4) hipLaunchKernelGGL((fit_pass_kernel<MODE, 4>), grid, dim3(kBlock), 0, st, y, ystride, x, HW, f, state, part);
  else hipLaunchKernelGGL((fit_pass_kernel<MODE, 1>), grid, dim3(kBlock), 0, st, y, ystride, x, HW, f, state, part);
}

}  // namespace

extern "C" {

long long dpf_affine_fit_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || B > kMaxB || H <= 0 || W <= 0) return -1;
  return (long long)B * (kState + (long long)blocks_per_sample((long long)H * W) * kRow) * (long long)sizeof(double);
}

int dpf_affine_fit(const float* pred, long long pred_batch_stride, const float* idepth, int B, int H, int W, double f_scale, int max_iters,
                   double tol, void* ws, long long ws_bytes, float* ab, double* info, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!pred || !idepth || !ws || !ab || !info || B <= 0 || H <= 0 || W <= 0 || max_iters < 0 || !(f_scale > 0.0) || !(tol >= 0.0))
    return DPF_ERR_INVALID_ARG;
  const long long HW = (long long)H * W;
  if (pred_batch_stride < HW) return DPF_ERR_INVALID_ARG;
  if (B > kMaxB) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, dpf_affine_fit_workspace_bytes(B, H, W), kWsAlign)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int gx = blocks_per_sample(HW);
  const dim3 grid(gx, B);
  double* state = (double*)ws;
  double* part = state + (size_t)B * kState;
  const bool v4 = HW % 4 == 0 && pred_batch_stride % 4 == 0 && dpf_aligned16(pred) && dpf_aligned16(idepth);
  launch_pass<PASS_FIRST>(v4, grid, st, pred, pred_batch_stride, idepth, HW, f_scale, state, part);
  hipLaunchKernelGGL(fit_fold_kernel, dim3(B), dim3(kBlock), 0, st, part, gx, 1, 0, f_scale, tol, state);
  for (int it = 1; it <= max_iters; ++it) {
    launch_pass<PASS_REWEIGHT>(v4, grid, st, pred, pred_batch_stride, idepth, HW, f_scale, state, part);
    hipLaunchKernelGGL(fit_fold_kernel, dim3(B), dim3(kBlock), 0, st, part, gx, 0, it, f_scale, tol, state);
  }
  launch_pass<PASS_OBJECTIVE>(v4, grid, st, pred, pred_batch_stride, idepth, HW, f_scale, state, part);
  hipLaunchKernelGGL(fit_finish_kernel, dim3(B), dim3(kBlock), 0, st, part, gx, f_scale, state, ab, info);
  return dpf_check_launch();
}

}  // extern "C"
