// Validation metrics on the device (dualpixelface_amd/metrics.py is the definition and the yardstick):
//
//   dpf_metric_absolute_dp   disp2depth + the eight expressions of depth_errors, one pass over the batch
//   dpf_metric_normal_dp     F.normalize of both maps, clamped dot, acos, the sums behind normal_error_mean / normal_error_rmse
//   dpf_metric_ranks         stable ascending ranks per sample (LSD radix sort of (key, index), 8-bit digits, four passes)
//   dpf_metric_affine_dp     weighted affine fit by IRLS, weighted RMSE and the weighted Spearman correlation of the ranks
//
// Element-wise arithmetic is fp32 in the order metrics.py writes it (this file is built with -ffp-contract=off; log and acos are the
// correctly rounded fp32 values); every sum is fp64.  Reductions are two-phase: each block leaves its partial sums in the workspace, one block
// per result folds them in a fixed order -- no floating-point atomics, so the bits repeat run to run.  Nothing here waits on the host.
#include "dpf_common.h"
#include "dpf_reduce.h"
#include "metrics_plan.h"
#include <float.h>
#include <math.h>

namespace {

using namespace dpf_metrics;

enum { DPF_METRIC_DISP = 0, DPF_METRIC_IDEPTH = 1, DPF_METRIC_DEPTH = 2 };      // target_type, as include/dpf_hip.h

// torch.maximum / torch.clamp propagate NaN
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
__device__ __forceinline__ double max_nan_d(double a, double b) { return (a != a || b != b) ? (double)NAN : (a > b ? a : b); }

// ------------------------------------------------------------------------------------------------------------- absolute_dp
__global__ __launch_bounds__(256) void abs_partial_kernel(const float* __restrict__ pred, const float* __restrict__ ab,
                                                          const float* __restrict__ gt, const float* __restrict__ mask, long long n,
                                                          int convert, float t1, float t2, float t3, double* __restrict__ part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * (size_t)n;
  const float fb = convert ? ab[2 * b] : 0.f, fa = convert ? ab[2 * b + 1] : 0.f;       // abvalue = [b, a]
  double acc[kAbsValues];
#pragma unroll
  for (int k = 0; k < kAbsValues; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const float m = mask ? mask[base + i] : 1.f;
    if (!(m > 0.f)) continue;
    const float g = gt[base + i];
    float p = pred[base + i];
    if (convert) {
      const float depth = fa / (p - fb);
      p = dpf_finite_f(depth) ? depth : 0.f;
    }
    const float thresh = max_nan(g / p, p / g);
    const float d = g - p;
    const float lg = (float)log((double)g) - (float)log((double)p);
    acc[0] += (double)(fabsf(d) / g);
    acc[1] += (double)fabsf(d);
    acc[2] += (double)((d * d) / g);
    acc[3] += (double)(d * d);
    acc[4] += (double)(lg * lg);
    acc[5] += thresh < t1 ? 1.0 : 0.0;
    acc[6] += thresh < t2 ? 1.0 : 0.0;
    acc[7] += thresh < t3 ? 1.0 : 0.0;
    acc[8] += 1.0;
  }
  dpf_block_reduce_d<kAbsValues>(acc, part + ((size_t)b * gridDim.x + blockIdx.x) * kAbsValues);
}

__global__ __launch_bounds__(256) void abs_fold_kernel(const double* __restrict__ part, long long rows, float* __restrict__ out) {
  __shared__ double tot[kAbsValues];
  dpf_fold_rows_d<kAbsValues>(part, rows, kAbsValues, tot);
  if (threadIdx.x == 0) {
    const double c = tot[8];                            // 0 selected pixels: 0 / 0 = NaN in every field, like the empty mean()
    out[0] = (float)(tot[0] / c);
    out[1] = (float)(tot[1] / c);
    out[2] = (float)(tot[2] / c);
    out[3] = (float)sqrt(tot[3] / c);
    out[4] = (float)sqrt(tot[4] / c);
    out[5] = (float)tot[5] / (float)c;                  // counts are exact, the fraction is the fp32 quotient torch's mean() takes
    out[6] = (float)tot[6] / (float)c;
    out[7] = (float)tot[7] / (float)c;
  }
}

// --------------------------------------------------------------------------------------------------------------- normal_dp
__global__ __launch_bounds__(256) void normal_partial_kernel(const float* __restrict__ a, const float* __restrict__ bmap,
                                                             const float* __restrict__ mask, long long n, double* __restrict__ part) {
  const int b = blockIdx.y;
  const size_t base3 = (size_t)b * 3 * (size_t)n, base = (size_t)b * (size_t)n;
  double acc[kNormalValues] = {0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const float m = mask ? mask[base + i] : 1.f;
    acc[2] += (double)m;                                // m.sum() runs over every pixel
    if (!(m > 0.f)) continue;
    const float a0 = a[base3 + i], a1 = a[base3 + n + i], a2 = a[base3 + 2 * n + i];
    const float b0 = bmap[base3 + i], b1 = bmap[base3 + n + i], b2 = bmap[base3 + 2 * n + i];
    float na = sqrtf((a0 * a0 + a1 * a1) + a2 * a2), nb = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
    na = na < 1e-12f ? 1e-12f : na;                     // F.normalize: x / max(||x||, eps)
    nb = nb < 1e-12f ? 1e-12f : nb;
    float dot = ((a0 / na) * (b0 / nb) + (a1 / na) * (b1 / nb)) + (a2 / na) * (b2 / nb);
    dot = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);  // NaN stays NaN, like torch.clamp
    const float ang = (float)acos((double)dot);
    const float am = ang * m;
    acc[0] += (double)(((ang * 180.0f) / 3.14159265358979323846f) * m);
    acc[1] += (double)(am * am);
  }
  dpf_block_reduce_d<kNormalValues>(acc, part + ((size_t)b * gridDim.x + blockIdx.x) * kNormalValues);
}

__global__ __launch_bounds__(256) void normal_fold_kernel(const double* __restrict__ part, long long rows, float* __restrict__ out) {
  __shared__ double tot[kNormalValues];
  dpf_fold_rows_d<kNormalValues>(part, rows, kNormalValues, tot);
  if (threadIdx.x == 0) {
    out[0] = (float)(tot[0] / tot[2]);
    out[1] = (float)(sqrt(tot[1] / tot[2]) * 180.0 / 3.14159265358979323846);
  }
}

// ------------------------------------------------------------------------------------------------------------------- ranks
// One wave owns kSortChunk consecutive elements and walks them 64 at a time in input order, so "position inside a digit" is
// (elements of earlier chunks) + (earlier rounds of this chunk) + (lower lanes of this round): the scatter is stable by construction.
template <bool FIRST>
__global__ __launch_bounds__(256) void sort_hist_kernel(const float* __restrict__ vals, const unsigned* __restrict__ keys_in, long long n,
                                                        long long chunks, int shift, int negate, unsigned* __restrict__ hist) {
  __shared__ unsigned h[kWaves][kRadix];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b = blockIdx.y, chunk = (long long)blockIdx.x * kWaves + w;
  const size_t base = (size_t)b * (size_t)n;
  for (int d = lane; d < kRadix; d += 64) h[w][d] = 0u;
  __syncthreads();
  if (chunk < chunks) {
    for (int r = 0; r < kSortRounds; ++r) {
      const long long i = sort_elem(chunk, r, lane);
      if (i < n) {
        const unsigned key = FIRST ? sort_key_bits(__float_as_uint(vals[base + i]), negate) : keys_in[base + i];
        atomicAdd(&h[w][(key >> shift) & 255u], 1u);    // integer: order-independent
      }
    }
  }
  __syncthreads();
  if (chunk < chunks)
    for (int d = lane; d < kRadix; d += 64) hist[hist_slot(b, chunks, chunk, d)] = h[w][d];
}

// per sample: counts[chunk][digit] -> exclusive offsets inside the digit (in place), base[digit] = first position of the digit
__global__ __launch_bounds__(256) void sort_scan_kernel(unsigned* __restrict__ hist, unsigned* __restrict__ basep, long long chunks) {
  __shared__ unsigned s[kRadix];
  const int d = threadIdx.x;
  const long long b = blockIdx.x;
  unsigned run = 0u;
  for (long long c = 0; c < chunks; ++c) {
    const long long slot = hist_slot(b, chunks, c, d);
    const unsigned v = hist[slot];
    hist[slot] = run;
    run += v;
  }
  s[d] = run;
  __syncthreads();
  for (int o = 1; o < kRadix; o <<= 1) {
    const unsigned t = d >= o ? s[d - o] : 0u;
    __syncthreads();
    s[d] += t;
    __syncthreads();
  }
  basep[b * kRadix + d] = s[d] - run;
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void sort_scatter_kernel(const float* __restrict__ vals, const unsigned* __restrict__ keys_in,
                                                           const unsigned* __restrict__ idx_in, unsigned* __restrict__ keys_out,
                                                           unsigned* __restrict__ idx_out, int* __restrict__ ranks, long long n,
                                                           long long chunks, int shift, int negate, const unsigned* __restrict__ hist,
                                                           const unsigned* __restrict__ basep) {
  __shared__ unsigned off[kWaves][kRadix];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b = blockIdx.y, chunk = (long long)blockIdx.x * kWaves + w;
  const bool live = chunk < chunks;
  const size_t base = (size_t)b * (size_t)n;
  for (int d = lane; d < kRadix; d += 64) off[w][d] = live ? basep[b * kRadix + d] + hist[hist_slot(b, chunks, chunk, d)] : 0u;
  __syncthreads();
  for (int r = 0; r < kSortRounds; ++r) {               // the same trip count in every wave: the barriers below are uniform
    const long long i = sort_elem(live ? chunk : 0, r, lane);
    const bool valid = live && i < n;
    unsigned key = 0u, id = 0u;
    if (valid) {
      key = FIRST ? sort_key_bits(__float_as_uint(vals[base + i]), negate) : keys_in[base + i];
      id = FIRST ? (unsigned)i : idx_in[base + i];
    }
    const unsigned digit = (key >> shift) & 255u;
    unsigned long long same = __ballot(valid);          // lanes of this round that hold my digit
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool bit = (digit >> k) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    const unsigned pos = valid ? off[w][digit] + below : 0u;
    __syncthreads();
    if (valid && below == 0u) off[w][digit] += (unsigned)__popcll(same);      // one lane per digit present in the round
    __syncthreads();
    if (valid && (long long)pos < n) {
      if (LAST) {
        if ((long long)id < n) ranks[base + id] = (int)pos;                   // the inverse permutation: rank of the element
      } else {
        keys_out[base + pos] = key;
        idx_out[base + pos] = id;
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------------- affine_dp
// One pass of the IRLS chain over sample blockIdx.y.  With the fit (s, t) of the previous pass it takes the residual r = |s p + t - d|,
// the next fit's moments with weight c / max(eps, r), and the two error sums of this fit: sum c r and sum c min(r^2, FLT_MAX).
// first: no fit yet, weight c.
__global__ __launch_bounds__(256) void affine_pass_kernel(const float* __restrict__ p, const float* __restrict__ d,
                                                          const float* __restrict__ c, long long n, const double* __restrict__ st,
                                                          int first, float eps, double* __restrict__ part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * (size_t)n;
  const float s = first ? 0.f : (float)st[2 * b], t = first ? 0.f : (float)st[2 * b + 1];
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const float x = p[base + i], y = d[base + i], cc = c[base + i];
    float w = cc, r = 0.f, q = 0.f;
    if (!first) {
      const float e = (x * s + t) - y;
      r = fabsf(e);
      q = e * e;
      q = q > FLT_MAX ? FLT_MAX : q;
      w = cc * (1.0f / (r < eps ? eps : r));
    }
    const double wd = (double)w, wx = wd * (double)x;
    acc[0] += wd;
    acc[1] += wx;
    acc[2] += wd * (double)y;
    acc[3] += wx * (double)x;
    acc[4] += wx * (double)y;
    acc[5] += (double)cc;
    acc[6] += (double)(cc * r);
    acc[7] += (double)(cc * q);
  }
  dpf_block_reduce_d<8>(acc, part + ((size_t)b * gridDim.x + blockIdx.x) * kAffineValues);
}

// sample blockIdx.x: fold the pass, solve the 2x2 normal equations (the determinant rule of _weighted_affine_fit), leave (s, t) for the
// next pass.  take_rmse: this pass ran with the first fit (weights c) -> wrmse; take_mae: it ran with the last fit -> wmae.
__global__ __launch_bounds__(256) void affine_fold_kernel(const double* __restrict__ part, int rows, double* __restrict__ st,
                                                          double* __restrict__ res, int take_rmse, int take_mae) {
  __shared__ double tot[8];
  const int b = blockIdx.x;
  dpf_fold_rows_d<8>(part + (size_t)b * rows * kAffineValues, rows, kAffineValues, tot);      // 8 of the 9-wide row
  if (threadIdx.x == 0) {
    const double sw = tot[0], sx = tot[1], sy = tot[2], sxx = tot[3], sxy = tot[4];
    const double det = sw * sxx - sx * sx;
    double s, t;
    if (fabs(det) < 1e-30) {
      s = 0.0;
      t = sw > 0.0 ? sy / sw : 0.0;
    } else {
      s = (sw * sxy - sx * sy) / det;
      t = (sxx * sy - sx * sxy) / det;
    }
    st[2 * b] = s;
    st[2 * b + 1] = t;
    if (take_mae) res[3 * b] = tot[6] / tot[5];
    if (take_rmse) res[3 * b + 1] = sqrt(tot[7] / tot[5]);
  }
}

// weighted moments of the rescaled ranks (r - n/2) / (n/2): y with x ascending and with x negated
__global__ __launch_bounds__(256) void rank_moment_kernel(const float* __restrict__ c, const int* __restrict__ rx,
                                                          const int* __restrict__ rxn, const int* __restrict__ ry, long long n,
                                                          double* __restrict__ part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * (size_t)n;
  const long long half = n / 2;
  const double h = (double)half;
  double acc[kAffineValues];
#pragma unroll
  for (int k = 0; k < kAffineValues; ++k) acc[k] = 0.0;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const double w = (double)c[base + i];
    const double x = (double)((long long)rx[base + i] - half) / h, xn = (double)((long long)rxn[base + i] - half) / h;
    const double y = (double)((long long)ry[base + i] - half) / h;
    acc[0] += w;
    acc[1] += w * x;
    acc[2] += w * xn;
    acc[3] += w * y;
    acc[4] += w * (x * x);
    acc[5] += w * (xn * xn);
    acc[6] += w * (y * y);
    acc[7] += w * (x * y);
    acc[8] += w * (xn * y);
  }
  dpf_block_reduce_d<kAffineValues>(acc, part + ((size_t)b * gridDim.x + blockIdx.x) * kAffineValues);
}

__device__ __forceinline__ double pearson(double ws, double sx, double sy, double sxx, double syy, double sxy) {
  const double mx = sx / ws, my = sy / ws;
  return (sxy / ws - mx * my) / sqrt((sxx / ws - mx * mx) * (syy / ws - my * my));
}

__global__ __launch_bounds__(256) void rank_fold_kernel(const double* __restrict__ part, int rows, double* __restrict__ res) {
  __shared__ double tot[kAffineValues];
  const int b = blockIdx.x;
  dpf_fold_rows_d<kAffineValues>(part + (size_t)b * rows * kAffineValues, rows, kAffineValues, tot);
  if (threadIdx.x == 0)
    res[3 * b + 2] = 1.0 - max_nan_d(pearson(tot[0], tot[1], tot[3], tot[4], tot[6], tot[7]),
                                     pearson(tot[0], tot[2], tot[3], tot[5], tot[6], tot[8]));
}

// batch means in sample order, as affine_metrics adds them
__global__ void affine_mean_kernel(const double* __restrict__ res, int B, float* __restrict__ out) {
  if (threadIdx.x < 3) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += res[3 * b + threadIdx.x] / (double)B;
    out[threadIdx.x] = (float)acc;
  }
}

constexpr int kWsAlign = 16;             // workspace alignment: the plans hand out 16-byte aligned sections

}  // namespace

extern "C" {

long long dpf_metric_absolute_dp_workspace_bytes(int B, long long n) { return reduce_bytes(B, n, kAbsValues); }
long long dpf_metric_normal_dp_workspace_bytes(int B, long long n) { return reduce_bytes(B, n, kNormalValues); }
long long dpf_metric_ranks_workspace_bytes(int B, long long n) { return ranks_plan(B, n).bytes; }
long long dpf_metric_affine_dp_workspace_bytes(int B, long long n) { return affine_plan(B, n).bytes; }

int dpf_metric_absolute_dp(const float* pred, const float* abvalue, const float* target, const float* mask, int B, long long n,
                           int target_type, double threshold, float* out8, void* ws, long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!pred || !target || !out8 || B <= 0 || n <= 0 || target_type < 0 || target_type > 2) return DPF_ERR_INVALID_ARG;
  const int convert = target_type != DPF_METRIC_DEPTH;
  if (convert && !abvalue) return DPF_ERR_INVALID_ARG;
  if (!shape_ok(B, n)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, reduce_bytes(B, n, kAbsValues), kWsAlign)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int gx = red_blocks(n);
  double* part = (double*)ws;
  // the constants torch compares with: the python doubles threshold ** k as fp32 scalars
  const float t1 = (float)threshold, t2 = (float)pow(threshold, 2.0), t3 = (float)pow(threshold, 3.0);
  hipLaunchKernelGGL(abs_partial_kernel, dim3(gx, B), dim3(kBlock), 0, st, pred, abvalue, target, mask, n, convert, t1, t2, t3, part);
  hipLaunchKernelGGL(abs_fold_kernel, dim3(1), dim3(kBlock), 0, st, part, (long long)B * gx, out8);
  return dpf_check_launch();
}

int dpf_metric_normal_dp(const float* pred, const float* target, const float* mask, int B, long long n, float* out2, void* ws,
                         long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!pred || !target || !out2 || B <= 0 || n <= 0) return DPF_ERR_INVALID_ARG;
  if (!shape_ok(B, n)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, reduce_bytes(B, n, kNormalValues), kWsAlign)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int gx = red_blocks(n);
  double* part = (double*)ws;
  hipLaunchKernelGGL(normal_partial_kernel, dim3(gx, B), dim3(kBlock), 0, st, pred, target, mask, n, part);
  hipLaunchKernelGGL(normal_fold_kernel, dim3(1), dim3(kBlock), 0, st, part, (long long)B * gx, out2);
  return dpf_check_launch();
}

int dpf_metric_ranks(const float* values, int* ranks, int B, long long n, int negate, void* ws, long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!values || !ranks || B <= 0 || n <= 0) return DPF_ERR_INVALID_ARG;
  if (!shape_ok(B, n)) return DPF_ERR_UNSUPPORTED;
  const RanksPlan pl = ranks_plan(B, n);
  if (!dpf_ws_ok(ws, ws_bytes, pl.bytes, kWsAlign)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  unsigned* keys[2] = {(unsigned*)(w + pl.keys[0]), (unsigned*)(w + pl.keys[1])};
  unsigned* idx[2] = {(unsigned*)(w + pl.idx[0]), (unsigned*)(w + pl.idx[1])};
  unsigned* hist = (unsigned*)(w + pl.hist);
  unsigned* basep = (unsigned*)(w + pl.base);
  const dim3 grid((unsigned)sort_blocks(n), B), blk(kBlock);
  negate = negate ? 1 : 0;
  // pass 0 reads the values, passes 1 and 2 ping-pong (key, index), pass 3 writes the ranks
  hipLaunchKernelGGL(sort_hist_kernel<true>, grid, blk, 0, st, values, (const unsigned*)nullptr, n, pl.chunks, 0, negate, hist);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(B), blk, 0, st, hist, basep, pl.chunks);
  hipLaunchKernelGGL((sort_scatter_kernel<true, false>), grid, blk, 0, st, values, (const unsigned*)nullptr, (const unsigned*)nullptr, keys[0],
                     idx[0], (int*)nullptr, n, pl.chunks, 0, negate, hist, basep);
  for (int pass = 1; pass < 4; ++pass) {
    const int src = (pass - 1) & 1, dst = pass & 1, shift = 8 * pass;
    hipLaunchKernelGGL(sort_hist_kernel<false>, grid, blk, 0, st, (const float*)nullptr, keys[src], n, pl.chunks, shift, 0, hist);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(B), blk, 0, st, hist, basep, pl.chunks);
    if (pass < 3)
      hipLaunchKernelGGL((sort_scatter_kernel<false, false>), grid, blk, 0, st, (const float*)nullptr, keys[src], idx[src], keys[dst], idx[dst],
                         (int*)nullptr, n, pl.chunks, shift, 0, hist, basep);
    else
      hipLaunchKernelGGL((sort_scatter_kernel<false, true>), grid, blk, 0, st, (const float*)nullptr, keys[src], idx[src], (unsigned*)nullptr,
                         (unsigned*)nullptr, ranks, n, pl.chunks, shift, 0, hist, basep);
  }
  return dpf_check_launch();
}

int dpf_metric_affine_dp(const float* pred, const float* target, const float* weight, const int* rank_pred, const int* rank_negpred,
                         const int* rank_target, int B, long long n, int irls_iters, float epsilon, float* out3, void* ws,
                         long long ws_bytes, void* stream) {
  dpf_clear_error();
  if (!pred || !target || !weight || !rank_pred || !rank_negpred || !rank_target || !out3 || B <= 0 || n <= 0 || irls_iters < 1)
    return DPF_ERR_INVALID_ARG;
  if (!shape_ok(B, n)) return DPF_ERR_UNSUPPORTED;
  const AffinePlan pl = affine_plan(B, n);
  if (!dpf_ws_ok(ws, ws_bytes, pl.bytes, kWsAlign)) return DPF_ERR_INVALID_ARG;
  hipStream_t stm = (hipStream_t)stream;
  char* w = (char*)ws;
  double* part = (double*)(w + pl.part);
  double* st = (double*)(w + pl.st);
  double* res = (double*)(w + pl.res);
  const int gx = red_blocks(n);
  const dim3 grid(gx, B), blk(kBlock);
  // Fused chain: pass k runs with fit k (pass 0: none) and gathers the moments of fit k + 1; fit 1 has weights c, so pass 1 also holds the
  // RMSE; the last pass holds the L1 error of the last fit.  irls_iters fits -> irls_iters + 1 passes.
  for (int k = 0; k <= irls_iters; ++k) {
    hipLaunchKernelGGL(affine_pass_kernel, grid, blk, 0, stm, pred, target, weight, n, st, k == 0 ? 1 : 0, epsilon, part);
    hipLaunchKernelGGL(affine_fold_kernel, dim3(B), blk, 0, stm, part, gx, st, res, k == 1 ? 1 : 0, k == irls_iters ? 1 : 0);
  }
  hipLaunchKernelGGL(rank_moment_kernel, grid, blk, 0, stm, weight, rank_pred, rank_negpred, rank_target, n, part);
  hipLaunchKernelGGL(rank_fold_kernel, dim3(B), blk, 0, stm, part, gx, res);
  hipLaunchKernelGGL(affine_mean_kernel, dim3(1), dim3(64), 0, stm, res, B, out3);
  return dpf_check_launch();
}

}  // extern "C"
