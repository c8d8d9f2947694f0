// What the per-head tile losses share (normal_geo.hip, photometric.hip, multiview.hip): a loss over pred [B, n <= 8, H, W] that is
// sum_h w_h (sum of terms_h / count_h).  One workgroup per 32 x 8 tile of one head of one sample leaves one row of NP (sum, count) pairs
// of fp64 in the workspace, part [n][B tiles][2 NP]; one workgroup folds the rows head by head (dpf_reduce.h) into the loss and the
// stats record the backward reads its counts from.  A new loss of this family writes its per-tile kernel and its parameter checks, and
// takes the head weights, the tile plan (limits, workspace size, grid, partial-row index) and the fold from here.
#pragma once
#include "dpf_common.h"
#include "dpf_reduce.h"

constexpr int kDpfMaxHeads = 8;
constexpr int kDpfTileW = 32, kDpfTileH = 8;   // output tile, one pixel per thread of a 256-thread block
constexpr int kDpfMaxGridZ = 65535;            // B n rides on gridDim.z
constexpr int kDpfMaxTileRows = 65535;         // the tile rows on gridDim.y

// one weight per head, by value into the kernels; 0 past the n heads in use
struct DpfHeadW { float w[kDpfMaxHeads]; };

inline void dpf_fill_head_weights(float (&w)[kDpfMaxHeads], const float* weights_host, int n) {
  for (int k = 0; k < kDpfMaxHeads; ++k) w[k] = k < n ? weights_host[k] : 0.f;
}

// the tile plan of a shape: -1 where it is refused, else the partial rows of all heads together (n B tiles)
inline long long dpf_tile_rows(int B, int n, int H, int W) {
  if (B <= 0 || n < 1 || n > kDpfMaxHeads || H <= 0 || W <= 0 || (long long)B * n > kDpfMaxGridZ ||
      dpf_div_up(H, kDpfTileH) > kDpfMaxTileRows || (long long)H * W > 0x7fffffffLL)
    return -1;
  return (long long)n * B * dpf_div_up(H, kDpfTileH) * dpf_div_up(W, kDpfTileW);
}

// grid (ceil(W / 32), ceil(H / 8), B n) of the per-tile kernels, forward and backward
inline dim3 dpf_tile_grid(int B, int n, int H, int W) { return dim3(dpf_div_up(W, kDpfTileW), dpf_div_up(H, kDpfTileH), B * n); }

namespace {      // (kernels have internal linkage in every file here; each file that includes this gets its own fold)

// the partial row of this block, sample s and head h of n, under dpf_tile_grid
__device__ __forceinline__ size_t dpf_tile_part_row(int s, int h, int n) {
  const size_t tiles = (size_t)gridDim.x * gridDim.y, rows = (size_t)(gridDim.z / n) * tiles;
  return (size_t)h * rows + (size_t)s * tiles + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
}

// one block: folds the rows (per head: B tiles) of every head in a fixed order, writes the stats record and the loss.  A row holds NP
// (sum, count) pairs; stats: for pair q the counts at [16 q, 16 q + 8) and the sums at [16 q + 8, 16 q + 16)
template <int NP>
__global__ __launch_bounds__(256) void dpf_head_fold_kernel(const double* __restrict__ part, long long rows, int n, DpfHeadW hw,
                                                            double* __restrict__ stats, float* __restrict__ out) {
  __shared__ double tot[2 * NP];
  double loss = 0.0;
  for (int k = 0; k < kDpfMaxHeads; ++k) {
    double sum[NP], cnt[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) sum[q] = 0.0, cnt[q] = 0.0;
    if (k < n) {
      dpf_fold_rows_d<2 * NP>(part + (size_t)k * (size_t)rows * 2 * NP, rows, 2 * NP, tot);
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        sum[q] = tot[2 * q], cnt[q] = tot[2 * q + 1];
        if (cnt[q] > 0.0) loss += (double)hw.w[k] * (sum[q] / cnt[q]);
      }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        stats[2 * kDpfMaxHeads * q + k] = cnt[q];
        stats[2 * kDpfMaxHeads * q + kDpfMaxHeads + k] = sum[q];
      }
    }
  }
  if (threadIdx.x == 0) out[0] = (float)loss;
}

}  // namespace

// the fold after a per-tile forward that ran under dpf_tile_grid(B, n, H, W)
template <int NP>
inline void dpf_launch_head_fold(const double* part, int B, int n, int H, int W, const DpfHeadW& hw, double* stats, float* out,
                                 hipStream_t st) {
  hipLaunchKernelGGL(dpf_head_fold_kernel<NP>, dim3(1), dim3(256), 0, st, part, dpf_tile_rows(B, n, H, W) / n, n, hw, stats, out);
}
