// Depthwise convolution (groups = channels), forward / data-gradient / weight-gradient: the 3x3 pad-1 kernels and a general window.
// Replaces nn.Conv2d(nin, nin, 3, padding=1, groups=nin) of depthwise_separable_conv
// (reference: src/module/asm/basics.py:39-58; used by DPBlock.conv5, src/model/stereodpnet/modules.py:31).
// 18 FLOP per output element against 8 bytes of compulsory traffic => HBM-bound; one thread per output
// element, lanes along W, the 3x3 taps come from L1/L2.
#include "dpf_common.h"

namespace {

// y[n,c,y,x] = sum_t w[c][t] * x[n,c,y+ty-1,x+tx-1]  (flip = 1: taps mirrored -> data gradient).  k = 3, pad = 1.
// grid.y = (n, c) plane, grid.x strides over row blocks; lanes along x: no integer division per element, the 9 weights of the
// plane are wave-uniform, every output reads 3 rows x 3 shifted (L1-resident) values.
__global__ __launch_bounds__(256) void dw_conv3_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int C, int H,
                                                       int W, int flip) {
  const int nc = blockIdx.y;
  const int c = nc % C;
  const float* xp = x + (long long)nc * H * W;
  float* yp = y + (long long)nc * H * W;
  float wv[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wv[t] = w[(long long)c * 9 + (flip ? 8 - t : t)];
  const int lanes_per_row = (W + 255) / 256;             // 256-thread segments per row
  const int nseg = H * lanes_per_row;
  for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    const int yy = seg / lanes_per_row;
    const int xx = (seg - yy * lanes_per_row) * 256 + threadIdx.x;
    if (xx >= W) continue;
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      const int sy = yy + ty - 1;
      if (sy < 0 || sy >= H) continue;
      const float* row = xp + (long long)sy * W;
      const float l = xx > 0 ? row[xx - 1] : 0.f, m = row[xx], r = xx + 1 < W ? row[xx + 1] : 0.f;
      acc = fmaf(wv[ty * 3], l, fmaf(wv[ty * 3 + 1], m, fmaf(wv[ty * 3 + 2], r, acc)));
    }
    yp[(long long)yy * W + xx] = acc;
  }
}

// dw[c][t] += sum_{n,y,x} g[n,c,y,x] * x[n,c,y+ty-1,x+tx-1];  grid = (row blocks, N*C): a block walks whole rows, lanes along x
// nrows > 1 (deterministic mode, dpf_common.h): grid = (1, C) and rows_per_block = H -- one workgroup per channel walks every sample, so
// each dw address receives a single atomic add
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ dw,
                                                       int C, int H, int W, int rows_per_block, int nrows) {
  __shared__ float sm[4];
  const int c = blockIdx.y % C;
  const long long S = (long long)H * W;
  const int y0 = blockIdx.x * rows_per_block, y1 = min(H, y0 + rows_per_block);
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int row = blockIdx.y; row < (nrows > 1 ? nrows : blockIdx.y + 1); row += C)
  for (int yy = y0; yy < y1; ++yy) {
    const float* gp = g + (long long)row * S;
    const float* xp = x + (long long)row * S;
    for (int xx = threadIdx.x; xx < W; xx += 256) {
      const float gv = gp[(long long)yy * W + xx];
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) {
        const int sy = yy + ty - 1;
        if (sy < 0 || sy >= H) continue;
        const float* r = xp + (long long)sy * W;
        acc[ty * 3] += gv * (xx > 0 ? r[xx - 1] : 0.f);
        acc[ty * 3 + 1] += gv * r[xx];
        acc[ty * 3 + 2] += gv * (xx + 1 < W ? r[xx + 1] : 0.f);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float v = dpf_block_sum_256(acc[t], sm);
    if (threadIdx.x == 0) atomicAdd(&dw[c * 9 + t], v);
  }
}

// General window (DPNet: src/module/asm/basics.py:42 behind src/model/dpnet/modules.py:13,68-70 and mainmodel.py:68-71): k in {1, 3}, any
// 0 <= pad <= 3, output extent H + 2 pad - k + 1.  out[n,c,oy,ox] = sum_t w[c][t] * in[n,c,oy+off+ty,ox+off+tx], zero outside the input;
// forward: off = -pad; data gradient: in = g, off = pad - (k - 1), taps mirrored (off may be positive: pad > k - 1 crops).
template <int K>
__global__ __launch_bounds__(256) void dw_convg_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int C, int IH,
                                                       int IW, int OH, int OW, int off, int flip) {
  const int nc = blockIdx.y;
  const int c = nc % C;
  const float* xp = x + (long long)nc * IH * IW;
  float* yp = y + (long long)nc * OH * OW;
  float wv[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wv[t] = w[(long long)c * K * K + (flip ? K * K - 1 - t : t)];
  const int lanes_per_row = (OW + 255) / 256;
  const int nseg = OH * lanes_per_row;
  for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    const int yy = seg / lanes_per_row;
    const int xx = (seg - yy * lanes_per_row) * 256 + threadIdx.x;
    if (xx >= OW) continue;
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < K; ++ty) {
      const int sy = yy + off + ty;
      if (sy < 0 || sy >= IH) continue;
      const float* row = xp + (long long)sy * IW;
#pragma unroll
      for (int tx = 0; tx < K; ++tx) {
        const int sx = xx + off + tx;
        const float v = (sx >= 0 && sx < IW) ? row[sx] : 0.f;
        acc = fmaf(wv[ty * K + tx], v, acc);
      }
    }
    yp[(long long)yy * OW + xx] = acc;
  }
}

// dw[c][t] += sum_{n,oy,ox} g[n,c,oy,ox] * x[n,c,oy-pad+ty,ox-pad+tx]; g [.., OH, OW], x [.., H, W].  Grid and deterministic mode as
// dw_wgrad_kernel: nrows > 1 -> one workgroup per channel walks every sample, one add per dw address.
template <int K>
__global__ __launch_bounds__(256) void dw_wgradg_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ dw, int C, int H,
                                                        int W, int OH, int OW, int pad, int rows_per_block, int nrows) {
  __shared__ float sm[4];
  const int c = blockIdx.y % C;
  const int y0 = blockIdx.x * rows_per_block, y1 = min(OH, y0 + rows_per_block);
  float acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
  for (int row = blockIdx.y; row < (nrows > 1 ? nrows : blockIdx.y + 1); row += C) {
    const float* gp = g + (long long)row * OH * OW;
    const float* xp = x + (long long)row * H * W;
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = threadIdx.x; xx < OW; xx += 256) {
        const float gv = gp[(long long)yy * OW + xx];
#pragma unroll
        for (int ty = 0; ty < K; ++ty) {
          const int sy = yy - pad + ty;
          if (sy < 0 || sy >= H) continue;
          const float* r = xp + (long long)sy * W;
#pragma unroll
          for (int tx = 0; tx < K; ++tx) {
            const int sx = xx - pad + tx;
            acc[ty * K + tx] += gv * ((sx >= 0 && sx < W) ? r[sx] : 0.f);
          }
        }
      }
  }
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    const float v = dpf_block_sum_256(acc[t], sm);
    if (threadIdx.x == 0) atomicAdd(&dw[c * K * K + t], v);
  }
}

// the general-window launches; `in` has extent (IH, IW), `out` (OH, OW)
int dw_general(const float* in, const float* w, float* out, int N, int C, int IH, int IW, int OH, int OW, int k, int off, int flip, hipStream_t st) {
  if (OH <= 0 || OW <= 0) return DPF_ERR_INVALID_ARG;
  const int nseg = OH * ((OW + 255) / 256);
  int gx = 4096 / (N * C) + 1;
  if (gx > nseg) gx = nseg;
  if (k == 3)
    hipLaunchKernelGGL(dw_convg_kernel<3>, dim3(gx, N * C), dim3(256), 0, st, in, w, out, C, IH, IW, OH, OW, off, flip);
  else
    hipLaunchKernelGGL(dw_convg_kernel<1>, dim3(gx, N * C), dim3(256), 0, st, in, w, out, C, IH, IW, OH, OW, off, flip);
  return dpf_check_launch();
}

bool dw_window_ok(int k, int pad) { return (k == 1 || k == 3) && pad >= 0 && pad <= 3; }

}  // namespace

extern "C" {

// x [N,C,H,W], w [C,1,k,k] -> y [N,C,H+2pad-k+1,W+2pad-k+1] (stride 1, dilation 1, padding `pad`); k in {1, 3}, 0 <= pad <= 3.
// k = 3, pad = 1 runs dw_conv3_kernel, every other window the general kernel.
int dpf_depthwise_conv2d_forward(const float* x, const float* w, float* y, int N, int C, int H, int W, int k, int pad, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!x || !w || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DPF_ERR_INVALID_ARG;
  if (!dw_window_ok(k, pad) || (long long)N * C > 65535) return DPF_ERR_UNSUPPORTED;
  if (k != 3 || pad != 1) return dw_general(x, w, y, N, C, H, W, H + 2 * pad - k + 1, W + 2 * pad - k + 1, k, -pad, 0, (hipStream_t)stream);
  {
    const int nseg = H * ((W + 255) / 256);
    int gx = 4096 / (N * C) + 1;
    if (gx > nseg) gx = nseg;
    hipLaunchKernelGGL(dw_conv3_kernel, dim3(gx, N * C), dim3(256), 0, (hipStream_t)stream, x, w, y, C, H, W, 0);
  }
  return dpf_check_launch();
}

// g [N,C,H+2pad-k+1,W+2pad-k+1] -> dx [N,C,H,W] (overwritten)
int dpf_depthwise_conv2d_backward_data(const float* g, const float* w, float* dx, int N, int C, int H, int W, int k, int pad, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!g || !w || !dx || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DPF_ERR_INVALID_ARG;
  if (!dw_window_ok(k, pad) || (long long)N * C > 65535) return DPF_ERR_UNSUPPORTED;
  if (k != 3 || pad != 1)
    return dw_general(g, w, dx, N, C, H + 2 * pad - k + 1, W + 2 * pad - k + 1, H, W, k, pad - (k - 1), 1, (hipStream_t)stream);
  {
    const int nseg = H * ((W + 255) / 256);
    int gx = 4096 / (N * C) + 1;
    if (gx > nseg) gx = nseg;
    hipLaunchKernelGGL(dw_conv3_kernel, dim3(gx, N * C), dim3(256), 0, (hipStream_t)stream, g, w, dx, C, H, W, 1);
  }
  return dpf_check_launch();
}

// dw [C,1,k,k] += ...   (x [N,C,H,W], g on the output grid)
int dpf_depthwise_conv2d_backward_weight(const float* g, const float* x, float* dw, int N, int C, int H, int W, int k, int pad, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!g || !x || !dw || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !dw_window_ok(k, pad) || (long long)N * C > 65535) return DPF_ERR_INVALID_ARG;
  if (k != 3 || pad != 1) {
    const int OH = H + 2 * pad - k + 1, OW = W + 2 * pad - k + 1;
    if (OH <= 0 || OW <= 0) return DPF_ERR_INVALID_ARG;
    const int rpb = dpf_div_up(4096, OW);                 // ~4096 elements per block
    const bool det = dpf_deterministic();
    const dim3 grid = det ? dim3(1, (unsigned)C) : dim3((unsigned)dpf_div_up(OH, rpb), (unsigned)(N * C));
    if (k == 3)
      hipLaunchKernelGGL(dw_wgradg_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, g, x, dw, C, H, W, OH, OW, pad, det ? OH : rpb, det ? N * C : 1);
    else
      hipLaunchKernelGGL(dw_wgradg_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, g, x, dw, C, H, W, OH, OW, pad, det ? OH : rpb, det ? N * C : 1);
    return dpf_check_launch();
  }
  {
    int rpb = dpf_div_up(4096, W);                 // ~4096 elements per block
    if (rpb < 1) rpb = 1;
    if (dpf_deterministic())
      hipLaunchKernelGGL(dw_wgrad_kernel, dim3(1, (unsigned)C), dim3(256), 0, (hipStream_t)stream, g, x, dw, C, H, W, H, N * C);
    else
      hipLaunchKernelGGL(dw_wgrad_kernel, dim3((unsigned)dpf_div_up(H, rpb), (unsigned)(N * C)), dim3(256), 0, (hipStream_t)stream, g, x, dw, C, H, W,
                         rpb, 1);
  }
  return dpf_check_launch();
}

}  // extern "C"
