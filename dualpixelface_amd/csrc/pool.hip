// Max-pool 2-D, forward (value + int32 arg-max plane) and backward (gather): nn.MaxPool2d(k, stride, padding) of DPNet
// (reference: src/model/dpnet/modules.py:20,46): k3 s1 p0, k3 s2 p0 and k7 s2 p1; floor output size, padding counts as -inf.
// HBM-bound: forward reads 4 B and writes 8 B per output element (the window's re-reads come from L1/L2), backward reads the gradient
// and index planes and writes 4 B per input element.  One thread per element, lanes along W.
//
// Tie rule (PyTorch's): the window is scanned row-major and the running maximum is replaced only by a strictly greater value or by a
// NaN.  Ties are the common case behind a padded 1x1 conv + BN + PReLU (constant border per channel) and on raw images.
//
// Backward is a gather: an input element sums, in ascending (oy, ox) order, the gradients of the <= ceil(k/s)^2 windows whose stored
// index names it.  No atomics: the same bits on every run, in every mode.
#include "dpf_common.h"

namespace {

struct PoolP {
  int H, W, OH, OW, k, s, pad;
  long long planes;
};

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx, PoolP p) {
  const int segs = (p.OW + 255) / 256;
  const long long nseg = (long long)p.OH * segs;
  for (long long plane = blockIdx.y; plane < p.planes; plane += gridDim.y) {
    const float* xp = x + plane * p.H * p.W;
    float* yp = y + plane * p.OH * p.OW;
    int* ip = idx + plane * p.OH * p.OW;
    for (long long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
      const int oy = (int)(seg / segs);
      const int ox = (int)(seg - (long long)oy * segs) * 256 + threadIdx.x;
      if (ox >= p.OW) continue;
      int y0 = oy * p.s - p.pad, x0 = ox * p.s - p.pad;
      const int y1 = min(y0 + p.k, p.H), x1 = min(x0 + p.k, p.W);
      y0 = max(y0, 0);
      x0 = max(x0, 0);
      float best = -INFINITY;
      int bi = y0 * p.W + x0;
      for (int yy = y0; yy < y1; ++yy) {
        const float* row = xp + (long long)yy * p.W;
        for (int xx = x0; xx < x1; ++xx) {
          const float v = row[xx];
          if (v > best || v != v) {
            best = v;
            bi = yy * p.W + xx;
          }
        }
      }
      yp[(long long)oy * p.OW + ox] = best;
      ip[(long long)oy * p.OW + ox] = bi;
    }
  }
}

// floor division for a possibly negative numerator
__device__ __forceinline__ int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ g, const int* __restrict__ idx, float* __restrict__ dx, PoolP p) {
  const int segs = (p.W + 255) / 256;
  const long long nseg = (long long)p.H * segs;
  for (long long plane = blockIdx.y; plane < p.planes; plane += gridDim.y) {
    const float* gp = g + plane * p.OH * p.OW;
    const int* ip = idx + plane * p.OH * p.OW;
    float* dp = dx + plane * p.H * p.W;
    for (long long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
      const int iy = (int)(seg / segs);
      const int ix = (int)(seg - (long long)iy * segs) * 256 + threadIdx.x;
      if (ix >= p.W) continue;
      // windows that contain (iy, ix): o*s - pad <= i <= o*s - pad + k - 1
      const int oy0 = max(fdiv(iy + p.pad - p.k + p.s, p.s), 0), oy1 = min((iy + p.pad) / p.s, p.OH - 1);
      const int ox0 = max(fdiv(ix + p.pad - p.k + p.s, p.s), 0), ox1 = min((ix + p.pad) / p.s, p.OW - 1);
      const int me = iy * p.W + ix;
      float acc = 0.f;
      for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
          const long long o = (long long)oy * p.OW + ox;
          if (ip[o] == me) acc += gp[o];
        }
      dp[(long long)iy * p.W + ix] = acc;
    }
  }
}

int fill(PoolP& p, int N, int C, int H, int W, int k, int stride, int pad) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return DPF_ERR_INVALID_ARG;
  if (k < 1 || k > 7 || (stride != 1 && stride != 2) || pad < 0 || pad > k / 2) return DPF_ERR_UNSUPPORTED;
  if ((long long)H * W >= (1LL << 31)) return DPF_ERR_UNSUPPORTED;          // int32 index plane
  p.H = H; p.W = W; p.k = k; p.s = stride; p.pad = pad;
  p.OH = (H + 2 * pad - k) / stride + 1;
  p.OW = (W + 2 * pad - k) / stride + 1;
  p.planes = (long long)N * C;
  if (H + 2 * pad < k || W + 2 * pad < k) return DPF_ERR_INVALID_ARG;
  return DPF_OK;
}

dim3 grid_for(const PoolP& p, int rows, int width) {
  const long long nseg = (long long)rows * ((width + 255) / 256);
  const long long gy = p.planes < 4096 ? p.planes : 4096;
  long long gx = 8192 / gy + 1;                  // ~8 workgroups per CU over the whole launch
  if (gx > nseg) gx = nseg;
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

extern "C" {

// x [N,C,H,W] -> y, idx [N,C,OH,OW] with OH = (H + 2 pad - k) / stride + 1 (floor); idx holds iy * W + ix of the chosen element
int dpf_maxpool2d_forward(const float* x, float* y, int* idx, int N, int C, int H, int W, int k, int stride, int pad, void* stream) {
  dpf_clear_error();
  if (!x || !y || !idx) return DPF_ERR_INVALID_ARG;
  PoolP p;
  const int rc = fill(p, N, C, H, W, k, stride, pad);
  if (rc != DPF_OK) return rc;
  hipLaunchKernelGGL(maxpool_fwd_kernel, grid_for(p, p.OH, p.OW), dim3(256), 0, (hipStream_t)stream, x, y, idx, p);
  return dpf_check_launch();
}

// g, idx [N,C,OH,OW] -> dx [N,C,H,W] (overwritten)
int dpf_maxpool2d_backward(const float* g, const int* idx, float* dx, int N, int C, int H, int W, int k, int stride, int pad, void* stream) {
  dpf_clear_error();
  if (!g || !idx || !dx) return DPF_ERR_INVALID_ARG;
  PoolP p;
  const int rc = fill(p, N, C, H, W, k, stride, pad);
  if (rc != DPF_OK) return rc;
  hipLaunchKernelGGL(maxpool_bwd_kernel, grid_for(p, p.H, p.W), dim3(256), 0, (hipStream_t)stream, g, idx, dx, p);
  return dpf_check_launch();
}

}  // extern "C"
