// Wide-window dense 2-D convolution: 28 <= kh * kw <= 49 taps (kh, kw <= 7), stride 1 or 2, dilation 1; forward, data gradient and weight
// gradient.  DPNet's 7x7 convolutions (reference: src/model/dpnet/modules.py:44, mainmodel.py:81-85): the 6 -> 8 stride-2 stem and the
// five C -> 1 heads (C = 8 ... 128), which the MFMA tile kernels (MAXT = 27 taps) and conv_smallk (kw <= 3) do not take.
//
// The heads are a per-pixel reduction over C x 49 with ONE output channel -- an MFMA tile would carry one real row -- and the whole
// family is well under 1 % of the step's FLOPs, so these are plain fp32 FMA kernels: exact fp32 products whatever dpf_set_f32_matrix_path
// says.  Input rows are staged in LDS (every input element is read from HBM once per tile and channel group); the weights are
// wave-uniform and come through the scalar cache.
//
// The weight gradient writes per-chunk partial sums to a slab and folds them in a fixed order: no float atomics, the same bits on every
// run in every mode (the deterministic-mode convention of dpf_common.h holds unconditionally).
#include "conv_internal.h"

namespace {

constexpr int WMAXK = 7;            // largest window extent per axis
constexpr int TW = 64, TH = 4;      // output tile of the forward / data-gradient kernels: one thread per position, lanes along W
constexpr int FCC = 4;              // reduction channels staged per pass

struct WideP {
  int N, R, K, Ktot, k0;            // R reduction channels, K output channels computed of Ktot, first one k0
  int IH, IW, OH, OW;               // `in` extent, `out` extent
  int kh, kw, s, ph, pw;
  int PH, PW;                       // staged patch extent
  int tilesW, tilesH;
  int wA, wB, mode;                 // weight tensor w[wA][wB][T]; mode 0: out = A, reduce = B; mode 1: reduce = A, out = B
};

__device__ __forceinline__ long long widx(const WideP& p, int o, int r) {
  return p.mode == 0 ? ((long long)o * p.wB + r) : ((long long)r * p.wB + o);
}

// out[n,k,oy,ox] = bias[k] + sum_{r,ty,tx} w[k][r][ty][tx] * in[n,r,oy*s-ph+ty,ox*s-pw+tx]
template <int KB>
__global__ __launch_bounds__(256) void wide_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, WideP p) {
  extern __shared__ float lds[];
  const int tile = blockIdx.x;
  const int tx0 = (tile % p.tilesW) * TW, ty0 = (tile / p.tilesW) * TH;
  const int kg = blockIdx.y * KB;                       // first output channel of this group (relative to k0)
  const int n = blockIdx.z;
  const int lx = threadIdx.x & (TW - 1), ly = threadIdx.x / TW;
  const int oy = ty0 + ly, ox = tx0 + lx;
  const int iy0 = ty0 * p.s - p.ph, ix0 = tx0 * p.s - p.pw;
  const int T = p.kh * p.kw, PS = p.PH * p.PW;
  float acc[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) acc[k] = 0.f;
  for (int r0 = 0; r0 < p.R; r0 += FCC) {
    const int rc = min(FCC, p.R - r0);
    __syncthreads();
    for (int i = threadIdx.x; i < rc * PS; i += 256) {
      const int r = i / PS, q = i - r * PS;
      const int py = q / p.PW, px = q - py * p.PW;
      const int iy = iy0 + py, ix = ix0 + px;
      float v = 0.f;
      if (iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) v = in[(((long long)n * p.R + r0 + r) * p.IH + iy) * p.IW + ix];
      lds[i] = v;
    }
    __syncthreads();
    for (int r = 0; r < rc; ++r) {
      const float* pl = lds + r * PS + (ly * p.s) * p.PW + lx * p.s;
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        if (kg + k >= p.K) break;                                                   // (wave-uniform)
        const float* wk = w + widx(p, p.k0 + kg + k, r0 + r) * T;                   // wave-uniform address: scalar loads
        float a = acc[k];
        for (int ty = 0; ty < p.kh; ++ty)
          for (int tx = 0; tx < p.kw; ++tx) a = fmaf(wk[ty * p.kw + tx], pl[ty * p.PW + tx], a);
        acc[k] = a;
      }
    }
  }
  if (oy < p.OH && ox < p.OW) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (kg + k >= p.K) break;
      const int kk = p.k0 + kg + k;
      out[(((long long)n * p.Ktot + kk) * p.OH + oy) * p.OW + ox] = acc[k] + (bias ? bias[kk] : 0.f);
    }
  }
}

// transposed (data gradient of the conv above / ConvTranspose): `in` lives on the strided grid,
// out[n,k,oy,ox] = bias[k] + sum_{r,ty,tx} w[r][k][ty][tx] * in[n,r,(oy+ph-ty)/s,(ox+pw-tx)/s]   (terms with a remainder or outside: none)
template <int KB>
__global__ __launch_bounds__(256) void wide_tr_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, WideP p) {
  extern __shared__ float lds[];
  const int tile = blockIdx.x;
  const int tx0 = (tile % p.tilesW) * TW, ty0 = (tile / p.tilesW) * TH;
  const int kg = blockIdx.y * KB;
  const int n = blockIdx.z;
  const int lx = threadIdx.x & (TW - 1), ly = threadIdx.x / TW;
  const int oy = ty0 + ly, ox = tx0 + lx;
  // first staged row / column: floor((o0 + p - (k - 1)) / s); the numerator may be negative -> shift by a multiple of s
  const int iy0 = (ty0 + p.ph - (p.kh - 1) + 8 * p.s) / p.s - 8, ix0 = (tx0 + p.pw - (p.kw - 1) + 8 * p.s) / p.s - 8;
  const int T = p.kh * p.kw, PS = p.PH * p.PW;
  float acc[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) acc[k] = 0.f;
  for (int r0 = 0; r0 < p.R; r0 += FCC) {
    const int rc = min(FCC, p.R - r0);
    __syncthreads();
    for (int i = threadIdx.x; i < rc * PS; i += 256) {
      const int r = i / PS, q = i - r * PS;
      const int py = q / p.PW, px = q - py * p.PW;
      const int iy = iy0 + py, ix = ix0 + px;
      float v = 0.f;
      if (iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) v = in[(((long long)n * p.R + r0 + r) * p.IH + iy) * p.IW + ix];
      lds[i] = v;
    }
    __syncthreads();
    for (int r = 0; r < rc; ++r) {
      const float* pl = lds + r * PS;
      for (int ty = 0; ty < p.kh; ++ty) {
        const int ny = oy + p.ph - ty;
        if (ny < 0 || (p.s == 2 && (ny & 1))) continue;
        const int py = ny / p.s - iy0;
        for (int tx = 0; tx < p.kw; ++tx) {
          const int nx = ox + p.pw - tx;
          if (nx < 0 || (p.s == 2 && (nx & 1))) continue;
          const int px = nx / p.s - ix0;
          if (py < 0 || py >= p.PH || px < 0 || px >= p.PW) continue;            // (only positions beyond the output extent)
          const float v = pl[py * p.PW + px];
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            if (kg + k >= p.K) break;
            acc[k] = fmaf(w[widx(p, p.k0 + kg + k, r0 + r) * T + ty * p.kw + tx], v, acc[k]);
          }
        }
      }
    }
  }
  if (oy < p.OH && ox < p.OW) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (kg + k >= p.K) break;
      const int kk = p.k0 + kg + k;
      out[(((long long)n * p.Ktot + kk) * p.OH + oy) * p.OW + ox] = acc[k] + (bias ? bias[kk] : 0.f);
    }
  }
}

// ---- weight gradient: dW[k][c][ty][tx] = sum_{n,qy,qx} g[n,k,qy,qx] * x[n,c,qy*s-ph+ty,qx*s-pw+tx]
constexpr int GW = 32, GH = 8;      // g tile (256 positions)
constexpr int GKB = 8;              // g channels per workgroup

struct WideWgP {
  int N, C, K, Ktot, k0;
  int IH, IW, QH, QW;
  int kh, kw, s, ph, pw;
  int PH, PW, CC;                   // staged x patch, x channels per workgroup (CC * T <= 256: one thread per (channel, tap))
  int tilesW, tilesH, cchunks, kgroups;
  long long ntiles;                 // N * tilesH * tilesW
  int nparts;                       // workgroups along the position axis; part i takes tiles i, i + nparts, ...
};

// grid = (nparts, cchunks, kgroups); slab[part][K][C][T]
__global__ __launch_bounds__(256) void wide_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ slab, WideWgP p) {
  extern __shared__ float lds[];
  const int T = p.kh * p.kw, PS = p.PH * p.PW;
  float* s_x = lds;                       // [CC][PH][PW]
  float* s_g = lds + p.CC * PS;           // [GKB][GH * GW]
  const int c0 = blockIdx.y * p.CC, kg = blockIdx.z * GKB;
  const int cn = min(p.CC, p.C - c0), kn = min(GKB, p.K - kg);
  const int cc = threadIdx.x / T, t = threadIdx.x - cc * T;
  const bool live = cc < cn;
  const int ty = t / p.kw, tx = t - ty * p.kw;
  float acc[GKB];
#pragma unroll
  for (int k = 0; k < GKB; ++k) acc[k] = 0.f;
  for (long long tile = blockIdx.x; tile < p.ntiles; tile += p.nparts) {
    const int tw = (int)(tile % p.tilesW);
    const long long rest = tile / p.tilesW;
    const int th = (int)(rest % p.tilesH), n = (int)(rest / p.tilesH);
    const int qy0 = th * GH, qx0 = tw * GW;
    const int iy0 = qy0 * p.s - p.ph, ix0 = qx0 * p.s - p.pw;
    __syncthreads();
    for (int i = threadIdx.x; i < cn * PS; i += 256) {
      const int r = i / PS, q = i - r * PS;
      const int py = q / p.PW, px = q - py * p.PW;
      const int iy = iy0 + py, ix = ix0 + px;
      float v = 0.f;
      if (iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) v = x[(((long long)n * p.C + c0 + r) * p.IH + iy) * p.IW + ix];
      s_x[i] = v;
    }
    for (int i = threadIdx.x; i < kn * GH * GW; i += 256) {
      const int k = i / (GH * GW), q = i - k * (GH * GW);
      const int qy = qy0 + q / GW, qx = qx0 + (q & (GW - 1));
      float v = 0.f;
      if (qy < p.QH && qx < p.QW) v = g[(((long long)n * p.Ktot + p.k0 + kg + k) * p.QH + qy) * p.QW + qx];
      s_g[i] = v;
    }
    __syncthreads();
    if (live) {
      const float* px = s_x + cc * PS + ty * p.PW + tx;
      for (int qy = 0; qy < GH; ++qy)
        for (int qx = 0; qx < GW; ++qx) {
          const float xv = px[(qy * p.s) * p.PW + qx * p.s];
#pragma unroll
          for (int k = 0; k < GKB; ++k) {
            if (k >= kn) break;
            acc[k] = fmaf(s_g[k * (GH * GW) + qy * GW + qx], xv, acc[k]);          // (s_g: one address per wave -> broadcast)
          }
        }
    }
  }
  if (live) {
    float* sp = slab + (long long)blockIdx.x * p.K * p.C * T;
#pragma unroll
    for (int k = 0; k < GKB; ++k) {
      if (k >= kn) break;
      sp[((long long)(kg + k) * p.C + c0 + cc) * T + t] = acc[k];
    }
  }
}

// dw[i] (+)= slab[0][i] + slab[1][i] + ... in this order
__global__ __launch_bounds__(256) void wide_wgrad_fold_kernel(const float* __restrict__ slab, float* __restrict__ dw, long long n, int nparts, int accumulate) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float a = 0.f;
    for (int q = 0; q < nparts; ++q) a += slab[(long long)q * n + i];
    dw[i] = accumulate ? dw[i] + a : a;
  }
}

bool wide_window(int kd, int kh, int kw, int sd, int sh, int sw, int pd, int dd, int dh, int dw) {
  const int T = kh * kw;
  return kd == 1 && sd == 1 && pd == 0 && dd == 1 && dh == 1 && dw == 1 && kh <= WMAXK && kw <= WMAXK && T >= 28 && T <= 49 && sh == sw &&
         (sh == 1 || sh == 2);
}

constexpr int WG_MAXPARTS = 256;

}  // namespace

bool dpf_wide_eligible(int T, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int dd, int dh, int dw) {
  return T == kh * kw && wide_window(kd, kh, kw, sd, sh, sw, pd, dd, dh, dw);
}

// One launch for the output channels [d.k0, d.k0 + d.K) (forward or transposed); DPF_ERR_UNSUPPORTED: not a wide 2-D window, or `accumulate`.
int dpf_wide_conv(const float* x, const float* w, const float* bias, float* out, const DpfConvDesc& d, hipStream_t st) {
  if (!wide_window(d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.dd, d.dh, d.dw) || d.ID != 1 || d.OD != 1 || d.accumulate) return DPF_ERR_UNSUPPORTED;
  if (d.ph < 0 || d.pw < 0 || d.OH <= 0 || d.OW <= 0) return DPF_ERR_INVALID_ARG;
  WideP p{};
  p.N = d.N; p.R = d.C; p.K = d.K; p.Ktot = d.Ktot; p.k0 = d.k0;
  p.IH = d.IH; p.IW = d.IW; p.OH = d.OH; p.OW = d.OW;
  p.kh = d.kh; p.kw = d.kw; p.s = d.sh; p.ph = d.ph; p.pw = d.pw;
  p.wA = d.wA; p.wB = d.wB; p.mode = d.mode;
  p.tilesW = dpf_div_up(d.OW, TW);
  p.tilesH = dpf_div_up(d.OH, TH);
  if (!d.transposed) {
    p.PH = (TH - 1) * p.s + p.kh;
    p.PW = (TW - 1) * p.s + p.kw;
  } else {
    p.PH = (TH + p.kh - 2) / p.s + 2;
    p.PW = (TW + p.kw - 2) / p.s + 2;
  }
  const size_t lds = (size_t)FCC * p.PH * p.PW * sizeof(float);
  if (lds > 48 * 1024 || d.N > 65535) return DPF_ERR_UNSUPPORTED;
  const long long tiles = (long long)p.tilesW * p.tilesH;
  if (tiles > 0x7fffffffLL) return DPF_ERR_UNSUPPORTED;
  const int KB = d.K == 1 ? 1 : (d.K <= 4 ? 4 : 8);
  const dim3 grid((unsigned)tiles, (unsigned)dpf_div_up(d.K, KB), (unsigned)d.N);
#define DPF_WIDE(KERN)                                                                                          \
  switch (KB) {                                                                                                 \
    case 1: hipLaunchKernelGGL((KERN<1>), grid, dim3(256), lds, st, x, w, bias, out, p); break;                 \
    case 4: hipLaunchKernelGGL((KERN<4>), grid, dim3(256), lds, st, x, w, bias, out, p); break;                 \
    default: hipLaunchKernelGGL((KERN<8>), grid, dim3(256), lds, st, x, w, bias, out, p); break;                \
  }
  if (d.transposed) {
    DPF_WIDE(wide_tr_kernel)
  } else {
    DPF_WIDE(wide_fwd_kernel)
  }
#undef DPF_WIDE
  return dpf_check_launch();
}

long long dpf_wide_wgrad_workspace_floats(int T, int C, int K) {
  if (T < 28 || T > 49) return 0;
  return (long long)WG_MAXPARTS * K * C * T;
}

// dw[d.K][C][T] for the g channels [d.k0, d.k0 + d.K); ws: the slab.  DPF_ERR_UNSUPPORTED: not a wide window, or no room for one slab row.
int dpf_wide_wgrad(const float* g, const float* x, float* dw, float* ws, long long ws_floats, const DpfWgradDesc& d, int accumulate,
                   hipStream_t st) {
  if (!wide_window(d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.dd, d.dh, d.dw) || d.ID != 1 || d.QD != 1) return DPF_ERR_UNSUPPORTED;
  if (d.ph < 0 || d.pw < 0 || d.QH <= 0 || d.QW <= 0) return DPF_ERR_INVALID_ARG;
  WideWgP p{};
  const int T = d.kh * d.kw;
  p.N = d.N; p.C = d.C; p.K = d.K; p.Ktot = d.Ktot; p.k0 = d.k0;
  p.IH = d.IH; p.IW = d.IW; p.QH = d.QH; p.QW = d.QW;
  p.kh = d.kh; p.kw = d.kw; p.s = d.sh; p.ph = d.ph; p.pw = d.pw;
  p.PH = (GH - 1) * p.s + p.kh;
  p.PW = (GW - 1) * p.s + p.kw;
  p.CC = 256 / T;
  if (p.CC > d.C) p.CC = d.C;
  p.tilesW = dpf_div_up(d.QW, GW);
  p.tilesH = dpf_div_up(d.QH, GH);
  p.cchunks = dpf_div_up(d.C, p.CC);
  p.kgroups = dpf_div_up(d.K, GKB);
  p.ntiles = (long long)d.N * p.tilesH * p.tilesW;
  const long long row = (long long)d.K * d.C * T;
  long long parts = p.ntiles < WG_MAXPARTS ? p.ntiles : WG_MAXPARTS;
  if (!ws || ws_floats < row) return DPF_ERR_UNSUPPORTED;
  if (parts > ws_floats / row) parts = ws_floats / row;
  p.nparts = (int)parts;
  const size_t lds = ((size_t)p.CC * p.PH * p.PW + (size_t)GKB * GH * GW) * sizeof(float);
  if (lds > 64 * 1024 || p.cchunks > 65535 || p.kgroups > 65535) return DPF_ERR_UNSUPPORTED;
  const int rc = conv_launch<wide_wgrad_kernel>(dim3((unsigned)p.nparts, (unsigned)p.cchunks, (unsigned)p.kgroups), dim3(256), lds, st, g, x, ws, p);
  if (rc != DPF_OK) return rc;
  hipLaunchKernelGGL(wide_wgrad_fold_kernel, dim3(dpf_ew_grid(row)), dim3(256), 0, st, ws, dw, row, p.nparts, accumulate);
  return dpf_check_launch();
}
