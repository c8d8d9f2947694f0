// The two label-free losses (loss_type 'photometric' and 'smoothness'; losses.PHOTOMETRICLoss / SMOOTHNESSLoss, ops.photometric_loss /
// ops.smoothness_loss): the target view warped onto the reference view by the predicted displacement and compared
// with it, and the edge-aware first-order smoothness of the prediction, each with a hand-written gradient into the prediction.  Every
// fp32 expression is written operation by operation under -ffp-contract=off, so that tests/photometric_cpu.py restates the warped
// values and the counted map bit for bit.
//
//   Y        (0.299 R + 0.587 G) + 0.114 B of the de-normalised image, R = x_0 std_0 + mean_0 and so on (dpf_image.h)
//   D        pred (target types 0, 1) or a / pred + b (2; pred <= 0 is not usable)
//   sample   sx = x + shift_x D, sy = y + shift_y D
//   warpable pred finite (and > 0 for type 2), mask NULL or > 0, 0 <= sx <= W - 1 and 0 <= sy <= H - 1
//   J        bilinear sample of Y_tgt: x0 = floor(sx), fx = sx - x0, x1 = min(x0 + 1, W - 1), likewise in y;
//            top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), J = top + fy (bot - top); 0 where not warpable
//   counted  the 3 x 3 window lies in the image and its nine pixels are warpable
//   window   i = I - I_centre, j = J - I_centre; sums of i, j, i i, j j, i j over the nine pixels in row-major order; m = sum / 9,
//            mu = I_centre + m, var = mean of squares - m^2, cov = mean of products - m_I m_J
//   term     alpha clamp((1 - SSIM) / 2, 0, 1) + (1 - alpha) sqrt((J - I)^2 + eps^2) at the centre
//   loss     sum_h w_h (sum terms_h / count_h), 0 for a head with count_h = 0
//
// Photometric forward: a luminance launch fills the caller's two planes, then one workgroup per 32 x 8 tile of one head of one sample
// (I, J and the warpable flag in LDS with a halo of 1) leaves one row (term sum, count) of fp64 in the workspace, and one workgroup
// folds the rows head by head (dpf_reduce.h).  Backward: a gather.  The workgroup warps its tile with a halo of 2, evaluates the windows
// of the tile and a halo of 1 -- d term / d J_k of a window is c0 + cI (I_k - mu_I) + cJ (J_k - mu_J), five numbers per window, zeros for
// a window that is not counted -- then every pixel adds what the nine windows through it owe it in row-major order, then the intensity term of its own
// window, and multiplies by d J / d D = shift_x d_x + shift_y d_y of its bilinear sample (the piecewise, right-sided derivative) and
// d D / d pred.  Windows on a tile edge are recomputed by both neighbours from the same inputs by the same instructions: no scratch, no
// atomics, and the bits repeat.  Samples are gathered from global memory wherever the displacement sends them.
//
//   pairs    (p, p + x^) and (p, p + y^); usable: both pred finite and both masks > 0
//   term     sqrt((pred_q - pred_p)^2 + eps^2) exp(-(gamma |Y_q - Y_p|))
//   loss     sum_h w_h (sum x-pairs / count_x,h + sum y-pairs / count_y,h)
//
// Smoothness forward: luminance launch, one workgroup per 32 x 8 tile leaves (x sum, x count, y sum, y count), one workgroup folds.
// Backward: every pixel gathers its left, right, upper and lower pair, in that order.
#include "dpf_head_loss.h"
#include "dpf_image.h"
#include "dpf_window.h"
#include <math.h>

extern "C" long long dpf_photometric_workspace_bytes(int B, int n, int H, int W);
extern "C" long long dpf_smoothness_workspace_bytes(int B, int n, int H, int W);

namespace {

constexpr int kBlock = 256;
constexpr int kTW = kDpfTileW, kTH = kDpfTileH;      // output tile, one pixel per thread (dpf_head_loss.h has the plan)

struct Photo {
  const float* pred;       // [B, n, H, W]
  const float* yref;       // [B, H, W]   luminance of the reference view
  const float* ytgt;       // [B, H, W]   luminance of the target view
  const float* ab;         // [B, 2] or NULL (types 0, 1)
  const float* mask;       // [B, H, W] or NULL
  int n, H, W, target_type;
  float sx, sy, alpha, eps;
};

struct Smooth {
  const float* pred;       // [B, n, H, W]
  const float* y;          // [B, H, W]   luminance of the guide
  const float* mask;       // [B, H, W] or NULL
  int n, H, W;
  float gamma, eps;
};

// grid (blocks over H W, planes): plane p of out [planes][HW] from the image p of img [planes][3][HW]
__global__ __launch_bounds__(256) void luma_kernel(const float* __restrict__ img0, const float* __restrict__ img1, int B, long long HW, DpfNorm nm,
                                                   float* __restrict__ out) {
  const int p = blockIdx.y;
  const float* __restrict__ g = (p < B ? img0 + (size_t)p * 3 * HW : img1 + (size_t)(p - B) * 3 * HW);
  float* __restrict__ o = out + (size_t)p * HW;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long long)gridDim.x * kBlock)
    o[i] = dpf_luma(g[i], g[i + HW], g[i + 2 * HW], nm);
}

// the warp of pixel (y, x), which lies in the image: -> warpable; J, and where asked the derivative of J with respect to pred
__device__ __forceinline__ bool warp_at(const Photo& g, const float* __restrict__ predh, const float* __restrict__ yt, size_t sbase, float a,
                                        float b, int y, int x, float& J, float* dJdpred) {
  J = 0.f;
  const size_t o = (size_t)y * g.W + x;
  const float p = predh[o];
  if (!dpf_finite_f(p)) return false;
  if (g.mask && !(g.mask[sbase + o] > 0.f)) return false;
  float D = p;
  if (g.target_type == 2) {
    if (!(p > 0.f)) return false;
    D = a / p + b;
  }
  const float sx = (float)x + g.sx * D, sy = (float)y + g.sy * D;
  if (!(sx >= 0.f && sx <= (float)(g.W - 1) && sy >= 0.f && sy <= (float)(g.H - 1))) return false;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const float fx = sx - fx0, fy = sy - fy0;
  const int x0 = min((int)fx0, g.W - 1), y0 = min((int)fy0, g.H - 1);      // (the clamp acts only where W - 1 is no fp32 number)
  const int x1 = min(x0 + 1, g.W - 1), y1 = min(y0 + 1, g.H - 1);
  const float* __restrict__ r0 = yt + (size_t)y0 * g.W;
  const float* __restrict__ r1 = yt + (size_t)y1 * g.W;
  const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
  const float dt = v01 - v00, db = v11 - v10;
  const float top = v00 + fx * dt, bot = v10 + fx * db;
  const float dv = bot - top;
  J = top + fy * dv;
  if (dJdpred) {
    const float gx = dt + fy * (db - dt);
    float dD = 1.f;                                        // d D / d pred = -a / pred^2
    if (g.target_type == 2) dD = -(a / (p * p));
    *dJdpred = (g.sx * gx + g.sy * dv) * dD;
  }
  return true;
}

// grid (ceil(W / 32), ceil(H / 8), B n), 256 threads = 8 rows x 32 columns.  part: [n][B tiles][2]
__global__ __launch_bounds__(256) void photo_forward_kernel(Photo g, double* __restrict__ part, float* __restrict__ warped_out,
                                                            unsigned char* __restrict__ counted_out) {
  constexpr int LW = kTW + 2, LH = kTH + 2;
  __shared__ float tI[LH * LW], tJ[LH * LW];
  __shared__ unsigned char tw[LH * LW];
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float* __restrict__ yr = g.yref + sbase;
  const float* __restrict__ yt = g.ytgt + sbase;
  const float b = g.target_type == 2 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 2 ? g.ab[2 * (size_t)s + 1] : 0.f;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  for (int i = t; i < LH * LW; i += kBlock) {
    const int ly = i / LW, lx = i - ly * LW;
    const int y = y0 - 1 + ly, x = x0 - 1 + lx;
    float I = 0.f, J = 0.f;
    bool ok = false;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
      I = yr[(size_t)y * g.W + x];
      ok = warp_at(g, predh, yt, sbase, a, b, y, x, J, nullptr);
    }
    tI[i] = I, tJ[i] = J, tw[i] = ok ? 1 : 0;
  }
  __syncthreads();
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  double acc[2] = {0.0, 0.0};
  if (x < g.W && y < g.H) {
    const int ly = ty + 1, lx = tx + 1;
    const bool counted = x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && all_nine<LW>(tw, ly, lx);
    if (counted) {
      Window w;
      window_of<LW>(tI, tJ, ly, lx, w);
      const float ds = fminf(fmaxf((1.f - w.ssim) / 2.f, 0.f), 1.f);
      const float d = tJ[ly * LW + lx] - tI[ly * LW + lx];
      const float ch = sqrtf(d * d + g.eps * g.eps);
      acc[0] = (double)(g.alpha * ds + (1.f - g.alpha) * ch);
      acc[1] = 1.0;
    }
    if (warped_out) {
      const size_t o = ((size_t)s * g.n + h) * HW + (size_t)y * g.W + x;
      warped_out[o] = tJ[ly * LW + lx];
      counted_out[o] = counted ? 1 : 0;
    }
  }
  dpf_block_reduce_d<2>(acc, part + dpf_tile_part_row(s, h, g.n) * 2);
}

// grid as the forward's
__global__ __launch_bounds__(256) void photo_backward_kernel(Photo g, DpfHeadW hw, const double* __restrict__ stats, const float* __restrict__ gout,
                                                             float* __restrict__ dpred) {
  constexpr int ZW = kTW + 4, ZH = kTH + 4;               // I, J, warpable: halo 2
  constexpr int CW = kTW + 2, CH = kTH + 2;               // windows: halo 1
  __shared__ float tI[ZH * ZW], tJ[ZH * ZW];
  __shared__ unsigned char tw[ZH * ZW];
  __shared__ float coef[5][CH * CW];
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float* __restrict__ yr = g.yref + sbase;
  const float* __restrict__ yt = g.ytgt + sbase;
  const float b = g.target_type == 2 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 2 ? g.ab[2 * (size_t)s + 1] : 0.f;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  for (int i = t; i < ZH * ZW; i += kBlock) {
    const int ly = i / ZW, lx = i - ly * ZW;
    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
    float I = 0.f, J = 0.f;
    bool ok = false;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
      I = yr[(size_t)y * g.W + x];
      ok = warp_at(g, predh, yt, sbase, a, b, y, x, J, nullptr);
    }
    tI[i] = I, tJ[i] = J, tw[i] = ok ? 1 : 0;
  }
  __syncthreads();
  for (int i = t; i < CH * CW; i += kBlock) {
    const int cy = i / CW, cx = i - cy * CW;
    const int y = y0 - 1 + cy, x = x0 - 1 + cx;
    const int ly = cy + 1, lx = cx + 1;
    float c0 = 0.f, cI = 0.f, cJ = 0.f, mI = 0.f, mJ = 0.f;
    if (x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && all_nine<ZW>(tw, ly, lx)) {
      Window w;
      window_of<ZW>(tI, tJ, ly, lx, w);
      const float ds = (1.f - w.ssim) / 2.f;
      if (ds >= 0.f && ds <= 1.f) {
        // d ssim / d J_k = (2 / 9) (muI A2 / (B1 B2) - ssim muJ / B1 + A1 / (B1 B2) (I_k - muI) - ssim / B2 (J_k - muJ)), and
        // d term / d ssim = -alpha / 2
        const float k = -(g.alpha / 9.f);
        const float den = w.B1 * w.B2;
        c0 = k * ((w.muI * w.A2) / den - (w.ssim * w.muJ) / w.B1);
        cI = k * (w.A1 / den);
        cJ = -(k * (w.ssim / w.B2));
        mI = w.muI, mJ = w.muJ;
      }
    }
    coef[0][i] = c0, coef[1][i] = cI, coef[2][i] = cJ, coef[3][i] = mI, coef[4][i] = mJ;
  }
  __syncthreads();
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= g.W || y >= g.H) return;                        // (no barrier below)
  const int ly = ty + 2, lx = tx + 2, cy = ty + 1, cx = tx + 1;
  float out = 0.f;
  if (tw[ly * ZW + lx]) {
    const float I = tI[ly * ZW + lx], J = tJ[ly * ZW + lx];
    float sum = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int c = (cy + dy) * CW + cx + dx;
        sum = sum + ((coef[0][c] + coef[1][c] * (I - coef[3][c])) + coef[2][c] * (J - coef[4][c]));
      }
    if (x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && all_nine<ZW>(tw, ly, lx)) {
      const float d = J - I;
      sum = sum + (1.f - g.alpha) * (d / sqrtf(d * d + g.eps * g.eps));
    }
    if (sum != 0.f) {
      float dJ = 0.f, Jagain;
      warp_at(g, predh, yt, sbase, a, b, y, x, Jagain, &dJ);
      const double cnt = stats[h];
      const float wk = cnt > 0.0 ? (float)((double)hw.w[h] / cnt) : 0.f;
      out = ((sum * dJ) * wk) * gout[0];
    }
  }
  dpred[((size_t)s * g.n + h) * HW + (size_t)y * g.W + x] = out;
}

// ---- smoothness
__device__ __forceinline__ bool smooth_ok(const Smooth& g, const float* __restrict__ predh, size_t sbase, size_t o) {
  return dpf_finite_f(predh[o]) && (!g.mask || g.mask[sbase + o] > 0.f);
}

// the pair (p, q), both usable: its term, and where asked d term / d pred_q (= -d term / d pred_p)
__device__ __forceinline__ float pair_term(const Smooth& g, const float* __restrict__ predh, const float* __restrict__ ys, size_t p, size_t q,
                                           float* dq) {
  const float d = predh[q] - predh[p];
  const float r = sqrtf(d * d + g.eps * g.eps);
  const float w = expf(-(g.gamma * fabsf(ys[q] - ys[p])));
  if (dq) *dq = (d / r) * w;
  return r * w;
}

// grid (ceil(W / 32), ceil(H / 8), B n).  part: [n][B tiles][4] = (x sum, x count, y sum, y count)
__global__ __launch_bounds__(256) void smooth_forward_kernel(Smooth g, double* __restrict__ part) {
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float* __restrict__ ys = g.y + sbase;
  const int x = blockIdx.x * kTW + (t & (kTW - 1)), y = blockIdx.y * kTH + t / kTW;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (x < g.W && y < g.H) {
    const size_t o = (size_t)y * g.W + x;
    if (smooth_ok(g, predh, sbase, o)) {
      if (x + 1 < g.W && smooth_ok(g, predh, sbase, o + 1)) acc[0] = (double)pair_term(g, predh, ys, o, o + 1, nullptr), acc[1] = 1.0;
      if (y + 1 < g.H && smooth_ok(g, predh, sbase, o + g.W)) acc[2] = (double)pair_term(g, predh, ys, o, o + g.W, nullptr), acc[3] = 1.0;
    }
  }
  dpf_block_reduce_d<4>(acc, part + dpf_tile_part_row(s, h, g.n) * 4);
}

// grid as the forward's, no LDS
__global__ __launch_bounds__(256) void smooth_backward_kernel(Smooth g, DpfHeadW hw, const double* __restrict__ stats, const float* __restrict__ gout,
                                                              float* __restrict__ dpred) {
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float* __restrict__ ys = g.y + sbase;
  const int x = blockIdx.x * kTW + (t & (kTW - 1)), y = blockIdx.y * kTH + t / kTW;
  if (x >= g.W || y >= g.H) return;
  const size_t o = (size_t)y * g.W + x;
  float out = 0.f;
  if (smooth_ok(g, predh, sbase, o)) {
    const double cx = stats[h], cy = stats[2 * kDpfMaxHeads + h];
    const float wx = cx > 0.0 ? (float)((double)hw.w[h] / cx) : 0.f, wy = cy > 0.0 ? (float)((double)hw.w[h] / cy) : 0.f;
    float sx = 0.f, sy = 0.f, d;
    if (x >= 1 && smooth_ok(g, predh, sbase, o - 1)) pair_term(g, predh, ys, o - 1, o, &d), sx = sx + d;
    if (x + 1 < g.W && smooth_ok(g, predh, sbase, o + 1)) pair_term(g, predh, ys, o, o + 1, &d), sx = sx - d;
    if (y >= 1 && smooth_ok(g, predh, sbase, o - g.W)) pair_term(g, predh, ys, o - g.W, o, &d), sy = sy + d;
    if (y + 1 < g.H && smooth_ok(g, predh, sbase, o + g.W)) pair_term(g, predh, ys, o, o + g.W, &d), sy = sy - d;
    out = (sx * wx + sy * wy) * gout[0];
  }
  dpred[((size_t)s * g.n + h) * HW + o] = out;
}

bool shape_ok(int B, int n, int H, int W) { return B > 0 && n >= 1 && n <= kDpfMaxHeads && H > 0 && W > 0; }

// the tile plan, refused as well where the 2 B luminance planes do not fit on gridDim.y of the luminance launch
long long tile_rows(int B, int n, int H, int W) { return 2LL * B > kDpfMaxGridZ ? -1 : dpf_tile_rows(B, n, H, W); }

int launch_luma(const float* img0, const float* img1, int B, int planes, long long HW, const DpfNorm& nm, float* out, hipStream_t st) {
  long long blocks = (HW + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(luma_kernel, dim3((unsigned)blocks, planes), dim3(kBlock), 0, st, img0, img1, B, HW, nm, out);
  return 0;
}

// argument checks shared by the photometric entry points; fills g and hw (the luminance planes are the caller's)
int prepare_photo(const float* pred, const float* ref_rgb, const float* tgt_rgb, const float* ab, const float* mask, int B, int n, int H, int W,
                  int target_type, float shift_x, float shift_y, float alpha, float eps, const float* norm_host, const float* weights,
                  const float* luma, Photo& g, DpfHeadW& hw) {
  if (!pred || !ref_rgb || !tgt_rgb || !norm_host || !weights || !luma || !shape_ok(B, n, H, W) || target_type < 0 || target_type > 2 ||
      (target_type == 2 && !ab) || !(alpha >= 0.f && alpha <= 1.f) || !(eps > 0.f) || !isfinite(eps) || !isfinite(shift_x) ||
      !isfinite(shift_y) || (shift_x == 0.f && shift_y == 0.f))
    return DPF_ERR_INVALID_ARG;
  if (tile_rows(B, n, H, W) < 0) return DPF_ERR_UNSUPPORTED;
  g.pred = pred, g.yref = luma, g.ytgt = luma + (size_t)B * H * W, g.ab = ab, g.mask = mask;
  g.n = n, g.H = H, g.W = W, g.target_type = target_type, g.sx = shift_x, g.sy = shift_y, g.alpha = alpha, g.eps = eps;
  dpf_fill_head_weights(hw.w, weights, n);
  return DPF_OK;
}

int prepare_smooth(const float* pred, const float* guide_rgb, const float* mask, int B, int n, int H, int W, float gamma, float eps,
                   const float* norm_host, const float* weights, const float* luma, Smooth& g, DpfHeadW& hw) {
  if (!pred || !guide_rgb || !norm_host || !weights || !luma || !shape_ok(B, n, H, W) || !(gamma >= 0.f) || !isfinite(gamma) || !(eps > 0.f) ||
      !isfinite(eps))
    return DPF_ERR_INVALID_ARG;
  if (tile_rows(B, n, H, W) < 0) return DPF_ERR_UNSUPPORTED;
  g.pred = pred, g.y = luma, g.mask = mask, g.n = n, g.H = H, g.W = W, g.gamma = gamma, g.eps = eps;
  dpf_fill_head_weights(hw.w, weights, n);
  return DPF_OK;
}

}  // namespace

extern "C" {

long long dpf_photometric_workspace_bytes(int B, int n, int H, int W) {
  const long long rows = tile_rows(B, n, H, W);
  return rows < 0 ? -1 : rows * 2 * (long long)sizeof(double);
}

long long dpf_smoothness_workspace_bytes(int B, int n, int H, int W) {
  const long long rows = tile_rows(B, n, H, W);
  return rows < 0 ? -1 : rows * 4 * (long long)sizeof(double);
}

int dpf_photometric_forward(const float* pred, const float* ref_rgb, const float* tgt_rgb, const float* ab, const float* mask, int B, int n,
                            int H, int W, int target_type, float shift_x, float shift_y, float alpha, float eps, const float* norm_host,
                            const float* head_weights_host, void* ws, long long ws_bytes, float* luma, double* stats, float* out,
                            float* warped_out, unsigned char* counted_out, void* stream) {
  dpf_clear_error();
  Photo g;
  DpfHeadW hw;
  const int rc = prepare_photo(pred, ref_rgb, tgt_rgb, ab, mask, B, n, H, W, target_type, shift_x, shift_y, alpha, eps, norm_host,
                               head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !out || (warped_out != nullptr) != (counted_out != nullptr) ||
      !dpf_ws_ok(ws, ws_bytes, dpf_photometric_workspace_bytes(B, n, H, W), 8))
    return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  launch_luma(ref_rgb, tgt_rgb, B, 2 * B, (long long)H * W, dpf_norm_of(norm_host), luma, st);
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  double* part = (double*)ws;
  hipLaunchKernelGGL(photo_forward_kernel, grid, block, 0, st, g, part, warped_out, counted_out);
  dpf_launch_head_fold<1>(part, B, n, H, W, hw, stats, out, st);
  return dpf_check_launch();
}

int dpf_photometric_backward(const float* pred, const float* ref_rgb, const float* tgt_rgb, const float* ab, const float* mask, int B, int n,
                             int H, int W, int target_type, float shift_x, float shift_y, float alpha, float eps, const float* norm_host,
                             const float* head_weights_host, const float* luma, const double* stats, const float* gout, float* dpred,
                             void* stream) {
  dpf_clear_error();
  Photo g;
  DpfHeadW hw;
  const int rc = prepare_photo(pred, ref_rgb, tgt_rgb, ab, mask, B, n, H, W, target_type, shift_x, shift_y, alpha, eps, norm_host,
                               head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !gout || !dpred) return DPF_ERR_INVALID_ARG;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  hipLaunchKernelGGL(photo_backward_kernel, grid, block, 0, (hipStream_t)stream, g, hw, stats, gout, dpred);
  return dpf_check_launch();
}

int dpf_smoothness_forward(const float* pred, const float* guide_rgb, const float* mask, int B, int n, int H, int W, float gamma, float eps,
                           const float* norm_host, const float* head_weights_host, void* ws, long long ws_bytes, float* luma, double* stats,
                           float* out, void* stream) {
  dpf_clear_error();
  Smooth g;
  DpfHeadW hw;
  const int rc = prepare_smooth(pred, guide_rgb, mask, B, n, H, W, gamma, eps, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !out || !dpf_ws_ok(ws, ws_bytes, dpf_smoothness_workspace_bytes(B, n, H, W), 8)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  launch_luma(guide_rgb, guide_rgb, B, B, (long long)H * W, dpf_norm_of(norm_host), luma, st);
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  double* part = (double*)ws;
  hipLaunchKernelGGL(smooth_forward_kernel, grid, block, 0, st, g, part);
  dpf_launch_head_fold<2>(part, B, n, H, W, hw, stats, out, st);
  return dpf_check_launch();
}

int dpf_smoothness_backward(const float* pred, const float* guide_rgb, const float* mask, int B, int n, int H, int W, float gamma, float eps,
                            const float* norm_host, const float* head_weights_host, const float* luma, const double* stats,
                            const float* gout, float* dpred, void* stream) {
  dpf_clear_error();
  Smooth g;
  DpfHeadW hw;
  const int rc = prepare_smooth(pred, guide_rgb, mask, B, n, H, W, gamma, eps, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !gout || !dpred) return DPF_ERR_INVALID_ARG;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  hipLaunchKernelGGL(smooth_backward_kernel, grid, block, 0, (hipStream_t)stream, g, hw, stats, gout, dpred);
  return dpf_check_launch();
}

}  // extern "C"
