// Confidence maps and a modal estimate from the hypothesis distribution of the disparity heads (ops.head_confidence, ops.confidence_curve;
// dualpixelface_amd/confidence.py; not in the reference).  Like unimodal.hip, no [B, n, L, H, W] volume is read or
// written: the distribution of a pixel is recomputed from the low-resolution logits with the head's own arithmetic (dpf_softargmin.h).
// Every fp32 expression is written operation by operation under -ffp-contract=off, so that tests/confidence_cpu.py restates it.
//
// Per head and pixel, every sum in ascending l, in fp32:
//   u_l, mx   the trilinear upsample of the head's logits and its maximum, exactly as in unimodal.hip (Pixel<FAST>)
//   x_l       u_l - mx;  e_l = __expf(x_l);  S = sum e_l;  p_l = e_l / S
//   l*        the smallest l with u_l == mx (0 where no l has: every u_l is NaN).  The half-pixel geometry has exact ties u_0 == u_1
//   peak      1 / S (e_{l*} is exactly 1)
//   Hent      logf(S) - sum p_l x_l;  entropy = 1 - Hent / logf((float)L), clamped to [0, 1]
//   mu        sum p_l d_l, the soft-argmin's value in the order of unimodal.hip's expect_out
//   var       sum p_l ((d_l - mu) (d_l - mu));  spread = sqrtf(var)
//   M, modal  lo = max(0, l* - r), hi = min(L - 1, l* + r);  M = sum_{lo..hi} p_l;  mass = fminf(M, 1);
//             modal = (sum_{lo..hi} p_l d_l) / M, safe because M >= 1 / S > 0
//   bad       any of S, Hent, var, modal not finite: peak = entropy = mass = 0, spread = modal = NaN
//
// head_confidence_kernel: one launch under dpf_tile_grid(B, n, H, W), one pixel per thread of a 32 x 8 tile, no workspace, no atomics.
// FAST (D = 8, L = 32, align_corners) unrolls every loop over the hypotheses and keeps e_l in registers; the window sums are predicated
// on |l - l*| <= r, so no register array is indexed at run time.  The general path keeps rolled loops and forms u_l and e_l again in each.
//
// The sparsification table (dpf_confidence_curve): curve[bins][2] of fp64 = (count, sum |pred - t|) per confidence bin over the pixels
// with mask on and t, pred, conf finite; bin = (int) min(bins - 1, max(0, conf bins)).  A workgroup walks kCurveChunks chunks of 256
// consecutive pixels of one sample: each chunk's (bin, err) goes to LDS, thread k < bins adds the entries of bin k in pixel order (all
// active threads read one LDS address: a broadcast), and the workgroup leaves one row of 2 bins doubles.  One workgroup per table entry
// folds the rows in the order of dpf_reduce.h.  No atomics and every order fixed: the same bits on every call.
#include "dpf_head_loss.h"
#include "dpf_softargmin.h"
#include <math.h>

extern "C" long long dpf_confidence_curve_workspace_bytes(int B, int H, int W, int bins);

namespace {

constexpr int kBlock = 256;
constexpr int kTW = kDpfTileW, kTH = kDpfTileH;
constexpr int kMaxWindow = 32;
constexpr int kMaxBins = 64;
constexpr int kCurveChunks = 8;                    // chunks of 256 pixels per workgroup of the curve pass
constexpr long long kCurveMaxRows = 1 << 24;

struct Conf {
  const float* k[kDpfMaxHeads];   // the logits of each head, [B, 1, D, h, w]
  int n;
  int r;                          // window radius
  HeadP p;                        // B, D, h, w, L, H, W, off, disp
};

struct ConfOut {
  float *peak, *entropy, *mass, *spread, *modal;   // [B, n, H, W] or NULL each
  int* lstar;
};

// grid dpf_tile_grid(B, n, H, W), 256 threads = 8 rows x 32 columns
template <bool FAST>
__global__ __launch_bounds__(256) void head_confidence_kernel(Conf g, ConfOut out) {
  const HeadP& p = g.p;
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)p.H * p.W;
  const int X = blockIdx.x * kTW + (t & (kTW - 1)), Y = blockIdx.y * kTH + t / kTW;
  if (X >= p.W || Y >= p.H) return;                       // (no barrier below)
  const size_t oo = ((size_t)s * g.n + h) * HW + (size_t)Y * p.W + X;
  const float rd = head_ratio(p.D, p.L, p.off), ry = head_ratio(p.h, p.H, p.off), rx = head_ratio(p.w, p.W, p.off);
  int y0, y1, x0, x1;
  float ly, lx;
  ac_src(Y, ry, p.h, y0, y1, ly, p.off);
  ac_src(X, rx, p.w, x0, x1, lx, p.off);
  Pixel<FAST> px;
  const float mx = px.upsample(g.k[h], p, s, rd, y0, y1, x0, x1, ly, lx);
  const int r = g.r;
  float S = 0.f, cross = 0.f, mu = 0.f, M = 0.f, N = 0.f, var = 0.f;
  int ls = -1;
  if (FAST) {
    float e[MAXL];
    UNI_FOR_L(l) {
      e[l] = __expf(px.u[l] - mx);
      S = S + e[l];
    }
#pragma unroll
    for (int l = MAXL - 1; l >= 0; --l) ls = px.u[l] == mx ? l : ls;      // the smallest l wins
    ls = max(ls, 0);
    UNI_FOR_L(l) {
      const float pl = e[l] / S;
      e[l] = pl;                                          // (p_l from here on)
      cross = cross + pl * (px.u[l] - mx);
      mu = mu + pl * p.disp[l];
      if (abs(l - ls) <= r) {
        M = M + pl;
        N = N + pl * p.disp[l];
      }
    }
    UNI_FOR_L(l) {
      const float dm = p.disp[l] - mu;
      var = var + e[l] * (dm * dm);
    }
  } else {
#pragma unroll 1
    for (int l = 0; l < p.L; ++l) {
      const float ul = px.logit(p, rd, l);
      S = S + __expf(ul - mx);
      ls = (ls < 0 && ul == mx) ? l : ls;
    }
    ls = max(ls, 0);
#pragma unroll 1
    for (int l = 0; l < p.L; ++l) {
      const float xl = px.logit(p, rd, l) - mx;
      const float pl = __expf(xl) / S;
      cross = cross + pl * xl;
      mu = mu + pl * p.disp[l];
      if (abs(l - ls) <= r) {
        M = M + pl;
        N = N + pl * p.disp[l];
      }
    }
#pragma unroll 1
    for (int l = 0; l < p.L; ++l) {
      const float dm = p.disp[l] - mu;
      var = var + (__expf((px.logit(p, rd, l) - mx)) / S) * (dm * dm);
    }
  }
  const float Hent = logf(S) - cross;
  const float modal = N / M;
  const bool bad = !(dpf_finite_f(S) && dpf_finite_f(Hent) && dpf_finite_f(var) && dpf_finite_f(modal));
  const float nan = __int_as_float(0x7fc00000);
  if (out.peak) out.peak[oo] = bad ? 0.f : 1.f / S;
  if (out.entropy) out.entropy[oo] = bad ? 0.f : fminf(fmaxf(1.f - Hent / logf((float)p.L), 0.f), 1.f);
  if (out.mass) out.mass[oo] = bad ? 0.f : fminf(M, 1.f);
  if (out.spread) out.spread[oo] = bad ? nan : sqrtf(var);
  if (out.modal) out.modal[oo] = bad ? nan : modal;
  if (out.lstar) out.lstar[oo] = ls;
}

struct Curve {
  const float *conf, *pred, *target, *mask, *ab;
  long long cbs, pbs;             // batch strides of conf and pred, in floats
  int HW, bins;
};

struct CurveEntry { int bin; float err; };   // bin -1: the pixel is left out

// grid (ceil(HW / (256 kCurveChunks)), B).  part: [B gridDim.x][2 bins]
__global__ __launch_bounds__(256) void curve_tile_kernel(Curve g, double* __restrict__ part) {
  __shared__ CurveEntry sm[kBlock];
  const int t = threadIdx.x, s = blockIdx.y;
  const float fb = (float)g.bins;
  double cnt = 0.0, sum = 0.0;
  const long long first = (long long)blockIdx.x * (kBlock * kCurveChunks);
  for (int c = 0; c < kCurveChunks; ++c) {
    const long long o = first + (long long)c * kBlock + t;
    CurveEntry en;
    en.bin = -1, en.err = 0.f;
    if (o < g.HW) {
      const size_t so = (size_t)s * g.HW + o;
      float tv = g.target[so];
      if (g.ab) {
        const float b = g.ab[2 * (size_t)s], a = g.ab[2 * (size_t)s + 1];
        tv = a / tv + b;
      }
      const float cf = g.conf[(size_t)s * g.cbs + o], pv = g.pred[(size_t)s * g.pbs + o];
      const bool on = !(g.mask && !(g.mask[so] > 0.f));
      if (on && dpf_finite_f(tv) && dpf_finite_f(pv) && dpf_finite_f(cf)) {
        en.bin = (int)fminf(fmaxf(cf * fb, 0.f), fb - 1.f);
        en.err = fabsf(pv - tv);
      }
    }
    __syncthreads();                 // the readers of the chunk before are done
    sm[t] = en;
    __syncthreads();
    if (t < g.bins) {
      for (int j = 0; j < kBlock; ++j) {
        const CurveEntry q = sm[j];
        if (q.bin == t) {
          cnt = cnt + 1.0;
          sum = sum + (double)q.err;
        }
      }
    }
  }
  if (t < g.bins) {
    double* row = part + ((size_t)s * gridDim.x + blockIdx.x) * 2 * (size_t)g.bins;
    row[2 * t] = cnt;
    row[2 * t + 1] = sum;
  }
}

// grid (2 bins): block k folds entry k of every row, in the order of dpf_fold_rows_d
__global__ __launch_bounds__(256) void curve_fold_kernel(const double* __restrict__ part, long long rows, int stride, int accumulate,
                                                         double* __restrict__ curve) {
  __shared__ double tot[1];
  dpf_fold_rows_d<1>(part + blockIdx.x, rows, stride, tot);
  if (threadIdx.x == 0) curve[blockIdx.x] = accumulate ? curve[blockIdx.x] + tot[0] : tot[0];
}

long long curve_rows(int B, int H, int W, int bins) {
  if (B <= 0 || H <= 0 || W <= 0 || bins < 1 || bins > kMaxBins || B > kDpfMaxGridZ || (long long)H * W > 0x7fffffffLL) return -1;
  const long long rows = (long long)B * dpf_div_up((long long)H * W, (long long)kBlock * kCurveChunks);
  return rows > kCurveMaxRows ? -1 : rows;
}

}  // namespace

extern "C" {

int dpf_head_confidence(const float* const* logits_host, int B, int n, int D, int h, int w, int L, int H, int W, int align_corners,
                        const float* disp_host, int window, float* peak, float* entropy, float* mass, float* spread, float* modal,
                        int* lstar, void* stream) {
  dpf_clear_error();
  if (!logits_host || !disp_host || n < 1 || n > kDpfMaxHeads || B <= 0 || D <= 0 || h <= 0 || w <= 0 || L <= 0 || H <= 0 || W <= 0 ||
      window < 0 || window > kMaxWindow || !(peak || entropy || mass || spread || modal || lstar))
    return DPF_ERR_INVALID_ARG;
  if (D > MAXD || L > MAXL || L < 2 || L % D != 0 || (long long)h * (L / D) != H || (long long)w * (L / D) != W) return DPF_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!logits_host[i]) return DPF_ERR_INVALID_ARG;
  for (int l = 0; l < L; ++l)
    if (!isfinite(disp_host[l]) || (l > 0 && !(disp_host[l] > disp_host[l - 1]))) return DPF_ERR_INVALID_ARG;
  if (dpf_tile_rows(B, n, H, W) < 0 || H > (1 << 24) || W > (1 << 24)) return DPF_ERR_UNSUPPORTED;     // (the limits of dpf_unimodal_forward)
  Conf g;
  for (int i = 0; i < kDpfMaxHeads; ++i) g.k[i] = i < n ? logits_host[i] : nullptr;
  g.n = n, g.r = window;
  g.p.B = B, g.p.D = D, g.p.h = h, g.p.w = w, g.p.L = L, g.p.H = H, g.p.W = W, g.p.pbs = 0, g.p.off = align_corners ? 0.f : 0.5f;
  for (int l = 0; l < MAXL; ++l) g.p.disp[l] = l < L ? disp_host[l] : 0.f;
  ConfOut out;
  out.peak = peak, out.entropy = entropy, out.mass = mass, out.spread = spread, out.modal = modal, out.lstar = lstar;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  if (D == 8 && L == 32 && align_corners)
    hipLaunchKernelGGL(head_confidence_kernel<true>, grid, block, 0, (hipStream_t)stream, g, out);
  else
    hipLaunchKernelGGL(head_confidence_kernel<false>, grid, block, 0, (hipStream_t)stream, g, out);
  return dpf_check_launch();
}

long long dpf_confidence_curve_workspace_bytes(int B, int H, int W, int bins) {
  const long long rows = curve_rows(B, H, W, bins);
  return rows < 0 ? -1 : rows * 2 * bins * (long long)sizeof(double);
}

int dpf_confidence_curve(const float* conf, long long conf_batch_stride, const float* pred, long long pred_batch_stride, const float* target,
                         const float* mask, const float* target_ab, int B, int H, int W, int bins, int accumulate, void* ws,
                         long long ws_bytes, double* curve, void* stream) {
  dpf_clear_error();
  if (!conf || !pred || !target || !curve || B <= 0 || H <= 0 || W <= 0 || bins < 1 || bins > kMaxBins) return DPF_ERR_INVALID_ARG;
  const long long rows = curve_rows(B, H, W, bins);
  if (rows < 0) return DPF_ERR_UNSUPPORTED;
  const long long HW = (long long)H * W;
  if (conf_batch_stride < HW || pred_batch_stride < HW || !dpf_ws_ok(ws, ws_bytes, dpf_confidence_curve_workspace_bytes(B, H, W, bins), 8))
    return DPF_ERR_INVALID_ARG;
  Curve g;
  g.conf = conf, g.pred = pred, g.target = target, g.mask = mask, g.ab = target_ab;
  g.cbs = conf_batch_stride, g.pbs = pred_batch_stride, g.HW = (int)HW, g.bins = bins;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  hipLaunchKernelGGL(curve_tile_kernel, dim3((unsigned)(rows / B), B), dim3(kBlock), 0, st, g, part);
  hipLaunchKernelGGL(curve_fold_kernel, dim3(2 * bins), dim3(kBlock), 0, st, part, rows, 2 * bins, accumulate ? 1 : 0, curve);
  return dpf_check_launch();
}

}  // extern "C"
