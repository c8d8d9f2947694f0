// The unimodal loss (loss_type 'unimodal'; losses.UNIMODALLoss, ops.unimodal_loss; not in the reference): the
// cross-entropy between the hypothesis distribution of every disparity head -- the softmax the soft-argmin takes its expectation of -- and
// a Laplace distribution over the hypotheses centred on the label.  Neither pass reads or writes a [B, n, L, H, W] volume: both recompute
// the distribution of a pixel from the low-resolution logits with the head's own arithmetic (dpf_softargmin.h).  Every fp32 expression is
// written operation by operation under -ffp-contract=off, so that tests/unimodal_cpu.py restates it.
//
//   u_l      the trilinear upsample of the head's logits k [B, 1, D, h, w] at (l, Y, X), l < L (pixel_logits / pixel_logits_8x32)
//   t        target, or a / target + b with target_ab [B, 2] = [b, a] (target is the depth map then)
//   counted  mask NULL or > 0, t finite, d_0 <= t <= d_{L-1}
//   P_l      e_l / Z, e_l = exp(-((|d_l - t| - m) / s)), m = min_j |d_j - t|, Z = the sum of e_l in the order of l
//   term     log(S) - sum_l P_l (u_l - mx), mx = max_j u_j, S = the sum of exp(u_l - mx) in the order of l
//   loss     sum_h w_h (sum of terms_h / count_h), 0 for a head with count_h = 0 (dpf_head_loss.h)
//   saved    log(S) of every pixel, [B, n, H, W], the caller's
//
// Forward: one workgroup per 32 x 8 tile of one head of one sample, one pixel per thread, leaves one row (term sum, count) of fp64 in the
// workspace; one workgroup folds the rows head by head.  Backward: d loss / d u_l = gout w_h / count_h (p_l - P_l) with p_l = exp((u_l - mx) - log(S))
// on the counted pixels, and d k is the adjoint of the upsample, as a GATHER: one thread per low-resolution cell (b, y, x) of a head walks
// the pixels (Y, X) whose ac_src taps name the cell, Y then X ascending -- membership is tested with ac_src itself, so the weights are the
// forward's bits -- forms per pixel the level adjoint db_d (l ascending, the first tap of a level before its second), and adds for the
// taps (y0, x0), (y0, x1), (y1, x0), (y1, x1) that name the cell, in that order, (wy wx) db_d.  At a clamped last row, column or level
// both taps name the same cell and both are added, as the scatter of softargmin.hip adds them.  No atomics, no workspace, one fixed
// order: the bits repeat whatever DPF_DETERMINISTIC says.  exp is __expf (v_exp_f32 of x log2(e), as in the soft-argmin), log is logf.
#include "dpf_head_loss.h"
#include "dpf_softargmin.h"
#include <math.h>

extern "C" long long dpf_unimodal_workspace_bytes(int B, int n, int H, int W);

namespace {

constexpr int kBlock = 256;
constexpr int kTW = kDpfTileW, kTH = kDpfTileH;      // one pixel (forward) or one low-resolution cell (backward) per thread

struct Uni {
  const float* k[kDpfMaxHeads];   // the logits of each head, [B, 1, D, h, w]
  const float* target;            // [B, H, W]
  const float* mask;              // [B, H, W] or NULL
  const float* ab;                // [B, 2] = [b, a] or NULL
  int n;
  float s;                        // Laplace scale
  float dlast;                    // d_{L-1}
  HeadP p;                        // B, D, h, w, L, H, W, off, disp
};

struct UniGrad { float* dk[kDpfMaxHeads]; };

// the label of pixel o of sample s -> counted
__device__ __forceinline__ bool label_at(const Uni& g, int s, size_t HW, size_t o, float& t) {
  t = g.target[(size_t)s * HW + o];
  if (g.ab) {
    const float b = g.ab[2 * (size_t)s], a = g.ab[2 * (size_t)s + 1];
    t = a / t + b;
  }
  if (g.mask && !(g.mask[(size_t)s * HW + o] > 0.f)) return false;
  return dpf_finite_f(t) && t >= g.p.disp[0] && t <= g.dlast;
}

// A wave-uniform value as a vector operand.  The backward's walk keeps the geometry live across three nested loops; as scalars those values
// exceed the scalar register file and the compiler parks them in vector-register lanes, as vector operands they cost one register each
__device__ __forceinline__ int as_vector(int v) {
  int r;
  asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(v));
  return r;
}
__device__ __forceinline__ float as_vector(float v) { return __int_as_float(as_vector(__float_as_int(v))); }

// e_l = exp(-((|d_l - t| - m) / s))
__device__ __forceinline__ float target_weight(float dl, float t, float m, float s) { return __expf(-((fabsf(dl - t) - m) / s)); }

// the output positions [a, b] that can hold a tap on input cell c (a superset: the walk tests each with ac_src).  fp32 with a margin of one
// position: good for out <= 2^24, which prepare() enforces
__device__ __forceinline__ void tap_span(int c, float ratio, int out, float off, int& a, int& b) {
  a = 0, b = out - 1;
  if (ratio > 0.f) {
    const float lo = ((float)(c - 1) + off) / ratio - off, hi = ((float)(c + 1) + off) / ratio - off;
    a = max(0, (int)fminf(floorf(lo), (float)out) - 1);
    b = min(out - 1, (int)fminf(ceilf(hi), (float)out) + 1);
  }
}

// (Pixel<FAST>, the work of one pixel for the shipped and for any other geometry, and UNI_FOR_L: dpf_softargmin.h)

// grid dpf_tile_grid(B, n, H, W), 256 threads = 8 rows x 32 columns.  part: [n][B tiles][2]
template <bool FAST>
__global__ __launch_bounds__(256) void uni_forward_kernel(Uni g, double* __restrict__ part, float* __restrict__ logsum_out,
                                                          unsigned char* __restrict__ counted_out, float* __restrict__ expect_out) {
  const HeadP& p = g.p;
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)p.H * p.W;
  const int X = blockIdx.x * kTW + (t & (kTW - 1)), Y = blockIdx.y * kTH + t / kTW;
  double acc[2] = {0.0, 0.0};
  if (X < p.W && Y < p.H) {
    const size_t o = (size_t)Y * p.W + X, oo = ((size_t)s * g.n + h) * HW + o;
    const float rd = head_ratio(p.D, p.L, p.off), ry = head_ratio(p.h, p.H, p.off), rx = head_ratio(p.w, p.W, p.off);
    int y0, y1, x0, x1;
    float ly, lx;
    ac_src(Y, ry, p.h, y0, y1, ly, p.off);
    ac_src(X, rx, p.w, x0, x1, lx, p.off);
    Pixel<FAST> px;
    const float mx = px.upsample(g.k[h], p, s, rd, y0, y1, x0, x1, ly, lx);
    float tv;
    const bool counted = label_at(g, s, HW, o, tv);
    float S = 0.f, m = 3.4e38f, Z = 0.f, cross = 0.f, ex = 0.f;
    if (FAST) {
      UNI_FOR_L(l) S = S + __expf(px.u[l] - mx);
      UNI_FOR_L(l) m = fminf(m, fabsf(p.disp[l] - tv));
    } else {
#pragma unroll 1
      for (int l = 0; l < p.L; ++l) {
        S = S + __expf(px.logit(p, rd, l) - mx);
        m = fminf(m, fabsf(p.disp[l] - tv));
      }
    }
    const float lg = logf(S);
    logsum_out[oo] = lg;
    if (counted) {
      if (FAST) {
        float e[MAXL];
        UNI_FOR_L(l) {
          e[l] = target_weight(p.disp[l], tv, m, g.s);
          Z = Z + e[l];
        }
        UNI_FOR_L(l) cross = cross + (e[l] / Z) * (px.u[l] - mx);
      } else {
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) Z = Z + target_weight(p.disp[l], tv, m, g.s);
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) cross = cross + (target_weight(p.disp[l], tv, m, g.s) / Z) * (px.logit(p, rd, l) - mx);
      }
      acc[0] = (double)(lg - cross);
      acc[1] = 1.0;
    }
    if (expect_out) {                  // the soft-argmin's value, in its expression order
      if (FAST) {
        UNI_FOR_L(l) ex = ex + (__expf(px.u[l] - mx) / S) * p.disp[l];
      } else {
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) ex = ex + (__expf(px.logit(p, rd, l) - mx) / S) * p.disp[l];
      }
      expect_out[oo] = ex;
      counted_out[oo] = counted ? 1 : 0;
    }
  }
  dpf_block_reduce_d<2>(acc, part + dpf_tile_part_row(s, h, g.n) * 2);
}

// grid dpf_tile_grid(B, n, h, w): one thread per low-resolution cell of a head of a sample, all D levels of it
template <bool FAST>
__global__ __launch_bounds__(256) void uni_backward_kernel(Uni g, DpfHeadW hw, const float* __restrict__ logsum, const double* __restrict__ stats,
                                                           const float* __restrict__ gout, UniGrad out) {
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const int x = blockIdx.x * kTW + (t & (kTW - 1)), y = blockIdx.y * kTH + t / kTW;
  __shared__ float disp[MAXL];                            // the hypothesis values as vector operands: 32 scalar registers less to hold
  if (t < MAXL) disp[t] = g.p.disp[t];
  __syncthreads();
  HeadP p;                                                // the geometry as vector operands (disp stays in LDS)
  p.B = g.p.B, p.D = as_vector(g.p.D), p.h = as_vector(g.p.h), p.w = as_vector(g.p.w), p.L = as_vector(g.p.L), p.H = as_vector(g.p.H);
  p.W = as_vector(g.p.W), p.pbs = 0, p.off = as_vector(g.p.off);
  if (x >= p.w || y >= p.h) return;                       // (no barrier below)
  const size_t HW = (size_t)p.H * p.W;
  const float* __restrict__ k = g.k[h];
  const float* __restrict__ lgh = logsum + ((size_t)s * g.n + h) * HW;
  const float rd = head_ratio(p.D, p.L, p.off), ry = head_ratio(p.h, p.H, p.off), rx = head_ratio(p.w, p.W, p.off);
  int Ya, Yb, Xa, Xb;
  tap_span(y, ry, p.H, p.off, Ya, Yb);
  tap_span(x, rx, p.W, p.off, Xa, Xb);
  float acc[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) acc[d] = 0.f;
  for (int Y = Ya; Y <= Yb; ++Y) {
    int y0, y1, x0, x1;
    float ly, lx;
    ac_src(Y, ry, p.h, y0, y1, ly, p.off);
    // the weight of each tap on this cell, 0 where the tap names another: adding (0 w) db changes no bit of a finite sum
    const float wa = y0 == y ? 1.f - ly : 0.f, wb = y1 == y ? ly : 0.f;
    if (y0 != y && y1 != y) continue;
    for (int X = Xa; X <= Xb; ++X) {
      ac_src(X, rx, p.w, x0, x1, lx, p.off);
      const float va = x0 == x ? 1.f - lx : 0.f, vb = x1 == x ? lx : 0.f;
      const size_t o = (size_t)Y * p.W + X;
      float tv;
      if ((x0 != x && x1 != x) || !label_at(g, s, HW, o, tv)) continue;
      Pixel<FAST> px;
      const float mx = px.upsample(k, p, s, rd, y0, y1, x0, x1, ly, lx);
      const float lg = lgh[o];
      float m = 3.4e38f, Z = 0.f;
      float db[MAXD];
#pragma unroll
      for (int d = 0; d < MAXD; ++d) db[d] = 0.f;
      if (FAST) {
        float e[MAXL];
        UNI_FOR_L(l) m = fminf(m, fabsf(disp[l] - tv));
        UNI_FOR_L(l) {
          e[l] = target_weight(disp[l], tv, m, g.s);
          Z = Z + e[l];
        }
        UNI_FOR_L(l) {
          const float gl = __expf((px.u[l] - mx) - lg) - e[l] / Z;
          int d0, d1;
          float ld;
          level_taps_8x32(l, d0, d1, ld);
          db[d0] = db[d0] + (1.f - ld) * gl;             // the first tap of a level before its second
          db[d1] = db[d1] + ld * gl;
        }
      } else {
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) m = fminf(m, fabsf(disp[l] - tv));
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) Z = Z + target_weight(disp[l], tv, m, g.s);
#pragma unroll 1
        for (int l = 0; l < p.L; ++l) {
          int d0, d1;
          float ld;
          ac_src(l, rd, p.D, d0, d1, ld, p.off);
          const float gl = __expf((level_value(px.bl, d0, d1, ld) - mx) - lg) - target_weight(disp[l], tv, m, g.s) / Z;
          const float g0 = (1.f - ld) * gl, g1 = ld * gl;
#pragma unroll
          for (int d = 0; d < MAXD; ++d) {                // register-resident select, the first tap before the second
            if (d == d0) db[d] = db[d] + g0;
            if (d == d1) db[d] = db[d] + g1;
          }
        }
      }
#pragma unroll
      for (int d = 0; d < MAXD; ++d) {
        const float v = db[d];
        acc[d] = acc[d] + (wa * va) * v;
        acc[d] = acc[d] + (wa * vb) * v;
        acc[d] = acc[d] + (wb * va) * v;
        acc[d] = acc[d] + (wb * vb) * v;
      }
    }
  }
  const double cnt = stats[h];
  const float wk = cnt > 0.0 ? (float)((double)hw.w[h] / cnt) : 0.f;
  const float sc = wk * gout[0];
  float* __restrict__ dk = out.dk[h] + (size_t)s * p.D * p.h * p.w + (size_t)y * p.w + x;
#pragma unroll
  for (int d = 0; d < MAXD; ++d)
    if (d < p.D) dk[(size_t)d * p.h * p.w] = acc[d] * sc;
}

// argument checks shared by the entry points; fills g and hw
int prepare(const float* const* logits_host, const float* target, const float* mask, const float* ab, int B, int n, int D, int h, int w, int L,
            int H, int W, int align_corners, const float* disp_host, float laplace_scale, const float* weights, Uni& g, DpfHeadW& hw) {
  if (!logits_host || !target || !disp_host || !weights || n < 1 || n > kDpfMaxHeads || B <= 0 || D <= 0 || h <= 0 || w <= 0 || L <= 0 ||
      H <= 0 || W <= 0 || !(laplace_scale > 0.f) || !isfinite(laplace_scale))
    return DPF_ERR_INVALID_ARG;
  if (D > MAXD || L > MAXL || L % D != 0 || (long long)h * (L / D) != H || (long long)w * (L / D) != W) return DPF_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!logits_host[i]) return DPF_ERR_INVALID_ARG;
  for (int l = 0; l < L; ++l)
    if (!isfinite(disp_host[l]) || (l > 0 && !(disp_host[l] > disp_host[l - 1]))) return DPF_ERR_INVALID_ARG;
  // (the backward's walk bounds its span in fp32, tap_span: exact positions up to 2^24)
  if (dpf_tile_rows(B, n, H, W) < 0 || H > (1 << 24) || W > (1 << 24)) return DPF_ERR_UNSUPPORTED;
  for (int i = 0; i < kDpfMaxHeads; ++i) g.k[i] = i < n ? logits_host[i] : nullptr;
  g.target = target, g.mask = mask, g.ab = ab, g.n = n, g.s = laplace_scale, g.dlast = disp_host[L - 1];
  g.p.B = B, g.p.D = D, g.p.h = h, g.p.w = w, g.p.L = L, g.p.H = H, g.p.W = W, g.p.pbs = 0, g.p.off = align_corners ? 0.f : 0.5f;
  for (int l = 0; l < MAXL; ++l) g.p.disp[l] = l < L ? disp_host[l] : 0.f;
  dpf_fill_head_weights(hw.w, weights, n);
  return DPF_OK;
}

bool fast_geometry(const Uni& g) { return g.p.D == 8 && g.p.L == 32 && g.p.off == 0.f; }

}  // namespace

extern "C" {

long long dpf_unimodal_workspace_bytes(int B, int n, int H, int W) {
  const long long rows = dpf_tile_rows(B, n, H, W);
  return rows < 0 ? -1 : rows * 2 * (long long)sizeof(double);
}

int dpf_unimodal_forward(const float* const* logits_host, const float* target, const float* mask, const float* target_ab, int B, int n, int D,
                         int h, int w, int L, int H, int W, int align_corners, const float* disp_host, float laplace_scale,
                         const float* head_weights_host, void* ws, long long ws_bytes, float* logsum, double* stats, float* out,
                         unsigned char* counted_out, float* expect_out, void* stream) {
  dpf_clear_error();
  Uni g;
  DpfHeadW hw;
  const int rc = prepare(logits_host, target, mask, target_ab, B, n, D, h, w, L, H, W, align_corners, disp_host, laplace_scale,
                         head_weights_host, g, hw);
  if (rc != DPF_OK) return rc;
  if (!logsum || !stats || !out || (counted_out != nullptr) != (expect_out != nullptr) ||
      !dpf_ws_ok(ws, ws_bytes, dpf_unimodal_workspace_bytes(B, n, H, W), 8))
    return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  double* part = (double*)ws;
  if (fast_geometry(g))
    hipLaunchKernelGGL(uni_forward_kernel<true>, grid, block, 0, st, g, part, logsum, counted_out, expect_out);
  else
    hipLaunchKernelGGL(uni_forward_kernel<false>, grid, block, 0, st, g, part, logsum, counted_out, expect_out);
  dpf_launch_head_fold<1>(part, B, n, H, W, hw, stats, out, st);
  return dpf_check_launch();
}

int dpf_unimodal_backward(const float* const* logits_host, const float* target, const float* mask, const float* target_ab, int B, int n, int D,
                          int h, int w, int L, int H, int W, int align_corners, const float* disp_host, float laplace_scale,
                          const float* head_weights_host, const float* logsum, const double* stats, const float* gout,
                          float* const* dlogits_host, void* stream) {
  dpf_clear_error();
  Uni g;
  DpfHeadW hw;
  const int rc = prepare(logits_host, target, mask, target_ab, B, n, D, h, w, L, H, W, align_corners, disp_host, laplace_scale,
                         head_weights_host, g, hw);
  if (rc != DPF_OK) return rc;
  if (!logsum || !stats || !gout || !dlogits_host) return DPF_ERR_INVALID_ARG;
  UniGrad dk;
  for (int i = 0; i < kDpfMaxHeads; ++i) {
    dk.dk[i] = i < n ? dlogits_host[i] : nullptr;
    if (i < n && !dk.dk[i]) return DPF_ERR_INVALID_ARG;
  }
  const dim3 grid = dpf_tile_grid(B, n, h, w), block(kBlock);
  if (fast_geometry(g))
    hipLaunchKernelGGL(uni_backward_kernel<true>, grid, block, 0, (hipStream_t)stream, g, hw, logsum, stats, gout, dk);
  else
    hipLaunchKernelGGL(uni_backward_kernel<false>, grid, block, 0, (hipStream_t)stream, g, hw, logsum, stats, gout, dk);
  return dpf_check_launch();
}

}  // extern "C"
