// The multi-view photometric loss (loss_type 'multiview'; losses.MULTIVIEWLoss, ops.multiview_loss): the centre
// image of each neighbouring camera warped into the target view through the predicted depth, K and P, and compared with the target image
// by 3 x 3 SSIM (dpf_window.h) and Barron's general robust loss, with a hand-written gradient into the prediction.  It stands where the
// reference has src/loss/depth/folded.py, which cannot run.  Every fp32 expression is written operation by operation under
// -ffp-contract=off, so that tests/multiview_cpu.py restates the rig, the sample coordinates, the warped values and the counted map bit
// for bit.
//
//   rig      per sample s and view v, in fp64, rounded to twelve fp32 numbers: T = Ps[s, v] P[s]^-1 (the adjugate inverse: general, no
//            assumption of a rigid pose), M = (Ks[s, v] T[:3, :3]) K[s]^-1, t = Ks[s, v] T[:3, 3]; products sum from the left
//   Y        the luminance of dpf_image.h, of the target image and of the S source images
//   z        pred (target type 'depth', 2), 1 / pred ('idepth', 1), a / (pred - b) ('disp', 0; ab = [b, a])
//   usable   pred finite, z finite and >= min_depth, mask NULL or > 0
//   sample   m = M [x, y, 1] = ((M_0 x + M_1 y) + M_2, ...), q = z m + t; warpable: q_z > 0, u = q_x / q_z, v = q_y / q_z,
//            0 <= u <= Ws - 1, 0 <= v <= Hs - 1 (the source image is Hs x Ws; pixel centres at integers; nothing outside is sampled)
//   J        the bilinear sample of photometric.hip: x0 = floor(u), fx = u - x0, x1 = min(x0 + 1, Ws - 1), likewise in y;
//            top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), J = top + fy (bot - top); 0 where not warpable
//   counted  the 3 x 3 window lies in the image and its nine pixels are warpable
//   term     weight_ssim clamp((1 - SSIM) / 2, 0, 1) + (1 - weight_ssim) rho(J - I; alpha, scale) at the centre; rho is the exact branch
//            set of folded.py::CharbonnierLoss with s = (d / scale)^2: alpha = 2: s / 2; alpha = 0: log1p(s / 2); otherwise
//            (beta / alpha') ((s / beta + 1)^(alpha / 2) - 1), beta = max(eps32, |alpha - 2|), alpha' = sign(alpha) max(eps32, |alpha|);
//            alpha = 1 takes sqrtf(s + 1) - 1, the same expression
//   loss     sum_h w_h mean over the views v with count_hv > 0 of (sum terms_hv / count_hv); 0 for a head no view of which counts
//
// Forward: one luminance launch over the B + B S planes, one workgroup per 32 x 8 tile of one (sample, head, view) (I, J and the warpable
// flag in LDS with a halo of 1) leaves one row (term sum, count) of fp64 in the workspace, part [n][S][B tiles][2], and one workgroup
// folds the rows (head, view) by (head, view) (dpf_reduce.h).  Backward: a gather, one workgroup per tile of one (sample, head), the view
// loop inside: per view the tile is warped with a halo of 2, the windows of the tile and a halo of 1 leave the five numbers of
// dpf_window.h::window_coef, every pixel adds what the nine windows through it owe it in row-major order, then the robust term of its
// own window, times d J / d z = g_x (m_x q_z - q_x m_z) / q_z^2 + g_y (m_y q_z - q_y m_z) / q_z^2 of its bilinear sample and the view's
// share w_h / (views counted_h count_hv); the views add up in their order, and d z / d pred (1, -1 / pred^2, -a / (pred - b)^2) and gout
// multiply the sum.  No atomics and no scratch: the bits repeat.
//
// Occlusion handling (dpf_multiview_occ_*, dpf_multiview_zbuffer; ops.multiview_loss(reduce=, visibility=); off in the entry points above):
//   zbuffer  visibility 'zbuffer': per (sample, head, view) Hc x Wc cells of cell x cell source pixels, each the smallest q_z any warpable
//            pixel splats into it (an integer atomicMin on the bits of the positive float: whatever the order of arrival, the same bits);
//            visible: q_z <= zmin + tolerance * zmin of the pixel's own cell; seen = warpable and visible stands for warpable in `counted`
//   min      reduce 'min': per head and pixel the smallest term over the views that count it, the lowest view at a tie; loss =
//            sum_h w_h (sum of those terms / count_h), count_h the pixels some view counts
// Fill and splat are launches of their own ahead of the tile kernel (a cell's minimum comes from pixels anywhere in the image).  The
// tile kernels are the ones above as templates: forward_tile<kVis>, backward_tile<kVis, kMin> (the plain kernels are the <false>
// instances), and for 'min' a forward with the view loop inside that writes the selection plane the backward reads with a halo of 1.
#include "dpf_head_loss.h"
#include "dpf_image.h"
#include "dpf_window.h"
#include <math.h>

extern "C" long long dpf_multiview_workspace_bytes(int B, int n, int S, int H, int W);

namespace {

constexpr int kBlock = 256;
constexpr int kTW = kDpfTileW, kTH = kDpfTileH;
constexpr int kMaxViews = 8;
constexpr int kStatCount = 0, kStatSum = 64, kStatViews = 128;      // stats: count[h][v], sum[h][v], views counted[h]: 136 doubles

struct Rho {
  int mode;                // 0: alpha = 2, 1: alpha = 0, 2: alpha = 1, 3: the general form
  float scale, alpha, beta, lead, dlead;      // lead = beta / alpha', dlead = alpha / alpha'
};

struct MV {
  const float* pred;       // [B, n, H, W]
  const float* ytgt;       // [B, H, W]        luminance of the target view
  const float* ysrc;       // [B, S, Hs, Ws]   luminance of the source views
  const float* rig;        // [B, S, 12]       M row-major, then t
  const float* ab;         // [B, 2] or NULL (types 1, 2)
  const float* mask;       // [B, H, W] or NULL
  int n, S, H, W, Hs, Ws, target_type;
  float wssim, min_depth;
  Rho rho;
};

struct Rig { float m[9], t[3]; };

__device__ __forceinline__ float rho_of(const Rho& r, float d) {
  const float xs = d / r.scale;
  const float s = xs * xs;
  if (r.mode == 2) return sqrtf(s + 1.f) - 1.f;
  if (r.mode == 0) return 0.5f * s;
  if (r.mode == 1) return log1pf(fminf(0.5f * s, 33e37f));
  return r.lead * (powf(s / r.beta + 1.f, 0.5f * r.alpha) - 1.f);
}

// d rho / d d
__device__ __forceinline__ float drho_of(const Rho& r, float d) {
  const float xs = d / r.scale;
  const float s = xs * xs;
  const float g = xs / r.scale;
  if (r.mode == 2) return g / sqrtf(s + 1.f);
  if (r.mode == 0) return g;
  if (r.mode == 1) return g / (0.5f * s + 1.f);
  return (r.dlead * g) * powf(s / r.beta + 1.f, 0.5f * r.alpha - 1.f);
}

// grid (blocks over the larger plane, B + B S planes): plane p < B is the target image p [3][HW], plane B + k the source image k of
// src [B][S][3][HsWs] (samples src_stride floats apart); out: [B][HW] then [B S][HsWs]
__global__ __launch_bounds__(256) void mv_luma_kernel(const float* __restrict__ tgt, const float* __restrict__ src, long long src_stride, int B,
                                                      int S, long long HW, long long HsWs, DpfNorm nm, float* __restrict__ out) {
  const int p = blockIdx.y;
  const float* __restrict__ g;
  float* __restrict__ o;
  long long N;
  if (p < B) {
    g = tgt + (size_t)p * 3 * HW, o = out + (size_t)p * HW, N = HW;
  } else {
    const int k = p - B, s = k / S, v = k - s * S;
    g = src + (size_t)s * src_stride + (size_t)v * 3 * HsWs, o = out + (size_t)B * HW + (size_t)k * HsWs, N = HsWs;
  }
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long long)gridDim.x * kBlock)
    o[i] = dpf_luma(g[i], g[i + N], g[i + 2 * N], nm);
}

// one thread per (sample, view); fp64, every product and sum as written
__global__ __launch_bounds__(64) void mv_rig_kernel(const float* __restrict__ K, const float* __restrict__ P, const float* __restrict__ Ks,
                                                    const float* __restrict__ Ps, int B, int S, float* __restrict__ rig) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * S) return;
  const int s = i / S;
  const float* __restrict__ p = P + (size_t)s * 16;
  const double a00 = p[0], a01 = p[1], a02 = p[2], a03 = p[3], a10 = p[4], a11 = p[5], a12 = p[6], a13 = p[7];
  const double a20 = p[8], a21 = p[9], a22 = p[10], a23 = p[11], a30 = p[12], a31 = p[13], a32 = p[14], a33 = p[15];
  const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03;
  const double s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
  const double c5 = a22 * a33 - a32 * a23, c4 = a21 * a33 - a31 * a23, c3 = a21 * a32 - a31 * a22;
  const double c2 = a20 * a33 - a30 * a23, c1 = a20 * a32 - a30 * a22, c0 = a20 * a31 - a30 * a21;
  const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
  double inv[4][4];
  inv[0][0] = ((a11 * c5 - a12 * c4) + a13 * c3) / det;
  inv[0][1] = ((a02 * c4 - a01 * c5) - a03 * c3) / det;
  inv[0][2] = ((a31 * s5 - a32 * s4) + a33 * s3) / det;
  inv[0][3] = ((a22 * s4 - a21 * s5) - a23 * s3) / det;
  inv[1][0] = ((a12 * c2 - a10 * c5) - a13 * c1) / det;
  inv[1][1] = ((a00 * c5 - a02 * c2) + a03 * c1) / det;
  inv[1][2] = ((a32 * s2 - a30 * s5) - a33 * s1) / det;
  inv[1][3] = ((a20 * s5 - a22 * s2) + a23 * s1) / det;
  inv[2][0] = ((a10 * c4 - a11 * c2) + a13 * c0) / det;
  inv[2][1] = ((a01 * c2 - a00 * c4) - a03 * c0) / det;
  inv[2][2] = ((a30 * s4 - a31 * s2) + a33 * s0) / det;
  inv[2][3] = ((a21 * s2 - a20 * s4) - a23 * s0) / det;
  inv[3][0] = ((a11 * c1 - a10 * c3) - a12 * c0) / det;
  inv[3][1] = ((a00 * c3 - a01 * c1) + a02 * c0) / det;
  inv[3][2] = ((a31 * s1 - a30 * s3) - a32 * s0) / det;
  inv[3][3] = ((a20 * s3 - a21 * s1) + a22 * s0) / det;
  const float* __restrict__ ps = Ps + (size_t)i * 16;
  double T[3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      T[r][c] = (((double)ps[4 * r] * inv[0][c] + (double)ps[4 * r + 1] * inv[1][c]) + (double)ps[4 * r + 2] * inv[2][c]) +
                (double)ps[4 * r + 3] * inv[3][c];
  const float* __restrict__ ks = Ks + (size_t)i * 9;
  double A[3][3], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = ((double)ks[3 * r] * T[0][c] + (double)ks[3 * r + 1] * T[1][c]) + (double)ks[3 * r + 2] * T[2][c];
    t[r] = ((double)ks[3 * r] * T[0][3] + (double)ks[3 * r + 1] * T[1][3]) + (double)ks[3 * r + 2] * T[2][3];
  }
  const float* __restrict__ k = K + (size_t)s * 9;
  const double k00 = k[0], k01 = k[1], k02 = k[2], k10 = k[3], k11 = k[4], k12 = k[5], k20 = k[6], k21 = k[7], k22 = k[8];
  const double d0 = k11 * k22 - k12 * k21, d1 = k12 * k20 - k10 * k22, d2 = k10 * k21 - k11 * k20;
  const double kdet = (k00 * d0 + k01 * d1) + k02 * d2;
  double ki[3][3];
  ki[0][0] = d0 / kdet, ki[0][1] = (k02 * k21 - k01 * k22) / kdet, ki[0][2] = (k01 * k12 - k02 * k11) / kdet;
  ki[1][0] = d1 / kdet, ki[1][1] = (k00 * k22 - k02 * k20) / kdet, ki[1][2] = (k02 * k10 - k00 * k12) / kdet;
  ki[2][0] = d2 / kdet, ki[2][1] = (k01 * k20 - k00 * k21) / kdet, ki[2][2] = (k00 * k11 - k01 * k10) / kdet;
  float* __restrict__ o = rig + (size_t)i * 12;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * r + c] = (float)((A[r][0] * ki[0][c] + A[r][1] * ki[1][c]) + A[r][2] * ki[2][c]);
    o[9 + r] = (float)t[r];
  }
}

__device__ __forceinline__ Rig load_rig(const MV& g, int s, int v) {
  Rig r;
  const float* __restrict__ p = g.rig + ((size_t)s * g.S + v) * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) r.m[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) r.t[k] = p[9 + k];
  return r;
}

// the depth of pixel o of one head, which lies in the image: -> usable; z, and where asked d z / d pred
__device__ __forceinline__ bool depth_at(const MV& g, const float* __restrict__ predh, size_t sbase, float a, float b, size_t o, float& z,
                                         float* dzdp) {
  z = 0.f;
  const float p = predh[o];
  if (!dpf_finite_f(p)) return false;
  if (g.mask && !(g.mask[sbase + o] > 0.f)) return false;
  float zz, dz;
  if (g.target_type == 2) {
    zz = p, dz = 1.f;
  } else if (g.target_type == 1) {
    zz = 1.f / p, dz = -(1.f / (p * p));
  } else {
    const float den = p - b;
    zz = a / den, dz = -(a / (den * den));
  }
  if (!dpf_finite_f(zz) || !(zz >= g.min_depth)) return false;
  z = zz;
  if (dzdp) *dzdp = dz;
  return true;
}

// the projection of the usable pixel (y, x) of depth z into a source view: -> warpable; m = M [x, y, 1], q = z m + t, the sample point
struct Proj { float mx, my, mz, qx, qy, qz, su, sv; };

__device__ __forceinline__ bool project_at(const MV& g, const Rig& r, float z, int y, int x, Proj& p) {
  const float xf = (float)x, yf = (float)y;
  p.mx = (r.m[0] * xf + r.m[1] * yf) + r.m[2];
  p.my = (r.m[3] * xf + r.m[4] * yf) + r.m[5];
  p.mz = (r.m[6] * xf + r.m[7] * yf) + r.m[8];
  p.qx = z * p.mx + r.t[0], p.qy = z * p.my + r.t[1], p.qz = z * p.mz + r.t[2];
  if (!(p.qz > 0.f)) return false;
  p.su = p.qx / p.qz, p.sv = p.qy / p.qz;
  return p.su >= 0.f && p.su <= (float)(g.Ws - 1) && p.sv >= 0.f && p.sv <= (float)(g.Hs - 1);
}

// the warp of the usable pixel (y, x) of depth z into the source plane ys: -> warpable; J, the sample point, where asked d J / d z and
// q_z (the occlusion modes compare it with the z-buffer)
__device__ __forceinline__ bool warp_at(const MV& g, const Rig& r, const float* __restrict__ ys, float z, int y, int x, float& J, float& u,
                                        float& v, float* dJdz, float* qz_out = nullptr) {
  J = 0.f, u = 0.f, v = 0.f;
  Proj p;
  if (!project_at(g, r, z, y, x, p)) return false;
  const float mx = p.mx, my = p.my, mz = p.mz, qx = p.qx, qy = p.qy, qz = p.qz, su = p.su, sv = p.sv;
  const float fx0 = floorf(su), fy0 = floorf(sv);
  const float fx = su - fx0, fy = sv - fy0;
  const int x0 = min((int)fx0, g.Ws - 1), y0 = min((int)fy0, g.Hs - 1);      // (the clamp acts only where Ws - 1 is no fp32 number)
  const int x1 = min(x0 + 1, g.Ws - 1), y1 = min(y0 + 1, g.Hs - 1);
  const float* __restrict__ r0 = ys + (size_t)y0 * g.Ws;
  const float* __restrict__ r1 = ys + (size_t)y1 * g.Ws;
  const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
  const float dt = v01 - v00, db = v11 - v10;
  const float top = v00 + fx * dt, bot = v10 + fx * db;
  const float dv = bot - top;
  J = top + fy * dv, u = su, v = sv;
  if (qz_out) *qz_out = qz;
  if (dJdz) {
    const float gx = dt + fy * (db - dt);
    const float qz2 = qz * qz;
    const float du = (mx * qz - qx * mz) / qz2, dw = (my * qz - qy * mz) / qz2;
    *dJdz = gx * du + dv * dw;
  }
  return true;
}

// ---- occlusion (visibility 'zbuffer'): one z-buffer of Hc x Wc cells per (sample, head, view), the bits of the smallest q_z splatted
// into each cell.  A warpable pixel is visible where q_z <= zmin + tolerance * zmin of its own cell, and "seen" = warpable and visible
// stands wherever the loss says warpable.  The buffer is the caller's: forward and backward read the same bits.
struct Occ {
  const unsigned* zbuf;    // [B, n, S, Hc, Wc], or NULL: visibility off
  int cell, Hc, Wc;
  float tol;
};

__device__ __forceinline__ size_t cell_of(const Occ& oc, float su, float sv) {
  const int cx = min(max((int)floorf(su + 0.5f) / oc.cell, 0), oc.Wc - 1);
  const int cy = min(max((int)floorf(sv + 0.5f) / oc.cell, 0), oc.Hc - 1);
  return (size_t)cy * oc.Wc + cx;
}

// zb: the z-buffer of this (sample, head, view)
__device__ __forceinline__ bool visible_at(const Occ& oc, const unsigned* __restrict__ zb, float qz, float su, float sv) {
  const float zmin = __uint_as_float(zb[cell_of(oc, su, sv)]);
  const float slack = oc.tol * zmin;
  return qz <= zmin + slack;
}

// grid (blocks, B n S): every cell to +infinity
__global__ __launch_bounds__(256) void mv_zfill_kernel(unsigned* __restrict__ zbuf, long long cells) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (long long)gridDim.x * kBlock) zbuf[i] = 0x7f800000u;
}

// grid (ceil(W / 32), ceil(H / 8), B n S): every warpable pixel splats q_z into its cell.  Positive floats order like their bit patterns,
// so the integer minimum is the float minimum whatever the order of arrival.
__global__ __launch_bounds__(256) void mv_zsplat_kernel(MV g, Occ oc, unsigned* __restrict__ zbuf) {
  const int sh = blockIdx.z / g.S, v = blockIdx.z - sh * g.S;
  const int s = sh / g.n, h = sh - s * g.n;
  const int x = blockIdx.x * kTW + (threadIdx.x & (kTW - 1)), y = blockIdx.y * kTH + threadIdx.x / kTW;
  if (x >= g.W || y >= g.H) return;
  const size_t HW = (size_t)g.H * g.W;
  const float b = g.target_type == 0 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 0 ? g.ab[2 * (size_t)s + 1] : 0.f;
  float z;
  if (!depth_at(g, g.pred + ((size_t)s * g.n + h) * HW, (size_t)s * HW, a, b, (size_t)y * g.W + x, z, nullptr)) return;
  Proj p;
  if (!project_at(g, load_rig(g, s, v), z, y, x, p)) return;
  atomicMin(zbuf + (size_t)blockIdx.z * ((size_t)oc.Hc * oc.Wc) + cell_of(oc, p.su, p.sv), __float_as_uint(p.qz));
}

// the tile of the forward kernels: I, J and the seen flag of view v in LDS with a halo of 1 (seen = warpable where kVis is false)
template <bool kVis>
__device__ __forceinline__ void load_view_tile(const MV& g, const Occ& oc, int s, int h, int v, const float* __restrict__ predh, float a, float b,
                                               int x0, int y0, float* __restrict__ tI, float* __restrict__ tJ, unsigned char* __restrict__ tw,
                                               float* __restrict__ xy_out) {
  constexpr int LW = kTW + 2, LH = kTH + 2;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const size_t shv = ((size_t)s * g.n + h) * g.S + v, obase = shv * HW;
  const float* __restrict__ yr = g.ytgt + sbase;
  const float* __restrict__ ys = g.ysrc + ((size_t)s * g.S + v) * ((size_t)g.Hs * g.Ws);
  const Rig r = load_rig(g, s, v);
  for (int i = threadIdx.x; i < LH * LW; i += kBlock) {
    const int ly = i / LW, lx = i - ly * LW;
    const int y = y0 - 1 + ly, x = x0 - 1 + lx;
    float I = 0.f, J = 0.f, su = 0.f, sv = 0.f;
    bool ok = false;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
      const size_t o = (size_t)y * g.W + x;
      I = yr[o];
      float z, qz = 0.f;
      ok = depth_at(g, predh, sbase, a, b, o, z, nullptr) && warp_at(g, r, ys, z, y, x, J, su, sv, nullptr, kVis ? &qz : nullptr);
      if (xy_out && ly >= 1 && ly <= kTH && lx >= 1 && lx <= kTW) {
        xy_out[2 * obase + o] = su;
        xy_out[2 * obase + HW + o] = sv;
      }
      if (kVis) ok = ok && visible_at(oc, oc.zbuf + shv * ((size_t)oc.Hc * oc.Wc), qz, su, sv);
    }
    tI[i] = I, tJ[i] = J, tw[i] = ok ? 1 : 0;
  }
}

// the term of the window whose centre is (ly, lx) of the forward tiles
__device__ __forceinline__ float term_at(const MV& g, const float* __restrict__ tI, const float* __restrict__ tJ, int ly, int lx) {
  constexpr int LW = kTW + 2;
  Window w;
  window_of<LW>(tI, tJ, ly, lx, w);
  const float ds = fminf(fmaxf((1.f - w.ssim) / 2.f, 0.f), 1.f);
  const float d = tJ[ly * LW + lx] - tI[ly * LW + lx];
  return g.wssim * ds + (1.f - g.wssim) * rho_of(g.rho, d);
}

// reduce 'min': grid (ceil(W / 32), ceil(H / 8), B n), the view loop inside.  Per pixel the smallest term over the views that count it
// (the lowest view wins a tie) and that view into sel (255: none).  part: [n][B tiles][kMinRow] = term sum, count, pixels won per view
constexpr int kMinRow = 2 + kMaxViews;

template <bool kVis>
__global__ __launch_bounds__(256) void mv_forward_min_kernel(MV g, Occ oc, double* __restrict__ part, unsigned char* __restrict__ sel,
                                                             float* __restrict__ warped_out, unsigned char* __restrict__ counted_out,
                                                             float* __restrict__ xy_out, unsigned char* __restrict__ visible_out) {
  constexpr int LW = kTW + 2, LH = kTH + 2;
  __shared__ float tI[LH * LW], tJ[LH * LW];
  __shared__ unsigned char tw[LH * LW];
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float b = g.target_type == 0 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 0 ? g.ab[2 * (size_t)s + 1] : 0.f;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty, ly = ty + 1, lx = tx + 1;
  const bool inside = x < g.W && y < g.H;
  float best = 0.f;
  int won = 255;
  for (int v = 0; v < g.S; ++v) {
    __syncthreads();                                       // the last view's readers are done
    load_view_tile<kVis>(g, oc, s, h, v, predh, a, b, x0, y0, tI, tJ, tw, xy_out);
    __syncthreads();
    if (inside) {
      const bool counted = x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && all_nine<LW>(tw, ly, lx);
      if (counted) {
        const float term = term_at(g, tI, tJ, ly, lx);
        if (won == 255 || term < best) best = term, won = v;
      }
      if (warped_out) {
        const size_t o = (((size_t)s * g.n + h) * g.S + v) * HW + (size_t)y * g.W + x;
        warped_out[o] = tJ[ly * LW + lx];
        counted_out[o] = counted ? 1 : 0;
        visible_out[o] = tw[ly * LW + lx];
      }
    }
  }
  double acc[kMinRow];
#pragma unroll
  for (int k = 0; k < kMinRow; ++k) acc[k] = 0.0;
  if (inside) {
    sel[((size_t)s * g.n + h) * HW + (size_t)y * g.W + x] = (unsigned char)won;
    if (won != 255) {
      acc[0] = (double)best, acc[1] = 1.0;
#pragma unroll
      for (int k = 0; k < kMaxViews; ++k) acc[2 + k] = won == k ? 1.0 : 0.0;
    }
  }
  dpf_block_reduce_d<kMinRow>(acc, part + dpf_tile_part_row(s, h, g.n) * kMinRow);
}

// one block: folds the rows of reduce 'min' head by head.  stats: the pixels view v won at [8 h + v], the term sum at [64 + 8 h], the
// pixels counted in some view at [128 + h]
__global__ __launch_bounds__(256) void mv_fold_min_kernel(const double* __restrict__ part, long long rows, int n, DpfHeadW hw,
                                                          double* __restrict__ stats, float* __restrict__ out) {
  __shared__ double tot[kMinRow];
  double loss = 0.0;
  for (int k = 0; k < kDpfMaxHeads; ++k) {
    double row[kMinRow];
#pragma unroll
    for (int q = 0; q < kMinRow; ++q) row[q] = 0.0;
    if (k < n) {
      dpf_fold_rows_d<kMinRow>(part + (size_t)k * (size_t)rows * kMinRow, rows, kMinRow, tot);
#pragma unroll
      for (int q = 0; q < kMinRow; ++q) row[q] = tot[q];
      if (row[1] > 0.0) loss += (double)hw.w[k] * (row[0] / row[1]);
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int v = 0; v < kMaxViews; ++v) stats[kStatCount + kMaxViews * k + v] = row[2 + v], stats[kStatSum + kMaxViews * k + v] = v == 0 ? row[0] : 0.0;
      stats[kStatViews + k] = row[1];
    }
  }
  if (threadIdx.x == 0) out[0] = (float)loss;
}

// reduce 'mean': grid (ceil(W / 32), ceil(H / 8), B n S), 256 threads = 8 rows x 32 columns.  part: [n][S][B tiles][2]
template <bool kVis>
__device__ __forceinline__ void forward_tile(const MV& g, const Occ& oc, double* __restrict__ part, float* __restrict__ warped_out,
                                             unsigned char* __restrict__ counted_out, float* __restrict__ xy_out,
                                             unsigned char* __restrict__ visible_out) {
  constexpr int LW = kTW + 2, LH = kTH + 2;
  __shared__ float tI[LH * LW], tJ[LH * LW];
  __shared__ unsigned char tw[LH * LW];
  const int t = threadIdx.x;
  const int sh = blockIdx.z / g.S, v = blockIdx.z - sh * g.S;
  const int s = sh / g.n, h = sh - s * g.n;
  const int B = gridDim.z / (g.n * g.S);
  const size_t HW = (size_t)g.H * g.W;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float b = g.target_type == 0 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 0 ? g.ab[2 * (size_t)s + 1] : 0.f;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const size_t obase = (((size_t)s * g.n + h) * g.S + v) * HW;
  load_view_tile<kVis>(g, oc, s, h, v, predh, a, b, x0, y0, tI, tJ, tw, xy_out);
  __syncthreads();
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  double acc[2] = {0.0, 0.0};
  if (x < g.W && y < g.H) {
    const int ly = ty + 1, lx = tx + 1;
    const bool counted = x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && all_nine<LW>(tw, ly, lx);
    if (counted) {
      acc[0] = (double)term_at(g, tI, tJ, ly, lx);
      acc[1] = 1.0;
    }
    if (warped_out) {
      const size_t o = obase + (size_t)y * g.W + x;
      warped_out[o] = tJ[ly * LW + lx];
      counted_out[o] = counted ? 1 : 0;
      if (kVis) visible_out[o] = tw[ly * LW + lx];
    }
  }
  const size_t tiles = (size_t)gridDim.x * gridDim.y;
  const size_t row = (((size_t)h * g.S + v) * B + s) * tiles + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  dpf_block_reduce_d<2>(acc, part + row * 2);
}

__global__ __launch_bounds__(256) void mv_forward_kernel(MV g, double* __restrict__ part, float* __restrict__ warped_out,
                                                         unsigned char* __restrict__ counted_out, float* __restrict__ xy_out) {
  forward_tile<false>(g, Occ{}, part, warped_out, counted_out, xy_out, nullptr);
}

__global__ __launch_bounds__(256) void mv_forward_vis_kernel(MV g, Occ oc, double* __restrict__ part, float* __restrict__ warped_out,
                                                             unsigned char* __restrict__ counted_out, float* __restrict__ xy_out,
                                                             unsigned char* __restrict__ visible_out) {
  forward_tile<true>(g, oc, part, warped_out, counted_out, xy_out, visible_out);
}

// one block: folds the rows (per head and view: B tiles) in a fixed order, writes the stats record and the loss
__global__ __launch_bounds__(256) void mv_fold_kernel(const double* __restrict__ part, long long rows, int n, int S, DpfHeadW hw,
                                                      double* __restrict__ stats, float* __restrict__ out) {
  __shared__ double tot[2];
  double loss = 0.0;
  for (int k = 0; k < kDpfMaxHeads; ++k) {
    double hsum = 0.0, views = 0.0;
    for (int v = 0; v < kMaxViews; ++v) {
      double sum = 0.0, cnt = 0.0;
      if (k < n && v < S) {
        dpf_fold_rows_d<2>(part + ((size_t)k * S + v) * (size_t)rows * 2, rows, 2, tot);
        sum = tot[0], cnt = tot[1];
        if (cnt > 0.0) hsum += sum / cnt, views += 1.0;
      }
      if (threadIdx.x == 0) stats[kStatCount + kMaxViews * k + v] = cnt, stats[kStatSum + kMaxViews * k + v] = sum;
    }
    if (views > 0.0) loss += (double)hw.w[k] * (hsum / views);
    if (threadIdx.x == 0) stats[kStatViews + k] = views;
  }
  if (threadIdx.x == 0) out[0] = (float)loss;
}

// grid (ceil(W / 32), ceil(H / 8), B n): the view loop runs inside, so a pixel's gradient is one sum in one order.  kVis: seen stands
// for warpable (the z-buffer is the forward's).  kMin: the window at centre c owes its nine pixels in view sel[c] only, the robust term of
// a pixel's own window is taken in its selected view only, and the share is w_h / count_h; stats is mv_fold_min_kernel's record
template <bool kVis, bool kMin>
__device__ __forceinline__ void backward_tile(const MV& g, const Occ& oc, const unsigned char* __restrict__ sel, const DpfHeadW& hw,
                                              const double* __restrict__ stats, const float* __restrict__ gout, float* __restrict__ dpred) {
  constexpr int ZW = kTW + 4, ZH = kTH + 4;               // I, z, J, warpable: halo 2
  constexpr int CW = kTW + 2, CH = kTH + 2;               // windows: halo 1
  __shared__ float tI[ZH * ZW], tZ[ZH * ZW], tJ[ZH * ZW];
  __shared__ unsigned char tu[ZH * ZW], tw[ZH * ZW];      // usable (per pixel), warpable (per pixel and view)
  __shared__ float coef[5][CH * CW];
  __shared__ unsigned char tsel[kMin ? CH * CW : 1];      // the selected view of the window centres
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const float* __restrict__ yr = g.ytgt + sbase;
  const float b = g.target_type == 0 ? g.ab[2 * (size_t)s] : 0.f, a = g.target_type == 0 ? g.ab[2 * (size_t)s + 1] : 0.f;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  if (kMin) {
    const unsigned char* __restrict__ selh = sel + ((size_t)s * g.n + h) * HW;
    for (int i = t; i < CH * CW; i += kBlock) {
      const int wy = i / CW, wx = i - wy * CW;
      const int py = y0 - 1 + wy, px = x0 - 1 + wx;
      tsel[i] = py >= 0 && py < g.H && px >= 0 && px < g.W ? selh[(size_t)py * g.W + px] : 255;
    }
  }
  for (int i = t; i < ZH * ZW; i += kBlock) {
    const int ly = i / ZW, lx = i - ly * ZW;
    const int y = y0 - 2 + ly, x = x0 - 2 + lx;
    float I = 0.f, z = 0.f;
    bool ok = false;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
      const size_t o = (size_t)y * g.W + x;
      I = yr[o];
      ok = depth_at(g, predh, sbase, a, b, o, z, nullptr);
    }
    tI[i] = I, tZ[i] = z, tu[i] = ok ? 1 : 0;
  }
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < g.W && y < g.H;
  const int ly = ty + 2, lx = tx + 2, cy = ty + 1, cx = tx + 1;
  const double views = stats[kStatViews + h];
  float total = 0.f;
  for (int v = 0; v < g.S; ++v) {
    const double cnt = stats[kStatCount + kMaxViews * h + v];
    if (!(cnt > 0.0)) continue;                            // (uniform over the block: a view that counts nothing owes nothing)
    const Rig r = load_rig(g, s, v);
    const float* __restrict__ ys = g.ysrc + ((size_t)s * g.S + v) * ((size_t)g.Hs * g.Ws);
    __syncthreads();                                       // tu / tZ are written; the last view's readers of tJ, tw, coef are done
    for (int i = t; i < ZH * ZW; i += kBlock) {
      const int py = i / ZW, px = i - py * ZW;
      float J = 0.f, su, sv;
      bool ok = false;
      float qz = 0.f;
      if (tu[i]) ok = warp_at(g, r, ys, tZ[i], y0 - 2 + py, x0 - 2 + px, J, su, sv, nullptr, kVis ? &qz : nullptr);
      if (kVis) ok = ok && visible_at(oc, oc.zbuf + (((size_t)s * g.n + h) * g.S + v) * ((size_t)oc.Hc * oc.Wc), qz, su, sv);
      tJ[i] = J, tw[i] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int i = t; i < CH * CW; i += kBlock) {
      const int wy = i / CW, wx = i - wy * CW;
      const int py = y0 - 1 + wy, px = x0 - 1 + wx;
      float c0 = 0.f, cI = 0.f, cJ = 0.f, mI = 0.f, mJ = 0.f;
      if (px >= 1 && px + 1 < g.W && py >= 1 && py + 1 < g.H && (!kMin || tsel[i] == v) && all_nine<ZW>(tw, wy + 1, wx + 1)) {
        Window w;
        window_of<ZW>(tI, tJ, wy + 1, wx + 1, w);
        window_coef(w, g.wssim, c0, cI, cJ, mI, mJ);
      }
      coef[0][i] = c0, coef[1][i] = cI, coef[2][i] = cJ, coef[3][i] = mI, coef[4][i] = mJ;
    }
    __syncthreads();
    if (inside && tw[ly * ZW + lx]) {
      const float I = tI[ly * ZW + lx], J = tJ[ly * ZW + lx];
      float sum = 0.f;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int c = (cy + dy) * CW + cx + dx;
          sum = sum + ((coef[0][c] + coef[1][c] * (I - coef[3][c])) + coef[2][c] * (J - coef[4][c]));
        }
      if (x >= 1 && x + 1 < g.W && y >= 1 && y + 1 < g.H && (!kMin || tsel[cy * CW + cx] == v) && all_nine<ZW>(tw, ly, lx))
        sum = sum + (1.f - g.wssim) * drho_of(g.rho, J - I);
      if (sum != 0.f) {
        float dJ = 0.f, Jagain, su, sv;
        warp_at(g, r, ys, tZ[ly * ZW + lx], y, x, Jagain, su, sv, &dJ);
        const float wk = (float)((double)hw.w[h] / (kMin ? views : views * cnt));
        total = total + (sum * dJ) * wk;
      }
    }
  }
  if (!inside) return;                                     // (no barrier below)
  float out = 0.f;
  if (total != 0.f) {
    float z, dz = 0.f;
    depth_at(g, predh, sbase, a, b, (size_t)y * g.W + x, z, &dz);
    out = (total * dz) * gout[0];
  }
  dpred[((size_t)s * g.n + h) * HW + (size_t)y * g.W + x] = out;
}

__global__ __launch_bounds__(256) void mv_backward_kernel(MV g, DpfHeadW hw, const double* __restrict__ stats, const float* __restrict__ gout,
                                                          float* __restrict__ dpred) {
  backward_tile<false, false>(g, Occ{}, nullptr, hw, stats, gout, dpred);
}

template <bool kVis, bool kMin>
__global__ __launch_bounds__(256) void mv_backward_occ_kernel(MV g, Occ oc, const unsigned char* __restrict__ sel, DpfHeadW hw,
                                                              const double* __restrict__ stats, const float* __restrict__ gout,
                                                              float* __restrict__ dpred) {
  backward_tile<kVis, kMin>(g, oc, sel, hw, stats, gout, dpred);
}

// the tile plan of the sibling (dpf_head_loss.h), refused as well where B n S does not fit on gridDim.z of the forward, the B + B S
// luminance planes on gridDim.y of their launch, or a source plane has 2^31 pixels or more
long long plan_rows(int B, int n, int S, int H, int W) {
  if (S < 1 || S > kMaxViews) return -1;
  const long long rows = dpf_tile_rows(B, n, H, W);
  if (rows < 0 || (long long)B * n * S > kDpfMaxGridZ || (long long)B * (S + 1) > kDpfMaxGridZ) return -1;
  return rows * S;
}

Rho rho_params(float alpha, float scale) {
  Rho r;
  const float eps = 1.1920929e-07f;
  r.scale = scale, r.alpha = alpha;
  r.beta = fmaxf(eps, fabsf(alpha - 2.f));
  const float safe = (alpha >= 0.f ? 1.f : -1.f) * fmaxf(eps, fabsf(alpha));
  r.lead = r.beta / safe, r.dlead = alpha / safe;
  r.mode = alpha == 2.f ? 0 : alpha == 0.f ? 1 : alpha == 1.f ? 2 : 3;
  return r;
}

// argument checks shared by forward and backward; fills g and hw (rig and the luminance planes are the caller's)
int prepare(const float* pred, const float* tgt_rgb, const float* src_rgb, long long src_stride, const float* rig, const float* ab,
            const float* mask, int B, int n, int S, int H, int W, int Hs, int Ws, int target_type, float weight_ssim, float alpha, float scale,
            float min_depth, const float* norm_host, const float* weights, const float* luma, MV& g, DpfHeadW& hw) {
  if (!pred || !tgt_rgb || !src_rgb || !rig || !norm_host || !weights || !luma || B <= 0 || n < 1 || n > kDpfMaxHeads || S < 1 ||
      S > kMaxViews || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || target_type < 0 || target_type > 2 || (target_type == 0 && !ab) ||
      !(weight_ssim >= 0.f && weight_ssim <= 1.f) || !isfinite(alpha) || !(scale > 0.f) || !isfinite(scale) || !(min_depth > 0.f) ||
      !isfinite(min_depth) || src_stride < 3LL * S * Hs * Ws)
    return DPF_ERR_INVALID_ARG;
  if (plan_rows(B, n, S, H, W) < 0 || (long long)Hs * Ws > 0x7fffffffLL) return DPF_ERR_UNSUPPORTED;
  g.pred = pred, g.ytgt = luma, g.ysrc = luma + (size_t)B * H * W, g.rig = rig, g.ab = ab, g.mask = mask;
  g.n = n, g.S = S, g.H = H, g.W = W, g.Hs = Hs, g.Ws = Ws, g.target_type = target_type;
  g.wssim = weight_ssim, g.min_depth = min_depth, g.rho = rho_params(alpha, scale);
  dpf_fill_head_weights(hw.w, weights, n);
  return DPF_OK;
}

bool cell_ok(int cell) { return cell == 1 || cell == 2 || cell == 4; }

Occ occ_of(const unsigned* zbuf, int cell, float tol, int Hs, int Ws) {
  Occ oc;
  oc.zbuf = zbuf, oc.cell = cell, oc.Hc = dpf_div_up(Hs, cell), oc.Wc = dpf_div_up(Ws, cell), oc.tol = tol;
  return oc;
}

// what the occlusion entry points add to prepare(): one of the two modes is on (the plain entry points serve the call with both off)
bool occ_args_ok(int reduce, int visibility, int cell, float tolerance, const float* zbuffer, const unsigned char* selected) {
  return reduce >= 0 && reduce <= 1 && visibility >= 0 && visibility <= 1 && (reduce || visibility) && cell_ok(cell) && tolerance >= 0.f &&
         isfinite(tolerance) && (!visibility || zbuffer) && (!reduce || selected);
}

// fill, then splat: two launches ahead of the forward on its stream (a cell's minimum comes from pixels anywhere in the image)
void launch_zbuffer(const MV& g, const Occ& oc, int B, hipStream_t st) {
  const long long cells = (long long)B * g.n * g.S * oc.Hc * oc.Wc;
  long long blocks = (cells + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  unsigned* zb = const_cast<unsigned*>(oc.zbuf);
  hipLaunchKernelGGL(mv_zfill_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, zb, cells);
  hipLaunchKernelGGL(mv_zsplat_kernel, dim3(dpf_div_up(g.W, kTW), dpf_div_up(g.H, kTH), B * g.n * g.S), dim3(kBlock), 0, st, g, oc, zb);
}

}  // namespace

extern "C" {

long long dpf_multiview_workspace_bytes(int B, int n, int S, int H, int W) {
  const long long rows = plan_rows(B, n, S, H, W);
  return rows < 0 ? -1 : rows * 2 * (long long)sizeof(double);
}

int dpf_multiview_rig(const float* K, const float* P, const float* Ks, const float* Ps, int B, int S, float* rig, void* stream) {
  dpf_clear_error();
  if (!K || !P || !Ks || !Ps || !rig || B <= 0 || S < 1 || S > kMaxViews) return DPF_ERR_INVALID_ARG;
  if ((long long)B * S > 0x7fffffffLL / 64) return DPF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mv_rig_kernel, dim3(dpf_div_up((long long)B * S, 64)), dim3(64), 0, (hipStream_t)stream, K, P, Ks, Ps, B, S, rig);
  return dpf_check_launch();
}

int dpf_multiview_forward(const float* pred, const float* tgt_rgb, const float* src_rgb, long long src_stride, const float* rig,
                          const float* ab, const float* mask, int B, int n, int S, int H, int W, int Hs, int Ws, int target_type,
                          float weight_ssim, float alpha, float scale, float min_depth, const float* norm_host,
                          const float* head_weights_host, void* ws, long long ws_bytes, float* luma, double* stats, float* out,
                          float* warped_out, unsigned char* counted_out, float* sample_xy_out, void* stream) {
  dpf_clear_error();
  MV g;
  DpfHeadW hw;
  const int rc = prepare(pred, tgt_rgb, src_rgb, src_stride, rig, ab, mask, B, n, S, H, W, Hs, Ws, target_type, weight_ssim, alpha, scale,
                         min_depth, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !out || (warped_out != nullptr) != (counted_out != nullptr) || (sample_xy_out && !warped_out) ||
      !dpf_ws_ok(ws, ws_bytes, dpf_multiview_workspace_bytes(B, n, S, H, W), 8))
    return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)H * W, HsWs = (long long)Hs * Ws;
  long long blocks = ((HW > HsWs ? HW : HsWs) + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mv_luma_kernel, dim3((unsigned)blocks, B * (S + 1)), dim3(kBlock), 0, st, tgt_rgb, src_rgb, src_stride, B, S, HW, HsWs,
                     dpf_norm_of(norm_host), luma);
  double* part = (double*)ws;
  hipLaunchKernelGGL(mv_forward_kernel, dim3(dpf_div_up(W, kTW), dpf_div_up(H, kTH), B * n * S), dim3(kBlock), 0, st, g, part, warped_out,
                     counted_out, sample_xy_out);
  hipLaunchKernelGGL(mv_fold_kernel, dim3(1), dim3(256), 0, st, part, dpf_tile_rows(B, n, H, W) / n, n, S, hw, stats, out);
  return dpf_check_launch();
}

int dpf_multiview_backward(const float* pred, const float* tgt_rgb, const float* src_rgb, long long src_stride, const float* rig,
                           const float* ab, const float* mask, int B, int n, int S, int H, int W, int Hs, int Ws, int target_type,
                           float weight_ssim, float alpha, float scale, float min_depth, const float* norm_host,
                           const float* head_weights_host, const float* luma, const double* stats, const float* gout, float* dpred,
                           void* stream) {
  dpf_clear_error();
  MV g;
  DpfHeadW hw;
  const int rc = prepare(pred, tgt_rgb, src_rgb, src_stride, rig, ab, mask, B, n, S, H, W, Hs, Ws, target_type, weight_ssim, alpha, scale,
                         min_depth, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !gout || !dpred) return DPF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(mv_backward_kernel, dpf_tile_grid(B, n, H, W), dim3(kBlock), 0, (hipStream_t)stream, g, hw, stats, gout, dpred);
  return dpf_check_launch();
}

long long dpf_multiview_occ_workspace_bytes(int B, int n, int S, int H, int W, int reduce) {
  const long long rows = plan_rows(B, n, S, H, W);
  if (rows < 0 || reduce < 0 || reduce > 1) return -1;
  return (reduce == 1 ? rows / S * kMinRow : rows * 2) * (long long)sizeof(double);
}

int dpf_multiview_zbuffer(const float* pred, const float* rig, const float* ab, const float* mask, int B, int n, int S, int H, int W, int Hs,
                          int Ws, int target_type, float min_depth, int cell, float* zbuffer, void* stream) {
  dpf_clear_error();
  if (!pred || !rig || !zbuffer || B <= 0 || n < 1 || n > kDpfMaxHeads || S < 1 || S > kMaxViews || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 ||
      target_type < 0 || target_type > 2 || (target_type == 0 && !ab) || !(min_depth > 0.f) || !isfinite(min_depth) || !cell_ok(cell))
    return DPF_ERR_INVALID_ARG;
  if (plan_rows(B, n, S, H, W) < 0 || (long long)Hs * Ws > 0x7fffffffLL) return DPF_ERR_UNSUPPORTED;
  MV g = {};
  g.pred = pred, g.rig = rig, g.ab = ab, g.mask = mask;
  g.n = n, g.S = S, g.H = H, g.W = W, g.Hs = Hs, g.Ws = Ws, g.target_type = target_type, g.min_depth = min_depth;
  launch_zbuffer(g, occ_of((unsigned*)zbuffer, cell, 0.f, Hs, Ws), B, (hipStream_t)stream);
  return dpf_check_launch();
}

int dpf_multiview_occ_forward(const float* pred, const float* tgt_rgb, const float* src_rgb, long long src_stride, const float* rig,
                              const float* ab, const float* mask, int B, int n, int S, int H, int W, int Hs, int Ws, int target_type,
                              float weight_ssim, float alpha, float scale, float min_depth, const float* norm_host,
                              const float* head_weights_host, int reduce, int visibility, int cell, float tolerance, void* ws,
                              long long ws_bytes, float* luma, float* zbuffer, unsigned char* selected, double* stats, float* out,
                              float* warped_out, unsigned char* counted_out, float* sample_xy_out, unsigned char* visible_out,
                              void* stream) {
  dpf_clear_error();
  MV g;
  DpfHeadW hw;
  const int rc = prepare(pred, tgt_rgb, src_rgb, src_stride, rig, ab, mask, B, n, S, H, W, Hs, Ws, target_type, weight_ssim, alpha, scale,
                         min_depth, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!occ_args_ok(reduce, visibility, cell, tolerance, zbuffer, selected) || !stats || !out ||
      (warped_out != nullptr) != (counted_out != nullptr) || (warped_out != nullptr) != (visible_out != nullptr) ||
      (sample_xy_out && !warped_out) || !dpf_ws_ok(ws, ws_bytes, dpf_multiview_occ_workspace_bytes(B, n, S, H, W, reduce), 8))
    return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)H * W, HsWs = (long long)Hs * Ws;
  long long blocks = ((HW > HsWs ? HW : HsWs) + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mv_luma_kernel, dim3((unsigned)blocks, B * (S + 1)), dim3(kBlock), 0, st, tgt_rgb, src_rgb, src_stride, B, S, HW, HsWs,
                     dpf_norm_of(norm_host), luma);
  const Occ oc = occ_of(visibility ? (unsigned*)zbuffer : nullptr, cell, tolerance, Hs, Ws);
  if (visibility) launch_zbuffer(g, oc, B, st);
  double* part = (double*)ws;
  const long long rows = dpf_tile_rows(B, n, H, W) / n;
  if (reduce == 1) {
    if (visibility)
      hipLaunchKernelGGL(mv_forward_min_kernel<true>, dpf_tile_grid(B, n, H, W), dim3(kBlock), 0, st, g, oc, part, selected, warped_out,
                         counted_out, sample_xy_out, visible_out);
    else
      hipLaunchKernelGGL(mv_forward_min_kernel<false>, dpf_tile_grid(B, n, H, W), dim3(kBlock), 0, st, g, oc, part, selected, warped_out,
                         counted_out, sample_xy_out, visible_out);
    hipLaunchKernelGGL(mv_fold_min_kernel, dim3(1), dim3(256), 0, st, part, rows, n, hw, stats, out);
  } else {
    hipLaunchKernelGGL(mv_forward_vis_kernel, dim3(dpf_div_up(W, kTW), dpf_div_up(H, kTH), B * n * S), dim3(kBlock), 0, st, g, oc, part,
                       warped_out, counted_out, sample_xy_out, visible_out);
    hipLaunchKernelGGL(mv_fold_kernel, dim3(1), dim3(256), 0, st, part, rows, n, S, hw, stats, out);
  }
  return dpf_check_launch();
}

int dpf_multiview_occ_backward(const float* pred, const float* tgt_rgb, const float* src_rgb, long long src_stride, const float* rig,
                               const float* ab, const float* mask, int B, int n, int S, int H, int W, int Hs, int Ws, int target_type,
                               float weight_ssim, float alpha, float scale, float min_depth, const float* norm_host,
                               const float* head_weights_host, int reduce, int visibility, int cell, float tolerance, const float* luma,
                               const float* zbuffer, const unsigned char* selected, const double* stats, const float* gout, float* dpred,
                               void* stream) {
  dpf_clear_error();
  MV g;
  DpfHeadW hw;
  const int rc = prepare(pred, tgt_rgb, src_rgb, src_stride, rig, ab, mask, B, n, S, H, W, Hs, Ws, target_type, weight_ssim, alpha, scale,
                         min_depth, norm_host, head_weights_host, luma, g, hw);
  if (rc != DPF_OK) return rc;
  if (!occ_args_ok(reduce, visibility, cell, tolerance, zbuffer, selected) || !stats || !gout || !dpred) return DPF_ERR_INVALID_ARG;
  const Occ oc = occ_of(visibility ? (const unsigned*)zbuffer : nullptr, cell, tolerance, Hs, Ws);
  const dim3 grid = dpf_tile_grid(B, n, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (reduce == 1 && visibility)
    hipLaunchKernelGGL((mv_backward_occ_kernel<true, true>), grid, dim3(kBlock), 0, st, g, oc, selected, hw, stats, gout, dpred);
  else if (reduce == 1)
    hipLaunchKernelGGL((mv_backward_occ_kernel<false, true>), grid, dim3(kBlock), 0, st, g, oc, selected, hw, stats, gout, dpred);
  else
    hipLaunchKernelGGL((mv_backward_occ_kernel<true, false>), grid, dim3(kBlock), 0, st, g, oc, selected, hw, stats, gout, dpred);
  return dpf_check_launch();
}

}  // extern "C"
