// What the disparity head (softargmin.hip), the loss on its hypothesis distribution (unimodal.hip) and the confidence planes read off it
// (head_confidence.hip) share: THE index arithmetic of the trilinear upsampling of the [B, 1, D, h, w] cost logits and the expression
// order of the upsampled logits, stated once, and for the latter two the work of one pixel (Pixel<FAST>).  A file that
// includes this computes the same u_l from the same logits, operation for operation (the rounding of the products and sums still follows
// the including file's -ffp-contract setting).
#pragma once
#include "dpf_common.h"

namespace {

constexpr int MAXD = 8;     // low-res depth levels
constexpr int MAXL = 32;    // upsampled hypotheses

struct HeadP {
  int B, D, h, w, L, H, W;
  long long pbs;        // batch stride of the probability output (0: L * H * W, dense)
  float off;            // 0: align_corners=True (ratio (in-1)/(out-1)); 0.5: align_corners=False (ratio in/out, half-pixel centres)
  float disp[MAXL];
};

__device__ __forceinline__ float head_ratio(int in, int out, float off) {
  return off > 0.f ? (float)in / (float)out : (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f);
}

__device__ __forceinline__ void ac_src(int dst, float ratio, int in, int& i0, int& i1, float& lam, float off = 0.f) {
  float src = ratio * ((float)dst + off) - off;       // ATen area_pixel_compute_source_index
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = src - (float)i0;
}

// the bilinear value of the plane q (row pitch w) at the taps (y0, y1) x (x0, x1), hy = 1 - ly, hx = 1 - lx: THE expression order
__device__ __forceinline__ float head_bilinear(const float* q, int w, int y0, int y1, int x0, int x1, float hy, float ly, float hx, float lx) {
  return hy * (hx * q[y0 * w + x0] + lx * q[y0 * w + x1]) + ly * (hx * q[y1 * w + x0] + lx * q[y1 * w + x1]);
}

// the level taps of hypothesis l of the shipped geometry (8 cost levels -> 32 hypotheses, align_corners): the expression of ac_src, which
// folds at compile time where l is a constant -- 32 FMAs on registers instead of 512 register-select instructions
__device__ __forceinline__ void level_taps_8x32(int l, int& d0, int& d1, float& ld) {
  constexpr int D = 8, L = 32;
  constexpr float rd = (float)(D - 1) / (float)(L - 1);
  const float src = rd * (float)l;
  d0 = (int)src;
  if (d0 > D - 1) d0 = D - 1;
  d1 = d0 + (d0 < D - 1 ? 1 : 0);
  ld = src - (float)d0;
}

// u_l from the level values and the level taps of hypothesis l
__device__ __forceinline__ float level_value(const float* bl, int d0, int d1, float ld) {
  float v0 = 0.f, v1 = 0.f;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) {   // register-resident select (no runtime-indexed array)
    v0 = (d == d0) ? bl[d] : v0;
    v1 = (d == d1) ? bl[d] : v1;
  }
  return (1.f - ld) * v0 + ld * v1;
}

// the upsampled logits u_l (l < p.L) of pixel (Y, X) of sample b and their maximum, any geometry; also the taps and fractions in y and x
__device__ __forceinline__ void pixel_logits(const float* __restrict__ k, const HeadP& p, int b, int Y, int X, float rd, float ry, float rx,
                                             float* u, float& mx, int& y0, int& y1, int& x0, int& x1, float& ly, float& lx) {
  ac_src(Y, ry, p.h, y0, y1, ly, p.off);
  ac_src(X, rx, p.w, x0, x1, lx, p.off);
  const float hy = 1.f - ly, hx = 1.f - lx;
  float bl[MAXD];
  const float* kb = k + (long long)b * p.D * p.h * p.w;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) {
    if (d < p.D) {
      const float* q = kb + (long long)d * p.h * p.w;
      bl[d] = head_bilinear(q, p.w, y0, y1, x0, x1, hy, ly, hx, lx);
    } else {
      bl[d] = 0.f;
    }
  }
  mx = -3.4e38f;
#pragma unroll
  for (int l = 0; l < MAXL; ++l) {
    if (l < p.L) {
      int d0, d1;
      float ld;
      ac_src(l, rd, p.D, d0, d1, ld, p.off);
      u[l] = level_value(bl, d0, d1, ld);
      mx = fmaxf(mx, u[l]);
    }
  }
}

// The same for the shipped geometry.  THE 8 -> 32 LOOP EXISTS THREE TIMES and the copies have to be changed together: here (used by
// unimodal.hip) and, written out, in head_fwd_8x32_kernel and head_bwd_8x32_kernel of softargmin.hip.  Those two keep their own loops around
// the shared expressions (head_bilinear, level_taps_8x32) because moving the loops into a function changed which product of a sum the
// compiler fuses, i.e. the bits of the shipped head.  Likewise the general path of unimodal.hip assembles u_l from head_bilinear, ac_src and
// level_value in rolled loops instead of calling pixel_logits.  kb: the logits of the sample, lplane = h w
__device__ __forceinline__ void pixel_logits_8x32(const float* kb, long long lplane, int w, int y0, int y1, int x0, int x1, float ly, float lx,
                                                  float* bl, float* u, float& mx) {
  constexpr int D = 8, L = 32;
  const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
  for (int d = 0; d < D; ++d) bl[d] = head_bilinear(kb + (long long)d * lplane, w, y0, y1, x0, x1, hy, ly, hx, lx);
  mx = -3.4e38f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    int d0, d1;
    float ld;
    level_taps_8x32(l, d0, d1, ld);
    u[l] = (1.f - ld) * bl[d0] + ld * bl[d1];
    mx = fmaxf(mx, u[l]);
  }
}

// The work of one pixel (unimodal.hip, head_confidence.hip), for the shipped geometry (FAST: D = 8, L = 32, align_corners; every loop over the hypotheses unrolled, the level
// taps constants) and for any other (loops over the hypotheses rolled, u_l formed again in each from the D level values in registers:
// no register array is indexed at run time, and the level taps of 32 hypotheses are not all held in scalar registers at once).  Both
// state the same operations in the same order.
template <bool FAST>
struct Pixel {
  float bl[MAXD];      // the bilinear value of every cost level
  float u[FAST ? MAXL : 1];

  // (general geometry) u_l
  __device__ __forceinline__ float logit(const HeadP& p, float rd, int l) const {
    int d0, d1;
    float ld;
    ac_src(l, rd, p.D, d0, d1, ld, p.off);
    return level_value(bl, d0, d1, ld);
  }

  // the level values, and mx = max_l u_l
  __device__ __forceinline__ float upsample(const float* __restrict__ k, const HeadP& p, int b, float rd, int y0, int y1, int x0, int x1, float ly,
                                            float lx) {
    const long long lplane = (long long)p.h * p.w;
    const float* kb = k + (long long)b * p.D * lplane;
    float mx;
    if (FAST) {
      pixel_logits_8x32(kb, lplane, p.w, y0, y1, x0, x1, ly, lx, bl, u, mx);
    } else {
      const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
      for (int d = 0; d < MAXD; ++d)      // (past the D levels in use: the last one again, never selected)
        bl[d] = head_bilinear(kb + (long long)min(d, p.D - 1) * lplane, p.w, y0, y1, x0, x1, hy, ly, hx, lx);
      mx = -3.4e38f;
#pragma unroll 1
      for (int l = 0; l < p.L; ++l) mx = fmaxf(mx, logit(p, rd, l));
    }
    return mx;
  }
};

#define UNI_FOR_L(l) _Pragma("unroll") for (int l = 0; l < MAXL; ++l)

}  // namespace
