// The 3 x 3 SSIM window of the image-reprojection losses (photometric.hip, multiview.hip): I and J in LDS tiles of
// row pitch LW, the warpable flags beside them.  Every fp32 expression is written operation by operation (the files that include this
// are built with -ffp-contract=off), so that the numpy restatements of the tests reproduce a window bit for bit.
//
//   window   i = I - I_centre, j = J - I_centre; sums of i, j, i i, j j, i j over the nine pixels in row-major order; m = sum / 9,
//            mu = I_centre + m, var = mean of squares - m^2, cov = mean of products - m_I m_J
//   SSIM     (((2 mu_I) mu_J + C1) (2 cov + C2)) / (((mu_I^2 + mu_J^2) + C1) ((var_I + var_J) + C2))
#pragma once
#include "dpf_common.h"

namespace {

constexpr float kC1 = 0.0001f, kC2 = 0.0009f;  // 0.01^2, 0.03^2

struct Window {
  float muI, muJ, vI, vJ, cov, A1, A2, B1, B2, ssim;
};

// the window whose centre is (ly, lx) of the LDS tiles (row pitch LW): sums in row-major order of the values less the centre's I, so
// that the variances are differences of small numbers
template <int LW>
__device__ __forceinline__ void window_of(const float* __restrict__ tI, const float* __restrict__ tJ, int ly, int lx, Window& w) {
  const float c = tI[ly * LW + lx];
  float sI = 0.f, sJ = 0.f, sII = 0.f, sJJ = 0.f, sIJ = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float i = tI[(ly + dy) * LW + lx + dx] - c, j = tJ[(ly + dy) * LW + lx + dx] - c;
      sI = sI + i;
      sJ = sJ + j;
      sII = sII + i * i;
      sJJ = sJJ + j * j;
      sIJ = sIJ + i * j;
    }
  const float mI = sI / 9.f, mJ = sJ / 9.f;
  w.muI = c + mI, w.muJ = c + mJ;
  w.vI = sII / 9.f - mI * mI;
  w.vJ = sJJ / 9.f - mJ * mJ;
  w.cov = sIJ / 9.f - mI * mJ;
  w.A1 = (2.f * w.muI) * w.muJ + kC1;
  w.A2 = 2.f * w.cov + kC2;
  w.B1 = (w.muI * w.muI + w.muJ * w.muJ) + kC1;
  w.B2 = (w.vI + w.vJ) + kC2;
  w.ssim = (w.A1 * w.A2) / (w.B1 * w.B2);
}

template <int LW>
__device__ __forceinline__ bool all_nine(const unsigned char* __restrict__ tw, int ly, int lx) {
  bool ok = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) ok = ok && tw[(ly + dy) * LW + lx + dx];
  return ok;
}

// d term / d J_k of a counted window, term = k_ssim clamp((1 - SSIM) / 2, 0, 1): c0 + cI (I_k - mu_I) + cJ (J_k - mu_J), zeros where the
// clamp is active.  d ssim / d J_k = (2 / 9) (muI A2 / (B1 B2) - ssim muJ / B1 + A1 / (B1 B2) (I_k - muI) - ssim / B2 (J_k - muJ)), and
// d term / d ssim = -k_ssim / 2
__device__ __forceinline__ void window_coef(const Window& w, float k_ssim, float& c0, float& cI, float& cJ, float& mI, float& mJ) {
  c0 = 0.f, cI = 0.f, cJ = 0.f, mI = 0.f, mJ = 0.f;
  const float ds = (1.f - w.ssim) / 2.f;
  if (ds >= 0.f && ds <= 1.f) {
    const float k = -(k_ssim / 9.f);
    const float den = w.B1 * w.B2;
    c0 = k * ((w.muI * w.A2) / den - (w.ssim * w.muJ) / w.B1);
    cI = k * (w.A1 / den);
    cJ = -(k * (w.ssim / w.B2));
    mI = w.muI, mJ = w.muJ;
  }
}

}  // namespace
