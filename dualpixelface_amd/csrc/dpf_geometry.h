// The camera geometry reconstruct.hip and normal_geo.hip share, stated once: Kinv, the ray of a pixel and the test
// that ties two neighbouring depths to one surface.  Every fp32 expression is written operation by operation; both files are compiled
// with -ffp-contract=off so that the numpy restatements (tests/reconstruct_cpu.py, tests/normal_geo_cpu.py) give the same bits.
// Kinv: the 3 x 3 adjugate over the determinant in fp64 from the fp32 K, each entry rounded to fp32 once; |det| < 1e-30 (or a non-finite
// det) makes the whole sample invalid.  Ray: (Kinv[k][0] x + Kinv[k][1] y) + Kinv[k][2] in fp32.
// Connected(p, q): both depths > 0 (0 stands for "not valid") and |z_p - z_q| <= ratio * min(z_p, z_q) (fp32: multiply, then compare).
#pragma once
#include "dpf_common.h"
#include <math.h>

struct Cam {
  float inv[9];       // Kinv, row-major
  float a, b;         // depth = a / (pred - b)
  int ok;             // K regular
};

// one thread per workgroup forms the sample's camera; the caller publishes it with a barrier.  ab [B, 2] = [b, a], unread for target
// type 2 (depth)
__device__ inline void cam_setup(const float* Kmat, const float* ab, int target_type, int s, Cam* cam) {
  const float* Kf = Kmat + (size_t)s * 9;
  double m[9];
  for (int k = 0; k < 9; ++k) m[k] = (double)Kf[k];
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
  cam->ok = isfinite(det) && fabs(det) >= 1e-30;
  const double adj[9] = {c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
  for (int k = 0; k < 9; ++k) cam->inv[k] = cam->ok ? (float)(adj[k] / det) : 0.f;
  cam->b = target_type == 2 ? 0.f : ab[2 * (size_t)s];
  cam->a = target_type == 2 ? 0.f : ab[2 * (size_t)s + 1];
}

__device__ __forceinline__ void ray_of(const Cam& cam, int y, int x, float (&r)[3]) {
  const float xf = (float)x, yf = (float)y;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = (cam.inv[3 * k] * xf + cam.inv[3 * k + 1] * yf) + cam.inv[3 * k + 2];
}

__device__ __forceinline__ bool connected(float zp, float zq, float ratio) {
  return zp > 0.f && zq > 0.f && fabsf(zp - zq) <= ratio * fminf(zp, zq);
}
