// The camera geometry reconstruct.hip, normal_geo.hip and normal_refine.hip share, stated once: Kinv, the ray of a
// pixel, the test that ties two neighbouring depths to one surface, and the valid depth of a prediction.  Every fp32 expression is written
// operation by operation; the files are compiled with -ffp-contract=off so that the numpy restatements (tests/reconstruct_cpu.py,
// tests/normal_geo_cpu.py, tests/normal_refine_cpu.py) give the same bits.
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

// The operands reconstruct.hip's three operators and normal_refine.hip share: head 0 of a prediction as an H W plane per sample, pstride
// floats apart, with what turns it into valid depths.
struct Scene {
  const float* pred;
  long long pstride;
  const float* ab;
  const float* Kmat;
  const float* mask;
  int target_type, H, W;
  float z_near, z_far;
};

// the depth of pixel (y, x) of sample s where it is valid, else 0: z = a / (pred - b) (target types 0, 1) or pred (2), non-finite -> 0;
// valid where near < z < far, the mask is NULL or > 0 and K is regular
__device__ __forceinline__ float valid_depth(const Scene& sc, const Cam& cam, int s, int y, int x) {
  const size_t o = (size_t)y * sc.W + x;
  const float p = sc.pred[(size_t)s * (size_t)sc.pstride + o];
  float z = sc.target_type == 2 ? p : cam.a / (p - cam.b);
  if (!isfinite(z)) z = 0.f;
  bool ok = cam.ok && z > sc.z_near && z < sc.z_far;
  if (sc.mask) ok = ok && sc.mask[(size_t)s * sc.H * sc.W + o] > 0.f;
  return ok ? z : 0.f;
}

inline bool scene_ok(const float* pred, long long pstride, int target_type, const float* ab, const float* Kmat, int B, int H, int W,
                     float z_near, float z_far) {
  return pred && Kmat && B > 0 && H > 0 && W > 0 && target_type >= 0 && target_type <= 2 && (target_type == 2 || ab) &&
         pstride >= (long long)H * W && z_near >= 0.f && z_far > z_near;      // (a NaN limit fails both comparisons)
}

inline Scene scene_of(const float* pred, long long pstride, int target_type, const float* ab, const float* Kmat, const float* mask, int H,
                      int W, float z_near, float z_far) {
  Scene sc;
  sc.pred = pred, sc.pstride = pstride, sc.ab = ab, sc.Kmat = Kmat, sc.mask = mask;
  sc.target_type = target_type, sc.H = H, sc.W = W, sc.z_near = z_near, sc.z_far = z_far;
  return sc;
}
