// The normalised RGB image as the kernels read it (photometric.hip, postprocess.hip; reconstruct.hip takes the record only): the data
// path's Normalizer constants arrive as six host floats (mean_0..2, std_0..2) and go by value into the kernels, and the luminance is
// Y = 0.299 R + 0.587 G + 0.114 B of the de-normalised image, R = x_0 std_0 + mean_0 and so on.
#pragma once
#include "dpf_common.h"

constexpr float kDpfLumaR = 0.299f, kDpfLumaG = 0.587f, kDpfLumaB = 0.114f;

struct DpfNorm { float mean[3], std[3]; };

inline DpfNorm dpf_norm_of(const float* norm_host) {
  DpfNorm nm;
  for (int c = 0; c < 3; ++c) nm.mean[c] = norm_host[c], nm.std[c] = norm_host[3 + c];
  return nm;
}

// the luminance of the normalised triple (x0, x1, x2); the products and sums associate from the left, as written
__device__ __forceinline__ float dpf_luma(float x0, float x1, float x2, const DpfNorm& nm) {
  return kDpfLumaR * (x0 * nm.std[0] + nm.mean[0]) + kDpfLumaG * (x1 * nm.std[1] + nm.mean[1]) + kDpfLumaB * (x2 * nm.std[2] + nm.mean[2]);
}
