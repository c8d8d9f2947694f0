// Internal (non-ABI) interface between the deformable-convolution translation units.
#pragma once
#include "dpf_common.h"

// replicas of the grad_weight scratch tensor dwtmp[rep][27][nchunk][64][16] that the backward kernels of BOTH translation units add into and
// dcn_wgrad_fold_kernel (dcn3d.hip) folds
constexpr int DCN_WG_NREP = 8;

#ifdef __HIPCC__
// grad_input / grad_weight-scratch accumulation: float atomics, or -- deterministic mode (dpf_common.h) -- order-independent integer pairs in a
// shadow array indexed like the float tensor (`shadow` != nullptr).  The shadow of grad_input lives behind the ordinary workspace
// (dpf_deform_conv3d_backward_workspace_floats), the grad_weight scratch is its own shadow (a replica of int64 pairs fits in 4 of its 8
// float replicas).
__device__ __forceinline__ void dcn_acc_add(float* base, long long* shadow, float* addr, float v) {
  if (shadow) dpf_det_add(shadow + 2 * (addr - base), v);
  else atomicAdd(addr, v);
}
#endif

// The family's environment switches (README "Environment switches"), read once per process by dcn_env() (dcn3d.hip).
struct DcnEnv {
  bool v1;           // DPF_DCN_V1 set: first-generation gather kernels only
  int lean;          // DPF_DCN_LEAN (1): 0 = lean kernels off; bit 2 (4) = only the lean grad_offset kernel off
  int fwd6;          // DPF_DCN_FWD6 (1): 0 = lean forward on the fp32 matrix instruction
  int lean_wide12;   // DPF_DCN_LEAN_WIDE12 (0): 1 = 12-channel lean forward on the wider x halo, one workgroup per CU (3.7 vs 2.6 ms)
  int gcol16;        // DPF_DCN_GCOL16 (1): 0 = the backward's gcol products on the fp32 matrix instruction
};
const DcnEnv& dcn_env();

// the configuration StereoDPNet runs: 3x3x3 taps, stride 1, padding 1, dilation 1
inline bool dcn_is_model_config(int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int dd, int dh, int dw) {
  return kd == 3 && kh == 3 && kw == 3 && sd == 1 && sh == 1 && sw == 1 && pd == 1 && ph == 1 && pw == 1 && dd == 1 && dh == 1 && dw == 1;
}

// channel-chunk width of the region and the lean kernels: 12 where it pads the channel count less than 16 does (35 -> 36 instead of 48)
inline int dcn_chunk(int C) { return ((C + 11) / 12 * 12 < (C + 15) / 16 * 16) ? 12 : 16; }

#ifdef __HIPCC__
// launch `kern`, first raising its dynamic-LDS limit where it needs more than the 48 KB default
template <typename... P, typename... A>
int dcn_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return DPF_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  return DPF_OK;
}
#endif

// "Lean" kernels (dcn_lean.hip) for the model configuration with depth <= 4, rows 16-byte aligned (W % 4 == 0), K <= 64.  Each returns
// DPF_ERR_UNSUPPORTED when the shape is not eligible (the caller then uses the generic region kernels of dcn3d.hip), DPF_OK when it launched.
//
// weight: the caller's [K][C][27] tensor; ws: workspace of at least dcn_lean_workspace_floats(C, K) floats (weights repacked into the
// matrix waves' fragment order; the larger of the forward and the backward repack).
long long dcn_lean_workspace_floats(int C, int K);
int dcn_lean_forward(const float* x, const float* offset, const float* weight, const float* bias, float* out, float* ws, int B, int C, int D, int H,
                     int W, int K, hipStream_t st);
// grad_offset + grad_weight partials: dwtmp[8][27][nchunk][64][16] (zero-initialised by the caller; chunk width dcn_chunk(C)).
// det != 0: the partials are added as integer pairs into replica 0 read as long long [27][nchunk][64][16][2] (deterministic mode).
int dcn_lean_bwd_offset(const float* x, const float* offset, const float* weight, const float* go, float* doff, float* dwtmp, float* ws, int B, int C,
                        int D, int H, int W, int K, hipStream_t st, int det = 0);
