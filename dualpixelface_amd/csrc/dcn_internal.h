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

// output positions per workgroup of the gather kernels (dcn3d.hip, dcn_gather.hip)
constexpr int DCN_TP = 64;

// Geometry of one call and the 3-D sampling rule, shared by the translation units of the family (dcn3d.hip, dcn_gather.hip, dcn2d.hip).  A 2-D
// call (dcn2d.hip) is the same record at depth 1: D = Do = kd = sd = dd = 1, pd = 0.
struct DcnP {
  int B, C, K;
  int D, H, W;        // input dims
  int Do, Ho, Wo;     // output dims
  int kd, kh, kw, T;
  int sd, sh, sw, pd, ph, pw, dd, dh, dw;
  int CP;             // C rounded up to even
  long long P;        // Do*Ho*Wo
  int tiles_per_b;
  int nchunk;
};

struct Corner {   // per output voxel and tap
  int d0, h0, w0;
  float ld, lh, lw;
  int valid;
};

struct Off3 {
  float d, h, w;
};

#ifdef __HIPCC__
// the three offset components of tap t at output voxel pos (cuh:238-243); zeros beyond the volume / tap range
__device__ __forceinline__ Off3 load_off(const DcnP& p, const float* __restrict__ off_b, int t, long long pos) {
  Off3 o = {0.f, 0.f, 0.f};
  if (pos < p.P && t < p.T) {
    o.d = off_b[(long long)(3 * t) * p.P + pos];
    o.h = off_b[(long long)(3 * t + 1) * p.P + pos];
    o.w = off_b[(long long)(3 * t + 2) * p.P + pos];
  }
  return o;
}

__device__ __forceinline__ Corner corner_from(const DcnP& p, int t, long long pos, const Off3& o) {
  Corner c;
  c.valid = 0;
  c.d0 = c.h0 = c.w0 = 0;
  c.ld = c.lh = c.lw = 0.f;
  if (pos >= p.P) return c;
  const int xo = (int)(pos % p.Wo);
  const int yo = (int)((pos / p.Wo) % p.Ho);
  const int zo = (int)(pos / ((long long)p.Wo * p.Ho));
  const int tk = t % p.kw, tj = (t / p.kw) % p.kh, ti = t / (p.kw * p.kh);
  const float fd = (float)(zo * p.sd - p.pd + ti * p.dd) + o.d;
  const float fh = (float)(yo * p.sh - p.ph + tj * p.dh) + o.h;
  const float fw = (float)(xo * p.sw - p.pw + tk * p.dw) + o.w;
  if (fd > -1.f && fh > -1.f && fw > -1.f && fd < (float)p.D && fh < (float)p.H && fw < (float)p.W) {   // cuh:248
    const float d0 = floorf(fd), h0 = floorf(fh), w0 = floorf(fw);
    c.d0 = (int)d0; c.h0 = (int)h0; c.w0 = (int)w0;
    c.ld = fd - d0; c.lh = fh - h0; c.lw = fw - w0;
    c.valid = 1;
  }
  return c;
}

__device__ __forceinline__ Corner make_corner(const DcnP& p, const float* __restrict__ off_b, int t, long long pos) {
  return corner_from(p, t, pos, load_off(p, off_b, t, pos));
}

// corner j = (jd, jh, jw) bits; returns flat voxel index or -1 (cuh:43-65), weight (cuh:67-68)
__device__ __forceinline__ long long corner_index(const DcnP& p, const Corner& c, int j, float& wgt) {
  const int jd = (j >> 2) & 1, jh = (j >> 1) & 1, jw = j & 1;
  const int d = c.d0 + jd, h = c.h0 + jh, w = c.w0 + jw;
  wgt = (jd ? c.ld : 1.f - c.ld) * (jh ? c.lh : 1.f - c.lh) * (jw ? c.lw : 1.f - c.lw);
  if (!c.valid || d < 0 || d > p.D - 1 || h < 0 || h > p.H - 1 || w < 0 || w > p.W - 1) return -1;
  return ((long long)d * p.H + h) * p.W + w;
}
#endif

// The family's environment switches (README "Environment switches"), read once per process by dcn_env() (dcn3d.hip).
struct DcnEnv {
  bool v1;           // DPF_DCN_V1 set: gather kernels only (grad_input still from the packed scatter where that fits)
  int lean;          // DPF_DCN_LEAN (1): 0 = lean kernels off; bit 2 (4) = only the lean grad_offset kernel off
  int fwd6;          // DPF_DCN_FWD6 (1): 0 = lean forward on the fp32 matrix instruction
  int lean_wide12;   // DPF_DCN_LEAN_WIDE12 (0): 1 = 12-channel lean forward on the wider x halo, one workgroup per CU (3.7 vs 2.6 ms)
  int gcol16;        // DPF_DCN_GCOL16 (1): 0 = the backward's gcol and weight-gradient products on the fp32 matrix instruction
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

// The gather family with the grouping as a kernel argument (dcn_gather.hip), rank 3 (dcn3d.hip: group > 1 or deformable_group > 1, and the single-group backward without the packed scatter) or rank 2
// (dcn2d.hip: every call): a fixed number of launches per call, every product on the fp32 matrix instruction.
// dcn_group_check: DPF_ERR_INVALID_ARG unless group divides C and K and deformable_group divides C.
// mask: [B][deformable_group * T][P] or nullptr; rank 3 has none.  wpack: room for wpack_floats floats, where the block-diagonal weights are
// repacked; DPF_ERR_UNSUPPORTED with nothing launched if they do not fit.
// Backward: grad_input, grad_offset, grad_mask, grad_weight may each be nullptr (not wanted); grad_input / grad_weight are zero-initialised by
// the caller; deterministic mode: dw_shadow / gi_shadow = zero-initialised integer shadows (dcn_acc_add) of grad_weight [K][C/group][T] and
// grad_input that the caller folds with dcn_finalize, else nullptr.  grad_input is produced for the channels [0, grad_input_channels).
// grad_offset and grad_mask are stored once per element in either mode.
int dcn_group_check(int C, int K, int group, int deformable_group);
int dcn_gather_forward(int rank, const DcnP& p, int group, int deformable_group, const float* input, const float* weight, const float* bias,
                       const float* offset, const float* mask, float* output, float* wpack, long long wpack_floats, hipStream_t st);
int dcn_gather_backward(int rank, const DcnP& p, int group, int deformable_group, const float* input, const float* weight, const float* offset,
                        const float* mask, const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                        float* wpack, long long wpack_floats, long long* dw_shadow, long long* gi_shadow, int grad_input_channels, hipStream_t st);
// deterministic mode: out[0 .. n) = value of its integer shadow (every contribution went there; the tensor itself was only zero-filled)
void dcn_finalize(const long long* shadow, float* out, long long n, hipStream_t st);
