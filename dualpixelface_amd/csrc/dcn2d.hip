// Deformable 2-D convolution, plain (DCN v1) and modulated (v2, per-sample mask): the C ABI of the reference's second compiled extension
// `deform_conv_cuda` (src/module/dcn/src/deform_conv_cuda.cpp:687-697).  The kernels are the rank-2 instantiations of the gather family in
// dcn_gather.hip, whose header describes the tensors, the sampling rule and the precision; here: argument checks, the workspace map, the
// zero-fills, the deterministic-mode shadows and grad_bias.
// LIMITS: whole C, K <= 256, T <= 49, H W < 2^31; any stride, padding, dilation and any dividing grouping.
#include "dpf_common.h"
#include "dcn_internal.h"

namespace {

constexpr int TP = DCN_TP;      // output positions per workgroup
constexpr int MAXC2 = 256;      // whole C and K
constexpr int MAXT2 = 49;

// DPF_ERR_INVALID_ARG: a size that is no size, or a grouping that does not divide; DPF_ERR_UNSUPPORTED: beyond the limits of the header
int fill_params2(DcnP& p, int B, int C, int H, int W, int K, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int group,
                 int deformable_group) {
  if (B <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0 || dh <= 0 || dw <= 0)
    return DPF_ERR_INVALID_ARG;
  if (dcn_group_check(C, K, group, deformable_group) != DPF_OK) return DPF_ERR_INVALID_ARG;
  const long long Ho = ((long long)H + 2LL * ph - ((long long)dh * (kh - 1) + 1)) / sh + 1;
  const long long Wo = ((long long)W + 2LL * pw - ((long long)dw * (kw - 1) + 1)) / sw + 1;
  if ((long long)H + 2LL * ph < (long long)dh * (kh - 1) + 1 || (long long)W + 2LL * pw < (long long)dw * (kw - 1) + 1) return DPF_ERR_INVALID_ARG;
  const long long T = (long long)kh * kw;
  if (C > MAXC2 || K > MAXC2 || T > MAXT2) return DPF_ERR_UNSUPPORTED;
  if ((long long)H * W >= 0x7fffffffLL || Ho * Wo >= 0x7fffffffLL - TP) return DPF_ERR_UNSUPPORTED;
  p.B = B; p.C = C; p.K = K; p.D = 1; p.H = H; p.W = W; p.Do = 1; p.Ho = (int)Ho; p.Wo = (int)Wo;
  p.kd = 1; p.kh = kh; p.kw = kw; p.T = (int)T;
  p.sd = 1; p.sh = sh; p.sw = sw; p.pd = 0; p.ph = ph; p.pw = pw; p.dd = 1; p.dh = dh; p.dw = dw;
  p.CP = (C + 1) & ~1;
  p.P = Ho * Wo;
  p.tiles_per_b = (int)((p.P + TP - 1) / TP);
  if ((long long)B * p.tiles_per_b >= 0x7fffffffLL) return DPF_ERR_UNSUPPORTED;
  p.nchunk = 1;
  return DPF_OK;
}

// The workspace of one call, as float offsets from its base: the repacked block-diagonal weights (the larger of the forward's [T][CP][KT] and
// the backward's [T][KP][CT]), then -- deterministic mode only -- the integer shadows of grad_weight and grad_input (4 floats per element).
// Sized from whole C and K, so one query holds for every grouping.
struct Dcn2Ws {
  long long dw_shadow, gi_shadow, total;
};

long long r32(long long v) { return (v + 31) / 32 * 32; }

Dcn2Ws ws_map2(int B, int C, int H, int W, int K, int T, int det) {
  auto pos = [](int v) { return (long long)(v > 0 ? v : 1); };
  Dcn2Ws m;
  m.dw_shadow = pos(T) * r32(pos(C)) * r32(pos(K));   // a multiple of 1024 floats: the shadows behind it are 8-byte aligned when ws is
  m.gi_shadow = m.dw_shadow + (det ? 4 * pos(K) * pos(C) * pos(T) : 0);
  m.total = m.gi_shadow + (det ? 4 * pos(B) * pos(C) * pos(H) * pos(W) : 0);
  return m;
}

}  // namespace

extern "C" {

int dpf_channel_sum(const float* g, float* out, int N, int C, long long S, void* stream);   // norm_act.hip

long long dpf_deform_conv2d_workspace_floats(int C, int K, int T) { return ws_map2(0, C, 0, 0, K, T, 0).total; }

long long dpf_deform_conv2d_backward_workspace_floats(int B, int C, int H, int W, int K, int T) {
  return ws_map2(B, C, H, W, K, T, dpf_deterministic()).total;
}

// deform_conv_forward_cuda / modulated_deform_conv_cuda_forward (deform_conv_cuda.cpp:156-263,491-569) without their column buffers:
// repack + one kernel.  mask == nullptr: the plain operator.
int dpf_deform_conv2d_forward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask, float* output,
                              float* ws, int B, int C, int H, int W, int K, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int group, int deformable_group, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!input || !weight || !offset || !output || !ws) return DPF_ERR_INVALID_ARG;
  DcnP p{};
  const int rc = fill_params2(p, B, C, H, W, K, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
  if (rc != DPF_OK) return rc;
  const long long room = ws_map2(0, C, 0, 0, K, p.T, 0).dw_shadow;
  return dcn_gather_forward(2, p, group, deformable_group, input, weight, bias, offset, mask, output, ws, room, (hipStream_t)stream);
}

// deform_conv_backward_input_cuda + deform_conv_backward_parameters_cuda / modulated_deform_conv_cuda_backward (deform_conv_cuda.cpp:265-489,
// 571-685).  Every result passed is fully written (the accumulated ones are zero-filled here).  grad_input, grad_offset, grad_mask,
// grad_weight and grad_bias may each be nullptr: a result that is not wanted; the data kernel is not launched when grad_input, grad_offset and
// grad_mask are all absent, the weight kernel not when grad_weight is.  grad_mask needs mask.
int dpf_deform_conv2d_backward(const float* input, const float* weight, const float* bias, const float* offset, const float* mask,
                               const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                               float* grad_bias, float* ws, int B, int C, int H, int W, int K, int kh, int kw, int sh, int sw, int ph, int pw,
                               int dh, int dw, int group, int deformable_group, void* stream) {
  dpf_clear_error();
  (void)bias;
  if (!input || !weight || !offset || !grad_output || !ws || (grad_mask && !mask)) return DPF_ERR_INVALID_ARG;
  DcnP p{};
  int rc = fill_params2(p, B, C, H, W, K, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
  if (rc != DPF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int det = dpf_deterministic();
  const Dcn2Ws m = ws_map2(B, C, H, W, K, p.T, det);
  if (det && (reinterpret_cast<uintptr_t>(ws) & 7)) return DPF_ERR_INVALID_ARG;
  const long long in_elems = (long long)B * C * H * W, dw_elems = (long long)K * (C / group) * p.T;
  // the accumulated results and, in deterministic mode, their integer shadows start from zero
  long long *gi_shadow = nullptr, *dw_shadow = nullptr;
  if (grad_input) {
    if (hipMemsetAsync(grad_input, 0, sizeof(float) * in_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    if (det) {
      gi_shadow = reinterpret_cast<long long*>(ws + m.gi_shadow);
      if (hipMemsetAsync(gi_shadow, 0, sizeof(long long) * 2 * (size_t)in_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    }
  }
  if (grad_weight) {
    if (hipMemsetAsync(grad_weight, 0, sizeof(float) * dw_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    if (det) {
      dw_shadow = reinterpret_cast<long long*>(ws + m.dw_shadow);
      if (hipMemsetAsync(dw_shadow, 0, sizeof(long long) * 2 * (size_t)dw_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    }
  }
  rc = dcn_gather_backward(2, p, group, deformable_group, input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, ws,
                           m.dw_shadow, dw_shadow, gi_shadow, C, st);
  if (rc != DPF_OK) return rc;
  if (gi_shadow) dcn_finalize(gi_shadow, grad_input, in_elems, st);
  if (dw_shadow) dcn_finalize(dw_shadow, grad_weight, dw_elems, st);
  if (grad_bias) {
    if (hipMemsetAsync(grad_bias, 0, sizeof(float) * K, st) != hipSuccess) return DPF_ERR_LAUNCH;
    // plain sum of grad_output per channel; dpf_channel_sum takes at most 65535 (image, channel) rows per launch and adds into its
    // result, so a batch beyond that (B >= 256 at K = 256) goes in slices of whole images -- no limit on B, one launch below it
    const int nb = 65535 / K;
    for (int b0 = 0; b0 < B; b0 += nb) {
      rc = dpf_channel_sum(grad_output + (long long)b0 * K * p.P, grad_bias, B - b0 < nb ? B - b0 : nb, K, p.P, stream);
      if (rc != DPF_OK) return rc;
    }
  }
  return dpf_check_launch();
}

}  // extern "C"
