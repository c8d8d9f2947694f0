// Public C ABI of the dense convolution family (include/dpf_hip.h) and the two dispatch chains behind it.  Host code only: the kernels
// live in conv_wide.hip, conv_pointwise.hip, conv_igemm2.hip / conv_wgrad2.hip (LDS-DMA) and conv_igemm.hip (first generation).
#include "conv_internal.h"
#include <cstdlib>

namespace {

int g_operand_bf16 = 0;
int g_f32_x9 = -1;      // < 0: not set by dpf_set_f32_matrix_path yet, conv_env().f32_x9 holds
int g_h3_guard = 1;

int clamp_x9(int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }

int out_dim(int I, int k, int s, int p, int d) { return (I + 2 * p - (d * (k - 1) + 1)) / s + 1; }

// x [N,C,ID,IH,IW], w [K,C,kd,kh,kw] -> out [N,K,OD,OH,OW] with the extents of nn.Conv3d
DpfConvDesc forward_desc(int N, int C, int ID, int IH, int IW, int K, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int dd,
                         int dh, int dw) {
  return {N, C, K, K, 0, ID, IH, IW, out_dim(ID, kd, sd, pd, dd), out_dim(IH, kh, sh, ph, dh), out_dim(IW, kw, sw, pw, dw),
          kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw, /*transposed*/ 0, /*w[K][C][T]*/ K, C, /*mode*/ 0, /*accumulate*/ 0};
}
// x [N,C,ID,IH,IW] on the strided grid, w [C][Ktot][T] of which the first K output channels are computed -> out [N,Ktot,OD,OH,OW] with the
// caller's extents (output_padding ambiguity)
DpfConvDesc transposed_desc(int N, int C, int ID, int IH, int IW, int K, int Ktot, int OD, int OH, int OW, int kd, int kh, int kw, int sd, int sh,
                            int sw, int pd, int ph, int pw, int dd, int dh, int dw, int accumulate) {
  return {N, C, K, Ktot, 0, ID, IH, IW, OD, OH, OW, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw, /*transposed*/ 1, C, Ktot, /*mode*/ 1, accumulate};
}

bool bad_args(const void* a, const void* b, const void* c, int N, int C, int K) { return !a || !b || !c || N <= 0 || C <= 0 || K <= 0; }

// Forward and transposed convolutions.  The output channels go to the kernels in slices of 128 (4 MFMA row tiles); each slice runs on the
// first tier that takes it: a tier passes a shape on with DPF_ERR_UNSUPPORTED, any other code returns.  Only the LDS-DMA tier leaves
// BatchNorm statistics (`stats`) or adds into `out` (d.accumulate); neither is offered more than one slice, whose failure midway would
// leave half a result.
int conv_dispatch(const float* x, const float* w, const float* bias, float* out, float* ws, const DpfConvDesc& d, DpfConvStats* stats, hipStream_t st) {
  const int T = d.kd * d.kh * d.kw;
  const bool plain = !stats && !d.accumulate;
  if (!plain && d.K > 128) return DPF_ERR_UNSUPPORTED;
  if (T > DPF_CONV_MAXT)                                          // 28 ... 49 taps, 2-D: one launch for all channels
    return !stats && dpf_wide_eligible(T, d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.dd, d.dh, d.dw) ? dpf_wide_conv(x, w, bias, out, d, st)
                                                                                                        : DPF_ERR_UNSUPPORTED;
  if (T < 1) return DPF_ERR_UNSUPPORTED;
  for (int k0 = 0; k0 < d.K; k0 += 128) {
    DpfConvDesc s = d;
    s.k0 = k0;
    s.K = d.K - k0 < 128 ? d.K - k0 : 128;
    int rc = DPF_ERR_UNSUPPORTED;
    if (plain && T == 1) rc = dpf_pointwise_conv(x, w, bias, out, s, st);
    if (rc == DPF_ERR_UNSUPPORTED) rc = dpf_igemm2_conv(x, w, bias, out, ws, s, st, stats);
    if (rc == DPF_ERR_UNSUPPORTED && plain) rc = dpf_gen1_conv(x, w, bias, out, ws, s, st);
    if (rc != DPF_OK) return rc;
  }
  return DPF_OK;
}

// Weight gradient, g channels in slices of 128.  The first three tiers need the caller's scratch and reduce their partial sums in a fixed
// order; the first-generation kernel adds into dw with float atomics, so dw is cleared first unless the caller accumulates.
int wgrad_dispatch(const float* g, const float* x, float* dw, float* ws, long long ws_floats, const DpfWgradDesc& d, int accumulate, hipStream_t st) {
  const int T = d.kd * d.kh * d.kw;
  for (int k0 = 0; k0 < d.K; k0 += 128) {
    DpfWgradDesc s = d;
    s.k0 = k0;
    s.K = d.K - k0 < 128 ? d.K - k0 : 128;
    float* dwk = dw + (long long)k0 * d.C * T;
    int rc = DPF_ERR_UNSUPPORTED;
    if (ws && T == 1) rc = dpf_pointwise_wgrad(g, x, dwk, ws, ws_floats, s, accumulate, st);
    if (rc == DPF_ERR_UNSUPPORTED && ws && T > DPF_CONV_MAXT) rc = dpf_wide_wgrad(g, x, dwk, ws, ws_floats, s, accumulate, st);
    if (rc == DPF_ERR_UNSUPPORTED && ws) rc = dpf_wgrad2(g, x, dwk, ws, ws_floats, s, accumulate, st);
    if (rc == DPF_ERR_UNSUPPORTED) {
      if (!accumulate && hipMemsetAsync(dwk, 0, sizeof(float) * (size_t)s.K * d.C * T, st) != hipSuccess) return DPF_ERR_LAUNCH;
      rc = dpf_gen1_wgrad(g, x, dwk, s, st);
    }
    if (rc != DPF_OK) return rc;
  }
  return DPF_OK;
}

}  // namespace

const ConvEnv& conv_env() {
  static const ConvEnv env = [] {
    auto num = [](const char* v, int unset) { return v ? atoi(v) : unset; };
    ConvEnv e;
    e.f32_x9 = clamp_x9(num(getenv("DPF_F32_X9"), 2));
    e.igemm2 = num(getenv("DPF_IGEMM2"), 1);
    e.igemm2_tr2 = num(getenv("DPF_IGEMM2_TR2"), 1);
    e.igemm2_1x1 = num(getenv("DPF_IGEMM2_1x1"), 1);
    e.igemm3 = num(getenv("DPF_IGEMM3"), 1);
    e.igemm3_cc = num(getenv("DPF_IGEMM3_CC"), 0);
    e.igemm3_sh = num(getenv("DPF_IGEMM3_SH"), -1);
    e.igemm3_rstep = num(getenv("DPF_IGEMM3_RSTEP"), 1);
    e.igemm3_bf = num(getenv("DPF_IGEMM3_BF"), 1);
    e.g2_pz = num(getenv("DPF_G2_PZ"), 0);
    e.g2_vec_store = num(getenv("DPF_G2_VEC_STORE"), 1);
    e.wgrad2 = num(getenv("DPF_WGRAD2"), 1);
    e.w2_sw1 = num(getenv("DPF_W2_SW1"), 1);
    e.w2_rstep = num(getenv("DPF_W2_RSTEP"), 1);
    e.pointwise = num(getenv("DPF_POINTWISE"), 1);
    return e;
  }();
  return env;
}

int dpf_conv_operand_bf16() { return g_operand_bf16; }
int dpf_conv_f32_x9() { return g_f32_x9 < 0 ? conv_env().f32_x9 : g_f32_x9; }
int dpf_h3_range_guard() { return g_h3_guard; }

extern "C" {

// 0: exact fp32 operands (default); 1: the dense convolution kernels (forward, stride-1 data gradient, weight gradient) round their
// operands to bf16 (RNE) while staging them, accumulate and store in fp32.  Process-wide; the host side sets it around each launch.
int dpf_set_conv_operand_precision(int bf16) {
  g_operand_bf16 = bf16 ? 1 : 0;
  return DPF_OK;
}
int dpf_get_conv_operand_precision(void) { return g_operand_bf16; }
int dpf_set_f32_matrix_path(int split_bf16) {
  g_f32_x9 = clamp_x9(split_bf16);
  return DPF_OK;
}
int dpf_get_f32_matrix_path(void) { return dpf_conv_f32_x9(); }
// diagnostic: 0 switches the position guard of the f16-component convolutions off (round 5's behaviour) so that a test can show what it buys
int dpf_debug_set_range_guard(int on) {
  g_h3_guard = on ? 1 : 0;
  return DPF_OK;
}

// workspace (floats) needed for the repacked weights of a conv with `T` taps, `reduce` reduction channels
// and `outc` output channels
long long dpf_conv_workspace_floats(int T, int reduce, int outc) {
  const long long a = (long long)T * reduce * (((outc + 31) / 32) * 32), b = dpf_igemm2_workspace_floats(T, reduce, outc);
  return a > b ? a : b;
}

// x [N,C,ID,IH,IW], w [K,C,kd,kh,kw], bias [K] or NULL, out [N,K,OD,OH,OW]
int dpf_conv_forward(const float* x, const float* w, const float* bias, float* out, float* ws, int N, int C, int ID, int IH, int IW,
                     int K, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int dd, int dh, int dw,
                     void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (bad_args(x, w, out, N, C, K) || !ws) return DPF_ERR_INVALID_ARG;
  const DpfConvDesc d = forward_desc(N, C, ID, IH, IW, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw);
  if (d.OD <= 0 || d.OH <= 0 || d.OW <= 0) return DPF_ERR_INVALID_ARG;
  return conv_dispatch(x, w, bias, out, ws, d, nullptr, (hipStream_t)stream);
}

// dpf_conv_forward that also leaves, per position tile, the (sum, sum of squares) of every output channel in `slab`
// ([*parts_host][K][2] doubles, capacity dpf_conv_stats_slab_doubles) for the BatchNorm that follows (dpf_bn_finalize_partials): the
// separate statistics pass over the output tensor disappears.  DPF_ERR_UNSUPPORTED when the shape does not run on the LDS-DMA
// kernel (K > 128, rows not 16-byte aligned, 1x1 kernels ...): the caller then uses dpf_conv_forward + dpf_bn_stats.
long long dpf_conv_stats_slab_doubles(int N, int K, int OD, int OH, int OW) {
  return 2LL * K * ((long long)N * OD * dpf_div_up(OH, 8) * dpf_div_up(OW, 32) + 64);     // + the 64 folded rows of the finalize step
}

int dpf_conv_forward_stats(const float* x, const float* w, const float* bias, float* out, float* ws, int N, int C, int ID, int IH, int IW,
                           int K, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int dd, int dh, int dw,
                           double* slab, long long slab_doubles, int* parts_host, void* stream) {
  dpf_clear_error();
  if (bad_args(x, w, out, N, C, K) || !ws || !slab || !parts_host) return DPF_ERR_INVALID_ARG;
  const DpfConvDesc d = forward_desc(N, C, ID, IH, IW, K, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw);
  if (d.OD <= 0 || d.OH <= 0 || d.OW <= 0) return DPF_ERR_INVALID_ARG;
  DpfConvStats stats{slab, slab_doubles - 2LL * K * 64, 0};
  const int rc = conv_dispatch(x, w, bias, out, ws, d, &stats, (hipStream_t)stream);
  if (rc == DPF_OK) *parts_host = stats.parts;
  return rc;
}

// Transposed convolution.  x [N,C,ID,IH,IW] lives on the strided (small) grid, out [N,Ktot,OD,OH,OW] on the dense grid;
// (OD,OH,OW) are given by the caller (output_padding ambiguity).  w is [C][Ktot][T] in memory: a forward-conv weight
// [C(x chans = conv out), Ktot(out chans = conv in), T] when this call is that conv's data gradient, or an nn.ConvTranspose3d weight
// [C_in = C, C_out = Ktot, T].  Only the first K <= Ktot output channels are computed, the others are left untouched: data gradients
// whose trailing input channels have no consumer (the constant XYZ channels of the ANM volume).
// accumulate != 0: out += result -- the data gradients of several convolutions that read the same tensor (the three dilated branches of
// a DPBlock, modules.py:43-45) are summed in the kernel epilogue instead of by separate add passes.  DPF_ERR_UNSUPPORTED (nothing
// written) when the shape would not run on the LDS-DMA kernel: compute into a temporary and add.
int dpf_conv_transpose(const float* x, const float* w, const float* bias, float* out, float* ws, int N, int C, int ID, int IH, int IW,
                       int K, int Ktot, int OD, int OH, int OW, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                       int dd, int dh, int dw, int accumulate, void* stream) {
  dpf_clear_error();
  if (bad_args(x, w, out, N, C, K) || !ws || Ktot < K) return DPF_ERR_INVALID_ARG;
  const DpfConvDesc d = transposed_desc(N, C, ID, IH, IW, K, Ktot, OD, OH, OW, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw, accumulate ? 1 : 0);
  return conv_dispatch(x, w, bias, out, ws, d, nullptr, (hipStream_t)stream);
}

long long dpf_conv_wgrad_workspace_floats(int T, int C, int K) {
  const long long a = dpf_wgrad2_workspace_floats(T, C, K), b = T == 1 ? dpf_pointwise_wgrad_workspace_floats(C, K < 128 ? K : 128) : 0;
  const long long c = dpf_wide_wgrad_workspace_floats(T, C, K < 128 ? K : 128);
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// dW[K][C][T] = (accumulate: +=) sum g[n,k,q] * x[n,c, q*s - p + t*dil]; g [N,K,QD,QH,QW] on the small grid, x [N,C,ID,IH,IW] on the dense
// grid.  With caller scratch (dpf_conv_wgrad_workspace_floats floats) eligible shapes run the kernels with a deterministic slab reduction
// (conv_pointwise.hip, conv_wide.hip, conv_wgrad2.hip) instead of float atomics; ws == NULL: every shape runs the
// first-generation kernel (float atomics into a dw that is cleared here unless `accumulate`).
int dpf_conv_wgrad_ws(const float* g, const float* x, float* dw, float* ws, long long ws_floats, int N, int C, int ID, int IH, int IW, int K,
                      int QD, int QH, int QW, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int dd, int dh, int dw_,
                      int accumulate, void* stream) {
  dpf_clear_error();
  if (bad_args(g, x, dw, N, C, K)) return DPF_ERR_INVALID_ARG;
  const DpfWgradDesc d{N, C, K, K, 0, ID, IH, IW, QD, QH, QW, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw_};
  return wgrad_dispatch(g, x, dw, ws, ws_floats, d, accumulate, (hipStream_t)stream);
}

}  // extern "C"
