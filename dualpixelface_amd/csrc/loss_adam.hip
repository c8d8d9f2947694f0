// Training-step tail: masked smooth-L1 (up to MAXHEADS heads) + masked "cosine" normal loss, and the fused Adam update over the
// flat parameter arena.
//   loss  : reference src/loss/loss_selector.py:29-42, src/loss/depth/smoothL1.py:15-49 ('given' conversion, target
//           'disp'), src/loss/normal/cosine.py:15-53 (the per-channel, non-summed cosine of SURVEY Q11)
//   Adam  : torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-5) as configured by src/model/model_selector.py:31-34
//   SGD / RMSprop : torch.optim.SGD(lr, momentum=0.9, weight_decay=2e-4) / torch.optim.RMSprop(lr, eps=1e-5), model_selector.py:36,38
// One reduction pass over the full-resolution maps (HBM-bound, reads 4+3+1+3+1 planes once), no boolean-mask gather.
#include "dpf_common.h"

namespace {

constexpr int MAXHEADS = 8;      // DPNet trains five heads; <= 4 heads add in the same order as before (same bits)
struct LossP {
  int B, n, H, W;
  float wts[MAXHEADS];
  float lam_depth, lam_normal;
};

__device__ __forceinline__ void cosine_terms(const float p[3], const float gt[3], float sim[3], float& pn_norm, float pn[3], float gn[3],
                                             float& den, float& n2, float& m2) {
  const float np = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const float ng = sqrtf(gt[0] * gt[0] + gt[1] * gt[1] + gt[2] * gt[2]);
  pn_norm = fmaxf(np, 1e-6f);
  const float gn_norm = fmaxf(ng, 1e-6f);
#pragma unroll
  for (int c = 0; c < 3; ++c) { pn[c] = p[c] / pn_norm; gn[c] = gt[c] / gn_norm; }
  n2 = sqrtf(pn[0] * pn[0] + pn[1] * pn[1] + pn[2] * pn[2]);
  m2 = sqrtf(gn[0] * gn[0] + gn[1] * gn[1] + gn[2] * gn[2]);
  den = fmaxf(n2 * m2, 1e-6f);
#pragma unroll
  for (int c = 0; c < 3; ++c) sim[c] = fminf(fmaxf((pn[c] * gn[c]) / den, -1.f), 1.f);
}

// acc[0..n-1] = sum smoothl1 per head, acc[n] = sum (1 - sim), acc[n+1] = count
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ pd, const float* __restrict__ pnorm,
                                                          const float* __restrict__ disp, const float* __restrict__ normal,
                                                          const float* __restrict__ mask, float* __restrict__ acc, LossP p) {
  __shared__ float sm[4];
  const long long hw = (long long)p.H * p.W;
  const long long total = (long long)p.B * hw;
  float s[MAXHEADS] = {};
  float sc = 0.f, cnt = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (!(mask[i] > 0.f)) continue;
    const long long pix = i % hw;
    const long long b = i / hw;
    const float gt = p.n > 0 ? disp[i] : 0.f;
#pragma unroll
    for (int k = 0; k < MAXHEADS; ++k)
      if (k < p.n) {
        const float d = pd[(b * p.n + k) * hw + pix] - gt;
        const float ad = fabsf(d);
        s[k] += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
      }
    if (pnorm) {
      float pv[3], gv[3], sim[3], pn[3], gn[3], nn, den, n2, m2;
#pragma unroll
      for (int c = 0; c < 3; ++c) { pv[c] = pnorm[(b * 3 + c) * hw + pix]; gv[c] = normal[(b * 3 + c) * hw + pix]; }
      cosine_terms(pv, gv, sim, nn, pn, gn, den, n2, m2);
      sc += (1.f - sim[0]) + (1.f - sim[1]) + (1.f - sim[2]);
    }
    cnt += 1.f;
  }
#pragma unroll
  for (int k = 0; k < MAXHEADS; ++k) {
    if (k >= p.n) break;                                  // (block-uniform)
    const float v = dpf_block_sum_256(s[k], sm);
    if (threadIdx.x == 0) atomicAdd(&acc[k], v);
  }
  sc = dpf_block_sum_256(sc, sm);
  cnt = dpf_block_sum_256(cnt, sm);
  if (threadIdx.x == 0) { atomicAdd(&acc[p.n], sc); atomicAdd(&acc[p.n + 1], cnt); }
}

// out[0] = smoothL1_loss, out[1] = cosine_loss, out[2] = final_loss
__global__ void loss_finalize_kernel(const float* __restrict__ acc, float* __restrict__ out, LossP p, int has_normal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float M = acc[p.n + 1];
  float sl1 = 0.f;
  for (int k = 0; k < p.n; ++k) sl1 += p.wts[k] * (acc[k] / M);
  const float cs = has_normal ? acc[p.n] / (3.f * M) : 0.f;
  out[0] = sl1;
  out[1] = cs;
  out[2] = p.lam_depth * sl1 + p.lam_normal * cs;
}

__global__ void loss_backward_kernel(const float* __restrict__ pd, const float* __restrict__ pnorm, const float* __restrict__ disp,
                                     const float* __restrict__ normal, const float* __restrict__ mask, const float* __restrict__ acc,
                                     const float* __restrict__ gout /*[3] grads of (sl1, cos, final)*/, float* __restrict__ dpd,
                                     float* __restrict__ dpn, LossP p) {
  const long long hw = (long long)p.H * p.W;
  const long long total = (long long)p.B * hw;
  const float M = acc[p.n + 1];
  const float g_sl1 = gout[0] + gout[2] * p.lam_depth;
  const float g_cos = gout[1] + gout[2] * p.lam_normal;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long pix = i % hw;
    const long long b = i / hw;
    const bool on = mask[i] > 0.f;
    const float gt = p.n > 0 ? disp[i] : 0.f;
#pragma unroll
    for (int k = 0; k < MAXHEADS; ++k)
      if (k < p.n) {
        float g = 0.f;
        if (on) {
          const float d = pd[(b * p.n + k) * hw + pix] - gt;
          g = g_sl1 * p.wts[k] / M * fminf(fmaxf(d, -1.f), 1.f);
        }
        dpd[(b * p.n + k) * hw + pix] = g;
      }
    if (dpn) {
      float out3[3] = {0.f, 0.f, 0.f};
      if (on) {
        float pv[3], gv[3], sim[3], pn[3], gn[3], nn, den, n2, m2;
#pragma unroll
        for (int c = 0; c < 3; ++c) { pv[c] = pnorm[(b * 3 + c) * hw + pix]; gv[c] = normal[(b * 3 + c) * hw + pix]; }
        cosine_terms(pv, gv, sim, nn, pn, gn, den, n2, m2);
        const float gs = -g_cos / (3.f * M);   // dL/dsim_c
        // q_c = pn_c*gn_c/den, den = max(n2*m2, eps)
        float a[3] = {0.f, 0.f, 0.f};
        const bool den_live = (n2 * m2) > 1e-6f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float q = (pn[c] * gn[c]) / den;
          if (q <= -1.f || q >= 1.f) continue;   // clamp kills the gradient
          a[c] += gs * gn[c] / den;
          if (den_live && n2 > 0.f) {
            const float coef = -gs * (pn[c] * gn[c]) / (den * den) * m2 / n2;
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] += coef * pn[k];
          }
        }
        // pn = p / max(|p|, eps)
        const float np = sqrtf(pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2]);
        if (np > 1e-6f) {
          const float dot = a[0] * pn[0] + a[1] * pn[1] + a[2] * pn[2];
#pragma unroll
          for (int c = 0; c < 3; ++c) out3[c] = (a[c] - pn[c] * dot) / np;
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) out3[c] = a[c] / 1e-6f;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) dpn[(b * 3 + c) * hw + pix] = out3[c];
    }
  }
}

// One kernel serves the three entry points, so a captured replay and an eager step run the same instructions.  The three step scalars
// are arguments, or come from device memory: hyper = { lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) }, which the host refreshes before each
// replay of a captured train step, or the gradient control record (grad_ctl.hip) -- ctl[0..1] as hyper, the gradient multiplier from
// ctl[4] (gscale times the clip coefficient, written by dpf_grad_finish) and nothing at all when ctl[3] (apply) is 0: a micro-step that
// does not end its group.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n,
                            float gscale, float lr_over_bc1, float inv_sqrt_bc2, const float* __restrict__ hyper,
                            const float* __restrict__ ctl, float b1, float b2, float omb1, float omb2, float eps) {
  // The loop's first test, taken ahead of the scalar loads below.  Measured: without it the form with all three scalars as arguments takes
  // 16.1 us against the 15.8 us of a kernel that has no pointer arguments to test (arena of 3 670 492 floats), with it 15.8 us.  Supposed cause:
  // this test loads n and the grid size, which lie in both cache lines of the kernel arguments, so the loads after it find them.
  if ((long long)blockIdx.x * blockDim.x + threadIdx.x >= n) return;
  if (ctl) {
    if (ctl[3] == 0.f) return;
    lr_over_bc1 = ctl[0];
    inv_sqrt_bc2 = ctl[1];
    gscale = ctl[4];
  } else if (hyper) {
    lr_over_bc1 = hyper[0];
    inv_sqrt_bc2 = hyper[1];
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + omb1 * gi;
    const float vi = b2 * v[i] + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_over_bc1 * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
  }
}

// ---- SGD with momentum and RMSprop over the same flat arenas.  One kernel per optimiser serves both entry points (lr as an argument /
// lr in device memory), so a captured replay and an eager step run the same instructions.  fmaf is written out: the rounding of an
// element must not depend on whether it sits in the 16-byte body or in the scalar head / tail.
struct SgdOp {
  float gscale, momentum, wd;
  __device__ __forceinline__ void operator()(float& p, float g, float& buf, float lr) const {
    const float d = fmaf(wd, p, g * gscale);               // weight decay joins the already scaled gradient
    buf = fmaf(momentum, buf, d);                          // (torch seeds buf = d on the first step: 0.9 * 0 + d is the same float)
    p = fmaf(-lr, buf, p);
  }
};
struct RmsOp {
  float gscale, alpha, oma, eps;
  __device__ __forceinline__ void operator()(float& p, float g, float& sq, float lr) const {
    const float gi = g * gscale;
    sq = fmaf(alpha, sq, oma * gi * gi);
    p = p - lr * gi / (sqrtf(sq) + eps);                   // eps outside the root
  }
};

// elements [head, head + 4 * nvec) as 16-byte vectors (the host picks `head` so that all three arenas are 16-byte aligned there, or
// head = n when they cannot be), the <= 3 + 3 elements around them one by one.  live: one byte per element, 0 = leave parameter and
// state exactly as they are (nullptr: every element is live).  ctl: nullptr, or the record whose multiplier replaces op.gscale.
template <class Op>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s,
                                                    const unsigned char* __restrict__ live, long long n, long long head, float lr_arg,
                                                    const float* __restrict__ lr_dev, const float* __restrict__ ctl, Op op) {
  if (ctl) {                                               // the gradient control record (grad_ctl.hip): apply flag, multiplier
    if (ctl[3] == 0.f) return;
    op.gscale = ctl[4];
  }
  const float lr = lr_dev ? lr_dev[0] : lr_arg;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  const long long nvec = (n - head) / 4;
  for (long long v = tid; v < nvec; v += stride) {
    const long long i = head + 4 * v;
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
    f32x4 sv = *reinterpret_cast<const f32x4*>(s + i);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], sk = sv[k];
      op(pk, gv[k], sk, lr);
      if (!live || live[i + k]) { pv[k] = pk; sv[k] = sk; }   // (a dead element is stored back with the bits it was loaded with)
    }
    *reinterpret_cast<f32x4*>(p + i) = pv;
    *reinterpret_cast<f32x4*>(s + i) = sv;
  }
  const long long tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
  for (long long k = tid; k < nscalar; k += stride) {
    const long long i = k < head ? k : tail0 + (k - head);
    if (live && !live[i]) continue;
    float pk = p[i], sk = s[i];
    op(pk, g[i], sk, lr);
    p[i] = pk;
    s[i] = sk;
  }
}

// first element at which param, grad and state are all 16-byte aligned; n (= everything scalar) when they never are together
long long optim_head(const float* p, const float* g, const float* s, long long n) {
  const uintptr_t a = (uintptr_t)p & 15, b = (uintptr_t)g & 15, c = (uintptr_t)s & 15;
  if (a != b || a != c || (a & 3)) return n;
  const long long head = (long long)((16 - a) & 15) / 4;
  return head < n ? head : n;
}

template <class Op>
int optim_launch(float* p, const float* g, float* s, const unsigned char* live, long long n, double lr, const float* lr_dev, Op op, void* stream,
                 const float* ctl = nullptr) {
  hipLaunchKernelGGL(optim_kernel<Op>, dim3(dpf_ew_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, g, s, live, n, optim_head(p, g, s, n),
                     (float)lr, lr_dev, ctl, op);
  return dpf_check_launch();
}

int adam_launch(float* p, const float* g, float* m, float* v, long long n, float gscale, float lr_over_bc1, float inv_sqrt_bc2, const float* hyper,
                const float* ctl, double beta1, double beta2, double eps, void* stream) {
  hipLaunchKernelGGL(adam_kernel, dim3(dpf_ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, gscale, lr_over_bc1, inv_sqrt_bc2, hyper, ctl,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps);
  return dpf_check_launch();
}

void fill(LossP& p, int B, int n, int H, int W, const float* w, float l0, float l1) {
  p.B = B; p.n = n; p.H = H; p.W = W;
  for (int i = 0; i < MAXHEADS; ++i) p.wts[i] = i < n ? w[i] : 0.f;
  p.lam_depth = l0; p.lam_normal = l1;
}

}  // namespace

extern "C" {

// pred_depth [B,n,H,W], pred_normal [B,3,H,W] or NULL, disp/mask [B,H,W], normal [B,3,H,W].
// acc_ws: n+2 floats (kept for the backward), out: 3 device floats {smoothL1_loss, cosine_loss, final_loss}.
int dpf_loss_forward(const float* pred_depth, const float* pred_normal, const float* disp, const float* normal, const float* mask,
                     float* acc_ws, float* out, int B, int n, int H, int W, const float* head_weights_host, float lambda_depth,
                     float lambda_normal, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if ((n > 0 && !pred_depth) || (n > 0 && !disp) || !mask || !acc_ws || !out || !head_weights_host || n < 0 || n > MAXHEADS || (pred_normal && !normal)) return DPF_ERR_INVALID_ARG;
  LossP p;
  fill(p, B, n, H, W, head_weights_host, lambda_depth, lambda_normal);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(acc_ws, 0, sizeof(float) * (n + 2), st) != hipSuccess) return DPF_ERR_LAUNCH;
  // deterministic mode: ONE workgroup, so the float atomics that merge the workgroups' partial sums have no partner (dpf_common.h)
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(dpf_deterministic() ? 1 : dpf_ew_grid((long long)B * H * W)), dim3(256), 0, st, pred_depth, pred_normal, disp,
                     normal, mask, acc_ws, p);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, st, acc_ws, out, p, pred_normal ? 1 : 0);
  return dpf_check_launch();
}

// gout: 3 device floats (upstream gradients of the three outputs); d_pred_depth [B,n,H,W], d_pred_normal [B,3,H,W] or NULL
int dpf_loss_backward(const float* pred_depth, const float* pred_normal, const float* disp, const float* normal, const float* mask,
                      const float* acc_ws, const float* gout, float* d_pred_depth, float* d_pred_normal, int B, int n, int H, int W,
                      const float* head_weights_host, float lambda_depth, float lambda_normal, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if ((n > 0 && (!pred_depth || !disp || !d_pred_depth)) || !mask || !acc_ws || !gout || n < 0 || n > MAXHEADS) return DPF_ERR_INVALID_ARG;
  LossP p;
  fill(p, B, n, H, W, head_weights_host, lambda_depth, lambda_normal);
  hipLaunchKernelGGL(loss_backward_kernel, dim3(dpf_ew_grid((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, pred_depth, pred_normal,
                     disp, normal, mask, acc_ws, gout, d_pred_depth, pred_normal ? d_pred_normal : nullptr, p);
  return dpf_check_launch();
}

// One fused Adam step over a flat arena of n floats; grad is pre-scaled by gscale (1/world_size after an all-reduce SUM).
int dpf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, int step, double lr, double beta1,
                  double beta2, double eps, float gscale, void* stream) {
  dpf_clear_error();   // drop any stale error left by other runtime users (e.g. PyTorch) in this thread
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return DPF_ERR_INVALID_ARG;
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  return adam_launch(param, grad, exp_avg, exp_avg_sq, n, gscale, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), nullptr, nullptr, beta1, beta2, eps, stream);
}

// dpf_adam_step with { (float)(lr / (1 - beta1^step)), (float)(1 / sqrt(1 - beta2^step)) } supplied in device memory (hyper[2])
int dpf_adam_step_hyper(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, const float* hyper, double beta1,
                        double beta2, double eps, float gscale, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper || n <= 0) return DPF_ERR_INVALID_ARG;
  return adam_launch(param, grad, exp_avg, exp_avg_sq, n, gscale, 0.f, 0.f, hyper, nullptr, beta1, beta2, eps, stream);
}

// One SGD step (momentum, weight decay, no dampening, no Nesterov) over a flat arena of n floats: d = grad * gscale + weight_decay * param;
// buf = momentum * buf + d; param -= lr * buf.  momentum_buf starts zero-filled.  live: n bytes, 0 = the element belongs to a parameter
// that received no gradient this step and is left untouched, state included (torch skips .grad is None); NULL = all live.
int dpf_sgd_step(float* param, const float* grad, float* momentum_buf, const unsigned char* live, long long n, double lr, double momentum,
                 double weight_decay, float gscale, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !momentum_buf || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, momentum_buf, live, n, lr, nullptr, SgdOp{gscale, (float)momentum, (float)weight_decay}, stream);
}

// dpf_sgd_step with (float)lr read from device memory (lr_dev[0]): the launch a captured train step replays while the schedule moves on
int dpf_sgd_step_lr(float* param, const float* grad, float* momentum_buf, const unsigned char* live, long long n, const float* lr_dev,
                    double momentum, double weight_decay, float gscale, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !momentum_buf || !lr_dev || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, momentum_buf, live, n, 0.0, lr_dev, SgdOp{gscale, (float)momentum, (float)weight_decay}, stream);
}

// One RMSprop step (no momentum, not centred, no weight decay): sq = alpha * sq + (1 - alpha) * (grad * gscale)^2;
// param -= lr * grad * gscale / (sqrt(sq) + eps).  square_avg starts zero-filled.
int dpf_rmsprop_step(float* param, const float* grad, float* square_avg, long long n, double lr, double alpha, double eps, float gscale,
                     void* stream) {
  dpf_clear_error();
  if (!param || !grad || !square_avg || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, square_avg, nullptr, n, lr, nullptr, RmsOp{gscale, (float)alpha, (float)(1.0 - alpha), (float)eps}, stream);
}

// dpf_rmsprop_step with (float)lr read from device memory (lr_dev[0])
int dpf_rmsprop_step_lr(float* param, const float* grad, float* square_avg, long long n, const float* lr_dev, double alpha, double eps,
                        float gscale, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !square_avg || !lr_dev || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, square_avg, nullptr, n, 0.0, lr_dev, RmsOp{gscale, (float)alpha, (float)(1.0 - alpha), (float)eps}, stream);
}

// The three steps behind the gradient control record (grad_ctl.hip; ctl: DPF_GRAD_CTL_FLOATS device floats): the per-step scalars come
// from ctl[0..1] (Adam's two floats; lr for the others), the gradient multiplier from ctl[4] in place of gscale, and with ctl[3] == 0
// the launch leaves every element of every arena as it is.
int dpf_adam_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, const float* ctl, double beta1,
                      double beta2, double eps, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ctl || n <= 0) return DPF_ERR_INVALID_ARG;
  return adam_launch(param, grad, exp_avg, exp_avg_sq, n, 1.f, 0.f, 0.f, nullptr, ctl, beta1, beta2, eps, stream);
}

int dpf_sgd_step_ctl(float* param, const float* grad, float* momentum_buf, const unsigned char* live, long long n, const float* ctl,
                     double momentum, double weight_decay, void* stream) {
  dpf_clear_error();
  if (!param || !grad || !momentum_buf || !ctl || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, momentum_buf, live, n, 0.0, ctl, SgdOp{1.f, (float)momentum, (float)weight_decay}, stream, ctl);
}

int dpf_rmsprop_step_ctl(float* param, const float* grad, float* square_avg, long long n, const float* ctl, double alpha, double eps,
                         void* stream) {
  dpf_clear_error();
  if (!param || !grad || !square_avg || !ctl || n <= 0) return DPF_ERR_INVALID_ARG;
  return optim_launch(param, grad, square_avg, nullptr, n, 0.0, ctl, RmsOp{1.f, (float)alpha, (float)(1.0 - alpha), (float)eps}, stream, ctl);
}

}  // extern "C"
