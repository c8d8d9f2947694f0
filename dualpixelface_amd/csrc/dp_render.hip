// Dual-pixel image formation (ops.dp_render; option key dp_render, dualpixelface_amd/dp_render.py): the two half-aperture views of an
// all-in-focus image under a signed defocus disparity d.  Every scene point spreads over a blur disc of radius r = rho |d| - 0.5; the
// reference view sees it through one half of the disc, the target view through the other, and the halves swap with the sign of d.
// The definition is this project's own (include/dpf_hip.h), next to the refocus one whose disc it shares.
//
//   plan      cells    c = sign(d) clamp(rho |d| - 0.5, 0, max_radius) per pixel, and per 16 x 16 cell the largest r = |c|, the extremes of
//                      c and one partial row (finite pixels, clamped pixels)                                               1 launch
//             fold     one workgroup per sample folds the rows in a fixed order (dpf_reduce.h) and the extremes into the stats     1 launch
//   render    one workgroup per 16 x 16 output tile and BOTH views.  It takes R_tile from the cells its halo touches -- the SOURCES'
//             radii, as refocus.hip does --, stages the halo of linear RGB, c and near_sign d in LDS once and gathers from there, one
//             receiver per lane, a (2 R_tile + 1)^2 window, two weight sums and six colour sums                            1 launch
//
// The plan's fp32 expressions are written operation by operation and the file is compiled with -ffp-contract=off, so
// tests/dp_render_cpu.py restates them in numpy bit for bit.  No atomics, every sum in a fixed order: the bits repeat.
#include "dpf_common.h"
#include "dpf_image.h"
#include "dpf_reduce.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kCell = 16;                      // the side of a cell of the plan and of a tile of the render
constexpr int kStats = 8;
constexpr int kMaxRadius = 32;
constexpr int kMaxBatch = 65535;               // B rides on gridDim.z, the cell rows on gridDim.y
constexpr float kPi = 3.14159265358979323846f;

struct Work {         // the workspace
  double* part;       // [B][cy][cx][2] per cell: finite pixels, pixels clamped at max_radius
  float* cellmax;     // [B][cy][cx] the largest r of a cell
  float* cellext;     // [B][cy][cx][2] the largest c and the largest -c of a cell
  int cxn, cyn;
};

struct Plan {
  const float* d;
  int H, W, maxr;
  float rho;
  float* radius;
  double* stats;
};

// grid (cx, cy, B): the signed blur radius of a cell's pixels, the cell's maxima and its counts
__global__ __launch_bounds__(256) void cells_kernel(Plan p, Work w) {
  __shared__ float sm[3][kDpfRedWaves];
  const int s = blockIdx.z, t = threadIdx.x;
  const int x = blockIdx.x * kCell + (t & 15), y = blockIdx.y * kCell + (t >> 4);
  const float lim = (float)p.maxr;
  float r = 0.f, hi = -INFINITY, lo = -INFINITY;
  double acc[2] = {0.0, 0.0};
  if (x < p.W && y < p.H) {
    const size_t i = ((size_t)s * p.H + y) * p.W + x;
    const float d = p.d[i];
    float c = 0.f;
    if (dpf_finite_f(d)) {
      const float wide = p.rho * fabsf(d) - 0.5f;
      r = fminf(fmaxf(wide, 0.f), lim);
      if (r > 0.f) c = d < 0.f ? -r : r;         // r == 0 leaves +0, never -0
      acc[0] = 1.0, acc[1] = wide > lim ? 1.0 : 0.0;
    }
    p.radius[i] = c;
    hi = c, lo = -c;
  }
  r = dpf_wave_max(r), hi = dpf_wave_max(hi), lo = dpf_wave_max(lo);
  if ((t & 63) == 0) sm[0][t >> 6] = r, sm[1][t >> 6] = hi, sm[2][t >> 6] = lo;
  const size_t cell = ((size_t)s * w.cyn + blockIdx.y) * w.cxn + blockIdx.x;
  dpf_block_reduce_d<2>(acc, w.part + cell * 2);   // (its barriers also publish sm)
  if (t >= 3) return;
  const float m = fmaxf(fmaxf(sm[t][0], sm[t][1]), fmaxf(sm[t][2], sm[t][3]));
  if (t == 0) w.cellmax[cell] = m;
  else w.cellext[cell * 2 + (t - 1)] = m;
}

// grid (B): the stats of a sample
__global__ __launch_bounds__(256) void fold_kernel(Plan p, Work w) {
  __shared__ double tot[2], ext[2];
  const int s = blockIdx.x;
  const long long cells = (long long)w.cxn * w.cyn;
  dpf_fold_rows_d<2>(w.part + (size_t)s * cells * 2, cells, 2, tot);
  const float* ce = w.cellext + (size_t)s * cells * 2;
  double acc[2] = {-(double)INFINITY, -(double)INFINITY};
  for (long long k = threadIdx.x; k < cells; k += kBlock) {
    acc[0] = fmax(acc[0], (double)ce[2 * k]);
    acc[1] = fmax(acc[1], (double)ce[2 * k + 1]);
  }
  dpf_block_reduce_d<0, 2>(acc, ext);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = p.stats + (size_t)s * kStats;
    out[0] = tot[0], out[1] = tot[1], out[2] = -ext[1], out[3] = ext[0];
    out[4] = 0.0, out[5] = 0.0, out[6] = 0.0, out[7] = 0.0;
  }
}

struct Render {
  const float *image, *radius, *d, *cellmax;
  DpfNorm nm;
  int in_normalised, out_normalised, H, W, cxn, cyn, maxr;
  float gamma, inv_gamma, ux, uy, ns;
  float *ref, *tgt;
};

// the halo of a tile at window R, laid out as in refocus.hip: a row pitch that is 16 mod 32 floats, so that the four rows of 16 lanes a
// wave reads at once fall on 64 different banks
__host__ __device__ inline int halo_side(int R) { return kCell + 2 * R; }
__host__ __device__ inline int halo_pitch(int R) { return ((2 * R + 31) / 32) * 32 + kCell; }
__host__ __device__ inline size_t halo_bytes(int R) {
  return (size_t)halo_side(R) * halo_pitch(R) * 20 + (size_t)(R + 1) * (R + 1) * 4;
}

// the encoded value in [0, 1] of channel c at a pixel
__device__ __forceinline__ float encoded_of(const Render& a, size_t at, int c) {
  const float x = a.image[at];
  const float e = a.in_normalised ? x * a.nm.std[c] + a.nm.mean[c] : x;
  return fminf(fmaxf(e, 0.f), 1.f);
}

// grid (cx, cy, B): one output tile of both views per workgroup, one receiver per lane
__global__ __launch_bounds__(256) void render_kernel(Render a) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int Rs;
  const int s = blockIdx.z, t = threadIdx.x;
  const int x0 = blockIdx.x * kCell, y0 = blockIdx.y * kCell;
  const size_t HW = (size_t)a.H * a.W;
  if (t < 64) {                                  // wave 0: the largest radius among the sources that can reach this tile
    const int hc = (a.maxr + kCell - 1) / kCell, side = 2 * hc + 1;        // at most 5 x 5 cells
    float val = 0.f;
    int reach = 1 << 30;                         // the smallest |q - p|_inf between a pixel of that cell and one of this tile
    if (t < side * side) {
      const int dcx = t % side - hc, dcy = t / side - hc;
      const int cx = (int)blockIdx.x + dcx, cy = (int)blockIdx.y + dcy;
      if (cx >= 0 && cx < a.cxn && cy >= 0 && cy < a.cyn) {
        val = a.cellmax[((size_t)s * a.cyn + cy) * a.cxn + cx];
        const int ax = dcx < 0 ? -dcx : dcx, ay = dcy < 0 ? -dcy : dcy;
        const int gx = ax ? (ax - 1) * kCell + 1 : 0, gy = ay ? (ay - 1) * kCell + 1 : 0;
        reach = gx > gy ? gx : gy;
      }
    }
    int R = a.maxr;
    for (;;) {                                   // a source further than R away counts only while some nearer one keeps R that large
      const float m = dpf_wave_max(reach <= R ? val : 0.f);
      const int next = min(R, (int)ceilf(m));
      if (next == R) break;
      R = next;
    }
    if (t == 0) Rs = R;
  }
  __syncthreads();
  const int R = Rs, n = halo_side(R), P = halo_pitch(R);
  f32x4* A = reinterpret_cast<f32x4*>(smem);     // linear R, G, B and the signed c (0 with black: contributes to nobody but itself)
  float* D = smem + (size_t)n * P * 4;           // near_sign d: a source is behind a receiver iff its value is smaller
  float* tab = D + (size_t)n * P;                // |q - p|_2 of the offsets 0 .. R
  for (int i = t; i < n * n; i += kBlock) {
    const int ly = i / n, lx = i - ly * n;
    const int gx = x0 + lx - R, gy = y0 + ly - R;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    float sd = 0.f;
    if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
      const size_t at = (size_t)gy * a.W + gx;
      const float d = a.d[(size_t)s * HW + at];
      if (dpf_finite_f(d)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float e = encoded_of(a, ((size_t)s * 3 + c) * HW + at, c);
          v[c] = a.gamma == 1.f ? e : powf(e, a.gamma);
        }
        v[3] = a.radius[(size_t)s * HW + at];
        sd = a.ns * d;
      }
    }
    A[ly * P + lx] = v;
    D[ly * P + lx] = sd;
  }
  for (int i = t; i < (R + 1) * (R + 1); i += kBlock) {
    const int dy = i / (R + 1), dx = i - dy * (R + 1);
    tab[i] = sqrtf((float)(dx * dx + dy * dy));
  }
  __syncthreads();
  const int px = t & 15, py = t >> 4;
  const int x = x0 + px, y = y0 + py;
  if (x >= a.W || y >= a.H) return;
  const int centre = (py + R) * P + px + R;
  const float rp = fabsf(A[centre][3]), dp = D[centre];
  const bool live = dpf_finite_f(a.d[(size_t)s * HW + (size_t)y * a.W + x]);
  float Wr = 0.f, Wt = 0.f, R0 = 0.f, R1 = 0.f, R2 = 0.f, T0 = 0.f, T1 = 0.f, T2 = 0.f;
  for (int dy = -R; dy <= R; ++dy) {             // a row's taps are summed first, then the rows
    const f32x4* arow = A + centre + dy * P;
    const float* drow = D + centre + dy * P;
    const float* trow = tab + (dy < 0 ? -dy : dy) * (R + 1);
    const float ty = (float)(-dy) * a.uy;        // o = p - q: the source sits at p + (dx, dy)
    float wr = 0.f, wt = 0.f, r0 = 0.f, r1 = 0.f, r2 = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
    float ox = (float)R;
    for (int dx = -R; dx <= R; ++dx, ox -= 1.f) {
      const f32x4 q = arow[dx];
      const float dist = trow[dx < 0 ? -dx : dx];
      const float rq = fabsf(q[3]);
      const float reff = drow[dx] < dp ? fminf(rq, rp) : rq;
      const float cov = fminf(fmaxf(reff + 1.f - dist, 0.f), 1.f);
      const float base = cov * __builtin_amdgcn_rcpf(fmaxf(1.f, kPi * (reff * reff)));
      const float tt = ox * a.ux + ty;
      const float st = q[3] < 0.f ? -tt : tt;    // sigma(q) t; where c(q) = 0 the tap is the receiver itself (t = 0) or weighs nothing
      const float hr = fminf(fmaxf(0.5f - st, 0.f), 1.f);
      const float ht = fminf(fmaxf(0.5f + st, 0.f), 1.f);
      const float ar = base * hr, at = base * ht;
      wr += ar, r0 += ar * q[0], r1 += ar * q[1], r2 += ar * q[2];
      wt += at, t0 += at * q[0], t1 += at * q[1], t2 += at * q[2];
    }
    Wr += wr, R0 += r0, R1 += r1, R2 += r2;
    Wt += wt, T0 += t0, T1 += t1, T2 += t2;
  }
  // a pixel that nobody else reached in a view keeps its input value there: its own weight is all there is
  const float self = __builtin_amdgcn_rcpf(fmaxf(1.f, kPi * (rp * rp))) * 0.5f;
  const bool keep_r = !live || Wr == self, keep_t = !live || Wt == self;
  const float Sr[3] = {R0, R1, R2}, St[3] = {T0, T1, T2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t at = ((size_t)s * 3 + c) * HW + (size_t)y * a.W + x;
    float kept = a.image[at];                    // bit for bit where the output is in the input's form
    if (a.in_normalised != a.out_normalised) {
      const float v = encoded_of(a, at, c);
      kept = a.out_normalised ? (v - a.nm.mean[c]) / a.nm.std[c] : v;
    }
#pragma unroll
    for (int view = 0; view < 2; ++view) {
      float e = kept;
      if (!(view ? keep_t : keep_r)) {
        const float o = view ? St[c] / Wt : Sr[c] / Wr;
        e = a.gamma == 1.f ? o : powf(o, a.inv_gamma);
        if (a.out_normalised) e = (e - a.nm.mean[c]) / a.nm.std[c];
      }
      (view ? a.tgt : a.ref)[at] = e;
    }
  }
}

bool shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0; }
bool radius_ok(int r) { return r >= 1 && r <= kMaxRadius; }
bool shape_supported(int B, int H, int W) {
  return B <= kMaxBatch && (long long)H * W <= 0x7fffffffLL && (H + kCell - 1) / kCell <= 65535;
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

Work work_of(void* ws, int B, int H, int W, long long* bytes) {
  Work w;
  w.cxn = (W + kCell - 1) / kCell, w.cyn = (H + kCell - 1) / kCell;
  const size_t cells = (size_t)B * w.cxn * w.cyn;
  char* at = (char*)ws;
  w.part = (double*)at, at += cells * 2 * 8;
  w.cellmax = (float*)at, at += round8(cells * 4);
  w.cellext = (float*)at, at += cells * 8;
  if (bytes) *bytes = (long long)(at - (char*)ws);
  return w;
}

}  // namespace

extern "C" {

long long dpf_dp_render_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W) || !shape_supported(B, H, W)) return -1;
  long long bytes = 0;
  work_of(nullptr, B, H, W, &bytes);
  return bytes;
}

int dpf_dp_render_plan(const float* disparity, int B, int H, int W, float radius_scale, int max_radius, void* ws, long long ws_bytes,
                       float* radius, double* stats, void* stream) {
  dpf_clear_error();
  if (!shape_ok(B, H, W) || !disparity || !radius || !stats || !(radius_scale >= 0.f) || !isfinite(radius_scale) || !radius_ok(max_radius))
    return DPF_ERR_INVALID_ARG;
  if (!shape_supported(B, H, W)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, dpf_dp_render_workspace_bytes(B, H, W), 8)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const Work w = work_of(ws, B, H, W, nullptr);
  Plan p;
  p.d = disparity, p.H = H, p.W = W, p.maxr = max_radius, p.rho = radius_scale, p.radius = radius, p.stats = stats;
  hipLaunchKernelGGL(cells_kernel, dim3(w.cxn, w.cyn, B), dim3(kBlock), 0, st, p, w);
  hipLaunchKernelGGL(fold_kernel, dim3(B), dim3(kBlock), 0, st, p, w);
  return dpf_check_launch();
}

int dpf_dp_render(const float* image, int normalised, const float* norm_host, const float* disparity, const float* radius, int B, int H,
                  int W, float shift_x, float shift_y, int max_radius, int near_sign, float gamma, int output_normalised, void* ws,
                  long long ws_bytes, float* reference, float* target, void* stream) {
  dpf_clear_error();
  if (!shape_ok(B, H, W) || !image || !disparity || !radius || !reference || !target || ((normalised || output_normalised) && !norm_host) ||
      !isfinite(shift_x) || !isfinite(shift_y) || (shift_x == 0.f && shift_y == 0.f) || !radius_ok(max_radius) ||
      (near_sign != 1 && near_sign != -1) || !(gamma > 0.f) || !isfinite(gamma))
    return DPF_ERR_INVALID_ARG;
  if (!shape_supported(B, H, W)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, dpf_dp_render_workspace_bytes(B, H, W), 8)) return DPF_ERR_INVALID_ARG;
  static bool widened = false;                   // the halo at max_radius 32 is past the default limit of dynamic LDS
  if (!widened) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(render_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)halo_bytes(kMaxRadius)) != hipSuccess)
      return DPF_ERR_LAUNCH;
    widened = true;
  }
  const Work w = work_of(ws, B, H, W, nullptr);
  Render a;
  a.image = image, a.radius = radius, a.d = disparity, a.cellmax = w.cellmax;
  a.in_normalised = normalised ? 1 : 0, a.out_normalised = output_normalised ? 1 : 0;
  if (normalised || output_normalised) a.nm = dpf_norm_of(norm_host);
  else
    for (int c = 0; c < 3; ++c) a.nm.mean[c] = 0.f, a.nm.std[c] = 1.f;
  a.H = H, a.W = W, a.cxn = w.cxn, a.cyn = w.cyn, a.maxr = max_radius;
  const float len = sqrtf(shift_x * shift_x + shift_y * shift_y);      // u = shift / |shift|, once, in fp32
  a.ux = shift_x / len, a.uy = shift_y / len, a.ns = (float)near_sign;
  a.gamma = gamma, a.inv_gamma = 1.f / gamma, a.ref = reference, a.tgt = target;
  hipLaunchKernelGGL(render_kernel, dim3(w.cxn, w.cyn, B), dim3(kBlock), halo_bytes(max_radius), (hipStream_t)stream, a);
  return dpf_check_launch();
}

}  // extern "C"
