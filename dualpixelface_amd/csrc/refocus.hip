// Synthetic depth of field at evaluation time (option key refocus; dualpixelface_amd/refocus.py): the view rendered again through a
// virtual aperture, from the defocus disparity the models predict.  The definition is this project's own (include/dpf_hip.h, DESIGN.md
// section 11).
//
//   plan      sums     d of every pixel into the workspace, and per workgroup one partial row (sum of d, counted pixels)     1 launch
//             focus    one workgroup per sample folds the rows in a fixed order (dpf_reduce.h) and leaves d_f, the counted
//                      pixels, the valid flag and the near sign in the stats                                              1 launch
//             cells    c = clamp(aperture (d - d_f)) per pixel, and per 16 x 16 cell the largest r = |c| and the extremes of c   1 launch
//             extremes one workgroup per sample folds the cells' extremes into stats 4..5                                1 launch
//   render    one workgroup per 16 x 16 output tile.  It takes R_tile from the cells its halo touches -- the SOURCES' radii: a sharp
//             tile beside a blurred one still receives from it --, stages the halo of linear RGB, r and the signed d in LDS once and
//             gathers from there, one receiver per lane, a (2 R_tile + 1)^2 window                                       1 launch
//
// The plan's fp32 expressions are written operation by operation and the file is compiled with -ffp-contract=off, so
// tests/refocus_cpu.py restates them in numpy bit for bit.  No atomics, every sum in a fixed order: the bits repeat.
#include "dpf_common.h"
#include "dpf_image.h"
#include "dpf_reduce.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kCell = 16;                      // the side of a cell of the plan and of a tile of the render
constexpr int kChunk = 2048;                   // pixels a workgroup of the sums pass walks at least ...
constexpr int kMaxRows = 512;                  // ... and more once a sample would need more partial rows than this
constexpr int kStats = 8;
constexpr int kMaxRadius = 32;
constexpr int kMaxBatch = 65535;               // B rides on gridDim.z, the cell rows on gridDim.y
constexpr float kPi = 3.14159265358979323846f;
enum { kFocusMean = 0, kFocusPoint = 1, kFocusValue = 2 };
enum { kDisp = 0, kIdepth = 1, kDepth = 2 };   // the target codes of reconstruct.hip

struct Work {         // the workspace
  double* part;       // [B][rows][2] partial sums of the focus
  float* d;           // [B][H W] the defocus disparity the render orders by
  float* cellmax;     // [B][cy][cx] the largest r of a cell
  float* cellext;     // [B][cy][cx][2] the largest c and the largest -c of a cell
  int rows, per_block, cxn, cyn;
};

struct Plan {
  const float *pred, *ab, *mask;
  long long stride, HW;
  int target, H, W, mode, fx, fy, near_sign, maxr;
  double value;
  float aperture;
  float* defocus;
  double* stats;
};

// grid (rows, B): d of every pixel, and one partial row per workgroup
__global__ __launch_bounds__(256) void sums_kernel(Plan p, Work w) {
  const int s = blockIdx.y, t = threadIdx.x;
  const long long begin = (long long)blockIdx.x * w.per_block;
  const long long end = begin + w.per_block < p.HW ? begin + w.per_block : p.HW;
  const float b = p.ab ? p.ab[2 * s] : 0.f, a = p.ab ? p.ab[2 * s + 1] : 0.f;
  double acc[2] = {0.0, 0.0};
  for (long long i = begin + t; i < end; i += kBlock) {
    const float x = p.pred[(size_t)s * p.stride + (size_t)i];
    float d = x;                                 // 'disp', and 'idepth': a / z + b at z = a / (x - b) is x itself
    if (p.target == kDepth) d = a / x + b;
    w.d[(size_t)s * p.HW + (size_t)i] = d;
    const bool on = !p.mask || p.mask[(size_t)s * p.HW + (size_t)i] > 0.f;
    if (on && dpf_finite_f(d)) acc[0] += (double)d, acc[1] += 1.0;
  }
  dpf_block_reduce_d<2>(acc, w.part + ((size_t)s * w.rows + blockIdx.x) * 2);
}

// grid (B): d_f, counted pixels, valid flag and near sign of a sample
__global__ __launch_bounds__(256) void focus_kernel(Plan p, Work w) {
  __shared__ double tot[2];
  const int s = blockIdx.x;
  dpf_fold_rows_d<2>(w.part + (size_t)s * w.rows * 2, w.rows, 2, tot);
  if (threadIdx.x != 0) return;
  double df = 0.0, count = 0.0, flag = 0.0;
  if (p.mode == kFocusMean) {
    count = tot[1];
    flag = count > 0.0 ? 1.0 : 0.0;
    df = count > 0.0 ? tot[0] / count : 0.0;
  } else if (p.mode == kFocusPoint) {
    const float v = w.d[(size_t)s * p.HW + (size_t)p.fy * p.W + p.fx];
    const bool fin = dpf_finite_f(v);
    count = fin ? 1.0 : 0.0, flag = count, df = fin ? (double)v : 0.0;
  } else {
    df = p.value, flag = 1.0;
  }
  double ns = (double)p.near_sign;
  if (p.near_sign == 0) ns = p.ab && p.ab[2 * s + 1] < 0.f ? -1.0 : 1.0;
  double* out = p.stats + (size_t)s * kStats;
  out[0] = df, out[1] = count, out[2] = flag, out[3] = ns;
  out[4] = 0.0, out[5] = 0.0, out[6] = 0.0, out[7] = 0.0;
}

// grid (cx, cy, B): the signed blur radius of a cell's pixels and the cell's maxima
__global__ __launch_bounds__(256) void cells_kernel(Plan p, Work w) {
  __shared__ float sm[3][kDpfRedWaves];
  const int s = blockIdx.z, t = threadIdx.x;
  const int x = blockIdx.x * kCell + (t & 15), y = blockIdx.y * kCell + (t >> 4);
  const float df = (float)p.stats[(size_t)s * kStats];
  const float lim = (float)p.maxr;
  float r = 0.f, hi = -INFINITY, lo = -INFINITY;
  if (x < p.W && y < p.H) {
    const size_t i = (size_t)s * p.HW + (size_t)y * p.W + x;
    const float d = w.d[i];
    float c = 0.f;
    if (dpf_finite_f(d)) c = fminf(fmaxf(p.aperture * (d - df), -lim), lim);
    p.defocus[i] = c;
    r = fabsf(c), hi = c, lo = -c;
  }
  r = dpf_wave_max(r), hi = dpf_wave_max(hi), lo = dpf_wave_max(lo);
  if ((t & 63) == 0) sm[0][t >> 6] = r, sm[1][t >> 6] = hi, sm[2][t >> 6] = lo;
  __syncthreads();
  if (t >= 3) return;
  const float m = fmaxf(fmaxf(sm[t][0], sm[t][1]), fmaxf(sm[t][2], sm[t][3]));
  const size_t cell = ((size_t)s * w.cyn + blockIdx.y) * w.cxn + blockIdx.x;
  if (t == 0) w.cellmax[cell] = m;
  else w.cellext[cell * 2 + (t - 1)] = m;
}

// grid (B): stats 4..5 = the smallest and the largest c of a sample
__global__ __launch_bounds__(256) void extremes_kernel(Plan p, Work w) {
  __shared__ double tot[2];
  const int s = blockIdx.x;
  const long long cells = (long long)w.cxn * w.cyn;
  const float* ext = w.cellext + (size_t)s * cells * 2;
  double acc[2] = {-(double)INFINITY, -(double)INFINITY};
  for (long long k = threadIdx.x; k < cells; k += kBlock) {
    acc[0] = fmax(acc[0], (double)ext[2 * k]);
    acc[1] = fmax(acc[1], (double)ext[2 * k + 1]);
  }
  dpf_block_reduce_d<0, 2>(acc, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = p.stats + (size_t)s * kStats;
    out[4] = -tot[1], out[5] = tot[0];
  }
}

struct Render {
  const float *image, *defocus, *d, *cellmax;
  const double* stats;
  DpfNorm nm;
  int normalised, H, W, cxn, cyn, maxr;
  float gamma, inv_gamma, gain;
  float* out;
};

// the halo of a tile at window R: rows and columns staged, and a row pitch that is 16 mod 32 floats, so that the four rows of 16 lanes a
// wave reads at once fall on 64 different banks
__host__ __device__ inline int halo_side(int R) { return kCell + 2 * R; }
__host__ __device__ inline int halo_pitch(int R) { return ((2 * R + 31) / 32) * 32 + kCell; }
__host__ __device__ inline size_t halo_bytes(int R) {
  return (size_t)halo_side(R) * halo_pitch(R) * 20 + (size_t)(R + 1) * (R + 1) * 4;
}

// the encoded value in [0, 1] of channel c at a pixel
__device__ __forceinline__ float encoded_of(const Render& a, size_t at, int c) {
  const float x = a.image[at];
  const float e = a.normalised ? x * a.nm.std[c] + a.nm.mean[c] : x;
  return fminf(fmaxf(e, 0.f), 1.f);
}

// grid (cx, cy, B): one output tile per workgroup, one receiver per lane
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
  f32x4* A = reinterpret_cast<f32x4*>(smem);     // linear R, G, B and r (-1: contributes to nobody)
  float* D = smem + (size_t)n * P * 4;           // near_sign d: a source is behind a receiver iff its value is smaller
  float* tab = D + (size_t)n * P;                // |q - p|_2 of the offsets 0 .. R
  const float ns = (float)a.stats[(size_t)s * kStats + 3];
  for (int i = t; i < n * n; i += kBlock) {
    const int ly = i / n, lx = i - ly * n;
    const int gx = x0 + lx - R, gy = y0 + ly - R;
    f32x4 v = {0.f, 0.f, 0.f, -1.f};
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
        v[3] = fabsf(a.defocus[(size_t)s * HW + at]);
        sd = ns * d;
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
  const float rp = A[centre][3], dp = D[centre];
  float W = 0.f, S0 = 0.f, S1 = 0.f, S2 = 0.f;
  for (int dy = -R; dy <= R; ++dy) {             // a row's taps are summed first, then the rows
    const f32x4* arow = A + centre + dy * P;
    const float* drow = D + centre + dy * P;
    const float* trow = tab + (dy < 0 ? -dy : dy) * (R + 1);
    float w = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int dx = -R; dx <= R; ++dx) {
      const f32x4 q = arow[dx];
      const float dist = trow[dx < 0 ? -dx : dx];
      const float reff = drow[dx] < dp ? fminf(q[3], rp) : q[3];
      const float cov = fminf(fmaxf(reff + 1.f - dist, 0.f), 1.f);
      const float wt = cov * __builtin_amdgcn_rcpf(fmaxf(1.f, kPi * (reff * reff)));
      w += wt, s0 += wt * q[0], s1 += wt * q[1], s2 += wt * q[2];
    }
    W += w, S0 += s0, S1 += s1, S2 += s2;
  }
  // a pixel nobody else reached keeps its encoded value: its own weight is all there is
  const bool alone = rp < 0.f || W == __builtin_amdgcn_rcpf(fmaxf(1.f, kPi * (rp * rp)));
  const float S[3] = {S0, S1, S2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t at = ((size_t)s * 3 + c) * HW + (size_t)y * a.W + x;
    float e;
    if (alone) {
      e = encoded_of(a, at, c);
    } else {
      const float o = S[c] / W;
      e = a.gamma == 1.f ? o : powf(o, a.inv_gamma);
    }
    a.out[at] = fminf(fmaxf(e * a.gain, 0.f), 1.f);
  }
}

bool shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0; }
bool radius_ok(int r) { return r >= 1 && r <= kMaxRadius; }
bool shape_supported(int B, int H, int W) {
  return B <= kMaxBatch && (long long)H * W <= 0x7fffffffLL && (H + kCell - 1) / kCell <= 65535;
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

Work work_of(void* ws, int B, int H, int W, long long* bytes) {
  const long long HW = (long long)H * W;
  Work w;
  const int rows = dpf_red_rows(HW, kChunk, kMaxRows);
  const long long each = (HW + rows - 1) / rows;
  w.per_block = (int)(((each + kBlock - 1) / kBlock) * kBlock);
  w.rows = (int)((HW + w.per_block - 1) / w.per_block);
  w.cxn = (W + kCell - 1) / kCell, w.cyn = (H + kCell - 1) / kCell;
  const size_t cells = (size_t)B * w.cxn * w.cyn;
  char* at = (char*)ws;
  w.part = (double*)at, at += (size_t)B * w.rows * 2 * 8;
  w.d = (float*)at, at += round8((size_t)B * HW * 4);
  w.cellmax = (float*)at, at += round8(cells * 4);
  w.cellext = (float*)at, at += cells * 8;
  if (bytes) *bytes = (long long)(at - (char*)ws);
  return w;
}

}  // namespace

extern "C" {

long long dpf_refocus_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W) || !shape_supported(B, H, W)) return -1;
  long long bytes = 0;
  work_of(nullptr, B, H, W, &bytes);
  return bytes;
}

int dpf_refocus_plan(const float* pred, long long pred_batch_stride, int target_type, const float* ab, const float* mask, int B, int H,
                     int W, int focus_mode, int focus_x, int focus_y, double focus_value, float aperture, int max_radius, int near_sign,
                     void* ws, long long ws_bytes, float* defocus, double* stats, void* stream) {
  dpf_clear_error();
  if (!shape_ok(B, H, W) || !pred || !defocus || !stats || pred_batch_stride < (long long)H * W || target_type < kDisp ||
      target_type > kDepth || (target_type != kDisp && !ab) || focus_mode < kFocusMean || focus_mode > kFocusValue ||
      (focus_mode == kFocusPoint && (focus_x < 0 || focus_x >= W || focus_y < 0 || focus_y >= H)) || !isfinite(focus_value) ||
      !(aperture >= 0.f) || !isfinite(aperture) || !radius_ok(max_radius) || near_sign < -1 || near_sign > 1)
    return DPF_ERR_INVALID_ARG;
  if (!shape_supported(B, H, W)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, dpf_refocus_workspace_bytes(B, H, W), 8)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const Work w = work_of(ws, B, H, W, nullptr);
  Plan p;
  p.pred = pred, p.ab = ab, p.mask = mask, p.stride = pred_batch_stride, p.HW = (long long)H * W;
  p.target = target_type, p.H = H, p.W = W, p.mode = focus_mode, p.fx = focus_x, p.fy = focus_y, p.near_sign = near_sign;
  p.maxr = max_radius, p.value = focus_value, p.aperture = aperture, p.defocus = defocus, p.stats = stats;
  hipLaunchKernelGGL(sums_kernel, dim3(w.rows, B), dim3(kBlock), 0, st, p, w);
  hipLaunchKernelGGL(focus_kernel, dim3(B), dim3(kBlock), 0, st, p, w);
  hipLaunchKernelGGL(cells_kernel, dim3(w.cxn, w.cyn, B), dim3(kBlock), 0, st, p, w);
  hipLaunchKernelGGL(extremes_kernel, dim3(B), dim3(kBlock), 0, st, p, w);
  return dpf_check_launch();
}

int dpf_refocus_render(const float* image, int normalised, const float* norm_host, const float* defocus, const double* stats, int B,
                       int H, int W, int max_radius, float gamma, float gain, void* ws, long long ws_bytes, float* out, void* stream) {
  dpf_clear_error();
  if (!shape_ok(B, H, W) || !image || !defocus || !stats || !out || (normalised && !norm_host) || !radius_ok(max_radius) ||
      !(gamma > 0.f) || !isfinite(gamma) || !(gain >= 0.f) || !isfinite(gain))
    return DPF_ERR_INVALID_ARG;
  if (!shape_supported(B, H, W)) return DPF_ERR_UNSUPPORTED;
  if (!dpf_ws_ok(ws, ws_bytes, dpf_refocus_workspace_bytes(B, H, W), 8)) return DPF_ERR_INVALID_ARG;
  static bool widened = false;                   // the halo at max_radius 32 is past the default limit of dynamic LDS
  if (!widened) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(render_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)halo_bytes(kMaxRadius)) != hipSuccess)
      return DPF_ERR_LAUNCH;
    widened = true;
  }
  const Work w = work_of(ws, B, H, W, nullptr);
  Render a;
  a.image = image, a.defocus = defocus, a.d = w.d, a.cellmax = w.cellmax, a.stats = stats;
  a.normalised = normalised ? 1 : 0;
  if (normalised) a.nm = dpf_norm_of(norm_host);
  else
    for (int c = 0; c < 3; ++c) a.nm.mean[c] = 0.f, a.nm.std[c] = 1.f;
  a.H = H, a.W = W, a.cxn = w.cxn, a.cyn = w.cyn, a.maxr = max_radius;
  a.gamma = gamma, a.inv_gamma = 1.f / gamma, a.gain = gain, a.out = out;
  hipLaunchKernelGGL(render_kernel, dim3(w.cxn, w.cyn, B), dim3(kBlock), halo_bytes(max_radius), (hipStream_t)stream, a);
  return dpf_check_launch();
}

}  // extern "C"
