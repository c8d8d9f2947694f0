// The geometric-normal loss (loss_type 'normal_geo'; losses.NORMAL_GEOLoss, ops.normal_geo_loss): the normals of
// the PREDICTED depth against the target normals, with a hand-written gradient into the prediction.  The geometry is reconstruct.hip's
// (dpf_geometry.h), and like it every fp32 expression is written operation by operation under -ffp-contract=off, so that
// tests/normal_geo_cpu.py restates the forward bit for bit.
//
//   z_p      a / (pred - b) (target types 0, 1) or pred (2), non-finite -> 0
//   usable   z_t finite and > 0, mask NULL or > 0, z_p > 0, K regular; z_p and z_t of a pixel that is not usable read 0
//   stencil  neighbours at distance S = step along each axis; connectivity from z_t (so it does not move with the prediction), the step
//            vector (z_to - z_from) r_to + (z_from D) Kinv[:, axis] from z_p; D = 2 S central, S one-sided
//   n        (d_row x d_col) / |.|, negated to face the camera (n . z_p r <= 0) when towards_camera, away from it otherwise
//   g        target_signs * normal, g^ = g / |g|
//   counted  usable, both axes have a step, |c| > 0 and finite, |g| > 1e-6 and finite
//   term     1 - clamp(n . g^, -1, 1);  loss = sum_h w_h (sum terms_h / count_h), 0 for a head with count_h = 0
//
// Forward: one workgroup per 32 x 8 tile of one head of one sample, z_p and z_t in LDS with a halo of S; it leaves one row (term sum,
// count) of fp64 in the workspace, and one workgroup folds the rows head by head (dpf_reduce.h) into the loss and the stats record.
// Backward: a gather.  The workgroup first evaluates the centres of its tile AND of a halo of S around it from z tiles with a halo of 2 S
// -- each centre's derivative with respect to the (up to) two depths of its row step and the two of its column step goes to LDS, zeros
// for a centre that is not counted -- then every pixel adds, in the fixed order centre, left, right, up, down, what those five centres
// owe it and writes its element of d pred (0 where nothing does, or the pixel is not usable).  Neighbouring centres are recomputed by
// the workgroups on both sides of a tile edge, from the same inputs by the same instructions, so nothing is exchanged between
// workgroups: no scratch, no atomics, and the bits repeat.  Validity, connectivity, the choice of step and the orientation sign are
// constants of the derivative; the clamp passes the gradient on [-1, 1].
#include "dpf_common.h"
#include "dpf_geometry.h"
#include "dpf_head_loss.h"
#include <math.h>

extern "C" long long dpf_normal_geo_workspace_bytes(int B, int n, int H, int W);

namespace {

constexpr int kBlock = 256;
constexpr int kTW = kDpfTileW, kTH = kDpfTileH;      // output tile, one pixel per thread (dpf_head_loss.h has the plan)

struct Geo {
  const float* pred;       // [B, n, H, W]
  const float* depth;      // [B, H, W]   z_t
  const float* normal;     // [B, 3, H, W]
  const float* Kmat;       // [B, 3, 3]
  const float* ab;         // [B, 2] or NULL (target type 2)
  const float* mask;       // [B, H, W] or NULL
  int n, H, W, target_type, towards;
  float ratio;
  float sg[3];
};

// z_p and z_t of pixel (y, x) where it is usable, else 0 and 0; outside the image 0 and 0
__device__ __forceinline__ void usable_depths(const Geo& g, const Cam& cam, const float* __restrict__ predh, size_t sbase, int y, int x,
                                              float& zp, float& zt) {
  zp = 0.f, zt = 0.f;
  if (y < 0 || y >= g.H || x < 0 || x >= g.W) return;
  const size_t o = (size_t)y * g.W + x;
  const float p = predh[o];
  float z = g.target_type == 2 ? p : cam.a / (p - cam.b);
  if (!isfinite(z)) z = 0.f;
  const float t = g.depth[sbase + o];
  bool ok = cam.ok && z > 0.f && dpf_finite_f(t) && t > 0.f;
  if (g.mask) ok = ok && g.mask[sbase + o] > 0.f;
  if (ok) zp = z, zt = t;
}

// reconstruct.hip's step_of with the two decisions taken by the caller (from z_t) and neighbours S apart: fs = (float)S
__device__ __forceinline__ void step_vec(const Cam& cam, int col, bool cm, bool cp, float zm, float zc, float zq, const float (&rc)[3],
                                         const float (&rq)[3], float fs, float (&d)[3], float (&rto)[3], float& delta) {
  const float zfrom = cm ? zm : zc, zto = cp ? zq : zc;
  delta = cm && cp ? 2.f * fs : fs;
  const float dz = zto - zfrom, t = zfrom * delta;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rto[k] = cp ? rq[k] : rc[k];
    d[k] = dz * rto[k] + t * cam.inv[3 * k + col];
  }
}

struct Centre {
  float n[3];          // the oriented unit normal (0 where not counted)
  float cosv;          // n . g^ before the clamp
  float gh[3];         // g^
  float drow[3], dcol[3], rtor[3], rtoc[3];
  float len, sigma, deltar, deltac;
};

// The centre (y, x) of the image from the depths of its stencil: zp*, zt* at the centre (c), left (l), right (r), up (u), down (d).
// -> counted
template <int S>
__device__ __forceinline__ bool centre_of(const Geo& g, const Cam& cam, size_t sbase, int y, int x, float zpc, float zpl, float zpr, float zpu,
                                          float zpd, float ztc, float ztl, float ztr, float ztu, float ztd, Centre& c) {
  c.n[0] = c.n[1] = c.n[2] = 0.f;
  if (!(zpc > 0.f)) return false;
  const bool cl = connected(ztl, ztc, g.ratio), cr = connected(ztc, ztr, g.ratio);
  const bool cu = connected(ztu, ztc, g.ratio), cd = connected(ztc, ztd, g.ratio);
  if (!((cl || cr) && (cu || cd))) return false;
  float rc[3], rr[3], rd[3];
  ray_of(cam, y, x, rc);
  ray_of(cam, y, x + S, rr);
  ray_of(cam, y + S, x, rd);
  step_vec(cam, 0, cl, cr, zpl, zpc, zpr, rc, rr, (float)S, c.drow, c.rtor, c.deltar);
  step_vec(cam, 1, cu, cd, zpu, zpc, zpd, rc, rd, (float)S, c.dcol, c.rtoc, c.deltac);
  const float cx = c.drow[1] * c.dcol[2] - c.drow[2] * c.dcol[1];
  const float cy = c.drow[2] * c.dcol[0] - c.drow[0] * c.dcol[2];
  const float cz = c.drow[0] * c.dcol[1] - c.drow[1] * c.dcol[0];
  const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
  if (!(len > 0.f && isfinite(len))) return false;
  const size_t HW = (size_t)g.H * g.W, o = (size_t)y * g.W + x;
  const float* N = g.normal + 3 * sbase + o;
  const float gx = g.sg[0] * N[0], gy = g.sg[1] * N[HW], gz = g.sg[2] * N[2 * HW];
  const float glen = sqrtf((gx * gx + gy * gy) + gz * gz);
  if (!(glen > 1e-6f && isfinite(glen))) return false;
  float n0 = cx / len, n1 = cy / len, n2 = cz / len;
  const float dot = (n0 * (zpc * rc[0]) + n1 * (zpc * rc[1])) + n2 * (zpc * rc[2]);
  c.sigma = 1.f;
  if (g.towards ? dot > 0.f : dot < 0.f) {
    n0 = -n0, n1 = -n1, n2 = -n2;
    c.sigma = -1.f;
  }
  c.n[0] = n0, c.n[1] = n1, c.n[2] = n2;
  c.gh[0] = gx / glen, c.gh[1] = gy / glen, c.gh[2] = gz / glen;
  c.cosv = (n0 * c.gh[0] + n1 * c.gh[1]) + n2 * c.gh[2];
  c.len = len;
  return true;
}

// grid (ceil(W / 32), ceil(H / 8), B n), 256 threads = 8 rows x 32 columns.  part: [n][B tiles][2]
template <int S>
__global__ __launch_bounds__(256) void geo_forward_kernel(Geo g, double* __restrict__ part, float* __restrict__ normal_out,
                                                          unsigned char* __restrict__ counted_out) {
  constexpr int LW = kTW + 2 * S, LH = kTH + 2 * S;
  __shared__ Cam scam;
  __shared__ float tp[LH][LW], tt[LH][LW];
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  if (t == 0) cam_setup(g.Kmat, g.ab, g.target_type, s, &scam);
  __syncthreads();
  const Cam cam = scam;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  for (int i = t; i < LH * LW; i += kBlock) {
    const int ly = i / LW, lx = i - ly * LW;
    usable_depths(g, cam, predh, sbase, y0 - S + ly, x0 - S + lx, tp[ly][lx], tt[ly][lx]);
  }
  __syncthreads();
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  double acc[2] = {0.0, 0.0};
  if (x < g.W && y < g.H) {
    const int ly = ty + S, lx = tx + S;
    Centre c;
    const bool counted = centre_of<S>(g, cam, sbase, y, x, tp[ly][lx], tp[ly][lx - S], tp[ly][lx + S], tp[ly - S][lx], tp[ly + S][lx],
                                      tt[ly][lx], tt[ly][lx - S], tt[ly][lx + S], tt[ly - S][lx], tt[ly + S][lx], c);
    if (counted) {
      const float cl = fminf(fmaxf(c.cosv, -1.f), 1.f);
      acc[0] = (double)(1.f - cl);
      acc[1] = 1.0;
    }
    if (normal_out) {
      const size_t o = (size_t)y * g.W + x;
      float* N = normal_out + ((size_t)s * g.n + h) * 3 * HW;
      N[o] = c.n[0];
      N[o + HW] = c.n[1];
      N[o + 2 * HW] = c.n[2];
      counted_out[((size_t)s * g.n + h) * HW + o] = counted ? 1 : 0;
    }
  }
  dpf_block_reduce_d<2>(acc, part + dpf_tile_part_row(s, h, g.n) * 2);
}

// grid as the forward's.  coef: per centre of the tile and its halo of S the derivative of its term with respect to the depth its row
// step ends at [0] and starts from [1], and its column step ends at [2] and starts from [3]
template <int S>
__global__ __launch_bounds__(256) void geo_backward_kernel(Geo g, DpfHeadW hw, const double* __restrict__ stats, const float* __restrict__ gout,
                                                           float* __restrict__ dpred) {
  constexpr int ZW = kTW + 4 * S, ZH = kTH + 4 * S;       // z tiles: halo 2 S
  constexpr int CW = kTW + 2 * S, CH = kTH + 2 * S;       // centres: halo S
  __shared__ Cam scam;
  __shared__ float tp[ZH][ZW], tt[ZH][ZW];
  __shared__ float coef[4][CH][CW];
  const int t = threadIdx.x;
  const int s = blockIdx.z / g.n, h = blockIdx.z - s * g.n;
  if (t == 0) cam_setup(g.Kmat, g.ab, g.target_type, s, &scam);
  __syncthreads();
  const Cam cam = scam;
  const size_t HW = (size_t)g.H * g.W, sbase = (size_t)s * HW;
  const float* __restrict__ predh = g.pred + ((size_t)s * g.n + h) * HW;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  for (int i = t; i < ZH * ZW; i += kBlock) {
    const int ly = i / ZW, lx = i - ly * ZW;
    usable_depths(g, cam, predh, sbase, y0 - 2 * S + ly, x0 - 2 * S + lx, tp[ly][lx], tt[ly][lx]);
  }
  __syncthreads();
  for (int i = t; i < CH * CW; i += kBlock) {
    const int cy = i / CW, cx = i - cy * CW;
    const int y = y0 - S + cy, x = x0 - S + cx;
    const int ly = cy + S, lx = cx + S;
    float a_row = 0.f, b_row = 0.f, a_col = 0.f, b_col = 0.f;
    Centre c;
    // (a centre outside the image has z_p = 0 and is not counted: its rays and its target normal are never formed)
    if (centre_of<S>(g, cam, sbase, y, x, tp[ly][lx], tp[ly][lx - S], tp[ly][lx + S], tp[ly - S][lx], tp[ly + S][lx], tt[ly][lx],
                     tt[ly][lx - S], tt[ly][lx + S], tt[ly - S][lx], tt[ly + S][lx], c) &&
        c.cosv >= -1.f && c.cosv <= 1.f) {
      // term = 1 - sigma (c . g^) / |c|:  d term / d c = -sigma (g^ - n cos) / |c|
      float gc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) gc[k] = -(c.sigma * (c.gh[k] - c.n[k] * c.cosv)) / c.len;
      // c = d_row x d_col:  d / d d_row = d_col x gc,  d / d d_col = gc x d_row
      const float gr[3] = {c.dcol[1] * gc[2] - c.dcol[2] * gc[1], c.dcol[2] * gc[0] - c.dcol[0] * gc[2], c.dcol[0] * gc[1] - c.dcol[1] * gc[0]};
      const float gq[3] = {gc[1] * c.drow[2] - gc[2] * c.drow[1], gc[2] * c.drow[0] - gc[0] * c.drow[2], gc[0] * c.drow[1] - gc[1] * c.drow[0]};
      // d = (z_to - z_from) r_to + (z_from D) Kinv[:, axis]:  d d / d z_to = r_to,  d d / d z_from = D Kinv[:, axis] - r_to
      a_row = (gr[0] * c.rtor[0] + gr[1] * c.rtor[1]) + gr[2] * c.rtor[2];
      b_row = (gr[0] * (c.deltar * cam.inv[0] - c.rtor[0]) + gr[1] * (c.deltar * cam.inv[3] - c.rtor[1])) +
              gr[2] * (c.deltar * cam.inv[6] - c.rtor[2]);
      a_col = (gq[0] * c.rtoc[0] + gq[1] * c.rtoc[1]) + gq[2] * c.rtoc[2];
      b_col = (gq[0] * (c.deltac * cam.inv[1] - c.rtoc[0]) + gq[1] * (c.deltac * cam.inv[4] - c.rtoc[1])) +
              gq[2] * (c.deltac * cam.inv[7] - c.rtoc[2]);
    }
    coef[0][cy][cx] = a_row;
    coef[1][cy][cx] = b_row;
    coef[2][cy][cx] = a_col;
    coef[3][cy][cx] = b_col;
  }
  __syncthreads();
  const int tx = t & (kTW - 1), ty = t / kTW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= g.W || y >= g.H) return;                        // (no barrier below)
  const int ly = ty + 2 * S, lx = tx + 2 * S, cy = ty + S, cx = tx + S;
  const float zpc = tp[ly][lx], ztc = tt[ly][lx];
  float out = 0.f;
  if (zpc > 0.f) {
    const bool cl = connected(tt[ly][lx - S], ztc, g.ratio), cr = connected(ztc, tt[ly][lx + S], g.ratio);
    const bool cu = connected(tt[ly - S][lx], ztc, g.ratio), cd = connected(ztc, tt[ly + S][lx], g.ratio);
    // the centre's own steps end at it where there is no neighbour after it, and start from it where there is none before it
    float sum = cr ? 0.f : coef[0][cy][cx];
    sum = sum + (cl ? 0.f : coef[1][cy][cx]);
    sum = sum + (cd ? 0.f : coef[2][cy][cx]);
    sum = sum + (cu ? 0.f : coef[3][cy][cx]);
    sum = sum + (cl ? coef[0][cy][cx - S] : 0.f);           // the left centre's row step ends here
    sum = sum + (cr ? coef[1][cy][cx + S] : 0.f);           // the right centre's starts here
    sum = sum + (cu ? coef[2][cy - S][cx] : 0.f);           // the upper centre's column step ends here
    sum = sum + (cd ? coef[3][cy + S][cx] : 0.f);           // the lower centre's starts here
    const double cnt = stats[h];
    const float wk = cnt > 0.0 ? (float)((double)hw.w[h] / cnt) : 0.f;
    float dz = 1.f;                                         // d z_p / d pred = -z_p / (pred - b)
    if (g.target_type != 2) dz = -(zpc / (predh[(size_t)y * g.W + x] - cam.b));
    out = ((sum * dz) * wk) * gout[0];
  }
  dpred[((size_t)s * g.n + h) * HW + (size_t)y * g.W + x] = out;
}

// argument checks shared by the entry points; fills g and hw
int prepare(const float* pred, const float* depth, const float* normal, const float* Kmat, const float* ab, const float* mask, int B, int n,
            int H, int W, int target_type, float ratio, int step, int towards, const float* signs, const float* weights, Geo& g, DpfHeadW& hw) {
  if (!pred || !depth || !normal || !Kmat || !signs || !weights || B <= 0 || n < 1 || n > kDpfMaxHeads || H <= 0 || W <= 0 || target_type < 0 ||
      target_type > 2 || (target_type != 2 && !ab) || !(ratio > 0.f) || step < 1)
    return DPF_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k)
    if (signs[k] != 1.f && signs[k] != -1.f) return DPF_ERR_INVALID_ARG;
  if (dpf_normal_geo_workspace_bytes(B, n, H, W) < 0 || !(step == 1 || step == 2 || step == 4)) return DPF_ERR_UNSUPPORTED;
  g.pred = pred, g.depth = depth, g.normal = normal, g.Kmat = Kmat, g.ab = ab, g.mask = mask;
  g.n = n, g.H = H, g.W = W, g.target_type = target_type, g.towards = towards ? 1 : 0, g.ratio = ratio;
  for (int k = 0; k < 3; ++k) g.sg[k] = signs[k];
  dpf_fill_head_weights(hw.w, weights, n);
  return DPF_OK;
}

}  // namespace

extern "C" {

long long dpf_normal_geo_workspace_bytes(int B, int n, int H, int W) {
  const long long rows = dpf_tile_rows(B, n, H, W);
  return rows < 0 ? -1 : rows * 2 * (long long)sizeof(double);
}

int dpf_normal_geo_forward(const float* pred, const float* depth, const float* normal, const float* Kmat, const float* ab, const float* mask,
                           int B, int n, int H, int W, int target_type, float max_edge_ratio, int step, int towards_camera,
                           const float* target_signs_host, const float* head_weights_host, void* ws, long long ws_bytes, double* stats,
                           float* out, float* normal_out, unsigned char* counted_out, void* stream) {
  dpf_clear_error();
  Geo g;
  DpfHeadW hw;
  const int rc = prepare(pred, depth, normal, Kmat, ab, mask, B, n, H, W, target_type, max_edge_ratio, step, towards_camera,
                         target_signs_host, head_weights_host, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !out || (normal_out != nullptr) != (counted_out != nullptr) ||
      !dpf_ws_ok(ws, ws_bytes, dpf_normal_geo_workspace_bytes(B, n, H, W), 8))
    return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  double* part = (double*)ws;
  if (step == 1) hipLaunchKernelGGL(geo_forward_kernel<1>, grid, block, 0, st, g, part, normal_out, counted_out);
  else if (step == 2) hipLaunchKernelGGL(geo_forward_kernel<2>, grid, block, 0, st, g, part, normal_out, counted_out);
  else hipLaunchKernelGGL(geo_forward_kernel<4>, grid, block, 0, st, g, part, normal_out, counted_out);
  dpf_launch_head_fold<1>(part, B, n, H, W, hw, stats, out, st);
  return dpf_check_launch();
}

int dpf_normal_geo_backward(const float* pred, const float* depth, const float* normal, const float* Kmat, const float* ab, const float* mask,
                            int B, int n, int H, int W, int target_type, float max_edge_ratio, int step, int towards_camera,
                            const float* target_signs_host, const float* head_weights_host, const double* stats, const float* gout,
                            float* dpred, void* stream) {
  dpf_clear_error();
  Geo g;
  DpfHeadW hw;
  const int rc = prepare(pred, depth, normal, Kmat, ab, mask, B, n, H, W, target_type, max_edge_ratio, step, towards_camera,
                         target_signs_host, head_weights_host, g, hw);
  if (rc != DPF_OK) return rc;
  if (!stats || !gout || !dpred) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = dpf_tile_grid(B, n, H, W), block(kBlock);
  if (step == 1) hipLaunchKernelGGL(geo_backward_kernel<1>, grid, block, 0, st, g, hw, stats, gout, dpred);
  else if (step == 2) hipLaunchKernelGGL(geo_backward_kernel<2>, grid, block, 0, st, g, hw, stats, gout, dpred);
  else hipLaunchKernelGGL(geo_backward_kernel<4>, grid, block, 0, st, g, hw, stats, gout, dpred);
  return dpf_check_launch();
}

}  // extern "C"
