// Edge-aware post-processing of a predicted disparity map (option key post_process; dualpixelface_amd/postprocess.py): the guided filter
// of He et al. with a grey guide, and the joint bilateral filter.  The reference declares the two switches and implements neither, so
// the definitions below are this project's own.
//
// Guide: I = 0.299 R + 0.587 G + 0.114 B with R = x_0 * std_0 + mean_0 and so on, formed on the device from the normalised image
// [B, 3, H, W]; mean and std arrive by value from the host (the data path's Normalizer constants).
//
//   dpf_guided_filter            luma plane, (I, p) -> (a, b'), (a, b', I) -> q      3 launches
//   dpf_joint_bilateral_filter   one launch, luma formed while the tile is loaded
//
// Guided filter, square window of radius r clipped at the image border, every mean over the window's own in-image count N:
//   a = (mean(I p) - mean(I) mean(p)) / (mean(I I) - mean(I)^2 + eps),  b = mean(p) - a mean(I),  q = mean(a) I + mean(b).
// A workgroup owns a band of rows x a strip of 256 - 2r columns and walks down it 8 rows at a time.  Column direction: thread t owns the
// column x0 - r + t of the strip with its halo and keeps running window sums in registers (add the row that enters, subtract the one that
// leaves), read straight from global memory, one coalesced row per step; 8 rows of sums go to LDS.  Row direction: a thread finishes four
// neighbouring pixels of one row: the first one's 2r + 1 window words from LDS left to right, 16 bytes per read (a wave reads consecutive
// 16-byte words: conflict-free), the other three as running sums in registers (drop the word that leaves, add the one that enters); the
// four results leave as one 16-byte store where the alignment allows.
// Moments are taken about the band's first pixel (I0, pt), never raw: cov = mean(I' p') - mean(I') mean(p'), var likewise, so a
// disparity of 200 px keeps 0.1 px of structure in fp32.  b is stored as b' = b - p(sample, head, 0, 0), which keeps mean(b') small for
// the same reason; the second pass adds that pixel back at the end.
// Joint bilateral filter: q(x) = sum w_s w_c p(y) / sum w_s w_c over the clipped (2r+1)^2 window, taken as p(x) + sum w (p(y) - p(x)) /
// sum w; I and p tiles with halo and the (r+1)^2 table of w_s sit in LDS; taps run row by row, left to right.
// No floating-point atomics, no hand-off between workgroups but kernel boundaries, every sum in a fixed order: the bits repeat.
#include "dpf_common.h"
#include "dpf_image.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 8;                // rows of column sums held in LDS at a time
constexpr int kRowLen = kBlock + 8;      // floats per LDS row: the 16-byte reads of the last working thread end at word 262 at most
                                         // (words 256.. hold zeros; they only reach sums of pixels outside the strip, which are dropped)
constexpr int kGuidedMaxR = 32;
constexpr int kBilateralMaxR = 16;
constexpr int kMaxPlanes = 65535;        // B * n rides on gridDim.z
constexpr int kMaxBands = 65535;         // and the bands of rows on gridDim.y
constexpr int kBTH = 16, kBTW = 32;      // bilateral output tile (two rows per thread)

// guide [B][3][HW] -> I [B][HW]; grid (blocks, B)
__global__ __launch_bounds__(256) void luma_kernel(const float* __restrict__ guide, long long HW, DpfNorm nm, float* __restrict__ I) {
  const float* g = guide + (size_t)blockIdx.y * 3 * (size_t)HW;
  float* o = I + (size_t)blockIdx.y * (size_t)HW;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long long)gridDim.x * kBlock)
    o[i] = dpf_luma(g[i], g[i + HW], g[i + 2 * HW], nm);
}

// The two guided passes.  grid (strips, bands, B * n), 256 threads; TW = 256 - 2r output columns per strip, BH (a multiple of kChunk) rows
// per band.  u, v: the two planes whose window sums are taken -- PASS 1: I [B][HW] and p (sample stride pstride, head stride HW);
// PASS 2: a and b' [B * n][HW].  out0, out1: PASS 1 writes a, b'; PASS 2 writes q to out0 (out1 unused).  vec: W % 4 == 0, TW % 4 == 0
// and I, out0, out1 16-byte aligned, so the four pixels of a thread are one 16-byte access.
template <int PASS>
__global__ __launch_bounds__(256) void guided_kernel(const float* __restrict__ u, const float* __restrict__ v, long long vstride,
                                                     const float* __restrict__ I, const float* __restrict__ p, long long pstride, int n,
                                                     int H, int W, int r, int BH, float eps, int vec, float* __restrict__ out0,
                                                     float* __restrict__ out1) {
  constexpr int Q = PASS == 1 ? 4 : 2;   // sums per pixel: I', p', I' I', I' p'  |  a, b'
  __shared__ __attribute__((aligned(16))) float sm[Q][kChunk][kRowLen];
  const int t = threadIdx.x;
  const int TW = kBlock - 2 * r;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * BH;
  const int plane = blockIdx.z, b = plane / n, head = plane - b * n;
  const size_t HW = (size_t)H * (size_t)W;
  const float* ub = PASS == 1 ? u + (size_t)b * HW : u + (size_t)plane * HW;
  const float* vb = PASS == 1 ? v + (size_t)b * (size_t)vstride + (size_t)head * HW : v + (size_t)plane * HW;
  const float* Ib = I + (size_t)b * HW;
  // PASS 1: the band's first pixel is the point the moments are taken about; p00 is what b' leaves out and PASS 2 puts back
  const float u0 = PASS == 1 ? ub[(size_t)y0 * W + x0] : 0.f;
  const float v0 = PASS == 1 ? vb[(size_t)y0 * W + x0] : 0.f;
  const float p00 = p[(size_t)b * (size_t)pstride + (size_t)head * HW];

  const int cx = x0 - r + t;                               // the column this thread sums down
  const bool col_in = cx >= 0 && cx < W;
  float acc[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) acc[k] = 0.f;
  auto row_terms = [&](int y, float (&term)[Q]) {
    const float a = ub[(size_t)y * W + cx] - u0, c = vb[(size_t)y * W + cx] - v0;
    term[0] = a;
    term[1] = c;
    if (PASS == 1) {
      term[Q - 2] = a * a;
      term[Q - 1] = a * c;
    }
  };
  if (col_in) {                                            // the window of the band's first row, but for its last row (added below)
    const int ya = max(y0 - r, 0), yb = min(y0 + r - 1, H - 1);
    for (int y = ya; y <= yb; ++y) {
      float term[Q];
      row_terms(y, term);
#pragma unroll
      for (int k = 0; k < Q; ++k) acc[k] += term[k];
    }
  }
  const int yend = min(y0 + BH, H);
  // row direction: thread (cg, jr) finishes the four pixels 4 cg .. 4 cg + 3 of the strip in rows jr and jr + 4 of the chunk
  const int cg = t & 63, jr = t >> 6;
  const int ox = x0 + 4 * cg;
  const int nvalid = min(4, min(TW - 4 * cg, W - ox));     // <= 0: nothing to finish
  const int m = 2 * r + 1, full = m >> 2, rem = m & 3;     // window words; whole 16-byte reads in it; words left over (1 or 3: m is odd)
  if (t < kRowLen - kBlock) {                              // the words past the columns: zero once (the first barrier below publishes them)
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
#pragma unroll
      for (int k = 0; k < Q; ++k) sm[k][j][kBlock + t] = 0.f;
  }
  for (int yc = y0; yc < yend; yc += kChunk) {
    if (col_in) {
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const int y = yc + j;
        if (y >= yend) break;                              // the band's last chunk may be short: no row past yend is summed or read
        const int yin = y + r, yout = y - r - 1;           // (yout < y < yend <= H)
        float term[Q];
        if (yin < H) {
          row_terms(yin, term);
#pragma unroll
          for (int k = 0; k < Q; ++k) acc[k] += term[k];
        }
        if (yout >= 0 && y > y0) {
          row_terms(yout, term);
#pragma unroll
          for (int k = 0; k < Q; ++k) acc[k] -= term[k];
        }
#pragma unroll
        for (int k = 0; k < Q; ++k) sm[k][j][t] = acc[k];
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
#pragma unroll
        for (int k = 0; k < Q; ++k) sm[k][j][t] = 0.f;
    }
    __syncthreads();
    if (nvalid > 0) {
      const int rows = min(kChunk, yend - yc);
      for (int j = jr; j < rows; j += 4) {
        const int y = yc + j;
        // the first pixel's window word by word, left to right; the next three slide: drop the word that leaves, add the one that enters
        float s[Q][4];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
          const float* row = &sm[k][j][4 * cg];
          const f32x4 first = *reinterpret_cast<const f32x4*>(row);
          float s0 = 0.f;
          for (int i = 0; i < full; ++i) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(row + 4 * i);
            s0 += w4[0];
            s0 += w4[1];
            s0 += w4[2];
            s0 += w4[3];
          }
          const f32x4 ta = *reinterpret_cast<const f32x4*>(row + 4 * full), tb = *reinterpret_cast<const f32x4*>(row + 4 * full + 4);
          float e0, e1, e2;
          if (rem == 1) {
            s0 += ta[0];
            e0 = ta[1], e1 = ta[2], e2 = ta[3];
          } else {
            s0 += ta[0];
            s0 += ta[1];
            s0 += ta[2];
            e0 = ta[3], e1 = tb[0], e2 = tb[1];
          }
          s[k][0] = s0;
          s[k][1] = (s[k][0] - first[0]) + e0;
          s[k][2] = (s[k][1] - first[1]) + e1;
          s[k][3] = (s[k][2] - first[2]) + e2;
        }
        const int ny = min(y + r, H - 1) - max(y - r, 0) + 1;
        const size_t yo = (size_t)y * W + ox, o = (size_t)plane * HW + yo;
        const bool vec4 = vec && nvalid == 4;
        f32x4 iv = {0.f, 0.f, 0.f, 0.f};
        if (PASS == 2) {
          if (vec4) {
            iv = *reinterpret_cast<const f32x4*>(Ib + yo);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (i < nvalid) iv[i] = Ib[yo + i];
          }
        }
        f32x4 r0, r1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int nx = min(ox + i + r, W - 1) - max(ox + i - r, 0) + 1;
          const float inv = 1.f / (float)(ny * nx);
          if (PASS == 1) {
            const float mi = s[0][i] * inv, mp = s[1][i] * inv;
            const float var = s[Q - 2][i] * inv - mi * mi, cov = s[Q - 1][i] * inv - mi * mp;
            const float a = cov / (var + eps);
            r0[i] = a;
            r1[i] = ((v0 - p00) + mp) - a * (u0 + mi);
          } else {
            r0[i] = (s[0][i] * inv) * iv[i] + s[1][i] * inv + p00;
          }
        }
        if (vec4) {
          *reinterpret_cast<f32x4*>(out0 + o) = r0;
          if (PASS == 1) *reinterpret_cast<f32x4*>(out1 + o) = r1;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (i < nvalid) {
              out0[o + i] = r0[i];
              if (PASS == 1) out1[o + i] = r1[i];
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// grid (ceil(W / 32), ceil(H / 16), B * n), 256 threads = 8 rows x 32 columns, each thread the pixels (ty, tx) and (ty + 8, tx) of the tile.
__global__ __launch_bounds__(256) void bilateral_kernel(const float* __restrict__ p, long long pstride, const float* __restrict__ guide, int n,
                                                        int H, int W, int r, float inv2ss, float inv2sc, DpfNorm nm, float* __restrict__ q) {
  constexpr int kMaxRows = kBTH + 2 * kBilateralMaxR, kMaxCols = kBTW + 2 * kBilateralMaxR;
  __shared__ float sI[kMaxRows * kMaxCols], sP[kMaxRows * kMaxCols];
  __shared__ float sW[(kBilateralMaxR + 1) * (kBilateralMaxR + 1)];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * kBTW, y0 = blockIdx.y * kBTH;
  const int plane = blockIdx.z, b = plane / n, head = plane - b * n;
  const size_t HW = (size_t)H * (size_t)W;
  const float* pb = p + (size_t)b * (size_t)pstride + (size_t)head * HW;
  const float* gb = guide + (size_t)b * 3 * HW;
  const int rows = kBTH + 2 * r, cols = kBTW + 2 * r;
  for (int i = t; i < rows * cols; i += kBlock) {
    const int ly = i / cols, lx = i - ly * cols;
    const int y = y0 - r + ly, x = x0 - r + lx;
    float vi = 0.f, vp = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t o = (size_t)y * W + x;
      vi = dpf_luma(gb[o], gb[o + HW], gb[o + 2 * HW], nm);
      vp = pb[o];
    }
    sI[i] = vi;
    sP[i] = vp;
  }
  for (int i = t; i < (r + 1) * (r + 1); i += kBlock) {
    const int dy = i / (r + 1), dx = i - dy * (r + 1);
    sW[i] = expf(-(float)(dy * dy + dx * dx) * inv2ss);
  }
  __syncthreads();
  const int tx = t & 31, ty = t >> 5;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int ly = ty + half * 8;
    const int y = y0 + ly, x = x0 + tx;
    if (y >= H || x >= W) continue;                        // (no barrier below)
    const int c = (ly + r) * cols + tx + r;
    const float ic = sI[c], pc = sP[c];
    float num = 0.f, den = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const bool row_in = y + dy >= 0 && y + dy < H;
      const float* wrow = sW + abs(dy) * (r + 1);
      const int base = c + dy * cols;
      for (int dx = -r; dx <= r; ++dx) {
        const float di = sI[base + dx] - ic;
        float w = wrow[abs(dx)] * __expf(-(di * di) * inv2sc);
        if (!(row_in && x + dx >= 0 && x + dx < W)) w = 0.f;
        num += w * (sP[base + dx] - pc);
        den += w;
      }
    }
    q[(size_t)plane * HW + (size_t)y * W + x] = pc + num / den;
  }
}

bool shape_ok(int B, int n, int H, int W) { return B > 0 && n > 0 && H > 0 && W > 0; }

// rows per band: 32, halved while the grid is small and the band still is as tall as the halo above it
int band_rows(int B, int n, int H, int W, int r) {
  const long long strips = dpf_div_up(W, kBlock - 2 * r);
  int bh = 32;
  while (bh > kChunk && bh / 2 >= r && strips * dpf_div_up(H, bh) * (long long)B * n < 1024) bh /= 2;
  return bh;
}

}  // namespace

extern "C" {

long long dpf_guided_filter_workspace_bytes(int B, int n, int H, int W, int r) {
  if (!shape_ok(B, n, H, W) || r < 1 || r > kGuidedMaxR || (long long)B * n > kMaxPlanes || dpf_div_up(H, kChunk) > kMaxBands) return -1;
  const long long HW = (long long)H * W;
  const long long floats = (long long)B * HW + 2 * (long long)B * n * HW;      // I, a, b'
  return ((floats * 4 + 7) / 8) * 8;
}

int dpf_guided_filter(const float* p, long long p_batch_stride, const float* guide_rgb, int B, int n, int H, int W, int r, double eps,
                      const float* norm_host, void* ws, long long ws_bytes, float* q, void* stream) {
  dpf_clear_error();
  if (!p || !guide_rgb || !norm_host || !ws || !q || !shape_ok(B, n, H, W) || r < 1 || !((float)eps > 0.f))
    return DPF_ERR_INVALID_ARG;                            // (eps is used as a float)
  const long long HW = (long long)H * W;
  if (p_batch_stride < (long long)n * HW) return DPF_ERR_INVALID_ARG;
  if (r > kGuidedMaxR || (long long)B * n > kMaxPlanes || dpf_div_up(H, kChunk) > kMaxBands) return DPF_ERR_UNSUPPORTED;
  if (ws_bytes < dpf_guided_filter_workspace_bytes(B, n, H, W, r) || ((uintptr_t)ws & 7u)) return DPF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const DpfNorm nm = dpf_norm_of(norm_host);
  float* I = (float*)ws;
  float* a = I + (size_t)B * HW;
  float* bq = a + (size_t)B * n * HW;
  hipLaunchKernelGGL(luma_kernel, dim3(dpf_ew_grid(HW), B), dim3(kBlock), 0, st, guide_rgb, HW, nm, I);
  const int bh = band_rows(B, n, H, W, r);
  const dim3 grid(dpf_div_up(W, kBlock - 2 * r), dpf_div_up(H, bh), B * n);
  const int vec = W % 4 == 0 && r % 2 == 0 && dpf_aligned16(ws) && dpf_aligned16(q);      // (the planes of ws are H W floats apart: aligned with it)
  hipLaunchKernelGGL((guided_kernel<1>), grid, dim3(kBlock), 0, st, (const float*)I, p, p_batch_stride, (const float*)I, p, p_batch_stride, n,
                     H, W, r, bh, (float)eps, vec, a, bq);
  hipLaunchKernelGGL((guided_kernel<2>), grid, dim3(kBlock), 0, st, (const float*)a, (const float*)bq, 0LL, (const float*)I, p,
                     p_batch_stride, n, H, W, r, bh, (float)eps, vec, q, (float*)nullptr);
  return dpf_check_launch();
}

int dpf_joint_bilateral_filter(const float* p, long long p_batch_stride, const float* guide_rgb, int B, int n, int H, int W, int r,
                               double sigma_space, double sigma_color, const float* norm_host, float* q, void* stream) {
  dpf_clear_error();
  if (!p || !guide_rgb || !norm_host || !q || !shape_ok(B, n, H, W) || r < 1 || !(sigma_space > 0.0) || !(sigma_color > 0.0))
    return DPF_ERR_INVALID_ARG;
  const long long HW = (long long)H * W;
  if (p_batch_stride < (long long)n * HW) return DPF_ERR_INVALID_ARG;
  if (r > kBilateralMaxR || (long long)B * n > kMaxPlanes || dpf_div_up(H, kBTH) > kMaxBands) return DPF_ERR_UNSUPPORTED;
  const float inv2ss = (float)(1.0 / (2.0 * sigma_space * sigma_space)), inv2sc = (float)(1.0 / (2.0 * sigma_color * sigma_color));
  if (!(inv2ss < INFINITY) || !(inv2sc < INFINITY)) return DPF_ERR_INVALID_ARG;      // a sigma too small for fp32
  const dim3 grid(dpf_div_up(W, kBTW), dpf_div_up(H, kBTH), B * n);
  hipLaunchKernelGGL(bilateral_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, p, p_batch_stride, guide_rgb, n, H, W, r, inv2ss, inv2sc,
                     dpf_norm_of(norm_host), q);
  return dpf_check_launch();
}

}  // extern "C"
