// Deformable 2-D convolution, plain (DCN v1) and modulated (v2, per-sample mask): the reference's second compiled extension
// `deform_conv_cuda` (src/module/dcn/src/deform_conv_cuda.cpp:687-697 over deform_conv_cuda_kernel.cu:190,279,373,570,635,695).
//   input [B][C][H][W], weight [K][C/group][kh][kw], offset [B][dg * 2T][Ho][Wo] (channel 2(i kw + j) = h, + 1 = w of tap (i, j), kernel.cu:214-221),
//   mask [B][dg * T][Ho][Wo] (kernel.cu:604-612) or nullptr for the plain operator, output [B][K][Ho][Wo]; T = kh kw, dg = deformable_group.
//   sample position h = ho sh - ph + i dh + off_h, w likewise; a sample counts only if h > -1 && w > -1 && h < H && w < W (kernel.cu:228,617),
//   corners outside the image contribute 0 (kernel.cu:84-114); the coordinate gradient is get_coordinate_weight's (kernel.cu:145-187), 0 for
//   an invalid sample; grad_mask = sum_c gcol * unmasked sample (kernel.cu:695-780).
//   input channel c uses deformable group c / (C/dg); output channel k of conv group k / (K/group) contracts over [g C/group, (g+1) C/group).
// Structure: that of dcn_grouped.hip, one dimension smaller (4 corners, 2 offset components) plus the mask.  The grouping is a kernel argument;
// a 256-thread workgroup owns a tile of 64 output positions for ALL groups; one call is a fixed number of launches.
//   sampling   : the bilinear corner block of a (position, tap) is computed once per deformable group and reused for that group's channels;
//                the mask value is multiplied into the samples before they are staged in LDS.
//   products   : the grouped weight is repacked as the block-diagonal [K x C] matrix of a tap; a 32-row tile of the matrix instruction walks
//                only the reduce range of the conv groups its rows belong to.  (Rows of different groups that share a tile see each other's
//                samples multiplied by an exact zero: invisible for finite data, a NaN for a non-finite sample.)
//   grad_offset, grad_mask: the workgroup holds gcol = W^T . grad_output of its tile for all channels, sums the two coordinate gradients and
//                the mask gradient per deformable group over that group's channels in a fixed order and stores each element once: no atomics,
//                bitwise reproducible in every mode.
//   grad_input, grad_weight: dcn_acc_add (dcn_internal.h) -- float atomics, or in deterministic mode the integer shadows of the workspace.
// PRECISION: every product here runs on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32) for every setting of dpf_set_f32_matrix_path;
// the split-operand (f16 / bf16 component) constructions of the single-group 3-D tiers and their range guards are NOT extended to this path.
// LIMITS: whole C, K <= 256, T <= 49, H W < 2^31; any stride, padding, dilation and any dividing grouping.
#include "dpf_common.h"
#include "dcn_internal.h"

namespace {

constexpr int TP = 64;          // output positions per workgroup
constexpr int SP = TP + 1;      // padded LDS row
constexpr int MAXC2 = 256;      // whole C and K
constexpr int MAXT2 = 49;

struct Dcn2P {
  int B, C, K, H, W, Ho, Wo;
  int kh, kw, T, sh, sw, ph, pw, dh, dw;
  int CP;              // C rounded up to even
  int P;               // Ho * Wo
  int tiles_per_b, nchunk, ntg;
  int G, DG;           // conv groups, deformable groups
  int Cg, Kg, Cdg;     // C / G, K / G, C / DG
  // the four thread rows (tid >> 6) of a workgroup sample `slots` deformable groups at a time, `nq` rows per group (slots * nq = 4)
  int slots, nq;
};

struct Smp {   // per output position, tap and deformable group
  int idx[4];      // corner (jh, jw) = (j >> 1, j & 1): flat pixel index or -1
  float wg[4];     // its bilinear weight
  float lh, lw, m;
  int valid;
};

// first and one-past-last index on the other side of the block-diagonal weight for rows [r0, r1) of one side
__device__ __forceinline__ void span2(int r0, int r1, int rw, int ow, int& lo, int& hi) {
  lo = (r0 / rw) * ow;
  hi = ((r1 - 1) / rw + 1) * ow;
}

// off_g: the [2T][P] offsets of one deformable group of one image; mask_g: its [T][P] mask values or nullptr (plain operator: m = 1)
__device__ __forceinline__ Smp make_smp(const Dcn2P& p, const float* __restrict__ off_g, const float* __restrict__ mask_g, int t, int pos) {
  Smp s;
  s.valid = 0;
  s.lh = s.lw = 0.f;
  s.m = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { s.idx[j] = -1; s.wg[j] = 0.f; }
  if (pos >= p.P) return s;
  const int xo = pos % p.Wo, yo = pos / p.Wo;
  const int tj = t % p.kw, ti = t / p.kw;
  const float fh = (float)(yo * p.sh - p.ph + ti * p.dh) + off_g[(long long)(2 * t) * p.P + pos];
  const float fw = (float)(xo * p.sw - p.pw + tj * p.dw) + off_g[(long long)(2 * t + 1) * p.P + pos];
  s.m = mask_g ? mask_g[(long long)t * p.P + pos] : 1.f;
  if (fh > -1.f && fw > -1.f && fh < (float)p.H && fw < (float)p.W) {   // kernel.cu:228
    const float h0f = floorf(fh), w0f = floorf(fw);
    const int h0 = (int)h0f, w0 = (int)w0f;
    s.lh = fh - h0f;
    s.lw = fw - w0f;
    s.valid = 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jh = j >> 1, jw = j & 1;
      const int h = h0 + jh, w = w0 + jw;
      s.wg[j] = (jh ? s.lh : 1.f - s.lh) * (jw ? s.lw : 1.f - s.lw);
      if (h >= 0 && h <= p.H - 1 && w >= 0 && w <= p.W - 1) s.idx[j] = h * p.W + w;   // kernel.cu:97-108
    }
  }
  return s;
}

// the block-diagonal matrix of every tap, zero-padded: mode 0 (forward) wt[t][c][k], mode 1 (backward) wt[t][k][c]; `rows` x `RT` per tap
__global__ void dcn2_repack_kernel(const float* __restrict__ w, float* __restrict__ wt, int K, int C, int T, int Cg, int Kg, int rows, int RT, int mode) {
  const long long total = (long long)T * rows * RT;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int o = (int)(i % RT);
    const int r = (int)((i / RT) % rows);
    const int t = (int)(i / ((long long)RT * rows));
    const int c = mode == 0 ? r : o, k = mode == 0 ? o : r;
    float v = 0.f;
    if (k < K && c < C && c / Cg == k / Kg) v = w[((long long)k * Cg + c % Cg) * T + t];
    wt[i] = v;
  }
}

// deterministic mode: a tensor = value of its integer shadow (every contribution went there; the tensor itself is overwritten)
__global__ void dcn2_finalize_kernel(const long long* __restrict__ shadow, float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = dpf_det_value(shadow + 2 * i);
}

// S[c][pp] = mask * bilinear sample of channel c at position pp of the tile, for tap t, every channel of every deformable group
// (row C of an odd channel count is zeroed: the matrix instruction reduces two channels at a time)
__device__ __forceinline__ void build_samples2(const Dcn2P& p, const float* __restrict__ xb, const float* __restrict__ off_b,
                                               const float* __restrict__ mask_b, int t, int pos, float* s_S, int tid) {
  const int pp = tid & 63, q = tid >> 6;
  const int slot = q / p.nq, sub = q - slot * p.nq;
  const long long chan = (long long)p.H * p.W;
  for (int dg = slot; dg < p.DG; dg += p.slots) {
    const Smp s = make_smp(p, off_b + (long long)dg * 2 * p.T * p.P, mask_b ? mask_b + (long long)dg * p.T * p.P : nullptr, t, pos);
    float wm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wm[j] = s.wg[j] * s.m;
    for (int cc = sub; cc < p.Cdg; cc += p.nq) {
      const int c = dg * p.Cdg + cc;
      const float* xc = xb + (long long)c * chan;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (s.idx[j] >= 0) v += wm[j] * xc[s.idx[j]];
      s_S[c * SP + pp] = v;
    }
  }
  if (q == 0 && p.CP > p.C) s_S[p.C * SP + pp] = 0.f;
}

// ------------------------------------------------------------------------------------------ forward
// NA: (row tile, position half) tiles per wave -- 1, 2 or 4 for K <= 64, 128, 256 (the accumulators of tiles a shape does not have would only cost occupancy)
template <int NA>
__global__ __launch_bounds__(256) void dcn2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ mask,
                                                       const float* __restrict__ wt /*[T][CP][KT]*/, const float* __restrict__ bias,
                                                       float* __restrict__ out, Dcn2P p) {
  extern __shared__ __align__(16) float smem[];
  float* s_S = smem;   // [CP][SP]
  const int MT = (p.K + 31) / 32, KT = 32 * MT, NTILES = 2 * MT;   // K <= 256: at most 16 (row tile, position half) tiles, NA per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const int pos0 = (blockIdx.x % p.tiles_per_b) * TP;
  const float* xb = x + (long long)b * p.C * p.H * p.W;
  const float* off_b = offset + (long long)b * p.DG * 2 * p.T * p.P;
  const float* mask_b = mask ? mask + (long long)b * p.DG * p.T * p.P : nullptr;

  f32x16 acc[NA];
  int cp0[NA], cp1[NA];   // reduce range of the tile, in channel pairs
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    const int m = (wave + 4 * i) >> 1;
    int lo = 0, hi = 0;
    if (wave + 4 * i < NTILES) span2(32 * m, min(32 * m + 32, p.K), p.Kg, p.Cg, lo, hi);
    cp0[i] = lo / 2;
    cp1[i] = (hi + 1) / 2;
  }

  for (int t = 0; t < p.T; ++t) {
    __syncthreads();
    build_samples2(p, xb, off_b, mask_b, t, pos0 + (tid & 63), s_S, tid);
    __syncthreads();
    const float* wtt = wt + (long long)t * p.CP * KT;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int tile = wave + 4 * i;
      if (tile < NTILES) {
        const int m = tile >> 1, nt = tile & 1;
        for (int cp = cp0[i]; cp < cp1[i]; ++cp) {
          const int c = 2 * cp + hh;
          const float a = wtt[(long long)c * KT + m * 32 + l31];
          const float bv = s_S[c * SP + nt * 32 + l31];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[i], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int tile = wave + 4 * i;
    if (tile < NTILES) {
      const int m = tile >> 1, nt = tile & 1;
      const int pos = pos0 + nt * 32 + l31;
      if (pos < p.P) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int k = m * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
          if (k < p.K) out[((long long)b * p.K + k) * p.P + pos] = acc[i][j] + (bias ? bias[k] : 0.f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ backward: offset + mask + input
// gcol[c][p] = sum_k W[k][c][t] * go[k][p] over the output channels of c's conv group, for all channels of the tile; then per deformable
// group the coordinate gradients and the mask gradient summed over its channels (grad_offset / grad_mask, one plain store per element) and
// the sampler's adjoint into grad_input (dcn_acc_add).  dx, doff, dmask may each be nullptr (not wanted).
__global__ __launch_bounds__(256) void dcn2_bwd_data_kernel(const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ mask,
                                                            const float* __restrict__ wt2 /*[T][KP][CT]*/, const float* __restrict__ go,
                                                            float* __restrict__ dx, float* __restrict__ doff, float* __restrict__ dmask, Dcn2P p,
                                                            long long* gi_shadow) {
  extern __shared__ __align__(16) float smem[];
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, NTILES = 2 * (CT / 32);   // C <= 256: at most 16 tiles, four per wave
  float* s_go = smem;                    // [KP][SP]
  float* s_gc = s_go + KP * SP;          // [CT][SP]
  float* s_red = s_gc + CT * SP;         // [3][4][TP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const int pos0 = (blockIdx.x % p.tiles_per_b) * TP;
  const long long chan = (long long)p.H * p.W;
  const float* xb = x + (long long)b * p.C * chan;
  float* dxb = dx ? dx + (long long)b * p.C * chan : nullptr;
  const float* off_b = offset + (long long)b * p.DG * 2 * p.T * p.P;
  const float* mask_b = mask ? mask + (long long)b * p.DG * p.T * p.P : nullptr;
  const int ndir = dmask ? 3 : 2;

  for (int i = tid; i < KP * TP; i += 256) {
    const int k = i / TP, pp = i - k * TP;
    const int pos = pos0 + pp;
    s_go[k * SP + pp] = (k < p.K && pos < p.P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
  }
  int kp0[4], kp1[4];   // reduce range of the tile, in output-channel pairs
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (wave + 4 * i) >> 1;
    int lo = 0, hi = 0;
    if (wave + 4 * i < NTILES && 32 * m < p.C) span2(32 * m, min(32 * m + 32, p.C), p.Cg, p.Kg, lo, hi);
    kp0[i] = lo / 2;
    kp1[i] = (hi + 1) / 2;
  }
  const int pp = tid & 63, q = tid >> 6;
  const int slot = q / p.nq, sub = q - slot * p.nq;

  for (int t = 0; t < p.T; ++t) {
    __syncthreads();   // s_go ready / previous tap's s_gc, s_red consumed
    const float* wtt = wt2 + (long long)t * KP * CT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tile = wave + 4 * i;
      if (tile < NTILES) {
        const int m = tile >> 1, nt = tile & 1;
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int kp = kp0[i]; kp < kp1[i]; ++kp) {
          const int k = 2 * kp + hh;
          const float a = wtt[(long long)k * CT + m * 32 + l31];
          const float bv = s_go[k * SP + nt * 32 + l31];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int c = m * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
          s_gc[c * SP + nt * 32 + l31] = acc[j];
        }
      }
    }
    __syncthreads();
    // thread = (position pp, row q): row q serves deformable group base + slot, the channels sub, sub + nq, ... of it
    for (int base = 0; base < p.DG; base += p.slots) {
      const int dg = base + slot;
      float gh = 0.f, gw = 0.f, gm = 0.f;
      if (dg < p.DG) {
        const Smp s = make_smp(p, off_b + (long long)dg * 2 * p.T * p.P, mask_b ? mask_b + (long long)dg * p.T * p.P : nullptr, t, pos0 + pp);
        if (s.valid) {
          for (int cc = sub; cc < p.Cdg; cc += p.nq) {
            const int c = dg * p.Cdg + cc;
            const float gcv = s_gc[c * SP + pp];
            const float gcm = gcv * s.m;
            const float* xc = xb + (long long)c * chan;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (s.idx[j] < 0) continue;
              const int jh = j >> 1, jw = j & 1;
              if (dxb) dcn_acc_add(dx, gi_shadow, &dxb[(long long)c * chan + s.idx[j]], s.wg[j] * gcm);   // kernel.cu:279-370
              const float xv = xc[s.idx[j]];
              gm += s.wg[j] * xv * gcv;                                                                  // kernel.cu:695-780
              gh += (jh ? 1.f : -1.f) * (jw ? s.lw : 1.f - s.lw) * xv * gcm;                             // kernel.cu:145-187
              gw += (jw ? 1.f : -1.f) * (jh ? s.lh : 1.f - s.lh) * xv * gcm;
            }
          }
        }
      }
      s_red[(0 * 4 + q) * TP + pp] = gh;
      s_red[(1 * 4 + q) * TP + pp] = gw;
      s_red[(2 * 4 + q) * TP + pp] = gm;
      __syncthreads();
      for (int i = tid; i < ndir * p.slots * TP; i += 256) {
        const int p2 = i % TP, dir = (i / TP) % ndir, sl = i / (ndir * TP);
        const int pos = pos0 + p2;
        if (base + sl < p.DG && pos < p.P) {
          const float* r = s_red + (dir * 4 + sl * p.nq) * TP + p2;
          float v = r[0];
          for (int j = 1; j < p.nq; ++j) v += r[j * TP];
          if (dir < 2) {
            if (doff) doff[(((long long)b * p.DG + base + sl) * 2 * p.T + 2 * t + dir) * p.P + pos] = v;
          } else {
            dmask[(((long long)b * p.DG + base + sl) * p.T + t) * p.P + pos] = v;
          }
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------ backward: weight
// grid = T * nchunk * ntg; block = one tap, a strided set of position tiles, 4 NA consecutive 32 x 32 tiles of the [K x C] product;
// dW[k][c - c0(group of k)][t] += sum_p go[k][p] * S[c][p] for the (k, c) of one conv group.  Only tiles that touch a diagonal block are
// computed; a workgroup none of whose tiles does returns at once.
// NA: tiles per wave (1, 2 or 4); WGT = 4 NA tiles per workgroup.
template <int NA>
__global__ __launch_bounds__(256) void dcn2_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ mask,
                                                         const float* __restrict__ go, float* __restrict__ dw, long long* dw_shadow, Dcn2P p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int WGT = 4 * NA;
  const int MT = (p.K + 31) / 32, MTC = (p.CP + 31) / 32, NTILES = MT * MTC;
  float* s_S = smem;                 // [32*MTC][SP]
  float* s_go = s_S + 32 * MTC * SP; // [32*MT][SP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int tg = blockIdx.x % p.ntg;
  const int chunk = (blockIdx.x / p.ntg) % p.nchunk;
  const int t = blockIdx.x / (p.ntg * p.nchunk);
  auto tile_on = [&](int tl) {
    if (tl >= NTILES) return false;
    const int m = tl / MTC, mc = tl - m * MTC;
    int lo, hi;
    span2(32 * m, min(32 * m + 32, p.K), p.Kg, p.Cg, lo, hi);   // the channels the rows of this tile contract with
    return 32 * mc < hi && lo < min(32 * mc + 32, p.C);
  };
  bool any = false;
  for (int i = 0; i < WGT; ++i) any = any || tile_on(tg * WGT + i);
  if (!any) return;   // uniform over the workgroup
  f32x16 acc[NA];
  bool on[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    on[i] = tile_on(tg * WGT + wave + 4 * i);
  }
  // zero the padded rows once
  for (int i = tid; i < 32 * MTC * SP; i += 256) s_S[i] = 0.f;
  const int ntile = p.B * p.tiles_per_b;
  for (int tile = chunk; tile < ntile; tile += p.nchunk) {
    const int b = tile / p.tiles_per_b;
    const int pos0 = (tile % p.tiles_per_b) * TP;
    const float* xb = x + (long long)b * p.C * p.H * p.W;
    const float* off_b = offset + (long long)b * p.DG * 2 * p.T * p.P;
    const float* mask_b = mask ? mask + (long long)b * p.DG * p.T * p.P : nullptr;
    __syncthreads();
    build_samples2(p, xb, off_b, mask_b, t, pos0 + (tid & 63), s_S, tid);
    for (int i = tid; i < 32 * MT * TP; i += 256) {
      const int k = i / TP, pp = i - k * TP;
      const int pos = pos0 + pp;
      s_go[k * SP + pp] = (k < p.K && pos < p.P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      if (on[i]) {
        const int tl = tg * WGT + wave + 4 * i;
        const int m = tl / MTC, mc = tl - m * MTC;
#pragma unroll 4
        for (int ps = 0; ps < TP / 2; ++ps) {
          const int pp = 2 * ps + hh;
          const float a = s_go[(m * 32 + l31) * SP + pp];
          const float bv = s_S[(mc * 32 + l31) * SP + pp];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[i], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    if (on[i]) {
      const int tl = tg * WGT + wave + 4 * i;
      const int m = tl / MTC, mc = tl - m * MTC;
      const int c = mc * 32 + l31;
      if (c < p.C) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int k = m * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
          if (k < p.K && k / p.Kg == c / p.Cg) dcn_acc_add(dw, dw_shadow, &dw[((long long)k * p.Cg + c % p.Cg) * p.T + t], acc[i][j]);
        }
      }
    }
  }
}

// DPF_ERR_INVALID_ARG: a size that is no size, or a grouping that does not divide; DPF_ERR_UNSUPPORTED: beyond the limits of the header
int fill_params2(Dcn2P& p, int B, int C, int H, int W, int K, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int group,
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
  p.B = B; p.C = C; p.K = K; p.H = H; p.W = W; p.Ho = (int)Ho; p.Wo = (int)Wo;
  p.kh = kh; p.kw = kw; p.T = (int)T; p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.CP = (C + 1) & ~1;
  p.P = (int)(Ho * Wo);
  p.tiles_per_b = (p.P + TP - 1) / TP;
  if ((long long)B * p.tiles_per_b >= 0x7fffffffLL) return DPF_ERR_UNSUPPORTED;
  p.nchunk = 1;
  p.ntg = 1;
  p.G = group;
  p.DG = deformable_group;
  p.Cg = C / group;
  p.Kg = K / group;
  p.Cdg = C / deformable_group;
  p.nq = deformable_group == 1 ? 4 : deformable_group == 2 ? 2 : 1;
  p.slots = 4 / p.nq;
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
  Dcn2P p{};
  const int rc = fill_params2(p, B, C, H, W, K, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
  if (rc != DPF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int KT = (p.K + 31) / 32 * 32;
  const long long pack = (long long)p.T * p.CP * KT;
  hipLaunchKernelGGL(dcn2_repack_kernel, dim3(dpf_ew_grid(pack)), dim3(256), 0, st, weight, ws, p.K, p.C, p.T, p.Cg, p.Kg, p.CP, KT, 0);
  const size_t lds = sizeof(float) * (size_t)p.CP * SP;
  auto kern = KT <= 64 ? dcn2_fwd_kernel<1> : KT <= 128 ? dcn2_fwd_kernel<2> : dcn2_fwd_kernel<4>;
  if (dcn_launch(kern, dim3((unsigned)(p.B * p.tiles_per_b)), dim3(256), lds, st, input, offset, mask, (const float*)ws, bias, output, p) != DPF_OK)
    return DPF_ERR_LAUNCH;
  return dpf_check_launch();
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
  Dcn2P p{};
  int rc = fill_params2(p, B, C, H, W, K, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group);
  if (rc != DPF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int det = dpf_deterministic();
  const Dcn2Ws m = ws_map2(B, C, H, W, K, p.T, det);
  if (det && (reinterpret_cast<uintptr_t>(ws) & 7)) return DPF_ERR_INVALID_ARG;
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, MT = (p.K + 31) / 32, MTC = CT / 32;
  const long long in_elems = (long long)B * C * H * W, dw_elems = (long long)K * p.Cg * p.T;
  const long long ntile = (long long)p.B * p.tiles_per_b;

  if (grad_input || grad_offset || grad_mask) {
    long long* gi_shadow = nullptr;
    if (grad_input) {
      if (hipMemsetAsync(grad_input, 0, sizeof(float) * in_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
      if (det) {
        gi_shadow = reinterpret_cast<long long*>(ws + m.gi_shadow);
        if (hipMemsetAsync(gi_shadow, 0, sizeof(long long) * 2 * (size_t)in_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
      }
    }
    const long long pack = (long long)p.T * KP * CT;
    hipLaunchKernelGGL(dcn2_repack_kernel, dim3(dpf_ew_grid(pack)), dim3(256), 0, st, weight, ws, p.K, p.C, p.T, p.Cg, p.Kg, KP, CT, 1);
    const size_t lds = sizeof(float) * ((size_t)KP * SP + (size_t)CT * SP + 3 * 4 * TP);
    if (dcn_launch(dcn2_bwd_data_kernel, dim3((unsigned)ntile), dim3(256), lds, st, input, offset, mask, (const float*)ws, grad_output, grad_input,
                   grad_offset, grad_mask, p, gi_shadow) != DPF_OK)
      return DPF_ERR_LAUNCH;
    if (gi_shadow) hipLaunchKernelGGL(dcn2_finalize_kernel, dim3(dpf_ew_grid(in_elems)), dim3(256), 0, st, gi_shadow, grad_input, in_elems);
  }
  if (grad_weight) {
    long long* dw_shadow = nullptr;
    if (hipMemsetAsync(grad_weight, 0, sizeof(float) * dw_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    if (det) {
      dw_shadow = reinterpret_cast<long long*>(ws + m.dw_shadow);
      if (hipMemsetAsync(dw_shadow, 0, sizeof(long long) * 2 * (size_t)dw_elems, st) != hipSuccess) return DPF_ERR_LAUNCH;
    }
    // (the partials of a tap's chunks meet in float atomics, or -- dw_shadow -- in integer pairs: any chunk count is reproducible there)
    long long nchunkw = 2048 / p.T;
    if (nchunkw > ntile) nchunkw = ntile;
    p.nchunk = (int)nchunkw;
    const int na = MT * MTC <= 4 ? 1 : MT * MTC <= 8 ? 2 : 4;
    p.ntg = (MT * MTC + 4 * na - 1) / (4 * na);
    const size_t lds = sizeof(float) * ((size_t)CT * SP + (size_t)32 * MT * SP);
    auto kern = na == 1 ? dcn2_wgrad_kernel<1> : na == 2 ? dcn2_wgrad_kernel<2> : dcn2_wgrad_kernel<4>;
    if (dcn_launch(kern, dim3((unsigned)(p.T * p.nchunk * p.ntg)), dim3(256), lds, st, input, offset, mask, grad_output, grad_weight, dw_shadow,
                   p) != DPF_OK)
      return DPF_ERR_LAUNCH;
    if (dw_shadow) hipLaunchKernelGGL(dcn2_finalize_kernel, dim3(dpf_ew_grid(dw_elems)), dim3(256), 0, st, dw_shadow, grad_weight, dw_elems);
  }
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
