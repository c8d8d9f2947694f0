// The gather-kernel family of the deformable convolutions with the grouping as a kernel argument, one set of kernels templated on the spatial
// rank ND:
//   ND = 3: deformable 3-D convolution, every grouping (deform_conv_cuda.cu:65-66,84-121; deform_im2col_cuda.cuh:222-232), reached from
//           dcn3d.hip: every call with group > 1 or deformable_group > 1, and the single-group backward whose grad_input the packed scatter
//           declines (K > 64, or no haloed region fits; with (1, 1) the reduce spans are the whole of C and K).  Weight [K][C/group][T], offset
//           [B][deformable_group * 3T][P], no mask.
//   ND = 2: deformable 2-D convolution, plain (DCN v1) and modulated (v2, per-sample mask), every grouping -- the reference's second compiled
//           extension `deform_conv_cuda` (src/module/dcn/src/deform_conv_cuda.cpp:687-697 over deform_conv_cuda_kernel.cu:190,279,373,570,635,
//           695), reached from dcn2d.hip: input [B][C][H][W], weight [K][C/group][kh][kw], offset [B][dg * 2T][Ho][Wo] (channel 2(i kw + j) = h,
//           + 1 = w of tap (i, j), kernel.cu:214-221), mask [B][dg * T][Ho][Wo] (kernel.cu:604-612) or nullptr for the plain operator.
//           Sample position h = ho sh - ph + i dh + off_h, w likewise; a sample counts only if h > -1 && w > -1 && h < H && w < W
//           (kernel.cu:228,617), corners outside the image contribute 0 (kernel.cu:84-114); the coordinate gradient is get_coordinate_weight's
//           (kernel.cu:145-187), 0 for an invalid sample; grad_mask = sum_c gcol * unmasked sample (kernel.cu:695-780).
// Input channel c is sampled with the offsets (and mask) of deformable group c / (C/deformable_group); output channel k of conv group
// k / (K/group) contracts over that group's C/group input channels [g C/group, (g+1) C/group).
// What depends on the rank is the sampling rule Sampler<ND> and nothing else: the corner block of a (position, tap, deformable group), the mask
// value, the coordinate gradient of one corner (each rank's floating-point expressions as the reference associates them), the index type and
// the offset stride.  Rank 3's rule is dcn_internal.h's, shared with the single-group tiers of dcn3d.hip.
// A 256-thread workgroup owns a tile of 64 output positions for ALL groups, like the gather tier of dcn3d.hip; one call is a fixed number of
// launches (forward: repack + 1; backward: repack + 2) whatever the group counts.
//   sampling   : the corner block of a (position, tap) is computed once per deformable group and reused for every channel of that group (the
//                reference recomputes it per channel); the mask value is multiplied into the samples before they are staged in LDS.
//   products   : the grouped weight is repacked as the block-diagonal [K x C] matrix of a tap (zeros off the blocks); a 32-row tile of the
//                matrix instruction walks only the reduce range of the conv groups its rows belong to, so groups of >= 32 rows cost exactly
//                their own products and narrower groups share a tile.  (Rows of different groups that share a tile see each other's samples
//                multiplied by an exact zero: invisible for finite data, a NaN for a non-finite sample.)
//   grad_offset, grad_mask: the workgroup holds gcol = W^T . grad_output of its tile for all channels, sums the ND coordinate gradients and the
//                mask gradient per deformable group over that group's channels (in whichever conv groups they sit) in a fixed order and stores
//                each element once: no atomics, bitwise reproducible in every mode.
//   grad_input, grad_weight: dcn_acc_add (dcn_internal.h) -- float atomics, or in deterministic mode the integer shadows of the workspace.
// PRECISION: every product here runs on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32) for every setting of dpf_set_f32_matrix_path;
// the split-operand (f16 / bf16 component) constructions of the single-group 3-D tiers and their range guards are NOT extended to this path.
// LIMITS: the kernels hold whole C, K <= 256 and any T; each entry point enforces its own (3-D: C, K <= 128, T <= 64; 2-D: C, K <= 256, T <= 49,
// H W < 2^31).  Any stride, padding, dilation and any dividing grouping.
#include "dpf_common.h"
#include "dcn_internal.h"

namespace {

constexpr int TP = DCN_TP;      // output positions per workgroup
constexpr int SP = TP + 1;      // padded LDS row

struct GrpP {
  int G, DG;          // conv groups, deformable groups
  int Cg, Kg, Cdg;    // C / G, K / G, C / DG
  // the four thread rows (tid >> 6) of a workgroup sample `slots` deformable groups at a time, `nq` rows per group (slots * nq = 4)
  int slots, nq;
  int ntg;            // weight gradient: workgroups that share the 32 x 32 tiles of one (tap, chunk)
};

// The sampling rule of a rank, per output position, tap and deformable group.  off_g: the [ND T][P] offsets of one deformable group of one
// image; mask_g: its [T][P] mask values or nullptr (m = 1).  idx[j]: flat input index of corner j or -1; wg[j]: its interpolation weight;
// grad(j, xv, gcv, g): adds corner j's share (input value xv, column gradient gcv) to the coordinate gradients g[0 .. ND) and, where the rank
// has a mask, to the mask gradient g[ND].
template <int ND>
struct Sampler;

template <>
struct Sampler<3> {
  using Idx = long long;
  static constexpr int NC = 8;
  static constexpr float m = 1.f;   // no mask in the 3-D operator
  Corner cn;
  Idx idx[NC];
  float wg[NC];
  int valid;
  __device__ __forceinline__ Sampler(const DcnP& p, const float* __restrict__ off_g, const float* __restrict__, int t, Idx pos)
      : cn(make_corner(p, off_g, t, pos)), valid(cn.valid) {
#pragma unroll
    for (int j = 0; j < NC; ++j) idx[j] = corner_index(p, cn, j, wg[j]);
  }
  __device__ __forceinline__ void grad(int j, float xv, float gcv, float* g) const {   // cuh:131-187
    const int jd = (j >> 2) & 1, jh = (j >> 1) & 1, jw = j & 1;
    const float v = xv * gcv;
    const float fd = jd ? cn.ld : 1.f - cn.ld, fh = jh ? cn.lh : 1.f - cn.lh, fw = jw ? cn.lw : 1.f - cn.lw;
    g[0] += (jd ? 1.f : -1.f) * fh * fw * v;
    g[1] += (jh ? 1.f : -1.f) * fd * fw * v;
    g[2] += (jw ? 1.f : -1.f) * fd * fh * v;
  }
};

template <>
struct Sampler<2> {
  using Idx = int;
  static constexpr int NC = 4;
  Idx idx[NC];     // corner (jh, jw) = (j >> 1, j & 1)
  float wg[NC];
  float lh, lw, m;
  int valid;
  __device__ __forceinline__ Sampler(const DcnP& p, const float* __restrict__ off_g, const float* __restrict__ mask_g, int t, Idx pos) {
    const int P = (int)p.P;
    valid = 0;
    lh = lw = 0.f;
    m = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) { idx[j] = -1; wg[j] = 0.f; }
    if (pos >= P) return;
    const int xo = pos % p.Wo, yo = pos / p.Wo;
    const int tj = t % p.kw, ti = t / p.kw;
    const float fh = (float)(yo * p.sh - p.ph + ti * p.dh) + off_g[(long long)(2 * t) * P + pos];
    const float fw = (float)(xo * p.sw - p.pw + tj * p.dw) + off_g[(long long)(2 * t + 1) * P + pos];
    m = mask_g ? mask_g[(long long)t * P + pos] : 1.f;
    if (fh > -1.f && fw > -1.f && fh < (float)p.H && fw < (float)p.W) {   // kernel.cu:228
      const float h0f = floorf(fh), w0f = floorf(fw);
      const int h0 = (int)h0f, w0 = (int)w0f;
      lh = fh - h0f;
      lw = fw - w0f;
      valid = 1;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int jh = j >> 1, jw = j & 1;
        const int h = h0 + jh, w = w0 + jw;
        wg[j] = (jh ? lh : 1.f - lh) * (jw ? lw : 1.f - lw);
        if (h >= 0 && h <= p.H - 1 && w >= 0 && w <= p.W - 1) idx[j] = h * p.W + w;   // kernel.cu:97-108
      }
    }
  }
  __device__ __forceinline__ void grad(int j, float xv, float gcv, float* g) const {
    const int jh = j >> 1, jw = j & 1;
    const float gcm = gcv * m;
    g[0] += (jh ? 1.f : -1.f) * (jw ? lw : 1.f - lw) * xv * gcm;   // kernel.cu:145-187
    g[1] += (jw ? 1.f : -1.f) * (jh ? lh : 1.f - lh) * xv * gcm;
    g[2] += wg[j] * xv * gcv;                                       // kernel.cu:695-780
  }
};

// first and one-past-last index on the other side of the block-diagonal weight for rows [r0, r1) of one side:
// rows of width `rw` per group, `ow` per group on the other side
__device__ __forceinline__ void grp_span(int r0, int r1, int rw, int ow, int& lo, int& hi) {
  lo = (r0 / rw) * ow;
  hi = ((r1 - 1) / rw + 1) * ow;
}

// the block-diagonal matrix of every tap, zero-padded: mode 0 (forward) wt[t][c][k], mode 1 (backward) wt[t][k][c]; `rows` x `RT` per tap
__global__ void dcn_gather_repack_kernel(const float* __restrict__ w, float* __restrict__ wt, int K, int C, int T, int Cg, int Kg, int rows, int RT,
                                         int mode) {
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

// what a workgroup needs of image b: its input, its offsets and its mask (or nullptr)
template <int ND>
struct Image {
  const float *x, *off, *mask;
  long long chan;   // elements of one input channel
  __device__ __forceinline__ Image(const DcnP& p, const GrpP& g, const float* x_, const float* offset, const float* mask_, int b)
      : chan((long long)p.D * p.H * p.W) {
    x = x_ + (long long)b * p.C * chan;
    off = offset + (long long)b * g.DG * ND * p.T * p.P;
    mask = mask_ ? mask_ + (long long)b * g.DG * p.T * p.P : nullptr;
  }
  __device__ __forceinline__ Sampler<ND> sampler(const DcnP& p, int dg, int t, typename Sampler<ND>::Idx pos) const {
    return Sampler<ND>(p, off + (long long)dg * ND * p.T * p.P, mask ? mask + (long long)dg * p.T * p.P : nullptr, t, pos);
  }
};

// S[c][pp] = mask * interpolated sample of channel c at position pp of the tile, for tap t, every channel of every deformable group
// (row C of an odd channel count is zeroed: the matrix instruction reduces two channels at a time)
template <int ND>
__device__ __forceinline__ void build_samples(const DcnP& p, const GrpP& g, const Image<ND>& im, int t, typename Sampler<ND>::Idx pos, float* s_S,
                                              int tid) {
  using S = Sampler<ND>;
  const int pp = tid & 63, q = tid >> 6;
  const int slot = q / g.nq, sub = q - slot * g.nq;
  for (int dg = slot; dg < g.DG; dg += g.slots) {
    const S s = im.sampler(p, dg, t, pos);
    float wm[S::NC];
#pragma unroll
    for (int j = 0; j < S::NC; ++j) wm[j] = s.wg[j] * s.m;
    for (int cc = sub; cc < g.Cdg; cc += g.nq) {
      const int c = dg * g.Cdg + cc;
      const float* xc = im.x + (long long)c * im.chan;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < S::NC; ++j)
        if (s.idx[j] >= 0) v += wm[j] * xc[s.idx[j]];
      s_S[c * SP + pp] = v;
    }
  }
  if (q == 0 && p.CP > p.C) s_S[p.C * SP + pp] = 0.f;
}

// ------------------------------------------------------------------------------------------ forward
// NA: (row tile, position half) tiles per wave -- 1, 2 or 4 for K <= 64, 128, 256 (the accumulators of tiles a shape does not have would only cost occupancy)
template <int ND, int NA>
__global__ __launch_bounds__(256) void dcn_gather_fwd_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                             const float* __restrict__ mask, const float* __restrict__ wt /*[T][CP][KT]*/,
                                                             const float* __restrict__ bias, float* __restrict__ out, DcnP p, GrpP g) {
  using Idx = typename Sampler<ND>::Idx;
  extern __shared__ __align__(16) float smem[];
  float* s_S = smem;   // [CP][SP]
  const int MT = (p.K + 31) / 32, KT = 32 * MT, NTILES = 2 * MT;   // K <= 256: at most 16 (row tile, position half) tiles, NA per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const Idx pos0 = (Idx)(blockIdx.x % p.tiles_per_b) * TP, P = (Idx)p.P;
  const Image<ND> im(p, g, x, offset, mask, b);

  f32x16 acc[NA];
  int cp0[NA], cp1[NA];   // reduce range of the tile, in channel pairs
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    const int m = (wave + 4 * i) >> 1;
    int lo = 0, hi = 0;
    if (wave + 4 * i < NTILES) grp_span(32 * m, min(32 * m + 32, p.K), g.Kg, g.Cg, lo, hi);
    cp0[i] = lo / 2;
    cp1[i] = (hi + 1) / 2;
  }

  for (int t = 0; t < p.T; ++t) {
    __syncthreads();
    build_samples<ND>(p, g, im, t, pos0 + (tid & 63), s_S, tid);
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
      const Idx pos = pos0 + nt * 32 + l31;
      if (pos < P) {
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
// the sampler's adjoint into the channels [0, CG) of grad_input (dcn_acc_add).  dx, doff, dmask may each be nullptr (not wanted).
template <int ND>
__global__ __launch_bounds__(256) void dcn_gather_bwd_data_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                                  const float* __restrict__ mask, const float* __restrict__ wt2 /*[T][KP][CT]*/,
                                                                  const float* __restrict__ go, float* __restrict__ dx, float* __restrict__ doff,
                                                                  float* __restrict__ dmask, DcnP p, GrpP g, int CG, long long* gi_shadow) {
  using S = Sampler<ND>;
  using Idx = typename S::Idx;
  extern __shared__ __align__(16) float smem[];
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, NTILES = 2 * (CT / 32);   // C <= 256: at most 16 tiles, four per wave
  float* s_go = smem;                    // [KP][SP]
  float* s_gc = s_go + KP * SP;          // [CT][SP]
  float* s_red = s_gc + CT * SP;         // [3][4][TP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const Idx pos0 = (Idx)(blockIdx.x % p.tiles_per_b) * TP, P = (Idx)p.P;
  const Image<ND> im(p, g, x, offset, mask, b);
  float* dxb = dx ? dx + (long long)b * p.C * im.chan : nullptr;
  const int ndir = dmask ? ND + 1 : ND;

  for (int i = tid; i < KP * TP; i += 256) {
    const int k = i / TP, pp = i - k * TP;
    const Idx pos = pos0 + pp;
    s_go[k * SP + pp] = (k < p.K && pos < P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
  }
  int kp0[4], kp1[4];   // reduce range of the tile, in output-channel pairs
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (wave + 4 * i) >> 1;
    int lo = 0, hi = 0;
    if (wave + 4 * i < NTILES && 32 * m < p.C) grp_span(32 * m, min(32 * m + 32, p.C), g.Cg, g.Kg, lo, hi);
    kp0[i] = lo / 2;
    kp1[i] = (hi + 1) / 2;
  }
  const int pp = tid & 63, q = tid >> 6;
  const int slot = q / g.nq, sub = q - slot * g.nq;

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
    for (int base = 0; base < g.DG; base += g.slots) {
      const int dg = base + slot;
      float gr[3] = {0.f, 0.f, 0.f};   // the ND coordinate gradients, then the mask gradient
      if (dg < g.DG) {
        const S s = im.sampler(p, dg, t, pos0 + pp);
        if (s.valid) {
          for (int cc = sub; cc < g.Cdg; cc += g.nq) {
            const int c = dg * g.Cdg + cc;
            const float gcv = s_gc[c * SP + pp];
            const float gcm = gcv * s.m;
            const float* xc = im.x + (long long)c * im.chan;
#pragma unroll
            for (int j = 0; j < S::NC; ++j) {
              if (s.idx[j] < 0) continue;
              if (dxb && c < CG) dcn_acc_add(dx, gi_shadow, &dxb[(long long)c * im.chan + s.idx[j]], s.wg[j] * gcm);   // cuh:313-331, kernel.cu:279-370
              s.grad(j, xc[s.idx[j]], gcv, gr);
            }
          }
        }
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) s_red[(d * 4 + q) * TP + pp] = gr[d];
      __syncthreads();
      for (int i = tid; i < ndir * g.slots * TP; i += 256) {
        const int p2 = i % TP, dir = (i / TP) % ndir, sl = i / (ndir * TP);
        const Idx pos = pos0 + p2;
        if (base + sl < g.DG && pos < P) {
          const float* r = s_red + (dir * 4 + sl * g.nq) * TP + p2;
          float v = r[0];
          for (int j = 1; j < g.nq; ++j) v += r[j * TP];
          if (dir < ND) {
            if (doff) doff[(((long long)b * g.DG + base + sl) * ND * p.T + ND * t + dir) * p.P + pos] = v;
          } else {
            dmask[(((long long)b * g.DG + base + sl) * p.T + t) * p.P + pos] = v;
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
template <int ND, int NA>
__global__ __launch_bounds__(256) void dcn_gather_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                               const float* __restrict__ mask, const float* __restrict__ go, float* __restrict__ dw,
                                                               long long* dw_shadow, DcnP p, GrpP g) {
  using Idx = typename Sampler<ND>::Idx;
  extern __shared__ __align__(16) float smem[];
  constexpr int WGT = 4 * NA;
  const int MT = (p.K + 31) / 32, MTC = (p.CP + 31) / 32, NTILES = MT * MTC;
  float* s_S = smem;                 // [32*MTC][SP]
  float* s_go = s_S + 32 * MTC * SP; // [32*MT][SP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int tg = blockIdx.x % g.ntg;
  const int chunk = (blockIdx.x / g.ntg) % p.nchunk;
  const int t = blockIdx.x / (g.ntg * p.nchunk);
  auto tile_on = [&](int tl) {
    if (tl >= NTILES) return false;
    const int m = tl / MTC, mc = tl - m * MTC;
    int lo, hi;
    grp_span(32 * m, min(32 * m + 32, p.K), g.Kg, g.Cg, lo, hi);   // the channels the rows of this tile contract with
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
  const Idx ntile = (Idx)p.B * p.tiles_per_b, P = (Idx)p.P;
  for (Idx tile = chunk; tile < ntile; tile += p.nchunk) {
    const int b = (int)(tile / p.tiles_per_b);
    const Idx pos0 = (tile % p.tiles_per_b) * TP;
    const Image<ND> im(p, g, x, offset, mask, b);
    __syncthreads();
    build_samples<ND>(p, g, im, t, pos0 + (tid & 63), s_S, tid);
    for (int i = tid; i < 32 * MT * TP; i += 256) {
      const int k = i / TP, pp = i - k * TP;
      const Idx pos = pos0 + pp;
      s_go[k * SP + pp] = (k < p.K && pos < P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
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
          if (k < p.K && k / g.Kg == c / g.Cg) dcn_acc_add(dw, dw_shadow, &dw[((long long)k * g.Cg + c % g.Cg) * p.T + t], acc[i][j]);
        }
      }
    }
  }
}

// deterministic mode: a tensor = value of its integer shadow (every contribution went there; the tensor itself was only zero-filled)
__global__ void dcn_finalize_kernel(const long long* __restrict__ shadow, float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = dpf_det_value(shadow + 2 * i);
}

GrpP grp_params(const DcnP& p, int group, int deformable_group) {
  GrpP g;
  g.G = group;
  g.DG = deformable_group;
  g.Cg = p.C / group;
  g.Kg = p.K / group;
  g.Cdg = p.C / deformable_group;
  g.nq = deformable_group == 1 ? 4 : deformable_group == 2 ? 2 : 1;
  g.slots = 4 / g.nq;
  g.ntg = 1;
  return g;
}

// the kernels of a rank by accumulator tiles per wave (every rank's kernels have one signature)
template <int ND>
auto fwd_kernel(int na) { return na == 1 ? dcn_gather_fwd_kernel<ND, 1> : na == 2 ? dcn_gather_fwd_kernel<ND, 2> : dcn_gather_fwd_kernel<ND, 4>; }
template <int ND>
auto wgrad_kernel(int na) { return na == 1 ? dcn_gather_wgrad_kernel<ND, 1> : na == 2 ? dcn_gather_wgrad_kernel<ND, 2> : dcn_gather_wgrad_kernel<ND, 4>; }

}  // namespace

int dcn_group_check(int C, int K, int group, int deformable_group) {
  if (group < 1 || deformable_group < 1 || C % group || K % group || C % deformable_group) return DPF_ERR_INVALID_ARG;
  return DPF_OK;
}

void dcn_finalize(const long long* shadow, float* out, long long n, hipStream_t st) {
  hipLaunchKernelGGL(dcn_finalize_kernel, dim3(dpf_ew_grid(n)), dim3(256), 0, st, shadow, out, n);
}

int dcn_gather_forward(int rank, const DcnP& p, int group, int deformable_group, const float* input, const float* weight, const float* bias,
                       const float* offset, const float* mask, float* output, float* wpack, long long wpack_floats, hipStream_t st) {
  const GrpP g = grp_params(p, group, deformable_group);
  const int KT = (p.K + 31) / 32 * 32;
  const long long pack = (long long)p.T * p.CP * KT;
  if (pack > wpack_floats) return DPF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dcn_gather_repack_kernel, dim3(dpf_ew_grid(pack)), dim3(256), 0, st, weight, wpack, p.K, p.C, p.T, g.Cg, g.Kg, p.CP, KT, 0);
  const size_t lds = sizeof(float) * (size_t)p.CP * SP;
  const int na = KT <= 64 ? 1 : KT <= 128 ? 2 : 4;
  if (dcn_launch(rank == 2 ? fwd_kernel<2>(na) : fwd_kernel<3>(na), dim3((unsigned)(p.B * p.tiles_per_b)), dim3(256), lds, st, input, offset, mask,
                 (const float*)wpack, bias, output, p, g) != DPF_OK)
    return DPF_ERR_LAUNCH;
  return dpf_check_launch();
}

int dcn_gather_backward(int rank, const DcnP& p0, int group, int deformable_group, const float* input, const float* weight, const float* offset,
                        const float* mask, const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                        float* wpack, long long wpack_floats, long long* dw_shadow, long long* gi_shadow, int grad_input_channels, hipStream_t st) {
  DcnP p = p0;
  GrpP g = grp_params(p, group, deformable_group);
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, MT = (p.K + 31) / 32, MTC = CT / 32;
  const int CG = grad_input_channels < p.C ? (grad_input_channels < 0 ? 0 : grad_input_channels) : p.C;
  const long long pack = (long long)p.T * KP * CT;
  if (pack > wpack_floats) return DPF_ERR_UNSUPPORTED;
  const long long ntile = (long long)p.B * p.tiles_per_b;
  if (grad_input || grad_offset || grad_mask) {
    hipLaunchKernelGGL(dcn_gather_repack_kernel, dim3(dpf_ew_grid(pack)), dim3(256), 0, st, weight, wpack, p.K, p.C, p.T, g.Cg, g.Kg, KP, CT, 1);
    const size_t lds = sizeof(float) * ((size_t)KP * SP + (size_t)CT * SP + 3 * 4 * TP);
    if (dcn_launch(rank == 2 ? dcn_gather_bwd_data_kernel<2> : dcn_gather_bwd_data_kernel<3>, dim3((unsigned)ntile), dim3(256), lds, st, input, offset, mask,
                   (const float*)wpack, grad_output, grad_input, grad_offset, grad_mask, p, g, CG, gi_shadow) != DPF_OK)
      return DPF_ERR_LAUNCH;
  }
  if (grad_weight) {
    // (the partials of a tap's chunks meet in float atomics, or -- dw_shadow -- in integer pairs: any chunk count is reproducible there)
    long long nchunkw = 2048 / p.T;   // T <= 64 at every entry point
    if (nchunkw > ntile) nchunkw = ntile;
    p.nchunk = (int)nchunkw;
    const int na = MT * MTC <= 4 ? 1 : MT * MTC <= 8 ? 2 : 4;
    g.ntg = (MT * MTC + 4 * na - 1) / (4 * na);
    const size_t lds = sizeof(float) * ((size_t)CT * SP + (size_t)32 * MT * SP);
    if (dcn_launch(rank == 2 ? wgrad_kernel<2>(na) : wgrad_kernel<3>(na), dim3((unsigned)(p.T * p.nchunk * g.ntg)), dim3(256), lds, st, input, offset,
                   mask, grad_output, grad_weight, dw_shadow, p, g) != DPF_OK)
      return DPF_ERR_LAUNCH;
  }
  return DPF_OK;
}
