// Deformable 3-D convolution with group > 1 and / or deformable_group > 1 (deform_conv_cuda.cu:65-66,84-121; deform_im2col_cuda.cuh:222-232):
//   weight [K][C/group][T], offset [B][deformable_group * 3T][P]; input channel c is sampled with the offsets of deformable group
//   c / (C/deformable_group); output channel k of conv group k / (K/group) contracts over that group's C/group input channels.
// The grouping is a kernel argument: one call is a fixed number of launches (forward: repack + 1; backward: repack + 2) whatever the group
// counts, and a workgroup owns 64 output voxels for ALL groups, like the gather tier of dcn3d.hip.
//   sampling   : the trilinear corner block of a (voxel, tap) is computed once per deformable group and reused for every channel of that
//                group (the reference recomputes it per channel); the sampling rule itself is dcn_internal.h's, shared with dcn3d.hip.
//   products   : the grouped weight is repacked as the block-diagonal [K x C] matrix of a tap (zeros off the blocks); a 32-row tile of the
//                matrix instruction walks only the reduce range of the conv groups its rows belong to, so groups of >= 32 rows cost exactly
//                their own products and narrower groups share a tile.  (Rows of different groups that share a tile see each other's samples
//                multiplied by an exact zero: invisible for finite data, a NaN for a non-finite sample.)
//   grad_offset: the workgroup holds gcol = W^T . grad_output of its tile for all channels, sums the three coordinate gradients per deformable
//                group over that group's channels (in whichever conv groups they sit) in a fixed order and stores each element once: no
//                atomics, bitwise reproducible in every mode.
//   grad_input, grad_weight: dcn_acc_add (dcn_internal.h) -- float atomics, or in deterministic mode the integer shadows of the workspace.
// PRECISION: every product here runs on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32) for every setting of dpf_set_f32_matrix_path;
// the split-operand (f16 / bf16 component) constructions of the single-group tiers and their range guards are NOT extended to this path.
#include "dpf_common.h"
#include "dcn_internal.h"

namespace {

constexpr int TP = 64;          // output voxels per workgroup
constexpr int SP = TP + 1;      // padded LDS row

struct GrpP {
  int G, DG;          // conv groups, deformable groups
  int Cg, Kg, Cdg;    // C / G, K / G, C / DG
  // the four thread rows (tid >> 6) of a workgroup sample `slots` deformable groups at a time, `nq` rows per group (slots * nq = 4)
  int slots, nq;
};

// first and one-past-last index on the other side of the block-diagonal weight for rows [r0, r1) of one side:
// rows of width `rw` per group, `ow` per group on the other side
__device__ __forceinline__ void grp_span(int r0, int r1, int rw, int ow, int& lo, int& hi) {
  lo = (r0 / rw) * ow;
  hi = ((r1 - 1) / rw + 1) * ow;
}

// the block-diagonal matrix of every tap, zero-padded: mode 0 (forward) wt[t][c][k], mode 1 (backward) wt[t][k][c]; `rows` x `RT` per tap
__global__ void dcng_repack_kernel(const float* __restrict__ w, float* __restrict__ wt, int K, int C, int T, int Cg, int Kg, int rows, int RT, int mode) {
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

// S[c][pp] = trilinear sample of channel c at voxel pp of the tile, for tap t, every channel of every deformable group
// (row C of an odd channel count is zeroed: the matrix instruction reduces two channels at a time)
__device__ __forceinline__ void grp_build_samples(const DcnP& p, const GrpP& g, const float* __restrict__ xb, const float* __restrict__ off_b, int t,
                                                  long long pos, float* s_S, int tid) {
  const int pp = tid & 63, q = tid >> 6;
  const int slot = q / g.nq, sub = q - slot * g.nq;
  const long long chan = (long long)p.D * p.H * p.W;
  for (int dg = slot; dg < g.DG; dg += g.slots) {
    const Corner cn = make_corner(p, off_b + (long long)dg * 3 * p.T * p.P, t, pos);
    long long idx[8];
    float wg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) idx[j] = corner_index(p, cn, j, wg[j]);
    for (int cc = sub; cc < g.Cdg; cc += g.nq) {
      const int c = dg * g.Cdg + cc;
      const float* xc = xb + (long long)c * chan;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (idx[j] >= 0) v += wg[j] * xc[idx[j]];
      s_S[c * SP + pp] = v;
    }
  }
  if (q == 0 && p.CP > p.C) s_S[p.C * SP + pp] = 0.f;
}

// ------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void dcng_fwd_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                       const float* __restrict__ wt /*[T][CP][KT]*/, const float* __restrict__ bias,
                                                       float* __restrict__ out, DcnP p, GrpP g) {
  extern __shared__ __align__(16) float smem[];
  float* s_S = smem;   // [CP][SP]
  const int MT = (p.K + 31) / 32, KT = 32 * MT, NTILES = 2 * MT;   // K <= 128: at most 8 (row tile, voxel half) tiles, two per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const long long pos0 = (long long)(blockIdx.x % p.tiles_per_b) * TP;
  const float* xb = x + (long long)b * p.C * p.D * p.H * p.W;
  const float* off_b = offset + (long long)b * g.DG * 3 * p.T * p.P;

  f32x16 acc[2];
  int cp0[2], cp1[2];   // reduce range of the tile, in channel pairs
#pragma unroll
  for (int i = 0; i < 2; ++i) {
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
    grp_build_samples(p, g, xb, off_b, t, pos0 + (tid & 63), s_S, tid);
    __syncthreads();
    const float* wtt = wt + (long long)t * p.CP * KT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
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
  for (int i = 0; i < 2; ++i) {
    const int tile = wave + 4 * i;
    if (tile < NTILES) {
      const int m = tile >> 1, nt = tile & 1;
      const long long pos = pos0 + nt * 32 + l31;
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

// ------------------------------------------------------------------------------------------ backward: offset + input
// gcol[c][p] = sum_k W[k][c][t] * go[k][p] over the output channels of c's conv group, for all channels of the tile; then per deformable
// group the coordinate gradients summed over its channels (grad_offset, one plain store per element) and the sampler's adjoint into the
// channels [0, CG) of grad_input (dcn_acc_add).
__global__ __launch_bounds__(256) void dcng_bwd_data_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                            const float* __restrict__ wt2 /*[T][KP][CT]*/, const float* __restrict__ go,
                                                            float* __restrict__ dx, float* __restrict__ doff, DcnP p, GrpP g, int CG, long long* gi_shadow) {
  extern __shared__ __align__(16) float smem[];
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, NTILES = 2 * (CT / 32);   // C <= 128: at most 8 tiles, two per wave
  float* s_go = smem;                    // [KP][SP]
  float* s_gc = s_go + KP * SP;          // [CT][SP]
  float* s_red = s_gc + CT * SP;         // [3][4][TP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_b;
  const long long pos0 = (long long)(blockIdx.x % p.tiles_per_b) * TP;
  const long long chan = (long long)p.D * p.H * p.W;
  const float* xb = x + (long long)b * p.C * chan;
  float* dxb = dx + (long long)b * p.C * chan;
  const float* off_b = offset + (long long)b * g.DG * 3 * p.T * p.P;
  float* doff_b = doff + (long long)b * g.DG * 3 * p.T * p.P;

  for (int i = tid; i < KP * TP; i += 256) {
    const int k = i / TP, pp = i - k * TP;
    const long long pos = pos0 + pp;
    s_go[k * SP + pp] = (k < p.K && pos < p.P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
  }
  int kp0[2], kp1[2];   // reduce range of the tile, in output-channel pairs
#pragma unroll
  for (int i = 0; i < 2; ++i) {
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
    for (int i = 0; i < 2; ++i) {
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
    // thread = (voxel pp, row q): row q serves deformable group base + slot, the channels sub, sub + nq, ... of it
    for (int base = 0; base < g.DG; base += g.slots) {
      const int dg = base + slot;
      float gd = 0.f, gh = 0.f, gw = 0.f;
      if (dg < g.DG) {
        const Corner cn = make_corner(p, off_b + (long long)dg * 3 * p.T * p.P, t, pos0 + pp);
        if (cn.valid) {
          long long idx[8];
          float wg[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) idx[j] = corner_index(p, cn, j, wg[j]);
          for (int cc = sub; cc < g.Cdg; cc += g.nq) {
            const int c = dg * g.Cdg + cc;
            const float gcv = s_gc[c * SP + pp];
            const float* xc = xb + (long long)c * chan;
            float* dxc = dxb + (long long)c * chan;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (idx[j] < 0) continue;
              const int jd = (j >> 2) & 1, jh = (j >> 1) & 1, jw = j & 1;
              if (c < CG) dcn_acc_add(dx, gi_shadow, &dxc[idx[j]], wg[j] * gcv);      // cuh:313-331
              const float v = xc[idx[j]] * gcv;
              const float fd = jd ? cn.ld : 1.f - cn.ld, fh = jh ? cn.lh : 1.f - cn.lh, fw = jw ? cn.lw : 1.f - cn.lw;
              gd += (jd ? 1.f : -1.f) * fh * fw * v;                                  // cuh:131-187
              gh += (jh ? 1.f : -1.f) * fd * fw * v;
              gw += (jw ? 1.f : -1.f) * fd * fh * v;
            }
          }
        }
      }
      s_red[(0 * 4 + q) * TP + pp] = gd;
      s_red[(1 * 4 + q) * TP + pp] = gh;
      s_red[(2 * 4 + q) * TP + pp] = gw;
      __syncthreads();
      for (int i = tid; i < 3 * g.slots * TP; i += 256) {
        const int p2 = i % TP, dir = (i / TP) % 3, sl = i / (3 * TP);
        const long long pos = pos0 + p2;
        if (base + sl < g.DG && pos < p.P) {
          const float* r = s_red + (dir * 4 + sl * g.nq) * TP + p2;
          float s = r[0];
          for (int j = 1; j < g.nq; ++j) s += r[j * TP];
          doff_b[((long long)(base + sl) * 3 * p.T + 3 * t + dir) * p.P + pos] = s;
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------ backward: weight
// grid = T * nchunk; block = one tap, a strided set of voxel tiles; dW[k][c - c0(group of k)][t] += sum_p go[k][p] * S[c][p] for the (k, c) of
// one conv group.  Of the 32 x 32 tiles of the [K x C] product only those that touch a diagonal block are computed.
__global__ __launch_bounds__(256) void dcng_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ offset, const float* __restrict__ go,
                                                         float* __restrict__ dw, long long* dw_shadow, DcnP p, GrpP g) {
  extern __shared__ __align__(16) float smem[];
  const int MT = (p.K + 31) / 32, MTC = (p.CP + 31) / 32, NTILES = MT * MTC;   // at most 16: four per wave
  float* s_S = smem;                 // [32*MTC][SP]
  float* s_go = s_S + 32 * MTC * SP; // [32*MT][SP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int t = blockIdx.x / p.nchunk;
  const int chunk = blockIdx.x % p.nchunk;
  f32x16 acc[4];
  bool on[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    const int tl = wave + 4 * i;
    on[i] = false;
    if (tl < NTILES) {
      const int m = tl / MTC, mc = tl - m * MTC;
      int lo, hi;
      grp_span(32 * m, min(32 * m + 32, p.K), g.Kg, g.Cg, lo, hi);   // the channels the rows of this tile contract with
      on[i] = 32 * mc < hi && lo < min(32 * mc + 32, p.C);
    }
  }
  // zero the padded rows once
  for (int i = tid; i < 32 * MTC * SP; i += 256) s_S[i] = 0.f;
  const long long ntile = (long long)p.B * p.tiles_per_b;
  const long long chan = (long long)p.D * p.H * p.W;
  for (long long tile = chunk; tile < ntile; tile += p.nchunk) {
    const int b = (int)(tile / p.tiles_per_b);
    const long long pos0 = (tile % p.tiles_per_b) * TP;
    const float* xb = x + (long long)b * p.C * chan;
    const float* off_b = offset + (long long)b * g.DG * 3 * p.T * p.P;
    __syncthreads();
    grp_build_samples(p, g, xb, off_b, t, pos0 + (tid & 63), s_S, tid);
    for (int i = tid; i < 32 * MT * TP; i += 256) {
      const int k = i / TP, pp = i - k * TP;
      const long long pos = pos0 + pp;
      s_go[k * SP + pp] = (k < p.K && pos < p.P) ? go[((long long)b * p.K + k) * p.P + pos] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (on[i]) {
        const int tl = wave + 4 * i;
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
  for (int i = 0; i < 4; ++i) {
    if (on[i]) {
      const int tl = wave + 4 * i;
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

GrpP grp_params(const DcnP& p, int group, int deformable_group) {
  GrpP g;
  g.G = group;
  g.DG = deformable_group;
  g.Cg = p.C / group;
  g.Kg = p.K / group;
  g.Cdg = p.C / deformable_group;
  g.nq = deformable_group == 1 ? 4 : deformable_group == 2 ? 2 : 1;
  g.slots = 4 / g.nq;
  return g;
}

}  // namespace

int dcn_group_check(int C, int K, int group, int deformable_group) {
  if (group < 1 || deformable_group < 1 || C % group || K % group || C % deformable_group) return DPF_ERR_INVALID_ARG;
  return DPF_OK;
}

long long dcn_grouped_pack_floats(const DcnP& p, bool backward) {
  const long long KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, KT = (p.K + 31) / 32 * 32;
  return backward ? (long long)p.T * KP * CT : (long long)p.T * p.CP * KT;
}

int dcn_grouped_forward(const DcnP& p, int group, int deformable_group, const float* input, const float* weight, const float* bias,
                        const float* offset, float* output, float* wpack, hipStream_t st) {
  const GrpP g = grp_params(p, group, deformable_group);
  const int KT = (p.K + 31) / 32 * 32;
  hipLaunchKernelGGL(dcng_repack_kernel, dim3(dpf_ew_grid(dcn_grouped_pack_floats(p, false))), dim3(256), 0, st, weight, wpack, p.K, p.C, p.T, g.Cg, g.Kg,
                     p.CP, KT, 0);
  const size_t lds = sizeof(float) * (size_t)p.CP * SP;
  if (dcn_launch(dcng_fwd_kernel, dim3((unsigned)(p.B * p.tiles_per_b)), dim3(256), lds, st, input, offset, (const float*)wpack, bias, output, p, g) != DPF_OK)
    return DPF_ERR_LAUNCH;
  return dpf_check_launch();
}

int dcn_grouped_backward(const DcnP& p0, int group, int deformable_group, const float* input, const float* weight, const float* offset,
                         const float* grad_output, float* grad_input, float* grad_offset, float* grad_weight, float* wpack, long long* dw_shadow,
                         long long* gi_shadow, int grad_input_channels, hipStream_t st) {
  DcnP p = p0;
  const GrpP g = grp_params(p, group, deformable_group);
  const int KP = (p.K + 1) & ~1, CT = (p.CP + 31) / 32 * 32, MT = (p.K + 31) / 32;
  const int CG = grad_input_channels < p.C ? (grad_input_channels < 0 ? 0 : grad_input_channels) : p.C;
  hipLaunchKernelGGL(dcng_repack_kernel, dim3(dpf_ew_grid(dcn_grouped_pack_floats(p, true))), dim3(256), 0, st, weight, wpack, p.K, p.C, p.T, g.Cg, g.Kg,
                     KP, CT, 1);
  const long long ntile = (long long)p.B * p.tiles_per_b;
  {
    const size_t lds = sizeof(float) * ((size_t)KP * SP + (size_t)CT * SP + 3 * 4 * TP);
    if (dcn_launch(dcng_bwd_data_kernel, dim3((unsigned)ntile), dim3(256), lds, st, input, offset, (const float*)wpack, grad_output, grad_input, grad_offset, p,
                   g, CG, gi_shadow) != DPF_OK)
      return DPF_ERR_LAUNCH;
  }
  // (the partials of a tap's chunks meet in float atomics, or -- dw_shadow -- in integer pairs: any chunk count is reproducible there)
  long long nchunkw = 2048 / p.T;
  if (nchunkw < 1) nchunkw = 1;
  if (nchunkw > ntile) nchunkw = ntile;
  p.nchunk = (int)nchunkw;
  const size_t lds = sizeof(float) * ((size_t)CT * SP + (size_t)32 * MT * SP);
  return dcn_launch(dcng_wgrad_kernel, dim3((unsigned)(p.T * p.nchunk)), dim3(256), lds, st, input, offset, grad_output, grad_weight, dw_shadow, p, g);
}
