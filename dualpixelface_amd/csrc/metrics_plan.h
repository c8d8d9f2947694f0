// Host-side plan of the validation-metric kernels (metrics.hip): grid sizes, workspace layout and the index arithmetic of the rank sort.
// Plain C++ (no HIP): tools/metrics_plan_check.cpp builds it with the address / undefined-behaviour sanitizers and replays the sort's
// histogram -> scan -> scatter on the CPU with exactly these functions.
#pragma once
#include <stdint.h>
#include "dpf_reduce.h"

#ifdef __HIPCC__
#define DPF_HD __host__ __device__
#else
#define DPF_HD
#endif

namespace dpf_metrics {

constexpr int kBlock = 256;              // threads per block of every metric kernel (4 waves)
constexpr int kWaves = 4;
constexpr int kRedItems = 4;             // elements per thread before the reduction grid stops growing
constexpr int kMaxRedBlocks = 256;       // reduction blocks per sample: the fold reads them with one block in a fixed order
constexpr int kRadix = 256;              // 8-bit digits, four passes over a 32-bit key
constexpr int kSortChunk = 2048;         // elements one wave ranks, in input order (32 rounds of 64 lanes)
constexpr int kSortRounds = kSortChunk / 64;
constexpr long long kMaxN = 2147483646LL;   // indices and ranks stay 32-bit: n < 2^31 - 1
constexpr int kMaxB = 65535;             // samples ride on gridDim.y

inline long long align16(long long v) { return (v + 15) & ~15LL; }

// blocks per sample of a reduction pass
inline int red_blocks(long long n) { return dpf_red_rows(n, (long long)kBlock * kRedItems, kMaxRedBlocks); }

inline bool shape_ok(long long B, long long n) { return B > 0 && B <= kMaxB && n > 0 && n <= kMaxN; }

// absolute_dp / normal_dp: [B][red_blocks][NV] doubles of partial sums
inline long long reduce_bytes(long long B, long long n, int nv) {
  if (!shape_ok(B, n)) return -1;
  return align16(B * red_blocks(n) * nv * (long long)sizeof(double));
}

constexpr int kAbsValues = 9;            // 8 sums + count
constexpr int kNormalValues = 3;
constexpr int kAffineValues = 9;         // 8 of a fit pass, 9 of the rank-moment pass

struct AffinePlan {
  long long part;                        // byte offsets into the workspace
  long long st;                          // [B][2] doubles: (s, t) of the latest fit
  long long res;                         // [B][3] doubles: wmae, wrmse, 1 - spearman per sample
  long long bytes;
};

inline AffinePlan affine_plan(long long B, long long n) {
  AffinePlan p = {0, 0, 0, -1};
  if (!shape_ok(B, n)) return p;
  p.part = 0;
  p.st = align16(B * red_blocks(n) * kAffineValues * (long long)sizeof(double));
  p.res = p.st + align16(B * 2 * (long long)sizeof(double));
  p.bytes = p.res + align16(B * 3 * (long long)sizeof(double));
  return p;
}

// ---- rank sort
inline long long sort_chunks(long long n) { return (n + kSortChunk - 1) / kSortChunk; }             // waves that own elements, per sample
inline long long sort_blocks(long long n) { return (sort_chunks(n) + kWaves - 1) / kWaves; }        // gridDim.x

struct RanksPlan {
  long long keys[2], idx[2];             // ping-pong (key, index) arrays, [B][n] uint32 each (byte offsets)
  long long hist;                        // [B][chunks][256] uint32: digit counts, turned into exclusive offsets inside a digit by the scan
  long long base;                        // [B][256] uint32: first output position of each digit
  long long chunks;
  long long bytes;
};

inline RanksPlan ranks_plan(long long B, long long n) {
  RanksPlan p = {{0, 0}, {0, 0}, 0, 0, 0, -1};
  if (!shape_ok(B, n)) return p;
  const long long arr = align16(B * n * (long long)sizeof(uint32_t));
  p.chunks = sort_chunks(n);
  p.keys[0] = 0;
  p.idx[0] = arr;
  p.keys[1] = 2 * arr;
  p.idx[1] = 3 * arr;
  p.hist = 4 * arr;
  p.base = p.hist + align16(B * p.chunks * kRadix * (long long)sizeof(uint32_t));
  p.bytes = p.base + align16(B * kRadix * (long long)sizeof(uint32_t));
  return p;
}

// element index of (chunk, round, lane); the caller compares it with n
DPF_HD inline long long sort_elem(long long chunk, int round, int lane) { return chunk * kSortChunk + (long long)round * 64 + lane; }
// slot of (sample, chunk, digit) in the histogram table
DPF_HD inline long long hist_slot(long long b, long long chunks, long long chunk, int digit) { return (b * chunks + chunk) * kRadix + digit; }

// Order-preserving 32-bit key of a float, torch's sort order: -0.0 == +0.0 (one key), every NaN last (one key), ties are left to the
// stable scatter.  Integer-only, so denormals keep their order whatever the float mode.  negate: the key of -v.
DPF_HD inline uint32_t sort_key_bits(uint32_t u, int negate) {
  if (negate) u ^= 0x80000000u;
  const uint32_t mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u) return 0xffffffffu;
  if (mag == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace dpf_metrics
