// CPU replay of the rank sort of dualpixelface_amd/csrc/metrics.hip with the grid sizes, workspace layout and index arithmetic of
// csrc/metrics_plan.h -- the same histogram -> scan -> scatter, wave by wave and round by round, inside a heap block of exactly
// dpf_metric_ranks_workspace_bytes() bytes.  Build it with the host sanitizers and run it (no GPU involved):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idualpixelface_amd/csrc tools/metrics_plan_check.cpp -o /tmp/metrics_plan_check
//
// A slot computed past its array is an address-sanitizer report; a wrong rank is a non-zero exit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "metrics_plan.h"

using namespace dpf_metrics;

static uint32_t bits_of(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// torch's order: NaN last, -0.0 == +0.0
static bool less_torch(float a, float b) { return (!std::isnan(a) && std::isnan(b)) || a < b; }

static int check(long long B, long long n, const std::vector<float>& vals, int negate) {
  const RanksPlan pl = ranks_plan(B, n);
  if (pl.bytes <= 0) return 1;
  std::vector<char> heap((size_t)pl.bytes);                          // exactly the bytes the query promises
  char* w = heap.data();
  uint32_t* keys[2] = {(uint32_t*)(w + pl.keys[0]), (uint32_t*)(w + pl.keys[1])};
  uint32_t* idx[2] = {(uint32_t*)(w + pl.idx[0]), (uint32_t*)(w + pl.idx[1])};
  uint32_t* hist = (uint32_t*)(w + pl.hist);
  uint32_t* basep = (uint32_t*)(w + pl.base);
  std::vector<int> ranks((size_t)(B * n), -1);
  const long long blocks = sort_blocks(n);
  for (int pass = 0; pass < 4; ++pass) {
    const int src = (pass - 1) & 1, dst = pass & 1, shift = 8 * pass;
    auto key_at = [&](long long b, long long i) { return pass == 0 ? sort_key_bits(bits_of(vals[b * n + i]), negate) : keys[src][b * n + i]; };
    for (long long b = 0; b < B; ++b)                                 // sort_hist_kernel
      for (long long blk = 0; blk < blocks; ++blk)
        for (int wv = 0; wv < kWaves; ++wv) {
          const long long chunk = blk * kWaves + wv;
          if (chunk >= pl.chunks) continue;
          uint32_t h[kRadix] = {0};
          for (int r = 0; r < kSortRounds; ++r)
            for (int lane = 0; lane < 64; ++lane) {
              const long long i = sort_elem(chunk, r, lane);
              if (i < n) ++h[(key_at(b, i) >> shift) & 255u];
            }
          for (int d = 0; d < kRadix; ++d) hist[hist_slot(b, pl.chunks, chunk, d)] = h[d];
        }
    for (long long b = 0; b < B; ++b) {                               // sort_scan_kernel
      uint32_t run[kRadix];
      for (int d = 0; d < kRadix; ++d) {
        run[d] = 0;
        for (long long c = 0; c < pl.chunks; ++c) {
          const long long slot = hist_slot(b, pl.chunks, c, d);
          const uint32_t v = hist[slot];
          hist[slot] = run[d];
          run[d] += v;
        }
      }
      uint32_t acc = 0;
      for (int d = 0; d < kRadix; ++d) {
        basep[b * kRadix + d] = acc;
        acc += run[d];
      }
      if ((long long)acc != n) return 2;
    }
    for (long long b = 0; b < B; ++b)                                 // sort_scatter_kernel
      for (long long blk = 0; blk < blocks; ++blk)
        for (int wv = 0; wv < kWaves; ++wv) {
          const long long chunk = blk * kWaves + wv;
          if (chunk >= pl.chunks) continue;
          uint32_t off[kRadix];
          for (int d = 0; d < kRadix; ++d) off[d] = basep[b * kRadix + d] + hist[hist_slot(b, pl.chunks, chunk, d)];
          for (int r = 0; r < kSortRounds; ++r)
            for (int lane = 0; lane < 64; ++lane) {                   // lanes in order = "lower lanes with my digit" + running offset
              const long long i = sort_elem(chunk, r, lane);
              if (i >= n) continue;
              const uint32_t key = key_at(b, i);
              const uint32_t id = pass == 0 ? (uint32_t)i : idx[src][b * n + i];
              const uint32_t pos = off[(key >> shift) & 255u]++;
              if ((long long)pos >= n || (long long)id >= n) return 3;
              if (pass == 3) {
                ranks[b * n + id] = (int)pos;
              } else {
                keys[dst][b * n + pos] = key;
                idx[dst][b * n + pos] = id;
              }
            }
        }
  }
  for (long long b = 0; b < B; ++b) {                                 // against a stable sort in torch's order
    std::vector<long long> order((size_t)n);
    std::iota(order.begin(), order.end(), 0LL);
    std::stable_sort(order.begin(), order.end(), [&](long long x, long long y) {
      const float fx = vals[b * n + x], fy = vals[b * n + y];
      return negate ? less_torch(-fx, -fy) : less_torch(fx, fy);
    });
    for (long long k = 0; k < n; ++k)
      if (ranks[b * n + order[k]] != (int)k) return 4;
  }
  return 0;
}

int main() {
  const long long lengths[] = {1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 8192, 8193, 70001};
  const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
  const float special[] = {0.f, -0.f, den, -den, inf, -inf, 1.f, -1.f, 3.5f, -3.5f, 2 * den, 1e-38f};
  int bad = 0;
  for (long long n : lengths)
    for (int set = 0; set < 4; ++set)
      for (int negate = 0; negate < 2; ++negate) {
        const long long B = 2;
        std::vector<float> v((size_t)(B * n));
        uint32_t s = 12345u + (uint32_t)n * 7u + (uint32_t)set;
        for (long long i = 0; i < B * n; ++i) {
          s = s * 1664525u + 1013904223u;
          const uint32_t r = s >> 8;
          if (set == 0) v[i] = (float)(r % 7u) - 3.f;                          // heavy ties
          else if (set == 1) v[i] = 2.5f;                                      // all equal
          else if (set == 2) v[i] = (i / n ? -1.f : 1.f) * (float)(i % n);     // sorted / reversed
          else v[i] = (r % 5u == 0u) ? special[r % 12u] : ((float)(r % 2001u) - 1000.f) * 1e-3f;
        }
        if (set == 3) v[(size_t)(n / 2)] = std::numeric_limits<float>::quiet_NaN();
        const int rc = check(B, n, v, negate);
        if (rc) {
          printf("FAIL n=%lld set=%d negate=%d rc=%d\n", n, set, negate, rc);
          ++bad;
        }
      }
  // layouts: offsets ascending, aligned, inside the total; the reduction grid inside what one fold block reads
  for (long long n : {1LL, 35LL, 1024LL, 1025LL, 262144LL, 262145LL, 1572864LL, kMaxN}) {
    const RanksPlan r = ranks_plan(4, n);
    const AffinePlan a = affine_plan(4, n);
    const bool ok = r.bytes > 0 && r.idx[0] >= 4 * n * 4 && r.keys[1] >= r.idx[0] + 4 * n * 4 && r.idx[1] >= r.keys[1] + 4 * n * 4 &&
                    r.hist >= r.idx[1] + 4 * n * 4 && r.base >= r.hist + 4 * r.chunks * kRadix * 4 && r.bytes >= r.base + 4 * kRadix * 4 &&
                    r.chunks * kSortChunk >= n && (r.chunks - 1) * kSortChunk < n && sort_blocks(n) * kWaves >= r.chunks &&
                    a.st >= 4LL * red_blocks(n) * kAffineValues * 8 && a.res >= a.st + 4 * 2 * 8 && a.bytes >= a.res + 4 * 3 * 8 &&
                    (r.idx[0] | r.keys[1] | r.idx[1] | r.hist | r.base | a.st | a.res) % 16 == 0 && red_blocks(n) >= 1 &&
                    red_blocks(n) <= kMaxRedBlocks;
    if (!ok) {
      printf("FAIL layout n=%lld\n", n);
      ++bad;
    }
  }
  if (ranks_plan(1, kMaxN + 1).bytes != -1 || ranks_plan(0, 5).bytes != -1 || affine_plan(kMaxB + 1, 5).bytes != -1) {
    printf("FAIL refusals\n");
    ++bad;
  }
  printf(bad ? "metrics plan check: %d failures\n" : "metrics plan check: ok\n", bad);
  return bad ? 1 : 0;
}
