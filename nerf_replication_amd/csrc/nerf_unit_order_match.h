// Unit order of one hidden layer from its co-dead counts (include/nerf_mi355x_order.h has the contract).
// Plain C++, host only, no HIP: the library's nerf_unit_order_match calls it, tests/unit_order_host.cpp compiles it alone.
//
// counts[i * 256 + j], i != j: the number of 32-point tiles in which units i and j of the layer were both off at every point.  Only
// the upper triangle (i < j) is read.  The rule, a function of `counts` alone, ties included:
//   1. the pairs i < j sorted by (count descending, i ascending, j ascending);
//   2. walking that list, a pair is taken when both of its units are still free, until 128 pairs exist (the list holds every pair,
//      so two free units always still have theirs ahead: the walk ends with all 256 units paired);
//   3. the 128 pairs sorted by (count descending, lower unit ascending) go to k-steps s = 0 .. 127 in that order: the deadest pairs
//      land in the first 4-k-step groups of the consuming GEMM;
//   4. k-step s = 16 t + r reads the register pair {act_feat(t, r, 0), act_feat(t, r, 1)} (nerf_layout.h): the pair's lower unit goes
//      to position act_feat(t, r, 0), lane half 0, the higher one to act_feat(t, r, 1).
// order[position] = the original unit that sits at `position` of the permuted layer.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nerf_layout.h"

namespace nerf {

inline void unit_order_match(const int32_t* counts, int32_t* order) {
  constexpr int N = kHidden;
  constexpr int kPairs = N * (N - 1) / 2;
  struct Pair { int32_t c; int16_t i, j; };
  // step 1: the pairs in (i, j) ascending order, sorted STABLY by count descending.  Counts are tile counts, a small range: one
  // counting pass (a count's slot range, then the pairs dropped into it in order); a comparison sort only for a range beyond 2^16
  int64_t lo = counts[1], hi = counts[1];
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j) { lo = std::min<int64_t>(lo, counts[i * N + j]); hi = std::max<int64_t>(hi, counts[i * N + j]); }
  std::vector<Pair> pairs(kPairs);
  if (hi - lo < (1 << 16)) {
    std::vector<int32_t> start(hi - lo + 2, 0);                // start[k + 1] counts the pairs whose (hi - count) is k
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) ++start[hi - counts[i * N + j] + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) pairs[start[hi - counts[i * N + j]]++] = Pair{counts[i * N + j], (int16_t)i, (int16_t)j};
  } else {
    int n = 0;
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) pairs[n++] = Pair{counts[i * N + j], (int16_t)i, (int16_t)j};
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.c > b.c; });
  }
  bool taken[N] = {};
  std::vector<Pair> chosen;
  chosen.reserve(N / 2);
  for (const Pair& p : pairs) {
    if (taken[p.i] || taken[p.j]) continue;
    taken[p.i] = taken[p.j] = true;
    chosen.push_back(p);
    if ((int)chosen.size() == N / 2) break;
  }
  std::sort(chosen.begin(), chosen.end(), [](const Pair& a, const Pair& b) { return a.c != b.c ? a.c > b.c : a.i < b.i; });
  for (int s = 0; s < N / 2; ++s) {
    order[act_feat(s >> 4, s & 15, 0)] = chosen[s].i;
    order[act_feat(s >> 4, s & 15, 1)] = chosen[s].j;
  }
}

}  // namespace nerf
