// Shared (host + device) layout of the level table of the V-cycle tail
// (csrc/hip/pmg_tail.h, host twin in csrc/host/bdx_host.cpp; built by
// ops/kernels.py: PmgTail).  int64 words, kTailWords per level, then the
// Chebyshev coefficients as doubles, (a, b) per step:
//   [0..20]  the level's lattice descriptor (bdx_lattice.h)
//   [21..27] pointers S, dinv, bc (bytes), r, z, d, y
//   [28..30] pointers cidx, cw, fpos: the tables to the next level (0: last)
//   [31]     number of Chebyshev steps   [32] word offset of their (a, b)
// r and z of the first level are call arguments (the caller's vectors).
#pragma once
#include <cstdint>

#include "bdx_lattice.h"

constexpr int kTailWords = 40;
constexpr int kTailMaxLevels = 16;
constexpr int64_t kTailMaxNodes = 32768;
enum {
  kTailS = 21,
  kTailDinv,
  kTailBc,
  kTailR,
  kTailZ,
  kTailD,
  kTailY,
  kTailCidx,
  kTailCw,
  kTailFpos,
  kTailNcoef,
  kTailCoef
};

// A level the tail can run: lattice layout, degree 1, no ghost planes (one
// rank), at most kTailMaxNodes nodes.
inline bool tail_level_ok(const BdxLattice& l) {
  if (l.tsy || l.P != 1) return false;
  for (int a = 0; a < 3; ++a)
    if (l.n[a] < 1 || l.L[a] != l.n[a] + 1 || l.gh[a] != 0 || l.L[a] > kTailMaxNodes) return false;
  if (l.L[0] * l.L[1] * l.L[2] > kTailMaxNodes) return false;
  return l.ld >= l.L[2] && l.ld <= l.L[2] + 64;
}

// The table's own consistency: level count, pointers, coefficient ranges;
// `pair_ok(coarse, fine)`: the transfer kernels' check of a level pair.
template <typename PairOk>
inline bool tail_table_ok(const int64_t* tab, int nlev, int64_t nwords, PairOk pair_ok) {
  if (!tab || nlev < 1 || nlev > kTailMaxLevels || nwords < static_cast<int64_t>(nlev) * kTailWords)
    return false;
  for (int l = 0; l < nlev; ++l) {
    const int64_t* w = tab + static_cast<int64_t>(l) * kTailWords;
    const BdxLattice lat = BdxLattice::from(w);
    if (!tail_level_ok(lat)) return false;
    if (!w[kTailS] || !w[kTailDinv] || !w[kTailBc] || !w[kTailD] || !w[kTailY]) return false;
    if (l > 0 && (!w[kTailR] || !w[kTailZ])) return false;
    const int64_t nc = w[kTailNcoef], off = w[kTailCoef];
    if (nc < 1 || nc > nwords || off < static_cast<int64_t>(nlev) * kTailWords ||
        off + 2 * nc > nwords)
      return false;
    if (l < nlev - 1) {
      if (!w[kTailCidx] || !w[kTailCw] || !w[kTailFpos]) return false;
      if (!pair_ok(BdxLattice::from(w + kTailWords), lat)) return false;
    }
  }
  return true;
}
