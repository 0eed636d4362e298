// Shared (host + device) layout of the level table of the V-cycle tail
// (csrc/hip/pmg_tail.h, host twin in csrc/host/bdx_host_mg.cpp; built by
// ops/kernels.py: PmgTail) and its decoder.  int64 words, kTailWords per level, then the
// Chebyshev coefficients as doubles, (a, b) per step:
//   [0..20]  the level's lattice descriptor (bdx_lattice.h)
//   [21..27] pointers S, dinv, bc (bytes), r, z, d, y
//   [28..30] pointers cidx, cw, fpos: the tables to the next level (0: last)
//   [31]     number of Chebyshev steps   [32] word offset of their (a, b)
// r and z of the first level are call arguments (the caller's vectors).
#pragma once
#include <cstddef>
#include <cstdint>

#include "bdx_mg_bodies.h"

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

// One level's words by name: what ops/kernels.py: PmgTail fills (through the
// mirror ops/hip_api.py: TailLevelWords).  Pointers travel as words.
struct BdxTailLevelWords {
  BdxLattice lat;
  int64_t S, dinv, bc, r, z, d, y;
  int64_t cidx, cw, fpos;
  int64_t ncoef, coef;
  int64_t pad[kTailWords - kTailCoef - 1];
};
static_assert(sizeof(BdxTailLevelWords) == kTailWords * 8, "a level is kTailWords words");
#define BDX_TAIL_SLOT(FIELD, SLOT)                                      \
  static_assert(offsetof(BdxTailLevelWords, FIELD) == (SLOT) * 8, \
                #FIELD " is not at word " #SLOT)
BDX_TAIL_SLOT(S, kTailS);
BDX_TAIL_SLOT(dinv, kTailDinv);
BDX_TAIL_SLOT(bc, kTailBc);
BDX_TAIL_SLOT(r, kTailR);
BDX_TAIL_SLOT(z, kTailZ);
BDX_TAIL_SLOT(d, kTailD);
BDX_TAIL_SLOT(y, kTailY);
BDX_TAIL_SLOT(cidx, kTailCidx);
BDX_TAIL_SLOT(cw, kTailCw);
BDX_TAIL_SLOT(fpos, kTailFpos);
BDX_TAIL_SLOT(ncoef, kTailNcoef);
BDX_TAIL_SLOT(coef, kTailCoef);
#undef BDX_TAIL_SLOT

// A level the tail can run: lattice layout, degree 1, no ghost planes (one
// rank), at most kTailMaxNodes nodes.
inline bool tail_level_ok(const BdxLattice& l) {
  if (l.tsy || l.P != 1) return false;
  for (int a = 0; a < 3; ++a)
    if (l.n[a] < 1 || l.L[a] != l.n[a] + 1 || l.gh[a] != 0 || l.L[a] > kTailMaxNodes) return false;
  if (l.L[0] * l.L[1] * l.L[2] > kTailMaxNodes) return false;
  return l.ld >= l.L[2] && l.ld <= l.L[2] + 64;
}

// The table's own consistency: level count, pointers, coefficient ranges, and
// the h-transfers' check of every level pair.
inline bool tail_table_ok(const int64_t* tab, int nlev, int64_t nwords) {
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
      if (!htransfer_pair_ok(BdxLattice::from(w + kTailWords), lat)) return false;
    }
  }
  return true;
}

// One level of a checked table, decoded.
template <typename T>
struct TailLevel {
  BdxLattice lat;
  const T* S;
  const T* dinv;
  const unsigned char* bc;
  T* r;
  T* z;
  T* d;
  T* y;
  const int* cidx;
  const T* cw;
  const int* fpos;
  int ncoef;
  const double* coef;
  int nodes;
};

template <typename P>
BDX_HD P tail_ptr(int64_t w) {
  return reinterpret_cast<P>(static_cast<uintptr_t>(w));
}

// Level l of the table; the first level's r and z are the call's.  The tiled
// words of the descriptor are not loaded: tail_level_ok has refused a tiled
// level, and as constants they let lat.size() and lat.idx() fold.
template <typename T>
BDX_HD TailLevel<T> tail_level(const int64_t* tab, int l, const T* r0, T* z0) {
  const int64_t* w = tab + static_cast<int64_t>(l) * kTailWords;
  TailLevel<T> v;
  for (int a = 0; a < 3; ++a) {
    v.lat.n[a] = w[a];
    v.lat.L[a] = w[3 + a];
    v.lat.g0[a] = w[6 + a];
    v.lat.N[a] = w[9 + a];
    v.lat.gh[a] = w[12 + a];
  }
  v.lat.P = w[15];
  v.lat.ld = w[16];
  v.lat.tsy = v.lat.tsz = v.lat.tntz = v.lat.tcol = 0;
  v.S = tail_ptr<const T*>(w[kTailS]);
  v.dinv = tail_ptr<const T*>(w[kTailDinv]);
  v.bc = tail_ptr<const unsigned char*>(w[kTailBc]);
  v.r = l == 0 ? const_cast<T*>(r0) : tail_ptr<T*>(w[kTailR]);
  v.z = l == 0 ? z0 : tail_ptr<T*>(w[kTailZ]);
  v.d = tail_ptr<T*>(w[kTailD]);
  v.y = tail_ptr<T*>(w[kTailY]);
  v.cidx = tail_ptr<const int*>(w[kTailCidx]);
  v.cw = tail_ptr<const T*>(w[kTailCw]);
  v.fpos = tail_ptr<const int*>(w[kTailFpos]);
  v.ncoef = static_cast<int>(w[kTailNcoef]);
  v.coef = reinterpret_cast<const double*>(tab + w[kTailCoef]);
  v.nodes = static_cast<int>(v.lat.L[0] * v.lat.L[1] * v.lat.L[2]);
  return v;
}
