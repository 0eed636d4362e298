// h-multigrid transfer operators between two degree-1 lattices whose coarse
// vertices are a subset of the fine vertices (fem/mesh.py: coarsened_lattice;
// solvers/pmg.py): trilinear interpolation in index space and its transpose.
//
// One table set per level pair, resident on the device, each the three axes
// concatenated (x | y | z):
//   cidx  int32, Lf[0] + Lf[1] + Lf[2]   lower coarse neighbour of fine node i
//   cw    T,     the same lengths        weight of the upper neighbour; exactly
//                                        0 where fine node i is a coarse node
//                                        (cidx + 1 is then never read)
//   fpos  int32, Lc[0] + Lc[1] + Lc[2]   fine index of coarse node j
// An axis that is not coarsened has the identity tables (cidx = fpos = i,
// cw = 0).
//
// Both kernels give one wave a 64-node piece of one lattice row (z fastest),
// so the row indices and the x / y table entries are wave-uniform and the
// stores of consecutive lanes are consecutive.
//
//   prolongation  vf = P vc (add = 0: every local fine node, ghost planes
//     included, written once; the coarse ghost planes are read) or vf += P vc
//     (add = 1: owned fine nodes only, everything else untouched).  One 1D
//     interpolation a + w (b - a) per axis, z then y then x; an axis with
//     w = 0 takes a and loads nothing else: at most 8 coarse loads per node.
//   restriction  vc = P^T (vf - y) (y null: P^T vf): one thread per local
//     coarse node, ghost planes included, gathers the fine nodes strictly
//     between fpos[j - 1] and fpos[j + 1] on every axis (at most 5) in
//     ascending order, x outermost, with the weights cw, 1, 1 - cw; only owned
//     fine nodes count.  No atomics, no zeroing: one launch, bitwise
//     reproducible.  The caller reverse-exchanges the coarse ghost planes.
#pragma once
#include "bdx_common.h"

// The device tables of one level pair, split per axis.
template <typename T>
struct HTransferTables {
  const int* cidx[3];
  const T* cw[3];
  const int* fpos[3];
};

constexpr int kHTransferThreads = 256;  // 4 waves, one row piece each

// Row piece of this wave: false when past the last.  row = i L[1] + j.
__device__ __forceinline__ bool htransfer_piece(const BdxLattice& l, int64_t npiece, int64_t& i,
                                                int64_t& j, int64_t& k) {
  const int64_t wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t item = static_cast<int64_t>(blockIdx.x) * (kHTransferThreads / 64) + wave;
  const int64_t nrow = l.L[0] * l.L[1];
  if (item >= nrow * npiece) return false;
  const int64_t row = item / npiece;
  i = row / l.L[1];
  j = row - i * l.L[1];
  k = (item - row * npiece) * 64 + (threadIdx.x & 63);
  return k < l.L[2];
}

// P vc at fine node (i, j, k): the per-node body of the prolongation (also the
// V-cycle tail's, pmg_tail.h).
template <typename T>
__device__ __forceinline__ T hprolong_node(const BdxLattice& lc, const HTransferTables<T>& tab,
                                           const T* vc, int64_t i, int64_t j, int64_t k) {
  const int64_t ci = tab.cidx[0][i], cj = tab.cidx[1][j], ck = tab.cidx[2][k];
  const T wi = tab.cw[0][i], wj = tab.cw[1][j], wk = tab.cw[2][k];
  const int na = wi != 0 ? 2 : 1, nb = wj != 0 ? 2 : 1;
  T gx[2] = {0, 0};
  for (int a = 0; a < na; ++a) {
    T gy[2] = {0, 0};
    for (int b = 0; b < nb; ++b) {
      const int64_t at = lc.idx(ci + a, cj + b, ck);
      T v = 0;
      if (!BDX_OOB(at, lc.size(), "hprolong load")) v = vc[at];
      if (wk != 0 && !BDX_OOB(at + 1, lc.size(), "hprolong load")) v += wk * (vc[at + 1] - v);
      gy[b] = v;
    }
    gx[a] = nb == 2 ? gy[0] + wj * (gy[1] - gy[0]) : gy[0];
  }
  return na == 2 ? gx[0] + wi * (gx[1] - gx[0]) : gx[0];
}

// vf (+)= P vc: one thread per fine node.
template <typename T>
__global__ void __launch_bounds__(kHTransferThreads)
    lap_hprolong_kernel(BdxLattice lc, BdxLattice lf, HTransferTables<T> tab, int64_t npiece,
                        const T* __restrict__ vc, T* __restrict__ vf, int add) {
  int64_t i, j, k;
  if (!htransfer_piece(lf, npiece, i, j, k)) return;
  if (add && !lf.is_owned(i, j, k)) return;
  const T out = hprolong_node<T>(lc, tab, vc, i, j, k);
  const int64_t to = lf.idx(i, j, k);
  if (!BDX_OOB(to, lf.size(), "hprolong store")) vf[to] = add ? vf[to] + out : out;
}

// Range [lo, hi] of the fine nodes coarse node j gathers on one axis and the
// fine index of j itself; only owned fine nodes (index < own).
__device__ __forceinline__ void hrestrict_range(const int* fpos, int64_t j, int64_t Lc, int64_t own,
                                                int64_t& lo, int64_t& mid, int64_t& hi) {
  mid = fpos[j];
  lo = j > 0 ? fpos[j - 1] + 1 : mid;
  hi = j < Lc - 1 ? fpos[j + 1] - 1 : mid;
  if (hi > own - 1) hi = own - 1;
}

// Weight of fine node f in coarse node (at fine index mid).
template <typename T>
__device__ __forceinline__ T hrestrict_weight(const T* cw, int64_t f, int64_t mid) {
  return f < mid ? cw[f] : (f == mid ? T(1) : T(1) - cw[f]);
}

// P^T (vf - y) at coarse node (i, j, k), a fixed-order gather: the per-node
// body of the restriction (also the V-cycle tail's, pmg_tail.h).
template <typename T>
__device__ __forceinline__ T hrestrict_node(const BdxLattice& lc, const BdxLattice& lf,
                                            const HTransferTables<T>& tab, const T* vf, const T* y,
                                            int64_t i, int64_t j, int64_t k) {
  int64_t lo[3], mid[3], hi[3];
  hrestrict_range(tab.fpos[0], i, lc.L[0], lf.L[0] - lf.gh[0], lo[0], mid[0], hi[0]);
  hrestrict_range(tab.fpos[1], j, lc.L[1], lf.L[1] - lf.gh[1], lo[1], mid[1], hi[1]);
  hrestrict_range(tab.fpos[2], k, lc.L[2], lf.L[2] - lf.gh[2], lo[2], mid[2], hi[2]);
  T sx = 0;
  for (int64_t fi = lo[0]; fi <= hi[0]; ++fi) {
    T sy = 0;
    for (int64_t fj = lo[1]; fj <= hi[1]; ++fj) {
      T sz = 0;
      for (int64_t fk = lo[2]; fk <= hi[2]; ++fk) {
        const int64_t at = lf.idx(fi, fj, fk);
        if (BDX_OOB(at, lf.size(), "hrestrict load")) continue;
        const T v = y ? vf[at] - y[at] : vf[at];
        sz += hrestrict_weight(tab.cw[2], fk, mid[2]) * v;
      }
      sy += hrestrict_weight(tab.cw[1], fj, mid[1]) * sz;
    }
    sx += hrestrict_weight(tab.cw[0], fi, mid[0]) * sy;
  }
  return sx;
}

// vc = P^T (vf - y): one thread per coarse node.
template <typename T>
__global__ void __launch_bounds__(kHTransferThreads)
    lap_hrestrict_kernel(BdxLattice lc, BdxLattice lf, HTransferTables<T> tab, int64_t npiece,
                         const T* __restrict__ vf, const T* __restrict__ y, T* __restrict__ vc) {
  int64_t i, j, k;
  if (!htransfer_piece(lc, npiece, i, j, k)) return;
  const T sx = hrestrict_node<T>(lc, lf, tab, vf, y, i, j, k);
  const int64_t to = lc.idx(i, j, k);
  if (!BDX_OOB(to, lc.size(), "hrestrict store")) vc[to] = sx;
}

// Two degree-1 descriptors in the lattice layout on the same piece of the
// partition, the coarse one with no more cells than the fine one per axis.
inline bool htransfer_pair_ok(const BdxLattice& lc, const BdxLattice& lf) {
  if (lc.tsy || lf.tsy) return false;
  if (lc.P != 1 || lf.P != 1) return false;
  for (int a = 0; a < 3; ++a) {
    if (lc.gh[a] != lf.gh[a]) return false;
    if (lc.n[a] < 0 || lc.n[a] > lf.n[a]) return false;
    if (lc.L[a] != lc.n[a] + 1 || lf.L[a] != lf.n[a] + 1) return false;
    if (lf.L[a] > 0x7fffffffLL) return false;  // int32 tables
  }
  return lc.ld >= lc.L[2] && lf.ld >= lf.L[2];
}

template <typename T>
__host__ __device__ inline HTransferTables<T> htransfer_tables(const BdxLattice& lc, const BdxLattice& lf,
                                           const int* cidx, const T* cw, const int* fpos) {
  HTransferTables<T> t;
  int64_t of = 0, oc = 0;
  for (int a = 0; a < 3; ++a) {
    t.cidx[a] = cidx + of;
    t.cw[a] = cw + of;
    t.fpos[a] = fpos + oc;
    of += lf.L[a];
    oc += lc.L[a];
  }
  return t;
}

// Blocks that give every 64-node row piece of lattice l a wave; -1: too many.
inline int64_t htransfer_blocks(const BdxLattice& l, int64_t& npiece) {
  npiece = (l.L[2] + 63) / 64;
  const int64_t items = l.L[0] * l.L[1] * npiece;
  const int64_t nblk = (items + kHTransferThreads / 64 - 1) / (kHTransferThreads / 64);
  return nblk > 0x7fffffffLL ? -1 : nblk;
}

template <typename T>
int launch_hprolong(const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw,
                    const int* fpos, const T* vc, T* vf, int add, hipStream_t st) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!htransfer_pair_ok(lc, lf) || !cidx || !cw || !fpos || !vc || !vf)
    return static_cast<int>(hipErrorInvalidValue);
  int64_t npiece;
  const int64_t nblk = htransfer_blocks(lf, npiece);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nblk == 0) return 0;
  lap_hprolong_kernel<T><<<static_cast<unsigned>(nblk), kHTransferThreads, 0, st>>>(
      lc, lf, htransfer_tables<T>(lc, lf, cidx, cw, fpos), npiece, vc, vf, add);
  BDX_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int launch_hrestrict(const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw,
                     const int* fpos, const T* vf, const T* y, T* vc, hipStream_t st) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!htransfer_pair_ok(lc, lf) || !cidx || !cw || !fpos || !vc || !vf)
    return static_cast<int>(hipErrorInvalidValue);
  int64_t npiece;
  const int64_t nblk = htransfer_blocks(lc, npiece);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nblk == 0) return 0;
  lap_hrestrict_kernel<T><<<static_cast<unsigned>(nblk), kHTransferThreads, 0, st>>>(
      lc, lf, htransfer_tables<T>(lc, lf, cidx, cw, fpos), npiece, vf, y, vc);
  BDX_CHECK(hipGetLastError());
  return 0;
}

// vf (+)= P vc and vc = P^T (vf - y) between the coarse and fine degree-1
// lattices latc / latf; cidx, cw, fpos: the device tables above.
// hipErrorInvalidValue for tiled descriptors, a degree other than 1, differing
// ghost flags, L != n + 1, more coarse than fine cells on an axis or ld < L[2].
#define BDX_HTRANSFER_API(T, SUF)                                                              \
  extern "C" int bdx_hprolong_##SUF(const int64_t* latc, const int64_t* latf, const int* cidx, \
                                    const T* cw, const int* fpos, const T* vc, T* vf, int add, \
                                    hipStream_t st) {                                          \
    return launch_hprolong<T>(latc, latf, cidx, cw, fpos, vc, vf, add, st);                    \
  }                                                                                            \
  extern "C" int bdx_hrestrict_##SUF(const int64_t* latc, const int64_t* latf, const int* cidx, \
                                     const T* cw, const int* fpos, const T* vf, const T* y,    \
                                     T* vc, hipStream_t st) {                                  \
    return launch_hrestrict<T>(latc, latf, cidx, cw, fpos, vf, y, vc, st);                     \
  }
