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
//
// The per-node bodies (hprolong_node, hrestrict_node), the split tables and
// the check of a level pair are csrc/include/bdx_mg_bodies.h, shared with the
// V-cycle tail (pmg_tail.h) and the host twins (csrc/host/bdx_host_mg.cpp);
// this file is the mapping of nodes to threads.
#pragma once
#include "bdx_common.h"
#include "bdx_mg_bodies.h"

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

#define BDX_HTRANSFER_API(T, SUF)                                                              \
  extern "C" int bdx_hprolong_##SUF BDX_P_HPROLONG(T) {                                        \
    return launch_hprolong<T>(latc, latf, cidx, cw, fpos, vc, vf, add, st);                    \
  }                                                                                            \
  extern "C" int bdx_hrestrict_##SUF BDX_P_HRESTRICT(T) {                                      \
    return launch_hrestrict<T>(latc, latf, cidx, cw, fpos, vf, y, vc, st);                     \
  }
