// The 27-point stencil of a degree-1 level assembled on the device
// (models/poisson.py: PoissonProblem.stencil27("direct"); solvers/pmg.py:
// q1_assembly="direct"): S[27][lat.size()] in the storage index, plane
// (di + 1) 9 + (dj + 1) 3 + (dk + 1), written whole in one launch from the
// vertex coordinates, kappa and the 1D tables -- what ops/kernels.py: stencil27
// makes of the host's assembled CSR matrix, without the matrix.
//
// One thread per node of the storage, with the thread mapping of the
// h-transfers and of lap_stencil27.h (lap_htransfer.h: htransfer_piece): a wave
// takes 64 consecutive z of one lattice row, so whether the cells at i - 1 / i
// and j - 1 / j exist is wave-uniform and each of the 27 plane stores is
// consecutive across the lanes.  A thread gathers its own row: the rows of its
// node in the element matrices of the at most 8 cells around it, each cell's
// geometry recomputed by each of its 8 nodes.  That costs 8 x the geometry
// flops and buys a kernel with no atomics, no colours, no LDS, no barrier and
// a fixed summation order (two runs are bitwise equal); it is setup, run once
// per level.  A missing z-neighbour cell is a zero weight, not a branch.  The
// rows of the storage padding (L[2] <= k < ld) are written too, as zeros,
// which is why the row pieces here cover ld and not L[2].
//
// The per-node arithmetic is stencil27_assemble_node (csrc/include/
// bdx_mg_bodies.h), shared with the host twin (csrc/host/bdx_host_mg.cpp:
// bdx_cpu_stencil27_assemble); this file is the mapping of nodes to threads.
// The 27 sums are indexed by compile-time constants only (the cell corner is a
// template parameter, the quadrature loops stay rolled), so they live in
// registers.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), no scratch:
//   f64  249 VGPRs, 106 SGPRs (14 of them kept in VGPR lanes), 2 waves / SIMD
//   f32  209 VGPRs, 106 SGPRs (8 of them kept in VGPR lanes), 2 waves / SIMD
#pragma once
#include "bdx_common.h"
#include "bdx_mg_bodies.h"
#include "lap_htransfer.h"
#include "lap_stencil27.h"  // stencil27_lattice_ok

// S[p][n] = row n of the assembled operator, all 27 planes: one thread per
// node of the storage.  pieces: lat with L[2] = ld, so that the row pieces
// cover the storage padding.
template <typename T>
__global__ void __launch_bounds__(kHTransferThreads)
    lap_stencil27_assemble_kernel(BdxLattice lat, BdxLattice pieces, int64_t npiece,
                                  Stencil27Tables<T> tb, const T* __restrict__ xv, T kappa,
                                  const T* __restrict__ kc, T* __restrict__ S) {
  int64_t i, j, k;
  if (!htransfer_piece(pieces, npiece, i, j, k)) return;
  T acc[27];
  stencil27_assemble_node<T>(lat, tb, xv, kappa, kc, static_cast<int>(i), static_cast<int>(j),
                             static_cast<int>(k), acc);
  const int64_t ns = lat.size(), at = lat.idx(i, j, k);
#pragma unroll
  for (int p = 0; p < 27; ++p)
    if (!BDX_OOB(p * ns + at, 27 * ns, "stencil27 assemble store")) S[p * ns + at] = acc[p];
}

template <typename T>
int launch_stencil27_assemble(const int64_t* latd, int nq, const double* phi0, const double* dphi1,
                              const double* wts, const double* qpts, const T* xv, double kappa,
                              const T* kc, T* S, hipStream_t st) {
  if (!latd || !phi0 || !dphi1 || !wts || !qpts || !xv || !S || nq < 2 || nq > kStencil27MaxNq)
    return static_cast<int>(hipErrorInvalidValue);
  const BdxLattice lat = BdxLattice::from(latd);
  if (!stencil27_lattice_ok(lat)) return static_cast<int>(hipErrorInvalidValue);
  BdxLattice pieces = lat;
  pieces.L[2] = lat.ld;
  int64_t npiece;
  const int64_t nblk = htransfer_blocks(pieces, npiece);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  lap_stencil27_assemble_kernel<T><<<static_cast<unsigned>(nblk), kHTransferThreads, 0, st>>>(
      lat, pieces, npiece, stencil27_tables<T>(nq, phi0, dphi1, wts, qpts), xv,
      static_cast<T>(kappa), kc, S);
  BDX_CHECK(hipGetLastError());
  return 0;
}

#define BDX_STENCIL27_ASSEMBLE_API(T, SUF)                                                  \
  extern "C" int bdx_stencil27_assemble_##SUF BDX_P_STENCIL27_ASSEMBLE(T) {                 \
    return launch_stencil27_assemble<T>(latd, nq, phi0, dphi1, wts, qpts, xv, kappa, kc, S, \
                                        st);                                                \
  }
