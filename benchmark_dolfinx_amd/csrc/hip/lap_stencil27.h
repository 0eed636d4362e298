// The assembled 27-point operator of a degree-1 level as streaming kernels
// (solvers/pmg.py: q1_operator="stencil"): S[27][lat.size()] in the storage
// index, plane (di + 1) 9 + (dj + 1) 3 + (dk + 1) (ops/kernels.py: stencil27).
//
//   apply  y = S u on every local row, ghost rows included; the caller
//          forward-exchanges u first.
//   cheb   one Chebyshev-Jacobi step over the owned rows in one launch:
//          d = a d + b dinv (r - S z_in);  z_out = z_in + d.  S z_in stays in a
//          register; z_out must not be z_in, because a neighbour's thread still
//          reads the old iterate.  Bit for bit `apply` into a scratch vector
//          followed by bdx_cheb_step.
//
// The thread mapping is the h-transfers' (lap_htransfer.h: htransfer_piece): a
// wave takes 64 consecutive z of one lattice row, so the row index and the
// tests for the i +- 1, j +- 1 neighbour rows are wave-uniform, and the 27
// coefficient loads of a plane are consecutive across the lanes.  S is read
// once per launch, the vector 27 times (9 rows x 3 z-shifts) out of the
// caches; both with the default cache policy: the Chebyshev steps of a level
// follow each other, and non-temporal loads of S kept a 164 MB stencil from
// staying in the 256 MiB Infinity Cache between them (46 against 32 us per
// apply, profiles/pmg_q1stencil.md).  No LDS, no barrier, no atomics.  The
// storage padding (k >= L[2]) is never loaded or stored.
//
// The row sum is stencil27_node and the entry update cheb_entry_fused
// (csrc/include/bdx_mg_bodies.h), shared with the host twins
// (csrc/host/bdx_host_mg.cpp); this file is the mapping of nodes to threads.
#pragma once
#include "bdx_common.h"
#include "bdx_mg_bodies.h"
#include "lap_htransfer.h"

// BDX_STENCIL27_NT=1 (a variant build, ops/build.py --variant): S with
// non-temporal loads, for A/B runs (profiles/pmg_q1stencil.md).
#ifndef BDX_STENCIL27_NT
#define BDX_STENCIL27_NT 0
#endif

// S as stencil27_node reads it.
template <typename T>
struct Stencil27Stream {
  const T* p;
  __device__ __forceinline__ T operator[](int64_t n) const {
    return BDX_STENCIL27_NT ? __builtin_nontemporal_load(p + n) : p[n];
  }
};

// The row sum as a value the compiler cannot contract into what follows, so
// the fused step rounds exactly where `apply` stores y.
template <typename T>
__device__ __forceinline__ T stencil27_value(const BdxLattice& lat, const T* S, const T* z, int i,
                                             int j, int k) {
  T s = stencil27_node<T>(lat, Stencil27Stream<T>{S}, z, i, j, k);
  asm volatile("" : "+v"(s));
  return s;
}

// y = S u: one thread per local node.
template <typename T>
__global__ void __launch_bounds__(kHTransferThreads)
    lap_stencil27_apply_kernel(BdxLattice lat, int64_t npiece, const T* __restrict__ S,
                               const T* __restrict__ u, T* __restrict__ y) {
  int64_t i, j, k;
  if (!htransfer_piece(lat, npiece, i, j, k)) return;
  const T s = stencil27_value<T>(lat, S, u, static_cast<int>(i), static_cast<int>(j),
                                 static_cast<int>(k));
  const int64_t to = lat.idx(i, j, k);
  if (!BDX_OOB(to, lat.size(), "stencil27 store")) y[to] = s;
}

// How bdx_cheb_step (blas.hip: for_each_owned, a lane's entries k = lane,
// lane + 64, ... of a row of o2 owned values) rounds the direction of entry k,
// which the fused step reproduces bit for bit: a fused multiply-add in FP64;
// in FP32 the compiler pairs a lane's iterations (v_pk_fma_f32) and gives the
// odd one left at the end a multiply and an add.  tests/
// test_gpu_pmg_q1stencil.py holds the two kernels together on rows of one to
// four iterations per lane.
template <typename T>
__device__ __forceinline__ bool cheb_step_fuses(int64_t k, int64_t o2) {
  if (sizeof(T) == 8) return true;
  const int64_t lane = k & 63, n = (o2 - lane + 63) >> 6;
  return (k >> 6) < (n & ~int64_t(1));
}

// d = a d + b dinv (r - S z_in);  z_out = z_in + d: one thread per owned node.
template <typename T>
__global__ void __launch_bounds__(kHTransferThreads)
    lap_stencil27_cheb_kernel(BdxLattice lat, int64_t npiece, int64_t o0, int64_t o1, int64_t o2,
                              const T* __restrict__ S, const T* __restrict__ dinv,
                              const T* __restrict__ r, const T* __restrict__ z_in,
                              T* __restrict__ d, T* __restrict__ z_out, T a, T b) {
  int64_t i, j, k;
  if (!htransfer_piece(lat, npiece, i, j, k)) return;
  if (i >= o0 || j >= o1 || k >= o2) return;
  const T s = stencil27_value<T>(lat, S, z_in, static_cast<int>(i), static_cast<int>(j),
                                 static_cast<int>(k));
  const int64_t at = lat.idx(i, j, k);
  if (!BDX_OOB(at, lat.size(), "stencil27 cheb"))
    cheb_entry_fused<T>(cheb_step_fuses<T>(k, o2), a, b, dinv, r, s, d, z_in, z_out, at);
}

// A degree-1 descriptor in the lattice layout whose extents fit int
// (stencil27_node's index type).
inline bool stencil27_lattice_ok(const BdxLattice& l) {
  if (l.tsy || l.P != 1) return false;
  for (int a = 0; a < 3; ++a)
    if (l.L[a] < 1 || l.L[a] > 0x7fffffffLL || l.L[a] != l.n[a] + 1) return false;
  return l.ld >= l.L[2] && l.ld <= 0x7fffffffLL;
}

template <typename T>
int launch_stencil27_apply(const int64_t* latd, const T* S, const T* u, T* y, hipStream_t st) {
  if (!latd || !S || !u || !y || y == u) return static_cast<int>(hipErrorInvalidValue);
  const BdxLattice lat = BdxLattice::from(latd);
  if (!stencil27_lattice_ok(lat)) return static_cast<int>(hipErrorInvalidValue);
  int64_t npiece;
  const int64_t nblk = htransfer_blocks(lat, npiece);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  lap_stencil27_apply_kernel<T><<<static_cast<unsigned>(nblk), kHTransferThreads, 0, st>>>(
      lat, npiece, S, u, y);
  BDX_CHECK(hipGetLastError());
  return 0;
}

template <typename T>
int launch_stencil27_cheb(const int64_t* latd, const int64_t* own, const T* S, const T* dinv,
                          const T* r, const T* z_in, T* d, T* z_out, double a, double b,
                          hipStream_t st) {
  if (!latd || !own || !S || !dinv || !r || !z_in || !d || !z_out || z_out == z_in)
    return static_cast<int>(hipErrorInvalidValue);
  const BdxLattice lat = BdxLattice::from(latd);
  if (!stencil27_lattice_ok(lat)) return static_cast<int>(hipErrorInvalidValue);
  for (int ax = 0; ax < 3; ++ax)
    if (own[ax] < 0 || own[ax] > lat.L[ax]) return static_cast<int>(hipErrorInvalidValue);
  int64_t npiece;
  const int64_t nblk = htransfer_blocks(lat, npiece);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  lap_stencil27_cheb_kernel<T><<<static_cast<unsigned>(nblk), kHTransferThreads, 0, st>>>(
      lat, npiece, own[0], own[1], own[2], S, dinv, r, z_in, d, z_out, static_cast<T>(a),
      static_cast<T>(b));
  BDX_CHECK(hipGetLastError());
  return 0;
}

#define BDX_STENCIL27_API(T, SUF)                                                          \
  extern "C" int bdx_stencil27_apply_##SUF BDX_P_STENCIL27_APPLY(T) {                      \
    return launch_stencil27_apply<T>(latd, S, u, y, st);                                   \
  }                                                                                        \
  extern "C" int bdx_stencil27_cheb_##SUF BDX_P_STENCIL27_CHEB(T) {                        \
    return launch_stencil27_cheb<T>(latd, own, S, dinv, r, z_in, d, z_out, a, b, st);      \
  }
