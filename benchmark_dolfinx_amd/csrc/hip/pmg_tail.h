// The tail of the multigrid V-cycle in one launch (solvers/pmg.py,
// `tail_nodes`): one workgroup of 1024 threads runs the smoothers, residuals,
// transfers and the coarse iteration of every level of a suffix of the
// hierarchy whose levels are all small degree-1 lattices, with the schedule
// and constants of `PMultigrid._vcycle`:
//   down, level l:  z = smooth(r, zero guess);  last level: stop
//                   y = A z;  r_c = R (r - y), Dirichlet entries zeroed
//   up, level l:    z += P z_c;  z = smooth(r, z)
// A Chebyshev step is y = A z; d = a d + b dinv (r - y); z += d (the first of
// a zero-guess smoother: d = z = b dinv r, no apply).
//
// Every phase is a loop n = tid; n < nodes; n += 1024 over the level's nodes,
// z fastest, so the lanes of a wave touch consecutive storage; the phases are
// separated by __syncthreads(), whose workgroup-scope fence makes one wave's
// global stores visible to the others of the workgroup (they share a CU).
// Every barrier sits in control flow that depends on the level table alone.
// No grid-wide synchronisation, no flags, no atomics: bitwise reproducible.
//
// The operator of a level is its assembled 27-point stencil S[27][nstore] in
// the level's storage index, plane (di + 1) 9 + (dj + 1) 3 + (dk + 1):
// y[n] = sum of S[p][n] z[n + offset(p)] over the neighbours inside the
// lattice, p ascending.
//
// The level table and its decoder: csrc/include/bdx_pmg_tail.h.  The
// Chebyshev entry update and the transfers are the per-node bodies of
// csrc/include/bdx_mg_bodies.h, shared with the stand-alone kernels and the
// host twin (csrc/host/bdx_host_mg.cpp); this file is the thread-stride phase
// loops and the barriers between them (and the stencil row, see tail_apply).
#pragma once
#include "bdx_common.h"
#include "bdx_pmg_tail.h"

constexpr int kTailThreads = 1024;

// Node n of the thread-stride loop, z fastest.
__device__ __forceinline__ void tail_node(const BdxLattice& lat, int n, int& i, int& j, int& k) {
  const int L1 = static_cast<int>(lat.L[1]), L2 = static_cast<int>(lat.L[2]);
  const int ij = n / L2;
  k = n - ij * L2;
  i = ij / L1;
  j = ij - i * L1;
}

// y = A z with the level's stencil: the sum of stencil27_node
// (bdx_mg_bodies.h), written out here.  Called through that function the
// kernel's code is no longer the one measured in profiles/pmg_tail.md: 670
// instructions and two VGPRs more, or, with the row's index passed in, the
// same size with the loads of every tap reordered and an FP32 call 1.3 %
// slower (profiles/mg_shared_bodies.md).
template <typename T>
__device__ __forceinline__ void tail_apply(const TailLevel<T>& v) {
  const int L0 = static_cast<int>(v.lat.L[0]), L1 = static_cast<int>(v.lat.L[1]),
            L2 = static_cast<int>(v.lat.L[2]);
  const int64_t ns = v.lat.size();
  for (int n = threadIdx.x; n < v.nodes; n += kTailThreads) {
    int i, j, k;
    tail_node(v.lat, n, i, j, k);
    const int64_t at = v.lat.idx(i, j, k);
    T s = 0;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int dk = -1; dk <= 1; ++dk) {
          if (i + di < 0 || i + di >= L0 || j + dj < 0 || j + dj >= L1 || k + dk < 0 ||
              k + dk >= L2)
            continue;
          const int64_t p = (di + 1) * 9 + (dj + 1) * 3 + (dk + 1);
          const int64_t from = v.lat.idx(i + di, j + dj, k + dk);
          if (BDX_OOB(p * ns + at, 27 * ns, "pmg_tail stencil") ||
              BDX_OOB(from, ns, "pmg_tail apply load"))
            continue;
          s += v.S[p * ns + at] * v.z[from];
        }
    if (!BDX_OOB(at, ns, "pmg_tail apply store")) v.y[at] = s;
  }
}

// One Chebyshev update (the entry update of blas.hip: cheb_step_kernel) on
// every node.
template <typename T>
__device__ __forceinline__ void tail_cheb(const TailLevel<T>& v, bool first, T a, T b) {
  for (int n = threadIdx.x; n < v.nodes; n += kTailThreads) {
    int i, j, k;
    tail_node(v.lat, n, i, j, k);
    const int64_t at = v.lat.idx(i, j, k);
    if (BDX_OOB(at, v.lat.size(), "pmg_tail cheb")) continue;
    cheb_entry<T>(first, a, b, v.dinv, v.r, v.y, v.d, v.z, at);
  }
}

// The level's Chebyshev iteration; ends behind a barrier.
template <typename T>
__device__ __forceinline__ void tail_smooth(const TailLevel<T>& v, bool zero_guess) {
  for (int s = 0; s < v.ncoef; ++s) {
    const T a = static_cast<T>(v.coef[2 * s]), b = static_cast<T>(v.coef[2 * s + 1]);
    const bool first = s == 0 && zero_guess;
    if (!first) {
      tail_apply(v);
      __syncthreads();
    }
    tail_cheb(v, first, a, b);
    __syncthreads();
  }
}

// r_c = R (r - y), Dirichlet entries zeroed.
template <typename T>
__device__ __forceinline__ void tail_restrict(const TailLevel<T>& f, const TailLevel<T>& c) {
  const HTransferTables<T> tab = htransfer_tables<T>(c.lat, f.lat, f.cidx, f.cw, f.fpos);
  for (int n = threadIdx.x; n < c.nodes; n += kTailThreads) {
    int i, j, k;
    tail_node(c.lat, n, i, j, k);
    const T s = hrestrict_node<T>(c.lat, f.lat, tab, f.r, f.y, i, j, k);
    const int64_t to = c.lat.idx(i, j, k);
    if (!BDX_OOB(to, c.lat.size(), "pmg_tail restrict store")) c.r[to] = c.bc[to] ? T(0) : s;
  }
}

// z += P z_c.
template <typename T>
__device__ __forceinline__ void tail_prolong(const TailLevel<T>& f, const TailLevel<T>& c) {
  const HTransferTables<T> tab = htransfer_tables<T>(c.lat, f.lat, f.cidx, f.cw, f.fpos);
  for (int n = threadIdx.x; n < f.nodes; n += kTailThreads) {
    int i, j, k;
    tail_node(f.lat, n, i, j, k);
    const T out = hprolong_node<T>(c.lat, tab, c.z, i, j, k);
    const int64_t to = f.lat.idx(i, j, k);
    if (!BDX_OOB(to, f.lat.size(), "pmg_tail prolong store")) f.z[to] = f.z[to] + out;
  }
}

// The tail's V-cycle: the levels of `tab` down, then up, by one workgroup.
// Nothing writes the table and no vector pointer is derived from `tab` itself
// (they are its words' values), so it is __restrict__: a level's words need no
// reload after the stores of a phase (no measurable gain: 77 against 78 us).
template <typename T>
__global__ void __launch_bounds__(kTailThreads)
    pmg_tail_kernel(const int64_t* __restrict__ tab, int nlev, const T* r0, T* z0) {
  for (int l = 0; l < nlev; ++l) {
    const TailLevel<T> v = tail_level<T>(tab, l, r0, z0);
    tail_smooth(v, true);
    if (l == nlev - 1) break;
    tail_apply(v);
    __syncthreads();
    tail_restrict(v, tail_level<T>(tab, l + 1, r0, z0));
    __syncthreads();
  }
  for (int l = nlev - 2; l >= 0; --l) {
    const TailLevel<T> v = tail_level<T>(tab, l, r0, z0);
    tail_prolong(v, tail_level<T>(tab, l + 1, r0, z0));
    __syncthreads();
    tail_smooth(v, false);
  }
}

// hipErrorInvalidValue for a null table or vector, a level count outside
// [1, kTailMaxLevels], and a level that is tiled, of a degree other than 1,
// with ghost planes, above the node cap, without its pointers or coefficients,
// or (all but the last) without the tables of a valid pair with the next.
template <typename T>
int launch_pmg_tail(const int64_t* htab, const int64_t* dtab, int nlev, int64_t nwords,
                    const T* r, T* z, hipStream_t st) {
  if (!dtab || !r || !z || !tail_table_ok(htab, nlev, nwords))
    return static_cast<int>(hipErrorInvalidValue);
  pmg_tail_kernel<T><<<1, kTailThreads, 0, st>>>(dtab, nlev, r, z);
  BDX_CHECK(hipGetLastError());
  return 0;
}

#define BDX_PMG_TAIL_API(T, SUF)                                                                 \
  extern "C" int bdx_pmg_tail_##SUF BDX_P_PMG_TAIL(T) {                                          \
    return launch_pmg_tail<T>(htab, dtab, nlev, nwords, r, z, st);                               \
  }
