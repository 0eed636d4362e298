// p-multigrid transfer operators between Q_Pc and Q_Pf on the same cells
// (solvers/pmg.py): the nodal interpolation P = J (x) J (x) J per cell, with
// J[a][i] = l_i^c(xi_a^f) the coarse GLL Lagrange basis at the fine GLL nodes,
// and the restriction R = P^T with every fine dof counted once.
//
// Both kernels are sum-factorised through LDS: V1Shape's cells per workgroup,
// one thread per fine node (q = (qx NF + qy) NF + qz), J in LDS, three 1D
// contractions with a barrier between them.
//
//   prolongation  vf = P vc:  z, y, x contractions NC -> NF.  Every fine node
//     is written exactly once and nothing is read back: a cell writes its local
//     node indices < Pf on each axis, and index Pf where it is the last local
//     cell of that axis.  The coarse ghost planes are read (the caller
//     forward-exchanges vc first).
//   restriction  vc += P^T vf:  a cell takes the same fine nodes, and of those
//     only the ones inside the owned extents (fine ghost planes count as 0),
//     contracts x, y, z NF -> NC and adds into the coarse vector.  No atomics:
//     one launch per cell-parity colour in a fixed order, as launch_diag does,
//     so no two cells of a launch share a coarse dof and the result is bitwise
//     reproducible.  Partial sums land on every local coarse node, ghost
//     planes included; the caller zeroes vc first and reverse-exchanges after.
//
// Compile-time extents for the six pairs of the level schedule Pc = max(1,
// Pf / 2): (2,1) (3,1) (4,2) (5,2) (6,3) (7,3).
#pragma once
#include "lap_v1.h"

#include "bdx_mg_bodies.h"  // transfer_pair_ok

// The 1D interpolation table in T, passed by value (NF x NC <= 8 x 4).
template <typename T>
struct TransferTable {
  T J[8 * 4];
};

// Shared-memory image of one transfer workgroup (CPB cells x NF^3 nodes).
template <typename T, int NF, int NC>
struct TransferSmem {
  static constexpr int nf3 = NF * NF * NF, CPB = V1Shape<NF>::cpb;
  T J[NF * NC];
  T s0[CPB][nf3];
  T s1[CPB][nf3];
};

// vf = P vc over the cells [0, n) of the local lattice.
template <typename T, int PF, int PC>
__global__ void __launch_bounds__(V1Shape<PF + 1>::threads)
    lap_prolong_kernel(BdxLattice lc, BdxLattice lf, TransferTable<T> tab,
                       const T* __restrict__ vc, T* __restrict__ vf) {
  constexpr int NF = PF + 1, NC = PC + 1, nf3 = NF * NF * NF;
  constexpr int CPB = V1Shape<NF>::cpb;
  __shared__ TransferSmem<T, NF, NC> sm;

  const int tid = threadIdx.x;
  for (int i = tid; i < NF * NC; i += blockDim.x) sm.J[i] = tab.J[i];

  const int cs_raw = tid / nf3;
  const bool active = cs_raw < CPB;
  const int cs = active ? cs_raw : 0;
  const int q = tid - cs_raw * nf3;
  const int qx = q / (NF * NF), qy = (q / NF) % NF, qz = q % NF;
  const int64_t ncell = lf.n[0] * lf.n[1] * lf.n[2];
  const int64_t cell_lin = static_cast<int64_t>(blockIdx.x) * CPB + cs;
  const bool valid = active && cell_lin < ncell;
  int64_t cx = 0, cy = 0, cz = 0;
  if (valid) {
    cz = cell_lin % lf.n[2];
    cy = (cell_lin / lf.n[2]) % lf.n[1];
    cx = cell_lin / (lf.n[1] * lf.n[2]);
  }
  // the cell's coarse nodes, embedded in the NF^3 grid
  if (active && qx < NC && qy < NC && qz < NC) {
    T v = 0;
    if (valid) {
      const int64_t at = lc.idx(cx * PC + qx, cy * PC + qy, cz * PC + qz);
      if (!BDX_OOB(at, lc.size(), "prolong load")) v = vc[at];
    }
    sm.s0[cs][q] = v;
  }
  __syncthreads();

  // z: thread (a = qx < NC, b = qy < NC, k = qz)
  if (active && qx < NC && qy < NC) {
    T acc = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc += sm.J[qz * NC + c] * sm.s0[cs][(qx * NF + qy) * NF + c];
    sm.s1[cs][q] = acc;
  }
  __syncthreads();
  // y: thread (a = qx < NC, j = qy, k)
  if (active && qx < NC) {
    T acc = 0;
#pragma unroll
    for (int b = 0; b < NC; ++b) acc += sm.J[qy * NC + b] * sm.s1[cs][(qx * NF + b) * NF + qz];
    sm.s0[cs][q] = acc;
  }
  __syncthreads();
  // x: thread (i = qx, j, k) owns fine node (i, j, k) of its cell
  if (valid) {
    T acc = 0;
#pragma unroll
    for (int a = 0; a < NC; ++a) acc += sm.J[qx * NC + a] * sm.s0[cs][(a * NF + qy) * NF + qz];
    const bool take = (qx < PF || cx == lf.n[0] - 1) && (qy < PF || cy == lf.n[1] - 1) &&
                      (qz < PF || cz == lf.n[2] - 1);
    if (take) {
      const int64_t at = lf.idx(cx * PF + qx, cy * PF + qy, cz * PF + qz);
      if (!BDX_OOB(at, lf.size(), "prolong store")) vf[at] = acc;
    }
  }
}

// vc += P^T vf over the cells (lo + 2 c) of one parity colour, c in [0, e).
template <typename T, int PF, int PC>
__global__ void __launch_bounds__(V1Shape<PF + 1>::threads)
    lap_restrict_kernel(BdxLattice lc, BdxLattice lf, TransferTable<T> tab,
                        const T* __restrict__ vf, T* __restrict__ vc, int64_t lo0, int64_t lo1,
                        int64_t lo2, int64_t e0, int64_t e1, int64_t e2) {
  constexpr int NF = PF + 1, NC = PC + 1, nf3 = NF * NF * NF;
  constexpr int CPB = V1Shape<NF>::cpb;
  __shared__ TransferSmem<T, NF, NC> sm;

  const int tid = threadIdx.x;
  for (int i = tid; i < NF * NC; i += blockDim.x) sm.J[i] = tab.J[i];

  const int cs_raw = tid / nf3;
  const bool active = cs_raw < CPB;
  const int cs = active ? cs_raw : 0;
  const int q = tid - cs_raw * nf3;
  const int qx = q / (NF * NF), qy = (q / NF) % NF, qz = q % NF;
  const int64_t ncell = e0 * e1 * e2;
  const int64_t cell_lin = static_cast<int64_t>(blockIdx.x) * CPB + cs;
  const bool valid = active && cell_lin < ncell;
  int64_t cx = 0, cy = 0, cz = 0;
  if (valid) {
    cz = lo2 + 2 * (cell_lin % e2);
    cy = lo1 + 2 * ((cell_lin / e2) % e1);
    cx = lo0 + 2 * (cell_lin / (e1 * e2));
  }
  // the cell's share of the fine nodes: each global fine dof once, owned only
  if (active) {
    T v = 0;
    if (valid) {
      const int64_t li = cx * PF + qx, lj = cy * PF + qy, lk = cz * PF + qz;
      const bool take = (qx < PF || cx == lf.n[0] - 1) && (qy < PF || cy == lf.n[1] - 1) &&
                        (qz < PF || cz == lf.n[2] - 1) && lf.is_owned(li, lj, lk);
      if (take) {
        const int64_t at = lf.idx(li, lj, lk);
        if (!BDX_OOB(at, lf.size(), "restrict load")) v = vf[at];
      }
    }
    sm.s0[cs][q] = v;
  }
  __syncthreads();

  // x: thread (a = qx < NC, j = qy, k = qz)
  if (active && qx < NC) {
    T acc = 0;
#pragma unroll
    for (int i = 0; i < NF; ++i) acc += sm.J[i * NC + qx] * sm.s0[cs][(i * NF + qy) * NF + qz];
    sm.s1[cs][q] = acc;
  }
  __syncthreads();
  // y: thread (a, b = qy < NC, k)
  if (active && qx < NC && qy < NC) {
    T acc = 0;
#pragma unroll
    for (int j = 0; j < NF; ++j) acc += sm.J[j * NC + qy] * sm.s1[cs][(qx * NF + j) * NF + qz];
    sm.s0[cs][q] = acc;
  }
  __syncthreads();
  // z: thread (a, b, c = qz < NC) owns coarse node (a, b, c) of its cell
  if (valid && qx < NC && qy < NC && qz < NC) {
    T acc = 0;
#pragma unroll
    for (int k = 0; k < NF; ++k) acc += sm.J[k * NC + qz] * sm.s0[cs][(qx * NF + qy) * NF + k];
    const int64_t at = lc.idx(cx * PC + qx, cy * PC + qy, cz * PC + qz);
    if (!BDX_OOB(at, lc.size(), "restrict store")) vc[at] += acc;
  }
}

template <typename T, int PF, int PC>
int launch_prolong(const BdxLattice& lc, const BdxLattice& lf, const TransferTable<T>& tab,
                   const T* vc, T* vf, hipStream_t st) {
  constexpr int cpb = V1Shape<PF + 1>::cpb;
  const int64_t ncell = lf.n[0] * lf.n[1] * lf.n[2];
  if (ncell <= 0) return 0;
  const int64_t nblk = (ncell + cpb - 1) / cpb;
  if (nblk > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
  lap_prolong_kernel<T, PF, PC>
      <<<static_cast<unsigned>(nblk), V1Shape<PF + 1>::threads, 0, st>>>(lc, lf, tab, vc, vf);
  BDX_CHECK(hipGetLastError());
  return 0;
}

// The eight colour launches over all local cells, in a fixed order.
template <typename T, int PF, int PC>
int launch_restrict(const BdxLattice& lc, const BdxLattice& lf, const TransferTable<T>& tab,
                    const T* vf, T* vc, hipStream_t st) {
  constexpr int cpb = V1Shape<PF + 1>::cpb;
  for (int colour = 0; colour < 8; ++colour) {
    const int64_t o[3] = {(colour >> 2) & 1, (colour >> 1) & 1, colour & 1};
    int64_t e[3];
    for (int a = 0; a < 3; ++a) {
      const int64_t span = lf.n[a] - o[a];
      e[a] = span > 0 ? (span + 1) / 2 : 0;
    }
    const int64_t ncell = e[0] * e[1] * e[2];
    if (ncell <= 0) continue;
    const int64_t nblk = (ncell + cpb - 1) / cpb;
    if (nblk > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
    lap_restrict_kernel<T, PF, PC><<<static_cast<unsigned>(nblk), V1Shape<PF + 1>::threads, 0, st>>>(
        lc, lf, tab, vf, vc, o[0], o[1], o[2], e[0], e[1], e[2]);
    BDX_CHECK(hipGetLastError());
  }
  return 0;
}

// transfer_pair_ok (bdx_mg_bodies.h): the check of a level pair, shared with
// the host twins.
template <typename T>
int dispatch_transfer(bool restrict_, const BdxLattice& lc, const BdxLattice& lf, const double* J,
                      const T* src, T* dst, hipStream_t st) {
  if (!transfer_pair_ok(lc, lf)) return static_cast<int>(hipErrorInvalidValue);
  TransferTable<T> tab{};
  const int n = static_cast<int>((lf.P + 1) * (lc.P + 1));
  for (int i = 0; i < n; ++i) tab.J[i] = static_cast<T>(J[i]);
#define BDX_TRANSFER_CASE(PF, PC)                                                     \
  case PF:                                                                            \
    return restrict_ ? launch_restrict<T, PF, PC>(lc, lf, tab, src, dst, st)          \
                     : launch_prolong<T, PF, PC>(lc, lf, tab, src, dst, st);
  switch (lf.P) {
    BDX_TRANSFER_CASE(2, 1)
    BDX_TRANSFER_CASE(3, 1)
    BDX_TRANSFER_CASE(4, 2)
    BDX_TRANSFER_CASE(5, 2)
    BDX_TRANSFER_CASE(6, 3)
    BDX_TRANSFER_CASE(7, 3)
  }
#undef BDX_TRANSFER_CASE
  return static_cast<int>(hipErrorInvalidValue);
}

#define BDX_TRANSFER_API(T, SUF)                                                          \
  extern "C" int bdx_prolong_##SUF BDX_P_PROLONG(T) {                                     \
    return dispatch_transfer<T>(false, BdxLattice::from(latc), BdxLattice::from(latf), J, \
                                vc, vf, st);                                              \
  }                                                                                       \
  extern "C" int bdx_restrict_##SUF BDX_P_RESTRICT(T) {                                   \
    return dispatch_transfer<T>(true, BdxLattice::from(latc), BdxLattice::from(latf), J,  \
                                vf, vc, st);                                              \
  }
