// p-multigrid transfer operators between Q_Pc and Q_Pf on the same cells, by
// lattice rows: the operators of lap_transfer.h (P = J (x) J (x) J per cell
// and R = P^T with every fine dof counted once) with the interface of the
// h-transfers (lap_htransfer.h), so a V-cycle treats both kinds of level pair
// alike (solvers/pmg.py: p_transfer="row").
//
//   prolongation  vf = P vc (add = 0: every local fine node, ghost planes
//     included, written once; the coarse ghost planes are read) or vf += P vc
//     (add = 1: owned fine nodes only, everything else untouched).
//   restriction  vc = P^T (vf - y) (y null: P^T vf): every local coarse node,
//     ghost planes included, written once; only owned fine nodes are read.  No
//     zeroing by the caller, no colours, no atomics: one launch, a fixed
//     summation order, bitwise reproducible.  The caller reverse-exchanges
//     the coarse ghost planes.
//
// Mapping (wave64): a wave owns a piece of lattice rows, lane = z index, so
// row indices and the x / y weights are wave-uniform and the loads and stores
// of consecutive lanes are consecutive.  The z contraction runs across the
// lanes of the wave with __shfl; no LDS is allocated and no barrier is used.
// Every lane of a wave reaches every shuffle: lanes without a node carry 0.
//
//   prolongation  a wave takes fine row (I, J) and a z-chunk of at most
//     63 / Pf whole cells (plus the closing node in the row's last chunk).
//     1. lane = coarse z: t = sum_a sum_b J[qx][a] J[qy][b] vc[row(a, b)], a
//        outermost; a row of weight exactly 0 is skipped (a face row loads
//        one coarse row on that axis).
//     2. lane = fine z: out = sum_c J[qz][c] shfl(t, coarse lane of c).
//   restriction  a wave takes the Pc x Pc coarse rows of one cell column that
//     are closed at their lower faces, A in [cx Pc, cx Pc + Pc) and likewise
//     B, with one more block index per axis for the closing rows, and a
//     z-chunk of at most 63 / Pf - 1 whole cells plus one cell of overlap
//     below it (the coarse vertex at the chunk's lower end gathers from it).
//     1. lane = fine z: every owned row piece of the block's x-y support is
//        loaded once (minus y), ascending I outermost, then J, and added into
//        the at most Pc^2 accumulators with wave-uniform weights; zero
//        weights are skipped.
//     2. lane = coarse z: each accumulator is contracted over its at most
//        2 Pf - 1 fine z nodes, ascending, by shuffles, and stored.
//
// The index helpers (ptransfer_cell, ptransfer_support, ptransfer_weight) are
// csrc/include/bdx_mg_bodies.h, shared with the host twins
// (csrc/host/bdx_host_mg.cpp), which sum in the same order.
#pragma once
#include "bdx_common.h"
#include "bdx_mg_bodies.h"

constexpr int kRowTransferThreads = 256;  // 4 waves, one item each

// The 1D interpolation table in T, passed by value ((Pf + 1) x (Pc + 1) <= 8 x 4).
template <typename T>
struct RowTransferTable {
  T J[8 * 4];
};

// Cells of a wave's z-chunk: lanes 0 .. cells Pf (prolongation, the closing
// node included) and 0 .. (cells + 1) Pf (restriction, lane 0 the unused lower
// vertex of the overlap cell) fit a wave.
template <int PF>
struct RowTransferShape {
  static constexpr int prolong_cells = 63 / PF;
  static constexpr int restrict_cells = 63 / PF - 1;
  static_assert(prolong_cells * PF + 1 <= 64 && (restrict_cells + 1) * PF + 1 <= 64 &&
                    restrict_cells >= 1,
                "a z-chunk must fit one wave");
};

// Item of this wave (wave-uniform); false when past the last.
__device__ __forceinline__ bool rowtransfer_item(int64_t nitem, int64_t& item) {
  const int64_t wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  item = static_cast<int64_t>(blockIdx.x) * (kRowTransferThreads / 64) + wave;
  return item < nitem;
}

// vf (+)= P vc: a wave per fine row and z-chunk.
template <typename T, int PF, int PC>
__global__ void __launch_bounds__(kRowTransferThreads)
    lap_prolong_row_kernel(BdxLattice lc, BdxLattice lf, RowTransferTable<T> tab, int64_t nchunk,
                           const T* __restrict__ vc, T* __restrict__ vf, int add) {
  constexpr int NC = PC + 1, CW = RowTransferShape<PF>::prolong_cells;
  int64_t item;
  if (!rowtransfer_item(lf.L[0] * lf.L[1] * nchunk, item)) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = item / nchunk, ch = item - row * nchunk;
  const int64_t I = row / lf.L[1], Jr = row - I * lf.L[1];
  if (add && (I >= lf.L[0] - lf.gh[0] || Jr >= lf.L[1] - lf.gh[1])) return;
  const int64_t cell0 = ch * CW;
  const int ncc = static_cast<int>(lf.n[2] - cell0 < CW ? lf.n[2] - cell0 : CW);
  const bool last = cell0 + ncc == lf.n[2];
  int64_t cx, qx, cy, qy;
  ptransfer_cell(I, PF, lf.n[0], cx, qx);
  ptransfer_cell(Jr, PF, lf.n[1], cy, qy);

  // 1. lane = coarse z node of the chunk: the x-y combination of the coarse rows
  const bool cvalid = lane <= ncc * PC;
  const int64_t kc = cell0 * PC + lane;
  T t = 0;
#pragma unroll
  for (int a = 0; a < NC; ++a) {
#pragma unroll
    for (int b = 0; b < NC; ++b) {
      const T w = tab.J[qx * NC + a] * tab.J[qy * NC + b];
      if (w == 0) continue;
      const int64_t at = lc.idx(cx * PC + a, cy * PC + b, kc);
      if (cvalid && !BDX_OOB(at, lc.size(), "prolong_row load")) t += w * vc[at];
    }
  }

  // 2. lane = fine z node of the chunk: the z contraction across the lanes
  const bool fvalid = lane < ncc * PF || (last && lane == ncc * PF);
  int czl = lane / PF;
  if (czl > ncc - 1) czl = ncc - 1;
  int qz = lane - czl * PF;
  if (!fvalid) czl = 0, qz = 0;
  T out = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) out += tab.J[qz * NC + c] * __shfl(t, czl * PC + c);

  const int64_t kf = cell0 * PF + lane;
  if (!fvalid || (add && kf >= lf.L[2] - lf.gh[2])) return;
  const int64_t to = lf.idx(I, Jr, kf);
  if (!BDX_OOB(to, lf.size(), "prolong_row store")) vf[to] = add ? vf[to] + out : out;
}

// vc = P^T (vf - y): a wave per block of Pc x Pc coarse rows and z-chunk.
template <typename T, int PF, int PC>
__global__ void __launch_bounds__(kRowTransferThreads)
    lap_restrict_row_kernel(BdxLattice lc, BdxLattice lf, RowTransferTable<T> tab, int64_t nchunk,
                            const T* __restrict__ vf, const T* __restrict__ y,
                            T* __restrict__ vc) {
  constexpr int CW = RowTransferShape<PF>::restrict_cells;
  const int64_t nby = lf.n[1] + 1;
  int64_t item;
  if (!rowtransfer_item((lf.n[0] + 1) * nby * nchunk, item)) return;
  const int lane = threadIdx.x & 63;
  const int64_t blk = item / nchunk, ch = item - blk * nchunk;
  const int64_t bx = blk / nby, by = blk - bx * nby;
  const int64_t cell0 = ch * CW;
  const int ncc = static_cast<int>(lf.n[2] - cell0 < CW ? lf.n[2] - cell0 : CW);
  const bool last = cell0 + ncc == lf.n[2];
  // coarse rows A0 + ai, B0 + bi of the block; the closing block has one
  const int nA = bx < lf.n[0] ? PC : 1, nB = by < lf.n[1] ? PC : 1;
  const int64_t A0 = bx * PC, B0 = by * PC;
  const int64_t own[3] = {lf.L[0] - lf.gh[0], lf.L[1] - lf.gh[1], lf.L[2] - lf.gh[2]};
  // the block's fine rows: the union of its coarse rows' supports, owned only
  const int64_t ilo = bx > 0 ? (bx - 1) * PF + 1 : 0, jlo = by > 0 ? (by - 1) * PF + 1 : 0;
  int64_t ihi = bx < lf.n[0] ? bx * PF + PF - 1 : lf.n[0] * PF;
  int64_t jhi = by < lf.n[1] ? by * PF + PF - 1 : lf.n[1] * PF;
  if (ihi > own[0] - 1) ihi = own[0] - 1;
  if (jhi > own[1] - 1) jhi = own[1] - 1;

  // 1. lane = fine z node zbase + lane, lane 0 the lower vertex of the overlap
  // cell (no coarse node of the chunk gathers it)
  const int64_t zbase = (cell0 - 1) * PF, kf = zbase + lane;
  const int lmax = (ncc + 1) * PF - (last ? 0 : 1);
  const bool fvalid = lane >= 1 && lane <= lmax && kf >= 0 && kf < own[2];
  T acc[PC][PC];
#pragma unroll
  for (int ai = 0; ai < PC; ++ai)
#pragma unroll
    for (int bi = 0; bi < PC; ++bi) acc[ai][bi] = 0;
  for (int64_t I = ilo; I <= ihi; ++I) {
    T wx[PC];
#pragma unroll
    for (int ai = 0; ai < PC; ++ai)
      wx[ai] = ai < nA ? ptransfer_weight<T>(tab.J, I, A0 + ai, PF, PC, lf.n[0]) : T(0);
    for (int64_t Jr = jlo; Jr <= jhi; ++Jr) {
      T wy[PC];
#pragma unroll
      for (int bi = 0; bi < PC; ++bi)
        wy[bi] = bi < nB ? ptransfer_weight<T>(tab.J, Jr, B0 + bi, PF, PC, lf.n[1]) : T(0);
      const int64_t at = lf.idx(I, Jr, kf);
      T v = 0;
      if (fvalid && !BDX_OOB(at, lf.size(), "restrict_row load")) v = y ? vf[at] - y[at] : vf[at];
#pragma unroll
      for (int ai = 0; ai < PC; ++ai)
#pragma unroll
        for (int bi = 0; bi < PC; ++bi) {
          const T w = wx[ai] * wy[bi];
          if (w != 0) acc[ai][bi] += w * v;
        }
    }
  }

  // 2. lane = coarse z node of the chunk: its owned fine z nodes, ascending
  const bool cvalid = lane < ncc * PC || (last && lane == ncc * PC);
  const int64_t C = cell0 * PC + lane;
  int64_t lo = 1, hi = 0;
  if (cvalid) ptransfer_support(C, PF, PC, lf.n[2], own[2], lo, hi);
  T out[PC][PC];
#pragma unroll
  for (int ai = 0; ai < PC; ++ai)
#pragma unroll
    for (int bi = 0; bi < PC; ++bi) out[ai][bi] = 0;
#pragma unroll
  for (int s = 0; s < 2 * PF - 1; ++s) {
    const int64_t k = lo + s;
    const bool ok = k <= hi;
    const T wz = ok ? ptransfer_weight<T>(tab.J, k, C, PF, PC, lf.n[2]) : T(0);
    const int src = ok ? static_cast<int>(k - zbase) : 0;
#pragma unroll
    for (int ai = 0; ai < PC; ++ai)
#pragma unroll
      for (int bi = 0; bi < PC; ++bi) {
        const T val = __shfl(acc[ai][bi], src);
        if (ok) out[ai][bi] += wz * val;
      }
  }
  if (!cvalid) return;
#pragma unroll
  for (int ai = 0; ai < PC; ++ai)
#pragma unroll
    for (int bi = 0; bi < PC; ++bi) {
      if (ai >= nA || bi >= nB) continue;
      const int64_t to = lc.idx(A0 + ai, B0 + bi, C);
      if (!BDX_OOB(to, lc.size(), "restrict_row store")) vc[to] = out[ai][bi];
    }
}

// Blocks that give each of nitem items a wave; -1: too many.
inline int64_t rowtransfer_blocks(int64_t nitem) {
  const int64_t nblk = (nitem + kRowTransferThreads / 64 - 1) / (kRowTransferThreads / 64);
  return nblk > 0x7fffffffLL ? -1 : nblk;
}

template <typename T, int PF, int PC>
int launch_prolong_row(const BdxLattice& lc, const BdxLattice& lf, const RowTransferTable<T>& tab,
                       const T* vc, T* vf, int add, hipStream_t st) {
  constexpr int CW = RowTransferShape<PF>::prolong_cells;
  const int64_t nchunk = (lf.n[2] + CW - 1) / CW;
  const int64_t nblk = rowtransfer_blocks(lf.L[0] * lf.L[1] * nchunk);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  lap_prolong_row_kernel<T, PF, PC><<<static_cast<unsigned>(nblk), kRowTransferThreads, 0, st>>>(
      lc, lf, tab, nchunk, vc, vf, add);
  BDX_CHECK(hipGetLastError());
  return 0;
}

template <typename T, int PF, int PC>
int launch_restrict_row(const BdxLattice& lc, const BdxLattice& lf, const RowTransferTable<T>& tab,
                        const T* vf, const T* y, T* vc, hipStream_t st) {
  constexpr int CW = RowTransferShape<PF>::restrict_cells;
  const int64_t nchunk = (lf.n[2] + CW - 1) / CW;
  const int64_t nblk = rowtransfer_blocks((lf.n[0] + 1) * (lf.n[1] + 1) * nchunk);
  if (nblk < 0) return static_cast<int>(hipErrorInvalidValue);
  lap_restrict_row_kernel<T, PF, PC><<<static_cast<unsigned>(nblk), kRowTransferThreads, 0, st>>>(
      lc, lf, tab, nchunk, vf, y, vc);
  BDX_CHECK(hipGetLastError());
  return 0;
}

// src / dst: vc / vf of the prolongation, vf / vc of the restriction.  A pair
// outside the schedule (transfer_pair_ok), a null pointer or a row too long
// for int lanes is refused before anything is launched; a lattice without
// cells has nothing to transfer.
template <typename T>
int dispatch_rowtransfer(bool restrict_, const int64_t* latc, const int64_t* latf,
                         const double* J, const T* src, const T* y, T* dst, int add,
                         hipStream_t st) {
  if (!latc || !latf || !J || !src || !dst) return static_cast<int>(hipErrorInvalidValue);
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!transfer_pair_ok(lc, lf)) return static_cast<int>(hipErrorInvalidValue);
  for (int a = 0; a < 3; ++a)
    if (lf.L[a] > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
  if (lf.n[0] == 0 || lf.n[1] == 0 || lf.n[2] == 0) return 0;
  RowTransferTable<T> tab{};
  const int n = static_cast<int>((lf.P + 1) * (lc.P + 1));
  for (int i = 0; i < n; ++i) tab.J[i] = static_cast<T>(J[i]);
#define BDX_ROWTRANSFER_CASE(PF, PC)                                                   \
  case PF:                                                                             \
    return restrict_ ? launch_restrict_row<T, PF, PC>(lc, lf, tab, src, y, dst, st)    \
                     : launch_prolong_row<T, PF, PC>(lc, lf, tab, src, dst, add, st);
  switch (lf.P) {
    BDX_ROWTRANSFER_CASE(2, 1)
    BDX_ROWTRANSFER_CASE(3, 1)
    BDX_ROWTRANSFER_CASE(4, 2)
    BDX_ROWTRANSFER_CASE(5, 2)
    BDX_ROWTRANSFER_CASE(6, 3)
    BDX_ROWTRANSFER_CASE(7, 3)
  }
#undef BDX_ROWTRANSFER_CASE
  return static_cast<int>(hipErrorInvalidValue);
}

#define BDX_ROWTRANSFER_API(T, SUF)                                                         \
  extern "C" int bdx_prolong_row_##SUF BDX_P_PROLONG_ROW(T) {                               \
    return dispatch_rowtransfer<T>(false, latc, latf, J, vc, nullptr, vf, add, st);         \
  }                                                                                         \
  extern "C" int bdx_restrict_row_##SUF BDX_P_RESTRICT_ROW(T) {                             \
    return dispatch_rowtransfer<T>(true, latc, latf, J, vf, y, vc, 0, st);                  \
  }
