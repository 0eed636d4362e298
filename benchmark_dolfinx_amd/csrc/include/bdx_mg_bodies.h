// Shared (host + device) per-node arithmetic of the multigrid V-cycle: what one
// thread of a device kernel (csrc/hip/lap_htransfer.h, pmg_tail.h, blas.hip)
// and one iteration of its host twin (csrc/host/bdx_host_mg.cpp) compute for
// one lattice node.  A V-cycle kernel is a thread mapping over these bodies
// and its host twin a loop over the same bodies, so the two sides share every
// expression and its order; they still differ where the device contracts a
// multiply-add into an FMA and the host build does not.
//
//   h-transfers   trilinear interpolation in index space between two degree-1
//                 lattices and its transpose (tables: lap_htransfer.h)
//   p-transfers by rows   the index helpers of lap_rowtransfer.h: cell and
//                 local index of a fine node, support and weights of a coarse one
//   stencil27     one row of a level's assembled 27-point operator
//   cheb_entry    one entry of a Chebyshev-Jacobi step (cheb_entry_fused: with
//                 the operator's value handed over, lap_stencil27.h)
// and the checks of a level pair of the p- and the h-transfers.
#pragma once
#include <cstdint>

#include "bdx_debug.h"
#include "bdx_lattice.h"

// p-transfers: both descriptors in the lattice layout, on the same cells and
// the same piece of the partition, with a degree pair of the schedule
// Pc = max(1, Pf / 2).
BDX_HD bool transfer_pair_ok(const BdxLattice& lc, const BdxLattice& lf) {
  if (lc.tsy || lf.tsy) return false;
  if (lf.P < 2 || lf.P > 7 || lc.P != (lf.P / 2 > 1 ? lf.P / 2 : 1)) return false;
  for (int a = 0; a < 3; ++a) {
    if (lc.n[a] != lf.n[a] || lc.n[a] < 0 || lc.gh[a] != lf.gh[a]) return false;
    if (lc.L[a] != lc.n[a] * lc.P + 1 || lf.L[a] != lf.n[a] * lf.P + 1) return false;
  }
  return lc.ld >= lc.L[2] && lf.ld >= lf.L[2];
}

// p-transfers by rows (csrc/hip/lap_rowtransfer.h), one axis of n cells with
// the degrees Pf / Pc and J the (Pf + 1) x (Pc + 1) table.  Fine node I
// belongs to cell min(I / Pf, n - 1) with local index q = I - cell Pf, and its
// weights are row q of J.  The first and the last row of J are unit vectors,
// so a fine vertex node weighs 1 in its coarse vertex and 0 everywhere else:
// every fine dof is counted once without a `take` rule.
BDX_HD void ptransfer_cell(int64_t I, int64_t Pf, int64_t n, int64_t& cell, int64_t& q) {
  cell = I / Pf;
  if (cell > n - 1) cell = n - 1;
  q = I - cell * Pf;
}

// Range [lo, hi] of the fine nodes coarse node A gathers, clipped to the owned
// fine nodes (index < own): a cell-interior coarse node takes the Pf - 1
// interior nodes of its cell, a coarse vertex those of each adjacent cell and
// itself.
BDX_HD void ptransfer_support(int64_t A, int64_t Pf, int64_t Pc, int64_t n, int64_t own,
                              int64_t& lo, int64_t& hi) {
  int64_t c = A / Pc;
  if (c > n - 1) c = n - 1;
  const int64_t a = A - c * Pc;
  lo = c * Pf + 1;
  hi = c * Pf + Pf - 1;
  if (a == 0) lo = c > 0 ? lo - Pf : 0;
  if (a == Pc) {
    lo = c * Pf + 1;
    hi = c * Pf + Pf;
  }
  if (hi > own - 1) hi = own - 1;
}

// Weight of fine node I in coarse node A: J[q][A - cell Pc], 0 where A is no
// node of I's cell.
template <typename T>
BDX_HD T ptransfer_weight(const T* J, int64_t I, int64_t A, int64_t Pf, int64_t Pc, int64_t n) {
  int64_t cell, q;
  ptransfer_cell(I, Pf, n, cell, q);
  const int64_t a = A - cell * Pc;
  return a >= 0 && a <= Pc ? J[q * (Pc + 1) + a] : T(0);
}

// h-transfers: two degree-1 descriptors in the lattice layout on the same
// piece of the partition, the coarse one with no more cells than the fine one
// per axis.
BDX_HD bool htransfer_pair_ok(const BdxLattice& lc, const BdxLattice& lf) {
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

// The tables of one h-level pair, split per axis.
template <typename T>
struct HTransferTables {
  const int* cidx[3];
  const T* cw[3];
  const int* fpos[3];
};

template <typename T>
BDX_HD HTransferTables<T> htransfer_tables(const BdxLattice& lc, const BdxLattice& lf,
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

// P vc at fine node (i, j, k): one 1D interpolation a + w (b - a) per axis, z
// then y then x; an axis with w = 0 takes a and loads nothing else.
template <typename T>
BDX_HD T hprolong_node(const BdxLattice& lc, const HTransferTables<T>& tab, const T* vc, int64_t i,
                       int64_t j, int64_t k) {
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

// Range [lo, hi] of the fine nodes coarse node j gathers on one axis and the
// fine index of j itself; only owned fine nodes (index < own).
BDX_HD void hrestrict_range(const int* fpos, int64_t j, int64_t Lc, int64_t own, int64_t& lo,
                            int64_t& mid, int64_t& hi) {
  mid = fpos[j];
  lo = j > 0 ? fpos[j - 1] + 1 : mid;
  hi = j < Lc - 1 ? fpos[j + 1] - 1 : mid;
  if (hi > own - 1) hi = own - 1;
}

// Weight of fine node f in coarse node (at fine index mid).
template <typename T>
BDX_HD T hrestrict_weight(const T* cw, int64_t f, int64_t mid) {
  return f < mid ? cw[f] : (f == mid ? T(1) : T(1) - cw[f]);
}

// P^T (vf - y) (y null: P^T vf) at coarse node (i, j, k): a gather of the
// owned fine nodes strictly between its coarse neighbours, ascending, x
// outermost, with the weights cw, 1, 1 - cw.
template <typename T>
BDX_HD T hrestrict_node(const BdxLattice& lc, const BdxLattice& lf, const HTransferTables<T>& tab,
                        const T* vf, const T* y, int64_t i, int64_t j, int64_t k) {
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

// (A z) at node (i, j, k) of a degree-1 lattice (lattice layout, every extent
// within int) with the assembled stencil S[27][lat.size()], plane (di + 1) 9 +
// (dj + 1) 3 + (dk + 1): the sum of S[p][n] z[n + offset(p)] over the
// neighbours inside the lattice, p ascending.  A neighbour outside the lattice
// is skipped without a branch: its term is 0 z[n], which leaves the sum as it
// is, bit for bit, for every finite z[n] (and z[n] is in the sum anyway), and
// its two loads are the node's own S[p][n] and z[n].  No load waits for a
// branch that way, and a streaming kernel keeps all 54 in flight.  The tail's kernel
// keeps this loop written out in its own `tail_apply` (pmg_tail.h explains
// why); both are checked against each other by tests/test_gpu_pmg_tail.py.
// SP: how S is read, `const T*` or anything else with its `S[n]`
// (csrc/hip/lap_stencil27.h chooses the cache policy of S that way).
template <typename T, typename SP>
BDX_HD T stencil27_node(const BdxLattice& lat, SP S, const T* z, int i, int j, int k) {
  const int L0 = static_cast<int>(lat.L[0]), L1 = static_cast<int>(lat.L[1]),
            L2 = static_cast<int>(lat.L[2]);
  const int64_t ns = lat.size();
  const int64_t at = lat.idx(i, j, k);
  T s = 0;
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
      for (int dk = -1; dk <= 1; ++dk) {
        const bool in = i + di >= 0 && i + di < L0 && j + dj >= 0 && j + dj < L1 &&
                        k + dk >= 0 && k + dk < L2;
        const int64_t p = (di + 1) * 9 + (dj + 1) * 3 + (dk + 1);
        const int64_t from = in ? lat.idx(i + di, j + dj, k + dk) : at;
        if (BDX_OOB(p * ns + at, 27 * ns, "pmg_tail stencil") ||
            BDX_OOB(from, ns, "pmg_tail apply load"))
          continue;
        const T c = S[p * ns + at];
        s += (in ? c : T(0)) * z[from];
      }
  return s;
}

// Entry `at` of one Chebyshev-Jacobi step, y = A z computed by the caller:
// d = a d + b dinv (r - y);  z += d.  first (the step from a zero guess):
// d = z = b dinv r, which reads neither y nor the old d and z.
template <typename T>
BDX_HD void cheb_entry(bool first, T a, T b, const T* dinv, const T* r, const T* y, T* d, T* z,
                       int64_t at) {
  if (first) {
    const T dn = b * dinv[at] * r[at];
    d[at] = dn;
    z[at] = dn;
  } else {
    const T dn = a * d[at] + b * dinv[at] * (r[at] - y[at]);
    d[at] = dn;
    z[at] = z[at] + dn;
  }
}

// The sum a d + t of a Chebyshev direction, t = b dinv (r - y), with its
// rounding spelled out: one fused multiply-add (`fused`), or a multiply and an
// add.  cheb_entry above leaves that choice to the compiler's contraction; a
// second device kernel that has to reproduce a compiled cheb_entry bit for bit
// (csrc/hip/lap_stencil27.h says which entries got which) makes it here.  The
// host build contracts nothing, so both are the plain expression there.
#if defined(__HIP_DEVICE_COMPILE__)
// (the empty asm keeps the rounded product out of the contraction's reach)
BDX_HD double cheb_sum(bool fused, double a, double d, double t) {
  if (fused) return __builtin_fma(a, d, t);
  double p = a * d;
  asm volatile("" : "+v"(p));
  return p + t;
}
BDX_HD float cheb_sum(bool fused, float a, float d, float t) {
  if (fused) return __builtin_fmaf(a, d, t);
  float p = a * d;
  asm volatile("" : "+v"(p));
  return p + t;
}
#else
template <typename T>
BDX_HD T cheb_sum(bool, T a, T d, T t) {
  return a * d + t;
}
#endif

// cheb_entry's update with (A z_in)[at] = y handed over as a value and the
// iterate ping-ponged: d = a d + b dinv (r - y);  z_out = z_in + d (never the
// first step, which has no operator); `fused`: cheb_sum.
template <typename T>
BDX_HD void cheb_entry_fused(bool fused, T a, T b, const T* dinv, const T* r, T y, T* d,
                             const T* z_in, T* z_out, int64_t at) {
  const T t = b * dinv[at] * (r[at] - y);
  const T dn = cheb_sum(fused, a, d[at], t);
  d[at] = dn;
  z_out[at] = z_in[at] + dn;
}
