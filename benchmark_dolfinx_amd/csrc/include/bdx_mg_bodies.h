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
//   stencil27     one row of a level's assembled 27-point operator, applied
//                 (stencil27_node) and assembled (stencil27_assemble_node)
//   cheb_entry    one entry of a Chebyshev-Jacobi step (cheb_entry_fused: with
//                 the operator's value handed over, lap_stencil27.h)
// and the checks of a level pair of the p- and the h-transfers.
#pragma once
#include <cstdint>

#include "bdx_debug.h"
#include "bdx_geometry.h"
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

// Assembly of that stencil.
//
// The 1D tables of a degree-1 level in T: B = phi0 and Dd = dphi1 phi0 (both
// nq x 2), the quadrature weights and points; nq is 2 or 3.
constexpr int kStencil27MaxNq = 3;
template <typename T>
struct Stencil27Tables {
  T B[kStencil27MaxNq * 2];
  T Dd[kStencil27MaxNq * 2];
  T wts[kStencil27MaxNq];
  T qpts[kStencil27MaxNq];
  int nq;
};

// From the FP64 tables of a launcher (bdx_diag's arguments), on the host.
template <typename T>
inline Stencil27Tables<T> stencil27_tables(int nq, const double* phi0, const double* dphi1,
                                           const double* wts, const double* qpts) {
  Stencil27Tables<T> t{};
  t.nq = nq;
  for (int q = 0; q < nq; ++q) {
    for (int a = 0; a < 2; ++a) {
      t.B[q * 2 + a] = static_cast<T>(phi0[q * 2 + a]);
      T acc = 0;
      for (int m = 0; m < nq; ++m)
        acc += static_cast<T>(dphi1[q * nq + m]) * static_cast<T>(phi0[m * 2 + a]);
      t.Dd[q * 2 + a] = acc;
    }
    t.wts[q] = static_cast<T>(wts[q]);
    t.qpts[q] = static_cast<T>(qpts[q]);
  }
  return t;
}

// acc += row (AI, AJ, AK) of the element matrix of the local cell (i - AI,
// j - AJ, k - AK), the cell that has node (i, j, k) as that corner:
//   Ke[a][b] = kappa_c sum_q grad phi_b . G_q grad phi_a   (G_q symmetric)
// over the tensor quadrature points, x outermost, with grad phi = (Dd B B,
// B Dd B, B B Dd) and G_q = trilinear_G with the weight w_x w_y w_z.  Entry b
// goes to the plane of the neighbour (b - a), a compile-time index: the 27
// sums stay in registers.  The quadrature loops stay rolled (eight corners x
// nq^3 points unrolled would be some 10^5 instructions).  A cell outside the
// lattice in x or y adds nothing (the same answer for every z of the row); one
// outside in z is computed on the nearest cell of the column with the weight
// kappa_c = 0, so the lanes of a wave do not diverge.
template <typename T, int AI, int AJ, int AK>
BDX_HD void stencil27_assemble_cell(const BdxLattice& lat, const Stencil27Tables<T>& tb,
                                    const T* xv, T kappa, const T* kc, int i, int j, int k,
                                    T (&acc)[27]) {
  const int64_t cx = i - AI, cy = j - AJ;
  if (cx < 0 || cx >= lat.n[0] || cy < 0 || cy >= lat.n[1] || lat.n[2] < 1) return;
  int64_t cz = k - AK;
  const bool has = cz >= 0 && cz < lat.n[2];
  cz = cz < 0 ? 0 : (cz > lat.n[2] - 1 ? lat.n[2] - 1 : cz);
  const int64_t nvert = (lat.n[0] + 1) * (lat.n[1] + 1) * (lat.n[2] + 1);
  (void)nvert;  // read by the BDX_DEBUG index checks only
  T X[8][3];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const int64_t at = lat.vidx(cx + (v >> 2), cy + ((v >> 1) & 1), cz + (v & 1));
#pragma unroll
    for (int c = 0; c < 3; ++c)
      X[v][c] = BDX_OOB(3 * at + c, 3 * nvert, "stencil27 assemble vertex") ? T(0) : xv[3 * at + c];
  }
  const int64_t cell = (cx * lat.n[1] + cy) * lat.n[2] + cz;
  T kap = kappa;
  if (kc && !BDX_OOB(cell, lat.n[0] * lat.n[1] * lat.n[2], "stencil27 assemble kappa"))
    kap = kc[cell];
  if (!has) kap = 0;
  const int nq = tb.nq;
#pragma unroll 1
  for (int qx = 0; qx < nq; ++qx)
#pragma unroll 1
    for (int qy = 0; qy < nq; ++qy)
#pragma unroll 1
      for (int qz = 0; qz < nq; ++qz) {
        T G[6];
        trilinear_G<T>(X, tb.qpts[qx], tb.qpts[qy], tb.qpts[qz],
                       tb.wts[qx] * tb.wts[qy] * tb.wts[qz], G);
        const T bx[2] = {tb.B[2 * qx], tb.B[2 * qx + 1]}, dx[2] = {tb.Dd[2 * qx], tb.Dd[2 * qx + 1]};
        const T by[2] = {tb.B[2 * qy], tb.B[2 * qy + 1]}, dy[2] = {tb.Dd[2 * qy], tb.Dd[2 * qy + 1]};
        const T bz[2] = {tb.B[2 * qz], tb.B[2 * qz + 1]}, dz[2] = {tb.Dd[2 * qz], tb.Dd[2 * qz + 1]};
        // kappa G grad phi_a
        const T g0 = dx[AI] * by[AJ] * bz[AK], g1 = bx[AI] * dy[AJ] * bz[AK],
                g2 = bx[AI] * by[AJ] * dz[AK];
        const T t0 = kap * (G[0] * g0 + G[1] * g1 + G[2] * g2);
        const T t1 = kap * (G[1] * g0 + G[3] * g1 + G[4] * g2);
        const T t2 = kap * (G[2] * g0 + G[4] * g1 + G[5] * g2);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int bk = 0; bk < 2; ++bk) {
              const T h0 = dx[bi] * by[bj] * bz[bk], h1 = bx[bi] * dy[bj] * bz[bk],
                      h2 = bx[bi] * by[bj] * dz[bk];
              acc[(bi - AI + 1) * 9 + (bj - AJ + 1) * 3 + (bk - AK + 1)] +=
                  h0 * t0 + h1 * t1 + h2 * t2;
            }
      }
}

// Row (i, j, k), k < lat.ld, of the assembled operator of a degree-1 lattice
// (stencil27_lattice_ok) in the 27 planes of stencil27_node: what
// ops/kernels.py: stencil27 makes of the rank's assembled matrix (csr_build,
// csrc/host/bdx_host.cpp).
//   a row of the storage padding (k >= L[2])   0
//   a Dirichlet row   0, and 1 in the centre where the node is owned
//   any other row     the rows of the node in the element matrices of the at
//                     most 8 local cells around it (a ghost-plane row: this
//                     rank's partial sums), cells in the order of their corner
//                     (0,0,0), (0,0,1), ... (1,1,1); then 0 in every Dirichlet
//                     column and for every neighbour outside the local lattice.
// Every plane is written; the order of cells, points and terms is fixed, so
// the row is the same on every run.
template <typename T>
BDX_HD void stencil27_assemble_node(const BdxLattice& lat, const Stencil27Tables<T>& tb,
                                    const T* xv, T kappa, const T* kc, int i, int j, int k,
                                    T (&acc)[27]) {
#pragma unroll
  for (int p = 0; p < 27; ++p) acc[p] = 0;
  if (k >= lat.L[2]) return;
  if (lat.is_bc(i, j, k)) {
    if (lat.is_owned(i, j, k)) acc[13] = 1;
    return;
  }
  stencil27_assemble_cell<T, 0, 0, 0>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 0, 0, 1>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 0, 1, 0>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 0, 1, 1>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 1, 0, 0>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 1, 0, 1>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 1, 1, 0>(lat, tb, xv, kappa, kc, i, j, k, acc);
  stencil27_assemble_cell<T, 1, 1, 1>(lat, tb, xv, kappa, kc, i, j, k, acc);
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
      for (int dk = -1; dk <= 1; ++dk) {
        const bool in = i + di >= 0 && i + di < lat.L[0] && j + dj >= 0 && j + dj < lat.L[1] &&
                        k + dk >= 0 && k + dk < lat.L[2];
        if (!in || lat.is_bc(i + di, j + dj, k + dk)) acc[(di + 1) * 9 + (dj + 1) * 3 + (dk + 1)] = 0;
      }
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
