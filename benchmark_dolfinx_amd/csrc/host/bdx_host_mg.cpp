// Host (CPU) runtime of benchmark_dolfinx_amd: the multigrid V-cycle.
//
// Host twins of the device kernels of the p-multigrid preconditioner
// (solvers/pmg.py; ops/kernels.py: HostKernels), the CPU platform's
// production path and the reference every GPU test of those kernels compares
// with.  The h-transfers, the Chebyshev step, the 27-point stencil and the
// V-cycle tail are loops over the per-node bodies of
// csrc/include/bdx_mg_bodies.h, which the device kernels map to threads; the
// p-transfers keep a per-cell sum-factorised structure of their own, and the
// p-transfers by rows loop over the index helpers of the same header.

#include <cstdint>

#include "../include/bdx_host_api.h"
#include "../include/bdx_lattice.h"
#include "../include/bdx_mg_bodies.h"
#include "../include/bdx_pmg_tail.h"

namespace {

// ------------------------------------------------- p-multigrid transfers
// Host twins of csrc/hip/lap_transfer.h: per cell P = J (x) J (x) J with
// J (nf x nc, row-major) the coarse Lagrange basis at the fine nodes.

// vf = P vc: every local fine node written once (a cell writes its local
// indices < Pf, and Pf where it is the last local cell of the axis).
template <typename T>
int prolong_host(const int64_t* latc, const int64_t* latf, const double* Jd, const T* vc,
                 T* vf) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!transfer_pair_ok(lc, lf)) return 1;
  const int PF = static_cast<int>(lf.P), PC = static_cast<int>(lc.P), nf = PF + 1, nc = PC + 1;
  T J[8 * 4];
  for (int i = 0; i < nf * nc; ++i) J[i] = static_cast<T>(Jd[i]);
  const int64_t n1 = lf.n[1], n2 = lf.n[2], ncell = lf.n[0] * n1 * n2;
#pragma omp parallel for schedule(static)
  for (int64_t cell = 0; cell < ncell; ++cell) {
    const int64_t cz = cell % n2, cy = (cell / n2) % n1, cx = cell / (n1 * n2);
    T s0[4 * 4 * 8], s1[4 * 8 * 8];
    // z: (a, b, c) -> (a, b, k)
    for (int a = 0; a < nc; ++a)
      for (int b = 0; b < nc; ++b)
        for (int k = 0; k < nf; ++k) {
          T acc = 0;
          for (int c = 0; c < nc; ++c)
            acc += J[k * nc + c] * vc[lc.idx(cx * PC + a, cy * PC + b, cz * PC + c)];
          s0[(a * nc + b) * nf + k] = acc;
        }
    // y: (a, b, k) -> (a, j, k)
    for (int a = 0; a < nc; ++a)
      for (int j = 0; j < nf; ++j)
        for (int k = 0; k < nf; ++k) {
          T acc = 0;
          for (int b = 0; b < nc; ++b) acc += J[j * nc + b] * s0[(a * nc + b) * nf + k];
          s1[(a * nf + j) * nf + k] = acc;
        }
    // x: (a, j, k) -> (i, j, k)
    const int ex = cx == lf.n[0] - 1 ? nf : PF, ey = cy == n1 - 1 ? nf : PF,
              ez = cz == n2 - 1 ? nf : PF;
    for (int i = 0; i < ex; ++i)
      for (int j = 0; j < ey; ++j)
        for (int k = 0; k < ez; ++k) {
          T acc = 0;
          for (int a = 0; a < nc; ++a) acc += J[i * nc + a] * s1[(a * nf + j) * nf + k];
          vf[lf.idx(cx * PF + i, cy * PF + j, cz * PF + k)] = acc;
        }
  }
  return 0;
}

// vc += P^T vf: each cell takes the fine nodes prolong_host writes, owned ones
// only; cells of one parity colour share no coarse dof, so the colours run
// one after the other (fixed order) and each in parallel.
template <typename T>
int restrict_host(const int64_t* latc, const int64_t* latf, const double* Jd, const T* vf,
                  T* vc) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!transfer_pair_ok(lc, lf)) return 1;
  const int PF = static_cast<int>(lf.P), PC = static_cast<int>(lc.P), nf = PF + 1, nc = PC + 1;
  T J[8 * 4];
  for (int i = 0; i < nf * nc; ++i) J[i] = static_cast<T>(Jd[i]);
  for (int colour = 0; colour < 8; ++colour) {
    const int64_t o[3] = {(colour >> 2) & 1, (colour >> 1) & 1, colour & 1};
    int64_t e[3];
    for (int a = 0; a < 3; ++a) e[a] = lf.n[a] > o[a] ? (lf.n[a] - o[a] + 1) / 2 : 0;
    const int64_t ncell = e[0] * e[1] * e[2];
#pragma omp parallel for schedule(static)
    for (int64_t cell = 0; cell < ncell; ++cell) {
      const int64_t cz = o[2] + 2 * (cell % e[2]), cy = o[1] + 2 * ((cell / e[2]) % e[1]),
                    cx = o[0] + 2 * (cell / (e[1] * e[2]));
      T s0[4 * 8 * 8], s1[4 * 4 * 8];
      const int ex = cx == lf.n[0] - 1 ? nf : PF, ey = cy == lf.n[1] - 1 ? nf : PF,
                ez = cz == lf.n[2] - 1 ? nf : PF;
      // x: (i, j, k) -> (a, j, k)
      for (int a = 0; a < nc; ++a)
        for (int j = 0; j < nf; ++j)
          for (int k = 0; k < nf; ++k) {
            T acc = 0;
            if (j < ey && k < ez)
              for (int i = 0; i < ex; ++i) {
                const int64_t li = cx * PF + i, lj = cy * PF + j, lk = cz * PF + k;
                if (lf.is_owned(li, lj, lk)) acc += J[i * nc + a] * vf[lf.idx(li, lj, lk)];
              }
            s0[(a * nf + j) * nf + k] = acc;
          }
      // y: (a, j, k) -> (a, b, k)
      for (int a = 0; a < nc; ++a)
        for (int b = 0; b < nc; ++b)
          for (int k = 0; k < nf; ++k) {
            T acc = 0;
            for (int j = 0; j < nf; ++j) acc += J[j * nc + b] * s0[(a * nf + j) * nf + k];
            s1[(a * nc + b) * nf + k] = acc;
          }
      // z: (a, b, k) -> (a, b, c)
      for (int a = 0; a < nc; ++a)
        for (int b = 0; b < nc; ++b)
          for (int c = 0; c < nc; ++c) {
            T acc = 0;
            for (int k = 0; k < nf; ++k) acc += J[k * nc + c] * s1[(a * nc + b) * nf + k];
            vc[lc.idx(cx * PC + a, cy * PC + b, cz * PC + c)] += acc;
          }
    }
  }
  return 0;
}

// ------------------------------------------- p-multigrid transfers by rows
// Host twins of csrc/hip/lap_rowtransfer.h with its index helpers
// (bdx_mg_bodies.h) and its summation order: the x-y combination of the rows
// first (I outermost, then J, ascending, zero weights skipped), then z
// ascending.

// A pair transfer_pair_ok accepts, no null pointer; the table in T.
template <typename T>
bool rowtransfer_setup(const int64_t* latc, const int64_t* latf, const double* Jd, const void* src,
                       const void* dst, BdxLattice& lc, BdxLattice& lf, T (&J)[8 * 4]) {
  if (!latc || !latf || !Jd || !src || !dst) return false;
  lc = BdxLattice::from(latc);
  lf = BdxLattice::from(latf);
  if (!transfer_pair_ok(lc, lf)) return false;
  for (int i = 0; i < (lf.P + 1) * (lc.P + 1); ++i) J[i] = static_cast<T>(Jd[i]);
  return true;
}

// add = 0: vf = P vc on every local fine node; add: vf += P vc on the owned ones.
template <typename T>
int prolong_row_host(const int64_t* latc, const int64_t* latf, const double* Jd, const T* vc,
                     T* vf, int add) {
  BdxLattice lc, lf;
  T J[8 * 4];
  if (!rowtransfer_setup<T>(latc, latf, Jd, vc, vf, lc, lf, J)) return 1;
  if (lf.n[0] == 0 || lf.n[1] == 0 || lf.n[2] == 0) return 0;
  const int64_t PF = lf.P, PC = lc.P, NC = PC + 1;
  const int64_t e[3] = {add ? lf.L[0] - lf.gh[0] : lf.L[0], add ? lf.L[1] - lf.gh[1] : lf.L[1],
                        add ? lf.L[2] - lf.gh[2] : lf.L[2]};
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t I = 0; I < e[0]; ++I)
    for (int64_t Jr = 0; Jr < e[1]; ++Jr) {
      int64_t cx, qx, cy, qy;
      ptransfer_cell(I, PF, lf.n[0], cx, qx);
      ptransfer_cell(Jr, PF, lf.n[1], cy, qy);
      for (int64_t k = 0; k < e[2]; ++k) {
        int64_t cz, qz;
        ptransfer_cell(k, PF, lf.n[2], cz, qz);
        T out = 0;
        for (int64_t c = 0; c < NC; ++c) {
          T t = 0;
          for (int64_t a = 0; a < NC; ++a)
            for (int64_t b = 0; b < NC; ++b) {
              const T w = J[qx * NC + a] * J[qy * NC + b];
              if (w == 0) continue;
              t += w * vc[lc.idx(cx * PC + a, cy * PC + b, cz * PC + c)];
            }
          out += J[qz * NC + c] * t;
        }
        const int64_t to = lf.idx(I, Jr, k);
        vf[to] = add ? vf[to] + out : out;
      }
    }
  return 0;
}

// vc = P^T (vf - y) (y null: P^T vf) on every local coarse node, from the
// owned fine nodes.
template <typename T>
int restrict_row_host(const int64_t* latc, const int64_t* latf, const double* Jd, const T* vf,
                      const T* y, T* vc) {
  BdxLattice lc, lf;
  T J[8 * 4];
  if (!rowtransfer_setup<T>(latc, latf, Jd, vf, vc, lc, lf, J)) return 1;
  if (lf.n[0] == 0 || lf.n[1] == 0 || lf.n[2] == 0) return 0;
  const int64_t PF = lf.P, PC = lc.P;
  const int64_t own[3] = {lf.L[0] - lf.gh[0], lf.L[1] - lf.gh[1], lf.L[2] - lf.gh[2]};
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t A = 0; A < lc.L[0]; ++A)
    for (int64_t B = 0; B < lc.L[1]; ++B) {
      int64_t ilo, ihi, jlo, jhi;
      ptransfer_support(A, PF, PC, lf.n[0], own[0], ilo, ihi);
      ptransfer_support(B, PF, PC, lf.n[1], own[1], jlo, jhi);
      for (int64_t C = 0; C < lc.L[2]; ++C) {
        int64_t klo, khi;
        ptransfer_support(C, PF, PC, lf.n[2], own[2], klo, khi);
        T out = 0;
        for (int64_t k = klo; k <= khi; ++k) {
          T s = 0;
          for (int64_t I = ilo; I <= ihi; ++I)
            for (int64_t Jr = jlo; Jr <= jhi; ++Jr) {
              const T w = ptransfer_weight<T>(J, I, A, PF, PC, lf.n[0]) *
                          ptransfer_weight<T>(J, Jr, B, PF, PC, lf.n[1]);
              if (w == 0) continue;
              const int64_t at = lf.idx(I, Jr, k);
              s += w * (y ? vf[at] - y[at] : vf[at]);
            }
          out += ptransfer_weight<T>(J, k, C, PF, PC, lf.n[2]) * s;
        }
        vc[lc.idx(A, B, C)] = out;
      }
    }
  return 0;
}

// ------------------------------------------------- h-multigrid transfers
// Host twins of csrc/hip/lap_htransfer.h: hprolong_node / hrestrict_node
// (bdx_mg_bodies.h) on every node; cidx / cw (fine lengths) and fpos (coarse
// lengths) hold the three axes one after the other.

// vf (+)= P vc on the nodes below e: vf[n] = P vc (add = 0) or vf[n] += P vc.
template <typename T>
void hprolong_nodes(const BdxLattice& lc, const BdxLattice& lf, const HTransferTables<T>& tab,
                    const int64_t (&e)[3], const T* vc, T* vf, int add) {
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t i = 0; i < e[0]; ++i)
    for (int64_t j = 0; j < e[1]; ++j)
      for (int64_t k = 0; k < e[2]; ++k) {
        const T out = hprolong_node<T>(lc, tab, vc, i, j, k);
        const int64_t to = lf.idx(i, j, k);
        vf[to] = add ? vf[to] + out : out;
      }
}

// vc = P^T (vf - y) (y null: P^T vf) on every local coarse node.
template <typename T>
void hrestrict_nodes(const BdxLattice& lc, const BdxLattice& lf, const HTransferTables<T>& tab,
                     const T* vf, const T* y, T* vc) {
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t i = 0; i < lc.L[0]; ++i)
    for (int64_t j = 0; j < lc.L[1]; ++j)
      for (int64_t k = 0; k < lc.L[2]; ++k)
        vc[lc.idx(i, j, k)] = hrestrict_node<T>(lc, lf, tab, vf, y, i, j, k);
}

// add = 0: every local fine node; add: owned fine nodes only.
template <typename T>
int hprolong_host(const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw,
                  const int* fpos, const T* vc, T* vf, int add) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!htransfer_pair_ok(lc, lf) || !cidx || !cw || !fpos || !vc || !vf) return 1;
  const int64_t e[3] = {add ? lf.L[0] - lf.gh[0] : lf.L[0], add ? lf.L[1] - lf.gh[1] : lf.L[1],
                        add ? lf.L[2] - lf.gh[2] : lf.L[2]};
  hprolong_nodes<T>(lc, lf, htransfer_tables<T>(lc, lf, cidx, cw, fpos), e, vc, vf, add);
  return 0;
}

template <typename T>
int hrestrict_host(const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw,
                   const int* fpos, const T* vf, const T* y, T* vc) {
  const BdxLattice lc = BdxLattice::from(latc), lf = BdxLattice::from(latf);
  if (!htransfer_pair_ok(lc, lf) || !cidx || !cw || !fpos || !vc || !vf) return 1;
  hrestrict_nodes<T>(lc, lf, htransfer_tables<T>(lc, lf, cidx, cw, fpos), vf, y, vc);
  return 0;
}

// Host twin of bdx_cheb_step (csrc/hip/blas.hip) over the owned rows.
template <typename T>
void cheb_step_host(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, int first, T a,
                    T b, const T* dinv, const T* r, const T* y, T* d, T* z) {
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t i = 0; i < o0; ++i)
    for (int64_t j = 0; j < o1; ++j) {
      const int64_t base = (i * L1 + j) * ld;
      for (int64_t k = base; k < base + o2; ++k) cheb_entry<T>(first, a, b, dinv, r, y, d, z, k);
    }
}

// out = (TO)a over the owned rows: the precision boundary of the mixed
// multigrid solve (csrc/hip/mixed.hip); nothing outside the rows is touched.
template <typename TI, typename TO>
void convert_rows_host(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, const TI* a,
                       TO* out) {
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t i = 0; i < o0; ++i)
    for (int64_t j = 0; j < o1; ++j) {
      const int64_t base = (i * L1 + j) * ld;
      for (int64_t k = base; k < base + o2; ++k) out[k] = static_cast<TO>(a[k]);
    }
}

// ------------------------------------------------------ V-cycle tail
// Host twin of csrc/hip/pmg_tail.h: the levels of the table (bdx_pmg_tail.h)
// walked down then up with the schedule of `PMultigrid._vcycle`, every phase
// a loop over the nodes of a level with the body the device kernel gives a
// thread.

// y = A z with the 27-point stencil S[27][lat.size()] (stencil27_node).
template <typename T>
void stencil_host(const BdxLattice& lat, const T* S, const T* z, T* y) {
  const int L0 = static_cast<int>(lat.L[0]), L1 = static_cast<int>(lat.L[1]),
            L2 = static_cast<int>(lat.L[2]);
  for (int i = 0; i < L0; ++i)
    for (int j = 0; j < L1; ++j)
      for (int k = 0; k < L2; ++k) y[lat.idx(i, j, k)] = stencil27_node<T>(lat, S, z, i, j, k);
}

// Host twin of bdx_stencil27_cheb (csrc/hip/lap_stencil27.h): the same bodies
// on the owned nodes.
template <typename T>
int stencil_cheb_host(const int64_t* latd, const int64_t* own, const T* S, const T* dinv,
                      const T* r, const T* z_in, T* d, T* z_out, T a, T b) {
  if (!latd || !own || !S || !dinv || !r || !z_in || !d || !z_out || z_out == z_in) return 1;
  const BdxLattice lat = BdxLattice::from(latd);
  if (lat.tsy || lat.P != 1 || lat.ld < lat.L[2] || lat.ld > 0x7fffffffLL) return 1;
  for (int ax = 0; ax < 3; ++ax)
    if (lat.L[ax] < 1 || lat.L[ax] > 0x7fffffffLL || lat.L[ax] != lat.n[ax] + 1 || own[ax] < 0 ||
        own[ax] > lat.L[ax])
      return 1;
  const int o0 = static_cast<int>(own[0]), o1 = static_cast<int>(own[1]),
            o2 = static_cast<int>(own[2]);
#pragma omp parallel for collapse(2) schedule(static)
  for (int i = 0; i < o0; ++i)
    for (int j = 0; j < o1; ++j)
      for (int k = 0; k < o2; ++k) {
        const T s = stencil27_node<T>(lat, S, z_in, i, j, k);
        cheb_entry_fused<T>(true, a, b, dinv, r, s, d, z_in, z_out, lat.idx(i, j, k));
      }
  return 0;
}

// Host twin of bdx_stencil27_assemble (csrc/hip/lap_stencil27_assemble.h):
// stencil27_assemble_node on every node of the storage, padding included.
template <typename T>
int stencil_assemble_host(const int64_t* latd, int nq, const double* phi0, const double* dphi1,
                          const double* wts, const double* qpts, const T* xv, T kappa,
                          const T* kc, T* S) {
  if (!latd || !phi0 || !dphi1 || !wts || !qpts || !xv || !S || nq < 2 || nq > kStencil27MaxNq)
    return 1;
  const BdxLattice lat = BdxLattice::from(latd);
  if (lat.tsy || lat.P != 1 || lat.ld < lat.L[2] || lat.ld > 0x7fffffffLL) return 1;
  for (int ax = 0; ax < 3; ++ax)
    if (lat.L[ax] < 1 || lat.L[ax] > 0x7fffffffLL || lat.L[ax] != lat.n[ax] + 1) return 1;
  const Stencil27Tables<T> tb = stencil27_tables<T>(nq, phi0, dphi1, wts, qpts);
  const int L0 = static_cast<int>(lat.L[0]), L1 = static_cast<int>(lat.L[1]),
            ld = static_cast<int>(lat.ld);
  const int64_t ns = lat.size();
#pragma omp parallel for collapse(2) schedule(static)
  for (int i = 0; i < L0; ++i)
    for (int j = 0; j < L1; ++j)
      for (int k = 0; k < ld; ++k) {
        T acc[27];
        stencil27_assemble_node<T>(lat, tb, xv, kappa, kc, i, j, k, acc);
        const int64_t at = lat.idx(i, j, k);
        for (int p = 0; p < 27; ++p) S[p * ns + at] = acc[p];
      }
  return 0;
}

template <typename T>
void tail_smooth_host(const TailLevel<T>& v, bool zero_guess) {
  const BdxLattice& l = v.lat;
  for (int s = 0; s < v.ncoef; ++s) {
    const T a = static_cast<T>(v.coef[2 * s]), b = static_cast<T>(v.coef[2 * s + 1]);
    const bool first = s == 0 && zero_guess;
    if (!first) stencil_host<T>(l, v.S, v.z, v.y);
    cheb_step_host<T>(l.L[1], l.ld, l.L[0], l.L[1], l.L[2], first, a, b, v.dinv, v.r, v.y, v.d,
                      v.z);
  }
}

template <typename T>
int pmg_tail_host(const int64_t* tab, int nlev, int64_t nwords, const T* r, T* z) {
  if (!r || !z || !tail_table_ok(tab, nlev, nwords)) return 1;
  for (int l = 0; l < nlev; ++l) {
    const TailLevel<T> v = tail_level<T>(tab, l, r, z);
    tail_smooth_host(v, true);
    if (l == nlev - 1) break;
    const TailLevel<T> c = tail_level<T>(tab, l + 1, r, z);
    stencil_host<T>(v.lat, v.S, v.z, v.y);
    // r_c = R (r - y), Dirichlet entries zeroed
    hrestrict_nodes<T>(c.lat, v.lat, htransfer_tables<T>(c.lat, v.lat, v.cidx, v.cw, v.fpos), v.r,
                       v.y, c.r);
    for (int64_t i = 0; i < c.lat.L[0]; ++i)
      for (int64_t j = 0; j < c.lat.L[1]; ++j)
        for (int64_t k = 0; k < c.lat.L[2]; ++k) {
          const int64_t at = c.lat.idx(i, j, k);
          if (c.bc[at]) c.r[at] = 0;
        }
  }
  for (int l = nlev - 2; l >= 0; --l) {
    const TailLevel<T> v = tail_level<T>(tab, l, r, z);
    const TailLevel<T> c = tail_level<T>(tab, l + 1, r, z);
    // z += P z_c (a tail level has no ghost planes: every node is owned)
    hprolong_nodes<T>(c.lat, v.lat, htransfer_tables<T>(c.lat, v.lat, v.cidx, v.cw, v.fpos),
                      v.lat.L, c.z, v.z, 1);
    tail_smooth_host(v, false);
  }
  return 0;
}

}  // namespace

extern "C" {

#define BDX_HOST_MG_API(T, SUF)                                               \
  int bdx_cpu_prolong_##SUF BDX_P_CPU_PROLONG(T) {                            \
    return prolong_host<T>(latc, latf, J, vc, vf);                            \
  }                                                                           \
  int bdx_cpu_restrict_##SUF BDX_P_CPU_RESTRICT(T) {                          \
    return restrict_host<T>(latc, latf, J, vf, vc);                           \
  }                                                                           \
  int bdx_cpu_hprolong_##SUF BDX_P_CPU_HPROLONG(T) {                          \
    return hprolong_host<T>(latc, latf, cidx, cw, fpos, vc, vf, add);         \
  }                                                                           \
  int bdx_cpu_hrestrict_##SUF BDX_P_CPU_HRESTRICT(T) {                        \
    return hrestrict_host<T>(latc, latf, cidx, cw, fpos, vf, y, vc);          \
  }                                                                           \
  int bdx_cpu_prolong_row_##SUF BDX_P_CPU_PROLONG_ROW(T) {                    \
    return prolong_row_host<T>(latc, latf, J, vc, vf, add);                   \
  }                                                                           \
  int bdx_cpu_restrict_row_##SUF BDX_P_CPU_RESTRICT_ROW(T) {                  \
    return restrict_row_host<T>(latc, latf, J, vf, y, vc);                    \
  }                                                                           \
  void bdx_cpu_cheb_step_##SUF BDX_P_CPU_CHEB_STEP(T) {                       \
    cheb_step_host<T>(L1, ld, o0, o1, o2, first, static_cast<T>(a),           \
                      static_cast<T>(b), dinv, r, y, d, z);                   \
  }                                                                           \
  int bdx_cpu_pmg_tail_##SUF BDX_P_CPU_PMG_TAIL(T) {                          \
    return pmg_tail_host<T>(tab, nlev, nwords, r, z);                         \
  }                                                                           \
  void bdx_cpu_stencil27_##SUF BDX_P_CPU_STENCIL27(T) {                       \
    stencil_host<T>(BdxLattice::from(latd), S, z, y);                         \
  }                                                                           \
  int bdx_cpu_stencil27_cheb_##SUF BDX_P_CPU_STENCIL27_CHEB(T) {              \
    return stencil_cheb_host<T>(latd, own, S, dinv, r, z_in, d, z_out,        \
                                static_cast<T>(a), static_cast<T>(b));        \
  }                                                                           \
  int bdx_cpu_stencil27_assemble_##SUF BDX_P_CPU_STENCIL27_ASSEMBLE(T) {      \
    return stencil_assemble_host<T>(latd, nq, phi0, dphi1, wts, qpts, xv,     \
                                    static_cast<T>(kappa), kc, S);            \
  }

BDX_HOST_MG_API(double, f64)
BDX_HOST_MG_API(float, f32)

// out = (float)a over the owned rows (round to nearest even): the host twin
// of bdx_demote_f64_f32 (csrc/hip/mixed.hip).
void bdx_cpu_demote_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                            const double* a, float* out) {
  convert_rows_host<double, float>(L1, ld, o0, o1, o2, a, out);
}

// out = (double)a over the owned rows (exact): the host twin of
// bdx_promote_f32_f64.
void bdx_cpu_promote_f32_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                             const float* a, double* out) {
  convert_rows_host<float, double>(L1, ld, o0, o1, o2, a, out);
}

}  // extern "C"
