// Matrix-free diagonal of the stiffness operator, diag(A) without assembly
// (the reference's hook: MatrixOperator::get_diag_inverse, src/csr.hpp:81-106,
// there read off the assembled matrix; here sum-factorised per cell).
//
// With B = phi0 and Dd = dphi1 phi0 (nq x nd) the element diagonal of node
// (i, j, k) is
//   d_e = kappa sum_q [ G0 DD[qx,i] BB[qy,j] BB[qz,k] + G3 BB DD BB + G5 BB BB DD
//                     + 2 G1 BD BD BB + 2 G2 BD BB BD + 2 G4 BB BD BD ]
// with BB = B.B, DD = Dd.Dd, BD = B.Dd (pointwise) and G = w adj(J) adj(J)^T
// / det J in the order (xx, xy, xz, yy, yz, zz) of geometry_G.  It is
// contracted 6 -> 6 -> 3 -> 1 arrays along z, y, x:
//   z:  a0 = sum G0 BBz   a1 = sum G3 BBz    a2 = sum G5 DDz
//       a3 = 2 sum G1 BBz a4 = 2 sum G2 BDz  a5 = 2 sum G4 BDz
//   y:  cDD = sum a0 BBy  cBB = sum (a1 DDy + a2 BBy + a5 BDy)
//       cBD = sum (a3 BDy + a4 BBy)
//   x:  d = sum (cDD DDx + cBB BBx + cBD BDx)
// One thread per quadrature point, V1Shape's cells per workgroup, tables and
// the six intermediates in LDS, geometry on the fly from the 8 cell vertices.
//
// No atomics: one launch per cell-parity colour (cx & 1, cy & 1, cz & 1).  No
// two cells of a colour share a dof, so the plain d[dof] += d_e is race-free
// and the summation order (colour 0..7) is fixed: results are bitwise
// reproducible.  Dirichlet dofs are skipped (the caller sets them to 1).
#pragma once
#include "lap_v1.h"

// Shared-memory image of one diagonal workgroup (CPB cells x nq^3 points).
template <typename T, int ND, int NQ>
struct DiagSmem {
  static constexpr int nq3 = NQ * NQ * NQ, CPB = V1Shape<NQ>::cpb;
  T B[NQ * ND];
  T Dd[NQ * ND];
  T s[6][CPB][nq3];
  T X[CPB][8][3];
};

// d[dof] += d_e over the cells (lo + 2 c) of one parity colour, c in [0, e).
template <typename T, int ND, int NQ>
__global__ void __launch_bounds__(V1Shape<NQ>::threads)
    lap_diag_kernel(BdxLattice lat, OpTables<T> tb, const T* __restrict__ xv, T kappa,
                    const T* __restrict__ kc, T* __restrict__ d, int64_t lo0, int64_t lo1,
                    int64_t lo2, int64_t e0, int64_t e1, int64_t e2) {
  constexpr int nq3 = NQ * NQ * NQ;
  constexpr int CPB = V1Shape<NQ>::cpb;
  __shared__ DiagSmem<T, ND, NQ> sm;

  const int tid = threadIdx.x;
  for (int i = tid; i < NQ * ND; i += blockDim.x) {
    const int q = i / ND, a = i - q * ND;
    sm.B[i] = tb.phi0[i];
    T acc = 0;
    for (int m = 0; m < NQ; ++m) acc += tb.dphi1[q * NQ + m] * tb.phi0[m * ND + a];
    sm.Dd[i] = acc;
  }

  const int cs_raw = tid / nq3;
  const bool active = cs_raw < CPB;
  const int cs = active ? cs_raw : 0;
  const int q = tid - cs_raw * nq3;
  const int qx = q / (NQ * NQ), qy = (q / NQ) % NQ, qz = q % NQ;
  const int64_t ncell = e0 * e1 * e2;
  const int64_t cell_lin = static_cast<int64_t>(blockIdx.x) * CPB + cs;
  const bool valid = active && cell_lin < ncell;
  int64_t cx = 0, cy = 0, cz = 0;
  if (valid) {
    cz = lo2 + 2 * (cell_lin % e2);
    cy = lo1 + 2 * ((cell_lin / e2) % e1);
    cx = lo0 + 2 * (cell_lin / (e1 * e2));
  }
  // the cell's 24 vertex coordinates, strided over its nq^3 threads (nq = 2: 8 threads)
  if (valid) {
    for (int i = q; i < 24; i += nq3) {
      const int v = i / 3, c = i % 3;
      sm.X[cs][v][c] = xv[3 * lat.vidx(cx + (v >> 2), cy + ((v >> 1) & 1), cz + (v & 1)) + c];
    }
  }
  __syncthreads();

  // kappa G at this thread's quadrature point
  {
    T Gd[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
      const T w = tb.wts[qx] * tb.wts[qy] * tb.wts[qz];
      geometry_G<T>(sm.X[cs], tb.qpts[qx], tb.qpts[qy], tb.qpts[qz], w, Gd);
      const T kap = kc ? kc[cell_index(lat, cx, cy, cz)] : kappa;
#pragma unroll
      for (int n = 0; n < 6; ++n) Gd[n] *= kap;
    }
    if (active) {
#pragma unroll
      for (int n = 0; n < 6; ++n) sm.s[n][cs][q] = Gd[n];
    }
  }
  __syncthreads();

  // z: thread (qx, qy, k = qz < ND)
  T a[6] = {0, 0, 0, 0, 0, 0};
  if (active && qz < ND) {
    const int row = (qx * NQ + qy) * NQ;
#pragma unroll
    for (int z = 0; z < NQ; ++z) {
      const T b = sm.B[z * ND + qz], dd = sm.Dd[z * ND + qz];
      const T bb = b * b, dD = dd * dd, bd = b * dd;
      a[0] += sm.s[0][cs][row + z] * bb;
      a[1] += sm.s[3][cs][row + z] * bb;
      a[2] += sm.s[5][cs][row + z] * dD;
      a[3] += sm.s[1][cs][row + z] * bb;
      a[4] += sm.s[2][cs][row + z] * bd;
      a[5] += sm.s[4][cs][row + z] * bd;
    }
    a[3] *= 2;
    a[4] *= 2;
    a[5] *= 2;
  }
  __syncthreads();
  if (active && qz < ND) {
#pragma unroll
    for (int n = 0; n < 6; ++n) sm.s[n][cs][q] = a[n];
  }
  __syncthreads();

  // y: thread (qx, j = qy < ND, k)
  T cDD = 0, cBB = 0, cBD = 0;
  if (active && qy < ND && qz < ND) {
#pragma unroll
    for (int y = 0; y < NQ; ++y) {
      const int at = (qx * NQ + y) * NQ + qz;
      const T b = sm.B[y * ND + qy], dd = sm.Dd[y * ND + qy];
      const T bb = b * b, dD = dd * dd, bd = b * dd;
      cDD += sm.s[0][cs][at] * bb;
      cBB += sm.s[1][cs][at] * dD + sm.s[2][cs][at] * bb + sm.s[5][cs][at] * bd;
      cBD += sm.s[3][cs][at] * bd + sm.s[4][cs][at] * bb;
    }
  }
  __syncthreads();
  if (active && qy < ND && qz < ND) {
    sm.s[0][cs][q] = cDD;
    sm.s[1][cs][q] = cBB;
    sm.s[2][cs][q] = cBD;
  }
  __syncthreads();

  // x: thread (i = qx < ND, j, k) owns node (i, j, k) of its cell
  if (valid && qx < ND && qy < ND && qz < ND) {
    T de = 0;
#pragma unroll
    for (int x = 0; x < NQ; ++x) {
      const int at = (x * NQ + qy) * NQ + qz;
      const T b = sm.B[x * ND + qx], dd = sm.Dd[x * ND + qx];
      de += sm.s[0][cs][at] * (dd * dd) + sm.s[1][cs][at] * (b * b) + sm.s[2][cs][at] * (b * dd);
    }
    const int64_t P = lat.P;
    const int64_t li = cx * P + qx, lj = cy * P + qy, lk = cz * P + qz;
    if (!lat.is_bc(li, lj, lk)) {
      const int64_t dof = lat.idx(li, lj, lk);
      if (!BDX_OOB(dof, lat.size(), "diag")) d[dof] += de;
    }
  }
}

// The eight colour launches over the cell box [lo, hi), in a fixed order.
template <typename T, int ND, int NQ>
int launch_diag(const BdxLattice& lat, const OpTables<T>& tb, const T* xv, T kappa, const T* kc,
                T* d, const int64_t* lo, const int64_t* hi, hipStream_t st) {
  constexpr int cpb = V1Shape<NQ>::cpb;
  for (int colour = 0; colour < 8; ++colour) {
    const int64_t o[3] = {(colour >> 2) & 1, (colour >> 1) & 1, colour & 1};
    int64_t e[3];
    for (int a = 0; a < 3; ++a) {
      const int64_t span = hi[a] - lo[a] - o[a];
      e[a] = span > 0 ? (span + 1) / 2 : 0;
    }
    const int64_t ncell = e[0] * e[1] * e[2];
    if (ncell <= 0) continue;
    const int64_t nblk = (ncell + cpb - 1) / cpb;
    if (nblk > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
    lap_diag_kernel<T, ND, NQ><<<static_cast<unsigned>(nblk), V1Shape<NQ>::threads, 0, st>>>(
        lat, tb, xv, kappa, kc, d, lo[0] + o[0], lo[1] + o[1], lo[2] + o[2], e[0], e[1], e[2]);
    BDX_CHECK(hipGetLastError());
  }
  return 0;
}

template <typename T>
int dispatch_diag(int P, int nq, const BdxLattice& lat, const OpTables<T>& tb, const T* xv,
                  T kappa, const T* kc, T* d, const int64_t* lo, const int64_t* hi,
                  hipStream_t st) {
#define BDX_DIAG_CASE(PP)                                                             \
  case PP:                                                                            \
    if (nq == PP + 1)                                                                 \
      return launch_diag<T, PP + 1, PP + 1>(lat, tb, xv, kappa, kc, d, lo, hi, st);   \
    if (nq == PP + 2)                                                                 \
      return launch_diag<T, PP + 1, PP + 2>(lat, tb, xv, kappa, kc, d, lo, hi, st);   \
    break;
  switch (P) {
    BDX_DIAG_CASE(1)
    BDX_DIAG_CASE(2)
    BDX_DIAG_CASE(3)
    BDX_DIAG_CASE(4)
    BDX_DIAG_CASE(5)
    BDX_DIAG_CASE(6)
    BDX_DIAG_CASE(7)
  }
#undef BDX_DIAG_CASE
  return static_cast<int>(hipErrorInvalidValue);
}

#define BDX_DIAG_API(T, SUF)                                                           \
  extern "C" int bdx_diag_##SUF BDX_P_DIAG(T) {                                        \
    const BdxLattice lat = BdxLattice::from(latd);                                     \
    if (lat.tsy) return static_cast<int>(hipErrorInvalidValue);                        \
    for (int a = 0; a < 3; ++a)                                                        \
      if (lo[a] < 0 || hi[a] > lat.n[a]) return static_cast<int>(hipErrorInvalidValue); \
    const int P = static_cast<int>(lat.P);                                             \
    if (P < 1 || P > 7 || nq < P + 1 || nq > P + 2)                                    \
      return static_cast<int>(hipErrorInvalidValue);                                   \
    const OpTables<T> tb =                                                             \
        make_op_tables<T>(P + 1, nq, phi0, dphi1, wts, qpts, identity);                \
    return dispatch_diag<T>(P, nq, lat, tb, xv, static_cast<T>(kappa), kc, d, lo, hi,  \
                            st);                                                       \
  }
