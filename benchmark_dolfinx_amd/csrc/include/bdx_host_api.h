// The C ABI of libbdx_host.so: every exported entry point, declared once.
//
// bdx_host.cpp and bdx_host_mg.cpp include this header before their
// definitions, so the compiler rejects a definition that disagrees; the ctypes
// table (ops/host_api.py) is pinned to it by tests/test_api_signatures.py.
// BDX_P_<NAME>(T) is the parameter list of the _f64 (T = double) and _f32
// (T = float) twins; the macro-generated definitions reuse it.
#pragma once
#include <cstdint>

#include "bdx_rt_setup.h"

#define BDX_HOST_TWINS(R, NAME, PARAMS) \
  R NAME##_f64 PARAMS(double);          \
  R NAME##_f32 PARAMS(float);

extern "C" {

// -------------------------------------------------------------- bdx_host.cpp
// ABI version of the host library.
int bdx_host_version();
// The CG runtimes' own checks of a setup record (bdx_rt_setup.h), as
// bdx_rt_create / bdx_rt_create_dofmap make them: 1 = accepted.  Nothing the
// record points to is read.
int bdx_cpu_rt_fused_setup_ok(const BdxRtFusedSetup* s);
int bdx_cpu_rt_dofmap_setup_ok(const BdxRtDofmapSetup* s);
// y += A u over the cells [lo, hi) of the local lattice (geometry on the fly).
#define BDX_P_CPU_STIFFNESS(T) (const int64_t* latd, int nq, const T* phi0, const T* dphi1, const T* wts, \
  const T* qpts, const T* nodes, int identity, const T* xv, T kappa, const T* kc, const T* u, T* y, \
  const int64_t* lo, const int64_t* hi)
BDX_HOST_TWINS(void, bdx_cpu_stiffness, BDX_P_CPU_STIFFNESS)
// The same with precomputed geometry factors G (null: on the fly).
#define BDX_P_CPU_STIFFNESS_G(T) (const int64_t* latd, int nq, const T* phi0, const T* dphi1, const T* wts, \
  const T* qpts, const T* nodes, int identity, const T* xv, const T* G, T kappa, const T* kc, const T* u, T* y, \
  const int64_t* lo, const int64_t* hi)
BDX_HOST_TWINS(void, bdx_cpu_stiffness_g, BDX_P_CPU_STIFFNESS_G)
// The reference data model on the CPU (dofmap_cells).
#define BDX_P_CPU_DOFMAP(T) (int P, int nq, const T* phi0, const T* dphi1, const T* wts, const T* qpts, \
  int identity, const int* cells, int ncl, const int* cdofs, const int* cverts, const T* coords, const T* G, \
  const unsigned char* flags, T kappa, const T* kc, const T* u, T* y)
BDX_HOST_TWINS(void, bdx_cpu_dofmap, BDX_P_CPU_DOFMAP)
// Stored geometry factors G of a cell list in the reference layout.
#define BDX_P_CPU_DOFMAP_GEOMETRY(T) (int P, int nq, const T* wts, const T* qpts, int ncells, const int* cverts, \
  const T* coords, T* G)
BDX_HOST_TWINS(void, bdx_cpu_dofmap_geometry, BDX_P_CPU_DOFMAP_GEOMETRY)
// Geometry factors of every local cell, reference layout [c][6][nq^3].
#define BDX_P_CPU_GEOMETRY(T) (const int64_t* latd, int nq, const T* wts, const T* qpts, const T* xv, T* G)
BDX_HOST_TWINS(void, bdx_cpu_geometry, BDX_P_CPU_GEOMETRY)
// b += M f (mass action) over the cells [lo, hi).
#define BDX_P_CPU_MASS(T) (const int64_t* latd, int nq, const T* phi0, const T* dphi1, const T* wts, const T* qpts, \
  const T* nodes, int identity, const T* xv, const T* f, T* b, const int64_t* lo, const int64_t* hi)
BDX_HOST_TWINS(void, bdx_cpu_mass, BDX_P_CPU_MASS)
// d += matrix-free diag(A) of the cells [lo, hi) (B = phi0, Dd = dphi1 phi0;
// Dirichlet dofs skipped): the host twin of bdx_diag.
#define BDX_P_CPU_DIAG(T) (const int64_t* latd, int nq, const T* B, const T* Dd, const T* wts, const T* qpts, \
  const T* xv, T kappa, const T* kc, T* d, const int64_t* lo, const int64_t* hi)
BDX_HOST_TWINS(void, bdx_cpu_diag, BDX_P_CPU_DIAG)
// Assembled CSR matrix of the local lattice (count_only: only row_ptr);
// returns the number of entries.
#define BDX_P_CPU_CSR(T) (const int64_t* latd, int nq, const T* B, const T* Dd, const T* wts, const T* qpts, \
  const T* xv, T kappa, const T* kc, int64_t* row_ptr, int32_t* cols, T* vals, int count_only)
BDX_HOST_TWINS(int64_t, bdx_cpu_csr, BDX_P_CPU_CSR)
// CSR y = A x (acc: y += A x), row r holding the entries [beg[r], end[r]).
#define BDX_P_CPU_SPMV(T) (int64_t nrows, const int64_t* beg, const int64_t* end, const int32_t* cols, \
  const T* vals, const T* x, T* y, int acc)
BDX_HOST_TWINS(void, bdx_cpu_spmv, BDX_P_CPU_SPMV)
// f = 1000 exp(-((x-1/2)^2 + (y-1/2)^2)/0.02) at the physical dof nodes.
#define BDX_P_CPU_INTERP_F(T) (const int64_t* latd, const T* nodes, const T* xv, T* f)
BDX_HOST_TWINS(void, bdx_cpu_interp_f, BDX_P_CPU_INTERP_F)
// CPU unit test of the RCCL deadline policy (bdx_watchdog.h); returns 1 if the
// watchdog fired, *fire_s and *reason say when and why (see the definition).
int bdx_watchdog_selftest(double timeout_s, double busy_s, double err_after_s, double* fire_s,
                          int* reason);

// ----------------------------------------------------------- bdx_host_mg.cpp
// p-multigrid transfers between the coarse and fine lattices latc / latf
// (J: the (Pf + 1) x (Pc + 1) 1D table): vf = P vc, vc += P^T vf; the host
// twins of bdx_prolong / bdx_restrict, nonzero for a bad pair.
#define BDX_P_CPU_PROLONG(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vc, T* vf)
BDX_HOST_TWINS(int, bdx_cpu_prolong, BDX_P_CPU_PROLONG)
// (see bdx_cpu_prolong)
#define BDX_P_CPU_RESTRICT(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vf, T* vc)
BDX_HOST_TWINS(int, bdx_cpu_restrict, BDX_P_CPU_RESTRICT)
// h-multigrid transfers between the degree-1 lattices latc / latf with the
// tables cidx, cw, fpos: vf (+)= P vc, vc = P^T (vf - y); the host twins of
// bdx_hprolong / bdx_hrestrict, nonzero for a bad pair.
#define BDX_P_CPU_HPROLONG(T) (const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw, \
  const int* fpos, const T* vc, T* vf, int add)
BDX_HOST_TWINS(int, bdx_cpu_hprolong, BDX_P_CPU_HPROLONG)
// (see bdx_cpu_hprolong)
#define BDX_P_CPU_HRESTRICT(T) (const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw, \
  const int* fpos, const T* vf, const T* y, T* vc)
BDX_HOST_TWINS(int, bdx_cpu_hrestrict, BDX_P_CPU_HRESTRICT)
// p-multigrid transfers by lattice rows: vf (+)= P vc, vc = P^T (vf - y) (y may
// be null); the host twins of bdx_prolong_row / bdx_restrict_row, nonzero for
// a bad pair or a null pointer.
#define BDX_P_CPU_PROLONG_ROW(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vc, T* vf, \
  int add)
BDX_HOST_TWINS(int, bdx_cpu_prolong_row, BDX_P_CPU_PROLONG_ROW)
// (see bdx_cpu_prolong_row)
#define BDX_P_CPU_RESTRICT_ROW(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vf, \
  const T* y, T* vc)
BDX_HOST_TWINS(int, bdx_cpu_restrict_row, BDX_P_CPU_RESTRICT_ROW)
// Chebyshev step d = a d + b dinv (r - y); z += d (first: d = z = b dinv r),
// the host twin of bdx_cheb_step.
#define BDX_P_CPU_CHEB_STEP(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, int first, double a, \
  double b, const T* dinv, const T* r, const T* y, T* d, T* z)
BDX_HOST_TWINS(void, bdx_cpu_cheb_step, BDX_P_CPU_CHEB_STEP)
// The V-cycle from the first level of the table (bdx_pmg_tail.h) down and
// back up, z = M r: the host twin of bdx_pmg_tail, nonzero for a bad table.
#define BDX_P_CPU_PMG_TAIL(T) (const int64_t* tab, int nlev, int64_t nwords, const T* r, T* z)
BDX_HOST_TWINS(int, bdx_cpu_pmg_tail, BDX_P_CPU_PMG_TAIL)
// y = A z with the 27-point stencil S of the degree-1 lattice latd (the
// tail's operator, alone).
#define BDX_P_CPU_STENCIL27(T) (const int64_t* latd, const T* S, const T* z, T* y)
BDX_HOST_TWINS(void, bdx_cpu_stencil27, BDX_P_CPU_STENCIL27)
// One Chebyshev step over the own[0] x own[1] x own[2] owned nodes with that
// stencil: d = a d + b dinv (r - S z_in); z_out = z_in + d; the host twin of
// bdx_stencil27_cheb, nonzero for a descriptor it refuses, a null pointer or
// z_out == z_in.
#define BDX_P_CPU_STENCIL27_CHEB(T) (const int64_t* latd, const int64_t* own, const T* S, const T* dinv, \
  const T* r, const T* z_in, T* d, T* z_out, double a, double b)
BDX_HOST_TWINS(int, bdx_cpu_stencil27_cheb, BDX_P_CPU_STENCIL27_CHEB)
// That stencil assembled from the vertices, kappa and the FP64 tables: the
// host twin of bdx_stencil27_assemble with its arguments, nonzero where that
// refuses.
#define BDX_P_CPU_STENCIL27_ASSEMBLE(T) (const int64_t* latd, int nq, const double* phi0, const double* dphi1, \
  const double* wts, const double* qpts, const T* xv, double kappa, const T* kc, T* S)
BDX_HOST_TWINS(int, bdx_cpu_stencil27_assemble, BDX_P_CPU_STENCIL27_ASSEMBLE)
// out = (float)a over the owned rows (round to nearest even): the host twin
// of bdx_demote_f64_f32 (csrc/hip/mixed.hip).
void bdx_cpu_demote_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                            const double* a, float* out);
// out = (double)a over the owned rows (exact): the host twin of
// bdx_promote_f32_f64.
void bdx_cpu_promote_f32_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                             const float* a, double* out);

}  // extern "C"
