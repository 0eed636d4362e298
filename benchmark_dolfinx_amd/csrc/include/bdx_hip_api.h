// The C ABI of libbdx_hip.so: every exported entry point, declared once.
//
// Every TU that defines an entry point includes this header before the
// definition, so the compiler rejects a definition that disagrees; the C++
// callers (runtime.hip) and the ctypes table (ops/hip_api.py, pinned to this
// file by tests/test_api_signatures.py) have no prototypes of their own.
//
// Twins: BDX_P_<NAME>(T) is the parameter list of bdx_<name>_f64 (T = double)
// and bdx_<name>_f32 (T = float); macro-generated definitions reuse it.
// Unless noted, an entry point returns a hipError_t value (0 = success) and
// launches on the stream st.  "Owned rows": the o0 x o1 z-rows of o2 values
// of a lattice-layout vector with L1 rows per x-plane and row pitch ld.
#pragma once
#include <cstdint>

#include "bdx_rt_setup.h"  // the CG runtimes' setup and result records

// as in hip/hip_runtime_api.h (a legal re-declaration): readable without HIP
typedef struct ihipStream_t* hipStream_t;

#define BDX_TWINS(R, NAME, PARAMS) \
  R NAME##_f64 PARAMS(double);     \
  R NAME##_f32 PARAMS(float);
// Degrees with a per-degree instance (TU lap_fused*_<suf>_p<P>.hip): the v1
// fused kernel, fused2 and fused3 take 1..7, fused5 takes 3..7.  M(P, ...).
#define BDX_FUSED_DEGREES(M, ...)                                                       \
  M(1, __VA_ARGS__) M(2, __VA_ARGS__) M(3, __VA_ARGS__) M(4, __VA_ARGS__) M(5, __VA_ARGS__) \
  M(6, __VA_ARGS__) M(7, __VA_ARGS__)
#define BDX_FUSED5_DEGREES(M, ...) \
  M(3, __VA_ARGS__) M(4, __VA_ARGS__) M(5, __VA_ARGS__) M(6, __VA_ARGS__) M(7, __VA_ARGS__)

extern "C" {

// ------------------------------------------------------------------ blas.hip
// Capacity (doubles) of the partials buffers every caller provides.
int bdx_hip_partials_size();
// Fixed-order reduction of n per-block partials into out[slot].
int bdx_reduce_partials(const double* partials, int n, double* out, int slot, hipStream_t st);
// out[slot] = a . b over the owned rows (partials: the block partials, summed
// in fixed order).
#define BDX_P_DOT(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, const T* a, const T* b, \
  double* partials, double* out, int slot, hipStream_t st)
BDX_TWINS(int, bdx_dot, BDX_P_DOT)
// alpha = s[rn_slot] / s[pap_slot]; x += alpha p; r -= alpha y; r.r over the
// owned rows -> s[out_slot].
#define BDX_P_CG_UPDATE(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* x, T* r, const T* p, \
  const T* y, double* scal, int rn_slot, int pap_slot, int out_slot, double* partials, hipStream_t st)
BDX_TWINS(int, bdx_cg_update, BDX_P_CG_UPDATE)
// p = (s[num] / s[den]) p + r over the owned rows.
#define BDX_P_P_UPDATE(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* p, const T* r, \
  const double* scal, int num, int den, hipStream_t st)
BDX_TWINS(int, bdx_p_update, BDX_P_P_UPDATE)
// Jacobi PCG update (z = dinv . r is never stored): alpha = s[rz_slot] /
// s[pap_slot]; x += alpha p; r -= alpha y; r.z -> scal[out_slot], r.r ->
// scal[rr_slot].
#define BDX_P_PCG_UPDATE(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* x, T* r, const T* p, \
  const T* y, const T* dinv, double* scal, int rz_slot, int pap_slot, int out_slot, int rr_slot, double* partials, \
  hipStream_t st)
BDX_TWINS(int, bdx_pcg_update, BDX_P_PCG_UPDATE)
// p = (s[num] / s[den]) p + dinv . r over the owned rows.
#define BDX_P_PCG_P_UPDATE(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* p, const T* r, \
  const T* dinv, const double* scal, int num, int den, hipStream_t st)
BDX_TWINS(int, bdx_pcg_p_update, BDX_P_PCG_P_UPDATE)
// Chebyshev step: d = a d + b dinv (r - y); z += d (first: d = z = b dinv r;
// y may then be null).
#define BDX_P_CHEB_STEP(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, int first, double a, \
  double b, const T* dinv, const T* r, const T* y, T* d, T* z, hipStream_t st)
BDX_TWINS(int, bdx_cheb_step, BDX_P_CHEB_STEP)
// out = alpha x + y over the owned rows.
#define BDX_P_AXPY(T) (int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* out, double alpha, const T* x, \
  const T* y, hipStream_t st)
BDX_TWINS(int, bdx_axpy, BDX_P_AXPY)
// Halo boxes of a lattice-layout vector <-> the contiguous buf of `total`
// values: mode 0 pack, 1 unpack (assign), 2 unpack (add, box by box).  boxes:
// device table, per box {lo0, lo1, lo2, e0, e1, e2, offset}.
#define BDX_P_BOX_COPY(T) (int mode, T* vec, int64_t L1, int64_t ld, const int64_t* boxes, int nboxes, \
  int64_t total, T* buf, hipStream_t st)
BDX_TWINS(int, bdx_box_copy, BDX_P_BOX_COPY)
// The same on a lattice descriptor (lattice or tiled storage).
#define BDX_P_BOX_COPY_LAT(T) (int mode, T* vec, const int64_t* latd, const int64_t* boxes, int nboxes, \
  int64_t total, T* buf, hipStream_t st)
BDX_TWINS(int, bdx_box_copy_lat, BDX_P_BOX_COPY_LAT)
// Lattice <-> tiled copy of a vector (dir 0: to tiled, 1: back).
#define BDX_P_LAYOUT_CONVERT(T) (int dir, const int64_t* latd_tiled, T* lat, T* tiled, hipStream_t st)
BDX_TWINS(int, bdx_layout_convert, BDX_P_LAYOUT_CONVERT)
// Tiled x += a1 p1 [+ a2 p2], exported to the lattice layout (p2 may be null;
// p2mask bits 0-1: tile colours that take it, bit 2: export only, the tiled
// iterate keeps its lagged terms pending).  a = scal[num] / scal[den], den < 0:
// scal[num] itself.
#define BDX_P_FLUSH_EXPORT(T) (const int64_t* latd_tiled, T* lat, T* tiled, const T* p1, const T* p2, \
  const double* scal, int num1, int den1, int num2, int den2, int p2mask, hipStream_t st)
BDX_TWINS(int, bdx_flush_export, BDX_P_FLUSH_EXPORT)

// ------------------------------------------- cg_update.hip, fused_common.hip
// CG update of the fused2..5 paths, lattice layout: alpha = s[rn_slot] /
// s[pap_slot]; r -= alpha (y + the tile-interface partials yb / zb / cb, folded
// on the fly); r.r over the owned nodes -> scal[out_slot].  x is not touched
// (its update is lagged into the next operator launch, see bdx_xflush).
#define BDX_P_CG_UPDATE_IFACE(T) (const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb, \
  const T* zb, const T* cb, int nty, int ntz, int sy, int sz, double* scal, int rn_slot, int pap_slot, int out_slot, \
  double* partials, hipStream_t st)
BDX_TWINS(int, bdx_cg_update_iface, BDX_P_CG_UPDATE_IFACE)
// x += (s[num] / s[den]) p over the owned nodes (den < 0: s[num] itself): the
// flush of the lagged x update.
#define BDX_P_XFLUSH(T) (const int64_t* latd, const int64_t* own, T* x, const T* p, const double* scal, int num, \
  int den, hipStream_t st)
BDX_TWINS(int, bdx_xflush, BDX_P_XFLUSH)
// Tiled-storage variant of the r update (latd: the tiled descriptor of
// bdx_lattice.h).
#define BDX_P_CG_UPDATE_TILED(T) (const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb, \
  const T* zb, const T* cb, int nty, int ntz, double* scal, int rn_slot, int pap_slot, int out_slot, \
  double* partials, hipStream_t st)
BDX_TWINS(int, bdx_cg_update_tiled, BDX_P_CG_UPDATE_TILED)
// Jacobi-preconditioned r update of the fused CG loop, lattice layout:
// bdx_cg_update_iface_* (same fold, same r, bit for bit) plus z = dinv . r
// stored for every vector r is stored for, r.z -> scal[out_slot] and
// r.r -> scal[rr_slot] over the owned nodes.  partials_rr: a second buffer of
// bdx_hip_partials_size() doubles; both sums are reduced in fixed order.
#define BDX_P_PCG_UPDATE_IFACE(T) (const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb, \
  const T* zb, const T* cb, int nty, int ntz, int sy, int sz, double* scal, int rn_slot, int pap_slot, int out_slot, \
  double* partials, const T* dinv, T* z, int rr_slot, double* partials_rr, hipStream_t st)
BDX_TWINS(int, bdx_pcg_update_iface, BDX_P_PCG_UPDATE_IFACE)
// The same on the tiled storage (latd: the tiled descriptor; dinv and z in
// tiled storage too): the kernel selection of bdx_cg_update_tiled_* -- the
// BDX_UPD_PLAIN hook and the 31-bit guard of the prefetching kernel included.
#define BDX_P_PCG_UPDATE_TILED(T) (const int64_t* latd, const int64_t* own, T* r, const T* y, const T* yb, \
  const T* zb, const T* cb, int nty, int ntz, double* scal, int rn_slot, int pap_slot, int out_slot, \
  double* partials, const T* dinv, T* z, int rr_slot, double* partials_rr, hipStream_t st)
BDX_TWINS(int, bdx_pcg_update_tiled, BDX_P_PCG_UPDATE_TILED)
// Tile shape (cells in y, z) used by the fused kernel for a given nq.
int bdx_fused_tile(int nq, int* ty, int* tz);
// y += the tile-interface partials yb / zb / cb (ghost_only: only the nodes
// of the ghost planes).
#define BDX_P_FUSED_FINALIZE(T) (const int64_t* latd, T* y, const T* yb, const T* zb, const T* cb, int nty, int ntz, \
  int sy, int sz, int ghost_only, hipStream_t st)
BDX_TWINS(int, bdx_fused_finalize, BDX_P_FUSED_FINALIZE)
// Packed 1D tables of the v1 / fused2 kernels, written to host memory `out`
// (which the caller uploads; null: only the count).  Returns the count of
// values, -1 for an element without an instance.  No stream.
#define BDX_P_FUSED_TABLES(T) (int nd, int nq, const double* phi0, const double* dphi1, T* out)
BDX_TWINS(int, bdx_fused_tables, BDX_P_FUSED_TABLES)
// The same for the fused3 core (B = phi0 and Dd = dphi1 phi0).
#define BDX_P_FUSED3_TABLES(T) (int nd, int nq, const double* phi0, const double* Dd, T* out)
BDX_TWINS(int, bdx_fused3_tables, BDX_P_FUSED3_TABLES)

// ------------------------------------------ lap_fused*_<suf>_p<P>.hip (per degree)
// v1 fused structured operator, nq in {P+1, P+2}; tabs: host memory,
// kFusedTabMax values (bdx_fused_tables).
#define BDX_P_FUSED_V1_APPLY(T) (int geom, int mode, const int64_t* latd, int nq, const double* phi0, \
  const double* dphi1, const double* wts, const double* qpts, const T* u, const T* pold, T* pnew, T* y, T* yb, \
  T* zb, T* cb, const T* G, const T* xv, const T* tabs, double kappa, const double* scal, double* partials, \
  int beta_num, int beta_den, int nty, int ntz, hipStream_t st)
#define BDX_DECL_FUSED_V1(PP, T, SUF) int bdx_fused_apply_##SUF##_p##PP BDX_P_FUSED_V1_APPLY(T);
BDX_FUSED_DEGREES(BDX_DECL_FUSED_V1, double, f64)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_V1, float, f32)
// The fused2 / fused3 / fused5 operator apply (the one 28-parameter list).
// mode: the word of fused_mode_pack below; rect: host {ty0, ty1, tz0, tz1} restricting the launch to a tile rectangle
// (null: every tile).  tabs: host memory for fused2 / fused3 (bdx_fused_tables,
// bdx_fused3_tables), the operator's device table buffer for fused5.
#define BDX_P_FUSED_APPLY(T) (int mode, int affine_ok, const int64_t* latd, int nq, const double* wts, \
  const double* qpts, const T* u, const T* pold, T* pnew, T* x, T* y, T* yb, T* zb, T* cb, const T* xv, const T* kc, \
  const T* tabs, double kappa, const double* scal, double* partials, int beta_num, int beta_den, int xa_num, \
  int xa_den, int nty, int ntz, const int* rect, hipStream_t st)
#define BDX_DECL_FUSED_APPLY(PP, V, T, SUF) \
  int bdx_fused##V##_apply_##SUF##_p##PP BDX_P_FUSED_APPLY(T);
BDX_FUSED_DEGREES(BDX_DECL_FUSED_APPLY, 2, double, f64)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_APPLY, 2, float, f32)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_APPLY, 3, double, f64)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_APPLY, 3, float, f32)
BDX_FUSED5_DEGREES(BDX_DECL_FUSED_APPLY, 5, double, f64)
BDX_FUSED5_DEGREES(BDX_DECL_FUSED_APPLY, 5, float, f32)
}  // extern "C"
// The mode word of BDX_P_FUSED_APPLY: kind (kFusedAction / kFusedCG, bits 0-3)
// | x mode of the lagged x update (kXSingle / kXSave / kXPair, bits 4-5) | the
// odd tiles' x mode + 1 (bits 6-7; 0, xmode1 = -1: not staggered) | x segments
// (bits 8-15, 0 -> 1) | parity of the saved-alpha slot to write (bit 16) and to
// read (bit 17).  Only fused5 has x modes; Python packs kind and segments
// (models/fused.py, with ops/hip_api.py: CONSTANTS).
enum { kFusedAction = 0, kFusedCG = 1 };
constexpr int kFusedModeSegShift = 8;
constexpr int fused_mode_pack(int kind, int nseg, int xmode = 0, int xmode1 = -1, int xsave_w = 0,
                              int xsave_r = 0) {
  return kind | (xmode << 4) | ((xmode1 + 1) << 6) | (nseg << kFusedModeSegShift) | (xsave_w << 16) |
         (xsave_r << 17);
}
constexpr int fused_mode_kind(int mode) { return mode & 0xf; }
// the kind as a kernel without x modes reads it: a word that carries one is
// no CG launch
constexpr int fused_mode_kind_nox(int mode) { return mode & 0xff; }
constexpr int fused_mode_xmode(int mode) { return (mode >> 4) & 3; }
constexpr int fused_mode_xmode1(int mode) { return ((mode >> 6) & 3) - 1; }
constexpr int fused_mode_nseg(int mode) { return (mode >> kFusedModeSegShift) & 0xff; }
constexpr int fused_mode_xsave_w(int mode) { return (mode >> 16) & 1; }
constexpr int fused_mode_xsave_r(int mode) { return (mode >> 17) & 1; }
extern "C" {
// x segments (fused_choose_segments) of a fused2 / fused3 CG launch of `tiles`
// tiles of ncx cell layers on this device.  Returns the count; no stream.
#define BDX_DECL_FUSED_SEGMENTS(PP, V, SUF) \
  int bdx_fused##V##_segments_##SUF##_p##PP(int affine_ok, int nq, int tiles, int ncx);
BDX_FUSED_DEGREES(BDX_DECL_FUSED_SEGMENTS, 2, f64)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_SEGMENTS, 2, f32)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_SEGMENTS, 3, f64)
BDX_FUSED_DEGREES(BDX_DECL_FUSED_SEGMENTS, 3, f32)
// fused5 per degree: the packed tables (host memory out; returns the count,
// negative when refused), the x segments of a CG launch, and the (y, z) tile
// shape in cells.  No stream.
#define BDX_DECL_FUSED5_AUX(PP, T, SUF)                                                     \
  int bdx_fused5_tables_##SUF##_p##PP(int nd, int nq, const double* phi0, const double* Dd, \
                                      const double* wts, T* out);                           \
  int bdx_fused5_segments_##SUF##_p##PP(int affine_ok, int tiles, int ncx);                 \
  int bdx_fused5_tile_p##PP##_##SUF(int affine_ok, int* ty, int* tz);
BDX_FUSED5_DEGREES(BDX_DECL_FUSED5_AUX, double, f64)
BDX_FUSED5_DEGREES(BDX_DECL_FUSED5_AUX, float, f32)

// ------------------------------------------------------------ lap_v1_<suf>.hip
// mode: 0 stiffness (stored G), 1 stiffness (on-the-fly geometry), 2 mass
#define BDX_P_V1_APPLY(T) (int mode, const int64_t* latd, int nq, const double* phi0, const double* dphi1, \
  const double* wts, const double* qpts, int identity, const T* G, const T* xv, double kappa, const T* kc, \
  const T* u, T* y, const int64_t* lo, const int64_t* hi, hipStream_t st)
BDX_TWINS(int, bdx_v1_apply, BDX_P_V1_APPLY)

// ---------------------------------------------------------- lap_diag_<suf>.hip
// d += diag(A) contributions of the cells [lo, hi) of the local lattice
// (d: lattice layout, zeroed by the caller; Dirichlet dofs are left alone).
// `identity` is taken only to keep the table arguments of bdx_v1_apply; the
// kernel does not use it (phi0 = I runs through the general contraction).
#define BDX_P_DIAG(T) (const int64_t* latd, int nq, const double* phi0, const double* dphi1, const double* wts, \
  const double* qpts, int identity, const T* xv, double kappa, const T* kc, T* d, const int64_t* lo, \
  const int64_t* hi, hipStream_t st)
BDX_TWINS(int, bdx_diag, BDX_P_DIAG)

// -------------------------------------------------------- lap_dofmap_<suf>.hip
// Dofmap operator apply: mode 0 = action (u -> y += A u), 1 = CG operator
// (u = r); returns the number of p.Ap partials written at partials (CG) in
// *nblocks.
#define BDX_P_DOFMAP_APPLY(T) (int P, int nq, int geom, int mode, const T* tab, const int* cells, int ncl, \
  int64_t nvec, const int* cdofs, const int* cverts, const T* coords, const unsigned char* flags, const T* G, \
  double kappa, const T* kc, const T* u, const T* pold, T* pnew, T* x, T* y, const double* scal, int beta_num, \
  int beta_den, int xa_num, int xa_den, double* partials, int* nblocks, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_apply, BDX_P_DOFMAP_APPLY)
// The same, also zeroing yz (the other buffer of the native runtime's y
// ping-pong; null: nothing).  Called from C++ only.
#define BDX_P_DOFMAP_APPLY_YZ(T) (int P, int nq, int geom, int mode, const T* tab, const int* cells, int ncl, \
  int64_t nvec, const int* cdofs, const int* cverts, const T* coords, const unsigned char* flags, const T* G, \
  double kappa, const T* kc, const T* u, const T* pold, T* pnew, T* x, T* y, T* yz, const double* scal, \
  int beta_num, int beta_den, int xa_num, int xa_den, double* partials, int* nblocks, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_apply_yz, BDX_P_DOFMAP_APPLY_YZ)
// Stored geometry factors G of a cell list in the reference layout.
#define BDX_P_DOFMAP_GEOMETRY(T) (int P, int nq, const double* phi0, const double* dphi1, const double* wts, \
  const double* qpts, int ncells, const int* cverts, const T* coords, T* G, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_geometry, BDX_P_DOFMAP_GEOMETRY)
// CG update of the dofmap path: alpha = s[rn_slot] / s[pap_slot]; r -= alpha y
// over every local dof, block partials of r.r over the owned ones (their
// count in *nblocks), y = 0 for the next operator.
#define BDX_P_DOFMAP_CG_UPDATE(T) (int64_t n, const unsigned char* flags, T* r, T* y, const double* scal, \
  int rn_slot, int pap_slot, double* partials, int* nblocks, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_cg_update, BDX_P_DOFMAP_CG_UPDATE)
// The same with the zeroing of y optional (zero_y).  Called from C++ only.
#define BDX_P_DOFMAP_CG_UPDATE_Z(T) (int64_t n, const unsigned char* flags, T* r, T* y, const double* scal, \
  int rn_slot, int pap_slot, double* partials, int* nblocks, int zero_y, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_cg_update_z, BDX_P_DOFMAP_CG_UPDATE_Z)
// x += (s[num] / s[den]) p over every local dof (the lagged x update's flush).
#define BDX_P_DOFMAP_XFLUSH(T) (int64_t n, T* x, const T* p, const double* scal, int num, int den, hipStream_t st)
BDX_TWINS(int, bdx_dofmap_xflush, BDX_P_DOFMAP_XFLUSH)
// Select the FP64 dofmap operator kernel for later launches (tests, A/B):
// 1 = MFMA, 0 = VALU, -1 = back to BDX_DOFMAP_MFMA / the default.
int bdx_dofmap_set_mfma(int mode);
// Which kernel an FP64 dofmap launch of this element takes right now (the
// selection of launch_dofmap): 1 = lap_dofmfma_kernel, 0 = lap_dofmap_kernel.
int bdx_dofmap_uses_mfma(int nd, int nq);
// Writer designation of the dofmap CG (type independent): the first
// occurrence of every dof over the launch order [cells_a..., cells_b...]
// gets the sign bit in cdofs, every other occurrence loses it.  first:
// scratch of ndofs unsigned.
int bdx_dofmap_mark_writers(const int* cells_a, int na, const int* cells_b, int nb, int* cdofs,
                            int nd3, unsigned* first, int64_t ndofs, hipStream_t st);
// p.Ap partials (blocks) of a CG launch over ncl cells at this rule (the
// native runtime places the boundary launch's partials after the interior's);
// -1 for a rule without an instance.  No stream.
int bdx_dofmap_nblocks(int nq, int ncl);

// ---------------------------------- lap_transfer_<suf>.hip, lap_htransfer_<suf>.hip
// p-multigrid transfers: vf = P vc (every local fine node, ghost planes
// included, written once) and vc += P^T vf (owned fine nodes; vc zeroed by
// the caller).  latc / latf: the coarse and fine lattice descriptors, J: the
// (Pf + 1) x (Pc + 1) 1D table.
#define BDX_P_PROLONG(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vc, T* vf, \
  hipStream_t st)
BDX_TWINS(int, bdx_prolong, BDX_P_PROLONG)
// (see bdx_prolong)
#define BDX_P_RESTRICT(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vf, T* vc, \
  hipStream_t st)
BDX_TWINS(int, bdx_restrict, BDX_P_RESTRICT)
// h-multigrid transfers: vf (+)= P vc and vc = P^T (vf - y) between the coarse
// and fine degree-1 lattices latc / latf; cidx, cw, fpos: the device tables of
// lap_htransfer.h.  hipErrorInvalidValue for tiled descriptors, a degree other
// than 1, differing ghost flags, L != n + 1, more coarse than fine cells on an
// axis or ld < L[2].
#define BDX_P_HPROLONG(T) (const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw, const int* fpos, \
  const T* vc, T* vf, int add, hipStream_t st)
BDX_TWINS(int, bdx_hprolong, BDX_P_HPROLONG)
// (see bdx_hprolong)
#define BDX_P_HRESTRICT(T) (const int64_t* latc, const int64_t* latf, const int* cidx, const T* cw, const int* fpos, \
  const T* vf, const T* y, T* vc, hipStream_t st)
BDX_TWINS(int, bdx_hrestrict, BDX_P_HRESTRICT)

// ------------------------------------------------- lap_rowtransfer_<suf>.hip
// p-multigrid transfers by lattice rows, with the h-transfers' modes: vf = P vc
// on every local fine node (add = 0) or vf += P vc on the owned ones (add = 1),
// and vc = P^T (vf - y) (y may be null: P^T vf) over the owned fine nodes,
// every local coarse node written by one launch.  latc, latf, J: as for
// bdx_prolong.  hipErrorInvalidValue for a pair bdx_prolong refuses or a null
// pointer, before anything is launched.
#define BDX_P_PROLONG_ROW(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vc, T* vf, \
  int add, hipStream_t st)
BDX_TWINS(int, bdx_prolong_row, BDX_P_PROLONG_ROW)
// (see bdx_prolong_row)
#define BDX_P_RESTRICT_ROW(T) (const int64_t* latc, const int64_t* latf, const double* J, const T* vf, const T* y, \
  T* vc, hipStream_t st)
BDX_TWINS(int, bdx_restrict_row, BDX_P_RESTRICT_ROW)

// --------------------------------------------------- lap_stencil27_<suf>.hip
// The assembled 27-point operator S[27][size] of the degree-1 lattice latd
// (ops/kernels.py: stencil27), streamed: y = S u on every local row, ghost rows
// included (u forward-exchanged by the caller).  hipErrorInvalidValue, before
// anything is launched, for a degree other than 1, a tiled descriptor, extents
// beyond int, a null pointer or y == u.
#define BDX_P_STENCIL27_APPLY(T) (const int64_t* latd, const T* S, const T* u, T* y, hipStream_t st)
BDX_TWINS(int, bdx_stencil27_apply, BDX_P_STENCIL27_APPLY)
// One Chebyshev step in one launch over the own[0] x own[1] x own[2] owned
// nodes: d = a d + b dinv (r - S z_in); z_out = z_in + d, bit for bit
// bdx_stencil27_apply into a scratch vector followed by bdx_cheb_step.  Refused
// like bdx_stencil27_apply, and for z_out == z_in.
#define BDX_P_STENCIL27_CHEB(T) (const int64_t* latd, const int64_t* own, const T* S, const T* dinv, const T* r, \
  const T* z_in, T* d, T* z_out, double a, double b, hipStream_t st)
BDX_TWINS(int, bdx_stencil27_cheb, BDX_P_STENCIL27_CHEB)

// ------------------------------------------ lap_stencil27_assemble_<suf>.hip
// That stencil assembled on the device: all of S[27][size] written, nothing
// zeroed by the caller, from the vertices xv, kappa (kc: per cell, or null)
// and the tables of bdx_diag (Dd = dphi1 phi0, nq 2 or 3); the rows are those
// of ops/kernels.py: stencil27 on the rank's assembled matrix, a ghost-plane
// row holding the rank's partial sums.  hipErrorInvalidValue, before anything
// is launched, for a descriptor bdx_stencil27_apply refuses, another nq or a
// null latd, table, xv or S.
#define BDX_P_STENCIL27_ASSEMBLE(T) (const int64_t* latd, int nq, const double* phi0, const double* dphi1, \
  const double* wts, const double* qpts, const T* xv, double kappa, const T* kc, T* S, hipStream_t st)
BDX_TWINS(int, bdx_stencil27_assemble, BDX_P_STENCIL27_ASSEMBLE)

// --------------------------------------------------------- pmg_tail_<suf>.hip
// z = the V-cycle from the first level of the table down and back up, applied
// to r (the table's other vectors are work space); htab / dtab: the host and
// device copies of the level table, nwords long.
#define BDX_P_PMG_TAIL(T) (const int64_t* htab, const int64_t* dtab, int nlev, int64_t nwords, const T* r, T* z, \
  hipStream_t st)
BDX_TWINS(int, bdx_pmg_tail, BDX_P_PMG_TAIL)

// ------------------------------------------------------------------ misc.hip
// Stored geometry factors G of every local cell (xv: the vertex coordinates).
#define BDX_P_GEOMETRY(T) (const int64_t* latd, int nq, const double* phi0, const double* dphi1, const double* wts, \
  const double* qpts, const T* xv, T* G, hipStream_t st)
BDX_TWINS(int, bdx_geometry, BDX_P_GEOMETRY)
// CSR y = A x (acc: y += A x), row r holding the entries [beg[r], end[r]).
#define BDX_P_SPMV(T) (int64_t nrows, const int64_t* beg, const int64_t* end, const int32_t* cols, const T* vals, \
  const T* x, T* y, int acc, hipStream_t st)
BDX_TWINS(int, bdx_spmv, BDX_P_SPMV)
// 1 when the library was built with the device bounds checks (BDX_DEBUG):
// correct numerics, but not a valid timing build.
int bdx_build_debug();
// Device banner (reference get_device_information, src/util.cpp:10-52).
int bdx_device_info(int dev, char* buf, int buflen);

// ----------------------------------------------------------------- mixed.hip
// out = (float)a over the owned rows (round to nearest even).
int bdx_demote_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                       const double* a, float* out, hipStream_t st);
// out = (double)a over the owned rows (exact).
int bdx_promote_f32_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                        const float* a, double* out, hipStream_t st);
// bdx_cg_update_f64 (alpha = s[rn] / s[pap]; x += alpha p; r -= alpha y; r.r
// into s[out_slot]) with r32 = (float)r stored in the same pass.
int bdx_cg_update_demote_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                             double* x, double* r, const double* p, const double* y,
                             double* scal, int rn_slot, int pap_slot, int out_slot,
                             double* partials, float* r32, hipStream_t st);
// out[slot] = sum over the owned rows of a (double)b32: the block partition
// and final pass of bdx_dot_f64.
int bdx_dot_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, const double* a,
                    const float* b32, double* partials, double* out, int slot, hipStream_t st);
// p = (s[num] / s[den]) p + (double)z32 over the owned rows.
int bdx_p_update_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, double* p,
                         const float* z32, const double* scal, int num, int den, hipStream_t st);

// --------------------------------------------------------------- runtime.hip
// A fresh ncclUniqueId into out128 (128 bytes); returns its size, -1 on error.
int bdx_rt_nccl_unique_id(void* out128);
// Hardware self-test of the RCCL transport on one GPU; buf: 3 n + 2 doubles.
int bdx_rt_rccl_selftest(double* buf, int n, hipStream_t st);
// The fused structured CG loop; returns the runtime handle h of the calls
// below (null when refused).  The records: bdx_rt_setup.h.
void* bdx_rt_create(const BdxRtFusedSetup* setup, hipStream_t st);
// The dofmap data model's CG loop (handle as above).
void* bdx_rt_create_dofmap(const BdxRtDofmapSetup* setup, hipStream_t st);
// Priority of the comm stream and the device's range.
int bdx_rt_comm_priority(void* h, BdxRtCommPriority* out);
// Transport pre-flight.
int bdx_rt_preflight(void* h, double timeout_s, BdxRtPreflight* out);
// Comm/compute overlap probe on one GPU (fused operators only); buf: 2 n
// doubles.
int bdx_rt_overlap_probe(void* h, int64_t n, double* buf, int reps, BdxRtOverlapProbe* out);
// 1 if the loop runs on the tiled storage layout.
int bdx_rt_tiled(void* h);
// Open the runtime's RCCL communicator (collective over the ranks).  0 on
// success (or when the transport is not RCCL).
int bdx_rt_connect(void* h, const void* uid, int rank);
// Ranks of the transport (ncclCommCount for RCCL; -1 if not connected).
int bdx_rt_comm_count(void* h);
// 1 if the overlapped (split, two-stream) schedule is active.
int bdx_rt_overlap(void* h);
// Reset the CG state after a new prologue (p_a zeroed by the caller).
int bdx_rt_reset(void* h);
// Bind a new iterate buffer x; drops the captured graphs.
int bdx_rt_bind_x(void* h, void* x);
// Bind (dinv != null) or clear the Jacobi preconditioner of a fused runtime.
int bdx_rt_set_precond(void* h, const void* dinv, void* z, void* dinv_tiled, void* z_tiled,
                       double* partials_rr, int rr_slot);
// Queue n CG iterations (asynchronous; see bdx_rt_wait).
int bdx_rt_iterate(void* h, long n);
// iterate() plus the device time of each of the n steps: step_ms[n].
int bdx_rt_iterate_timed(void* h, long n, float* step_ms);
// Host wait for everything iterate() queued, bounded by the RCCL deadline.
int bdx_rt_wait(void* h);
// n eager CG iterations with hipEvent phase timers; out: mean ms per phase.
int bdx_rt_profile(void* h, long n, BdxRtPhases* out);
// it (iterations done) and whether steady-state graphs are in use.
int bdx_rt_state(void* h, long* it, int* graphs);
// Destroy a runtime handle.
void bdx_rt_destroy(void* h);
// Forget the shared state of a thread-transport group (tests).
void bdx_rt_release_group(int64_t group_id);

}  // extern "C"
