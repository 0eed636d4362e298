// Fused structured operator kernel, v2 ("fused2"): the same x-march /
// (y, z)-tile / atomic-free design as lap_fused.h (and the same operator as
// the reference's stiffness_operator_gpu + geometry_computation_gpu,
// src/laplacian_gpu.hpp:91-426, src/geometry_gpu.hpp:26-132), re-engineered
// for instruction economy after rocprofv3 showed v1 spending ~45 % of its
// VALU issue on index arithmetic and SGPR spill traffic:
//
// * All per-element addressing is precomputed once per thread before the
//   march: the input-staging elements, the output elements (their <= 4 LDS
//   sources in the element-vector scratch, the destination class and a
//   32-bit offset), and the vertex elements.  Per layer only 64-bit uniform
//   base pointers advance (SGPRs), so the march body carries no 64-bit index
//   math and no lattice struct.
// * Dirichlet tests are per-thread bits for y/z (layer invariant) plus one
//   compare against the local index of the global x boundary plane.
// * 1/det uses the hardware reciprocal + two Newton steps.
// * OTF geometry only (the stored-G layout stays on v1).
//
// Interface partials (YB/ZB/CB) and the finalize pass are those of v1.
#pragma once
#include <algorithm>
#include "lap_fused.h"

// The LDS-fed contraction loops stay rolled (BDX_PRAGMA_UNROLL(1)): keeps the
// register budget of 3 waves/SIMD.
#define BDX_PRAGMA(x) _Pragma(#x)
#define BDX_PRAGMA_UNROLL(n) BDX_PRAGMA(unroll n)

template <typename T>
struct Fused2Args {
  const T* __restrict__ u;     // action: input; CG: r
  const T* __restrict__ pold;  // CG: previous p
  T* __restrict__ pnew;        // CG: new p (tile-owned dofs)
  T* __restrict__ x;           // CG: iterate, lagged update x += alpha_prev p_old
  T* __restrict__ y;
  T* __restrict__ yb;
  T* __restrict__ zb;
  T* __restrict__ cb;
  const T* __restrict__ xv;
  const T* __restrict__ kc;    // per-cell coefficient [n0][n1][n2] or null (constant kappa)
  const double* __restrict__ scal;
  double* __restrict__ partials;
  int64_t ps;      // x-plane stride of the vectors (Ly * ld)
  int64_t ybps;    // x-plane strides of the interface buffers
  int64_t zbps;
  int64_t cbps;
  int64_t vps;     // x-plane stride of the vertex array ((n1+1)(n2+1)*3)
  int ncx, n1, n2;
  int Ly, Lz, ld;
  int ownx, owny, ownz;          // rank-owned extents (L - gh)
  int bcx_lo, bcx_hi;            // local index of the global boundary plane, -1 if none
  int bcy_lo, bcy_hi, bcz_lo, bcz_hi;
  int nty, ntz;
  int ty0, tz0, rwz, rtiles;     // tile rectangle of this launch: [ty0, ty0 + rtiles / rwz) x [tz0, tz0 + rwz)
  int nseg, seglen;              // x segments per tile (work item = (tile, segment)), cells per segment
  int nblk;                      // workgroups of the launch = rtiles * nseg
  int beta_num, beta_den;        // CG: beta = scal[num] / scal[den]; num < 0 -> 0
  int xa_num, xa_den;            // CG: alpha_prev = scal[num] / scal[den]; num < 0 -> no x update
  // fused5 CG: paired lagged x update (kXSave, kXPair; 0 = one term per
  // iteration).  kXSave: no x update, alpha_prev is stored to
  // scal[xslot_w]; kXPair: x += alpha_prev p_old + scal[xslot_r] p_prev2,
  // p_prev2 being read from pnew before it is overwritten (runtime.hip).
  // xmode1 >= 0: the x mode of the odd tiles ((ty + tz) odd) of a staggered
  // pairing, in which the two tile colours pair on alternate iterations.
  int xmode, xmode1, xslot_w, xslot_r;
  T kappa;
  // tiled vector storage (bdx_lattice.h; tsy = 0: lattice layout): the
  // x-plane stride ps is then tsy * tsz and a node's (y, z) offset is its
  // tile's column base plus the in-tile position (fused5 only)
  int tsy, tsz, tntz;
  int64_t tcol;
  int64_t vsize;   // elements of one vector (BDX_DEBUG bounds checks)
  int64_t ibsize;  // elements of the interface buffers yb / zb / cb (max of the three)
};

// (y, z) part of a vector offset (the x-plane part is x * ps)
template <typename T>
__host__ __device__ __forceinline__ int64_t fused_yzoff(const Fused2Args<T>& A, int gy, int gz) {
  if (A.tsy)
    return (static_cast<int64_t>(gy / A.tsy) * A.tntz + gz / A.tsz) * A.tcol +
           (gy % A.tsy) * A.tsz + gz % A.tsz;
  return static_cast<int64_t>(gy) * A.ld + gz;
}

// fused2: x-march over (y, z) tiles with general (trilinear) or affine geometry.
template <typename T, int ND, int NQ, int TY, int TZ, int MODE, int AFF>
__global__ void __launch_bounds__((FusedShape<T, ND, NQ, TY, TZ>::threads), FusedWaves<NQ>::value)
    lap_fused2_kernel(Fused2Args<T> A, FusedTables<T> tb) {
  using S = FusedShape<T, ND, NQ, TY, TZ>;
  constexpr int P = S::P, DY = S::DY, DZ = S::DZ, PL = DY * DZ;
  constexpr int DZP = S::DZP, PLP = DY * DZP;
  constexpr int NQ2 = NQ * NQ;
  constexpr bool IDENT = (ND == NQ);
  constexpr int NT = S::threads;
  constexpr int NPF = (P * PL + NT - 1) / NT;     // staged input dofs per thread and layer
  constexpr int NOUT = (ND * PL + NT - 1) / NT;   // output dofs per thread and layer
  constexpr int NCP = (PL + NT - 1) / NT;         // carried-plane copies per thread
  constexpr int NV = (TY + 1) * (TZ + 1) * 3;
  constexpr int NPV = (NV + NT - 1) / NT;
  constexpr int XP = S::XP, NP = S::NP;
  constexpr int ZSLOT = S::work;                  // a zero row at the end of s_w2
  static_assert(S::work + XP < 32768, "16-bit LDS source offsets");
  static_assert(PL < 256, "8-bit plane index");

  __shared__ __attribute__((aligned(16))) T s_tab[S::TAB];
  __shared__ T s_qw[2 * NQ];
  __shared__ T s_u[2][ND * PLP];
  __shared__ T s_c[2][PL];
  __shared__ __attribute__((aligned(16))) T s_w1[S::work];
  __shared__ __attribute__((aligned(16))) T s_w2[S::work + XP];
  __shared__ __attribute__((aligned(16))) T s_w3[S::work];
  __shared__ T s_X[2][2 * NV];
  __shared__ double s_red[16];

  const int tid = threadIdx.x;
  for (int i = tid; i < S::TAB; i += NT) s_tab[i] = tb.tab[i];
  if (tid < NQ) {
    s_qw[tid] = tb.qpts[tid];
    s_qw[NQ + tid] = tb.wts[tid];
  }
  if (tid < XP) s_w2[ZSLOT + tid] = T(0);

  // XCD-aware bijective remap of the block id (cdna_hip_programming.md T1).
  const int nblk = gridDim.x, ob = blockIdx.x;
  const int q8 = nblk / 8, r8 = nblk % 8, xcd = ob % 8;
  const int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + ob / 8;
  // work item = (tile of the launch rectangle, x segment); see fused_set_segments
  const int tix = bid % A.rtiles, seg = bid / A.rtiles;
  const int ty = A.ty0 + tix / A.rwz, tz = A.tz0 + tix % A.rwz;
  // own cell layers [sa, cend); the march starts one layer early (redundant)
  // in every segment but the first
  const int sa = seg * A.seglen;
  const int cend = (sa + A.seglen < A.ncx) ? sa + A.seglen : A.ncx;
  const int cbeg = sa > 0 ? sa - 1 : 0;
  const int y0 = ty * TY * P, z0 = tz * TZ * P;
  const int Ly = A.Ly, Lz = A.Lz, ld = A.ld;
  const int ncx = A.ncx;
  const bool top_y = (ty == A.nty - 1), top_z = (tz == A.ntz - 1);
  const int ey = (y0 + DY <= Ly) ? DY : Ly - y0;
  const int ez = (z0 + DZ <= Lz) ? DZ : Lz - z0;
  const int oy = top_y ? ey : TY * P;
  const int oz = top_z ? ez : TZ * P;

  const int c = (tid / NQ2 < S::cells) ? tid / NQ2 : S::cells - 1;
  const int a = (tid / NQ) % NQ, b = tid % NQ;
  const int cy = c / TZ, cz = c % TZ;
  const bool lane_on = tid < S::lanes;
  const bool cell_on = lane_on && (ty * TY + cy < A.n1) && (tz * TZ + cz < A.n2);
  const int ycell = cy * P, zcell = cz * P;
  T* w1c = s_w1 + c * NQ2 * XP;
  T* w2c = s_w2 + c * NQ2 * XP;
  T* w3c = s_w3 + c * NQ2 * XP;

  T beta = T(0), xalpha = T(0);
  const bool xupd = MODE == kFusedCG && A.xa_num >= 0;
  if constexpr (MODE == kFusedCG) {
    if (A.beta_num >= 0) beta = static_cast<T>(A.scal[A.beta_num] / A.scal[A.beta_den]);
    if (xupd) xalpha = static_cast<T>(A.scal[A.xa_num] / A.scal[A.xa_den]);
  }
  double pap = 0.0;

  // y/z classification of a slab position (layer invariant)
  enum { kValid = 1, kOwnT = 2, kBcYZ = 4, kRownYZ = 8 };
  auto yz_flags = [&](int ly, int lz) -> int {
    if (ly >= ey || lz >= ez) return 0;
    const int gy = y0 + ly, gz = z0 + lz;
    int f = kValid;
    if (ly < oy && lz < oz) f |= kOwnT;
    if (gy == A.bcy_lo || gy == A.bcy_hi || gz == A.bcz_lo || gz == A.bcz_hi) f |= kBcYZ;
    if (gy < A.owny && gz < A.ownz) f |= kRownYZ;
    return f;
  };
  // Input value of a staged dof + its CG / Dirichlet side effects.
  // (wr = false: a redundant layer, whose planes the previous segment owns:
  // the value only, no side effects)
  auto stage = [&](int f, int gx, const T* __restrict__ ul, T* __restrict__ pn, T* __restrict__ yl,
                   int goff, bool wr) -> T {
    T v;
    if (!wr) f &= ~kOwnT;
    if constexpr (MODE == kFusedCG) {
      const T po = A.pold[(ul - A.u) + goff];
      v = ul[goff] + beta * po;
      if (xupd && (f & kOwnT)) {
        T* __restrict__ xl = A.x + (ul - A.u);
        xl[goff] += xalpha * po;
      }
    } else {
      v = ul[goff];
    }
    (void)pn;
    if constexpr (MODE == kFusedCG) {
      if (f & kOwnT) pn[goff] = v;
    }
    if ((f & kBcYZ) || gx == A.bcx_lo || gx == A.bcx_hi) {
      if (f & kOwnT) {
        const bool rown = (f & kRownYZ) && gx < A.ownx;
        yl[goff] = rown ? v : T(0);
        if constexpr (MODE == kFusedCG) {
          if (rown) pap += static_cast<double>(v) * static_cast<double>(v);
        }
      }
      v = T(0);
    }
    return v;
  };

  // ---- per-thread staging descriptors (planes 1..P of a layer)
  int st_goff[NPF], st_meta[NPF];
#pragma unroll
  for (int k = 0; k < NPF; ++k) {
    const int e = tid + k * NT;
    st_goff[k] = 0;
    st_meta[k] = 0;
    if (e < P * PL) {
      const int pl = 1 + e / PL, rem = e % PL, ly = rem / DZ, lz = rem % DZ;
      const int f = yz_flags(ly, lz);
      st_goff[k] = (pl * Ly + y0 + ly) * ld + z0 + lz;
      st_meta[k] = f | (pl << 4) | ((pl * PLP + ly * DZP + lz) << 8);
    }
  }
  // ---- per-thread output descriptors (planes 0..P of a layer)
  int o_src[NOUT][2], o_off[NOUT], o_meta[NOUT];
#pragma unroll
  for (int k = 0; k < NOUT; ++k) {
    const int e = tid + k * NT;
    o_src[k][0] = o_src[k][1] = ZSLOT | (ZSLOT << 16);
    o_off[k] = 0;
    o_meta[k] = 0;
    if (e < ND * PL) {
      const int pl = e / PL, rem = e % PL, ly = rem / DZ, lz = rem % DZ;
      const int f = yz_flags(ly, lz);
      if (f & kValid) {
        const int cyh = (ly / P < TY - 1) ? ly / P : TY - 1;
        const int cyl = (ly % P == 0 && ly > 0 && ly / P - 1 < cyh) ? ly / P - 1 : cyh;
        const int czh = (lz / P < TZ - 1) ? lz / P : TZ - 1;
        const int czl = (lz % P == 0 && lz > 0 && lz / P - 1 < czh) ? lz / P - 1 : czh;
        int src[4] = {ZSLOT, ZSLOT, ZSLOT, ZSLOT};
        int ns = 0;
        for (int ccy = cyl; ccy <= cyh; ++ccy)
          for (int ccz = czl; ccz <= czh; ++ccz)
            src[ns++] = (((ccy * TZ + ccz) * NQ + (ly - ccy * P)) * NQ + (lz - ccz * P)) * XP + pl;
        o_src[k][0] = src[0] | (src[1] << 16);
        o_src[k][1] = src[2] | (src[3] << 16);
        const int gy = y0 + ly, gz = z0 + lz;
        const bool iy = ly < oy, iz = lz < oz;
        int kind, off;
        if (iy && iz) {
          kind = 0;
          off = (pl * Ly + gy) * ld + gz;
        } else if (!iy && iz) {
          kind = 1;
          off = static_cast<int>(pl * A.ybps) + ty * Lz + gz;
        } else if (iy && !iz) {
          kind = 2;
          off = static_cast<int>(pl * A.zbps) + tz * Ly + gy;
        } else {
          kind = 3;
          off = static_cast<int>(pl * A.cbps) + ty * (A.ntz - 1) + tz;
        }
        o_off[k] = off;
        o_meta[k] = f | (kind << 4) | (pl << 8) | (rem << 12);
      }
    }
  }
  // ---- carried-plane copy descriptors (plane P of a slab -> plane 0 of the next)
  int cp_lds[NCP];
#pragma unroll
  for (int k = 0; k < NCP; ++k) {
    const int e = tid + k * NT;
    cp_lds[k] = (e < PL) ? (e / DZ) * DZP + e % DZ : -1;
  }
  // ---- vertex descriptors
  int v_off[NPV];
#pragma unroll
  for (int k = 0; k < NPV; ++k) {
    const int e = tid + k * NT;
    v_off[k] = -1;
    if (e < NV) {
      const int d = e % 3, r = e / 3;
      const int vz = r % (TZ + 1), vy = r / (TZ + 1);
      const int gy = ty * TY + vy, gz = tz * TZ + vz;
      if (gy <= A.n1 && gz <= A.n2) v_off[k] = (gy * (A.n2 + 1) + gz) * 3 + d;
    }
  }

  // ---- prologue: layer cbeg (planes 0..P), vertex planes cbeg/cbeg+1, zero carry
  {
    const int64_t l0 = static_cast<int64_t>(cbeg) * P * A.ps;
    const bool wr = cbeg == sa;  // not a redundant layer
    for (int e = tid; e < ND * PL; e += NT) {
      const int pl = e / PL, rem = e % PL, ly = rem / DZ, lz = rem % DZ;
      const int f = yz_flags(ly, lz);
      T v = T(0);
      if (f & kValid)
        v = stage(f, cbeg * P + pl, A.u + l0, A.pnew + l0, A.y + l0,
                  (pl * Ly + y0 + ly) * ld + z0 + lz, wr);
      s_u[0][pl * PLP + ly * DZP + lz] = v;
    }
  }
  for (int e = tid; e < 2 * NV; e += NT) {
    const int k = e % NV;
    int off = -1;
    {
      const int d = k % 3, r = k / 3;
      const int vz = r % (TZ + 1), vy = r / (TZ + 1);
      const int gy = ty * TY + vy, gz = tz * TZ + vz;
      if (gy <= A.n1 && gz <= A.n2) off = (gy * (A.n2 + 1) + gz) * 3 + d;
    }
    s_X[0][e] = off >= 0 ? A.xv[static_cast<int64_t>(cbeg + e / NV) * A.vps + off] : T(0);
  }
  for (int e = tid; e < PL; e += NT) s_c[0][e] = T(0);

  T Js[3] = {0, 0, 0};                        // AFF = 0 only
  T Jt0[3] = {0, 0, 0}, Jt1[3] = {0, 0, 0};
  T Ju0[3] = {0, 0, 0}, Ju1[3] = {0, 0, 0};
  // AFF = 2 only (x-trilinear cells, see lap_fused3.h): 1/x_s, 1/hy, 1/hz,
  // x_t/hy = bt0 + s bt1, x_u/hz = cu0 + s cu1, kappa w_t w_u det J / w_s
  T xia = 0, xihy = 0, xihz = 0, xbt0 = 0, xbt1 = 0, xcu0 = 0, xcu1 = 0, xcs = 0;

  for (int cx = cbeg; cx < cend; ++cx) {
    const int cur = (cx - cbeg) & 1, nxt = cur ^ 1;
    const bool last = (cx == cend - 1);   // end of this segment
    const bool glast = (cx == ncx - 1);   // end of the march
    const bool red = (cx < sa);           // redundant layer: carry only
    __syncthreads();

    // ---- prefetch the next layer (planes 1..P of layer cx+1, vertex plane cx+2)
    const int64_t lnext = static_cast<int64_t>(cx + 1) * P * A.ps;
    T pf_r[NPF], pf_p[NPF], pf_x[NPF];
    T pf_v[NPV];
#pragma unroll
    for (int k = 0; k < NPF; ++k) {
      pf_r[k] = T(0);
      pf_p[k] = T(0);
      pf_x[k] = T(0);
      if (!last && (st_meta[k] & kValid)) {
        pf_r[k] = A.u[lnext + st_goff[k]];
        if constexpr (MODE == kFusedCG) {
          pf_p[k] = A.pold[lnext + st_goff[k]];
          if (xupd && (st_meta[k] & kOwnT)) pf_x[k] = A.x[lnext + st_goff[k]];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NPV; ++k) {
      pf_v[k] = T(0);
      if (!last && v_off[k] >= 0) pf_v[k] = A.xv[static_cast<int64_t>(cx + 2) * A.vps + v_off[k]];
    }

    int toff = 0;
    asm volatile("" : "+s"(toff));
    const T* __restrict__ gt = tb.tab + toff;
    const T* __restrict__ su = s_u[cur];
    const T* __restrict__ sX = s_X[cur];

    const T* __restrict__ ua = su + (ycell + a) * DZP + zcell;
    T* __restrict__ w1ab = w1c + (a * NQ + b) * XP;
    T* __restrict__ w2ab = w2c + (a * NQ + b) * XP;
    T* __restrict__ w3ab = w3c + (a * NQ + b) * XP;
    const T* __restrict__ w1b = w1c + b * XP;
    const T* __restrict__ w2b = w2c + b * XP;
    const T* __restrict__ w1a = w1c + a * NQ * XP;
    const T* __restrict__ w2a = w2c + a * NQ * XP;
    const T* __restrict__ w3a = w3c + a * NQ * XP;

    // ------------------------------------------------ interpolate to qpts
    T U[NQ];
    if constexpr (IDENT) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) U[i] = lane_on ? ua[i * PLP + b] : T(0);
    } else {
      if (lane_on && a < ND) {
        const T* __restrict__ ph = s_tab + S::OFF_PR + b * NP;
        T o[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) o[i] = 0;
BDX_PRAGMA_UNROLL(1)
        for (int k = 0; k < ND; ++k) {
          const T cc = ph[k];
#pragma unroll
          for (int i = 0; i < ND; ++i) o[i] += cc * ua[i * PLP + k];
        }
        strow<ND>(w1ab, o);
      }
      __syncthreads();
      const T* __restrict__ pa = s_tab + S::OFF_PR + a * NP;
      T t2[ND];
#pragma unroll
      for (int i = 0; i < ND; ++i) t2[i] = 0;
BDX_PRAGMA_UNROLL(1)
      for (int j = 0; j < ND; ++j) {
        T row[ND];
        ldrow<ND>(w1b + j * NQ * XP, row);
        const T cc = pa[j];
#pragma unroll
        for (int i = 0; i < ND; ++i) t2[i] += cc * row[i];
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) U[q] = 0;
#pragma unroll
      for (int i = 0; i < ND; ++i) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) U[q] += gt[S::OFF_PC + i * XP + q] * t2[i];
      }
    }

    // ------------------------------------------------ reference gradient
    if (lane_on) strow<NQ>(w2ab, U);
    __syncthreads();
    T gx[NQ], gy[NQ], gz[NQ];
    {
      const T* __restrict__ dra = s_tab + S::OFF_DR + a * XP;
      const T* __restrict__ drb = s_tab + S::OFF_DR + b * XP;
#pragma unroll
      for (int q = 0; q < NQ; ++q) gx[q] = gy[q] = gz[q] = T(0);
BDX_PRAGMA_UNROLL(1)
      for (int m = 0; m < NQ; ++m) {
        T ry[NQ], rz[NQ];
        ldrow<NQ>(w2b + m * NQ * XP, ry);
        ldrow<NQ>(w2a + m * XP, rz);
        const T um = w2ab[m], cy_ = dra[m], cz_ = drb[m];
        const T* __restrict__ dc = gt + S::OFF_DC + m * XP;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          gx[q] += dc[q] * um;
          gy[q] += cy_ * ry[q];
          gz[q] += cz_ * rz[q];
        }
      }
    }

    // ------------------------------------------------ geometry coefficients
    // AFF = 0: general trilinear map, dX/ds = Js (constant along the thread's
    // x column), dX/dt = Jt0 + s Jt1, dX/du = Ju0 + s Ju1, G formed per point.
    // AFF = 1: every cell of the launch is a parallelepiped (host-verified by
    // bitwise edge equality, models/fused.py), so J is constant per cell and
    // G = kappa w_a w_b adj(J) adj(J)^T / det J is formed once per thread and
    // layer; per point only the weight w_q remains (same operator, same maths).
    T Gc[6] = {0, 0, 0, 0, 0, 0};
    const T kcell = A.kc ? (cell_on ? A.kc[(static_cast<int64_t>(cx) * A.n1 + ty * TY + cy) * A.n2 +
                                          tz * TZ + cz]
                                    : T(0))
                         : A.kappa;
    const T kwyz = kcell * s_qw[NQ + a] * s_qw[NQ + b];
    {
      const T* X0 = sX;
      const T* X1 = sX + NV;
      const int v00 = (cy * (TZ + 1) + cz) * 3, v01 = v00 + 3;
      const int v10 = v00 + (TZ + 1) * 3;
      if constexpr (AFF == 1) {
        T E[3], F[3], G[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const T X000 = X0[v00 + d];
          E[d] = X1[v00 + d] - X000;
          F[d] = X0[v10 + d] - X000;
          G[d] = X0[v01 + d] - X000;
        }
        const T J00 = E[0], J10 = E[1], J20 = E[2];
        const T J01 = F[0], J11 = F[1], J21 = F[2];
        const T J02 = G[0], J12 = G[1], J22 = G[2];
        const T K00 = J11 * J22 - J12 * J21, K01 = J02 * J21 - J01 * J22, K02 = J01 * J12 - J02 * J11;
        const T K10 = J12 * J20 - J10 * J22, K11 = J00 * J22 - J02 * J20, K12 = J02 * J10 - J00 * J12;
        const T K20 = J10 * J21 - J11 * J20, K21 = J01 * J20 - J00 * J21, K22 = J00 * J11 - J01 * J10;
        const T det = J00 * K00 + J01 * K10 + J02 * K20;
        const T sc = kwyz * fast_rcp(det);
        Gc[0] = sc * (K00 * K00 + K01 * K01 + K02 * K02);
        Gc[1] = sc * (K00 * K10 + K01 * K11 + K02 * K12);
        Gc[2] = sc * (K00 * K20 + K01 * K21 + K02 * K22);
        Gc[3] = sc * (K10 * K10 + K11 * K11 + K12 * K12);
        Gc[4] = sc * (K10 * K20 + K11 * K21 + K12 * K22);
        Gc[5] = sc * (K20 * K20 + K21 * K21 + K22 * K22);
      } else if constexpr (AFF == 2) {
        // x-trilinear cells (y/z on the lattice; lap_fused3.h AFF = 2)
        const T t = s_qw[a], uu = s_qw[b];
        const int v11 = v10 + 3;
        const T X000 = X0[v00], X001 = X0[v01], X010 = X0[v10], X011 = X0[v11];
        const T X100 = X1[v00], X101 = X1[v01], X110 = X1[v10], X111 = X1[v11];
        const T xs = (1 - t) * ((1 - uu) * (X100 - X000) + uu * (X101 - X001)) +
                     t * ((1 - uu) * (X110 - X010) + uu * (X111 - X011));
        const T xt0 = (1 - uu) * (X010 - X000) + uu * (X011 - X001);
        const T xt1 = (1 - uu) * (X110 - X100) + uu * (X111 - X101) - xt0;
        const T xu0 = (1 - t) * (X001 - X000) + t * (X011 - X010);
        const T xu1 = (1 - t) * (X101 - X100) + t * (X111 - X110) - xu0;
        const T hy = X0[v10 + 1] - X0[v00 + 1], hz = X0[v01 + 2] - X0[v00 + 2];
        xia = fast_rcp(xs);
        xihy = fast_rcp(hy);
        xihz = fast_rcp(hz);
        xbt0 = xt0 * xihy;
        xbt1 = xt1 * xihy;
        xcu0 = xu0 * xihz;
        xcu1 = xu1 * xihz;
        xcs = kwyz * xs * hy * hz;
      } else {
        const T t = s_qw[a], uu = s_qw[b];
        const int v11 = v10 + 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const T X000 = X0[v00 + d], X001 = X0[v01 + d], X010 = X0[v10 + d], X011 = X0[v11 + d];
          const T X100 = X1[v00 + d], X101 = X1[v01 + d], X110 = X1[v10 + d], X111 = X1[v11 + d];
          Js[d] = (1 - t) * ((1 - uu) * (X100 - X000) + uu * (X101 - X001)) +
                  t * ((1 - uu) * (X110 - X010) + uu * (X111 - X011));
          Jt0[d] = (1 - uu) * (X010 - X000) + uu * (X011 - X001);
          Jt1[d] = (1 - uu) * (X110 - X100) + uu * (X111 - X101) - Jt0[d];
          Ju0[d] = (1 - t) * (X001 - X000) + t * (X011 - X010);
          Ju1[d] = (1 - t) * (X101 - X100) + t * (X111 - X110) - Ju0[d];
        }
      }
    }

    // ------------------------------------------------ F = kappa G grad
    T Fx[NQ];
    using V = typename VecOf<T>::type;
    constexpr int VW = VecOf<T>::W;
    V vy, vz;
    auto emit = [&](int q, T fx, T fy, T fz) {
      BDX_PIN3(fx, fy, fz);
      Fx[q] = fx;
      vy[q % VW] = fy;
      vz[q % VW] = fz;
      if (q % VW == VW - 1 || q == NQ - 1) {
        if (q % VW != VW - 1) {
#pragma unroll
          for (int e = q % VW + 1; e < VW; ++e) vy[e] = vz[e] = T(0);
        }
        if (lane_on) {
          *reinterpret_cast<V*>(w1ab + (q / VW) * VW) = vy;
          *reinterpret_cast<V*>(w3ab + (q / VW) * VW) = vz;
        }
      }
    };
    if constexpr (AFF == 1) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const T w = s_qw[NQ + q];
        const T t0 = w * gx[q], t1 = w * gy[q], t2 = w * gz[q];
        emit(q, Gc[0] * t0 + Gc[1] * t1 + Gc[2] * t2, Gc[1] * t0 + Gc[3] * t1 + Gc[4] * t2,
             Gc[2] * t0 + Gc[4] * t1 + Gc[5] * t2);
      }
    } else if constexpr (AFF == 2) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const T s = s_qw[q];
        const T bb = xbt0 + s * xbt1, cc = xcu0 + s * xcu1;
        const T p = gx[q] * xia;
        const T q1 = gy[q] * xihy - bb * p, q2 = gz[q] * xihz - cc * p;
        const T sq = xcs * s_qw[NQ + q];
        const T m0 = sq * p, m1 = sq * q1, m2 = sq * q2;
        emit(q, (m0 - bb * m1 - cc * m2) * xia, m1 * xihy, m2 * xihz);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const T s = s_qw[q];
        const T J00 = Js[0], J10 = Js[1], J20 = Js[2];
        const T J01 = Jt0[0] + s * Jt1[0], J11 = Jt0[1] + s * Jt1[1], J21 = Jt0[2] + s * Jt1[2];
        const T J02 = Ju0[0] + s * Ju1[0], J12 = Ju0[1] + s * Ju1[1], J22 = Ju0[2] + s * Ju1[2];
        const T K00 = J11 * J22 - J12 * J21, K01 = J02 * J21 - J01 * J22, K02 = J01 * J12 - J02 * J11;
        const T K10 = J12 * J20 - J10 * J22, K11 = J00 * J22 - J02 * J20, K12 = J02 * J10 - J00 * J12;
        const T K20 = J10 * J21 - J11 * J20, K21 = J01 * J20 - J00 * J21, K22 = J00 * J11 - J01 * J10;
        const T det = J00 * K00 + J01 * K10 + J02 * K20;
        const T sc = kwyz * s_qw[NQ + q] * fast_rcp(det);
        const T h0 = K00 * gx[q] + K10 * gy[q] + K20 * gz[q];
        const T h1 = K01 * gx[q] + K11 * gy[q] + K21 * gz[q];
        const T h2 = K02 * gx[q] + K12 * gy[q] + K22 * gz[q];
        emit(q, sc * (K00 * h0 + K01 * h1 + K02 * h2), sc * (K10 * h0 + K11 * h1 + K12 * h2),
             sc * (K20 * h0 + K21 * h1 + K22 * h2));
      }
    }
    __syncthreads();

    // ------------------------------------------------ transposed gradient
    T r[NQ];
    {
      if (lane_on) strow<NQ>(w2ab, Fx);
      const T* __restrict__ dca = s_tab + S::OFF_DC + a * XP;
      const T* __restrict__ dcb = s_tab + S::OFF_DC + b * XP;
#pragma unroll
      for (int q = 0; q < NQ; ++q) r[q] = T(0);
BDX_PRAGMA_UNROLL(1)
      for (int m = 0; m < NQ; ++m) {
        T r1[NQ], r3[NQ];
        ldrow<NQ>(w1b + m * NQ * XP, r1);
        ldrow<NQ>(w3a + m * XP, r3);
        const T fm = w2ab[m], ca = dca[m], cb_ = dcb[m];
        const T* __restrict__ dr = gt + S::OFF_DR + m * XP;
#pragma unroll
        for (int q = 0; q < NQ; ++q) r[q] += dr[q] * fm + ca * r1[q] + cb_ * r3[q];
      }
    }
    T sx[ND];
    if constexpr (IDENT) {
#pragma unroll
      for (int i = 0; i < ND; ++i) sx[i] = r[i];
    } else {
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        T acc = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc += gt[S::OFF_PC + i * XP + q] * r[q];
        sx[i] = acc;
      }
    }

    // ------------------------------------------------ back to the dofs
    T ye[ND];
    if constexpr (IDENT) {
#pragma unroll
      for (int i = 0; i < ND; ++i) ye[i] = sx[i];
    } else {
      // (no barrier: the transposed-gradient stage read only this lane's own
      // w2 row; the S8 write into w1 below is ordered by the next barrier)
      if (lane_on) strow<ND>(w2ab, sx);
      __syncthreads();
      if (lane_on && a < ND) {
        const T* __restrict__ pca = s_tab + S::OFF_PC + a * XP;
        T o[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) o[i] = 0;
BDX_PRAGMA_UNROLL(1)
        for (int q = 0; q < NQ; ++q) {
          T row[ND];
          ldrow<ND>(w2b + q * NQ * XP, row);
          const T cc = pca[q];
#pragma unroll
          for (int i = 0; i < ND; ++i) o[i] += cc * row[i];
        }
        strow<ND>(w1ab, o);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < ND; ++i) ye[i] = 0;
      if (a < ND && b < ND) {
        const T* __restrict__ pcb = s_tab + S::OFF_PC + b * XP;
BDX_PRAGMA_UNROLL(1)
        for (int q = 0; q < NQ; ++q) {
          T row[ND];
          ldrow<ND>(w1a + q * XP, row);
          const T cc = pcb[q];
#pragma unroll
          for (int i = 0; i < ND; ++i) ye[i] += cc * row[i];
        }
      }
    }

    // ------------------------------------------------ element vectors -> LDS
    const bool dof_lane = cell_on && a < ND && b < ND;
    if constexpr (MODE == kFusedCG) {
      if (dof_lane && !red) {
#pragma unroll
        for (int i = 0; i < ND; ++i)
          pap += static_cast<double>(ua[i * PLP + b]) * static_cast<double>(ye[i]);
      }
    }
    if constexpr (IDENT) {
      __syncthreads();
    }
    if (lane_on && a < ND && b < ND) {
      if (!dof_lane) {
#pragma unroll
        for (int i = 0; i < ND; ++i) ye[i] = T(0);
      }
      strow<ND>(w2ab, ye);
    }
    __syncthreads();

    // ------------------------------------------------ gather-sum and write out
    {
      const int64_t lbase = static_cast<int64_t>(cx) * P;
      T* __restrict__ ybase[4] = {A.y + lbase * A.ps, A.yb + lbase * A.ybps,
                                  A.zb + lbase * A.zbps, A.cb + lbase * A.cbps};
#pragma unroll
      for (int k = 0; k < NOUT; ++k) {
        const int m = o_meta[k];
        if (!(m & kValid)) continue;
        const int pl = (m >> 8) & 15, rem = m >> 12;
        T v = s_w2[o_src[k][0] & 0xffff] + s_w2[o_src[k][0] >> 16] +
              s_w2[o_src[k][1] & 0xffff] + s_w2[o_src[k][1] >> 16];
        if (pl == 0) v += s_c[cur][rem];
        if (pl == P && !last) {
          s_c[nxt][rem] = v;
          continue;
        }
        // a redundant layer only carries; a segment's end plane is completed
        // (and written) by the next segment
        if (red || (pl == P && !glast)) continue;
        const int gxx = cx * P + pl;
        const bool bc = (m & kBcYZ) || gxx == A.bcx_lo || gxx == A.bcx_hi;
        const int kind = (m >> 4) & 3;
        if (bc) {
          if (kind == 0) continue;  // Dirichlet y was written at staging
          v = T(0);
        }
        T* __restrict__ dst = kind == 0 ? ybase[0] : kind == 1 ? ybase[1] : kind == 2 ? ybase[2] : ybase[3];
        dst[o_off[k]] = v;
      }
    }

    // ------------------------------------------------ stage the next layer
    if (!last) {
      T* __restrict__ un = s_u[nxt];
#pragma unroll
      for (int k = 0; k < NCP; ++k)
        if (cp_lds[k] >= 0) un[cp_lds[k]] = su[P * PLP + cp_lds[k]];
      T* __restrict__ pnl = A.pnew + lnext;
      T* __restrict__ yl = A.y + lnext;
#pragma unroll
      for (int k = 0; k < NPF; ++k) {
        const int m = st_meta[k];
        if (tid + k * NT < P * PL) {
          T v = T(0);
          if (m & kValid) {
            const int gxx = (cx + 1) * P + ((m >> 4) & 15);
            T val;
            if constexpr (MODE == kFusedCG) {
              val = pf_r[k] + beta * pf_p[k];
            } else {
              val = pf_r[k];
            }
            if constexpr (MODE == kFusedCG) {
              if (m & kOwnT) {
                pnl[st_goff[k]] = val;
                if (xupd) A.x[lnext + st_goff[k]] = pf_x[k] + xalpha * pf_p[k];
              }
            }
            if ((m & kBcYZ) || gxx == A.bcx_hi) {
              if (m & kOwnT) {
                const bool rown = (m & kRownYZ) && gxx < A.ownx;
                yl[st_goff[k]] = rown ? val : T(0);
                if constexpr (MODE == kFusedCG) {
                  if (rown) pap += static_cast<double>(val) * static_cast<double>(val);
                }
              }
              val = T(0);
            }
            v = val;
          }
          un[m >> 8] = v;
        }
      }
#pragma unroll
      for (int k = 0; k < NPV; ++k) {
        const int e = tid + k * NT;
        if (e < NV) s_X[nxt][e] = sX[NV + e];
      }
#pragma unroll
      for (int k = 0; k < NPV; ++k) {
        const int e = tid + k * NT;
        if (e < NV) s_X[nxt][NV + e] = pf_v[k];
      }
    }
  }
  if constexpr (MODE == kFusedCG) {
    const double t = block_sum(pap, s_red);
    // indexed by (tile, segment): invariant under any launch split
    if (tid == 0) A.partials[(ty * A.ntz + tz) * A.nseg + seg] = t;
  }
}

// Host-side launch: build the argument block from the packed lattice
// descriptor (fem/mesh.py LocalLattice.as_int64) and launch one workgroup per
// (y, z) tile.
template <typename T, int ND, int NQ, int MODE>
int launch_fused2(int affine, const Fused2Args<T>& a, const FusedTables<T>& tb, hipStream_t st) {
  using TF = TileFor<NQ>;
  using S = FusedShape<T, ND, NQ, TF::TY, TF::TZ>;
  const int nblk = a.nblk;
  if (nblk <= 0) return 0;
  // affine: 1 = parallelepipeds, 2 = x-trilinear (y/z lattice), 0 = trilinear
  if (affine == 1)
    lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, MODE, 1><<<nblk, S::threads, 0, st>>>(a, tb);
  else if (affine == 2)
    lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, MODE, 2><<<nblk, S::threads, 0, st>>>(a, tb);
  else
    lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, MODE, 0><<<nblk, S::threads, 0, st>>>(a, tb);
  return static_cast<int>(hipGetLastError());
}

// Workgroups of `kernel` (blocks of `threads`, no dynamic LDS) the chip holds
// at once: the segment sizing of fused2 / fused3 / fused5.  0 if a query fails.
template <typename K>
int resident_workgroups(K kernel, int threads) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess)
    return 0;
  return per_cu * cus;
}

// The fused2 CG instance that sizes the segments of a launch.
template <typename T, int ND, int NQ>
int fused2_resident(int affine) {
  using TF = TileFor<NQ>;
  using S = FusedShape<T, ND, NQ, TF::TY, TF::TZ>;
  return resident_workgroups(
      affine == 1   ? lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, kFusedCG, 1>
      : affine == 2 ? lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, kFusedCG, 2>
                    : lap_fused2_kernel<T, ND, NQ, TF::TY, TF::TZ, kFusedCG, 0>,
      S::threads);
}

template <typename T>
inline int make_fused2_args(Fused2Args<T>& a, const int64_t* latd, int nty, int ntz) {
  const BdxLattice L = BdxLattice::from(latd);
  a.xmode = 0;
  a.xmode1 = -1;
  a.xslot_w = a.xslot_r = kScalXSave;
  const int64_t P = L.P;
  // 32-bit per-layer offsets: one layer of the vector must be < 2^31 elements
  if ((P + 1) * L.L[1] * L.ld >= (int64_t(1) << 31)) return static_cast<int>(hipErrorInvalidValue);
  a.ps = L.L[1] * L.ld;
  a.tsy = static_cast<int>(L.tsy);
  a.tsz = static_cast<int>(L.tsz);
  a.tntz = static_cast<int>(L.tntz);
  a.tcol = L.tcol;
  a.vsize = L.size();
  if (L.tsy) {
    // tiled: in-tile offsets are whole-vector offsets, still 32-bit
    if (L.size() >= (int64_t(1) << 31) || L.tsz <= 0) return static_cast<int>(hipErrorInvalidValue);
    a.ps = L.tsy * L.tsz;
  }
  const IfaceLayout F = IfaceLayout::of(L, nty, ntz);
  a.ybps = F.ybps();
  a.zbps = F.zbps();
  a.cbps = F.cbps();
  a.ibsize = std::max({F.yb_size(), F.zb_size(), F.cb_size()});
  a.vps = (L.n[1] + 1) * (L.n[2] + 1) * 3;
  a.ncx = static_cast<int>(L.n[0]);
  a.n1 = static_cast<int>(L.n[1]);
  a.n2 = static_cast<int>(L.n[2]);
  a.Ly = static_cast<int>(L.L[1]);
  a.Lz = static_cast<int>(L.L[2]);
  a.ld = static_cast<int>(L.ld);
  a.ownx = static_cast<int>(L.L[0] - L.gh[0]);
  a.owny = static_cast<int>(L.L[1] - L.gh[1]);
  a.ownz = static_cast<int>(L.L[2] - L.gh[2]);
  auto lo = [&](int d) { return L.g0[d] == 0 ? 0 : -1; };
  auto hi = [&](int d) {
    const int64_t i = L.N[d] - 1 - L.g0[d];
    return (i >= 0 && i < L.L[d]) ? static_cast<int>(i) : -1;
  };
  a.bcx_lo = lo(0);
  a.bcx_hi = hi(0);
  a.bcy_lo = lo(1);
  a.bcy_hi = hi(1);
  a.bcz_lo = lo(2);
  a.bcz_hi = hi(2);
  a.nty = nty;
  a.ntz = ntz;
  a.ty0 = a.tz0 = 0;
  a.rwz = ntz;
  a.rtiles = nty * ntz;
  a.nseg = 1;
  a.seglen = a.ncx;
  a.nblk = a.rtiles;
  return 0;
}

// Restrict a launch to the tile rectangle rect = {ty0, ty1, tz0, tz1} (host
// memory; null = every tile).  The runtime splits one operator apply into
// disjoint rectangles to overlap the halo exchange with the tiles that do not
// touch a ghost plane; p.Ap partials are tile-indexed, so the reduction is
// identical for any split.
template <typename T>
inline int fused_set_rect(Fused2Args<T>& a, const int* rect) {
  if (!rect) return 0;
  const int ty0 = rect[0], ty1 = rect[1], tz0 = rect[2], tz1 = rect[3];
  if (ty0 < 0 || tz0 < 0 || ty1 > a.nty || tz1 > a.ntz || ty1 < ty0 || tz1 < tz0)
    return static_cast<int>(hipErrorInvalidValue);
  a.ty0 = ty0;
  a.tz0 = tz0;
  a.rwz = tz1 > tz0 ? tz1 - tz0 : 1;
  a.rtiles = (ty1 - ty0) * (tz1 - tz0);
  a.nblk = a.rtiles * a.nseg;
  return 0;
}

// x segmentation.  A launch of R tiles on a chip that holds W workgroups at
// once runs ceil(R / W) rounds of whole x-marches; at the benchmark sizes the
// last round is nearly empty (1 GPU, Q3: 3136 tiles = 6.1 rounds of 512 ->
// 7 rounds, measured 12 % slower per DoF than an exact 6 or 7).  Cutting each
// tile's march into S segments makes R * S shorter work items whose rounds
// pack evenly.  A segment [a, b) of cell layers starts one layer early (a - 1,
// "redundant": computed but never written) so the partial sum it carries into
// plane a*P completes that plane locally; it writes planes [a*P, b*P) (plus
// the last plane if b is the end) and stages layers a .. b-1 (the redundant
// layer's planes belong to the previous segment).  No inter-workgroup
// synchronisation, bitwise identical to S = 1 except for the order of the
// p.Ap partial sums (one per work item).
//   S travels in the apply entry points' mode word (fused_mode_pack), 0 -> 1.
inline int fused_choose_segments(int tiles, int ncx, int resident) {
  if (tiles <= 0 || ncx <= 1 || resident <= 0) return 1;
  int best = 1;
  double best_cost = 1e300;
  for (int S = 1; S <= 16 && S <= ncx; ++S) {
    const int len = (ncx + S - 1) / S;
    const int segs = (ncx + len - 1) / len;
    // fractional rounds plus half a round of tail: workgroups do not run in
    // lock-step rounds, so a launch of 17.02 rounds costs about 17.5, not 18
    // (whole-round model vs this one, same box: fused5 Q3 6 -> 3 segments
    // 61.0 -> 61.7 GDoF/s, Q6 1 -> 2 segments 53.5 -> 54.3, fused3
    // x-trilinear Q6 1 -> 2 28.8 -> 29.8; profiles/r2_segments.md)
    const double rounds =
        static_cast<double>(static_cast<int64_t>(tiles) * segs) / resident + 0.5;
    // per work item: its layers, the redundant layer, and ~1 layer of
    // unpipelined prologue
    const double cost = rounds * (len + (S > 1 ? 2.0 : 1.0));
    if (cost < best_cost * 0.995) {
      best_cost = cost;
      best = segs;
    }
  }
  return best;
}

template <typename T>
inline int fused_set_segments(Fused2Args<T>& a, int nseg) {
  if (nseg < 1) nseg = 1;
  if (nseg > a.ncx) nseg = a.ncx > 0 ? a.ncx : 1;
  a.seglen = (a.ncx + nseg - 1) / nseg;
  a.nseg = a.seglen > 0 ? (a.ncx + a.seglen - 1) / a.seglen : 1;
  a.nblk = a.rtiles * a.nseg;
  return 0;
}

// Host-side launch prologue of the fused2 / fused3 / fused5 apply entry points
// (BDX_P_FUSED_APPLY, bdx_hip_api.h): the argument block from the lattice
// descriptor, the tile rectangle, the x segments of the mode word and the entry
// point's vectors, scalar slots and kappa.  What differs between the three
// (tiled storage, x-mode bits, tables) stays at their call sites.
template <typename T>
int fill_fused2_args(Fused2Args<T>& a, int mode, const int64_t* latd, int nty, int ntz,
                     const int* rect, const T* u, const T* pold, T* pnew, T* x, T* y, T* yb, T* zb,
                     T* cb, const T* xv, const T* kc, double kappa, const double* scal,
                     double* partials, int beta_num, int beta_den, int xa_num, int xa_den) {
  BDX_CHECK(static_cast<hipError_t>(make_fused2_args(a, latd, nty, ntz)));
  BDX_CHECK(static_cast<hipError_t>(fused_set_rect(a, rect)));
  BDX_CHECK(static_cast<hipError_t>(fused_set_segments(a, fused_mode_nseg(mode))));
  a.u = u;
  a.pold = pold;
  a.pnew = pnew;
  a.x = x;
  a.y = y;
  a.yb = yb;
  a.zb = zb;
  a.cb = cb;
  a.xv = xv;
  a.kc = kc;
  a.scal = scal;
  a.partials = partials;
  a.beta_num = beta_num;
  a.beta_den = beta_den;
  a.xa_num = xa_num;
  a.xa_den = xa_den;
  a.kappa = static_cast<T>(kappa);
  return 0;
}
// The prologue's arguments, by the parameter names of BDX_P_FUSED_APPLY.
#define BDX_FUSED_FILL_ARGS                                                              \
  a, mode, latd, nty, ntz, rect, u, pold, pnew, x, y, yb, zb, cb, xv, kc, kappa, scal,   \
      partials, beta_num, beta_den, xa_num, xa_den

#define BDX_FUSED2_TU(T, SUF, PP)                                                   \
  extern "C" int bdx_fused2_apply_##SUF##_p##PP BDX_P_FUSED_APPLY(T) {             \
    Fused2Args<T> a;                                                               \
    BDX_CHECK(static_cast<hipError_t>(fill_fused2_args<T>(BDX_FUSED_FILL_ARGS)));  \
    if (a.tsy) return static_cast<int>(hipErrorInvalidValue); /* lattice layout only */ \
    mode = fused_mode_kind_nox(mode);                                              \
    if (!tabs) return static_cast<int>(hipErrorInvalidValue);                      \
    FusedTables<T> tb;                                                             \
    for (int i = 0; i < kFusedTabMax; ++i) tb.tab[i] = tabs[i];                    \
    for (int q = 0; q < kMaxNq; ++q) {                                             \
      tb.qpts[q] = q < nq ? static_cast<T>(qpts[q]) : T(0);                        \
      tb.wts[q] = q < nq ? static_cast<T>(wts[q]) : T(0);                          \
    }                                                                              \
    if (nq == PP + 1)                                                              \
      return mode == kFusedCG ? launch_fused2<T, PP + 1, PP + 1, kFusedCG>(affine_ok, a, tb, st) \
                              : launch_fused2<T, PP + 1, PP + 1, kFusedAction>(affine_ok, a, tb, st); \
    if (nq == PP + 2)                                                              \
      return mode == kFusedCG ? launch_fused2<T, PP + 1, PP + 2, kFusedCG>(affine_ok, a, tb, st) \
                              : launch_fused2<T, PP + 1, PP + 2, kFusedAction>(affine_ok, a, tb, st); \
    return static_cast<int>(hipErrorInvalidValue);                                 \
  }                                                                                \
  extern "C" int bdx_fused2_segments_##SUF##_p##PP(int affine_ok, int nq, int tiles, int ncx) { \
    const int res = nq == PP + 1 ? fused2_resident<T, PP + 1, PP + 1>(affine_ok)   \
                                 : fused2_resident<T, PP + 1, PP + 2>(affine_ok);  \
    return fused_choose_segments(tiles, ncx, res);                                 \
  }
