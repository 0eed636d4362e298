// Device BLAS-1, CG vector updates, halo pack/unpack (gfx950).
//
// Replaces the reference's Thrust calls (src/vector.hpp:151-292,
// src/cg.hpp:21-79) and pack/unpack kernels (src/vector.hpp:31-62).
// Differences by design:
//   * every reduction is device-resident: per-block partials + one
//     fixed-order final pass into a float64 scalar slot (deterministic, no
//     host round trip); the all-reduce then runs on that device scalar;
//   * the CG scalars (alpha, beta) are formed on the device from those slots;
//   * x/r updates and the r.r reduction are one fused pass;
//   * reductions and updates walk the owned sub-box of the local lattice
//     one z-row per wave (rows are 128-byte aligned by the storage pitch):
//     `for_each_owned` of blas_rows.h, which also holds the dot, cg_update and
//     p_update kernels (instantiated here and, with an FP32 operand, in
//     mixed.hip).
#include "blas_rows.h"

#include "bdx_mg_bodies.h"  // cheb_entry (after the HIP runtime's BDX_HD)

namespace {

using bdx_rows::cg_update_kernel;
using bdx_rows::dot_rows_kernel;
using bdx_rows::for_each_owned;
using bdx_rows::grid_for_rows;
using bdx_rows::kBlock;
using bdx_rows::p_update_kernel;
using bdx_rows::RowSpace;

// Fixed-order sum of partials into out[slot] (single block).
__global__ void __launch_bounds__(kBlock)
    reduce_partials_kernel(const double* __restrict__ partials, int n,
                           double* __restrict__ out, int slot) {
  __shared__ double lds[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  const double t = block_sum(acc, lds);
  if (threadIdx.x == 0) out[slot] = t;
}

// Jacobi-preconditioned CG (z = dinv . r is never stored):
// alpha = s[rz] / s[pap];  x += alpha p;  r -= alpha y;  per-block partials of
// r.z = sum dinv r^2 (partials[0 .. grid)) and r.r (partials[grid .. 2 grid)).
template <typename T>
__global__ void __launch_bounds__(kBlock)
    pcg_update_kernel(RowSpace s, T* __restrict__ x, T* __restrict__ r,
                      const T* __restrict__ p, const T* __restrict__ y,
                      const T* __restrict__ dinv, const double* __restrict__ scal, int rz_slot,
                      int pap_slot, double* __restrict__ partials) {
  __shared__ double lds_rz[16], lds_rr[16];
  const T alpha = static_cast<T>(scal[rz_slot] / scal[pap_slot]);
  double acc_rz = 0.0, acc_rr = 0.0;
  for_each_owned(s, [&](int64_t i) {
    x[i] = x[i] + alpha * p[i];
    const T rn = r[i] - alpha * y[i];
    r[i] = rn;
    const double rr = static_cast<double>(rn) * static_cast<double>(rn);
    acc_rr += rr;
    acc_rz += static_cast<double>(dinv[i]) * rr;
  });
  const double tz = block_sum(acc_rz, lds_rz);
  const double tr = block_sum(acc_rr, lds_rr);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = tz;
    partials[gridDim.x + blockIdx.x] = tr;
  }
}

// p = beta p + dinv . r with beta = s[num] / s[den] (owned rows).
template <typename T>
__global__ void __launch_bounds__(kBlock)
    pcg_p_update_kernel(RowSpace s, T* __restrict__ p, const T* __restrict__ r,
                        const T* __restrict__ dinv, const double* __restrict__ scal, int num,
                        int den) {
  const T beta = static_cast<T>(scal[num] / scal[den]);
  for_each_owned(s, [&](int64_t i) { p[i] = beta * p[i] + dinv[i] * r[i]; });
}

// One step of the Chebyshev-Jacobi smoother (solvers/pmg.py) over the owned
// rows, y = A z computed by the caller:  d = a d + b dinv (r - y);  z += d.
// FIRST (the step from a zero guess):  d = b dinv r;  z = d, which reads
// neither y nor the old d and z.  One pass of five reads and two writes; the
// entry update is cheb_entry (bdx_mg_bodies.h), shared with the V-cycle tail
// and the host twin.
template <typename T, bool FIRST>
__global__ void __launch_bounds__(kBlock)
    cheb_step_kernel(RowSpace s, T a, T b, const T* __restrict__ dinv, const T* __restrict__ r,
                     const T* __restrict__ y, T* __restrict__ d, T* __restrict__ z) {
  for_each_owned(s, [&](int64_t i) { cheb_entry<T>(FIRST, a, b, dinv, r, y, d, z, i); });
}

// out = alpha x + y over owned rows (reference axpy, src/vector.hpp:228-240).
template <typename T>
__global__ void __launch_bounds__(kBlock)
    axpy_kernel(RowSpace s, T* __restrict__ out, T alpha, const T* __restrict__ x,
                const T* __restrict__ y) {
  for_each_owned(s, [&](int64_t i) { out[i] = alpha * x[i] + y[i]; });
}

// ------------------------------------------------------------- halo boxes
// Box table in device memory: per box {lo0,lo1,lo2, e0,e1,e2, offset} (int64).
constexpr int kBoxFields = 7;

// MODE 0 pack, 1 unpack (assign), 2 unpack (add).  `only` >= 0 restricts the
// pass to one box: the owned lower-face boxes overlap on edges/corners (a dof
// there receives partial sums from up to 7 neighbours), so the add-unpack runs
// box by box -- race-free and in a fixed order.
// Storage index of lattice node (i, j, k): the lattice layout or the tiled
// one of the CG runtime (bdx_lattice.h, tsy != 0).
struct VecIdx {
  int64_t L1, ld, tsy, tsz, tntz, tcol;
  __device__ __forceinline__ int64_t operator()(int64_t i, int64_t j, int64_t k) const {
    if (tsy) return ((j / tsy) * tntz + k / tsz) * tcol + (i * tsy + j % tsy) * tsz + k % tsz;
    return (i * L1 + j) * ld + k;
  }
};

// Pack / unpack of the halo boxes (see the box table above).
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock)
    box_copy_kernel(T* __restrict__ vec, VecIdx vi,
                    const int64_t* __restrict__ boxes, int nboxes, int64_t total,
                    T* __restrict__ buf, int only = -1) {
  int64_t t0 = 0, t1 = total;
  if (only >= 0) {
    t0 = boxes[only * kBoxFields + 6];
    t1 = only + 1 < nboxes ? boxes[(only + 1) * kBoxFields + 6] : total;
  }
  for (int64_t t = t0 + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < t1;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    int b = only >= 0 ? only : 0;
    while (only < 0 && b + 1 < nboxes && boxes[(b + 1) * kBoxFields + 6] <= t) ++b;
    const int64_t* bx = boxes + b * kBoxFields;
    const int64_t o = t - bx[6];
    const int64_t e1 = bx[4], e2 = bx[5];
    const int64_t k = o % e2, j = (o / e2) % e1, i = o / (e1 * e2);
    const int64_t v = vi(bx[0] + i, bx[1] + j, bx[2] + k);
    if constexpr (MODE == 0)
      buf[t] = vec[v];
    else if constexpr (MODE == 1)
      vec[v] = buf[t];
    else
      vec[v] += buf[t];
  }
}

// Lattice layout <-> tiled layout of one vector, every node of the local
// lattice (owned and ghost).  dir 0: tiled[t(i,j,k)] = lat[l(i,j,k)]; 1: back.
template <typename T>
__global__ void __launch_bounds__(kBlock)
    layout_convert_kernel(int dir, VecIdx lat, VecIdx til, int64_t L0, int64_t L1v,
                          int64_t L2, T* __restrict__ a, T* __restrict__ t) {
  const int64_t n = L0 * L1v * L2;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < n;
       e += static_cast<int64_t>(gridDim.x) * kBlock) {
    // e enumerates the tiled order (tile, x, ly, lz) of valid nodes would need
    // divisions by run-time tile sizes; enumerate lattice order instead (the
    // lattice side then streams, the tiled side moves in 8..16-node runs)
    const int64_t k = e % L2, r = e / L2, j = r % L1v, i = r / L1v;
    if (BDX_OOB(til(i, j, k), til.tsy ? ((L1v - 1) / til.tsy + 1) * til.tntz * til.tcol : n,
                "layout convert"))
      continue;
    if (dir == 0)
      t[til(i, j, k)] = a[lat(i, j, k)];
    else
      a[lat(i, j, k)] = t[til(i, j, k)];
  }
}

constexpr int kFeTiles = 16;  // tiles per flush_export block along z

// End of a CG call on tiled storage: the lagged x terms folded into the tiled
// iterate and the result exported to the lattice layout in one pass
// (t += a1 p1 [+ a2 p2]; lat = t) instead of a flush pass per term plus a
// conversion pass.  a = scal[num] / scal[den], den < 0: scal[num] itself.
// One block per (x-plane, tile row, group of kFeTiles tiles along z): it
// reads the group's tiled chunks ([tile][x][ly][lz], contiguous) in 16-byte
// vectors, stages the result in LDS in lattice order and writes the group's
// z-rows contiguously, so both sides stream (the element-wise forms ran at
// 2-3.7 TB/s: 64-bit divisions per element, then 96-byte lattice runs).
// Every access is non-temporal (+0.2 % on the 20-step Q3 / Q6 runs that
// carry one flush each, profiles/r4_update_pass_ab.txt).
template <typename T>
__global__ void __launch_bounds__(kBlock)
    flush_export_kernel(int64_t L0, int64_t L1, int64_t L2, int64_t ld, int tsy, int tsz,
                        int tntz, int ngz, T* __restrict__ a, T* __restrict__ t,
                        const T* __restrict__ p1, const T* __restrict__ p2,
                        const double* __restrict__ scal, int num1, int den1, int num2, int den2,
                        int p2mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fe_lds[];
  T* const sv = reinterpret_cast<T*>(fe_lds);  // [tsy][kFeTiles * tsz]
  const T a1 = static_cast<T>(den1 < 0 ? scal[num1] : scal[num1] / scal[den1]);
  const T a2 = p2 ? static_cast<T>(den2 < 0 ? scal[num2] : scal[num2] / scal[den2]) : T(0);
  constexpr int W = 16 / sizeof(T);
  typedef T V __attribute__((ext_vector_type(W)));
  // block -> (x, tile row ty, z group g); x fastest
  const int64_t bidx = blockIdx.x;
  const int64_t x = bidx % L0, rest = bidx / L0;
  const int g = static_cast<int>(rest % ngz), ty = static_cast<int>(rest / ngz);
  const int tz0 = g * kFeTiles;
  const int nt = tntz - tz0 < kFeTiles ? tntz - tz0 : kFeTiles;  // tiles of this group
  const int C = tsy * tsz, CV = C / W;                              // chunk, vectors per chunk
  const int pitch = kFeTiles * tsz;                                 // LDS row pitch
  const int64_t cbase = (static_cast<int64_t>(ty) * tntz + tz0) * L0 + x;  // chunk index of tile tz0
  for (int q = threadIdx.x; q < nt * CV; q += kBlock) {
    const int tl = q / CV, e = (q - tl * CV) * W;
    const int64_t off = (cbase + static_cast<int64_t>(tl) * L0) * C + e;
    V vt = __builtin_nontemporal_load(reinterpret_cast<const V*>(t + off));
    vt += a1 * __builtin_nontemporal_load(reinterpret_cast<const V*>(p1 + off));
    // p2mask: the tile colours ((ty + tz) & 1) with the second term pending
    if (p2 && ((p2mask >> ((ty + tz0 + tl) & 1)) & 1))
      vt += a2 * __builtin_nontemporal_load(reinterpret_cast<const V*>(p2 + off));
    if (!(p2mask & 4)) __builtin_nontemporal_store(vt, reinterpret_cast<V*>(t + off));
    int ly = e / tsz, lz = e - ly * tsz;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      sv[ly * pitch + tl * tsz + lz] = vt[w];
      if (++lz == tsz) {
        lz = 0;
        ++ly;
      }
    }
  }
  __syncthreads();
  const int64_t k0 = static_cast<int64_t>(tz0) * tsz;
  const int64_t kend = (k0 + nt * tsz < L2) ? k0 + nt * tsz : L2;
  const int nk = static_cast<int>(kend - k0);
  const int64_t j0 = static_cast<int64_t>(ty) * tsy;
  const int nj = static_cast<int>((j0 + tsy <= L1) ? tsy : L1 - j0);
  for (int r = threadIdx.x; r < nj * nk; r += kBlock) {
    const int ly = r / nk, kk = r - ly * nk;
    __builtin_nontemporal_store(sv[ly * pitch + kk], a + (x * L1 + j0 + ly) * ld + k0 + kk);
  }
}

template <typename T>
int box_copy_vi(int mode, T* vec, VecIdx vi, const int64_t* boxes, int nboxes, int64_t total,
                T* buf, hipStream_t st) {
  if (total <= 0) return 0;
  const int64_t g64 = (total + kBlock - 1) / kBlock;
  const int g = static_cast<int>(g64 < 4096 ? g64 : 4096);
  if (mode == 0) {
    box_copy_kernel<T, 0><<<g, kBlock, 0, st>>>(vec, vi, boxes, nboxes, total, buf);
  } else if (mode == 1) {
    box_copy_kernel<T, 1><<<g, kBlock, 0, st>>>(vec, vi, boxes, nboxes, total, buf);
  } else {  // add: boxes may overlap (edges/corners), one launch per box
    for (int b = 0; b < nboxes; ++b)
      box_copy_kernel<T, 2><<<g, kBlock, 0, st>>>(vec, vi, boxes, nboxes, total, buf, b);
  }
  return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int bdx_hip_partials_size() { return 65536; }  // >= kPartialsCap (cg_update.hip)

// Fixed-order reduction of n per-block partials into out[slot].
int bdx_reduce_partials(const double* partials, int n, double* out, int slot,
                        hipStream_t st) {
  reduce_partials_kernel<<<1, kBlock, 0, st>>>(partials, n, out, slot);
  return static_cast<int>(hipGetLastError());
}

#define BDX_BLAS_API(T, SUF)                                                  \
  int bdx_dot_##SUF BDX_P_DOT(T) {                                            \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    const int g = grid_for_rows(o0 * o1);                                     \
    dot_rows_kernel<T, T><<<g, kBlock, 0, st>>>(s, a, b, partials);           \
    reduce_partials_kernel<<<1, kBlock, 0, st>>>(partials, g, out, slot);     \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_cg_update_##SUF BDX_P_CG_UPDATE(T) {                                \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    const int g = grid_for_rows(o0 * o1);                                     \
    cg_update_kernel<T, false><<<g, kBlock, 0, st>>>(                         \
        s, x, r, p, y, scal, rn_slot, pap_slot, partials, nullptr);           \
    reduce_partials_kernel<<<1, kBlock, 0, st>>>(partials, g, scal, out_slot); \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_p_update_##SUF BDX_P_P_UPDATE(T) {                                  \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    p_update_kernel<T, T><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(         \
        s, p, r, scal, num, den);                                             \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_pcg_update_##SUF BDX_P_PCG_UPDATE(T) {                              \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    const int g = grid_for_rows(o0 * o1);                                     \
    pcg_update_kernel<T><<<g, kBlock, 0, st>>>(s, x, r, p, y, dinv, scal,     \
                                               rz_slot, pap_slot, partials);  \
    reduce_partials_kernel<<<1, kBlock, 0, st>>>(partials, g, scal, out_slot); \
    reduce_partials_kernel<<<1, kBlock, 0, st>>>(partials + g, g, scal,       \
                                                 rr_slot);                    \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_pcg_p_update_##SUF BDX_P_PCG_P_UPDATE(T) {                          \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    pcg_p_update_kernel<T><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(        \
        s, p, r, dinv, scal, num, den);                                       \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_cheb_step_##SUF BDX_P_CHEB_STEP(T) {                                \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    const int g = grid_for_rows(o0 * o1);                                     \
    if (first)                                                                \
      cheb_step_kernel<T, true><<<g, kBlock, 0, st>>>(                        \
          s, static_cast<T>(a), static_cast<T>(b), dinv, r, y, d, z);         \
    else                                                                      \
      cheb_step_kernel<T, false><<<g, kBlock, 0, st>>>(                       \
          s, static_cast<T>(a), static_cast<T>(b), dinv, r, y, d, z);         \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_axpy_##SUF BDX_P_AXPY(T) {                                          \
    RowSpace s{L1, ld, o0, o1, o2};                                           \
    axpy_kernel<T><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(                \
        s, out, static_cast<T>(alpha), x, y);                                 \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_box_copy_##SUF BDX_P_BOX_COPY(T) {                                  \
    const VecIdx vi{L1, ld, 0, 0, 0, 0};                                      \
    return box_copy_vi<T>(mode, vec, vi, boxes, nboxes, total, buf, st);      \
  }                                                                           \
  int bdx_box_copy_lat_##SUF BDX_P_BOX_COPY_LAT(T) {                          \
    const BdxLattice L = BdxLattice::from(latd);                              \
    const VecIdx vi{L.L[1], L.ld, L.tsy, L.tsz, L.tntz, L.tcol};              \
    return box_copy_vi<T>(mode, vec, vi, boxes, nboxes, total, buf, st);      \
  }                                                                           \
  int bdx_layout_convert_##SUF BDX_P_LAYOUT_CONVERT(T) {                      \
    const BdxLattice L = BdxLattice::from(latd_tiled);                        \
    if (!L.tsy) return static_cast<int>(hipErrorInvalidValue);                \
    const VecIdx lv{L.L[1], L.ld, 0, 0, 0, 0};                                \
    const VecIdx tv{L.L[1], L.ld, L.tsy, L.tsz, L.tntz, L.tcol};              \
    const int64_t n = L.L[0] * L.L[1] * L.L[2];                               \
    const int64_t g64 = (n + kBlock - 1) / kBlock;                            \
    const int g = static_cast<int>(g64 < 65536 ? g64 : 65536);                \
    layout_convert_kernel<T><<<g, kBlock, 0, st>>>(dir, lv, tv, L.L[0], L.L[1], \
                                                   L.L[2], lat, tiled);       \
    return static_cast<int>(hipGetLastError());                               \
  }                                                                           \
  int bdx_flush_export_##SUF BDX_P_FLUSH_EXPORT(T) {                          \
    const BdxLattice L = BdxLattice::from(latd_tiled);                        \
    if (!L.tsy || (L.tsy * L.tsz * static_cast<int64_t>(sizeof(T))) % 16)    \
      return static_cast<int>(hipErrorInvalidValue);                          \
    const int64_t nty = (L.L[1] - 1) / L.tsy + 1;                             \
    const int ngz = static_cast<int>((L.tntz + kFeTiles - 1) / kFeTiles);     \
    const int64_t nblk = L.L[0] * nty * ngz;                                  \
    const size_t lds = static_cast<size_t>(L.tsy) * kFeTiles * L.tsz * sizeof(T); \
    if (nblk <= 0) return 0;                                                  \
    if (nblk > 0x7fffffffLL || lds > 64 * 1024)                               \
      return static_cast<int>(hipErrorInvalidValue);                          \
    flush_export_kernel<T><<<static_cast<unsigned>(nblk), kBlock, lds, st>>>( \
        L.L[0], L.L[1], L.L[2], L.ld, static_cast<int>(L.tsy),                \
        static_cast<int>(L.tsz), static_cast<int>(L.tntz), ngz, lat, tiled,   \
        p1, p2, scal, num1, den1, num2, den2, p2mask);                        \
    return static_cast<int>(hipGetLastError());                               \
  }

BDX_BLAS_API(double, f64)
BDX_BLAS_API(float, f32)

}  // extern "C"
