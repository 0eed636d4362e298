// Fused-kernel helpers: tile query, table packing, the interface-partials
// finalize pass and the flush of the lagged x update (the CG update pass is
// cg_update.hip).
#include "lap_fused3.h"

// Packed 1D tables of the fused kernel (layout: FusedShape::OFF_*), written
// to host memory `out` (which the caller uploads).  Returns the count.
template <typename T, int ND, int NQ>
int pack_tables(const double* phi0, const double* dphi1, T* out) {
  using S = FusedShape<T, ND, NQ, 1, 1>;
  if (!out) return kFusedTabMax;
  for (int i = 0; i < kFusedTabMax; ++i) out[i] = T(0);
  for (int q = 0; q < NQ; ++q)
    for (int m = 0; m < NQ; ++m) {
      out[S::OFF_DR + q * S::XP + m] = static_cast<T>(dphi1[q * NQ + m]);
      out[S::OFF_DC + m * S::XP + q] = static_cast<T>(dphi1[q * NQ + m]);
    }
  for (int q = 0; q < NQ; ++q)
    for (int i = 0; i < ND; ++i) {
      out[S::OFF_PR + q * S::NP + i] = static_cast<T>(phi0[q * ND + i]);
      out[S::OFF_PC + i * S::XP + q] = static_cast<T>(phi0[q * ND + i]);
    }
  return kFusedTabMax;
}

// x += (s[num] / s[den]) p over the owned rows (flush of the lagged x update).
template <typename T>
__global__ void __launch_bounds__(256)
    xflush_kernel(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, T* __restrict__ x,
                  const T* __restrict__ p, const double* __restrict__ scal, int num, int den) {
  // den < 0: alpha stored directly in scal[num] (kScalXSave, runtime.hip)
  const T alpha = static_cast<T>(den < 0 ? scal[num] : scal[num] / scal[den]);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t nrows = o0 * o1;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + wid; row < nrows;
       row += static_cast<int64_t>(gridDim.x) * 4) {
    const int64_t i = row / o1, j = row - i * o1;
    const int64_t base = (i * L1 + j) * ld;
    for (int64_t k = lane; k < o2; k += 64) x[base + k] += alpha * p[base + k];
  }
}

static int rows_grid(int64_t nrows) {
  const int64_t want = (nrows + 3) / 4;
  return static_cast<int>(want < 2048 ? (want > 0 ? want : 1) : 2048);
}

extern "C" {

// Tile shape (cells in y, z) used by the fused kernel for a given nq.
int bdx_fused_tile(int nq, int* ty, int* tz) {
  switch (nq) {
#define BDX_T(NQ)                 \
  case NQ:                        \
    *ty = TileFor<NQ>::TY;        \
    *tz = TileFor<NQ>::TZ;        \
    return 0;
    BDX_T(2) BDX_T(3) BDX_T(4) BDX_T(5) BDX_T(6) BDX_T(7) BDX_T(8) BDX_T(9)
#undef BDX_T
  }
  return static_cast<int>(hipErrorInvalidValue);
}

#define BDX_FIN(T, SUF)                                                          \
  int bdx_fused_finalize_##SUF BDX_P_FUSED_FINALIZE(T) {                           \
    const BdxLattice lat = BdxLattice::from(latd);                                 \
    const IfaceLayout F = IfaceLayout::of(lat, nty, ntz);                                \
    if (ghost_only) {                                                              \
      const int64_t xB = lat.gh[0] ? F.Lx - 1 : F.Lx;                              \
      const int64_t n = (lat.gh[0] ? F.ybps() + F.zbps() : 0) +                    \
                        (lat.gh[1] ? xB * (ntz - 1) : 0) + (lat.gh[2] ? xB * (nty - 1) : 0); \
      if (n <= 0) return 0;                                                        \
      int64_t g = (n + 255) / 256;                                                 \
      if (g > 4096) g = 4096;                                                      \
      fused_finalize_ghost_kernel<T><<<static_cast<unsigned>(g), 256, 0, st>>>(    \
          lat, y, yb, zb, cb, nty, ntz, sy, sz);                                   \
      return static_cast<int>(hipGetLastError());                                  \
    }                                                                              \
    const int64_t n = F.yb_size() + F.zb_size();                                   \
    if (n <= 0) return 0;                                                          \
    int64_t g = (n + 255) / 256;                                                   \
    if (g > 8192) g = 8192;                                                        \
    fused_finalize_kernel<T><<<static_cast<unsigned>(g), 256, 0, st>>>(            \
        lat, y, yb, zb, cb, nty, ntz, sy, sz, 0);                                  \
    return static_cast<int>(hipGetLastError());                                    \
  }                                                                                \
  int bdx_xflush_##SUF BDX_P_XFLUSH(T) {                                           \
    const BdxLattice lat = BdxLattice::from(latd);                                 \
    xflush_kernel<T><<<rows_grid(own[0] * own[1]), 256, 0, st>>>(                  \
        lat.L[1], lat.ld, own[0], own[1], own[2], x, p, scal, num, den);           \
    return static_cast<int>(hipGetLastError());                                    \
  }

BDX_FIN(double, f64)
BDX_FIN(float, f32)

#define BDX_TABS(T, SUF)                                                           \
  int bdx_fused_tables_##SUF BDX_P_FUSED_TABLES(T) {                               \
    switch (nd * 16 + nq) {                                                        \
      case 2 * 16 + 2: return pack_tables<T, 2, 2>(phi0, dphi1, out);              \
      case 2 * 16 + 3: return pack_tables<T, 2, 3>(phi0, dphi1, out);              \
      case 3 * 16 + 3: return pack_tables<T, 3, 3>(phi0, dphi1, out);              \
      case 3 * 16 + 4: return pack_tables<T, 3, 4>(phi0, dphi1, out);              \
      case 4 * 16 + 4: return pack_tables<T, 4, 4>(phi0, dphi1, out);              \
      case 4 * 16 + 5: return pack_tables<T, 4, 5>(phi0, dphi1, out);              \
      case 5 * 16 + 5: return pack_tables<T, 5, 5>(phi0, dphi1, out);              \
      case 5 * 16 + 6: return pack_tables<T, 5, 6>(phi0, dphi1, out);              \
      case 6 * 16 + 6: return pack_tables<T, 6, 6>(phi0, dphi1, out);              \
      case 6 * 16 + 7: return pack_tables<T, 6, 7>(phi0, dphi1, out);              \
      case 7 * 16 + 7: return pack_tables<T, 7, 7>(phi0, dphi1, out);              \
      case 7 * 16 + 8: return pack_tables<T, 7, 8>(phi0, dphi1, out);              \
      case 8 * 16 + 8: return pack_tables<T, 8, 8>(phi0, dphi1, out);              \
      case 8 * 16 + 9: return pack_tables<T, 8, 9>(phi0, dphi1, out);              \
    }                                                                              \
    return -1;                                                                     \
  }
BDX_TABS(double, f64)
BDX_TABS(float, f32)

#define BDX_TABS3(T, SUF)                                                          \
  int bdx_fused3_tables_##SUF BDX_P_FUSED3_TABLES(T) {                             \
    switch (nd * 16 + nq) {                                                        \
      case 2 * 16 + 3: return pack_tables3<T, 2, 3>(phi0, Dd, out);                \
      case 3 * 16 + 4: return pack_tables3<T, 3, 4>(phi0, Dd, out);                \
      case 4 * 16 + 5: return pack_tables3<T, 4, 5>(phi0, Dd, out);                \
      case 5 * 16 + 6: return pack_tables3<T, 5, 6>(phi0, Dd, out);                \
      case 6 * 16 + 7: return pack_tables3<T, 6, 7>(phi0, Dd, out);                \
      case 7 * 16 + 8: return pack_tables3<T, 7, 8>(phi0, Dd, out);                \
      case 8 * 16 + 9: return pack_tables3<T, 8, 9>(phi0, Dd, out);                \
    }                                                                              \
    return -1;                                                                     \
  }
BDX_TABS3(double, f64)
BDX_TABS3(float, f32)

}  // extern "C"
