// Row walk of the device BLAS-1 kernels and the loop bodies that blas.hip and
// mixed.hip share: the owned sub-box of the local lattice, one z-row per wave
// (rows are 128-byte aligned by the storage pitch, which is 16 elements in
// both precisions, so one index serves the FP64 and the FP32 vector of a
// node).  A kernel of mixed.hip that must reproduce a kernel of blas.hip bit
// for bit instantiates the same body here.
#pragma once
#include "bdx_common.h"

namespace bdx_rows {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct RowSpace {
  int64_t L1, ld;       // storage strides
  int64_t o0, o1, o2;   // owned extents
};

__device__ __forceinline__ int64_t row_base(const RowSpace& s, int64_t row) {
  const int64_t i = row / s.o1, j = row - i * s.o1;
  return (i * s.L1 + j) * s.ld;
}

// Blocks of kWaves rows, capped: beyond the cap the kernels stride the grid.
inline int grid_for_rows(int64_t nrows) {
  const int64_t want = (nrows + kWaves - 1) / kWaves;
  return static_cast<int>(want < 2048 ? (want > 0 ? want : 1) : 2048);
}

// This thread's share of a.b in double (fixed order: rows by grid stride,
// entries by lane stride).
template <typename TA, typename TB>
__device__ __forceinline__ double dot_rows(const RowSpace& s, const TA* __restrict__ a,
                                           const TB* __restrict__ b) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t nrows = s.o0 * s.o1;
  double acc = 0.0;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wid; row < nrows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {
    const int64_t base = row_base(s, row);
    for (int64_t k = lane; k < s.o2; k += 64)
      acc += static_cast<double>(a[base + k]) * static_cast<double>(b[base + k]);
  }
  return acc;
}

// x += alpha p;  r -= alpha y;  returns this thread's share of r.r.  DEMOTE:
// the new residual is also stored rounded to float in r32 (same index).
template <typename T, bool DEMOTE>
__device__ __forceinline__ double cg_update_rows(const RowSpace& s, T alpha, T* __restrict__ x,
                                                 T* __restrict__ r, const T* __restrict__ p,
                                                 const T* __restrict__ y,
                                                 float* __restrict__ r32) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t nrows = s.o0 * s.o1;
  double acc = 0.0;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wid; row < nrows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {
    const int64_t base = row_base(s, row);
    for (int64_t k = lane; k < s.o2; k += 64) {
      const int64_t i = base + k;
      x[i] = x[i] + alpha * p[i];
      const T rn = r[i] - alpha * y[i];
      r[i] = rn;
      if constexpr (DEMOTE) r32[i] = static_cast<float>(rn);
      acc += static_cast<double>(rn) * static_cast<double>(rn);
    }
  }
  return acc;
}

// p = beta p + z over the owned rows, z converted to T.
template <typename T, typename TZ>
__device__ __forceinline__ void p_update_rows(const RowSpace& s, T beta, T* __restrict__ p,
                                              const TZ* __restrict__ z) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t nrows = s.o0 * s.o1;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wid; row < nrows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {
    const int64_t base = row_base(s, row);
    for (int64_t k = lane; k < s.o2; k += 64)
      p[base + k] = beta * p[base + k] + static_cast<T>(z[base + k]);
  }
}

}  // namespace bdx_rows
