// The owned-row walk of the device BLAS-1 kernels, and the kernels that
// blas.hip and mixed.hip both instantiate.  `for_each_owned` is the one place
// that knows the walk: the owned sub-box of the local lattice, one z-row per
// wave, rows by grid stride and entries by lane stride (rows are 128-byte
// aligned by the storage pitch, which is 16 elements in both precisions, so
// one storage index serves the FP64 and the FP32 vector of a node).  A kernel
// of mixed.hip that must reproduce a kernel of blas.hip bit for bit is another
// instance of the same template here.
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

// f(i) for the storage index i of every owned entry that falls to this
// thread, in a fixed order: rows by grid stride, entries by lane stride.
template <typename F>
__device__ __forceinline__ void for_each_owned(const RowSpace& s, F&& f) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t nrows = s.o0 * s.o1;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wid; row < nrows;
       row += static_cast<int64_t>(gridDim.x) * kWaves) {
    const int64_t base = row_base(s, row);
    for (int64_t k = lane; k < s.o2; k += 64) f(base + k);
  }
}

// Per-block partial sums of a.b in double (deterministic order), either
// operand promoted in registers.
template <typename TA, typename TB>
__global__ void __launch_bounds__(kBlock)
    dot_rows_kernel(RowSpace s, const TA* __restrict__ a, const TB* __restrict__ b,
                    double* __restrict__ partials) {
  __shared__ double lds[16];
  double acc = 0.0;
  for_each_owned(s, [&](int64_t i) {
    acc += static_cast<double>(a[i]) * static_cast<double>(b[i]);
  });
  const double t = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// CG: alpha = s[rn] / s[pap];  x += alpha p;  r -= alpha y;  partial r.r.
// DEMOTE: the new residual is also stored rounded to float in r32 (same index).
template <typename T, bool DEMOTE>
__global__ void __launch_bounds__(kBlock)
    cg_update_kernel(RowSpace s, T* __restrict__ x, T* __restrict__ r,
                     const T* __restrict__ p, const T* __restrict__ y,
                     const double* __restrict__ scal, int rn_slot, int pap_slot,
                     double* __restrict__ partials, float* __restrict__ r32) {
  __shared__ double lds[16];
  const T alpha = static_cast<T>(scal[rn_slot] / scal[pap_slot]);
  double acc = 0.0;
  for_each_owned(s, [&](int64_t i) {
    x[i] = x[i] + alpha * p[i];
    const T rn = r[i] - alpha * y[i];
    r[i] = rn;
    if constexpr (DEMOTE) r32[i] = static_cast<float>(rn);
    acc += static_cast<double>(rn) * static_cast<double>(rn);
  });
  const double t = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// p = beta p + z with beta = s[num] / s[den] (owned rows), z converted to T.
template <typename T, typename TZ>
__global__ void __launch_bounds__(kBlock)
    p_update_kernel(RowSpace s, T* __restrict__ p, const TZ* __restrict__ z,
                    const double* __restrict__ scal, int num, int den) {
  const T beta = static_cast<T>(scal[num] / scal[den]);
  for_each_owned(s, [&](int64_t i) { p[i] = beta * p[i] + static_cast<T>(z[i]); });
}

}  // namespace bdx_rows
