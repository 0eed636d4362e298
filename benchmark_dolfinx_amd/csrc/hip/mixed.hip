// The precision boundary of the mixed-precision multigrid solve (gfx950): an
// FP64 CG loop around an FP32 V-cycle (solvers/pmg.py, cycle_dtype=float32).
//
//   * demote / promote: out = (float)a, out = (double)a over the owned rows
//     (plain C++ conversions: round to nearest even, promotion exact);
//   * cg_update_demote: bdx_cg_update_f64 that also stores the new residual
//     demoted, one extra 4-byte store per dof instead of a separate pass;
//   * dot_f64_f32, p_update_f64_f32: dot and p_update reading the FP32 z and
//     promoting it in registers, so the FP64 z never exists on the device.
//
// Every kernel walks the owned sub-box one z-row per wave like blas.hip and
// touches no entry outside it; the storage pitch is 16 elements in both
// precisions, so one index serves both vectors of a node.  The three fused
// entry points launch further instances of the kernel templates that blas.hip
// instantiates (blas_rows.h: cg_update_kernel<double, true>,
// dot_rows_kernel<double, float>, p_update_kernel<double, float>) and reduce
// with its final pass, so they reproduce the composition of the existing
// kernels bit for bit.
#include "blas_rows.h"

namespace {

using bdx_rows::for_each_owned;
using bdx_rows::grid_for_rows;
using bdx_rows::kBlock;
using bdx_rows::RowSpace;

// out = (TO)a over the owned rows.
template <typename TI, typename TO>
__global__ void __launch_bounds__(kBlock)
    convert_rows_kernel(RowSpace s, const TI* __restrict__ a, TO* __restrict__ out) {
  for_each_owned(s, [&](int64_t i) { out[i] = static_cast<TO>(a[i]); });
}

}  // namespace

extern "C" {

// out = (float)a over the owned rows (round to nearest even).
int bdx_demote_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                       const double* a, float* out, hipStream_t st) {
  RowSpace s{L1, ld, o0, o1, o2};
  convert_rows_kernel<double, float><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(s, a, out);
  return static_cast<int>(hipGetLastError());
}

// out = (double)a over the owned rows (exact).
int bdx_promote_f32_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                        const float* a, double* out, hipStream_t st) {
  RowSpace s{L1, ld, o0, o1, o2};
  convert_rows_kernel<float, double><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(s, a, out);
  return static_cast<int>(hipGetLastError());
}

// bdx_cg_update_f64 (alpha = s[rn] / s[pap]; x += alpha p; r -= alpha y; r.r
// into s[out_slot]) with r32 = (float)r stored in the same pass.
int bdx_cg_update_demote_f64(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2,
                             double* x, double* r, const double* p, const double* y,
                             double* scal, int rn_slot, int pap_slot, int out_slot,
                             double* partials, float* r32, hipStream_t st) {
  RowSpace s{L1, ld, o0, o1, o2};
  const int g = grid_for_rows(o0 * o1);
  bdx_rows::cg_update_kernel<double, true><<<g, kBlock, 0, st>>>(s, x, r, p, y, scal, rn_slot,
                                                                 pap_slot, partials, r32);
  return bdx_reduce_partials(partials, g, scal, out_slot, st);
}

// out[slot] = sum over the owned rows of a (double)b32: the block partition
// and final pass of bdx_dot_f64.
int bdx_dot_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, const double* a,
                    const float* b32, double* partials, double* out, int slot,
                    hipStream_t st) {
  RowSpace s{L1, ld, o0, o1, o2};
  const int g = grid_for_rows(o0 * o1);
  bdx_rows::dot_rows_kernel<double, float><<<g, kBlock, 0, st>>>(s, a, b32, partials);
  return bdx_reduce_partials(partials, g, out, slot, st);
}

// p = (s[num] / s[den]) p + (double)z32 over the owned rows.
int bdx_p_update_f64_f32(int64_t L1, int64_t ld, int64_t o0, int64_t o1, int64_t o2, double* p,
                         const float* z32, const double* scal, int num, int den,
                         hipStream_t st) {
  RowSpace s{L1, ld, o0, o1, o2};
  bdx_rows::p_update_kernel<double, float><<<grid_for_rows(o0 * o1), kBlock, 0, st>>>(
      s, p, z32, scal, num, den);
  return static_cast<int>(hipGetLastError());
}

}  // extern "C"
