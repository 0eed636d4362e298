// Shared (host + device) geometry factor of a trilinear hexahedron: the
// expressions of the device kernels' geometry_G (csrc/hip/bdx_common.h, which
// forwards here), so that a host twin that includes this header evaluates the
// same terms in the same order.
#pragma once
#include "bdx_lattice.h"

// Trilinear geometry at reference point (s, t, u) of the cell with vertices
// X (v = 4a+2b+c): returns det J and writes G = w adj(J) adj(J)^T / det J.
template <typename T>
BDX_HD T trilinear_G(const T (*X)[3], T s, T t, T u, T w, T G[6]) {
  T J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    // d x_i / d s = sum over the 4 edges in s of (x_hi - x_lo) * bilinear(t, u)
    const T e00 = X[4][i] - X[0][i], e01 = X[5][i] - X[1][i];
    const T e10 = X[6][i] - X[2][i], e11 = X[7][i] - X[3][i];
    J[i][0] = (1 - t) * ((1 - u) * e00 + u * e01) + t * ((1 - u) * e10 + u * e11);
    const T f00 = X[2][i] - X[0][i], f01 = X[3][i] - X[1][i];
    const T f10 = X[6][i] - X[4][i], f11 = X[7][i] - X[5][i];
    J[i][1] = (1 - s) * ((1 - u) * f00 + u * f01) + s * ((1 - u) * f10 + u * f11);
    const T g00 = X[1][i] - X[0][i], g01 = X[3][i] - X[2][i];
    const T g10 = X[5][i] - X[4][i], g11 = X[7][i] - X[6][i];
    J[i][2] = (1 - s) * ((1 - t) * g00 + t * g01) + s * ((1 - t) * g10 + t * g11);
  }
  const T K00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const T K01 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
  const T K02 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  const T K10 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const T K11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  const T K12 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
  const T K20 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const T K21 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
  const T K22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  const T det = J[0][0] * K00 + J[0][1] * K10 + J[0][2] * K20;
  const T sc = w / det;
  G[0] = (K00 * K00 + K01 * K01 + K02 * K02) * sc;
  G[1] = (K10 * K00 + K11 * K01 + K12 * K02) * sc;
  G[2] = (K20 * K00 + K21 * K01 + K22 * K02) * sc;
  G[3] = (K10 * K10 + K11 * K11 + K12 * K12) * sc;
  G[4] = (K20 * K10 + K21 * K11 + K22 * K12) * sc;
  G[5] = (K20 * K20 + K21 * K21 + K22 * K22) * sc;
  return det;
}
