"""Plain reference of the Jacobi-preconditioned update pass of the fused CG
loop (csrc/hip/cg_update.hip, bdx_pcg_update_iface_* / bdx_pcg_update_tiled_*),
on top of tests/vector_ref.py:

    r_new = r - alpha (y + interface terms)     on the owned nodes
    z     = dinv * r                            on every 16-byte vector stored
    r.z   = sum double(r_new) double(z)         over the owned nodes
    r.r   = sum double(r_new)^2                 over the owned nodes

Dense (L0, L1, L2) node arrays and explicit storage maps, as in vector_ref.py;
nothing is shared with the kernels.  Used by tests/test_gpu_pcg_update_kernels.py;
self-checked without a GPU by tests/test_pcg_update_ref.py.
"""

from __future__ import annotations

import numpy as np

import vector_ref as vr


def update(r, y, yb, zb, cb, dinv, alpha, g):
    """(r_new, z, mag) on every node, in the arrays' own float type: the r
    update with the folded interface terms, z = dinv * r_new, and the sum of
    the magnitudes behind the fold (for tolerances).  Only the owned nodes of
    r_new and z mean anything: the pass updates nothing else."""
    f, mag = vr.fold(y, yb, zb, cb, g)
    rn = r - alpha * f
    return rn, dinv * rn, mag


def z_of(dinv, r_new):
    """z of stored values: one multiply in the arrays' type (correctly
    rounded, so a kernel's single multiply gives the same bits)."""
    assert dinv.dtype == r_new.dtype
    return dinv * r_new


def scalar_terms(r_new, z):
    """(terms of r.z, terms of r.r) as the kernels form them: products of the
    stored values converted to float64."""
    rd, zd = np.asarray(r_new, dtype=np.float64), np.asarray(z, dtype=np.float64)
    return rd * zd, rd * rd


def stored_elements(g, tiled: bool, W: int) -> np.ndarray:
    """Per storage element: whether the update pass stores the 16-byte vector
    (W elements) that holds it.

    Lattice layout: every vector of the owned rows (i < o0, j < o1), pad
    columns and columns k >= o2 included -- the pass streams whole rows.
    Tiled layout: the vectors that hold at least one owned node."""
    size = g.size(tiled)
    assert size % W == 0
    if not tiled:
        s = np.arange(size)
        row = s // g.ld
        return (row // g.L[1] < g.own[0]) & (row % g.L[1] < g.own[1])
    owned = np.zeros(size, dtype=bool)
    owned[g.map(True)[g.owned_mask()]] = True
    return np.repeat(owned.reshape(-1, W).any(axis=1), W)


# --------------------------------------------------------------- by definition
def update_naive(r, y, yb, zb, cb, dinv, alpha, g):
    """(r_new, z) node by node."""
    f = vr.fold_naive(y, yb, zb, cb, g)
    rn = np.array(r, copy=True)
    z = np.zeros_like(rn)
    L0, L1, L2 = r.shape
    for i in range(L0):
        for j in range(L1):
            for k in range(L2):
                rn[i, j, k] = r[i, j, k] - alpha * f[i, j, k]
                z[i, j, k] = dinv[i, j, k] * rn[i, j, k]
    return rn, z


def stored_elements_naive(g, tiled: bool, W: int) -> np.ndarray:
    """The same set, vector by vector, decoding every storage position back
    to its node by the layouts' definitions (bdx_lattice.h)."""
    size = g.size(tiled)
    L0, L1, L2 = g.L
    o0, o1, o2 = g.own
    out = np.zeros(size, dtype=bool)
    for v in range(size // W):
        keep = False
        for s in range(v * W, (v + 1) * W):
            if tiled:
                tcol = L0 * g.tsy * g.tsz
                t, rest = divmod(s, tcol)
                ty, tz = divmod(t, g.tntz)
                iy, lz = divmod(rest, g.tsz)
                i, ly = divmod(iy, g.tsy)
                j, k = ty * g.tsy + ly, tz * g.tsz + lz
                keep = keep or (i < o0 and j < o1 and k < o2)   # padding: j >= L1 or k >= L2
            else:
                row, _ = divmod(s, g.ld)
                i, j = divmod(row, L1)
                keep = keep or (i < o0 and j < o1)
        out[v * W: (v + 1) * W] = keep
    return out
