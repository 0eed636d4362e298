"""Plain references of the CG runtime's vector kernels (csrc/hip/blas.hip,
csrc/hip/cg_update.hip, the finalize kernels of csrc/hip/lap_fused.h).

Everything here works on dense (L0, L1, L2) node arrays and on explicit
storage maps; nothing is shared with the kernels.  The array functions use
only slicing and arithmetic, so they take numpy arrays (any float type; the
tests pass np.longdouble so that the reference's own rounding is far below
the kernels') or torch tensors (the one large case, on the device).

Used by tests/test_gpu_vector_kernels.py; self-checked without a GPU by
tests/test_vector_ref.py.
"""

from __future__ import annotations

import math

import numpy as np

from benchmark_dolfinx_amd.fem.mesh import LocalLattice

U53 = 2.0 ** -53  # unit roundoff of the float64 accumulations


def make_lattice(P, n, gh, lower=False) -> LocalLattice:
    """One rank's lattice with `n` local cells and ghost planes `gh`, built
    directly (no communicator).  lower: give the rank a lower neighbour on
    every axis too, so that it has halo send boxes as well as ghost boxes."""
    r = 1 if lower else 0
    pgrid = tuple(r + 1 + int(bool(g)) for g in gh)
    rcoord = (r, r, r)
    ncg = tuple(m * p for m, p in zip(n, pgrid))
    c0 = tuple(m * r for m in n)
    c1 = tuple(a + m for a, m in zip(c0, n))
    lat = LocalLattice(0, int(np.prod(pgrid)), P, ncg, pgrid, rcoord, c0, c1)
    assert lat.gh == tuple(int(bool(g)) for g in gh) and lat.n == tuple(n)
    return lat


class Geom:
    """A lattice with a kernel tile of TY x TZ cells: the interface geometry
    (as models/fused.py sizes it) and both storage layouts."""

    def __init__(self, P, tile, n, gh=(0, 0, 0), lower=False):
        self.lat = lat = make_lattice(P, n, gh, lower)
        self.P, (self.TY, self.TZ) = P, tile
        self.sy = self.tsy = self.TY * P
        self.sz = self.tsz = self.TZ * P
        self.nty = max(1, math.ceil(lat.n[1] / self.TY))
        self.ntz = max(1, math.ceil(lat.n[2] / self.TZ))
        self.L = lat.L
        self.own = lat.owned_hi
        self.ld = lat.ld
        self.tnty = (lat.L[1] - 1) // self.tsy + 1   # storage tiles
        self.tntz = (lat.L[2] - 1) // self.tsz + 1
        self.lat_size = lat.nstore
        self.til_size = lat.tiled_size(self.tsy, self.tsz)
        self.latd = lat.as_int64()
        self.latd_tiled = lat.as_int64(tile=(self.tsy, self.tsz))
        L0, L1, L2 = lat.L
        self.yb_shape = (L0, self.nty - 1, L2)
        self.zb_shape = (L0, self.ntz - 1, L1)
        self.cb_shape = (L0, self.nty - 1, self.ntz - 1)

    def size(self, tiled: bool) -> int:
        return self.til_size if tiled else self.lat_size

    def desc(self, tiled: bool) -> np.ndarray:
        return self.latd_tiled if tiled else self.latd

    def map(self, tiled: bool) -> np.ndarray:
        return tiled_map(self.lat, self.tsy, self.tsz) if tiled else lattice_map(self.lat)

    def owned_mask(self) -> np.ndarray:
        i, j, k = np.ogrid[: self.L[0], : self.L[1], : self.L[2]]
        return (i < self.own[0]) & (j < self.own[1]) & (k < self.own[2])

    def iface_masks(self):
        """(on a y-interface row, on a z-interface column) per node."""
        _, j, k = np.ogrid[: self.L[0], : self.L[1], : self.L[2]]
        my = (j % self.sy == 0) & (j // self.sy >= 1) & (j // self.sy < self.nty)
        mz = (k % self.sz == 0) & (k // self.sz >= 1) & (k // self.sz < self.ntz)
        full = np.ones(self.L, dtype=bool)
        return my & full, mz & full

    def iface_owned(self):
        """Per entry of yb, zb, cb: whether the node it belongs to is owned."""
        o0, o1, o2 = self.own
        L0, L1, L2 = self.L
        ix = (np.arange(L0) < o0)
        ya = ((np.arange(1, self.nty) * self.sy) < o1)
        zb_ = ((np.arange(1, self.ntz) * self.sz) < o2)
        yb = ix[:, None, None] & ya[None, :, None] & (np.arange(L2) < o2)[None, None, :]
        zb = ix[:, None, None] & zb_[None, :, None] & (np.arange(L1) < o1)[None, None, :]
        cb = ix[:, None, None] & ya[None, :, None] & zb_[None, None, :]
        return yb, zb, cb


def lattice_map(lat) -> np.ndarray:
    """Storage index of node (i, j, k) in the lattice layout."""
    i, j, k = np.ogrid[: lat.L[0], : lat.L[1], : lat.L[2]]
    return ((i * lat.L[1] + j) * lat.ld + k).astype(np.int64)


def tiled_map(lat, tsy, tsz) -> np.ndarray:
    """Storage index of node (i, j, k) in the tiled layout (bdx_lattice.h)."""
    i, j, k = np.ogrid[: lat.L[0], : lat.L[1], : lat.L[2]]
    tntz = (lat.L[2] - 1) // tsz + 1
    tcol = lat.L[0] * tsy * tsz
    return (((j // tsy) * tntz + k // tsz) * tcol + (i * tsy + j % tsy) * tsz
            + k % tsz).astype(np.int64)


def _swap12(a):
    return a.transpose(0, 2, 1) if isinstance(a, np.ndarray) else a.permute(0, 2, 1)


def iface_sum(like, yb, zb, cb, g):
    """Dense array of the interface terms of every node: yb[i, ty-1, k] on the
    rows j = ty sy, zb[i, tz-1, j] on the columns k = tz sz, cb on both."""
    add = np.zeros_like(like) if isinstance(like, np.ndarray) else like.new_zeros(like.shape)
    js = slice(g.sy, (g.nty - 1) * g.sy + 1, g.sy)
    ks = slice(g.sz, (g.ntz - 1) * g.sz + 1, g.sz)
    add[:, js, :] += yb
    add[:, :, ks] += _swap12(zb)
    add[:, js, ks] += cb
    return add


def fold(y, yb, zb, cb, g):
    """(y + interface terms, sum of the terms' magnitudes) per node."""
    return y + iface_sum(y, yb, zb, cb, g), abs(y) + iface_sum(y, abs(yb), abs(zb), abs(cb), g)


def fold_naive(y, yb, zb, cb, g):
    """The same by the definition, node by node."""
    out = np.array(y, copy=True)
    L0, L1, L2 = y.shape
    for i in range(L0):
        for j in range(L1):
            for k in range(L2):
                ty, tz = j // g.sy, k // g.sz
                oy = j % g.sy == 0 and 1 <= ty < g.nty
                oz = k % g.sz == 0 and 1 <= tz < g.ntz
                t = y[i, j, k]
                if oy:
                    t = t + yb[i, ty - 1, k]
                if oz:
                    t = t + zb[i, tz - 1, j]
                if oy and oz:
                    t = t + cb[i, ty - 1, tz - 1]
                out[i, j, k] = t
    return out


def tile_colour(g) -> np.ndarray:
    """(ty + tz) & 1 of the storage tile of every node."""
    _, j, k = np.ogrid[: g.L[0], : g.L[1], : g.L[2]]
    return ((j // g.tsy + k // g.tsz) & 1) + np.zeros(g.L, dtype=np.int64)


def coefficient(scal, num, den, dtype):
    """a = scal[num] / scal[den] (den < 0: scal[num]), rounded to `dtype`."""
    a = np.float64(scal[num]) if den < 0 else np.float64(scal[num]) / np.float64(scal[den])
    return dtype(a)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------------
# Lengths of the longest chain of float64 additions behind one reduction
# result, from the launch shapes in the sources.  Every term is >= 0 (or the
# bound is taken against the sum of magnitudes), so the relative error of the
# result is at most chain * 2^-53 to first order.

def chain_block(per_thread: int) -> int:
    """One 256-thread block: the thread's serial adds, 6 wave shuffle steps,
    4 adds of the wave sums (block_sum, bdx_common.h)."""
    return per_thread + 6 + 4


def chain_final(g: int, two_stage_above: int | None = None) -> int:
    """Sum of g block partials: one block (ceil(g / 256) serial adds per
    thread), or, above the threshold, 256 slices of ceil(g / 256) partials
    (one block each) followed by one block over the 256 slice sums."""
    if two_stage_above is not None and g > two_stage_above:
        per = cdiv(g, 256)
        return chain_block(cdiv(per, 256)) + chain_block(1)
    return chain_block(cdiv(g, 256))


def sum_hi(values) -> float:
    """Correctly rounded sum of a float array."""
    return math.fsum(np.asarray(values, dtype=np.float64).ravel().tolist())
