"""Python front-ends of the native kernels, one per platform with the same
method names: `HipKernels` (torch tensors in, kernels on the current HIP
stream) and `HostKernels`.  Errors are raised loudly (no silent fallback)."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import hip_api, native
from .native import ptr


def _suf(dtype) -> str:
    if dtype == torch.float64:
        return "f64"
    if dtype == torch.float32:
        return "f32"
    raise TypeError(f"unsupported dtype {dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _box(lo, hi):
    """A cell box's corners as int64 arrays (kept alive by the caller)."""
    return np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)


class HipError(RuntimeError):
    pass


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise HipError(f"{what} failed with hipError {rc}")


class TableSet:
    """float64 copies of the 1D tables kept alive for ctypes calls."""

    def __init__(self, tables):
        self.nq = tables.nq
        self.nd = tables.nd
        self.identity = int(tables.is_identity)
        self.phi0 = np.ascontiguousarray(tables.phi0, dtype=np.float64)
        self.dphi1 = np.ascontiguousarray(tables.dphi1, dtype=np.float64)
        self.wts = np.ascontiguousarray(tables.qwts, dtype=np.float64)
        self.qpts = np.ascontiguousarray(tables.qpts, dtype=np.float64)


class HTransferTables:
    """Tables of one h-multigrid level pair (csrc/hip/lap_htransfer.h), on
    `device`: from `fpos[a]`, the fine vertex index of every coarse vertex of
    axis a (strictly increasing from 0 to the last fine vertex),
    cidx[a][i] = the lower coarse neighbour of fine node i, cw[a][i] = the
    weight (i - lo) / (hi - lo) of its upper neighbour, exactly 0 (and cidx =
    the node itself) where i is a coarse node.  The three axes are stored one
    after the other."""

    def __init__(self, fpos, dtype, device):
        cidx, cw, fp = [], [], []
        for f in fpos:
            f = np.asarray(f, dtype=np.int64)
            if f.ndim != 1 or f.size < 1 or f[0] != 0 or np.any(np.diff(f) < 1):
                raise ValueError("fpos must increase strictly from 0")
            i = np.arange(int(f[-1]) + 1)
            lo = np.searchsorted(f, i, side="right") - 1       # f[lo] <= i
            hi = np.minimum(lo + 1, f.size - 1)
            span = np.maximum(f[hi] - f[lo], 1)
            cidx.append(lo)
            cw.append((i - f[lo]) / span)                       # 0 at coarse nodes
            fp.append(f)
        self.Lf = tuple(int(f[-1]) + 1 for f in fp)
        self.Lc = tuple(int(f.size) for f in fp)
        self.fpos_host = fp
        self.cidx = torch.from_numpy(np.concatenate(cidx).astype(np.int32)).to(device)
        self.cw = torch.from_numpy(np.concatenate(cw)).to(device, dtype)
        self.fpos = torch.from_numpy(np.concatenate(fp).astype(np.int32)).to(device)

    def check(self, latd_c, latd_f) -> None:
        """The tables' extents are those of the two lattice descriptors (the
        kernels index the tables by lattice node)."""
        lc, lf = (hip_api.Lattice.from_buffer_copy(d) for d in (latd_c, latd_f))
        if tuple(lc.L) != self.Lc or tuple(lf.L) != self.Lf:
            raise ValueError("h-transfer tables do not belong to this lattice pair")


def stencil27(A, lat) -> np.ndarray:
    """The assembled degree-1 operator `A` (a `CSROperator` on the lattice
    `lat`) as a 27-point stencil S[27][nstore] in the storage index: plane
    (di + 1) 9 + (dj + 1) 3 + (dk + 1) holds row n's entry in the column of
    its lattice neighbour (di, dj, dk); rows of the storage padding are zero.
    Raises if an entry's column is not a lattice neighbour of its row."""
    if lat.degree != 1:
        raise ValueError("stencil27 needs a degree-1 lattice")
    row_ptr, cols, vals = A._host
    L1, L2, ld = int(lat.L[1]), int(lat.L[2]), int(lat.ld)
    rows = np.repeat(np.arange(lat.nstore, dtype=np.int64), np.diff(row_ptr))
    cols = cols.astype(np.int64)
    rk, ck = rows % ld, cols % ld
    ri, ci = rows // ld // L1, cols // ld // L1
    rj, cj = rows // ld % L1, cols // ld % L1
    di, dj, dk = ci - ri, cj - rj, ck - rk
    if np.any(rk >= L2) or np.any(ck >= L2) or np.any(np.abs(di) > 1) or np.any(np.abs(dj) > 1) \
            or np.any(np.abs(dk) > 1):
        raise ValueError("stencil27: a matrix entry is not a lattice neighbour of its row")
    S = np.zeros((27, lat.nstore), dtype=vals.dtype)
    S[(di + 1) * 9 + (dj + 1) * 3 + (dk + 1), rows] = vals
    return S


def _lattice_vectors(shape, dtype, *vecs) -> None:
    """`vecs` (None: absent) are `dtype` vectors of the lattice shape `shape`
    (the kernels index them by lattice node)."""
    for v in vecs:
        if v is not None and (v.dtype != dtype or tuple(v.shape) != tuple(shape)):
            raise TypeError(f"expected a {dtype} lattice vector of shape {tuple(shape)}, "
                            f"got {v.dtype} {tuple(v.shape)}")


def _stencil27_check(lat, dtype, S, *vecs) -> None:
    """S is the (27, nstore) stencil of lattice `lat` and `vecs` its lattice
    vectors, all of `dtype`."""
    if S.dtype != dtype or tuple(S.shape) != (27, lat.nstore) or not S.is_contiguous():
        raise TypeError(f"expected a contiguous {dtype} stencil of shape (27, {lat.nstore}), got "
                        f"{S.dtype} {tuple(S.shape)}")
    _lattice_vectors(lat.shape, dtype, *vecs)


def _stencil27_assemble_check(lat, dtype, xv, kc, S) -> None:
    """S as `_stencil27_check`; xv the lattice's vertices (n + 1 per axis, x 3)
    and kc its per-cell kappa or None, contiguous and of `dtype` (the assembly
    indexes them by cell)."""
    _stencil27_check(lat, dtype, S)
    n = tuple(int(m) for m in lat.n)
    for name, v, shape in (("xv", xv, tuple(m + 1 for m in n) + (3,)), ("kc", kc, n)):
        if v is None and name == "kc":
            continue
        if v is None or v.dtype != dtype or tuple(v.shape) != shape or not v.is_contiguous():
            raise TypeError(f"stencil27_assemble: expected contiguous {dtype} {name} of shape "
                            f"{shape}")


class PmgTail:
    """The device data of the V-cycle tail (csrc/hip/pmg_tail.h): per level of
    `levels` (consecutive degree-1 levels of a `PMultigrid`, the last one its
    coarsest) the 27-point stencil of the assembled operator, and one level
    table (csrc/include/bdx_pmg_tail.h) with every level's descriptor, the
    pointers of its stencil, `dinv`, `bc`, work vectors and transfer tables,
    and its Chebyshev coefficients, kept on the host (`host`, read by the
    launch checks) and on the device (`dev`, read by the kernel).  Everything
    is uploaded here, once; the tensors the table points to are kept alive.
    `assembly`: how the stencils are built (`PoissonProblem.stencil27`)."""

    WORDS = hip_api.CONSTANTS["kTailWords"]
    MAX_NODES = hip_api.CONSTANTS["kTailMaxNodes"]

    def __init__(self, levels, dtype, device, assembly: str = "csr"):
        self.nlev = len(levels)
        self.dtype = dtype
        self.shape = tuple(levels[0].pb.lat.shape)
        W = self.WORDS
        tab = np.zeros(self.nlev * W + 2 * sum(len(lv.coef) for lv in levels), dtype=np.int64)
        words = (hip_api.TailLevelWords * self.nlev).from_buffer(tab)  # the same bytes, by name
        coef = tab.view(np.float64)
        self.S, self._keep = [], []
        off = self.nlev * W
        for l, lv in enumerate(levels):
            S = lv.pb.stencil27(assembly)
            self.S.append(S)
            w = words[l]
            w.lat = hip_api.Lattice.from_buffer_copy(lv.latd)
            vecs = {"S": S, "dinv": lv.dinv, "bc": lv.bc, "r": lv.r, "z": lv.z, "d": lv.d, "y": lv.y}
            if l < self.nlev - 1:
                lv.H.check(levels[l + 1].latd, lv.latd)
                vecs.update(cidx=lv.H.cidx, cw=lv.H.cw, fpos=lv.H.fpos)
            for name, v in vecs.items():
                if name not in ("bc", "cidx", "fpos") and v is not None and v.dtype != dtype:
                    raise TypeError(f"tail level {l}: expected {dtype} data, got {v.dtype}")
                setattr(w, name, ptr(v))
            w.ncoef, w.coef = len(lv.coef), off
            for a, b in lv.coef:
                coef[off], coef[off + 1] = a, b
                off += 2
            self._keep.append(list(vecs.values()))
        del w, words  # the table is plain words from here on
        self.nwords = int(tab.size)
        self.host = tab
        self.dev = torch.from_numpy(tab).to(device)

    def check(self, r, z) -> None:
        _lattice_vectors(self.shape, self.dtype, r, z)


class _Kernels:
    """What the front-ends of the two native libraries share: one problem's
    lattice, tables (None: a front-end for the table-free kernels only) and
    dtype, bound to the library `lib`.  The kernels that platform-neutral
    callers use have the same names and parameters on both
    (tests/test_kernel_frontends.py)."""

    def __init__(self, lib, lat, tables, dtype):
        self.lib = lib
        self.lat = lat
        self.latd = lat.as_int64()
        self.t = None if tables is None else TableSet(tables)
        self.dtype = dtype
        self.suf = _suf(dtype)
        self.o = lat.owned_hi
        self.own = np.asarray(self.o, dtype=np.int64)
        self.rows = (lat.L[1], lat.ld, *self.o)  # the owned-row walk's arguments

    def _f(self, name):
        return getattr(self.lib, f"{name}_{self.suf}")

    def _rows(self, v64=(), v32=()):
        """The row-walk arguments, after checking that the float64 and
        float32 vectors are lattice vectors of those types (the kernels index
        both with one offset)."""
        _lattice_vectors(self.lat.shape, torch.float64, *v64)
        _lattice_vectors(self.lat.shape, torch.float32, *v32)
        return self.rows


class HipKernels(_Kernels):
    """Bound kernel launchers for one problem (lattice + tables + dtype)."""

    def __init__(self, lat, tables, dtype):
        super().__init__(native.hip(), lat, tables, dtype)
        self.npart = self.lib.bdx_hip_partials_size()

    # --------------------------------------------------------------- operator
    def v1_apply(self, mode: int, G, xv, kappa: float, u, y, lo, hi, kc=None):
        lo, hi = _box(lo, hi)
        t = self.t
        _check(self._f("bdx_v1_apply")(mode, ptr(self.latd), t.nq, ptr(t.phi0),
                                       ptr(t.dphi1), ptr(t.wts), ptr(t.qpts), t.identity,
                                       ptr(G), ptr(xv), kappa, ptr(kc), ptr(u), ptr(y), ptr(lo),
                                       ptr(hi), _stream()), "v1_apply")

    def diagonal(self, xv, kappa: float, kc, d, lo, hi):
        """d += matrix-free diag(A) of the cells [lo, hi) (lap_diag.h; Dirichlet
        dofs skipped, no atomics: eight colour launches in a fixed order)."""
        lo, hi = _box(lo, hi)
        t = self.t
        _check(self._f("bdx_diag")(ptr(self.latd), t.nq, ptr(t.phi0), ptr(t.dphi1), ptr(t.wts),
                                   ptr(t.qpts), t.identity, ptr(xv), kappa, ptr(kc), ptr(d),
                                   ptr(lo), ptr(hi), _stream()), "diagonal")

    def dofmap_tables(self, device):
        """Device copy of the 1D tables the dofmap kernels read:
        [phi0 (nq x nd) | dphi1 (nq x nq) | qpts | wts | Dd = dphi1 phi0 (nq x nd) |
        phi0^T | Dd^T] in the vector dtype (Dd and the transposes: the MFMA kernel,
        lap_dofmfma.h)."""
        t = self.t
        dd = np.asarray(t.dphi1, dtype=np.float64) @ np.asarray(t.phi0, dtype=np.float64)
        h = np.concatenate([t.phi0.ravel(), t.dphi1.ravel(), t.qpts.ravel(), t.wts.ravel(),
                            dd.ravel(), np.ascontiguousarray(t.phi0.T).ravel(),
                            np.ascontiguousarray(dd.T).ravel()])
        return torch.from_numpy(h).to(device, self.dtype)

    def dofmap_apply(self, geom: int, tab, cells, ncl: int, cdofs, cverts, coords, flags, G,
                     kappa: float, kc, u, y, mode: int = 0, pold=None, pnew=None, x=None,
                     scal=None, beta=(-1, -1), xa=(-1, -1), partials=None) -> int:
        """mode 0: y += A u; 1: the CG operator (u = r; see lap_dofmap.h).
        Returns the number of p.Ap partials written (CG)."""
        t, P = self.t, self.lat.degree
        nb = ctypes.c_int(0)
        nvec = int(u.numel())
        if nvec * u.element_size() >= 2 ** 32 - 16:
            raise ValueError("dofmap operator: vectors beyond 4 GiB exceed the 32-bit buffer range")
        _check(self._f("bdx_dofmap_apply")(P, t.nq, geom, mode, ptr(tab), ptr(cells), ncl, nvec,
                                           ptr(cdofs), ptr(cverts), ptr(coords), ptr(flags),
                                           ptr(G), kappa, ptr(kc), ptr(u), ptr(pold), ptr(pnew),
                                           ptr(x), ptr(y), ptr(scal), beta[0], beta[1], xa[0],
                                           xa[1], ptr(partials), ctypes.byref(nb), _stream()),
               "dofmap_apply")
        return nb.value

    def dofmap_cg_update(self, flags, r, y, scal, rn_slot: int, pap_slot: int, partials) -> int:
        nb = ctypes.c_int(0)
        _check(self._f("bdx_dofmap_cg_update")(r.numel(), ptr(flags), ptr(r), ptr(y), ptr(scal),
                                               rn_slot, pap_slot, ptr(partials), ctypes.byref(nb),
                                               _stream()), "dofmap_cg_update")
        return nb.value

    def dofmap_xflush(self, x, p, scal, num: int, den: int):
        _check(self._f("bdx_dofmap_xflush")(x.numel(), ptr(x), ptr(p), ptr(scal), num, den,
                                            _stream()), "dofmap_xflush")

    def dofmap_mark_writers(self, cells_a, cells_b, cdofs, nd3: int, ndofs: int):
        first = torch.empty(max(1, ndofs), dtype=torch.int32, device=cdofs.device)
        _check(self.lib.bdx_dofmap_mark_writers(ptr(cells_a), int(cells_a.numel()), ptr(cells_b),
                                                int(cells_b.numel()), ptr(cdofs), nd3, ptr(first),
                                                ndofs, _stream()), "dofmap_mark_writers")

    def reduce_partials(self, partials, n: int, out, slot: int):
        _check(self.lib.bdx_reduce_partials(ptr(partials), n, ptr(out), slot, _stream()),
               "reduce_partials")

    def dofmap_geometry(self, ncells: int, cverts, coords, G):
        t, P = self.t, self.lat.degree
        _check(self._f("bdx_dofmap_geometry")(P, t.nq, ptr(t.phi0), ptr(t.dphi1), ptr(t.wts),
                                              ptr(t.qpts), ncells, ptr(cverts), ptr(coords),
                                              ptr(G), _stream()), "dofmap_geometry")

    def geometry(self, xv, G):
        t = self.t
        _check(self._f("bdx_geometry")(ptr(self.latd), t.nq, ptr(t.phi0), ptr(t.dphi1),
                                       ptr(t.wts), ptr(t.qpts), ptr(xv), ptr(G), _stream()),
               "geometry")

    # ------------------------------------------------------------------ BLAS
    def dot(self, a, b, partials, out, slot: int):
        _check(self._f("bdx_dot")(*self.rows, ptr(a), ptr(b), ptr(partials), ptr(out), slot,
                                  _stream()), "dot")

    def cg_update(self, x, r, p, y, scal, rn_slot, pap_slot, out_slot, partials):
        _check(self._f("bdx_cg_update")(*self.rows, ptr(x), ptr(r), ptr(p), ptr(y), ptr(scal),
                                        rn_slot, pap_slot, out_slot, ptr(partials), _stream()),
               "cg_update")

    def p_update(self, p, r, scal, num, den):
        _check(self._f("bdx_p_update")(*self.rows, ptr(p), ptr(r), ptr(scal), num, den, _stream()),
               "p_update")

    def pcg_update(self, x, r, p, y, dinv, scal, rz_slot, pap_slot, out_slot, rr_slot, partials):
        """Jacobi PCG: alpha = s[rz] / s[pap]; x += alpha p; r -= alpha y;
        s[out] = sum dinv r^2 (the new r.z), s[rr] = sum r^2."""
        _check(self._f("bdx_pcg_update")(*self.rows, ptr(x), ptr(r), ptr(p), ptr(y), ptr(dinv),
                                         ptr(scal), rz_slot, pap_slot, out_slot, rr_slot,
                                         ptr(partials), _stream()), "pcg_update")

    def pcg_p_update(self, p, r, dinv, scal, num, den):
        """p = (s[num] / s[den]) p + dinv . r."""
        _check(self._f("bdx_pcg_p_update")(*self.rows, ptr(p), ptr(r), ptr(dinv), ptr(scal), num,
                                           den, _stream()), "pcg_p_update")

    def axpy(self, out, alpha: float, x, y):
        _check(self._f("bdx_axpy")(*self.rows, ptr(out), float(alpha), ptr(x), ptr(y), _stream()),
               "axpy")

    # --------------------------------------------------------- p-multigrid
    def cheb_step(self, first: bool, a: float, b: float, dinv, r, y, d, z):
        """d = a d + b dinv (r - y); z += d over the owned rows (first: d = z =
        b dinv r, y unused)."""
        _check(self._f("bdx_cheb_step")(*self.rows, int(first), float(a), float(b), ptr(dinv),
                                        ptr(r), ptr(y), ptr(d), ptr(z), _stream()), "cheb_step")

    def prolong(self, latd_c, J, vc, vf):
        """vf = P vc from the coarse lattice `latd_c` to this (fine) lattice;
        J: the (Pf + 1) x (Pc + 1) float64 table (lap_transfer.h)."""
        _check(self._f("bdx_prolong")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vc), ptr(vf),
                                      _stream()), "prolong")

    def restrict(self, latd_c, J, vf, vc):
        """vc += P^T vf (owned fine dofs; vc zeroed by the caller; eight colour
        launches in a fixed order, no atomics)."""
        _check(self._f("bdx_restrict")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vf), ptr(vc),
                                       _stream()), "restrict")

    def prolong_row(self, latd_c, J, vc, vf, add: bool = False):
        """`prolong` by lattice rows (lap_rowtransfer.h): vf = P vc on every
        local fine node, or with `add` vf += P vc on the owned ones."""
        _check(self._f("bdx_prolong_row")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vc), ptr(vf),
                                          int(add), _stream()), "prolong_row")

    def restrict_row(self, latd_c, J, vf, y, vc):
        """vc = P^T (vf - y) over the owned fine nodes (y None: P^T vf), every
        local coarse node written; one launch, no zeroing, no atomics."""
        _check(self._f("bdx_restrict_row")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vf), ptr(y),
                                           ptr(vc), _stream()), "restrict_row")

    def hprolong(self, latd_c, tab: HTransferTables, vc, vf, add: bool = False):
        """h-multigrid: vf = P vc on every node of this (fine, degree-1)
        lattice, or with `add` vf += P vc on its owned nodes (lap_htransfer.h)."""
        tab.check(latd_c, self.latd)
        _check(self._f("bdx_hprolong")(ptr(latd_c), ptr(self.latd), ptr(tab.cidx), ptr(tab.cw),
                                       ptr(tab.fpos), ptr(vc), ptr(vf), int(add), _stream()),
               "hprolong")

    def hrestrict(self, latd_c, tab: HTransferTables, vf, y, vc):
        """h-multigrid: vc = P^T (vf - y) over the owned fine nodes (y None:
        P^T vf), every local coarse node written; one launch, no atomics."""
        tab.check(latd_c, self.latd)
        _check(self._f("bdx_hrestrict")(ptr(latd_c), ptr(self.latd), ptr(tab.cidx), ptr(tab.cw),
                                        ptr(tab.fpos), ptr(vf), ptr(y), ptr(vc), _stream()),
               "hrestrict")

    def stencil27_apply(self, S, u, y):
        """y = S u on every local row of this (degree-1) lattice, ghost rows
        included, with its assembled 27-point stencil S (`stencil27`;
        lap_stencil27.h).  u is forward-exchanged by the caller."""
        _stencil27_check(self.lat, self.dtype, S, u, y)
        _check(self._f("bdx_stencil27_apply")(ptr(self.latd), ptr(S), ptr(u), ptr(y), _stream()),
               "stencil27_apply")

    def stencil27_cheb(self, S, dinv, r, z_in, d, z_out, a: float, b: float):
        """One Chebyshev step in one launch over the owned rows: d = a d + b
        dinv (r - S z_in); z_out = z_in + d (z_out is not z_in); bit for bit
        `stencil27_apply` followed by `cheb_step`."""
        _stencil27_check(self.lat, self.dtype, S, dinv, r, z_in, d, z_out)
        _check(self._f("bdx_stencil27_cheb")(ptr(self.latd), ptr(self.own), ptr(S), ptr(dinv),
                                             ptr(r), ptr(z_in), ptr(d), ptr(z_out), float(a),
                                             float(b), _stream()), "stencil27_cheb")

    def stencil27_assemble(self, xv, kappa: float, kc, S):
        """S = the assembled 27-point stencil of this (degree-1) lattice, every
        entry written (lap_stencil27_assemble.h): `stencil27` of the assembled
        matrix, built on the device from the vertices xv and kappa (kc: per
        cell, or None)."""
        _stencil27_assemble_check(self.lat, self.dtype, xv, kc, S)
        t = self.t
        _check(self._f("bdx_stencil27_assemble")(ptr(self.latd), t.nq, ptr(t.phi0), ptr(t.dphi1),
                                                 ptr(t.wts), ptr(t.qpts), ptr(xv), float(kappa),
                                                 ptr(kc), ptr(S), _stream()), "stencil27_assemble")

    def pmg_tail(self, tail: PmgTail, r, z):
        """z = the V-cycle of the tail's levels applied to r, in one launch of
        one workgroup (pmg_tail.h); r, z: vectors of its first level."""
        tail.check(r, z)
        _check(self._f("bdx_pmg_tail")(ptr(tail.host), ptr(tail.dev), tail.nlev, tail.nwords,
                                       ptr(r), ptr(z), _stream()), "pmg_tail")

    # ------------------------------------- FP64 CG around an FP32 cycle
    def demote(self, a, out):
        """out (float32) = a (float64) over the owned rows, round to nearest even."""
        _check(self.lib.bdx_demote_f64_f32(*self._rows((a,), (out,)), ptr(a), ptr(out), _stream()), "demote")

    def promote(self, a, out):
        """out (float64) = a (float32) over the owned rows (exact)."""
        _check(self.lib.bdx_promote_f32_f64(*self._rows((out,), (a,)), ptr(a), ptr(out), _stream()), "promote")

    def cg_update_demote(self, x, r, p, y, scal, rn_slot, pap_slot, out_slot, partials, r32):
        """`cg_update` in float64 that also stores r32 = (float32) r."""
        _check(self.lib.bdx_cg_update_demote_f64(*self._rows((x, r, p, y), (r32,)), ptr(x), ptr(r),
                                                 ptr(p), ptr(y),
                                                 ptr(scal), rn_slot, pap_slot, out_slot,
                                                 ptr(partials), ptr(r32), _stream()),
               "cg_update_demote")

    def dot_f64_f32(self, a, b32, partials, out, slot: int):
        """out[slot] = sum a (float64) . b32 (float32), b32 promoted in registers."""
        _check(self.lib.bdx_dot_f64_f32(*self._rows((a,), (b32,)), ptr(a), ptr(b32), ptr(partials),
                                        ptr(out), slot, _stream()), "dot_f64_f32")

    def p_update_f64_f32(self, p, z32, scal, num, den):
        """p (float64) = (s[num] / s[den]) p + z32 (float32)."""
        _check(self.lib.bdx_p_update_f64_f32(*self._rows((p,), (z32,)), ptr(p), ptr(z32), ptr(scal),
                                             num, den, _stream()), "p_update_f64_f32")

    def box_copy(self, mode: int, vec, lat, side, buf):
        _check(self._f("bdx_box_copy")(mode, ptr(vec), lat.L[1], lat.ld, ptr(side.table),
                                       len(side.boxes), side.total, ptr(buf), _stream()),
               "box_copy")

    def spmv(self, nrows, beg, end, cols, vals, x, y, acc=False):
        """y[r] (+)= sum of vals[p] x[cols[p]] over p in [beg[r], end[r])."""
        _check(self._f("bdx_spmv")(nrows, ptr(beg), ptr(end), ptr(cols), ptr(vals), ptr(x),
                                   ptr(y), int(acc), _stream()), "spmv")


class HostKernels(_Kernels):
    """The front-end of the host library: `HipKernels`' twin on the CPU
    platform (host tensors or numpy arrays in), and the host-only work of
    either platform (interpolation of f, CSR assembly, the dofmap operator).
    The operator kernels read the 1D tables in the vector dtype (`host_tables`);
    without `tables` only the table-free multigrid kernels can be called."""

    def __init__(self, lat, dtype, tables=None):
        super().__init__(native.host(), lat, tables, dtype)
        npdt = np.float64 if dtype == torch.float64 else np.float32
        self.host_tables = None if tables is None else {
            k: np.ascontiguousarray(v, dtype=npdt) for k, v in dict(
                phi0=tables.phi0, dphi1=tables.dphi1, wts=tables.qwts, qpts=tables.qpts,
                nodes=tables.nodes, B=tables.B, Dd=tables.Dd).items()}

    # --------------------------------------------------------------- operator
    def v1_apply(self, mode: int, G, xv, kappa: float, u, y, lo, hi, kc=None):
        """Over the cells [lo, hi): y += A u with the stored geometry G (mode
        0) or per-point geometry (1); y += M u (2)."""
        lo, hi = _box(lo, hi)
        t, h = self.t, self.host_tables
        tabs = (ptr(self.latd), t.nq, ptr(h["phi0"]), ptr(h["dphi1"]), ptr(h["wts"]), ptr(h["qpts"]),
                ptr(h["nodes"]), t.identity, ptr(xv))
        if mode == 2:
            self._f("bdx_cpu_mass")(*tabs, ptr(u), ptr(y), ptr(lo), ptr(hi))
        else:
            self._f("bdx_cpu_stiffness_g")(*tabs, ptr(G) if mode == 0 else None, kappa, ptr(kc),
                                           ptr(u), ptr(y), ptr(lo), ptr(hi))

    def diagonal(self, xv, kappa: float, kc, d, lo, hi):
        lo, hi = _box(lo, hi)
        t, h = self.t, self.host_tables
        self._f("bdx_cpu_diag")(ptr(self.latd), t.nq, ptr(h["B"]), ptr(h["Dd"]), ptr(h["wts"]),
                                ptr(h["qpts"]), ptr(xv), kappa, ptr(kc), ptr(d), ptr(lo), ptr(hi))

    def geometry(self, xv, G):
        h = self.host_tables
        self._f("bdx_cpu_geometry")(ptr(self.latd), self.t.nq, ptr(h["wts"]), ptr(h["qpts"]),
                                    ptr(xv), ptr(G))

    def spmv(self, nrows, beg, end, cols, vals, x, y, acc=False):
        self._f("bdx_cpu_spmv")(nrows, ptr(beg), ptr(end), ptr(cols), ptr(vals), ptr(x), ptr(y),
                                int(acc))

    def box_copy(self, mode: int, vec, lat, side, buf):
        """Mode 0: buf = the entries of `side`'s boxes in table order; 1: those
        entries = buf; 2: += buf."""
        flat, buf = vec.view(-1), buf[: side.total]
        if mode == 0:
            torch.index_select(flat, 0, side.index, out=buf)
        elif mode == 1:
            flat.index_copy_(0, side.index, buf)
        else:
            flat.index_add_(0, side.index, buf)

    # -------------------------------------------------------------- host only
    def interp_f(self, xv, f):
        """f = the source term at the physical dof nodes, all local points."""
        self._f("bdx_cpu_interp_f")(ptr(self.latd), ptr(self.host_tables["nodes"]), ptr(xv), ptr(f))

    def csr(self, xv, kappa: float, kc, row_ptr, cols=None, vals=None) -> int:
        """The assembled local matrix: without `cols` and `vals` the row counts
        into `row_ptr`, with them the matrix (`row_ptr` zeroed by the caller).
        Returns the number of entries."""
        t, h = self.t, self.host_tables
        return self._f("bdx_cpu_csr")(ptr(self.latd), t.nq, ptr(h["B"]), ptr(h["Dd"]), ptr(h["wts"]),
                                      ptr(h["qpts"]), ptr(xv), kappa, ptr(kc), ptr(row_ptr),
                                      ptr(cols), ptr(vals), int(cols is None))

    def dofmap_apply(self, cells, cdofs, cverts, coords, G, flags, kappa: float, kc, u, y):
        """y += A u over `cells` of the unstructured data model (G None:
        per-point geometry)."""
        t, h = self.t, self.host_tables
        self._f("bdx_cpu_dofmap")(self.lat.degree, t.nq, ptr(h["phi0"]), ptr(h["dphi1"]),
                                  ptr(h["wts"]), ptr(h["qpts"]), t.identity, ptr(cells),
                                  int(cells.size), ptr(cdofs), ptr(cverts), ptr(coords), ptr(G),
                                  ptr(flags), kappa, ptr(kc), ptr(u), ptr(y))

    def dofmap_geometry(self, ncells: int, cverts, coords, G):
        h = self.host_tables
        self._f("bdx_cpu_dofmap_geometry")(self.lat.degree, self.t.nq, ptr(h["wts"]), ptr(h["qpts"]),
                                           ncells, ptr(cverts), ptr(coords), ptr(G))

    # --------------------------------------------------------- p-multigrid
    def cheb_step(self, first: bool, a: float, b: float, dinv, r, y, d, z):
        self._f("bdx_cpu_cheb_step")(*self.rows, int(first), float(a), float(b), ptr(dinv), ptr(r),
                                     ptr(y), ptr(d), ptr(z))

    def prolong(self, latd_c, J, vc, vf):
        if self._f("bdx_cpu_prolong")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vc), ptr(vf)):
            raise ValueError("prolong: lattice pair outside the p-multigrid schedule")

    def restrict(self, latd_c, J, vf, vc):
        if self._f("bdx_cpu_restrict")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vf), ptr(vc)):
            raise ValueError("restrict: lattice pair outside the p-multigrid schedule")

    def prolong_row(self, latd_c, J, vc, vf, add: bool = False):
        if self._f("bdx_cpu_prolong_row")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vc), ptr(vf),
                                          int(add)):
            raise ValueError("prolong_row: lattice pair outside the p-multigrid schedule")

    def restrict_row(self, latd_c, J, vf, y, vc):
        if self._f("bdx_cpu_restrict_row")(ptr(latd_c), ptr(self.latd), ptr(J), ptr(vf), ptr(y),
                                           ptr(vc)):
            raise ValueError("restrict_row: lattice pair outside the p-multigrid schedule")

    def hprolong(self, latd_c, tab: HTransferTables, vc, vf, add: bool = False):
        tab.check(latd_c, self.latd)
        if self._f("bdx_cpu_hprolong")(ptr(latd_c), ptr(self.latd), ptr(tab.cidx), ptr(tab.cw),
                                       ptr(tab.fpos), ptr(vc), ptr(vf), int(add)):
            raise ValueError("hprolong: not a pair of degree-1 lattices of one partition")

    def hrestrict(self, latd_c, tab: HTransferTables, vf, y, vc):
        tab.check(latd_c, self.latd)
        if self._f("bdx_cpu_hrestrict")(ptr(latd_c), ptr(self.latd), ptr(tab.cidx), ptr(tab.cw),
                                        ptr(tab.fpos), ptr(vf), ptr(y), ptr(vc)):
            raise ValueError("hrestrict: not a pair of degree-1 lattices of one partition")

    def pmg_tail(self, tail: PmgTail, r, z):
        tail.check(r, z)
        if self._f("bdx_cpu_pmg_tail")(ptr(tail.host), tail.nlev, tail.nwords, ptr(r), ptr(z)):
            raise ValueError("pmg_tail: not a table of small degree-1 levels of one rank")

    def stencil27(self, S, z, y):
        """y = A z with the 27-point stencil S of this (degree-1) lattice."""
        self._f("bdx_cpu_stencil27")(ptr(self.latd), ptr(S), ptr(z), ptr(y))

    def stencil27_apply(self, S, u, y):
        """`HipKernels.stencil27_apply` on the host twin (`stencil27`, checked)."""
        _stencil27_check(self.lat, self.dtype, S, u, y)
        if self.lat.degree != 1 or u is y:
            raise ValueError("stencil27_apply: not a degree-1 lattice, or y is u")
        self.stencil27(S, u, y)

    def stencil27_cheb(self, S, dinv, r, z_in, d, z_out, a: float, b: float):
        _stencil27_check(self.lat, self.dtype, S, dinv, r, z_in, d, z_out)
        if self._f("bdx_cpu_stencil27_cheb")(ptr(self.latd), ptr(self.own), ptr(S), ptr(dinv),
                                             ptr(r), ptr(z_in), ptr(d), ptr(z_out), float(a),
                                             float(b)):
            raise ValueError("stencil27_cheb: not a degree-1 lattice, or z_out is z_in")

    def stencil27_assemble(self, xv, kappa: float, kc, S):
        """`HipKernels.stencil27_assemble` on the host twin."""
        _stencil27_assemble_check(self.lat, self.dtype, xv, kc, S)
        t = self.t
        if self._f("bdx_cpu_stencil27_assemble")(ptr(self.latd), t.nq, ptr(t.phi0), ptr(t.dphi1),
                                                 ptr(t.wts), ptr(t.qpts), ptr(xv), float(kappa),
                                                 ptr(kc), ptr(S)):
            raise ValueError("stencil27_assemble: not a degree-1 lattice with 2 or 3 quadrature "
                             "points per axis")

    def demote(self, a, out):
        """out (float32) = a (float64) over the owned rows, round to nearest even."""
        self.lib.bdx_cpu_demote_f64_f32(*self._rows((a,), (out,)), ptr(a), ptr(out))

    def promote(self, a, out):
        """out (float64) = a (float32) over the owned rows (exact)."""
        self.lib.bdx_cpu_promote_f32_f64(*self._rows((out,), (a,)), ptr(a), ptr(out))

    def axpy(self, out, alpha: float, x, y):
        o = self.o
        sl = (slice(0, o[0]), slice(0, o[1]), slice(0, o[2]))
        torch.add(y[sl], x[sl], alpha=float(alpha), out=out[sl])


def device_info(dev: int = 0) -> str:
    import ctypes
    lib = native.hip()
    buf = ctypes.create_string_buffer(1024)
    rc = lib.bdx_device_info(dev, buf, 1024)
    if rc != 0:
        return f"(device info unavailable: hipError {rc})\n"
    return buf.value.decode()


def device_name(dev: int = 0) -> str:
    """hipDeviceProp name + gcnArchName (torch's get_device_name() returns a
    generic marketing string on this stack)."""
    info = device_info(dev)
    fields = {}
    for line in info.splitlines():
        key, sep, val = line.partition(":")
        if sep:
            fields[key.strip()] = val.strip()
    name = fields.get("Device", "unknown")
    arch = fields.get("gcnArch", "")
    return f"{name} ({arch})" if arch else name
