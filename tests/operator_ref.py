"""Entry-by-entry reference of the operator action y = A u (CPU only), shared
by tests/test_operator_ref.py and tests/test_gpu_partitioned_operators.py.

A case is one global problem (mesh, degree, quadrature, geometry, kappa).  Its
reference is the one-rank FP64 `MatFreeLaplacianCPU` action on a random global
input, and the error of a result is measured per entry in units of
eps_T . m_i with m = |A| |u| taken from the assembled matrix: the only bound a
rounded sum meets under cancellation, and one that does not grow with the
largest entry of y the way `tol . max|y|` does.
"""

import functools
from typing import NamedTuple

import numpy as np
import torch

import oracle
from benchmark_dolfinx_amd.fem.mesh import cell_coefficients, make_local_lattice, vertex_coordinates
from benchmark_dolfinx_amd.fem.quadrature import OperatorTables

from benchmark_dolfinx_amd.models.poisson import CSROperator, MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.parallel.comm import Comm

EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
NAN = float("nan")
# the CPU operator itself: over ranks within 1.6 eps64 m of one rank's, the FP32
# problem within 10.2 eps32 m of the FP64 one (tests/test_operator_ref.py), the
# CSR and matrix-free FP64 results within 15 eps64 m
K_CPU = 64
# no GPU row may record a ratio above 64, and asserts 10 x its measured one:
# the largest K any test can use, which every planted fault has to exceed
K_CAP = 640
# degrees up to which m = |A| |u| is read off `CSROperator` itself
CSR_MAX_P = 4

# (ranks, partition policy): one rank; x whole (the native runtime's overlap
# layout); a 2 x 2 x 2 grid with all eight ghost patterns
LAYOUTS = [(1, "xyz"), (4, "yz"), (8, "xyz")]
# local blocks (make_local_lattice): (3, 3, 2) at 8/xyz (1,1,1) (1,2,1) (2,1,1)
# (2,2,1), at 4/yz (3,1,1) (3,2,1); (2, 3, 4) at 8/xyz (1,1,2) (1,2,2), at 4/yz
# (2,1,2) (2,2,2); (5, 3, 4) at 4/yz (5,1,2) (5,2,2): an x-march of several
# layers with y and z ghosts
MESHES = [(3, 3, 2), (2, 3, 4), (5, 3, 4)]
SHEAR_MESH = (2, 2, 4)   # power-of-two counts keep the bitwise parallelepiped check


class Case(NamedTuple):
    nc: tuple
    P: int
    qm: int = 1
    pert: float = 0.0
    coef: str = "constant"
    shear: float = 0.0

    def problem(self, comm, dt, platform, partition=None):
        return PoissonProblem(comm, self.nc, self.P, self.qm, False, dt, platform, self.pert,
                              self.coef, self.shear, partition=partition)


class Ref(NamedTuple):
    ug: np.ndarray   # global input, rounded to the vector dtype
    y: np.ndarray    # A ug, one-rank FP64 matrix-free CPU operator
    m: np.ndarray    # |A| |ug| from the assembled matrix


@functools.lru_cache(maxsize=None)
def _host(case):
    """One-rank FP64 CPU problem and its matrix-free operator."""
    cpu = case.problem(Comm(), torch.float64, "cpu")
    return cpu, MatFreeLaplacianCPU(cpu)


def csr_abs_action(case, u_store):
    """|A| |u| in storage order from `CSROperator(cpu)._host`, the assembled
    matrix of the package (its element loop is scalar code: 11 s for the 60
    cells of (5, 3, 4) at P = 7, which is why `abs_action` below exists)."""
    cpu = _host(case)[0]
    row_ptr, cols, vals = CSROperator(cpu)._host
    rows = np.repeat(np.arange(cpu.lat.nstore, dtype=np.int64), np.diff(row_ptr))
    m = np.bincount(rows, weights=np.abs(vals) * np.abs(u_store.ravel()[cols]),
                    minlength=cpu.lat.nstore)
    return m.reshape(cpu.lat.shape)[:, :, : cpu.lat.L[2]].ravel()


@functools.lru_cache(maxsize=None)
def _assembled(case):
    """The same assembled matrix from dense element matrices, one matrix
    product per cell: kappa_c gref^T G gref with the trilinear geometry of
    tests/oracle.py, Dirichlet rows and columns replaced by the identity,
    summed over the cells that share a pair of dofs before the magnitude is
    taken.  Rows are stored as `csr_build` stores them (the box of columns of
    the cells around a node).  Returns (row of every entry, its column,
    |value|) in global lexicographic indices.  Equal to `csr_abs_action` to
    rounding (tests/test_operator_ref.py); a P = 7 case takes a second."""
    t = OperatorTables(case.P, case.qm, False)
    one = make_local_lattice(0, 1, case.nc, case.P)
    n, P, N = case.nc, case.P, one.N
    nd = P + 1
    X = vertex_coordinates(one, case.pert, shear=case.shear)
    kc = cell_coefficients(one, case.coef, oracle.KAPPA)
    gref, _ = oracle._ref_grad_tables(t)                       # (nd^3, nq^3, 3)
    g2 = np.ascontiguousarray(gref.reshape(nd ** 3, -1))
    gq = np.ascontiguousarray(gref.transpose(1, 0, 2))         # (nq^3, nd^3, 3)
    dphi, w3 = t.geometry_dphi(), t.weights3d()
    lo, w = [], []
    for d in range(3):                                         # csr_build's col_range
        i = np.arange(N[d])
        c_hi = np.minimum(i // P, n[d] - 1)
        c_lo = np.where((i % P == 0) & (i > 0), i // P - 1, c_hi)
        lo.append(c_lo * P)
        w.append((c_hi - c_lo + 1) * P + 1)
    cnt = w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]
    row_ptr = np.concatenate([[0], np.cumsum(cnt.ravel())])
    vals = np.zeros(row_ptr[-1])
    cols = np.zeros(row_ptr[-1], dtype=np.int64)
    bc = one.bc_mask()
    li = np.arange(nd)
    for cx in range(n[0]):
        for cy in range(n[1]):
            for cz in range(n[2]):
                cv = np.stack([X[cx + a, cy + b, cz + c] for a in (0, 1) for b in (0, 1)
                               for c in (0, 1)])
                J = np.einsum("vi,jqv->qij", cv, dphi)
                Ji = np.linalg.inv(J)
                G = np.einsum("qid,qjd->qij", Ji, Ji) * (w3 * np.linalg.det(J))[:, None, None]
                kap = oracle.KAPPA if kc is None else kc[cx, cy, cz]
                T = np.matmul(gq, G.transpose(0, 2, 1))          # T[q, b, d] = G[q, d, e] gref[b, q, e]
                Ae = kap * (g2 @ T.transpose(1, 0, 2).reshape(nd ** 3, -1).T)
                gi, gj, gk = np.meshgrid(cx * P + li, cy * P + li, cz * P + li, indexing="ij")
                gi, gj, gk = gi.ravel(), gj.ravel(), gk.ravel()
                on = bc[gi, gj, gk]
                Ae[on, :] = 0.0
                Ae[:, on] = 0.0
                r = (gi * N[1] + gj) * N[2] + gk
                off = (((gi[None, :] - lo[0][gi][:, None]) * w[1][gj][:, None]
                        + (gj[None, :] - lo[1][gj][:, None])) * w[2][gk][:, None]
                       + (gk[None, :] - lo[2][gk][:, None]))
                at = row_ptr[r][:, None] + off
                vals[at] += Ae                                  # distinct entries within a cell
                cols[at] = r[None, :]
    ri, rj, rk = np.nonzero(bc)
    r = (ri * N[1] + rj) * N[2] + rk
    at = row_ptr[r] + ((ri - lo[0][ri]) * w[1][rj] + (rj - lo[1][rj])) * w[2][rk] + (rk - lo[2][rk])
    vals[at], cols[at] = 1.0, r
    rows = np.repeat(np.arange(one.ndofs_global, dtype=np.int64), np.diff(row_ptr))
    return rows, cols, np.abs(vals)


def abs_action(case, ug):
    """m = |A| |ug| on the global lattice."""
    rows, cols, avals = _assembled(case)
    return np.bincount(rows, weights=avals * np.abs(ug[cols]), minlength=ug.size)


@functools.lru_cache(maxsize=None)
def reference(case, dt=torch.float64, seed=3):
    """Ref of `case` for vectors of dtype `dt` (read-only, shared)."""
    cpu, op = _host(case)
    lat = cpu.lat
    ug = np.random.default_rng(seed).standard_normal(lat.ndofs_global)
    ug = torch.from_numpy(ug).to(dt).double().numpy()
    u = cpu.new_vector()
    u[:, :, : lat.L[2]] = torch.from_numpy(ug.reshape(lat.L))
    y = cpu.new_vector()
    op.apply(u, y)
    # from the package's assembled matrix where that is quick, from the dense
    # element matrices above it (tests/test_operator_ref.py compares the two)
    m = csr_abs_action(case, u.numpy()) if case.P <= CSR_MAX_P else abs_action(case, ug)
    assert (m > 0).all()
    out = Ref(ug, cpu.to_global_array(y), m)
    for a in out:
        a.setflags(write=False)
    return out


def local_input(pb, ug):
    """Lattice-shaped vector of `pb`: ug on the owned box, NaN on every ghost
    plane and in the storage padding, so the operator's own forward exchange
    has to fill what it reads."""
    lat, o = pb.lat, pb.lat.owned_hi
    v = np.full(lat.shape, NAN)
    gi = lat.global_indices()[: o[0], : o[1], : o[2]]
    v[: o[0], : o[1], : o[2]] = np.asarray(ug)[gi]
    return torch.from_numpy(v).to(pb.dtype).to(pb.device)


def _ijk(w, N):
    return tuple(int(v) for v in np.unravel_index(w, N))


def ratio(got_global, case, dt):
    """max_i |got_i - y_i| / (eps_T m_i)."""
    ref = reference(case, dt)
    return float((np.abs(np.asarray(got_global) - ref.y) / (EPS[dt] * ref.m)).max())


def check(got_global, case, dt, K):
    """Every entry finite and within K eps_T m_i of the reference; returns the ratio."""
    got = np.asarray(got_global, dtype=np.float64)
    ref = reference(case, dt)
    N = tuple(n * case.P + 1 for n in case.nc)
    bad = np.flatnonzero(~np.isfinite(got))
    assert bad.size == 0, (f"{bad.size} non-finite entries, first at global index {bad[0]} "
                           f"(i, j, k) = {_ijk(bad[0], N)}: {case}")
    r = np.abs(got - ref.y) / (EPS[dt] * ref.m)
    w = int(np.argmax(r))
    assert r[w] <= K, (f"ratio {r[w]:.3e} > K = {K} at global index {w} (i, j, k) = "
                       f"{_ijk(w, N)}: got {float(got[w])!r}, reference {float(ref.y[w])!r}, "
                       f"|A||u| {float(ref.m[w])!r}: {case} {dt}")
    return float(r[w])


# ------------------------------------------------- right-hand side, diagonal
# b = M f sums terms of both signs (the narrow Gaussian f falls by e^-24 across
# one cell of these meshes), so its entries are bounded against the magnitude
# of their terms, (|B|^T W |B| |f|)_i from the numpy oracle.  K_RHS: f =
# 1000 exp(-E) with E = r^2 / 0.02 <= 25; the node coordinates are rounded to
# the vector dtype (dE <= 2 (0.5 u + 0.5 u) / 0.02 = 100 u, u = eps / 2) and E
# takes about four roundings (dE <= 100 u), so df / f <= 100 eps; the two
# sum-factorised passes of the mass action are six dot products of at most 9
# terms and det J about ten operations: 32 eps.  Doubled for the summation
# order and FMA contraction, rounded up to a power of two.
K_RHS = 256
# diag(A) sums the positive quadratic forms of its cells: a relative bound per
# entry, the FP32 value of tests/test_gpu_diagonal.py (2e-5 = 168 eps32) and,
# the kernel being the same code, the same multiple of eps64
K_DIAG = 168


def _mass_action(case, absolute):
    """b = M f before the boundary condition, in numpy on the one-rank mesh:
    B^T (w det J (B f)) per cell, sum-factorised; `absolute`: every factor by
    its magnitude, the sum of the |terms| behind each entry."""
    t = OperatorTables(case.P, case.qm, False)
    one = make_local_lattice(0, 1, case.nc, case.P)
    X = vertex_coordinates(one, case.pert, shear=case.shear)
    n, P = case.nc, case.P
    cv = np.stack([X[a: n[0] + a, b: n[1] + b, c: n[2] + c] for a in (0, 1) for b in (0, 1)
                   for c in (0, 1)], axis=3).reshape(-1, 2, 2, 2, 3)
    lin = lambda x: np.array([1 - x, x])                              # noqa: E731
    dlin = lambda x: np.array([-np.ones_like(x), np.ones_like(x)])     # noqa: E731
    Nn, Nq, Dq = lin(t.nodes), lin(t.qpts), dlin(t.qpts)
    xn = np.einsum("ai,bj,dk,cabde->cijke", Nn, Nn, Nn, cv, optimize=True)
    J = np.stack([np.einsum("ai,bj,dk,cabde->cijke", *[Dq if ax == d else Nq for d in range(3)], cv,
                            optimize=True) for ax in range(3)], axis=-1)
    wdet = np.einsum("i,j,k->ijk", t.qwts, t.qwts, t.qwts)[None] * np.linalg.det(J)
    fe = oracle.f_source(xn[..., 0], xn[..., 1], xn[..., 2])
    B = t.B
    if absolute:
        B, wdet, fe = np.abs(B), np.abs(wdet), np.abs(fe)
    be = np.einsum("xi,yj,zk,cxyz->cijk", B, B, B,
                   np.einsum("xi,yj,zk,cijk->cxyz", B, B, B, fe, optimize=True) * wdet,
                   optimize=True)
    cx, cy, cz = (a.ravel() for a in np.meshgrid(*(np.arange(m) for m in n), indexing="ij"))
    li = np.arange(P + 1)
    N = one.N
    dofs = (((cx[:, None] * P + li)[:, :, None, None] * N[1]
             + (cy[:, None] * P + li)[:, None, :, None]) * N[2]
            + (cz[:, None] * P + li)[:, None, None, :])
    out = np.zeros(one.ndofs_global)
    np.add.at(out, dofs.ravel(), be.ravel())
    return out


@functools.lru_cache(maxsize=None)
def rhs_reference(case):
    """(b, magnitude of b's terms) of `case`: the one-rank FP64 host
    right-hand side and the numpy model's sum of |terms| (global arrays,
    read-only)."""
    cpu = _host(case)[0]
    b = cpu.to_global_array(cpu.assemble_rhs())
    mag = _mass_action(case, True)
    bc = cpu.lat.bc_mask().ravel()
    # the host twin and the model, two FP64 evaluations, agree far inside the bound
    model = np.where(bc, 0.0, _mass_action(case, False))
    assert (np.abs(b - model) <= 64 * EPS[torch.float64] * mag).all()
    for a in (b, mag):
        a.setflags(write=False)
    return b, mag


def check_rhs(got_global, case, dt):
    """Dirichlet entries exactly zero, every other entry within K_RHS eps_T of
    its terms' magnitude; returns the largest ratio."""
    b, mag = rhs_reference(case)
    got = np.asarray(got_global, dtype=np.float64)
    bc = make_local_lattice(0, 1, case.nc, case.P).bc_mask().ravel()
    assert np.isfinite(got).all() and (got[bc] == 0).all()
    r = np.abs(got - b)[~bc] / (EPS[dt] * mag[~bc])
    assert r.max() <= K_RHS, f"rhs ratio {r.max():.3e} > {K_RHS}: {case} {dt}"
    return float(r.max())


def check_diagonal(got_global, host_diagonal, dt):
    """Relative error per entry against the FP64 host diagonal (positive)."""
    rel = np.abs(np.asarray(got_global) - host_diagonal) / host_diagonal
    assert np.isfinite(rel).all() and rel.max() <= K_DIAG * EPS[dt], \
        f"diagonal: relative error {rel.max():.3e} > {K_DIAG} eps"
    return float(rel.max() / EPS[dt])
