"""p-multigrid preconditioned CG on the CPU path: the host twins of the
transfer kernels and of `cheb_step` against dense numpy models, the V-cycle's
symmetry, `cg_solve(precond=pmg.apply)` against a numpy PCG on dense level
matrices, convergence against Jacobi-PCG, and the `--precond pmg` CLI.

Per-entry bound of a transfer (used throughout): each of the three 1D passes
is a dot product of at most 2 Pf + 1 terms, so
    |err_i| <= 2 . 3 (2 Pf + 1) eps_T (|J| (x) |J| (x) |J| . |v|)_i,
the factor 2 covering another summation order and FMA contraction."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from benchmark_dolfinx_amd.fem.mesh import (_hash_uniform, cell_coefficients, make_local_lattice,
                                            vertex_coordinates)
from benchmark_dolfinx_amd.fem.quadrature import OperatorTables, gll, lagrange_tables
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops.kernels import HostKernels
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid, chebyshev_coefficients, level_degrees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, 3)]
CELLS = [(2, 3, 2), (1, 1, 1)]
DTYPES = [torch.float64, torch.float32]
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
NAN = float("nan")


# ------------------------------------------------------------ dense model
def axis_matrix(n, Pf, Pc):
    """Global 1D interpolation matrix (n Pf + 1) x (n Pc + 1): J placed per cell."""
    J, _ = lagrange_tables(gll(Pc + 1)[0], gll(Pf + 1)[0])
    G = np.zeros((n * Pf + 1, n * Pc + 1))
    for c in range(n):
        G[c * Pf: c * Pf + Pf + 1, c * Pc: c * Pc + Pc + 1] = J
    return G


def along_axes(mats, v):
    """(M0 (x) M1 (x) M2) v for a 3D array v."""
    v = np.tensordot(mats[0], v, axes=(1, 0))
    v = np.moveaxis(np.tensordot(mats[1], v, axes=(1, 1)), 0, 1)
    return np.moveaxis(np.tensordot(mats[2], v, axes=(1, 2)), 0, 2)


def model_prolong(nc, Pf, Pc, vc):
    """(exact P vc, per-entry bound / eps) on global 3D arrays."""
    G = [axis_matrix(n, Pf, Pc) for n in nc]
    return along_axes(G, vc), 6 * (2 * Pf + 1) * along_axes([np.abs(g) for g in G], np.abs(vc))


def model_restrict(nc, Pf, Pc, vf):
    G = [axis_matrix(n, Pf, Pc).T for n in nc]
    return along_axes(G, vf), 6 * (2 * Pf + 1) * along_axes([np.abs(g) for g in G], np.abs(vf))


def _shape(nc, P):
    return tuple(n * P + 1 for n in nc)


def _fill(pb, glob, fill=NAN):
    """Lattice-shaped vector holding the global array `glob` on every local
    node (ghost planes included) and `fill` in the storage padding."""
    v = np.full(pb.lat.shape, fill, dtype=np.float64)
    v[:, :, : pb.lat.L[2]] = glob.ravel()[pb.lat.global_indices()]
    return torch.from_numpy(v).to(pb.dtype).to(pb.device)


def _glob(pb, v):
    return pb.to_global_array(v).reshape(pb.lat.N)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _problem(nc, P, dt=torch.float64, pert=0.0, coef="constant", comm=None, platform="cpu"):
    return PoissonProblem(comm or Comm(), nc, P, 1, False, dt, platform, pert, coef)


@functools.lru_cache(maxsize=None)
def _pmg(nc, Pf, dt):
    return PMultigrid(_problem(nc, Pf, dt))


def _random(shape, seed, dt):
    """Random global array, rounded to the vector dtype (so the model sees the
    values the kernel sees)."""
    v = np.random.default_rng(seed).standard_normal(shape)
    return torch.from_numpy(v).to(dt).double().numpy()


# -------------------------------------------------- 1. transfers vs model
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", CELLS)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_prolong_vs_dense_model(Pf, Pc, nc, dt):
    pmg = _pmg(nc, Pf, dt)
    assert pmg.degrees[:2] == [Pf, Pc]
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    gc = _random(_shape(nc, Pc), 3, dt)
    vc = _fill(coarse, gc)                               # NaN in the coarse padding
    vf0 = torch.full(fine.lat.shape, NAN, dtype=dt)      # never read, written once
    vf = vf0.clone()
    pmg.prolong(0, vc, vf)
    L2 = fine.lat.L[2]
    assert torch.isfinite(vf[:, :, :L2]).all()
    assert torch.equal(_bits(vf[:, :, L2:]), _bits(vf0[:, :, L2:]))   # outside the lattice
    ref, bnd = model_prolong(nc, Pf, Pc, gc)
    err = np.abs(_glob(fine, vf) - ref)
    print(f"prolong {Pc}->{Pf} {nc} {dt}: max err / bound {(err / (EPS[dt] * bnd)).max():.3e}")
    assert (err <= EPS[dt] * bnd).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", CELLS)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_restrict_vs_dense_model(Pf, Pc, nc, dt):
    pmg = _pmg(nc, Pf, dt)
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    gf = _random(_shape(nc, Pf), 5, dt)
    vf = _fill(fine, gf)                                 # NaN in the fine padding
    vf0 = vf.clone()
    vc = torch.full(coarse.lat.shape, NAN, dtype=dt)     # zeroed by restrict()
    pmg.restrict(0, vf, vc)
    assert torch.equal(_bits(vf), _bits(vf0))
    ref, bnd = model_restrict(nc, Pf, Pc, gf)
    bc = coarse.lat.bc_mask()
    ref[bc] = 0.0                                        # Dirichlet entries are zeroed
    got = _glob(coarse, vc)
    assert np.isfinite(got).all() and (got[bc] == 0).all()
    err = np.abs(got - ref)
    print(f"restrict {Pf}->{Pc} {nc} {dt}: max err / bound {(err / (EPS[dt] * bnd)).max():.3e}")
    assert (err <= EPS[dt] * bnd).all()
    vc2 = torch.full(coarse.lat.shape, NAN, dtype=dt)
    pmg.restrict(0, vf, vc2)
    assert torch.equal(_bits(vc), _bits(vc2))            # bitwise reproducible


def test_raw_restrict_keeps_dirichlet_sums_and_rejects_bad_pairs():
    """The kernel itself applies no boundary condition (the mask is
    `PMultigrid.restrict`'s), and pairs outside the schedule are refused."""
    nc, Pf, Pc = (2, 3, 2), 4, 2
    fine, coarse = _problem(nc, Pf), _problem(nc, Pc)
    J = np.ascontiguousarray(lagrange_tables(gll(Pc + 1)[0], gll(Pf + 1)[0])[0])
    gf = _random(_shape(nc, Pf), 7, torch.float64)
    vc = coarse.new_vector()
    HostKernels(fine.lat, fine.dtype).restrict(coarse.lat.as_int64(), J, _fill(fine, gf), vc)
    ref, bnd = model_restrict(nc, Pf, Pc, gf)
    assert (np.abs(_glob(coarse, vc) - ref) <= EPS[torch.float64] * bnd).all()
    bad = _problem(nc, 3)
    with pytest.raises(ValueError):
        HostKernels(fine.lat, fine.dtype).restrict(bad.lat.as_int64(), J, _fill(fine, gf),
                                                   bad.new_vector())
    other = _problem((2, 3, 3), Pc)
    with pytest.raises(ValueError):
        HostKernels(fine.lat, fine.dtype).prolong(other.lat.as_int64(), J, other.new_vector(),
                                                  fine.new_vector())


# ------------------------------------------------------- 2. adjointness
def _adjoint_gap(comm, nc, Pf, dt, platform="cpu"):
    pmg = PMultigrid(_problem(nc, Pf, dt, comm=comm, platform=platform))
    Pc = pmg.degrees[1]
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    gu, gv = _random(_shape(nc, Pc), 11, dt), _random(_shape(nc, Pf), 13, dt)
    uc, vf = _fill(coarse, gu), _fill(fine, gv)
    # NaN on the fine ghost planes: a restriction must not read them
    o = fine.lat.owned_hi
    vf[o[0]:], vf[:, o[1]:], vf[:, :, o[2]: fine.lat.L[2]] = NAN, NAN, NAN
    pu, rv = fine.new_vector(), coarse.new_vector()
    pmg.restrict(0, vf, rv)
    # R zeroes Dirichlet rows: compare on a u that vanishes there
    uc[:, :, : coarse.lat.L[2]][torch.from_numpy(coarse.lat.bc_mask()).to(uc.device)] = 0.0
    pmg.prolong(0, uc, pu)
    gap = fine.inner(pu, vf), coarse.inner(uc, rv), Pc, gu, gv
    pmg.close()
    return gap


def _adjoint_bound(nc, Pf, Pc, gu, gv, dt):
    G = [np.abs(axis_matrix(n, Pf, Pc)) for n in nc]
    gu = np.where(make_local_lattice(0, 1, nc, Pc).bc_mask(), 0.0, gu)
    return 2 * 6 * (2 * Pf + 1) * EPS[dt] * float(np.sum(np.abs(gv) * along_axes(G, np.abs(gu))))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_adjointness(Pf, Pc, dt):
    """<P u, v> = <u, R v>; the bound is the sum of the per-entry bounds of
    both transfers, sum_i |v_i| b_P(u)_i + sum_j |u_j| b_R(v)_j."""
    nc = (2, 3, 2)
    a, b, pc, gu, gv = _adjoint_gap(Comm(), nc, Pf, dt)
    assert pc == Pc
    bound = _adjoint_bound(nc, Pf, Pc, gu, gv, dt)
    print(f"adjoint {Pf}/{Pc} {dt}: {a!r} {b!r} gap {abs(a - b):.3e} bound {bound:.3e}")
    assert np.isfinite(a) and abs(a - b) <= bound


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_adjointness_threaded_ranks(Pf, Pc, R):
    nc = (4, 5, 3)
    for a, b, pc, gu, gv in run_threaded(R, _adjoint_gap, nc, Pf, torch.float64):
        bound = _adjoint_bound(nc, Pf, Pc, gu, gv, torch.float64)
        assert np.isfinite(a) and abs(a - b) <= bound, (a, b, bound)


# --------------------------------------------- 3. polynomial reproduction
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_prolong_reproduces_polynomials(Pf, Pc, dt):
    """Nodal samples of a product polynomial of degree Pc per axis in the
    global lattice coordinate prolong to its fine samples."""
    nc = (2, 3, 2)
    pmg = _pmg(nc, Pf, dt)
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    coefs = [np.array([0.3, -1.1, 0.7, 0.9][: Pc + 1]) * (1 + 0.25 * ax) for ax in range(3)]

    def samples(P):
        axes = []
        for ax, n in enumerate(nc):
            t = np.concatenate([(c + gll(P + 1)[0][:-1]) / n for c in range(n)] + [[1.0]])
            axes.append(np.polynomial.polynomial.polyval(2 * t - 1, coefs[ax]))
        return np.einsum("i,j,k->ijk", *axes)

    gc = torch.from_numpy(samples(Pc)).to(dt).double().numpy()
    vf = fine.new_vector()
    pmg.prolong(0, _fill(coarse, gc), vf)
    _, bnd = model_prolong(nc, Pf, Pc, gc)
    err = np.abs(_glob(fine, vf) - samples(Pf))
    print(f"polynomial {Pc}->{Pf} {dt}: max err / bound {(err / (EPS[dt] * bnd)).max():.3e}")
    assert (err <= EPS[dt] * bnd).all()


# --------------------------------- 4. restriction is partition-invariant
def _rank_restrict(comm, nc, Pf, platform="cpu"):
    pmg = PMultigrid(_problem(nc, Pf, comm=comm, platform=platform))
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    vf = _fill(fine, _random(_shape(nc, Pf), 17, torch.float64))
    o = fine.lat.owned_hi
    vf[o[0]:], vf[:, o[1]:], vf[:, :, o[2]: fine.lat.L[2]] = NAN, NAN, NAN
    vc = coarse.new_vector()
    pmg.restrict(0, vf, vc)
    # forwarded: the coarse ghost planes hold their owners' values
    gi = coarse.lat.global_indices()
    out = _glob(coarse, vc), (gi, vc[:, :, : coarse.lat.L[2]].cpu().numpy().copy())
    pmg.close()
    return out


@pytest.mark.parametrize("Pf,Pc", [(3, 1), (4, 2), (6, 3)])
def test_restrict_partition_invariance(Pf, Pc):
    nc = (4, 5, 3)
    ref, bnd = model_restrict(nc, Pf, Pc, _random(_shape(nc, Pf), 17, torch.float64))
    ref[make_local_lattice(0, 1, nc, Pc).bc_mask()] = 0.0
    one = run_threaded(1, _rank_restrict, nc, Pf)[0][0]
    assert (np.abs(one - ref) <= EPS[torch.float64] * bnd).all()
    for R in (2, 4):
        for got, (gi, loc) in run_threaded(R, _rank_restrict, nc, Pf):
            assert (np.abs(got - one) <= EPS[torch.float64] * bnd).all()
            assert np.array_equal(loc, got.ravel()[gi])


# ------------------------------------------------------------ 5. cheb_step
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("first", [True, False])
def test_cheb_step_host_twin(first, dt):
    """Each entry within the rounding of its own operations: d = a d + b dinv
    (r - y) is 5 roundings on terms of magnitude |a d| + |b dinv| (|r| + |y|),
    z += d one more on |z| + |d|; asserted with 8 eps.  Bitwise untouched
    outside the owned box, inputs untouched, and `first` reads no y, d, z."""
    lat = make_local_lattice(0, 8, (2, 2, 2), 3)            # owned (3, 3, 3) of (4, 4, 16)
    assert lat.owned_hi == (3, 3, 3) and lat.shape == (4, 4, 16)
    k = HostKernels(lat, dt)
    rng = np.random.default_rng(23)
    sl = (slice(0, 3),) * 3

    def vec(positive=False, owned=True):
        a = np.full(lat.shape, NAN)
        if owned:
            v = rng.standard_normal((3, 3, 3))
            a[sl] = np.abs(v) + 0.5 if positive else v
        return torch.from_numpy(a).to(dt)

    dinv, r = vec(True), vec()
    y, d, z = (vec(owned=not first) for _ in range(3))
    a, b = 0.3125, 1.7
    d0, z0, ins = d.clone(), z.clone(), [t.clone() for t in (dinv, r, y)]
    k.cheb_step(first, a, b, dinv, r, None if first else y, d, z)
    T = np.float64 if dt == torch.float64 else np.float32
    a, b = float(T(a)), float(T(b))
    di, ri = dinv[sl].double().numpy(), r[sl].double().numpy()
    if first:
        dref, dmag = b * di * ri, np.abs(b * di * ri)
        zref, zmag = dref, dmag
    else:
        yo, do, zo = (t[sl].double().numpy() for t in (y, d0, z0))
        dref = a * do + b * di * (ri - yo)
        dmag = np.abs(a * do) + np.abs(b * di) * (np.abs(ri) + np.abs(yo))
        zref, zmag = zo + dref, np.abs(zo) + dmag
    ed = np.abs(d[sl].double().numpy() - dref) / dmag
    ez = np.abs(z[sl].double().numpy() - zref) / zmag
    print(f"cheb_step first={first} {dt}: d err {ed.max():.3e}, z err {ez.max():.3e}")
    assert ed.max() <= 8 * EPS[dt] and ez.max() <= 8 * EPS[dt]
    out = torch.ones(lat.shape, dtype=torch.bool)
    out[sl] = False
    assert torch.equal(_bits(d)[out], _bits(d0)[out]) and torch.equal(_bits(z)[out], _bits(z0)[out])
    for t, t0 in zip((dinv, r, y), ins):
        assert torch.equal(_bits(t), _bits(t0))


# ----------------------------------------------- 6. symmetry, positivity
def test_vcycle_symmetric_positive():
    """|<M^-1 a, b> - <a, M^-1 b>| <= 1e-12 |<M^-1 a, b>| (a numpy prototype
    measured 3e-16; the bound allows for the reductions' order), <M^-1 a, a> > 0."""
    pb = _problem((4, 4, 4), 3, pert=0.2, coef="random")
    pmg = PMultigrid(pb)
    assert pmg.degrees == [3, 1] and len(pmg.lambda_max) == 2
    bc = pb.bc_mask()
    gen = torch.Generator().manual_seed(5)
    a, b = (torch.randn(pb.lat.shape, dtype=torch.float64, generator=gen).masked_fill_(bc, 0.0)
            for _ in range(2))
    a0 = a.clone()
    za, zb = pb.new_vector(), pb.new_vector()
    pmg.apply(a, za)
    pmg.apply(b, zb)
    assert torch.equal(a, a0)                      # r is not modified
    s1, s2 = pb.inner(za, b), pb.inner(a, zb)
    print(f"<M^-1 a, b> = {s1!r}, <a, M^-1 b> = {s2!r}, rel gap {abs(s1 - s2) / abs(s1):.3e}")
    assert abs(s1 - s2) <= 1e-12 * abs(s1)
    assert pb.inner(za, a) > 0 and pb.inner(zb, b) > 0


def test_level_schedule_and_coefficients():
    assert [level_degrees(P) for P in range(1, 8)] == [
        [1], [2, 1], [3, 1], [4, 2, 1], [5, 2, 1], [6, 3, 1], [7, 3, 1]]
    # degree-2 Chebyshev on [0.2, 2]: theta = 1.1, delta = 0.9
    (a0, b0), (a1, b1) = chebyshev_coefficients(2.0, 10.0, 2)
    sigma = 1.1 / 0.9
    rho1 = 1.0 / (2 * sigma - 1 / sigma)
    assert a0 == 0.0 and abs(b0 - 1 / 1.1) < 1e-15
    assert abs(a1 - rho1 / sigma) < 1e-15 and abs(b1 - 2 * rho1 / 0.9) < 1e-15
    one = PMultigrid(_problem((2, 2, 2), 1))
    assert one.degrees == [1] and len(one.levels[0].coef) == 8


# --------------------------------------- 7. cg_solve(precond=) vs numpy PCG
def _dense_matrix(nc, d, X, kc):
    """Dense stiffness matrix of degree d from the element matrices kappa_c
    sum_q gref^T G gref with the geometry of oracle.box_model (as
    tests/test_cpu_diagonal.py builds its diagonal), Dirichlet rows and
    columns replaced by the identity; checked against the oracle's apply."""
    t = OperatorTables(d, 1, False)
    m = oracle.box_model(nc, d, 1, vertices=X, kappa_cells=kc)
    cx, cy, cz = (a.ravel() for a in np.meshgrid(*(np.arange(n) for n in nc), indexing="ij"))
    cv = np.empty((cx.size, 8, 3))
    for v in range(8):
        cv[:, v] = X[cx + (v >> 2), cy + ((v >> 1) & 1), cz + (v & 1)]
    J = np.einsum("cvi,jqv->cqij", cv, t.geometry_dphi())
    Jinv = np.linalg.inv(J)
    G = np.einsum("cqid,cqjd->cqij", Jinv, Jinv) * (t.weights3d()[None] * np.linalg.det(J))[
        ..., None, None]
    kap = np.full(cx.size, oracle.KAPPA) if kc is None else np.asarray(kc, float).reshape(-1)
    gref, _ = oracle._ref_grad_tables(t)
    Ae = kap[:, None, None] * np.einsum("aqd,cqde,bqe->cab", gref, G, gref, optimize=True)
    dofs, bc = m["dofs"], m["bc"]
    Ae[bc[dofs][:, :, None] | bc[dofs][:, None, :]] = 0.0
    A = np.zeros((bc.size, bc.size))
    np.add.at(A, (dofs[:, :, None], dofs[:, None, :]), Ae)
    A[bc, bc] = 1.0
    v = np.random.default_rng(1).standard_normal(bc.size)
    assert np.abs(A @ v - m["apply"](v)).max() <= 1e-12 * np.abs(A @ v).max()
    return A, m


def _dense_levels(nc, P, pert, coef):
    """Dense level matrices, Jacobi diagonals and global transfer factors."""
    X = vertex_coordinates(make_local_lattice(0, 1, nc, 1), pert)
    kc = cell_coefficients(make_local_lattice(0, 1, nc, 1), coef, oracle.KAPPA)
    levels = []
    for d in level_degrees(P):
        A, m = _dense_matrix(nc, d, X, kc)
        levels.append(dict(A=A, dinv=1.0 / np.diag(A), bc=m["bc"], b=m["b"], P=d,
                           shape=_shape(nc, d)))
    for fine, coarse in zip(levels, levels[1:]):
        fine["G"] = [axis_matrix(n, fine["P"], coarse["P"]) for n in nc]
    return levels


def _np_lambda(lv, iters=10):
    gid = np.arange(lv["bc"].size, dtype=np.uint64)
    v = np.where(lv["bc"], 0.0, 2.0 * _hash_uniform(gid, 11) - 1.0)
    lam = 0.0
    for _ in range(iters):
        v = v / np.linalg.norm(v)
        w = lv["dinv"] * (lv["A"] @ v)
        lam, v = v @ w, w
    return lam


def _np_smooth(lv, r, z, zero_guess):
    for i, (a, b) in enumerate(lv["coef"]):
        if i == 0 and zero_guess:
            lv["d"] = b * lv["dinv"] * r
            z = lv["d"].copy()
        else:
            lv["d"] = a * lv["d"] + b * lv["dinv"] * (r - lv["A"] @ z)
            z = z + lv["d"]
    return z


def _np_vcycle(levels, l, r):
    lv = levels[l]
    z = _np_smooth(lv, r, None, True)
    if l == len(levels) - 1:
        return z
    nxt = levels[l + 1]
    res = (r - lv["A"] @ z).reshape(lv["shape"])
    rc = along_axes([g.T for g in lv["G"]], res).ravel()
    rc[nxt["bc"]] = 0.0
    zc = _np_vcycle(levels, l + 1, rc).reshape(nxt["shape"])
    z = z + along_axes(lv["G"], zc).ravel()
    return _np_smooth(lv, r, z, False)


@pytest.mark.parametrize("P", [3, 4])
def test_pmg_pcg_vs_numpy(P):
    nc, pert, coef, its = (3, 3, 3), 0.2, "random", 6
    levels = _dense_levels(nc, P, pert, coef)
    for i, lv in enumerate(levels):
        last = i == len(levels) - 1
        lv["lam"] = _np_lambda(lv)
        lv["coef"] = chebyshev_coefficients(1.1 * lv["lam"], 100.0 if last else 10.0,
                                            8 if last else 2)
    A, b = levels[0]["A"], levels[0]["b"]
    x = np.zeros_like(b)
    r = b - A @ x
    z = _np_vcycle(levels, 0, r)
    p, rz = z.copy(), r @ z
    for _ in range(its):
        y = A @ p
        alpha = rz / (p @ y)
        x, r = x + alpha * p, r - alpha * y
        z = _np_vcycle(levels, 0, r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    pb = _problem(nc, P, pert=pert, coef=coef)
    pmg = PMultigrid(pb)
    lam = np.array([lv["lam"] for lv in levels])
    print(f"lambda_max {pmg.lambda_max} numpy {lam}")
    # ten applications of D^-1 A (norm about 2), each rounded to about 1e-15:
    # the two power iterations stay far closer than 1e-10
    assert np.abs(np.array(pmg.lambda_max) - lam).max() <= 1e-10 * lam.max()
    xh = pb.new_vector()
    assert cg_solve(MatFreeLaplacianCPU(pb), pb, xh, pb.assemble_rhs(), its,
                    precond=pmg.apply) == its
    gap = np.abs(pb.to_global_array(xh) - x).max() / np.abs(x).max()
    print(f"pmg-PCG vs numpy, Q{P}: max |dx| / max |x| = {gap:.3e}")
    assert gap <= 1e-10


def test_cg_solve_precond_arguments():
    pb = _problem((2, 2, 2), 2)
    with pytest.raises(ValueError):
        cg_solve(MatFreeLaplacianCPU(pb), pb, pb.new_vector(), pb.assemble_rhs(), 1,
                 dinv=pb.jacobi_inverse(), precond=lambda r, z: z.copy_(r))
    with pytest.raises(ValueError):
        DeviceCG(pb, "pmg", loop="fused")


# ---------------------------------------------------------- 8. convergence
def _iterations(pb, op, b, **kw):
    x = pb.new_vector()
    k = cg_solve(op, pb, x, b, 1000, 1e-8, **kw)
    y = pb.new_vector()
    op.apply(x.clone(), y)
    return k, pb.norm(b - y) / pb.norm(b)


@pytest.mark.parametrize("nc,P", [((8, 8, 8), 3), ((6, 6, 6), 6)])
def test_pmg_converges_in_a_quarter_of_jacobi_iterations(nc, P):
    """Iterations to a relative residual of 1e-8 from x0 = 0, perturbed mesh,
    random kappa: pmg-PCG needs at most a quarter of Jacobi-PCG's (a numpy
    prototype measured 13 against 103 and 12 against 206)."""
    pb = _problem(nc, P, pert=0.2, coef="random")
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    kj, rj = _iterations(pb, op, b, dinv=pb.jacobi_inverse())
    pmg = PMultigrid(pb)
    kp, rp = _iterations(pb, op, b, precond=pmg.apply)
    print(f"{nc} Q{P}: Jacobi-PCG {kj} its (true residual {rj:.2e}), "
          f"pmg-PCG {kp} its (true residual {rp:.2e})")
    assert rp <= 1e-8 and 4 * kp <= kj


# ------------------------------------------------------------------ 9. CLI
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


CLI = ["-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs_global", "1000", "--degree",
       "3", "--cg", "--nreps", "10", "--mat_comp", "--precond", "pmg"]


def _cli(launch, js):
    r = subprocess.run([*launch, *CLI, "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, json.load(open(js))


def test_cli_precond_pmg(tmp_path):
    out, d = _cli([sys.executable], tmp_path / "p.json")
    assert "Preconditioner: pmg" in out
    assert d["mi355x"]["precond"] == "pmg"
    blk = d["mi355x"]["pmg"]
    assert set(blk) == {"degrees", "lambda_max", "smooth_degree", "coarse_degree"}
    assert blk["degrees"] == [3, 1] and blk["smooth_degree"] == 2 and blk["coarse_degree"] == 8
    assert len(blk["lambda_max"]) == 2 and all(1.0 < v < 4.0 for v in blk["lambda_max"])
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"matrix-free pmg-PCG vs CSR pmg-PCG: relative error norm {rel:.3e}")
    assert rel < 1e-10
    out2, d2 = _cli([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                     "--nproc-per-node=2", "--master-addr=127.0.0.1", "--master-port=29657"],
                    tmp_path / "p2.json")
    assert d2["input"]["mpi_size"] == 2
    y1, y2 = d["output"]["y_norm"], d2["output"]["y_norm"]
    print(f"y_norm 1 process {y1!r}, 2 processes {y2!r}")
    assert abs(y1 - y2) <= 1e-12 * abs(y1)


def test_cli_pmg_options(tmp_path):
    r = subprocess.run([sys.executable, *CLI, "--pmg_smooth", "3", "--pmg_coarse", "5", "--json",
                        str(tmp_path / "o.json")], cwd=ROOT, env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    blk = json.load(open(tmp_path / "o.json"))["mi355x"]["pmg"]
    assert blk["smooth_degree"] == 3 and blk["coarse_degree"] == 5


@pytest.mark.parametrize("args,word", [
    (["--precond", "pmg"], "precond"),
    (["--cg", "--precond", "pmg", "--pcg_loop", "fused"], "pcg_loop"),
])
def test_cli_pmg_refusals(args, word):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and word in (r.stdout + r.stderr)
