"""The entry-by-entry CG reference (tests/cg_ref.py) on the CPU: the host loop
`cg_solve` over threaded CPU ranks stays inside the bound on every layout the
GPU test uses, and the checker rejects planted structural faults of a CG loop
at the largest K a GPU row may assert."""

import numpy as np
import pytest
import torch

import cg_ref as cref
from cg_ref import Case
from benchmark_dolfinx_amd.fem.mesh import make_local_lattice
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU
from benchmark_dolfinx_amd.parallel.comm import run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve

DTYPES = [torch.float64, torch.float32]
CASES = [Case((3, 3, 2), 3, 1, 0.2, "random"), Case((2, 3, 4), 2, 0, 0.2, "constant"),
         Case((2, 3, 4), 4, 1, 0.2, "random"), Case((5, 3, 4), 1, 1, 0.2, "random"),
         Case((5, 3, 4), 3, 1, 0.0, "random"), Case((3, 3, 2), 6, 1, 0.0, "constant"),
         Case(cref.SHEAR_MESH, 3, 1, 0.0, "random", 0.5)]
ITERATIONS = (3, 4)


def _lattices(case, ranks, partition):
    return [make_local_lattice(r, ranks, case.nc, case.P, whole_x=partition == "yz")
            for r in range(ranks)]


def _one_cell_axes(lat):
    return [d for d in range(3) if lat.pgrid[d] > 1 and lat.n[d] == 1]


def test_refusal_by_free_dofs():
    """(3, 3, 2) at P = 1 has 4 free dofs; (5, 3, 4) at P = 1 has 24 (k = 3, not
    k = 4), (2, 3, 4) at P = 2 has 105."""
    assert int(cref.free_mask(Case((3, 3, 2), 1)).sum()) == 4
    assert int(cref.free_mask(Case((5, 3, 4), 1)).sum()) == 24
    assert int(cref.free_mask(Case((2, 3, 4), 2)).sum()) == 105
    assert cref.allowed(Case((5, 3, 4), 1), 3) and not cref.allowed(Case((5, 3, 4), 1), 4)
    assert cref.allowed(Case((2, 3, 4), 2), 4) and not cref.allowed(Case((3, 3, 2), 1), 3)
    with pytest.raises(ValueError, match="free dofs"):
        cref.reference(Case((5, 3, 4), 1), torch.float64, 4)


def _host_job(comm, case, dt, partition, k, jacobi):
    pb = case.problem(comm, dt, "cpu", partition)
    b, x = cref.local_vectors(pb, cref.reference(case, dt, k, jacobi))
    b0 = b.clone()
    cg_solve(MatFreeLaplacianCPU(pb), pb, x, b, k, dinv=pb.jacobi_inverse() if jacobi else None)
    assert torch.equal(pb.owned(b), pb.owned(b0))
    return pb.to_global_array(x), pb.lat.gh


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("ranks,partition", cref.LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_host_loop_within_bound(case, ranks, partition, jacobi, dt):
    """`cg_solve` over `MatFreeLaplacianCPU` on threaded CPU ranks, b and x0
    with NaN ghosts and padding, within K_CPU = 64 of the one-rank FP64
    recurrence after 3 and 4 iterations.  Measured over all of these cases and
    layouts, largest entry ratio: FP64 0.58 (k = 3) and 0.31 (k = 4), FP32
    0.48 (k = 3) and 0.25 (k = 4); Jacobi 0.17 and 0.24.  The planted faults
    below give 4.6e3 .. 1.1e6 in FP32 and 4e13 .. 6e14 in FP64."""
    for k in ITERATIONS:
        if not cref.allowed(case, k):
            continue
        cref.reference(case, dt, k, jacobi)          # cached, before the threads start
        res = run_threaded(ranks, _host_job, case, dt, partition, k, jacobi)
        for got, _ in res:
            assert np.array_equal(got, res[0][0])
        r, _ = cref.check(res[0][0], case, dt, k, cref.K_CPU, jacobi)
        print(f"{case} {ranks}/{partition} {dt} {'jacobi' if jacobi else 'plain'} k={k}: "
              f"entry ratio {r:.3g}")
        if ranks > 1:
            assert any(_one_cell_axes(lat) for lat in _lattices(case, ranks, partition))
        if ranks == 8:
            assert {gh for _, gh in res} == {(a, b, c) for a in (0, 1) for b in (0, 1)
                                             for c in (0, 1)}


# ------------------------------------------------------------ planted faults
FAULTS = ["stale_ghosts", "no_reverse", "no_flush", "swapped_rho", "dot_ghost", "skip_plane"]
FAULT_CASE = Case((3, 3, 2), 3, 1, 0.2, "random")
FAULT_K = 3


def _loop(op, pb, x, b, k, dinv, fault):
    """The recurrence of `cg_solve` (rtol = 0) written out around the CPU
    operator's steps, with one structural fault planted; returns the plain
    r.r.  Exchanges are collective, so they are skipped on every rank; the
    other faults sit on one rank."""
    lat, halo, comm = pb.lat, pb.halo, pb.comm
    lats = _lattices(Case(lat.ncells_global, lat.degree), lat.nranks,
                     "yz" if pb.partition == "yz" else "xyz")
    # the first rank with a ghost plane / with a single cell on a split axis
    face_rank = next(l.rank for l in lats if any(l.gh))
    cell_rank = next(l.rank for l in lats if _one_cell_axes(l))
    o = lat.owned_hi
    ghost = torch.ones(lat.shape, dtype=torch.bool)
    ghost[: o[0], : o[1], : o[2]] = False
    state = {"it": -1, "prev": None}

    def apply(u, y):
        y.zero_()
        if fault == "stale_ghosts" and state["it"] >= 1:
            u[ghost] = state["prev"][ghost]          # what the last exchange left there
        else:
            halo.forward(u)
        state["prev"] = u.clone()
        for lo, hi in [lat.interior_cell_box()] + lat.boundary_cell_boxes():
            if all(h > l for l, h in zip(lo, hi)):
                op._cells(u, y, lo, hi)
        if not (fault == "no_reverse" and state["it"] == 1):
            halo.reverse(y)

    def inner(a, c, ghost_plane=False):
        s = torch.sum(pb.owned(a).double() * pb.owned(c).double())
        if ghost_plane and lat.rank == face_rank:
            d = lat.gh.index(1)
            sl = [slice(0, o[0]), slice(0, o[1]), slice(0, o[2])]
            sl[d] = lat.L[d] - 1
            s = s + torch.sum(a[tuple(sl)].double() * c[tuple(sl)].double())
        s = s.view(1)
        if comm.size > 1:
            comm.allreduce_(s)
        return float(s.item())

    r, y = pb.new_vector(), pb.new_vector()
    apply(x, y)
    r.copy_(b - y)
    z = r if dinv is None else dinv * r
    p = z.clone()
    rz = inner(r, z)
    for it in range(k):
        state["it"] = it
        apply(p, y)
        alpha = rz / inner(p, y, ghost_plane=fault == "dot_ghost")
        if fault == "no_flush" and it == k - 1 and lat.rank == cell_rank:
            pass                                     # the pending x += alpha p is lost
        elif fault == "skip_plane" and lat.rank == cell_rank:
            d = _one_cell_axes(lat)[0]
            sl = [slice(None)] * 3
            sl[d] = slice(0, o[d] - 1)               # all but the last owned plane
            x[tuple(sl)] += alpha * p[tuple(sl)]
        else:
            x.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        if dinv is not None:
            z = dinv * r
        rz_new = inner(r, z)
        beta = rz / rz_new if fault == "swapped_rho" else rz_new / rz
        rz = rz_new
        p.mul_(beta).add_(z)
    return inner(r, r)


def _fault_job(comm, dt, partition, jacobi, fault):
    case, k = FAULT_CASE, FAULT_K
    pb = case.problem(comm, dt, "cpu", partition)
    b, x = cref.local_vectors(pb, cref.reference(case, dt, k, jacobi))
    rr = _loop(MatFreeLaplacianCPU(pb), pb, x, b, k, pb.jacobi_inverse() if jacobi else None,
               fault)
    return pb.to_global_array(x), rr


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ranks,partition", cref.LAYOUTS[1:])
@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected(fault, ranks, partition, dt):
    """Each fault fails `check` at K_CAP = 640, the largest K a GPU row may
    assert; the unfaulted copy of the loop passes at K_CPU, entries and r.r."""
    case, k = FAULT_CASE, FAULT_K
    cref.reference(case, dt, k)
    good, rr = run_threaded(ranks, _fault_job, dt, partition, False, "none")[0]
    r, rs = cref.check(good, case, dt, k, cref.K_CPU, rr=rr)
    got, rr = run_threaded(ranks, _fault_job, dt, partition, False, fault)[0]
    with pytest.raises(AssertionError) as e:
        cref.check(got, case, dt, k, cref.K_CAP)
    print(f"{fault} {ranks}/{partition} {dt}: unfaulted {r:.3g} (r.r {rs:.3g}); "
          f"{str(e.value)[:150]}")
    assert np.isfinite(got).all() and "ratio" in str(e.value)


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_unfaulted_jacobi_loop_copy_passes(dt):
    """The loop copy with the Jacobi recurrence, entries and plain r.r, on 8 ranks."""
    case, k = FAULT_CASE, FAULT_K
    cref.reference(case, dt, k, True)
    good, rr = run_threaded(8, _fault_job, dt, "xyz", True, "none")[0]
    r, rs = cref.check(good, case, dt, k, cref.K_CPU, True, rr=rr)
    print(f"jacobi {dt}: entry ratio {r:.3g}, scalar ratio {rs:.3g}")


def test_check_names_the_worst_entry():
    case, dt, k = FAULT_CASE, torch.float64, FAULT_K
    ref = cref.reference(case, dt, k)
    assert cref.ratio(ref.x, case, dt, k) == 0.0
    assert cref.check(ref.x, case, dt, k, 1, rr=ref.rr) == (0.0, 0.0)
    N = tuple(n * case.P + 1 for n in case.nc)
    at = (4, 7, 2)
    w = int(np.ravel_multi_index(at, N))
    assert ref.free[w]
    got = ref.x.copy()
    got[w] += 100 * cref.EPS[dt] * ref.s[w]
    assert 99 < cref.ratio(got, case, dt, k) < 101      # the perturbation itself is rounded
    assert cref.check(got, case, dt, k, 101)[0] > 99
    with pytest.raises(AssertionError, match=rf"global index {w} \(i, j, k\) = \(4, 7, 2\)"):
        cref.check(got, case, dt, k, 64)
    got[w] = np.inf
    with pytest.raises(AssertionError, match=f"non-finite.*global index {w} "):
        cref.check(got, case, dt, k, 64)
    # a Dirichlet entry that moved is an error whatever its size
    got = ref.x.copy()
    got[0] = 1e-300
    with pytest.raises(AssertionError, match=r"Dirichlet.*global index 0 \(i, j, k\) = \(0, 0, 0\)"):
        cref.check(got, case, dt, k, 64)
    with pytest.raises(AssertionError, match="scalar ratio"):
        cref.check(ref.x, case, dt, k, 64, rr=ref.rr + 100 * cref.EPS[dt] * ref.rr_scale)
