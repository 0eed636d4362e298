"""The entry-by-entry operator reference (tests/operator_ref.py) on the CPU: the
C++ CPU operator over threaded ranks stays inside the bound on every layout and
mesh the GPU tests use, and the checker rejects planted faults at the largest K
a GPU test may assert."""

import functools

import numpy as np
import pytest
import torch

import operator_ref as oref
from operator_ref import Case
from benchmark_dolfinx_amd.fem.mesh import make_local_lattice
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU
from benchmark_dolfinx_amd.parallel.comm import run_threaded

DTYPES = [torch.float64, torch.float32]
# per mesh: box / random kappa, x-perturbed / random kappa, collocation (qmode 0)
CASES = [Case(nc, P, qm, pert, coef)
         for nc in oref.MESHES
         for P, qm, pert, coef in [(1, 1, 0.2, "random"), (2, 0, 0.2, "constant"),
                                   (3, 1, 0.0, "random"), (3, 1, 0.2, "random"),
                                   (4, 1, 0.2, "random"), (5, 1, 0.0, "constant"),
                                   (6, 1, 0.2, "random"), (7, 1, 0.2, "constant")]]
CASES += [Case(oref.SHEAR_MESH, P, 1, 0.0, "random", 0.5) for P in (3, 6)]


def _job(comm, case, dt, partition, fault=None):
    pb = case.problem(comm, dt, "cpu", partition)
    op = MatFreeLaplacianCPU(pb)
    if fault is not None:
        op = _Faulty(op, fault, dt)
    u = oref.local_input(pb, oref.reference(case, dt).ug)
    y = torch.full(pb.lat.shape, oref.NAN, dtype=dt)
    op.apply(u, y)
    return pb.to_global_array(y), (pb.lat.n, pb.lat.gh)


@functools.lru_cache(maxsize=None)
def _one_rank(case, dt):
    return run_threaded(1, _job, case, dt, "xyz")[0][0]


def _lattices(case, ranks, partition):
    return [make_local_lattice(r, ranks, case.nc, case.P, whole_x=partition == "yz")
            for r in range(ranks)]


def _one_cell_axes(lat):
    return [d for d in range(3) if lat.pgrid[d] > 1 and lat.n[d] == 1]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ranks,partition", oref.LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_cpu_operator_within_bound(case, ranks, partition, dt):
    """The FP64 CPU operator over ranks within 64 eps64 m of one rank's, and
    the FP32 CPU problem within 64 eps32 m (measured: 1.6 and 10.2 at the most;
    the gap between rank counts is at most 1.4e-16 max|y| in FP64)."""
    oref.reference(case, dt)
    res = run_threaded(ranks, _job, case, dt, partition)
    for got, _ in res:
        assert np.array_equal(got, res[0][0])
    r = oref.check(res[0][0], case, dt, oref.K_CPU)
    print(f"{case} {ranks}/{partition} {dt}: ratio {r:.3g}")
    if ranks > 1:
        one = _one_rank(case, dt)
        gap = np.abs(res[0][0] - one).max() / np.abs(one).max()
        print(f"  gap to one rank {gap:.3e} max|y|")
        assert any(_one_cell_axes(lat) for lat in _lattices(case, ranks, partition))
    if ranks == 8:
        assert {gh for _, (_, gh) in res} == {(a, b, c) for a in (0, 1) for b in (0, 1)
                                              for c in (0, 1)}


# ------------------------------------------------------------ planted faults
class _Faulty:
    """`MatFreeLaplacianCPU.apply` with one fault planted."""

    def __init__(self, op, kind, dt):
        self.op, self.kind = op, kind
        self.scale = 1 + (1e-6 if dt == torch.float64 else 1e-3)
        lat = op.pb.lat
        lats = _lattices(Case(lat.ncells_global, lat.degree), lat.nranks,
                         "yz" if op.pb.partition == "yz" else "xyz")
        # the first rank with a ghost plane / with a single cell on a split axis
        self.face_rank = next(l.rank for l in lats if any(l.gh))
        self.cell_rank = next(l.rank for l in lats if _one_cell_axes(l))

    def apply(self, u, y):
        op, pb, lat, kind = self.op, self.op.pb, self.op.pb.lat, self.kind
        y.zero_()
        if kind != "no_forward":
            pb.halo.forward(u)
        boxes = [lat.interior_cell_box()] + lat.boundary_cell_boxes()
        if kind == "drop_cell" and lat.rank == self.cell_rank:
            n = lat.n          # every cell but the last one (n - 1, n - 1, n - 1)
            boxes = [((0, 0, 0), (n[0] - 1, n[1], n[2])),
                     ((n[0] - 1, 0, 0), (n[0], n[1] - 1, n[2])),
                     ((n[0] - 1, n[1] - 1, 0), (n[0], n[1], n[2] - 1))]
        for lo, hi in boxes:
            if all(h > l for l, h in zip(lo, hi)):
                op._cells(u, y, lo, hi)
        if kind == "scale_face" and lat.rank == self.face_rank:
            d = lat.gh.index(1)
            sl = [slice(None)] * 3
            sl[d] = lat.L[d] - 1
            y[tuple(sl)] *= self.scale
        if kind != "no_reverse":
            pb.halo.reverse(y)


FAULT_CASE = Case((3, 3, 2), 3, 1, 0.2, "random")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ranks,partition", oref.LAYOUTS[1:])
@pytest.mark.parametrize("fault", ["no_forward", "no_reverse", "scale_face", "drop_cell"])
def test_planted_faults_are_rejected(fault, ranks, partition, dt):
    """Each fault fails `check` at the largest K a GPU test may assert (the
    unfaulted wrapper passes at the CPU bound)."""
    oref.reference(FAULT_CASE, dt)
    good = run_threaded(ranks, _job, FAULT_CASE, dt, partition, "none")[0][0]
    oref.check(good, FAULT_CASE, dt, oref.K_CPU)
    got = run_threaded(ranks, _job, FAULT_CASE, dt, partition, fault)[0][0]
    with pytest.raises(AssertionError) as e:
        oref.check(got, FAULT_CASE, dt, oref.K_CAP)
    print(f"{fault} {ranks}/{partition} {dt}: {str(e.value)[:160]}")
    if fault == "no_forward":
        assert "non-finite" in str(e.value)
    else:
        assert np.isfinite(got).all() and "ratio" in str(e.value)


@pytest.mark.parametrize("case", [c for c in CASES if c.P <= oref.CSR_MAX_P]
                         + [Case((3, 3, 2), 5, 1, 0.2, "random"), Case((2, 3, 4), 5, 1, 0.0, "constant"),
                            Case(oref.SHEAR_MESH, 5, 1, 0.0, "random", 0.5)], ids=str)
def test_dense_assembly_matches_the_csr_operator(case):
    """m = |A| |u| from the dense element matrices (what `reference` uses above
    P = 4, where the package's own assembly takes seconds per case) against
    the one read off `CSROperator`: the same matrix, so equal to the rounding
    of an element-matrix entry, far below what moves a ratio."""
    cpu = oref._host(case)[0]
    lat = cpu.lat
    ug = np.random.default_rng(9).standard_normal(lat.ndofs_global)
    u = cpu.new_vector()
    u[:, :, : lat.L[2]] = torch.from_numpy(ug.reshape(lat.L))
    m_csr, m_dense = oref.csr_abs_action(case, u.numpy()), oref.abs_action(case, ug)
    gap = (np.abs(m_csr - m_dense) / m_csr).max()
    print(f"{case}: max relative gap {gap:.3e}")
    assert (m_csr > 0).all() and gap <= 1e-13


def test_check_names_the_worst_entry():
    case, dt = FAULT_CASE, torch.float64
    ref = oref.reference(case, dt)
    assert oref.ratio(ref.y, case, dt) == 0.0
    N = tuple(n * case.P + 1 for n in case.nc)
    at = (4, 7, 2)
    w = int(np.ravel_multi_index(at, N))
    got = ref.y.copy()
    got[w] += 100 * oref.EPS[dt] * ref.m[w]
    assert 99 < oref.ratio(got, case, dt) < 101      # the perturbation itself is rounded
    assert oref.check(got, case, dt, 101) > 99
    with pytest.raises(AssertionError, match=rf"global index {w} \(i, j, k\) = \(4, 7, 2\)"):
        oref.check(got, case, dt, 64)
    got[w] = np.inf
    with pytest.raises(AssertionError, match=f"non-finite.*global index {w} "):
        oref.check(got, case, dt, 64)
