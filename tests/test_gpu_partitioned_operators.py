"""Every GPU operator kernel, entry by entry against the FP64 CPU operator, on
partitioned lattices with one-cell blocks (tests/operator_ref.py): one rank,
4 ranks with x whole (the native runtime's overlap layout) and a 2 x 2 x 2
grid with all eight ghost patterns, threaded ranks on one GPU.

The input holds NaN on every ghost plane and in the storage padding, the
output starts as NaN: the operator's own forward exchange has to fill what its
kernel reads, and the kernel may read nothing else.

Bound: |got_i - y_i| <= K eps_T (|A| |u|)_i with K = 10 x the largest ratio
measured on an MI355X over the row's layouts and meshes (`MEASURED`,
profiles/partitioned_entrywise.md), never below 8; the 10 x covers another
summation order, FMA contraction and the order of dofmap's atomics.  No
measured ratio above 64 is recorded (the CPU operator's own is 1.5 in FP64 and
10 in FP32)."""

import contextlib

import numpy as np
import pytest
import torch

import operator_ref as oref
from operator_ref import Case
from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.fused import FusedLaplacianGPU, fused_supported
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianGPU
from benchmark_dolfinx_amd.models.unstructured import DofmapLaplacianGPU
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from test_gpu_diagonal import _host_diagonal

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
BOTH = (F64, F32)
ALL_GH = {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


def _variant(kind, nc, P):
    return {"box-const": Case(nc, P, 1, 0.0, "constant"),
            "box-rand": Case(nc, P, 1, 0.0, "random"),
            "pert": Case(nc, P, 1, 0.2, "random"),        # x-trilinear cells
            "pert-q0": Case(nc, P, 0, 0.2, "constant"),   # GLL collocation: phi0 = I
            "shear": Case(nc, P, 1, 0.0, "random", 0.5)}[kind]


def _fused(version, **kw):
    return lambda pb: FusedLaplacianGPU(pb, "otf", version, **kw)


# row -> (mesh variant, degrees, dtypes, fused version or None, builder,
#         (name, geometry, affine_code) every rank has to report)
ROWS = {
    "fused5-const": ("box-const", range(3, 8), BOTH, 5, _fused(5), ("fused5", "otf-affine", 2)),
    "fused5-rand": ("box-rand", range(3, 8), BOTH, 5, _fused(5), ("fused5", "otf-affine", 2)),
    "fused3-affine": ("box-rand", range(1, 8), BOTH, 3, _fused(3), ("fused3", "otf-affine", 1)),
    "fused3-sheared": ("shear", range(1, 8), BOTH, 3, _fused(3), ("fused3", "otf-affine", 1)),
    "fused3-xtri": ("pert", range(1, 8), BOTH, 3, _fused(3), ("fused3", "otf-xtrilinear", 2)),
    "fused3-general": ("pert", range(1, 8), BOTH, 3,
                       lambda pb: make_operator(pb, "fused3", "otf-general"),
                       ("fused3", "otf-general", 0)),
    "fused2-xtri-q0": ("pert-q0", (1, 2, 3, 6), BOTH, 2, _fused(2),
                       ("fused2", "otf-xtrilinear", 2)),
    "fused2-general": ("pert", (1, 2, 3, 6), BOTH, 2, _fused(2, affine=False),
                       ("fused2", "otf-general", 0)),
    "fused-v1": ("box-const", (3, 6), BOTH, 1, _fused(1), ("fused", "otf", 1)),
    "v1-stored": ("pert", (1, 3, 6), BOTH, None, lambda pb: MatFreeLaplacianGPU(pb, "stored"),
                  ("v1", "stored", None)),
    "v1-otf": ("pert", (1, 3, 6), BOTH, None, lambda pb: MatFreeLaplacianGPU(pb, "otf"),
               ("v1", "otf", None)),
    "dofmap-valu-otf": ("pert", range(1, 8), BOTH, None, lambda pb: DofmapLaplacianGPU(pb, "otf"),
                        ("dofmap", "dofmap-otf", "valu")),
    "dofmap-valu-stored": ("pert", (3, 6), BOTH, None,
                           lambda pb: DofmapLaplacianGPU(pb, "stored"),
                           ("dofmap", "dofmap-stored", "valu")),
    # the MFMA kernel has no nq = 9 instance: P = 7 with qmode 1 is the VALU row
    "dofmap-mfma-otf": ("pert", range(1, 7), (F64,), None,
                        lambda pb: DofmapLaplacianGPU(pb, "otf"),
                        ("dofmap", "dofmap-otf", "mfma")),
    "dofmap-mfma-stored": ("pert", (3, 6), (F64,), None,
                           lambda pb: DofmapLaplacianGPU(pb, "stored"),
                           ("dofmap", "dofmap-stored", "mfma")),
}
PARAMS = [(row, P, dt) for row, spec in ROWS.items() for P in spec[1] for dt in spec[2]]


def _runs(row):
    """(ranks, partition, cells) of a row: every layout on every mesh; the
    (5, 3, 4) x-march at one rank and at 4 / yz."""
    if ROWS[row][0] == "shear":
        return [(r, p, oref.SHEAR_MESH) for r, p in oref.LAYOUTS]
    return [(r, p, nc) for r, p in oref.LAYOUTS for nc in oref.MESHES
            if not (r == 8 and nc == (5, 3, 4))]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


@contextlib.contextmanager
def _dofmap_core(row):
    """The FP64 dofmap kernel of the row (as the fixture of tests/test_gpu_dofmap.py)."""
    if not row.startswith("dofmap"):
        yield
        return
    lib = native.hip()
    lib.bdx_dofmap_set_mfma(1 if "mfma" in row else 0)
    try:
        yield
    finally:
        lib.bdx_dofmap_set_mfma(-1)


def job(comm, case, instance, dt, partition):
    pb = case.problem(comm, dt, "gpu", partition)
    refusal = None
    try:
        op = ROWS[instance][4](pb)
    except (ValueError, RuntimeError) as e:      # HipError is a RuntimeError
        refusal = f"{type(e).__name__}: {e}"
    # a refusal has to be the same on every rank (and is agreed on before the
    # collective apply); the automatic choice still has to work there
    refusals = comm.gather_objects(refusal)
    assert len(set(refusals)) == 1, refusals
    if refusal is not None:
        op = make_operator(pb)
    u = oref.local_input(pb, oref.reference(case, dt).ug)
    u0 = u.clone()
    y = torch.full(pb.lat.shape, oref.NAN, dtype=dt, device=pb.device)
    op.apply(u, y)
    got = pb.to_global_array(y)
    unchanged = torch.equal(_bits(pb.owned(u)), _bits(pb.owned(u0)))
    third = getattr(op, "core", None) if instance.startswith("dofmap") else \
        getattr(op, "affine_code", None)
    rec = (getattr(op, "name", "v1"), op.geometry, third, pb.lat.n, pb.lat.gh, pb.lat.pgrid)
    if hasattr(op, "close"):
        op.close()
    torch.cuda.synchronize()
    return got, rec, unchanged, refusal


def measure(row, P, dt):
    """{(ranks, partition, cells): ratio or the refusal} of one row, with every
    assertion but the bound."""
    kind, _, _, _, _, instance = ROWS[row]
    out = {}
    with _dofmap_core(row):
        for ranks, partition, nc in _runs(row):
            case = _variant(kind, nc, P)
            oref.reference(case, dt)              # cached, before the threads start
            res = run_threaded(ranks, job, case, row, dt, partition)
            key = (ranks, partition, nc)
            got, rec0, _, refusal = res[0]
            for g, rec, unchanged, _ in res:
                assert np.array_equal(g, got), key      # every rank gathered the same array
                assert rec[:3] == rec0[:3], (key, rec, rec0)   # ... built the same instance
                assert unchanged, key                   # ... and left u alone
            if ranks > 1:
                assert any(p > 1 and n == 1 for _, rec, _, _ in res
                           for p, n in zip(rec[5], rec[3])), (key, [r[1] for r in res])
            if ranks == 8:
                assert {rec[4] for _, rec, _, _ in res} == ALL_GH, key
            if refusal is not None:
                oref.check(got, case, dt, oref.K_CAP)   # the automatic choice works
                out[key] = refusal
                continue
            want = instance if (dt == F64 or instance[2] != "mfma") else instance[:2] + ("valu",)
            assert rec0[:3] == want, (key, rec0)
            oref.check(got, case, dt, oref.K_CAP)       # finite, and no gross error
            out[key] = oref.ratio(got, case, dt)
    return out


# Largest ratio measured on an MI355X per (row, P, dtype): (one rank, 4 / yz
# and 8 / xyz); profiles/partitioned_entrywise.md has them per layout.
MEASURED = {
    ("fused5-const", 3, F64): (5.19, 5.19),
    ("fused5-const", 3, F32): (2.31, 2.31),
    ("fused5-const", 4, F64): (5.09, 5.09),
    ("fused5-const", 4, F32): (2.32, 2.32),
    ("fused5-const", 5, F64): (5.01, 5.01),
    ("fused5-const", 5, F32): (2.21, 2.21),
    ("fused5-const", 6, F64): (5.3, 5.3),
    ("fused5-const", 6, F32): (1.89, 1.89),
    ("fused5-const", 7, F64): (18.2, 18.2),
    ("fused5-const", 7, F32): (2.19, 2.19),
    ("fused5-rand", 3, F64): (5.3, 5.3),
    ("fused5-rand", 3, F32): (2.62, 2.62),
    ("fused5-rand", 4, F64): (4.64, 4.64),
    ("fused5-rand", 4, F32): (1.97, 1.97),
    ("fused5-rand", 5, F64): (4.8, 4.8),
    ("fused5-rand", 5, F32): (2.54, 2.54),
    ("fused5-rand", 6, F64): (5.71, 5.71),
    ("fused5-rand", 6, F32): (2.09, 2.09),
    ("fused5-rand", 7, F64): (19, 19),
    ("fused5-rand", 7, F32): (2.26, 2.26),
    ("fused3-affine", 1, F64): (1.31, 1.31),
    ("fused3-affine", 1, F32): (1.62, 1.69),
    ("fused3-affine", 2, F64): (1.92, 1.92),
    ("fused3-affine", 2, F32): (1.47, 1.47),
    ("fused3-affine", 3, F64): (3.31, 3.31),
    ("fused3-affine", 3, F32): (2.02, 2.02),
    ("fused3-affine", 4, F64): (3.23, 3.23),
    ("fused3-affine", 4, F32): (1.96, 1.96),
    ("fused3-affine", 5, F64): (3.87, 3.87),
    ("fused3-affine", 5, F32): (2.73, 2.73),
    ("fused3-affine", 6, F64): (4.5, 4.5),
    ("fused3-affine", 6, F32): (2.75, 2.75),
    ("fused3-affine", 7, F64): (5.04, 5.04),
    ("fused3-affine", 7, F32): (2.66, 2.66),
    ("fused3-sheared", 1, F64): (1.74, 1.74),
    ("fused3-sheared", 1, F32): (0.858, 0.858),
    ("fused3-sheared", 2, F64): (3.74, 3.74),
    ("fused3-sheared", 2, F32): (1.3, 1.3),
    ("fused3-sheared", 3, F64): (2.03, 2.03),
    ("fused3-sheared", 3, F32): (1.15, 1.15),
    ("fused3-sheared", 4, F64): (2.3, 2.3),
    ("fused3-sheared", 4, F32): (1.34, 1.34),
    ("fused3-sheared", 5, F64): (2.61, 2.61),
    ("fused3-sheared", 5, F32): (1.74, 1.74),
    ("fused3-sheared", 6, F64): (3.05, 3.05),
    ("fused3-sheared", 6, F32): (1.72, 1.72),
    ("fused3-sheared", 7, F64): (3.1, 3.1),
    ("fused3-sheared", 7, F32): (2.15, 2.15),
    ("fused3-xtri", 1, F64): (1.33, 1.52),
    ("fused3-xtri", 1, F32): (1.29, 1.55),
    ("fused3-xtri", 2, F64): (2.6, 2.6),
    ("fused3-xtri", 2, F32): (2.03, 2.03),
    ("fused3-xtri", 3, F64): (2.54, 2.54),
    ("fused3-xtri", 3, F32): (2.06, 2.06),
    ("fused3-xtri", 4, F64): (3.85, 3.85),
    ("fused3-xtri", 4, F32): (2.22, 2.22),
    ("fused3-xtri", 5, F64): (3.48, 3.48),
    ("fused3-xtri", 5, F32): (2.95, 2.95),
    ("fused3-xtri", 6, F64): (4.31, 4.31),
    ("fused3-xtri", 6, F32): (2.39, 2.39),
    ("fused3-xtri", 7, F64): (4.78, 4.78),
    ("fused3-xtri", 7, F32): (2.96, 2.96),
    ("fused3-general", 1, F64): (1.52, 1.52),
    ("fused3-general", 1, F32): (1.29, 1.42),
    ("fused3-general", 2, F64): (3.45, 3.45),
    ("fused3-general", 2, F32): (1.8, 1.8),
    ("fused3-general", 3, F64): (3.05, 3.05),
    ("fused3-general", 3, F32): (2.06, 2.06),
    ("fused3-general", 4, F64): (3.45, 3.45),
    ("fused3-general", 4, F32): (2.54, 2.54),
    ("fused3-general", 5, F64): (4.18, 4.18),
    ("fused3-general", 5, F32): (2.62, 2.62),
    ("fused3-general", 6, F64): (4.18, 4.18),
    ("fused3-general", 6, F32): (3.27, 3.27),
    ("fused3-general", 7, F64): (5.02, 5.02),
    ("fused3-general", 7, F32): (2.93, 2.93),
    ("fused2-xtri-q0", 1, F64): (1.42, 1.08),
    ("fused2-xtri-q0", 1, F32): (1.37, 1.37),
    ("fused2-xtri-q0", 2, F64): (2.09, 2.4),
    ("fused2-xtri-q0", 2, F32): (2.18, 2.18),
    ("fused2-xtri-q0", 3, F64): (4.23, 4.23),
    ("fused2-xtri-q0", 3, F32): (2.16, 1.75),
    ("fused2-xtri-q0", 6, F64): (5.17, 5.17),
    ("fused2-xtri-q0", 6, F32): (2.79, 2.79),
    ("fused2-general", 1, F64): (1.52, 1.52),
    ("fused2-general", 1, F32): (1.29, 1.29),
    ("fused2-general", 2, F64): (3.47, 3.47),
    ("fused2-general", 2, F32): (2.32, 2.32),
    ("fused2-general", 3, F64): (2.54, 2.54),
    ("fused2-general", 3, F32): (2.06, 2.06),
    ("fused2-general", 6, F64): (4.39, 4.39),
    ("fused2-general", 6, F32): (3.79, 3.79),
    ("fused-v1", 3, F64): (3.14, 3.14),
    ("fused-v1", 3, F32): (2.38, 2.38),
    ("fused-v1", 6, F64): (4.17, 4.17),
    ("fused-v1", 6, F32): (2.56, 2.56),
    ("v1-stored", 1, F64): (0.955, 1.52),
    ("v1-stored", 1, F32): (1.55, 1.66),
    ("v1-stored", 3, F64): (2.77, 2.77),
    ("v1-stored", 3, F32): (2.27, 2.27),
    ("v1-stored", 6, F64): (4.55, 4.55),
    ("v1-stored", 6, F32): (3.33, 3.33),
    ("v1-otf", 1, F64): (0.955, 1.52),
    ("v1-otf", 1, F32): (1.66, 1.66),
    ("v1-otf", 3, F64): (2.77, 2.77),
    ("v1-otf", 3, F32): (2.27, 2.27),
    ("v1-otf", 6, F64): (4.55, 4.55),
    ("v1-otf", 6, F32): (3.33, 3.33),
    ("dofmap-valu-otf", 1, F64): (0.888, 0.955),
    ("dofmap-valu-otf", 1, F32): (1.68, 1.66),
    ("dofmap-valu-otf", 2, F64): (2.6, 2.6),
    ("dofmap-valu-otf", 2, F32): (2.2, 2.2),
    ("dofmap-valu-otf", 3, F64): (2.32, 2.32),
    ("dofmap-valu-otf", 3, F32): (2.27, 2.27),
    ("dofmap-valu-otf", 4, F64): (2.94, 2.94),
    ("dofmap-valu-otf", 4, F32): (2.72, 2.72),
    ("dofmap-valu-otf", 5, F64): (3.97, 3.97),
    ("dofmap-valu-otf", 5, F32): (2.61, 2.61),
    ("dofmap-valu-otf", 6, F64): (4.47, 4.47),
    ("dofmap-valu-otf", 6, F32): (3.63, 3.63),
    ("dofmap-valu-otf", 7, F64): (4.28, 4.28),
    ("dofmap-valu-otf", 7, F32): (4.1, 4.1),
    ("dofmap-valu-stored", 3, F64): (2.61, 2.61),
    ("dofmap-valu-stored", 3, F32): (2.15, 2.15),
    ("dofmap-valu-stored", 6, F64): (4.47, 4.47),
    ("dofmap-valu-stored", 6, F32): (3.43, 3.43),
    ("dofmap-mfma-otf", 1, F64): (1.15, 1.52),
    ("dofmap-mfma-otf", 2, F64): (2.74, 2.74),
    ("dofmap-mfma-otf", 3, F64): (3.24, 3.24),
    ("dofmap-mfma-otf", 4, F64): (3.85, 3.85),
    ("dofmap-mfma-otf", 5, F64): (3.76, 3.76),
    ("dofmap-mfma-otf", 6, F64): (5.06, 5.06),
    ("dofmap-mfma-stored", 3, F64): (3.24, 3.24),
    ("dofmap-mfma-stored", 6, F64): (5.06, 5.06),
}
REFUSED = {}   # (row, P, dtype) -> shapes the instance refuses (none found)


def _K(row, P, dt):
    return max(8.0, 10.0 * max(MEASURED[(row, P, dt)]))


@pytest.mark.parametrize("row,P,dt", PARAMS, ids=lambda v: str(v).replace("torch.", ""))
def test_operator_entrywise(row, P, dt):
    version = ROWS[row][3]
    if version is not None:
        probe = _variant(ROWS[row][0], _runs(row)[0][2], P).problem(Comm(), dt, "gpu")
        if not fused_supported(probe, version):
            pytest.skip(f"fused{version} does not cover this element / mesh / dtype")
    got = measure(row, P, dt)
    ratios = {k: v for k, v in got.items() if not isinstance(v, str)}
    one = max(v for k, v in ratios.items() if k[0] == 1)
    multi = max(v for k, v in ratios.items() if k[0] > 1)
    print(f"{row} P{P} {dt}: ratio one rank {one:.3g}, partitioned {multi:.3g}; per run "
          + ", ".join(f"{k[0]}/{k[1]}{k[2]}: {v if isinstance(v, str) else format(v, '.3g')}"
                      for k, v in got.items()))
    refused = sorted(k for k, v in got.items() if isinstance(v, str))
    assert refused == sorted(REFUSED.get((row, P, dt), [])), refused
    assert {k[:2] for k in ratios} == set(oref.LAYOUTS)      # every layout ran the instance
    K = _K(row, P, dt)
    assert max(one, multi) <= K, (row, P, dt, one, multi, K)
    # a cut may not cost a row more than 2 x its one-rank ratio (recorded values)
    assert MEASURED[(row, P, dt)][1] <= 2 * MEASURED[(row, P, dt)][0]


# ---------------------------------------------- diagonal and right-hand side
def _setup_job(comm, case, dt, partition):
    pb = case.problem(comm, dt, "gpu", partition)
    d = pb.to_global_array(pb.operator_diagonal())
    b = pb.to_global_array(pb.assemble_rhs())
    torch.cuda.synchronize()
    return d, b, pb.lat.n, pb.lat.gh, pb.lat.pgrid


@pytest.mark.parametrize("dt", BOTH, ids=["f64", "f32"])
@pytest.mark.parametrize("P", range(1, 8))
def test_diagonal_and_rhs_entrywise(P, dt):
    """`operator_diagonal()` (relative per entry, K_DIAG eps) and
    `assemble_rhs()` (K_RHS eps of the magnitude of its terms) against the
    one-rank FP64 host values, on the same layouts."""
    for ranks, partition in oref.LAYOUTS:
        for nc in oref.MESHES[:2]:
            case = _variant("pert", nc, P)
            host_d = _host_diagonal(nc, P, 1, False, case.pert, case.coef)
            oref.rhs_reference(case)
            res = run_threaded(ranks, _setup_job, case, dt, partition)
            d, b = res[0][:2]
            for r in res:
                assert np.array_equal(r[0], d) and np.array_equal(r[1], b)
            if ranks > 1:
                assert any(p > 1 and n == 1 for r in res for p, n in zip(r[4], r[2]))
            if ranks == 8:
                assert {r[3] for r in res} == ALL_GH
            rd, rb = oref.check_diagonal(d, host_d, dt), oref.check_rhs(b, case, dt)
            print(f"P{P} {dt} {ranks}/{partition} {nc}: diagonal {rd:.3g} eps (relative), "
                  f"rhs {rb:.3g} eps of its terms")
