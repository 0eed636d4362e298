"""Every CG loop, entry by entry against k iterations of the FP64 one-rank host
recurrence (tests/cg_ref.py), on partitioned lattices with one-cell blocks: one
rank, 4 ranks with x whole (the native runtime's split schedule, here on blocks
without an interior tile) and a 2 x 2 x 2 grid with all eight ghost patterns,
threaded ranks on one GPU.

b and x0 are random, zero on the Dirichlet dofs, and hold NaN on every ghost
plane and in the storage padding: a loop owns the owned box only.  Totals of 3
and 4 iterations in the call splits iterate(1) + iterate(2), iterate(2) +
iterate(2) and iterate(4), each call followed by wait(): the lagged x update is
flushed between calls, fused5's paired update ends with 1 and with 2 pending
terms, the rho slots end on both parities.

Bound: |x_i - x_k,i| <= K eps_T s_k,i and |rr - r_k.r_k| <= K eps_T sum |r_k| t_k
with K = 10 x the largest ratio measured on an MI355X over the row's layouts,
meshes and call splits (`MEASURED`, profiles/partitioned_cg_entrywise.md), never
below 8; the 10 x covers another summation order, FMA contraction, the order of
dofmap's atomics and the tiled r.r order.  Every run is first checked at
K_CAP = 640, and no measured ratio above 64 is recorded."""

import contextlib
from typing import NamedTuple

import numpy as np
import pytest
import torch

import cg_ref as cref
from cg_ref import Case
from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.fused import FusedLaplacianGPU
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianGPU
from benchmark_dolfinx_amd.models.unstructured import DofmapLaplacianGPU
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.parallel.comm import run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
BOTH = (F64, F32)
ALL_GH = {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
# call splits per total; the single call comes last
SPLITS = {3: [(1, 2)], 4: [(2, 2), (4,)]}


def _variant(kind, nc, P):
    return {"box-const": Case(nc, P, 1, 0.0, "constant"),
            "box-rand": Case(nc, P, 1, 0.0, "random"),
            "pert": Case(nc, P, 1, 0.2, "random"),        # x-trilinear cells
            "pert-q0": Case(nc, P, 0, 0.2, "constant"),   # GLL collocation: phi0 = I
            "shear": Case(nc, P, 1, 0.0, "random", 0.5)}[kind]


class Row(NamedTuple):
    kind: str            # mesh variant
    degrees: tuple
    dtypes: tuple
    build: object        # (pb, runtime) -> operator
    instance: tuple      # (name, geometry) every rank has to report
    runtime: str         # native | lattice (native, BDX_TILED=0) | python | generic
    precond: object = None
    tiled: bool = False  # tiled storage by default (where the tile plane is 16-byte)


def _fused(version, **kw):
    return lambda pb, runtime: FusedLaplacianGPU(pb, "otf", version, runtime=runtime, **kw)


def _dofmap(geometry):
    return lambda pb, runtime: DofmapLaplacianGPU(pb, geometry, runtime=runtime)


def _rows():
    rows = {}

    def add(name, runtimes, *a, **kw):
        for rt, degrees in runtimes.items():
            rows[f"{name}/{rt}"] = Row(a[0], tuple(degrees), *a[1:], runtime=rt, **kw)

    f5 = {"native": (3, 4, 6), "lattice": (3, 4, 6), "python": (3, 4, 6)}     # tiles 4x4, 2x4, 2x2
    add("fused5-const", f5, "box-const", BOTH, _fused(5), ("fused5", "otf-affine"), tiled=True)
    add("fused5-rand", f5, "box-rand", BOTH, _fused(5), ("fused5", "otf-affine"), tiled=True)
    f3 = {"native": (1, 2, 3, 6), "python": (3,)}
    add("fused3-affine", f3, "box-rand", BOTH, _fused(3), ("fused3", "otf-affine"))
    # P = 1 runs on (5, 3, 4) only (cg_ref's refusal), which leaves the sheared mesh none
    add("fused3-sheared", {"native": (2, 3, 6), "python": (3,)}, "shear", BOTH, _fused(3),
        ("fused3", "otf-affine"))
    add("fused3-xtri", f3, "pert", BOTH, _fused(3), ("fused3", "otf-xtrilinear"), tiled=True)
    add("fused3-general", f3, "pert", BOTH, _fused(3, affine=False, xtri=False),
        ("fused3", "otf-general"))
    f2 = {"native": (2, 3), "python": (2, 3)}
    add("fused2-general", f2, "pert", (F64,), _fused(2, affine=False), ("fused2", "otf-general"))
    add("fused2-xtri-q0", f2, "pert-q0", (F64,), _fused(2), ("fused2", "otf-xtrilinear"))
    add("fused-v1", {"python": (3,)}, "box-const", (F64,), _fused(1), ("fused", "otf"))
    pc = {"native": (3, 6), "python": (3, 6)}
    add("jacobi-fused5", pc, "box-rand", BOTH, _fused(5), ("fused5", "otf-affine"),
        precond="fused", tiled=True)
    add("jacobi-fused3-xtri", pc, "pert", BOTH, _fused(3), ("fused3", "otf-xtrilinear"),
        precond="fused", tiled=True)
    dm = {"native": (3, 6), "python": (3, 6)}
    for geometry in ("otf", "stored"):
        add(f"dofmap-valu-{geometry}", dm, "pert", BOTH, _dofmap(geometry),
            ("dofmap", f"dofmap-{geometry}"))
        add(f"dofmap-mfma-{geometry}", dm, "pert", (F64,), _dofmap(geometry),
            ("dofmap", f"dofmap-{geometry}"))
    v1 = lambda pb, runtime: MatFreeLaplacianGPU(pb, "otf")               # noqa: E731
    add("generic-plain", {"generic": (3,)}, "pert", BOTH, v1, ("v1", "otf"))
    add("generic-jacobi", {"generic": (3,)}, "pert", BOTH, v1, ("v1", "otf"), precond="generic")
    return rows


ROWS = _rows()
PARAMS = [(name, P, dt) for name, row in ROWS.items() for P in row.degrees for dt in row.dtypes]
NATIVE = [p for p in PARAMS if ROWS[p[0]].runtime in ("native", "lattice")]


def _runs(row, P):
    """(ranks, partition, cells, call splits): every layout on every mesh the
    reference allows at this degree; 8 ranks skip the (5, 3, 4) x-march."""
    meshes = [cref.SHEAR_MESH] if ROWS[row].kind == "shear" else cref.MESHES
    out = []
    for ranks, partition in cref.LAYOUTS:
        for nc in meshes:
            if ranks == 8 and nc == (5, 3, 4):
                continue
            case = _variant(ROWS[row].kind, nc, P)
            splits = [s for k, ss in SPLITS.items() if cref.allowed(case, k) for s in ss]
            if splits:
                out.append((ranks, partition, nc, tuple(splits)))
    return out


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


def _new_cg(pb, precond):
    if precond is None:
        return DeviceCG(pb)
    return DeviceCG(pb, "jacobi", loop=precond)


def job(comm, case, name, dt, partition, splits):
    row = ROWS[name]
    pb = case.problem(comm, dt, "gpu", partition)
    refusal = None
    try:
        op = row.build(pb, "python" if row.runtime == "python" else "native")
    except (ValueError, RuntimeError) as e:      # HipError is a RuntimeError
        refusal = f"{type(e).__name__}: {e}"
    # a refusal has to be the same on every rank (and is agreed on before the
    # collective loop); the automatic choice still has to work there
    refusals = comm.gather_objects(refusal)
    assert len(set(refusals)) == 1, refusals
    if refusal is not None:
        op = make_operator(pb)
    jacobi = row.precond is not None
    out = []
    for split in splits:
        k = sum(split)
        b, x = cref.local_vectors(pb, cref.reference(case, dt, k, jacobi))
        b0 = b.clone()
        cg = _new_cg(pb, row.precond)            # a new loop state (and runtime) per split
        cg.start(op, x, b)
        for n in split:
            cg.iterate(n)
            cg.wait()
        assert cg.it == k
        rr = cg.residual_norm2()
        got = pb.to_global_array(x)
        unchanged = torch.equal(_bits(pb.owned(b)), _bits(pb.owned(b0)))
        rt = getattr(op, "_rt", None)
        loop = (getattr(op, "runtime", "generic"), rt is not None,
                rt.transport if rt else None, rt.tiled if rt else None,
                rt.overlap if rt else None, rt.graphs if rt else None)
        out.append((split, got, rr, unchanged, loop))
    third = getattr(op, "core", None) if name.startswith("dofmap") else None
    # tiles without a ghost plane (fused) / cells that touch none (dofmap)
    if hasattr(op, "nty"):
        interior = (op.nty - pb.lat.gh[1]) * (op.ntz - pb.lat.gh[2])
        plane16 = (op.sy * op.sz * op.pb.dtype.itemsize) % 16 == 0
    else:
        interior = int(op.inner.numel()) if hasattr(op, "inner") else None
        plane16 = False
    rec = (getattr(op, "name", "v1"), op.geometry, third, pb.lat.n, pb.lat.gh, pb.lat.pgrid,
           interior, plane16)
    if hasattr(op, "close"):
        op.close()
    torch.cuda.synchronize()
    return out, rec, refusal


def _expected_loop(name, dt, ranks, rec, graph):
    """(runtime, has a native runtime, transport, tiled) a rank has to report."""
    row = ROWS[name]
    if row.runtime == "generic":
        return ("generic", False, None, None)
    if row.runtime == "python":
        return ("python", False, None, None)
    tiled = row.tiled and row.runtime == "native" and rec[7]
    return ("native", True, "thread" if ranks > 1 else "none", tiled)


def measure(name, P, dt, graph=False):
    """{(ranks, partition, cells, split): (entry ratio, scalar ratio) or the
    refusal} of one row and the per-rank records, with every assertion but the
    row's own bound.  `graph`: one rank under BDX_GRAPH=1 (set by the caller)."""
    row = ROWS[name]
    jacobi = row.precond is not None
    out, records = {}, {}
    with _dofmap_core(name):
        for ranks, partition, nc, splits in _runs(name, P):
            if graph and ranks > 1:
                continue
            case = _variant(row.kind, nc, P)
            for k in {sum(s) for s in splits}:
                cref.reference(case, dt, k, jacobi)       # cached, before the threads start
            res = run_threaded(ranks, job, case, name, dt, partition, splits)
            key = (ranks, partition, nc)
            runs0, rec0, refusal = res[0]
            records[key] = [(rec[3:7], [r[4] for r in runs]) for runs, rec, _ in res]
            for runs, rec, _ in res:
                assert rec[:3] == rec0[:3], (key, rec, rec0)   # every rank built the same instance
                for (split, got, rr, unchanged, loop), (_, got0, rr0, _, _) in zip(runs, runs0):
                    assert np.array_equal(got, got0), (key, split)   # ... gathered the same array
                    assert rr == rr0, (key, split, rr, rr0)          # ... holds the same r.r
                    assert unchanged, (key, split)                   # ... and left b alone
            if ranks > 1:
                assert any(p > 1 and n == 1 for _, rec, _ in res
                           for p, n in zip(rec[5], rec[3])), (key, [r[1] for r in res])
            if ranks == 8:
                assert {rec[4] for _, rec, _ in res} == ALL_GH, key
            want = row.instance + (("mfma" if "mfma" in name and dt == F64 else "valu")
                                   if name.startswith("dofmap") else None,)
            for split, got, rr, _, _ in runs0:
                k = sum(split)
                if refusal is not None:           # the automatic choice works
                    cref.check(got, case, dt, k, cref.K_CAP, jacobi, rr=rr)
                    out[key + (split,)] = refusal
                    continue
                assert rec0[:3] == want, (key, rec0, want)
                # finite, Dirichlet zeros kept, and no gross error
                out[key + (split,)] = cref.check(got, case, dt, k, cref.K_CAP, jacobi, rr=rr)
            if refusal is not None:
                continue
            # no silent fallback: every rank ran the loop the row names
            for runs, rec, _ in res:
                for split, _, _, _, loop in runs:
                    assert loop[:4] == _expected_loop(name, dt, ranks, rec, graph), \
                        (key, split, loop, rec)
                    if graph:
                        # graphs replay the steady state: an iteration with a
                        # lagged x term pending (on tiled storage the staggered
                        # pairing keeps its terms across calls and is periodic
                        # from the third iteration on), reached in every split
                        assert loop[5] is True, (key, split, loop)
            if (ranks, partition) == (4, "yz") and row.runtime in ("native", "lattice"):
                # x whole: a rank with an upper y / z neighbour runs the split
                # schedule, and on these blocks its interior set is empty
                for runs, rec, _ in res:
                    assert name.startswith("dofmap") or all(
                        r[4][4] == bool(rec[4][1] or rec[4][2]) for r in runs), (key, rec)
                assert any(runs[0][4][4] and rec[6] == 0 for runs, rec, _ in res), \
                    (key, records[key])
    return out, records


# Largest ratios measured on an MI355X per (row, P, dtype): (entry ratio on one
# rank, on 4 / yz and 8 / xyz), (scalar ratio likewise);
# profiles/partitioned_cg_entrywise.md has them per layout.
MEASURED = {
    ("fused5-const/native", 3, F64): ((1.03, 1.03), (0.0079, 0.00988)),
    ("fused5-const/native", 3, F32): ((0.273, 0.361), (0.00352, 0.00351)),
    ("fused5-const/native", 4, F64): ((0.323, 0.434), (0.00851, 0.00711)),
    ("fused5-const/native", 4, F32): ((0.236, 0.236), (0.00388, 0.00402)),
    ("fused5-const/native", 6, F64): ((0.954, 0.763), (0.0204, 0.0149)),
    ("fused5-const/native", 6, F32): ((0.375, 0.289), (0.00123, 0.00116)),
    ("fused5-const/lattice", 3, F64): ((1.03, 0.686), (0.00593, 0.0079)),
    ("fused5-const/lattice", 3, F32): ((0.273, 0.361), (0.00352, 0.00351)),
    ("fused5-const/lattice", 4, F64): ((0.418, 0.35), (0.00356, 0.00711)),
    ("fused5-const/lattice", 4, F32): ((0.274, 0.274), (0.00388, 0.00402)),
    ("fused5-const/lattice", 6, F64): ((0.954, 0.763), (0.0204, 0.0149)),
    ("fused5-const/lattice", 6, F32): ((0.375, 0.375), (0.00123, 0.00116)),
    ("fused5-const/python", 3, F64): ((1.03, 0.686), (0.00593, 0.0079)),
    ("fused5-const/python", 3, F32): ((0.241, 0.361), (0.00352, 0.00351)),
    ("fused5-const/python", 4, F64): ((0.35, 0.35), (0.00356, 0.00711)),
    ("fused5-const/python", 4, F32): ((0.274, 0.274), (0.00388, 0.00402)),
    ("fused5-const/python", 6, F64): ((0.94, 0.763), (0.0204, 0.0149)),
    ("fused5-const/python", 6, F32): ((0.321, 0.321), (0.00123, 0.00116)),
    ("fused5-rand/native", 3, F64): ((1.28, 1.02), (0.0167, 0.0144)),
    ("fused5-rand/native", 3, F32): ((0.276, 0.276), (0.00255, 0.00277)),
    ("fused5-rand/native", 4, F64): ((0.827, 0.827), (0.0181, 0.0148)),
    ("fused5-rand/native", 4, F32): ((0.567, 0.647), (0.00372, 0.00394)),
    ("fused5-rand/native", 6, F64): ((1.43, 1.02), (0.0291, 0.0302)),
    ("fused5-rand/native", 6, F32): ((0.487, 0.487), (0.00373, 0.00376)),
    ("fused5-rand/lattice", 3, F64): ((1.28, 1.15), (0.0144, 0.0144)),
    ("fused5-rand/lattice", 3, F32): ((0.209, 0.237), (0.00255, 0.00277)),
    ("fused5-rand/lattice", 4, F64): ((0.869, 0.869), (0.0115, 0.0131)),
    ("fused5-rand/lattice", 4, F32): ((0.567, 0.567), (0.00372, 0.00394)),
    ("fused5-rand/lattice", 6, F64): ((1.08, 1.07), (0.0202, 0.0179)),
    ("fused5-rand/lattice", 6, F32): ((0.487, 0.487), (0.00373, 0.00376)),
    ("fused5-rand/python", 3, F64): ((1.28, 1.02), (0.0144, 0.0144)),
    ("fused5-rand/python", 3, F32): ((0.276, 0.276), (0.00255, 0.00277)),
    ("fused5-rand/python", 4, F64): ((1.1, 1.1), (0.0115, 0.0131)),
    ("fused5-rand/python", 4, F32): ((0.567, 0.567), (0.00372, 0.00394)),
    ("fused5-rand/python", 6, F64): ((1.08, 1.02), (0.0202, 0.0179)),
    ("fused5-rand/python", 6, F32): ((0.487, 0.487), (0.00373, 0.00376)),
    ("fused3-affine/native", 1, F64): ((0.158, 0.164), (0.00147, 0.00295)),
    ("fused3-affine/native", 1, F32): ((0.0926, 0.141), (0.00217, 6.67e-05)),
    ("fused3-affine/native", 2, F64): ((0.394, 0.398), (0.0127, 0.0255)),
    ("fused3-affine/native", 2, F32): ((0.24, 0.262), (0.00963, 0.0109)),
    ("fused3-affine/native", 3, F64): ((0.848, 0.848), (0.0167, 0.012)),
    ("fused3-affine/native", 3, F32): ((0.273, 0.273), (0.00345, 0.00337)),
    ("fused3-affine/native", 6, F64): ((0.838, 0.847), (0.0151, 0.00635)),
    ("fused3-affine/native", 6, F32): ((0.575, 0.575), (0.0025, 0.00261)),
    ("fused3-affine/python", 3, F64): ((0.848, 0.848), (0.0167, 0.012)),
    ("fused3-affine/python", 3, F32): ((0.273, 0.273), (0.00345, 0.00337)),
    ("fused3-sheared/native", 2, F64): ((0.336, 0.357), (0.00794, 0.0119)),
    ("fused3-sheared/native", 2, F32): ((0.228, 0.178), (0.00403, 0.00296)),
    ("fused3-sheared/native", 3, F64): ((0.239, 0.35), (0.000708, 0.0111)),
    ("fused3-sheared/native", 3, F32): ((0.2, 0.22), (0.00163, 0.00164)),
    ("fused3-sheared/native", 6, F64): ((0.4, 0.481), (0.00172, 0.00862)),
    ("fused3-sheared/native", 6, F32): ((0.295, 0.295), (0.00118, 0.00171)),
    ("fused3-sheared/python", 3, F64): ((0.239, 0.35), (0.000708, 0.0111)),
    ("fused3-sheared/python", 3, F32): ((0.2, 0.22), (0.00163, 0.00164)),
    ("fused3-xtri/native", 1, F64): ((0.179, 0.157), (0, 0.00461)),
    ("fused3-xtri/native", 1, F32): ((0.146, 0.116), (0.00468, 0.00311)),
    ("fused3-xtri/native", 2, F64): ((0.406, 0.495), (0.0187, 0.00859)),
    ("fused3-xtri/native", 2, F32): ((0.305, 0.305), (0.00644, 0.00632)),
    ("fused3-xtri/native", 3, F64): ((0.535, 0.839), (0.0141, 0.00939)),
    ("fused3-xtri/native", 3, F32): ((0.409, 0.409), (0.00595, 0.00593)),
    ("fused3-xtri/native", 6, F64): ((0.832, 0.795), (0.00442, 0.0111)),
    ("fused3-xtri/native", 6, F32): ((0.389, 0.389), (0.00174, 0.0025)),
    ("fused3-xtri/python", 3, F64): ((0.535, 0.559), (0.0141, 0.00941)),
    ("fused3-xtri/python", 3, F32): ((0.409, 0.409), (0.00595, 0.00593)),
    ("fused3-general/native", 1, F64): ((0.147, 0.196), (0.00154, 0.00154)),
    ("fused3-general/native", 1, F32): ((0.115, 0.115), (0.00708, 0.00188)),
    ("fused3-general/native", 2, F64): ((0.742, 0.742), (0.0208, 0.025)),
    ("fused3-general/native", 2, F32): ((0.253, 0.253), (0.00169, 0.00598)),
    ("fused3-general/native", 3, F64): ((0.562, 0.556), (0.0188, 0.0141)),
    ("fused3-general/native", 3, F32): ((0.414, 0.414), (0.0015, 0.00126)),
    ("fused3-general/native", 6, F64): ((1.06, 0.905), (0.00936, 0.00468)),
    ("fused3-general/native", 6, F32): ((0.493, 0.493), (0.00449, 0.00442)),
    ("fused3-general/python", 3, F64): ((0.562, 0.556), (0.0188, 0.0141)),
    ("fused3-general/python", 3, F32): ((0.414, 0.414), (0.0015, 0.00126)),
    ("fused2-general/native", 2, F64): ((0.406, 0.482), (0.0167, 0.0193)),
    ("fused2-general/native", 3, F64): ((0.535, 0.556), (0.0139, 0.00939)),
    ("fused2-general/python", 2, F64): ((0.406, 0.482), (0.0167, 0.0193)),
    ("fused2-general/python", 3, F64): ((0.535, 0.556), (0.0139, 0.00939)),
    ("fused2-xtri-q0/native", 2, F64): ((0.39, 0.585), (0.0265, 0.0217)),
    ("fused2-xtri-q0/native", 3, F64): ((0.653, 0.848), (0.0213, 0.0165)),
    ("fused2-xtri-q0/python", 2, F64): ((0.39, 0.585), (0.0265, 0.0217)),
    ("fused2-xtri-q0/python", 3, F64): ((0.653, 0.848), (0.0213, 0.0165)),
    ("fused-v1/python", 3, F64): ((0.294, 0.346), (0.00395, 0.00929)),
    ("jacobi-fused5/native", 3, F64): ((0.343, 0.375), (0.00863, 0.0098)),
    ("jacobi-fused5/native", 3, F32): ((0.15, 0.16), (0.000414, 0.00147)),
    ("jacobi-fused5/native", 6, F64): ((0.429, 0.429), (0.0125, 0.0125)),
    ("jacobi-fused5/native", 6, F32): ((0.154, 0.154), (0.00181, 0.00177)),
    ("jacobi-fused5/python", 3, F64): ((0.343, 0.342), (0.00718, 0.00914)),
    ("jacobi-fused5/python", 3, F32): ((0.15, 0.16), (0.000414, 0.00147)),
    ("jacobi-fused5/python", 6, F64): ((0.429, 0.429), (0.0119, 0.0125)),
    ("jacobi-fused5/python", 6, F32): ((0.154, 0.154), (0.00181, 0.00177)),
    ("jacobi-fused3-xtri/native", 3, F64): ((0.257, 0.257), (0.00501, 0.00331)),
    ("jacobi-fused3-xtri/native", 3, F32): ((0.199, 0.185), (0.00119, 0.00146)),
    ("jacobi-fused3-xtri/native", 6, F64): ((0.266, 0.252), (0.00349, 0.00409)),
    ("jacobi-fused3-xtri/native", 6, F32): ((0.223, 0.214), (0.00154, 0.0016)),
    ("jacobi-fused3-xtri/python", 3, F64): ((0.257, 0.257), (0.00501, 0.00331)),
    ("jacobi-fused3-xtri/python", 3, F32): ((0.199, 0.185), (0.00119, 0.00146)),
    ("jacobi-fused3-xtri/python", 6, F64): ((0.268, 0.252), (0.00232, 0.00291)),
    ("jacobi-fused3-xtri/python", 6, F32): ((0.223, 0.214), (0.00154, 0.0016)),
    ("dofmap-valu-otf/native", 3, F64): ((0.556, 0.556), (0.0118, 0.011)),
    ("dofmap-valu-otf/native", 3, F32): ((0.392, 0.392), (0.0032, 0.00329)),
    ("dofmap-valu-otf/native", 6, F64): ((0.655, 0.648), (0.00702, 0.00468)),
    ("dofmap-valu-otf/native", 6, F32): ((0.517, 0.517), (0.00318, 0.00251)),
    ("dofmap-valu-otf/python", 3, F64): ((0.556, 0.556), (0.00894, 0.011)),
    ("dofmap-valu-otf/python", 3, F32): ((0.441, 0.441), (0.00241, 0.00283)),
    ("dofmap-valu-otf/python", 6, F64): ((0.655, 0.648), (0.00702, 0.00663)),
    ("dofmap-valu-otf/python", 6, F32): ((0.517, 0.517), (0.00291, 0.00261)),
    ("dofmap-mfma-otf/native", 3, F64): ((0.493, 0.556), (0.0188, 0.00894)),
    ("dofmap-mfma-otf/native", 6, F64): ((0.791, 0.791), (0.00936, 0.0155)),
    ("dofmap-mfma-otf/python", 3, F64): ((0.493, 0.834), (0.0165, 0.00795)),
    ("dofmap-mfma-otf/python", 6, F64): ((0.791, 0.791), (0.00702, 0.0155)),
    ("dofmap-valu-stored/native", 3, F64): ((0.368, 0.351), (0.0165, 0.0165)),
    ("dofmap-valu-stored/native", 3, F32): ((0.392, 0.392), (0.00351, 0.00318)),
    ("dofmap-valu-stored/native", 6, F64): ((0.783, 0.734), (0.0117, 0.00468)),
    ("dofmap-valu-stored/native", 6, F32): ((0.494, 0.49), (0.00341, 0.00421)),
    ("dofmap-valu-stored/python", 3, F64): ((0.368, 0.351), (0.0141, 0.0188)),
    ("dofmap-valu-stored/python", 3, F32): ((0.392, 0.392), (0.0028, 0.00282)),
    ("dofmap-valu-stored/python", 6, F64): ((0.783, 0.734), (0.0117, 0.00468)),
    ("dofmap-valu-stored/python", 6, F32): ((0.494, 0.49), (0.00343, 0.00421)),
    ("dofmap-mfma-stored/native", 3, F64): ((0.493, 0.556), (0.0188, 0.00795)),
    ("dofmap-mfma-stored/native", 6, F64): ((0.791, 0.791), (0.00936, 0.00884)),
    ("dofmap-mfma-stored/python", 3, F64): ((0.493, 0.493), (0.0188, 0.0141)),
    ("dofmap-mfma-stored/python", 6, F64): ((0.791, 0.791), (0.00936, 0.0155)),
    ("generic-plain/generic", 3, F64): ((0.432, 0.556), (0.0165, 0.0125)),
    ("generic-plain/generic", 3, F32): ((0.392, 0.356), (0.00816, 0.00689)),
    ("generic-jacobi/generic", 3, F64): ((0.251, 0.232), (0.0022, 0.0022)),
    ("generic-jacobi/generic", 3, F32): ((0.165, 0.16), (0.00164, 0.00162)),
}
REFUSED = {}   # (row, P, dtype) -> runs the instance refuses (none found)


def _K(key):
    entry, scalar = MEASURED[key]
    return max(8.0, 10.0 * max(entry)), max(8.0, 10.0 * max(scalar))


def _report(name, P, dt, got, records, tag=""):
    ratios = {k: v for k, v in got.items() if not isinstance(v, str)}
    fmt = lambda v: v if isinstance(v, str) else f"{v[0]:.3g}/{v[1]:.3g}"     # noqa: E731
    print(f"CGROW{tag} {name} P{P} {dt}: entry/scalar ratio per run "
          + ", ".join(f"{k[0]}/{k[1]}{k[2]}{k[3]}: {fmt(v)}" for k, v in got.items()))
    for key, ranks in records.items():
        print(f"CGREC{tag} {name} P{P} {dt} {key[0]}/{key[1]}{key[2]}: "
              + "; ".join(f"n{n} gh{gh} pgrid{pg} interior {it} "
                          f"tiled {loops[0][3]} overlap {loops[0][4]} "
                          f"graphs {[l[5] for l in loops]}"
                          for (n, gh, pg, it), loops in ranks))
    return ratios


@pytest.mark.parametrize("name,P,dt", PARAMS, ids=lambda v: str(v).replace("torch.", ""))
def test_cg_entrywise(monkeypatch, name, P, dt):
    monkeypatch.setenv("BDX_GRAPH", "0")
    if ROWS[name].runtime == "lattice":
        monkeypatch.setenv("BDX_TILED", "0")
    else:
        monkeypatch.delenv("BDX_TILED", raising=False)
    got, records = measure(name, P, dt)
    ratios = _report(name, P, dt, got, records)
    refused = sorted(k for k, v in got.items() if isinstance(v, str))
    assert refused == sorted(REFUSED.get((name, P, dt), [])), refused
    # every layout ran the loop (P = 1: the (5, 3, 4) x-march, which 8 ranks skip)
    assert {k[:2] for k in ratios} == set(cref.LAYOUTS if P > 1 else cref.LAYOUTS[:2])
    one = [max(v[i] for k, v in ratios.items() if k[0] == 1) for i in (0, 1)]
    multi = [max(v[i] for k, v in ratios.items() if k[0] > 1) for i in (0, 1)]
    print(f"CGMAX {name} P{P} {dt}: entry {one[0]:.3g} {multi[0]:.3g} scalar {one[1]:.3g} "
          f"{multi[1]:.3g}")
    Ke, Ks = _K((name, P, dt))
    assert max(one[0], multi[0]) <= Ke, (name, P, dt, one, multi, Ke)
    assert max(one[1], multi[1]) <= Ks, (name, P, dt, one, multi, Ks)
    # no recorded ratio above 64, and a cut may not cost a row more than 2 x
    # its one-rank ratio (recorded values)
    entry, scalar = MEASURED[(name, P, dt)]
    assert max(entry + scalar) <= 64
    assert entry[1] <= 2 * entry[0]


@pytest.mark.parametrize("name,P,dt", NATIVE, ids=lambda v: str(v).replace("torch.", ""))
def test_cg_entrywise_graph_replay(monkeypatch, name, P, dt):
    """The native rows once more on one rank with BDX_GRAPH=1: the steady-state
    iterations replayed from captured graphs, inside the row's bound."""
    monkeypatch.setenv("BDX_GRAPH", "1")
    if ROWS[name].runtime == "lattice":
        monkeypatch.setenv("BDX_TILED", "0")
    else:
        monkeypatch.delenv("BDX_TILED", raising=False)
    got, records = measure(name, P, dt, graph=True)
    ratios = _report(name, P, dt, got, records, tag="-GRAPH")
    assert ratios and len(ratios) == len(got)
    Ke, Ks = _K((name, P, dt))
    assert max(v[0] for v in ratios.values()) <= Ke
    assert max(v[1] for v in ratios.values()) <= Ks
