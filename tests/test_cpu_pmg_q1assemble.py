"""The degree-1 levels' 27-point stencils assembled without the CSR matrix
(`PoissonProblem.stencil27("direct")`, `PMultigrid(q1_assembly="direct")`,
`--pmg_q1_assembly direct`), CPU path: the host twin `bdx_cpu_stencil27_assemble`
entry by entry against the host's CSR stencil, its refusals, the option in the
cycle (coefficients, end to end, with the other options, threaded ranks, no
`CSROperator` in setup, defaults unchanged) and the CLI.  The `check_*` and
`rank_*` functions take the platform; tests/test_gpu_pmg_q1assemble.py runs
them on the device kernel.

Configurations (degree 1): the meshes (1, 1, 1), every row Dirichlet;
(2, 2, 2), one interior node; (2, 3, 70), rows of 71 nodes (two wave pieces,
the second partial) on strongly anisotropic cells; (5, 4, 3); the h-levels
(6, 7, 8) and (3, 3, 4) of (13, 15, 17) built by `PMultigrid(h_levels=-1)`
(merged pairs and triples of cells with their mean kappa); two threaded ranks
on (5, 4, 3), each rank's S against its own CSR stencil, ghost rows included.
Each with the tables (qmode, use_gauss) = (0, False), (1, False), (1, True),
with (perturbation 0.2, random kappa) and (0, constant kappa), in both dtypes.

Entrywise check.  S_ref is the host CSR stencil of the FP64 problem.  Rows that
are Dirichlet or storage padding, and entries whose neighbour is outside the
lattice or a Dirichlet column, equal the same-dtype CSR stencil exactly (0 or
1); S is allocated full of NaN, so an unwritten entry shows.  Every other row n
is measured as e = |S[p][n] - S_ref[p][n]| / (u S_ref[13][n]), u = 2^-53 /
2^-24, the row's diagonal being the scale (many off-diagonal entries vanish by
cancellation on undistorted cells; the row's absolute sum is 1 to 2.7
diagonals on these meshes).  The yardstick R is that metric of the reference
path itself, the FP32 host CSR stencil against S_ref, maximum over all the
configurations above, computed on every run (64.4 here: (2, 3, 70), Gauss,
perturbed; 0 to 9 on the other meshes).  The new path is held to max e <= 4 R
in both precisions: it adds the same <= 8 x 3 x nq^3 products per entry in
another order and with FMAs, so its distance from the exact entry obeys the
reference's rounding bound, and 4 covers the difference of two such errors
with room to spare; a wrong cell, weight, sign, neighbour or kappa shows as
1e5 or more in this unit.  FP64 has no higher-precision reference here and
gets the same 4 R in units of its own u.  Measured maxima:
profiles/pmg_q1assemble.md."""

import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models import poisson
from benchmark_dolfinx_amd.models.poisson import CSROperator, MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import stencil27
from benchmark_dolfinx_amd.ops.native import ptr
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import NAN, _bits
from test_cpu_pmg_q1stencil import DTYPES, FOUR, ITS, ROOT, UNIT, _env, _residual
from test_gpu_pmg_q1stencil import E2E_BOUND, FUSED3, FUSED5, _host_solve

MESHES = [(1, 1, 1), (2, 2, 2), (2, 3, 70), (5, 4, 3)]
H_MESH, H_CELLS = (13, 15, 17), [(6, 7, 8), (3, 3, 4)]
RANK_MESH = (5, 4, 3)
TABLES = [(0, False), (1, False), (1, True)]
GEOMETRY = [(0.2, "random"), (0.0, "constant")]
VARIANTS = [(q, g, p, c) for q, g in TABLES for p, c in GEOMETRY]
FACTOR = 4      # the bound is FACTOR x the yardstick (module docstring)


def _pb(nc, variant, dt, platform="cpu", comm=None, P=1, partition=None):
    qmode, gauss, pert, coef = variant
    return PoissonProblem(comm or Comm(), nc, P, qmode, gauss, dt, platform, pert, coef,
                          partition=partition)


def _h_levels(pb):
    """The problems of the h-levels under the degree-1 problem pb."""
    pmg = PMultigrid(pb, h_levels=-1)
    assert pmg.h_cells == H_CELLS
    out = [lv.pb for lv in pmg.levels[1:]]
    pmg.close()
    return out


def _csr(pb) -> np.ndarray:
    return stencil27(CSROperator(pb), pb.lat)


def assemble(pb) -> torch.Tensor:
    """The new path through the launcher, into an S full of NaN."""
    S = torch.full((27, pb.lat.nstore), NAN, dtype=pb.dtype).to(pb.device)
    k = pb.kernels
    k.stencil27_assemble(pb.xv, pb.kappa, pb.kc, S)
    return S


# ------------------------------------------------------------- the metric
def _fixed(lat):
    """(rows, entries): the storage rows that are Dirichlet or padding, and the
    entries (27, nstore) that are 0 or 1 by definition."""
    L0, L1, L2, ld = (int(x) for x in (*lat.L, lat.ld))
    bc = np.asarray(lat.bc_mask(), dtype=bool)
    rows = np.ones((L0, L1, ld), dtype=bool)
    rows[:, :, :L2] = bc
    entries = np.empty((27, L0, L1, ld), dtype=bool)
    for p in range(27):
        d = (p // 9 - 1, p // 3 % 3 - 1, p % 3 - 1)
        to = tuple(slice(max(0, -s), n - max(0, s)) for s, n in zip(d, (L0, L1, L2)))
        fr = tuple(slice(max(0, s), n - max(0, -s)) for s, n in zip(d, (L0, L1, L2)))
        nb = np.ones((L0, L1, L2), dtype=bool)          # outside the lattice
        nb[to] = bc[fr]                                 # or a Dirichlet column
        entries[p] = rows
        entries[p, :, :, :L2] |= nb
    return rows.reshape(-1), entries.reshape(27, -1)


def entry_metric(lat, S, S_ref, u, S_exact=None, other=None) -> float:
    """max e over the free rows (module docstring); with S_exact, the entries
    fixed by definition are first held to it bit for bit.  With `other`, the
    distance is taken from it instead of from S_ref, whose diagonal stays the
    scale (two implementations of the new path against each other)."""
    S, S_ref = np.asarray(S), np.asarray(S_ref)
    assert S.shape == S_ref.shape == (27, lat.nstore) and S_ref.dtype == np.float64
    rows, entries = _fixed(lat)
    if S_exact is not None:
        assert S.dtype == S_exact.dtype
        assert np.array_equal(S[entries], S_exact[entries]), "an entry fixed by definition"
        assert np.isin(S[entries], (0.0, 1.0)).all()
    free = ~rows
    if not free.any():
        return 0.0
    scale = S_ref[13][free]
    assert (scale > 0).all()
    base = S_ref if other is None else np.asarray(other).astype(np.float64)
    e = np.abs(S[:, free].astype(np.float64) - base[:, free]) / (u * scale)
    assert np.isfinite(e).all()
    return float(e.max())


# ------------------------------------- the references and the yardstick, once
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cpu_reference(dt):
    """label -> the host CSR stencil in dt of every one-rank configuration."""
    out = {}
    for v in VARIANTS:
        for nc in MESHES:
            out[(nc, v)] = _frozen(_csr(_pb(nc, v, dt)))
        for lpb in _h_levels(_pb(H_MESH, v, dt)):
            out[(tuple(int(n) for n in lpb.lat.n), v)] = _frozen(_csr(lpb))
    return out


def rank_reference(comm, dt, partition):
    return {v: _csr(_pb(RANK_MESH, v, dt, comm=comm, partition=partition)) for v in VARIANTS}


@functools.lru_cache(maxsize=None)
def cpu_rank_reference(dt, partition):
    return run_threaded(2, rank_reference, dt, partition)


@functools.lru_cache(maxsize=None)
def yardstick() -> float:
    """R: the FP32 host CSR stencil against the FP64 one, every configuration."""
    worst = {}
    r32, r64 = cpu_reference(torch.float32), cpu_reference(torch.float64)
    for v in VARIANTS:
        for nc in MESHES:
            lat = _pb(nc, v, torch.float32).lat
            worst[(nc, v)] = entry_metric(lat, r32[(nc, v)], r64[(nc, v)], UNIT[torch.float32])
        for lpb in _h_levels(_pb(H_MESH, v, torch.float32)):
            key = (tuple(int(n) for n in lpb.lat.n), v)
            worst[key] = entry_metric(lpb.lat, r32[key], r64[key], UNIT[torch.float32])

    k32, k64 = cpu_rank_reference(torch.float32, "xyz"), cpu_rank_reference(torch.float64, "xyz")

    def ranks(comm):
        out = {}
        for v in VARIANTS:
            lat = _pb(RANK_MESH, v, torch.float32, comm=comm, partition="xyz").lat
            out[v] = entry_metric(lat, k32[comm.rank][v], k64[comm.rank][v], UNIT[torch.float32])
        return out
    for r, d in enumerate(run_threaded(2, ranks)):
        worst.update({(f"rank {r} of 2", v): e for v, e in d.items()})
    key = max(worst, key=worst.get)
    print(f"yardstick R = {worst[key]:.1f} at {key}")
    return worst[key]


def test_yardstick_is_the_reference_paths_own_error():
    R = yardstick()
    assert np.isfinite(R) and R >= 1.0


# ------------------------------------------------ 1. the kernel, entry by entry
def check_entries(platform, pb, S_same, S_ref, label) -> float:
    """pb's new-path stencil against the references; returns max e."""
    S = assemble(pb)
    assert torch.equal(_bits(pb.stencil27("direct").cpu()), _bits(S.cpu())), "the public method"
    e = entry_metric(pb.lat, S.cpu().numpy(), S_ref, UNIT[pb.dtype], S_same)
    assert e <= FACTOR * yardstick(), f"{platform} {label}: max e = {e:.1f}"
    return e


def check_mesh(platform, nc, dt) -> float:
    worst = 0.0
    for v in VARIANTS:
        worst = max(worst, check_entries(platform, _pb(nc, v, dt, platform),
                                         cpu_reference(dt)[(nc, v)],
                                         cpu_reference(torch.float64)[(nc, v)], (nc, v)))
    print(f"stencil27_assemble {platform} {nc} {dt}: max e = {worst:.2f} "
          f"(bound {FACTOR} R = {FACTOR * yardstick():.1f})")
    return worst


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
def test_host_twin_entries(nc, dt):
    check_mesh("cpu", nc, dt)


def check_h_levels(platform, dt) -> float:
    worst = 0.0
    for v in VARIANTS:
        for lpb in _h_levels(_pb(H_MESH, v, dt, platform)):
            key = (tuple(int(n) for n in lpb.lat.n), v)
            assert lpb.kc is not None or v[3] == "constant"
            worst = max(worst, check_entries(platform, lpb, cpu_reference(dt)[key],
                                             cpu_reference(torch.float64)[key], key))
    print(f"stencil27_assemble {platform} h-levels {H_CELLS} {dt}: max e = {worst:.2f} "
          f"(bound {FACTOR} R = {FACTOR * yardstick():.1f})")
    return worst


@pytest.mark.parametrize("dt", DTYPES)
def test_host_twin_entries_on_h_levels(dt):
    check_h_levels("cpu", dt)


def rank_entries(comm, platform, dt, same, ref, partition):
    worst, ghost_rows = 0.0, 0
    for v in VARIANTS:
        pb = _pb(RANK_MESH, v, dt, platform, comm, partition=partition)
        worst = max(worst, check_entries(platform, pb, same[comm.rank][v], ref[comm.rank][v],
                                         (comm.rank, v)))
        ghost_rows = int(np.prod(pb.lat.L)) - int(np.prod(pb.lat.owned_hi))
    return worst, ghost_rows


def check_two_ranks(platform, dt) -> float:
    part = "yz" if platform == "gpu" else "xyz"         # the platforms' defaults
    yardstick()                                         # not inside the rank threads
    res = run_threaded(2, rank_entries, platform, dt, cpu_rank_reference(dt, part),
                       cpu_rank_reference(torch.float64, part), part)
    assert max(g for _, g in res) > 0                   # a rank has ghost rows
    worst = max(e for e, _ in res)
    print(f"stencil27_assemble {platform} two ranks on {RANK_MESH} {dt}: max e = {worst:.2f}")
    return worst


@pytest.mark.parametrize("dt", DTYPES)
def test_host_twin_entries_on_two_ranks(dt):
    check_two_ranks("cpu", dt)


def check_refusals(platform, dt):
    """A degree-2 and a tiled descriptor, nq = 4 and each null pointer: refused,
    nothing written; then the good call is accepted."""
    v = (1, False, 0.2, "random")
    pb, pb2 = _pb((2, 2, 2), v, dt, platform), _pb((2, 2, 2), v, dt, platform, P=2)
    suf = "f64" if dt == torch.float64 else "f32"
    S = torch.full((27, pb.lat.nstore), NAN, dtype=dt).to(pb.device)
    t = {n: np.ascontiguousarray(getattr(pb.tables, a), dtype=np.float64)
         for n, a in (("phi0", "phi0"), ("dphi1", "dphi1"), ("wts", "qwts"), ("qpts", "qpts"))}
    latd, latd2 = pb.lat.as_int64(), pb2.lat.as_int64()
    tiled = latd.copy()
    tiled[17:21] = (2, 2, (pb.lat.L[2] + 1) // 2, pb.lat.L[0] * 4)
    if platform == "gpu":
        fn, st, invalid = getattr(native.hip(), f"bdx_stencil27_assemble_{suf}"), \
            (torch.cuda.current_stream().cuda_stream,), (1,)       # hipErrorInvalidValue
    else:
        fn, st, invalid = getattr(native.host(), f"bdx_cpu_stencil27_assemble_{suf}"), (), None

    def call(latd=latd, nq=pb.tables.nq, phi0=t["phi0"], dphi1=t["dphi1"], wts=t["wts"],
             qpts=t["qpts"], xv=pb.xv, S=S):
        return fn(ptr(latd), nq, ptr(phi0), ptr(dphi1), ptr(wts), ptr(qpts), ptr(xv), pb.kappa,
                  ptr(pb.kc), ptr(S), *st)
    bad = [dict(latd=latd2), dict(latd=tiled), dict(nq=4), dict(nq=1)]
    bad += [{n: None} for n in ("latd", "phi0", "dphi1", "wts", "qpts", "xv", "S")]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0 and (invalid is None or rc in invalid), kw
    if platform == "gpu":
        torch.cuda.synchronize()
    assert torch.isnan(S.cpu()).all()                   # nothing was launched
    assert call() == 0
    if platform == "gpu":
        torch.cuda.synchronize()
    assert torch.isfinite(S.cpu()).all()
    # the launchers raise
    k2 = pb2.kernels
    S2 = torch.zeros((27, pb2.lat.nstore), dtype=dt).to(pb2.device)
    with pytest.raises((ValueError, RuntimeError)):
        k2.stencil27_assemble(pb2.xv, pb2.kappa, pb2.kc, S2)
    k = pb.kernels
    with pytest.raises(TypeError):
        k.stencil27_assemble(pb.xv, pb.kappa, pb.kc, S[:26])
    with pytest.raises(TypeError):
        k.stencil27_assemble(pb.xv[:-1], pb.kappa, pb.kc, S)
    with pytest.raises(TypeError):
        k.stencil27_assemble(pb.xv, pb.kappa, pb.kc[:-1], S)


@pytest.mark.parametrize("dt", DTYPES)
def test_host_twin_refusals(dt):
    check_refusals("cpu", dt)


def check_method(platform, dt):
    """`stencil27("csr")` is today's expression bit for bit; the default is
    "csr"; another value and another degree raise."""
    v = (1, False, 0.2, "random")
    pb = _pb((5, 4, 3), v, dt, platform)
    old = torch.from_numpy(stencil27(CSROperator(pb), pb.lat)).to(pb.device)
    for S in (pb.stencil27(), pb.stencil27("csr"), pb.stencil27(assembly="csr")):
        assert S.dtype == dt and S.device == pb.device and tuple(S.shape) == (27, pb.lat.nstore)
        assert torch.equal(_bits(S.cpu()), _bits(old.cpu()))
    D = pb.stencil27("direct")
    assert D.dtype == dt and D.device == pb.device and tuple(D.shape) == (27, pb.lat.nstore)
    for bad in ("device", "", None, 1, True):
        with pytest.raises(ValueError):
            pb.stencil27(bad)
    for how in ("csr", "direct"):
        with pytest.raises(ValueError):
            _pb((2, 2, 2), v, dt, platform, P=2).stencil27(how)


@pytest.mark.parametrize("dt", DTYPES)
def test_stencil27_method(dt):
    check_method("cpu", dt)


# ------------------------------------------------------------- 2. the cycle
def _solve(pb, pmg, kernel="auto"):
    """ITS iterations of pmg-PCG on pb's platform; the global x."""
    x = pb.new_vector()
    if pb.platform == "gpu":
        from benchmark_dolfinx_amd.solvers.cg import DeviceCG
        op = make_operator(pb, kernel, "otf" if kernel != "auto" else "auto")
        if kernel != "auto":
            assert getattr(op, "name", None) == kernel
        cg = DeviceCG(pb, "pmg", pmg=pmg)
        cg.solve(op, x, pb.assemble_rhs(), ITS)
        cg.wait()
        if hasattr(op, "close"):
            op.close()
    else:
        cg_solve(MatFreeLaplacianCPU(pb), pb, x, pb.assemble_rhs(), ITS, precond=pmg.apply)
    return pb.to_global_array(x)


def rank_cycle(comm, platform, case, cycle, kw):
    """The direct hierarchy against the csr one (coefficients exactly) and
    against the FP64 host solve on the default hierarchy (E2E_BOUND)."""
    kernel, nc, P, pert, coef = case
    pb = PoissonProblem(comm, nc, P, 1, False, torch.float64, platform, pert, coef)
    kw = dict(dict(h_levels=-1, cycle_dtype=cycle, q1_operator="stencil"), **kw)
    d, c = PMultigrid(pb, q1_assembly="direct", **kw), PMultigrid(pb, q1_assembly="csr", **kw)
    assert d.lambda_max == c.lambda_max
    assert [lv.coef for lv in d.levels] == [lv.coef for lv in c.levels]
    assert [lv.S is not None for lv in d.levels] == [lv.S is not None for lv in c.levels]
    for lv in d.levels:
        assert lv.S is None or (lv.S.dtype == cycle and lv.S.device == pb.device)
    assert d.info() == dict(c.info(), q1_assembly="direct") and "q1_assembly" not in c.info()
    x = _solve(pb, d, kernel if comm.size == 1 else "auto")
    stencils = sum(lv.S is not None for lv in d.levels) + (len(d.tail.S) if d.tail else 0)
    for p in (d, c):
        p.close()
    return x, stencils


def check_cycle(platform, case, cycle, ranks=1, **kw):
    _, nc, P, pert, coef = case
    xr = _host_solve(nc, P, pert, coef, 2)
    for x, stencils in run_threaded(ranks, rank_cycle, platform, case, cycle, kw):
        gap = np.abs(x - xr).max() / np.abs(xr).max()
        print(f"{platform} {case} cycle {cycle} {kw} on {ranks} rank(s): {stencils} stencils "
              f"assembled directly, max rel gap to the host solve {gap:.3e} "
              f"(bound {E2E_BOUND[cycle]:.0e})")
        assert stencils >= 1
        assert gap < E2E_BOUND[cycle]


@pytest.mark.parametrize("cycle", DTYPES)
@pytest.mark.parametrize("case", [FUSED3, FUSED5], ids=lambda c: c[0])
def test_direct_hierarchy_matches_host_solve(case, cycle):
    check_cycle("cpu", case, cycle)


@pytest.mark.parametrize("cycle", DTYPES)
@pytest.mark.parametrize("kw", [dict(tail_nodes=4096), dict(p_transfer="row")], ids=str)
def test_direct_hierarchy_with_the_other_options(kw, cycle):
    check_cycle("cpu", FUSED5, cycle, **kw)


@pytest.mark.parametrize("cycle", DTYPES)
def test_direct_hierarchy_on_two_ranks(cycle):
    check_cycle("cpu", ("auto", (4, 4, 4), 3, 0.2, "random"), cycle, ranks=2)


def check_tail_only(platform, dt):
    """q1_operator="matfree" with a tail: accepted, no level stencil, and the
    tail's stencils (all three levels of H_MESH: 4032, 504 and 80 nodes) obey
    the entrywise bound."""
    v = (1, False, 0.2, "random")
    pb = _pb(H_MESH, v, dt, platform)
    pmg = PMultigrid(pb, h_levels=-1, tail_nodes=4096, q1_operator="matfree", q1_assembly="direct")
    assert pmg.tail is not None and pmg.tail_levels == 3 and all(lv.S is None for lv in pmg.levels)
    assert pmg.info()["q1_assembly"] == "direct" and "q1_operator" not in pmg.info()
    same, ref = (PMultigrid(_pb(H_MESH, v, t), h_levels=-1) for t in (dt, torch.float64))
    worst = 0.0
    for lv, ls, lr, S in zip(pmg.levels, same.levels, ref.levels, pmg.tail.S):
        assert S.dtype == dt and S.device == pb.device
        e = entry_metric(lv.pb.lat, S.cpu().numpy(), _csr(lr.pb), UNIT[dt], _csr(ls.pb))
        worst = max(worst, e)
    for p in (same, ref):
        p.close()
    print(f"tail stencils {platform} {dt}: max e = {worst:.2f} (bound {FACTOR * yardstick():.1f})")
    assert worst <= FACTOR * yardstick()
    r, z = _residual(pb), pb.new_vector()
    pmg.apply(r, z)
    assert torch.isfinite(z).all()
    pmg.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_tail_stencils_assembled_directly(dt):
    check_tail_only("cpu", dt)


def check_no_csr_in_setup(platform, monkeypatch):
    def refuse(self, problem):
        raise AssertionError("CSROperator built during a direct setup")
    monkeypatch.setattr(poisson.CSROperator, "__init__", refuse)
    pb = PoissonProblem(Comm(), (8, 8, 8), 3, 1, False, torch.float64, platform, 0.2, "random")
    with pytest.raises(AssertionError):                 # the patch is in place
        poisson.CSROperator(pb)
    pmg = PMultigrid(pb, h_levels=-1, q1_operator="stencil", tail_nodes=125, q1_assembly="direct")
    assert pmg.tail_levels == 2 and pmg.levels[1].S is not None
    pmg.close()


def test_direct_setup_builds_no_csr_operator(monkeypatch):
    check_no_csr_in_setup("cpu", monkeypatch)


def check_defaults(platform):
    """Without the option a hierarchy is the q1_assembly="csr" one bit for bit:
    S, one cycle, info(); and the option is checked."""
    pb = PoissonProblem(Comm(), (4, 4, 4), 3, 1, False, torch.float64, platform, 0.2, "random")
    kw = dict(h_levels=-1, q1_operator="stencil")
    a, b = PMultigrid(pb, **kw), PMultigrid(pb, q1_assembly="csr", **kw)
    assert a.q1_assembly == b.q1_assembly == "csr"
    assert a.info() == b.info() and set(a.info()) == FOUR | {"h_levels", "h_cells", "q1_operator"}
    for la, lb in zip(a.levels, b.levels):
        assert (la.S is None) == (lb.S is None)
        if la.S is not None:
            assert torch.equal(_bits(la.S.cpu()), _bits(lb.S.cpu()))
            assert torch.equal(_bits(la.S.cpu()), _bits(torch.from_numpy(_csr(la.pb))))
    r, za, zb = _residual(pb), pb.new_vector(), pb.new_vector()
    a.apply(r, za)
    b.apply(r, zb)
    assert torch.equal(_bits(za.cpu()), _bits(zb.cpu()))
    for bad in ("device", "", None, 1, True):
        with pytest.raises(ValueError):
            PMultigrid(pb, q1_assembly=bad, **kw)
    with pytest.raises(ValueError, match="nothing to assemble"):
        PMultigrid(pb, h_levels=-1, q1_assembly="direct")
    with pytest.raises(ValueError, match="nothing to assemble"):
        PMultigrid(pb, h_levels=-1, q1_operator="matfree", tail_nodes=0, q1_assembly="direct")
    for p in (a, b):
        p.close()


def test_default_is_bitwise_unchanged_and_option_is_checked():
    check_defaults("cpu")


# ------------------------------------------------------------------ 3. CLI
def check_cli(platform, tmp_path):
    js = tmp_path / "q1a.json"
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", platform,
                        "--ndofs=1000", "--degree=3", "--cg", "--nreps", "10", "--mat_comp",
                        "--precond", "pmg", "--pmg_q1", "stencil", "--pmg_q1_assembly", "direct",
                        "--json", str(js)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    blk = d["mi355x"]["pmg"]
    assert set(blk) == FOUR | {"q1_operator", "q1_assembly"}
    assert blk["q1_operator"] == "stencil" and blk["q1_assembly"] == "direct"
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"matrix-free vs CSR pmg-PCG with --pmg_q1_assembly direct on {platform}: relative "
          f"error norm {rel:.3e}")
    assert rel < 1e-10


def test_cli_pmg_q1_assembly_direct(tmp_path):
    check_cli("cpu", tmp_path)


@pytest.mark.parametrize("args", [
    ["--pmg_q1_assembly", "direct"],
    ["--cg", "--pmg_q1_assembly", "direct"],
    ["--cg", "--precond", "jacobi", "--pmg_q1_assembly", "direct"],
    ["--cg", "--precond", "pmg", "--pmg_q1_assembly", "direct"],
    ["--cg", "--precond", "pmg", "--pmg_q1", "stencil", "--pmg_q1_assembly", "device"],
])
def test_cli_pmg_q1_assembly_refusals(args):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and "pmg_q1_assembly" in (r.stdout + r.stderr)
