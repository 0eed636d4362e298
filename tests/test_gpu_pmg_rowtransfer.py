"""Row-streaming p-multigrid transfers on the GPU: `bdx_prolong_row` /
`bdx_restrict_row` (lap_rowtransfer.h) against their host twins and the dense
model of tests/test_cpu_pmg.py with the checks of
tests/test_cpu_pmg_rowtransfer.py, their fold modes against the two-pass
composition on the device, ghost planes on threaded ranks, the launcher's
refusals, `DeviceCG(pb, "pmg", pmg=PMultigrid(pb, p_transfer="row"))` against
the host solve, and the CLI.

Meshes: (2, 3, 2) cells, the seam mesh (1, 2, 33), whose rows take more than
one z-chunk of a wave for every pair, and (33, 2, 1), whose rows are one cell
(tests/test_cpu_pmg_rowtransfer.py)."""

import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops.kernels import HipError
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import (EPS, NAN, PAIRS, _adjoint_bound, _bits, _fill, _glob, _random, _shape,
                          model_prolong, model_restrict)
from test_cpu_pmg_rowtransfer import (PARTITIONED, SEAM, SEAM_SWAPPED, _ghost_nan, _kern, _pair,
                                      _table, check_prolong_row, check_restrict_row, rank_adjoint_gap,
                                      rank_fold_modes, rank_restrict_row)
from test_gpu_pmg import E2E, ITS, _bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
MESHES = [(2, 3, 2), SEAM, SEAM_SWAPPED]


# ------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_prolong_row_kernel(Pf, Pc, nc, dt):
    """Against the dense model (in check_prolong_row) and the host twin,
    run-to-run bitwise."""
    dev, bnd = check_prolong_row("gpu", nc, Pf, Pc, dt)
    again, _ = check_prolong_row("gpu", nc, Pf, Pc, dt)
    assert torch.equal(_bits(dev), _bits(again))
    host, _ = check_prolong_row("cpu", nc, Pf, Pc, dt)
    fine = _pair(nc, Pf, Pc, dt)[0]
    e_twin = np.abs(_glob(fine, dev) - _glob(fine, host))
    print(f"prolong_row {Pc}->{Pf} {nc} {dt}: vs host twin {(e_twin / (EPS[dt] * bnd)).max():.3e}")
    assert (e_twin <= EPS[dt] * bnd).all()


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_restrict_row_kernel(Pf, Pc, nc, dt, with_y):
    """Against the dense model, run-to-run bitwise (both in
    check_restrict_row) and the host twin."""
    dev, bnd = check_restrict_row("gpu", nc, Pf, Pc, dt, with_y)
    host, _ = check_restrict_row("cpu", nc, Pf, Pc, dt, with_y)
    coarse = _pair(nc, Pf, Pc, dt)[1]
    e_twin = np.abs(_glob(coarse, dev) - _glob(coarse, host))
    print(f"restrict_row {Pf}->{Pc} {nc} {dt} y={with_y}: vs host twin "
          f"{(e_twin / (EPS[dt] * bnd)).max():.3e}")
    assert (e_twin <= EPS[dt] * bnd).all()


# ------------------------------------------------------------ 2. fold modes
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_fold_modes_bitwise_on_the_device(Pf, Pc, nc, dt):
    rank_fold_modes(Comm(), nc, Pf, Pc, dt, "gpu")


# ----------------------------------------------------------- 3. ghost planes
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_fold_modes_bitwise_threaded_ranks(Pf, Pc, R):
    ghosts = run_threaded(R, rank_fold_modes, PARTITIONED, Pf, Pc, torch.float64, "gpu")
    assert sum(ghosts) > 0


def _rank_transfers(comm, nc, Pf, Pc, platform):
    """This rank's raw transfers of global fields: ghost planes NaN on the
    restriction's inputs, a NaN-filled target.  The GPU platform's partition
    on both platforms, so device and host ranks hold the same pieces."""
    fine, coarse = (PoissonProblem(comm, nc, P, 1, False, torch.float64, platform, partition="yz")
                    for P in (Pf, Pc))
    k, latc, J = _kern(fine), coarse.lat.as_int64(), _table(Pf, Pc)
    vf = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 5, torch.float64)))
    y = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 6, torch.float64)))
    vc = torch.full(coarse.lat.shape, NAN, dtype=torch.float64).to(coarse.device)
    k.restrict_row(latc, J, vf, y, vc)
    uc = _fill(coarse, _random(_shape(nc, Pc), 3, torch.float64))
    pu = torch.full(fine.lat.shape, NAN, dtype=torch.float64).to(fine.device)
    k.prolong_row(latc, J, uc, pu)
    return vc.cpu(), pu.cpu(), coarse.lat, fine.lat


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_partitioned_kernels_match_host_twins(Pf, Pc, R):
    """Every local node of every rank, ghost planes included (the coarse ones
    hold the restriction's partial sums): device against host within the sum
    of both sides' bounds against the exact operator, 2 EPS bnd."""
    nc, dt = PARTITIONED, torch.float64
    gf, gy = _random(_shape(nc, Pf), 5, dt), _random(_shape(nc, Pf), 6, dt)
    _, bR = model_restrict(nc, Pf, Pc, np.abs(gf) + np.abs(gy))
    _, bP = model_prolong(nc, Pf, Pc, _random(_shape(nc, Pc), 3, dt))
    dev = run_threaded(R, _rank_transfers, nc, Pf, Pc, "gpu")
    host = run_threaded(R, _rank_transfers, nc, Pf, Pc, "cpu")
    ghosts = 0
    for (dc, df, latc, latf), (hc, hf, hlatc, hlatf) in zip(dev, host):
        assert latc.as_int64().tolist() == hlatc.as_int64().tolist()
        assert latf.as_int64().tolist() == hlatf.as_int64().tolist()
        ghosts += sum(latc.gh)
        for d, h, lat, bnd in ((dc, hc, latc, bR), (df, hf, latf, bP)):
            L2 = lat.L[2]
            assert torch.isfinite(d[:, :, :L2]).all()
            assert torch.equal(_bits(d[:, :, L2:]), _bits(h[:, :, L2:]))     # NaN as before
            loc = bnd.ravel()[lat.global_indices()]
            err = (d[:, :, :L2] - h[:, :, :L2]).abs().numpy()
            assert (err <= 2 * EPS[dt] * loc).all()
    assert ghosts > 0


@pytest.mark.parametrize("R", [2, 4])
def test_row_adjointness_and_partition_invariance_on_the_device(R):
    nc, Pf, Pc = PARTITIONED, 6, 3
    for a, b, pc, gu, gv in run_threaded(R, rank_adjoint_gap, nc, Pf, torch.float64, "gpu"):
        bound = _adjoint_bound(nc, Pf, Pc, gu, gv, torch.float64)
        assert pc == Pc and np.isfinite(a) and abs(a - b) <= bound, (a, b, bound)
    gf, gy = (_random(_shape(nc, Pf), s, torch.float64) for s in (17, 19))
    _, bnd = model_restrict(nc, Pf, Pc, np.abs(gf) + np.abs(gy))
    one = run_threaded(1, rank_restrict_row, nc, Pf, "cpu")[0][0]
    for got, (gi, loc) in run_threaded(R, rank_restrict_row, nc, Pf, "gpu"):
        assert (np.abs(got - one) <= 2 * EPS[torch.float64] * bnd).all()
        assert np.array_equal(loc, got.ravel()[gi])


# -------------------------------------------------------------- 4. refusals
def test_row_kernels_reject_bad_descriptors_and_null_pointers():
    """hipErrorInvalidValue before anything is launched."""
    nc, dt = (2, 3, 2), torch.float64
    fine, coarse, k, latc, J = _pair(nc, 4, 2, dt, "gpu")
    vf, vc = fine.new_vector(), coarse.new_vector()
    wrong_degree = PoissonProblem(Comm(), nc, 3, 1, False, dt, "gpu")
    other_cells = PoissonProblem(Comm(), (2, 3, 3), 2, 1, False, dt, "gpu")
    for latd in (wrong_degree.lat.as_int64(), other_cells.lat.as_int64(),
                 coarse.lat.as_int64(tile=(4, 4))):
        with pytest.raises(HipError):
            k.prolong_row(latd, J, vc, vf)
        with pytest.raises(HipError):
            k.restrict_row(latd, J, vf, None, vc)
    for a, b in ((None, vf), (vc, None)):
        with pytest.raises(HipError):
            k.prolong_row(latc, J, a, b)
        with pytest.raises(HipError):
            k.restrict_row(latc, J, b, None, a)
    torch.cuda.synchronize()


# ------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _host_row_pcg(nc, P, pert, coef, its, h_levels=0, cycle_dtype=None):
    cpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "cpu", pert, coef)
    x = cpu.new_vector()
    pmg = PMultigrid(cpu, p_transfer="row", h_levels=h_levels, cycle_dtype=cycle_dtype)
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), its, precond=pmg.apply)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


def _device_solve(gpu, kernel, its, **kw):
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    x = gpu.new_vector()
    pmg = PMultigrid(gpu, **kw)
    cg = DeviceCG(gpu, "pmg", pmg=pmg)
    assert cg.pmg is pmg
    cg.solve(op, x, gpu.assemble_rhs(), its)
    cg.wait()
    rr = cg.residual_norm2()
    pmg.close()
    if hasattr(op, "close"):
        op.close()
    return gpu.to_global_array(x), rr


@pytest.mark.parametrize("mode", ["f64", "f32", "mixed"])
@pytest.mark.parametrize("kernel,nc,P,pert,coef", E2E)
def test_device_row_pmg_pcg_matches_host(kernel, nc, P, pert, coef, mode):
    """ITS iterations against the host solve with the row transfers, within
    the end-to-end bound of tests/test_gpu_pmg.py (`_bound`).  The mixed solve
    (FP64 CG around an FP32 cycle) is compared with the host's mixed solve;
    device and host differ by the FP32 roundings of the cycle, so it takes
    the FP32 bound."""
    dt = torch.float32 if mode == "f32" else torch.float64
    gpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "gpu", pert, coef)
    kw = {"cycle_dtype": torch.float32} if mode == "mixed" else {}
    x, rr = _device_solve(gpu, kernel, ITS, p_transfer="row", **kw)
    xr = _host_row_pcg(nc, P, pert, coef, ITS, 0, kw.get("cycle_dtype"))
    gap = np.abs(x - xr).max() / np.abs(xr).max()
    bound = _bound(kernel, P, torch.float32 if mode != "f64" else torch.float64)
    print(f"{kernel} Q{P} {mode}: max rel gap to the host row pmg-PCG {gap:.3e} (bound {bound:.1e})")
    assert math.isfinite(rr) and rr >= 0 and gap <= bound


def test_device_row_pmg_with_h_levels_and_tail():
    nc, P, pert, coef = (8, 8, 8), 3, 0.2, "random"
    gpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "gpu", pert, coef)
    x, rr = _device_solve(gpu, "fused3", ITS, p_transfer="row", h_levels=-1, tail_nodes=600)
    xr = _host_row_pcg(nc, P, pert, coef, ITS, -1)
    gap = np.abs(x - xr).max() / np.abs(xr).max()
    print(f"row transfers, h-levels and tail: gap to the host solve {gap:.3e}")
    # the tail's assembled stencil is a rounding-level perturbation of the
    # host's matrix-free levels: the FP64 cap of tests/test_gpu_pmg.py
    assert math.isfinite(rr) and gap <= 1e-10


def _rank_row_pmg(comm):
    pb = PoissonProblem(comm, (4, 5, 3), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    return _device_solve(pb, "fused3", ITS, p_transfer="row")


def test_device_row_pmg_two_threaded_ranks():
    xr = _host_row_pcg((4, 5, 3), 3, 0.2, "random", ITS)
    x1, rr1 = run_threaded(1, _rank_row_pmg)[0]
    for xg, rr in run_threaded(2, _rank_row_pmg):
        gap = np.abs(xg - xr).max() / np.abs(xr).max()
        print(f"2 ranks: gap to host {gap:.3e}, r.r {rr:.6e} vs one rank {rr1:.6e}")
        assert gap <= _bound("fused3", 3, torch.float64)
        assert abs(rr - rr1) <= 1e-5 * rr1


def _device_iterations(pb, op, b, pmg, limit=100):
    """Iterations until the device r.r / r0.r0 < 1e-16 (tests/test_gpu_pmg.py)."""
    x = pb.new_vector()
    cg = DeviceCG(pb, "pmg", pmg=pmg)
    cg.start(op, x, b)
    rr0 = cg.residual_norm2()
    k = 0
    while k < limit and cg.residual_norm2() >= 1e-16 * rr0:
        cg.iterate(1)
        k += 1
    cg.wait()
    y = pb.new_vector()
    op.apply(x.clone(), y)
    pmg.close()
    return k, pb.norm(b - y) / pb.norm(b)


def test_device_row_pmg_converges_like_the_cell_transfers():
    pb = PoissonProblem(Comm(), (8, 8, 8), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    op, b = make_operator(pb), pb.assemble_rhs()
    kc, rc = _device_iterations(pb, op, b, PMultigrid(pb))
    kr, rr = _device_iterations(pb, op, b, PMultigrid(pb, p_transfer="row"))
    print(f"cell {kc} its (true residual {rc:.2e}), row {kr} its (true residual {rr:.2e})")
    assert rr <= 1e-8 and rc <= 1e-8 and abs(kr - kc) <= 1
    if hasattr(op, "close"):
        op.close()


# ------------------------------------------------------------------ 6. CLI
def test_cli_pmg_transfer_row_gpu(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "r.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=1000",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "pmg", "--pmg_transfer", "row",
           "--mat_comp", "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    assert d["mi355x"]["pmg"]["p_transfer"] == "row" and d["mi355x"]["pmg"]["degrees"] == [3, 1]
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"row pmg-PCG vs CSR row pmg-PCG: relative error norm {rel:.3e}")
    assert rel < 1e-10
