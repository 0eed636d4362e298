"""h-multigrid levels on the GPU: the h-transfer kernels (lap_htransfer.h)
against their host twins and the dense model of tests/test_cpu_hpmg.py, the
operator on a coarsened (graded, degree-1) problem against the CPU operator,
`DeviceCG(pb, "pmg", pmg=PMultigrid(pb, h_levels=-1))` against the host
`cg_solve(precond=)` with the same hierarchy, threaded ranks and the CLI."""

import ctypes
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
from benchmark_dolfinx_amd.fem.mesh import coarsened_lattice
from benchmark_dolfinx_amd.fem.quadrature import OperatorTables
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import HipError, HipKernels, HostKernels, HTransferTables
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_hpmg import SHAPES, _pair, check_prolong, check_restrict
from test_cpu_pmg import _bits
from test_gpu_pmg import ITS, _bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]


def _hip(dt):
    tables = OperatorTables(1, 1, False)
    return lambda lat: HipKernels(lat, tables, dt)


def _cuda(t):
    return t.to("cuda")


# ------------------------------------------------------------ 9. kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ghosts", [False, True])
@pytest.mark.parametrize("n", list(SHAPES))
def test_hprolong_kernel_vs_host_twin_and_model(n, ghosts, dt):
    dev, bnd = check_prolong(_hip(dt), _cuda, n, ghosts, dt)
    host, _ = check_prolong(lambda lat: HostKernels(lat, dt), lambda t: t, n, ghosts, dt)
    L2 = bnd.shape[2]
    gap = np.abs(dev[:, :, :L2].double().numpy() - host[:, :, :L2].double().numpy())
    print(f"hprolong {n} ghosts={ghosts} {dt}: vs host twin, max gap / bound {(gap / bnd).max():.3e}")
    assert (gap <= bnd).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ghosts", [False, True])
@pytest.mark.parametrize("n", list(SHAPES))
def test_hrestrict_kernel_vs_host_twin_and_model(n, ghosts, dt):
    dev, bnd = check_restrict(_hip(dt), _cuda, n, ghosts, dt)     # runs twice, bitwise equal
    host, _ = check_restrict(lambda lat: HostKernels(lat, dt), lambda t: t, n, ghosts, dt)
    L2 = bnd.shape[2]
    gap = np.abs(dev[:, :, :L2].double().numpy() - host[:, :, :L2].double().numpy())
    print(f"hrestrict {n} ghosts={ghosts} {dt}: vs host twin, max gap / bound "
          f"{(gap / np.maximum(bnd, 1e-300)).max():.3e}")
    assert (gap <= bnd).all()


def test_h_transfer_kernels_reject_bad_descriptors():
    lf, lc, fpos = _pair((5, 4, 7), True)
    tab = HTransferTables(fpos, torch.float64, "cuda")
    k = _hip(torch.float64)(lf)
    vf = torch.zeros(lf.shape, dtype=torch.float64, device="cuda")
    vc = torch.zeros(lc.shape, dtype=torch.float64, device="cuda")
    vf0, vc0 = vf.clone(), vc.clone()
    for slot, val in ((17, 4), (15, 2), (12, 0)):                  # tiled, degree 2, gh
        d = lc.as_int64()
        d[slot] = val
        with pytest.raises(HipError):
            k.hprolong(d, tab, vc, vf)
        with pytest.raises(HipError):
            k.hrestrict(d, tab, vf, None, vc)
    torch.cuda.synchronize()
    assert torch.equal(_bits(vf.cpu()), _bits(vf0.cpu())) and torch.equal(vc, vc0)


def test_h_entry_points_are_declared():
    lib = native.hip()
    for suf in ("f64", "f32"):
        for name in ("bdx_hprolong", "bdx_hrestrict"):
            f = getattr(lib, f"{name}_{suf}")
            assert f.argtypes is not None and len(f.argtypes) == 9, name
            assert f.restype is ctypes.c_int, name


# ------------------------------------------------- 10. coarse-level operator
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pert,coef", [(0.0, "constant"), (0.2, "random")])
def test_operator_on_a_coarsened_problem_matches_cpu(pert, coef, dt):
    """Fine (9, 8, 11) -> (4, 4, 5): graded cells (pairs and a triple), P = 1;
    the bound of tests/test_gpu_kernels.py::test_v1_stiffness_matches_cpu."""
    nc = (9, 8, 11)
    gpu_f = PoissonProblem(Comm(), nc, 1, 1, False, dt, "gpu", pert, coef)
    cpu_f = PoissonProblem(Comm(), nc, 1, 1, False, torch.float64, "cpu", pert, coef)
    lat, fpos = coarsened_lattice(cpu_f.lat)
    assert lat.n == (4, 4, 5)
    gpu, cpu = (PoissonProblem.coarsened(p, lat, fpos) for p in (gpu_f, cpu_f))
    assert gpu.all_affine == (pert == 0.0) and gpu.all_axis_aligned == (pert == 0.0)
    u64 = torch.from_numpy(np.random.default_rng(1).standard_normal(cpu.lat.shape))
    yc = cpu.new_vector()
    MatFreeLaplacianCPU(cpu).apply(u64, yc)
    op = make_operator(gpu, "auto", "auto")
    yg = gpu.new_vector()
    op.apply(u64.to(gpu.device, dt), yg)
    yg = yg.double().cpu()
    err = (cpu.owned(yg) - cpu.owned(yc)).abs().max().item()
    tol = (1e-12 if dt == torch.float64 else 2e-5) * 50 * max(1.0, yc.abs().max().item())
    print(f"coarse operator {getattr(op, 'name', type(op).__name__)} pert={pert} {dt}: "
          f"max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    dg, dc = gpu.operator_diagonal().double().cpu(), cpu.operator_diagonal()
    assert (cpu.owned(dg) - cpu.owned(dc)).abs().max().item() <= tol
    if hasattr(op, "close"):
        op.close()


# ------------------------------------------- 11. device solve vs host solve
NC = (6, 5, 9)
E2E = [("fused5", 0.0, "constant"), ("fused3", 0.2, "random"), ("dofmap", 0.2, "random")]


@functools.lru_cache(maxsize=None)
def _host_hpmg_pcg(pert, coef):
    cpu = PoissonProblem(Comm(), NC, 3, 1, False, torch.float64, "cpu", pert, coef)
    pmg = PMultigrid(cpu, h_levels=-1)
    assert pmg.h_cells == [(3, 2, 4)]
    x = cpu.new_vector()
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), ITS, precond=pmg.apply)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kernel,pert,coef", E2E)
def test_device_hpmg_pcg_matches_host(kernel, pert, coef, dt):
    """The bounds of tests/test_gpu_pmg.py::test_device_pmg_pcg_matches_host."""
    gpu = PoissonProblem(Comm(), NC, 3, 1, False, dt, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    x = gpu.new_vector()
    cg = DeviceCG(gpu, "pmg", pmg=PMultigrid(gpu, h_levels=-1))
    assert cg.pmg.degrees == [3, 1] and cg.pmg.h_cells == [(3, 2, 4)]
    cg.solve(op, x, gpu.assemble_rhs(), ITS)
    cg.wait()
    xr = _host_hpmg_pcg(pert, coef)
    gap = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    rr = cg.residual_norm2()
    print(f"{kernel} {dt}: max rel gap to host h-pmg-PCG {gap:.3e} (bound "
          f"{_bound(kernel, 3, dt):.1e}), r.r {rr:.3e}, lambda_max {cg.pmg.lambda_max}")
    assert math.isfinite(rr) and rr >= 0
    assert gap <= _bound(kernel, 3, dt)
    cg.pmg.close()
    if hasattr(op, "close"):
        op.close()


def _rank_hpmg(comm):
    pb = PoissonProblem(comm, NC, 3, 1, False, torch.float64, "gpu", 0.2, "random")
    op = make_operator(pb, "fused3", "otf")
    x = pb.new_vector()
    cg = DeviceCG(pb, "pmg", pmg=PMultigrid(pb, h_levels=-1))
    cg.solve(op, x, pb.assemble_rhs(), ITS)
    cg.wait()
    xg, rr, cells = pb.to_global_array(x), cg.residual_norm2(), list(cg.pmg.h_cells)
    cg.pmg.close()
    if hasattr(op, "close"):
        op.close()
    return xg, rr, cells


@pytest.mark.parametrize("R", [2, 4])
def test_device_hpmg_threaded_ranks(R):
    """(6, 5, 9) cells cut at y = 2 and z = 4: every cut is an even vertex, so
    the ranks build the one-rank hierarchy and the iterate agrees with one
    rank's host solve within the end-to-end bound; r.r to 1e-5, as
    tests/test_gpu_pmg.py::test_device_pmg_threaded_ranks."""
    xr = _host_hpmg_pcg(0.2, "random")
    x1, rr1, _ = run_threaded(1, _rank_hpmg)[0]
    for xg, rr, cells in run_threaded(R, _rank_hpmg):
        gap = np.abs(xg - xr).max() / np.abs(xr).max()
        print(f"{R} ranks: gap to host {gap:.3e}, to one rank "
              f"{np.abs(xg - x1).max() / np.abs(x1).max():.3e}, r.r {rr:.6e} vs {rr1:.6e}")
        assert cells == [(3, 2, 4)]
        assert gap <= _bound("fused3", 3, torch.float64)
        assert abs(rr - rr1) <= 1e-5 * rr1


# ------------------------------------------------------------------ 12. CLI
def test_cli_pmg_hlevels_gpu(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "h.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=15625",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "pmg", "--pmg_hlevels", "-1",
           "--mat_comp", "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    blk = d["mi355x"]["pmg"]
    assert blk["h_levels"] == 2 and blk["h_cells"] == [[4, 4, 4], [2, 2, 2]]
    assert len(blk["lambda_max"]) == 4 and blk["degrees"] == [3, 1]
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"h-pmg-PCG vs CSR h-pmg-PCG: relative error norm {rel:.3e} (kernel {d['mi355x']['kernel']})")
    assert rel < 1e-10
