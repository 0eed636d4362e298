"""p-multigrid preconditioned CG on the GPU: the transfer kernels
(lap_transfer.h) and `bdx_cheb_step` (blas.hip) against their host twins and
the dense model of tests/test_cpu_pmg.py, `DeviceCG(pb, "pmg")` against the
host `cg_solve(precond=)`, threaded ranks, convergence and the CLI."""

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
from benchmark_dolfinx_amd.fem.quadrature import gll, lagrange_tables
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import HipError, HostKernels
from benchmark_dolfinx_amd.ops.native import ptr
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import (EPS, NAN, PAIRS, _bits, _fill, _glob, _random, _shape, model_prolong,
                          model_restrict)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
NC = (2, 3, 2)   # 12 cells: several cells per workgroup, a tail, two cells of a colour on y


def _pb(P, dt, platform, nc=NC):
    return PoissonProblem(Comm(), nc, P, 1, False, dt, platform)


def _table(Pf, Pc):
    return np.ascontiguousarray(lagrange_tables(gll(Pc + 1)[0], gll(Pf + 1)[0])[0])


# ------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_prolong_kernel_vs_host_twin(Pf, Pc, dt):
    fine, coarse, hf, hc = _pb(Pf, dt, "gpu"), _pb(Pc, dt, "gpu"), _pb(Pf, dt, "cpu"), _pb(Pc, dt, "cpu")
    J = _table(Pf, Pc)
    gc = _random(_shape(NC, Pc), 3, dt)
    vc = _fill(hc, gc)                                     # NaN in the coarse padding
    vf0 = torch.full(hf.lat.shape, NAN, dtype=dt)          # never read, written once
    host = vf0.clone()
    HostKernels(hf.lat, dt).prolong(hc.lat.as_int64(), J, vc, host)
    dev = vf0.to("cuda")
    fine.kernels.prolong(coarse.lat.as_int64(), J, vc.to("cuda"), dev)
    torch.cuda.synchronize()
    dev = dev.cpu()
    L2 = hf.lat.L[2]
    assert torch.isfinite(dev[:, :, :L2]).all()
    assert torch.equal(_bits(dev[:, :, L2:]), _bits(vf0[:, :, L2:]))   # outside the lattice
    ref, bnd = model_prolong(NC, Pf, Pc, gc)
    e_model = np.abs(_glob(hf, dev) - ref)
    e_twin = np.abs(_glob(hf, dev) - _glob(hf, host))
    print(f"prolong {Pc}->{Pf} {dt}: err / bound vs model {(e_model / (EPS[dt] * bnd)).max():.3e}, "
          f"vs host twin {(e_twin / (EPS[dt] * bnd)).max():.3e}")
    assert (e_model <= EPS[dt] * bnd).all() and (e_twin <= EPS[dt] * bnd).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_restrict_kernel_vs_host_twin(Pf, Pc, dt):
    fine, coarse, hf, hc = _pb(Pf, dt, "gpu"), _pb(Pc, dt, "gpu"), _pb(Pf, dt, "cpu"), _pb(Pc, dt, "cpu")
    J = _table(Pf, Pc)
    gf = _random(_shape(NC, Pf), 5, dt)
    vf = _fill(hf, gf)                                     # NaN in the fine padding
    host = torch.zeros(hc.lat.shape, dtype=dt)
    host[:, :, hc.lat.L[2]:] = NAN
    vc0 = host.clone()
    HostKernels(hf.lat, dt).restrict(hc.lat.as_int64(), J, vf, host)
    d_vf, outs = vf.to("cuda"), []
    for _ in range(2):
        dev = vc0.to("cuda")
        fine.kernels.restrict(coarse.lat.as_int64(), J, d_vf, dev)
        torch.cuda.synchronize()
        outs.append(dev.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))     # bitwise reproducible
    assert torch.equal(_bits(d_vf.cpu()), _bits(vf))
    L2 = hc.lat.L[2]
    assert torch.equal(_bits(outs[0][:, :, L2:]), _bits(vc0[:, :, L2:]))
    ref, bnd = model_restrict(NC, Pf, Pc, gf)
    got = _glob(hc, outs[0])
    assert np.isfinite(got).all()
    e_model, e_twin = np.abs(got - ref), np.abs(got - _glob(hc, host))
    print(f"restrict {Pf}->{Pc} {dt}: err / bound vs model {(e_model / (EPS[dt] * bnd)).max():.3e}, "
          f"vs host twin {(e_twin / (EPS[dt] * bnd)).max():.3e}")
    assert (e_model <= EPS[dt] * bnd).all() and (e_twin <= EPS[dt] * bnd).all()


def test_transfer_kernels_reject_bad_descriptors():
    fine, coarse = _pb(4, torch.float64, "gpu"), _pb(2, torch.float64, "gpu")
    J = _table(4, 2)
    vf, vc = fine.new_vector(), coarse.new_vector()
    wrong_degree = _pb(3, torch.float64, "gpu")
    other_cells = _pb(2, torch.float64, "gpu", (2, 3, 3))
    tiled = coarse.lat.as_int64(tile=(4, 4))
    for latd in (wrong_degree.lat.as_int64(), other_cells.lat.as_int64(), tiled):
        with pytest.raises(HipError):
            fine.kernels.prolong(latd, J, vc, vf)
        with pytest.raises(HipError):
            fine.kernels.restrict(latd, J, vf, vc)
    torch.cuda.synchronize()


# owned box (5, 3, 70) inside storage (6, 4, 80): rows longer than one wave's
# 64 lanes and no multiple of it; everything outside the owned box is NaN
BOX = (5, 3, 70), 4, 80, 6
# the other shapes of the owned-row walk: rows shorter than a wave, and more
# than 4 x 2048 rows (the grid-stride branch of the row loop)
ROW_WALK_BOXES = {"short": ((3, 5, 19), 6, 32, 4), "rows": ((96, 96, 3), 97, 16, 97)}


@pytest.mark.parametrize("suf,dt", [("f64", torch.float64), ("f32", torch.float32)])
@pytest.mark.parametrize("first", [True, False])
def test_cheb_step_kernel_vs_host_twin(first, suf, dt, box=BOX):
    """Against the host twin and numpy, each entry within 8 eps of the
    magnitude of its terms (tests/test_cpu_pmg.py::test_cheb_step_host_twin);
    bitwise untouched outside the owned box; `first` reads no y, d, z."""
    OWN, L1, LD, L0 = box
    SL = tuple(slice(0, n) for n in OWN)
    rng = np.random.default_rng(29)

    def vec(positive=False, owned=True):
        a = np.full((L0, L1, LD), NAN)
        if owned:
            v = rng.standard_normal(OWN)
            a[SL] = (np.abs(v) + 0.5) if positive else v
        return torch.from_numpy(a).to(dt)

    dinv, r = vec(True), vec()
    y, d0, z0 = (vec(owned=not first) for _ in range(3))
    a, b = 0.3125, 1.7
    hd, hz = d0.clone(), z0.clone()
    getattr(native.host(), f"bdx_cpu_cheb_step_{suf}")(
        L1, LD, *OWN, int(first), a, b, ptr(dinv), ptr(r), ptr(y), ptr(hd), ptr(hz))
    dev = [t.to("cuda") for t in (dinv, r, y, d0, z0)]
    rc = getattr(native.hip(), f"bdx_cheb_step_{suf}")(
        L1, LD, *OWN, int(first), a, b, ptr(dev[0]), ptr(dev[1]), None if first else ptr(dev[2]),
        ptr(dev[3]), ptr(dev[4]), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    gd, gz = dev[3].cpu(), dev[4].cpu()
    T = np.float64 if dt == torch.float64 else np.float32
    a, b = float(T(a)), float(T(b))
    di, ri = dinv[SL].double().numpy(), r[SL].double().numpy()
    if first:
        dref = b * di * ri
        dmag = np.abs(dref)
        zref, zmag = dref, dmag
    else:
        yo, do, zo = (t[SL].double().numpy() for t in (y, d0, z0))
        dref = a * do + b * di * (ri - yo)
        dmag = np.abs(a * do) + np.abs(b * di) * (np.abs(ri) + np.abs(yo))
        zref, zmag = zo + dref, np.abs(zo) + dmag
    assert torch.isfinite(gd[SL]).all() and torch.isfinite(gz[SL]).all()
    for name, got, twin, ref, mag in (("d", gd, hd, dref, dmag), ("z", gz, hz, zref, zmag)):
        e_ref = (np.abs(got[SL].double().numpy() - ref) / mag).max()
        e_twin = (np.abs(got[SL].double().numpy() - twin[SL].double().numpy()) / mag).max()
        print(f"cheb_step first={first} {suf} {name}: vs numpy {e_ref:.3e}, vs host twin {e_twin:.3e}")
        assert e_ref <= 8 * EPS[dt] and e_twin <= 8 * EPS[dt]
    out = torch.ones((L0, L1, LD), dtype=torch.bool)
    out[SL] = False
    assert torch.equal(_bits(gd)[out], _bits(d0)[out]) and torch.equal(_bits(gz)[out], _bits(z0)[out])
    for t, t0 in zip(dev[:3], (dinv, r, y)):
        assert torch.equal(_bits(t.cpu()), _bits(t0))


@pytest.mark.parametrize("suf,dt", [("f64", torch.float64), ("f32", torch.float32)])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("box", list(ROW_WALK_BOXES))
def test_cheb_step_kernel_row_walk_shapes(box, first, suf, dt):
    """The same checks at the remaining shapes of the row walk."""
    assert ROW_WALK_BOXES["short"][0][2] < 64 and math.prod(ROW_WALK_BOXES["rows"][0][:2]) > 4 * 2048
    test_cheb_step_kernel_vs_host_twin(first, suf, dt, ROW_WALK_BOXES[box])


def test_entry_points_are_declared():
    """ctypes signatures exist for the new entry points (an undeclared
    function would take its int64 and double arguments as C ints)."""
    lib = native.hip()
    for suf in ("f64", "f32"):
        for name, nargs in (("bdx_prolong", 6), ("bdx_restrict", 6), ("bdx_cheb_step", 14)):
            f = getattr(lib, f"{name}_{suf}")
            assert f.argtypes is not None and len(f.argtypes) == nargs, name
            assert f.restype is ctypes.c_int, name


# ------------------------------------------------------------ 2. end to end
ITS = 6
E2E = [
    ("fused5", (4, 4, 4), 3, 0.0, "constant"),
    ("fused5", (4, 4, 4), 6, 0.0, "constant"),
    ("fused3", (4, 5, 3), 3, 0.2, "random"),
    ("dofmap", (4, 5, 3), 3, 0.2, "random"),
]
# max |x - x_host| / max |x_host| after ITS iterations, measured on an MI355X
# (profiles/pmg.md); the asserted bound is 10 x the measured gap and never
# looser than the Jacobi test's 1e-10 (FP64) / 2e-4 (FP32)
MEASURED = {
    ("fused5", 3, torch.float64): 4.889e-15, ("fused5", 3, torch.float32): 2.167e-07,
    ("fused5", 6, torch.float64): 3.590e-14, ("fused5", 6, torch.float32): 4.194e-06,
    ("fused3", 3, torch.float64): 5.441e-16, ("fused3", 3, torch.float32): 3.222e-07,
    ("dofmap", 3, torch.float64): 4.080e-16, ("dofmap", 3, torch.float32): 3.017e-07,
}
CAP = {torch.float64: 1e-10, torch.float32: 2e-4}


def _bound(kernel, P, dt):
    return min(10 * MEASURED[(kernel, P, dt)], CAP[dt])


@functools.lru_cache(maxsize=None)
def _host_pmg_pcg(nc, P, pert, coef, its):
    cpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "cpu", pert, coef)
    x = cpu.new_vector()
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), its,
             precond=PMultigrid(cpu).apply)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kernel,nc,P,pert,coef", E2E)
def test_device_pmg_pcg_matches_host(kernel, nc, P, pert, coef, dt):
    gpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    x = gpu.new_vector()
    cg = DeviceCG(gpu, "pmg")
    assert cg.pmg.degrees == ([3, 1] if P == 3 else [6, 3, 1])
    cg.solve(op, x, gpu.assemble_rhs(), ITS)
    cg.wait()
    assert getattr(op, "_rt", None) is None          # no native runtime was started
    assert all(getattr(lv.op, "_rt", None) is None for lv in cg.pmg.levels)
    xr = _host_pmg_pcg(nc, P, pert, coef, ITS)
    gap = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    rr = cg.residual_norm2()
    print(f"{kernel} Q{P} {dt}: max rel gap to host pmg-PCG {gap:.3e} (bound "
          f"{_bound(kernel, P, dt):.1e}), r.r {rr:.3e}, lambda_max {cg.pmg.lambda_max}")
    assert math.isfinite(rr) and rr >= 0
    assert gap <= _bound(kernel, P, dt)
    cg.pmg.close()
    if hasattr(op, "close"):
        op.close()


def test_device_cg_pmg_arguments():
    pb = PoissonProblem(Comm(), (2, 2, 2), 3, 1, False, torch.float64, "gpu")
    with pytest.raises(ValueError):
        DeviceCG(pb, "pmg", loop="fused")
    pmg = PMultigrid(pb, smooth_degree=3)
    with pytest.raises(ValueError):
        DeviceCG(pb, "jacobi", pmg=pmg)
    assert DeviceCG(pb, "pmg", pmg=pmg).pmg is pmg


# -------------------------------------------------------- 3. threaded ranks
def _rank_pmg(comm):
    pb = PoissonProblem(comm, (4, 5, 3), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    op = make_operator(pb, "fused3", "otf")
    x = pb.new_vector()
    cg = DeviceCG(pb, "pmg")
    cg.solve(op, x, pb.assemble_rhs(), ITS)
    cg.wait()
    xg, rr = pb.to_global_array(x), cg.residual_norm2()
    cg.pmg.close()
    if hasattr(op, "close"):
        op.close()
    return xg, rr


@pytest.mark.parametrize("R", [2, 4])
def test_device_pmg_threaded_ranks(R):
    """The iterate agrees with one rank's host solve within the end-to-end
    bound; r.r (all-reduced, reported) to 1e-5 as in
    test_device_pcg_threaded_ranks."""
    xr = _host_pmg_pcg((4, 5, 3), 3, 0.2, "random", ITS)
    x1, rr1 = run_threaded(1, _rank_pmg)[0]
    for xg, rr in run_threaded(R, _rank_pmg):
        gap = np.abs(xg - xr).max() / np.abs(xr).max()
        print(f"{R} ranks: gap to host {gap:.3e}, to one rank "
              f"{np.abs(xg - x1).max() / np.abs(x1).max():.3e}, r.r {rr:.6e} vs {rr1:.6e}")
        assert gap <= _bound("fused3", 3, torch.float64)
        assert abs(rr - rr1) <= 1e-5 * rr1


# ---------------------------------------------------------- 4. convergence
def _device_iterations(pb, op, b, precond, limit):
    """Iterations until the device r.r / r0.r0 < 1e-16 (checked every iteration)."""
    x = pb.new_vector()
    cg = DeviceCG(pb, precond)
    cg.start(op, x, b)
    rr0 = cg.residual_norm2()
    k = 0
    while k < limit and cg.residual_norm2() >= 1e-16 * rr0:
        cg.iterate(1)
        k += 1
    cg.wait()
    y = pb.new_vector()
    op.apply(x.clone(), y)
    if cg.pmg is not None:
        cg.pmg.close()
    return k, pb.norm(b - y) / pb.norm(b)


def test_device_pmg_converges_in_a_quarter_of_jacobi_iterations():
    """(8, 8, 8) cells, Q3, perturbed, random kappa: iterations to a relative
    residual of 1e-8 (the CPU test measured 13 against 103)."""
    pb = PoissonProblem(Comm(), (8, 8, 8), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    op = make_operator(pb)
    b = pb.assemble_rhs()
    kj, rj = _device_iterations(pb, op, b, "jacobi", 400)
    kp, rp = _device_iterations(pb, op, b, "pmg", 100)
    print(f"Jacobi-PCG {kj} its (true residual {rj:.2e}), pmg-PCG {kp} its (true residual {rp:.2e})")
    assert rp <= 1e-8 and 4 * kp <= kj
    if hasattr(op, "close"):
        op.close()


# ------------------------------------------------------------------ 5. CLI
def test_cli_precond_pmg_gpu(tmp_path):
    """--cg --precond pmg --mat_comp on the GPU: the CSR solve runs the same
    PMultigrid object, so the relative error norm is within the bound of
    tests/test_cpu_diagonal.py::test_cli_precond_jacobi."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "p.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=1000",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "pmg", "--mat_comp", "--json",
           str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Preconditioner: pmg" in r.stdout
    d = json.load(open(js))
    assert d["mi355x"]["precond"] == "pmg" and d["mi355x"]["pmg"]["degrees"] == [3, 1]
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"pmg-PCG vs CSR pmg-PCG: relative error norm {rel:.3e} (kernel {d['mi355x']['kernel']})")
    assert rel < 1e-10
