"""Jacobi-preconditioned CG in the fused CG loop: `DeviceCG(pb, "jacobi",
loop="fused")` on fused2 / fused3 / fused5, end to end on the GPU -- the native
runtime (tiled and lattice storage, threaded ranks), the Python driver of the
same kernels, and the command line -- against the host PCG on the independent
CPU operator.  Every case has at least two kernel tiles along y and z, so the
interface fold of the update pass really runs.

Bounds: max |x - x_ref| / max |x_ref| < 1e-10 (FP64) and < 2e-4 (FP32), the
bounds tests/test_gpu_diagonal.py uses for the generic loop against the same
reference; r.r within 1e-5 relative of the generic loop's / the one-rank value
(derivation: test_gpu_diagonal.py::test_device_pcg_threaded_ranks)."""

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
from benchmark_dolfinx_amd.models.fused import FusedLaplacianGPU
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITS = 20
F64, F32 = torch.float64, torch.float32


def _tile(P):
    """Kernel tile (cells in y, z) of fused2 / fused3 at qmode 1 (nq = P + 2)."""
    ty, tz = ctypes.c_int(0), ctypes.c_int(0)
    assert native.hip().bdx_fused_tile(P + 2, ctypes.byref(ty), ctypes.byref(tz)) == 0
    return ty.value, tz.value


def _two_tiles(P, nx=3, ranks_y=1, ranks_z=1):
    """Cell counts with two fused2/3 tiles along y and z (per rank)."""
    ty, tz = _tile(P)
    return (nx, ranks_y * (ty + 1), ranks_z * (tz + 1))


# kernel, cells (None: two fused2/3 tiles each way, from bdx_fused_tile at run
# time), P, perturbation, dtype; kappa is random throughout
CASES = [
    ("fused5", (3, 5, 6), 3, 0.0, F64),
    ("fused5", (3, 5, 6), 3, 0.0, F32),
    ("fused5", (2, 3, 3), 6, 0.0, F64),
    ("fused3", None, 3, 0.2, F64),
    ("fused3", None, 3, 0.2, F32),
    ("fused2", None, 3, 0.2, F64),
]
IDS = ["fused5-P3-f64", "fused5-P3-f32", "fused5-P6-f64", "fused3-P3-f64", "fused3-P3-f32",
       "fused2-P3-f64"]
cases = pytest.mark.parametrize("case", CASES, ids=IDS)


def _unpack(case):
    kernel, nc, P, pert, dt = case
    return kernel, nc or _two_tiles(P), P, pert, dt


def _tol(dt):
    return 1e-10 if dt == F64 else 2e-4


@functools.lru_cache(maxsize=None)
def _host_pcg(nc, P, pert, its, precond=True):
    """Host (P)CG on the CPU operator, FP64, random kappa (read-only, shared)."""
    cpu = PoissonProblem(Comm(), nc, P, 1, False, F64, "cpu", pert, "random")
    x = cpu.new_vector()
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), its,
             dinv=cpu.jacobi_inverse() if precond else None)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


def _problem(nc, P, pert, dt, comm=None):
    return PoissonProblem(comm or Comm(), nc, P, 1, False, dt, "gpu", pert, "random")


def _operator(pb, kernel, runtime="native"):
    if runtime == "native":
        op = make_operator(pb, kernel, "otf")
    else:
        proto = make_operator(pb, kernel, "otf")
        op = FusedLaplacianGPU(pb, geometry="otf", version=proto.version, runtime=runtime)
    assert op.name == kernel
    assert op.nty >= 2 and op.ntz >= 2, (op.nty, op.ntz)
    return op


def _solve(pb, kernel, loop="fused", runtime="native", its=ITS, precond="jacobi"):
    """(global x, r.r, op info) of one solve on a fresh operator."""
    op = _operator(pb, kernel, runtime)
    x = pb.new_vector()
    cg = DeviceCG(pb, precond, loop=loop) if precond else DeviceCG(pb)
    cg.solve(op, x, pb.assemble_rhs(), its)
    cg.wait()
    torch.cuda.synchronize()
    rt = op._rt
    info = {"rt": rt is not None, "tiled": bool(rt.tiled) if rt is not None else None,
            "runtime": op.runtime}
    out = pb.to_global_array(x), cg.residual_norm2(), info
    op.close()
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ one rank
@cases
def test_fused_pcg_matches_host_pcg(case):
    kernel, nc, P, pert, dt = _unpack(case)
    pb = _problem(nc, P, pert, dt)
    xg, rr, info = _solve(pb, kernel)
    assert info["rt"] and info["runtime"] == "native"       # the native runtime ran it
    if kernel == "fused5":
        assert info["tiled"] is True
    xr = _host_pcg(nc, P, pert, ITS)
    rel = _rel(xg, xr)
    _, rr_gen, info_gen = _solve(pb, kernel, loop="generic")
    assert not info_gen["rt"]
    print(f"{kernel} P{P} {dt}: max rel err vs host PCG {rel:.3e}; r.r fused {rr:.6e} "
          f"generic {rr_gen:.6e}")
    assert rel < _tol(dt)
    assert math.isfinite(rr) and rr >= 0
    assert abs(rr - rr_gen) <= 1e-5 * rr_gen


@cases
def test_fused_pcg_flat_layout(case, monkeypatch):
    """BDX_TILED=0: the lattice layout and the flat update kernel."""
    monkeypatch.setenv("BDX_TILED", "0")
    kernel, nc, P, pert, dt = _unpack(case)
    xg, rr, info = _solve(_problem(nc, P, pert, dt), kernel)
    assert info["rt"] and info["tiled"] is False
    rel = _rel(xg, _host_pcg(nc, P, pert, ITS))
    print(f"{kernel} P{P} {dt} lattice layout: max rel err {rel:.3e}")
    assert rel < _tol(dt) and math.isfinite(rr)


@cases
def test_fused_pcg_python_driver(case):
    """The Python driver of the same kernels (runtime="python", also the
    fallback when the native runtime is unavailable)."""
    kernel, nc, P, pert, dt = _unpack(case)
    pb = _problem(nc, P, pert, dt)
    xp, rrp, info = _solve(pb, kernel, runtime="python")
    assert not info["rt"] and info["runtime"] == "python"
    xn, rrn, _ = _solve(pb, kernel)
    xr = _host_pcg(nc, P, pert, ITS)
    print(f"{kernel} P{P} {dt}: python driver vs host {_rel(xp, xr):.3e}, vs native "
          f"{_rel(xp, xn):.3e}")
    assert _rel(xp, xr) < _tol(dt)
    assert _rel(xp, xn) < _tol(dt)
    assert math.isfinite(rrp)
    print(f"r.r python driver {rrp:.9e}, native {rrn:.9e}")
    assert abs(rrp - rrn) <= 1e-5 * rrn


@pytest.mark.parametrize("kernel,nc,pert", [("fused5", (3, 5, 6), 0.0), ("fused3", None, 0.2)],
                         ids=["fused5", "fused3"])
def test_fused_pcg_split_iteration_restart_determinism(kernel, nc, pert):
    """iterate(7) + iterate(13) == iterate(20) within 1e-13 max|x| (the
    rounding level the README states for two runs of one build); a second
    start() on another x buffer reproduces a fresh solve to the same bound;
    two fresh solves are bitwise equal (no atomics on the path)."""
    nc = nc or _two_tiles(3)
    pb = _problem(nc, 3, pert, F64)
    b = pb.assemble_rhs()

    def fresh(split):
        op = _operator(pb, kernel)
        x = pb.new_vector()
        cg = DeviceCG(pb, "jacobi", loop="fused")
        cg.start(op, x, b)
        for n in split:
            cg.iterate(n)
        cg.wait()
        torch.cuda.synchronize()
        return op, cg, x

    op, cg, x20 = fresh([ITS])
    op2, _, x20b = fresh([ITS])
    assert torch.equal(x20, x20b), "two fresh fused PCG solves differ"
    op2.close()
    op3, _, x713 = fresh([7, 13])
    op3.close()
    scale = float(x20.abs().max())
    d = float((x713 - x20).abs().max())
    print(f"{kernel}: |x(7+13) - x(20)| = {d:.3e} (max|x| {scale:.3e})")
    assert d <= 1e-13 * scale
    # restart on another x buffer, same operator / runtime / cg
    x2 = pb.new_vector()
    cg.start(op, x2, b)
    cg.iterate(ITS)
    cg.wait()
    torch.cuda.synchronize()
    d2 = float((x2 - x20).abs().max())
    print(f"{kernel}: restart on another x: |dx| = {d2:.3e}")
    assert d2 <= 1e-13 * scale
    assert _rel(pb.to_global_array(x2), _host_pcg(nc, 3, pert, ITS)) < 1e-10
    op.close()


@pytest.mark.parametrize("kernel,nc,pert", [("fused5", (3, 5, 6), 0.0), ("fused3", None, 0.2)],
                         ids=["fused5", "fused3"])
def test_no_leak_into_unpreconditioned_cg(kernel, nc, pert):
    """After a fused PCG solve, DeviceCG(pb) on the same operator equals,
    bitwise, the same solve on a freshly built operator."""
    nc = nc or _two_tiles(3)
    pb = _problem(nc, 3, pert, F64)
    b = pb.assemble_rhs()
    op = _operator(pb, kernel)
    xp = pb.new_vector()
    pcg = DeviceCG(pb, "jacobi", loop="fused")
    pcg.solve(op, xp, b, ITS)
    pcg.wait()
    xa = pb.new_vector()
    cg = DeviceCG(pb)
    cg.solve(op, xa, b, ITS)
    cg.wait()
    torch.cuda.synchronize()
    rra = cg.residual_norm2()
    assert op._rt is not None and op._rt.cg is cg
    op.close()
    op_f = _operator(pb, kernel)
    xb = pb.new_vector()
    cg_f = DeviceCG(pb)
    cg_f.solve(op_f, xb, b, ITS)
    cg_f.wait()
    torch.cuda.synchronize()
    assert torch.equal(xa, xb)
    assert rra == cg_f.residual_norm2()
    assert not torch.equal(xa, xp)      # and it was not the preconditioned solve
    assert _rel(pb.to_global_array(xa), _host_pcg(nc, 3, pert, ITS, False)) < 1e-10
    op_f.close()


def test_cleared_binding_is_the_unpreconditioned_loop():
    """bdx_rt_set_precond with a null dinv clears the binding: a runtime that
    was bound and cleared before its first iteration runs the unpreconditioned
    solve, bit for bit."""
    pb = _problem((3, 5, 6), 3, 0.0, F64)
    b = pb.assemble_rhs()
    op0 = _operator(pb, "fused5")
    x0 = pb.new_vector()
    cg0 = DeviceCG(pb)
    cg0.solve(op0, x0, b, ITS)
    cg0.wait()
    op0.close()
    op = _operator(pb, "fused5")
    x = pb.new_vector()
    cg = DeviceCG(pb)
    cg.start(op, x, b)
    rt = op._rt
    z, prr = pb.new_vector(), torch.zeros_like(cg.partials)
    rt.set_precond(pb.jacobi_inverse(), z, prr, cg.RNORM)
    assert rt.lib.bdx_rt_set_precond(rt.h, None, None, None, None, None, -1) == 0
    # a binding needs z, a second partials buffer and a free scalar slot
    assert rt.lib.bdx_rt_set_precond(rt.h, pb.jacobi_inverse().data_ptr(), None, None, None,
                                     prr.data_ptr(), cg.RNORM) != 0
    assert rt.lib.bdx_rt_set_precond(rt.h, pb.jacobi_inverse().data_ptr(), z.data_ptr(), None,
                                     None, prr.data_ptr(), cg.PAP) != 0
    cg.iterate(ITS)
    cg.wait()
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
    assert torch.equal(z, torch.zeros_like(z))      # never written
    op.close()


@pytest.mark.parametrize("kernel,nc,pert", [("fused5", (3, 5, 6), 0.0), ("fused3", None, 0.2)],
                         ids=["fused5", "fused3"])
def test_fused_pcg_graph_replay(kernel, nc, pert, monkeypatch):
    """BDX_GRAPH=1: the steady-state iterations (update pass with z, the
    operator reading z) replayed from captured graphs give the eager
    launches' iterate bit for bit, also after a restart on another x buffer
    (the binding and the new x drop the captured graphs)."""
    nc = nc or _two_tiles(3)
    pb = _problem(nc, 3, pert, F64)
    b = pb.assemble_rhs()
    xs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("BDX_GRAPH", mode)
        op = _operator(pb, kernel)
        cg = DeviceCG(pb, "jacobi", loop="fused")
        x = pb.new_vector()
        cg.solve(op, x, b, ITS)
        cg.wait()
        assert op._rt.graphs is (mode == "1")
        x2 = pb.new_vector()
        cg.solve(op, x2, b, ITS)
        cg.wait()
        torch.cuda.synchronize()
        assert torch.equal(x, x2)
        xs[mode] = x
        op.close()
    assert torch.equal(xs["0"], xs["1"])
    assert _rel(pb.to_global_array(xs["1"]), _host_pcg(nc, 3, pert, ITS)) < 1e-10


# ------------------------------------------------------------ threaded ranks
def _rank_job(comm, kernel, nc, pert):
    pb = _problem(nc, 3, pert, F64, comm)
    xg, rr, info = _solve(pb, kernel)
    return xg, rr, info, tuple(pb.lat.pgrid)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("kernel,pert", [("fused3", 0.2), ("fused5", 0.0)])
def test_fused_pcg_threaded_ranks(kernel, pert, R):
    """The z halo and both all-reduces (r.z steers the iterate, r.r is
    reported): a missing one is off by the rank count.  Two tiles per rank
    along y and z at every rank count (asserted in every rank)."""
    if kernel == "fused5":
        nc = (2, 10, 10)                      # tile 4 x 4: 5 x 5 cells per rank at R = 4
    else:
        ty, tz = _tile(3)
        nc = (2, 2 * (ty + 1), 2 * (tz + 1))
    xr = _host_pcg(nc, 3, pert, ITS)
    rr1 = run_threaded(1, _rank_job, kernel, nc, pert)[0][1]
    for xg, rr, info, pgrid in run_threaded(R, _rank_job, kernel, nc, pert):
        assert info["rt"] and pgrid[0] == 1 and pgrid[1] * pgrid[2] == R
        assert _rel(xg, xr) < 1e-10
        assert abs(rr - rr1) <= 1e-5 * rr1, (rr, rr1)


# --------------------------------------------------------------- convergence
def test_fused_pcg_converges_faster_than_cg():
    """(4, 4, 4) cells, P = 3, perturbed, random kappa, fused3: after 40
    iterations the fused PCG's true residual is at most a tenth of CG's (the
    margin of the generic loop's test)."""
    pb = _problem((4, 4, 4), 3, 0.2, F64)
    b = pb.assemble_rhs()
    res = {}
    for pre in (None, "jacobi"):
        op = make_operator(pb, "fused3", "otf")
        assert op.name == "fused3"
        x = pb.new_vector()
        cg = DeviceCG(pb, pre, loop="fused") if pre else DeviceCG(pb)
        cg.solve(op, x, b, 40)
        cg.wait()
        assert op._rt is not None
        y = pb.new_vector()
        op.apply(x.clone(), y)
        res[pre] = pb.norm(b - y) / pb.norm(b)
        op.close()
    print(f"true residual after 40 its: CG {res[None]:.3e}, fused PCG {res['jacobi']:.3e}")
    assert res["jacobi"] <= 0.1 * res[None]


# ------------------------------------------------------- unsupported / errors
@pytest.mark.parametrize("kernel", ["v1", "dofmap", "fused"])
def test_fused_loop_on_an_unsupported_operator_raises(kernel):
    pb = PoissonProblem(Comm(), (4, 5, 3), 3, 1, False, F64, "gpu", 0.2, "constant")
    op = make_operator(pb, kernel, "otf")
    assert getattr(op, "name", "v1") == kernel
    cg = DeviceCG(pb, "jacobi", loop="fused")
    with pytest.raises(ValueError, match="no fused preconditioned CG loop") as e:
        cg.solve(op, pb.new_vector(), pb.assemble_rhs(), 3)
    assert getattr(op, "name", type(op).__name__) in str(e.value)   # names the operator
    assert getattr(op, "_rt", None) is None
    if hasattr(op, "close"):
        op.close()


def test_loop_argument_validation():
    pb = PoissonProblem(Comm(), (2, 2, 2), 3, 1, False, F64, "gpu")
    with pytest.raises(ValueError):
        DeviceCG(pb, "jacobi", loop="native")
    with pytest.raises(ValueError):
        DeviceCG(pb, None, loop="fused")
    with pytest.raises(ValueError):
        DeviceCG(pb, loop="fused")
    assert DeviceCG(pb).loop == "generic" and DeviceCG(pb, "jacobi").loop == "generic"


# ------------------------------------------------------------------------ CLI
def test_cli_pcg_loop_fused(tmp_path):
    """--cg --precond jacobi --pcg_loop fused --mat_comp on the GPU: the
    relative error norm against the CSR solve (preconditioned with the
    assembled matrix's own diagonal) within the bound of
    tests/test_cpu_diagonal.py::test_cli_precond_jacobi."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "f.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=1000",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "jacobi", "--pcg_loop", "fused",
           "--mat_comp", "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    assert d["mi355x"]["pcg_loop"] == "fused"
    assert d["mi355x"]["precond"] == "jacobi"
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"fused PCG vs CSR PCG: relative error norm {rel:.3e} (kernel {d['mi355x']['kernel']})")
    assert rel < 1e-10
