"""The V-cycle tail on the GPU: the one-workgroup kernel (csrc/hip/pmg_tail.h)
against its host twin and against the untailed device cycle, the launcher's
refusals, `DeviceCG(pb, "pmg", pmg=PMultigrid(pb, h_levels=-1, tail_nodes=N))`
against the host solve of tests/test_gpu_hpmg.py, and the CLI.

Meshes and the bound convention: tests/test_cpu_pmg_tail.py.  The figures in
MEASURED were taken on an MI355X (profiles/pmg_tail.md); a bound is 10 x the
measured gap, capped at 1e-10 (FP64) / 2e-4 (FP32)."""

import copy
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import HipError
from benchmark_dolfinx_amd.parallel.comm import Comm
from benchmark_dolfinx_amd.solvers.cg import DeviceCG
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import NAN, _bits
from test_cpu_pmg_tail import CAP, CASES, GEOM, _lattice, _residual
from test_gpu_hpmg import E2E, NC, _host_hpmg_pcg
from test_gpu_pmg import ITS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
F32, F64 = torch.float32, torch.float64
KERNEL_CASES = ["a", "b100", "b600", "b5000", "d"]
# max |z - z_ref| / max |z_ref| of one cycle on the device with the tail:
# (against the host twin's cycle, against the untailed device cycle)
MEASURED = {
    ("a", 0.0, torch.float64): (3.474e-16, 5.558e-16),
    ("a", 0.0, torch.float32): (2.238e-07, 2.238e-07),
    ("a", 0.2, torch.float64): (3.567e-16, 4.280e-16),
    ("a", 0.2, torch.float32): (2.298e-07, 3.064e-07),
    ("b100", 0.0, torch.float64): (5.379e-16, 3.074e-16),
    ("b100", 0.0, torch.float32): (2.063e-07, 2.063e-07),
    ("b100", 0.2, torch.float64): (3.540e-16, 2.832e-16),
    ("b100", 0.2, torch.float32): (2.280e-07, 1.520e-07),
    ("b600", 0.0, torch.float64): (4.995e-16, 3.074e-16),
    ("b600", 0.0, torch.float32): (2.888e-07, 1.650e-07),
    ("b600", 0.2, torch.float64): (4.247e-16, 2.832e-16),
    ("b600", 0.2, torch.float32): (1.900e-07, 1.900e-07),
    ("b5000", 0.0, torch.float64): (4.611e-16, 6.916e-16),
    ("b5000", 0.0, torch.float32): (2.063e-07, 3.300e-07),
    ("b5000", 0.2, torch.float64): (4.247e-16, 7.079e-16),
    ("b5000", 0.2, torch.float32): (1.900e-07, 3.040e-07),
    ("d", 0.0, torch.float64): (4.899e-16, 5.599e-16),
    ("d", 0.0, torch.float32): (2.254e-07, 3.006e-07),
    ("d", 0.2, torch.float64): (3.212e-16, 6.423e-16),
    ("d", 0.2, torch.float32): (5.173e-07, 3.017e-07),
}
# max |x - x_host| / max |x_host| after ITS iterations with tail_nodes=1024;
# "mixed": the FP32 cycle inside the FP64 loop (its cap is FP32's)
MEASURED_E2E = {
    ("fused5", torch.float64): 1.406e-14, ("fused5", torch.float32): 3.786e-07, ("fused5", "mixed"): 1.380e-10,
    ("fused3", torch.float64): 4.834e-16, ("fused3", torch.float32): 3.084e-07, ("fused3", "mixed"): 8.120e-11,
    ("dofmap", torch.float64): 4.834e-16, ("dofmap", torch.float32): 3.578e-07, ("dofmap", "mixed"): 8.094e-11,
}


def _bound(measured, dt):
    return min(10 * measured, CAP[dt])


def _gap(pb, z, zref):
    zl, zr = _lattice(pb, z.cpu()).double(), _lattice(pb, zref.cpu()).double()
    return ((zl - zr).abs().max() / zr.abs().max()).item()


# ----------------------------------------- 1. kernel vs host twin and untailed
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pert,coef", GEOM)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_tail_kernel_vs_host_twin_and_untailed_cycle(name, pert, coef, dt):
    nc, P, N, want, nlev = CASES[name]
    gpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "gpu", pert, coef)
    cpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "cpu", pert, coef)
    ref, pmg = PMultigrid(gpu, h_levels=-1), PMultigrid(gpu, h_levels=-1, tail_nodes=N)
    twin = PMultigrid(cpu, h_levels=-1, tail_nodes=N)
    assert pmg.tail_levels == want and twin.tail_levels == want and len(pmg.levels) == nlev
    assert pmg.lambda_max == ref.lambda_max and pmg.info()["tail_levels"] == want
    s = pmg.tail_start
    r = _residual(cpu, 5)                                       # NaN in the storage padding
    rd = r.to("cuda")
    zh = torch.full(cpu.lat.shape, NAN, dtype=dt)
    twin.apply(r.clone(), zh)
    zu = torch.full(gpu.lat.shape, NAN, dtype=dt, device="cuda")
    ref.apply(rd.clone(), zu)
    z = torch.full(gpu.lat.shape, NAN, dtype=dt, device="cuda")
    pmg.apply(rd, z)
    torch.cuda.synchronize()
    assert torch.equal(_bits(rd.cpu()), _bits(r))               # r unchanged bitwise
    assert torch.isnan(z[:, :, gpu.lat.L[2]:]).all()            # the padding's sentinels
    assert torch.isfinite(_lattice(gpu, z)).all()
    g_twin, g_untailed = _gap(gpu, z, zh), _gap(gpu, z, zu)
    print(f"{name} pert={pert} {dt}: tail kernel vs host twin {g_twin:.3e}, vs untailed device "
          f"cycle {g_untailed:.3e}")
    m_twin, m_untailed = MEASURED[(name, pert, dt)]
    assert g_twin <= _bound(m_twin, dt) and g_untailed <= _bound(m_untailed, dt)
    # run to run, and the levels above the tail while the kernel runs alone
    z2 = torch.full(gpu.lat.shape, NAN, dtype=dt, device="cuda")
    pmg.apply(rd, z2)
    assert torch.equal(_bits(z2.cpu()), _bits(z.cpu()))
    if s > 0:
        first = pmg.levels[s]
        upper = [v for lv in pmg.levels[:s] for v in (lv.y, lv.d, lv.t, lv.r, lv.z)
                 if v is not None]
        before = [v.clone() for v in upper]
        rt = _residual(twin.levels[s].pb, 9).to("cuda")
        rt0 = rt.clone()
        zt = torch.full(first.pb.lat.shape, NAN, dtype=dt, device="cuda")
        first.k.pmg_tail(pmg.tail, rt, zt)
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a.cpu()), _bits(b.cpu())) for a, b in zip(upper, before))
        assert torch.equal(_bits(rt.cpu()), _bits(rt0.cpu()))
        assert torch.isnan(zt[:, :, first.pb.lat.L[2]:]).all()
        assert torch.isfinite(_lattice(first.pb, zt)).all()
    zero = gpu.new_vector()
    z3 = torch.full(gpu.lat.shape, NAN, dtype=dt, device="cuda")
    pmg.apply(zero, z3)
    assert (_lattice(gpu, z3) == 0).all()                       # r = 0 gives z = 0
    for h in (ref, pmg):
        h.close()


# ------------------------------------------------------------------ 2. symbols
def test_tail_entry_points_are_declared():
    lib = native.hip()
    for suf in ("f64", "f32"):
        f = getattr(lib, f"bdx_pmg_tail_{suf}")
        assert f.argtypes is not None and len(f.argtypes) == 7
        assert f.restype is ctypes.c_int


@pytest.mark.parametrize("dt", DTYPES)
def test_tail_kernel_rejects_bad_tables(dt):
    """Following tests/test_gpu_hpmg.py::test_h_transfer_kernels_reject_bad_descriptors:
    the launcher reads the host copy of the table and launches nothing."""
    nc, P, N, want, _ = CASES["a"]
    gpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "gpu", 0.0, "constant")
    pmg = PMultigrid(gpu, h_levels=-1, tail_nodes=N)
    tail, k = pmg.tail, pmg.levels[0].k
    r = _residual(PoissonProblem(Comm(), nc, P, 1, False, dt, "cpu", 0.0, "constant"), 5).to("cuda")
    z = torch.full(gpu.lat.shape, NAN, dtype=dt, device="cuda")
    z0 = z.clone()

    def broken(level, edits):
        t = copy.copy(tail)
        t.host = tail.host.copy()
        for slot, val in edits:
            t.host[level * tail.WORDS + slot] = val
        return t

    big = [(0, 40), (1, 40), (2, 40), (3, 41), (4, 41), (5, 41), (16, 48)]   # 68921 nodes
    for what, t in (("node cap", broken(0, big)), ("node cap, level 1", broken(1, big)),
                    ("degree 2", broken(0, [(15, 2)])), ("degree 2, level 1", broken(1, [(15, 2)])),
                    ("tiled", broken(0, [(17, 4)])), ("ghost plane", broken(1, [(12, 1)])),
                    ("no stencil", broken(1, [(21, 0)])), ("no coefficients", broken(0, [(31, 0)])),
                    ("no transfer tables", broken(0, [(28, 0)]))):
        with pytest.raises(HipError, match="pmg_tail"):
            k.pmg_tail(t, r, z)
    f = getattr(native.hip(), "bdx_pmg_tail_" + ("f64" if dt == F64 else "f32"))
    st = torch.cuda.current_stream().cuda_stream
    host, dev = tail.host.ctypes.data, tail.dev.data_ptr()
    invalid = 1                                                 # hipErrorInvalidValue
    assert f(0, dev, tail.nlev, tail.nwords, r.data_ptr(), z.data_ptr(), st) == invalid
    assert f(host, 0, tail.nlev, tail.nwords, r.data_ptr(), z.data_ptr(), st) == invalid
    assert f(host, dev, 0, tail.nwords, r.data_ptr(), z.data_ptr(), st) == invalid
    assert f(host, dev, 17, tail.nwords, r.data_ptr(), z.data_ptr(), st) == invalid
    assert f(host, dev, tail.nlev, tail.nwords, 0, z.data_ptr(), st) == invalid
    assert f(host, dev, tail.nlev, tail.nwords, r.data_ptr(), 0, st) == invalid
    torch.cuda.synchronize()
    assert torch.equal(_bits(z.cpu()), _bits(z0.cpu()))         # nothing ran
    k.pmg_tail(tail, r, z)                                      # the table itself is fine
    torch.cuda.synchronize()
    assert torch.isfinite(_lattice(gpu, z)).all()
    pmg.close()


# ------------------------------------------------------- 3. end-to-end solve
def _e2e(kernel, pert, coef, dt, cycle_dtype, key):
    gpu = PoissonProblem(Comm(), NC, 3, 1, False, dt, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    x = gpu.new_vector()
    pmg = PMultigrid(gpu, h_levels=-1, tail_nodes=1024, cycle_dtype=cycle_dtype)
    cg = DeviceCG(gpu, "pmg", pmg=pmg)
    assert pmg.degrees == [3, 1] and pmg.h_cells == [(3, 2, 4)]
    assert pmg.tail_start == 1 and pmg.tail_levels == 2
    cg.solve(op, x, gpu.assemble_rhs(), ITS)
    cg.wait()
    xr = _host_hpmg_pcg(pert, coef)
    gap = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    rr = cg.residual_norm2()
    print(f"{key}: max rel gap to host h-pmg-PCG {gap:.3e}, r.r {rr:.3e}")
    assert math.isfinite(rr) and rr >= 0
    assert gap <= _bound(MEASURED_E2E[key], pmg.cycle_dtype)
    pmg.close()
    if hasattr(op, "close"):
        op.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kernel,pert,coef", E2E)
def test_device_tailed_pcg_matches_host(kernel, pert, coef, dt):
    _e2e(kernel, pert, coef, dt, None, (kernel, dt))


@pytest.mark.parametrize("kernel,pert,coef", E2E)
def test_device_tailed_mixed_pcg_matches_host(kernel, pert, coef):
    """The FP32 cycle with its FP32 tail inside the FP64 loop, against the
    all-FP64 host solve."""
    _e2e(kernel, pert, coef, F64, F32, (kernel, "mixed"))


# ------------------------------------------------------------------ 4. CLI
def test_cli_pmg_tail_gpu(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "t.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=15625",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "pmg", "--pmg_hlevels", "-1",
           "--pmg_tail", "1024", "--mat_comp", "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    blk = d["mi355x"]["pmg"]
    assert blk["h_levels"] == 2 and blk["h_cells"] == [[4, 4, 4], [2, 2, 2]]
    assert blk["tail_nodes"] == 1024 and blk["tail_levels"] == 3
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"tailed h-pmg-PCG vs CSR tailed h-pmg-PCG: relative error norm {rel:.3e} "
          f"(kernel {d['mi355x']['kernel']})")
    assert rel < 1e-10
