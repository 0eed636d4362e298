"""Mixed-precision multigrid on the GPU (csrc/hip/mixed.hip): the five kernels
of the precision boundary against the host twins and the existing kernels
(bitwise), `DeviceCG` in mixed mode against the unfused composition of
existing methods (bitwise) and against the host mixed `cg_solve`, convergence,
threaded ranks and the `--pmg_float` CLI.

The kernels are driven through their entry points with the extents of
tests/test_cpu_pmg_mixed.py: (3, 5, 67) (rows longer than a wave, ghost planes
and padding), (96, 96, 3) (9216 rows, above the 8192 that 2048 blocks cover:
the grid-stride branch) and (1, 1, 1).  Every entry outside the owned box is a
NaN sentinel and must keep its bits."""

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

import vector_ref as vr
from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.native import ptr
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg_mixed import (EXTENTS, check_boundary_kernels, nan_sentinel, owned_mask,
                                same_bits)
from test_gpu_pmg import E2E, ITS
from test_gpu_vector_kernels import check_sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
RN, PAP, OUT, NUM = 0, 2, 5, 6           # scalar slots used by the calls
SCAL = {RN: 0.8125, PAP: 1.37, 3: -0.4375, NUM: 2.25}


def lib():
    return native.hip()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rows(o):
    """(L1, ld, o0, o1, o2) of the extents `o` in their storage shape."""
    shape = EXTENTS[o]
    return (shape[1], shape[2], *o)


def scalars():
    s = np.full(8, np.nan)
    for k, v in SCAL.items():
        s[k] = v
    return s


def new_partials():
    n = lib().bdx_hip_partials_size()
    assert n >= 2048
    return torch.full((n,), np.nan, dtype=F64, device="cuda")


def vec64(o, seed):
    """Random doubles on the owned box, NaN sentinels elsewhere."""
    a = nan_sentinel(EXTENTS[o], np.float64)
    own = owned_mask(o, EXTENTS[o])
    a[own] = np.random.default_rng(seed).standard_normal(int(own.sum()))
    return a


def _dev_call(name, o):
    """The entry point `name` on numpy arrays: `out` is uploaded with its
    sentinels, the call runs on the device, `out` receives the result."""
    f = getattr(lib(), name)

    def call(a, out):
        d_a, d_out = dev(a), dev(out)
        assert f(*rows(o), ptr(d_a), ptr(d_out), stream()) == 0
        out[...] = host(d_out)
        assert same_bits(host(d_a), a)
    return call


def _host_call(name, o):
    fn = getattr(native.host(), name)
    return lambda a, out: fn(*rows(o), a.ctypes.data, out.ctypes.data)


# ------------------------------------------------------ 1. demote, promote
@pytest.mark.parametrize("o", list(EXTENTS))
def test_demote_promote_vs_host_twins(o):
    if o == (96, 96, 3):
        assert o[0] * o[1] > 4 * 2048
    d32, d64 = check_boundary_kernels(_dev_call("bdx_demote_f64_f32", o),
                                      _dev_call("bdx_promote_f32_f64", o), o, EXTENTS[o])
    h32, h64 = check_boundary_kernels(_host_call("bdx_cpu_demote_f64_f32", o),
                                      _host_call("bdx_cpu_promote_f32_f64", o), o, EXTENTS[o])
    assert same_bits(d32, h32) and same_bits(d64, h64)


# --------------------------------------------------- 2. cg_update_demote_f64
@pytest.mark.parametrize("o", list(EXTENTS))
def test_cg_update_demote(o):
    """x, r and the r.r slot bitwise those of bdx_cg_update_f64 on copies;
    r32 bitwise the demoted new residual; everything else untouched."""
    shape, own = EXTENTS[o], owned_mask(o, EXTENTS[o])
    x0, r0, p0, y0 = (vec64(o, s) for s in (11, 12, 13, 14))
    # y = 0 on the first owned entries, so the new residual there is r itself:
    # a tie between two floats, an FP32 subnormal, -0 and a large value
    first = np.flatnonzero(own.ravel())[:4]
    r0.ravel()[first] = [1.0 + 2.0 ** -24, 1e-40, -0.0, 1e30][: first.size]
    y0.ravel()[first] = 0.0
    scal0 = scalars()
    # the existing kernel on copies
    e_x, e_r, e_scal, e_part = dev(x0), dev(r0), dev(scal0), new_partials()
    d_p, d_y = dev(p0), dev(y0)
    assert lib().bdx_cg_update_f64(*rows(o), ptr(e_x), ptr(e_r), ptr(d_p), ptr(d_y), ptr(e_scal),
                                   RN, PAP, OUT, ptr(e_part), stream()) == 0
    d_x, d_r, d_scal, d_part = dev(x0), dev(r0), dev(scal0), new_partials()
    d_r32 = dev(nan_sentinel(shape, np.float32))
    assert lib().bdx_cg_update_demote_f64(*rows(o), ptr(d_x), ptr(d_r), ptr(d_p), ptr(d_y),
                                          ptr(d_scal), RN, PAP, OUT, ptr(d_part), ptr(d_r32),
                                          stream()) == 0
    x1, r1, s1, r32 = host(d_x), host(d_r), host(d_scal), host(d_r32)
    assert same_bits(x1, host(e_x)) and same_bits(r1, host(e_r))
    assert same_bits(s1, host(e_scal)) and math.isfinite(s1[OUT])
    others = [s for s in range(8) if s != OUT]
    assert same_bits(s1[others], scal0[others])
    assert same_bits(x1[~own], x0[~own]) and same_bits(r1[~own], r0[~own])
    assert np.isfinite(x1[own]).all() and np.isfinite(r1[own]).all()
    # r32 = demote(r): the device kernel and numpy
    d_dem = dev(nan_sentinel(shape, np.float32))
    assert lib().bdx_demote_f64_f32(*rows(o), ptr(d_r), ptr(d_dem), stream()) == 0
    with np.errstate(over="ignore", under="ignore"):
        want = r1.astype(np.float32)
    assert same_bits(r32, host(d_dem)) and same_bits(r32[own], want[own])
    assert same_bits(r32[~own], nan_sentinel(shape, np.float32)[~own])
    assert same_bits(host(d_p), p0) and same_bits(host(d_y), y0)


# ---------------------------------------- 3. dot_f64_f32, p_update_f64_f32
def _chain(o):
    """Longest chain of float64 additions behind a row reduction
    (tests/test_gpu_vector_kernels.py::rows_launch)."""
    nrows = o[0] * o[1]
    grid = min(max(vr.cdiv(nrows, 4), 1), 2048)
    per_thread = vr.cdiv(nrows, 4 * grid) * vr.cdiv(o[2], 64)
    return vr.chain_block(per_thread) + vr.chain_final(grid)


@pytest.mark.parametrize("o", list(EXTENTS))
def test_dot_f64_f32(o):
    shape, own = EXTENTS[o], owned_mask(o, EXTENTS[o])
    a = vec64(o, 21)
    b32 = vec64(o, 22).astype(np.float32)
    b64 = b32.astype(np.float64)                                 # promote: exact
    scal0 = scalars()
    d_a, d_b32, d_b64 = dev(a), dev(b32), dev(nan_sentinel(shape, np.float64))
    assert lib().bdx_promote_f32_f64(*rows(o), ptr(d_b32), ptr(d_b64), stream()) == 0
    assert same_bits(host(d_b64)[own], b64[own])
    e_scal, d_scal, e_part, d_part = dev(scal0), dev(scal0), new_partials(), new_partials()
    assert lib().bdx_dot_f64(*rows(o), ptr(d_a), ptr(d_b64), ptr(e_part), ptr(e_scal), OUT,
                             stream()) == 0
    assert lib().bdx_dot_f64_f32(*rows(o), ptr(d_a), ptr(d_b32), ptr(d_part), ptr(d_scal), OUT,
                                 stream()) == 0
    s1 = host(d_scal)
    assert same_bits(s1, host(e_scal))
    others = [s for s in range(8) if s != OUT]
    assert same_bits(s1[others], scal0[others])
    prod = (a[own].astype(np.longdouble) * b64[own].astype(np.longdouble)).astype(np.float64)
    check_sum(float(s1[OUT]), prod, _chain(o), what="dot_f64_f32")
    assert same_bits(host(d_a), a) and same_bits(host(d_b32), b32)


@pytest.mark.parametrize("o", list(EXTENTS))
def test_p_update_f64_f32(o):
    own = owned_mask(o, EXTENTS[o])
    p0 = vec64(o, 31)
    z32 = vec64(o, 32).astype(np.float32)
    z64 = z32.astype(np.float64)
    d_scal = dev(scalars())
    e_p, d_p, d_z32, d_z64 = dev(p0), dev(p0), dev(z32), dev(z64)
    assert lib().bdx_p_update_f64(*rows(o), ptr(e_p), ptr(d_z64), ptr(d_scal), NUM, PAP,
                                  stream()) == 0
    assert lib().bdx_p_update_f64_f32(*rows(o), ptr(d_p), ptr(d_z32), ptr(d_scal), NUM, PAP,
                                      stream()) == 0
    p1 = host(d_p)
    assert same_bits(p1, host(e_p)) and np.isfinite(p1[own]).all()
    assert same_bits(p1[~own], p0[~own]) and same_bits(host(d_z32), z32)
    beta = SCAL[NUM] / SCAL[PAP]
    ref = beta * p0[own] + z64[own]
    assert (np.abs(p1[own] - ref) <= 4 * 2.0 ** -52 * (np.abs(beta * p0[own]) + np.abs(z64[own]))).all()


# -------------------------------------------------- 4. entry points declared
def test_entry_points_are_declared():
    """ctypes signatures exist for the new entry points (an undeclared
    function would take its int64 and pointer arguments as C ints)."""
    for name, nargs in (("bdx_demote_f64_f32", 8), ("bdx_promote_f32_f64", 8),
                        ("bdx_cg_update_demote_f64", 16), ("bdx_dot_f64_f32", 11),
                        ("bdx_p_update_f64_f32", 11)):
        f = getattr(lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == nargs, name
        assert f.restype is ctypes.c_int and f.argtypes[0] is ctypes.c_int64, name


def test_kernel_methods_refuse_other_vectors():
    pb = PoissonProblem(Comm(), (2, 2, 2), 2, 1, False, F64, "gpu")
    k = pb.kernels
    a, a32 = pb.new_vector(), torch.zeros(pb.lat.shape, dtype=F32, device=pb.device)
    with pytest.raises(TypeError):
        k.demote(a32, a32)
    with pytest.raises(TypeError):
        k.promote(a, a)
    with pytest.raises(TypeError):
        k.p_update_f64_f32(a, a, torch.zeros(8, dtype=F64, device=pb.device), 0, 1)
    with pytest.raises(TypeError):
        k.dot_f64_f32(a, a32[:1], None, None, 0)
    torch.cuda.synchronize()


# ----------------------------------------- 5. fused loop = unfused loop
def _unfused_mixed(pb, op, pmg, b, its):
    """The mixed solve composed by hand of the existing methods plus demote /
    promote, with the FP64 z stored: (x, r.r)."""
    k = pb.kernels
    RR0, RR1, PAPS, RNORM = DeviceCG.RR0, DeviceCG.RR1, DeviceCG.PAP, DeviceCG.RNORM
    scal = torch.zeros(8, dtype=F64, device=pb.device)
    part = torch.zeros(k.npart, dtype=F64, device=pb.device)
    x, r, y, p, z = (pb.new_vector() for _ in range(5))
    op.apply(x, y)
    k.axpy(r, -1.0, y, b)
    k.demote(r, pmg.rc)
    pmg.apply_cycle(pmg.rc, pmg.zc)
    k.promote(pmg.zc, z)
    p.copy_(z)
    k.dot(r, z, part, scal, RR0)
    k.dot(r, r, part, scal, RNORM)
    for it in range(its):
        cur, nxt = (RR0, RR1) if it % 2 == 0 else (RR1, RR0)
        op.apply(p, y)
        k.dot(p, y, part, scal, PAPS)
        k.cg_update(x, r, p, y, scal, cur, PAPS, RNORM, part)
        k.demote(r, pmg.rc)
        pmg.apply_cycle(pmg.rc, pmg.zc)
        k.promote(pmg.zc, z)
        k.dot(r, z, part, scal, nxt)
        k.p_update(p, z, scal, nxt, cur)
    torch.cuda.synchronize()
    return x, float(scal[RNORM].item())


@pytest.mark.parametrize("kernel,nc,pert,coef,hl", [
    ("fused5", (4, 4, 4), 0.0, "constant", 0),
    ("fused3", (4, 5, 3), 0.2, "random", -1),
])
def test_fused_mixed_loop_is_the_unfused_loop(kernel, nc, pert, coef, hl):
    its = 4
    pb = PoissonProblem(Comm(), nc, 3, 1, False, F64, "gpu", pert, coef)
    op = make_operator(pb, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    pmg = PMultigrid(pb, h_levels=hl, cycle_dtype=F32)
    b = pb.assemble_rhs()
    xr, rr_ref = _unfused_mixed(pb, op, pmg, b, its)
    cg = DeviceCG(pb, "pmg", pmg=pmg)
    assert cg.mixed and cg.z is None                             # no FP64 z on the device
    x = pb.new_vector()
    cg.solve(op, x, b, its)
    cg.wait()
    rr = cg.residual_norm2()
    print(f"{kernel} {nc}: r.r after {its} iterations {rr!r} (unfused {rr_ref!r})")
    assert math.isfinite(rr) and rr > 0
    assert torch.equal(x.view(torch.int64), xr.view(torch.int64))
    assert np.float64(rr).view(np.int64) == np.float64(rr_ref).view(np.int64)
    pmg.close()
    if hasattr(op, "close"):
        op.close()


# ------------------------------------ 6. device against host mixed solve
# max |x - x_host| / max |x_host| after ITS iterations of the FP64 loop around
# the FP32 cycle, measured on an MI355X (profiles/pmg_mixed.md); the asserted
# bound is 10 x the measured gap and never looser than the project's FP32 cap
MEASURED = {
    ("fused5", 3): 1.980e-09, ("fused5", 6): 1.419e-10, ("fused3", 3): 1.122e-10,
    ("dofmap", 3): 1.122e-10,
}
CAP32 = 2e-4


def _bound(kernel, P):
    return min(10 * MEASURED[(kernel, P)], CAP32)


@functools.lru_cache(maxsize=None)
def _host_mixed_pcg(nc, P, pert, coef, its):
    cpu = PoissonProblem(Comm(), nc, P, 1, False, F64, "cpu", pert, coef)
    x = cpu.new_vector()
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), its,
             precond=PMultigrid(cpu, cycle_dtype=F32).apply)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


@pytest.mark.parametrize("kernel,nc,P,pert,coef", E2E)
def test_device_mixed_pcg_matches_host(kernel, nc, P, pert, coef):
    gpu = PoissonProblem(Comm(), nc, P, 1, False, F64, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", None) == kernel
    pmg = PMultigrid(gpu, cycle_dtype=F32)
    cg = DeviceCG(gpu, "pmg", pmg=pmg)
    assert cg.mixed and pmg.info()["cycle_float"] == 32
    x = gpu.new_vector()
    cg.solve(op, x, gpu.assemble_rhs(), ITS)
    cg.wait()
    assert getattr(op, "_rt", None) is None                      # no native runtime was started
    assert all(getattr(lv.op, "_rt", None) is None for lv in pmg.levels)
    xr = _host_mixed_pcg(nc, P, pert, coef, ITS)
    gap = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    rr = cg.residual_norm2()
    print(f"{kernel} Q{P} mixed: max rel gap to host mixed pmg-PCG {gap:.3e} (bound "
          f"{_bound(kernel, P):.1e}), r.r {rr:.3e}, lambda_max {pmg.lambda_max}")
    assert math.isfinite(rr) and rr >= 0
    assert gap <= _bound(kernel, P)
    pmg.close()
    if hasattr(op, "close"):
        op.close()


# ----------------------------------------------------------- 7. convergence
def _device_iterations(pb, op, b, pmg, limit=100):
    """Iterations until the device r.r / r0.r0 < 1e-16, and the true residual
    from the FP64 operator."""
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


def test_device_mixed_convergence():
    pb = PoissonProblem(Comm(), (8, 8, 8), 3, 1, False, F64, "gpu", 0.2, "random")
    op = make_operator(pb)
    b = pb.assemble_rhs()
    k64, r64 = _device_iterations(pb, op, b, PMultigrid(pb, h_levels=-1))
    k32, r32 = _device_iterations(pb, op, b, PMultigrid(pb, h_levels=-1, cycle_dtype=F32))
    print(f"to 1e-8: FP64 cycle {k64} its (true residual {r64:.2e}), FP32 cycle {k32} its "
          f"(true residual {r32:.2e})")
    assert abs(k32 - k64) <= 1 and r32 <= 1e-8 and r64 <= 1e-8
    if hasattr(op, "close"):
        op.close()


# -------------------------------------------------------- 8. threaded ranks
def _rank_mixed(comm):
    pb = PoissonProblem(comm, (4, 5, 3), 3, 1, False, F64, "gpu", 0.2, "random")
    op = make_operator(pb, "fused3", "otf")
    x = pb.new_vector()
    cg = DeviceCG(pb, "pmg", pmg=PMultigrid(pb, cycle_dtype=F32))
    cg.solve(op, x, pb.assemble_rhs(), ITS)
    cg.wait()
    xg, rr = pb.to_global_array(x), cg.residual_norm2()
    cg.pmg.close()
    if hasattr(op, "close"):
        op.close()
    return xg, rr


def test_device_mixed_threaded_ranks():
    """Two ranks, in the style of tests/test_gpu_pmg.py::
    test_device_pmg_threaded_ranks: the iterate within the end-to-end bound of
    the host solve and of the one-rank device solve (the FP32 cycle of two
    ranks sums in another order than one rank's, so the two differ at the
    cycle's precision, which is what that bound measures); r.r to 1e-5."""
    xr = _host_mixed_pcg((4, 5, 3), 3, 0.2, "random", ITS)
    x1, rr1 = run_threaded(1, _rank_mixed)[0]
    for xg, rr in run_threaded(2, _rank_mixed):
        gap = np.abs(xg - xr).max() / np.abs(xr).max()
        gap1 = np.abs(xg - x1).max() / np.abs(x1).max()
        print(f"2 ranks: gap to host {gap:.3e}, to one rank {gap1:.3e}, r.r {rr:.6e} vs {rr1:.6e}")
        assert gap <= _bound("fused3", 3) and gap1 <= _bound("fused3", 3)
        assert abs(rr - rr1) <= 1e-5 * rr1


# ------------------------------------------------------------------ 9. CLI
def test_cli_pmg_float_gpu(tmp_path):
    """--pmg_float 32 --mat_comp: both solves run one mixed preconditioner, so
    its precision cancels in the error norm."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    js = tmp_path / "m.json"
    cmd = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "gpu", "--ndofs=1000",
           "--degree=3", "--cg", "--nreps", "10", "--precond", "pmg", "--pmg_float", "32",
           "--mat_comp", "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    assert d["mi355x"]["pmg"]["cycle_float"] == 32 and d["input"]["scalar_size"] == 64
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"mixed pmg-PCG vs CSR mixed pmg-PCG: relative error norm {rel:.3e}")
    assert rel < 1e-10
