"""The matrix-free diagonal kernel (lap_diag.h), the Jacobi-PCG vector kernels
(blas.hip) and `DeviceCG(pb, "jacobi")` on the GPU, against the FP64 host twin,
numpy / math.fsum references and the host PCG."""

import functools
import math

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.native import ptr
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from test_gpu_kernels import CASES

pytestmark = pytest.mark.gpu

# >= 3 cells on an axis (a colour holds two cells), odd counts (the last
# workgroup has a tail), every P, both nq
DIAG_CASES = CASES + [
    ((3, 5, 2), 2, 0, False, 0.0, torch.float64),
    ((1, 1, 1), 7, 1, False, 0.0, torch.float64),
    # nq = 2: 8 threads per cell stage its 24 vertex coordinates (32 cells per workgroup)
    ((3, 5, 2), 1, 0, False, 0.2, torch.float64),
    ((3, 5, 2), 1, 0, False, 0.2, torch.float32),
]
KAPPAS = ["constant", "random"]


@functools.lru_cache(maxsize=None)
def _host_diagonal(nc, P, qm, g, pert, coef):
    """FP64 host twin on the owned dofs (global array; read-only, shared)."""
    cpu = PoissonProblem(Comm(), nc, P, qm, g, torch.float64, "cpu", pert, coef)
    d = cpu.to_global_array(cpu.operator_diagonal())
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("coef", KAPPAS)
@pytest.mark.parametrize("nc,P,qm,g,pert,dt", DIAG_CASES)
def test_diagonal_matches_host_twin(nc, P, qm, g, pert, dt, coef):
    gpu = PoissonProblem(Comm(), nc, P, qm, g, dt, "gpu", pert, coef)
    d = gpu.operator_diagonal()
    assert d.dtype == dt and d.device == gpu.device and d.shape == tuple(gpu.lat.shape)
    assert torch.isfinite(d).all()                         # padding included
    assert torch.all(d[gpu.bc_mask()] == 1.0)
    assert torch.all(d[:, :, gpu.lat.L[2]:] == 1.0)
    assert torch.isfinite(gpu.jacobi_inverse()).all()
    dg, dc = gpu.to_global_array(d), _host_diagonal(nc, P, qm, g, pert, coef)
    if dt == torch.float64:
        err = np.abs(dg - dc).max()
        print(f"f64 diag: max err {err:.3e}, max |d| {np.abs(dc).max():.3e}")
        assert err <= 1e-12 * np.abs(dc).max()
    else:
        rel = (np.abs(dg - dc) / dc).max()
        print(f"f32 diag: max entrywise rel err {rel:.3e}")
        assert rel <= 2e-5


@pytest.mark.parametrize("nc,P,qm,g,pert,dt", [DIAG_CASES[1], DIAG_CASES[7], DIAG_CASES[9]])
def test_diagonal_bitwise_reproducible(nc, P, qm, g, pert, dt):
    ds = [PoissonProblem(Comm(), nc, P, qm, g, dt, "gpu", pert, "random").operator_diagonal()
          for _ in range(2)]
    assert torch.equal(ds[0], ds[1])


def _rank_diag(comm):
    pb = PoissonProblem(comm, (4, 5, 3), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    d = pb.to_global_array(pb.operator_diagonal())
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("R", [2, 4])
def test_diagonal_threaded_ranks(R):
    ref = run_threaded(1, _rank_diag)[0]
    for d in run_threaded(R, _rank_diag):
        assert np.abs(d - ref).max() <= 1e-13 * np.abs(ref).max()


# ------------------------------------------------------ PCG vector kernels
# owned box (5, 3, 70) inside storage (6, 4, 80): rows longer than one wave's
# 64 lanes and no multiple of it; everything outside the owned box is NaN
BOX = OWN, L1, LD, L0 = (5, 3, 70), 4, 80, 6
# the other shapes of the owned-row walk: rows shorter than a wave, and more
# than 4 x 2048 rows (the grid-stride branch of the row loop)
ROW_WALK_BOXES = {"short": ((3, 5, 19), 6, 32, 4), "rows": ((96, 96, 3), 97, 16, 97)}
RZ, PAP, OUT, RR = 0, 2, 1, 5
TYPES = {"f64": (np.float64, 1e-14), "f32": (np.float32, 1e-6)}
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def _vec(rng, T, positive=False, box=BOX):
    OWN, L1, LD, L0 = box
    a = np.full((L0, L1, LD), NAN, dtype=T)
    v = rng.standard_normal(OWN)
    a[: OWN[0], : OWN[1], : OWN[2]] = (np.abs(v) + 0.5) if positive else v
    return a


def _dev(a):
    return torch.from_numpy(a.copy()).to("cuda")


def _own(a, box=BOX):
    OWN = box[0]
    return a[: OWN[0], : OWN[1], : OWN[2]]


def _outside(box=BOX):
    OWN, L1, LD, L0 = box
    m = np.ones((L0, L1, LD), dtype=bool)
    m[: OWN[0], : OWN[1], : OWN[2]] = False
    return m


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_pcg_update_kernel(suf, box=BOX):
    """x += alpha p, r -= alpha y per entry within tol (|term| + |term|) of the
    float64 numpy value (tol 1e-14 / 1e-6: relative to the magnitude of the
    terms, the only bound a rounded sum can meet under cancellation); both
    reductions against math.fsum of the stored r within n eps sum|terms|."""
    T, tol = TYPES[suf]
    OWN, L1, LD, L0 = box
    rng = np.random.default_rng(17)
    x0, r0, p0, y0 = (_vec(rng, T, box=box) for _ in range(4))
    dinv0 = _vec(rng, T, True, box)
    scal0 = np.full(8, NAN)
    scal0[RZ], scal0[PAP] = 0.8125, 1.37
    lib = native.hip()
    d_x, d_r, d_p, d_y, d_d, d_s = (_dev(a) for a in (x0, r0, p0, y0, dinv0, scal0))
    part = torch.full((lib.bdx_hip_partials_size(),), NAN, dtype=torch.float64, device="cuda")
    rc = getattr(lib, f"bdx_pcg_update_{suf}")(
        L1, LD, *OWN, ptr(d_x), ptr(d_r), ptr(d_p), ptr(d_y), ptr(d_d), ptr(d_s), RZ, PAP, OUT,
        RR, ptr(part), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    x1, r1, s1 = d_x.cpu().numpy(), d_r.cpu().numpy(), d_s.cpu().numpy()
    alpha = float(T(scal0[RZ] / scal0[PAP]))
    xo, ro, po, yo = (_own(a, box).astype(np.float64) for a in (x0, r0, p0, y0))
    assert np.isfinite(_own(x1, box)).all() and np.isfinite(_own(r1, box)).all()
    ex = np.abs(_own(x1, box) - (xo + alpha * po)) / (np.abs(xo) + np.abs(alpha * po))
    er = np.abs(_own(r1, box) - (ro - alpha * yo)) / (np.abs(ro) + np.abs(alpha * yo))
    print(f"{suf} pcg_update: x err {ex.max():.3e}, r err {er.max():.3e}")
    assert ex.max() <= tol and er.max() <= tol
    out = _outside(box)
    assert np.array_equal(_bits(x1)[out], _bits(x0)[out])
    assert np.array_equal(_bits(r1)[out], _bits(r0)[out])
    for d, h in ((d_p, p0), (d_y, y0), (d_d, dinv0)):
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(h))
    rs = _own(r1, box).astype(np.float64).ravel()
    dv = _own(dinv0, box).astype(np.float64).ravel()
    n, eps = rs.size, 2.0 ** -52
    for slot, terms in ((RR, rs * rs), (OUT, dv * rs * rs)):
        ref = math.fsum(terms)
        bound = n * eps * math.fsum(np.abs(terms))
        print(f"{suf} slot {slot}: got {s1[slot]!r} ref {ref!r} bound {bound:.3e}")
        assert math.isfinite(s1[slot]) and abs(s1[slot] - ref) <= bound
    others = [s for s in range(8) if s not in (OUT, RR)]
    assert np.array_equal(_bits(s1)[others], _bits(scal0)[others])


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_pcg_p_update_kernel(suf, box=BOX):
    """p = beta p + dinv . r per entry, same tolerance model."""
    T, tol = TYPES[suf]
    OWN, L1, LD, L0 = box
    rng = np.random.default_rng(19)
    p0, r0 = _vec(rng, T, box=box), _vec(rng, T, box=box)
    dinv0 = _vec(rng, T, True, box)
    scal0 = np.full(8, NAN)
    scal0[1], scal0[0] = 0.59375, 1.21
    lib = native.hip()
    d_p, d_r, d_d, d_s = (_dev(a) for a in (p0, r0, dinv0, scal0))
    rc = getattr(lib, f"bdx_pcg_p_update_{suf}")(
        L1, LD, *OWN, ptr(d_p), ptr(d_r), ptr(d_d), ptr(d_s), 1, 0,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    p1 = d_p.cpu().numpy()
    beta = float(T(scal0[1] / scal0[0]))
    po, ro, do = (_own(a, box).astype(np.float64) for a in (p0, r0, dinv0))
    assert np.isfinite(_own(p1, box)).all()
    ep = np.abs(_own(p1, box) - (beta * po + do * ro)) / (np.abs(beta * po) + np.abs(do * ro))
    print(f"{suf} pcg_p_update: p err {ep.max():.3e}")
    assert ep.max() <= tol
    out = _outside(box)
    assert np.array_equal(_bits(p1)[out], _bits(p0)[out])
    for d, h in ((d_r, r0), (d_d, dinv0), (d_s, scal0)):
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(h))


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("box", list(ROW_WALK_BOXES))
def test_pcg_kernels_row_walk_shapes(box, suf):
    """The two kernels above, same checks, at the remaining shapes of the row walk."""
    assert ROW_WALK_BOXES["short"][0][2] < 64 and math.prod(ROW_WALK_BOXES["rows"][0][:2]) > 4 * 2048
    test_pcg_update_kernel(suf, ROW_WALK_BOXES[box])
    test_pcg_p_update_kernel(suf, ROW_WALK_BOXES[box])


# ------------------------------------------------------------ end to end
E2E = [
    ("fused5", (4, 4, 4), 3, 0.0, "constant", torch.float64),
    ("fused3", (4, 5, 3), 3, 0.2, "random", torch.float64),
    ("v1", (4, 5, 3), 3, 0.2, "random", torch.float64),
    ("dofmap", (4, 5, 3), 3, 0.2, "random", torch.float64),
    ("fused5", (4, 4, 4), 3, 0.0, "constant", torch.float32),
    ("fused3", (4, 5, 3), 3, 0.2, "random", torch.float32),
]


@functools.lru_cache(maxsize=None)
def _host_pcg(nc, P, pert, coef, its):
    cpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "cpu", pert, coef)
    x = cpu.new_vector()
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), its,
             dinv=cpu.jacobi_inverse())
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


@pytest.mark.parametrize("kernel,nc,P,pert,coef,dt", E2E)
def test_device_pcg_matches_host_pcg(kernel, nc, P, pert, coef, dt):
    """The generic Jacobi loop on every operator, also those with a fused CG
    of their own (which it must bypass)."""
    gpu = PoissonProblem(Comm(), nc, P, 1, False, dt, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf")
    assert getattr(op, "name", "v1" if kernel == "v1" else None) == kernel
    if kernel != "v1":
        assert hasattr(op, "cg_iterate")
    x = gpu.new_vector()
    cg = DeviceCG(gpu, "jacobi")
    cg.solve(op, x, gpu.assemble_rhs(), 20)
    cg.wait()
    assert getattr(op, "_rt", None) is None      # no native runtime was started
    xr = _host_pcg(nc, P, pert, coef, 20)
    rel = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    rr = cg.residual_norm2()
    print(f"{kernel} {dt}: max rel err vs host PCG {rel:.3e}, r.r {rr:.3e}")
    assert math.isfinite(rr) and rr >= 0
    assert rel < (1e-10 if dt == torch.float64 else 2e-4)
    if hasattr(op, "close"):
        op.close()


def _rank_pcg(comm):
    pb = PoissonProblem(comm, (4, 5, 3), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    op = make_operator(pb, "fused3", "otf")
    x = pb.new_vector()
    cg = DeviceCG(pb, "jacobi")
    cg.solve(op, x, pb.assemble_rhs(), 20)
    cg.wait()
    xg, rr = pb.to_global_array(x), cg.residual_norm2()
    if hasattr(op, "close"):
        op.close()
    return xg, rr


@pytest.mark.parametrize("R", [2, 4])
def test_device_pcg_threaded_ranks(R):
    """The two all-reduced scalars of the preconditioned loop: r.z steers the
    iterate (same 1e-10 bound as one rank), r.r is reported.  An x error of
    1e-10 |x| moves r.r by at most 2 |r| |A| 1e-10 |x|, here (|r| ~ 0.02,
    |A| ~ 10, |x| ~ 1e2) about 1e-5 of r.r; a missing all-reduce is off by
    a factor of the rank count."""
    xr = _host_pcg((4, 5, 3), 3, 0.2, "random", 20)
    rr1 = run_threaded(1, _rank_pcg)[0][1]
    for xg, rr in run_threaded(R, _rank_pcg):
        assert np.abs(xg - xr).max() < 1e-10 * np.abs(xr).max()
        assert abs(rr - rr1) <= 1e-5 * rr1


def test_device_pcg_converges_faster_than_cg():
    """(4, 4, 4) cells, P = 3, perturbed, random kappa, fused3: after 40
    iterations the true residual of Jacobi-PCG is at most a tenth of CG's."""
    gpu = PoissonProblem(Comm(), (4, 4, 4), 3, 1, False, torch.float64, "gpu", 0.2, "random")
    b = gpu.assemble_rhs()
    res = {}
    for pre in (None, "jacobi"):
        op = make_operator(gpu, "fused3", "otf")
        assert op.name == "fused3"
        x = gpu.new_vector()
        cg = DeviceCG(gpu, pre)
        cg.solve(op, x, b, 40)
        cg.wait()
        y = gpu.new_vector()
        op.apply(x.clone(), y)
        res[pre] = gpu.norm(b - y) / gpu.norm(b)
        if hasattr(op, "close"):
            op.close()
    print(f"true residual after 40 its: CG {res[None]:.3e}, PCG {res['jacobi']:.3e}")
    assert res["jacobi"] <= 0.1 * res[None]
