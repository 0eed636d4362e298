"""Matrix-free operator diagonal and Jacobi-preconditioned CG on the CPU path:
the host twin `bdx_cpu_diag_*` (through `PoissonProblem.operator_diagonal`)
against the diagonal of the assembled CSR matrix and a numpy oracle, the
host `cg_solve(..., dinv=...)` against a numpy PCG, and the `--precond` CLI."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from benchmark_dolfinx_amd.fem.mesh import (cell_coefficients, make_local_lattice,
                                            vertex_coordinates)
from benchmark_dolfinx_amd.fem.quadrature import OperatorTables
from benchmark_dolfinx_amd.models.poisson import CSROperator, MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from test_cpu_operator import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPAS = ["constant", "random"]
# nq = 2: the only instance with fewer quadrature points (8) than vertex coordinates (24)
CASES = CASES + [((3, 5, 2), 1, 0, False, 0.2)]


def _problem(nc, P, qm=1, g=False, pert=0.0, coef="constant", comm=None, dt=torch.float64):
    return PoissonProblem(comm or Comm(), nc, P, qm, g, dt, "cpu", pert, coef)


def _csr_diagonal(pb):
    """diag of the assembled matrix from its host arrays (rows == cols),
    reverse-accumulated like any vector.  A deliberate copy of what
    `CSROperator.diagonal()` does: the reference stays independent of it."""
    row_ptr, cols, vals = CSROperator(pb)._host
    rows = np.repeat(np.arange(pb.lat.nstore), np.diff(row_ptr))
    on = rows == cols
    d = np.zeros(pb.lat.nstore)
    d[rows[on]] = vals[on]
    d = torch.from_numpy(d.reshape(pb.lat.shape))
    pb.halo.reverse(d)
    return d


@pytest.mark.parametrize("coef", KAPPAS)
@pytest.mark.parametrize("nc,P,qm,g,pert", CASES)
def test_host_diagonal_vs_csr(nc, P, qm, g, pert, coef):
    pb = _problem(nc, P, qm, g, pert, coef)
    d = pb.to_global_array(pb.operator_diagonal())
    dc = pb.to_global_array(_csr_diagonal(pb))
    err = np.abs(d - dc).max()
    print(f"diag vs csr: max err {err:.3e}, max |d_csr| {np.abs(dc).max():.3e}")
    assert err <= 1e-12 * np.abs(dc).max()


def _oracle_diagonal(nc, P, qm, g, pert, coef):
    """d_e[a] = kappa sum_q gref[a, q]^T G[q] gref[a, q] with the trilinear
    geometry of oracle.box_model, scattered; Dirichlet entries 1."""
    t = OperatorTables(P, qm, g)
    X = vertex_coordinates(make_local_lattice(0, 1, nc, 1), pert)
    ref = oracle.box_model(nc, P, qm, g, vertices=X)
    cx, cy, cz = (a.ravel() for a in np.meshgrid(*(np.arange(n) for n in nc), indexing="ij"))
    cv = np.empty((cx.size, 8, 3))
    for v in range(8):
        cv[:, v] = X[cx + (v >> 2), cy + ((v >> 1) & 1), cz + (v & 1)]
    J = np.einsum("cvi,jqv->cqij", cv, t.geometry_dphi())
    Jinv = np.linalg.inv(J)
    G = np.einsum("cqid,cqjd->cqij", Jinv, Jinv) * (t.weights3d()[None] * np.linalg.det(J))[
        ..., None, None]
    kc = cell_coefficients(make_local_lattice(0, 1, nc, P), coef, oracle.KAPPA)
    kap = np.full(cx.size, oracle.KAPPA) if kc is None else np.asarray(kc, float).reshape(-1)
    gref, _ = oracle._ref_grad_tables(t)
    de = kap[:, None] * np.einsum("aqd,cqde,aqe->ca", gref, G, gref)
    dofs, bc = ref["dofs"], ref["bc"]
    d = np.zeros(bc.size)
    np.add.at(d, dofs.ravel(), np.where(bc[dofs], 0.0, de).ravel())
    d[bc] = 1.0
    return d


@pytest.mark.parametrize("coef", KAPPAS)
@pytest.mark.parametrize("nc,P,qm,g,pert", [CASES[1], CASES[2], CASES[5]])
def test_host_diagonal_vs_numpy_oracle(nc, P, qm, g, pert, coef):
    pb = _problem(nc, P, qm, g, pert, coef)
    d = pb.to_global_array(pb.operator_diagonal())
    dr = _oracle_diagonal(nc, P, qm, g, pert, coef)
    err = np.abs(d - dr).max()
    print(f"diag vs numpy: max err {err:.3e}, max |d| {np.abs(dr).max():.3e}")
    assert err <= 1e-12 * np.abs(dr).max()


@pytest.mark.parametrize("coef", KAPPAS)
@pytest.mark.parametrize("nc,P,qm,g,pert", CASES)
def test_host_diagonal_float32(nc, P, qm, g, pert, coef):
    d64 = _problem(nc, P, qm, g, pert, coef).operator_diagonal()
    pb = _problem(nc, P, qm, g, pert, coef, dt=torch.float32)
    d32 = pb.operator_diagonal()
    assert d32.dtype == torch.float32 and d32.shape == tuple(pb.lat.shape)
    rel = (np.abs(pb.to_global_array(d32) - pb.to_global_array(d64))
           / pb.to_global_array(d64)).max()
    print(f"f32 vs f64 diag: max entrywise rel err {rel:.3e}")
    assert rel <= 2e-5


@pytest.mark.parametrize("nc,P,qm,g,pert", CASES)
def test_diagonal_boundary_and_positivity(nc, P, qm, g, pert):
    pb = _problem(nc, P, qm, g, pert, "random")
    d = pb.operator_diagonal()
    assert d.dtype == torch.float64 and d.shape == tuple(pb.lat.shape)
    assert d is pb.operator_diagonal()  # cached
    assert torch.all(d[pb.bc_mask()] == 1.0)
    assert torch.all(pb.owned(d) > 0)
    assert torch.all(d[:, :, pb.lat.L[2]:] == 1.0)  # storage padding
    dinv = pb.jacobi_inverse()
    assert torch.isfinite(dinv).all() and torch.equal(dinv, 1.0 / d)


@pytest.mark.parametrize("R", [2, 4])
def test_diagonal_partition_invariance(R):
    def body(comm):
        pb = _problem((4, 5, 3), 3, 1, False, 0.2, "random", comm=comm)
        return pb.to_global_array(pb.operator_diagonal())

    ref = body(Comm())
    for d in run_threaded(R, body):
        assert np.abs(d - ref).max() <= 1e-13 * np.abs(ref).max()


def _numpy_pcg(apply, b, dinv, its):
    x = np.zeros_like(b)
    r = b - apply(x)
    z = dinv * r
    p = z.copy()
    rz = r @ z
    for _ in range(its):
        y = apply(p)
        alpha = rz / (p @ y)
        x = x + alpha * p
        r = r - alpha * y
        z = dinv * r
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    return x


def test_pcg_vs_numpy():
    nc, P, pert, its = (3, 3, 3), 3, 0.2, 15
    pb = _problem(nc, P, 1, False, pert)
    ref = oracle.box_model(nc, P, 1, vertices=vertex_coordinates(make_local_lattice(0, 1, nc, 1),
                                                                 pert))
    dinv = pb.jacobi_inverse()
    u = pb.assemble_rhs()
    x = pb.new_vector()
    assert cg_solve(MatFreeLaplacianCPU(pb), pb, x, u, its, dinv=dinv) == its
    xr = _numpy_pcg(ref["apply"], ref["u"], pb.to_global_array(dinv), its)
    err = np.abs(pb.to_global_array(x) - xr).max()
    print(f"PCG vs numpy: max err {err:.3e}, max |x_ref| {np.abs(xr).max():.3e}")
    assert err <= 1e-10 * np.abs(xr).max()


def true_residual(pb, op, x, b):
    y = pb.new_vector()
    op.apply(x.clone(), y)
    return pb.norm(b - y) / pb.norm(b)


def test_pcg_converges_faster_than_cg():
    """(4, 4, 4) cells, P = 3, perturbed, random kappa: after 40 iterations
    the true residual of Jacobi-PCG is at most a tenth of CG's (a numpy
    prototype gave 6.8e-7 vs 3.4e-5)."""
    pb = _problem((4, 4, 4), 3, 1, False, 0.2, "random")
    op = MatFreeLaplacianCPU(pb)
    b = pb.assemble_rhs()
    x_cg, x_pcg = pb.new_vector(), pb.new_vector()
    cg_solve(op, pb, x_cg, b, 40)
    cg_solve(op, pb, x_pcg, b, 40, dinv=pb.jacobi_inverse())
    r_cg, r_pcg = true_residual(pb, op, x_cg, b), true_residual(pb, op, x_pcg, b)
    print(f"true residual after 40 its: CG {r_cg:.3e}, PCG {r_pcg:.3e}")
    assert r_pcg <= 0.1 * r_cg


def test_cg_without_dinv_unchanged():
    """dinv=None is today's code path: bitwise the same iterate as the
    unpreconditioned recurrence written out here."""
    pb = _problem((3, 2, 2), 2, 1, False, 0.1)
    op = MatFreeLaplacianCPU(pb)
    b = pb.assemble_rhs()
    x = pb.new_vector()
    cg_solve(op, pb, x, b, 6, dinv=None)
    xr, r, y = pb.new_vector(), pb.new_vector(), pb.new_vector()
    op.apply(xr, y)
    r.copy_(b - y)
    p = r.clone()
    rn = pb.inner(p, r)
    for _ in range(6):
        op.apply(p, y)
        alpha = rn / pb.inner(p, y)
        xr.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        rn, rn_old = pb.inner(r, r), rn
        p.mul_(rn / rn_old).add_(r)
    assert torch.equal(x, xr)


@pytest.mark.parametrize("stop", [{"max_iter": 12}, {"max_iter": 200, "rtol": 1e-6}])
def test_pcg_dinv_equals_callable(stop):
    """`dinv=d` and `precond=` the callable that multiplies by d are one
    recurrence: the same iteration count and bitwise the same iterate."""
    pb = _problem((3, 2, 4), 2, 1, False, 0.2, "random")
    op = MatFreeLaplacianCPU(pb)
    b = pb.assemble_rhs()
    d = pb.jacobi_inverse()
    x_d, x_c = pb.new_vector(), pb.new_vector()
    k_d = cg_solve(op, pb, x_d, b, dinv=d, **stop)
    k_c = cg_solve(op, pb, x_c, b, precond=lambda r, z: torch.mul(d, r, out=z), **stop)
    print(f"iterations: dinv {k_d}, callable {k_c}")
    assert k_d == k_c and (k_d == 12 if "rtol" not in stop else 0 < k_d < 200)
    assert torch.equal(x_d, x_c)


# ------------------------------------------------------------------- CLI
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


CLI = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs", "1000",
       "--degree", "3", "--cg", "--nreps", "10", "--mat_comp"]


def _cli(args, js):
    r = subprocess.run([*CLI, *args, "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, json.load(open(js))


def test_cli_precond_jacobi(tmp_path):
    out, d = _cli(["--precond", "jacobi"], tmp_path / "j.json")
    assert "Preconditioner: jacobi" in out
    assert d["mi355x"]["precond"] == "jacobi"
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"matrix-free PCG vs CSR PCG (own diagonal): relative error norm {rel:.3e}")
    assert rel < 1e-10


def test_cli_precond_default_unchanged(tmp_path):
    """Without --precond: no console line, no key removed, and every
    deterministic value equals the unpreconditioned solve run here through
    the same calls the driver made before the option existed."""
    out, d = _cli([], tmp_path / "n.json")
    assert "Preconditioner" not in out
    out2, d2 = _cli(["--precond", "none"], tmp_path / "n2.json")
    assert "Preconditioner" not in out2
    assert set(d["input"]) == {"p", "mpi_size", "ndofs_local_requested", "nreps", "scalar_size",
                               "use_gauss", "mat_comp", "qmode", "cg"}
    assert set(d["output"]) == {"ncells_global", "ndofs_global", "mat_free_time", "u_norm",
                                "y_norm", "z_norm", "gdof_per_second"}
    assert set(d["mi355x"]) >= {"gdof_per_second_per_gpu", "mesh", "partition", "e_norm", "device",
                                "build_flags", "kernel", "geometry"}
    assert "precond" not in d["mi355x"] and "precond" not in d2["mi355x"]
    from benchmark_dolfinx_amd.fem.mesh import compute_mesh_size
    nx = compute_mesh_size(1000, 3)
    pb = _problem(nx, 3)
    u = pb.assemble_rhs()
    y, z = pb.new_vector(), pb.new_vector()
    cg_solve(MatFreeLaplacianCPU(pb), pb, y, u, 10, 0.0)
    cg_solve(CSROperator(pb), pb, z, u, 10, 0.0)
    want = {"u_norm": pb.norm(u), "y_norm": pb.norm(y), "z_norm": pb.norm(z)}
    for run in (d, d2):
        assert run["mi355x"]["mesh"] == list(nx)
        assert run["output"]["ndofs_global"] == pb.ndofs_global
        for k, v in want.items():
            assert abs(run["output"][k] - v) <= 1e-13 * abs(v), k
        assert abs(run["mi355x"]["e_norm"] - pb.norm(z - y)) <= 1e-13 * want["z_norm"]
    for k in ("u_norm", "y_norm", "z_norm"):
        assert d["output"][k] == d2["output"][k]


def test_cli_precond_needs_cg():
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu",
                        "--precond", "jacobi"], cwd=ROOT, env=_env(), capture_output=True,
                       text=True)
    assert r.returncode != 0 and "precond" in (r.stdout + r.stderr)
