"""The `--pcg_loop` option (no GPU): accepted with `--cg --precond jacobi`,
refused without either, refused on the CPU platform, and absent from a default
run's JSON, which is otherwise what it was before the option existed."""

import json
import os
import subprocess
import sys

import pytest
import torch

from benchmark_dolfinx_amd.cli import parse_args
from benchmark_dolfinx_amd.driver import laplace_action
from benchmark_dolfinx_amd.fem.mesh import compute_mesh_size
from benchmark_dolfinx_amd.models.poisson import (CSROperator, MatFreeLaplacianCPU,
                                                  PoissonProblem)
from benchmark_dolfinx_amd.parallel.comm import Comm
from benchmark_dolfinx_amd.solvers.cg import cg_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_args_accepts_the_fused_loop():
    args, unknown = parse_args(["--cg", "--precond", "jacobi", "--pcg_loop", "fused"])
    assert args.pcg_loop == "fused" and args.precond == "jacobi" and args.cg
    assert unknown == []
    args, _ = parse_args(["--cg", "--precond", "jacobi", "--pcg_loop", "generic"])
    assert args.pcg_loop == "generic"
    args, _ = parse_args(["--cg", "--precond", "jacobi"])
    assert args.pcg_loop == "generic"             # the default
    args, _ = parse_args([])
    assert args.pcg_loop == "generic"


def test_parse_args_rejects_the_fused_loop_without_jacobi():
    with pytest.raises(SystemExit) as e:
        parse_args(["--cg", "--pcg_loop", "fused"])
    assert "pcg_loop" in str(e.value) and "precond" in str(e.value)
    with pytest.raises(SystemExit):
        parse_args(["--cg", "--precond", "none", "--pcg_loop", "fused"])


def test_parse_args_rejects_the_fused_loop_without_cg():
    with pytest.raises(SystemExit) as e:
        parse_args(["--pcg_loop", "fused"])
    assert "pcg_loop" in str(e.value) and "cg" in str(e.value)
    with pytest.raises(SystemExit):       # unknown values are refused, not swallowed
        parse_args(["--cg", "--precond", "jacobi", "--pcg_loop", "native"])


def test_driver_refuses_the_fused_loop_off_the_gpu():
    pb = PoissonProblem(Comm(), (2, 2, 2), 2, 1, False, torch.float64, "cpu")
    with pytest.raises(ValueError, match="pcg_loop"):
        laplace_action(pb, 2, True, False, precond="jacobi", pcg_loop="fused")
    with pytest.raises(ValueError, match="pcg_loop"):
        laplace_action(pb, 2, True, False, precond="none", pcg_loop="fused")
    with pytest.raises(ValueError, match="pcg_loop"):
        laplace_action(pb, 2, True, False, precond="jacobi", pcg_loop="bogus")


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


CLI = [sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs", "1000",
       "--degree", "3", "--cg", "--nreps", "10"]


def test_cpu_platform_run_with_the_fused_loop_fails(tmp_path):
    js = tmp_path / "f.json"
    r = subprocess.run([*CLI, "--precond", "jacobi", "--pcg_loop", "fused", "--json", str(js)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "pcg_loop" in r.stderr and "gpu" in r.stderr
    assert not js.exists()


def test_default_cpu_run_has_no_pcg_loop_key_and_is_unchanged(tmp_path):
    """Same keys and the same deterministic values as the unpreconditioned
    solve run here through the calls the driver made before the option."""
    js = tmp_path / "d.json"
    r = subprocess.run([*CLI, "--mat_comp", "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pcg_loop" not in r.stdout and "Preconditioner" not in r.stdout
    d = json.load(open(js))
    assert set(d) == {"input", "output", "mi355x"}
    assert set(d["input"]) == {"p", "mpi_size", "ndofs_local_requested", "nreps", "scalar_size",
                               "use_gauss", "mat_comp", "qmode", "cg"}
    assert set(d["output"]) == {"ncells_global", "ndofs_global", "mat_free_time", "u_norm",
                                "y_norm", "z_norm", "gdof_per_second"}
    assert set(d["mi355x"]) == {"gdof_per_second_per_gpu", "mesh", "partition", "e_norm", "device",
                                "build_flags", "kernel", "geometry"}
    nx = compute_mesh_size(1000, 3)
    pb = PoissonProblem(Comm(), nx, 3, 1, False, torch.float64, "cpu")
    u = pb.assemble_rhs()
    y, z = pb.new_vector(), pb.new_vector()
    cg_solve(MatFreeLaplacianCPU(pb), pb, y, u, 10, 0.0)
    cg_solve(CSROperator(pb), pb, z, u, 10, 0.0)
    want = {"u_norm": pb.norm(u), "y_norm": pb.norm(y), "z_norm": pb.norm(z)}
    assert d["mi355x"]["mesh"] == list(nx)
    assert d["output"]["ndofs_global"] == pb.ndofs_global
    for k, v in want.items():
        assert abs(d["output"][k] - v) <= 1e-13 * abs(v), k
    assert abs(d["mi355x"]["e_norm"] - pb.norm(z - y)) <= 1e-13 * want["z_norm"]
    # with the preconditioner and the generic loop the key stays away too
    js2 = tmp_path / "j.json"
    r = subprocess.run([*CLI, "--precond", "jacobi", "--pcg_loop", "generic", "--json", str(js2)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d2 = json.load(open(js2))
    assert "pcg_loop" not in d2["mi355x"] and d2["mi355x"]["precond"] == "jacobi"
