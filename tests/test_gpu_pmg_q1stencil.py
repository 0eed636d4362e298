"""Degree-1 multigrid levels on assembled 27-point stencils on the GPU:
`bdx_stencil27_apply` / `bdx_stencil27_cheb` (csrc/hip/lap_stencil27.h) with
the checks of tests/test_cpu_pmg_q1stencil.py (NumPy reference, the fused step
against apply + `bdx_cheb_step` bit for bit on the device, refusals, the
matrix-free operator), the kernels against their host twins, and
`DeviceCG(pb, "pmg", pmg=PMultigrid(pb, q1_operator="stencil"))` against the
FP64 host solve with the default hierarchy: end to end, combined with the
other options, on threaded ranks and through the CLI.

Meshes and bounds: tests/test_cpu_pmg_q1stencil.py."""

import functools

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import DeviceCG, cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg_q1stencil import (DTYPES, FUSED_MESHES, ITS, MEASURED_MATFREE, MESHES, UNIT, _kern, _pb, _stencil,
                                    _vector, check_apply_vs_numpy, check_cli, check_default_unchanged,
                                    check_launches, check_refusals, check_stencil_vs_matfree,
                                    check_threaded_ranks, numpy_stencil, rank_fused_vs_composition,
                                    rank_stencil_solve)

pytestmark = pytest.mark.gpu

# max_i |S u - A_matfree u|_i / (u (|S||u|)_i) on the owned entries of MESHES,
# bdx_stencil27_apply against make_operator(pb, "auto", "auto") (fused3), measured
# on an MI355X (profiles/pmg_q1stencil.md)
MEASURED_MATFREE.update({("gpu", torch.float64): 4.78, ("gpu", torch.float32): 4.51})


# ------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
def test_apply_kernel_vs_numpy(nc, dt):
    check_apply_vs_numpy("gpu", nc, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
def test_apply_kernel_vs_host_twin(nc, dt):
    """Both sums are within gamma_27 of the exact one: the same 64 u."""
    gpu, cpu = _pb(nc, 1, dt, "gpu"), _pb(nc, 1, dt, "cpu")
    S, u = _stencil(cpu), _vector(cpu, 3)
    yh, yd = cpu.new_vector(), gpu.new_vector()
    _kern(cpu).stencil27_apply(S, u, yh)
    _kern(gpu).stencil27_apply(S.to("cuda"), u.to("cuda"), yd)
    _, ya = numpy_stencil(cpu, S, u)
    L2 = cpu.lat.L[2]
    err = np.abs(yd.cpu().double().numpy() - yh.double().numpy())[:, :, :L2]
    print(f"stencil27_apply {nc} {dt}: device vs host twin, max err / (u |S||u|) = "
          f"{(err / np.maximum(UNIT[dt] * ya, 1e-300)).max():.3f}")
    assert (err <= 64 * UNIT[dt] * ya).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", FUSED_MESHES)
def test_fused_step_is_the_composition_bitwise_on_the_device(nc, dt):
    assert rank_fused_vs_composition(Comm(), nc, dt, "gpu") == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_step_leaves_ghost_planes_alone_on_two_ranks(dt):
    assert max(run_threaded(2, rank_fused_vs_composition, (5, 4, 3), dt, "gpu")) > 0


@pytest.mark.parametrize("dt", DTYPES)
def test_launcher_refusals(dt):
    check_refusals("gpu", dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_stencil_vs_matfree_operator(dt):
    check_stencil_vs_matfree("gpu", dt)


# ------------------------------------------------------------ 2. the cycle
def test_default_is_bitwise_unchanged_and_option_is_checked():
    check_default_unchanged("gpu")


@pytest.mark.parametrize("smooth", [2, 3])
def test_a_stencil_level_fuses_every_step_on_one_rank(smooth):
    check_launches("gpu", smooth)


@functools.lru_cache(maxsize=None)
def _host_solve(nc, P, pert, coef, smooth):
    """ITS iterations of the FP64 host pmg-PCG with the default (matrix-free)
    hierarchy, every h-level."""
    cpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "cpu", pert, coef)
    x = cpu.new_vector()
    pmg = PMultigrid(cpu, h_levels=-1, smooth_degree=smooth)
    cg_solve(MatFreeLaplacianCPU(cpu), cpu, x, cpu.assemble_rhs(), ITS, precond=pmg.apply)
    xg = cpu.to_global_array(x)
    xg.setflags(write=False)
    return xg


E2E_BOUND = {torch.float64: 1e-10, torch.float32: 2e-4}    # those of tests/test_gpu_pmg.py
FUSED3 = ("fused3", (4, 5, 3), 3, 0.2, "random")
FUSED5 = ("fused5", (4, 4, 4), 3, 0.0, "constant")


def _device_solve(kernel, nc, P, pert, coef, cycle, smooth=2, **kw):
    gpu = PoissonProblem(Comm(), nc, P, 1, False, torch.float64, "gpu", pert, coef)
    op = make_operator(gpu, kernel, "otf" if kernel != "auto" else "auto")
    if kernel != "auto":
        assert getattr(op, "name", None) == kernel
    pmg = PMultigrid(gpu, h_levels=-1, cycle_dtype=cycle, q1_operator="stencil",
                     smooth_degree=smooth, **kw)
    assert [lv.S is not None for lv in pmg.levels] == \
        [lv.pb.degree == 1 and (pmg.tail_start is None or i < pmg.tail_start)
         for i, lv in enumerate(pmg.levels)]
    assert all(lv.S.dtype == cycle and lv.S.is_cuda for lv in pmg.levels if lv.S is not None)
    x = gpu.new_vector()
    cg = DeviceCG(gpu, "pmg", pmg=pmg)
    cg.solve(op, x, gpu.assemble_rhs(), ITS)
    cg.wait()
    xr = _host_solve(nc, P, pert, coef, smooth)
    gap = np.abs(gpu.to_global_array(x) - xr).max() / np.abs(xr).max()
    print(f"{kernel} {nc} Q{P} cycle {cycle} smooth {smooth} {kw}: levels "
          f"{[tuple(int(n) for n in lv.pb.lat.n) for lv in pmg.levels]}, max rel gap to the host "
          f"solve {gap:.3e} (bound {E2E_BOUND[cycle]:.0e})")
    info = pmg.info()
    pmg.close()
    if hasattr(op, "close"):
        op.close()
    assert info["q1_operator"] == "stencil"
    assert gap < E2E_BOUND[cycle]
    return pmg


@pytest.mark.parametrize("cycle", DTYPES)
@pytest.mark.parametrize("case", [FUSED3, FUSED5], ids=lambda c: c[0])
def test_device_stencil_pmg_pcg_matches_host(case, cycle):
    _device_solve(*case, cycle)


@pytest.mark.parametrize("cycle", DTYPES)
def test_stencil_levels_above_a_tail(cycle):
    """(4, 4, 4) has one h-level only, so this is the fused5 case on (8, 8, 8):
    with tail_nodes = 125 the two h-levels (125 and 27 nodes) are the tail and
    the degree-1 p-level (729 nodes) is a stencil level."""
    pmg = _device_solve("fused5", (8, 8, 8), 3, 0.0, "constant", cycle, tail_nodes=125)
    assert pmg.tail_start == 2 and pmg.tail_levels == 2 and pmg.levels[1].S is not None


@pytest.mark.parametrize("cycle", DTYPES)
def test_stencil_levels_with_row_transfers(cycle):
    _device_solve(*FUSED5, cycle, p_transfer="row")


@pytest.mark.parametrize("cycle", DTYPES)
def test_stencil_levels_with_an_odd_smoothing_degree(cycle):
    """smooth_degree = 3: the post-smoothing's three fused steps end in `t`
    and are copied."""
    _device_solve(*FUSED5, cycle, smooth=3)


@pytest.mark.parametrize("cycle", DTYPES)
def test_degree_one_problem_has_a_stencil_level_zero(cycle):
    pmg = _device_solve("auto", (4, 4, 4), 1, 0.2, "random", cycle)
    assert pmg.degrees == [1] and pmg.levels[0].S is not None and pmg.h_levels >= 1


# -------------------------------------------------------- 3. threaded ranks
@pytest.fixture(scope="module")
def one_rank_solve():
    x = run_threaded(1, rank_stencil_solve, "stencil", "gpu")[0][0]
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("R", [2, 4, 8])
def test_stencil_solve_on_threaded_ranks(R, one_rank_solve):
    """Every rank's global x against the one-rank stencil solve to 1e-10;
    lambda_max is the matrix-free hierarchy's exactly (asserted per rank)."""
    cells = check_threaded_ranks("gpu", R, one_rank_solve)
    if R == 8:
        assert cells[1:] == [(2, 2, 2), (1, 1, 1)]


# ------------------------------------------------------------------ 4. CLI
def test_cli_pmg_q1_stencil_gpu(tmp_path):
    check_cli("gpu", tmp_path)
