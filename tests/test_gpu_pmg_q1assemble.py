"""The degree-1 levels' 27-point stencils assembled on the GPU:
`bdx_stencil27_assemble` (csrc/hip/lap_stencil27_assemble.h) with the checks of
tests/test_cpu_pmg_q1assemble.py (entry by entry against the host's CSR
stencil, refusals, the option in the cycle, no `CSROperator` in setup, defaults
unchanged, the CLI), the kernel against its host twin in the same metric and
bound, and two runs of it bit for bit.

Configurations, metric, yardstick and bound: tests/test_cpu_pmg_q1assemble.py."""

import pytest
import torch

from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import _bits
from test_cpu_pmg_q1assemble import (FACTOR, H_MESH, MESHES, VARIANTS, _h_levels, _pb, assemble,
                                     check_cli, check_cycle, check_defaults, check_h_levels,
                                     check_mesh, check_method, check_no_csr_in_setup,
                                     check_refusals, check_tail_only, check_two_ranks,
                                     cpu_reference, entry_metric, yardstick)
from test_cpu_pmg_q1stencil import DTYPES, UNIT
from test_gpu_pmg_q1stencil import FUSED3, FUSED5

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
def test_kernel_entries(nc, dt):
    check_mesh("gpu", nc, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_entries_on_h_levels(dt):
    check_h_levels("gpu", dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_entries_on_two_ranks(dt):
    check_two_ranks("gpu", dt)


def _pairs(dt):
    """(label, device problem, host problem) of every one-rank configuration."""
    for v in VARIANTS:
        for nc in MESHES:
            yield (nc, v), _pb(nc, v, dt, "gpu"), _pb(nc, v, dt, "cpu")
        for g, c in zip(_h_levels(_pb(H_MESH, v, dt, "gpu")), _h_levels(_pb(H_MESH, v, dt, "cpu"))):
            yield (tuple(int(n) for n in c.lat.n), v), g, c


@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_vs_host_twin_and_reruns_bitwise(dt):
    """The twins share stencil27_assemble_node and differ by FMA contraction:
    their distance in the metric of the CSR check, under its bound.  A second
    device run gives the same bits."""
    worst, equal = 0.0, 0
    for key, gpu, cpu in _pairs(dt):
        Sd, Sh = assemble(gpu).cpu(), assemble(cpu)
        assert torch.equal(_bits(assemble(gpu).cpu()), _bits(Sd)), key
        e = entry_metric(cpu.lat, Sd.numpy(), cpu_reference(torch.float64)[key], UNIT[dt],
                         S_exact=Sh.numpy(), other=Sh.numpy())
        equal += int(torch.equal(_bits(Sd), _bits(Sh)))
        worst = max(worst, e)
    print(f"stencil27_assemble {dt}: device vs host twin, max e = {worst:.2f} "
          f"(bound {FACTOR * yardstick():.1f}); bitwise equal on {equal} configurations")
    assert worst <= FACTOR * yardstick()


@pytest.mark.parametrize("dt", DTYPES)
def test_launcher_refusals(dt):
    check_refusals("gpu", dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_stencil27_method(dt):
    check_method("gpu", dt)


# ------------------------------------------------------------ 2. the cycle
@pytest.mark.parametrize("cycle", DTYPES)
@pytest.mark.parametrize("case", [FUSED3, FUSED5], ids=lambda c: c[0])
def test_direct_hierarchy_matches_host_solve(case, cycle):
    check_cycle("gpu", case, cycle)


@pytest.mark.parametrize("cycle", DTYPES)
@pytest.mark.parametrize("kw", [dict(tail_nodes=4096), dict(p_transfer="row")], ids=str)
def test_direct_hierarchy_with_the_other_options(kw, cycle):
    check_cycle("gpu", FUSED5, cycle, **kw)


@pytest.mark.parametrize("cycle", DTYPES)
def test_direct_hierarchy_on_two_ranks(cycle):
    check_cycle("gpu", ("auto", (4, 4, 4), 3, 0.2, "random"), cycle, ranks=2)


@pytest.mark.parametrize("dt", DTYPES)
def test_tail_stencils_assembled_directly(dt):
    check_tail_only("gpu", dt)


def test_direct_setup_builds_no_csr_operator(monkeypatch):
    check_no_csr_in_setup("gpu", monkeypatch)


def test_default_is_bitwise_unchanged_and_option_is_checked():
    check_defaults("gpu")


def test_stencils_live_on_the_device():
    pb = _pb((4, 4, 4), (1, False, 0.2, "random"), torch.float64, "gpu", P=3)
    pmg = PMultigrid(pb, h_levels=-1, cycle_dtype=torch.float32, q1_operator="stencil",
                     q1_assembly="direct")
    S = [lv.S for lv in pmg.levels if lv.S is not None]
    assert len(S) == 2 and all(s.is_cuda and s.dtype == torch.float32 for s in S)
    pmg.close()


# ------------------------------------------------------------------ 3. CLI
def test_cli_pmg_q1_assembly_direct_gpu(tmp_path):
    check_cli("gpu", tmp_path)
