"""The V-cycle tail (`PMultigrid(pb, tail_nodes=N)`, `--pmg_tail N`), CPU path:
the 27-point stencils against the matrix-free operator, the host twin of the
one-launch tail against the untailed cycle, the unchanged default, the calls
it replaces, symmetry, `cg_solve(precond=)`, the refusals and the CLI.

Meshes (cells, degree, N, expected tail levels):
  a  (6, 5, 9)    P = 1, h-level (3, 2, 4): 420 + 60 nodes, the whole cycle
  b  (13, 15, 17) P = 1, h-levels (6, 7, 8), (3, 3, 4): 4032 / 504 / 80 nodes,
     triples on every axis; N = 100, 600, 5000: one, two, all three levels
  c  (6, 5, 9)    P = 3: degrees [3, 1] + (3, 2, 4), the tail under degree 3
  d  (4, 4, 4)    P = 1, h-level (2, 2, 2): 27 nodes on the coarsest level
each on the box and with perturbation 0.2 and random kappa, in FP64 and FP32.

The reference of the cycle tests is the untailed cycle of the same hierarchy
(pinned to dense models by tests/test_cpu_pmg.py and tests/test_cpu_hpmg.py).
The tail's operator is the assembled stencil, equal to the matrix-free one to
rounding, so the two cycles differ at rounding level: the bound is 10 x the
measured max |z - z_ref| / max |z_ref| (MEASURED, also profiles/pmg_tail.md),
capped at 1e-10 (FP64) / 2e-4 (FP32), the convention of
tests/test_gpu_pmg.py::_bound."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.models.poisson import CSROperator, MatFreeLaplacianCPU
from benchmark_dolfinx_amd.ops.kernels import stencil27
from benchmark_dolfinx_amd.parallel.comm import run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import NAN, _bits, _iterations, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
GEOM = [(0.0, "constant"), (0.2, "random")]
# name: cells, degree, N, tail levels, levels in all
CASES = {
    "a": ((6, 5, 9), 1, 1024, 2, 2),
    "b100": ((13, 15, 17), 1, 100, 1, 3),
    "b600": ((13, 15, 17), 1, 600, 2, 3),
    "b5000": ((13, 15, 17), 1, 5000, 3, 3),
    "c": ((6, 5, 9), 3, 1024, 2, 3),
    "d": ((4, 4, 4), 1, 1024, 2, 2),
}
CAP = {torch.float64: 1e-10, torch.float32: 2e-4}
# max |z - z_ref| / max |z_ref| of one cycle, host twin against the untailed
# host cycle, measured (x86-64, g++ -O3 without FMA contraction)
MEASURED = {
    ("a", 0.0, torch.float64): 4.169e-16, ("a", 0.0, torch.float32): 3.730e-07,
    ("a", 0.2, torch.float64): 3.567e-16, ("a", 0.2, torch.float32): 2.298e-07,
    ("b100", 0.0, torch.float64): 3.074e-16, ("b100", 0.0, torch.float32): 1.857e-07,
    ("b100", 0.2, torch.float64): 2.832e-16, ("b100", 0.2, torch.float32): 1.520e-07,
    ("b600", 0.0, torch.float64): 3.074e-16, ("b600", 0.0, torch.float32): 1.650e-07,
    ("b600", 0.2, torch.float64): 4.247e-16, ("b600", 0.2, torch.float32): 1.520e-07,
    ("b5000", 0.0, torch.float64): 6.916e-16, ("b5000", 0.0, torch.float32): 3.713e-07,
    ("b5000", 0.2, torch.float64): 4.955e-16, ("b5000", 0.2, torch.float32): 4.561e-07,
    ("c", 0.0, torch.float64): 5.991e-16, ("c", 0.0, torch.float32): 2.144e-07,
    ("c", 0.2, torch.float64): 4.957e-16, ("c", 0.2, torch.float32): 2.129e-07,
    ("d", 0.0, torch.float64): 5.599e-16, ("d", 0.0, torch.float32): 6.763e-07,
    ("d", 0.2, torch.float64): 8.029e-16, ("d", 0.2, torch.float32): 5.173e-07,
}
# the same for `pmg_tail` called on its first level alone (perturbed mesh, another residual)
MEASURED_SUB = {
    ("b100", torch.float64): 1.358e-15, ("b100", torch.float32): 1.822e-07,
    ("b600", torch.float64): 7.560e-16, ("b600", torch.float32): 3.479e-07,
    ("c", torch.float64): 5.016e-16, ("c", torch.float32): 4.039e-07,
}
# |y_norm - y_norm_ref| / y_norm_ref of the CLI run below (10 iterations): the
# two norms agreed in every bit, which is taken as one FP64 ulp
MEASURED_CLI = 2.0 ** -52


def _bound(name, pert, dt):
    return min(10 * MEASURED[(name, pert, dt)], CAP[dt])


@functools.lru_cache(maxsize=None)
def _pair(name, pert, coef, dt):
    """(problem, untailed hierarchy, tailed hierarchy, residual, reference z)
    of one case; the residual has NaN in the storage padding and vanishes on
    Dirichlet nodes, the reference is computed once and never written."""
    nc, P, N, want, nlev = CASES[name]
    pb = _problem(nc, P, dt, pert=pert, coef=coef)
    ref, pmg = PMultigrid(pb, h_levels=-1), PMultigrid(pb, h_levels=-1, tail_nodes=N)
    assert len(pmg.levels) == nlev and pmg.tail_levels == want
    assert pmg.tail_start == nlev - want and pmg.tail.nlev == want
    assert pmg.lambda_max == ref.lambda_max
    assert all(a.coef == b.coef for a, b in zip(pmg.levels, ref.levels))
    r = _residual(pb, 5)
    z = torch.full(pb.lat.shape, NAN, dtype=dt)
    ref.apply(r.clone(), z)
    return pb, ref, pmg, r, z


def _residual(pb, seed):
    gen = torch.Generator().manual_seed(seed)
    r = torch.randn(pb.lat.shape, dtype=torch.float64, generator=gen).to(pb.dtype)
    r.masked_fill_(pb.bc_mask(), 0.0)
    r[:, :, pb.lat.L[2]:] = NAN
    return r


def _lattice(pb, v):
    return v[:, :, : pb.lat.L[2]]


def test_cases_have_the_node_counts_of_the_table():
    pmg = _pair("b5000", 0.0, "constant", torch.float64)[2]
    assert pmg.h_cells == [(6, 7, 8), (3, 3, 4)]
    assert [int(np.prod(lv.pb.lat.L)) for lv in pmg.levels] == [4032, 504, 80]
    assert _pair("a", 0.0, "constant", torch.float64)[2].h_cells == [(3, 2, 4)]
    assert [int(np.prod(lv.pb.lat.L)) for lv in _pair("a", 0.0, "constant",
                                                      torch.float64)[2].levels] == [420, 60]
    c = _pair("c", 0.0, "constant", torch.float64)[2]
    assert c.degrees == [3, 1] and c.h_cells == [(3, 2, 4)]
    d = _pair("d", 0.0, "constant", torch.float64)[2]
    assert d.h_cells == [(2, 2, 2)] and int(np.prod(d.levels[-1].pb.lat.L)) == 27


# ------------------------------------------------------ 1. stencil vs operator
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pert,coef", GEOM)
@pytest.mark.parametrize("name", ["a", "b5000", "c", "d"])
def test_stencil_matches_operator(name, pert, coef, dt):
    """Every tail level: the stencil applied to a random vector, non-zero on
    Dirichlet nodes, against `lv.op.apply`; the bound of tests/test_gpu_hpmg.py::
    test_operator_on_a_coarsened_problem_matches_cpu."""
    pmg = _pair(name, pert, coef, dt)[2]
    for l in range(pmg.tail_start, len(pmg.levels)):
        lv, S = pmg.levels[l], pmg.tail.S[l - pmg.tail_start]
        assert S.shape == (27, lv.pb.lat.nstore) and S.dtype == dt
        u = torch.from_numpy(np.random.default_rng(1).standard_normal(lv.pb.lat.shape)).to(dt)
        y, ys = lv.pb.new_vector(), torch.full(lv.pb.lat.shape, NAN, dtype=dt)
        lv.op.apply(u.clone(), y)
        lv.k.stencil27(S, u, ys)
        assert torch.isnan(ys[:, :, lv.pb.lat.L[2]:]).all()
        y, ys = _lattice(lv.pb, y).double(), _lattice(lv.pb, ys).double()
        err = (ys - y).abs().max().item()
        tol = (1e-12 if dt == torch.float64 else 2e-5) * 50 * max(1.0, y.abs().max().item())
        print(f"{name} level {l} pert={pert} {dt}: stencil vs operator max err {err:.3e} "
              f"(bound {tol:.3e})")
        assert err <= tol


def test_stencil_refuses_entries_that_are_no_lattice_neighbours():
    """A degree-2 problem is refused outright; in a degree-1 matrix one column
    moved to a node two planes away is caught."""
    with pytest.raises(ValueError):
        stencil27(CSROperator(_problem((2, 2, 2), 2)), _problem((2, 2, 2), 2).lat)
    pb = _problem((4, 4, 4), 1)
    A = CSROperator(pb)
    row_ptr, cols, vals = A._host
    cols[row_ptr[(2 * 5 + 2) * pb.lat.ld + 2]] = 0  # node (2, 2, 2) coupled to node (0, 0, 0)
    with pytest.raises(ValueError):
        stencil27(A, pb.lat)


# ------------------------------------------------ 2. tail cycle vs untailed
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pert,coef", GEOM)
@pytest.mark.parametrize("name", list(CASES))
def test_tail_cycle_matches_untailed_cycle(name, pert, coef, dt):
    pb, ref, pmg, r, zref = _pair(name, pert, coef, dt)
    want = CASES[name][3]
    assert pmg.tail_levels == want and pmg.info()["tail_levels"] == want
    r0 = r.clone()
    z = torch.full(pb.lat.shape, NAN, dtype=dt)
    pmg.apply(r, z)
    assert torch.equal(_bits(r), _bits(r0))                     # r unchanged bitwise
    assert torch.isnan(z[:, :, pb.lat.L[2]:]).all()             # the padding's sentinels
    zl, zr = _lattice(pb, z).double(), _lattice(pb, zref).double()
    assert torch.isfinite(zl).all()
    gap = ((zl - zr).abs().max() / zr.abs().max()).item()
    print(f"{name} pert={pert} {dt}: tail vs untailed cycle, max |dz| / max |z| = {gap:.3e} "
          f"(bound {_bound(name, pert, dt):.1e})")
    assert gap <= _bound(name, pert, dt)
    z2 = torch.full(pb.lat.shape, NAN, dtype=dt)
    pmg.apply(r, z2)
    assert torch.equal(_bits(z2), _bits(z))                     # run to run
    zero, z3 = pb.new_vector(), torch.full(pb.lat.shape, NAN, dtype=dt)
    pmg.apply(zero, z3)
    assert (_lattice(pb, z3) == 0).all()                        # r = 0 gives z = 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["b100", "b600", "c"])
def test_tail_call_leaves_the_upper_levels_alone(name, dt):
    """`pmg_tail` called directly on its first level's vectors: the vectors of
    the levels above keep their bits, and so does its right-hand side."""
    pb, ref, pmg, r, _ = _pair(name, 0.2, "random", dt)
    s = pmg.tail_start
    assert s > 0
    first = pmg.levels[s]
    pmg.apply(r.clone(), pb.new_vector())                       # work vectors hold a cycle's data
    upper = [v for lv in pmg.levels[:s] for v in (lv.y, lv.d, lv.t, lv.r, lv.z) if v is not None]
    before = [v.clone() for v in upper]
    assert all(v.abs().max() > 0 for lv in pmg.levels[:s] for v in (lv.y, lv.d))
    rt = _residual(first.pb, 9)
    rt0 = rt.clone()
    zt = torch.full(first.pb.lat.shape, NAN, dtype=dt)
    first.k.pmg_tail(pmg.tail, rt, zt)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(upper, before))
    assert torch.equal(_bits(rt), _bits(rt0))
    assert torch.isnan(zt[:, :, first.pb.lat.L[2]:]).all()
    assert torch.isfinite(_lattice(first.pb, zt)).all()
    # the same sub-cycle through the untailed hierarchy's levels
    zr = torch.full(first.pb.lat.shape, NAN, dtype=dt)
    ref._vcycle(s, rt.clone(), zr)
    gap = ((_lattice(first.pb, zt).double() - _lattice(first.pb, zr).double()).abs().max()
           / _lattice(first.pb, zr).double().abs().max()).item()
    print(f"{name} {dt}: pmg_tail vs _vcycle({s}), gap {gap:.3e}")
    assert gap <= min(10 * MEASURED_SUB[(name, dt)], CAP[dt])
    with pytest.raises(TypeError):
        first.k.pmg_tail(pmg.tail, rt.to(torch.float16), zt)
    with pytest.raises(TypeError):
        first.k.pmg_tail(pmg.tail, pb.new_vector(), pb.new_vector())    # level 0's shape


# ---------------------------------------------------------- 3. default unchanged
@pytest.mark.parametrize("dt", DTYPES)
def test_default_and_empty_tail_are_bitwise_unchanged(dt):
    pb, ref, _, r, zref = _pair("a", 0.2, "random", dt)
    for N in (0, 10):                                           # 10: below every level (60)
        pmg = PMultigrid(pb, h_levels=-1, tail_nodes=N)
        assert pmg.tail is None and pmg.tail_start is None and pmg.tail_levels == 0
        z = torch.full(pb.lat.shape, NAN, dtype=dt)
        pmg.apply(r.clone(), z)
        assert torch.equal(_bits(z), _bits(zref))
        keys = {"degrees", "lambda_max", "smooth_degree", "coarse_degree", "h_levels", "h_cells"}
        assert set(pmg.info()) == (keys if N == 0 else keys | {"tail_nodes", "tail_levels"})
        if N:
            assert pmg.info()["tail_nodes"] == 10 and pmg.info()["tail_levels"] == 0
    assert set(ref.info()) == keys
    assert set(PMultigrid(pb).info()) == keys - {"h_levels", "h_cells"}


def test_tail_stops_at_the_first_level_that_does_not_qualify():
    """Degree 3 never joins, however large N; without h-levels the tail is the
    degree-1 level alone."""
    pb = _problem((4, 4, 4), 3)
    pmg = PMultigrid(pb, h_levels=-1, tail_nodes=32768)
    assert pmg.degrees == [3, 1] and pmg.tail_start == 1 and pmg.tail_levels == 1 + pmg.h_levels
    flat = PMultigrid(pb, tail_nodes=32768)
    assert flat.tail_start == 1 and flat.tail_levels == 1


# ------------------------------------------------------- 4. launch replacement
class _Counting:
    """Forwards to `real` and logs (level, method) of every call."""

    def __init__(self, real, level, log):
        self._real, self._level, self._log = real, level, log

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            self._log.append((self._level, name))
            return attr(*args, **kw)
        return call


def _logged_apply(pmg, r):
    log = []
    saved = [(lv.k, lv.op) for lv in pmg.levels]
    for i, lv in enumerate(pmg.levels):
        lv.k, lv.op = _Counting(lv.k, i, log), _Counting(lv.op, i, log)
    try:
        pmg.apply(r.clone(), pmg.pb.new_vector())
    finally:
        for lv, (k, op) in zip(pmg.levels, saved):
            lv.k, lv.op = k, op
    return log


@pytest.mark.parametrize("name", list(CASES))
def test_one_tail_call_replaces_the_tail_levels_calls(name):
    pb, ref, pmg, r, _ = _pair(name, 0.0, "constant", torch.float64)
    s = pmg.tail_start
    untailed, tailed = _logged_apply(ref, r), _logged_apply(pmg, r)
    assert tailed.count((s, "pmg_tail")) == 1
    assert sum(name == "pmg_tail" for _, name in tailed) == 1
    assert not [c for c in tailed if c[0] >= s and c != (s, "pmg_tail")]
    assert {n for lv, n in untailed if lv >= s} >= {"cheb_step", "apply"}
    # the levels above: the untailed sequence, the tail's calls collapsed into one
    want, placed = [], False
    for c in untailed:
        if c[0] < s:
            want.append(c)
        elif not placed:
            want.append((s, "pmg_tail"))
            placed = True
    assert tailed == want
    if s == 0:
        assert tailed == [(0, "pmg_tail")]


# ------------------------------------------------- 5. symmetry and positivity
@pytest.mark.parametrize("name", ["b600", "c"])
def test_tailed_vcycle_symmetric_positive(name):
    """The bound of tests/test_cpu_hpmg.py::test_h_vcycle_symmetric_positive."""
    pb, _, pmg, _, _ = _pair(name, 0.2, "random", torch.float64)
    bc = pb.bc_mask()
    gen = torch.Generator().manual_seed(5)
    a, b = (torch.randn(pb.lat.shape, dtype=torch.float64, generator=gen).masked_fill_(bc, 0.0)
            for _ in range(2))
    a0 = a.clone()
    za, zb = pb.new_vector(), pb.new_vector()
    pmg.apply(a, za)
    pmg.apply(b, zb)
    assert torch.equal(a, a0)
    s1, s2 = pb.inner(za, b), pb.inner(a, zb)
    print(f"{name}: <M^-1 a, b> = {s1!r}, <a, M^-1 b> = {s2!r}, rel gap "
          f"{abs(s1 - s2) / abs(s1):.3e}")
    assert abs(s1 - s2) <= 1e-12 * abs(s1)
    assert pb.inner(za, a) > 0 and pb.inner(zb, b) > 0


# ------------------------------------------------------------------ 6. solve
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("nc,P,N,want", [((13, 15, 17), 1, 600, 2), ((6, 5, 9), 3, 1024, 2),
                                         ((8, 8, 8), 3, 1024, 3)])
def test_tailed_solve_converges_like_the_untailed_one(nc, P, N, want, mixed):
    """Iterations to 1e-8: the preconditioners differ by rounding only, so at
    most one iteration more."""
    pb = _problem(nc, P, pert=0.2, coef="random")
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    kw = dict(h_levels=-1, cycle_dtype=torch.float32 if mixed else None)
    ref, pmg = PMultigrid(pb, **kw), PMultigrid(pb, tail_nodes=N, **kw)
    assert pmg.tail_levels == want and pmg.mixed == mixed
    assert pmg.tail.dtype == (torch.float32 if mixed else torch.float64)
    k0, r0 = _iterations(pb, op, b, precond=ref.apply)
    k1, r1 = _iterations(pb, op, b, precond=pmg.apply)
    print(f"{nc} Q{P} mixed={mixed}: {k0} iterations untailed ({r0:.2e}), {k1} tailed ({r1:.2e})")
    assert r0 <= 1e-8 and r1 <= 1e-8 and k1 <= k0 + 1


# -------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("N", [-1, -5, 32769, 10 ** 6, 2.0, True])
def test_tail_nodes_out_of_range_is_refused(N):
    with pytest.raises(ValueError, match="tail_nodes"):
        PMultigrid(_problem((4, 4, 4), 1), h_levels=-1, tail_nodes=N)


def test_tail_nodes_cap_is_accepted():
    pmg = PMultigrid(_problem((4, 4, 4), 1), h_levels=-1, tail_nodes=32768)
    assert pmg.tail_levels == 2 and pmg.info()["tail_nodes"] == 32768


def _rank_refusal(comm):
    pb = _problem((8, 8, 8), 1, comm=comm)
    try:
        PMultigrid(pb, h_levels=-1, tail_nodes=1024)
    except ValueError as e:
        return str(e)
    return None


def test_more_than_one_rank_is_refused():
    for msg in run_threaded(2, _rank_refusal):
        assert msg is not None and "tail_nodes" in msg and "single rank" in msg
    assert run_threaded(1, _rank_refusal)[0] is None


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


# --ndofs_global 15625 at Q3: (8, 8, 8) cells; degree 1 has 729 nodes
CLI = ["-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs_global", "15625", "--degree",
       "3", "--cg", "--nreps", "10", "--precond", "pmg"]


@pytest.mark.parametrize("args", [
    ["--cg", "--pmg_tail", "1024"],
    ["--cg", "--precond", "jacobi", "--pmg_tail", "1024"],
    ["--precond", "pmg", "--pmg_tail", "1024"],
    ["--cg", "--precond", "pmg", "--pmg_tail", "-1"],
    ["--cg", "--precond", "pmg", "--pmg_tail", "32769"],
])
def test_cli_pmg_tail_refusals(args):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and "pmg_tail" in (r.stdout + r.stderr)


def test_cli_pmg_tail_refuses_two_processes(tmp_path):
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node=2", "--master-addr=127.0.0.1", "--master-port=29671",
                        *CLI, "--pmg_hlevels", "-1", "--pmg_tail", "1024", "--json",
                        str(tmp_path / "t2.json")],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "'pmg_tail' needs a single rank" in (r.stdout + r.stderr)
    assert not (tmp_path / "t2.json").exists()


def _cli(extra, js):
    r = subprocess.run([sys.executable, *CLI, *extra, "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(js))


def test_cli_pmg_tail(tmp_path):
    d = _cli(["--pmg_hlevels", "-1", "--pmg_tail", "1024", "--mat_comp"], tmp_path / "t.json")
    blk = d["mi355x"]["pmg"]
    assert blk["tail_nodes"] == 1024 and blk["tail_levels"] == 3
    assert blk["h_cells"] == [[4, 4, 4], [2, 2, 2]] and blk["degrees"] == [3, 1]
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"matrix-free tailed pmg-PCG vs CSR tailed pmg-PCG: relative error norm {rel:.3e}")
    assert rel < 1e-10
    d0 = _cli(["--pmg_hlevels", "-1"], tmp_path / "h.json")
    assert "tail_nodes" not in d0["mi355x"]["pmg"] and "tail_levels" not in d0["mi355x"]["pmg"]
    assert d0["mi355x"]["pmg"]["lambda_max"] == blk["lambda_max"]
    assert d["output"]["u_norm"] == d0["output"]["u_norm"]      # the right-hand side's
    y1, y0 = d["output"]["y_norm"], d0["output"]["y_norm"]
    gap = abs(y1 - y0) / abs(y0)
    print(f"y_norm tailed {y1!r}, untailed {y0!r}, relative gap {gap:.3e}")
    assert gap <= min(10 * MEASURED_CLI, CAP[torch.float64])
