"""Mixed-precision multigrid (FP32 V-cycle inside FP64 CG), CPU path: the host
twins of the demote / promote kernels against numpy, the unchanged default,
the mixed `apply` against the composition of existing code (bitwise), its
closeness to the FP64 cycle, symmetry and positivity, iteration counts and the
outer accuracy, threaded ranks, and the `--pmg_float` CLI.

Bounds.  Closeness 1e-5 against a measured <= 2.3e-7 (a level built with the
wrong kappa or geometry is off by 1e-2 or more); symmetry 1e-6 |u| |M v|
against a measured <= 4.7e-9; the true residual of the rtol = 1e-12 solve is
asserted at 1e-12 itself, which a pure FP32 solve cannot reach."""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import HostKernels
from benchmark_dolfinx_amd.parallel.comm import run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import _bits, _iterations, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
FOUR = {"degrees", "lambda_max", "smooth_degree", "coarse_degree"}


# --------------------------------------------------- 1. host twins vs numpy
# (owned extents, storage shape): rows longer than a wave with ghost planes in
# x and y and a pitch of 80; more rows than 2048 blocks of 4 cover; one entry
EXTENTS = {
    (3, 5, 67): (4, 6, 80),
    (96, 96, 3): (97, 97, 16),
    (1, 1, 1): (2, 2, 16),
}
# +-0, exact ties between two floats (to even: down to 1, up to 1 + 2^-22), a
# large value, values that demote to FP32 subnormals (one of them a tie)
SPECIAL = [0.0, -0.0, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1e30, -1e30,
           1e-40, -3e-42, 2.0 ** -149 * 1.5, 2.0 ** -150]


def owned_mask(o, shape):
    m = np.zeros(shape, dtype=bool)
    m[: o[0], : o[1], : o[2]] = True
    return m


def boundary_input(o, shape, seed=0):
    """Random doubles on the owned box with SPECIAL at its start (as far as it
    has room), NaN on every other entry: ghost planes and pitch padding."""
    a = np.full(shape, np.nan)
    own = owned_mask(o, shape)
    vals = np.random.default_rng(seed).standard_normal(int(own.sum())) * 3.0
    n = min(len(SPECIAL), vals.size)
    vals[:n] = SPECIAL[:n]
    if vals.size == 1:
        vals[0] = SPECIAL[2]
    a[own] = vals
    return a, own


def nan_sentinel(shape, np_dtype):
    return np.full(shape, np.nan, dtype=np_dtype)


def same_bits(a, b):
    return np.array_equal(a.view(f"u{a.itemsize}"), b.view(f"u{b.itemsize}"))


def check_boundary_kernels(demote, promote, o, shape):
    """`demote(a64, out32)` / `promote(a32, out64)` on numpy arrays of the
    storage shape.  Shared with tests/test_gpu_pmg_mixed.py."""
    a, own = boundary_input(o, shape)
    a0 = a.copy()
    out = nan_sentinel(shape, np.float32)
    sent32 = out.copy()
    demote(a, out)
    assert same_bits(a, a0)
    with np.errstate(over="ignore", under="ignore"):
        want = a.astype(np.float32)
    assert same_bits(out[own], want[own])
    assert same_bits(out[~own], sent32[~own])                    # still the NaN bit pattern
    back = nan_sentinel(shape, np.float64)
    sent64 = back.copy()
    promote(out, back)
    assert same_bits(back[own], want[own].astype(np.float64))    # exact
    assert same_bits(back[~own], sent64[~own])
    return out, back


def _host_call(name, o):
    """The entry point on numpy arrays of the storage shape, extents `o`."""
    fn = getattr(native.host(), name)
    return lambda a, out: fn(a.shape[1], a.shape[2], *o, a.ctypes.data, out.ctypes.data)


@pytest.mark.parametrize("o", list(EXTENTS))
def test_host_twins_vs_numpy(o):
    out, _ = check_boundary_kernels(_host_call("bdx_cpu_demote_f64_f32", o),
                                    _host_call("bdx_cpu_promote_f32_f64", o), o, EXTENTS[o])
    if o == (3, 5, 67):
        row = out[0, 0]
        assert row[2] == np.float32(1.0) and row[3] == np.float32(1.0 + 2.0 ** -22)
        assert row[5] == np.float32(1e30) and 0 < row[7] < np.finfo(np.float32).tiny


def test_host_twins_are_declared_and_typed():
    lib = native.host()
    for name in ("bdx_cpu_demote_f64_f32", "bdx_cpu_promote_f32_f64"):
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == 7 and f.argtypes[0] is ctypes.c_int64
    pb = _problem((2, 2, 2), 2)
    k = HostKernels(pb.lat, F32)
    a, out = pb.new_vector(), torch.zeros(pb.lat.shape, dtype=F32)
    with pytest.raises(TypeError):
        k.demote(out, out)
    with pytest.raises(TypeError):
        k.promote(a, a)
    with pytest.raises(TypeError):
        k.demote(a, out[:1])


# ------------------------------------------------------ 2. default unchanged
def _rhs(pb, seed=3):
    return torch.randn(pb.lat.shape, dtype=F64,
                       generator=torch.Generator().manual_seed(seed)).masked_fill_(pb.bc_mask(), 0.0)


def test_default_is_unchanged():
    pb = _problem((4, 4, 4), 3, pert=0.2, coef="random")
    ms = [PMultigrid(pb), PMultigrid(pb, cycle_dtype=None), PMultigrid(pb, cycle_dtype=F64)]
    r = _rhs(pb)
    zs = []
    for m in ms:
        assert not m.mixed and m.rc is None and m.zc is None
        assert m.levels[0].pb is pb and m.pb is pb
        assert set(m.info()) == FOUR
        z = pb.new_vector()
        m.apply(r, z)
        zs.append(z)
    assert torch.equal(_bits(zs[0]), _bits(zs[1])) and torch.equal(_bits(zs[0]), _bits(zs[2]))
    zc = pb.new_vector()
    ms[0].apply_cycle(r, zc)                                     # unmixed: the same cycle
    assert torch.equal(_bits(zc), _bits(zs[0]))
    h = PMultigrid(pb, h_levels=-1, cycle_dtype=F64)
    assert set(h.info()) == FOUR | {"h_levels", "h_cells"}
    pb32 = _problem((4, 4, 4), 3, F32)
    m32 = PMultigrid(pb32, cycle_dtype=F32)                      # equal to the problem's: unmixed
    assert not m32.mixed and m32.levels[0].pb is pb32 and set(m32.info()) == FOUR


def test_cycle_dtype_refusals():
    pb, pb32 = _problem((2, 2, 2), 2), _problem((2, 2, 2), 2, F32)
    with pytest.raises(ValueError):
        PMultigrid(pb32, cycle_dtype=F64)
    for bad in (torch.float16, torch.bfloat16, torch.int32, 32, "float32", np.float32):
        with pytest.raises(ValueError):
            PMultigrid(pb, cycle_dtype=bad)


# ------------------------------- 3. mixed apply = composition of existing code
@pytest.mark.parametrize("nc,pert,coef,hl", [
    ((4, 4, 4), 0.2, "random", 0),
    ((5, 4, 7), 0.0, "constant", -1),
    ((5, 4, 7), 0.2, "random", -1),
])
def test_mixed_apply_is_the_fp32_cycle_promoted(nc, pert, coef, hl):
    pb = _problem(nc, 3, pert=pert, coef=coef)
    pb32 = _problem(nc, 3, F32, pert=pert, coef=coef)
    mixed = PMultigrid(pb, h_levels=hl, cycle_dtype=F32)
    ref = PMultigrid(pb32, h_levels=hl)
    assert mixed.mixed and mixed.pb is pb and mixed.cycle_dtype == F32
    assert all(lv.pb.dtype == F32 for lv in mixed.levels) and len(mixed.levels) == len(ref.levels)
    assert mixed.levels[0].pb is not pb and mixed.levels[0].pb.lat.shape == pb.lat.shape
    assert mixed.rc.dtype == F32 and mixed.zc.dtype == F32
    assert tuple(mixed.rc.shape) == tuple(mixed.zc.shape) == tuple(pb.lat.shape)
    assert mixed.lambda_max == ref.lambda_max and mixed.h_cells == ref.h_cells
    info = mixed.info()
    assert info["cycle_float"] == 32 and "cycle_float" not in ref.info()
    assert set(info) == FOUR | ({"h_levels", "h_cells"} if hl else set()) | {"cycle_float"}
    r = _rhs(pb)
    r0 = r.clone()
    z = torch.full(pb.lat.shape, float("nan"), dtype=F64)
    mixed.apply(r, z)
    assert torch.equal(_bits(r), _bits(r0))
    z32 = pb32.new_vector()
    ref.apply(r.float(), z32)
    own = torch.from_numpy(owned_mask(pb.lat.owned_hi, pb.lat.shape))
    assert torch.equal(_bits(z[own]), _bits(z32.double()[own]))
    assert torch.isnan(z[~own]).all()                            # only owned entries are written
    # apply_cycle is the raw FP32 cycle
    zc = pb32.new_vector()
    mixed.apply_cycle(r.float(), zc)
    assert torch.equal(_bits(zc[own]), _bits(z32[own]))


# --------------------------------- 4. closeness, symmetry and positivity
@pytest.mark.parametrize("nc,P", [((4, 4, 4), 3), ((6, 6, 6), 6)])
def test_mixed_cycle_close_symmetric_positive(nc, P):
    pb = _problem(nc, P, pert=0.2, coef="random")
    mixed, full = PMultigrid(pb, h_levels=-1, cycle_dtype=F32), PMultigrid(pb, h_levels=-1)
    lam = np.abs(np.array(mixed.lambda_max) - np.array(full.lambda_max))
    print(f"{nc} Q{P}: lambda_max gaps {lam}")
    u, v = _rhs(pb, 5), _rhs(pb, 6)
    mu, mv, fu = pb.new_vector(), pb.new_vector(), pb.new_vector()
    mixed.apply(u, mu)
    mixed.apply(v, mv)
    full.apply(u, fu)
    gap = pb.norm(mu - fu) / pb.norm(fu)
    s1, s2 = pb.inner(v, mu), pb.inner(u, mv)
    sym = abs(s1 - s2) / (pb.norm(u) * pb.norm(mv))
    print(f"{nc} Q{P}: |Mu - M64 u| / |M64 u| = {gap:.3e}; symmetry gap {sym:.3e}; "
          f"<u, Mu> = {pb.inner(u, mu):.6e}")
    assert gap <= 1e-5
    assert sym <= 1e-6
    assert pb.inner(u, mu) > 0 and pb.inner(v, mv) > 0


# -------------------------------------- 5. iterations and outer accuracy
TABLE = [
    ((8, 8, 8), 3, 0.2, "random", 0),
    ((8, 8, 8), 3, 0.2, "random", -1),
    ((6, 6, 6), 6, 0.2, "random", -1),
    ((16, 16, 16), 3, 0.0, "constant", -1),
    ((5, 4, 7), 5, 0.2, "random", -1),
    ((6, 5, 4), 2, 0.1, "random", -1),
]


@pytest.mark.parametrize("nc,P,pert,coef,hl", TABLE)
def test_iterations_and_outer_accuracy(nc, P, pert, coef, hl):
    pb = _problem(nc, P, pert=pert, coef=coef)
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    mixed, full = PMultigrid(pb, h_levels=hl, cycle_dtype=F32), PMultigrid(pb, h_levels=hl)
    k64, r64 = _iterations(pb, op, b, precond=full.apply)
    k32, r32 = _iterations(pb, op, b, precond=mixed.apply)
    x = pb.new_vector()
    k12 = cg_solve(op, pb, x, b, 1000, 1e-12, precond=mixed.apply)
    y = pb.new_vector()
    op.apply(x.clone(), y)
    res = pb.norm(b - y) / pb.norm(b)
    print(f"{nc} Q{P} pert {pert} {coef} h {hl}: to 1e-8 {k64} (FP64 cycle, {r64:.2e}) / {k32} "
          f"(FP32 cycle, {r32:.2e}); to 1e-12 {k12} iterations, true residual {res:.2e}")
    assert r64 <= 1e-8 and r32 <= 1e-8 and k32 <= k64 + 1
    assert k12 < 1000 and res <= 1e-12


# ------------------------------------------------------ 6. threaded ranks
def _rank_solve(comm, nc, P):
    pb = _problem(nc, P, pert=0.2, coef="random", comm=comm)
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    pmg = PMultigrid(pb, h_levels=-1, cycle_dtype=F32)
    k, res = _iterations(pb, op, b, precond=pmg.apply)
    return k, res, pmg.info()


def test_mixed_solve_over_threaded_ranks():
    """(8, 8, 8) cells: every cut is an even vertex, so the ranks build the
    one-rank hierarchy."""
    nc, P = (8, 8, 8), 3
    k1, res1, info1 = run_threaded(1, _rank_solve, nc, P)[0]
    assert res1 <= 1e-8 and info1["cycle_float"] == 32
    for R in (2, 4):
        for k, res, info in run_threaded(R, _rank_solve, nc, P):
            print(f"{R} ranks: {k} iterations (one rank {k1}), true residual {res:.2e}")
            assert res <= 1e-8 and abs(k - k1) <= 1
            assert info["h_cells"] == info1["h_cells"] and info["cycle_float"] == 32


# ------------------------------------------------------------------ 7. CLI
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


# --ndofs_global 15625 at Q3: (8, 8, 8) cells, every cut an even vertex
CLI = ["-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs_global", "15625", "--degree",
       "3", "--cg", "--nreps", "10", "--precond", "pmg"]
TORCHRUN2 = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
             "--master-addr=127.0.0.1", "--master-port=29669"]


def _cli(launch, extra, js):
    r = subprocess.run([*launch, *CLI, *extra, "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(js))


def test_cli_pmg_float(tmp_path):
    mixed = ["--pmg_float", "32", "--pmg_hlevels", "-1", "--mat_comp"]
    d = _cli([sys.executable], mixed, tmp_path / "m.json")
    blk = d["mi355x"]["pmg"]
    assert set(blk) == FOUR | {"h_levels", "h_cells", "cycle_float"} and blk["cycle_float"] == 32
    assert blk["h_cells"] == [[4, 4, 4], [2, 2, 2]] and d["input"]["scalar_size"] == 64
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"1 process: matrix-free vs CSR with one mixed preconditioner, relative error {rel:.3e}")
    assert rel < 1e-10
    d2 = _cli(TORCHRUN2, mixed, tmp_path / "m2.json")
    assert d2["input"]["mpi_size"] == 2 and d2["mi355x"]["pmg"]["cycle_float"] == 32
    assert set(d2["mi355x"]["pmg"]) == set(blk)
    rel2 = d2["mi355x"]["e_norm"] / d2["output"]["z_norm"]
    print(f"2 processes: relative error {rel2:.3e}")
    assert rel2 < 1e-10
    # without the option, and with it equal to --float: the pinned key sets
    h = _cli([sys.executable], ["--pmg_hlevels", "-1"], tmp_path / "h.json")
    assert set(h["mi355x"]["pmg"]) == FOUR | {"h_levels", "h_cells"}
    same = _cli([sys.executable], ["--pmg_float", "64"], tmp_path / "s.json")
    assert set(same["mi355x"]["pmg"]) == FOUR                    # equal to --float: unmixed


@pytest.mark.parametrize("args", [
    ["--cg", "--pmg_float", "32"],
    ["--cg", "--precond", "jacobi", "--pmg_float", "32"],
    ["--precond", "pmg", "--pmg_float", "32"],
    ["--cg", "--precond", "pmg", "--float", "32", "--pmg_float", "64"],
])
def test_cli_pmg_float_refusals(args):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and "pmg_float" in (r.stdout + r.stderr)
