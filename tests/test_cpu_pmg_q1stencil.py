"""Degree-1 multigrid levels on assembled 27-point stencils
(`PMultigrid(q1_operator="stencil")`), CPU path: the host twins of
`bdx_stencil27_apply` / `bdx_stencil27_cheb` against a NumPy evaluation of the
27 shifted products, the fused Chebyshev step against apply + `cheb_step` bit
for bit, the stencil against the matrix-free operator, the cycle (default
unchanged, launches, options, threaded ranks) and the `--pmg_q1` CLI.  The
`check_*` and `rank_*` functions take the platform; tests/
test_gpu_pmg_q1stencil.py runs them on the device kernels.

Meshes (degree 1, perturbed 0.2, random kappa): (2, 3, 70), whose rows of 71
nodes are two z-chunks of a wave, the second of 7 lanes; (1, 1, 1), where
every neighbour test hits a lattice face; (5, 4, 3).

Bounds.  Apply against the float64 reference: both sums have at most 27
terms, so each is within gamma_27 (|S||u|)_i of the exact sum in its
precision, 27 u / (1 - 27 u) < 32 u; the two together stay below
64 u (|S||u|)_i with u = 2^-53 or 2^-24, the reference's own error in float64
included.  Stencil against the matrix-free operator: a multiple of u (|S||u|)_i
measured on this code (MEASURED_MATFREE, recorded in
profiles/pmg_q1stencil.md) and asserted at 10 x, the project's allowance for
box-to-box differences in rounding order, never looser than 1e-12 (FP64) /
1e-4 (FP32) of max |y|."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.driver import make_operator
from benchmark_dolfinx_amd.models.poisson import CSROperator, MatFreeLaplacianCPU, PoissonProblem
from benchmark_dolfinx_amd.ops import native
from benchmark_dolfinx_amd.ops.kernels import stencil27
from benchmark_dolfinx_amd.ops.native import ptr
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid
from test_cpu_pmg import NAN, _bits
from test_cpu_pmg_tail import _logged_apply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
MESHES = [(2, 3, 70), (1, 1, 1), (5, 4, 3)]
# the fused step against `cheb_step` also on rows of 131 and 201 nodes: three
# and four entries per lane of `cheb_step`'s row walk, whose FP32 device code
# rounds a lane's paired entries and its odd last one differently
# (csrc/hip/lap_stencil27.h: cheb_step_fuses)
FUSED_MESHES = MESHES + [(1, 1, 130), (1, 2, 200)]
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}     # unit roundoff
CAP_MATFREE = {torch.float64: 1e-12, torch.float32: 1e-4}
# max_i |S u - A_matfree u|_i / (u (|S||u|)_i) on the owned entries of MESHES,
# host twins against MatFreeLaplacianCPU (profiles/pmg_q1stencil.md)
MEASURED_MATFREE = {("cpu", torch.float64): 3.38, ("cpu", torch.float32): 3.25}
FOUR = {"degrees", "lambda_max", "smooth_degree", "coarse_degree"}


def _pb(nc, P=1, dt=torch.float64, platform="cpu", comm=None, pert=0.2, coef="random"):
    return PoissonProblem(comm or Comm(), nc, P, 1, False, dt, platform, pert, coef)


def _kern(pb):
    return pb.kernels


def _stencil(pb):
    return torch.from_numpy(stencil27(CSROperator(pb), pb.lat)).to(pb.device)


def _vector(pb, seed, pad=NAN, positive=False):
    """Random lattice vector with `pad` in the storage padding."""
    v = torch.randn(pb.lat.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    if positive:
        v = v.abs() + 0.5
    v[:, :, pb.lat.L[2]:] = pad
    return v.to(pb.dtype).to(pb.device)


def _owned(pb):
    m = torch.zeros(pb.lat.shape, dtype=torch.bool)
    o = pb.lat.owned_hi
    m[: o[0], : o[1], : o[2]] = True
    return m


def numpy_stencil(pb, S, u):
    """(S u, |S||u|) on the lattice in float64: the 27 shifted products, the
    neighbours outside the lattice skipped."""
    L = [int(x) for x in pb.lat.L]
    S = S.cpu().double().numpy().reshape(27, L[0], L[1], int(pb.lat.ld))[:, :, :, : L[2]]
    u = u.cpu().double().numpy()[:, :, : L[2]]
    y, ya = np.zeros(L), np.zeros(L)
    for p in range(27):
        d = (p // 9 - 1, p // 3 % 3 - 1, p % 3 - 1)
        to = tuple(slice(max(0, -s), n - max(0, s)) for s, n in zip(d, L))
        fr = tuple(slice(max(0, s), n - max(0, -s)) for s, n in zip(d, L))
        y[to] += S[p][to] * u[fr]
        ya[to] += np.abs(S[p][to] * u[fr])
    return y, ya


# ------------------------------------------------------ 1. the kernels, one rank
def check_apply_vs_numpy(platform, nc, dt):
    pb = _pb(nc, 1, dt, platform)
    k, S, L2 = _kern(pb), _stencil(pb), pb.lat.L[2]
    u = _vector(pb, 3)                                    # NaN in the padding
    y0 = torch.full(pb.lat.shape, NAN, dtype=dt)
    y = y0.clone().to(pb.device)
    k.stencil27_apply(S, u, y)
    y = y.cpu()
    assert torch.isfinite(y[:, :, :L2]).all()
    assert torch.equal(_bits(y[:, :, L2:]), _bits(y0[:, :, L2:]))     # padding untouched
    ref, ya = numpy_stencil(pb, S, u)
    err = np.abs(y[:, :, :L2].double().numpy() - ref)
    ratio = (err / np.maximum(UNIT[dt] * ya, 1e-300)).max()
    print(f"stencil27_apply {platform} {nc} {dt}: max err / (u |S||u|) = {ratio:.3f} (bound 64)")
    assert (err <= 64 * UNIT[dt] * ya).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
def test_apply_host_twin_vs_numpy(nc, dt):
    check_apply_vs_numpy("cpu", nc, dt)


def rank_fused_vs_composition(comm, nc, dt, platform="cpu"):
    """One and three chained `stencil27_cheb` steps against `stencil27_apply`
    into a scratch y followed by `cheb_step`, bit for bit; NaN in every
    padding; what is not owned in z_out keeps its bits."""
    pb = _pb(nc, 1, dt, platform, comm)
    k, S, own = _kern(pb), _stencil(pb), _owned(pb)
    dinv, r = _vector(pb, 5, positive=True), _vector(pb, 6)
    zc, dc = _vector(pb, 7), _vector(pb, 8)               # the composition, in place
    d = dc.clone()
    # the other buffer: a sentinel where z_out is written, the iterate's ghost
    # values (and NaN padding) elsewhere, as the composition reads them in place
    buf = [zc.clone(), torch.where(own, 7.0, zc.cpu().double()).to(dt).to(pb.device)]
    keep = [b.cpu().clone() for b in buf]
    y = torch.full(pb.lat.shape, NAN, dtype=dt).to(pb.device)
    coef = [(0.37, 0.81), (0.21, 1.3), (0.55, 0.66)]
    for s, (a, b) in enumerate(coef):
        k.stencil27_apply(S, zc, y)
        k.cheb_step(False, a, b, dinv, r, y, dc, zc)
        k.stencil27_cheb(S, dinv, r, buf[s % 2], d, buf[1 - s % 2], a, b)
        if s in (0, 2):
            out = buf[1 - s % 2].cpu()
            assert torch.isfinite(out[own]).all()
            assert torch.equal(_bits(out[own]), _bits(zc.cpu()[own])), f"z after {s + 1} steps"
            assert torch.equal(_bits(out[~own]), _bits(keep[1][~own]))
            assert torch.equal(_bits(d.cpu()), _bits(dc.cpu())), f"d after {s + 1} steps"
    assert torch.equal(_bits(buf[0].cpu()[~own]), _bits(keep[0][~own]))
    return int((~own[:, :, : pb.lat.L[2]]).sum())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", FUSED_MESHES)
def test_fused_step_is_the_composition_bitwise(nc, dt):
    assert rank_fused_vs_composition(Comm(), nc, dt) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_step_leaves_ghost_planes_alone_on_two_ranks(dt):
    ghosts = run_threaded(2, rank_fused_vs_composition, (5, 4, 3), dt)
    assert max(ghosts) > 0


def check_refusals(platform, dt):
    """z_out is z_in, a degree-2 descriptor and a null pointer: non-zero, and
    nothing written."""
    pb, pb2 = _pb((2, 2, 2), 1, dt, platform), _pb((2, 2, 2), 2, dt, platform)
    S = _stencil(pb)
    suf = "f64" if dt == torch.float64 else "f32"
    vec = {n: _vector(pb, i, pad=0.0, positive=True) for i, n in enumerate(("dinv", "r", "z", "d", "o"))}
    before = {n: v.cpu().clone() for n, v in vec.items()}
    latd, latd2, own = pb.lat.as_int64(), pb2.lat.as_int64(), np.asarray(pb.lat.owned_hi, np.int64)
    if platform == "gpu":
        lib, st = native.hip(), (torch.cuda.current_stream().cuda_stream,)
        cheb, apply = getattr(lib, f"bdx_stencil27_cheb_{suf}"), getattr(lib, f"bdx_stencil27_apply_{suf}")
    else:
        lib, st = native.host(), ()
        cheb, apply = getattr(lib, f"bdx_cpu_stencil27_cheb_{suf}"), None

    def step(latd=latd, own=own, S=S, dinv=vec["dinv"], r=vec["r"], z_in=vec["z"], d=vec["d"],
             z_out=vec["o"]):
        return cheb(ptr(latd), ptr(own), ptr(S), ptr(dinv), ptr(r), ptr(z_in), ptr(d), ptr(z_out),
                    0.5, 0.5, *st)
    assert step(z_out=vec["z"]) != 0
    assert step(latd=latd2) != 0
    for name in ("latd", "own", "S", "dinv", "r", "z_in", "d", "z_out"):
        assert step(**{name: None}) != 0, name
    if apply is not None:
        assert apply(ptr(latd2), ptr(S), ptr(vec["z"]), ptr(vec["o"]), *st) != 0
        assert apply(ptr(latd), ptr(S), ptr(vec["z"]), ptr(vec["z"]), *st) != 0
        for bad in ((None, S, vec["z"], vec["o"]), (latd, None, vec["z"], vec["o"]),
                    (latd, S, None, vec["o"]), (latd, S, vec["z"], None)):
            assert apply(*(ptr(x) for x in bad), *st) != 0
        torch.cuda.synchronize()
    for n, v in vec.items():
        assert torch.equal(_bits(v.cpu()), _bits(before[n])), n
    # the launchers raise
    k, k2 = _kern(pb), _kern(pb2)
    with pytest.raises((ValueError, RuntimeError)):
        k.stencil27_cheb(S, vec["dinv"], vec["r"], vec["z"], vec["d"], vec["z"], 0.5, 0.5)
    v2 = pb2.new_vector()
    S2 = torch.zeros((27, pb2.lat.nstore), dtype=dt).to(pb2.device)
    with pytest.raises((ValueError, RuntimeError)):
        k2.stencil27_apply(S2, v2, pb2.new_vector())
    with pytest.raises((ValueError, RuntimeError)):
        k2.stencil27_cheb(S2, v2, v2, v2, pb2.new_vector(), pb2.new_vector(), 0.5, 0.5)
    with pytest.raises(TypeError):
        k.stencil27_apply(S[:26], vec["z"], vec["o"])
    assert step() == 0                                    # and the good call is accepted


@pytest.mark.parametrize("dt", DTYPES)
def test_host_twin_refusals(dt):
    check_refusals("cpu", dt)


# ------------------------------------- 2. stencil against the matrix-free operator
def check_stencil_vs_matfree(platform, dt):
    """Returns the measured multiple of u (|S||u|)_i over the three meshes."""
    worst = 0.0
    for nc in MESHES:
        pb = _pb(nc, 1, dt, platform)
        k, S, L2, own = _kern(pb), _stencil(pb), pb.lat.L[2], _owned(pb)
        u = _vector(pb, 11, pad=0.0).masked_fill_(pb.bc_mask(), 0.0)
        ys, ym = pb.new_vector(), pb.new_vector()
        k.stencil27_apply(S, u, ys)
        make_operator(pb, "auto", "auto").apply(u, ym)
        _, ya = numpy_stencil(pb, S, u)
        m = own[:, :, :L2].numpy()
        err = np.abs(ys.cpu().double().numpy() - ym.cpu().double().numpy())[:, :, :L2]
        ymax = float(ym.cpu().abs().max())
        ratio = float((err[m] / np.maximum(UNIT[dt] * ya[m], 1e-300)).max()) if ya[m].max() > 0 else 0.0
        print(f"stencil vs matfree {platform} {nc} {dt}: max err / (u |S||u|) = {ratio:.3f}, "
              f"max err / max |y| = {err[m].max() / max(ymax, 1e-300):.3e}")
        bound = np.minimum(10 * MEASURED_MATFREE[(platform, dt)] * UNIT[dt] * ya,
                           CAP_MATFREE[dt] * ymax)
        assert (err[m] <= bound[m]).all()
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("dt", DTYPES)
def test_stencil_vs_matfree_operator(dt):
    check_stencil_vs_matfree("cpu", dt)


# ------------------------------------------------------------ 3. the cycle
def _residual(pb, seed=3):
    r = torch.randn(pb.lat.shape, dtype=pb.dtype, generator=torch.Generator().manual_seed(seed))
    return r.to(pb.device).masked_fill_(pb.bc_mask(), 0.0)


def check_default_unchanged(platform):
    pb = _pb((4, 4, 4), 3, platform=platform)
    kw = dict(h_levels=-1)
    a, b, s = PMultigrid(pb, **kw), PMultigrid(pb, q1_operator="matfree", **kw), \
        PMultigrid(pb, q1_operator="stencil", **kw)
    assert a.q1_operator == b.q1_operator == "matfree" and s.q1_operator == "stencil"
    assert set(a.info()) == set(b.info()) == FOUR | {"h_levels", "h_cells"}
    assert set(s.info()) == set(a.info()) | {"q1_operator"} and s.info()["q1_operator"] == "stencil"
    assert a.lambda_max == b.lambda_max == s.lambda_max
    assert all(lv.S is None for lv in a.levels + b.levels)
    assert [lv.S is not None for lv in s.levels] == [lv.pb.degree == 1 for lv in s.levels]
    r = _residual(pb)
    za, zb = pb.new_vector(), pb.new_vector()
    a.apply(r, za)
    b.apply(r, zb)
    assert torch.equal(_bits(za.cpu()), _bits(zb.cpu()))
    assert _logged_apply(a, r) == _logged_apply(b, r)
    for bad in ("stencil27", "", None, 1, True):
        with pytest.raises(ValueError):
            PMultigrid(pb, q1_operator=bad)
    for p in (a, b, s):
        p.close()


def test_default_is_bitwise_unchanged_and_option_is_checked():
    check_default_unchanged("cpu")


def check_launches(platform, smooth):
    """One rank: a stencil level issues one `stencil27_cheb` per step that has
    an operator and one `stencil27_apply` for the residual, never the
    matrix-free operator or a second vector pass; the other levels keep their
    sequence."""
    pb = _pb((4, 4, 4), 3, platform=platform)
    kw = dict(h_levels=-1, smooth_degree=smooth)
    ref, s = PMultigrid(pb, **kw), PMultigrid(pb, q1_operator="stencil", **kw)
    r = _residual(pb)
    log, log0 = _logged_apply(s, r), _logged_apply(ref, r)
    last = len(s.levels) - 1
    for l, lv in enumerate(s.levels):
        mine = [n for i, n in log if i == l]
        if lv.S is None:
            assert mine == [n for i, n in log0 if i == l]
            continue
        assert "apply" not in mine
        if l == last:
            assert mine.count("stencil27_cheb") == s.coarse_degree - 1
            assert mine.count("cheb_step") == 1 and "stencil27_apply" not in mine
        else:
            assert mine.count("stencil27_cheb") == 2 * smooth - 1
            assert mine.count("cheb_step") == 1 and mine.count("stencil27_apply") == 1
    for p in (ref, s):
        p.close()


@pytest.mark.parametrize("smooth", [2, 3])
def test_a_stencil_level_fuses_every_step_on_one_rank(smooth):
    check_launches("cpu", smooth)


# 10 x the difference measured on this code (profiles/pmg_q1stencil.md:
# 4.2e-16 / 2.8e-7 of max |z| over the four cases), capped at 1e-13 / 1e-5
CYCLE_GAP = {torch.float64: min(10 * 4.2e-16, 1e-13), torch.float32: min(10 * 2.8e-7, 1e-5)}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kw", [dict(), dict(smooth_degree=3), dict(tail_nodes=27),
                                dict(p_transfer="row")], ids=str)
def test_cpu_cycle_differs_at_rounding_level_only(kw, dt):
    pb = _pb((4, 4, 4), 3, dt)
    a, s = PMultigrid(pb, h_levels=-1, **kw), PMultigrid(pb, h_levels=-1, q1_operator="stencil", **kw)
    if "tail_nodes" in kw:      # the h-level in the tail, the degree-1 p-level above it
        assert s.tail_start == 2 and s.levels[1].S is not None and s.levels[2].S is None
    r = _residual(pb)
    za, zs = pb.new_vector(), pb.new_vector()
    a.apply(r, za)
    s.apply(r, zs)
    gap = float((za - zs).abs().max() / za.abs().max())
    print(f"one cycle {kw} {dt}: max |dz| / max |z| = {gap:.3e} (bound {CYCLE_GAP[dt]:.1e})")
    assert gap <= CYCLE_GAP[dt]


def test_degree_one_problem_and_fp32_cycle_on_the_cpu():
    """Level 0 of a degree-1 problem is a stencil level; the FP32 cycle under
    an FP64 problem holds FP32 stencils.  Six PCG iterations against the
    default hierarchy."""
    for P, kw, tol in ((1, dict(), 1e-10), (3, dict(cycle_dtype=torch.float32), 2e-4)):
        pb = _pb((4, 4, 4), P)
        xs = []
        for q1 in ("matfree", "stencil"):
            pmg = PMultigrid(pb, h_levels=-1, q1_operator=q1, **kw)
            if q1 == "stencil":
                assert all((lv.S is not None) == (lv.pb.degree == 1) for lv in pmg.levels)
                assert all(lv.S.dtype == pmg.cycle_dtype for lv in pmg.levels if lv.S is not None)
            x = pb.new_vector()
            cg_solve(MatFreeLaplacianCPU(pb), pb, x, pb.assemble_rhs(), 6, precond=pmg.apply)
            xs.append(pb.to_global_array(x))
        gap = np.abs(xs[0] - xs[1]).max() / np.abs(xs[0]).max()
        print(f"Q{P} {kw}: stencil vs matfree after 6 iterations {gap:.3e}")
        assert gap < tol


# ------------------------------------------------------- 4. threaded ranks
ITS = 6


def rank_stencil_solve(comm, q1, platform="cpu", partition=None):
    """(global x after ITS iterations, lambda_max, the matfree hierarchy's,
    the levels' local cells)."""
    pb = PoissonProblem(comm, (4, 4, 4), 3, 1, False, torch.float64, platform, 0.2, "random",
                        partition=partition)
    pmg = PMultigrid(pb, h_levels=-1, q1_operator=q1)
    lam0 = PMultigrid(pb, h_levels=-1).lambda_max
    x = pb.new_vector()
    if platform == "gpu":
        from benchmark_dolfinx_amd.solvers.cg import DeviceCG
        op = make_operator(pb, "auto", "auto")
        cg = DeviceCG(pb, "pmg", pmg=pmg)
        cg.solve(op, x, pb.assemble_rhs(), ITS)
        cg.wait()
        if hasattr(op, "close"):
            op.close()
    else:
        cg_solve(MatFreeLaplacianCPU(pb), pb, x, pb.assemble_rhs(), ITS, precond=pmg.apply)
    out = pb.to_global_array(x), list(pmg.lambda_max), list(lam0), \
        [tuple(int(n) for n in lv.pb.lat.n) for lv in pmg.levels]
    pmg.close()
    return out


def check_threaded_ranks(platform, R, ref):
    """Eight ranks are split 2 x 2 x 2 on either platform (the device's default
    keeps x whole, which leaves 4 x 1 x 2 cells and no h-level: another
    hierarchy than one rank's, fem/mesh.py)."""
    for x, lam, lam0, cells in run_threaded(R, rank_stencil_solve, "stencil", platform,
                                            "xyz" if R == 8 else None):
        gap = np.abs(x - ref).max() / np.abs(ref).max()
        print(f"{platform} {R} ranks, local cells {cells}: gap to the one-rank stencil solve {gap:.3e}")
        assert gap <= 1e-10
        assert lam == lam0
    return cells


@pytest.fixture(scope="module")
def one_rank_solve():
    x = run_threaded(1, rank_stencil_solve, "stencil")[0][0]
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("R", [2, 4, 8])
def test_stencil_solve_on_threaded_ranks(R, one_rank_solve):
    cells = check_threaded_ranks("cpu", R, one_rank_solve)
    if R == 8:
        assert cells[1:] == [(2, 2, 2), (1, 1, 1)]


# ------------------------------------------------------------------ 5. CLI
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


def check_cli(platform, tmp_path):
    js = tmp_path / "q1.json"
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", platform,
                        "--ndofs=1000", "--degree=3", "--cg", "--nreps", "10", "--mat_comp",
                        "--precond", "pmg", "--pmg_q1", "stencil", "--json", str(js)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.load(open(js))
    blk = d["mi355x"]["pmg"]
    assert set(blk) == FOUR | {"q1_operator"} and blk["q1_operator"] == "stencil"
    assert d["output"]["ndofs_global"] == 1000
    rel = d["mi355x"]["e_norm"] / d["output"]["z_norm"]
    print(f"matrix-free vs CSR pmg-PCG with --pmg_q1 stencil on {platform}: relative error norm {rel:.3e}")
    assert rel < 1e-10


def test_cli_pmg_q1_stencil(tmp_path):
    check_cli("cpu", tmp_path)


@pytest.mark.parametrize("args", [
    ["--pmg_q1", "stencil"],
    ["--cg", "--pmg_q1", "stencil"],
    ["--cg", "--precond", "jacobi", "--pmg_q1", "stencil"],
    ["--cg", "--precond", "pmg", "--pmg_q1", "stencil27"],
])
def test_cli_pmg_q1_refusals(args):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and "pmg_q1" in (r.stdout + r.stderr)
