"""Row-streaming p-multigrid transfers (`p_transfer="row"`), CPU path: the
host twins of `bdx_prolong_row` / `bdx_restrict_row` against the dense model
of tests/test_cpu_pmg.py, their fold modes against the two-pass definitions,
agreement with the cell transfers, adjointness and partition invariance over
threaded ranks, `PMultigrid(p_transfer="row")` (default unchanged, refusals,
launch counts, symmetry, numpy PCG, convergence, combined options, ranks) and
the `--pmg_transfer` CLI.

Meshes: (2, 3, 2) and (1, 1, 1) cells as in tests/test_cpu_pmg.py, the seam
mesh (1, 2, 33) whose z axis has more cells than one wave's z-chunk holds for
every pair (the device kernels chunk a row by at most 63 // Pf <= 31 cells in
the prolongation and 63 // Pf - 1 <= 30 in the restriction), and the seam mesh
with x and z swapped, (33, 2, 1): a one-cell z row, whose only chunk is also
its last.  The per-entry bound is that module's: its factor 6 (2 Pf + 1)
covers the at most 2 Pf + 1 terms per axis of the gather."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchmark_dolfinx_amd.fem.mesh import make_local_lattice
from benchmark_dolfinx_amd.fem.quadrature import gll, lagrange_tables
from benchmark_dolfinx_amd.models.poisson import MatFreeLaplacianCPU
from benchmark_dolfinx_amd.parallel.comm import Comm, run_threaded
from benchmark_dolfinx_amd.solvers.cg import cg_solve
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid, chebyshev_coefficients
from test_cpu_pmg import (EPS, NAN, PAIRS, _adjoint_bound, _bits, _dense_levels, _fill, _glob,
                          _iterations, _np_lambda, _np_vcycle, _problem, _random, _shape,
                          model_prolong, model_restrict)
from test_cpu_pmg_tail import _logged_apply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
SEAM, SEAM_SWAPPED = (1, 2, 33), (33, 2, 1)
MESHES = [(2, 3, 2), (1, 1, 1), SEAM, SEAM_SWAPPED]
PARTITIONED = (4, 5, 3)          # the partitioned mesh of tests/test_cpu_pmg.py


def test_the_seam_mesh_exceeds_every_chunk():
    assert all(SEAM[2] > 63 // Pf and SEAM[2] > 63 // Pf - 1 for Pf, _ in PAIRS)
    assert SEAM_SWAPPED[2] == 1


def _table(Pf, Pc):
    return np.ascontiguousarray(lagrange_tables(gll(Pc + 1)[0], gll(Pf + 1)[0])[0])


def _kern(pb):
    return pb.kernels


def _pair(nc, Pf, Pc, dt, platform="cpu", comm=None):
    """Fine problem, coarse problem, fine kernels, coarse descriptor, table."""
    fine = _problem(nc, Pf, dt, comm=comm, platform=platform)
    coarse = _problem(nc, Pc, dt, comm=comm, platform=platform)
    return fine, coarse, _kern(fine), coarse.lat.as_int64(), _table(Pf, Pc)


def _ghost_nan(pb, v):
    """NaN on the ghost planes of v: a restriction must not read them."""
    o = pb.lat.owned_hi
    v[o[0]:], v[:, o[1]:], v[:, :, o[2]: pb.lat.L[2]] = NAN, NAN, NAN
    return v


def _owned_mask(pb):
    m = torch.zeros(pb.lat.shape, dtype=torch.bool)
    o = pb.lat.owned_hi
    m[: o[0], : o[1], : o[2]] = True
    return m


# -------------------------------------------- 1. the kernels vs the dense model
def check_prolong_row(platform, nc, Pf, Pc, dt):
    """vf = P vc against the dense model: NaN in the coarse padding, the fine
    vector NaN before; finite on the lattice, bitwise untouched outside it,
    the input bitwise unchanged.  Returns the result on the host."""
    fine, coarse, k, latc, J = _pair(nc, Pf, Pc, dt, platform)
    gc = _random(_shape(nc, Pc), 3, dt)
    vc = _fill(coarse, gc)
    vc0 = vc.clone()
    vf0 = torch.full(fine.lat.shape, NAN, dtype=dt)
    vf = vf0.clone().to(fine.device)
    k.prolong_row(latc, J, vc, vf)
    vf = vf.cpu()
    assert torch.equal(_bits(vc.cpu()), _bits(vc0.cpu()))
    L2 = fine.lat.L[2]
    assert torch.isfinite(vf[:, :, :L2]).all()
    assert torch.equal(_bits(vf[:, :, L2:]), _bits(vf0[:, :, L2:]))
    ref, bnd = model_prolong(nc, Pf, Pc, gc)
    err = np.abs(_glob(fine, vf) - ref)
    print(f"prolong_row {platform} {Pc}->{Pf} {nc} {dt}: max err / bound "
          f"{(err / (EPS[dt] * bnd)).max():.3e}")
    assert (err <= EPS[dt] * bnd).all()
    return vf, bnd


def check_restrict_row(platform, nc, Pf, Pc, dt, with_y):
    """vc = P^T (vf - y) against the dense model: NaN in the padding of vf and
    y and on their ghost planes, the coarse vector NaN before; finite on the
    lattice, bitwise untouched outside it, bitwise reproducible, the inputs
    bitwise unchanged.  Returns the result on the host."""
    fine, coarse, k, latc, J = _pair(nc, Pf, Pc, dt, platform)
    gf = _random(_shape(nc, Pf), 5, dt)
    gy = _random(_shape(nc, Pf), 6, dt) if with_y else None
    vf = _ghost_nan(fine, _fill(fine, gf))
    y = _ghost_nan(fine, _fill(fine, gy)) if with_y else None
    ins = [t.clone() for t in (vf, y) if t is not None]
    vc0 = torch.full(coarse.lat.shape, NAN, dtype=dt)
    outs = []
    for _ in range(2):
        vc = vc0.clone().to(coarse.device)
        k.restrict_row(latc, J, vf, y, vc)
        outs.append(vc.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    for t, t0 in zip([t for t in (vf, y) if t is not None], ins):
        assert torch.equal(_bits(t.cpu()), _bits(t0.cpu()))
    L2 = coarse.lat.L[2]
    assert torch.isfinite(outs[0][:, :, :L2]).all()
    assert torch.equal(_bits(outs[0][:, :, L2:]), _bits(vc0[:, :, L2:]))
    # vf - y is one rounding of a difference the model forms exactly: its
    # error eps |vf - y| enters the bound through |vf| + |y|
    ref, _ = model_restrict(nc, Pf, Pc, gf - gy if with_y else gf)
    _, bnd = model_restrict(nc, Pf, Pc, np.abs(gf) + np.abs(gy) if with_y else gf)
    err = np.abs(_glob(coarse, outs[0]) - ref)
    print(f"restrict_row {platform} {Pf}->{Pc} {nc} {dt} y={with_y}: max err / bound "
          f"{(err / (EPS[dt] * bnd)).max():.3e}")
    assert (err <= EPS[dt] * bnd).all()
    return outs[0], bnd


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_prolong_row_host_twin_vs_dense_model(Pf, Pc, nc, dt):
    check_prolong_row("cpu", nc, Pf, Pc, dt)


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_restrict_row_host_twin_vs_dense_model(Pf, Pc, nc, dt, with_y):
    check_restrict_row("cpu", nc, Pf, Pc, dt, with_y)


def test_row_host_twins_reject_bad_pairs_and_null_pointers():
    nc, Pf, Pc = (2, 3, 2), 4, 2
    fine, coarse, k, latc, J = _pair(nc, Pf, Pc, torch.float64)
    vf, vc = fine.new_vector(), coarse.new_vector()
    bad, other = _problem(nc, 3), _problem((2, 3, 3), Pc)
    for latd in (bad.lat.as_int64(), other.lat.as_int64(), coarse.lat.as_int64(tile=(4, 4))):
        with pytest.raises(ValueError):
            k.prolong_row(latd, J, vc, vf)
        with pytest.raises(ValueError):
            k.restrict_row(latd, J, vf, None, vc)
    for a, b in ((None, vf), (vc, None)):
        with pytest.raises(ValueError):
            k.prolong_row(latc, J, a, b)
        with pytest.raises(ValueError):
            k.restrict_row(latc, J, b, None, a)


# ------------------------------------------------------------ 2. fold modes
def rank_fold_modes(comm, nc, Pf, Pc, dt, platform="cpu"):
    """On this rank's piece: restrict_row(vf, y) is bitwise restrict_row(vf -
    y) with the difference formed by axpy, and prolong_row(add) is bitwise old
    + prolong_row on the owned nodes and leaves a NaN-filled rest alone."""
    fine, coarse, k, latc, J = _pair(nc, Pf, Pc, dt, platform, comm)
    vf = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 5, dt)))
    y = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 6, dt)))
    folded, two_pass = coarse.new_vector(), coarse.new_vector()
    k.restrict_row(latc, J, vf, y, folded)
    t = torch.full(fine.lat.shape, NAN, dtype=dt).to(fine.device)
    k.axpy(t, -1.0, y, vf)                                  # t = vf - y on the owned rows
    k.restrict_row(latc, J, t, None, two_pass)
    assert torch.equal(_bits(folded.cpu()), _bits(two_pass.cpu()))

    vc = _fill(coarse, _random(_shape(nc, Pc), 3, dt))
    plain = torch.full(fine.lat.shape, NAN, dtype=dt).to(fine.device)
    k.prolong_row(latc, J, vc, plain)
    own = _owned_mask(fine)
    old = torch.full(fine.lat.shape, NAN, dtype=dt)
    old[own] = torch.from_numpy(_random((int(own.sum()),), 7, dt)).to(dt)
    got = old.clone().to(fine.device)
    k.prolong_row(latc, J, vc, got, True)
    got, plain = got.cpu(), plain.cpu()
    assert torch.isfinite(got[own]).all()
    assert torch.equal(_bits(got[own]), _bits(old[own] + plain[own]))
    assert torch.equal(_bits(got[~own]), _bits(old[~own]))
    return int((~own)[:, :, : fine.lat.L[2]].sum())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_fold_modes_bitwise(Pf, Pc, nc, dt):
    rank_fold_modes(Comm(), nc, Pf, Pc, dt)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_fold_modes_bitwise_threaded_ranks(Pf, Pc, R):
    ghosts = run_threaded(R, rank_fold_modes, PARTITIONED, Pf, Pc, torch.float64)
    assert sum(ghosts) > 0          # some rank had ghost planes to leave alone


# ------------------------------------------- 3. agreement and adjointness
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nc", MESHES)
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_row_and_cell_transfers_agree(Pf, Pc, nc, dt):
    """Both are within EPS bnd of the exact operator, so within 2 EPS bnd of
    each other."""
    fine, coarse, k, latc, J = _pair(nc, Pf, Pc, dt)
    vc = _fill(coarse, _random(_shape(nc, Pc), 3, dt))
    row, bnd = check_prolong_row("cpu", nc, Pf, Pc, dt)
    cell = fine.new_vector()
    k.prolong(latc, J, vc, cell)
    assert (np.abs(_glob(fine, row) - _glob(fine, cell)) <= 2 * EPS[dt] * bnd).all()
    vf = _fill(fine, _random(_shape(nc, Pf), 5, dt))
    row, bnd = check_restrict_row("cpu", nc, Pf, Pc, dt, False)
    cell = coarse.new_vector()
    k.restrict(latc, J, vf, cell)
    assert (np.abs(_glob(coarse, row) - _glob(coarse, cell)) <= 2 * EPS[dt] * bnd).all()


def rank_adjoint_gap(comm, nc, Pf, dt, platform="cpu"):
    """tests/test_cpu_pmg.py::_adjoint_gap with the row transfers."""
    pmg = PMultigrid(_problem(nc, Pf, dt, comm=comm, platform=platform), p_transfer="row")
    Pc = pmg.degrees[1]
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    gu, gv = _random(_shape(nc, Pc), 11, dt), _random(_shape(nc, Pf), 13, dt)
    uc, vf = _fill(coarse, gu), _ghost_nan(fine, _fill(fine, gv))
    pu, rv = fine.new_vector(), coarse.new_vector()
    pmg.restrict(0, vf, rv)
    uc[:, :, : coarse.lat.L[2]][torch.from_numpy(coarse.lat.bc_mask()).to(uc.device)] = 0.0
    pmg.prolong(0, uc, pu)
    gap = fine.inner(pu, vf), coarse.inner(uc, rv), Pc, gu, gv
    pmg.close()
    return gap


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("Pf,Pc", PAIRS)
def test_row_adjointness_threaded_ranks(Pf, Pc, R):
    for a, b, pc, gu, gv in run_threaded(R, rank_adjoint_gap, PARTITIONED, Pf, torch.float64):
        bound = _adjoint_bound(PARTITIONED, Pf, Pc, gu, gv, torch.float64)
        assert pc == Pc and np.isfinite(a) and abs(a - b) <= bound, (a, b, bound)


def rank_restrict_row(comm, nc, Pf, platform="cpu"):
    """tests/test_cpu_pmg.py::_rank_restrict with the row transfers and y."""
    pmg = PMultigrid(_problem(nc, Pf, comm=comm, platform=platform), p_transfer="row")
    fine, coarse = pmg.levels[0].pb, pmg.levels[1].pb
    vf = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 17, torch.float64)))
    y = _ghost_nan(fine, _fill(fine, _random(_shape(nc, Pf), 19, torch.float64)))
    vc = coarse.new_vector()
    pmg.restrict(0, vf, vc, y)
    gi = coarse.lat.global_indices()
    out = _glob(coarse, vc), (gi, vc[:, :, : coarse.lat.L[2]].cpu().numpy().copy())
    pmg.close()
    return out


@pytest.mark.parametrize("Pf,Pc", [(3, 1), (4, 2), (6, 3)])
def test_restrict_row_partition_invariance(Pf, Pc):
    nc = PARTITIONED
    gf, gy = (_random(_shape(nc, Pf), s, torch.float64) for s in (17, 19))
    ref, _ = model_restrict(nc, Pf, Pc, gf - gy)
    _, bnd = model_restrict(nc, Pf, Pc, np.abs(gf) + np.abs(gy))
    ref[make_local_lattice(0, 1, nc, Pc).bc_mask()] = 0.0
    one = run_threaded(1, rank_restrict_row, nc, Pf)[0][0]
    assert (np.abs(one - ref) <= EPS[torch.float64] * bnd).all()
    for R in (2, 4):
        for got, (gi, loc) in run_threaded(R, rank_restrict_row, nc, Pf):
            assert (np.abs(got - one) <= EPS[torch.float64] * bnd).all()
            assert np.array_equal(loc, got.ravel()[gi])


# ------------------------------------------------------------ 4. PMultigrid
FOUR = {"degrees", "lambda_max", "smooth_degree", "coarse_degree"}


def _residual(pb, seed=3):
    return torch.randn(pb.lat.shape, dtype=pb.dtype,
                       generator=torch.Generator().manual_seed(seed)).masked_fill_(pb.bc_mask(), 0.0)


def test_default_is_bitwise_unchanged_and_option_is_checked():
    pb = _problem((4, 4, 4), 3, pert=0.2, coef="random")
    a, b, row = PMultigrid(pb), PMultigrid(pb, p_transfer="cell"), PMultigrid(pb, p_transfer="row")
    assert a.p_transfer == b.p_transfer == "cell" and row.p_transfer == "row"
    assert set(a.info()) == set(b.info()) == FOUR
    assert set(row.info()) == FOUR | {"p_transfer"} and row.info()["p_transfer"] == "row"
    assert a.lambda_max == b.lambda_max == row.lambda_max
    r = _residual(pb)
    za, zb = pb.new_vector(), pb.new_vector()
    a.apply(r, za)
    b.apply(r, zb)
    assert torch.equal(_bits(za), _bits(zb))
    assert _logged_apply(a, r) == _logged_apply(b, r)
    for bad in ("rows", "", None, 1, True):
        with pytest.raises(ValueError):
            PMultigrid(pb, p_transfer=bad)


def test_fold_arguments_refused_by_cell_and_accepted_by_row():
    pb = _problem((2, 3, 2), 4)
    cell, row = PMultigrid(pb), PMultigrid(pb, p_transfer="row")
    fine, coarse = cell.levels[0].pb, cell.levels[1].pb
    vf, vc, y = fine.new_vector(), coarse.new_vector(), fine.new_vector()
    with pytest.raises(ValueError, match="h-transfer's mode"):
        cell.prolong(0, vc, vf, True)
    with pytest.raises(ValueError, match="h-transfer's mode"):
        cell.restrict(0, vf, vc, y)
    row.prolong(0, vc, vf, True)
    row.restrict(0, vf, vc, y)


@pytest.mark.parametrize("P", [3, 6])
def test_a_p_pair_is_one_restriction_and_one_prolongation(P, monkeypatch):
    """Launch proxies: per p-pair exactly one restrict_row and one
    prolong_row, and no axpy, zero_, restrict or prolong anywhere."""
    pb = _problem((2, 3, 2), P)
    cell, row = PMultigrid(pb), PMultigrid(pb, p_transfer="row")
    zeroed = []
    real = torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, "zero_", lambda t: (zeroed.append(t.data_ptr()), real(t))[1])
    r = _residual(pb)
    pairs = len(row.degrees) - 1
    log = _logged_apply(row, r)
    coarse_r = {lv.r.data_ptr() for lv in row.levels[1:]}
    assert not coarse_r & set(zeroed)
    for l in range(pairs):
        assert log.count((l, "restrict_row")) == 1 and log.count((l, "prolong_row")) == 1
    names = [n for _, n in log]
    assert names.count("restrict_row") == names.count("prolong_row") == pairs
    assert not {"axpy", "restrict", "prolong"} & set(names)
    # the cell transfers: the sequence this replaces
    zeroed.clear()
    names = [n for _, n in _logged_apply(cell, r)]
    assert names.count("axpy") == 2 * pairs and names.count("restrict") == pairs
    assert names.count("prolong") == pairs and not {"restrict_row", "prolong_row"} & set(names)
    assert {lv.r.data_ptr() for lv in cell.levels[1:]} <= set(zeroed)
    # and everything else of the cycle is the same sequence
    drop = {"axpy", "restrict", "prolong", "restrict_row", "prolong_row"}
    assert [c for c in log if c[1] not in drop] == \
        [c for c in _logged_apply(cell, r) if c[1] not in drop]


def test_row_vcycle_symmetric_positive():
    """The bound of tests/test_cpu_pmg.py::test_vcycle_symmetric_positive."""
    pb = _problem((4, 4, 4), 3, pert=0.2, coef="random")
    pmg = PMultigrid(pb, p_transfer="row")
    a, b = _residual(pb, 5), _residual(pb, 6)
    a0 = a.clone()
    za, zb = pb.new_vector(), pb.new_vector()
    pmg.apply(a, za)
    pmg.apply(b, zb)
    assert torch.equal(a, a0)
    s1, s2 = pb.inner(za, b), pb.inner(a, zb)
    print(f"<M^-1 a, b> = {s1!r}, <a, M^-1 b> = {s2!r}, rel gap {abs(s1 - s2) / abs(s1):.3e}")
    assert abs(s1 - s2) <= 1e-12 * abs(s1)
    assert pb.inner(za, a) > 0 and pb.inner(zb, b) > 0


@pytest.mark.parametrize("P", [3, 4])
def test_row_pmg_pcg_vs_numpy(P):
    """tests/test_cpu_pmg.py::test_pmg_pcg_vs_numpy with the row transfers,
    its numpy PCG and its tolerance."""
    nc, pert, coef, its = (3, 3, 3), 0.2, "random", 6
    levels = _dense_levels(nc, P, pert, coef)
    for i, lv in enumerate(levels):
        last = i == len(levels) - 1
        lv["lam"] = _np_lambda(lv)
        lv["coef"] = chebyshev_coefficients(1.1 * lv["lam"], 100.0 if last else 10.0,
                                            8 if last else 2)
    A, b = levels[0]["A"], levels[0]["b"]
    x = np.zeros_like(b)
    r = b - A @ x
    z = _np_vcycle(levels, 0, r)
    p, rz = z.copy(), r @ z
    for _ in range(its):
        y = A @ p
        alpha = rz / (p @ y)
        x, r = x + alpha * p, r - alpha * y
        z = _np_vcycle(levels, 0, r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    pb = _problem(nc, P, pert=pert, coef=coef)
    pmg = PMultigrid(pb, p_transfer="row")
    xh = pb.new_vector()
    assert cg_solve(MatFreeLaplacianCPU(pb), pb, xh, pb.assemble_rhs(), its,
                    precond=pmg.apply) == its
    gap = np.abs(pb.to_global_array(xh) - x).max() / np.abs(x).max()
    print(f"row pmg-PCG vs numpy, Q{P}: max |dx| / max |x| = {gap:.3e}")
    assert gap <= 1e-10


@pytest.mark.parametrize("pert,coef", [(0.0, "constant"), (0.2, "random")])
@pytest.mark.parametrize("nc,P", [((6, 6, 6), 3), ((4, 4, 4), 6)])
def test_row_transfers_do_not_cost_iterations(nc, P, pert, coef):
    """Iterations to a relative residual of 1e-8: the same operator in another
    summation order, so within one iteration of the cell-transfer solve."""
    pb = _problem(nc, P, pert=pert, coef=coef)
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    kc, rc = _iterations(pb, op, b, precond=PMultigrid(pb).apply)
    kr, rr = _iterations(pb, op, b, precond=PMultigrid(pb, p_transfer="row").apply)
    print(f"{nc} Q{P} pert {pert} {coef}: cell {kc} its ({rc:.2e}), row {kr} its ({rr:.2e})")
    assert rr <= 1e-8 and rc <= 1e-8 and abs(kr - kc) <= 1


def test_row_transfers_with_h_levels_fp32_cycle_and_tail():
    """Q4 (levels 4, 2, 1 and one h-level), FP32 cycle under FP64 CG, the
    h-levels in the one-call tail: the row option changes the iteration
    count by at most one and the JSON block gains its key only."""
    pb = _problem((5, 4, 7), 4, pert=0.2, coef="random")
    op, b = MatFreeLaplacianCPU(pb), pb.assemble_rhs()
    kw = dict(h_levels=-1, cycle_dtype=torch.float32, tail_nodes=600)
    cell, row = PMultigrid(pb, **kw), PMultigrid(pb, p_transfer="row", **kw)
    assert row.mixed and row.h_levels == 1 and row.tail_levels >= 1
    assert set(row.info()) == set(cell.info()) | {"p_transfer"}
    names = [n for _, n in _logged_apply(row, _residual(pb))]
    assert names.count("restrict_row") == names.count("prolong_row") == 2
    assert names.count("pmg_tail") == 1 and "axpy" not in names
    kc, rc = _iterations(pb, op, b, precond=cell.apply)
    kr, rr = _iterations(pb, op, b, precond=row.apply)
    print(f"combined: cell {kc} its ({rc:.2e}), row {kr} its ({rr:.2e})")
    assert rr <= 1e-8 and rc <= 1e-8 and abs(kr - kc) <= 1


ITS = 6


def rank_row_solve(comm, nc, P, transfer, platform="cpu"):
    pb = _problem(nc, P, pert=0.2, coef="random", comm=comm, platform=platform)
    pmg = PMultigrid(pb, p_transfer=transfer)
    x = pb.new_vector()
    cg_solve(MatFreeLaplacianCPU(pb), pb, x, pb.assemble_rhs(), ITS, precond=pmg.apply)
    pmg.close()
    return pb.to_global_array(x)


@pytest.mark.parametrize("P", [3, 4])
def test_row_solve_on_threaded_ranks(P):
    """ITS iterations on 1, 2 and 4 ranks against the one-rank cell-transfer
    solve, with the tolerance of test_row_pmg_pcg_vs_numpy: the partition and
    the transfer kernels change summation orders only."""
    ref = run_threaded(1, rank_row_solve, PARTITIONED, P, "cell")[0]
    for R in (1, 2, 4):
        for x in run_threaded(R, rank_row_solve, PARTITIONED, P, "row"):
            gap = np.abs(x - ref).max() / np.abs(ref).max()
            print(f"Q{P}, {R} ranks: gap to the one-rank cell solve {gap:.3e}")
            assert gap <= 1e-10


# ------------------------------------------------------------------ 5. CLI
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    return env


CLI = ["-m", "benchmark_dolfinx_amd", "--platform", "cpu", "--ndofs_global", "1000", "--degree",
       "3", "--cg", "--nreps", "10", "--mat_comp", "--precond", "pmg"]


def _cli(launch, extra, js):
    r = subprocess.run([*launch, *CLI, *extra, "--json", str(js)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(js))


def check_cg_output(d):
    """utils.check_output.check without its golden y_norm, which is the
    operator action's and not a CG iterate's: the size, and the matrix-free
    solve against the CSR solve."""
    out = d["output"]
    assert out["ndofs_global"] == 1000
    assert np.isclose(out["y_norm"], out["z_norm"])
    rel = d["mi355x"]["e_norm"] / out["z_norm"]
    print(f"matrix-free row pmg-PCG vs CSR row pmg-PCG: relative error norm {rel:.3e}")
    assert rel < 1e-10


def test_cli_pmg_transfer_row(tmp_path):
    d = _cli([sys.executable], ["--pmg_transfer", "row"], tmp_path / "r.json")
    blk = d["mi355x"]["pmg"]
    assert set(blk) == FOUR | {"p_transfer"} and blk["p_transfer"] == "row"
    check_cg_output(d)
    for extra in ([], ["--pmg_transfer", "cell"]):
        d0 = _cli([sys.executable], extra, tmp_path / "c.json")
        assert set(d0["mi355x"]["pmg"]) == FOUR
    d2 = _cli([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr=127.0.0.1", "--master-port=29671"],
              ["--pmg_transfer", "row"], tmp_path / "r2.json")
    assert d2["input"]["mpi_size"] == 2 and d2["mi355x"]["pmg"]["p_transfer"] == "row"
    check_cg_output(d2)
    y1, y2 = d["output"]["y_norm"], d2["output"]["y_norm"]
    print(f"y_norm 1 process {y1!r}, 2 processes {y2!r}")
    assert abs(y1 - y2) <= 1e-12 * abs(y1)


@pytest.mark.parametrize("args", [
    ["--pmg_transfer", "row"],
    ["--cg", "--pmg_transfer", "row"],
    ["--cg", "--precond", "jacobi", "--pmg_transfer", "row"],
    ["--cg", "--precond", "pmg", "--pmg_transfer", "rows"],
])
def test_cli_pmg_transfer_refusals(args):
    r = subprocess.run([sys.executable, "-m", "benchmark_dolfinx_amd", "--platform", "cpu", *args],
                       cwd=ROOT, env=_env(), capture_output=True, text=True)
    assert r.returncode != 0 and "pmg_transfer" in (r.stdout + r.stderr)
