"""Entry-by-entry reference of k CG iterations (CPU only), shared by
tests/test_cg_ref.py and tests/test_gpu_partitioned_cg.py.

A case is one global problem of tests/operator_ref.py.  Its right-hand side b
and start x0 are random (standard normal, rounded to the vector dtype, exactly
zero on the Dirichlet dofs), so every entry of the iterate is O(1) and an error
anywhere counts: nothing hides in the tail of a narrow source term.  The
reference is `cg_solve` (rtol = 0) in FP64 on one rank over
`MatFreeLaplacianCPU`, plain or Jacobi-preconditioned with the host diagonal.

The error of an iterate is measured per entry against the same recurrence run
on magnitudes, the running first-order bound on what rounding can do to each
entry.  With |A| v from `operator_ref.abs_action`, D = |dinv| (1 when
unpreconditioned) and the reference run's own alpha_j, beta_j:

    t_0 = |b| + |A| |x0|      q_0 = D t_0                 s_0 = |x0|
    s_{j+1} = s_j + |alpha_j| q_j
    t_{j+1} = t_j + |alpha_j| |A| q_j
    q_{j+1} = D t_{j+1} + |beta_j| q_j

entry ratio  max_i |x_i - x_k,i| / (eps_T s_k,i) over the non-Dirichlet entries
(the Dirichlet ones have to be x0's zeros exactly), scalar ratio
|rr - r_k.r_k| / (eps_T sum_i |r_k,i| t_k,i) for the plain r.r that
`DeviceCG.residual_norm2()` reports.

The scale grows with k (median s_k / |x_k| about 5 at k = 1, 35 to 100 at
k = 3, 400 to 3000 at k = 5), so the iteration counts stay small: 3 and 4.  CG
on a case needs far more free dofs than iterations; a case with fewer than
8 k non-Dirichlet dofs is refused.
"""

import functools
from typing import NamedTuple

import numpy as np
import torch

import operator_ref as oref
from operator_ref import (EPS, K_CAP, K_CPU, LAYOUTS, MESHES, SHEAR_MESH, Case,  # noqa: F401
                          _host, _ijk, local_input)
from benchmark_dolfinx_amd.fem.mesh import make_local_lattice
from benchmark_dolfinx_amd.solvers.cg import cg_solve

SEED_B, SEED_X0 = 5, 6
# free dofs a case needs per iteration
FREE_PER_ITERATION = 8


class Ref(NamedTuple):
    b: np.ndarray        # global right-hand side, rounded to the vector dtype
    x0: np.ndarray       # global start
    x: np.ndarray        # x_k of the FP64 one-rank recurrence
    rr: float            # plain r_k . r_k
    s: np.ndarray        # entry scale s_k
    rr_scale: float      # sum_i |r_k,i| t_k,i
    free: np.ndarray     # non-Dirichlet entries (bool)
    alpha: tuple
    beta: tuple


@functools.lru_cache(maxsize=None)
def free_mask(case):
    """Non-Dirichlet entries of the global lattice (bool, flat)."""
    one = make_local_lattice(0, 1, case.nc, case.P)
    free = ~one.bc_mask().ravel()
    free.setflags(write=False)
    return free


def allowed(case, k):
    """CG with k iterations on `case`: at least 8 k free dofs."""
    return int(free_mask(case).sum()) >= FREE_PER_ITERATION * k


class _Recorder:
    """The problem as `cg_solve` sees it (new_vector, inner), keeping the
    vectors it creates (r, y, z in that order) and every inner product."""

    def __init__(self, pb):
        self.pb, self.vectors, self.inners = pb, [], []

    def new_vector(self):
        self.vectors.append(self.pb.new_vector())
        return self.vectors[-1]

    def inner(self, a, b):
        self.inners.append(self.pb.inner(a, b))
        return self.inners[-1]


def _to_store(cpu, vg):
    v = cpu.new_vector()
    v[:, :, : cpu.lat.L[2]] = torch.from_numpy(np.asarray(vg).reshape(cpu.lat.L))
    return v


@functools.lru_cache(maxsize=None)
def host_dinv(case):
    """1 / diag(A) of the host problem as a global array (1 on Dirichlet dofs)."""
    cpu = _host(case)[0]
    d = cpu.to_global_array(cpu.jacobi_inverse())
    d.setflags(write=False)
    return d


def inputs(case, dt):
    """(b, x0): global, rounded to dt, zero on the Dirichlet dofs."""
    free = free_mask(case)
    out = []
    for seed in (SEED_B, SEED_X0):
        v = np.random.default_rng(seed).standard_normal(free.size)
        v = torch.from_numpy(v).to(dt).double().numpy()
        out.append(np.where(free, v, 0.0))
    return out


@functools.lru_cache(maxsize=None)
def reference(case, dt, k, jacobi=False):
    """Ref of k iterations on `case` for vectors of dtype `dt` (read-only, shared)."""
    free = free_mask(case)
    if not allowed(case, k):
        raise ValueError(f"{int(free.sum())} free dofs are fewer than {FREE_PER_ITERATION} x "
                         f"{k} iterations: {case}")
    cpu, op = _host(case)
    bg, x0g = inputs(case, dt)
    rec = _Recorder(cpu)
    x = _to_store(cpu, x0g)
    dinv = cpu.jacobi_inverse() if jacobi else None
    assert cg_solve(op, rec, x, _to_store(cpu, bg), k, dinv=dinv) == k
    # inner products of cg_solve at rtol = 0: r0.z0, then (p.Ap, r.z) per iteration
    assert len(rec.inners) == 1 + 2 * k
    rz = rec.inners[0::2]
    alpha = tuple(rz[j] / rec.inners[1 + 2 * j] for j in range(k))
    beta = tuple(rz[j + 1] / rz[j] for j in range(k))
    r = cpu.to_global_array(rec.vectors[0])
    D = np.abs(host_dinv(case)) if jacobi else 1.0
    t = np.abs(bg) + oref.abs_action(case, np.abs(x0g))
    q = D * t
    s = np.abs(x0g)
    for a, b in zip(alpha, beta):
        s = s + abs(a) * q
        t = t + abs(a) * oref.abs_action(case, q)
        q = D * t + abs(b) * q
    assert (s[free] > 0).all() and (t[~free] == 0).all() and (r[~free] == 0).all()
    out = Ref(bg, x0g, cpu.to_global_array(x), float(r @ r), s, float(np.abs(r) @ t), free,
              alpha, beta)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def local_vectors(pb, ref):
    """(b, x0) of rank `pb`: the owned box from the global arrays, NaN on every
    ghost plane and in the storage padding (`operator_ref.local_input`)."""
    return local_input(pb, ref.b), local_input(pb, ref.x0)


def ratio(got_global, case, dt, k, jacobi=False):
    """max_i |got_i - x_k,i| / (eps_T s_k,i) over the non-Dirichlet entries."""
    ref = reference(case, dt, k, jacobi)
    f = ref.free
    return float((np.abs(np.asarray(got_global) - ref.x)[f] / (EPS[dt] * ref.s[f])).max())


def rr_ratio(rr, case, dt, k, jacobi=False):
    """|rr - r_k.r_k| / (eps_T sum_i |r_k,i| t_k,i)."""
    ref = reference(case, dt, k, jacobi)
    return abs(float(rr) - ref.rr) / (EPS[dt] * ref.rr_scale)


def check(got_global, case, dt, k, K, jacobi=False, rr=None):
    """Every entry finite, the Dirichlet entries exactly x0's zeros, every
    other entry within K eps_T s_k,i of the reference and, if `rr` is given,
    the scalar within K eps_T of its scale; returns (entry ratio, scalar
    ratio or None)."""
    got = np.asarray(got_global, dtype=np.float64)
    ref = reference(case, dt, k, jacobi)
    N = tuple(n * case.P + 1 for n in case.nc)
    what = f"{case} {dt} k = {k}{' jacobi' if jacobi else ''}"
    bad = np.flatnonzero(~np.isfinite(got))
    assert bad.size == 0, (f"{bad.size} non-finite entries, first at global index {bad[0]} "
                           f"(i, j, k) = {_ijk(bad[0], N)}: {what}")
    bad = np.flatnonzero(~ref.free & (got != 0))
    assert bad.size == 0, (f"{bad.size} Dirichlet entries moved, first at global index {bad[0]} "
                           f"(i, j, k) = {_ijk(bad[0], N)}: got {float(got[bad[0]])!r}: {what}")
    r = np.where(ref.free, np.abs(got - ref.x) / (EPS[dt] * np.where(ref.free, ref.s, 1.0)), 0.0)
    w = int(np.argmax(r))
    assert r[w] <= K, (f"ratio {r[w]:.3e} > K = {K} at global index {w} (i, j, k) = "
                       f"{_ijk(w, N)}: got {float(got[w])!r}, reference {float(ref.x[w])!r}, "
                       f"scale s_k {float(ref.s[w])!r}: {what}")
    rs = None
    if rr is not None:
        assert np.isfinite(rr), f"r.r = {rr!r}: {what}"
        rs = rr_ratio(rr, case, dt, k, jacobi)
        assert rs <= K, (f"scalar ratio {rs:.3e} > K = {K}: r.r got {float(rr)!r}, reference "
                         f"{ref.rr!r}, scale {ref.rr_scale!r}: {what}")
    return float(r[w]), rs
