#!/usr/bin/env python
"""Record the bits the multigrid host twins (csrc/host/bdx_host_mg.cpp) produce
on fixed inputs: tests/golden/mg_host_bits.npz, which
tests/test_cpu_mg_host_bits.py compares with `tobytes()`.

    python scripts/record_mg_host_bits.py            # rewrite the fixture
    python scripts/record_mg_host_bits.py --check    # compare, exit 1 on a difference

The fixture was recorded before the per-node bodies moved to
csrc/include/bdx_mg_bodies.h; record it again only when a change of the
results is intended.  The host build has neither FMA contraction nor fast-math,
so the bits do not depend on the compiler's version.

Every input is `fem.mesh._hash_uniform` of the storage index (mapped to
[-1, 1)), so no generator's stream is involved; the storage padding holds NaN,
and so do the ghost planes of a restriction's fine vector.  Cases, each in
FP64 and FP32 (`cases()` yields them in this order):
  hprolong   the pairs (5, 4, 7) -> (2, 2, 3) and (3, 1, 70) -> (3, 1, 35) of
             tests/test_cpu_hpmg.py, ghost planes off / on, add 0 / 1
  hrestrict  the same pairs, ghost planes off / on, y null / given
  cheb       the (5, 4, 7) lattice with ghost planes (the owned box is smaller
             than the lattice), first 0 / 1: d and z
  stencil27  every tail level of meshes a and d of tests/test_cpu_pmg_tail.py,
             perturbation 0.2, random kappa
  tail       `bdx_cpu_pmg_tail`'s z: cases a, c, d through `PMultigrid.apply`,
             case b600 called on its first tail level, each on the box and
             perturbed with random kappa
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_dolfinx_amd.fem.mesh import (LocalLattice, _hash_uniform,  # noqa: E402
                                            coarsened_lattice, make_local_lattice)
from benchmark_dolfinx_amd.models.poisson import PoissonProblem  # noqa: E402
from benchmark_dolfinx_amd.ops.kernels import HostKernels, HTransferTables  # noqa: E402
from benchmark_dolfinx_amd.parallel.comm import Comm  # noqa: E402
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "mg_host_bits.npz")
DTYPES = {"f64": torch.float64, "f32": torch.float32}
NAN = float("nan")
PAIRS = [(5, 4, 7), (3, 1, 70)]
# name: cells, degree, tail_nodes (tests/test_cpu_pmg_tail.py: CASES)
TAIL = {"a": ((6, 5, 9), 1, 1024), "b600": ((13, 15, 17), 1, 600), "c": ((6, 5, 9), 3, 1024),
        "d": ((4, 4, 4), 1, 1024)}
GEOM = {"box": (0.0, "constant"), "pert": (0.2, "random")}


def hashed(lat, seed, dt, ghost_nan=False):
    """Lattice vector 2 hash(storage index) - 1, NaN in the storage padding
    (and, with `ghost_nan`, on the ghost planes)."""
    n = int(np.prod(lat.shape))
    v = (2.0 * _hash_uniform(np.arange(n), seed) - 1.0).reshape(lat.shape)
    v[:, :, lat.L[2]:] = NAN
    if ghost_nan:
        o = lat.owned_hi
        v[o[0]:], v[:, o[1]:], v[:, :, o[2]:] = NAN, NAN, NAN
    return torch.from_numpy(v).to(dt)


def pair(n, ghosts):
    """tests/test_cpu_hpmg.py: _pair."""
    if not ghosts:
        lf = make_local_lattice(0, 1, n, 1)
    elif n == (5, 4, 7):
        lf = LocalLattice(0, 8, 1, (10, 8, 14), (2, 2, 2), (0, 0, 0), (0, 0, 0), n)
    else:
        lf = LocalLattice(0, 2, 1, (3, 1, 140), (1, 1, 2), (0, 0, 0), (0, 0, 0), n)
    lc, fpos = coarsened_lattice(lf)
    return lf, lc, fpos


def transfer_cases(sn, dt):
    for n in PAIRS:
        for ghosts in (0, 1):
            lf, lc, fpos = pair(n, bool(ghosts))
            tab = HTransferTables(fpos, dt, torch.device("cpu"))
            k = HostKernels(lf, dt)
            tag = f"{'x'.join(map(str, n))}_g{ghosts}_{sn}"
            vc = hashed(lc, 3, dt)
            for add in (0, 1):
                vf = hashed(lf, 4, dt) if add else torch.full(lf.shape, NAN, dtype=dt)
                k.hprolong(lc.as_int64(), tab, vc, vf, bool(add))
                yield f"hprolong_{tag}_add{add}", vf
            vf = hashed(lf, 5, dt, ghost_nan=bool(ghosts))
            for name, y in (("ynull", None), ("y", hashed(lf, 6, dt, ghost_nan=bool(ghosts)))):
                out = torch.full(lc.shape, NAN, dtype=dt)
                k.hrestrict(lc.as_int64(), tab, vf, y, out)
                yield f"hrestrict_{tag}_{name}", out


def cheb_cases(sn, dt):
    lat = pair((5, 4, 7), True)[0]
    assert tuple(lat.owned_hi) != tuple(lat.L)
    k = HostKernels(lat, dt)
    dinv, r, y = (hashed(lat, s, dt) for s in (7, 8, 9))
    for first in (0, 1):
        d, z = hashed(lat, 10, dt), hashed(lat, 11, dt)
        k.cheb_step(bool(first), 0.37, 1.21, dinv, r, None if first else y, d, z)
        yield f"cheb_first{first}_{sn}_d", d
        yield f"cheb_first{first}_{sn}_z", z


def tailed(name, geom, dt):
    nc, P, N = TAIL[name]
    pert, coef = GEOM[geom]
    pb = PoissonProblem(Comm(), nc, P, 1, False, dt, "cpu", pert, coef)
    pmg = PMultigrid(pb, h_levels=-1, tail_nodes=N)
    assert pmg.tail is not None and pmg.tail_levels == 2
    return pb, pmg


def residual(pb, seed):
    r = hashed(pb.lat, seed, pb.dtype)
    r.masked_fill_(pb.bc_mask() & ~torch.isnan(r), 0.0)
    return r


def stencil_cases(sn, dt):
    for name in ("a", "d"):
        _, pmg = tailed(name, "pert", dt)
        for l in range(pmg.tail_start, len(pmg.levels)):
            lv = pmg.levels[l]
            ys = torch.full(lv.pb.lat.shape, NAN, dtype=dt)
            lv.k.stencil27(pmg.tail.S[l - pmg.tail_start], hashed(lv.pb.lat, 12, dt), ys)
            yield f"stencil27_{name}_l{l}_{sn}", ys


def tail_cases(sn, dt):
    for name in TAIL:
        for geom in GEOM:
            pb, pmg = tailed(name, geom, dt)
            first = pmg.levels[pmg.tail_start]
            if name == "b600":      # the tail called on its first level alone
                assert pmg.tail_start == 1
                zt = torch.full(first.pb.lat.shape, NAN, dtype=dt)
                first.k.pmg_tail(pmg.tail, residual(first.pb, 13), zt)
            else:                   # the tail's own output inside a whole cycle
                seen, real = [], first.k.pmg_tail

                def spy(tail, r, z):
                    real(tail, r, z)
                    seen.append(z.clone())
                first.k.pmg_tail = spy
                pmg.apply(residual(pb, 14), torch.full(pb.lat.shape, NAN, dtype=dt))
                del first.k.pmg_tail
                (zt,) = seen
            yield f"tail_{name}_{geom}_{sn}", zt


def cases():
    """(key, raw output array) of every case."""
    for sn, dt in DTYPES.items():
        for gen in (transfer_cases, cheb_cases, stencil_cases, tail_cases):
            for key, t in gen(sn, dt):
                yield key, t.contiguous().numpy().copy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the fixture, write nothing")
    a = ap.parse_args(argv)
    got = dict(cases())
    if a.check:
        want = np.load(FIXTURE)
        bad = [k for k in sorted(set(got) | set(want.files))
               if k not in got or k not in want.files or got[k].dtype != want[k].dtype
               or got[k].tobytes() != want[k].tobytes()]
        print(f"{len(got)} cases, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
        return 1 if bad else 0
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    np.savez_compressed(FIXTURE, **got)
    print(f"wrote {len(got)} arrays, {os.path.getsize(FIXTURE)} bytes: {FIXTURE}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
