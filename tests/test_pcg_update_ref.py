"""Self-checks of tests/pcg_update_ref.py (no GPU): the reference of the
preconditioned update pass against its definition, node by node and vector by
vector."""

import numpy as np
import pytest

import pcg_update_ref as pr
import vector_ref as vr

SHAPES = [
    # P, tile (cells), n, gh: the shapes of tests/test_gpu_pcg_update_kernels.py
    (3, (4, 4), (3, 5, 6), (0, 0, 0)),
    (3, (4, 4), (2, 8, 8), (1, 1, 1)),
    (5, (2, 2), (2, 3, 5), (0, 1, 0)),
    (4, (2, 4), (3, 3, 9), (1, 0, 1)),
    (7, (2, 2), (2, 2, 3), (0, 0, 0)),
    (6, (2, 2), (2, 5, 4), (0, 0, 1)),
]


def _inputs(g, seed, T=np.float64):
    rng = np.random.default_rng(seed)
    r, y = (rng.standard_normal(g.L).astype(T) for _ in range(2))
    ifc = [rng.standard_normal(s).astype(T) for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    dinv = rng.uniform(0.5, 2.0, g.L).astype(T)
    return r, y, ifc, dinv


@pytest.mark.parametrize("P,tile,n,gh", SHAPES)
def test_update_matches_the_naive_loop(P, tile, n, gh):
    g = vr.Geom(P, tile, n, gh)
    r, y, ifc, dinv = _inputs(g, 5)
    alpha = vr.coefficient([0.8125, 0.0, 1.37], 0, 2, np.float64)
    rn, z, mag = pr.update(r, y, *ifc, dinv, alpha, g)
    rn0, z0 = pr.update_naive(r, y, *ifc, dinv, alpha, g)
    eps = np.finfo(np.float64).eps
    # three adds of the fold in either order, the product, the subtraction
    tol = 4 * eps * (np.abs(r) + abs(alpha) * mag)
    assert np.all(np.abs(rn - rn0) <= tol)
    assert np.all(np.abs(z - z0) <= dinv * tol + 2 * eps * np.abs(z0))
    # z of the stored r is one multiply: identical bits by either route
    assert np.array_equal(pr.z_of(dinv, rn0), z0)
    # interface nodes, and only those, see the fold
    my, mz = g.iface_masks()
    plain = r - alpha * y
    assert np.array_equal(rn != plain, (my | mz) & (rn != plain))
    assert (my | mz).sum() == 0 or np.any(rn != plain)


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_z_and_scalar_terms_keep_the_storage_type(T):
    g = vr.Geom(3, (4, 4), (3, 5, 6))
    r, _, _, dinv = _inputs(g, 6, T)
    z = pr.z_of(dinv, r)
    assert z.dtype == T
    # against the exact product (float32: exact in float64; float64: within
    # half a unit in the last place of the extended-precision product)
    if T == np.float32:
        assert np.array_equal(z, (dinv.astype(np.float64) * r.astype(np.float64)).astype(T))
    else:
        hi = dinv.astype(np.longdouble) * r.astype(np.longdouble)
        assert np.all(np.abs(z.astype(np.longdouble) - hi) <= 0.5 * np.spacing(np.abs(z)) * (1 + 2.0 ** -10))
    rz, rr = pr.scalar_terms(r, z)
    assert rz.dtype == rr.dtype == np.float64
    i = (1, 2, 3)
    assert rz[i] == float(r[i]) * float(z[i]) and rr[i] == float(r[i]) ** 2
    assert np.all(rr >= 0) and np.all(rz >= 0)       # dinv > 0
    with pytest.raises(AssertionError):
        pr.z_of(dinv.astype(np.float64), r.astype(np.float32))


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("tiled", [False, True], ids=["lattice", "tiled"])
@pytest.mark.parametrize("P,tile,n,gh", SHAPES)
def test_stored_elements_match_the_vector_loop(P, tile, n, gh, tiled, W):
    g = vr.Geom(P, tile, n, gh)
    assert (g.tsy * g.tsz) % W == 0     # no vector straddles two tile planes
    got = pr.stored_elements(g, tiled, W)
    assert np.array_equal(got, pr.stored_elements_naive(g, tiled, W))
    # whole vectors; every owned node lies in one; with ghost planes or
    # padding some storage is left alone
    assert np.array_equal(got.reshape(-1, W).all(axis=1), got.reshape(-1, W).any(axis=1))
    assert got[g.map(tiled)[g.owned_mask()]].all()
    if gh[0] or gh[1] or (tiled and gh[2]):   # the flat pass streams whole rows
        assert not got.all()
    if not tiled:   # the flat pass also stores the pad columns of the owned rows
        assert got.sum() == g.own[0] * g.own[1] * g.ld
