"""Self-checks of tests/vector_ref.py (no GPU): the references the vector
kernel tests rely on are themselves checked against their definitions."""

import numpy as np
import pytest

import vector_ref as vr

SHAPES = [
    # P, tile (cells), n, gh
    (3, (4, 4), (3, 5, 6), (0, 0, 0)),
    (3, (4, 4), (2, 8, 8), (1, 1, 1)),
    (5, (2, 2), (2, 3, 5), (0, 1, 0)),
    (4, (2, 4), (3, 3, 9), (1, 0, 1)),
    (7, (2, 2), (2, 2, 3), (0, 0, 0)),
    (3, (4, 4), (1, 1, 1), (0, 0, 0)),
    (3, (2, 5), (2, 5, 11), (0, 0, 0)),
]


@pytest.mark.parametrize("P,tile,n,gh", SHAPES)
def test_tiled_map_is_a_bijection_onto_storage_minus_padding(P, tile, n, gh):
    g = vr.Geom(P, tile, n, gh)
    m = g.map(True).ravel()
    assert m.min() >= 0 and m.max() < g.til_size
    assert np.unique(m).size == m.size == np.prod(g.L)
    # the storage positions that hold no node are exactly the padding: local
    # coordinates of the last tile row / column beyond L1 / L2
    hit = np.zeros(g.til_size, dtype=bool)
    hit[m] = True
    pos = np.arange(g.til_size)
    tile_i, rest = pos // (g.L[0] * g.tsy * g.tsz), pos % (g.L[0] * g.tsy * g.tsz)
    ty, tz = tile_i // g.tntz, tile_i % g.tntz
    ly, lz = (rest // g.tsz) % g.tsy, rest % g.tsz
    valid = (ty * g.tsy + ly < g.L[1]) & (tz * g.tsz + lz < g.L[2])
    assert np.array_equal(hit, valid)
    # and the descriptor agrees with the map's parameters
    d = g.latd_tiled
    assert tuple(d[17:21]) == (g.tsy, g.tsz, g.tntz, g.L[0] * g.tsy * g.tsz)
    assert g.til_size == g.tnty * g.tntz * d[20]


@pytest.mark.parametrize("P,tile,n,gh", SHAPES)
def test_lattice_map_is_injective_and_skips_the_pad_columns(P, tile, n, gh):
    g = vr.Geom(P, tile, n, gh)
    m = g.map(False).ravel()
    assert np.unique(m).size == m.size and m.max() < g.lat_size
    assert np.all(m % g.ld < g.L[2])


@pytest.mark.parametrize("P,tile,n,gh", SHAPES)
def test_fold_matches_the_naive_loop(P, tile, n, gh):
    g = vr.Geom(P, tile, n, gh)
    rng = np.random.default_rng(3)
    y = rng.standard_normal(g.L)
    yb = rng.standard_normal(g.yb_shape)
    zb = rng.standard_normal(g.zb_shape)
    cb = rng.standard_normal(g.cb_shape)
    f, mag = vr.fold(y, yb, zb, cb, g)
    naive = vr.fold_naive(y, yb, zb, cb, g)
    # at most three additions in either order
    assert np.all(np.abs(f - naive) <= 4 * np.finfo(np.float64).eps * mag)
    naive_mag = vr.fold_naive(np.abs(y), np.abs(yb), np.abs(zb), np.abs(cb), g)
    assert np.all(np.abs(mag - naive_mag) <= 4 * np.finfo(np.float64).eps * naive_mag)
    my, mz = g.iface_masks()
    assert np.array_equal(f != y, (my | mz) & (f != y))   # only interface nodes change
    assert (my | mz).sum() == 0 or np.any(f != y)
    # interface entries belong to owned nodes exactly where the node is owned
    own = g.owned_mask()
    oyb, ozb, ocb = g.iface_owned()
    cnt = vr.iface_sum(np.zeros(g.L), oyb * 1.0, ozb * 1.0, ocb * 1.0, g)
    ref = my * 1.0 + mz * 1.0 + (my & mz) * 1.0
    assert np.array_equal(cnt, ref * own)


def test_fold_on_torch_tensors_matches_numpy():
    import torch
    g = vr.Geom(3, (4, 4), (2, 8, 8), (1, 1, 1))
    rng = np.random.default_rng(4)
    arrs = [rng.standard_normal(s) for s in (g.L, g.yb_shape, g.zb_shape, g.cb_shape)]
    f, mag = vr.fold(*arrs, g)
    ft, magt = vr.fold(*[torch.from_numpy(a) for a in arrs], g)
    assert np.array_equal(ft.numpy(), f) and np.array_equal(magt.numpy(), mag)


def test_chain_lengths():
    assert vr.chain_block(3) == 13
    assert vr.chain_final(1) == 11 and vr.chain_final(257) == 12
    assert vr.chain_final(1024, 1024) == 14
    # 2231 partials: 256 slices of 9 (one add per thread), then one block of 256
    assert vr.chain_final(2231, 1024) == 11 + 11


def test_lattice_builder_and_coefficient():
    lat = vr.make_lattice(3, (2, 3, 4), (1, 0, 1))
    assert lat.L == (7, 10, 13) and lat.owned_hi == (6, 10, 12) and lat.halo_send_boxes() == []
    lo = vr.make_lattice(3, (2, 3, 4), (1, 0, 1), lower=True)
    assert lo.gh == (1, 0, 1) and len(lo.halo_send_boxes()) == 7 and len(lo.halo_recv_boxes()) == 3
    assert vr.coefficient([3.0, 7.0], 0, 1, np.float32) == np.float32(3.0 / 7.0)
    assert vr.coefficient([3.0, 7.0], 0, -1, np.float64) == 3.0
    assert vr.sum_hi(np.array([1e16, 1.0, -1e16])) == 1.0
