"""The CG runtime's vector kernels, each driven directly through its C entry
point with hand-built lattice descriptors and compared per node with the
plain references of tests/vector_ref.py.

Common to every case:

* inputs are seeded random; every element a kernel must not use is NaN (ghost
  planes where only owned nodes are read, lattice pad columns, tiled padding),
  and every checked output and reduction must be finite;
* every output element outside the kernel's write set must keep its bits;
* per-element tolerance |out - ref| <= 4 eps_T sum|terms| (at most 8 unit
  roundoffs: three adds of the fold, the product, the subtraction, fused or
  not); references are evaluated in np.longdouble; copies are bitwise;
* reductions are compared with math.fsum of the terms, within
  (chain + 3) 2^-53 relative, where `chain` is the longest chain of float64
  additions behind the result (vector_ref.chain_*: a thread's serial adds, 6
  wave steps, 4 wave sums, then the final pass over the block partials) and
  the 3 covers the rounding of the term itself in the kernel and in the
  reference and the second-order part.  The chains that occur here:
    interface-fold update, shapes A1-A8: one block pass per vector chunk,
      2 U W = 4 (FP64) or 8 (FP32) adds per thread + 10, final ceil(g/256) + 10:
      chain <= 8 + 10 + 1 + 10 = 29          -> 3.6e-15
    A9 (two-stage, g = 2231 / 1164 / 2306 / 1153): 8 + 10, slices 1 + 10,
      final 1 + 10: chain <= 40              -> 4.8e-15
    A10 (grid-stride, 2 passes): 16 + 10 + 11 + 11 = 48; its reference sums
      4096-term rows on the device first (+ 4096)   -> 4.6e-13
    dot / cg_update rows: ceil(rows / (4 g)) ceil(o2 / 64) adds per thread
      (<= 2 * 3 = 6) + 10, final ceil(g / 256) + 10 <= 18: chain <= 34 -> 4.1e-15
    reduce_partials(n): ceil(n / 256) + 10 <= 266   -> 3.0e-14
  All are below the flat 1e-12 the older FP64 tests use.
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import kernel_harness as kh
import vector_ref as vr
from benchmark_dolfinx_amd.ops.native import ptr
from kernel_harness import (assert_same_bits, dev, fn, geom, host, iface_flat, lib,
                            new_partials, store, stream)
from benchmark_dolfinx_amd.parallel.halo import _Side

pytestmark = pytest.mark.gpu

HI = np.longdouble
NAN = float("nan")
TYPES = {"f64": (np.float64, torch.float64), "f32": (np.float32, torch.float32)}
RN, PAP, OUT, XS = 0, 2, 5, 3        # scalar slots used by the calls
SCAL = {RN: 0.8125, PAP: 1.37, XS: -0.4375, 6: 2.25}
TWO_STAGE = 1024                      # 4 * kStage1 (cg_update.hip)
scalars = functools.partial(kh.scalars, SCAL)

# P, kernel tile (cells), local cells, ghost planes
A_SHAPES = {
    "A1": (3, (4, 4), (3, 5, 6), (0, 0, 0)),
    "A2": (3, (4, 4), (2, 8, 8), (1, 1, 1)),
    "A2o": (3, (4, 4), (2, 8, 8), (0, 0, 0)),    # the same with the last plane owned
    "A3": (5, (2, 2), (2, 3, 5), (0, 1, 0)),
    "A4": (4, (2, 4), (3, 3, 9), (1, 0, 1)),
    "A5": (7, (2, 2), (2, 2, 3), (0, 0, 0)),
    "A6": (6, (2, 2), (2, 5, 4), (0, 0, 1)),
    "A7a": (3, (4, 4), (2, 3, 4), (0, 0, 0)),
    "A7b": (3, (4, 4), (1, 1, 1), (0, 0, 0)),
    "A8": (3, (2, 5), (2, 5, 11), (0, 0, 0)),
    "A9": (3, (4, 4), (32, 48, 48), (0, 0, 0)),
}
B_SHAPES = {
    "B1": (5, (2, 2), (2, 3, 33)),
    "B2": (3, (4, 4), (3, 4, 61)),
    "B3": (3, (4, 4), (2, 5, 64)),
    "B4a": (3, (4, 4), (3, 5, 6)),
    "B4b": (7, (2, 2), (2, 3, 3)),
    "B4c": (4, (2, 4), (2, 3, 5)),
}


# ------------------------------------------------------------------ helpers
def assert_close(out, ref, tol, where, what):
    """|out - ref| <= tol on `where` (NaN fails)."""
    assert np.isfinite(out[where]).all(), f"{what}: non-finite output"
    err = np.abs(out.astype(HI) - ref)
    bad = where & ~(err <= tol)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        worst = float(np.max(np.where(bad, err / np.maximum(tol, HI(1e-300)), 0)))
        raise AssertionError(f"{what}: {int(bad.sum())} nodes beyond the tolerance "
                             f"(worst {worst:.3g} x), first at {idx.tolist()}")


def rand(rng, shape, T):
    return rng.standard_normal(shape).astype(T)


def check_sum(got, terms, chain, mag=None, extra=0.0, what="sum"):
    """got against fsum(terms) within (chain + 3) 2^-53 of sum|terms| (+ extra)."""
    ref = vr.sum_hi(terms)
    scale = vr.sum_hi(np.abs(terms)) if mag is None else mag
    assert math.isfinite(got), f"{what}: {got}"
    bound = (chain + 3) * vr.U53 * scale + extra
    assert abs(got - ref) <= bound, (f"{what}: got {got!r}, reference {ref!r}, "
                                     f"difference {abs(got - ref):.3e} > bound {bound:.3e}")


# ------------------------------------------------ A: interface-fold update
def update_launch(g, T, tiled):
    """(blocks wanted, grid, chain length) of the update pass: one block per
    512 vectors (256 threads x 2 vectors of W elements), capped at the
    partials capacity - 256 with a grid-stride loop beyond."""
    W = 16 // np.dtype(T).itemsize
    if tiled:
        want = vr.cdiv(g.til_size // W, 512)
    else:
        want = g.own[0] * vr.cdiv(g.own[1] * (g.ld // W), 512)
    cap = lib().bdx_hip_partials_size() - 256
    grid = min(max(want, 1), cap)
    chain = vr.chain_block(vr.cdiv(want, grid) * 2 * W) + vr.chain_final(grid, TWO_STAGE)
    return want, grid, chain


@functools.lru_cache(maxsize=4)
def update_case(shape, suf):
    """Inputs and reference of the update on one shape (shared by the paths)."""
    g = geom(*A_SHAPES[shape])
    T = TYPES[suf][0]
    rng = np.random.default_rng(sum(map(ord, shape + suf)))
    own = g.owned_mask()
    r = rand(rng, g.L, T)
    y = rand(rng, g.L, T)
    y[~own] = NAN
    ifc = [rand(rng, s, T) for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    for a, o in zip(ifc, g.iface_owned()):
        a[~o] = NAN
    alpha = HI(vr.coefficient(scalars(), RN, PAP, T))
    f, mag = vr.fold(*[a.astype(HI) for a in [y] + ifc], g)
    ref = r.astype(HI) - alpha * f
    tol = 4 * HI(np.finfo(T).eps) * (np.abs(r.astype(HI)) + abs(alpha) * mag)
    for a in (r, y, *ifc, ref, tol):
        a.setflags(write=False)
    return g, own, r, y, ifc, ref, tol


def call_update(g, suf, tiled, d_r, d_y, d_ifc, d_scal, part):
    own64 = np.array(g.own, dtype=np.int64)
    desc = g.desc(tiled)
    if tiled:
        return fn("bdx_cg_update_tiled", suf)(
            ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]),
            ptr(d_ifc[2]), g.nty, g.ntz, ptr(d_scal), RN, PAP, OUT, ptr(part), stream())
    return fn("bdx_cg_update_iface", suf)(
        ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]), ptr(d_ifc[2]),
        g.nty, g.ntz, g.sy, g.sz, ptr(d_scal), RN, PAP, OUT, ptr(part), stream())


@pytest.mark.parametrize("path", ["flat", "tiled_pre", "tiled_plain"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(A_SHAPES))
def test_interface_fold_update(shape, suf, path, monkeypatch):
    g, own, r, y, ifc, ref, tol = update_case(shape, suf)
    T = TYPES[suf][0]
    tiled = path != "flat"
    if path == "tiled_plain":
        monkeypatch.setenv("BDX_UPD_PLAIN", "1")
    else:
        monkeypatch.delenv("BDX_UPD_PLAIN", raising=False)
    want, grid, chain = update_launch(g, T, tiled)
    if shape == "A9":   # the two-stage reduction of the block partials
        assert want > TWO_STAGE, (want, "A9 no longer reaches the two-stage reduction")
    r0, y0 = store(g, tiled, r, T), store(g, tiled, y, T)
    d_r, d_y = dev(r0), dev(y0)
    d_ifc = [dev(iface_flat(a, T)) for a in ifc]
    scal0 = scalars()
    d_scal, part = dev(scal0), new_partials()
    rc = call_update(g, suf, tiled, d_r, d_y, d_ifc, d_scal, part)
    r1 = host(d_r)
    chunk_bytes = g.tsy * g.tsz * np.dtype(T).itemsize
    if tiled and chunk_bytes % 16:
        # A8 in FP32: a 16-byte vector would straddle two chunks; refused
        assert shape == "A8" and suf == "f32"
        assert rc != 0
        assert_same_bits(r1, r0, "r after a refused call")
        assert_same_bits(host(d_scal), scal0, "scalars after a refused call")
        return
    assert rc == 0
    m = g.map(tiled)
    out = r1[m]
    assert_close(out, ref, tol, own, f"{shape} {suf} {path} r")
    keep = np.ones(r1.size, dtype=bool)
    keep[m[own]] = False
    assert_same_bits(r1[keep], r0[keep], "r outside the owned box")
    assert_same_bits(host(d_y), y0, "y")
    scal1 = host(d_scal)
    others = [s for s in range(8) if s != OUT]
    assert_same_bits(scal1[others], scal0[others], "scalar slots")
    # r.r: the kernel sums the squares of the values it stored ...
    sq = out[own].astype(np.float64) ** 2
    check_sum(float(scal1[OUT]), sq, chain, what="r.r of the stored r")
    # ... and against the reference r, with what the element tolerance allows
    rr, tt = np.abs(ref[own]), tol[own]
    extra = float(np.sum(2 * rr * tt + tt * tt)) * (1 + 1e-9)
    check_sum(float(scal1[OUT]), (rr * rr).astype(np.float64), chain, extra=extra,
              what="r.r of the reference r")


# ------------------------------------------------------------- A: finalize
@functools.lru_cache(maxsize=4)
def finalize_case(shape, suf, ghost_only):
    g = geom(*A_SHAPES[shape])
    T = TYPES[suf][0]
    rng = np.random.default_rng(sum(map(ord, shape + suf)) + 1000 + ghost_only)
    own = g.owned_mask()
    y = rand(rng, g.L, T)
    ifc = [rand(rng, s, T) for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    if ghost_only:   # the entries of owned nodes belong to the update pass
        for a, o in zip(ifc, g.iface_owned()):
            a[o] = NAN
    my, mz = g.iface_masks()
    wr = (my | mz) & (~own if ghost_only else True)
    yh = y.astype(HI)
    ref = yh + vr.iface_sum(yh, *[a.astype(HI) for a in ifc], g)
    mag = np.abs(yh) + vr.iface_sum(yh, *[np.abs(a.astype(HI)) for a in ifc], g)
    tol = 4 * HI(np.finfo(T).eps) * mag
    for a in (y, *ifc, ref, tol, wr):
        a.setflags(write=False)
    return g, y, ifc, ref, tol, wr


@pytest.mark.parametrize("ghost_only", [0, 1])
@pytest.mark.parametrize("tiled", [False, True], ids=["lattice", "tiled"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(A_SHAPES))
def test_fused_finalize(shape, suf, tiled, ghost_only):
    g, y, ifc, ref, tol, wr = finalize_case(shape, suf, ghost_only)
    T = TYPES[suf][0]
    y0 = store(g, tiled, y, T)
    d_y = dev(y0)
    d_ifc = [dev(iface_flat(a, T)) for a in ifc]
    desc = g.desc(tiled)
    rc = fn("bdx_fused_finalize", suf)(ptr(desc), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]),
                                       ptr(d_ifc[2]), g.nty, g.ntz, g.sy, g.sz, ghost_only,
                                       stream())
    assert rc == 0
    y1 = host(d_y)
    m = g.map(tiled)
    assert_close(y1[m], ref, tol, wr, f"{shape} {suf} finalize")
    keep = np.ones(y1.size, dtype=bool)
    keep[m[wr]] = False
    assert_same_bits(y1[keep], y0[keep], "y outside the interface nodes")
    if wr.any():   # every interface node did receive its terms
        assert np.all(y1[m][wr] != y[wr])


# ------------------------------------- A10: grid-stride beyond the grid cap
def _a10_shape(suf, tiled):
    """The smallest lattice of its family whose update pass wants more blocks
    than the cap.  Flat: one block per x-plane (a plane of 16 x 16 nodes is
    at most 512 vectors), so L0 > cap planes.  Tiled: 35 x 35 storage tiles
    of 12 x 12 nodes (34 x 34 kernel tiles; the last storage row and column
    hold only the last plane), L0 just large enough."""
    T = TYPES[suf][0]
    W = 16 // np.dtype(T).itemsize
    cap = lib().bdx_hip_partials_size() - 256
    if not tiled:
        n0 = vr.cdiv(cap + 1, 3)            # L0 = 3 n0 + 1 > cap + 1 (one ghost plane)
        return (3, (4, 4), (n0, 5, 5), (1, 0, 1))
    chunks = vr.cdiv(cap * 512 * W + 1, 144)
    n0 = vr.cdiv(vr.cdiv(chunks, 35 * 35) - 1, 3)
    return (3, (4, 4), (n0, 136, 136), (1, 1, 1))


@pytest.mark.parametrize("tiled", [False, True], ids=["flat", "tiled"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_update_grid_stride_beyond_cap(suf, tiled, monkeypatch):
    """Inputs and reference on the device in float64 (the lattices have 17 M
    to 127 M nodes).  The reference sum adds rows of 4096 terms on the device
    (a chain of at most 4096 more additions) and the row sums exactly."""
    monkeypatch.delenv("BDX_UPD_PLAIN", raising=False)
    T, tt = TYPES[suf]
    g = geom(*_a10_shape(suf, tiled))
    want, grid, chain = update_launch(g, T, tiled)
    cap = lib().bdx_hip_partials_size() - 256
    assert want > cap and grid == cap, (want, cap)
    assert want < 1.01 * cap    # and hardly larger than it has to be
    gen = torch.Generator(device="cuda").manual_seed(10 + tiled)

    def _tdev(*shape, dtype):
        return torch.randn(*shape, dtype=dtype, device="cuda", generator=gen)

    L0, L1, L2 = g.L
    o0, o1, o2 = g.own
    i = torch.arange(L0, device="cuda").view(-1, 1, 1)
    j = torch.arange(L1, device="cuda").view(1, -1, 1)
    k = torch.arange(L2, device="cuda").view(1, 1, -1)
    if tiled:
        m = ((j // g.tsy) * g.tntz + k // g.tsz) * (L0 * g.tsy * g.tsz) \
            + (i * g.tsy + j % g.tsy) * g.tsz + k % g.tsz
    else:
        m = (i * L1 + j) * g.ld + k
    m = m.reshape(-1)
    own = ((i < o0) & (j < o1) & (k < o2)).reshape(-1)
    del i, j, k
    size = g.size(tiled)
    node = torch.zeros(size, dtype=torch.bool, device="cuda")
    node[m] = True
    r0 = _tdev(size, dtype=tt)
    r0[~node] = NAN
    y0 = _tdev(size, dtype=tt)
    y0[~node] = NAN
    y0[m[~own]] = NAN
    del node
    ifc = [_tdev(*s, dtype=tt) for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    for a in ifc:   # entries of unowned nodes
        a[o0:] = NAN
    ifc[0][:, :, o2:] = NAN
    ifc[1][:, :, o1:] = NAN
    for a in range(g.nty - 1):
        if (a + 1) * g.sy >= o1:
            ifc[0][:, a] = NAN
            ifc[2][:, a] = NAN
    for b in range(g.ntz - 1):
        if (b + 1) * g.sz >= o2:
            ifc[1][:, b] = NAN
            ifc[2][:, :, b] = NAN
    d_r, scal0 = r0.clone(), scalars()
    d_scal, part = dev(scal0), new_partials()
    rc = call_update(g, suf, tiled, d_r, y0, [a.reshape(-1) for a in ifc], d_scal, part)
    torch.cuda.synchronize()
    assert rc == 0
    # reference, float64 on the device
    alpha = float(vr.coefficient(scal0, RN, PAP, T))
    f, mag = vr.fold(y0[m].double().view(g.L), *[a.double() for a in ifc], g)
    rd = r0[m].double()
    ref = rd - alpha * f.reshape(-1)
    tol = 4 * float(np.finfo(T).eps) * (rd.abs() + abs(alpha) * mag.reshape(-1))
    del f, mag, rd
    out = d_r[m].double()
    err = (out - ref).abs()
    ok = (err <= tol) | ~own
    nbad = int((~ok).sum().item())
    assert nbad == 0, f"{nbad} nodes beyond the tolerance, first at {torch.nonzero(~ok)[:5]}"
    assert bool(torch.isfinite(out[own]).all().item())
    del err, ok, ref, tol
    keep = torch.ones(size, dtype=torch.bool, device="cuda")
    keep[m[own]] = False
    ib = torch.int64 if suf == "f64" else torch.int32
    assert torch.equal(d_r.view(ib)[keep], r0.view(ib)[keep]), "r outside the owned box"
    scal1 = host(d_scal)
    others = [s for s in range(8) if s != OUT]
    assert_same_bits(scal1[others], scal0[others], "scalar slots")
    sq = out[own] ** 2
    pad = (-sq.numel()) % 4096
    rows = torch.cat([sq, sq.new_zeros(pad)]).view(-1, 4096).sum(dim=1)
    check_sum(float(scal1[OUT]), rows.cpu().numpy(), chain + 4096, what="r.r (grid-stride)")


# ----------------------------------------------------------- B: flush/export
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(B_SHAPES))
def test_flush_export(shape, suf):
    g = geom(*B_SHAPES[shape])
    T = TYPES[suf][0]
    if shape == "B1":
        assert g.tntz == 17
    if shape == "B2":
        assert g.tntz == 16
    if shape == "B3":
        assert g.tntz == 17 and (g.tntz - 1) * g.tsz == g.L[2] - 1
    rng = np.random.default_rng(sum(map(ord, shape + suf)) + 2000)
    t, p1, p2 = (rand(rng, g.L, T) for _ in range(3))
    mt, ml = g.map(True), g.map(False)
    t0, d_p1, d_p2 = store(g, True, t, T), dev(store(g, True, p1, T)), dev(store(g, True, p2, T))
    lat0 = rand(rng, g.lat_size, T)
    lat0[np.setdiff1d(np.arange(g.lat_size), ml.ravel())] = NAN
    scal0 = scalars()
    d_scal = dev(scal0)
    a1 = HI(vr.coefficient(scal0, RN, PAP, T))       # a ratio
    a2 = HI(vr.coefficient(scal0, XS, -1, T))        # stored directly (den < 0)
    colour = vr.tile_colour(g)
    th, p1h, p2h = t.astype(HI), p1.astype(HI), p2.astype(HI)
    eps = HI(np.finfo(T).eps)
    everywhere = np.ones(g.L, dtype=bool)
    for with_p2, mask in [(False, 0), (False, 4)] + [(True, q) for q in (1, 2, 3, 5, 6, 7)]:
        what = f"{shape} {suf} p2mask={mask}"
        on = (((mask >> colour) & 1) == 1) if with_p2 else np.zeros(g.L, dtype=bool)
        ref = th + a1 * p1h + np.where(on, a2 * p2h, 0)
        tol = 4 * eps * (np.abs(th) + np.abs(a1 * p1h) + np.where(on, np.abs(a2 * p2h), 0))
        d_t, d_lat = dev(t0), dev(lat0)
        rc = fn("bdx_flush_export", suf)(ptr(g.latd_tiled), ptr(d_lat), ptr(d_t), ptr(d_p1),
                                         ptr(d_p2) if with_p2 else 0, ptr(d_scal), RN, PAP, XS,
                                         -1, mask, stream())
        assert rc == 0, what
        lat1, t1 = host(d_lat), host(d_t)
        assert_close(lat1[ml], ref, tol, everywhere, what + " lattice export")
        keep = np.ones(lat1.size, dtype=bool)
        keep[ml.ravel()] = False
        assert_same_bits(lat1[keep], lat0[keep], what + " lattice pad columns")
        if mask & 4:
            assert_same_bits(t1, t0, what + " tiled iterate (export only)")
        else:   # the flushed iterate is what was exported
            assert_same_bits(t1[mt], lat1[ml], what + " tiled iterate against the export")
    assert_same_bits(host(d_scal), scal0, "scalars")


# ---------------------------------------------------- C: layout conversion
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["A1", "A2", "A3", "A4", "A5", "A6"])
def test_layout_convert(shape, suf):
    g = geom(*A_SHAPES[shape])
    T = TYPES[suf][0]
    rng = np.random.default_rng(sum(map(ord, shape + suf)) + 3000)
    a = rand(rng, g.L, T)
    mt, ml = g.map(True), g.map(False)
    lat0, til0 = store(g, False, a, T), rand(rng, g.til_size, T)
    d_lat, d_til = dev(lat0), dev(til0)
    conv = fn("bdx_layout_convert", suf)
    assert conv(0, ptr(g.latd_tiled), ptr(d_lat), ptr(d_til), stream()) == 0
    til1 = host(d_til)
    assert_same_bits(til1[mt], a, "tiled copy")
    keep = np.ones(til1.size, dtype=bool)
    keep[mt.ravel()] = False
    assert_same_bits(til1[keep], til0[keep], "tiled padding")
    assert_same_bits(host(d_lat), lat0, "lattice source")
    # back, from a tiled vector whose padding is poisoned
    til2 = store(g, True, a[::-1, ::-1, ::-1], T)
    lat2 = rand(rng, g.lat_size, T)
    d_lat2, d_til2 = dev(lat2), dev(til2)
    assert conv(1, ptr(g.latd_tiled), ptr(d_lat2), ptr(d_til2), stream()) == 0
    lat3 = host(d_lat2)
    assert_same_bits(lat3[ml], a[::-1, ::-1, ::-1], "lattice copy")
    keep = np.ones(lat3.size, dtype=bool)
    keep[ml.ravel()] = False
    assert_same_bits(lat3[keep], lat2[keep], "lattice pad columns")
    assert_same_bits(host(d_til2), til2, "tiled source")
    # round trip of the first conversion
    assert conv(1, ptr(g.latd_tiled), ptr(d_lat2), ptr(d_til), stream()) == 0
    assert_same_bits(host(d_lat2)[ml], a, "round trip")
    # the lattice descriptor is refused
    assert conv(0, ptr(g.latd), ptr(d_lat), ptr(d_til), stream()) != 0


# ------------------------------------------------------------ C: halo boxes
class _Table:
    def __init__(self, boxes):
        """boxes: [(lo, extent)] in order; offsets are cumulative."""
        self.boxes, rows, off = boxes, [], 0
        for lo, e in boxes:
            rows.append(list(lo) + list(e) + [off])
            off += int(np.prod(e))
        self.total = off
        self.table = torch.tensor(np.array(rows, dtype=np.int64).reshape(-1, 7), device="cuda")

    @classmethod
    def of_side(cls, side):
        t = cls([(b.lo, tuple(h - l for l, h in zip(b.lo, b.hi))) for b in side.boxes])
        assert t.total == side.total and torch.equal(t.table, side.table)
        t.table = side.table
        return t

    def nodes(self):
        """Per box, the (i, j, k) index arrays of its nodes in buffer order."""
        out = []
        for lo, e in self.boxes:
            ii, jj, kk = np.meshgrid(*[np.arange(a, a + b) for a, b in zip(lo, e)], indexing="ij")
            out.append((ii.ravel(), jj.ravel(), kk.ravel()))
        return out


def _box_tables(g):
    lat = g.lat
    L0, L1, L2 = g.L
    hand = _Table([((0, 0, 0), (1, L1, L2)), ((0, 0, 0), (L0, 1, L2)), ((0, 0, 0), (L0, L1, 1)),
                   ((0, 0, 0), (1, 1, L2)), ((0, 0, 0), (1, 1, 1)),
                   ((L0 - 2, L1 - 3, L2 - 4), (2, 3, 4))])
    return {"send": (_Table.of_side(_Side(lat.halo_send_boxes(), lat.nranks, lat, "cuda")), True),
            "recv": (_Table.of_side(_Side(lat.halo_recv_boxes(), lat.nranks, lat, "cuda")), False),
            "hand": (hand, True)}


def _call_box(api, suf, mode, g, d_vec, tab, d_buf):
    if api == "plain":
        return fn("bdx_box_copy", suf)(mode, ptr(d_vec), g.L[1], g.ld, ptr(tab.table),
                                       len(tab.boxes), tab.total, ptr(d_buf), stream())
    return fn("bdx_box_copy_lat", suf)(mode, ptr(d_vec), ptr(g.desc(api == "tiled")),
                                       ptr(tab.table), len(tab.boxes), tab.total, ptr(d_buf),
                                       stream())


@pytest.mark.parametrize("api", ["plain", "lattice", "tiled"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("gh", [(1, 0, 0), (0, 1, 1), (1, 1, 1)])
@pytest.mark.parametrize("P,tile,n", [(3, (4, 4), (2, 5, 6)), (4, (2, 4), (3, 3, 9))])
def test_box_copy(P, tile, n, gh, suf, api):
    g = geom(P, tile, n, gh, True)
    T = TYPES[suf][0]
    tiled = api == "tiled"
    m = g.map(tiled)
    rng = np.random.default_rng(4000 + sum(gh) + P)
    tables = _box_tables(g)
    assert len(tables["send"][0].boxes) == 7 and len(tables["recv"][0].boxes) == 2 ** sum(gh) - 1
    for name, (tab, overlapping) in tables.items():
        nodes = tab.nodes()
        inbox = np.zeros(g.L, dtype=bool)
        for ii, jj, kk in nodes:
            inbox[ii, jj, kk] = True
        assert inbox.any() and not inbox.all()
        # pack: nodes outside every box are never read
        a = rand(rng, g.L, T)
        a[~inbox] = NAN
        v0, b0 = store(g, tiled, a, T), rand(rng, tab.total + 5, T)
        d_v, d_b = dev(v0), dev(b0)
        assert _call_box(api, suf, 0, g, d_v, tab, d_b) == 0
        b1 = host(d_b)
        want = np.concatenate([a[ii, jj, kk] for ii, jj, kk in nodes])
        assert_same_bits(b1[: tab.total], want, f"{name} pack")
        assert_same_bits(b1[tab.total:], b0[tab.total:], f"{name} pack: beyond the buffer")
        assert_same_bits(host(d_v), v0, f"{name} pack: the vector")
        # unpack (assign; disjoint boxes only) and add-unpack (box by box, in order)
        for mode in ([2] if overlapping else [1, 2]):
            a = rand(rng, g.L, T)
            v0, b0 = store(g, tiled, a, T), rand(rng, tab.total + 5, T)
            d_v, d_b = dev(v0), dev(b0)
            assert _call_box(api, suf, mode, g, d_v, tab, d_b) == 0
            exp, off = a.copy(), 0
            for ii, jj, kk in nodes:
                seg = b0[off: off + ii.size]
                exp[ii, jj, kk] = seg if mode == 1 else exp[ii, jj, kk] + seg
                off += ii.size
            v1 = host(d_v)
            assert_same_bits(v1[m], exp, f"{name} unpack mode {mode}")
            keep = np.ones(v1.size, dtype=bool)
            keep[m[inbox]] = False
            assert_same_bits(v1[keep], v0[keep], f"{name} unpack mode {mode}: outside the boxes")
            assert_same_bits(host(d_b), b0, f"{name} unpack mode {mode}: the buffer")


# ----------------------------------------------------------------- D: BLAS-1
D_LATTICES = {
    "short": (3, (4, 4), (3, 5, 6)),        # rows of 19 < 64 (A1)
    "long": (5, (2, 2), (2, 3, 33)),        # rows of 166 > 64 (B1)
    "rows": (3, (4, 4), (32, 48, 48)),      # 14065 rows > 8192: the row grid-stride (A9)
}


def rows_launch(g):
    """(grid, chain) of the row kernels: 4 rows per block pass (one per wave),
    at most 2048 blocks, each lane 64 apart along the row."""
    nrows = g.own[0] * g.own[1]
    grid = min(max(vr.cdiv(nrows, 4), 1), 2048)
    per_thread = vr.cdiv(nrows, 4 * grid) * vr.cdiv(g.own[2], 64)
    return grid, vr.chain_block(per_thread) + vr.chain_final(grid)


def blas_cases(f):
    for deco in (pytest.mark.parametrize("suf", ["f64", "f32"]),
                 pytest.mark.parametrize("gh", [(0, 0, 0), (1, 1, 1), (0, 1, 0)]),
                 pytest.mark.parametrize("which", list(D_LATTICES))):
        f = deco(f)
    return f


def blas_setup(which, gh, suf):
    """(g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only,
    chain, scal0, others) of one BLAS-1 case."""
    P, tile, n = D_LATTICES[which]
    g = geom(P, tile, n, gh)
    T = TYPES[suf][0]
    eps = HI(np.finfo(T).eps)
    own = g.owned_mask()
    o0, o1, o2 = g.own
    L1, ld = g.L[1], g.ld
    if which == "rows":
        assert o0 * o1 > 4 * 2048
    rng = np.random.default_rng(5000 + sum(gh) + P)
    m = g.map(False)
    outside = np.ones(g.lat_size, dtype=bool)
    outside[m[own]] = False

    def full():       # finite on every node (an in/out vector), pad = NaN
        a = rand(rng, g.L, T)
        return a, store(g, False, a, T)

    def owned_only():  # an input read on owned nodes only
        a = rand(rng, g.L, T)
        a[~own] = NAN
        return a, store(g, False, a, T)

    _, chain = rows_launch(g)
    scal0 = scalars()
    others = [s for s in range(8) if s != OUT]
    return (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
            others)


@blas_cases
def test_dot(which, gh, suf):
    (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
     others) = blas_setup(which, gh, suf)
    (a, a0), (b, b0) = owned_only(), owned_only()
    d_a, d_b, d_scal, part = dev(a0), dev(b0), dev(scal0), new_partials()
    assert fn("bdx_dot", suf)(L1, ld, o0, o1, o2, ptr(d_a), ptr(d_b), ptr(part),
                              ptr(d_scal), OUT, stream()) == 0
    s1 = host(d_scal)
    prod = (a[own].astype(HI) * b[own].astype(HI)).astype(np.float64)
    check_sum(float(s1[OUT]), prod, chain, what="dot")
    assert_same_bits(s1[others], scal0[others], "dot: scalar slots")


@blas_cases
def test_cg_update(which, gh, suf):
    """x += alpha p, r -= alpha y, r.r"""
    (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
     others) = blas_setup(which, gh, suf)
    (x, x0), (r, r0), (p, p0), (y, y0) = full(), full(), owned_only(), owned_only()
    d_x, d_r, d_scal, part = dev(x0), dev(r0), dev(scal0), new_partials()
    d_p, d_y = dev(p0), dev(y0)
    assert fn("bdx_cg_update", suf)(L1, ld, o0, o1, o2, ptr(d_x), ptr(d_r), ptr(d_p),
                                    ptr(d_y), ptr(d_scal), RN, PAP, OUT, ptr(part),
                                    stream()) == 0
    al = HI(vr.coefficient(scal0, RN, PAP, T))
    x1, r1, s1 = host(d_x), host(d_r), host(d_scal)
    xh, rh, ph, yh = (v.astype(HI) for v in (x, r, p, y))
    assert_close(x1[m], xh + al * ph, 4 * eps * (np.abs(xh) + np.abs(al * ph)), own, "cg_update x")
    assert_close(r1[m], rh - al * yh, 4 * eps * (np.abs(rh) + np.abs(al * yh)), own, "cg_update r")
    assert_same_bits(x1[outside], x0[outside], "cg_update: x outside the owned box")
    assert_same_bits(r1[outside], r0[outside], "cg_update: r outside the owned box")
    check_sum(float(s1[OUT]), r1[m][own].astype(np.float64) ** 2, chain, what="cg_update r.r")
    assert_same_bits(s1[others], scal0[others], "cg_update: scalar slots")


@blas_cases
def test_p_update(which, gh, suf):
    """p = beta p + r"""
    (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
     others) = blas_setup(which, gh, suf)
    (p, p0), (r, r0) = full(), owned_only()
    d_p, d_r, d_scal = dev(p0), dev(r0), dev(scal0)
    assert fn("bdx_p_update", suf)(L1, ld, o0, o1, o2, ptr(d_p), ptr(d_r), ptr(d_scal),
                                   6, PAP, stream()) == 0
    be = HI(vr.coefficient(scal0, 6, PAP, T))
    p1, ph, rh = host(d_p), p.astype(HI), r.astype(HI)
    assert_close(p1[m], be * ph + rh, 4 * eps * (np.abs(be * ph) + np.abs(rh)), own, "p_update")
    assert_same_bits(p1[outside], p0[outside], "p_update: outside the owned box")


@blas_cases
def test_axpy(which, gh, suf):
    """out = alpha x + y"""
    (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
     others) = blas_setup(which, gh, suf)
    (_, out0), (x, x0), (y, y0) = full(), owned_only(), owned_only()
    d_o, d_x, d_y = dev(out0), dev(x0), dev(y0)
    assert fn("bdx_axpy", suf)(L1, ld, o0, o1, o2, ptr(d_o), -1.7, ptr(d_x), ptr(d_y),
                               stream()) == 0
    al = HI(T(-1.7))
    o1_, xh, yh = host(d_o), x.astype(HI), y.astype(HI)
    assert_close(o1_[m], al * xh + yh, 4 * eps * (np.abs(al * xh) + np.abs(yh)), own, "axpy")
    assert_same_bits(o1_[outside], out0[outside], "axpy: outside the owned box")


@blas_cases
def test_xflush(which, gh, suf):
    """x += a p, both forms of the coefficient"""
    (g, T, eps, own, (L1, ld, o0, o1, o2), m, outside, full, owned_only, chain, scal0,
     others) = blas_setup(which, gh, suf)
    own64 = np.array(g.own, dtype=np.int64)
    for num, den in ((RN, PAP), (XS, -1)):
        (x, x0), (p, p0) = full(), owned_only()
        d_x, d_p, d_scal = dev(x0), dev(p0), dev(scal0)
        assert fn("bdx_xflush", suf)(ptr(g.latd), ptr(own64), ptr(d_x), ptr(d_p),
                                     ptr(d_scal), num, den, stream()) == 0
        al = HI(vr.coefficient(scal0, num, den, T))
        x1, xh, ph = host(d_x), x.astype(HI), p.astype(HI)
        assert_close(x1[m], xh + al * ph, 4 * eps * (np.abs(xh) + np.abs(al * ph)), own,
                     f"xflush den={den}")
        assert_same_bits(x1[outside], x0[outside], "xflush: outside the owned box")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536])
def test_reduce_partials(n):
    rng = np.random.default_rng(n)
    p = np.full(lib().bdx_hip_partials_size(), NAN)
    assert n <= p.size
    p[:n] = rng.random(n) * 10.0 ** rng.integers(-3, 4, n)
    scal0 = scalars()
    d_scal, d_p = dev(scal0), dev(p)
    assert lib().bdx_reduce_partials(ptr(d_p), n, ptr(d_scal), OUT, stream()) == 0
    s1 = host(d_scal)
    check_sum(float(s1[OUT]), p[:n], vr.chain_block(vr.cdiv(n, 256)), what=f"reduce_partials({n})")
    others = [s for s in range(8) if s != OUT]
    assert_same_bits(s1[others], scal0[others], "scalar slots")


def test_entry_points_are_declared():
    """ctypes signatures exist for every entry point used above (an
    undeclared function would take its int64 arguments as C ints)."""
    for suf in TYPES:
        for name in ("bdx_cg_update_tiled", "bdx_flush_export", "bdx_cg_update_iface",
                     "bdx_fused_finalize", "bdx_layout_convert", "bdx_box_copy_lat"):
            f = fn(name, suf)
            assert f.argtypes is not None and f.restype is ctypes.c_int, name
