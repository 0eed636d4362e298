"""The Jacobi-preconditioned update pass of the fused CG loop
(bdx_pcg_update_iface_*, bdx_pcg_update_tiled_*; csrc/hip/cg_update.hip),
driven directly through its C entry points with hand-built lattice descriptors.

Per case:

* r after the call is bitwise what the unpreconditioned entry point
  (bdx_cg_update_iface_* / bdx_cg_update_tiled_*) writes from the same inputs,
  over the whole buffer, and agrees with the numpy reference of
  tests/pcg_update_ref.py within 4 eps_T sum|terms| on the owned nodes;
* z on the owned nodes is bitwise T(dinv) * T(r_new): one correctly rounded
  multiply, so numpy in T gives the same bits;
* outside the 16-byte vectors the r update stores (pcg_update_ref.stored_elements)
  z keeps its initial bits; y, dinv and the interface buffers are unchanged;
* inputs carry NaN wherever the pass must not use them: y and the interface
  entries of unowned nodes, every padding element, all of z, every unused
  scalar slot; dinv is random in [0.5, 2];
* both scalars lie within n eps_double sum|terms| of math.fsum of the terms,
  the terms being products of the stored T values in float64 (the bound form
  of tests/test_gpu_diagonal.py::test_pcg_update_kernel); every other scalar
  slot keeps its bits;
* a second call on identical inputs gives bitwise identical scalars (fixed-order
  reductions, no atomics).
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import kernel_harness as kh
import pcg_update_ref as pr
import vector_ref as vr
from benchmark_dolfinx_amd.ops.native import ptr
from kernel_harness import (assert_same_bits, dev, fn, geom, host, iface_flat, lib,
                            new_partials, store, stream)

pytestmark = pytest.mark.gpu

HI = np.longdouble
NAN = float("nan")
EPS = 2.0 ** -52
TYPES = {"f64": (np.float64, torch.float64), "f32": (np.float32, torch.float32)}
RN, PAP, OUT, RR = 0, 2, 1, 5         # scalar slots: r.z (old), p.Ap, r.z (new), r.r
SCAL = {RN: 0.8125, PAP: 1.37}
PATHS = ["flat", "tiled_pre", "tiled_plain"]
scalars = functools.partial(kh.scalars, SCAL)

# P, kernel tile (cells), local cells, ghost planes: the smallest shapes with
# both interface kinds, ghost planes, a tile-corner buffer, a non-ROW FP32
# tile (tsz % 4 != 0: S3, S5) and a partly filled last vector
SHAPES = {
    "S1": (3, (4, 4), (3, 5, 6), (0, 0, 0)),
    "S2": (3, (4, 4), (2, 8, 8), (1, 1, 1)),
    "S3": (5, (2, 2), (2, 3, 5), (0, 1, 0)),
    "S4": (4, (2, 4), (3, 3, 9), (1, 0, 1)),
    "S5": (7, (2, 2), (2, 2, 3), (0, 0, 0)),
    "S6": (6, (2, 2), (2, 5, 4), (0, 0, 1)),
}
# Tile planes (tsy tsz = P^2 TY TZ elements) of the table: 144, 144, 100, 128,
# 196, 144.  Every one is a multiple of 4, so in FP32 (4 bytes) and in FP64
# they are multiples of 16 bytes: the host wrapper refuses none of them.
REFUSED_EXPECTED = 0


def _refused(shape, suf, path):
    P, (ty, tz), _, _ = SHAPES[shape]
    return path != "flat" and (P * ty * P * tz * np.dtype(TYPES[suf][0]).itemsize) % 16 != 0


ALL = [(s, f, p) for s in SHAPES for f in TYPES for p in PATHS]
CASES = [c for c in ALL if not _refused(*c)]


def test_refused_combinations_are_what_the_shape_table_predicts():
    assert len(ALL) - len(CASES) == REFUSED_EXPECTED
    # and the wrapper does refuse such a plane (5 x 10 nodes in FP32: 200 bytes)
    g = vr.Geom(5, (1, 2), (2, 3, 5))
    T = np.float32
    assert (g.tsy * g.tsz * 4) % 16 != 0 and (g.tsy * g.tsz * 8) % 16 == 0
    bufs = [dev(np.zeros(g.til_size, dtype=T)) for _ in range(4)]
    ifc = [dev(np.zeros(max(1, int(np.prod(s))), dtype=T))
           for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    scal0 = scalars()
    d_scal, parts = dev(scal0), [new_partials(), new_partials()]
    rc = call_pcg(g, "f32", True, bufs[0], bufs[1], ifc, d_scal, parts, bufs[2], bufs[3])
    assert rc != 0
    assert_same_bits(host(d_scal), scal0, "scalars after a refused call")


# ------------------------------------------------------------------ helpers
def check_sum(got, terms, what):
    """got against math.fsum(terms) within n eps sum|terms|."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    ref = math.fsum(terms.tolist())
    bound = terms.size * EPS * math.fsum(np.abs(terms).tolist())
    print(f"{what}: got {got!r} ref {ref!r} |diff| {abs(got - ref):.3e} bound {bound:.3e}")
    assert math.isfinite(got), f"{what}: {got}"
    assert abs(got - ref) <= bound, f"{what}: got {got!r}, reference {ref!r}, bound {bound:.3e}"


def call_cg(g, suf, tiled, d_r, d_y, d_ifc, d_scal, part):
    """The unpreconditioned entry point (the r this pass must reproduce)."""
    own64 = np.array(g.own, dtype=np.int64)
    desc = g.desc(tiled)
    if tiled:
        return fn("bdx_cg_update_tiled", suf)(
            ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]),
            ptr(d_ifc[2]), g.nty, g.ntz, ptr(d_scal), RN, PAP, OUT, ptr(part), stream())
    return fn("bdx_cg_update_iface", suf)(
        ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]), ptr(d_ifc[2]),
        g.nty, g.ntz, g.sy, g.sz, ptr(d_scal), RN, PAP, OUT, ptr(part), stream())


def call_pcg(g, suf, tiled, d_r, d_y, d_ifc, d_scal, parts, d_dinv, d_z):
    own64 = np.array(g.own, dtype=np.int64)
    desc = g.desc(tiled)
    if tiled:
        return fn("bdx_pcg_update_tiled", suf)(
            ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]),
            ptr(d_ifc[2]), g.nty, g.ntz, ptr(d_scal), RN, PAP, OUT, ptr(parts[0]), ptr(d_dinv),
            ptr(d_z), RR, ptr(parts[1]), stream())
    return fn("bdx_pcg_update_iface", suf)(
        ptr(desc), ptr(own64), ptr(d_r), ptr(d_y), ptr(d_ifc[0]), ptr(d_ifc[1]), ptr(d_ifc[2]),
        g.nty, g.ntz, g.sy, g.sz, ptr(d_scal), RN, PAP, OUT, ptr(parts[0]), ptr(d_dinv), ptr(d_z),
        RR, ptr(parts[1]), stream())


@functools.lru_cache(maxsize=4)
def update_case(shape, suf):
    """Inputs and the numpy reference on one shape (shared by the paths,
    read-only)."""
    g = geom(*SHAPES[shape])
    T = TYPES[suf][0]
    rng = np.random.default_rng(sum(map(ord, shape + suf)) + 7000)
    own = g.owned_mask()
    r = rng.standard_normal(g.L).astype(T)
    y = rng.standard_normal(g.L).astype(T)
    y[~own] = NAN
    ifc = [rng.standard_normal(s).astype(T) for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    for a, o in zip(ifc, g.iface_owned()):
        a[~o] = NAN
    dinv = rng.uniform(0.5, 2.0, g.L).astype(T)
    alpha = HI(vr.coefficient(scalars(), RN, PAP, T))
    ref, _, mag = pr.update(*[a.astype(HI) for a in (r, y, *ifc, dinv)], alpha, g)
    tol = 4 * HI(np.finfo(T).eps) * (np.abs(r.astype(HI)) + abs(alpha) * mag)
    for a in (r, y, *ifc, dinv, ref, tol):
        a.setflags(write=False)
    return g, own, r, y, ifc, dinv, ref, tol


@pytest.mark.parametrize("shape,suf,path", CASES)
def test_pcg_update(shape, suf, path, monkeypatch):
    g, own, r, y, ifc, dinv, ref, tol = update_case(shape, suf)
    T = TYPES[suf][0]
    W = 16 // np.dtype(T).itemsize
    tiled = path != "flat"
    if path == "tiled_plain":
        monkeypatch.setenv("BDX_UPD_PLAIN", "1")
    else:
        monkeypatch.delenv("BDX_UPD_PLAIN", raising=False)
    if suf == "f32" and tiled and shape in ("S3", "S5"):
        assert g.tsz % 4 != 0          # the per-element (non-ROW) FP32 kernels
    r0, y0, dinv0 = (store(g, tiled, a, T) for a in (r, y, dinv))
    z0 = np.full(g.size(tiled), NAN, dtype=T)
    ifc0 = [iface_flat(a, T) for a in ifc]
    scal0 = scalars()

    # the unpreconditioned pass on the same inputs
    d_r, d_y, d_ifc, d_scal = dev(r0), dev(y0), [dev(a) for a in ifc0], dev(scal0)
    assert call_cg(g, suf, tiled, d_r, d_y, d_ifc, d_scal, new_partials()) == 0
    r_cg = host(d_r)

    runs = []
    for _ in range(2):
        d_r, d_y, d_ifc, d_scal = dev(r0), dev(y0), [dev(a) for a in ifc0], dev(scal0)
        d_dinv, d_z = dev(dinv0), dev(z0)
        parts = [new_partials(), new_partials()]
        assert call_pcg(g, suf, tiled, d_r, d_y, d_ifc, d_scal, parts, d_dinv, d_z) == 0
        runs.append((host(d_r), host(d_z), host(d_scal)))
        assert_same_bits(host(d_y), y0, "y")
        assert_same_bits(host(d_dinv), dinv0, "dinv")
        for a, b, name in zip(d_ifc, ifc0, ("yb", "zb", "cb")):
            assert_same_bits(host(a), b, name)
    r1, z1, scal1 = runs[0]
    what = f"{shape} {suf} {path}"

    # r: the unpreconditioned kernel's, bit for bit, and the reference's
    assert_same_bits(r1, r_cg, what + ": r against the unpreconditioned pass")
    m = g.map(tiled)
    out = r1[m]
    assert np.isfinite(out[own]).all()
    err = np.abs(out.astype(HI) - ref)
    assert not (own & ~(err <= tol)).any(), what + ": r beyond the tolerance of the reference"

    # z: one multiply of the stored values on the owned nodes ...
    zn = z1[m]
    assert np.isfinite(zn[own]).all()
    assert_same_bits(zn[own], pr.z_of(np.asarray(dinv)[own], out[own]), what + ": z = dinv * r")
    # ... and nothing outside the vectors the r update stores
    stored = pr.stored_elements(g, tiled, W)
    assert stored[m[own]].all()
    assert_same_bits(z1[~stored], z0[~stored], what + ": z outside the stored vectors")
    if tiled and any(SHAPES[shape][3]):
        assert not stored.all()

    # scalars: from the stored values
    rz, rr = pr.scalar_terms(out[own], zn[own])
    check_sum(float(scal1[OUT]), rz, what + " r.z")
    check_sum(float(scal1[RR]), rr, what + " r.r")
    others = [s for s in range(8) if s not in (OUT, RR)]
    assert_same_bits(scal1[others], scal0[others], what + ": other scalar slots")

    # determinism
    assert_same_bits(runs[1][2], scal1, what + ": scalars of a second call")
    assert_same_bits(runs[1][0], r1, what + ": r of a second call")
    assert_same_bits(runs[1][1], z1, what + ": z of a second call")


def test_bad_arguments_are_refused():
    """No dinv / z / second partials buffer, or one buffer or slot for both
    sums: an error, nothing launched."""
    g = geom(*SHAPES["S1"])
    T = np.float64
    bufs = [dev(np.zeros(g.lat_size, dtype=T)) for _ in range(4)]
    ifc = [dev(np.zeros(max(1, int(np.prod(s))), dtype=T))
           for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
    scal0 = scalars()
    d_scal, p = dev(scal0), [new_partials(), new_partials()]
    assert call_pcg(g, "f64", False, bufs[0], bufs[1], ifc, d_scal, p, None, bufs[3]) != 0
    assert call_pcg(g, "f64", False, bufs[0], bufs[1], ifc, d_scal, p, bufs[2], None) != 0
    assert call_pcg(g, "f64", False, bufs[0], bufs[1], ifc, d_scal, [p[0], None], bufs[2],
                    bufs[3]) != 0
    assert call_pcg(g, "f64", False, bufs[0], bufs[1], ifc, d_scal, [p[0], p[0]], bufs[2],
                    bufs[3]) != 0
    assert_same_bits(host(d_scal), scal0, "scalars after refused calls")


# ------------------------------------------- grid-stride beyond the grid cap
def _big_shape(suf, tiled):
    """The smallest lattice of its family whose update pass wants more blocks
    than the cap (the shapes of test_update_grid_stride_beyond_cap)."""
    T = TYPES[suf][0]
    W = 16 // np.dtype(T).itemsize
    cap = lib().bdx_hip_partials_size() - 256
    if not tiled:
        n0 = vr.cdiv(cap + 1, 3)
        return (3, (4, 4), (n0, 5, 5), (1, 0, 1))
    chunks = vr.cdiv(cap * 512 * W + 1, 144)
    n0 = vr.cdiv(vr.cdiv(chunks, 35 * 35) - 1, 3)
    return (3, (4, 4), (n0, 136, 136), (1, 1, 1))


@pytest.mark.parametrize("suf,tiled", [("f64", False), ("f32", True)], ids=["flat", "tiled"])
def test_pcg_update_grid_stride_beyond_cap(suf, tiled, monkeypatch):
    """One case per layout with more work than the 65280-block cap (the PC
    instances are code of their own).  Inputs and checks on the device (17 M
    and 134 M nodes).  The reference sums add rows of 4096 terms on the device
    and the row sums exactly: an extra relative error of at most 4096 eps,
    far inside the n eps bound at these n."""
    monkeypatch.delenv("BDX_UPD_PLAIN", raising=False)
    T, tt = TYPES[suf]
    W = 16 // np.dtype(T).itemsize
    g = geom(*_big_shape(suf, tiled))
    cap = lib().bdx_hip_partials_size() - 256
    want = (vr.cdiv(g.til_size // W, 512) if tiled
            else g.own[0] * vr.cdiv(g.own[1] * (g.ld // W), 512))
    assert cap < want < 1.01 * cap, (want, cap)
    gen = torch.Generator(device="cuda").manual_seed(20 + tiled)
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
    mo = m[own]
    node = torch.zeros(size, dtype=torch.bool, device="cuda")
    node[m] = True
    r0 = torch.randn(size, dtype=tt, device="cuda", generator=gen)
    r0[~node] = NAN
    y0 = torch.randn(size, dtype=tt, device="cuda", generator=gen)
    y0[~node] = NAN
    y0[m[~own]] = NAN
    dinv0 = torch.rand(size, dtype=tt, device="cuda", generator=gen) * 1.5 + 0.5
    dinv0[~node] = NAN
    del node
    z0 = torch.full((size,), NAN, dtype=tt, device="cuda")
    ifc = [torch.randn(*s, dtype=tt, device="cuda", generator=gen)
           for s in (g.yb_shape, g.zb_shape, g.cb_shape)]
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
    ifc = [a.reshape(-1) for a in ifc]
    scal0 = scalars()
    ib = torch.int64 if suf == "f64" else torch.int32

    r_cg, d_scal = r0.clone(), dev(scal0)
    assert call_cg(g, suf, tiled, r_cg, y0, ifc, d_scal, new_partials()) == 0
    d_r, d_z, d_scal = r0.clone(), z0.clone(), dev(scal0)
    parts = [new_partials(), new_partials()]
    assert call_pcg(g, suf, tiled, d_r, y0, ifc, d_scal, parts, dinv0, d_z) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_r.view(ib), r_cg.view(ib)), "r against the unpreconditioned pass"
    assert not torch.equal(d_r.view(ib), r0.view(ib))
    del r_cg
    ro, zo = d_r[mo], d_z[mo]
    assert bool(torch.isfinite(ro).all().item()) and bool(torch.isfinite(zo).all().item())
    assert torch.equal(zo.view(ib), (dinv0[mo] * ro).view(ib)), "z = dinv * r on the owned nodes"
    # z outside the stored vectors
    if tiled:
        owned_s = torch.zeros(size, dtype=torch.bool, device="cuda")
        owned_s[mo] = True
        stored = owned_s.view(-1, W).any(dim=1).repeat_interleave(W)
        del owned_s
    else:
        row = torch.arange(size, device="cuda") // g.ld
        stored = (row // L1 < o0) & (row % L1 < o1)
        del row
    assert not bool(stored.all().item())
    assert torch.equal(d_z.view(ib)[~stored], z0.view(ib)[~stored]), "z outside the stored vectors"
    del stored
    scal1 = host(d_scal)
    others = [s for s in range(8) if s not in (OUT, RR)]
    assert_same_bits(scal1[others], scal0[others], "other scalar slots")
    rd, zd = ro.double(), zo.double()
    n = rd.numel()
    for slot, terms, name in ((OUT, rd * zd, "r.z"), (RR, rd * rd, "r.r")):
        pad = (-n) % 4096
        rows = torch.cat([terms, terms.new_zeros(pad)]).view(-1, 4096).sum(dim=1).cpu().numpy()
        ref = math.fsum(rows.tolist())
        mag = math.fsum(torch.cat([terms.abs(), terms.new_zeros(pad)]).view(-1, 4096)
                        .sum(dim=1).cpu().numpy().tolist())
        got = float(scal1[slot])
        bound = n * EPS * mag
        print(f"{name} (grid-stride): got {got!r} ref {ref!r} |diff| {abs(got - ref):.3e} "
              f"bound {bound:.3e}")
        assert math.isfinite(got) and abs(got - ref) <= bound


def test_entry_points_are_declared():
    """ctypes signatures exist for the new entry points (an undeclared
    function would take its pointer arguments as C ints)."""
    for suf in TYPES:
        for name in ("bdx_pcg_update_iface", "bdx_pcg_update_tiled"):
            f = fn(name, suf)
            assert f.argtypes is not None and f.restype is ctypes.c_int, name
    f = lib().bdx_rt_set_precond
    assert f.argtypes is not None and len(f.argtypes) == 7 and f.restype is ctypes.c_int
