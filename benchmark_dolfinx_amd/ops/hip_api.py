"""ctypes signatures of libbdx_hip.so, one row per prototype of
csrc/include/bdx_hip_api.h (tests/test_api_signatures.py compares the two),
one `ctypes.Structure` per struct of the ABI and one table of its constants
(tests/test_abi_layouts.py compares those with the headers)."""

from __future__ import annotations

import ctypes

vp = ctypes.c_void_p
i32 = ctypes.c_int
i64 = ctypes.c_int64
f64 = ctypes.c_double
f32 = ctypes.c_float

# degrees with a per-degree operator instance (BDX_FUSED_DEGREES / BDX_FUSED5_DEGREES)
FUSED_DEGREES = range(1, 8)
FUSED5_DEGREES = range(3, 8)

# Constants of the headers under their C names (bdx_lattice.h, bdx_pmg_tail.h,
# bdx_rt_setup.h, bdx_hip_api.h).
CONSTANTS = {
    "kLatticeWords": 21,
    "kTailWords": 40, "kTailMaxLevels": 16, "kTailMaxNodes": 32768,
    "kTailS": 21, "kTailDinv": 22, "kTailBc": 23, "kTailR": 24, "kTailZ": 25, "kTailD": 26,
    "kTailY": 27, "kTailCidx": 28, "kTailCw": 29, "kTailFpos": 30, "kTailNcoef": 31,
    "kTailCoef": 32,
    "kBdxTransportNone": 0, "kBdxTransportRccl": 1, "kBdxTransportThread": 2,
    "kBdxTransportEmulated": 3,
    "kFusedModeSegShift": 8,
}


def _ptrs(*names):
    return [(n, vp) for n in names]


def _ints(*names):
    return [(n, i32) for n in names]


class Lattice(ctypes.Structure):
    """BdxLattice: the packed int64 lattice descriptor, word for word."""
    _fields_ = [("n", i64 * 3), ("L", i64 * 3), ("g0", i64 * 3), ("N", i64 * 3), ("gh", i64 * 3),
                ("P", i64), ("ld", i64), ("tsy", i64), ("tsz", i64), ("tntz", i64), ("tcol", i64)]


class TailLevelWords(ctypes.Structure):
    """BdxTailLevelWords: one level of the V-cycle tail's table."""
    _fields_ = [("lat", Lattice)] + [(n, i64) for n in (
        "S", "dinv", "bc", "r", "z", "d", "y", "cidx", "cw", "fpos", "ncoef", "coef")] + [
        ("pad", i64 * (CONSTANTS["kTailWords"] - CONSTANTS["kTailCoef"] - 1))]


_Latd = i64 * CONSTANTS["kLatticeWords"]


class BdxRtHalo(ctypes.Structure):
    _fields_ = _ptrs("buf_a", "buf_b", "face_boxes", "ghost_boxes", "face_cnt", "ghost_cnt") + [
        ("nface_boxes", i32), ("face_total", i64), ("nghost_boxes", i32), ("ghost_total", i64),
        ("transport", i32), ("nranks", i32), ("rank", i32), ("group_id", i64)]


class BdxRtFusedSetup(ctypes.Structure):
    _fields_ = [("latd", _Latd), ("latd_tiled", _Latd), ("own", i64 * 3)] + _ints(
        "is_f64", "version", "affine", "P", "nq", "nblocks", "nty", "ntz", "sy", "sz", "nseg",
        "use_graph", "overlap") + [("kappa", f64)] + _ptrs(
        "wts", "qpts", "tabs", "x", "r", "p_a", "p_b", "y", "yb", "zb", "cb", "xv", "kc", "scal",
        "partials", "upart", "xt", "rt", "pat", "pbt", "yt") + [("halo", BdxRtHalo)]


class BdxRtDofmapSetup(ctypes.Structure):
    _fields_ = [("latd", _Latd)] + _ints(
        "is_f64", "P", "nq", "geom", "n_inner", "n_outer", "use_graph", "overlap") + [
        ("nvec", i64), ("kappa", f64)] + _ptrs(
        "x", "r", "p_a", "p_b", "y", "scal", "partials", "upart", "tab", "inner", "outer", "cdofs",
        "cverts", "coords", "flags", "G", "kc") + [("halo", BdxRtHalo)]


class BdxRtPhases(ctypes.Structure):
    _fields_ = [(n, f64) for n in (
        "halo_fwd", "op_interior", "op_boundary", "halo_rev", "join_rev_add",
        "reduce_allreduce_pap", "update_rr", "allreduce_rr", "iteration",
        # offsets from the iteration start: the comm-stream chain (forward
        # exchange, boundary tiles, reverse send) is hidden when it ends
        # before the interior tiles on the compute stream do
        "t_halo_fwd_done", "t_boundary_done", "t_halo_rev_done", "t_op_interior_done")]


class BdxRtOverlapProbe(ctypes.Structure):
    _fields_ = [(n, f64) for n in (
        "chain_alone_ms", "interior_alone_ms", "chain_done_ms", "interior_done_ms",
        "exchange_alone_ms", "fwd_exchange_done_ms")]


class BdxRtPreflight(ctypes.Structure):
    _fields_ = [("ms", f64), ("allreduce", f64)]


class BdxRtCommPriority(ctypes.Structure):
    _fields_ = _ints("least", "greatest", "comm_stream")


# header struct name -> mirror
STRUCTS = {"BdxLattice": Lattice, "BdxTailLevelWords": TailLevelWords,
           **{c.__name__: c for c in (BdxRtHalo, BdxRtFusedSetup, BdxRtDofmapSetup, BdxRtPhases,
                                      BdxRtOverlapProbe, BdxRtPreflight, BdxRtCommPriority)}}


def fields(rec) -> dict:
    """{field name: value} of a record of scalars, in the struct's order."""
    return {n: getattr(rec, n) for n, _ in rec._fields_}


def _d(lib, name, argtypes, restype=i32):
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    fn.restype = restype


def declare(lib) -> None:
    _d(lib, "bdx_hip_partials_size", [])
    _d(lib, "bdx_device_info", [i32, ctypes.c_char_p, i32])
    _d(lib, "bdx_build_debug", [])
    for suf in ("f64", "f32"):
        _d(lib, f"bdx_dot_{suf}", [i64, i64, i64, i64, i64, vp, vp, vp, vp, i32, vp])
        _d(lib, f"bdx_cg_update_{suf}",
           [i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp])
        _d(lib, f"bdx_p_update_{suf}", [i64, i64, i64, i64, i64, vp, vp, vp, i32, i32, vp])
        _d(lib, f"bdx_pcg_update_{suf}",
           [i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp])
        _d(lib, f"bdx_pcg_p_update_{suf}",
           [i64, i64, i64, i64, i64, vp, vp, vp, vp, i32, i32, vp])
        _d(lib, f"bdx_diag_{suf}",
           [vp, i32, vp, vp, vp, vp, i32, vp, f64, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_axpy_{suf}", [i64, i64, i64, i64, i64, vp, f64, vp, vp, vp])
        _d(lib, f"bdx_cheb_step_{suf}",
           [i64, i64, i64, i64, i64, i32, f64, f64, vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_prolong_{suf}", [vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_restrict_{suf}", [vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_hprolong_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32, vp])
        _d(lib, f"bdx_hrestrict_{suf}", [vp, vp, vp, vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_prolong_row_{suf}", [vp, vp, vp, vp, vp, i32, vp])
        _d(lib, f"bdx_restrict_row_{suf}", [vp, vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_stencil27_apply_{suf}", [vp, vp, vp, vp, vp])
        _d(lib, f"bdx_stencil27_cheb_{suf}", [vp, vp, vp, vp, vp, vp, vp, vp, f64, f64, vp])
        _d(lib, f"bdx_stencil27_assemble_{suf}", [vp, i32, vp, vp, vp, vp, vp, f64, vp, vp, vp])
        _d(lib, f"bdx_pmg_tail_{suf}", [vp, vp, i32, i64, vp, vp, vp])
        _d(lib, f"bdx_box_copy_{suf}", [i32, vp, i64, i64, vp, i32, i64, vp, vp])
        _d(lib, f"bdx_box_copy_lat_{suf}", [i32, vp, vp, vp, i32, i64, vp, vp])
        _d(lib, f"bdx_layout_convert_{suf}", [i32, vp, vp, vp, vp])
        _d(lib, f"bdx_v1_apply_{suf}",
           [i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, f64, vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_geometry_{suf}", [vp, i32, vp, vp, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_dofmap_apply_{suf}",
           [i32, i32, i32, i32, vp, vp, i32, i64, vp, vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp,
            vp, i32, i32, i32, i32, vp, vp, vp])
        _d(lib, f"bdx_dofmap_cg_update_{suf}", [i64, vp, vp, vp, vp, i32, i32, vp, vp, vp])
        _d(lib, f"bdx_dofmap_xflush_{suf}", [i64, vp, vp, vp, i32, i32, vp])
        _d(lib, f"bdx_dofmap_geometry_{suf}", [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp])
        _d(lib, f"bdx_spmv_{suf}", [i64, vp, vp, vp, vp, vp, vp, i32, vp])
        for P in FUSED_DEGREES:
            name = f"bdx_fused_apply_{suf}_p{P}"
            if hasattr(lib, name):
                _d(lib, name, [i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                               vp, vp, vp, vp, f64, vp, vp, i32, i32, i32, i32, vp])
        for P, v in [(P, v) for P in FUSED_DEGREES for v in (2, 3)]:
            if hasattr(lib, f"bdx_fused{v}_segments_{suf}_p{P}"):
                _d(lib, f"bdx_fused{v}_segments_{suf}_p{P}", [i32, i32, i32, i32])
        for P, v in [(P, v) for v in (2, 3) for P in FUSED_DEGREES] + [(P, 5) for P in FUSED5_DEGREES]:
            name = f"bdx_fused{v}_apply_{suf}_p{P}"
            if hasattr(lib, name):
                _d(lib, name, [i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                               vp, vp, f64, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp])
        _d(lib, f"bdx_fused_finalize_{suf}", [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp])
        _d(lib, f"bdx_cg_update_iface_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32,
                                                vp, i32, i32, i32, vp, vp])
        _d(lib, f"bdx_cg_update_tiled_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                                vp, i32, i32, i32, vp, vp])
        _d(lib, f"bdx_pcg_update_iface_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32,
                                                 vp, i32, i32, i32, vp, vp, vp, i32, vp, vp])
        _d(lib, f"bdx_pcg_update_tiled_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                                 vp, i32, i32, i32, vp, vp, vp, i32, vp, vp])
        _d(lib, f"bdx_xflush_{suf}", [vp, vp, vp, vp, vp, i32, i32, vp])
        _d(lib, f"bdx_flush_export_{suf}", [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp])
        _d(lib, f"bdx_fused_tables_{suf}", [i32, i32, vp, vp, vp])
        _d(lib, f"bdx_fused3_tables_{suf}", [i32, i32, vp, vp, vp])
        for P in FUSED5_DEGREES:
            if hasattr(lib, f"bdx_fused5_tables_{suf}_p{P}"):
                _d(lib, f"bdx_fused5_tables_{suf}_p{P}", [i32, i32, vp, vp, vp, vp])
                _d(lib, f"bdx_fused5_tile_p{P}_{suf}", [i32, vp, vp])
                _d(lib, f"bdx_fused5_segments_{suf}_p{P}", [i32, i32, i32])
    # FP64 CG around an FP32 multigrid cycle (mixed.hip)
    _d(lib, "bdx_demote_f64_f32", [i64, i64, i64, i64, i64, vp, vp, vp])
    _d(lib, "bdx_promote_f32_f64", [i64, i64, i64, i64, i64, vp, vp, vp])
    _d(lib, "bdx_cg_update_demote_f64",
       [i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp])
    _d(lib, "bdx_dot_f64_f32", [i64, i64, i64, i64, i64, vp, vp, vp, vp, i32, vp])
    _d(lib, "bdx_p_update_f64_f32", [i64, i64, i64, i64, i64, vp, vp, vp, i32, i32, vp])
    _d(lib, "bdx_fused_tile", [i32, vp, vp])
    # native CG runtime (runtime.hip)
    _d(lib, "bdx_rt_nccl_unique_id", [vp])
    _d(lib, "bdx_rt_rccl_selftest", [vp, i32, vp])
    _d(lib, "bdx_rt_create", [ctypes.POINTER(BdxRtFusedSetup), vp], vp)
    _d(lib, "bdx_rt_create_dofmap", [ctypes.POINTER(BdxRtDofmapSetup), vp], vp)
    _d(lib, "bdx_dofmap_nblocks", [i32, i32])
    _d(lib, "bdx_dofmap_set_mfma", [i32])
    _d(lib, "bdx_dofmap_uses_mfma", [i32, i32])
    _d(lib, "bdx_rt_tiled", [vp])
    _d(lib, "bdx_rt_connect", [vp, vp, i32])
    _d(lib, "bdx_rt_comm_count", [vp])
    _d(lib, "bdx_rt_overlap", [vp])
    _d(lib, "bdx_rt_comm_priority", [vp, ctypes.POINTER(BdxRtCommPriority)])
    _d(lib, "bdx_rt_preflight", [vp, f64, ctypes.POINTER(BdxRtPreflight)])
    _d(lib, "bdx_rt_overlap_probe", [vp, i64, vp, i32, ctypes.POINTER(BdxRtOverlapProbe)])
    _d(lib, "bdx_rt_bind_x", [vp, vp])
    _d(lib, "bdx_rt_set_precond", [vp, vp, vp, vp, vp, vp, i32])
    _d(lib, "bdx_rt_wait", [vp])
    _d(lib, "bdx_rt_profile", [vp, ctypes.c_long, ctypes.POINTER(BdxRtPhases)])
    _d(lib, "bdx_rt_reset", [vp])
    _d(lib, "bdx_rt_iterate", [vp, ctypes.c_long])
    _d(lib, "bdx_rt_iterate_timed", [vp, ctypes.c_long, vp])
    _d(lib, "bdx_rt_state", [vp, vp, vp])
    _d(lib, "bdx_rt_destroy", [vp], None)
    _d(lib, "bdx_rt_release_group", [i64], None)
    _d(lib, "bdx_reduce_partials", [vp, i32, vp, i32, vp])
    _d(lib, "bdx_dofmap_mark_writers", [vp, i32, vp, i32, vp, i32, vp, i64, vp])
