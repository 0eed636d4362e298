"""ctypes signatures of libbdx_host.so, one row per prototype of
csrc/include/bdx_host_api.h (tests/test_api_signatures.py compares the two)."""

from __future__ import annotations

import ctypes

from .hip_api import BdxRtDofmapSetup, BdxRtFusedSetup

vp = ctypes.c_void_p
i32 = ctypes.c_int
i64 = ctypes.c_int64
f64 = ctypes.c_double
f32 = ctypes.c_float


def _d(lib, name, argtypes, restype=None):
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    fn.restype = restype


def declare(lib) -> None:
    _d(lib, "bdx_host_version", [], i32)
    _d(lib, "bdx_cpu_rt_fused_setup_ok", [ctypes.POINTER(BdxRtFusedSetup)], i32)
    _d(lib, "bdx_cpu_rt_dofmap_setup_ok", [ctypes.POINTER(BdxRtDofmapSetup)], i32)
    _d(lib, "bdx_watchdog_selftest", [f64, f64, f64, vp, vp], i32)
    for suf, ft in (("f64", f64), ("f32", f32)):
        _d(lib, f"bdx_cpu_stiffness_{suf}",
           [vp, i32, vp, vp, vp, vp, vp, i32, vp, ft, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_stiffness_g_{suf}",
           [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, ft, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_geometry_{suf}", [vp, i32, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_dofmap_{suf}",
           [i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, ft, vp, vp, vp])
        _d(lib, f"bdx_cpu_dofmap_geometry_{suf}", [i32, i32, vp, vp, i32, vp, vp, vp])
        _d(lib, f"bdx_cpu_mass_{suf}", [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_diag_{suf}", [vp, i32, vp, vp, vp, vp, vp, ft, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_csr_{suf}", [vp, i32, vp, vp, vp, vp, vp, ft, vp, vp, vp, vp, i32], i64)
        _d(lib, f"bdx_cpu_spmv_{suf}", [i64, vp, vp, vp, vp, vp, vp, i32])
        _d(lib, f"bdx_cpu_interp_f_{suf}", [vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_prolong_{suf}", [vp, vp, vp, vp, vp], i32)
        _d(lib, f"bdx_cpu_restrict_{suf}", [vp, vp, vp, vp, vp], i32)
        _d(lib, f"bdx_cpu_hprolong_{suf}", [vp, vp, vp, vp, vp, vp, vp, i32], i32)
        _d(lib, f"bdx_cpu_hrestrict_{suf}", [vp, vp, vp, vp, vp, vp, vp, vp], i32)
        _d(lib, f"bdx_cpu_prolong_row_{suf}", [vp, vp, vp, vp, vp, i32], i32)
        _d(lib, f"bdx_cpu_restrict_row_{suf}", [vp, vp, vp, vp, vp, vp], i32)
        _d(lib, f"bdx_cpu_cheb_step_{suf}",
           [i64, i64, i64, i64, i64, i32, f64, f64, vp, vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_pmg_tail_{suf}", [vp, i32, i64, vp, vp], i32)
        _d(lib, f"bdx_cpu_stencil27_{suf}", [vp, vp, vp, vp])
        _d(lib, f"bdx_cpu_stencil27_cheb_{suf}", [vp, vp, vp, vp, vp, vp, vp, vp, f64, f64], i32)
        _d(lib, f"bdx_cpu_stencil27_assemble_{suf}", [vp, i32, vp, vp, vp, vp, vp, f64, vp, vp], i32)
    # the precision boundary of the mixed multigrid solve
    _d(lib, "bdx_cpu_demote_f64_f32", [i64, i64, i64, i64, i64, vp, vp])
    _d(lib, "bdx_cpu_promote_f32_f64", [i64, i64, i64, i64, i64, vp, vp])
