"""The records and constants of the native libraries' C ABI against their
Python mirrors (ops/hip_api.py: STRUCTS, CONSTANTS): tests/test_api_signatures.py
pins every argument list, this pins what the arguments point to.

* every struct of csrc/include/bdx_rt_setup.h, BdxLattice and
  BdxTailLevelWords: the same field names in the same order (both ways, from
  the preprocessed headers), the same offset and size per field and the same
  total size (from a probe generated out of the mirrors, compiled with g++);
* every entry of CONSTANTS equals the header's value (the same probe);
* LocalLattice.as_int64() is the Lattice mirror filled by name, and the word
  order the tests and device decoders rely on;
* the runtimes' setup checks (bdx_rt_fused_setup_ok, bdx_rt_dofmap_setup_ok)
  through the host library: every refusal, and what is accepted.

CPU only.  The setup records hold made-up addresses; the checkers only compare
them with null, nothing ever dereferences one.
"""

from __future__ import annotations

import ctypes
import re
import shutil
import subprocess

import numpy as np
import pytest

from benchmark_dolfinx_amd.fem.mesh import LocalLattice
from benchmark_dolfinx_amd.ops import hip_api, native
from benchmark_dolfinx_amd.ops.hip_api import (BdxRtDofmapSetup, BdxRtFusedSetup, CONSTANTS,
                                               STRUCTS, Lattice)

from test_api_signatures import CSRC

HEADERS = ("bdx_hip_api.h", "bdx_host_api.h", "bdx_pmg_tail.h")


def _cxx() -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    return cxx


def _struct_fields(text: str) -> dict:
    """{struct name: [field names in order]} of every `struct Bdx...` of the
    preprocessed headers (member functions and nested blocks skipped)."""
    out = {}
    for m in re.finditer(r"\bstruct\s+(Bdx\w+)\s*\{", text):
        depth, i, body = 1, m.end(), []
        while depth:
            c = text[i]
            depth += (c == "{") - (c == "}")
            if depth == 1 and c not in "{}":
                body.append(c)
            elif depth == 2 and c == "{":
                body.append(";")      # a member function's body ends its declaration
            i += 1
        names = []
        for stmt in "".join(body).split(";"):
            if not stmt.strip() or "(" in stmt:
                continue
            for decl in stmt.split(","):
                names.append(re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", decl.strip()).group(1))
        out[m.group(1)] = names
    return out


@pytest.fixture(scope="module")
def header_fields():
    src = "".join(f'#include "{h}"\n' for h in HEADERS)
    text = subprocess.run([_cxx(), "-E", "-P", "-x", "c++", "-std=c++17", "-I",
                           str(CSRC / "include"), "-"], input=src, check=True,
                          capture_output=True, text=True).stdout
    return _struct_fields(text)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """{key: numbers} printed by a C++ program generated from the mirrors:
    `Struct` -> (sizeof,), `Struct.field` -> (offsetof, sizeof), `NAME` ->
    (value,) for every constant."""
    lines = ["#include <cstddef>", "#include <cstdio>"] + [f'#include "{h}"' for h in HEADERS]
    lines.append("int main() {")
    for cname, cls in STRUCTS.items():
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  std::printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), '
                         f"sizeof({cname}::{f}));")
    for name in CONSTANTS:
        lines.append(f'  std::printf("{name} %lld\\n", static_cast<long long>({name}));')
    lines.append("  return 0;\n}")
    d = tmp_path_factory.mktemp("abi_probe")
    (d / "probe.cpp").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_cxx(), "-std=c++17", "-Wno-invalid-offsetof", "-I", str(CSRC / "include"),
                        str(d / "probe.cpp"), "-o", str(d / "probe")],
                       capture_output=True, text=True)
    assert r.returncode == 0, ("a mirror of ops/hip_api.py names what the headers do not have:\n"
                               + r.stderr[-2000:])
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    return {k: tuple(int(v) for v in vs) for k, *vs in (ln.split() for ln in out.splitlines())}


def test_every_abi_struct_has_a_mirror_with_the_same_fields(header_fields):
    assert sorted(header_fields) == sorted(STRUCTS)
    for cname, cls in STRUCTS.items():
        assert [f for f, _ in cls._fields_] == header_fields[cname], \
            f"{cname}: the mirror's fields (left) are not the header's (right)"


def test_mirror_layouts_are_the_compilers(probe):
    bad = []
    for cname, cls in STRUCTS.items():
        if (ctypes.sizeof(cls),) != probe[cname]:
            bad.append(f"{cname}: sizeof {ctypes.sizeof(cls)}, the header's is {probe[cname][0]}")
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            if (d.offset, d.size) != probe[f"{cname}.{f}"]:
                bad.append(f"{cname}.{f}: (offset, size) {(d.offset, d.size)}, the header's is "
                           f"{probe[f'{cname}.{f}']}")
    assert bad == []


def test_result_records_are_doubles_and_ints():
    # runtime.hip divides BdxRtPhases as an array of doubles
    for name in ("BdxRtPhases", "BdxRtOverlapProbe", "BdxRtPreflight"):
        assert all(t is ctypes.c_double for _, t in STRUCTS[name]._fields_)
    assert len(hip_api.BdxRtPhases._fields_) == 13
    assert all(t is ctypes.c_int for _, t in hip_api.BdxRtCommPriority._fields_)


def test_constants_are_the_headers(probe):
    assert {k: (v,) for k, v in CONSTANTS.items()} == {k: probe[k] for k in CONSTANTS}
    for k in ("kLatticeWords", "kTailWords", "kTailMaxNodes", "kTailMaxLevels", "kTailS",
              "kTailCoef", "kBdxTransportNone", "kBdxTransportRccl", "kBdxTransportThread",
              "kBdxTransportEmulated", "kFusedModeSegShift"):
        assert k in CONSTANTS
    assert ctypes.sizeof(Lattice) == 8 * CONSTANTS["kLatticeWords"]
    assert ctypes.sizeof(hip_api.TailLevelWords) == 8 * CONSTANTS["kTailWords"]


# cells (2, 3, 4) at degree 2 on one rank: n, L, g0, N, gh, P, ld, then the tiled words
WORDS = [2, 3, 4, 5, 7, 9, 0, 0, 0, 5, 7, 9, 0, 0, 0, 2, 16]
TILED = {None: [0, 0, 0, 0], (4, 6): [4, 6, 2, 120]}


@pytest.mark.parametrize("tile", list(TILED), ids=["lattice", "tiled"])
def test_as_int64_is_the_lattice_mirror_filled_by_name(tile):
    lat = LocalLattice(0, 1, 2, (2, 3, 4), (1, 1, 1), (0, 0, 0), (0, 0, 0), (2, 3, 4))
    got = lat.as_int64(tile) if tile else lat.as_int64()
    assert got.dtype == np.int64 and got.tolist() == WORDS + TILED[tile]
    m = Lattice()
    m.n[:], m.L[:], m.g0[:], m.N[:], m.gh[:] = lat.n, lat.L, lat.g0, lat.N, lat.gh
    m.P, m.ld = lat.degree, lat.ld
    if tile:
        m.tsy, m.tsz = tile
        m.tntz, m.tcol = (lat.L[2] - 1) // tile[1] + 1, lat.L[0] * tile[0] * tile[1]
    assert bytes(m) == got.tobytes()


# ------------------------------------------------------- the setup checkers
def _filled(cls):
    """A record whose pointers, the halo's included, are made-up non-null
    addresses (never dereferenced)."""
    s = cls()
    for rec in (s, s.halo):
        for name, t in rec._fields_:
            if t is ctypes.c_void_p:
                setattr(rec, name, 0x1000)
    return s


def _fused(tiled: bool, **changes):
    s = _filled(BdxRtFusedSetup)
    s.version, s.sy, s.sz = 5, 4, 6
    if tiled:
        s.latd_tiled[:] = WORDS + TILED[(4, 6)]
    for k, v in changes.items():
        setattr(s, k, v)
    return s


def _dofmap(**changes):
    s = _filled(BdxRtDofmapSetup)
    for k, v in changes.items():
        setattr(s, k, v)
    return s


TILED_BUFS = ("xt", "rt", "pat", "pbt", "yt")


@pytest.mark.parametrize("tiled, changes", [
    (False, {}), (True, {}), (True, {"version": 3}),
    # lattice layout (a tiled descriptor of all zeros): any kernel, no tiled buffers
    (False, {"version": 2, **{b: None for b in TILED_BUFS}}),
    (False, {"kc": None}),
], ids=["lattice", "tiled5", "tiled3", "lattice2_no_tiled_bufs", "no_kc"])
def test_fused_setup_accepted(tiled, changes):
    assert native.host().bdx_cpu_rt_fused_setup_ok(ctypes.byref(_fused(tiled, **changes))) == 1


@pytest.mark.parametrize("tiled, changes", [
    (False, {"tabs": None}), (True, {"tabs": None}),
    (True, {"version": 2}), (True, {"sy": 5}), (True, {"sz": 4}),
    *[(True, {b: None}) for b in TILED_BUFS],
], ids=["no_tabs", "tiled_no_tabs", "tiled_fused2", "tile_sy", "tile_sz",
        *[f"no_{b}" for b in TILED_BUFS]])
def test_fused_setup_refused(tiled, changes):
    assert native.host().bdx_cpu_rt_fused_setup_ok(ctypes.byref(_fused(tiled, **changes))) == 0


@pytest.mark.parametrize("changes, ok", [
    ({}, 1), ({"geom": 1, "G": None}, 1), ({"kc": None, "inner": None, "outer": None}, 1),
    ({"tab": None}, 0), ({"cdofs": None}, 0), ({"flags": None}, 0), ({"geom": 0, "G": None}, 0),
], ids=["filled", "otf_no_G", "no_kc_no_cells", "no_tab", "no_cdofs", "no_flags", "stored_no_G"])
def test_dofmap_setup_checked(changes, ok):
    assert native.host().bdx_cpu_rt_dofmap_setup_ok(ctypes.byref(_dofmap(**changes))) == ok
