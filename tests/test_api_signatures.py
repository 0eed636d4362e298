"""The ctypes tables of ops/hip_api.py and ops/host_api.py against the two
headers that are the native libraries' C ABI (csrc/include/bdx_hip_api.h,
bdx_host_api.h).  The compiler checks every definition against those headers;
this checks every Python argument list against them, so an entry point cannot
take its int64 arguments as C ints, or a pointer as an int, unnoticed.

CPU only: the headers are preprocessed with g++, no library is loaded.
"""

from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from benchmark_dolfinx_amd.ops import hip_api, host_api

CSRC = Path(hip_api.__file__).resolve().parents[1] / "csrc"

# Entry points that only C++ calls (the native runtime, csrc/hip/runtime.hip):
# they have a prototype and no ctypes row.  Names only; nothing is added here
# to make the test pass.
CXX_ONLY = {
    "hip": {f"{stem}_{suf}" for stem in ("bdx_dofmap_apply_yz", "bdx_dofmap_cg_update_z")
            for suf in ("f64", "f32")},
    "host": set(),
}
LIBS = {"hip": ("bdx_hip_api.h", hip_api.declare), "host": ("bdx_host_api.h", host_api.declare)}

_PROTO = re.compile(r"(?:^|(?<=[;{}]))\s*([^;{}()]*?)\b(bdx_\w+)\s*\(([^()]*)\)\s*;", re.S)
_VALUE_KINDS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long": ctypes.c_long,
                "double": ctypes.c_double, "float": ctypes.c_float,
                "hipStream_t": ctypes.c_void_p, "void": None}


def _kind(ctype: str):
    """ctypes kind of a C type (without a parameter name)."""
    t = " ".join(ctype.replace("*", " * ").split())
    if "*" in t:
        base = t.replace("const", "").replace("*", "").strip()
        if base in hip_api.STRUCTS:  # a record of the ABI: a pointer to its mirror, not void*
            return ctypes.POINTER(hip_api.STRUCTS[base])
        return ctypes.c_char_p if t in ("char *", "const char *") else ctypes.c_void_p
    words = [w for w in t.split() if w != "const"]
    assert len(words) == 1 and words[0] in _VALUE_KINDS, f"unmapped C type {ctype!r}"
    return _VALUE_KINDS[words[0]]


def _param_type(param: str) -> str:
    """The type of one parameter declaration: its name, if any, removed."""
    m = re.fullmatch(r"(.*?)(\w+)", param.strip(), re.S)
    # the last word is the name unless nothing but a qualifier stands before it
    if m and m.group(1).replace("const", "").strip():
        return m.group(1)
    return param.strip()


def _prototypes(header: str) -> dict:
    """{name: (restype kind, [argument kinds])} of every bdx_* prototype."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler to preprocess the header"
    text = subprocess.run([cxx, "-E", "-P", "-x", "c++", "-I", str(CSRC / "include"),
                           str(CSRC / "include" / header)],
                          check=True, capture_output=True, text=True).stdout
    out = {}
    for ret, name, params in _PROTO.findall(text):
        ret = ret.replace('extern "C"', "").strip()
        args = [] if params.strip() in ("", "void") else \
            [_kind(_param_type(p)) for p in params.split(",")]
        assert name not in out, f"{name} declared twice in {header}"
        out[name] = (_kind(ret), args)
    return out


class _Fn:
    argtypes = None
    restype = "unset"


class _Recorder:
    """Stands in for a ctypes library: every name exists, rows are recorded."""

    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.fns.setdefault(name, _Fn())


@pytest.fixture(scope="module", params=sorted(LIBS))
def tables(request):
    header, declare = LIBS[request.param]
    rec = _Recorder()
    declare(rec)
    rows = {n: f for n, f in rec.fns.items() if f.argtypes is not None}
    return request.param, _prototypes(header), rows


def test_headers_declare_the_known_entry_points(tables):
    lib, protos, _ = tables
    assert len(protos) > (100 if lib == "hip" else 30)
    probe = {"hip": ("bdx_rt_create", ctypes.c_void_p, 2), "host": ("bdx_cpu_csr_f32", ctypes.c_int64, 13)}
    name, ret, nargs = probe[lib]
    assert protos[name][0] is ret and len(protos[name][1]) == nargs


def test_every_ctypes_row_is_a_prototype(tables):
    _, protos, rows = tables
    assert sorted(set(rows) - set(protos)) == []


def test_ctypes_rows_match_the_prototypes(tables):
    _, protos, rows = tables
    bad = []
    for name, fn in sorted(rows.items()):
        if name not in protos:
            continue
        ret, args = protos[name]
        if fn.restype is not ret:
            bad.append(f"{name}: restype {fn.restype} != {ret}")
        if len(fn.argtypes) != len(args):
            bad.append(f"{name}: {len(fn.argtypes)} arguments != {len(args)}")
            continue
        bad += [f"{name}: argument {i} is {a}, the header says {b}"
                for i, (a, b) in enumerate(zip(fn.argtypes, args)) if a is not b]
    assert bad == []


def test_every_prototype_has_a_row_or_is_cxx_only(tables):
    lib, protos, rows = tables
    assert CXX_ONLY[lib] <= set(protos)
    assert not CXX_ONLY[lib] & set(rows)
    assert sorted(set(protos) - set(rows) - CXX_ONLY[lib]) == []
    runtime = (CSRC / "hip" / "runtime.hip").read_text()
    for name in CXX_ONLY[lib]:
        assert f"BDX_TWIN(T, {name[:-4]})" in runtime, f"{name} is not called from C++"


def test_per_degree_probes_are_the_headers_degree_lists(tables):
    _, protos, rows = tables

    def per_degree(names):
        return sorted(n for n in names if re.search(r"_p\d", n))
    assert per_degree(rows) == per_degree(protos)
