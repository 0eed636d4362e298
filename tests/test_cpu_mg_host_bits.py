"""The multigrid host twins (csrc/host/bdx_host_mg.cpp: h-transfers, Chebyshev
step, 27-point stencil, V-cycle tail) give, bit for bit, the outputs recorded in
tests/golden/mg_host_bits.npz before their per-node bodies were shared with the
device kernels (csrc/include/bdx_mg_bodies.h).  Cases and inputs:
scripts/record_mg_host_bits.py, which also rewrites the fixture."""

import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import record_mg_host_bits as rec  # noqa: E402

GROUPS = ["hprolong", "hrestrict", "cheb", "stencil27", "tail"]


@functools.lru_cache(maxsize=None)
def _got():
    return dict(rec.cases())


@functools.lru_cache(maxsize=None)
def _want():
    with np.load(rec.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_holds_the_cases_of_the_recorder_and_is_small():
    assert sorted(_want()) == sorted(_got())
    # 2 pairs x 2 ghost settings x 2 variants, 2 x (d, z), 2 levels of 2 meshes, 4 x 2
    count = {"hprolong": 8, "hrestrict": 8, "cheb": 4, "stencil27": 4, "tail": 8}
    for g, n in count.items():
        for sn in rec.DTYPES:
            assert sum(k.startswith(g + "_") and f"_{sn}_" in k + "_" for k in _want()) == n
    # about 8600 lattice values of full entropy at 8 + 4 bytes each: the
    # compressed file cannot go below some 100 KB without dropping a case
    assert os.path.getsize(rec.FIXTURE) < 128 * 1024


@pytest.mark.parametrize("group", GROUPS)
def test_host_twin_bits_are_the_recorded_ones(group):
    keys = [k for k in sorted(_want()) if k.startswith(group + "_")]
    assert keys
    bad = []
    for k in keys:
        got, want = _got()[k], _want()[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert np.isfinite(got).any(), k                       # a case that ran
        if got.tobytes() != want.tobytes():
            diff = got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1)
            bad.append(f"{k}: {int(diff.sum())} bytes differ")
    assert not bad, "\n".join(bad)
