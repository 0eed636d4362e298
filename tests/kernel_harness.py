"""What the tests that drive the vector kernels through their C entry points
share (test_gpu_vector_kernels.py, test_gpu_pcg_update_kernels.py): the
library handle, host <-> device copies, bitwise comparison, and the storage
arrays of a vector_ref.Geom."""

import functools

import numpy as np
import torch

import vector_ref as vr
from benchmark_dolfinx_amd.ops import native

NAN = float("nan")


def lib():
    return native.hip()


def stream():
    return torch.cuda.current_stream().cuda_stream


def fn(name, suf):
    return getattr(lib(), f"{name}_{suf}")


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def assert_same_bits(a, b, what):
    diff = np.flatnonzero(bits(a) != bits(b))
    assert diff.size == 0, f"{what}: {diff.size} elements differ, first at {diff[:8]}"


def store(g, tiled, dense, T, fill=NAN):
    """Storage array of a dense node array (padding = fill)."""
    s = np.full(g.size(tiled), fill, dtype=T)
    s[g.map(tiled)] = dense
    return s


def iface_flat(a, T):
    """An interface buffer as production allocates it: max(1, size) elements."""
    return a.ravel() if a.size else np.full(1, NAN, dtype=T)


def scalars(values):
    """The 8 scalar slots: `values` ({slot: value}) set, every other slot NaN."""
    s = np.full(8, NAN)
    for k, v in values.items():
        s[k] = v
    return s


def new_partials():
    return torch.full((lib().bdx_hip_partials_size(),), NAN, dtype=torch.float64, device="cuda")


@functools.lru_cache(maxsize=None)
def geom(P, tile, n, gh=(0, 0, 0), lower=False):
    return vr.Geom(P, tile, n, gh, lower)
