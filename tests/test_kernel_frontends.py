"""The two kernel front-ends of ops/kernels.py: `HipKernels` (libbdx_hip.so)
and `HostKernels` (libbdx_host.so) offer the platform-neutral kernels under the
same names with the same parameters, a problem has exactly one of them
(`PoissonProblem.kernels`, shared with its halo exchange and its multigrid
levels), and nothing outside ops/ chooses the host library by itself.

CPU only.  The device front-end's results are held to the same references as
the host's by the GPU suite (test_gpu_kernels.py, test_gpu_diagonal.py,
test_gpu_pmg*.py, operator_ref.check_rhs).
"""

from __future__ import annotations

import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import benchmark_dolfinx_amd
from benchmark_dolfinx_amd.fem.mesh import make_local_lattice
from benchmark_dolfinx_amd.models.poisson import PoissonProblem
from benchmark_dolfinx_amd.ops.kernels import HipKernels, HostKernels
from benchmark_dolfinx_amd.parallel.comm import Comm
from benchmark_dolfinx_amd.parallel.halo import _Side
from benchmark_dolfinx_amd.solvers.pmg import PMultigrid

SHARED = ["v1_apply", "diagonal", "geometry", "spmv", "box_copy", "axpy",
          "cheb_step", "prolong", "restrict", "prolong_row", "restrict_row", "hprolong", "hrestrict",
          "stencil27_apply", "stencil27_cheb", "stencil27_assemble", "pmg_tail", "demote", "promote"]


@pytest.mark.parametrize("name", SHARED)
def test_same_surface(name):
    """A kernel added to one front-end only, or with other parameters, fails here."""
    hip, host = (list(inspect.signature(getattr(cls, name)).parameters)
                 for cls in (HipKernels, HostKernels))
    assert hip == host


def test_one_frontend_per_problem():
    pb = PoissonProblem(Comm(), (1, 1, 1), 1, 1, False, torch.float64, "cpu")
    assert isinstance(pb.kernels, HostKernels)
    assert pb.halo.kernels is pb.kernels
    assert PMultigrid(pb).levels[0].k is pb.kernels


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# rank 0 of 2 has the ghost plane; the owned face that fills it is rank 1's
@pytest.mark.parametrize("rank,side", [(0, "ghosts"), (1, "owned_faces")])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_host_box_copy_against_numpy(dt, rank, side):
    """(2, 2, 2) cells at degree 2 on 2 ranks, `xyz` partition: a lattice of
    (3, 5, 5) nodes stored as (3, 5, 16), one plane of 25 nodes exchanged.
    Every comparison is bitwise: modes 0 and 1 copy, mode 2 is one IEEE
    addition per entry (the box's indices are distinct)."""
    lat = make_local_lattice(rank, 2, (2, 2, 2), 2, whole_x=False)
    boxes = lat.halo_recv_boxes() if side == "ghosts" else lat.halo_send_boxes()
    assert len(boxes) == 1 and lat.ld > lat.L[2]
    s = _Side(boxes, 2, lat, "cpu")
    k = HostKernels(lat, dt)
    # the box's storage indices in table order, by numpy alone
    b = boxes[0]
    ijk = np.mgrid[tuple(slice(l, h) for l, h in zip(b.lo, b.hi))].reshape(3, -1)
    idx = np.ravel_multi_index(ijk, lat.shape)
    assert idx.size == s.total == 25

    rng = np.random.default_rng(3)
    npdt = np.float64 if dt == torch.float64 else np.float32
    v0 = np.full(lat.shape, np.nan, dtype=npdt)
    v0[:, :, : lat.L[2]] = rng.standard_normal(lat.L)
    sent = rng.standard_normal(s.total + 3).astype(npdt)   # 3 slots past the box's data

    buf = torch.from_numpy(sent.copy())
    vec = torch.from_numpy(v0.copy())
    k.box_copy(0, vec, lat, s, buf)
    want = sent.copy()
    want[: s.total] = v0.ravel()[idx]
    assert np.array_equal(_bits(buf.numpy()), _bits(want))
    assert np.array_equal(_bits(vec.numpy()), _bits(v0))

    for mode in (1, 2):
        vec = torch.from_numpy(v0.copy())
        buf = torch.from_numpy(sent.copy())
        k.box_copy(mode, vec, lat, s, buf)
        want = v0.copy().ravel()
        want[idx] = sent[: s.total] if mode == 1 else want[idx] + sent[: s.total]
        assert np.array_equal(_bits(vec.numpy().ravel()), _bits(want))   # NaN padding included
        assert np.array_equal(_bits(buf.numpy()), _bits(sent))


def test_no_other_chooser_of_the_host_library():
    pkg = Path(benchmark_dolfinx_amd.__file__).resolve().parent
    naming = {pkg / "ops" / n for n in ("kernels.py", "native.py", "host_api.py")}
    files = sorted(pkg.rglob("*.py"))
    assert naming <= set(files)
    bad = []
    for f in files:
        text = f.read_text()
        if f not in naming and "bdx_cpu_" in text:
            bad.append(f"{f.relative_to(pkg)} names a host entry point")
        if f.parent != pkg / "ops" and "native.host(" in text:
            bad.append(f"{f.relative_to(pkg)} loads the host library itself")
    assert bad == []
