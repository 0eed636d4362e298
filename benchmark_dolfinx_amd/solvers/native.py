"""Python handle of the native C++ CG runtime (csrc/hip/runtime.hip).

After the CG prologue (r0 = b - A x0, rho0 = r0.r0; FusedLaplacianGPU.cg_start)
the whole iteration loop -- halo exchange, fused operator, reductions,
all-reduces, r/x updates -- runs in C++ on the current HIP stream, with the
steady-state iterations replayed from hipGraphs.  Transport:

* ``rccl``   one process per GPU (torchrun or bench.py's own launcher); the
  runtime opens its own RCCL communicator, bootstrapped by exchanging an
  ncclUniqueId over the existing torch.distributed group, and exchanges halos
  with grouped ncclSend/ncclRecv to the neighbours only, on a second stream
  overlapped with the interior tiles of the operator;
* ``thread`` ranks are threads of one process on one GPU (ThreadComm tests);
* single rank: no communication.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from ..ops import hip_api, native
from ..ops.kernels import _check, _stream
from ..ops.native import ptr


PHASES = tuple(n for n, _ in hip_api.BdxRtPhases._fields_)
TRANSPORTS = {"none": hip_api.CONSTANTS["kBdxTransportNone"],
              "rccl": hip_api.CONSTANTS["kBdxTransportRccl"],
              "thread": hip_api.CONSTANTS["kBdxTransportThread"],
              "emulated": hip_api.CONSTANTS["kBdxTransportEmulated"]}


def _agree(comm, ok: bool) -> bool:
    """True iff every rank reports ok (a MIN all-reduce over the torch group)."""
    if comm.size == 1:
        return ok
    return comm.allreduce_scalar(1.0 if ok else 0.0, "min") > 0.5


class NativeCGRuntime:
    """Handle of one rank's native CG loop.

    Construction is collective and all-or-nothing: every rank first builds
    its runtime locally (no communication), the ranks agree that all
    succeeded, then the RCCL communicator is opened (bounded by the
    watchdog deadline) and the ranks agree again.  If any rank fails at
    either step every rank releases its handle and raises
    NativeRuntimeUnavailable, so all ranks take the same fallback (a rank
    on native RCCL calls and a rank on torch collectives would never match).
    """

    # test hook: rank whose local creation is made to fail
    _inject_fail_rank: int | None = None

    def __init__(self, op, cg, use_graph: bool | None = None, overlap: bool | None = None):
        pb = op.pb
        self.op, self.cg, self.pb = op, cg, pb
        self.lib = native.hip()
        self.h = None
        comm = pb.comm
        halo = pb.halo
        if use_graph is None:
            # BDX_GRAPH=0 (default) eager launches at every rank count, 1 graph
            # replay on a single rank, 2 also with RCCL (the two-stream
            # fork/join iteration captures RCCL calls).  One launch mode for
            # every N keeps the weak-scaling points comparable; at N = 1 graph
            # replay and eager launches measured equal (60.12 vs 60.17 GDoF/s
            # same box, profiles/r3_graph_ab.md): the host runs far ahead of
            # a 5 ms iteration, so launch overhead is hidden either way.
            mode = os.environ.get("BDX_GRAPH", "0")
            use_graph = mode == "2" or (mode == "1" and comm.size == 1)
        if overlap is None:
            overlap = os.environ.get("BDX_OVERLAP", "1") != "0"
        self.kind = "dofmap" if getattr(op, "name", "") == "dofmap" else "fused"
        self.group = 0
        if comm.size == 1:
            self.transport = "none"
        elif hasattr(comm, "g"):  # ThreadComm: ranks are threads of this process
            self.transport = "thread"
            self.group = comm.g.uid  # unique per group: a reused id() could
            # pick up a stale group of a runtime that was not closed yet
        elif comm.backend == "nccl":
            self.transport = "rccl"
        elif comm.backend == "emulated":  # EmulatedRankComm: modelled links
            self.transport = "emulated"
            halo.buf_a.zero_()  # the emulated copies move finite data only
            halo.buf_b.zero_()
        else:
            self.transport = "unsupported"
        self.upart = torch.zeros(self.lib.bdx_hip_partials_size(), dtype=torch.float64,
                                 device=pb.device)
        self.x = cg.x
        self._keep = []  # the tensors and arrays a setup record points to
        ok = self.transport in TRANSPORTS and comm.rank != self._inject_fail_rank
        if self.kind == "dofmap":
            ok = ok and self._create_dofmap(op, cg, use_graph, overlap)
        else:
            ok = ok and self._create_fused(op, cg, use_graph, overlap)
        self._connect(comm, ok)

    def _p(self, buf) -> int:
        """The address of `buf` for a setup record; `buf` is kept alive."""
        self._keep.append(buf)
        return ptr(buf)

    def _fill_common(self, s, cg, use_graph, overlap) -> None:
        """What both setup records share: the descriptor, the flags, the CG
        buffers and the halo record."""
        pb, halo = self.pb, self.pb.halo
        s.latd[:] = [int(v) for v in pb.latd]
        s.is_f64 = int(pb.dtype == torch.float64)
        s.use_graph, s.overlap = int(use_graph), int(overlap)
        s.kappa = float(pb.kappa)
        s.x = self._p(cg.x)  # the first one kept: bind_x replaces it
        s.r, s.y, s.scal = self._p(cg.r), self._p(cg.y), self._p(cg.scal)
        s.upart = self._p(self.upart)
        fo, gh, h = halo.owned_faces, halo.ghosts, s.halo
        h.buf_a, h.buf_b = self._p(halo.buf_a), self._p(halo.buf_b)
        h.face_boxes, h.ghost_boxes = self._p(fo.table), self._p(gh.table)
        h.face_cnt = self._p(np.array(fo.counts, dtype=np.int64))
        h.ghost_cnt = self._p(np.array(gh.counts, dtype=np.int64))
        h.nface_boxes, h.face_total = len(fo.boxes), int(fo.total)
        h.nghost_boxes, h.ghost_total = len(gh.boxes), int(gh.total)
        h.transport = TRANSPORTS[self.transport]
        h.nranks, h.rank, h.group_id = pb.comm.size, pb.comm.rank, self.group

    def _create_dofmap(self, op, cg, use_graph, overlap) -> bool:
        """The dofmap data model's loop (runtime.hip DofCGRuntime)."""
        pb = self.pb
        self.tiled = False
        s = hip_api.BdxRtDofmapSetup()
        self._fill_common(s, cg, use_graph, overlap)
        s.P, s.nq, s.geom = pb.degree, pb.tables.nq, op.geom
        s.n_inner, s.n_outer = int(op.inner.numel()), int(op.outer.numel())
        s.nvec = int(cg.r.numel())
        s.p_a, s.p_b, s.partials = self._p(op.p_a), self._p(op.p_b), self._p(cg.partials)
        s.tab = self._p(op.tab)
        s.inner, s.outer = self._p(op.inner), self._p(op.outer)
        s.cdofs, s.cverts = self._p(op.cdofs), self._p(op.cverts)
        s.coords, s.flags = self._p(op.coords), self._p(op.flags)
        s.G, s.kc = self._p(op.G), self._p(op.kc)
        self.h = self.lib.bdx_rt_create_dofmap(ctypes.byref(s), _stream())
        return bool(self.h)

    def _create_fused(self, op, cg, use_graph, overlap) -> bool:
        pb = self.pb
        t = op.t
        s = hip_api.BdxRtFusedSetup()
        self._fill_common(s, cg, use_graph, overlap)
        s.own[:] = [int(v) for v in pb.lat.owned_hi]
        s.version, s.affine, s.P, s.nq = op.version, op.affine_code, pb.degree, t.nq
        s.nblocks, s.nseg = op.nblocks, op.nseg
        s.nty, s.ntz, s.sy, s.sz = op.nty, op.ntz, op.sy, op.sz
        s.wts = self._p(np.ascontiguousarray(t.wts, dtype=np.float64))
        s.qpts = self._p(np.ascontiguousarray(t.qpts, dtype=np.float64))
        # Tiled vector storage for the x-march kernels: each (y, z) tile's
        # patch of an x-plane is contiguous, so the kernels' writes are whole
        # lines (profiles/r2_march_bw.md).  BDX_TILED=0: the lattice layout;
        # 1 (default): fused5 and fused3's x-trilinear instance
        # (perturbed Q3 +2 %, Q6 +3 %, Q6 FP32 +5 %, profiles/r2_xtrilinear.md);
        # 2: every fused3 instance (the general-geometry kernel is
        # compute-bound: Q3 +0.6 %, Q6 -2.4 % on tiled storage,
        # profiles/r2_launder.md).  The tiled r update needs 16-byte tile
        # planes.
        mode = os.environ.get("BDX_TILED", "1")
        esz = 8 if pb.dtype == torch.float64 else 4
        f3 = op.version == 3 and (mode == "2" or getattr(op, "x_trilinear", False))
        self.tiled = (mode != "0" and (op.version == 5 or f3)
                      and (op.sy * op.sz * esz) % 16 == 0)
        if self.tiled:  # zeroed: the padding of the tiled vectors stays zero
            s.latd_tiled[:] = [int(v) for v in pb.lat.as_int64((op.sy, op.sz))]
            n = pb.lat.tiled_size(op.sy, op.sz)
            s.xt, s.rt, s.pat, s.pbt, s.yt = (
                self._p(torch.zeros(n, dtype=pb.dtype, device=pb.device)) for _ in range(5))
        s.tabs = self._p(op.tabs)
        s.p_a, s.p_b, s.partials = self._p(op.p_old), self._p(op.p_new), self._p(op.partials)
        s.yb, s.zb, s.cb = self._p(op.yb), self._p(op.zb), self._p(op.cb)
        s.xv, s.kc = self._p(pb.xv), self._p(pb.kc)
        self.h = self.lib.bdx_rt_create(ctypes.byref(s), _stream())
        return bool(self.h)

    def _connect(self, comm, ok: bool) -> None:
        """1) every rank created its runtime locally (no communication): agree;
        2) open the RCCL communicator (ncclUniqueId from rank 0 over the torch
        group), bounded by the watchdog deadline: agree again."""
        if not _agree(comm, ok):
            self.close()
            raise NativeRuntimeUnavailable(
                "bdx_rt_create failed on at least one rank (unsupported kernel, no transport "
                f"for backend {comm.backend!r}, or an injected failure)")
        # 2) open the runtime's own RCCL communicator (ncclUniqueId from rank 0
        #    over the torch group); bounded by the watchdog deadline
        if self.transport == "rccl":
            uid = (ctypes.c_char * 128)()
            good = True
            if comm.rank == 0:
                good = self.lib.bdx_rt_nccl_unique_id(uid) > 0
            ids = comm.gather_objects(bytes(uid) if (comm.rank == 0 and good) else None)
            if ids[0] is None:
                self.close()
                raise NativeRuntimeUnavailable("ncclGetUniqueId failed on rank 0")
            ctypes.memmove(uid, ids[0], 128)
            ok = self.lib.bdx_rt_connect(self.h, uid, comm.rank) == 0
            if not _agree(comm, ok):
                self.close()
                raise NativeRuntimeUnavailable("ncclCommInitRank failed on at least one rank")
        self.overlap = bool(self.lib.bdx_rt_overlap(self.h))
        self.tiled = bool(self.lib.bdx_rt_tiled(self.h))
        self.graphs = False

    def comm_priority(self) -> dict:
        """Priority of the comm stream and the device's range (HIP: a lower
        value is a higher priority)."""
        out = hip_api.BdxRtCommPriority()
        _check(self.lib.bdx_rt_comm_priority(self.h, ctypes.byref(out)), "rt_comm_priority")
        return hip_api.fields(out)

    def preflight(self, timeout_s: float = 60.0) -> dict:
        """One forward halo exchange and a device all-reduce of (rank + 1),
        bounded by `timeout_s`: raises if a peer never joins or the sum is
        wrong (every rank must call it)."""
        out = hip_api.BdxRtPreflight()
        _check(self.lib.bdx_rt_preflight(self.h, float(timeout_s), ctypes.byref(out)),
               "rt_preflight")
        n = self.pb.comm.size
        want = n * (n + 1) / 2
        if out.allreduce != want:
            raise RuntimeError(f"pre-flight all-reduce returned {out.allreduce}, expected {want}")
        return hip_api.fields(out)

    def overlap_probe(self, n: int, reps: int = 5) -> dict:
        """One-rank probe of the split schedule (runtime.hip overlap_probe):
        an RCCL self send/recv of n doubles, the boundary tiles and a second
        send/recv on the comm stream under the interior tiles.  Clobbers the
        CG state (restart CG afterwards)."""
        buf = torch.zeros(2 * int(n), dtype=torch.float64, device=self.pb.device)
        buf[:n] = torch.arange(n, dtype=torch.float64, device=self.pb.device)
        out = hip_api.BdxRtOverlapProbe()
        torch.cuda.synchronize()
        _check(self.lib.bdx_rt_overlap_probe(self.h, int(n), ptr(buf), int(reps),
                                             ctypes.byref(out)), "rt_overlap_probe")
        torch.cuda.synchronize()
        rec = hip_api.fields(out)
        rec["exchange_ok"] = bool(torch.equal(buf[n:], buf[:n]))
        rec["bytes"] = int(n) * 8
        return rec

    def comm_ranks(self) -> int:
        """Ranks of the runtime's own communicator (ncclCommCount for RCCL)."""
        return int(self.lib.bdx_rt_comm_count(self.h))

    def bind_x(self, x: torch.Tensor) -> None:
        """Point the runtime at a new iterate (drops the captured graphs)."""
        if x.data_ptr() != self.x.data_ptr():
            _check(self.lib.bdx_rt_bind_x(self.h, ptr(x)), "rt_bind_x")
            self.x = x
            self._keep[0] = x

    def set_precond(self, dinv: torch.Tensor, z: torch.Tensor, partials_rr: torch.Tensor,
                    rr_slot: int) -> None:
        """Bind the Jacobi preconditioner (fused operators): the loop then
        feeds the operator and the forward halo with z = dinv . r, stores z in
        the update pass, keeps r.z in the r.r slots and the plain r.r in
        scalar slot `rr_slot`.  z holds dinv . r0 when the iterations start
        (FusedLaplacianGPU.cg_start).  Drops the captured graphs."""
        if self.kind != "fused":
            raise ValueError("the dofmap runtime has no preconditioned loop")
        pb = self.pb
        tb = [None, None]
        if self.tiled:  # zeroed: the padding of the tiled z stays zero
            n = pb.lat.tiled_size(self.op.sy, self.op.sz)
            tb = [torch.zeros(n, dtype=pb.dtype, device=pb.device) for _ in range(2)]
        self._keep += [dinv, z, partials_rr] + tb
        _check(self.lib.bdx_rt_set_precond(self.h, ptr(dinv), ptr(z), ptr(tb[0]), ptr(tb[1]),
                                           ptr(partials_rr), int(rr_slot)), "rt_set_precond")

    def reset(self) -> None:
        _check(self.lib.bdx_rt_reset(self.h), "rt_reset")

    def _sync_state(self) -> None:
        it, graphs = ctypes.c_long(0), ctypes.c_int(0)
        self.lib.bdx_rt_state(self.h, ctypes.byref(it), ctypes.byref(graphs))
        self.cg.it = it.value
        self.graphs = bool(graphs.value)

    def iterate(self, n: int) -> None:
        _check(self.lib.bdx_rt_iterate(self.h, int(n)), "rt_iterate")
        self._sync_state()

    def iterate_timed(self, n: int) -> list[float]:
        """iterate(n) and return the device time (ms) of each step, from
        timing events recorded between the steps (waits for the steps)."""
        out = (ctypes.c_float * max(1, int(n)))()
        _check(self.lib.bdx_rt_iterate_timed(self.h, int(n), out), "rt_iterate_timed")
        self._sync_state()
        return [float(v) for v in out[:int(n)]]

    def wait(self) -> None:
        """Host wait for the queued iterations, bounded by the RCCL deadline
        (BDX_RCCL_TIMEOUT_S): a hung peer raises instead of blocking forever."""
        _check(self.lib.bdx_rt_wait(self.h), "rt_wait")

    def profile(self, n: int) -> dict:
        """n eager iterations with hipEvent phase timers -> mean ms per phase."""
        out = hip_api.BdxRtPhases()
        _check(self.lib.bdx_rt_profile(self.h, int(n), ctypes.byref(out)), "rt_profile")
        self._sync_state()
        ph = hip_api.fields(out)
        # meaningful only for the split (two-stream) schedule
        split = self.overlap
        ph["halo_fwd_hidden"] = (ph["t_halo_fwd_done"] <= ph["t_op_interior_done"]) if split else None
        ph["halo_rev_hidden"] = (ph["t_halo_rev_done"] <= ph["t_op_interior_done"]) if split else None
        return ph

    def close(self) -> None:
        if getattr(self, "h", None):
            # bounded by the RCCL deadline (a hung peer must not block the
            # teardown forever), then the device for the caller's stream
            rc = self.lib.bdx_rt_wait(self.h)
            if rc == 0:
                torch.cuda.synchronize()
            self.lib.bdx_rt_destroy(self.h)
            self.h = None
        if getattr(self, "group", 0):
            self.lib.bdx_rt_release_group(self.group)
            self.group = 0

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


class NativeRuntimeUnavailable(RuntimeError):
    """Raised on every rank when the native runtime cannot run on all ranks."""
