"""Conjugate gradients (reference: `cg_solve`, src/cg.hpp:89-169), unpreconditioned
by default, optionally Jacobi-preconditioned with the matrix-free diagonal
(`cg_solve(..., dinv=...)`, `DeviceCG(pb, precond="jacobi")`) or with any
symmetric positive definite M^-1 given as a callable (`cg_solve(...,
precond=...)`), such as the p-multigrid V-cycle of solvers/pmg.py
(`DeviceCG(pb, precond="pmg")`).

Two implementations with the reference's algorithm (x0 given, r0 = b - A x0,
p0 = z0 = M^-1 r0, rtol = 0 runs exactly max_iter iterations).  Each holds the
recurrence once; a preconditioner only changes how z and rho = r.z are formed:

* `cg_solve`: generic, host scalars (used by the CPU platform and the CSR
  comparison path).  z = M^-1 r comes from one callable; without a
  preconditioner z is r itself.
* `DeviceCG` (`cg_solve_device`): GPU, every scalar stays on the device.  Per
  iteration the common head, apply (+ halo), dot(p, y) -> all-reduce, then the
  preconditioner's tail: {x += a p; r -= a y; r.r}, z, rho = r.z ->
  all-reduce, p = b p + z (unpreconditioned: the fused cg_update, then
  p_update).  alpha/beta are formed inside the kernels from float64 device
  slots, ping-ponging the rho slot between iterations (`DeviceCG.slots`) so no
  kernel reads a slot another kernel of the same iteration writes.  One halo
  exchange per iteration (the reference does two, quirk Q2) and no host
  synchronisation (quirk Q3).

When the operator provides `cg_start` / `cg_iterate` (the fused structured
kernel, models/fused.py) the device loop delegates to it.  The preconditioned
solve does so only on request (`loop="fused"`): the fused kernels then run
with u = z = dinv . r, r.z in the r.r slots, and an update pass that also
stores z (csrc/hip/cg_update.hip).
"""

from __future__ import annotations

import torch


def cg_solve(op, pb, x: torch.Tensor, b: torch.Tensor, max_iter: int,
             rtol: float = 0.0, dinv: torch.Tensor | None = None, precond=None) -> int:
    """`dinv` (lattice-shaped 1 / diag(A), `PoissonProblem.jacobi_inverse`):
    Jacobi-preconditioned CG; `precond`: a callable `precond(r, z)` that
    writes z = M^-1 r (e.g. `PMultigrid.apply`); neither: the unpreconditioned
    algorithm.  Standard PCG: beta = r.z (new) / r.z (old), stop test on r.r
    (the reference's hook for the diagonal: MatrixOperator::get_diag_inverse,
    src/csr.hpp:81-106)."""
    if dinv is not None and precond is not None:
        raise ValueError("give dinv or precond, not both")
    if dinv is not None:
        def precond(r, z):
            torch.mul(dinv, r, out=z)
    r = pb.new_vector()
    y = pb.new_vector()
    op.apply(x, y)
    r.copy_(b - y)
    # unpreconditioned: z is r, so r.z is the r.r of the stop test
    z = r if precond is None else pb.new_vector()
    if precond is not None:
        precond(r, z)
    p = z.clone()
    rz = pb.inner(r, z)
    rtol2 = rtol * rtol
    if precond is None:
        rnorm0 = rz
    else:
        rnorm0 = pb.inner(r, r) if rtol2 > 0 else 0.0
    k = 0
    while k < max_iter:
        k += 1
        op.apply(p, y)
        alpha = rz / pb.inner(p, y)
        x.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        if precond is not None:
            precond(r, z)
        rz_new = pb.inner(r, z)
        beta = rz_new / rz
        rz = rz_new
        if rnorm0 > 0:
            rnorm = rz if precond is None else pb.inner(r, r)
            if rnorm / rnorm0 < rtol2:
                break
        p.mul_(beta).add_(z)
    return k


class DeviceCG:
    """Device-resident CG state for the GPU platform.

    One prologue and one loop (`start`, `iterate`); the preconditioner picks,
    once in `__init__`, the pair of methods that form the first direction and
    the tail of an iteration (`_first_*`, `_tail_*`).

    precond="jacobi": Jacobi-preconditioned CG with the problem's matrix-free
    diagonal.  loop="generic" (default) runs op.apply + dot + pcg_update +
    pcg_p_update (z = dinv . r never stored), also for operators that offer a
    fused `cg_start` / `cg_iterate`.  loop="fused" (precond="jacobi" only)
    delegates to the operator's fused CG loop and its native runtime
    (fused2/3/5); an operator without it raises ValueError in `start`.

    precond="pmg": CG preconditioned with a p-multigrid V-cycle (`pmg`: a
    `PMultigrid` of the problem; None builds the default one).  Generic loop
    only, composed of existing kernels: op.apply, dot, cg_update (r.r into
    RNORM), `pmg.apply(r, z)` with z stored here, dot(r, z), p_update.

    With a mixed-precision `pmg` (`pmg.mixed`: FP32 cycle, FP64 problem) the
    boundary between the precisions is fused into the loop's own passes
    (csrc/hip/mixed.hip): cg_update_demote also stores the residual as FP32
    into `pmg.rc`, `pmg.apply_cycle(pmg.rc, pmg.zc)` runs the raw cycle, and
    dot_f64_f32 / p_update_f64_f32 read the FP32 `pmg.zc`, so no FP64 z is
    allocated."""

    # float64 scalar slots
    RR0, RR1, PAP = 0, 1, 2
    # preconditioned: RR0 / RR1 carry r.z, RNORM the plain r.r; ZERO / ONE give
    # the Jacobi prologue's beta = 0 (slots 3, 4: the fused kernels' lagged alphas)
    RNORM, ZERO, ONE = 5, 6, 7

    def __init__(self, pb, precond: str | None = None, loop: str = "generic", pmg=None):
        if precond not in (None, "jacobi", "pmg"):
            raise ValueError(f"unknown preconditioner {precond!r}")
        if loop not in ("generic", "fused"):
            raise ValueError(f"unknown loop {loop!r}")
        if loop == "fused" and precond != "jacobi":
            raise ValueError("loop='fused' selects the loop of the preconditioned solve: it "
                             "needs precond='jacobi'")
        if pmg is not None and precond != "pmg":
            raise ValueError("pmg= needs precond='pmg'")
        self.loop = loop
        self.dinv = pb.jacobi_inverse() if precond == "jacobi" else None
        self.pmg = None
        if precond == "pmg":
            from .pmg import PMultigrid
            self.pmg = pmg if pmg is not None else PMultigrid(pb)
        # fused loop: z = dinv . r and the r.r block partials (allocated by
        # the operator's cg_start)
        self.z = None
        self.partials_rr = None
        self.pb = pb
        self.k = pb.kernels
        dev = pb.device
        self.scal = torch.zeros(8, dtype=torch.float64, device=dev)
        if precond == "jacobi":
            self.scal[self.ONE] = 1.0
        self.partials = torch.zeros(self.k.npart, dtype=torch.float64, device=dev)
        self.r = pb.new_vector()
        self.y = pb.new_vector()
        # FP32 cycle under this FP64 loop: z lives in the preconditioner (pmg.zc)
        self.mixed = self.pmg is not None and bool(getattr(self.pmg, "mixed", False))
        if self.pmg is not None and not self.mixed:
            self.z = pb.new_vector()
        # the fused loop keeps its search directions in the operator
        self.p = pb.new_vector() if loop == "generic" else None
        self._first, self._tail = self._MODES[
            "mixed" if self.mixed else "pmg" if self.pmg is not None
            else "jacobi" if self.dinv is not None else "plain"]

    @property
    def fused_pcg(self) -> bool:
        return self.dinv is not None and self.loop == "fused"

    @property
    def _op_drives_loop(self) -> bool:
        """The operator's own CG loop (and native runtime) runs the solve."""
        return self.pmg is None and (self.dinv is None or self.fused_pcg)

    def _allreduce(self, slot: int) -> None:
        if self.pb.comm.size > 1:
            self.pb.comm.allreduce_(self.scal[slot: slot + 1])

    def slots(self) -> tuple[int, int]:
        """(cur, nxt): the rho slot iteration `it` reads and the one it writes
        (ping-pong).  After an iteration `nxt` is the slot that one read."""
        return (self.RR0, self.RR1) if self.it % 2 == 0 else (self.RR1, self.RR0)

    def rho0(self, a: torch.Tensor, b: torch.Tensor, dot=None) -> None:
        """End of a prologue: rho0 = a.b into RR0 and, preconditioned, the
        plain r0.r0 into RNORM, each all-reduced."""
        (dot or self.k.dot)(a, b, self.partials, self.scal, self.RR0)
        self._allreduce(self.RR0)
        if self.dinv is not None or self.pmg is not None:
            self.k.dot(self.r, self.r, self.partials, self.scal, self.RNORM)
            self._allreduce(self.RNORM)

    # Per preconditioner: `_first_*` forms p0 = M^-1 r0 and rho0; `_tail_*`
    # is an iteration after the common head: the update with alpha =
    # s[cur] / s[PAP], the new rho into s[nxt], p = (s[nxt] / s[cur]) p + z.
    def _first_plain(self) -> None:
        self.p.copy_(self.r)
        self.rho0(self.p, self.r)

    def _tail_plain(self, cur: int, nxt: int) -> None:
        k, r, p, scal = self.k, self.r, self.p, self.scal
        k.cg_update(self.x, r, p, self.y, scal, cur, self.PAP, nxt, self.partials)
        self._allreduce(nxt)
        k.p_update(p, r, scal, nxt, cur)

    def _first_jacobi(self) -> None:
        # p0 = dinv . r0 (beta = 0 / 1)
        self.p.zero_()
        self.k.pcg_p_update(self.p, self.r, self.dinv, self.scal, self.ZERO, self.ONE)
        self.rho0(self.p, self.r)

    def _tail_jacobi(self, cur: int, nxt: int) -> None:
        k, r, p, scal = self.k, self.r, self.p, self.scal
        k.pcg_update(self.x, r, p, self.y, self.dinv, scal, cur, self.PAP, nxt, self.RNORM,
                     self.partials)
        self._allreduce(nxt)
        self._allreduce(self.RNORM)
        k.pcg_p_update(p, r, self.dinv, scal, nxt, cur)

    def _first_pmg(self) -> None:
        self.pmg.apply(self.r, self.z)
        self.p.copy_(self.z)
        self.rho0(self.r, self.z)

    def _tail_pmg(self, cur: int, nxt: int) -> None:
        k, r, p, z, scal = self.k, self.r, self.p, self.z, self.scal
        k.cg_update(self.x, r, p, self.y, scal, cur, self.PAP, self.RNORM, self.partials)
        self._allreduce(self.RNORM)
        self.pmg.apply(r, z)
        k.dot(r, z, self.partials, scal, nxt)
        self._allreduce(nxt)
        k.p_update(p, z, scal, nxt, cur)

    def _first_mixed(self) -> None:
        # z0 kept in FP32 (pmg.zc) and promoted into p0
        k, pmg = self.k, self.pmg
        k.demote(self.r, pmg.rc)
        pmg.apply_cycle(pmg.rc, pmg.zc)
        k.promote(pmg.zc, self.p)
        self.rho0(self.r, pmg.zc, k.dot_f64_f32)

    def _tail_mixed(self, cur: int, nxt: int) -> None:
        k, r, p, pmg, scal = self.k, self.r, self.p, self.pmg, self.scal
        k.cg_update_demote(self.x, r, p, self.y, scal, cur, self.PAP, self.RNORM, self.partials,
                           pmg.rc)
        self._allreduce(self.RNORM)
        pmg.apply_cycle(pmg.rc, pmg.zc)
        k.dot_f64_f32(r, pmg.zc, self.partials, scal, nxt)
        self._allreduce(nxt)
        k.p_update_f64_f32(p, pmg.zc, scal, nxt, cur)

    # Plain functions, called with the instance: a bound method kept on the
    # instance would be a reference cycle, and the vectors would then live
    # until the garbage collector runs instead of going with the last reference.
    _MODES = {"plain": (_first_plain, _tail_plain), "jacobi": (_first_jacobi, _tail_jacobi),
              "pmg": (_first_pmg, _tail_pmg), "mixed": (_first_mixed, _tail_mixed)}

    def start(self, op, x: torch.Tensor, b: torch.Tensor) -> None:
        """r0 = b - A x0, p0 = M^-1 r0, rho0 = p0.r0 (the prologue of
        src/cg.hpp:98-112)."""
        self.op, self.x, self.it = op, x, 0
        if self.fused_pcg and not getattr(op, "supports_fused_pcg", False):
            name = getattr(op, "name", type(op).__name__)
            raise ValueError(f"operator {name!r} has no fused preconditioned CG loop "
                             "(fused2, fused3 and fused5 do); use loop='generic'")
        # the operator's own loop: on request for Jacobi, whenever it has one
        # for the unpreconditioned solve
        self._delegated = self.fused_pcg or (self._op_drives_loop and hasattr(op, "cg_start"))
        if self._delegated:
            op.cg_start(self, x, b)
            return
        op.apply(x, self.y)
        self.k.axpy(self.r, -1.0, self.y, b)
        self._first(self)

    def iterate(self, n: int, flush: bool = True) -> None:
        """Run n CG iterations (state persists across calls).  A fused
        operator lags its x update by one iteration; `flush=False` leaves the
        last one pending for the next call (x is then one update behind)."""
        if self._delegated:
            self.op.cg_iterate(self, n, flush=flush)
            return
        op, k, y, p = self.op, self.k, self.y, self.p
        for _ in range(n):
            cur, nxt = self.slots()
            op.apply(p, y)
            k.dot(p, y, self.partials, self.scal, self.PAP)
            self._allreduce(self.PAP)
            self._tail(self, cur, nxt)
            self.it += 1

    def iterate_timed(self, n: int) -> list[float]:
        """iterate(n) plus the device time (ms) of each step.  The native
        runtime records timing events between its steps (same launches as
        iterate); the Python loop records torch events around each step."""
        rt = getattr(self.op, "_rt", None) if self._op_drives_loop else None
        if rt is not None:
            return rt.iterate_timed(n)
        if self.pb.platform != "gpu":
            self.iterate(n)
            return []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            # one x flush at the end of the timed window (inside the last
            # step), as the native runtime's iterate(n) does
            self.iterate(1, flush=i == n - 1)
            ev[i + 1].record()
        ev[n].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    def wait(self) -> None:
        """Host wait for the queued iterations.  With the native runtime the
        wait is bounded by the RCCL deadline (a hung peer raises instead of
        blocking torch.cuda.synchronize forever)."""
        rt = getattr(self.op, "_rt", None) if self._op_drives_loop else None
        if rt is not None:
            rt.wait()
        elif self.pb.platform == "gpu":
            torch.cuda.synchronize()

    def solve(self, op, x: torch.Tensor, b: torch.Tensor, max_iter: int) -> int:
        self.start(op, x, b)
        self.iterate(max_iter)
        return max_iter

    def residual_norm2(self) -> float:
        preconditioned = self.dinv is not None or self.pmg is not None
        return float(self.scal[self.RNORM if preconditioned else self.slots()[0]].item())


def cg_solve_device(op, pb, x: torch.Tensor, b: torch.Tensor, max_iter: int) -> int:
    return DeviceCG(pb).solve(op, x, b, max_iter)
