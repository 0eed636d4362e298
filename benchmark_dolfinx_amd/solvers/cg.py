"""Conjugate gradients (reference: `cg_solve`, src/cg.hpp:89-169), unpreconditioned
by default, optionally Jacobi-preconditioned with the matrix-free diagonal
(`cg_solve(..., dinv=...)`, `DeviceCG(pb, precond="jacobi")`) or with any
symmetric positive definite M^-1 given as a callable (`cg_solve(...,
precond=...)`), such as the p-multigrid V-cycle of solvers/pmg.py
(`DeviceCG(pb, precond="pmg")`).

Two implementations with the reference's algorithm (x0 given, r0 = b - A x0,
p0 = r0, rtol = 0 runs exactly max_iter iterations):

* `cg_solve`: generic, host scalars (used by the CPU platform and the CSR
  comparison path).
* `cg_solve_device`: GPU, every scalar stays on the device.  Per iteration:
  apply (+ halo), dot(p, y) -> all-reduce, fused {x += a p; r -= a y;
  r.r} -> all-reduce, p = b p + r.  alpha/beta are formed inside the kernels
  from float64 device slots, ping-ponging the r.r slot between iterations
  so no kernel reads a slot another kernel of the same iteration writes.
  One halo exchange per iteration (the reference does two, quirk Q2) and no
  host synchronisation (quirk Q3).

When the operator provides `cg_start` / `cg_iterate` (the fused structured
kernel, models/fused.py) the device loop delegates to it.  The preconditioned
solve does so only on request (`loop="fused"`): the fused kernels then run
with u = z = dinv . r, r.z in the r.r slots, and an update pass that also
stores z (csrc/hip/fused_common.hip).
"""

from __future__ import annotations

import torch


def cg_solve(op, pb, x: torch.Tensor, b: torch.Tensor, max_iter: int,
             rtol: float = 0.0, dinv: torch.Tensor | None = None, precond=None) -> int:
    """`dinv` (lattice-shaped 1 / diag(A), `PoissonProblem.jacobi_inverse`):
    Jacobi-preconditioned CG; `precond`: a callable `precond(r, z)` that
    writes z = M^-1 r (e.g. `PMultigrid.apply`); neither: the unpreconditioned
    algorithm."""
    if dinv is not None and precond is not None:
        raise ValueError("give dinv or precond, not both")
    if dinv is not None:
        return _pcg_solve(op, pb, x, b, max_iter, rtol, dinv)
    if precond is not None:
        return _pcg_solve_callable(op, pb, x, b, max_iter, rtol, precond)
    r = pb.new_vector()
    y = pb.new_vector()
    op.apply(x, y)
    r.copy_(b - y)
    p = r.clone()
    rnorm0 = pb.inner(p, r)
    rnorm = rnorm0
    rtol2 = rtol * rtol
    k = 0
    while k < max_iter:
        k += 1
        op.apply(p, y)
        alpha = rnorm / pb.inner(p, y)
        x.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        rnorm_new = pb.inner(r, r)
        beta = rnorm_new / rnorm
        rnorm = rnorm_new
        if rnorm0 > 0 and rnorm / rnorm0 < rtol2:
            break
        p.mul_(beta).add_(r)
    return k


def _pcg_solve(op, pb, x, b, max_iter: int, rtol: float, dinv) -> int:
    """Standard PCG with M^-1 = diag(dinv): z = dinv . r, beta = r.z (new) /
    r.z (old), stop test on r.r (the reference's hook for it:
    MatrixOperator::get_diag_inverse, src/csr.hpp:81-106)."""
    r = pb.new_vector()
    y = pb.new_vector()
    op.apply(x, y)
    r.copy_(b - y)
    z = dinv * r
    p = z.clone()
    rz = pb.inner(r, z)
    rtol2 = rtol * rtol
    rnorm0 = pb.inner(r, r) if rtol2 > 0 else 0.0
    k = 0
    while k < max_iter:
        k += 1
        op.apply(p, y)
        alpha = rz / pb.inner(p, y)
        x.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        torch.mul(dinv, r, out=z)
        rz_new = pb.inner(r, z)
        beta = rz_new / rz
        rz = rz_new
        if rnorm0 > 0 and pb.inner(r, r) / rnorm0 < rtol2:
            break
        p.mul_(beta).add_(z)
    return k


def _pcg_solve_callable(op, pb, x, b, max_iter: int, rtol: float, precond) -> int:
    """PCG with z = M^-1 r computed by `precond(r, z)`; same recurrence and
    stop test as `_pcg_solve`."""
    r = pb.new_vector()
    y = pb.new_vector()
    z = pb.new_vector()
    op.apply(x, y)
    r.copy_(b - y)
    precond(r, z)
    p = z.clone()
    rz = pb.inner(r, z)
    rtol2 = rtol * rtol
    rnorm0 = pb.inner(r, r) if rtol2 > 0 else 0.0
    k = 0
    while k < max_iter:
        k += 1
        op.apply(p, y)
        alpha = rz / pb.inner(p, y)
        x.add_(p, alpha=alpha)
        r.add_(y, alpha=-alpha)
        precond(r, z)
        rz_new = pb.inner(r, z)
        beta = rz_new / rz
        rz = rz_new
        if rnorm0 > 0 and pb.inner(r, r) / rnorm0 < rtol2:
            break
        p.mul_(beta).add_(z)
    return k


class DeviceCG:
    """Device-resident CG state for the GPU platform.

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
    # Jacobi PCG: RR0 / RR1 carry r.z, RNORM the plain r.r; ZERO / ONE give the
    # prologue's beta = 0 (slots 3, 4: the fused kernels' lagged alphas)
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

    def start(self, op, x: torch.Tensor, b: torch.Tensor) -> None:
        """r0 = b - A x0, p0 = r0, rho0 = p0.r0 (the prologue of src/cg.hpp:98-112)."""
        self.op, self.x, self.it = op, x, 0
        k, r, y, p, scal = self.k, self.r, self.y, self.p, self.scal
        if self.fused_pcg:
            if not getattr(op, "supports_fused_pcg", False):
                name = getattr(op, "name", type(op).__name__)
                raise ValueError(f"operator {name!r} has no fused preconditioned CG loop "
                                 "(fused2, fused3 and fused5 do); use loop='generic'")
            op.cg_start(self, x, b)
            return
        if self.mixed:
            # the same prologue with z0 kept in FP32 (pmg.zc) and promoted into p0
            pmg = self.pmg
            op.apply(x, y)
            k.axpy(r, -1.0, y, b)
            k.demote(r, pmg.rc)
            pmg.apply_cycle(pmg.rc, pmg.zc)
            k.promote(pmg.zc, p)
            k.dot_f64_f32(r, pmg.zc, self.partials, scal, self.RR0)
            self._allreduce(self.RR0)
            k.dot(r, r, self.partials, scal, self.RNORM)
            self._allreduce(self.RNORM)
            return
        if self.pmg is not None:
            # r0 = b - A x0, z0 = M^-1 r0, p0 = z0, rz0 = r0.z0, rr0 = r0.r0
            z = self.z
            op.apply(x, y)
            k.axpy(r, -1.0, y, b)
            self.pmg.apply(r, z)
            p.copy_(z)
            k.dot(r, z, self.partials, scal, self.RR0)
            self._allreduce(self.RR0)
            k.dot(r, r, self.partials, scal, self.RNORM)
            self._allreduce(self.RNORM)
            return
        if self.dinv is not None:
            # p0 = dinv . r0 (beta = 0 / 1), rz0 = p0.r0, rr0 = r0.r0
            op.apply(x, y)
            k.axpy(r, -1.0, y, b)
            p.zero_()
            k.pcg_p_update(p, r, self.dinv, scal, self.ZERO, self.ONE)
            k.dot(p, r, self.partials, scal, self.RR0)
            self._allreduce(self.RR0)
            k.dot(r, r, self.partials, scal, self.RNORM)
            self._allreduce(self.RNORM)
            return
        if hasattr(op, "cg_start"):
            op.cg_start(self, x, b)
            return
        op.apply(x, y)
        k.axpy(r, -1.0, y, b)
        p.copy_(r)
        k.dot(p, r, self.partials, scal, self.RR0)
        self._allreduce(self.RR0)

    def iterate(self, n: int, flush: bool = True) -> None:
        """Run n CG iterations (state persists across calls).  A fused
        operator lags its x update by one iteration; `flush=False` leaves the
        last one pending for the next call (x is then one update behind)."""
        op, x = self.op, self.x
        k, r, y, p, scal = self.k, self.r, self.y, self.p, self.scal
        if self.fused_pcg:
            op.cg_iterate(self, n, flush=flush)
            return
        if self.mixed:
            pmg = self.pmg
            for _ in range(n):
                cur = self.RR0 if self.it % 2 == 0 else self.RR1
                nxt = self.RR1 if self.it % 2 == 0 else self.RR0
                op.apply(p, y)
                k.dot(p, y, self.partials, scal, self.PAP)
                self._allreduce(self.PAP)
                k.cg_update_demote(x, r, p, y, scal, cur, self.PAP, self.RNORM, self.partials,
                                   pmg.rc)
                self._allreduce(self.RNORM)
                pmg.apply_cycle(pmg.rc, pmg.zc)
                k.dot_f64_f32(r, pmg.zc, self.partials, scal, nxt)
                self._allreduce(nxt)
                k.p_update_f64_f32(p, pmg.zc, scal, nxt, cur)
                self.it += 1
            return
        if self.pmg is not None:
            z = self.z
            for _ in range(n):
                cur = self.RR0 if self.it % 2 == 0 else self.RR1
                nxt = self.RR1 if self.it % 2 == 0 else self.RR0
                op.apply(p, y)
                k.dot(p, y, self.partials, scal, self.PAP)
                self._allreduce(self.PAP)
                k.cg_update(x, r, p, y, scal, cur, self.PAP, self.RNORM, self.partials)
                self._allreduce(self.RNORM)
                self.pmg.apply(r, z)
                k.dot(r, z, self.partials, scal, nxt)
                self._allreduce(nxt)
                k.p_update(p, z, scal, nxt, cur)
                self.it += 1
            return
        if self.dinv is not None:
            dinv = self.dinv
            for _ in range(n):
                cur = self.RR0 if self.it % 2 == 0 else self.RR1
                nxt = self.RR1 if self.it % 2 == 0 else self.RR0
                op.apply(p, y)
                k.dot(p, y, self.partials, scal, self.PAP)
                self._allreduce(self.PAP)
                k.pcg_update(x, r, p, y, dinv, scal, cur, self.PAP, nxt, self.RNORM,
                             self.partials)
                self._allreduce(nxt)
                self._allreduce(self.RNORM)
                k.pcg_p_update(p, r, dinv, scal, nxt, cur)
                self.it += 1
            return
        if hasattr(op, "cg_iterate"):
            op.cg_iterate(self, n, flush=flush)
            return
        for _ in range(n):
            cur = self.RR0 if self.it % 2 == 0 else self.RR1
            nxt = self.RR1 if self.it % 2 == 0 else self.RR0
            op.apply(p, y)
            k.dot(p, y, self.partials, scal, self.PAP)
            self._allreduce(self.PAP)
            k.cg_update(x, r, p, y, scal, cur, self.PAP, nxt, self.partials)
            self._allreduce(nxt)
            k.p_update(p, r, scal, nxt, cur)
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
        if self.dinv is not None or self.pmg is not None:
            return float(self.scal[self.RNORM].item())
        slot = self.RR0 if self.it % 2 == 0 else self.RR1
        return float(self.scal[slot].item())


def cg_solve_device(op, pb, x: torch.Tensor, b: torch.Tensor, max_iter: int) -> int:
    return DeviceCG(pb).solve(op, x, b, max_iter)
