"""p-multigrid preconditioner: one V-cycle over the degrees P, max(1, P // 2),
..., 1 on the same cells, with Chebyshev-Jacobi smoothing on every level.

Every level is a `PoissonProblem` of its degree on the same cells, partition,
perturbation and per-cell kappa; its operator comes from `make_operator`, its
smoothing diagonal from `jacobi_inverse()`.  The transfers are the nodal
interpolation J (x) J (x) J per cell (J[a, i] = l_i^c(xi_a^f), the coarse GLL
Lagrange basis at the fine GLL nodes) and its exact transpose
(csrc/hip/lap_transfer.h, host twins in csrc/host/bdx_host_mg.cpp).

V-cycle on level l with residual r:
    z = smooth(r, zero guess);  res = r - A z;  r_c = R res;
    z += P Vcycle(l + 1, r_c);  z = smooth(r, z)
with the same polynomial before and after, so M^-1 is symmetric and plain PCG
applies.  The coarsest level (degree 1) is the same Chebyshev iteration from a
zero guess with a higher degree and a wider interval.

Chebyshev-Jacobi of degree k on [lhi / range, lhi], lhi = 1.1 x the estimate
of lambda_max(D^-1 A) from `eig_iters` power iterations: with theta = (lhi +
llo) / 2, delta = (lhi - llo) / 2, sigma = theta / delta, rho_0 = 1 / sigma
    d = (1 / theta) D^-1 res;  z += d
    rho' = 1 / (2 sigma - rho);  d = rho' rho d + (2 rho' / delta) D^-1 (r - A z);  z += d
All coefficients are host doubles fixed at setup, so a cycle runs without any
host synchronisation: operator applies, one fused vector kernel per Chebyshev
step (`cheb_step`), axpy, the two transfer kernels and the halo exchanges.

h-levels (`h_levels != 0`, off by default): the hierarchy continues below
degree 1 with geometrically coarsened degree-1 problems on the lattices of
`fem.mesh.h_hierarchy` (`PoissonProblem.coarsened`: subsampled vertices, the
children's mean kappa, rediscretised operator and diagonal).  The levels form
one list, the p-levels then the h-levels; every level but the last is smoothed
and the last takes the coarse iteration, so degree 1 becomes an ordinary
smoothed level.  Between two degree-1 levels the transfers are trilinear in
index space (csrc/hip/lap_htransfer.h) and fold the cycle's two vector passes:
r_c = R (r - A z) in the restriction's load, z += P z_c in the prolongation's
store.  The exchange protocol around them is that of the p-transfers.

Mixed precision (`cycle_dtype=torch.float32` on an FP64 problem, off by
default): every level, level 0 and the h-levels included, is an FP32 problem
with the FP64 problem's comm, cells, partition, perturbation, coefficient and
shear, and the whole setup and cycle above run on them unchanged.  `apply`
keeps its FP64 contract by demoting r into `rc`, running `apply_cycle(rc, zc)`
and promoting `zc` (csrc/hip/mixed.hip, host twins in csrc/host/bdx_host_mg.cpp);
a caller that fuses the boundary into its own kernels (`DeviceCG`) calls
`apply_cycle` directly.  The cycle is linear in r and is applied unscaled.

Tail (`tail_nodes=N > 0`, off by default): the longest suffix of the level
list whose levels all have degree 1 and at most N local nodes runs in one
call, `pmg_tail` (csrc/hip/pmg_tail.h: one launch of one workgroup, the phases
separated by workgroup barriers; host twin in csrc/host/bdx_host_mg.cpp), where
the cycle reaches its first level.  The schedule, the coefficients, `dinv`,
`bc` and the transfer tables are the levels' own; setup is unchanged, lambda_max
included.  Inside the tail a level's operator is its assembled 27-point
stencil (`ops.kernels.stencil27` of `CSROperator`), which equals the
matrix-free operator to rounding, not bitwise: the tailed preconditioner is a
rounding-level perturbation of the untailed one.  One rank only: the tail
levels of a partitioned mesh would need halo exchanges inside the kernel.

Row transfers (`p_transfer="row"`, off by default): the p-pairs use the
row-streaming kernels of csrc/hip/lap_rowtransfer.h, which have the
h-transfers' modes, so a p-pair runs the h-pair's branch of the cycle: one
restriction that folds the residual and one prolongation that folds the
update, with no axpy, no zeroing and no colour launches.  The operators are
those of the cell kernels in another summation order.

Stencil levels (`q1_operator="stencil"`, off by default): every degree-1
level outside the tail (the degree-1 p-level, the h-levels, level 0 of a
degree-1 problem) applies its assembled 27-point stencil `lv.S`
(`ops.kernels.stencil27` of `CSROperator`, as in the tail) with the streaming
kernels of csrc/hip/lap_stencil27.h instead of the matrix-free operator, which
it equals to rounding.  Setup is unchanged: the power iteration runs on
`lv.op`, so lambda_max and every coefficient are those of the default.  On one
rank a Chebyshev step is one launch, `stencil27_cheb`, that never stores A z
and ping-pongs the iterate between `z` and the level's `t` (free on degree-1
levels: the h-pair branch of the cycle does not use it); the first step from a
zero guess writes the buffer from which the last step lands in `z`, and only
an odd number of steps from a nonzero guess ends with a copy.  On more ranks S
holds the rank's own cells, a ghost row its partial sums, so a step keeps
`CSROperator.apply`'s protocol: forward exchange, `stencil27_apply` on every
local row, reverse exchange, `cheb_step`.

Stencil assembly (`q1_assembly="direct"`, default "csr"): the stencils of the
stencil levels and of the tail are written by `PoissonProblem.stencil27
("direct")` (csrc/hip/lap_stencil27_assemble.h, one launch per level; host twin
in csrc/host/bdx_host_mg.cpp) in place of `CSROperator` on the host, the sort
into planes and the upload.  The entries agree with the host's to rounding; the
rest of setup is untouched.
"""

from __future__ import annotations

import numpy as np
import torch

from ..fem.mesh import _hash_uniform, h_hierarchy
from ..fem.quadrature import lagrange_tables
from ..models.poisson import PoissonProblem
from ..ops.hip_api import CONSTANTS


def level_degrees(P: int) -> list[int]:
    """P, max(1, P // 2), ... down to 1 (7-3-1, 6-3-1, 5-2-1, 4-2-1, 3-1, 2-1, 1)."""
    out = [int(P)]
    while out[-1] > 1:
        out.append(max(1, out[-1] // 2))
    return out


def chebyshev_coefficients(lam_hi: float, rng: float, degree: int) -> list[tuple[float, float]]:
    """(a, b) of every step d = a d + b D^-1 res of the degree-`degree`
    Chebyshev iteration on [lam_hi / rng, lam_hi]; the first has a = 0."""
    lo = lam_hi / rng
    theta, delta = 0.5 * (lam_hi + lo), 0.5 * (lam_hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(degree - 1):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out


class _Level:
    """One degree of the hierarchy: problem, operator, smoother data, work vectors."""

    def __init__(self, pb: PoissonProblem):
        from ..driver import make_operator  # driver imports solvers.cg: import lazily
        self.pb = pb
        self.op = make_operator(pb, "auto", "auto")
        self.k = pb.kernels
        self.dinv = pb.jacobi_inverse()
        self.bc = pb.bc_mask()
        self.latd = pb.lat.as_int64()
        self.y = pb.new_vector()    # A z
        self.d = pb.new_vector()    # Chebyshev direction
        self.t = pb.new_vector()    # residual, then the prolonged correction
        self.r = None               # coarse levels: the restricted residual
        self.z = None               # coarse levels: the correction
        self.J = None               # p-transfer table to the next coarser level
        self.H = None               # or the h-transfer tables to it
        self.S = None               # q1_operator="stencil": the 27-point stencil
        self.coef = []
        self.lambda_max = 0.0


class PMultigrid:
    """z = M^-1 r by one p-multigrid V-cycle (module docstring).

    degrees: the level degrees; lambda_max: the estimate of lambda_max(D^-1 A)
    per level (the smoothers' upper bound is 1.1 x it).

    h_levels: 0 = the p-levels only; N > 0 = at most N geometric h-levels
    under degree 1; -1 = as many as `fem.mesh.h_hierarchy` allows.  `h_levels`
    then holds the number built and `h_cells` their global cell counts; the
    hierarchy depends on the partition's cut points (fem/mesh.py).

    cycle_dtype: None or the problem's dtype = the hierarchy in the problem's
    precision, level 0 being `pb` itself; torch.float32 on a float64 problem =
    the mixed mode of the module docstring (`mixed` is then True, `rc` / `zc`
    are the FP32 level-0 work vectors and `info()` carries `cycle_float`).

    tail_nodes: 0 = off; N > 0 = the levels of the tail (module docstring) run
    in one `pmg_tail` call; `tail_start` is then the index of the tail's first
    level (None: no level qualifies, the cycle is the untailed one),
    `tail_levels` their number and `tail` the `ops.kernels.PmgTail`.

    p_transfer: "cell" = the per-cell transfer kernels between the p-levels;
    "row" = the row-streaming ones (module docstring), which accept `add` and
    `y` in `prolong` / `restrict` as the h-pairs do.

    q1_operator: "matfree" = every level applies its matrix-free operator;
    "stencil" = the degree-1 levels outside the tail apply their assembled
    27-point stencil `lv.S` (module docstring).

    q1_assembly: how those stencils and the tail's are built
    (`PoissonProblem.stencil27`): "csr" = from the host's assembled matrix;
    "direct" = by the assembly kernel on the problem's device, so that setup
    builds no `CSROperator`; refused where there is nothing to assemble
    (q1_operator="matfree" without a tail).  Setup is otherwise the same:
    lambda_max, `dinv` and every coefficient do not depend on it."""

    TAIL_MAX_NODES = CONSTANTS["kTailMaxNodes"]

    def __init__(self, pb: PoissonProblem, smooth_degree: int = 2, smooth_range: float = 10.0,
                 coarse_degree: int = 8, coarse_range: float = 100.0, eig_iters: int = 10,
                 h_levels: int = 0, cycle_dtype: torch.dtype | None = None, tail_nodes: int = 0,
                 p_transfer: str = "cell", q1_operator: str = "matfree",
                 q1_assembly: str = "csr"):
        if smooth_degree < 1 or coarse_degree < 1 or eig_iters < 1:
            raise ValueError("smoother degrees and eig_iters must be positive")
        if smooth_range <= 1.0 or coarse_range <= 1.0:
            raise ValueError("smoother ranges must exceed 1")
        if isinstance(h_levels, bool) or not isinstance(h_levels, (int, np.integer)) or h_levels < -1:
            raise ValueError("h_levels must be -1 (all), 0 (none) or a positive count")
        if isinstance(tail_nodes, bool) or not isinstance(tail_nodes, (int, np.integer)) \
                or not 0 <= tail_nodes <= self.TAIL_MAX_NODES:
            raise ValueError(f"tail_nodes must be 0 (off) or a node count up to "
                             f"{self.TAIL_MAX_NODES}")
        if tail_nodes > 0 and pb.comm.size > 1:
            raise ValueError("tail_nodes needs a single rank: the tail levels of a partitioned "
                             "mesh would need halo exchanges inside the kernel")
        if p_transfer not in ("cell", "row"):
            raise ValueError(f"p_transfer must be 'cell' or 'row', got {p_transfer!r}")
        self.p_transfer = p_transfer
        if q1_operator not in ("matfree", "stencil"):
            raise ValueError(f"q1_operator must be 'matfree' or 'stencil', got {q1_operator!r}")
        self.q1_operator = q1_operator
        if not isinstance(q1_assembly, str) or q1_assembly not in ("csr", "direct"):
            raise ValueError(f"q1_assembly must be 'csr' or 'direct', got {q1_assembly!r}")
        if q1_assembly == "direct" and q1_operator == "matfree" and tail_nodes == 0:
            raise ValueError("q1_assembly='direct' has nothing to assemble: it needs "
                             "q1_operator='stencil' or tail_nodes > 0")
        self.q1_assembly = q1_assembly
        if cycle_dtype is None:
            cycle_dtype = pb.dtype
        if cycle_dtype not in (torch.float32, torch.float64) or \
                (cycle_dtype == torch.float64 and pb.dtype != torch.float64):
            raise ValueError(f"cycle_dtype must be None, the problem's {pb.dtype} or, on a "
                             f"float64 problem, torch.float32; got {cycle_dtype!r}")
        self.pb = pb
        self.cycle_dtype = cycle_dtype
        self.mixed = cycle_dtype != pb.dtype    # FP32 cycle under an FP64 problem
        self.smooth_degree, self.smooth_range = int(smooth_degree), float(smooth_range)
        self.coarse_degree, self.coarse_range = int(coarse_degree), float(coarse_range)
        self.degrees = level_degrees(pb.degree)
        self.levels: list[_Level] = []
        ncells = pb.lat.ncells_global
        for i, P in enumerate(self.degrees):
            lpb = pb if i == 0 and not self.mixed else PoissonProblem(
                pb.comm, ncells, P, pb.qmode, pb.use_gauss, cycle_dtype, pb.platform,
                pb.perturb, pb.coefficient, shear=pb.shear, partition=pb.partition)
            lv = _Level(lpb)
            if i > 0:
                lv.r, lv.z = lpb.new_vector(), lpb.new_vector()
            self.levels.append(lv)
        # h-levels under degree 1 (fem/mesh.py: h_hierarchy), each a degree-1
        # problem on the coarsened lattice; lv.H: the tables to the next one
        self.h_cells: list[tuple[int, int, int]] = []
        if h_levels != 0:
            from ..ops.kernels import HTransferTables
            for lat, fpos in h_hierarchy(self.levels[-1].pb.lat, int(h_levels)):
                above = self.levels[-1]
                lv = _Level(PoissonProblem.coarsened(above.pb, lat, fpos))
                lv.r, lv.z = lv.pb.new_vector(), lv.pb.new_vector()
                above.H = HTransferTables(fpos, cycle_dtype, pb.device)
                self.levels.append(lv)
                self.h_cells.append(tuple(int(c) for c in lat.ncells_global))
        self.h_levels_requested = int(h_levels)
        self.h_levels = len(self.h_cells)                   # the number built
        for i, lv in enumerate(self.levels):
            coarsest = i == len(self.levels) - 1
            if not coarsest and lv.H is None:
                nxt = self.levels[i + 1].pb
                J, _ = lagrange_tables(nxt.tables.nodes, lv.pb.tables.nodes)
                lv.J = np.ascontiguousarray(J, dtype=np.float64)
            lv.lambda_max = self._power_iteration(lv, eig_iters)
            if coarsest:
                lv.coef = chebyshev_coefficients(1.1 * lv.lambda_max, self.coarse_range,
                                                 self.coarse_degree)
            else:
                lv.coef = chebyshev_coefficients(1.1 * lv.lambda_max, self.smooth_range,
                                                 self.smooth_degree)
        self.lambda_max = [lv.lambda_max for lv in self.levels]
        # mixed mode: the level-0 residual and correction at cycle precision
        self.rc = self.zc = None
        if self.mixed:
            self.rc, self.zc = self.levels[0].pb.new_vector(), self.levels[0].pb.new_vector()
        # the tail: the trailing degree-1 levels of at most tail_nodes local nodes
        self.tail_nodes = int(tail_nodes)
        self.tail_start, self.tail_levels, self.tail = None, 0, None
        if self.tail_nodes > 0:
            start = len(self.levels)
            while start > 0 and self.levels[start - 1].pb.degree == 1 and \
                    int(np.prod(self.levels[start - 1].pb.lat.L)) <= self.tail_nodes:
                start -= 1
            if start < len(self.levels):
                from ..ops.kernels import PmgTail
                self.tail_start, self.tail_levels = start, len(self.levels) - start
                self.tail = PmgTail(self.levels[start:], cycle_dtype, pb.device, q1_assembly)
        # the stencils of the degree-1 levels above the tail
        if self.q1_operator == "stencil":
            end = len(self.levels) if self.tail_start is None else self.tail_start
            for lv in self.levels[:end]:
                if lv.pb.degree == 1:
                    lv.S = lv.pb.stencil27(q1_assembly)

    # ---------------------------------------------------------------- setup
    @staticmethod
    def _power_iteration(lv: _Level, iters: int) -> float:
        """Rayleigh quotient <v, D^-1 A v>, |v| = 1, after `iters` power
        iterations from a start vector hashed from the global lexicographic
        dof index (the same for every partition), zero on Dirichlet dofs."""
        pb = lv.pb
        v0 = np.zeros(pb.lat.shape, dtype=np.float64)
        gid = pb.lat.global_indices().astype(np.uint64)
        v0[:, :, : pb.lat.L[2]] = np.where(pb.lat.bc_mask(), 0.0, 2.0 * _hash_uniform(gid, 11) - 1.0)
        v = torch.from_numpy(v0).to(pb.device, pb.dtype)
        w = pb.new_vector()
        lam = 0.0
        for _ in range(iters):
            nrm = pb.norm(v)
            if not nrm > 0.0:
                return 1.0  # no interior dof: D^-1 A is the identity
            pb.scale(v, 1.0 / nrm)
            lv.op.apply(v, lv.y)
            pb.pointwise_mult(w, lv.dinv, lv.y)
            lam = pb.inner(v, w)
            pb.copy(v, w)
        return float(lam)

    # ------------------------------------------------------------ transfers
    def prolong(self, l: int, vc: torch.Tensor, vf: torch.Tensor, add: bool = False) -> None:
        """vf = P vc from level l + 1 to level l (every local fine node; the
        coarse ghost planes are read, so vc is forward-exchanged first).
        `add` (h-pairs, and p-pairs with p_transfer="row"): vf += P vc on the
        owned fine nodes instead."""
        fine, coarse = self.levels[l], self.levels[l + 1]
        coarse.pb.halo.forward(vc)
        if fine.H is not None:
            fine.k.hprolong(coarse.latd, fine.H, vc, vf, add)
            return
        if self.p_transfer == "row":
            fine.k.prolong_row(coarse.latd, fine.J, vc, vf, add)
            return
        if add:
            raise ValueError("prolong(add=True) is the h-transfer's mode")
        fine.k.prolong(coarse.latd, fine.J, vc, vf)

    def restrict(self, l: int, vf: torch.Tensor, vc: torch.Tensor,
                 y: torch.Tensor | None = None) -> None:
        """vc = P^T vf from level l to level l + 1: owned fine dofs only, the
        partial sums on the coarse ghost planes reverse-exchanged to their
        owners, Dirichlet entries zeroed, then forwarded to the ghosts.
        `y` (h-pairs, and p-pairs with p_transfer="row"): vc = P^T (vf - y)."""
        fine, coarse = self.levels[l], self.levels[l + 1]
        if fine.H is not None:
            fine.k.hrestrict(coarse.latd, fine.H, vf, y, vc)
        elif self.p_transfer == "row":
            fine.k.restrict_row(coarse.latd, fine.J, vf, y, vc)
        else:
            if y is not None:
                raise ValueError("restrict(y=) is the h-transfer's mode")
            vc.zero_()
            fine.k.restrict(coarse.latd, fine.J, vf, vc)
        coarse.pb.halo.reverse(vc)
        vc.masked_fill_(coarse.bc, 0.0)
        coarse.pb.halo.forward(vc)

    # ---------------------------------------------------------------- cycle
    @staticmethod
    def _apply(lv: _Level, z: torch.Tensor, y: torch.Tensor) -> None:
        """y = A z on the owned rows of level lv."""
        if lv.S is None:
            lv.op.apply(z, y)
            return
        lv.pb.halo.forward(z)
        lv.k.stencil27_apply(lv.S, z, y)
        lv.pb.halo.reverse(y)

    @staticmethod
    def _smooth_stencil(lv: _Level, r: torch.Tensor, z: torch.Tensor, zero_guess: bool) -> None:
        """`_smooth` on a stencil level."""
        if lv.pb.halo.active:
            for i, (a, b) in enumerate(lv.coef):
                if i == 0 and zero_guess:
                    lv.k.cheb_step(True, 0.0, b, lv.dinv, r, None, lv.d, z)
                else:
                    PMultigrid._apply(lv, z, lv.y)
                    lv.k.cheb_step(False, a, b, lv.dinv, r, lv.y, lv.d, z)
            return
        # one rank: every step with an operator reads `cur` and writes the
        # other of z and t; the first step of a zero guess has none and writes
        # the buffer from which the others end in z
        fused = len(lv.coef) - (1 if zero_guess else 0)
        cur = lv.t if zero_guess and fused % 2 else z
        for i, (a, b) in enumerate(lv.coef):
            if i == 0 and zero_guess:
                lv.k.cheb_step(True, 0.0, b, lv.dinv, r, None, lv.d, cur)
                continue
            nxt = lv.t if cur is z else z
            lv.k.stencil27_cheb(lv.S, lv.dinv, r, cur, lv.d, nxt, a, b)
            cur = nxt
        if cur is not z:        # an odd number of steps from a nonzero guess
            z.copy_(cur)

    @staticmethod
    def _smooth(lv: _Level, r: torch.Tensor, z: torch.Tensor, zero_guess: bool) -> None:
        if lv.S is not None:
            PMultigrid._smooth_stencil(lv, r, z, zero_guess)
            return
        for i, (a, b) in enumerate(lv.coef):
            if i == 0 and zero_guess:
                lv.k.cheb_step(True, 0.0, b, lv.dinv, r, None, lv.d, z)
            else:
                lv.op.apply(z, lv.y)
                lv.k.cheb_step(False, a, b, lv.dinv, r, lv.y, lv.d, z)

    def _vcycle(self, l: int, r: torch.Tensor, z: torch.Tensor) -> None:
        lv = self.levels[l]
        if l == self.tail_start:
            lv.k.pmg_tail(self.tail, r, z)      # this level and everything below it
            return
        self._smooth(lv, r, z, True)
        if l == len(self.levels) - 1:
            return
        nxt = self.levels[l + 1]
        self._apply(lv, z, lv.y)
        if lv.H is not None or self.p_transfer == "row":
            # h-pair, or a p-pair by rows: the residual and the correction's
            # sum are folded into the transfer kernels' load and store
            self.restrict(l, r, nxt.r, lv.y)    # r_c = R (r - A z)
            self._vcycle(l + 1, nxt.r, nxt.z)
            self.prolong(l, nxt.z, z, True)     # z += P z_c
        else:
            lv.k.axpy(lv.t, -1.0, lv.y, r)          # res = r - A z
            self.restrict(l, lv.t, nxt.r)
            self._vcycle(l + 1, nxt.r, nxt.z)
            self.prolong(l, nxt.z, lv.t)
            lv.k.axpy(z, 1.0, lv.t, z)              # z += P z_c
        self._smooth(lv, r, z, False)

    def apply(self, r: torch.Tensor, z: torch.Tensor) -> None:
        """z = M^-1 r (lattice-shaped; the owned entries are valid).  r is not
        modified; it must vanish on Dirichlet dofs, as every CG residual does."""
        if not self.mixed:
            self._vcycle(0, r, z)
            return
        k = self.levels[0].k
        k.demote(r, self.rc)
        self._vcycle(0, self.rc, self.zc)
        k.promote(self.zc, z)

    def apply_cycle(self, rc: torch.Tensor, zc: torch.Tensor) -> None:
        """The raw V-cycle zc = M^-1 rc on level-0 vectors of the cycle
        precision (`apply` without the demotion and promotion of mixed mode)."""
        self._vcycle(0, rc, zc)

    def info(self) -> dict:
        out = {"degrees": list(self.degrees), "lambda_max": list(self.lambda_max),
               "smooth_degree": self.smooth_degree, "coarse_degree": self.coarse_degree}
        if self.h_levels_requested != 0:
            out["h_levels"] = self.h_levels
            out["h_cells"] = [list(c) for c in self.h_cells]
        if self.mixed:
            out["cycle_float"] = 32
        if self.tail_nodes != 0:
            out["tail_nodes"] = self.tail_nodes
            out["tail_levels"] = self.tail_levels
        if self.p_transfer != "cell":
            out["p_transfer"] = self.p_transfer
        if self.q1_operator != "matfree":
            out["q1_operator"] = self.q1_operator
        if self.q1_assembly != "csr":
            out["q1_assembly"] = self.q1_assembly
        return out

    def close(self) -> None:
        """Close the level operators (native runtimes, if any was started)."""
        for lv in self.levels:
            if hasattr(lv.op, "close"):
                lv.op.close()
