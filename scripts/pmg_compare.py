#!/usr/bin/env python3
"""p-multigrid preconditioned CG against fused Jacobi-PCG and unpreconditioned
fused CG on one GPU: one JSON line per configuration (profiles/pmg.md).

  python scripts/pmg_compare.py --degree 3 --perturb 0.2 --kappa random [--ndofs 20000000]
  python scripts/pmg_compare.py --degree 6 --perturb 0.0 --kappa constant
  python scripts/pmg_compare.py --degree 3 --hlevels -1      (adds the hpmg column, profiles/hpmg.md)
  python scripts/pmg_compare.py --hlevels -1 --cycle_float 32 --tol2 1e-12 --no-yardsticks
                                                             (FP32 cycles, profiles/pmg_mixed.md)
  python scripts/pmg_compare.py --hlevels -1 --cycle_float 32 --tail 512,4096,32768 --no-yardsticks
                                                             (one-launch tail, profiles/pmg_tail.md)
  python scripts/pmg_compare.py --hlevels -1 --transfer cell,row --cycle_float 32 --no-yardsticks
                                                             (row transfers, profiles/pmg_rowtransfer.md)
  python scripts/pmg_compare.py --degree 6 --transfer-kernels
                                                             (their kernels against the launches they replace)
  python scripts/pmg_compare.py --hlevels -1 --cycle_float 32 --q1 matfree,stencil --no-yardsticks
                                                             (stencil levels, profiles/pmg_q1stencil.md)
  python scripts/pmg_compare.py --hlevels -1 --cycle_float 32 --q1 matfree,stencil \
                                --q1-assembly csr,direct --no-yardsticks
                                                             (their assembly, profiles/pmg_q1assemble.md)

One process per configuration.  FP64, qmode 1 (GLL).  Three variants, each on
its own auto-selected operator:

  cg_fused   DeviceCG(pb)                          fused CG, native runtime
  pcg_fused  DeviceCG(pb, "jacobi", loop="fused")  fused Jacobi-PCG, native runtime
  pmg        DeviceCG(pb, "pmg")                   generic loop + one V-cycle per iteration
  hpmg       (--hlevels N, N != 0) the same with PMultigrid(pb, h_levels=N): h-levels under
             degree 1; interleaved with the others window by window, whole solves alternating
             with pmg's; --no-yardsticks leaves the two fused loops out
  pmg32      (--cycle_float 32) pmg with PMultigrid(pb, cycle_dtype=float32): the FP32 V-cycle
  hpmg32     inside the FP64 loop, and the same for hpmg; interleaved like hpmg.  --tol2 T also
             counts and times every pmg variant's solve to the second tolerance T, and the five
             kernels of the precision boundary (csrc/hip/mixed.hip) are timed alone
  hpmg_tN    (--tail N[,N...], with --hlevels) hpmg with PMultigrid(pb, tail_nodes=N): the
  hpmg32_tN  trailing small levels in one launch (csrc/hip/pmg_tail.h), and the same for hpmg32;
             interleaved like hpmg.  The "tail" block also times the tail's one call against
             the untailed `_vcycle` of the same levels, with device events

  <v>_row    (--transfer cell,row) every pmg variant v again with PMultigrid(p_transfer="row"):
             the row-streaming transfers between the p-levels (csrc/hip/lap_rowtransfer.h);
             interleaved like hpmg, so the yardstick of v_row is v in the same process

  <v>_s27    (--q1 matfree,stencil) every pmg variant v again with PMultigrid(q1_operator=
             "stencil"): the degree-1 levels on their assembled 27-point stencils
             (csrc/hip/lap_stencil27.h); interleaved like hpmg, the yardstick of v_s27 is v.  The
             "q1" block also times, per variant pair, the first degree-1 level and everything
             below it alone, both ways, the construction of the two hierarchies (the difference is
             the host CSR assembly of the stencils plus their upload) and, per stencil level,
             `stencil27_apply` and `stencil27_cheb` against the matrix-free apply and apply +
             `cheb_step` they replace, with the effective TB/s over S and the vectors (apply:
             27 + 2 values per node, fused step: 27 + 6)

  <v>_s27d   (--q1-assembly csr,direct, with --q1 matfree,stencil) every v_s27 again with
             PMultigrid(q1_assembly="direct"): the stencils written by the assembly kernel
             (csrc/hip/lap_stencil27_assemble.h) instead of the host's CSR matrix; interleaved like
             hpmg, the yardstick of v_s27d is v_s27.  The "q1_assembly" block holds, per pair, the
             iterations and ms per iteration of both, the wall time to build the matfree, the csr
             and the direct hierarchy (--reps repetitions, the three in turn in this process) and,
             per stencil level, the assembly kernel alone: ms, the flop rate for a source-level
             count of 337 flops per quadrature point of each of a node's 8 cells (an FMA = 2), and
             the ratio to the time of storing S at the measured stream rate

--transfer-kernels: no solve.  For every p-pair of the configured problem, in FP64 and FP32
vectors, device-event times (the median of --reps batches of five calls, the candidates
interleaved batch by batch) of
  restrict   axpy (t = r - y) + zero_ + restrict (eight colour launches)   against
             restrict_row with y;   compulsory bytes: two fine reads + one coarse write
  prolong    prolong + axpy (z += t)   against   prolong_row with add;
             compulsory bytes: one coarse read + one fine read + one fine write
with the effective TB/s over the compulsory bytes and the 2-read 1-write stream rate.

Per-iteration time: device events between the steps of `iterate_timed(n)`, per
window the mean of the first n - 1 steps, per variant the median over the
windows (min, max), the variants interleaved window by window after two
warm-up windows each.  Iterations to the tolerance use the recurrence residual
(`residual_norm2()` read back after every iteration, outside the timed
windows).  The time to the tolerance of pmg is also measured directly: the
wall time of start + iterate(k) + a device synchronisation, median of three.
The V-cycle's parts are timed alone with device events (median of `--reps`
batches of five calls).  Bandwidths count the owned entries a kernel must move
(cheb_step: 5 reads + 2 writes; prolong: coarse read + fine write; restrict:
fine read + coarse read and write); the stream rate is a 2-read 1-write torch
update of vectors of the problem's size.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def transfer_kernels(a, nx) -> dict:
    """--transfer-kernels (module docstring): one record with a block per
    vector type and p-pair."""
    import numpy as np
    import torch

    from benchmark_dolfinx_amd.fem.quadrature import lagrange_tables
    from benchmark_dolfinx_amd.models.poisson import PoissonProblem
    from benchmark_dolfinx_amd.parallel.comm import Comm
    from benchmark_dolfinx_amd.solvers.pmg import level_degrees

    def batch(fn):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 5

    def interleaved(fns):
        """Median ms per call of each candidate, one batch of each in turn."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        out = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                out[k].append(batch(fn))
        return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                for k, v in out.items()}

    rec = {"degree": a.degree, "perturb": a.perturb, "kappa": a.kappa, "mesh": list(nx),
           "device": torch.cuda.get_device_name(0), "pairs": []}
    degrees = level_degrees(a.degree)
    for dt, size in ((torch.float64, 8), (torch.float32, 4)):
        pbs = [PoissonProblem(Comm(), nx, P, 1, False, dt, "gpu", a.perturb, a.kappa)
               for P in degrees]
        for fine, coarse in zip(pbs, pbs[1:]):
            J = np.ascontiguousarray(
                lagrange_tables(coarse.tables.nodes, fine.tables.nodes)[0], dtype=np.float64)
            k, latc = fine.kernels, coarse.lat.as_int64()
            gen = torch.Generator(device="cuda").manual_seed(1)
            r, y, t, z = (torch.randn(fine.lat.shape, dtype=dt, device="cuda", generator=gen)
                          for _ in range(4))
            rc, zc = (torch.randn(coarse.lat.shape, dtype=dt, device="cuda", generator=gen)
                      for _ in range(2))

            def cell_restrict():
                k.axpy(t, -1.0, y, r)
                rc.zero_()
                k.restrict(latc, J, t, rc)

            def cell_prolong():
                k.prolong(latc, J, zc, t)
                k.axpy(z, 1.0e-3, t, z)

            ms = interleaved({
                "cell_restrict": cell_restrict,
                "row_restrict": lambda: k.restrict_row(latc, J, r, y, rc),
                "cell_prolong": cell_prolong,
                "row_prolong": lambda: k.prolong_row(latc, J, zc, z, True),
                "stream_2r1w": lambda: t.add_(y, alpha=-1e-9)})
            nf, nc_ = fine.lat.ndofs_local, coarse.lat.ndofs_local
            nbytes = {"restrict": size * (2 * nf + nc_), "prolong": size * (nc_ + 2 * nf),
                      "stream_2r1w": size * 3 * t.numel()}
            tbs = {name: nbytes[name.split("_", 1)[1] if name != "stream_2r1w" else name]
                   / (v["median"] * 1e-3) / 1e12 for name, v in ms.items()}
            rec["pairs"].append({"float": 8 * size, "pair": [fine.degree, coarse.degree],
                                 "dofs": [nf, nc_], "ms": ms, "tb_per_s": tbs,
                                 "speedup": {"restrict": ms["cell_restrict"]["median"]
                                             / ms["row_restrict"]["median"],
                                             "prolong": ms["cell_prolong"]["median"]
                                             / ms["row_prolong"]["median"]}})
            del r, y, t, z, rc, zc
        del pbs
        torch.cuda.empty_cache()
    return rec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--ndofs", type=int, default=20_000_000)
    ap.add_argument("--perturb", type=float, default=0.2)
    ap.add_argument("--kappa", default="random", choices=["constant", "random"])
    ap.add_argument("--iters", type=int, default=10, help="iterations per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=6000)
    ap.add_argument("--hlevels", type=int, default=0,
                    help="add the hpmg variant: PMultigrid(pb, h_levels=N) (-1: all)")
    ap.add_argument("--cycle_float", type=int, default=64, choices=[32, 64],
                    help="32: add pmg32 (and, with --hlevels, hpmg32), the FP32 V-cycle in FP64 CG")
    ap.add_argument("--tol2", type=float, default=0.0,
                    help="a second, tighter tolerance for the pmg variants' solves (0: none)")
    ap.add_argument("--tail", default="",
                    help="comma-separated tail_nodes values: add hpmg_tN (and hpmg32_tN) per value")
    ap.add_argument("--transfer", default="cell",
                    help="comma-separated p_transfer values (cell,row): row adds <variant>_row")
    ap.add_argument("--q1", default="matfree",
                    help="comma-separated q1_operator values (matfree,stencil): stencil adds "
                         "<variant>_s27")
    ap.add_argument("--q1-assembly", default="csr",
                    help="comma-separated q1_assembly values (csr,direct): direct adds "
                         "<variant>_s27d (needs --q1 matfree,stencil)")
    ap.add_argument("--transfer-kernels", action="store_true",
                    help="time the row transfer kernels against the launches they replace, and stop")
    ap.add_argument("--no-yardsticks", action="store_true",
                    help="leave out cg_fused and pcg_fused")
    a = ap.parse_args(argv)

    import torch

    from benchmark_dolfinx_amd.driver import make_operator
    from benchmark_dolfinx_amd.fem.mesh import compute_mesh_size
    from benchmark_dolfinx_amd.models.poisson import PoissonProblem
    from benchmark_dolfinx_amd.parallel.comm import Comm
    from benchmark_dolfinx_amd.solvers.cg import DeviceCG
    from benchmark_dolfinx_amd.solvers.pmg import PMultigrid

    if not torch.cuda.is_available():
        raise SystemExit("pmg_compare needs a GPU (no timing is taken without one)")
    torch.cuda.set_device(0)
    tails = [int(t) for t in a.tail.split(",") if t]
    if tails and not a.hlevels:
        raise SystemExit("--tail needs --hlevels (the tail without h-levels is not measured)")
    transfers = [t for t in a.transfer.split(",") if t]
    if not transfers or set(transfers) - {"cell", "row"} or "cell" not in transfers:
        raise SystemExit("--transfer takes cell or cell,row (cell is the yardstick)")
    q1s = [t for t in a.q1.split(",") if t]
    if not q1s or set(q1s) - {"matfree", "stencil"} or "matfree" not in q1s:
        raise SystemExit("--q1 takes matfree or matfree,stencil (matfree is the yardstick)")
    asms = [t for t in a.q1_assembly.split(",") if t]
    if not asms or set(asms) - {"csr", "direct"} or "csr" not in asms:
        raise SystemExit("--q1-assembly takes csr or csr,direct (csr is the yardstick)")
    if "direct" in asms and "stencil" not in q1s:
        raise SystemExit("--q1-assembly csr,direct needs --q1 matfree,stencil")
    nx = compute_mesh_size(a.ndofs, a.degree)
    if a.transfer_kernels:
        print(json.dumps(transfer_kernels(a, nx)), flush=True)
        return 0
    pb = PoissonProblem(Comm(), nx, a.degree, 1, False, torch.float64, "gpu", a.perturb, a.kappa)
    b = pb.assemble_rhs()

    def pmg_kwargs(variant):
        """The PMultigrid options a variant's name spells: [h]pmg[32][_tN][_row][_s27[d]]."""
        kw = {}
        if variant.endswith("_s27d"):
            kw["q1_assembly"], variant = "direct", variant[:-1]
        if variant.endswith("_s27"):
            kw["q1_operator"], variant = "stencil", variant[:-4]
        if variant.endswith("_row"):
            kw["p_transfer"], variant = "row", variant[:-4]
        base, _, n = variant.partition("_t")
        if n:
            kw["tail_nodes"] = int(n)
        if base.startswith("hpmg"):
            kw["h_levels"] = a.hlevels
        if base.endswith("32"):
            kw["cycle_dtype"] = torch.float32
        return kw

    build_s = {}

    def make(variant):
        op = make_operator(pb)
        if variant == "cg_fused":
            cg = DeviceCG(pb)
        elif variant == "pcg_fused":
            cg = DeviceCG(pb, "jacobi", loop="fused")
        else:
            t0 = time.perf_counter()
            hierarchy = PMultigrid(pb, **pmg_kwargs(variant))
            torch.cuda.synchronize()
            build_s[variant] = time.perf_counter() - t0
            cg = DeviceCG(pb, "pmg", pmg=hierarchy)
        x = pb.new_vector()
        cg.start(op, x, b)
        return op, cg, x

    variants = (() if a.no_yardsticks else ("cg_fused", "pcg_fused")) + ("pmg",) + (
        ("hpmg",) if a.hlevels else ())
    if a.cycle_float == 32:
        variants += ("pmg32",) + (("hpmg32",) if a.hlevels else ())
    for n in tails:
        variants += (f"hpmg_t{n}",) + ((f"hpmg32_t{n}",) if a.cycle_float == 32 else ())
    if "row" in transfers:
        variants += tuple(f"{v}_row" for v in variants if "pmg" in v)
    if "stencil" in q1s:
        variants += tuple(f"{v}_s27" for v in variants if "pmg" in v)
    if "direct" in asms:
        variants += tuple(f"{v}d" for v in variants if v.endswith("_s27"))
    solves = tuple(v for v in variants if "pmg" in v)
    state = {v: make(v) for v in variants}
    pmg = state["pmg"][1].pmg

    def window(v):
        steps = state[v][1].iterate_timed(a.iters)
        torch.cuda.synchronize()
        return sum(steps[:-1]) / (len(steps) - 1)

    for _ in range(2):
        for v in variants:
            window(v)
    samples = {v: [] for v in variants}
    for _ in range(a.windows):
        for v in variants:
            samples[v].append(window(v))
    ms = {v: {"median": statistics.median(s), "min": min(s), "max": max(s)}
          for v, s in samples.items()}

    iters, iters2 = {}, {}
    for v in variants:
        op, cg, x = state[v]
        cg.start(op, x.zero_(), b)
        rr0 = cg.residual_norm2()
        k = 0
        while k < a.max_iter:
            cg.iterate(1)
            k += 1
            if cg.residual_norm2() < a.tol * a.tol * rr0:
                break
        iters[v] = k if k < a.max_iter else None
        if a.tol2 > 0 and v in solves and iters[v]:
            while k < a.max_iter and cg.residual_norm2() >= a.tol2 * a.tol2 * rr0:
                cg.iterate(1)
                k += 1
            iters2[v] = k if k < a.max_iter else None

    # pmg (and hpmg): the whole solve, wall clock, the variants alternating
    wall = {v: [] for v in solves if iters[v]}
    true_res = {}
    for _ in range(3):
        for v in wall:
            op, cg, x = state[v]
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cg.start(op, x, b)
            cg.iterate(iters[v])
            torch.cuda.synchronize()
            wall[v].append(time.perf_counter() - t0)
    for v in wall:
        op, cg, x = state[v]
        y = pb.new_vector()
        op.apply(x.clone(), y)
        true_res[v] = pb.norm(b - y) / pb.norm(b)
    # the same to the second tolerance
    wall2 = {v: [] for v in solves if iters2.get(v)}
    true_res2 = {}
    for _ in range(3):
        for v in wall2:
            op, cg, x = state[v]
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cg.start(op, x, b)
            cg.iterate(iters2[v])
            torch.cuda.synchronize()
            wall2[v].append(time.perf_counter() - t0)
    for v in wall2:
        op, cg, x = state[v]
        y = pb.new_vector()
        op.apply(x.clone(), y)
        true_res2[v] = pb.norm(b - y) / pb.norm(b)

    # the V-cycle's parts, each alone
    def timed(fn):
        out = []
        fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / 5)
        return statistics.median(out)

    lv = pmg.levels[0]
    r, z = state["pmg"][1].r, state["pmg"][1].z
    coef = lv.coef[-1]
    parts = {"cycle": timed(lambda: pmg.apply(r, z)),
             "fine_apply": timed(lambda: lv.op.apply(z, lv.y)),
             "cheb_step": timed(lambda: lv.k.cheb_step(False, coef[0], coef[1], lv.dinv, r, lv.y,
                                                       lv.d, z)),
             "cheb_step_first": timed(lambda: lv.k.cheb_step(True, 0.0, coef[1], lv.dinv, r, None,
                                                             lv.d, z)),
             "axpy": timed(lambda: lv.k.axpy(lv.t, -1.0, lv.y, r))}
    bw = {}
    if len(pmg.levels) > 1:
        nxt = pmg.levels[1]
        parts["restrict"] = timed(lambda: pmg.restrict(0, lv.t, nxt.r))
        parts["prolong"] = timed(lambda: pmg.prolong(0, nxt.z, lv.t))
        parts["restrict_kernel"] = timed(lambda: lv.k.restrict(nxt.latd, lv.J, lv.t, nxt.r))
        parts["coarse_levels"] = timed(lambda: pmg._vcycle(1, nxt.r, nxt.z))
        nc_ = nxt.pb.lat.ndofs_local
        nf_ = pb.lat.ndofs_local
        bw["prolong_tb_s"] = 8 * (nc_ + nf_) / (parts["prolong"] * 1e-3) / 1e12
        bw["restrict_kernel_tb_s"] = 8 * (nf_ + 2 * nc_) / (parts["restrict_kernel"] * 1e-3) / 1e12
    hparts = None
    if "hpmg" in state and state["hpmg"][1].pmg.h_levels:
        # the degree-1 level and everything below it, without and with h-levels,
        # and the first h-pair's transfer kernels alone
        hp = state["hpmg"][1].pmg
        i1 = len(hp.degrees) - 1
        f1, c1 = hp.levels[i1], hp.levels[i1 + 1]
        p1 = pmg.levels[i1]
        if i1 > 0:
            parts["degree1_level"] = timed(lambda: pmg._vcycle(i1, p1.r, p1.z))
        hparts = {"cycle": timed(lambda: hp.apply(r, z)),
                  "hrestrict_y": timed(lambda: f1.k.hrestrict(c1.latd, f1.H, f1.t, f1.y, c1.r)),
                  "hprolong": timed(lambda: f1.k.hprolong(c1.latd, f1.H, c1.z, f1.t, False)),
                  "hprolong_add": timed(lambda: f1.k.hprolong(c1.latd, f1.H, c1.z, f1.t, True))}
        if i1 > 0:
            hparts["degree1_and_h_levels"] = timed(lambda: hp._vcycle(i1, f1.r, f1.z))
        n1, n2 = f1.pb.lat.ndofs_local, c1.pb.lat.ndofs_local
        bw["hrestrict_y_tb_s"] = 8 * (2 * n1 + n2) / (hparts["hrestrict_y"] * 1e-3) / 1e12
        bw["hprolong_tb_s"] = 8 * (n1 + n2) / (hparts["hprolong"] * 1e-3) / 1e12
        bw["hprolong_add_tb_s"] = 8 * (2 * n1 + n2) / (hparts["hprolong_add"] * 1e-3) / 1e12
        hparts["pair_dofs"] = [n1, n2]
    nown = pb.lat.ndofs_owned
    bw["cheb_step_tb_s"] = 8 * 7 * nown / (parts["cheb_step"] * 1e-3) / 1e12
    bw["cheb_step_first_tb_s"] = 8 * 4 * nown / (parts["cheb_step_first"] * 1e-3) / 1e12
    napply = 2 * len(lv.coef)  # pre: k - 1, residual: 1, post: k
    parts["fine_applies_per_cycle"] = napply if len(pmg.levels) > 1 else len(lv.coef) - 1

    n = pb.new_vector().numel()
    sr, sy = (torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(2))
    stream_ms = timed(lambda: sr.add_(sy, alpha=-1e-9))
    stream_tbs = 3 * 8 * n / (stream_ms * 1e-3) / 1e12

    rec = {"degree": a.degree, "perturb": a.perturb, "kappa": a.kappa, "mesh": list(nx),
           "ndofs": pb.ndofs_global, "kernel": state["pmg"][0].name,
           "level_kernels": [getattr(v.op, "name", type(v.op).__name__) for v in pmg.levels],
           "pmg": pmg.info(), "ms_per_iter": ms, "tol": a.tol, "iters_to_tol": iters,
           "time_to_tol_s": {v: (iters[v] * ms[v]["median"] * 1e-3 if iters.get(v) else None)
                             for v in iters},
           "pmg_wall_s": {"median": statistics.median(wall["pmg"]), "min": min(wall["pmg"]),
                          "max": max(wall["pmg"])} if "pmg" in wall else None,
           "pmg_true_residual": true_res.get("pmg"), "cycle_parts_ms": parts, "bandwidth": bw,
           "stream_2r1w": {"ms": stream_ms, "tb_per_s": stream_tbs},
           "device": torch.cuda.get_device_name(0)}
    def spread(s):
        return {"median": statistics.median(s), "min": min(s), "max": max(s)}

    if a.tol2 > 0:
        rec["tol2"] = {"tol": a.tol2, "iters": iters2, "true_residual": true_res2,
                       "wall_s": {v: spread(s) for v, s in wall2.items()}}
    if "row" in transfers:
        rec["transfer"] = {v: {"info": state[v][1].pmg.info(), "yardstick": v[:-4],
                               "wall_s": spread(wall[v]) if v in wall else None,
                               "true_residual": true_res.get(v)}
                           for v in variants if v.endswith("_row")}
    if "stencil" in q1s:
        rec["q1"] = {}
        for v in variants:
            if not v.endswith("_s27"):
                continue
            sp, mp = state[v][1].pmg, state[v[:-4]][1].pmg
            i1 = next(i for i, lv in enumerate(sp.levels) if lv.pb.degree == 1)
            blk = {"info": sp.info(), "yardstick": v[:-4],
                   "wall_s": spread(wall[v]) if v in wall else None,
                   "true_residual": true_res.get(v),
                   "build_s": {"matfree": build_s[v[:-4]], "stencil": build_s[v]},
                   "level_nodes": [int(lv.pb.lat.L[0] * lv.pb.lat.L[1] * lv.pb.lat.L[2])
                                   for lv in sp.levels],
                   "stencil_bytes": [int(lv.S.numel() * lv.S.element_size()) if lv.S is not None
                                     else 0 for lv in sp.levels]}
            if i1 > 0:
                s1, m1 = sp.levels[i1], mp.levels[i1]
                blk["degree1_and_below_ms"] = {
                    "matfree": timed(lambda: mp._vcycle(i1, m1.r, m1.z)),
                    "stencil": timed(lambda: sp._vcycle(i1, s1.r, s1.z))}
            blk["levels"] = []
            for sl, ml in zip(sp.levels, mp.levels):
                if sl.S is None or sl.r is None:
                    continue
                ca, cb = sl.coef[-1]
                size, n = sl.S.element_size(), int(sl.pb.lat.ndofs_local)

                def composed():
                    ml.op.apply(ml.z, ml.y)
                    ml.k.cheb_step(False, ca, cb, ml.dinv, ml.r, ml.y, ml.d, ml.z)

                t = {"matfree_apply": timed(lambda: ml.op.apply(ml.z, ml.y)),
                     "stencil27_apply": timed(lambda: sl.k.stencil27_apply(sl.S, sl.z, sl.y)),
                     "matfree_apply_cheb_step": timed(composed),
                     "stencil27_cheb": timed(lambda: sl.k.stencil27_cheb(
                         sl.S, sl.dinv, sl.r, sl.z, sl.d, sl.t, ca, cb))}
                blk["levels"].append({
                    "nodes": n, "float": 8 * size, "ms": t,
                    "tb_per_s": {"stencil27_apply": 29 * n * size / (t["stencil27_apply"] * 1e-3) / 1e12,
                                 "stencil27_cheb": 33 * n * size / (t["stencil27_cheb"] * 1e-3) / 1e12}})
            rec["q1"][v] = blk
    if "direct" in asms:
        rec["q1_assembly"] = {}
        for v in variants:
            if not v.endswith("_s27d"):
                continue
            dp, y = state[v][1].pmg, v[:-1]
            kws = {"matfree": pmg_kwargs(y[:-4]), "csr": pmg_kwargs(y), "direct": pmg_kwargs(v)}
            built = {k: [] for k in kws}
            for _ in range(a.reps):
                for k, kw in kws.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h = PMultigrid(pb, **kw)
                    torch.cuda.synchronize()
                    built[k].append(time.perf_counter() - t0)
                    h.close()
                    del h
            blk = {"info": dp.info(), "yardstick": y,
                   "iters_to_tol": {y: iters.get(y), v: iters.get(v)},
                   "ms_per_iter": {y: ms[y], v: ms[v]},
                   "build_s": {k: spread(t) for k, t in built.items()},
                   "build_s_all": built,
                   "direct_faster_every_rep": all(d < c for d, c in zip(built["direct"],
                                                                        built["csr"])),
                   "levels": []}
            for dl in dp.levels:
                if dl.S is None:
                    continue
                lpb, size = dl.pb, dl.S.element_size()
                nodes = int(lpb.lat.L[0] * lpb.lat.L[1] * lpb.lat.L[2])
                t = timed(lambda: lpb.kernels.stencil27_assemble(lpb.xv, lpb.kappa, lpb.kc, dl.S))
                flops = 8 * lpb.tables.nq ** 3 * 337 * nodes
                store_ms = 27 * dl.S.shape[1] * size / (stream_tbs * 1e12) * 1e3
                blk["levels"].append({"nodes": nodes, "float": 8 * size, "nq": lpb.tables.nq,
                                      "assemble_ms": t, "model_tflops": flops / (t * 1e-3) / 1e12,
                                      "store_ms_at_stream_rate": store_ms,
                                      "ratio_to_store": t / store_ms})
            rec["q1_assembly"][v] = blk
    if tails:
        # per tailed variant: the whole cycle, and the tail's one call against the
        # untailed hierarchy's `_vcycle` from the same level (the launches it replaces)
        rec["tail"] = {}
        for v in variants:
            if "_t" not in v or v.endswith(("_row", "_s27", "_s27d")):
                continue
            tp = state[v][1].pmg
            up = state[v.partition("_t")[0]][1].pmg
            blk = {"info": tp.info(), "wall_s": spread(wall[v]) if v in wall else None,
                   "true_residual": true_res.get(v),
                   "level_nodes": [int(lv.pb.lat.L[0] * lv.pb.lat.L[1] * lv.pb.lat.L[2])
                                   for lv in tp.levels]}
            if tp.mixed:
                blk["cycle_ms"] = timed(lambda: tp.apply_cycle(tp.rc, tp.zc))
            else:
                blk["cycle_ms"] = timed(lambda: tp.apply(r, z))
            if tp.tail is not None and tp.tail_start > 0:
                s0 = tp.tail_start
                tl, ul = tp.levels[s0], up.levels[s0]
                blk["tail_call_ms"] = timed(lambda: tl.k.pmg_tail(tp.tail, tl.r, tl.z))
                blk["untailed_levels_ms"] = timed(lambda: up._vcycle(s0, ul.r, ul.z))
            rec["tail"][v] = blk
            tp.close()
    if a.cycle_float == 32:
        # the mixed variants, and the kernels of the precision boundary alone:
        # bytes per owned dof a kernel must move (f64 8, f32 4)
        cg32 = state["pmg32"][1]
        m32 = cg32.pmg
        k, p_, y_ = pb.kernels, cg32.p, cg32.y
        scal = torch.ones(8, dtype=torch.float64, device="cuda")
        xs = pb.new_vector()
        kern = {
            "demote": (12, lambda: k.demote(r, m32.rc)),
            "promote": (12, lambda: k.promote(m32.zc, z)),
            "cg_update_demote": (52, lambda: k.cg_update_demote(xs, r, p_, y_, scal, 0, 1, 5,
                                                                cg32.partials, m32.rc)),
            "cg_update": (48, lambda: k.cg_update(xs, r, p_, y_, scal, 0, 1, 5, cg32.partials)),
            "dot_f64_f32": (12, lambda: k.dot_f64_f32(r, m32.zc, cg32.partials, scal, 5)),
            "dot": (16, lambda: k.dot(r, z, cg32.partials, scal, 5)),
            "p_update_f64_f32": (20, lambda: k.p_update_f64_f32(p_, m32.zc, scal, 6, 7)),
            "p_update": (24, lambda: k.p_update(p_, z, scal, 6, 7)),
        }
        mk = {}
        for name, (nbytes, fn) in kern.items():
            t = timed(fn)
            mk[name] = {"ms": t, "bytes_per_dof": nbytes,
                        "tb_per_s": nbytes * nown / (t * 1e-3) / 1e12}
        rec["mixed"] = {"pmg32": m32.info(), "kernels": mk,
                        "cycle_ms": {"pmg": parts["cycle"],
                                     "pmg32": timed(lambda: m32.apply_cycle(m32.rc, m32.zc))},
                        "wall_s": {v: spread(wall[v]) for v in ("pmg32", "hpmg32") if v in wall},
                        "true_residual": {v: true_res[v] for v in ("pmg32", "hpmg32")
                                          if v in true_res}}
        if "hpmg32" in state:
            h32 = state["hpmg32"][1].pmg
            rec["mixed"]["hpmg32"] = h32.info()
            rec["mixed"]["cycle_ms"]["hpmg"] = hparts["cycle"] if hparts else None
            rec["mixed"]["cycle_ms"]["hpmg32"] = timed(lambda: h32.apply_cycle(h32.rc, h32.zc))
            h32.close()
        m32.close()
    if "hpmg" in state:
        hp = state["hpmg"][1].pmg
        rec["hpmg"] = hp.info()
        rec["hpmg_level_kernels"] = [getattr(v.op, "name", type(v.op).__name__) for v in hp.levels]
        rec["hpmg_wall_s"] = {"median": statistics.median(wall["hpmg"]), "min": min(wall["hpmg"]),
                              "max": max(wall["hpmg"])} if "hpmg" in wall else None
        rec["hpmg_true_residual"] = true_res.get("hpmg")
        rec["hpmg_parts_ms"] = hparts
        hp.close()
    for v in variants:
        if v.endswith(("_row", "_s27", "_s27d")):
            state[v][1].pmg.close()
    pmg.close()
    for op, _, _ in state.values():
        op.close()
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
