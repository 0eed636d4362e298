#!/usr/bin/env python3
"""Fused Jacobi-PCG against the generic PCG loop and unpreconditioned fused CG
on one GPU: one JSON line per configuration (profiles/jacobi_pcg_fused.md).

  python scripts/pcg_fused_compare.py --degree 3 --perturb 0.2 [--ndofs 20000000]
  python scripts/pcg_fused_compare.py --degree 6 --perturb 0.2
  python scripts/pcg_fused_compare.py --degree 3 --perturb 0.0 [--ndofs 300000000]

One process per configuration.  FP64, qmode 1 (GLL), random per-cell kappa.
Three variants, each on its own auto-selected operator (fused3 on the perturbed
mesh, fused5 on the box):

  cg_fused     DeviceCG(pb)                          fused CG, native runtime
  pcg_generic  DeviceCG(pb, "jacobi")                op.apply + dot + update + p-update
  pcg_fused    DeviceCG(pb, "jacobi", loop="fused")  fused CG fusion with z = dinv . r

Timing: device events between the steps of `iterate_timed(n)`; per window the
mean of the first n - 1 steps (the last carries the loop's final x flush), per
variant the median over the windows, with min and max.  The variants are
interleaved window by window after two warm-up windows each.  `update_rr` is
the phase of that name from the runtime's `profile()` (eager iterations with
events between the phases).  Iterations to the tolerance use the recurrence
residual (`residual_norm2()` read back after every iteration, outside the
timed windows); the time to the tolerance is computed: iterations x ms per
iteration.  The box's stream rate is a 2-read 1-write torch update of vectors
of the problem's size.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--ndofs", type=int, default=20_000_000)
    ap.add_argument("--perturb", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=6000)
    ap.add_argument("--no-converge", action="store_true", help="skip the runs to the tolerance")
    a = ap.parse_args(argv)

    import torch

    from benchmark_dolfinx_amd.driver import make_operator
    from benchmark_dolfinx_amd.fem.mesh import compute_mesh_size
    from benchmark_dolfinx_amd.models.poisson import PoissonProblem
    from benchmark_dolfinx_amd.parallel.comm import Comm
    from benchmark_dolfinx_amd.solvers.cg import DeviceCG

    if not torch.cuda.is_available():
        raise SystemExit("pcg_fused_compare needs a GPU (no timing is taken without one)")
    torch.cuda.set_device(0)
    nx = compute_mesh_size(a.ndofs, a.degree)
    pb = PoissonProblem(Comm(), nx, a.degree, 1, False, torch.float64, "gpu", a.perturb, "random")
    b = pb.assemble_rhs()

    def make(variant):
        op = make_operator(pb)
        if variant == "cg_fused":
            cg = DeviceCG(pb)
        elif variant == "pcg_generic":
            cg = DeviceCG(pb, "jacobi")
        else:
            cg = DeviceCG(pb, "jacobi", loop="fused")
        x = pb.new_vector()
        cg.start(op, x, b)
        return op, cg, x

    variants = ("cg_fused", "pcg_generic", "pcg_fused")
    state = {v: make(v) for v in variants}
    kernel = state["cg_fused"][0].name
    tiled = {v: bool(getattr(state[v][0]._rt, "tiled", False)) if state[v][0]._rt else None
             for v in variants}

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

    # the update pass with and without the preconditioner (eager, phase events)
    phases = {}
    for v in ("cg_fused", "pcg_fused"):
        op, cg, x = state[v]
        cg.start(op, x.zero_(), b)
        ph = op._rt.profile(a.iters)
        phases[v] = {"update_rr": ph["update_rr"], "iteration": ph["iteration"],
                     "op_interior": ph["op_interior"]}

    # stream rate of the box at this vector size (2 reads + 1 write)
    n = pb.new_vector().numel()
    r, y = (torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(2))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    r.add_(y, alpha=-1e-9)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        r.add_(y, alpha=-1e-9)
    e1.record()
    torch.cuda.synchronize()
    stream_ms = e0.elapsed_time(e1) / 20
    stream_tbs = 3 * 8 * n / (stream_ms * 1e-3) / 1e12
    del r, y

    iters = {}
    if not a.no_converge:
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

    rec = {"degree": a.degree, "perturb": a.perturb, "mesh": list(nx), "ndofs": pb.ndofs_global,
           "kernel": kernel, "tiled": tiled, "iters_per_window": a.iters, "windows": a.windows,
           "ms_per_iter": ms, "phases_ms": phases,
           "stream_2r1w": {"ms": stream_ms, "tb_per_s": stream_tbs},
           "tol": a.tol, "iters_to_tol": iters,
           "time_to_tol_s": {v: (iters[v] * ms[v]["median"] * 1e-3 if iters.get(v) else None)
                             for v in iters},
           "device": torch.cuda.get_device_name(0)}
    for op, _, _ in state.values():
        op.close()
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
