"""`bench_dolfinx` command line (same options, console lines and JSON as the
reference's src/main.cpp:136-320).

Run:  python -m benchmark_dolfinx_amd [options]
      torchrun --nproc-per-node N -m benchmark_dolfinx_amd [options]

Reference options (src/main.cpp:144-183): --platform, --float, --ndofs,
--ndofs_global, --qmode, --cg, --nreps, --degree, --mat_comp,
--geom_perturb_fact, --use_gauss, --json.  Unknown options are accepted
(like `allow_unregistered`, used for `SPDLOG_LEVEL=...`).

MI355X extensions (additive): --kernel {auto,fused5,fused3,fused2,
fused,v1,dofmap}, --geometry {auto,otf,otf-general,stored}, --kappa {constant,random},
--warmup N (untimed repetitions before the timed loop), --precond {none,jacobi,pmg}
(with --cg: CG preconditioned with the matrix-free operator diagonal, or with
a p-multigrid V-cycle; --pmg_smooth N / --pmg_coarse N: Chebyshev degree of
its smoothers / of its coarsest-level solve; --pmg_hlevels N: geometric
h-levels under its degree-1 level, -1 = as many as the mesh allows;
--pmg_float {32,64}: precision of its V-cycle, 32 under --float 64 = the
mixed-precision solve; --pmg_tail N: its trailing degree-1 levels of at most
N nodes run in one kernel launch, one rank only; --pmg_transfer {cell,row}:
the transfer kernels between its p-levels, row = the row-streaming ones that
fold the residual and the update; --pmg_q1 {matfree,stencil}: the operator
of its degree-1 levels, stencil = their assembled 27-point stencils streamed,
with the Chebyshev step fused into the apply on one rank; --pmg_q1_assembly
{csr,direct}: how those stencils and the tail's are built, direct = by the
assembly kernel on the device instead of the host's CSR matrix),
--pcg_loop {generic,fused} (with --cg --precond jacobi on the GPU: the generic
device loop, or the fused operators' CG fusion and native runtime).
The JSON gains an additive "mi355x" object; the reference keys are
unchanged.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

BANNER = """DOLFINx benchmark (MI355X-native)
-----------------

  Finite Element Operator Action Benchmark which computes
  the Laplacian operator on a cube mesh of hexahedral elements.
"""


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="bench_dolfinx", description=BANNER,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--platform", default=None, help="Compute platform (cpu or gpu)")
    ap.add_argument("--float", type=int, default=64, help="Float size (bits). 32 or 64.")
    ap.add_argument("--ndofs", type=int, default=None,
                    help="Number of degrees-of-freedom per process (default 1000)")
    ap.add_argument("--ndofs_global", type=int, default=None,
                    help="Number of global degrees-of-freedom")
    ap.add_argument("--qmode", type=int, default=1,
                    help="Quadrature mode (0 or 1): qmode=0 has P+1 points in each "
                         "direction, qmode=1 has P+2 points in each direction.")
    ap.add_argument("--cg", action="store_true",
                    help="Do CG iterations, rather than simple operator action")
    ap.add_argument("--nreps", type=int, default=1000, help="Number of repetitions")
    ap.add_argument("--degree", type=int, default=3, help='Polynomial degree "P" (1-7)')
    ap.add_argument("--mat_comp", action="store_true",
                    help="Compare result to matrix operator (slow with large ndofs)")
    ap.add_argument("--geom_perturb_fact", type=float, default=0.0,
                    help="Randomly perturb the geometry (useful to check correctness)")
    ap.add_argument("--use_gauss", action="store_true",
                    help="Use Gauss quadrature rather than GLL quadrature")
    ap.add_argument("--json", default="", help="Filename for JSON output")
    # MI355X extensions
    ap.add_argument("--kernel", default="auto",
                    choices=["auto", "fused5", "fused3", "fused2", "fused", "v1", "dofmap"],
                    help="GPU operator kernel: fused structured kernel, the generic v1, or the "
                         "unstructured dofmap data model")
    ap.add_argument("--geometry", default="auto", choices=["auto", "otf", "otf-general", "stored"],
                    help="Geometry factors on the fly (otf: constant-Jacobian fast path for "
                         "parallelepiped cells; otf-general: always the trilinear path) or "
                         "precomputed (stored, the reference's layout)")
    ap.add_argument("--kappa", default="constant", choices=["constant", "random"],
                    help="Diffusion coefficient: the reference's constant 2.0, or a random "
                         "per-cell field U(1, 3) (partition-invariant)")
    ap.add_argument("--warmup", type=int, default=0,
                    help="Untimed repetitions before the timed loop")
    ap.add_argument("--precond", default="none", choices=["none", "jacobi", "pmg"],
                    help="CG preconditioner (needs --cg): jacobi = the inverse of the "
                         "matrix-free operator diagonal; pmg = one p-multigrid V-cycle over "
                         "the degrees P, P // 2, ..., 1 with Chebyshev-Jacobi smoothing")
    ap.add_argument("--pmg_smooth", type=int, default=2,
                    help="Chebyshev degree of the p-multigrid smoothers (--precond pmg)")
    ap.add_argument("--pmg_coarse", type=int, default=8,
                    help="Chebyshev degree of the p-multigrid coarsest-level solve (degree 1, or "
                         "the last h-level; --precond pmg)")
    ap.add_argument("--pmg_hlevels", type=int, default=0,
                    help="Geometric h-levels under the p-multigrid's degree-1 level (--cg "
                         "--precond pmg): 0 = none, N = at most N, -1 = as many as the mesh allows")
    ap.add_argument("--pmg_float", type=int, default=None, choices=[32, 64],
                    help="Float size of the p-multigrid V-cycle (--cg --precond pmg; default: "
                         "--float): 32 with --float 64 runs the FP32 cycle inside the FP64 CG")
    ap.add_argument("--pmg_tail", type=int, default=0,
                    help="Run the trailing degree-1 levels of the p-multigrid V-cycle that have "
                         "at most N local nodes in one kernel launch (--cg --precond pmg, one "
                         "rank): 0 = off, N <= 32768")
    ap.add_argument("--pmg_transfer", default="cell", choices=["cell", "row"],
                    help="Transfer kernels between the p-multigrid's p-levels (--cg --precond "
                         "pmg): cell = per cell; row = by lattice rows, one restriction that "
                         "folds the residual and one prolongation that folds the update")
    ap.add_argument("--pmg_q1", default="matfree", choices=["matfree", "stencil"],
                    help="Operator of the p-multigrid's degree-1 levels, h-levels included (--cg "
                         "--precond pmg): matfree = the matrix-free kernels; stencil = the "
                         "assembled 27-point stencil, streamed")
    ap.add_argument("--pmg_q1_assembly", default="csr", choices=["csr", "direct"],
                    help="How the 27-point stencils of --pmg_q1 stencil and --pmg_tail are built "
                         "(--cg --precond pmg): csr = from the host's assembled matrix; direct = "
                         "by the assembly kernel on the problem's device, no matrix")
    ap.add_argument("--pcg_loop", default="generic", choices=["generic", "fused"],
                    help="Loop of the preconditioned CG (needs --cg --precond jacobi): generic = "
                         "operator apply + vector kernels; fused = the fused operators' CG "
                         "fusion driven by the native runtime (GPU platform, fused2/3/5)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args, unknown = ap.parse_known_args(argv)
    if args.ndofs is not None and args.ndofs_global is not None:
        raise SystemExit("error: Conflicting options 'ndofs' and 'ndofs_global'")
    if args.float not in (32, 64):
        raise SystemExit("error: Invalid float size. Must be 32 or 64.")
    if args.qmode > 1 or args.qmode < 0:
        raise SystemExit("error: Invalid qmode.")
    if args.pmg_float is not None and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_float' needs 'cg' and 'precond pmg'")
    if args.pmg_float is not None and args.pmg_float > args.float:
        raise SystemExit("error: Option 'pmg_float' cannot exceed 'float'")
    if args.pmg_tail < 0 or args.pmg_tail > 32768:
        raise SystemExit("error: Option 'pmg_tail' must be 0 or a node count up to 32768")
    if args.pmg_tail != 0 and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_tail' needs 'cg' and 'precond pmg'")
    if args.pmg_transfer != "cell" and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_transfer' needs 'cg' and 'precond pmg'")
    if args.pmg_q1 != "matfree" and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_q1' needs 'cg' and 'precond pmg'")
    if args.pmg_q1_assembly != "csr" and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_q1_assembly' needs 'cg' and 'precond pmg'")
    if args.pmg_q1_assembly != "csr" and args.pmg_q1 == "matfree" and args.pmg_tail == 0:
        raise SystemExit("error: Option 'pmg_q1_assembly' needs 'pmg_q1 stencil' or 'pmg_tail'")
    if args.precond != "none" and not args.cg:
        raise SystemExit("error: Option 'precond' needs 'cg'")
    if args.pmg_smooth < 1 or args.pmg_coarse < 1:
        raise SystemExit("error: Options 'pmg_smooth' and 'pmg_coarse' must be positive")
    if args.pmg_hlevels < -1:
        raise SystemExit("error: Option 'pmg_hlevels' must be -1, 0 or a positive count")
    if args.pmg_hlevels != 0 and not (args.cg and args.precond == "pmg"):
        raise SystemExit("error: Option 'pmg_hlevels' needs 'cg' and 'precond pmg'")
    if args.pcg_loop == "fused" and not args.cg:
        raise SystemExit("error: Option 'pcg_loop fused' needs 'cg'")
    if args.pcg_loop == "fused" and args.precond != "jacobi":
        raise SystemExit("error: Option 'pcg_loop fused' needs 'precond jacobi'")
    return args, unknown


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    args, unknown = parse_args(argv)

    import torch

    from .fem.mesh import compute_mesh_size
    from .parallel.comm import finalize, init_distributed
    from .utils.log import init_logging
    from .utils.timing import list_timings

    platform = args.platform
    if platform is None:
        platform = "gpu" if torch.cuda.is_available() else "cpu"
    if platform not in ("cpu", "gpu"):
        raise RuntimeError("Invalid platform: " + platform)
    if args.pcg_loop == "fused" and platform != "gpu":
        raise SystemExit("error: Option 'pcg_loop fused' needs the gpu platform")
    comm = init_distributed(platform)
    if args.pmg_tail != 0 and comm.size > 1:
        finalize()
        raise SystemExit("error: Option 'pmg_tail' needs a single rank")
    log = init_logging(unknown, comm.rank)
    size = comm.size
    ndofs = args.ndofs if args.ndofs is not None else 1000
    if args.ndofs_global is None:
        ndofs_global = ndofs * size
    else:
        ndofs_global = args.ndofs_global
        ndofs = ndofs_global // size

    rank0 = comm.rank == 0
    if rank0:
        if platform == "gpu":
            from .ops.kernels import device_info
            print(device_info(torch.cuda.current_device()), end="")
        print("-----------------------------------")
        print(f"Platform: {platform}")
        print(f"Polynomial degree : {args.degree}")
        print(f"Number of ranks : {size}")
        print(f"Requested number of local DoFs : {ndofs}")
        print(f"Number of repetitions : {args.nreps}")
        print(f"Scalar Type: {args.float}")
        print(f"Use Gauss-Jacobi: {int(args.use_gauss)}")
        print(f"Compare to matrix: {int(args.mat_comp)}")
        if args.precond != "none":
            print(f"Preconditioner: {args.precond}")
        print("-----------------------------------", flush=True)

    in_root = {"p": args.degree, "mpi_size": size, "ndofs_local_requested": ndofs,
               "nreps": args.nreps, "scalar_size": args.float, "use_gauss": args.use_gauss,
               "mat_comp": args.mat_comp, "qmode": args.qmode, "cg": args.cg}
    nx = compute_mesh_size(ndofs_global, args.degree)
    log.info("Mesh cells in each direction: %s", nx)
    out_root, extra = run_benchmark(comm, nx, args, platform)
    if rank0 and args.json:
        root = {"input": in_root, "output": out_root, "mi355x": extra}
        print(f"*** Writing output to:       {args.json}")
        print(f"*** Writing output to (abs): {os.path.abspath(args.json)}")
        with open(args.json, "w") as fh:
            fh.write(json.dumps(root) + "\n")
    elif rank0:
        print(f"*** Empty file: {args.json}")
    table = list_timings(comm)
    if rank0:
        print(table, flush=True)
    finalize()
    return 0


def _device_name() -> str:
    import torch

    from .ops.kernels import device_name
    return device_name(torch.cuda.current_device())


def _build_flags() -> dict:
    from .ops.native import build_flags
    return build_flags()


def run_benchmark(comm, nx, args, platform):
    import torch

    from .driver import laplace_action
    from .models.poisson import PoissonProblem

    dtype = torch.float64 if args.float == 64 else torch.float32
    pb = PoissonProblem(comm, nx, args.degree, args.qmode, args.use_gauss, dtype,
                        platform, args.geom_perturb_fact, args.kappa)
    pmg_opts = {"smooth_degree": args.pmg_smooth, "coarse_degree": args.pmg_coarse,
                "h_levels": args.pmg_hlevels}
    if args.pmg_float is not None:
        pmg_opts["cycle_dtype"] = torch.float64 if args.pmg_float == 64 else torch.float32
    if args.pmg_tail != 0:
        pmg_opts["tail_nodes"] = args.pmg_tail
    if args.pmg_transfer != "cell":
        pmg_opts["p_transfer"] = args.pmg_transfer
    if args.pmg_q1 != "matfree":
        pmg_opts["q1_operator"] = args.pmg_q1
    if args.pmg_q1_assembly != "csr":
        pmg_opts["q1_assembly"] = args.pmg_q1_assembly
    res = laplace_action(pb, args.nreps, args.cg, args.mat_comp, kernel=args.kernel,
                         geometry=args.geometry, warmup=args.warmup, precond=args.precond,
                         pcg_loop=args.pcg_loop,
                         pmg_opts=pmg_opts)
    t = res.mat_free_time
    gdofs = pb.ndofs_global * args.nreps / (1e9 * t) if t > 0 else 0.0
    out = {"ncells_global": pb.ncells_global, "ndofs_global": pb.ndofs_global,
           "mat_free_time": t, "u_norm": res.unorm, "y_norm": res.ynorm,
           "z_norm": res.znorm, "gdof_per_second": gdofs}
    extra = {"gdof_per_second_per_gpu": gdofs / comm.size, "mesh": list(nx),
             "partition": list(pb.lat.pgrid), "e_norm": res.enorm,
             "device": _device_name() if platform == "gpu" else "cpu",
             "build_flags": _build_flags() if platform == "gpu" else None,
             **res.extra}
    return out, extra


if __name__ == "__main__":
    raise SystemExit(main())
