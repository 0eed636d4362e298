"""The launch sequence of `DeviceCG`'s generic loops, kernel by kernel: a CPU
problem whose `kernels`, operator, preconditioner and communicator are
recording stand-ins, so `start` + `iterate` leave a log of (launch, arguments)
that is compared with the sequences written out below.  Tensors are logged by
identity under the names x b r p y z dinv rc zc partials scal, scalar slots as
integers (RR0 RR1 PAP = 0 1 2, RNORM ZERO ONE = 5 6 7); "ar" is the all-reduce
of one slot."""

import gc
import weakref

import pytest
import torch

from benchmark_dolfinx_amd.models.poisson import PoissonProblem
from benchmark_dolfinx_amd.parallel.comm import Comm
from benchmark_dolfinx_amd.solvers.cg import DeviceCG


class Recorder:
    def __init__(self):
        self.log = []
        self.names = {}

    def name(self, **tensors):
        for n, t in tensors.items():
            if t is not None:
                self.names[id(t)] = n

    def arg(self, a):
        return self.names.get(id(a), "?") if isinstance(a, torch.Tensor) else a

    def call(self, what, *args):
        self.log.append((what, *(self.arg(a) for a in args)))


class RecKernels:
    """Every kernel call is logged and does nothing, except that axpy (the
    residual) fills its output with 2 so the prologue's p0 can be told apart."""
    npart = 8

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, what):
        def launch(*args):
            self._rec.call(what, *args)
            if what == "axpy":
                args[0].fill_(2.0)
        return launch


class RecComm:
    size = 2

    def __init__(self, rec):
        self._rec = rec

    def allreduce_(self, t):
        assert t.numel() == 1
        self._rec.call("ar", t.storage_offset())


class RecOp:
    def __init__(self, rec):
        self._rec = rec

    def apply(self, u, y):
        self._rec.call("apply", u, y)


class RecFusedOp(RecOp):
    """An operator with its own CG loop."""
    name = "rec"

    def __init__(self, rec, pcg):
        super().__init__(rec)
        self.supports_fused_pcg = pcg

    def cg_start(self, cg, x, b):
        self._rec.call("op.cg_start", x, b)

    def cg_iterate(self, cg, n, flush=True):
        self._rec.call("op.cg_iterate", n, flush)


class RecPmg:
    def __init__(self, rec, pb, mixed):
        self._rec, self.mixed = rec, mixed
        self.rc = torch.zeros(pb.lat.shape, dtype=torch.float32) if mixed else None
        self.zc = torch.zeros(pb.lat.shape, dtype=torch.float32) if mixed else None

    def apply(self, r, z):
        self._rec.call("pmg.apply", r, z)
        z.fill_(3.0)

    def apply_cycle(self, rc, zc):
        self._rec.call("pmg.apply_cycle", rc, zc)


def _setup(mode, op_cls=RecOp, loop="generic", **op_kw):
    rec = Recorder()
    pb = PoissonProblem(Comm(), (2, 2, 2), 2, 1, False, torch.float64, "cpu", 0.0, "constant")
    pb.jacobi_inverse()  # cached, with the real communicator
    pb.kernels, pb.comm = RecKernels(rec), RecComm(rec)
    pmg = RecPmg(rec, pb, mode == "mixed") if mode in ("pmg", "mixed") else None
    precond = {"plain": None, "jacobi": "jacobi", "pmg": "pmg", "mixed": "pmg"}[mode]
    cg = DeviceCG(pb, precond=precond, loop=loop, pmg=pmg)
    x, b = pb.new_vector(), pb.new_vector()
    rec.name(x=x, b=b, r=cg.r, p=cg.p, y=cg.y, z=cg.z, dinv=cg.dinv, partials=cg.partials,
             scal=cg.scal, rc=getattr(pmg, "rc", None), zc=getattr(pmg, "zc", None))
    return rec, cg, op_cls(rec, **op_kw), x, b


RESIDUAL = [("apply", "x", "y"), ("axpy", "r", -1.0, "y", "b")]
RNORM0 = [("dot", "r", "r", "partials", "scal", 5), ("ar", 5)]
HEAD = [("apply", "p", "y"), ("dot", "p", "y", "partials", "scal", 2), ("ar", 2)]

# mode -> (prologue after the residual, tail of an even iteration (cur, nxt =
# 0, 1), tail of an odd one (1, 0))
SEQUENCES = {
    "plain": (
        [("dot", "p", "r", "partials", "scal", 0), ("ar", 0)],
        [("cg_update", "x", "r", "p", "y", "scal", 0, 2, 1, "partials"), ("ar", 1),
         ("p_update", "p", "r", "scal", 1, 0)],
        [("cg_update", "x", "r", "p", "y", "scal", 1, 2, 0, "partials"), ("ar", 0),
         ("p_update", "p", "r", "scal", 0, 1)],
    ),
    "jacobi": (
        [("pcg_p_update", "p", "r", "dinv", "scal", 6, 7),
         ("dot", "p", "r", "partials", "scal", 0), ("ar", 0)] + RNORM0,
        [("pcg_update", "x", "r", "p", "y", "dinv", "scal", 0, 2, 1, 5, "partials"), ("ar", 1),
         ("ar", 5), ("pcg_p_update", "p", "r", "dinv", "scal", 1, 0)],
        [("pcg_update", "x", "r", "p", "y", "dinv", "scal", 1, 2, 0, 5, "partials"), ("ar", 0),
         ("ar", 5), ("pcg_p_update", "p", "r", "dinv", "scal", 0, 1)],
    ),
    "pmg": (
        [("pmg.apply", "r", "z"), ("dot", "r", "z", "partials", "scal", 0), ("ar", 0)] + RNORM0,
        [("cg_update", "x", "r", "p", "y", "scal", 0, 2, 5, "partials"), ("ar", 5),
         ("pmg.apply", "r", "z"), ("dot", "r", "z", "partials", "scal", 1), ("ar", 1),
         ("p_update", "p", "z", "scal", 1, 0)],
        [("cg_update", "x", "r", "p", "y", "scal", 1, 2, 5, "partials"), ("ar", 5),
         ("pmg.apply", "r", "z"), ("dot", "r", "z", "partials", "scal", 0), ("ar", 0),
         ("p_update", "p", "z", "scal", 0, 1)],
    ),
    "mixed": (
        [("demote", "r", "rc"), ("pmg.apply_cycle", "rc", "zc"), ("promote", "zc", "p"),
         ("dot_f64_f32", "r", "zc", "partials", "scal", 0), ("ar", 0)] + RNORM0,
        [("cg_update_demote", "x", "r", "p", "y", "scal", 0, 2, 5, "partials", "rc"), ("ar", 5),
         ("pmg.apply_cycle", "rc", "zc"), ("dot_f64_f32", "r", "zc", "partials", "scal", 1),
         ("ar", 1), ("p_update_f64_f32", "p", "zc", "scal", 1, 0)],
        [("cg_update_demote", "x", "r", "p", "y", "scal", 1, 2, 5, "partials", "rc"), ("ar", 5),
         ("pmg.apply_cycle", "rc", "zc"), ("dot_f64_f32", "r", "zc", "partials", "scal", 0),
         ("ar", 0), ("p_update_f64_f32", "p", "zc", "scal", 0, 1)],
    ),
}
# p0 after `start` with r0 = 2 and M^-1 r0 = 3 from the stand-ins: r0, zero
# (before the recorded pcg_p_update), z0, and whatever `promote` wrote
P0 = {"plain": 2.0, "jacobi": 0.0, "pmg": 3.0, "mixed": 9.0}


@pytest.mark.parametrize("mode", list(SEQUENCES))
def test_generic_loop_launch_sequence(mode):
    prologue, even, odd = SEQUENCES[mode]
    rec, cg, op, x, b = _setup(mode)
    cg.p.fill_(9.0)
    cg.start(op, x, b)
    assert rec.log == RESIDUAL + prologue
    assert torch.all(cg.p == P0[mode])
    assert (cg.z is None) == (mode != "pmg") and cg.it == 0
    cg.iterate(3)
    assert rec.log == RESIDUAL + prologue + HEAD + even + HEAD + odd + HEAD + even
    assert cg.it == 3 and cg.x is x

    rec2, cg2, op2, x2, b2 = _setup(mode)
    cg2.start(op2, x2, b2)
    cg2.iterate(2)
    cg2.iterate(1)
    assert rec2.log == rec.log


@pytest.mark.parametrize("mode,loop", [("plain", "generic"), ("jacobi", "fused")])
def test_operator_loop_is_delegated(mode, loop):
    rec, cg, op, x, b = _setup(mode, RecFusedOp, loop, pcg=True)
    assert cg.fused_pcg == (loop == "fused") and (cg.p is None) == (loop == "fused")
    cg.start(op, x, b)
    cg.iterate(3)
    cg.iterate(2, flush=False)
    assert rec.log == [("op.cg_start", "x", "b"), ("op.cg_iterate", 3, True),
                       ("op.cg_iterate", 2, False)]


def test_generic_jacobi_ignores_operator_loop():
    rec, cg, op, x, b = _setup("jacobi", RecFusedOp, pcg=True)
    cg.start(op, x, b)
    cg.iterate(1)
    prologue, even, _ = SEQUENCES["jacobi"]
    assert rec.log == RESIDUAL + prologue + HEAD + even


@pytest.mark.parametrize("mode", list(SEQUENCES))
def test_state_goes_with_the_last_reference(mode):
    """No reference cycle through the mode's methods: the vectors of a solve
    (gigabytes at full size) are freed without waiting for the collector."""
    gc.collect()
    gc.disable()
    try:
        rec, cg, op, x, b = _setup(mode)
        cg.start(op, x, b)
        cg.iterate(1)
        gone = weakref.ref(cg)
        del cg
        assert gone() is None
    finally:
        gc.enable()


def test_fused_loop_needs_operator_support():
    for op_cls, kw in ((RecOp, {}), (RecFusedOp, {"pcg": False})):
        rec, cg, op, x, b = _setup("jacobi", op_cls, "fused", **kw)
        with pytest.raises(ValueError, match="no fused preconditioned CG loop"):
            cg.start(op, x, b)
        assert rec.log == []
