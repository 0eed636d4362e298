"""bench.py's plain run and its options: a plain run times the headline only
(no action check, companions, variants, phase profile or box probe: those
need --full), --steps sets the number of timed steps, and --dump-outputs
writes what the timed steps computed as float64 .npy files, the same from run
to run.  Run here on the CPU platform (the GPU path is the same code)."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from benchmark_dolfinx_amd.parallel.comm import Comm  # noqa: E402

ARGS = ["--platform", "cpu", "--dofs-per-gpu", "20000", "--steps", "3", "--warmup", "1"]


def test_plain_run_times_the_headline_only():
    a = bench.parse_args(ARGS)
    assert not a.full and a.companions == "off" and a.extras == "off"
    assert a.box_probe == "off" and a.profile_steps == 0
    rec = bench.run(Comm(), a)
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["unit"] == "GDoF/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp64"
    # value and ms_per_step describe the same 3 timed steps
    ndofs = rec["config"]["global_batch"]
    assert abs(rec["value"] - ndofs / (1e6 * rec["ms_per_step"])) <= 1e-9 * rec["value"]
    assert not rec["companions"] and not rec["variants"]
    assert rec["q6_gdofs"] is None and rec["config"]["action_check"] is None
    assert rec["config"]["phases_ms"] is None and rec["config"]["box_stream"] is None
    assert rec["consistency"]["ok"] and not rec["consistency"]["pairs"]


def test_full_restores_the_secondary_defaults():
    a = bench.parse_args(ARGS + ["--full"])
    assert a.companions == "auto" and a.extras == "auto"
    assert a.box_probe == "on" and a.profile_steps == 5
    a = bench.parse_args(ARGS + ["--full", "--companions", "off", "--profile-steps", "0"])
    assert a.companions == "off" and a.profile_steps == 0 and a.extras == "auto"
    # turning a secondary measurement off is accepted without --full ...
    a = bench.parse_args(ARGS + ["--companions", "off", "--extras", "off", "--profile-steps", "0"])
    assert a.companions == "off" and a.extras == "off" and a.profile_steps == 0


@pytest.mark.parametrize("opt", [["--extras", "on"], ["--companions", "auto"],
                                 ["--box-probe", "on"], ["--profile-steps", "2"]])
def test_secondary_measurement_without_full_is_refused(opt, capsys):
    # ... asking for one is an error, not silently dropped
    with pytest.raises(SystemExit) as e:
        bench.parse_args(ARGS + opt)
    assert e.value.code == 2 and "needs --full" in capsys.readouterr().err


def _dump(tmp_path, name, extra=()):
    d = tmp_path / name
    rec = bench.run(Comm(), bench.parse_args(ARGS + ["--dump-outputs", str(d), *extra]))
    assert sorted(os.listdir(d)) == ["x.npy", "y_norm.npy"]
    return rec, np.load(d / "x.npy"), np.load(d / "y_norm.npy")


def test_dump_outputs_writes_the_iterate_of_the_last_step(tmp_path, monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    rec, x, yn = _dump(tmp_path, "a")
    assert x.dtype == np.float64 and yn.dtype == np.float64 and yn.shape == (1,)
    mesh = rec["config"]["mesh"]
    assert x.shape == tuple(3 * n + 1 for n in mesh)  # every owned dof, lattice order
    assert yn[0] == rec["config"]["y_norm"]
    assert abs(np.sqrt(np.sum(x * x)) - yn[0]) <= 1e-12 * yn[0]
    # the same arguments: the same inputs, hence the same outputs
    _, x2, yn2 = _dump(tmp_path, "b")
    assert np.abs(x - x2).max() <= 1e-13 * np.abs(x).max() and abs(yn2[0] - yn[0]) <= 1e-13 * yn[0]
    # ... also under --full (the action check does not touch the CG)
    _, x3, _ = _dump(tmp_path, "c", ["--full", "--companions", "off", "--profile-steps", "0"])
    assert np.abs(x - x3).max() <= 1e-13 * np.abs(x).max()
    # a different step count is a different iterate
    d = tmp_path / "d"
    bench.run(Comm(), bench.parse_args(ARGS[:-4] + ["--steps", "4", "--warmup", "1",
                                                    "--dump-outputs", str(d)]))
    assert np.abs(np.load(d / "x.npy") - x).max() > 1e-6 * np.abs(x).max()


@pytest.mark.gpu
def test_dump_outputs_on_the_gpu(tmp_path, monkeypatch):
    """The device path: the whole iterate of a small problem against the
    record's norm, and the seeded sample (gathered on the device) against the
    same positions of the whole one.  Two GPU runs agree to rounding."""
    args = ["--dofs-per-gpu", "200000", "--steps", "4", "--warmup", "2"]

    def dump(name):
        d = tmp_path / name
        rec = bench.run(Comm(), bench.parse_args(args + ["--dump-outputs", str(d)]))
        return rec, np.load(d / "x.npy"), np.load(d / "y_norm.npy")

    rec, x, yn = dump("whole")
    assert rec["steps"] == 4 and rec["ms_per_step"] > 0 and rec["config"]["action_check"] is None
    assert x.dtype == np.float64 and x.shape == tuple(3 * n + 1 for n in rec["config"]["mesh"])
    assert yn[0] == rec["config"]["y_norm"] > 0
    assert abs(np.sqrt(np.sum(x * x)) - yn[0]) <= 1e-12 * yn[0]
    monkeypatch.setattr(bench, "DUMP_FULL_MAX", 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    _, s, _ = dump("sample")
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, x.size, size=4096))
    assert s.shape == (4096,) and np.abs(s - x.ravel()[pos]).max() <= 1e-12 * np.abs(x).max()


def test_dump_outputs_samples_a_large_iterate(tmp_path, monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    _, x, _ = _dump(tmp_path, "whole")
    monkeypatch.setattr(bench, "DUMP_FULL_MAX", 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 512)
    _, s, _ = _dump(tmp_path, "sample")
    assert s.dtype == np.float64 and s.shape == (512,)
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, x.size, size=512))
    assert np.abs(s - x.ravel()[pos]).max() <= 1e-13 * np.abs(x).max()
    _, s2, _ = _dump(tmp_path, "sample2")
    assert np.abs(s - s2).max() <= 1e-13 * np.abs(x).max()  # the same positions every run
