"""DifMachine::fused_trial_step (lm_machine.h) against the generic DifMachine::run, on the CPU.

tests/cpp/dif_fused_harness.cpp steps two DifMachine<3> through whole fits with the reference-order pass executor, one
by run() alone and one that tries the fused trial -> trial step first.  Both consume the same sums; after EVERY step the
whole hot state (CoreInts, CoreReals, Cool, Request) must be memcmp-equal, and p, info, covar, ret at the end.  The
harness is compiled here (g++ -O2 -ffp-contract=off) against oracle/liboracle.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from brdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("dif_fused") / "libdif_fused_harness.so"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-O2", "-fPIC", "-ffp-contract=off", "-std=c++17", "-shared", "-o", str(out),
                    os.path.join(ROOT, "tests", "cpp", "dif_fused_harness.cpp"), "-L" + oracle, "-loracle",
                    "-Wl,-rpath," + oracle, "-lm"], check=True)
    return C.CDLL(str(out))


def _pair(lib, model, angles, x, itmax=synth.ITMAX, delta=1e-6, multi=1, covar=1):
    """-> (code, steps, fused, trial_steps, p, info); code 0: identical after every step and at the end"""
    a = np.ascontiguousarray(np.asarray(angles, dtype=np.float64).reshape(-1))
    xx = np.ascontiguousarray(x, dtype=np.float64)
    p0 = np.array(synth.P0[model], dtype=np.float64)
    opts = np.array(synth.OPTS, dtype=np.float64)
    opts[4] = delta
    counts = (C.c_longlong * 3)()
    p, info = np.zeros(3), np.zeros(10)
    code = lib.dfh_fit_pair(model, a.ctypes.data_as(D), xx.ctypes.data_as(D), xx.size, p0.ctypes.data_as(D), itmax,
                            opts.ctypes.data_as(D), multi, covar, counts, p.ctypes.data_as(D), info.ctypes.data_as(D))
    return code, counts[0], counts[1], counts[2], p, info


@pytest.fixture(scope="module")
def singles():
    return {(m, n): synth.make_single(m, n)[:2] for m in (0, 1, 2) for n in (1000, 5000, 20000)}


def test_whole_state_identical_after_every_step(harness, singles):
    steps = fused = 0
    for (model, n), (angles, x) in singles.items():
        for delta in (1e-6, -1e-6):  # forward, central differences
            for multi in (1, 8):
                code, s, f, t, p, info = _pair(harness, model, angles, x, delta=delta, multi=multi)
                print(f"model {model} n {n} delta {delta:+.0e} multi {multi}: {s} steps, {t} behind a trial, {f} fused, "
                      f"stop {info[6]:.0f}")
                assert code == 0, (model, n, delta, multi, code)
                assert info[6] != 0 and np.all(np.isfinite(p))
                steps += s
                fused += f
    # not vacuous: this transition is 60-73 % of the steps of these fits
    print(f"fused {fused} of {steps} steps")
    assert 2 * fused >= steps, (fused, steps)


def test_surfels_with_early_stops_and_large_damping(harness):
    # 256 small Ward fits: some stop on a small gradient or step, some run into itmax, some push nu past 16
    angles, x, _ = synth.make_surfels(2, 256, first=0, count=256)
    stops = {}
    fused = steps = 0
    for s in range(256):
        code, st, f, t, p, info = _pair(harness, 2, angles[s], x[s], itmax=50, multi=8 if s & 1 else 1)
        assert code == 0, (s, code)
        stops[int(info[6])] = stops.get(int(info[6]), 0) + 1
        fused += f
        steps += st
    print(f"stop reasons {stops}; fused {fused} of {steps} steps")
    assert fused > 0


@pytest.mark.parametrize("itmax", [1, 2, 3])
def test_iteration_caps(harness, singles, itmax):
    angles, x = singles[(2, 1000)]
    for multi in (1, 8):
        code, s, f, t, p, info = _pair(harness, 2, angles, x, itmax=itmax, multi=multi)
        assert code == 0, (itmax, multi, code)
        assert info[5] <= itmax
