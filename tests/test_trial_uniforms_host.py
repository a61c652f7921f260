"""PassUniforms::build_trial (brdf_models.h) against PassUniforms::build, on the CPU.

The resident dlevmar_dif kernel forms the uniforms of the trial request its fused step issues from the step's own values
(DifMachine::NextTrial) instead of reading the request back from LDS.  tests/cpp/trial_uniforms_harness.cpp drives whole fits,
fused step first, and keeps two PassUniforms side by side: one built by build() from every request, one by build_trial() behind
every fused step.  They must be memcmp-equal after EVERY step, for the three models.  Compiled here (g++ -O2 -ffp-contract=off)
against oracle/liboracle.so."""
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
    out = tmp_path_factory.mktemp("trial_uniforms") / "libtrial_uniforms_harness.so"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-O2", "-fPIC", "-ffp-contract=off", "-std=c++17", "-shared", "-o", str(out),
                    os.path.join(ROOT, "tests", "cpp", "trial_uniforms_harness.cpp"), "-L" + oracle, "-loracle",
                    "-Wl,-rpath," + oracle, "-lm"], check=True)
    return C.CDLL(str(out))


def _fit(lib, model, angles, x, itmax=synth.ITMAX, delta=1e-6, multi=1):
    a = np.ascontiguousarray(np.asarray(angles, dtype=np.float64).reshape(-1))
    xx = np.ascontiguousarray(x, dtype=np.float64)
    p0 = np.array(synth.P0[model], dtype=np.float64)
    opts = np.array(synth.OPTS, dtype=np.float64)
    opts[4] = delta
    counts = (C.c_longlong * 2)()
    code = lib.tuh_fit_uniforms(model, a.ctypes.data_as(D), xx.ctypes.data_as(D), xx.size, p0.ctypes.data_as(D), itmax,
                                opts.ctypes.data_as(D), multi, counts)
    return code, counts[0], counts[1]


@pytest.mark.parametrize("model", (0, 1, 2))
def test_uniforms_identical_after_every_step_of_whole_fits(harness, model):
    steps = fused = 0
    for n in (1000, 5000, 20000):
        angles, x, _ = synth.make_single(model, n)
        for delta in (1e-6, -1e-6):  # forward, central differences: the trial request never carries `central`
            for multi in (1, 8):
                code, s, f = _fit(harness, model, angles, x, delta=delta, multi=multi)
                print(f"model {model} n {n} delta {delta:+.0e} multi {multi}: {s} steps, {f} fused")
                assert code == 0, (model, n, delta, multi, code)
                steps += s
                fused += f
    assert 2 * fused >= steps, (fused, steps)  # not vacuous: most steps take the fused path


def test_small_fits_with_early_stops(harness):
    angles, x, _ = synth.make_surfels(2, 256, first=0, count=64)
    fused = 0
    for s in range(64):
        code, _, f = _fit(harness, 2, angles[s], x[s], itmax=50, multi=8 if s & 1 else 1)
        assert code == 0, (s, code)
        fused += f
    assert fused > 0
