"""The host side of one single fit (stream_fit_run -> resident_fit_try): launch timing and the environment switches.

Launch timing (brdf_hip_set_launch_timing) may change no result by a bit, and kernel_us is the kernel's duration: positive and no
longer than an event pair around the whole call.  The switches are read from the environment on every call: one set between two
fits of one process takes effect on the next one.  Sizes: 17,409 samples (18 workgroups in two groups: the exchange runs) and
4,096 (one workgroup: no exchange); Ward and Blinn-Phong, dlevmar_dif and dlevmar_bc_dif.  (Bit-identity of the fits themselves
against recorded bytes: tests/test_gpu_resident_plumbing.py.)"""
import os

import numpy as np
import pytest

SIZES = (17409, 4096)
MODELS = (2, 1)  # Ward, Blinn-Phong
SWITCHES = ("BRDF_HIP_DIF_FUSED", "BRDF_HIP_RESIDENT")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import brdf_amd
    from brdf_amd import synth

    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    dev = torch.device("cuda:0")
    data = {}
    for model in MODELS:
        for n in SIZES:
            angles, x, _ = synth.make_single(model, n)
            data[(model, n)] = (torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev))

    def fit(model, method, n):
        a, x = data[(model, n)]
        res = brdf_amd.fit_single(method, model, a, x, synth.P0[model], lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS,
                                  want_covar=True)
        return res, brdf_amd.last_fit_stats()

    yield {"torch": torch, "brdf_amd": brdf_amd, "fit": fit}
    brdf_amd.set_launch_timing(False)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def timed(gpu):
    """every case once with launch timing off and once with it on, the second inside an event pair of the test's own"""
    torch, brdf_amd, fit = gpu["torch"], gpu["brdf_amd"], gpu["fit"]
    out = {}
    for model in MODELS:
        for method in (brdf_amd.METHOD_DIF, brdf_amd.METHOD_BC_DIF):
            for n in SIZES:
                brdf_amd.set_launch_timing(False)
                off, st_off = fit(model, method, n)
                brdf_amd.set_launch_timing(True)
                fit(model, method, n)  # (the event pair is created on first use: not inside the bracket below)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                on, st_on = fit(model, method, n)
                e1.record()
                e1.synchronize()
                out[(model, method, n)] = (off, st_off, on, st_on, 1e3 * e0.elapsed_time(e1))
    brdf_amd.set_launch_timing(False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", (0, 1), ids=("dif", "bc_dif"))
@pytest.mark.parametrize("model", MODELS)
def test_results_identical_with_launch_timing_on_and_off(timed, gpu, model, method, n):
    m = (gpu["brdf_amd"].METHOD_DIF, gpu["brdf_amd"].METHOD_BC_DIF)[method]
    off, st_off, on, st_on, around_us = timed[(model, m, n)]
    assert off.ret >= 0 and st_off["launches"] == 1 and st_on["launches"] == 1  # the resident kernel ran
    assert on.ret == off.ret
    for a, b in ((on.p, off.p), (on.info, off.info), (on.covar, off.covar)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    assert st_on["passes"] == st_off["passes"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", (0, 1), ids=("dif", "bc_dif"))
@pytest.mark.parametrize("model", MODELS)
def test_kernel_us_is_the_kernels_duration(timed, gpu, model, method, n):
    m = (gpu["brdf_amd"].METHOD_DIF, gpu["brdf_amd"].METHOD_BC_DIF)[method]
    off, st_off, on, st_on, around_us = timed[(model, m, n)]
    print(f"model {model} method {method} n {n}: kernel_us {st_on['kernel_us']:.1f}, device clock {st_on['device_us']:.1f}, "
          f"events around the call {around_us:.1f}")
    assert st_off["kernel_us"] == -1.0  # timing off: nothing measured
    assert 0.0 < st_on["kernel_us"] <= around_us


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_switches_set_between_two_fits_take_effect_on_the_next(gpu, n):
    brdf_amd, fit = gpu["brdf_amd"], gpu["fit"]
    model, method = 2, brdf_amd.METHOD_DIF
    for k in SWITCHES:
        os.environ.pop(k, None)
    first, st = fit(model, method, n)
    assert st["launches"] == 1 and st["fused_steps"] > 0
    try:
        os.environ["BRDF_HIP_DIF_FUSED"] = "0"
        unfused, st = fit(model, method, n)
        assert st["launches"] == 1 and st["fused_steps"] == 0
        assert unfused.ret == first.ret and unfused.p.tobytes() == first.p.tobytes() and unfused.info.tobytes() == first.info.tobytes()
        del os.environ["BRDF_HIP_DIF_FUSED"]
        again, st = fit(model, method, n)
        assert st["launches"] == 1 and st["fused_steps"] > 0
        assert again.p.tobytes() == first.p.tobytes()
        os.environ["BRDF_HIP_RESIDENT"] = "0"
        chain, st = fit(model, method, n)
        assert chain.ret >= 0 and st["launches"] > 1 and st["fused_steps"] == 0
        del os.environ["BRDF_HIP_RESIDENT"]
        back, st = fit(model, method, n)
        assert st["launches"] == 1 and st["fused_steps"] > 0
        assert back.p.tobytes() == first.p.tobytes()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
