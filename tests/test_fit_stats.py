"""Per-fit statistics at a fitted point (brdf_hip_fit_stats_batch_dev and friends): what can be checked without a GPU --
the ABI, the argument checks, the kernels' resources, and the claim the feature rests on: for a converged dlevmar_bc_dif
fit, levmar's returned covariance IS sumsq/(n-3) (J^T J)^-1 with J taken at the fitted p."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from brdf_amd import synth
from tests import oracle_libs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brdf_hip_fit_stats_batch_dev", "brdf_hip_fit_stats_batch", "brdf_hip_fit_capture_stats_dev")


def test_the_three_entry_points_exist():
    import brdf_amd
    from brdf_amd._lib import ABI
    lib = C.CDLL(brdf_amd.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in ABI and re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+BRDF_STATS_SZ\s+8\b", header)
    assert callable(brdf_amd.fit_stats_batch) and brdf_amd.FitStats is not None


def test_argument_errors_return_lm_error_before_any_hip_call(capfd):
    """null planes / x / p, S or n out of range (n < 3 included), an unknown model or method, all three outputs NULL: LM_ERROR
    with a text that names the entry point.  The pointers are never dereferenced and no HIP call is made, so this runs
    on a machine without a GPU (and would crash on one if the checks came late: the addresses are not memory)."""
    import brdf_amd
    from brdf_amd._lib import lib
    ok = dict(method=1, model=1, a=C.c_void_p(64), x=C.c_void_p(64), S=4, n=16, p=C.c_void_p(64), covar=C.c_void_p(64),
              stats=C.c_void_p(64), rank=C.c_void_p(64))
    bad = [dict(a=None), dict(x=None), dict(p=None), dict(S=0), dict(S=-3), dict(n=0), dict(n=2), dict(n=-1), dict(n=2**31 - 1), dict(model=3),
           dict(model=-1), dict(method=4), dict(method=-1), dict(covar=None, stats=None, rank=None)]
    for change in bad:
        k = dict(ok, **change)
        rc = lib.brdf_hip_fit_stats_batch_dev(k["method"], k["model"], k["a"], k["x"], k["S"], k["n"], k["p"], None, k["covar"], k["stats"],
                                              k["rank"], None)
        assert rc == -1 and "brdf_hip_fit_stats_batch_dev()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    # the host-pointer entry checks the same things under its own name
    angles, x, p = np.zeros(3 * 4 * 16), np.zeros(4 * 16), np.zeros(12)
    covar, rank = np.zeros(36), np.zeros(4, dtype=np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    host_ok = dict(method=1, model=1, a=angles.ctypes.data_as(D), x=x.ctypes.data_as(D), S=4, n=16, p=p.ctypes.data_as(D),
                   covar=covar.ctypes.data_as(D), stats=None, rank=rank.ctypes.data_as(I))
    for change in [dict(a=None), dict(x=None), dict(p=None), dict(S=0), dict(n=2), dict(model=7), dict(method=9), dict(covar=None, rank=None)]:
        k = dict(host_ok, **change)
        rc = lib.brdf_hip_fit_stats_batch(k["method"], k["model"], k["a"], k["x"], k["S"], k["n"], k["p"], None, k["covar"], k["stats"], k["rank"])
        assert rc == -1 and "brdf_hip_fit_stats_batch()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    # the capture variant: fewer than three images cannot give a covariance -- refused before the capture runs, under its own name
    led, v3 = np.zeros(6), np.zeros(3)
    rc = lib.brdf_hip_fit_capture_stats_dev(1, C.c_void_p(64), 2, 4, 4, C.c_void_p(64), C.c_void_p(64), C.c_void_p(64), C.c_void_p(64), 5,
                                            led.ctypes.data_as(D), v3.ctypes.data_as(D), 1, v3.ctypes.data_as(D), None, None, 100, None,
                                            C.c_void_p(64), None, None, None, C.c_void_p(64), None, None)
    assert rc == -1 and "brdf_hip_fit_capture_stats_dev()" in brdf_amd.last_error(), brdf_amd.last_error()
    capfd.readouterr()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_fit_stats_kernels_use_no_scratch(tmp_path):
    """fit_stats.hip cross-compiled for gfx950: every kernel in it reports 0 spilled VGPRs and 0 bytes of scratch"""
    src = os.path.join(ROOT, "brdf_amd", "csrc", "fit_stats.hip")
    cmd = ["hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
           "--cuda-device-only", "-c", src, "-o", str(tmp_path / "fit_stats.o")]
    pr = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(src), timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", pr.stderr)
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", pr.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", pr.stderr)]
    assert len(names) == len(spills) == len(scratch)
    kernels = {n: (sp, sc) for n, sp, sc in zip(names, spills, scratch) if "fit_stats_" in n}
    # rows / wave / block / partial: 3 models x 3 Jacobian kinds each, and the prepared-sample A/B variants of the two pow models;
    # the spread and fold kernels
    for stem, count in (("fit_stats_rows_kernel", 15), ("fit_stats_wave_kernel", 15), ("fit_stats_block_kernel", 15),
                        ("fit_stats_partial_kernel", 15), ("fit_stats_spread_kernel", 1), ("fit_stats_fold_kernel", 1)):
        assert sum(stem in n for n in kernels) == count, (stem, sorted(kernels))
    assert all(v == (0, 0) for v in kernels.values()), {n: v for n, v in kernels.items() if v != (0, 0)}


@pytest.mark.parametrize("n,count", [(256, 256), (4096, 64)])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_levmars_returned_covariance_is_the_one_at_the_fitted_point(model, n, count):
    """Reference only (passes without the feature; it guards the definition the feature uses).  Side A: the covariance
    orc_dlevmar_bc_dif returns.  Side B: at the returned p, orc_brdf_func, orc_fdif_forward, J^T J, orc_covar.  All nine entries
    agree to 1e-8 relative (measured: at most 1.4e-9 at n = 256, 4.0e-10 at n = 4096)."""
    from tests.stats_yardstick import _Extra
    angles, x, _ = synth.make_surfels(model, n, 0, count)
    lb, ub = (np.array(v, dtype=np.float64) for v in synth.bounds(model))
    opts = np.array(synth.OPTS)
    cb = C.cast(L.orc.orc_brdf_func, C.c_void_p)
    worst = 0.0
    for s in range(count):
        a, xs = np.ascontiguousarray(angles[s].reshape(-1)), np.ascontiguousarray(x[s])
        ed = _Extra(L.ptr(a), model)
        p, info, cov_a = np.array(synth.P0[model]), np.zeros(10), np.zeros(9)
        r = L.orc.orc_dlevmar_bc_dif(cb, L.ptr(p), L.ptr(xs), 3, n, L.ptr(lb), L.ptr(ub), None, synth.ITMAX, L.ptr(opts), L.ptr(info), None,
                                     L.ptr(cov_a), C.byref(ed))
        assert r >= 0, (model, s)
        hx, hxx, jac = np.zeros(n), np.zeros(n), np.zeros((n, 3))
        L.orc.orc_brdf_func(L.ptr(p), L.ptr(hx), 3, n, C.byref(ed))
        L.orc.orc_fdif_forward(cb, L.ptr(p), L.ptr(hx), L.ptr(hxx), C.c_double(opts[4]), L.ptr(jac), 3, n, C.byref(ed))
        e = xs - hx
        jtj, cov_b = np.ascontiguousarray(jac.T @ jac), np.zeros(9)
        assert L.orc.orc_covar(L.ptr(jtj), L.ptr(cov_b), C.c_double(float(e @ e)), 3, n) == 3
        worst = max(worst, float(np.max(np.abs(cov_a - cov_b) / np.abs(cov_b))))
    print(f"model {model} n {n}: levmar's returned covar vs recomputed at p, max relative difference {worst:.2e}")
    assert worst <= 1e-8
