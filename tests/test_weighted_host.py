"""Per-sample weights (n <= 16) and the per-face capture over per-light means: what can be checked without a GPU -- the ABI, the
argument checks that come before any HIP call, and the identity the means capture rests on, between capture_light_means and
group_capture_samples on the fixture capture of tests/test_gpu_capture_faces.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import oracle_libs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brdf_hip_fit_batch_weighted_dev", "brdf_hip_fit_batch_weighted", "brdf_hip_fit_stats_batch_weighted_dev",
       "brdf_hip_fit_stats_batch_weighted", "brdf_hip_fit_capture_means_dev")
D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
ADDR = C.c_void_p(64)  # not memory: a check that came late would crash


def test_the_new_entry_points_exist():
    import brdf_amd
    from brdf_amd._lib import ABI
    lib = C.CDLL(brdf_amd.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in ABI and re.search(r"\b" + name + r"\s*\(", header), name
    for name in ("fit_batch_weighted", "fit_stats_batch_weighted", "fit_capture_means", "capture_light_means"):
        assert callable(getattr(brdf_amd, name)), name
    assert "n <= 16" in header and "Not covered: weights above 16 samples per fit" in header  # the header states the limit


def test_refusals_come_before_any_hip_call(capfd):
    """n = 17, methods 0 and 3, NULL weights, lb > ub (and what batch_fit_check refuses) return -1 with the entry's name in
    last_error(); the pointers are never dereferenced and no HIP call is made, so this runs on a machine without a GPU."""
    import brdf_amd
    from brdf_amd._lib import lib
    lb, ub_bad, ub = np.zeros(3), np.array([1.0, -1.0, 1.0]), np.ones(3)
    ok = dict(method=1, model=1, a=ADDR, x=ADDR, w=ADDR, counts=None, S=4, n=16, p=ADDR, lb=lb, ub=ub)
    bad = [dict(n=17), dict(n=64), dict(method=0), dict(method=3), dict(method=7), dict(w=None), dict(ub=ub_bad), dict(a=None), dict(x=None),
           dict(p=None), dict(S=0), dict(n=0), dict(model=3)]
    for change in bad:
        k = dict(ok, **change)
        rc = lib.brdf_hip_fit_batch_weighted_dev(k["method"], k["model"], k["a"], k["x"], k["w"], k["counts"], k["S"], k["n"], k["p"],
                                                 k["lb"].ctypes.data_as(D), k["ub"].ctypes.data_as(D), 100, None, None, None, None)
        assert rc == -1 and "brdf_hip_fit_batch_weighted_dev()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    for change in [dict(n=17), dict(method=0), dict(method=3), dict(w=None), dict(n=2), dict(p=None)]:
        k = dict(ok, **change)
        rc = lib.brdf_hip_fit_stats_batch_weighted_dev(k["method"], k["model"], k["a"], k["x"], k["w"], None, k["S"], k["n"], k["p"], None, None, None,
                                                       ADDR, ADDR, ADDR, None)
        assert rc == -1 and "brdf_hip_fit_stats_batch_weighted_dev()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    # the host-pointer twins check the same things under their own names
    S, n = 4, 16
    angles, x, w, p = np.zeros(3 * S * n), np.zeros(S * n), np.ones(S * n), np.zeros(3 * S)
    info, ret = np.zeros(10 * S), np.zeros(S, dtype=np.int32)
    host = dict(method=1, n=n, w=w.ctypes.data_as(D), ub=ub)
    for change in [dict(n=17), dict(method=0), dict(method=3), dict(w=None), dict(ub=ub_bad)]:
        k = dict(host, **change)
        rc = lib.brdf_hip_fit_batch_weighted(k["method"], 1, angles.ctypes.data_as(D), x.ctypes.data_as(D), k["w"], None, S, k["n"], p.ctypes.data_as(D),
                                             lb.ctypes.data_as(D), k["ub"].ctypes.data_as(D), 100, None, info.ctypes.data_as(D), ret.ctypes.data_as(I))
        assert rc == -1 and "brdf_hip_fit_batch_weighted()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
        rc = lib.brdf_hip_fit_stats_batch_weighted(k["method"], 1, angles.ctypes.data_as(D), x.ctypes.data_as(D), k["w"], None, S, k["n"],
                                                   p.ctypes.data_as(D), None, None, None, info.ctypes.data_as(D), None, None)
        if "ub" not in change:  # (the statistics have no box)
            assert rc == -1 and "brdf_hip_fit_stats_batch_weighted()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    # the means capture: 16 < L <= 64 is the faces capture's, v_min > v_max, lb > ub
    led, v3 = np.zeros(3 * 64), np.zeros(3)
    cap = dict(L=16, v_min=0, v_max=255, ub=ub, images=ADDR)
    for change in [dict(L=17), dict(L=64), dict(L=0), dict(v_min=200, v_max=100), dict(ub=ub_bad), dict(images=None)]:
        k = dict(cap, **change)
        rc = lib.brdf_hip_fit_capture_means_dev(1, k["images"], k["L"], 4, 4, ADDR, ADDR, ADDR, ADDR, 5, led.ctypes.data_as(D), v3.ctypes.data_as(D), 1,
                                                v3.ctypes.data_as(D), lb.ctypes.data_as(D), k["ub"].ctypes.data_as(D), 100, None, k["v_min"], k["v_max"],
                                                -2.0, ADDR, None, None, None, None, None, None, None, None, None, None, None, None)
        assert rc == -1 and "brdf_hip_fit_capture_means_dev()" in brdf_amd.last_error(), (change, brdf_amd.last_error())
    capfd.readouterr()


@pytest.fixture(scope="module")
def capture():
    from tests.test_gpu_capture_faces import make_faces_capture
    return make_faces_capture()


def test_light_means_are_the_grouped_samples(capture):
    """capture_light_means against group_capture_samples, rule 1, 254, 0.0: for every fit and for p = P0 and two other points,
    sum w (mean - f)^2 + within equals the grouped sum of squares to 1e-12 relative (1.1e-15 measured), and k is the packed count."""
    import brdf_amd
    from tests.test_gpu_capture_faces import MODEL, P0, RULE
    images, pixel_map, ang = capture["images"], capture["pixel_map"], capture["ang"]
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(images, pixel_map, ang, MODEL, **RULE)
    m = brdf_amd.capture_light_means(images, pixel_map, ang, MODEL, **RULE)
    assert np.array_equal(m.fit_face, fit_face) and np.array_equal(m.fit_channel, fit_channel) and np.array_equal(m.face_pixels, face_pixels)
    assert np.array_equal(m.k, np.diff(off)) and len(fit_face) == 111
    worst = 0.0
    for s in range(len(fit_face)):
        k, n = int(off[s + 1] - off[s]), int(m.counts[s])
        assert (n == 0) == (k == 0) and np.all(m.w[s, :n] >= 1) and m.w[s, :n].sum() == k
        assert np.all(np.isnan(m.x[s, n:])) and np.all(np.isnan(m.w[s, n:])) and np.all(np.isnan(m.angles[s, :, n:]))
        if k == 0:
            assert m.within[s] == 0.0
            continue
        a_v, x_v = np.ascontiguousarray(a[3 * off[s]:3 * off[s + 1]].reshape(3, k)), x[off[s]:off[s + 1]]
        a_m = np.ascontiguousarray(m.angles[s, :, :n])
        for p in (P0, (0.3, 0.4, 12.0), (0.7, 0.1, 3.5)):
            e = x_v - L.model_values(MODEL, a_v, p)
            full = float(e @ e)
            em = m.x[s, :n] - L.model_values(MODEL, a_m, p)
            grouped = float((m.w[s, :n] * em * em).sum()) + float(m.within[s])
            worst = max(worst, abs(grouped - full) / full)
    print(f"largest relative difference of the two sums of squares: {worst:.3e}")
    assert worst <= 1e-12
