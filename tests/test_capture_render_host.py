"""Rendering a fitted capture -- brdf_hip_capture_render_dev, brdf_hip_capture_render_residuals_dev, brdf_hip_surfaces_from_materials_dev --
the part that needs no device: the header's declarations; every entry's refusals, each before any HIP call and under the entry's own
name; the NumPy twins brdf_amd.render_capture_host and brdf_amd.render_residuals_host -- the definitions as code -- on a hand-made
3 x 4 map: the row flip, each background mode, each branch of the quantisation, the lowest-light tie of worst_light, the rule off and
on; and the edge values of psnr()."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER, RESIDUALS, SURFACES = ("brdf_hip_capture_render_dev", "brdf_hip_capture_render_residuals_dev", "brdf_hip_surfaces_from_materials_dev")
INT_MAX = 2 ** 31 - 1


def test_header_declares_the_three_entries():
    import brdf_amd
    from brdf_amd._lib import ABI
    text = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in (RENDER, RESIDUALS, SURFACES):
        assert f"int {name}(" in text, name
        assert name in ABI and hasattr(brdf_amd.lib, name)
    for word in ("capture_render", "capture_render_residuals", "surfaces_from_materials", "render_capture_host", "render_residuals_host"):
        assert callable(getattr(brdf_amd, word)), word


def _callers():
    """per entry: a function of keyword overrides that calls it with pointers that are never read"""
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)
    ptr, dbl = C.c_void_p(buf.ctypes.data), buf.ctypes.data_as(D)
    base = dict(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, vertices=ptr, faces=ptr, normals=ptr, nf=10, leds=dbl, view=dbl, rv=1, surfaces=ptr,
                background=0, values=ptr, rendered=ptr, v_min=0, v_max=255, cos_min=-2.0, labels=ptr, materials=ptr, K=2, fill=dbl)

    def render(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_capture_render_dev(k["model"], k["H_"], k["W_"], k["pm"], k["vertices"], k["faces"], k["normals"], k["nf"], k["leds"], k["L"],
                                               k["view"], k["rv"], k["surfaces"], k["background"], k["values"], k["rendered"], None)

    def residuals(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_capture_render_residuals_dev(k["model"], k["images"], k["L"], k["H_"], k["W_"], k["pm"], k["vertices"], k["faces"], k["normals"],
                                                         k["nf"], k["leds"], k["view"], k["rv"], k["surfaces"], k["v_min"], k["v_max"], k["cos_min"], ptr, ptr,
                                                         ptr, ptr, ptr, ptr, ptr, ptr, k["values"], None, None)

    def surfaces(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_surfaces_from_materials_dev(k["labels"], k["nf"], k["materials"], k["K"], k["fill"], k["surfaces"], None)
    return {RENDER: render, RESIDUALS: residuals, SURFACES: surfaces}, buf


def test_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    callers, buf = _callers()
    capture = [dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None), dict(surfaces=None),  # null pointers
               dict(L=0), dict(L=65), dict(H_=0), dict(W_=-2), dict(nf=0), dict(nf=INT_MAX // 3 + 1), dict(model=3), dict(model=-1), dict(rv=2)]
    cases = {RENDER: capture + [dict(values=None, rendered=None), dict(background=-2), dict(background=256)],
             RESIDUALS: capture + [dict(images=None), dict(v_min=200, v_max=100), dict(cos_min=float("nan"))],
             SURFACES: [dict(labels=None), dict(materials=None), dict(fill=None), dict(surfaces=None), dict(nf=0), dict(nf=INT_MAX // 3 + 1), dict(K=0),
                        dict(K=-3)]}
    for name, call in callers.items():
        for kw in cases[name]:
            assert call(**kw) == -1, (name, kw)
            assert name + "()" in brdf_amd.last_error(), (name, kw, brdf_amd.last_error())
    assert callers[RENDER](L=65) == -1 and "1 <= Lr <= 64" in brdf_amd.last_error()
    assert callers[RENDER](values=None, rendered=None) == -1 and "both null" in brdf_amd.last_error()
    assert callers[RENDER](background=256) == -1 and "background = 256" in brdf_amd.last_error()
    assert callers[RESIDUALS](L=65) == -1 and "<= 64" in brdf_amd.last_error()
    assert callers[RESIDUALS](surfaces=None) == -1 and "brdf_surfaces" in brdf_amd.last_error()
    assert callers[SURFACES](K=0) == -1 and "K = 0" in brdf_amd.last_error()
    assert not buf.any()  # a refused call writes nothing
    capfd.readouterr()


# ---- the twins on a hand-made map ---------------------------------------------------------------------------------------------------
NF, LR = 3, 2
MAP = np.array([[0, 1, -1, 2],
                [2, 3, 0, -5],      # 3 = nf and -5: background
                [1, 1, 2, 0]], dtype=np.int32)


def _values():
    """[3,3,2]: face 0 plain values, face 1 every branch of the quantisation, face 2 the rounding boundary from both sides"""
    v = np.zeros((NF, 3, LR))
    v[0] = [[0.0, 0.25], [0.5, 1.0], [100.0 / 255.0, 200.0 / 255.0]]
    v[1] = [[np.nan, -0.3], [1.7, np.inf], [-np.inf, 255.4 / 255.0]]
    v[2] = [[np.nextafter(0.5 / 255.0, 0.0), np.nextafter(0.5 / 255.0, 1.0)], [-0.5 / 255.0, np.nextafter(-0.5 / 255.0, -1.0)], [255.5 / 255.0, 0.999]]
    return v


def test_quantisation_branches():
    from brdf_amd.fit import _grey_levels
    q = _grey_levels(_values())
    assert q.dtype == np.uint8
    assert q[0].tolist() == [[0, 64], [128, 255], [100, 200]]          # 255 * 0.25 + 0.5 = 64.25, 255 * 0.5 + 0.5 = 128.0
    assert q[1].tolist() == [[0, 0], [255, 255], [0, 255]]             # NaN, t < 0, t >= 256, +inf, -inf, t = 255.9
    t = 255.0 * _values()[2] + 0.5
    assert q[2].tolist() == [[int(t[0, 0]), int(t[0, 1])], [0, 0], [255, 255]]
    assert q[2, 0, 1] == 1 and t[1, 0] == 0.0 and t[1, 1] < 0.0 and t[2, 0] >= 256.0  # t = 0 is inside; just below it is not


def test_render_twin_flips_rows_and_knows_each_background():
    import brdf_amd
    from brdf_amd.fit import _grey_levels
    values, q = _values(), _grey_levels(_values())
    H, W = MAP.shape
    carried = (MAP >= 0) & (MAP < NF)
    for background in (0, 200):
        img = brdf_amd.render_capture_host(values, MAP, background)
        assert img.shape == (LR, H, W, 3) and img.dtype == np.uint8
        for y in range(H):
            for x in range(W):
                want = q[MAP[y, x]].T if carried[y, x] else np.full((LR, 3), background)
                assert np.array_equal(img[:, H - 1 - y, x, :], want), (background, y, x)
    held = np.full((LR, H, W, 3), 77, dtype=np.uint8)
    img = brdf_amd.render_capture_host(values, MAP, -1, out=held)
    assert img is held and np.all(img[:, ~carried[::-1], :] == 77)
    assert np.array_equal(img[:, carried[::-1], :], brdf_amd.render_capture_host(values, MAP, 0)[:, carried[::-1], :])
    assert not brdf_amd.render_capture_host(values, MAP, -1)[:, ~carried[::-1], :].any()  # without `out`: zeros
    with pytest.raises(ValueError):
        brdf_amd.render_capture_host(values, MAP, 256)
    with pytest.raises(ValueError):
        brdf_amd.render_capture_host(values[:, :2], MAP, 0)


def _residual_problem():
    """MAP under LR = 3 lights, model Blinn-Phong (planes 0 and 1): grey levels 10 * (face + 1) + channel + light"""
    L = 3
    q = np.array([[[10 * (f + 1) + c + l for l in range(L)] for c in range(3)] for f in range(NF)], dtype=np.int64)
    values = (q + 0.0) / 255.0
    assert np.array_equal(__import__("brdf_amd").fit._grey_levels(values), q)
    H, W = MAP.shape
    images = np.zeros((L, H, W, 3), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            f = MAP[y, x]
            images[:, H - 1 - y, x, :] = (q[f].T if 0 <= f < NF else 99)
    ang = np.full((NF, 3, L), 0.5)
    return L, q, values, images, ang


def test_residual_twin_rule_off_ties_and_signs():
    import brdf_amd
    L, q, values, images, ang = _residual_problem()
    H, W = MAP.shape
    images[:, H - 1 - 0, 0, 0] = q[0, 0] + [4, -4, 4]      # pixel (0, 0), face 0, channel 0: |d| = 4 at every light -> the lowest
    images[:, H - 1 - 2, 1, 2] = q[1, 2] + [0, -7, 7]      # pixel (2, 1), face 1, channel 2: the tie is between lights 1 and 2 -> 1
    images[2, H - 1 - 1, 2, 1] = q[0, 1, 2] - 9            # pixel (1, 2), face 0, channel 1: light 2 alone
    r = brdf_amd.render_residuals_host(images, MAP, ang, 1, values)
    carried = (MAP >= 0) & (MAP < NF)
    assert r.light_count.dtype == np.int64 and r.face_light_count.dtype == np.int32 and r.abs_max.dtype == np.uint8
    assert np.all(r.light_count == carried.sum()) and r.light_count.shape == (L, 3)
    assert r.light_sum.tolist() == [[4, 0, 0], [-4, 0, -7], [4, -9, 7]]
    assert r.light_sumsq.tolist() == [[16, 0, 0], [16, 0, 49], [16, 81, 49]]
    assert r.face_light_count[:, 0, 0].tolist() == [3, 3, 3] and r.face_light_count.shape == (NF, 3, L)
    assert r.face_light_sum[0, 0].tolist() == [4, -4, 4] and r.face_light_sum[1, 2].tolist() == [0, -7, 7] and r.face_light_sumsq[0, 1].tolist() == [0, 0, 81]
    assert np.array_equal(r.face_light_sum.sum(axis=0).T, r.light_sum) and np.array_equal(r.face_light_sumsq.sum(axis=0).T, r.light_sumsq)
    want_max, want_worst = np.zeros((H, W, 3), dtype=np.uint8), np.full((H, W, 3), 255, dtype=np.uint8)
    want_worst[carried] = 0                                  # every light compared, all d = 0: the lowest light
    want_max[0, 0, 0], want_max[2, 1, 2], want_max[1, 2, 1] = 4, 7, 9
    want_worst[2, 1, 2], want_worst[1, 2, 1] = 1, 2
    assert np.array_equal(r.abs_max, want_max) and np.array_equal(r.worst_light, want_worst)


def test_residual_twin_under_the_rule():
    import brdf_amd
    L, q, values, images, ang = _residual_problem()
    H, W = MAP.shape
    ang[0, 1, 1] = -0.1       # face 0, light 1: plane 1 fails (Blinn-Phong reads it); plane 2 is not read
    ang[1, 2, :] = -1.0       # (not read by Blinn-Phong: no effect; Phong reads it)
    ang[2, 0, 2] = np.nan     # face 2, light 2: a NaN cosine is never a sample
    images[0, H - 1 - 2, 3, 1] = 255    # pixel (2, 3), face 0, channel 1, light 0: above v_max
    images[2, H - 1 - 0, 1, 0] = 0      # pixel (0, 1), face 1, channel 0, light 2: below v_min
    images[1, H - 1 - 2, 3, 1] = q[0, 1, 1] + 50  # light 1 of face 0: not compared, whatever it shows
    r = brdf_amd.render_residuals_host(images, MAP, ang, 1, values, v_min=1, v_max=254, cos_min=0.0)
    faces = [int((MAP == f).sum()) for f in range(NF)]  # 3 pixels each
    assert faces == [3, 3, 3]
    want = np.zeros((NF, 3, L), dtype=np.int32)
    want[:] = 3
    want[0, :, 1] = 0
    want[2, :, 2] = 0
    want[0, 1, 0] -= 1
    want[1, 0, 2] -= 1
    assert np.array_equal(r.face_light_count, want) and np.array_equal(r.light_count, want.sum(axis=0).T)
    assert not r.light_sum.any() and not r.light_sumsq.any() and not r.abs_max.any()
    assert r.worst_light[2, 3, 1] == 2 and r.worst_light[2, 3, 0] == 0 and r.worst_light[0, 1, 0] == 0  # the lowest COMPARED light
    phong = brdf_amd.render_residuals_host(images, MAP, ang, 0, values, v_min=1, v_max=254, cos_min=0.0)
    assert not phong.face_light_count[1].any() and np.all(phong.face_light_count[0, 0] == 3)  # plane 2 read, plane 1 not
    one = images.copy()
    one[:, H - 1 - 0, 1, :] = 0  # pixel (0, 1): nothing compared in any channel
    r = brdf_amd.render_residuals_host(one, MAP, ang, 1, values, v_min=1, v_max=254, cos_min=0.0)
    assert r.abs_max[0, 1].tolist() == [0, 0, 0] and r.worst_light[0, 1].tolist() == [255, 255, 255]
    assert np.all(r.worst_light[~((MAP >= 0) & (MAP < NF))] == 255)


def test_psnr_edges():
    import brdf_amd
    from brdf_amd.fit import _psnr

    class Host(np.ndarray):
        def cpu(self):
            return self

        def numpy(self):
            return np.asarray(self)
    count = np.array([[10, 10, 0], [4, 0, 0]], dtype=np.int64).view(Host)
    sumsq = np.array([[10, 0, 0], [4 * 65025, 0, 0]], dtype=np.int64).view(Host)
    res = brdf_amd.CaptureRenderResiduals(count, None, sumsq, None, None, None, None, None, None, 0)
    per, overall = res.psnr()
    assert per.shape == (2, 3)
    assert per[0, 0] == pytest.approx(10.0 * math.log10(65025.0)) and per[0, 1] == np.inf and np.isnan(per[0, 2])
    assert per[1, 0] == pytest.approx(0.0, abs=1e-12) and np.isnan(per[1, 1])
    assert overall == pytest.approx(10.0 * math.log10(65025.0 * 24 / (10 + 4 * 65025)))
    assert _psnr(0, 0) != _psnr(0, 0) and _psnr(5, 0) == np.inf  # count = 0 wins over sumsq = 0
