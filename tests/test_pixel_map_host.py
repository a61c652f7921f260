"""Mesh + camera -> pixel map and face normals (brdf_amd/raster.py, brdf_amd/csrc/pixel_map.hip), the part that needs no device: the
header's declarations; every refusal of the two entries, each before any HIP call and under the entry's own name; the NumPy twins
face_normals_host and pixel_map_host on hand-written expectations (identity matrices, an 8 x 8 viewport, dyadic coordinates: every
operation is exact); the GL matrices against hand-computed ones; the reference's MakeFrustum; the committed .cal files; and the
calibrated pinhole of tsai_camera against the direct formula."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import pixel_map_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMALS, MAP = "brdf_hip_face_normals_dev", "brdf_hip_pixel_map_dev"
INT_MAX = 2 ** 31 - 1


def test_header_declares_the_two_entries_and_the_package_exports_the_module():
    import brdf_amd
    from brdf_amd._lib import ABI
    text = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in (NORMALS, MAP):
        assert f"int {name}(" in text and name in ABI and hasattr(brdf_amd.lib, name)
    for word in ("face_normals", "face_normals_host", "pixel_map", "pixel_map_host", "gl_frustum", "gl_look_at", "make_frustum", "parse_cal",
                 "tsai_camera"):
        assert callable(getattr(brdf_amd, word)) and getattr(brdf_amd, word) is getattr(brdf_amd.raster, word)


def test_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read as device memory: every call below is refused before any HIP call
    ptr = C.c_void_p(buf.ctypes.data)
    eye, vp, stats = np.eye(4).reshape(-1), np.array([0.0, 0.0, 8.0, 8.0]), np.full(8, -7, dtype=np.int64)
    base = dict(vertices=ptr, nv=12, faces=ptr, nf=4, mv=eye, pr=eye, vp=vp, H_=8, W_=8, mode=1, cull=0, pm=ptr, depth=ptr, fp=ptr)

    def call_map(**kw):
        k = {**base, **kw}
        host = [None if k[n] is None else np.ascontiguousarray(k[n], dtype=np.float64) for n in ("mv", "pr", "vp")]
        return lib.brdf_hip_pixel_map_dev(k["vertices"], k["nv"], k["faces"], k["nf"], *[None if h is None else h.ctypes.data_as(D) for h in host],
                                          k["H_"], k["W_"], k["mode"], k["cull"], k["pm"], k["depth"], k["fp"],
                                          stats.ctypes.data_as(C.POINTER(C.c_longlong)), None)

    def with_entry(a, i, v):
        a = np.array(a, dtype=np.float64)
        a[i] = v
        return a
    refused = [dict(H_=0), dict(W_=0), dict(H_=-3), dict(H_=65536, W_=32768), dict(nf=INT_MAX + 1), dict(nf=0), dict(nv=0), dict(nv=INT_MAX + 1),
               dict(mode=2), dict(mode=-1), dict(cull=2), dict(cull=-1),
               dict(vertices=None), dict(faces=None), dict(mv=None), dict(pr=None), dict(vp=None), dict(pm=None),
               dict(mv=with_entry(eye, 5, np.nan)), dict(mv=with_entry(eye, 12, np.inf)), dict(pr=with_entry(eye, 0, -np.inf)),
               dict(pr=with_entry(eye, 15, np.nan)), dict(vp=with_entry(vp, 0, np.nan)), dict(vp=with_entry(vp, 1, np.inf)),
               dict(vp=with_entry(vp, 2, 0.0)), dict(vp=with_entry(vp, 3, -8.0)), dict(vp=with_entry(vp, 2, np.inf))]
    for kw in refused:
        assert call_map(**kw) == -1, kw
        assert MAP + "()" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert call_map(H_=65536, W_=32768) == -1 and "H W <= INT_MAX" in brdf_amd.last_error()
    assert call_map(mode=2) == -1 and "mode = 2" in brdf_amd.last_error()
    assert call_map(vp=with_entry(vp, 3, -8.0)) == -1 and "viewport[3] = -8" in brdf_amd.last_error()
    for args in ((None, 12, ptr, 4, ptr), (ptr, 12, None, 4, ptr), (ptr, 12, ptr, 4, None), (ptr, 0, ptr, 4, ptr), (ptr, 12, ptr, 0, ptr),
                 (ptr, 12, ptr, INT_MAX + 1, ptr), (ptr, INT_MAX + 1, ptr, 4, ptr)):
        assert lib.brdf_hip_face_normals_dev(*args, None) == -1, args
        assert NORMALS + "()" in brdf_amd.last_error()
    assert not buf.any() and np.all(stats == -7)  # a refused call writes nothing
    capfd.readouterr()


def test_twin_refuses_what_the_entry_refuses():
    import brdf_amd
    v, f = P.window_mesh([P.tri(1, 1, 7, 1, 1, 7)])
    for kw in (dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(mode=2), dict(cull=-1), dict(viewport=(0, 0, 0, 8)), dict(viewport=(0, 0, 8, np.nan)),
               dict(model_view=np.full(16, np.inf))):
        args = dict(model_view=P.IDENTITY, projection=P.IDENTITY, viewport=P.VIEWPORT, H=P.N, W=P.N)
        args.update(kw)
        with pytest.raises(ValueError):
            brdf_amd.pixel_map_host(v, f, **args)


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def test_face_normals_twin():
    import brdf_amd
    v = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0], [6.0, 0.0, 0.0], [1e-200, 0.0, 0.0], [0.0, 1e-200, 0.0]])
    f = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [0, 4, 5], [0, 1, 6]])
    n = brdf_amd.face_normals_host(v, f)
    assert n[0].tolist() == [0.0, 0.0, 1.0] and n[1].tolist() == [0.0, 0.0, -1.0]  # the right triangle, both windings
    assert n[2].tolist() == [0.0, 0.0, 0.0]              # collinear: squared norm 0, stays unnormalised
    assert n[3].tolist() == [0.0, 0.0, 0.0]              # 1e-400 underflows: squared norm 0, stays as it is
    assert np.all(np.isnan(n[4]))                        # a vertex index outside [0, nv)
    rng = np.random.default_rng(3)
    v, f = rng.normal(size=(50, 3)) * 100.0, rng.integers(0, 50, size=(400, 3))
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    got = brdf_amd.face_normals_host(v, f)
    want = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))  # 1 ulp


# ---- the map, by hand -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.hand_cases()))
def test_pixel_map_twin_on_hand_written_maps(name):
    import brdf_amd
    tris, kw, rule = P.hand_cases()[name]
    v, f = P.window_mesh(tris)
    r = brdf_amd.pixel_map_host(v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, **kw)
    want = P.expected_map(rule)
    assert r.pixel_map.dtype == np.int32 and np.array_equal(r.pixel_map, want), (name, r.pixel_map[::-1])
    assert np.array_equal(r.face_pixels, np.bincount(want[want >= 0], minlength=len(tris)))
    assert r.stats[6] == (want >= 0).sum() and r.stats[7] == 0
    assert np.all(r.depth[want < 0] == 2.0)


def test_pixel_map_twin_details():
    import brdf_amd
    cases = P.hand_cases()
    run = lambda name: brdf_amd.pixel_map_host(*P.window_mesh(cases[name][0]), P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, **cases[name][1])
    one = run("one_triangle")
    assert one.stats.tolist() == [1, 0, 0, 0, 0, 36, 21, 0]  # the box: columns and rows 1 ... 6
    assert np.all(one.depth[one.pixel_map == 0] == 0.5)
    quad = run("quad")
    assert quad.stats[5] == 72 and quad.stats[6] == 36 and quad.face_pixels.tolist() == [21, 15]  # the diagonal's six go to face 0
    assert not (quad.pixel_map[1:7, 1:7] < 0).any()
    near = run("nearer_over_farther")
    assert np.all(near.depth[near.pixel_map == 1] == 0.25) and near.face_pixels.tolist() == [0, 21]
    assert run("identical").face_pixels.tolist() == [21, 0]
    assert run("clockwise_culled").stats.tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert run("clockwise_kept").stats.tolist() == [1, 0, 0, 0, 0, 36, 21, 0]
    # a face between the centres is rasterised and holds no candidate; a zero-area face is degenerate
    v, f = P.window_mesh([P.tri(2.6, 2.6, 2.9, 2.6, 2.6, 2.9), P.tri(1, 1, 3, 3, 5, 5)])
    assert brdf_amd.pixel_map_host(v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N).stats.tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    # depth is interpolated: z = x / 8 on this face
    v, f = P.window_mesh([[(0, 0, 0.0), (8, 0, 1.0), (0, 8, 0.0)]])
    r = brdf_amd.pixel_map_host(v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N)
    assert np.array_equal(r.depth[0], (np.arange(8) + 0.5) / 8)


def test_pixel_map_twin_trouble():
    import brdf_amd
    v, f = P.trouble_mesh()
    r = brdf_amd.pixel_map_host(v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N)
    assert r.stats[:5].tolist() == [3, 2, 0, 0, 1]  # faces 0, 2, 5 rasterised; 3 (NaN) and 4 (index) unprojectable; 1 outside
    assert r.face_pixels[[1, 2, 3, 4]].tolist() == [0, 0, 0, 0] and r.face_pixels[0] > 0 and r.face_pixels[5] > 0
    assert r.pixel_map[3, 0] == 0 and r.depth[3, 0] == 0.25 and r.pixel_map[1, 1] == 5  # face 0 in front of face 5; beyond z = 1: nothing


def test_reference_map_twin():
    import brdf_amd
    tris, want, depth, stats = P.centroid_case()
    v, f = P.window_mesh(tris)
    r = brdf_amd.pixel_map_host(v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, mode=0)
    assert np.array_equal(r.pixel_map, want) and np.array_equal(r.depth, depth) and r.stats.tolist() == stats.tolist()
    assert r.face_pixels.tolist() == [0, 0, 1, 0, 0, 1, 0]


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------
def test_gl_matrices_by_hand():
    import brdf_amd
    assert brdf_amd.gl_frustum(-1, 1, -1, 1, 1, 3).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -2, -1, 0, 0, -3, 0]
    assert brdf_amd.gl_frustum(-1, 3, -2, 2, 2, 6).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0.5, 0, -2, -1, 0, 0, -6, 0]
    assert brdf_amd.gl_look_at((0, 0, 5), (0, 0, 0), (0, 1, 0)).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -5, 1]
    # from +x towards the origin, z up: s = (0, 1, 0), u = (0, 0, 1), -f = (1, 0, 0)
    assert brdf_amd.gl_look_at((3, 0, 0), (0, 0, 0), (0, 0, 1)).tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -3, 1]
    # the up vector need not be normal to the view: eye (0, 0, 5), up (0, 1, 1) gives the same frame as up (0, 1, 0)
    assert np.array_equal(brdf_amd.gl_look_at((0, 0, 5), (0, 0, 0), (0, 2, 2)), brdf_amd.gl_look_at((0, 0, 5), (0, 0, 0), (0, 1, 0)))


def test_make_frustum_is_the_references_formula():
    import brdf_amd
    cal = P.read_cal("bunny.cal")
    H, W, fovy, near, far = 576, 768, 46.6, 0.1, 1000.0
    m = brdf_amd.make_frustum(fovy, W / H, near, far, cal["cx"], cal["cy"], H, W)
    height = near * math.tan(fovy / 2 * (3.14159265 / 180))  # glutcallbacks.cpp:628-632
    width = height * (W / H)
    off_y, off_x = 2.0 * (H / 2.0 - cal["cy"]) / H, 2.0 * (W / 2.0 - cal["cx"]) / W
    l, r, b, t = -width + off_x, width + off_x, -height - off_y, height - off_y
    want = [2 * near / (r - l), 0, 0, 0, 0, 2 * near / (t - b), 0, 0, (r + l) / (r - l), (t + b) / (t - b), -(far + near) / (far - near), -1, 0, 0,
            -2 * far * near / (far - near), 0]
    assert m.tolist() == want
    assert m[8] != 0.0 and m[9] != 0.0  # the principal point is off centre: the frustum is asymmetric


def test_parse_cal_reads_every_committed_file():
    import brdf_amd
    names = P.cal_files()
    assert len(names) == 15 and "bunny.cal" in names
    for name in names:
        cal = P.read_cal(name)
        assert cal["camera_model"] == "CameraTsai" and set(cal) == {"camera_model", *brdf_amd.raster.CAL_TAGS}
        n, o, a = (np.array([cal[k + "x"], cal[k + "y"], cal[k + "z"]]) for k in "noa")
        assert np.max(np.abs(np.cross(n, o) - a)) < 1e-12, name  # a right-handed frame, a the viewing direction
    assert P.read_cal("bunny.cal")["f"] == 669.79581407830256
    text = open(os.path.join(P.CAL_DIR, "bunny.cal")).read()
    for bad in (text + "<zoom>2</zoom>\n", text.replace("<sx>", "<sy>").replace("</sx>", "</sy>"), "\n".join(text.splitlines()[:-1]), text + "<cx>1</cx>\n",
                text.replace("</f>", "</g>")):
        with pytest.raises(ValueError):
            brdf_amd.parse_cal(bad)


@pytest.mark.parametrize("name", P.cal_files())
def test_tsai_camera_is_the_calibrated_pinhole(name):
    """100 seeded points in front of the camera: winX = u, winY = H - v of the direct formula to 1e-9 pixel (a cap: the matrix
    composition costs a few ulp of coordinates below 1e4, i.e. about 1e-12)"""
    import brdf_amd
    cal = P.read_cal(name)
    H, W = 576, 768
    mv, pr, vp = brdf_amd.tsai_camera(cal, H, W, 1.0, 5000.0)
    assert vp.tolist() == [0.0, 0.0, W, H]
    n, o, a, p = (np.array([cal[k + "x"], cal[k + "y"], cal[k + "z"]]) for k in "noap")
    rng = np.random.default_rng(sum(map(ord, name)))
    d = rng.uniform(50.0, 2000.0, size=(100, 1))
    X = p + d * a + rng.uniform(-0.6, 0.6, size=(100, 1)) * d * n + rng.uniform(-0.6, 0.6, size=(100, 1)) * d * o
    win, w, ok = brdf_amd.project_host(X, mv, pr, vp)
    xc = np.stack([(X - p) @ n, (X - p) @ o, (X - p) @ a], axis=1)
    u, v = cal["cx"] + cal["sx"] * cal["f"] * xc[:, 0] / xc[:, 2], cal["cy"] + cal["f"] * xc[:, 1] / xc[:, 2]
    assert ok.all() and np.all(w > 0) and np.max(np.abs(u)) < 1e4 and np.max(np.abs(v)) < 1e4
    assert np.max(np.abs(win[:, 0] - u)) <= 1e-9 and np.max(np.abs(win[:, 1] - (H - v))) <= 1e-9
    order = np.argsort(xc[:, 2])
    assert np.all(np.diff(win[order, 2]) > 0) and np.all((win[:, 2] > 0) & (win[:, 2] < 1))  # depth increases along a
