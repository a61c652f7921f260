"""Pixel maps and face normals on the device (brdf_hip_pixel_map_dev, brdf_hip_face_normals_dev) against their NumPy twins
(brdf_amd.pixel_map_host, brdf_amd.face_normals_host).  Meshes and cameras: tests/pixel_map_problems.py.  Every comparison is exact --
the BYTES of pixel_map, depth, face_pixels and stats:

  (1) by hand    the hand-written maps of tests/test_pixel_map_host.py, both modes, H = W = 1;
  (2) trouble    faces partly and wholly outside the viewport, beyond z = 1, behind the eye, with a NaN vertex and with a vertex index
                 outside the vertex array (dropped under validate=False, refused under validate=True);
  (3) scene      a full-viewport pair of triangles behind 70,001 small faces in perspective, 257 x 131: more than 256 setup workgroups
                 (so the offsets kernel walks more than one total per thread), boxes from one pixel to the whole viewport, degenerate
                 faces; twice the same bytes; without depth and face_pixels the same map; mode 0 on the same centroids into 64 x 64;
  (4) normals    the twin's bytes on the scene's 70,003 faces, degenerate ones among them, and cosines() takes them for the twin's;
  (5) pipeline   a sphere under the calibrated camera of a committed .cal: map and normals from the two entries, images painted by
                 capture_render, fitted by fit_capture_faces -- whose per-face pixel counts are the map's face_pixels."""
import copy
import functools

import numpy as np
import pytest

from tests import pixel_map_problems as P

pytestmark = pytest.mark.gpu
SCENE_H, SCENE_W = 131, 257


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what=""):
    """device result == twin, byte for byte"""
    assert np.array_equal(got.pixel_map.cpu().numpy().view(np.uint8), want.pixel_map.view(np.uint8)), (what, "pixel_map")
    if got.depth is not None:
        assert np.array_equal(got.depth.cpu().numpy().view(np.uint8), want.depth.view(np.uint8)), (what, "depth")
    if got.face_pixels is not None:
        assert np.array_equal(got.face_pixels.cpu().numpy().view(np.uint8), want.face_pixels.view(np.uint8)), (what, "face_pixels")
    assert got.stats.dtype == np.int64 and got.stats.tolist() == want.stats.tolist(), (what, got.stats, want.stats)


def _both(gpu, v, f, mv, pr, vp, H, W, **kw):
    _, brdf_amd, _ = gpu
    got = brdf_amd.pixel_map(_dev(gpu, v), _dev(gpu, f), mv, pr, vp, H, W, want_depth=True, **kw)
    want = brdf_amd.pixel_map_host(v, f, mv, pr, vp, H, W, **{k: x for k, x in kw.items() if k in ("mode", "cull")})
    return got, want


@functools.lru_cache(maxsize=None)
def _scene():
    v, f, mv, pr = P.perspective_scene()
    return v, f, mv, pr, (0.0, 0.0, float(SCENE_W), float(SCENE_H))


@functools.lru_cache(maxsize=None)
def _scene_twin():
    import brdf_amd
    v, f, mv, pr, vp = _scene()
    return brdf_amd.pixel_map_host(v, f, mv, pr, vp, SCENE_H, SCENE_W)


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.hand_cases()))
def test_hand_written_maps(gpu, name):
    tris, kw, rule = P.hand_cases()[name]
    v, f = P.window_mesh(tris)
    got, want = _both(gpu, v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, **kw)
    assert np.array_equal(got.pixel_map.cpu().numpy(), P.expected_map(rule))
    _same(got, want, name)


def test_reference_map_by_hand(gpu):
    tris, want_map, want_depth, want_stats = P.centroid_case()
    v, f = P.window_mesh(tris)
    got, want = _both(gpu, v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, mode=0)
    assert np.array_equal(got.pixel_map.cpu().numpy(), want_map) and np.array_equal(got.depth.cpu().numpy(), want_depth)
    assert got.stats.tolist() == want_stats.tolist()
    _same(got, want)


@pytest.mark.parametrize("mode", [0, 1])
def test_one_pixel(gpu, mode):
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.5, 0.5, 0.5]])  # the centre (0, 0) is on the first face's hypotenuse
    f = np.array([[3, 3, 3], [0, 1, 2]], dtype=np.int32)
    got, want = _both(gpu, v, f, P.IDENTITY, P.IDENTITY, (0.0, 0.0, 1.0, 1.0), 1, 1, mode=mode)
    assert got.pixel_map.cpu().numpy().tolist() == [[1]] and got.stats[6] == 1
    _same(got, want)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------------
def test_trouble(gpu):
    _, brdf_amd, _ = gpu
    v, f = P.trouble_mesh()
    got, want = _both(gpu, v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, validate=False)
    assert got.stats[:5].tolist() == [3, 2, 0, 0, 1] and got.face_pixels.cpu().numpy()[[1, 2, 3, 4]].tolist() == [0, 0, 0, 0]
    _same(got, want, "mode 1")
    _same(*_both(gpu, v, f, P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N, mode=0, validate=False), "mode 0")
    for call in (lambda: brdf_amd.pixel_map(_dev(gpu, v), _dev(gpu, f), P.IDENTITY, P.IDENTITY, P.VIEWPORT, P.N, P.N),
                 lambda: brdf_amd.face_normals(_dev(gpu, v), _dev(gpu, f))):
        with pytest.raises(ValueError, match="face index outside the vertex array"):
            call()


def test_behind_the_eye(gpu):
    """the eye at z = 6 looks down -z: a face at z = 10 has w < 0 (dropped: no near-plane clipping), one through the eye's plane too"""
    _, brdf_amd, _ = gpu
    mv, pr = brdf_amd.gl_look_at((0.0, 0.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), brdf_amd.gl_frustum(-0.5, 0.5, -0.5, 0.5, 1.0, 20.0)
    v = np.array([[-1.0, -1.0, 10.0], [1.0, -1.0, 10.0], [0.0, 1.0, 10.0], [-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 7.0],
                  [0.0, 1.0, 6.0]])
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 6], [3, 4, 7]], dtype=np.int32)  # behind; in front; across the eye's plane; a vertex ON it (w = 0)
    got, want = _both(gpu, v, f, mv, pr, (0.0, 0.0, 32.0, 24.0), 24, 32)
    assert got.stats[:2].tolist() == [1, 3] and got.face_pixels.cpu().numpy().tolist()[0::2] == [0, 0] and got.face_pixels[1] > 0
    _same(got, want)
    _same(*_both(gpu, v, f, mv, pr, (0.0, 0.0, 32.0, 24.0), 24, 32, mode=0), "mode 0")  # gluProject only refuses w == 0


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------------
def test_scene_of_70001_small_faces_before_a_backdrop(gpu):
    _, brdf_amd, _ = gpu
    v, f, mv, pr, vp = _scene()
    want = _scene_twin()
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    got = brdf_amd.pixel_map(tv, tf, mv, pr, vp, SCENE_H, SCENE_W, want_depth=True)
    _same(got, want)
    assert f.shape[0] > 256 * 256 and want.stats[0] > 50000 and want.stats[2] >= 70  # multi-block scan; the degenerate faces
    assert want.stats[6] == SCENE_H * SCENE_W and want.face_pixels[:2].sum() > 0 and want.stats[5] > 2 * SCENE_H * SCENE_W  # the backdrop shows through
    again = brdf_amd.pixel_map(tv, tf, mv, pr, vp, SCENE_H, SCENE_W, want_depth=True)  # twice the same bytes
    _same(again, want, "again")
    bare = brdf_amd.pixel_map(tv, tf, mv, pr, vp, SCENE_H, SCENE_W, want_depth=False, want_face_pixels=False)
    assert bare.depth is None and bare.face_pixels is None
    _same(bare, want, "without depth and face_pixels")
    culled = brdf_amd.pixel_map(tv, tf, mv, pr, vp, SCENE_H, SCENE_W, cull=1, want_depth=True)
    _same(culled, brdf_amd.pixel_map_host(v, f, mv, pr, vp, SCENE_H, SCENE_W, cull=1), "cull")
    assert culled.stats[3] > 25000


def test_reference_map_of_70001_centroids_in_64_by_64(gpu):
    v, f, mv, pr, _ = _scene()
    got, want = _both(gpu, v, f, mv, pr, (0.0, 0.0, 64.0, 64.0), 64, 64, mode=0)
    assert want.stats[0] > 8 * 64 * 64 and want.stats[6] <= 64 * 64  # heavy collisions: more than eight centroids a pixel
    _same(got, want)
    off, want_off = _both(gpu, v, f, mv, pr, (-20.0, 10.0, 64.0, 64.0), 40, 30, mode=0)  # a viewport that is not the map: refusals on both sides
    assert want_off.stats[4] > 0 and want_off.stats[7] > 0
    _same(off, want_off, "shifted viewport")


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------------
def test_face_normals_bytes_and_cosines_takes_them(gpu):
    _, brdf_amd, _ = gpu
    v, f, _, _, _ = _scene()
    f = f.copy()
    f[7, 0] = v.shape[0]  # validate=False: NaN
    want = brdf_amd.face_normals_host(v, f)
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    got = brdf_amd.face_normals(tv, tf, validate=False)
    assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
    assert np.isnan(want[7]).all()
    degenerate = np.flatnonzero(f[:, 1] == f[:, 2])
    assert degenerate.size >= 70 and not want[degenerate].any()  # zero cross product: stays unnormalised
    f[7, 0] = 0
    tf, leds, view = _dev(gpu, f), brdf_amd.led_table(), np.array([0.3, -0.2, 6.0])
    tn = brdf_amd.face_normals(tv, tf)
    a = brdf_amd.cosines(tv, tf, tn, leds, view, rv_mode=1).cpu().numpy()
    b = brdf_amd.cosines(tv, tf, _dev(gpu, brdf_amd.face_normals_host(v, f)), leds, view, rv_mode=1).cpu().numpy()
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------------
def test_sphere_under_a_calibrated_camera_feeds_the_capture(gpu):
    torch, brdf_amd, _ = gpu
    H, W, model = 120, 160, brdf_amd.MODEL_BLINN_PHONG
    cal = copy.deepcopy(P.read_cal("bunny.cal"))  # calibrated for 768 x 576: scaled to 160 x 120 and re-posed to look at the origin
    cal.update(f=cal["f"] * W / 768, cx=cal["cx"] * W / 768, cy=cal["cy"] * H / 576)
    n, o, a = (np.array([cal[k + "x"], cal[k + "y"], cal[k + "z"]]) for k in "noa")
    eye = -2.8 * a
    cal.update(px=eye[0], py=eye[1], pz=eye[2])
    mv, pr, vp = brdf_amd.tsai_camera(cal, H, W, 0.5, 10.0)
    v, f = P.sphere(32, 32)
    assert 1900 <= f.shape[0] <= 2100
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    pm = brdf_amd.pixel_map(tv, tf, mv, pr, vp, H, W, want_depth=True)
    _same(pm, brdf_amd.pixel_map_host(v, f, mv, pr, vp, H, W), "sphere")
    tn = brdf_amd.face_normals(tv, tf)
    fp = pm.face_pixels.cpu().numpy()
    nrm = tn.cpu().numpy()
    centre = v[f].mean(axis=1)
    assert np.all((nrm * centre).sum(axis=1) > 0.99)  # outward unit normals
    assert np.all(((centre - eye) * nrm).sum(axis=1)[fp > 0] < 0) and 500 < (fp > 0).sum() < 1000 and 4000 < pm.stats[6] < 12000  # only the near side is seen
    ring = np.arange(16) * (2 * np.pi / 16)
    leds = eye + 1.5 * (np.cos(ring)[:, None] * n + np.sin(ring)[:, None] * o)
    rng = np.random.default_rng(5)
    truth = np.array([0.4, 0.5, 8.0]) * rng.uniform(0.7, 1.3, size=(f.shape[0], 3, 3))
    images = brdf_amd.capture_render(model, pm.pixel_map, tv, tf, tn, leds, eye, truth, rv_mode=1, want_values=False).rendered
    r = brdf_amd.fit_capture_faces(model, images, pm.pixel_map, tv, tf, tn, leds, eye, rv_mode=1, itmax=20, want_stats=False)
    assert np.array_equal(r.face_pixels.cpu().numpy(), fp) and r.n_pixels == pm.stats[6] and r.n_faces == (fp > 0).sum()
    assert np.array_equal(r.count.cpu().numpy(), 16 * np.repeat(fp[:, None], 3, axis=1))  # the rule is off: 16 samples a pixel and channel
