"""Rendering a fitted capture on the device (brdf_hip_capture_render_dev, brdf_hip_capture_render_residuals_dev,
brdf_hip_surfaces_from_materials_dev).  Captures: tests/capture_problems.py, tests/materials_problems.py.  Everything is exact:

  (1) values     face_values has the BYTES of model_eval on cosines' planes, every model at 1, 5, 16 and 64 lights, the surfaces a
                 fit_capture_faces result; a face of NaN cosines and a NaN surface row give NaN values and grey level 0;
  (2) images     rendered == render_capture_host on the DEVICE's face_values, byte for byte: rows of 93 bytes (3 W % 4 = 1), images of
                 2139 bytes (so every image starts at another offset from a 16-byte boundary), a base address off by one, background
                 0, 200 and -1 (a pre-filled buffer), map entries < -1 and >= nf, a surface scaled until both clamps are hit;
  (3) residuals  every integer map == render_residuals_host, byte for byte, rule off and under RULE, two calls the same bytes: every
                 model, 5 / 16 / 64 lights, big_capture() (70,001 faces, faces that span tiles and workgroups), wide_capture(64, ...),
                 lights the fit never saw (fit on 0 ... 11, evaluated on 12 ... 15), and calls that ask for one kind of map only;
  (4) round trip rendered images fed back with the same surfaces: every sumsq and abs_max is 0, every count the carried pixels;
  (5) materials  surfaces_from_materials has the bytes of the NumPy gather (labels -1 and K among them), and a fit_capture_materials
                 result on the planted capture renders through it."""
import functools

import numpy as np
import pytest

from tests import capture_problems as P
from tests import materials_problems as M

pytestmark = pytest.mark.gpu
INT_MAPS = ("light_count", "light_sum", "light_sumsq", "face_light_count", "face_light_sum", "face_light_sumsq", "abs_max", "worst_light")
OFF = dict(v_min=0, v_max=255, cos_min=-2.0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mesh(gpu, cap):
    return _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]), _dev(gpu, cap["nrm"])


def _planes(gpu, cap, leds=None):
    """the device's cosine planes of ALL faces, [nf,3,L], on the host"""
    _, brdf_amd, _ = gpu
    return brdf_amd.cosines(*_mesh(gpu, cap), cap["leds"] if leds is None else leds, cap["view"], rv_mode=1).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fitted(gpu, model, lights, nan_face=False):
    """(the capture, fit_capture_faces' surfaces on it [nf,3,3] on the host)"""
    _, brdf_amd, _ = gpu
    cap = P.rule_capture(model, nan_face=nan_face, lights=lights)
    r = brdf_amd.fit_capture_faces(model, _dev(gpu, cap["images"]), _dev(gpu, cap["pixel_map"]), *_mesh(gpu, cap), cap["leds"], cap["view"], rv_mode=1,
                                   p0=P.P0, lb=P.LB, ub=P.UB, opts=P.OPTS, want_stats=False, **P.RULE)
    return cap, r.surfaces.cpu().numpy()


def _plausible_surfaces(model, nf, seed):
    """[nf,3,3]: the renderers' truth, a factor in [0.5, 1.5] per entry"""
    from brdf_amd import synth
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.array(synth.TRUTH[model])[None, None, :] * rng.uniform(0.5, 1.5, size=(nf, 3, 3)))


def _render(gpu, cap, model, surfaces, leds=None, pixel_map=None, **kw):
    _, brdf_amd, _ = gpu
    return brdf_amd.capture_render(model, _dev(gpu, cap["pixel_map"] if pixel_map is None else pixel_map), *_mesh(gpu, cap),
                                   cap["leds"] if leds is None else leds, cap["view"], surfaces, rv_mode=1, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- (1) values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [1, 5, 16, 64])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_values_have_the_bytes_of_model_eval_on_the_cosine_planes(gpu, model, lights):
    torch, brdf_amd, _ = gpu
    cap, surfaces = _fitted(gpu, model, lights)
    got = _render(gpu, cap, model, surfaces, want_images=False)
    assert got.rendered is None and tuple(got.face_values.shape) == (cap["nf"], 3, lights)
    values = got.face_values.cpu().numpy()
    planes = brdf_amd.cosines(*_mesh(gpu, cap), cap["leds"], cap["view"], rv_mode=1)
    for f in range(cap["nf"]):
        for c in range(3):
            want = brdf_amd.model_eval(model, planes[f], surfaces[f, c]).cpu().numpy()
            assert np.array_equal(_bits(values[f, c]), _bits(want)), (f, c)
    assert np.nanmax(values) > 0.05  # (Phong's pow of a negative cosine is NaN: its bytes are compared like any other)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_nan_cosines_and_a_nan_surface_row_give_nan_values_and_grey_level_zero(gpu, model):
    torch, brdf_amd, _ = gpu
    cap, surfaces = _fitted(gpu, model, 16, True)
    surfaces = surfaces.copy()
    carried = np.unique(cap["pixel_map"][cap["pixel_map"] >= 0])
    row = int(carried[carried != cap["nan_face"]][2])
    surfaces[row, 1, :] = np.nan
    got = _render(gpu, cap, model, surfaces, background=9)
    values, img = got.face_values.cpu().numpy(), got.rendered.cpu().numpy()
    assert np.isnan(values[cap["nan_face"]]).all() and np.isnan(values[row, 1]).all() and np.isfinite(values[row, 0]).all()
    planes = brdf_amd.cosines(*_mesh(gpu, cap), cap["leds"], cap["view"], rv_mode=1)
    for f, c in ((cap["nan_face"], 0), (row, 1), (row, 2)):
        assert np.array_equal(_bits(values[f, c]), _bits(brdf_amd.model_eval(model, planes[f], surfaces[f, c]).cpu().numpy())), (f, c)
    flipped = cap["pixel_map"][::-1]
    assert (flipped == cap["nan_face"]).sum() == 10 and not img[:, flipped == cap["nan_face"], :].any()
    assert (flipped == row).any() and not img[:, flipped == row, 1].any()
    assert np.array_equal(img, brdf_amd.render_capture_host(values, cap["pixel_map"], 9))


# ---- (2) images -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _image_problem(gpu):
    """rule_capture(1) with map entries < -1 and >= nf, and one carried face -- 8 pixels, its planes 0 and 1 above 0.4 at every light --
    scaled until its values pass 1 (channel 0: {40, 40, 1}) and fall below 0 (channel 1: {-1, -1, 1})"""
    cap, surfaces = _fitted(gpu, 1, 16)
    surfaces = surfaces.copy()
    pixel_map = cap["pixel_map"].copy()
    ys, xs = np.nonzero(pixel_map == -1)
    pixel_map[ys[:4], xs[:4]] = [-5, cap["nf"], cap["nf"] + 7, -2 ** 31]
    pixel_map[0, 0], pixel_map[-1, -1] = -3, cap["nf"]  # the first and the last byte of every image: background
    face = 16
    assert cap["ang"][face, :2].min() > 0.4
    surfaces[face, 0] = [40.0, 40.0, 1.0]
    surfaces[face, 1] = [-1.0, -1.0, 1.0]
    return cap, surfaces, pixel_map, face


@pytest.mark.parametrize("background", [0, 200, -1])
def test_images_are_the_twin_on_the_device_values(gpu, background):
    torch, brdf_amd, dev = gpu
    cap, surfaces, pixel_map, face = _image_problem(gpu)
    H, W = pixel_map.shape
    assert (3 * W) % 4 != 0 and (3 * H * W) % 16 != 0 and int((pixel_map == face).sum()) == 8
    held = torch.full((16, H, W, 3), 77, dtype=torch.uint8, device=dev)
    got = _render(gpu, cap, 1, surfaces, pixel_map=pixel_map, background=background, rendered=held, validate=False)
    assert got.rendered is held
    values, img = got.face_values.cpu().numpy(), got.rendered.cpu().numpy()
    assert values[face, 0].min() >= 1.0 and values[face, 1].max() < 0.0
    want = brdf_amd.render_capture_host(values, pixel_map, background, out=np.full((16, H, W, 3), 77, dtype=np.uint8))
    assert np.array_equal(img, want)
    flipped = pixel_map[::-1]
    assert np.all(img[:, flipped == face, 0] == 255) and not img[:, flipped == face, 1].any()       # both clamps
    outside = (flipped < 0) | (flipped >= cap["nf"])
    assert outside.sum() > 100 and np.all(img[:, outside, :] == (77 if background < 0 else background))
    inner = img[:, ~outside & (flipped != face), :]
    assert len(np.unique(inner)) > 20  # a picture, not a clamp
    # the same image through a base address that is off a boundary by one, and without the value table
    raw = torch.full((16 * H * W * 3 + 1,), 77, dtype=torch.uint8, device=dev)
    off = _render(gpu, cap, 1, surfaces, pixel_map=pixel_map, background=background, rendered=raw[1:].view(16, H, W, 3), want_values=False, validate=False)
    assert off.face_values is None and off.rendered.data_ptr() % 16 == 1
    assert np.array_equal(off.rendered.cpu().numpy(), want) and int(raw[0]) == 77


# ---- (3) residuals --------------------------------------------------------------------------------------------------------------------
def _residuals(gpu, cap, model, surfaces, images=None, leds=None, **rule):
    _, brdf_amd, _ = gpu
    return brdf_amd.capture_render_residuals(model, _dev(gpu, cap["images"] if images is None else images), _dev(gpu, cap["pixel_map"]), *_mesh(gpu, cap),
                                             cap["leds"] if leds is None else leds, cap["view"], surfaces, rv_mode=1, validate=False, **rule)


def _check_residuals(gpu, cap, model, surfaces, images=None, leds=None):
    """both rules: every integer map against the twin on the device's planes and values, twice; returns the rule-off result"""
    torch, brdf_amd, _ = gpu
    images = cap["images"] if images is None else images
    planes = _planes(gpu, cap, leds)
    carried = int(((cap["pixel_map"] >= 0) & (cap["pixel_map"] < cap["nf"])).sum())
    first = None
    for rule in (OFF, P.RULE):
        got = _residuals(gpu, cap, model, surfaces, images, leds, **rule)
        again = _residuals(gpu, cap, model, surfaces, images, leds, **rule)
        values = got.face_values.cpu().numpy()
        want = brdf_amd.render_residuals_host(images, cap["pixel_map"], planes, model, values, **rule)
        assert got.n_pixels == carried
        for name in INT_MAPS:
            mine, twin = getattr(got, name).cpu().numpy(), getattr(want, name)
            assert mine.dtype == twin.dtype and mine.shape == twin.shape, name
            assert np.array_equal(mine, twin), (name, rule, int((mine != twin).sum()))
            assert mine.tobytes() == getattr(again, name).cpu().numpy().tobytes(), name
        count = got.light_count.cpu().numpy()
        if rule is OFF:
            with np.errstate(invalid="ignore"):
                nan_faces = np.isnan(planes).any(axis=(1, 2))
            assert np.all(count == carried - int(np.isin(cap["pixel_map"], np.flatnonzero(nan_faces)).sum()))
            first = got
        else:
            assert 0 < count.sum() < 3 * planes.shape[2] * carried
        per, overall = got.psnr()
        print(f"model {model} L {planes.shape[2]} rule {rule['v_min'], rule['v_max'], rule['cos_min']}: compared {int(count.sum())}, "
              f"PSNR {overall:.2f} dB, max |d| {int(got.abs_max.max())}")
    return first


@pytest.mark.parametrize("lights", [5, 16, 64])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_residual_maps_are_the_twin(gpu, model, lights):
    cap, surfaces = _fitted(gpu, model, lights, lights == 16)  # (16 lights: with the face of NaN cosines)
    got = _check_residuals(gpu, cap, model, surfaces)
    sumsq = got.light_sumsq.cpu().numpy()
    assert sumsq.sum() > 0 and (got.light_sum.cpu().numpy() != 0).any()


def test_residuals_of_many_faces_and_faces_that_span_tiles(gpu):
    cap = P.big_capture()
    assert cap["nf"] == 70001 and cap["sizes"].max() >= 300  # 16 pixels a tile: a face of 300 pixels spans 19 tiles
    got = _check_residuals(gpu, cap, 1, _plausible_surfaces(1, cap["nf"], 3))
    count = got.face_light_count.cpu().numpy()
    assert np.all(count[cap["big_face"]] == 300) and np.all(count[[0, 65535, 65536, cap["nf"] - 1]] > 0)
    assert int((count[:, 0, 0] > 0).sum()) == 644


def test_residuals_at_64_lights_over_many_workgroups(gpu):
    cap = P.wide_capture(64, 150, 150)  # 22,500 pixels, 4 a tile: 5,625 tiles, more than the grid
    _check_residuals(gpu, cap, 1, _plausible_surfaces(1, cap["nf"], 5))


def test_residuals_at_lights_the_fit_never_saw(gpu):
    torch, brdf_amd, _ = gpu
    model = 1
    cap = P.rule_capture(model)
    fit = brdf_amd.fit_capture_faces(model, _dev(gpu, cap["images"][:12]), _dev(gpu, cap["pixel_map"]), *_mesh(gpu, cap), cap["leds"][:12], cap["view"],
                                     rv_mode=1, p0=P.P0, lb=P.LB, ub=P.UB, opts=P.OPTS, want_stats=False, **P.RULE)
    held_images, held_leds = np.ascontiguousarray(cap["images"][12:]), np.ascontiguousarray(cap["leds"][12:])
    got = _check_residuals(gpu, cap, model, fit.surfaces, held_images, held_leds)
    assert tuple(got.light_count.shape) == (4, 3)
    fitted = _residuals(gpu, cap, model, fit.surfaces, np.ascontiguousarray(cap["images"][:12]), np.ascontiguousarray(cap["leds"][:12]), **P.RULE)
    print(f"fit on lights 0 ... 11: PSNR {fitted.psnr()[1]:.2f} dB there, {_residuals(gpu, cap, model, fit.surfaces, held_images, held_leds, **P.RULE).psnr()[1]:.2f} dB "
          "on lights 12 ... 15")


def test_a_call_may_ask_for_one_kind_of_map(gpu):
    """the raw entry with NULL maps: what is asked for has the bytes of the call that asks for everything"""
    import ctypes as C
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, lib
    model = 1
    cap, surfaces = _fitted(gpu, model, 16)
    full = _residuals(gpu, cap, model, surfaces, **P.RULE)
    t = [_dev(gpu, cap[k]) for k in ("images", "pixel_map", "vertices", "faces", "nrm")] + [_dev(gpu, surfaces)]
    leds, view = np.ascontiguousarray(cap["leds"]), np.ascontiguousarray(cap["view"])
    H, W = cap["pixel_map"].shape
    nf = cap["nf"]
    shapes = dict(light_count=((16, 3), torch.int64), light_sum=((16, 3), torch.int64), light_sumsq=((16, 3), torch.int64),
                  face_light_count=((nf, 3, 16), torch.int32), face_light_sum=((nf, 3, 16), torch.int64), face_light_sumsq=((nf, 3, 16), torch.int64),
                  abs_max=((H, W, 3), torch.uint8), worst_light=((H, W, 3), torch.uint8))
    for asked in (("light_sumsq",), ("face_light_sum",), ("worst_light",), ("light_count", "abs_max"), ()):
        out = {k: torch.full(shapes[k][0], 5, dtype=shapes[k][1], device=dev) for k in asked}
        ptrs = [out[k].data_ptr() if k in out else None for k in INT_MAPS]
        npx = C.c_longlong(-1)
        with torch.cuda.device(dev):
            rc = lib.brdf_hip_capture_render_residuals_dev(model, t[0].data_ptr(), 16, H, W, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                                           nf, leds.ctypes.data_as(D), view.ctypes.data_as(D), 1, t[5].data_ptr(), 1, 254, 0.0, *ptrs, None,
                                                           C.byref(npx), None)
        torch.cuda.synchronize()
        assert rc == 0, brdf_amd.last_error()
        assert npx.value == full.n_pixels
        for k in asked:
            assert out[k].cpu().numpy().tobytes() == getattr(full, k).cpu().numpy().tobytes(), (asked, k)


# ---- (4) round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rule", "big"])
def test_rendered_images_have_no_residual_against_their_surfaces(gpu, which):
    if which == "rule":
        model = 2
        cap, surfaces = _fitted(gpu, model, 16)
    else:
        model, cap = 1, P.big_capture()
        surfaces = _plausible_surfaces(model, cap["nf"], 3)
    rendered = _render(gpu, cap, model, surfaces, background=31, validate=False).rendered
    got = _residuals(gpu, cap, model, surfaces, images=rendered.cpu().numpy(), **OFF)
    carried = int(((cap["pixel_map"] >= 0) & (cap["pixel_map"] < cap["nf"])).sum())
    assert got.n_pixels == carried and carried > 0
    assert np.all(got.light_count.cpu().numpy() == carried)
    assert not got.light_sumsq.cpu().numpy().any() and not got.light_sum.cpu().numpy().any()
    assert not got.face_light_sumsq.cpu().numpy().any() and not got.abs_max.cpu().numpy().any()
    assert int(got.face_light_count.cpu().numpy()[:, 0, 0].sum()) == carried
    worst = got.worst_light.cpu().numpy()
    inside = (cap["pixel_map"] >= 0) & (cap["pixel_map"] < cap["nf"])
    assert not worst[inside].any() and np.all(worst[~inside] == 255)
    assert got.psnr()[1] == np.inf


# ---- (5) materials --------------------------------------------------------------------------------------------------------------------
def test_surfaces_from_materials_is_the_gather(gpu):
    torch, brdf_amd, dev = gpu
    rng = np.random.default_rng(11)
    nf, K = 1000, 5
    materials = rng.uniform(0.1, 60.0, size=(K, 3, 3))
    labels = rng.integers(-1, K + 1, size=nf).astype(np.int32)  # -1 and K among them
    labels[:4] = [-1, K, 0, K - 1]
    fill = np.array([0.25, 0.5, 7.0])
    got = brdf_amd.surfaces_from_materials(_dev(gpu, labels), materials, fill).cpu().numpy()
    inside = (labels >= 0) & (labels < K)
    want = np.where(inside[:, None, None], materials[np.where(inside, labels, 0)], fill[None, None, :])
    assert got.shape == (nf, 3, 3) and got.tobytes() == np.ascontiguousarray(want).tobytes()
    one = brdf_amd.surfaces_from_materials(torch.zeros(7, dtype=torch.int32, device=dev), materials[2:3]).cpu().numpy()  # the single-BRDF case
    assert one.tobytes() == np.ascontiguousarray(np.broadcast_to(materials[2], (7, 3, 3))).tobytes()


def test_a_materials_result_renders_through_its_labels(gpu):
    torch, brdf_amd, _ = gpu
    cap = M.planted_capture()
    args = tuple(_dev(gpu, cap[k]) for k in ("images", "pixel_map", "vertices", "faces", "nrm")) + (cap["leds"], cap["view"])
    fit = brdf_amd.fit_capture_materials(M.MODEL, *args, np.ascontiguousarray(cap["truth"]), rounds=2, rv_mode=1, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS,
                                         want_stats=False, validate=False, **M.RULE)
    labels = fit.labels.cpu().numpy()
    assert M.purity(labels, cap["planted"], M.K_PLANTED) == 1.0  # the planted truth as seeds: every face finds its material
    surfaces = brdf_amd.surfaces_from_materials(fit.labels, fit.materials)
    assert surfaces.cpu().numpy().tobytes() == fit.materials.cpu().numpy()[labels].tobytes()
    got = _check_residuals(gpu, cap, M.MODEL, surfaces)
    rendered = _render(gpu, cap, M.MODEL, surfaces).rendered.cpu().numpy()
    assert np.array_equal(rendered, brdf_amd.render_capture_host(got.face_values.cpu().numpy(), cap["pixel_map"], 0))
    single = brdf_amd.surfaces_from_materials(torch.zeros_like(fit.labels), fit.materials[:1])
    one = _residuals(gpu, cap, M.MODEL, single, **M.RULE)
    print(f"planted capture: PSNR {_residuals(gpu, cap, M.MODEL, surfaces, **M.RULE).psnr()[1]:.2f} dB with its 4 materials, {one.psnr()[1]:.2f} dB with one")
