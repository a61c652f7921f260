"""Cast shadows on the device (brdf_hip_light_visibility_dev, brdf_hip_capture_apply_visibility_dev) against their NumPy twins
(brdf_amd.light_visibility_host, brdf_amd.apply_visibility_host).  Scenes: tests/light_visibility_problems.py.  Every comparison is
exact -- the BYTES of the words, the stats, the images and the counts:

  (1) by hand    the hand-written scenes of tests/test_light_visibility_host.py;
  (2) random     the jittered floor under floating blocker quads (its shadowed share lies between 10 % and 90 %: the host tests) at
                 face counts around the wave, the workgroup and the LDS tile; 2,051 faces are 17 tiles of 128 in 5 occluder ranges of
                 4 tiles and 9 workgroups of origins; 1, 5 and 64 lights (one, one partly filled and eight groups of 8); with and
                 without normals; t_min = 0; twice the same bytes; invalid faces among valid ones;
  (3) painting   3 W % 4 = 1 (so the images' bases take every alignment modulo 4), a base one byte off a 16-byte boundary, a tail
                 of fewer than four pixels, in place and out of place, map entries -1, -2 and >= nf, the counts; capture_render followed
                 by apply_visibility against the composition of the twins;
  (4) pipeline   a flat floor under a floating blocker, rendered with one planted Blinn-Phong material, shadows planted with the HOST
                 twin's words and removed with the DEVICE's: the per-face sample counts are pixels x lit lights; the single-BRDF fit
                 of the masked capture reproduces it as well as that of the shadow-free one (within one grey level), the fit of the
                 unmasked one does not."""
import functools

import numpy as np
import pytest

from tests import light_visibility_problems as P

pytestmark = pytest.mark.gpu


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
    lit = got.face_lit.cpu().numpy()
    assert lit.dtype == np.int64 and np.array_equal(lit.view(np.uint8), want.face_lit.view(np.uint8)), (what, "face_lit", int((lit != want.face_lit).sum()))
    assert got.stats.dtype == np.int64 and got.stats.tolist() == want.stats.tolist(), (what, got.stats, want.stats)


@functools.lru_cache(maxsize=None)
def _scene(nf, L=16):
    return P.random_scene(nf, L)


@functools.lru_cache(maxsize=None)
def _twin(nf, L=16, with_normals=False, t_min=1e-9):
    import brdf_amd
    v, f, leds = _scene(nf, L)
    return brdf_amd.light_visibility_host(v, f, leds, normals=P.scene_normals(v, f) if with_normals else None, t_min=t_min)


def _device(gpu, nf, L=16, with_normals=False, t_min=1e-9):
    _, brdf_amd, _ = gpu
    v, f, leds = _scene(nf, L)
    normals = _dev(gpu, P.scene_normals(v, f)) if with_normals else None
    return brdf_amd.light_visibility(_dev(gpu, v), _dev(gpu, f), leds, normals=normals, t_min=t_min)


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.hand_scenes()))
def test_hand_written_scenes(gpu, name):
    _, brdf_amd, _ = gpu
    v, f, leds, with_normals, expected, stats = P.hand_scenes()[name]
    normals = P.scene_normals(v, f) if with_normals else None
    got = brdf_amd.light_visibility(_dev(gpu, v), _dev(gpu, f), leds, normals=None if normals is None else _dev(gpu, normals), validate=False)
    assert got.face_lit.cpu().numpy().tolist() == P.words(expected).tolist() and got.stats.tolist() == stats
    _same(got, brdf_amd.light_visibility_host(v, f, leds, normals=normals), name)
    m = brdf_amd.lit_matrix(got.face_lit, len(leds))
    assert m.is_cuda and np.array_equal(m.cpu().numpy(), brdf_amd.lit_matrix(P.words(expected), len(leds)))


def test_bad_index_is_refused_under_validate(gpu):
    _, brdf_amd, _ = gpu
    v, f, leds = P.hand_scenes()["bad_index"][:3]
    with pytest.raises(ValueError, match="face index outside the vertex array"):
        brdf_amd.light_visibility(_dev(gpu, v), _dev(gpu, f), leds)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2051])
def test_random_scene_under_sixteen_lights(gpu, nf):
    want = _twin(nf)
    print(nf, "faces:", dict(zip(("valid", "invalid", "away", "lit", "shadowed"), want.stats.tolist())))
    _same(_device(gpu, nf), want, nf)


@pytest.mark.parametrize("L", [1, 5, 64])
def test_random_scene_of_257_faces_under_other_light_counts(gpu, L):
    _same(_device(gpu, 257, L), _twin(257, L), L)
    _same(_device(gpu, 257, L, with_normals=True), _twin(257, L, True), (L, "normals"))


def test_random_scene_with_normals_and_at_t_min_zero(gpu):
    for nf in (257, 1025):
        want = _twin(nf, 16, True)
        assert want.stats[2] > 0 and want.stats[4] > 0  # pairs that face away next to shadowed ones
        _same(_device(gpu, nf, 16, with_normals=True), want, (nf, "normals"))
    _same(_device(gpu, 257, 16, t_min=0.0), _twin(257, 16, False, 0.0), "t_min = 0")
    _same(_device(gpu, 257, 16, with_normals=True, t_min=0.25), _twin(257, 16, True, 0.25), "t_min = 0.25")


def test_two_calls_give_the_same_bytes(gpu):
    torch, brdf_amd, _ = gpu
    v, f, leds = _scene(2051)
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    first, second = brdf_amd.light_visibility(tv, tf, leds), brdf_amd.light_visibility(tv, tf, leds)
    assert torch.equal(first.face_lit, second.face_lit) and first.stats.tolist() == second.stats.tolist()
    _same(second, _twin(2051), "again")


def test_invalid_faces_among_valid_ones(gpu):
    _, brdf_amd, _ = gpu
    v, f, leds = _scene(257)
    v, f = P.spoil(v, f)
    normals = P.scene_normals(v, f)  # (NaN for the spoilt faces)
    want = brdf_amd.light_visibility_host(v, f, leds, normals=normals)
    assert 4 <= want.stats[1] <= 40 and not want.face_lit[[3, 5, 128, 255]].any()
    got = brdf_amd.light_visibility(_dev(gpu, v), _dev(gpu, f), leds, normals=_dev(gpu, normals), validate=False)
    _same(got, want, "with normals")
    _same(brdf_amd.light_visibility(_dev(gpu, v), _dev(gpu, f), leds, validate=False), brdf_amd.light_visibility_host(v, f, leds), "without")


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------------
def _off_boundary(gpu, a, off):
    """a copy of the uint8 array `a` on the device whose first byte lies `off` bytes behind a 16-byte boundary"""
    torch, _, dev = gpu
    raw = torch.zeros(a.size + 32, dtype=torch.uint8, device=dev)
    start = (-raw.data_ptr()) % 16 + off
    t = raw[start:start + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


@pytest.mark.parametrize("L,H,W,nf,off", [(5, 13, 11, 9, 0), (5, 13, 11, 9, 1), (3, 64, 67, 40, 1), (64, 5, 3, 4, 0), (1, 1, 1, 1, 1), (2, 32, 32, 7, 0)])
def test_painting_against_the_twin(gpu, L, H, W, nf, off):
    torch, brdf_amd, _ = gpu
    images, pm, lit = P.paint_case(L, H, W, nf)
    assert (3 * W) % 4 == 1 or (H, W) in ((1, 1), (32, 32))  # (one pixel; every chunk whole and on a dword)
    assert H * W == 1 or ((pm < 0).any() and (pm >= nf).any())
    tpm, tlit = _dev(gpu, pm), _dev(gpu, lit)
    for level in (0, 200):
        want = brdf_amd.apply_visibility_host(images, pm, lit, level=level)
        src = _off_boundary(gpu, images, off)
        got = brdf_amd.apply_visibility(src, tpm, tlit, level=level)  # out of place, a new tensor
        assert got.images.data_ptr() != src.data_ptr() and np.array_equal(src.cpu().numpy(), images)
        assert np.array_equal(got.images.cpu().numpy(), want.images), ("out of place", level)
        assert got.shadowed.dtype == torch.int64 and got.shadowed.cpu().numpy().tolist() == want.shadowed.tolist()
        dst = _off_boundary(gpu, np.full_like(images, 77), (off + 2) % 16)  # out of place into a buffer of another alignment
        other = brdf_amd.apply_visibility(src, tpm, tlit, level=level, out=dst)
        assert other.images is dst and np.array_equal(dst.cpu().numpy(), want.images), ("into out", level)
        same = brdf_amd.apply_visibility(src, tpm, tlit, level=level, out=src)  # in place
        assert same.images is src and np.array_equal(src.cpu().numpy(), want.images), ("in place", level)
        assert same.shadowed.cpu().numpy().tolist() == want.shadowed.tolist()


def test_partly_overlapping_buffers_are_refused(gpu):
    torch, brdf_amd, dev = gpu
    images, pm, lit = P.paint_case(2, 4, 4, 3)
    raw = torch.zeros(images.size + 16, dtype=torch.uint8, device=dev)
    src, dst = raw[:images.size].view(images.shape), raw[16:16 + images.size].view(images.shape)
    with pytest.raises(RuntimeError, match="overlaps"):
        brdf_amd.apply_visibility(src, _dev(gpu, pm), _dev(gpu, lit), out=dst)


def _floor_under_a_blocker(g=12):
    """a flat g x g floor over [-1, 1]^2 at z = 0 and a quad over [-0.35, 0.35]^2 at z = 0.5, all counter-clockwise seen from above; eight
    lights on a ring of radius 1 at z = 2: every cosine varies smoothly over the floor and stays well above 0"""
    v, f = P.grid(g)
    v = v * [2.0 / g, 2.0 / g, 1.0] - [1.0, 1.0, 0.0]
    b = v.shape[0]
    v = np.concatenate([v, [(-0.35, -0.35, 0.5), (0.35, -0.35, 0.5), (0.35, 0.35, 0.5), (-0.35, 0.35, 0.5)]])
    f = np.concatenate([f, [(b, b + 1, b + 2), (b, b + 2, b + 3)]]).astype(np.int32)
    ring = (np.arange(8) + 0.25) * (2.0 * np.pi / 8)
    leds = np.stack([np.cos(ring), np.sin(ring), np.full(8, 2.0)], axis=1)
    return v, f, leds


def test_render_then_paint_equals_the_twins_composed(gpu):
    _, brdf_amd, _ = gpu
    v, f, leds = _floor_under_a_blocker()
    H, W, eye = 45, 67, np.array([0.0, 0.0, 3.0])
    cam = (brdf_amd.gl_look_at(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), brdf_amd.gl_frustum(-0.4, 0.4, -0.4, 0.4, 1.0, 10.0), (0.0, 0.0, float(W), float(H)))
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    pm, tn = brdf_amd.pixel_map(tv, tf, *cam, H, W).pixel_map, brdf_amd.face_normals(tv, tf)
    surfaces = np.tile(np.array([[0.4, 0.3, 10.0], [0.45, 0.3, 10.0], [0.5, 0.3, 10.0]]), (f.shape[0], 1, 1))
    r = brdf_amd.capture_render(brdf_amd.MODEL_BLINN_PHONG, pm, tv, tf, tn, leds, eye, surfaces, rv_mode=1, background=3)
    vis = brdf_amd.light_visibility(tv, tf, leds, normals=tn)
    got = brdf_amd.apply_visibility(r.rendered, pm, vis.face_lit, level=0, out=r.rendered)
    rendered = brdf_amd.render_capture_host(r.face_values.cpu().numpy(), pm.cpu().numpy(), 3)
    want = brdf_amd.apply_visibility_host(rendered, pm.cpu().numpy(), brdf_amd.light_visibility_host(v, f, leds, normals=tn.cpu().numpy()).face_lit)
    assert np.array_equal(got.images.cpu().numpy(), want.images) and got.shadowed.cpu().numpy().tolist() == want.shadowed.tolist()
    assert want.shadowed.min() > 0 and (want.images == 3).any()  # every light casts a shadow the camera sees; the background stays


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_masked_shadows_do_not_bias_the_fits(gpu):
    """Measured on the MI355X: the largest abs_max is 1 grey level on the shadow-free render, 1 on the masked capture and
    167 on the shadowed, unmasked one.  Only the relations are asserted."""
    torch, brdf_amd, _ = gpu
    model, rule = brdf_amd.MODEL_BLINN_PHONG, dict(v_min=1, v_max=254, cos_min=0.0)
    v, f, leds = _floor_under_a_blocker()
    nf, L, H, W, eye = f.shape[0], leds.shape[0], 96, 96, np.array([0.0, 0.0, 3.0])
    cam = (brdf_amd.gl_look_at(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), brdf_amd.gl_frustum(-0.4, 0.4, -0.4, 0.4, 1.0, 10.0), (0.0, 0.0, float(W), float(H)))
    tv, tf = _dev(gpu, v), _dev(gpu, f)
    pmap, tn = brdf_amd.pixel_map(tv, tf, *cam, H, W), brdf_amd.face_normals(tv, tf)
    pm, face_pixels = pmap.pixel_map, pmap.face_pixels.cpu().numpy()
    mesh = (pm, tv, tf, tn, leds, eye)
    planted = np.tile(np.array([[0.4, 0.3, 10.0], [0.45, 0.3, 10.0], [0.5, 0.3, 10.0]]), (nf, 1, 1))
    clean = brdf_amd.capture_render(model, *mesh, planted, rv_mode=1, want_values=False).rendered
    # shadows planted with the HOST twin's words ...
    twin = brdf_amd.light_visibility_host(v, f, leds, normals=tn.cpu().numpy())
    shadowed = brdf_amd.apply_visibility(clean, pm, _dev(gpu, twin.face_lit), level=12)
    dark = (shadowed.images != clean).any(dim=3)
    assert shadowed.shadowed.sum() > 200 and int(dark.sum()) == int(shadowed.shadowed.sum())
    assert int(clean[dark].min()) >= 12 + 30  # every planted sample lies at least 30 grey levels under the rendered value
    lit_lights = brdf_amd.lit_matrix(twin.face_lit, L).sum(axis=1)
    assert lit_lights[face_pixels > 0].min() >= 3 and lit_lights[face_pixels > 0].min() < L  # every face the camera sees keeps a fit
    # ... and removed with the DEVICE's
    vis = brdf_amd.light_visibility(tv, tf, leds, normals=tn)
    masked = brdf_amd.apply_visibility(shadowed.images, pm, vis.face_lit, level=0).images
    # (a) the per-face counts are the integers the twin predicts: the face's pixels times its lit lights
    means = brdf_amd.fit_capture_means(model, masked, *mesh, rv_mode=1, want_stats=False, **rule)
    assert np.array_equal(means.count.cpu().numpy(), np.repeat((face_pixels * lit_lights)[:, None], 3, axis=1))

    def worst(images):
        fit = brdf_amd.fit_capture_single_faces(model, images, *mesh, rv_mode=1, p0=(0.4, 0.4, 8.0), want_stats=False, **rule)
        assert (fit.ret >= 0).all()
        res = brdf_amd.capture_render_residuals(model, images, *mesh, np.tile(fit.single_brdf[None], (nf, 1, 1)), rv_mode=1, **rule)
        return int(res.abs_max.max())
    free, with_mask, without = worst(clean), worst(masked), worst(shadowed.images)
    print("largest abs_max: shadow-free", free, "masked", with_mask, "shadowed and unmasked", without)
    assert with_mask <= free + 1  # (b): one rounding of the quantiser
    assert without > with_mask    # (c): one model cannot serve both sides of a shadow edge
