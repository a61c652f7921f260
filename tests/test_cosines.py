"""Vectors -> cosines (brdfdata.cpp:799-943, LED table :683-752).

PARITY UNPINNED: the reference computes these with Eigen/OpenCV types that cannot be built here and holds no expected
values for them.  The CPU tests check the C restatement (oracle/cosines_oracle.c) against an independent numpy
restatement of the same formulas; the GPU tests check the HIP kernel against the C restatement, bit for bit (both perform
the same IEEE operations in the same order; the library is built with -ffp-contract=off)."""
import numpy as np
import pytest

from tests import oracle_libs as L


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def make_mesh(nv=500, nf=900, seed=7):
    rng = np.random.default_rng(seed)
    vertices = rng.uniform(-80.0, 80.0, size=(nv, 3)) + np.array([0.0, -80.0, 60.0])
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    e1 = vertices[faces[:, 1]] - vertices[faces[:, 0]]
    e2 = vertices[faces[:, 2]] - vertices[faces[:, 0]]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    view = np.array([310.0, -75.0, 700.0])
    return vertices, faces, nrm, view


def numpy_cosines(vertices, faces, nrm, leds, view, rv_mode):
    c = vertices[faces].sum(axis=1) / 3.0                       # [nf,3]
    def unit(v):
        return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))
    ld = unit(leds[None, :, :] - c[:, None, :])                 # [nf,L,3]
    cos_ln = (ld * nrm[:, None, :]).sum(-1)
    h = unit(leds[None, :, :] - 2 * c[:, None, :] + view[None, None, :])
    cos_nh = (h * nrm[:, None, :]).sum(-1)
    if rv_mode == 0:
        md = unit(c[:, None, 0:1] - leds[None, :, :])           # centroid x for all three components (brdfdata.cpp:835)
    else:
        md = unit(c[:, None, :] - leds[None, :, :])
    sf = (nrm[:, None, :] * md).sum(-1, keepdims=True)
    P = sf * nrm[:, None, :]
    R = md - 2 * P
    if rv_mode == 0:
        cos_rv = (R * P).sum(-1)                                # R.P (brdfdata.cpp:849)
    else:
        cos_rv = (R * unit(view[None, :] - c)[:, None, :]).sum(-1)
    return np.stack([cos_ln, cos_nh, cos_rv], axis=1)           # [nf,3,L]


def test_led_table_is_the_rig_of_the_reference():
    """InitLEDs, brdfdata.cpp:695-752: x = 303.5 for all; y/z on a 4 x 4 grid wired boustrophedon"""
    t = L.led_table()
    assert t.shape == (16, 3) and np.all(t[:, 0] == 303.5)
    y0, y1, z0, z1 = -157.1, -2.3, 555.3, 645.8
    assert t[0, 1] == y1 and t[0, 2] == z0 and t[3, 1] == y0 and t[4, 1] == y0 and t[7, 1] == y1
    assert t[12, 1] == y0 and t[15, 1] == y1 and t[15, 2] == z1 and t[12, 2] == z1
    assert np.allclose(np.unique(np.round(t[:, 2], 9)), np.round([z0, z0 + (z1 - z0) / 3, z1 - (z1 - z0) / 3, z1], 9))
    assert len({(round(a, 9), round(b, 9)) for a, b in t[:, 1:]}) == 16  # sixteen distinct positions


@pytest.mark.parametrize("rv_mode", [0, 1])
def test_c_restatement_against_numpy_restatement(rv_mode):
    vertices, faces, nrm, view = make_mesh()
    leds = L.led_table()
    got = L.cosines(vertices, faces, nrm, leds, view, rv_mode=rv_mode)
    want = numpy_cosines(vertices, faces, nrm, leds, view, rv_mode)
    assert got.shape == want.shape == (faces.shape[0], 3, 16)
    assert np.max(np.abs(got - want)) <= 4e-15  # numpy sums/divides in another order: a few ulp of values <= 1
    assert np.all(np.abs(got[:, :2, :]) <= 1.0 + 1e-15)  # plain cosines of unit vectors
    if rv_mode == 1:
        assert np.all(np.abs(got[:, 2, :]) <= 1.0 + 1e-15)


def test_surfel_indirection_and_ragged_batches():
    vertices, faces, nrm, view = make_mesh()
    leds = L.led_table()[:5]  # L need not be 16
    surfels = np.array([3, 3, 899, 0, 17], dtype=np.int32)  # repeated and unordered faces (a pixel map's entries)
    got = L.cosines(vertices, faces, nrm, leds, view, surfels=surfels)
    full = L.cosines(vertices, faces, nrm, leds, view)
    assert got.shape == (5, 3, 5) and np.array_equal(got, full[surfels])


@pytest.mark.gpu
@pytest.mark.parametrize("rv_mode", [0, 1])
def test_device_cosines_bit_exact(gpu, rv_mode):
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view = make_mesh(nv=4000, nf=30011, seed=11)
    leds = brdf_amd.led_table()
    assert np.array_equal(leds, L.led_table())
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    got = brdf_amd.cosines(tv, tf, tn, leds, view, rv_mode=rv_mode).cpu().numpy()
    want = L.cosines(vertices, faces, nrm, leds, view, rv_mode=rv_mode)
    assert np.array_equal(got, want)
    surfels = np.random.default_rng(5).integers(0, faces.shape[0], size=1001).astype(np.int32)
    got = brdf_amd.cosines(tv, tf, tn, leds[:7], view, surfels=torch.from_numpy(surfels).to(dev), rv_mode=rv_mode).cpu().numpy()
    assert np.array_equal(got, L.cosines(vertices, faces, nrm, leds[:7], view, surfels=surfels, rv_mode=rv_mode))


@pytest.mark.gpu
def test_cosines_feed_the_batched_fitter(gpu):
    """f1 -> the path: planes produced on the device go straight into brdf_hip_fit_batch_dev (n = 16 lights per
    surfel, the application's own size); the result equals fitting the oracle's planes."""
    torch, brdf_amd, dev = gpu
    from brdf_amd import synth
    vertices, faces, nrm, view = make_mesh(nv=300, nf=64, seed=3)
    # orient the normals towards the rig so that the cosines are positive (a lit, visible surfel)
    leds = brdf_amd.led_table()
    c = vertices[faces].sum(axis=1) / 3.0
    flip = ((leds.mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0
    nrm[flip] *= -1.0
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    angles = brdf_amd.cosines(tv, tf, tn, leds, view, rv_mode=1)
    ref_angles = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)
    assert np.array_equal(angles.cpu().numpy(), ref_angles)
    model, truth = 1, np.array(synth.TRUTH[1])
    x = np.stack([L.model_values(model, np.abs(a), truth) for a in ref_angles])
    pos = torch.abs(angles)
    p0 = torch.tensor(synth.P0[model], dtype=torch.float64, device=dev).repeat(angles.shape[0], 1)
    lb, ub = synth.bounds(model)
    p, info, ret = brdf_amd.fit_batch(1, model, pos, torch.from_numpy(x).to(dev), p0, lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    p, info, ret = p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
    # n = 16 fits are ill-conditioned (SURVEY.md section 6 ii): same bar as the other tiny-fit tests -- the device must
    # reach at least the objective the CPU restatement of levmar reaches from the same planes
    for s in range(angles.shape[0]):
        r, _, info_ref = L.brdf_fit("orc", 1, model, np.abs(ref_angles[s]), x[s], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
        assert ret[s] >= 0 or r < 0
        if r >= 0 and ret[s] >= 0:
            assert info[s, 1] <= info_ref[1] * (1 + 1e-3) + 1e-20


# ---- the capture loop (brdfdata.cpp:1188-1227) ------------------------------------
def make_capture(H=23, W=31, nf=40, seed=5):
    """a synthetic capture: a lit mesh, a pixel map with holes and with several pixels per face, and 16 8-bit BGR images
    rendered from per-face, per-channel Blinn-Phong truths through the cosines of the oracle"""
    from brdf_amd import synth
    vertices, faces, nrm, view = make_mesh(nv=200, nf=nf, seed=seed)
    leds = L.led_table()
    c = vertices[faces].sum(axis=1) / 3.0
    flip = ((leds.mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0
    nrm[flip] *= -1.0
    rng = np.random.default_rng(seed)
    pixel_map = rng.integers(-1, nf - 3, size=(H, W)).astype(np.int32)  # -1 = background; the last faces get no pixel
    pixel_map[rng.random((H, W)) < 0.3] = -1
    ang = np.abs(L.cosines(vertices, faces, nrm, leds, view, rv_mode=1))  # [nf,3,16]
    images = np.zeros((16, H, W, 3), dtype=np.uint8)
    truth = np.array(synth.TRUTH[1])
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f < 0:
                continue
            for ch in range(3):
                val = L.model_values(1, ang[f], truth * (0.6 + 0.2 * ch))
                images[:, H - 1 - y, x, ch] = np.clip(np.round(val * 255.0 * 0.5), 0, 255).astype(np.uint8)
    return vertices, faces, nrm, view, leds, pixel_map, images


def _objective(model, angles, x, p):
    e = x - L.model_values(model, angles, p)
    return float(e @ e)


def test_capture_oracle_walks_like_the_reference():
    """x outer / y inner, image row H-1-y, value/255, three channels per pixel, last pixel of a face wins"""
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture()
    surf, avg, npx = L.fit_capture(1, images, pixel_map, vertices, faces, nrm, leds, view, rv_mode=1, opts=(1e-3, 1e-15, 1e-15, 1e-20, 1e-6))
    assert npx == int((pixel_map > -1).sum())
    untouched = np.setdiff1d(np.arange(faces.shape[0]), np.unique(pixel_map[pixel_map > -1]))
    assert untouched.size > 0 and np.all(surf[untouched] == 0.0)
    ang = np.abs(L.cosines(vertices, faces, nrm, leds, view, rv_mode=1))
    H, W = pixel_map.shape
    f = int(pixel_map[pixel_map > -1][0])
    last = max((x, y) for y in range(H) for x in range(W) if pixel_map[y, x] == f)  # x-major order: the largest (x, y)
    x_, y_ = last
    for ch in range(3):
        I = images[:, H - 1 - y_, x_, ch] / 255.0
        _, p_ref, _ = L.brdf_fit("orc", 1, 1, L.cosines(vertices, faces, nrm, leds, view, surfels=[f], rv_mode=1)[0], I, (0.5, 1.0, 1.0),
                                 100, (1e-3, 1e-15, 1e-15, 1e-20, 1e-6), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0))
        assert np.array_equal(surf[f, ch], p_ref)
    assert np.all(np.isfinite(avg))


@pytest.mark.gpu
def test_device_capture_loop_against_oracle(gpu):
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture()
    opts = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
    want, avg_ref, npx_ref = L.fit_capture(1, images, pixel_map, vertices, faces, nrm, leds, view, rv_mode=1, opts=opts)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    got, avg, npx = brdf_amd.fit_capture(1, torch.from_numpy(images).to(dev), torch.from_numpy(pixel_map).to(dev), tv, tf, tn, leds, view,
                                         rv_mode=1, opts=opts)
    got = got.cpu().numpy()
    assert npx == npx_ref
    touched = np.unique(pixel_map[pixel_map > -1])
    untouched = np.setdiff1d(np.arange(faces.shape[0]), touched)
    assert np.all(got[untouched] == 0.0)
    # 16-sample fits are ill-conditioned (SURVEY.md section 6 ii): parity on the objective of the pixel that owns the face
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)
    H, W = pixel_map.shape
    errs = []
    for f in touched:
        x_, y_ = max((x, y) for y in range(H) for x in range(W) if pixel_map[y, x] == f)
        for ch in range(3):
            I = images[:, H - 1 - y_, x_, ch] / 255.0
            o_got, o_ref = _objective(1, ang[f], I, got[f, ch]), _objective(1, ang[f], I, want[f, ch])
            assert o_got <= o_ref * (1 + 1e-3) + 1e-12, (f, ch, got[f, ch], want[f, ch])
            errs.append(L.rel_err(got[f, ch], want[f, ch]))
    # the {kd, ks, n} written to brdf_surfaces themselves: the lane-per-fit kernel sums in the reference's order, so the fits
    # differ from the CPU walk only where a last-bit difference of exp/pow sends an ill-conditioned fit down another path
    errs = np.array(errs)
    print(f"capture: {np.mean(errs <= 1e-5):.3f} of {errs.size} (face, channel) fits within 1e-5 of the CPU walk, worst {errs.max():.2e}")
    assert np.mean(errs <= 1e-5) >= 0.9
    assert np.all(np.isfinite(avg)) and np.all(np.abs(avg - avg_ref) <= 0.05 * np.abs(avg_ref) + 1e-6)


@pytest.mark.gpu
def test_device_single_brdf_capture_against_oracle(gpu):
    """CalcBRDFEquation_SingleBRDF (brdfdata.cpp:1138-1186): one fit per channel over every visible face's 16 samples, with
    the reference's own call-site settings (p0 = 0, itmax = 2000, FD step 1).  n = 16 x faces is well conditioned, so
    the parameters themselves are compared."""
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture(H=40, W=50, nf=300, seed=9)
    want, info_ref, F_ref = L.fit_capture_single(1, images, pixel_map, vertices, faces, nrm, leds, view, rv_mode=1)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    got, info, F = brdf_amd.fit_capture_single(1, torch.from_numpy(images).to(dev), torch.from_numpy(pixel_map).to(dev), tv, tf, tn,
                                                leds, view, rv_mode=1)
    assert F == F_ref == np.unique(pixel_map[pixel_map > -1]).size
    for ch in range(3):
        assert L.rel_err(got[ch], want[ch]) <= 1e-5, (ch, got[ch], want[ch])
        assert abs(info[ch, 1] - info_ref[ch, 1]) <= 1e-8 * info_ref[ch, 1]


# ---- both cosines kernels at the light counts, surfel counts and centroids the tests above do not reach ---------------------
_BIG_MESH = []


def _big_mesh():
    """the mesh of test_device_cosines_bit_exact, built once"""
    if not _BIG_MESH:
        _BIG_MESH.append(make_mesh(nv=4000, nf=30011, seed=11))
    return _BIG_MESH[0]


def _device_cosines(gpu, mesh, leds, rv_mode, surfels=None):
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view = mesh
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    ts = None if surfels is None else torch.from_numpy(surfels).to(dev)
    return brdf_amd.cosines(tv, tf, tn, leds, view, surfels=ts, rv_mode=rv_mode).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("rv_mode", [0, 1])
def test_device_cosines_one_lane_per_light_kernel_at_16_lights(gpu, monkeypatch, rv_mode):
    """BRDF_HIP_COSINES_ROWS=0: cosines_kernel where the rows kernel runs by default -- the oracle's bits, and so the default's"""
    mesh = _big_mesh()
    vertices, faces, nrm, view = mesh
    leds = L.led_table()
    surfels = np.random.default_rng(5).integers(0, faces.shape[0], size=1001).astype(np.int32)
    want = L.cosines(vertices, faces, nrm, leds, view, rv_mode=rv_mode)
    want_s = L.cosines(vertices, faces, nrm, leds, view, surfels=surfels, rv_mode=rv_mode)
    rows, rows_s = _device_cosines(gpu, mesh, leds, rv_mode), _device_cosines(gpu, mesh, leds, rv_mode, surfels)
    monkeypatch.setenv("BRDF_HIP_COSINES_ROWS", "0")
    lanes, lanes_s = _device_cosines(gpu, mesh, leds, rv_mode), _device_cosines(gpu, mesh, leds, rv_mode, surfels)
    assert np.array_equal(lanes, want) and np.array_equal(lanes_s, want_s)
    assert lanes.tobytes() == rows.tobytes() and lanes_s.tobytes() == rows_s.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("lights", [1, 64])
@pytest.mark.parametrize("rv_mode", [0, 1])
def test_device_cosines_at_1_and_64_lights(gpu, rv_mode, lights):
    from tests.capture_problems import leds_for
    mesh = _big_mesh()
    vertices, faces, nrm, view = mesh
    leds = leds_for(lights)
    got = _device_cosines(gpu, mesh, leds, rv_mode)
    assert got.shape == (faces.shape[0], 3, lights) and np.array_equal(got, L.cosines(vertices, faces, nrm, leds, view, rv_mode=rv_mode))
    surfels = np.random.default_rng(6).integers(0, faces.shape[0], size=1001).astype(np.int32)
    assert np.array_equal(_device_cosines(gpu, mesh, leds, rv_mode, surfels), L.cosines(vertices, faces, nrm, leds, view, surfels=surfels, rv_mode=rv_mode))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["1", "0"])
def test_device_cosines_past_one_trip_of_the_grid(gpu, monkeypatch, rows):
    """262,144 + 53 surfels at 16 lights: 16,384 workgroups of 16 surfels and a second trip of the grid-stride loop, in both kernels"""
    mesh = _big_mesh()
    vertices, faces, nrm, view = mesh
    leds = L.led_table()
    surfels = np.random.default_rng(7).integers(0, faces.shape[0], size=262144 + 53).astype(np.int32)
    want = L.cosines(vertices, faces, nrm, leds, view, surfels=surfels, rv_mode=1)
    monkeypatch.setenv("BRDF_HIP_COSINES_ROWS", rows)
    got = _device_cosines(gpu, mesh, leds, 1, surfels)
    assert np.array_equal(got, want)
    assert np.array_equal(got[262144:], want[262144:]) and np.array_equal(got[-53:], L.cosines(vertices, faces, nrm, leds, view, surfels=surfels[-53:], rv_mode=1))


def zero_sum_mesh():
    """faces whose vertex sums are exactly 0.0 in one, two and three axes (small integers: every partial sum is exact), and one
    ordinary face; the centroid's zero components take the `t == 0` branch in front of the kernels' division by three"""
    vertices = np.array([[1.0, 2.0, 3.0], [2.0, -5.0, 1.0], [-3.0, 3.0, -4.0],     # face 0: sums (0, 0, 0)
                         [4.0, 1.0, 7.0], [-1.0, -3.0, 2.0], [-3.0, 2.0, 5.0],     # face 1: sums (0, 0, 14)
                         [6.0, -2.0, 1.0], [-2.0, 5.0, 9.0], [-4.0, 8.0, 3.0],     # face 2: sums (0, 11, 13)
                         [3.0, 7.0, -6.0], [5.0, -7.0, 2.0], [9.0, 4.0, 4.0],      # face 3: sums (17, 4, 0)
                         [8.0, 1.0, 2.0], [1.0, 6.0, -3.0], [2.0, 2.0, 5.0]])      # face 4: sums (11, 9, 4)
    faces = np.arange(15, dtype=np.int32).reshape(5, 3)
    nrm = np.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return vertices, faces, nrm, np.array([310.0, -75.0, 700.0])


def test_zero_sum_mesh_has_zero_centroid_components():
    vertices, faces, nrm, _ = zero_sum_mesh()
    sums = vertices[faces].sum(axis=1)
    assert [int((s == 0.0).sum()) for s in sums] == [3, 2, 1, 1, 0] and np.all(np.isfinite(nrm))
    for rv_mode in (0, 1):  # the oracle and the numpy restatement agree there too
        got = L.cosines(vertices, faces, nrm, L.led_table(), np.array([310.0, -75.0, 700.0]), rv_mode=rv_mode)
        assert np.max(np.abs(got - numpy_cosines(vertices, faces, nrm, L.led_table(), np.array([310.0, -75.0, 700.0]), rv_mode))) <= 4e-15


@pytest.mark.gpu
@pytest.mark.parametrize("rv_mode", [0, 1])
def test_device_cosines_with_zero_centroid_components(gpu, monkeypatch, rv_mode):
    mesh = zero_sum_mesh()
    vertices, faces, nrm, view = mesh
    surfels = np.array([0, 4, 1, 0, 2, 3, 3, 0], dtype=np.int32)
    for lights in (16, 5):
        leds = L.led_table()[:lights]
        for rows in ("1", "0"):
            monkeypatch.setenv("BRDF_HIP_COSINES_ROWS", rows)
            assert np.array_equal(_device_cosines(gpu, mesh, leds, rv_mode), L.cosines(vertices, faces, nrm, leds, view, rv_mode=rv_mode), equal_nan=True)
            assert np.array_equal(_device_cosines(gpu, mesh, leds, rv_mode, surfels),
                                  L.cosines(vertices, faces, nrm, leds, view, surfels=surfels, rv_mode=rv_mode), equal_nan=True)
