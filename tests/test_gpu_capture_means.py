"""The per-face capture over per-light means (brdf_hip_fit_capture_means_dev) on the 23 x 31, 40-face, 16-light fixture of
tests/test_gpu_capture_faces.py.

  1. objective: every carried (face, channel) is refused exactly where fewer than 3 lights have a sample, or its full-sample objective
     at the returned p is <= the oracle's grouped fit objective * (1 + 1e-3) + 1e-20 (the capture tests' bar);
  2. against the reference's weighted fit of capture_light_means' rows, on the bars of the sixteen-sample parity test;
  3. stats[0] = info[1] + within at the fitted p; covariance, sigma, rho, R2 against the weighted statistics yardstick with nobs = k,
     at P0 (a call with itmax = 0), where the yardstick can judge every fit;
  4. one pixel per face, rule off: the bytes of fit_capture_faces;
  5. two calls, L = 5, sentinel maps, an all-background map, a face of 300 pixels and 300 faces of one pixel."""
import numpy as np
import pytest

from tests import oracle_libs as L
from tests import stats_yardstick as Y
from tests import weighted_yardstick as WY
from tests.test_gpu_capture_faces import H, LB, LIGHTS, MODEL, NF, OPTS, P0, RULE, SENTINEL, UB, W, make_faces_capture

pytestmark = pytest.mark.gpu
MAPS = ("surfaces", "info", "ret", "count", "lights", "face_pixels", "covar", "stats", "rank")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


@pytest.fixture(scope="module")
def capture():
    return make_faces_capture()


@pytest.fixture(scope="module")
def masked_capture(capture):
    """every fifth touched face black, every fifth saturated: tests/test_gpu_capture_faces.py's masked fixture"""
    cap = dict(capture)
    images, pixel_map = capture["images"].copy(), capture["pixel_map"]
    touched = np.unique(pixel_map[pixel_map > -1])
    black, saturated = touched[0::5], touched[1::5]
    images[:, np.isin(pixel_map, black)[::-1], :] = 0       # image row H-1-y shows pixel-map row y
    images[:, np.isin(pixel_map, saturated)[::-1], :] = 255
    cap["images"] = images
    return cap


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sentinel_maps(gpu, nf=NF):
    torch, brdf_amd, dev = gpu

    def full(*shape, dtype=torch.float64):
        return torch.full((nf, *shape), SENTINEL, dtype=dtype, device=dev)
    return brdf_amd.CaptureMeans(full(3, 3), full(3, 10), full(3, dtype=torch.int32),
                                 brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=torch.int32)), full(3, dtype=torch.int32),
                                 full(3, dtype=torch.int32), full(dtype=torch.int32), None, 0, 0)


def _means(gpu, cap, images=None, pixel_map=None, leds=None, out=None, **kw):
    """fit_capture_means on the capture, everything on the host: a dict of numpy arrays"""
    torch, brdf_amd, _ = gpu
    images = cap["images"] if images is None else images
    pixel_map = cap["pixel_map"] if pixel_map is None else pixel_map
    leds = cap["leds"] if leds is None else leds
    r = brdf_amd.fit_capture_means(MODEL, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]),
                                   _dev(gpu, cap["nrm"]), leds, cap["view"], rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, out=out, **kw)
    torch.cuda.synchronize()
    return dict(surfaces=r.surfaces.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), covar=r.stats.covar.cpu().numpy(),
                stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy(), count=r.count.cpu().numpy(), lights=r.lights.cpu().numpy(),
                face_pixels=r.face_pixels.cpu().numpy(), avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)


@pytest.mark.parametrize("which", ["plain", "masked"])
def test_means_fits_reach_the_grouped_fits_objective(gpu, capture, masked_capture, which):
    torch, brdf_amd, _ = gpu
    cap = capture if which == "plain" else masked_capture
    a, x, off, fit_face, fit_channel, _ = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    m = brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    got = _means(gpu, cap, **RULE)
    judged = refused = 0
    worst = -np.inf
    for s, (f, ch) in enumerate(zip(fit_face, fit_channel)):
        k = int(off[s + 1] - off[s])
        assert got["count"][f, ch] == k == m.k[s] and got["lights"][f, ch] == m.counts[s], (f, ch)
        if m.counts[s] < 3:  # levmar's n < m refusal, on the lights
            assert got["ret"][f, ch] == -1 and np.array_equal(got["surfaces"][f, ch], P0) and not got["info"][f, ch].any() and got["rank"][f, ch] == 0
            refused += 1
            continue
        assert got["ret"][f, ch] >= 0, (f, ch)
        p = got["surfaces"][f, ch]
        assert np.all(np.isfinite(p)) and np.all(p >= np.array(LB)) and np.all(p <= np.array(UB)), (f, ch, k, p)
        a_v, x_v = np.ascontiguousarray(a[3 * off[s]:3 * off[s + 1]].reshape(3, k)), np.ascontiguousarray(x[off[s]:off[s + 1]])
        _, p_ref, _ = L.brdf_fit("orc", 1, MODEL, a_v, x_v, P0, 100, OPTS, LB, UB)
        e_got, e_ref = x_v - L.model_values(MODEL, a_v, p), x_v - L.model_values(MODEL, a_v, p_ref)
        o_got, o_ref = float(e_got @ e_got), float(e_ref @ e_ref)
        worst = max(worst, (o_got - o_ref) / o_ref)
        print(f"{which} face {f} channel {ch} count {k} lights {m.counts[s]}: objective {o_got:.6e} grouped oracle fit {o_ref:.6e}")
        assert o_got <= o_ref * (1 + 1e-3) + 1e-20, (f, ch, k, p, p_ref, o_got, o_ref)
        judged += 1
    print(f"{which}: judged {judged}, refused {refused}, largest relative excess over the grouped oracle fit {worst:.3e}")
    assert judged + refused == len(fit_face) == 3 * (NF - 3) and judged >= 1  # no carried (face, channel) was skipped
    if which == "masked":
        assert refused >= 1


def test_means_fits_against_the_references_weighted_fit_and_statistics(gpu, masked_capture):
    torch, brdf_amd, _ = gpu
    cap = masked_capture
    m = brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    got = _means(gpu, cap, **RULE)
    at = (m.fit_face, m.fit_channel)
    keep = m.counts >= 3
    fits = int(keep.sum())
    ret_ref, p_ref, info_ref = np.zeros(fits, dtype=np.int32), np.zeros((fits, 3)), np.zeros((fits, 10))
    for j, s in enumerate(np.flatnonzero(keep)):
        n = int(m.counts[s])
        ret_ref[j], p_ref[j], info_ref[j] = WY.weighted_fit(MODEL, m.angles[s][:, :n], m.x[s][:n], m.w[s][:n], P0, lb=LB, ub=UB, itmax=100, opts=OPTS)
    both, close, near, worst = WY.parity_figures(got["ret"][at][keep], got["surfaces"][at][keep], got["info"][at][keep], ret_ref, p_ref, info_ref)
    print(f"means capture against the reference's weighted fit: {both}/{fits} converge on both sides, {close}/{both} of them within 1e-5 on p, "
          f"{near}/{fits} objectives within 1e-6, worst objective excess {worst:.3e}")
    assert close >= 0.97 * both and near >= 0.99 * fits and worst <= 0.3, (both, close, near, worst)
    # at the fitted p: stats[0] = info[1] + within
    stats, info = got["stats"][at], got["info"][at]
    want0 = info[keep, 1] + m.within[keep]
    assert np.all(np.abs(stats[keep, 0] - want0) <= Y.E_TOL * want0), np.max(np.abs(stats[keep, 0] - want0) / want0)


@pytest.mark.parametrize("which", ["plain", "masked"])
def test_means_capture_statistics_against_the_yardstick(gpu, capture, masked_capture, which):
    """The statistics maps against the yardstick of the weighted statistics test (tests/weighted_yardstick.py: the reference's
    dlevmar_covar on J^T W J with nobs = k, sumsq and SStot with `within`; covar_bound, E_TOL, max_left_out = 0.35).  They are taken
    at P0: a call with itmax = 0 leaves p = p0 and runs the same statistics pass.  At the FITTED points the yardstick can judge few of
    this fixture's fits -- all pixels of a face share 16 cosine triples and the truth has n = 24: cond(J^T W J) <= 1e8 on 18 of the
    masked capture's 63 -- while at P0 it judges every one (111 of 111 and 63 of 63, largest cond about 1e6), so every covariance the
    capture writes is held to the bound."""
    torch, brdf_amd, _ = gpu
    cap = capture if which == "plain" else masked_capture
    m = brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    got = _means(gpu, cap, itmax=0, **RULE)
    at = (m.fit_face, m.fit_channel)
    idx = np.flatnonzero(m.counts >= 3)
    assert idx.size >= 60 and np.all(got["surfaces"][at][idx] == np.array(P0)) and np.all(got["ret"][at][idx] >= 0)
    stats, info = got["stats"][at], got["info"][at]
    want0 = info[idx, 1] + m.within[idx]
    assert np.all(np.abs(stats[idx, 0] - want0) <= Y.E_TOL * want0), np.max(np.abs(stats[idx, 0] - want0) / want0)
    _, compared, S = WY.compare_weighted_stats(Y.FORWARD, MODEL, m.angles[idx], m.x[idx], m.w[idx], got["surfaces"][at][idx], got["covar"][at][idx],
                                               stats[idx], got["rank"][at][idx], counts=m.counts[idx], nobs=m.k[idx], extra_ss=m.within[idx],
                                               max_left_out=0.35, label=f"means capture, {which}, at P0")
    assert compared == S, (compared, S)  # the yardstick judges every fit at P0


def test_one_pixel_per_face_is_the_faces_capture(gpu, capture):
    torch, brdf_amd, _ = gpu
    pixel_map = np.full((H, W), -1, dtype=np.int32)
    flat = pixel_map.reshape(-1)
    for f in range(NF - 3):  # the map of test_one_pixel_per_face_is_the_last_pixel_capture
        flat[np.flatnonzero(capture["pixel_map"].reshape(-1) == f)[0]] = f
    r = brdf_amd.fit_capture_faces(MODEL, _dev(gpu, capture["images"]), _dev(gpu, pixel_map), _dev(gpu, capture["vertices"]), _dev(gpu, capture["faces"]),
                                   _dev(gpu, capture["nrm"]), capture["leds"], capture["view"], rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS)
    torch.cuda.synchronize()
    want = dict(surfaces=r.surfaces, info=r.info, ret=r.ret, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank, count=r.count,
                face_pixels=r.face_pixels)
    got = _means(gpu, capture, pixel_map=pixel_map)  # the rule switched off: weights 1, means v / 255, within 0, k = 16
    for name, t in want.items():
        assert got[name].tobytes() == t.cpu().numpy().tobytes(), name
    assert np.all(got["count"][:NF - 3] == LIGHTS) and np.all(got["lights"][:NF - 3] == LIGHTS) and (got["ret"][:NF - 3] >= 0).any()
    assert got["avg"].tobytes() == r.avg.tobytes() and (got["n_pixels"], got["n_faces"]) == (r.n_pixels, r.n_faces)


def test_nothing_but_the_definition_shows(gpu, capture):
    torch, brdf_amd, _ = gpu
    first = _means(gpu, capture, out=_sentinel_maps(gpu), **RULE)
    again = _means(gpu, capture, out=_sentinel_maps(gpu), **RULE)
    for name in MAPS + ("avg",):
        assert again[name].tobytes() == first[name].tobytes(), name
    untouched = np.arange(NF - 3, NF)  # faces no pixel carries keep the sentinel
    for name in MAPS:
        if name != "face_pixels":
            assert np.all(first[name][untouched] == SENTINEL) and not np.all(first[name][:NF - 3] == SENTINEL), name
    assert np.all(first["face_pixels"][untouched] == 0) and first["n_faces"] == NF - 3
    carried = np.arange(NF - 3)
    ref = first["surfaces"][carried].reshape(-1, 3).sum(axis=0) / (NF * 3)
    assert np.all(np.abs(first["avg"] - ref) <= 1e-12 * np.abs(ref)), (first["avg"], ref)
    # L = 5: counts and lights against the NumPy twin on the first five images
    five = _means(gpu, capture, images=capture["images"][:5], leds=capture["leds"][:5], **RULE)
    ang5 = L.cosines(capture["vertices"], capture["faces"], capture["nrm"], capture["leds"][:5], capture["view"], rv_mode=1)
    m5 = brdf_amd.capture_light_means(capture["images"][:5], capture["pixel_map"], ang5, MODEL, **RULE)
    at = (m5.fit_face, m5.fit_channel)
    assert np.array_equal(five["count"][at], m5.k) and np.array_equal(five["lights"][at], m5.counts) and m5.counts.max() <= 5
    ok = m5.counts >= 3
    assert ok.any() and np.all(five["ret"][at][~ok] == -1) and np.all(five["ret"][at][ok] >= 0)
    st = five["stats"][at][ok, 0]
    want0 = five["info"][at][ok, 1] + m5.within[ok]
    assert np.all(np.abs(st - want0) <= Y.E_TOL * want0)
    # an all-background map: returns 0 with zeros, writes nothing but the pixel counts
    empty = _means(gpu, capture, pixel_map=np.full((H, W), -1, dtype=np.int32), out=_sentinel_maps(gpu), **RULE)
    assert empty["n_pixels"] == empty["n_faces"] == 0 and not empty["avg"].any() and not empty["face_pixels"].any()
    for name in MAPS:
        if name != "face_pixels":
            assert np.all(empty[name] == SENTINEL), name


def test_one_big_face_and_many_small_faces_accumulate_alike(gpu, capture):
    """a face of 300 pixels (several workgroups add to the same words) and 300 faces of one pixel (a workgroup's words belong to 16
    faces): the accumulators, as the count map shows them, are the NumPy twin's"""
    torch, brdf_amd, _ = gpu
    from tests.test_cosines import make_mesh
    big = capture["class_faces"][0]
    m = brdf_amd.capture_light_means(capture["images"], capture["pixel_map"], capture["ang"], MODEL, **RULE)
    got = _means(gpu, capture, **RULE)
    rows = np.flatnonzero(m.fit_face == big)
    assert int((capture["pixel_map"] == big).sum()) == 300 and np.array_equal(got["count"][big], m.k[rows]) and m.k[rows].min() > 16 * 200
    # 300 faces of one pixel each: a mesh of 320 faces, the fixture's images
    nf = 320
    vertices, faces, nrm, view = make_mesh(nv=400, nf=nf, seed=9)
    pixel_map = np.full((H, W), -1, dtype=np.int32)
    where = np.random.default_rng(3).permutation(H * W)[:300]
    pixel_map.reshape(-1)[where] = np.arange(300)
    ang = L.cosines(vertices, faces, nrm, capture["leds"], view, rv_mode=1)
    m1 = brdf_amd.capture_light_means(capture["images"], pixel_map, ang, MODEL, **RULE)
    r = brdf_amd.fit_capture_means(MODEL, _dev(gpu, capture["images"]), _dev(gpu, pixel_map), _dev(gpu, vertices), _dev(gpu, faces), _dev(gpu, nrm),
                                   capture["leds"], view, rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, **RULE)
    torch.cuda.synchronize()
    at = (m1.fit_face, m1.fit_channel)
    assert r.n_faces == 300 and r.n_pixels == 300
    assert np.array_equal(r.count.cpu().numpy()[at], m1.k) and np.array_equal(r.lights.cpu().numpy()[at], m1.counts) and np.array_equal(m1.k, m1.counts)
    assert np.array_equal(r.face_pixels.cpu().numpy(), m1.face_pixels)
