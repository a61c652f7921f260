"""The per-light-means capture with sigma-clipped fits (brdf_hip_fit_capture_means_clipped_dev).

  (a) rounds = 0, and kappa = inf with rounds = 3: fit_capture_means' bytes in all of its maps, avg and the scalars -- every model, the
      rule on and off; kept == count, rounds == 0, the interval maps are the initial intervals;
  (b) rounds = 2, kappa = 2.5 on the brightened rule_capture: every output has the bytes of a host-driven replay of the definition --
      fit_batch_weighted and fit_stats_batch_weighted(extra_ss=, nobs=) on the device, brdf_amd.clip_light_means on the host, only the
      active fits refitted; a fit is left out where the twin finds a grey level within 1e-9 sigma of the threshold, at most 2 % of them;
  (c) one pixel per face, the rule off, a few single lights brightened: the bytes of fit_capture_faces_clipped;
  (d) the invariant: LightMeans rebuilt on the host under the returned intervals give the returned statistics' bytes, kept and lights;
  (e) shapes: a face of 300 pixels, 300 one-pixel faces, L = 5, an all-background map, a clip that would leave two lights, two calls;
  (f) the clip loop of the definition around the compiled reference's weighted dlevmar_bc_dif, and its +-1 ulp twin."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import capture_problems as P
from tests import oracle_libs as L
from tests import stats_yardstick as Y
from tests import weighted_yardstick as WY

pytestmark = pytest.mark.gpu
OPTS, P0, LB, UB, RULE = P.OPTS, P.P0, P.LB, P.UB, P.RULE
OFF = dict(v_min=0, v_max=255, cos_min=-2.0)
SENTINEL = -7
SIGMA_MIN = 1.0 / (255.0 * np.sqrt(12.0))
KAPPA, ROUNDS = 2.5, 2
MEANS_MAPS = ("surfaces", "info", "ret", "count", "lights", "face_pixels", "covar", "stats", "rank")
CLIP_MAPS = MEANS_MAPS + ("kept", "rounds", "vlo", "vhi")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _on_device(gpu, cap, images=None, pixel_map=None, leds=None):
    return (_dev(gpu, cap["images"] if images is None else images), _dev(gpu, cap["pixel_map"] if pixel_map is None else pixel_map),
            _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]), _dev(gpu, cap["nrm"]), cap["leds"] if leds is None else leds, cap["view"])


def _numpy(r, clipped):
    got = dict(surfaces=r.surfaces.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), count=r.count.cpu().numpy(),
               lights=r.lights.cpu().numpy(), face_pixels=r.face_pixels.cpu().numpy(), covar=r.stats.covar.cpu().numpy(),
               stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy(), avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)
    if clipped:
        got.update(kept=r.kept.cpu().numpy(), rounds=r.rounds.cpu().numpy(), vlo=r.vlo.cpu().numpy(), vhi=r.vhi.cpu().numpy())
    return got


def _means(gpu, cap, model, images=None, pixel_map=None, **kw):
    torch, brdf_amd, _ = gpu
    r = brdf_amd.fit_capture_means(model, *_on_device(gpu, cap, images, pixel_map), rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, **kw)
    torch.cuda.synchronize()
    return _numpy(r, False)


def _sentinel_maps(gpu, nf, lights):
    torch, brdf_amd, dev = gpu

    def full(*shape, dtype=torch.float64):
        return torch.full((nf, *shape), SENTINEL, dtype=dtype, device=dev)
    i32 = torch.int32
    u8 = lambda: torch.full((nf, 3, lights), 249, dtype=torch.uint8, device=dev)  # noqa: E731 (uint8's sentinel)
    return brdf_amd.CaptureMeansClipped(full(3, 3), full(3, 10), full(3, dtype=i32), brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=i32)),
                                        full(3, dtype=i32), full(3, dtype=i32), full(dtype=i32), None, 0, 0, full(3, dtype=i32), full(3, dtype=i32), u8(), u8())


def _clipped(gpu, cap, model, rounds, images=None, pixel_map=None, leds=None, kappa=KAPPA, sentinel=False, p0=P0, **kw):
    torch, brdf_amd, _ = gpu
    args = _on_device(gpu, cap, images, pixel_map, leds)
    out = _sentinel_maps(gpu, cap["faces"].shape[0], args[0].shape[0]) if sentinel else None
    r = brdf_amd.fit_capture_means_clipped(model, *args, kappa=kappa, sigma_min=SIGMA_MIN, rounds=rounds, rv_mode=1, p0=p0, lb=LB, ub=UB, opts=OPTS,
                                           out=out, **kw)
    torch.cuda.synchronize()
    return _numpy(r, True)


def _same(got, want, names, rows=None):
    for name in names:
        g, w = got[name], want[name]
        if rows is not None and name != "face_pixels":
            g, w = g[rows], w[rows]
        assert g.dtype == w.dtype and g.shape == w.shape and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), name


@functools.lru_cache(maxsize=None)
def brightened(model):
    from tests.test_gpu_capture_faces_clipped import _brightened
    cap = P.rule_capture(model)
    images, big = _brightened(cap, model)
    return cap, images, big


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [RULE, OFF], ids=["rule", "off"])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_no_rounds_and_an_infinite_kappa_are_the_means_capture(gpu, model, rule):
    _, brdf_amd, _ = gpu
    cap = P.rule_capture(model)
    want = _means(gpu, cap, model, **rule)
    carried = np.flatnonzero(want["face_pixels"])
    fit_face = np.repeat(carried, 3)
    lo, hi = brdf_amd.initial_light_intervals(cap["ang"], fit_face, model, **rule)
    for rounds, kappa in ((0, KAPPA), (3, np.inf)):
        got = _clipped(gpu, cap, model, rounds, kappa=kappa, **rule)
        _same(got, want, MEANS_MAPS + ("avg",))
        assert (got["n_pixels"], got["n_faces"]) == (want["n_pixels"], want["n_faces"]) and got["n_faces"] == 37
        assert np.array_equal(got["kept"], got["count"]) and not got["rounds"].any()
        assert np.array_equal(got["vlo"][carried].reshape(-1, 16), lo) and np.array_equal(got["vhi"][carried].reshape(-1, 16), hi)
        rest = np.setdiff1d(np.arange(cap["nf"]), carried)
        assert not got["vlo"][rest].any() and not got["vhi"][rest].any()
        assert brdf_amd.last_clip_stats() == ([] if rounds == 0 else [dict(active=0, clipped=0)])


# ---- (b): the replay ---------------------------------------------------------------------------------------------------------------
def device_fit(gpu, model):
    torch, brdf_amd, _ = gpu

    def fit(lm, rows, p):
        pd, info, ret = brdf_amd.fit_batch_weighted(brdf_amd.METHOD_BC_DIF, model, _dev(gpu, np.nan_to_num(lm.angles[rows])), _dev(gpu, np.nan_to_num(lm.x[rows])),
                                                    _dev(gpu, np.nan_to_num(lm.w[rows])), _dev(gpu, p[rows]), lb=LB, ub=UB, itmax=100, opts=OPTS,
                                                    counts=_dev(gpu, lm.counts[rows].astype(np.int32)))
        torch.cuda.synchronize()
        return pd.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
    return fit


def device_stats(gpu, model):
    torch, brdf_amd, _ = gpu

    def stats(lm, p):
        st = brdf_amd.fit_stats_batch_weighted(brdf_amd.METHOD_BC_DIF, model, _dev(gpu, np.nan_to_num(lm.angles)), _dev(gpu, np.nan_to_num(lm.x)),
                                               _dev(gpu, np.nan_to_num(lm.w)), _dev(gpu, p), opts=OPTS, counts=_dev(gpu, lm.counts.astype(np.int32)),
                                               extra_ss=_dev(gpu, lm.within), nobs=_dev(gpu, lm.k.astype(np.int32)))
        torch.cuda.synchronize()
        return st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()
    return stats


def replay(cap, images, model, rule, fit, stats, kappa=KAPPA, rounds=ROUNDS, sigma_min=SIGMA_MIN):
    """the definition, round by round: `fit` and `stats` on the weighted rows, brdf_amd.clip_light_means on the host; only the active
    fits are refitted.  -> (the outputs by fit, the fits a grey level of which the twin found within 1e-9 sigma of its threshold)"""
    import brdf_amd
    from brdf_amd import synth
    pm, ang = cap["pixel_map"], cap["ang"]
    lm = brdf_amd.capture_light_means(images, pm, ang, model, **rule)
    S = len(lm.k)
    count = lm.k.copy()
    lo, hi = brdf_amd.initial_light_intervals(ang, lm.fit_face, model, **rule)
    p, info, ret = fit(lm, np.arange(S), np.tile(np.array(P0), (S, 1)))
    settled, used, near = np.zeros(S, dtype=bool), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=bool)
    grey = np.arange(256)
    for r in range(1, rounds + 1):
        covar, st, rank = stats(lm, p)
        nlo, nhi, done = brdf_amd.clip_light_means(images, pm, ang, model, p, st[:, 0], ret, lo, hi, kappa=kappa, sigma_min=sigma_min, **rule)
        for s in np.flatnonzero(~settled):
            k = int(lm.k[s])
            if ret[s] >= 0 and lm.counts[s] >= 3 and np.isfinite(st[s, 0]):
                sigma = max(np.sqrt(st[s, 0] / (k - 3)), sigma_min) if k > 3 else sigma_min
                a = ang[lm.fit_face[s]]
                with np.errstate(all="ignore"):
                    e = np.abs(grey[None, :] / 255.0 - synth.model_value(model, p[s], a[0], a[1], a[2])[:, None])  # [L,256]
                inside = (grey[None, :] >= lo[s].astype(int)[:, None]) & (grey[None, :] <= hi[s].astype(int)[:, None])
                near[s] |= bool((np.abs(e - kappa * sigma)[inside] < 1e-9 * sigma).any())
        active = ~settled & ~done
        settled |= done
        if not active.any():
            break
        lo[active], hi[active] = nlo[active], nhi[active]
        lm = brdf_amd.capture_light_means(images, pm, ang, model, v_lo=lo, v_hi=hi, **rule)
        rows = np.flatnonzero(active)
        p[rows], info[rows], ret[rows] = fit(lm, rows, p)
        used[rows] = r
    covar, st, rank = stats(lm, p)
    return dict(p=p, info=info, ret=ret, covar=covar, stats=st, rank=rank, count=count, kept=lm.k, lights=lm.counts, rounds=used, vlo=lo, vhi=hi,
                fit_face=lm.fit_face, fit_channel=lm.fit_channel, face_pixels=lm.face_pixels), near


def expected_maps(want, nf, lights):
    """the replay's outputs scattered by (face, channel) into sentinel maps"""
    at = (want["fit_face"], want["fit_channel"])
    out = dict(surfaces=np.full((nf, 3, 3), SENTINEL, dtype=np.float64), info=np.full((nf, 3, 10), SENTINEL, dtype=np.float64),
               covar=np.full((nf, 3, 3, 3), SENTINEL, dtype=np.float64), stats=np.full((nf, 3, 8), SENTINEL, dtype=np.float64),
               vlo=np.full((nf, 3, lights), 249, dtype=np.uint8), vhi=np.full((nf, 3, lights), 249, dtype=np.uint8), face_pixels=want["face_pixels"])
    for name in ("ret", "count", "lights", "rank", "kept", "rounds"):
        out[name] = np.full((nf, 3), SENTINEL, dtype=np.int32)
    for name, src in (("surfaces", "p"), ("info", "info"), ("ret", "ret"), ("covar", "covar"), ("stats", "stats"), ("rank", "rank"), ("count", "count"),
                      ("lights", "lights"), ("kept", "kept"), ("rounds", "rounds"), ("vlo", "vlo"), ("vhi", "vhi")):
        out[name][at] = want[src]
    return out


@pytest.mark.parametrize("model", [0, 1, 2])
def test_replay_of_the_definition(gpu, model):
    """Left out on the MI355X and, with the compiled reference's weighted fit in place of the device's, on the CPU: see DESIGN.md,
    "Sigma-clipped fits in the means capture"."""
    _, brdf_amd, _ = gpu
    cap, images, big = brightened(model)
    nf = cap["nf"]
    want, near = replay(cap, images, model, RULE, device_fit(gpu, model), device_stats(gpu, model))
    S = len(near)
    got = _clipped(gpu, cap, model, ROUNDS, images=images, sentinel=True, **RULE)
    rec = brdf_amd.last_clip_stats()
    print(f"model {model}: kept {int(want['kept'].sum())} of {int(want['count'].sum())} samples, rounds {np.bincount(want['rounds'], minlength=3)}, "
          f"left out {int(near.sum())} of {S} fits; the call's rounds {rec}")
    assert near.sum() <= 0.02 * S, np.flatnonzero(near)  # the cap: change the fixture, not the cap
    exp = expected_maps(want, nf, 16)
    for s in np.flatnonzero(near):  # a fit that is left out: whatever the entry returned
        at = (want["fit_face"][s], want["fit_channel"][s])
        for name in CLIP_MAPS:
            if name != "face_pixels":
                exp[name][at] = got[name][at]
    _same(got, exp, CLIP_MAPS)
    carried = np.unique(want["fit_face"])
    assert np.all(got["kept"][carried] <= got["count"][carried]) and np.all(got["rounds"][carried] <= ROUNDS)
    assert any((got["kept"][f] < got["count"][f]).any() for f in big), (big, got["kept"][big], got["count"][big])
    untouched = np.setdiff1d(np.arange(nf), carried)
    assert untouched.size >= 3 and np.all(got["kept"][untouched] == SENTINEL) and np.all(got["vhi"][untouched] == 249)
    # the faces the rule leaves fewer than 3 lights: refused, with fit_capture_means' outputs
    few = got["lights"][carried] < 3
    assert few.any()
    assert np.all(got["ret"][carried][few] == -1) and np.all(got["kept"][carried][few] == got["count"][carried][few]) and not got["rounds"][carried][few].any()
    assert np.all(got["surfaces"][carried][few] == np.array(P0))
    plain = _means(gpu, cap, model, images=images, **RULE)
    for name in MEANS_MAPS:
        if name != "face_pixels":
            assert np.array_equal(got[name][carried][few], plain[name][carried][few], equal_nan=True), name
    # the per-round record of the call
    assert 1 <= len(rec) <= ROUNDS and rec[0]["active"] == int((got["rounds"][carried] >= 1).sum())
    assert sum(r["clipped"] for r in rec) == int((got["count"][carried] - got["kept"][carried]).sum())


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def check_invariant(gpu, got, images, pixel_map, ang, model, rule):
    """the returned statistics, kept and lights are those of the rows rebuilt on the host under the returned intervals, at the returned p"""
    _, brdf_amd, _ = gpu
    plain = brdf_amd.capture_light_means(images, pixel_map, ang, model, **rule)
    at = (plain.fit_face, plain.fit_channel)
    lm = brdf_amd.capture_light_means(images, pixel_map, ang, model, v_lo=got["vlo"][at], v_hi=got["vhi"][at], **rule)
    assert np.array_equal(got["count"][at], plain.k) and np.array_equal(got["kept"][at], lm.k) and np.array_equal(got["lights"][at], lm.counts)
    assert np.all(lm.k <= plain.k) and np.all(got["vlo"][at][got["rounds"][at] == 0] == brdf_amd.initial_light_intervals(ang, plain.fit_face, model, **rule)[0][got["rounds"][at] == 0])
    if ang.shape[2] >= 3:
        covar, stats, rank = device_stats(gpu, model)(lm, np.ascontiguousarray(got["surfaces"][at]))
        assert covar.tobytes() == np.ascontiguousarray(got["covar"][at]).tobytes() and stats.tobytes() == np.ascontiguousarray(got["stats"][at]).tobytes()
        assert rank.tobytes() == np.ascontiguousarray(got["rank"][at]).tobytes()
    return plain, lm


@pytest.mark.parametrize("model", [0, 1, 2])
def test_returned_statistics_are_those_of_the_returned_intervals(gpu, model):
    cap, images, big = brightened(model)
    got = _clipped(gpu, cap, model, ROUNDS, images=images, **RULE)
    plain, lm = check_invariant(gpu, got, images, cap["pixel_map"], cap["ang"], model, RULE)
    assert (lm.k < plain.k).sum() >= 2
    again = _clipped(gpu, cap, model, ROUNDS, images=images, **RULE)  # two calls return the same bytes
    _same(again, got, CLIP_MAPS + ("avg",))


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_one_pixel_per_face_is_the_clipped_faces_capture(gpu):
    from tests.test_gpu_capture_faces import H, MODEL, NF, W, make_faces_capture
    torch, brdf_amd, _ = gpu
    cap = make_faces_capture()
    pixel_map = np.full((H, W), -1, dtype=np.int32)
    flat = pixel_map.reshape(-1)
    images = cap["images"].copy()
    for f in range(NF - 3):  # the map of test_one_pixel_per_face_is_the_faces_capture
        g = np.flatnonzero(cap["pixel_map"].reshape(-1) == f)[0]
        flat[g] = f
        if f % 3 == 0:  # a single light brightened: the light drops out and the rows compact
            y, x = divmod(g, W)
            i = (5 * f) % 16
            images[i, H - 1 - y, x, :] = np.minimum(images[i, H - 1 - y, x, :].astype(int) + 90, 255).astype(np.uint8)
    r = brdf_amd.fit_capture_faces_clipped(MODEL, *_on_device(gpu, cap, images, pixel_map), kappa=KAPPA, sigma_min=SIGMA_MIN, rounds=2, rv_mode=1, p0=P0,
                                           lb=LB, ub=UB, opts=OPTS)
    torch.cuda.synchronize()
    want = dict(surfaces=r.surfaces, info=r.info, ret=r.ret, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank, count=r.count, kept=r.kept,
                rounds=r.rounds)
    got = _clipped(gpu, cap, MODEL, 2, images=images, pixel_map=pixel_map)  # the rule off: weights 1, means v / 255, within exactly 0
    for name, t in want.items():
        assert got[name].tobytes() == t.cpu().numpy().tobytes(), name
    assert (got["lights"][:NF - 3] < 16).any() and (got["rounds"][:NF - 3] > 0).any() and np.array_equal(got["lights"][:NF - 3], got["kept"][:NF - 3])
    assert got["avg"].tobytes() == r.avg.tobytes()


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
def test_shapes(gpu):
    from tests.test_cosines import make_mesh
    from tests.test_gpu_capture_faces import H, MODEL, W, make_faces_capture
    torch, brdf_amd, _ = gpu
    cap = make_faces_capture()
    pm = cap["pixel_map"]
    # a face of 300 pixels with a brightened patch: several workgroups add to the same words under intervals
    big = cap["class_faces"][0]
    images = cap["images"].copy()
    ys, xs = np.nonzero(pm == big)
    assert ys.size == 300
    for i in range(0, 16, 2):
        images[i, H - 1 - ys[::12], xs[::12], :] = np.minimum(images[i, H - 1 - ys[::12], xs[::12], :].astype(int) + 60, 255).astype(np.uint8)
    got = _clipped(gpu, cap, MODEL, 2, images=images, sentinel=True, **RULE)
    check_invariant(gpu, got, images, pm, cap["ang"], MODEL, RULE)
    assert np.all(got["kept"][big] < got["count"][big]) and got["count"][big].min() > 16 * 200 and np.all(got["rounds"][big] >= 1)
    assert np.all(got["kept"][37:] == SENTINEL) and np.all(got["vlo"][37:] == 249)
    # L = 5
    ang5 = L.cosines(cap["vertices"], cap["faces"], cap["nrm"], cap["leds"][:5], cap["view"], rv_mode=1)
    five = _clipped(gpu, cap, MODEL, 2, images=images[:5], leds=cap["leds"][:5], **RULE)
    assert five["vlo"].shape == (cap["faces"].shape[0], 3, 5)
    check_invariant(gpu, five, images[:5], pm, ang5, MODEL, RULE)
    assert np.all(five["kept"][big] < five["count"][big])
    # 300 faces of one pixel each, some of them with one light brightened: a mesh of 320 faces, the fixture's images
    nf = 320
    vertices, faces, nrm, view = make_mesh(nv=400, nf=nf, seed=9)
    one = np.full((H, W), -1, dtype=np.int32)
    where = np.random.default_rng(3).permutation(H * W)[:300]
    one.reshape(-1)[where] = np.arange(300)
    images1 = cap["images"].copy()
    for j, g in enumerate(where[::4]):
        y, x = divmod(int(g), W)
        images1[j % 16, H - 1 - y, x, :] = np.minimum(images1[j % 16, H - 1 - y, x, :].astype(int) + 90, 254).astype(np.uint8)
    ang = L.cosines(vertices, faces, nrm, cap["leds"], view, rv_mode=1)
    mesh = dict(vertices=vertices, faces=faces, nrm=nrm, leds=cap["leds"], view=view)
    ones = _clipped(gpu, mesh, MODEL, 2, images=images1, pixel_map=one, **RULE)
    assert ones["n_faces"] == 300 and ones["n_pixels"] == 300
    check_invariant(gpu, ones, images1, one, ang, MODEL, RULE)
    assert (ones["kept"] < ones["count"]).any()
    # an all-background map writes nothing but the pixel counts
    empty = _clipped(gpu, cap, MODEL, 2, pixel_map=np.full((H, W), -1, dtype=np.int32), sentinel=True, **RULE)
    assert empty["n_pixels"] == empty["n_faces"] == 0 and not empty["avg"].any() and not empty["face_pixels"].any()
    for name in CLIP_MAPS:
        if name != "face_pixels":
            assert np.all(empty[name] == (249 if name in ("vlo", "vhi") else SENTINEL)), name


def test_a_clip_that_would_leave_two_lights_is_not_applied(gpu):
    """by hand: three lights carry a face's samples and all of one light's samples are far off.  At itmax = 0 the fit stays at p0, the
    other two lights show the model's own values there: the round would drop the third light whole, and is not applied"""
    from brdf_amd import synth
    from tests.test_gpu_capture_faces import H, MODEL, make_faces_capture
    _, brdf_amd, _ = gpu
    cap = make_faces_capture()
    pm = cap["pixel_map"]
    f = cap["class_faces"][2]  # 40 pixels, lit by every light
    p0 = (0.3, 0.1, 2.0)
    rule = dict(v_min=1, v_max=254, cos_min=-2.0)
    ys, xs = np.nonzero(pm == f)
    images = cap["images"].copy()
    images[:, H - 1 - ys, xs, :] = 0  # below v_min: no samples under the other thirteen lights
    a = cap["ang"][f]
    base = np.round(255.0 * synth.model_value(MODEL, np.array(p0), a[0], a[1], a[2])).astype(int)
    assert np.all((base[:3] > 5) & (base[:3] < 150)), base[:3]
    for i in range(3):
        images[i, H - 1 - ys, xs, :] = (base[i] + (np.arange(ys.size) % 3 - 1) + (100 if i == 1 else 0))[:, None]
    got = _clipped(gpu, cap, MODEL, 2, images=images, kappa=1.0, p0=p0, itmax=0, **rule)
    lo, hi = brdf_amd.initial_light_intervals(cap["ang"], [f], MODEL, **rule)
    assert np.all(got["lights"][f] == 3) and np.all(got["count"][f] == 120) and np.all(got["kept"][f] == 120) and not got["rounds"][f].any()
    assert np.array_equal(got["vlo"][f], np.tile(lo, (3, 1))) and np.array_equal(got["vhi"][f], np.tile(hi, (3, 1)))
    # with two far-off pixels instead of the whole light the clip stands
    images[1, H - 1 - ys[2:], xs[2:], :] -= 100
    got = _clipped(gpu, cap, MODEL, 2, images=images, kappa=2.0, p0=p0, itmax=0, **rule)
    assert np.all(got["kept"][f] == 118) and np.all(got["rounds"][f] == 1) and np.all(got["vhi"][f][:, 1] < base[1] + 99)


# ---- (f) -------------------------------------------------------------------------------------------------------------------------
def _reference_weighted_fit(model, angles, x, w, p0, sign):
    """tests.weighted_yardstick.weighted_fit with every model value moved by sign ulp (sign [n], or None)"""
    a, xx = L.f64(angles), L.f64(x)
    sw = np.sqrt(L.f64(w))
    n = xx.size
    ed = Y._Extra(L.ptr(a), model)

    def func(p, hx, m, nn, adata):
        L.orc.orc_brdf_func(p, hx, m, nn, C.c_void_p(adata))
        out = np.ctypeslib.as_array(hx, shape=(nn,))
        if sign is not None:
            out[:] = np.nextafter(out, sign * np.inf)
        out *= sw

    cb = WY._FUNC(func)
    p, info = L.f64(p0).copy(), np.zeros(10)
    xs = np.ascontiguousarray(sw * xx)
    r = WY._BC_DIF(cb, L.ptr(p), L.ptr(xs), 3, n, L.ptr(L.f64(LB)), L.ptr(L.f64(UB)), None, 100, L.ptr(L.f64(OPTS)), L.ptr(info), None, None, C.byref(ed))
    return int(r), p


def histograms(cap, images, model, rule):
    """per fit (ascending face, then channel) and light the histogram of the valid grey levels: [fits,L,256], and the fits' faces"""
    g, face = P.walk(cap["pixel_map"], cap["nf"])
    vals = P.pixel_values(images, g)  # [P,3,L]
    valid = P.rule_valid(model, vals, cap["ang"][face], **rule)
    faces = np.unique(face)
    hist = np.zeros((3 * faces.size, vals.shape[2], 256), dtype=np.int64)
    for r, f in enumerate(faces):
        for ch in range(3):
            for l in range(vals.shape[2]):
                rows = (face == f) & valid[:, ch, l]
                hist[3 * r + ch, l] = np.bincount(vals[rows, ch, l], minlength=256)
    return hist, np.repeat(faces, 3)


@functools.lru_cache(maxsize=None)
def reference_loop(model, seed, kappa=KAPPA, rounds=ROUNDS):
    """the clip loop of the definition around the reference's weighted fit, fit by fit, on the brightened capture; seed: None, or the
    seed of the +-1 ulp perturbation of every model value.  -> (kept [fits], p [fits,3], ret [fits], lo, hi [fits,L])"""
    import brdf_amd
    cap, images, _ = brightened(model)
    hist, fit_face = histograms(cap, images, model, RULE)
    fits, lights = hist.shape[:2]
    lo, hi = brdf_amd.initial_light_intervals(cap["ang"], fit_face, model, **RULE)
    lo, hi = lo.astype(int), hi.astype(int)
    grey = np.arange(256)
    rng = np.random.default_rng(seed) if seed is not None else None
    kept, ps, rets = np.zeros(fits, dtype=np.int64), np.tile(np.array(P0), (fits, 1)), np.full(fits, -1)

    def rows(s):
        h = hist[s] * ((grey[None, :] >= lo[s][:, None]) & (grey[None, :] <= hi[s][:, None]))
        c, s1, s2 = h.sum(axis=1), (h * grey).sum(axis=1), (h * grey * grey).sum(axis=1)
        on = np.flatnonzero(c)
        within = sum(float(c[l] * s2[l] - s1[l] * s1[l]) / (65025.0 * float(c[l])) for l in on)
        return on, c[on].astype(float), s1[on] / (255.0 * c[on]), within

    for s in range(fits):
        sign = None if rng is None else np.where(rng.random(lights) < 0.5, -1.0, 1.0)
        a = cap["ang"][fit_face[s]]
        on, w, x, within = rows(s)
        kept[s] = int(w.sum())
        if on.size < 3:
            continue
        ret, p = _reference_weighted_fit(model, np.ascontiguousarray(a[:, on]), x, w, P0, None if sign is None else sign[on])
        for _ in range(rounds):
            if ret < 0:
                break
            f = L.model_values(model, np.ascontiguousarray(a), p)
            if sign is not None:
                f = np.nextafter(f, sign * np.inf)
            k = int(w.sum())
            sumsq = float(np.sum(w * (x - f[on]) ** 2) + within)
            if not np.isfinite(sumsq):
                break
            sigma = max(np.sqrt(sumsq / (k - 3)), SIGMA_MIN) if k > 3 else SIGMA_MIN
            with np.errstate(invalid="ignore"):
                ok = (np.abs(grey[None, :] / 255.0 - f[:, None]) <= kappa * sigma) & (grey[None, :] >= lo[s][:, None]) & (grey[None, :] <= hi[s][:, None])
            any_ok = ok.any(axis=1)
            old = lo[s].copy(), hi[s].copy()
            lo[s], hi[s] = np.where(any_ok, ok.argmax(axis=1), 1), np.where(any_ok, 255 - ok[:, ::-1].argmax(axis=1), 0)
            on2, w2, x2, within2 = rows(s)
            if int(w2.sum()) >= k or on2.size < 3:
                lo[s], hi[s] = old
                break
            on, w, x, within = on2, w2, x2, within2
            ret, p = _reference_weighted_fit(model, np.ascontiguousarray(a[:, on]), x, w, p, None if sign is None else sign[on])
        kept[s], ps[s], rets[s] = int(w.sum()), p, ret
    return kept, ps, rets, lo, hi


def _agreement(kept_a, p_a, ret_a, kept_b, p_b, ret_b):
    same = (kept_a == kept_b) & ((ret_a >= 0) == (ret_b >= 0))
    return int(same.sum()), int(sum(ret_a[s] < 0 or L.rel_err(p_a[s], p_b[s]) <= 1e-5 for s in np.flatnonzero(same)))


@pytest.mark.parametrize("model", [1, 2])
def test_fit_by_fit_against_the_reference_loop(gpu, model):
    """Figures printed by this test on the MI355X (A_kept, A_p of the reference against its perturbed twin; the entry's agreement):
    see DESIGN.md, "Sigma-clipped fits in the means capture"."""
    cap, images, _ = brightened(model)
    _, fit_face = histograms(cap, images, model, RULE)
    at = (fit_face, np.tile(np.arange(3), fit_face.size // 3))
    k_ref, p_ref, r_ref, _, _ = reference_loop(model, None)
    k_twin, p_twin, r_twin, _, _ = reference_loop(model, 12345)
    a_kept, a_p = _agreement(k_ref, p_ref, r_ref, k_twin, p_twin, r_twin)
    got = _clipped(gpu, cap, model, ROUNDS, images=images, **RULE)
    d_kept, d_p = _agreement(k_ref, p_ref, r_ref, got["kept"][at].astype(np.int64), got["surfaces"][at], got["ret"][at])
    print(f"model {model}: reference against its +-1 ulp twin A_kept {a_kept} A_p {a_p} of {k_ref.size}; the entry against the reference: kept {d_kept} "
          f"parameters {d_p}; samples dropped by the reference loop {int((got['count'][at] - k_ref).sum())}, by the entry "
          f"{int((got['count'][at] - got['kept'][at]).sum())}")
    assert d_kept >= a_kept - 2 and d_p >= a_p - 2, (a_kept, a_p, d_kept, d_p)
