"""The per-face capture with sigma-clipped fits (brdf_hip_fit_capture_faces_clipped_dev) on tests.capture_problems.rule_capture
(23 x 31 pixels, 37 carried faces, 16 lights):

  (a) rounds = 0: fit_capture_faces' bytes in every map and scalar -- every model, the rule on and off;
  (b) rounds = 2, kappa = 2.5 with a patch of pixels of the two faces with the most samples brightened by 60 grey levels under every
      second light: every map has the bytes of fit_batch_packed_clipped on group_capture_samples, scattered by face; kept <= count
      everywhere and kept < count on a brightened face; faces no pixel carries keep a sentinel in every map, the two new ones included;
  (c) an all-background map, and the faces whose every sample the rule removes, behave as in the faces capture."""
import numpy as np
import pytest

from tests import capture_problems as P

pytestmark = pytest.mark.gpu
OPTS, P0, LB, UB, RULE = P.OPTS, P.P0, P.LB, P.UB, P.RULE
OFF = dict(v_min=0, v_max=255, cos_min=-2.0)
SENTINEL = -7
SIGMA_MIN = 1.0 / (255.0 * np.sqrt(12.0))
MAPS = ("surfaces", "info", "ret", "count", "face_pixels", "covar", "stats", "rank")
CLIP_MAPS = MAPS + ("kept", "rounds")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _on_device(gpu, cap, images=None, pixel_map=None):
    return (_dev(gpu, cap["images"] if images is None else images), _dev(gpu, cap["pixel_map"] if pixel_map is None else pixel_map),
            _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]), _dev(gpu, cap["nrm"]), cap["leds"], cap["view"])


def _numpy(r, clipped):
    got = dict(surfaces=r.surfaces.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), count=r.count.cpu().numpy(),
               face_pixels=r.face_pixels.cpu().numpy(), covar=r.stats.covar.cpu().numpy(), stats=r.stats.stats.cpu().numpy(),
               rank=r.stats.rank.cpu().numpy(), avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)
    if clipped:
        got.update(kept=r.kept.cpu().numpy(), rounds=r.rounds.cpu().numpy())
    return got


def _faces(gpu, cap, model, images=None, pixel_map=None, **rule):
    torch, brdf_amd, _ = gpu
    r = brdf_amd.fit_capture_faces(model, *_on_device(gpu, cap, images, pixel_map), rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, **rule)
    torch.cuda.synchronize()
    return _numpy(r, False)


def _sentinel_maps(gpu, nf):
    torch, brdf_amd, dev = gpu

    def full(*shape, dtype=torch.float64):
        return torch.full((nf, *shape), SENTINEL, dtype=dtype, device=dev)
    i32 = torch.int32
    return brdf_amd.CaptureFacesClipped(full(3, 3), full(3, 10), full(3, dtype=i32), brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=i32)),
                                        full(3, dtype=i32), full(dtype=i32), None, 0, 0, full(3, dtype=i32), full(3, dtype=i32))


def _clipped(gpu, cap, model, rounds, images=None, pixel_map=None, kappa=2.5, sentinel=False, **rule):
    torch, brdf_amd, _ = gpu
    r = brdf_amd.fit_capture_faces_clipped(model, *_on_device(gpu, cap, images, pixel_map), kappa=kappa, sigma_min=SIGMA_MIN, rounds=rounds, rv_mode=1,
                                           p0=P0, lb=LB, ub=UB, opts=OPTS, out=_sentinel_maps(gpu, cap["nf"]) if sentinel else None, **rule)
    torch.cuda.synchronize()
    return _numpy(r, True)


def _same(got, want, names):
    for name in names:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), name


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [RULE, OFF], ids=["rule", "off"])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_no_rounds_is_the_faces_capture(gpu, model, rule):
    cap = P.rule_capture(model)
    want = _faces(gpu, cap, model, **rule)
    got = _clipped(gpu, cap, model, 0, **rule)
    _same(got, want, MAPS + ("avg",))
    assert (got["n_pixels"], got["n_faces"]) == (want["n_pixels"], want["n_faces"]) and got["n_faces"] == 37
    assert np.array_equal(got["kept"], got["count"]) and not got["rounds"].any()


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def _brightened(cap, model):
    """the capture with every twelfth pixel of two faces brightened by 60 grey levels under every second light: the two faces with the
    most samples under RULE (Ward's have 6 pixels: one of them is brightened, a twelfth of the fit's samples)"""
    import brdf_amd
    pm = cap["pixel_map"]
    H = pm.shape[0]
    _, _, off, fit_face, fit_channel, _ = brdf_amd.group_capture_samples(cap["images"], pm, cap["ang"], model, **RULE)
    sizes = np.zeros(cap["nf"], dtype=np.int64)
    sizes[fit_face[fit_channel == 0]] = np.diff(off)[fit_channel == 0]
    big = np.argsort(sizes, kind="stable")[-2:]
    assert sizes[big].min() >= 40, sizes[big]
    images = cap["images"].copy()
    for f in big:
        ys, xs = np.nonzero(pm == f)
        ys, xs = ys[::12], xs[::12]
        for i in range(0, images.shape[0], 2):  # a highlight: under every second light
            patch = images[i, H - 1 - ys, xs, :].astype(np.int64) + 60
            images[i, H - 1 - ys, xs, :] = np.minimum(patch, 255).astype(np.uint8)
    return images, [int(f) for f in big]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_clipped_maps_are_the_clipped_packed_batch_of_the_grouped_samples(gpu, model):
    torch, brdf_amd, _ = gpu
    cap = P.rule_capture(model)
    nf = cap["nf"]
    images, big = _brightened(cap, model)
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(images, cap["pixel_map"], cap["ang"], model, **RULE)
    S = len(fit_face)
    r = brdf_amd.fit_batch_packed_clipped(brdf_amd.METHOD_BC_DIF, model, _dev(gpu, a), _dev(gpu, x), _dev(gpu, off), _dev(gpu, np.tile(np.array(P0), (S, 1))),
                                          kappa=2.5, sigma_min=SIGMA_MIN, rounds=2, lb=LB, ub=UB, itmax=100, opts=OPTS)
    torch.cuda.synchronize()
    at = (fit_face, fit_channel)
    want = dict(surfaces=np.full((nf, 3, 3), SENTINEL, dtype=np.float64), info=np.full((nf, 3, 10), SENTINEL, dtype=np.float64),
                covar=np.full((nf, 3, 3, 3), SENTINEL, dtype=np.float64), stats=np.full((nf, 3, 8), SENTINEL, dtype=np.float64), face_pixels=face_pixels)
    for name in ("ret", "count", "rank", "kept", "rounds"):
        want[name] = np.full((nf, 3), SENTINEL, dtype=np.int32)
    want["surfaces"][at], want["info"][at], want["ret"][at] = r.p.cpu().numpy(), r.info.cpu().numpy(), r.ret.cpu().numpy()
    want["covar"][at], want["stats"][at], want["rank"][at] = r.stats.covar.cpu().numpy(), r.stats.stats.cpu().numpy(), r.stats.rank.cpu().numpy()
    want["count"][at], want["kept"][at], want["rounds"][at] = np.diff(off), r.kept.cpu().numpy(), r.rounds_used.cpu().numpy()
    got = _clipped(gpu, cap, model, 2, images=images, sentinel=True, **RULE)
    _same(got, want, CLIP_MAPS)
    carried = np.unique(fit_face)
    assert np.all(got["kept"][carried] <= got["count"][carried]) and np.all(got["rounds"][carried] <= 2)
    assert any((got["kept"][f] < got["count"][f]).any() for f in big), (big, got["kept"][big], got["count"][big])
    untouched = np.setdiff1d(np.arange(nf), carried)
    assert untouched.size >= 3 and np.all(got["kept"][untouched] == SENTINEL) and np.all(got["rounds"][untouched] == SENTINEL)
    # the faces the rule leaves fewer than 3 samples (none among them): refused, as in the faces capture, nothing clipped
    few = got["count"][carried] < 3
    assert few.any() and (got["count"][carried] == 0).any()
    assert np.all(got["ret"][carried][few] == -1) and np.all(got["kept"][carried][few] == got["count"][carried][few]) and not got["rounds"][carried][few].any()
    assert np.all(got["surfaces"][carried][few] == np.array(P0))
    plain = _faces(gpu, cap, model, images=images, **RULE)
    for name in MAPS:
        if name != "face_pixels":  # ([nf]: compared as a whole above)
            assert np.array_equal(got[name][carried][few], plain[name][carried][few], equal_nan=True), name


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_an_all_background_map_writes_nothing_but_the_pixel_counts(gpu):
    cap = P.rule_capture(1)
    empty = _clipped(gpu, cap, 1, 2, pixel_map=np.full(cap["pixel_map"].shape, -1, dtype=np.int32), sentinel=True, **RULE)
    assert empty["n_pixels"] == empty["n_faces"] == 0 and not empty["avg"].any() and not empty["face_pixels"].any()
    for name in CLIP_MAPS:
        if name != "face_pixels":
            assert np.all(empty[name] == SENTINEL), name
