"""The single-BRDF capture over every valid sample (brdf_hip_fit_capture_single_faces_dev): one fit per colour channel over the samples
of all pixels of all carried faces, its statistics, and the carried faces' residuals against it.  Captures: tests/capture_problems.py.

  (1) the definition, every model, at 16 and 5 lights under RULE: single_brdf / info / ret have the bytes of fit_single on the twin's
      channel set (group_capture_single_samples), covar / stats / rank those of fit_stats_batch with S = 1; counts, face counts, pixel
      counts and scalars are the twin's; untouched faces keep a sentinel; a second call gives the same bytes;
  (2) the residual map against NumPy sums over the oracle's model values, to the statistics yardstick's bound on a sum of squares; its
      sum over the faces against stats[c][0] and info[c][1];
  (3) the rule switched off: every candidate is a sample, the three channel sets coincide; a face of NaN cosines has no sample;
  (4) Blinn-Phong against the compiled reference's dlevmar_bc_dif on the twin's sets: objective and p;
  (5) big_capture(): the scans with two items per thread, a 300-pixel face, fits that run resident on several workgroups;
  (6) wide_capture(64, 150, 150): above 2^20 samples per channel, the launch chain;
  (7) a channel without samples, and one of two samples, is refused on its own; an all-background map refuses all three."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import capture_problems as P
from tests import oracle_libs as L
from tests import stats_yardstick as Y

pytestmark = pytest.mark.gpu
SENTINEL = -7
HOST = ("single_brdf", "info", "ret", "count", "covar", "stats", "rank")
EVERY = HOST + ("face_sumsq", "face_count", "face_pixels")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sentinel_maps(gpu, nf):
    torch, brdf_amd, dev = gpu
    return brdf_amd.CaptureSingleFaces(None, None, None, None, None, torch.full((nf, 3), float(SENTINEL), dtype=torch.float64, device=dev),
                                       torch.full((nf, 3), SENTINEL, dtype=torch.int32, device=dev),
                                       torch.full((nf,), SENTINEL, dtype=torch.int32, device=dev), 0, 0)


def _single(gpu, cap, model, images=None, pixel_map=None, sentinel=True, **rule):
    """fit_capture_single_faces on the capture, everything on the host: a dict of numpy arrays"""
    torch, brdf_amd, _ = gpu
    images = cap["images"] if images is None else images
    pixel_map = cap["pixel_map"] if pixel_map is None else pixel_map
    r = brdf_amd.fit_capture_single_faces(model, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]),
                                          _dev(gpu, cap["nrm"]), cap["leds"], cap["view"], rv_mode=1, p0=P.P0, lb=P.LB, ub=P.UB, itmax=100,
                                          opts=P.OPTS, validate=False, out=_sentinel_maps(gpu, cap["nf"]) if sentinel else None, **rule)
    torch.cuda.synchronize()
    return dict(single_brdf=r.single_brdf, info=r.info, ret=r.ret, count=r.count, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank,
                face_sumsq=r.face_sumsq.cpu().numpy(), face_count=r.face_count.cpu().numpy(), face_pixels=r.face_pixels.cpu().numpy(),
                n_pixels=r.n_pixels, n_faces=r.n_faces)


def _twin(cap, model, images=None, pixel_map=None, **rule):
    import brdf_amd
    return brdf_amd.group_capture_single_samples(cap["images"] if images is None else images, cap["pixel_map"] if pixel_map is None else pixel_map,
                                                 cap["ang"], model, **rule)


def _definition(gpu, model, twin):
    """fit_single and fit_stats_batch (S = 1) on the twin's channel sets, laid out as the entry's host outputs; a channel of fewer than 3
    samples is levmar's refusal"""
    torch, brdf_amd, _ = gpu
    want = dict(single_brdf=np.tile(np.array(P.P0), (3, 1)), info=np.zeros((3, 10)), ret=np.full(3, -1, dtype=np.int32), count=np.zeros(3, dtype=np.int64),
                covar=np.zeros((3, 3, 3)), stats=np.zeros((3, 8)), rank=np.zeros(3, dtype=np.int32))
    for c in range(3):
        ang, x, _ = twin.channels[c]
        want["count"][c] = x.size
        if 0 < x.size < 3:  # refused; its statistics are the ragged pass's on a row of stride 3 at p0
            rows, xs = np.full((1, 3, 3), np.nan), np.full((1, 3), np.nan)
            rows[0, :, :x.size], xs[0, :x.size] = ang, x
            st = brdf_amd.fit_stats_batch(brdf_amd.METHOD_BC_DIF, model, _dev(gpu, rows), _dev(gpu, xs), _dev(gpu, np.array([P.P0])), opts=P.OPTS,
                                          counts=_dev(gpu, np.array([x.size], dtype=np.int32)))
            torch.cuda.synchronize()
            want["covar"][c], want["stats"][c], want["rank"][c] = st.covar.cpu().numpy()[0], st.stats.cpu().numpy()[0], st.rank.cpu().numpy()[0]
        if x.size < 3:
            continue
        da, dx = _dev(gpu, ang), _dev(gpu, x)
        res = brdf_amd.fit_single(brdf_amd.METHOD_BC_DIF, model, da, dx, P.P0, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS)
        st = brdf_amd.fit_stats_batch(brdf_amd.METHOD_BC_DIF, model, da[None], dx[None], _dev(gpu, res.p[None]), opts=P.OPTS)
        torch.cuda.synchronize()
        want["single_brdf"][c], want["info"][c], want["ret"][c] = res.p, res.info, res.ret
        want["covar"][c], want["stats"][c], want["rank"][c] = st.covar.cpu().numpy()[0], st.stats.cpu().numpy()[0], st.rank.cpu().numpy()[0]
    return want


def _check_definition(got, want, twin, nf, stats=True):
    for name in HOST if stats else HOST[:4]:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])
    carried = twin.faces
    assert got["n_faces"] == carried.size and got["n_pixels"] == int(twin.face_pixels.sum())
    assert np.array_equal(got["face_pixels"], twin.face_pixels)
    for c in range(3):
        assert np.array_equal(got["face_count"][carried, c], np.diff(twin.channels[c][2])), c
    untouched = np.setdiff1d(np.arange(nf), carried)
    assert np.all(got["face_count"][untouched] == SENTINEL) and np.all(got["face_sumsq"][untouched] == SENTINEL)


def _check_residuals(got, twin, model):
    """face_sumsq[f][c] against the NumPy sum over the oracle's model values; the bound: the project's E_TOL on a sum of squares, or the
    yardstick's first-order bound (4 ulp per model value, the reordered sum) with its margin, whichever is larger"""
    worst = 0.0
    for c in range(3):
        ang, x, fo = twin.channels[c]
        if x.size == 0:
            assert not got["face_sumsq"][twin.faces, c].any()
            continue
        with np.errstate(all="ignore"):
            hx = L.model_values(model, ang, got["single_brdf"][c])
            e = x - hx
        total = 0.0
        for r, f in enumerate(twin.faces):
            seg = slice(int(fo[r]), int(fo[r + 1]))
            k = seg.stop - seg.start
            mine = float(got["face_sumsq"][f, c])
            if k == 0:
                assert mine == 0.0 and got["face_count"][f, c] == 0, (f, c, mine)
                continue
            with np.errstate(all="ignore"):
                ref = float(e[seg] @ e[seg])
            if not np.isfinite(ref):
                assert not np.isfinite(mine), (f, c, mine, ref)
                total = np.nan
                continue
            bound = max(Y.E_TOL, Y.MARGIN * Y.sumsq_bound(dict(sumsq=ref, fnorm=float(np.linalg.norm(hx[seg])), n=k))) * ref
            worst = max(worst, abs(mine - ref) / bound if bound > 0 else (0.0 if mine == ref else np.inf))
            assert abs(mine - ref) <= bound, (f, c, k, mine, ref, bound)
            total += mine
        if np.isfinite(total):
            print(f"model {model} channel {c}: sum of the face map {total:.17e} stats[0] {got['stats'][c, 0]:.17e} info[1] {got['info'][c, 1]:.17e}")
            assert abs(total - got["stats"][c, 0]) <= Y.E_TOL * got["stats"][c, 0], (c, total, got["stats"][c, 0])
            if got["info"][c, 6] != 0:  # (a refused channel has no fit: zero info)
                assert abs(total - got["info"][c, 1]) <= Y.E_TOL * got["info"][c, 1], (c, total, got["info"][c, 1])
    print(f"model {model}: worst face residual error / bound = {worst:.3e}")


def _check_reference(got, twin, model, iterations):
    """the compiled reference's dlevmar_bc_dif on every channel's set: it converges (reason 2); the capture tests' bar on the objective,
    the project's bar on a converged p"""
    for c in range(3):
        ang, x, _ = twin.channels[c]
        ret, p_ref, info_ref = L.brdf_fit("ref", 1, model, ang, x, P.P0, 100, P.OPTS, P.LB, P.UB)
        print(f"channel {c}: K {x.size} reference ret {ret} reason {info_ref[6]:.0f} objective {info_ref[1]:.17e} p {p_ref}; "
              f"entry ret {got['ret'][c]} reason {got['info'][c, 6]:.0f} objective {got['info'][c, 1]:.17e} p {got['single_brdf'][c]}")
        assert info_ref[6] == 2 and iterations[0] <= ret <= iterations[1], (c, ret, info_ref)
        assert got["ret"][c] >= 0
        assert got["info"][c, 1] <= info_ref[1] * (1 + 1e-3) + 1e-20, (c, got["info"][c, 1], info_ref[1])
        assert L.rel_err(got["single_brdf"][c], p_ref) <= 1e-5, (c, got["single_brdf"][c], p_ref)


@functools.lru_cache(maxsize=None)
def _ruled(gpu, model, lights):
    """the entry and its twin on rule_capture(model, lights=lights) under RULE: tests (1), (2) and (7) share the call"""
    cap = P.rule_capture(model, lights=lights)
    return cap, _single(gpu, cap, model, **P.RULE), _twin(cap, model, **P.RULE)


@pytest.mark.parametrize("lights", [16, 5])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_definition_every_model(gpu, model, lights):
    cap, got, twin = _ruled(gpu, model, lights)
    counts = [int(got["count"][c]) for c in range(3)]
    print("model", model, "lights", lights, "K", counts, "ret", got["ret"], "reason", got["info"][:, 6])
    want = {16: {0: [6822] * 3, 1: [2267, 2258, 2257], 2: [993, 1006, 1013]}, 5: {0: [2106] * 3, 1: [558] * 3}}[lights].get(model)
    assert counts == want if want else all(287 <= k <= 289 for k in counts)
    assert got["n_pixels"] == 604 and got["n_faces"] == 37
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    again = _single(gpu, cap, model, **P.RULE)
    for name in EVERY:
        assert again[name].tobytes() == got[name].tobytes(), name
    if model == 2 and lights == 16:  # the reference ends these two the same way: the byte contract holds whatever the stop reason
        assert got["info"][0, 6] == 7 and got["info"][1, 6] == 7 and list(got["ret"][:2]) == [-1, -1]


@pytest.mark.parametrize("lights", [16, 5])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_residual_map(gpu, model, lights):
    _, got, twin = _ruled(gpu, model, lights)
    _check_residuals(got, twin, model)


@pytest.mark.parametrize("lights", [16, 5])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_rule_off_every_candidate_is_a_sample(gpu, model, lights):
    cap = P.rule_capture(model, lights=lights)
    got, twin = _single(gpu, cap, model), _twin(cap, model)
    print("model", model, "lights", lights, "ret", got["ret"], "reason", got["info"][:, 6])
    assert list(got["count"]) == [604 * lights] * 3 and (lights != 16 or got["count"][0] == 9664)
    assert twin.channels[0][0].tobytes() == twin.channels[1][0].tobytes() == twin.channels[2][0].tobytes()
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    assert np.all(got["face_count"][twin.faces] == (twin.face_pixels[twin.faces] * lights)[:, None])
    _check_residuals(got, twin, model)


def test_rule_off_a_face_of_nan_cosines_has_no_sample(gpu):
    model = 1
    cap = P.rule_capture(model, nan_face=True)
    got, twin = _single(gpu, cap, model), _twin(cap, model)
    f = cap["nan_face"]
    assert list(got["count"]) == [9504] * 3
    assert np.all(got["face_count"][f] == 0) and np.all(got["face_sumsq"][f] == 0.0) and got["face_pixels"][f] == 10
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    without = _single(gpu, cap, model, pixel_map=cap["pixel_map_without"])
    for name in HOST:
        assert without[name].tobytes() == got[name].tobytes(), name
    assert without["n_faces"] == got["n_faces"] - 1 and without["n_pixels"] == got["n_pixels"] - 10


def test_against_the_compiled_reference(gpu):
    _, got, twin = _ruled(gpu, 1, 16)
    _check_reference(got, twin, 1, (17, 18))


def test_scans_and_the_multi_workgroup_resident_fit(gpu):
    model = 1
    cap = P.big_capture()
    got, twin = _single(gpu, cap, model, **P.RULE), _twin(cap, model, **P.RULE)
    assert list(got["count"]) == [31072, 31088, 31110] and got["n_pixels"] == 4500 and got["n_faces"] == 644
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    _check_residuals(got, twin, model)
    _check_reference(got, twin, model, (20, 25))
    nf = cap["nf"]
    for f in (0, 65535, 65536, nf - 1):  # carried faces at both ends of the map and across 2^16
        r = int(np.searchsorted(twin.faces, f))
        assert twin.faces[r] == f and got["face_pixels"][f] == twin.face_pixels[f] > 0
        for c in range(3):
            assert got["face_count"][f, c] == twin.channels[c][2][r + 1] - twin.channels[c][2][r]
            assert got["face_sumsq"][f, c] != SENTINEL
    big = cap["big_face"]
    assert np.all(got["face_count"][big] == 4800) and got["face_pixels"][big] == 300  # five residual chunks
    again = _single(gpu, cap, model, **P.RULE)
    for name in EVERY:
        assert again[name].tobytes() == got[name].tobytes(), name


def test_above_two_to_the_twenty_samples_at_64_lights(gpu):
    model = 1
    cap = P.wide_capture(64, 150, 150)
    got, twin = _single(gpu, cap, model, **P.RULE), _twin(cap, model, **P.RULE)
    print("K", got["count"], "ret", got["ret"], "reason", got["info"][:, 6])
    assert list(got["count"]) == [1390156, 1393015, 1395137] and min(got["count"]) > 2 ** 20
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])


def test_a_channel_of_two_samples_is_refused_with_the_ragged_statistics(gpu):
    """channel B keeps two valid values of one pixel: K_0 = 2, the n < m refusal; its statistics are those of the two samples"""
    model = 1
    cap, first, _ = _ruled(gpu, model, 16)
    g, face = P.walk(cap["pixel_map"], cap["nf"])
    valid = P.rule_valid(model, P.pixel_values(cap["images"], g), cap["ang"][face], **P.RULE)[:, 0, :]  # [pixels, lights] of channel B
    pixel = int(np.flatnonzero(valid.sum(axis=1) >= 2)[0])
    lights = np.flatnonzero(valid[pixel])[:2]
    H = cap["images"].shape[1]
    x_, y_ = int(g[pixel] // H), int(g[pixel] % H)
    images = cap["images"].copy()
    images[..., 0] = 0
    images[lights, H - 1 - y_, x_, 0] = cap["images"][lights, H - 1 - y_, x_, 0]
    got, twin = _single(gpu, cap, model, images=images, **P.RULE), _twin(cap, model, images=images, **P.RULE)
    assert list(got["count"]) == [2, 2258, 2257]
    assert got["ret"][0] == -1 and not got["info"][0].any() and np.array_equal(got["single_brdf"][0], P.P0) and got["rank"][0] == 0
    assert got["stats"][0, 0] > 0.0 and not got["covar"][0].any()  # sumsq of the two samples at p0; no covariance
    f = int(face[pixel])
    assert got["face_count"][f, 0] == 2 and got["face_count"][twin.faces, 0].sum() == 2
    assert abs(got["face_sumsq"][f, 0] - got["stats"][0, 0]) <= Y.E_TOL * got["stats"][0, 0]
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    _check_residuals(got, twin, model)
    for name in HOST:  # the other two channels do not notice
        assert got[name][1:].tobytes() == first[name][1:].tobytes(), name


def _raw_call(gpu, cap, model, images, pixel_map, maps, **rule):
    """the C entry itself: (its return value, single_brdf, info, ret, rank, n_pixels, n_faces)"""
    torch, brdf_amd, dev = gpu
    from brdf_amd import fit as F
    args, keep, _ = F._capture_args(model, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]),
                                    _dev(gpu, cap["nrm"]), cap["leds"], cap["view"], 1, P.P0, P.LB, P.UB, 100, P.OPTS, False)
    single, info, ret, rank = np.full((3, 3), np.nan), np.full((3, 10), np.nan), np.full(3, SENTINEL, dtype=np.int32), np.full(3, SENTINEL, dtype=np.int32)
    npx, nfc = C.c_longlong(-1), C.c_longlong(-1)
    with torch.cuda.device(dev):
        rc = brdf_amd.lib.brdf_hip_fit_capture_single_faces_dev(*args, rule["v_min"], rule["v_max"], rule["cos_min"], F._dptr(single), F._dptr(info),
                                                                F._iptr(ret), None, None, F._iptr(rank), None, maps.face_sumsq.data_ptr(),
                                                                maps.face_count.data_ptr(), maps.face_pixels.data_ptr(), C.byref(npx), C.byref(nfc),
                                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, single, info, ret, rank, npx.value, nfc.value


def test_refused_channels(gpu):
    model = 1
    cap, first, _ = _ruled(gpu, model, 16)
    images = cap["images"].copy()
    images[..., 0] = 0  # channel B is black everywhere: under RULE it has no sample
    got, twin = _single(gpu, cap, model, images=images, **P.RULE), _twin(cap, model, images=images, **P.RULE)
    assert list(got["count"]) == [0, 2258, 2257]
    assert got["ret"][0] == -1 and not got["info"][0].any() and np.array_equal(got["single_brdf"][0], P.P0) and got["rank"][0] == 0
    assert not got["covar"][0].any() and not got["stats"][0].any()
    assert not got["face_count"][twin.faces, 0].any() and not got["face_sumsq"][twin.faces, 0].any()
    for name in HOST:  # the other two channels do not notice
        assert got[name][1:].tobytes() == first[name][1:].tobytes(), name
    assert got["face_sumsq"][:, 1:].tobytes() == first["face_sumsq"][:, 1:].tobytes()
    assert got["face_count"][:, 1:].tobytes() == first["face_count"][:, 1:].tobytes()
    _check_definition(got, _definition(gpu, model, twin), twin, cap["nf"])
    rc, single, info, ret, rank, npx, nfc = _raw_call(gpu, cap, model, images, cap["pixel_map"], _sentinel_maps(gpu, cap["nf"]), **P.RULE)
    assert rc == 1 and list(ret) == list(got["ret"]) and single.tobytes() == got["single_brdf"].tobytes() and (npx, nfc) == (604, 37)
    # an all-background map: every channel is refused, nothing is written on the device but the pixel counts
    maps = _sentinel_maps(gpu, cap["nf"])
    rc, single, info, ret, rank, npx, nfc = _raw_call(gpu, cap, model, cap["images"], np.full_like(cap["pixel_map"], -1), maps, **P.RULE)
    assert rc == 3 and list(ret) == [-1] * 3 and not info.any() and list(rank) == [0] * 3 and (npx, nfc) == (0, 0)
    assert np.array_equal(single, np.tile(np.array(P.P0), (3, 1)))
    assert np.all(maps.face_sumsq.cpu().numpy() == SENTINEL) and np.all(maps.face_count.cpu().numpy() == SENTINEL)
    assert not maps.face_pixels.cpu().numpy().any()
