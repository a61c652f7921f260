"""The capture pipeline on the device at the shapes of tests/capture_problems.py: every model's plane set in the validity rule,
rv_mode = 0, scans whose threads own more than one item, grid-stride loops that wrap, L != 16 in the masked capture, nullable maps,
a face whose cosines are NaN.  Bytes are compared against brdf_amd.group_capture_samples (checked against a plain loop on the CPU),
the C oracle's cosine planes and the batched / packed entries, which other tests check against levmar; never against a second call
of the entry under test, except for the nullable maps in (D).

  (A) rule_capture(model), rule `1, 254, 0.0`, models 0, 1, 2: the per-face entry is fit_batch_packed + fit_stats_batch_packed on the
      host twin's grouping; the masked capture is the ragged batch built in NumPy; both count maps are the rule evaluated in NumPy
  (B) rv_mode = 0, whose third plane is -sf^2: with cos_min = 0 Phong and Ward have no sample at all; with cos_min = -2: as (A)
  (C) big_capture(): the definition of (A) on all maps, the pixel counts, the sentinel of untouched faces, avg; models 0 and 2
  (D) the per-face entry's nullable maps, through ctypes
  (E) the masked capture at 5 and 64 lights (mask_serial_kernel), rule on and off
  (F) wide_capture at (16, 300, 300) and (64, 150, 150): gather_kernel and both cosines kernels past one trip of their grids
  (G) a face with a NaN normal: the other faces do not notice; what each entry does with it"""
import ctypes as C

import numpy as np
import pytest

from tests import capture_problems as P
from tests import oracle_libs as L

pytestmark = pytest.mark.gpu
OPTS, P0, LB, UB, RULE = P.OPTS, P.P0, P.LB, P.UB, P.RULE
SENTINEL = -7
MAPS = ("surfaces", "info", "ret", "count", "face_pixels", "covar", "stats", "rank")
MASKED_MAPS = ("surfaces", "count", "covar", "stats", "rank")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _capture_on_device(gpu, cap, images=None, pixel_map=None):
    return (_dev(gpu, cap["images"] if images is None else images), _dev(gpu, cap["pixel_map"] if pixel_map is None else pixel_map),
            _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]), _dev(gpu, cap["nrm"]), cap["leds"], cap["view"])


def _sentinel_maps(gpu, nf):
    torch, brdf_amd, dev = gpu

    def full(*shape, dtype=torch.float64):
        return torch.full((nf, *shape), SENTINEL, dtype=dtype, device=dev)
    return brdf_amd.CaptureFaces(full(3, 3), full(3, 10), full(3, dtype=torch.int32),
                                 brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=torch.int32)), full(3, dtype=torch.int32),
                                 full(dtype=torch.int32), None, 0, 0)


def _faces(gpu, cap, model, rv_mode=1, pixel_map=None, out=None, validate=True, want_stats=True, **rule):
    """fit_capture_faces, everything on the host: a dict of numpy arrays"""
    torch, brdf_amd, _ = gpu
    r = brdf_amd.fit_capture_faces(model, *_capture_on_device(gpu, cap, pixel_map=pixel_map), rv_mode=rv_mode, p0=P0, lb=LB, ub=UB, opts=OPTS,
                                   out=out, validate=validate, want_stats=want_stats, **rule)
    torch.cuda.synchronize()
    got = dict(surfaces=r.surfaces.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), count=r.count.cpu().numpy(),
               face_pixels=r.face_pixels.cpu().numpy(), avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)
    if want_stats:
        got.update(covar=r.stats.covar.cpu().numpy(), stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy())
    return got


def _packed(gpu, cap, model, ang, fill=0, pixel_map=None, want_stats=True, **rule):
    """the per-face entry's definition: group_capture_samples -> fit_batch_packed + fit_stats_batch_packed, laid out as the entry's maps"""
    torch, brdf_amd, _ = gpu
    nf = cap["nf"]
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"] if pixel_map is None else pixel_map,
                                                                                  ang, model, **rule)
    S = len(fit_face)
    da, dx, do = _dev(gpu, a), _dev(gpu, x), _dev(gpu, off)
    p, info, ret = brdf_amd.fit_batch_packed(brdf_amd.METHOD_BC_DIF, model, da, dx, do, _dev(gpu, np.tile(np.array(P0), (S, 1))), lb=LB, ub=UB,
                                             itmax=100, opts=OPTS)
    at = (fit_face, fit_channel)
    want = dict(surfaces=np.full((nf, 3, 3), fill, dtype=np.float64), info=np.full((nf, 3, 10), fill, dtype=np.float64),
                ret=np.full((nf, 3), fill, dtype=np.int32), count=np.full((nf, 3), fill, dtype=np.int32), face_pixels=face_pixels)
    want["surfaces"][at], want["info"][at], want["ret"][at] = p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
    want["count"][at] = np.diff(off)
    if want_stats:
        st = brdf_amd.fit_stats_batch_packed(brdf_amd.METHOD_BC_DIF, model, da, dx, do, p, opts=OPTS)
        want.update(covar=np.full((nf, 3, 3, 3), fill, dtype=np.float64), stats=np.full((nf, 3, 8), fill, dtype=np.float64),
                    rank=np.full((nf, 3), fill, dtype=np.int32))
        want["covar"][at], want["stats"][at], want["rank"][at] = st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()
    torch.cuda.synchronize()
    return want, dict(off=off, fit_face=fit_face, fit_channel=fit_channel)


def _numpy_face_counts(cap, model, ang, **rule):
    """count[nf,3] of the per-face entry: the rule over all pixels of a face, without the host twin"""
    g, face = P.walk(cap["pixel_map"], cap["nf"])
    valid = P.rule_valid(model, P.pixel_values(cap["images"], g), ang[face], **rule)
    counts = np.zeros((cap["nf"], 3), dtype=np.int32)
    np.add.at(counts, face, valid.sum(axis=2).astype(np.int32))
    return counts


def _capture_result(out):
    surf, avg, npx, st = out[:4]
    got = dict(surfaces=surf.cpu().numpy(), avg=avg, n_pixels=npx, covar=st.covar.cpu().numpy(), stats=st.stats.cpu().numpy(),
               rank=st.rank.cpu().numpy())
    if len(out) > 4:
        got["count"] = out[4].cpu().numpy()
    return got


def _masked(gpu, cap, model, rv_mode=1, pixel_map=None, **rule):
    torch, brdf_amd, _ = gpu
    out = brdf_amd.fit_capture_masked(model, *_capture_on_device(gpu, cap, pixel_map=pixel_map), rv_mode=rv_mode, p0=P0, lb=LB, ub=UB, opts=OPTS, **rule)
    torch.cuda.synchronize()
    return _capture_result(out)


def _plain(gpu, cap, model, rv_mode=1, pixel_map=None):
    torch, brdf_amd, _ = gpu
    out = brdf_amd.fit_capture(model, *_capture_on_device(gpu, cap, pixel_map=pixel_map), rv_mode=rv_mode, p0=P0, lb=LB, ub=UB, opts=OPTS,
                               want_stats=True)
    torch.cuda.synchronize()
    return _capture_result(out)


def _ragged(gpu, cap, model, ang, **rule):
    """the masked capture's definition, built in NumPy as tests/test_gpu_capture_masked.py builds it: every carried pixel's three fits
    (q = 3 * place in the walk + channel) with the oracle's planes, the rule, compact_samples, fit_batch and fit_stats_batch with the
    counts; a face's maps hold the fits of its LAST pixel.  Returns (the maps, the counts of all fits)."""
    torch, brdf_amd, _ = gpu
    nf = cap["nf"]
    g, face = P.walk(cap["pixel_map"], nf)
    value = P.pixel_values(cap["images"], g)  # [P,3,L]
    valid = P.rule_valid(model, value, ang[face], **rule)
    lights = value.shape[2]
    a_c, x_c, counts = brdf_amd.compact_samples(np.repeat(ang[face], 3, axis=0), value.reshape(-1, lights) / 255.0, valid.reshape(-1, lights))
    assert np.array_equal(counts, valid.reshape(-1, lights).sum(axis=1))
    da, dx, dc = _dev(gpu, a_c), _dev(gpu, x_c), _dev(gpu, counts)
    p, _, _ = brdf_amd.fit_batch(brdf_amd.METHOD_BC_DIF, model, da, dx, _dev(gpu, np.tile(np.array(P0), (len(counts), 1))), lb=LB, ub=UB, itmax=100,
                                 opts=OPTS, counts=dc)
    st = brdf_amd.fit_stats_batch(brdf_amd.METHOD_BC_DIF, model, da, dx, p, opts=OPTS, counts=dc)
    torch.cuda.synchronize()
    carried, last = P.last_pixels(cap["pixel_map"], nf)
    want = dict(surfaces=np.zeros((nf, 3, 3)), count=np.zeros((nf, 3), dtype=np.int32), covar=np.zeros((nf, 3, 3, 3)), stats=np.zeros((nf, 3, 8)),
                rank=np.zeros((nf, 3), dtype=np.int32))
    per_pixel = lambda t, *shape: t.cpu().numpy().reshape(-1, 3, *shape)[last]  # noqa: E731
    want["surfaces"][carried], want["count"][carried] = per_pixel(p, 3), counts.reshape(-1, 3)[last]
    want["covar"][carried], want["stats"][carried], want["rank"][carried] = per_pixel(st.covar, 3, 3), per_pixel(st.stats, 8), per_pixel(st.rank)
    return want, counts


def _same_bytes(got, want, names, rows=None):
    for name in names:
        g, w = (got[name], want[name]) if rows is None else (got[name][rows], want[name][rows])
        assert g.dtype == w.dtype and g.shape == w.shape and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), name


# ---- (A) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_rule_reads_the_planes_of_the_model(gpu, model):
    cap = P.rule_capture(model)
    nf = cap["nf"]
    want, group = _packed(gpu, cap, model, cap["ang"], fill=SENTINEL, **RULE)
    got = _faces(gpu, cap, model, out=_sentinel_maps(gpu, nf), **RULE)
    _same_bytes(got, want, MAPS)
    counts = _numpy_face_counts(cap, model, cap["ang"], **RULE)
    carried = np.unique(group["fit_face"])
    assert carried.size == 37 and np.array_equal(got["count"][carried], counts[carried])
    assert (counts[carried] >= 3).any() and (counts[carried] < 3).any()
    assert got["n_pixels"] == int((cap["pixel_map"] > -1).sum()) and got["n_faces"] == 37


@pytest.mark.parametrize("model", [0, 1, 2])
def test_masked_rule_reads_the_planes_of_the_model(gpu, model):
    cap = P.rule_capture(model)
    want, fit_counts = _ragged(gpu, cap, model, cap["ang"], **RULE)
    assert fit_counts.min() < 3 <= fit_counts.max()
    got = _masked(gpu, cap, model, **RULE)
    _same_bytes(got, want, MASKED_MAPS)  # (the count map: the rule evaluated in NumPy, as asserted in _ragged)
    assert got["n_pixels"] == int((cap["pixel_map"] > -1).sum())


# ---- (B) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 2])
def test_rv_mode_0(gpu, model):
    cap = P.rule_capture(model)
    nf = cap["nf"]
    ang = L.cosines(cap["vertices"], cap["faces"], cap["nrm"], cap["leds"], cap["view"], rv_mode=0)
    assert (ang[:, 2] <= 0.0).all()  # R.P = -sf^2: Phong and Ward, which read it, keep nothing at cos_min = 0
    carried = np.unique(cap["pixel_map"][cap["pixel_map"] > -1])
    got = _faces(gpu, cap, model, rv_mode=0, out=_sentinel_maps(gpu, nf), **RULE)  # (returns 0: a failure raises)
    assert got["n_faces"] == carried.size == 37
    assert not got["count"][carried].any() and np.all(got["ret"][carried] == -1) and not got["info"][carried].any()
    assert np.all(got["surfaces"][carried] == np.array(P0)) and not got["rank"][carried].any()
    untouched = np.setdiff1d(np.arange(nf), carried)
    assert np.all(got["surfaces"][untouched] == SENTINEL) and np.all(got["count"][untouched] == SENTINEL)
    got_m = _masked(gpu, cap, model, rv_mode=0, **RULE)
    assert not got_m["count"].any() and np.all(got_m["surfaces"][carried] == np.array(P0)) and not got_m["rank"].any() and not got_m["covar"].any()
    # the cosine test off, the intensity test on: the definitions of (A) with the planes of rv_mode = 0
    rule = dict(v_min=1, v_max=254, cos_min=-2.0)
    want, _ = _packed(gpu, cap, model, ang, fill=SENTINEL, **rule)
    _same_bytes(_faces(gpu, cap, model, rv_mode=0, out=_sentinel_maps(gpu, nf), **rule), want, MAPS)
    assert want["count"][carried].max() > 16
    want_m, _ = _ragged(gpu, cap, model, ang, **rule)
    _same_bytes(_masked(gpu, cap, model, rv_mode=0, **rule), want_m, MASKED_MAPS)


# ---- (C) ------------------------------------------------------------------------------------------------------------------------
def test_big_capture_is_the_packed_batch_of_its_grouping(gpu):
    torch, brdf_amd, _ = gpu
    cap = P.big_capture()
    nf, carried = cap["nf"], cap["carried"]
    want, group = _packed(gpu, cap, 1, cap["ang"], fill=SENTINEL, **RULE)
    got = _faces(gpu, cap, 1, out=_sentinel_maps(gpu, nf), validate=False, **RULE)
    classes = brdf_amd.last_packed_stats()
    print("size classes of the entry's statistics call:", classes)
    assert all(classes[c]["fits"] > 0 for c in (0, 1, 2, 3, 5)), classes
    _same_bytes(got, want, MAPS)
    flat = cap["pixel_map"].reshape(-1)
    face_pixels = np.bincount(flat[(flat > -1) & (flat < nf)], minlength=nf)
    assert np.array_equal(got["face_pixels"], face_pixels) and got["n_pixels"] == 4500 == int(face_pixels.sum()) and got["n_faces"] == 644
    assert np.array_equal(got["count"][carried], _numpy_face_counts(cap, 1, cap["ang"], **RULE)[carried])
    untouched = np.ones(nf, dtype=bool)
    untouched[carried] = False
    for name in MAPS:
        if name != "face_pixels":
            assert np.all(got[name][untouched] == SENTINEL), name
    # 3 F = 1932 addends per parameter, all >= 0 (the box): any order of the sum is within 3 F * 2^-53 relative of any other
    written = got["surfaces"][carried].reshape(-1, 3)
    assert np.all(written >= 0.0)
    ref = written.sum(axis=0) / (nf * 3)
    print("avg:", got["avg"], "numpy:", ref, "relative difference:", np.abs(got["avg"] - ref) / np.abs(ref))
    assert np.all(np.abs(got["avg"] - ref) <= 3 * carried.size * 2.0 ** -53 * np.abs(ref)), (got["avg"], ref)


@pytest.mark.parametrize("model", [0, 2])
def test_big_capture_in_the_other_models(gpu, model):
    cap = P.big_capture()
    want, _ = _packed(gpu, cap, model, cap["ang"], want_stats=False, **RULE)
    got = _faces(gpu, cap, model, validate=False, want_stats=False, **RULE)
    _same_bytes(got, want, ("count", "ret", "surfaces"))
    assert want["count"].max() > 4096 and (want["count"][cap["carried"]] < 3).any()


# ---- (D) ------------------------------------------------------------------------------------------------------------------------
def _faces_raw(gpu, cap, model, passed, **rule):
    """brdf_hip_fit_capture_faces_dev through ctypes with only the maps named in `passed` (and d_brdf_surfaces): the others are NULL"""
    torch, brdf_amd, dev = gpu
    from brdf_amd import fit
    nf = cap["nf"]
    images, pixel_map, vertices, faces, nrm, leds, view = _capture_on_device(gpu, cap)
    lights, H, W = cap["images"].shape[:3]
    host = [np.ascontiguousarray(a, dtype=np.float64) for a in (leds, view, P0, LB, UB, OPTS)]
    dbl = [a.ctypes.data_as(fit.D) for a in host]
    m = _sentinel_maps(gpu, nf)
    maps = dict(surfaces=m.surfaces, info=m.info, ret=m.ret, covar=m.stats.covar, stats=m.stats.stats, rank=m.stats.rank, count=m.count,
                face_pixels=m.face_pixels)
    ptr = lambda name: maps[name].data_ptr() if name in passed or name == "surfaces" else None  # noqa: E731
    avg, npx, nfc = np.zeros(3), C.c_longlong(0), C.c_longlong(0)
    fit._call("brdf_hip_fit_capture_faces_dev", dev, model, images.data_ptr(), lights, H, W, pixel_map.data_ptr(), vertices.data_ptr(),
              faces.data_ptr(), nrm.data_ptr(), nf, dbl[0], dbl[1], 1, dbl[2], dbl[3], dbl[4], 100, dbl[5], rule["v_min"], rule["v_max"],
              rule["cos_min"], 0, ptr("surfaces"), ptr("info"), ptr("ret"), ptr("covar"), ptr("stats"), ptr("rank"), ptr("count"),
              ptr("face_pixels"), avg.ctypes.data_as(fit.D), C.byref(npx), C.byref(nfc), fit._STREAM)
    torch.cuda.synchronize()
    got = {name: t.cpu().numpy() for name, t in maps.items()}
    got.update(avg=avg, n_pixels=npx.value, n_faces=nfc.value)
    return got


def test_nullable_maps(gpu):
    cap = P.rule_capture(1)
    full = _faces_raw(gpu, cap, 1, MAPS, **RULE)
    assert (full["count"][full["face_pixels"] > 0] >= 3).any() and not np.all(full["rank"] == SENTINEL)
    for passed in ((), ("info",), ("ret",), ("count",), ("face_pixels",), ("rank",)):  # rank alone: the statistics pass, covar and stats NULL
        got = _faces_raw(gpu, cap, 1, passed, **RULE)
        _same_bytes(got, full, ("surfaces", "avg") + passed)
        assert (got["n_pixels"], got["n_faces"]) == (full["n_pixels"], full["n_faces"]), passed
        for name in MAPS:  # what was not passed was not written through a stale pointer either
            if name not in passed and name != "surfaces":
                assert np.all(got[name] == SENTINEL), (passed, name)


# ---- (E) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [5, 64])
def test_masked_capture_at_other_light_counts(gpu, lights):
    cap = P.rule_capture(1, False, lights)
    assert cap["images"].shape[0] == lights and cap["ang"].shape == (cap["nf"], 3, lights)
    want, counts = _ragged(gpu, cap, 1, cap["ang"], **RULE)
    assert counts.min() < 3 <= counts.max() and (counts < lights).any() and (lights == 5 or counts.max() > 16)
    _same_bytes(_masked(gpu, cap, 1, **RULE), want, MASKED_MAPS)
    off, plain = _masked(gpu, cap, 1), _plain(gpu, cap, 1)  # the rule switched off
    _same_bytes(off, plain, ("surfaces", "avg", "covar", "stats", "rank"))
    carried = np.unique(cap["pixel_map"][cap["pixel_map"] > -1])
    assert off["n_pixels"] == plain["n_pixels"] and np.all(off["count"][carried] == lights) and int(off["count"].sum()) == 3 * lights * carried.size


# ---- (F) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 300, 300), (64, 150, 150)])
def test_grid_stride_loops_wrap(gpu, shape):
    torch, brdf_amd, _ = gpu
    lights, H, W = shape
    cap = P.wide_capture(*shape)
    nf = cap["nf"]
    assert 3 * H * W * lights > P.GATHER_CAP
    plain = _plain(gpu, cap, 1)
    assert plain["n_pixels"] == H * W
    # every face's stored fit: its LAST pixel's three channels, fitted alone at n = L on the oracle's planes
    carried, last = P.last_pixels(cap["pixel_map"], nf)
    assert carried.size == nf
    g, _ = P.walk(cap["pixel_map"], nf)
    value = P.pixel_values(cap["images"], g[last])  # [nf,3,L]
    p, _, _ = brdf_amd.fit_batch(brdf_amd.METHOD_BC_DIF, 1, _dev(gpu, np.repeat(cap["ang"], 3, axis=0)), _dev(gpu, value.reshape(-1, lights) / 255.0),
                                 _dev(gpu, np.tile(np.array(P0), (3 * nf, 1))), lb=LB, ub=UB, itmax=100, opts=OPTS)
    torch.cuda.synchronize()
    assert plain["surfaces"].tobytes() == p.cpu().numpy().tobytes()
    off = _masked(gpu, cap, 1)  # the rule switched off
    _same_bytes(off, plain, ("surfaces", "avg", "covar", "stats", "rank"))
    assert off["n_pixels"] == H * W and np.all(off["count"] == lights)
    on = _masked(gpu, cap, 1, **RULE)
    counts = P.rule_valid(1, value, cap["ang"], **RULE).sum(axis=2).astype(np.int32)
    assert counts.min() < lights and counts.max() >= 3
    assert on["n_pixels"] == H * W and np.array_equal(on["count"], counts)


# ---- (G) ------------------------------------------------------------------------------------------------------------------------
def test_a_face_with_nan_cosines(gpu):
    """Observed on the MI355X: see the assertions at the end -- the masked and the per-face entry never take a NaN cosine for a sample,
    also with the rule switched off, and refuse the face's fits for their count of 0, where the unmasked capture runs the fit on the
    NaN planes."""
    cap = P.rule_capture(1, True)
    f, nf, without = cap["nan_face"], cap["nf"], cap["pixel_map_without"]
    others = np.arange(nf) != f
    p0 = np.array(P0)
    # the other faces have the bytes they have when the NaN face's pixels are background
    faces_on, faces_off = _faces(gpu, cap, 1, **RULE), _faces(gpu, cap, 1)
    _same_bytes(faces_on, _faces(gpu, cap, 1, pixel_map=without, **RULE), tuple(n for n in MAPS if n != "face_pixels"), rows=others)
    masked_on, masked_off, plain = _masked(gpu, cap, 1, **RULE), _masked(gpu, cap, 1), _plain(gpu, cap, 1)
    _same_bytes(masked_on, _masked(gpu, cap, 1, pixel_map=without, **RULE), MASKED_MAPS, rows=others)
    _same_bytes(plain, _plain(gpu, cap, 1, pixel_map=without), ("surfaces", "covar", "stats", "rank"), rows=others)
    for got in (faces_on, faces_off, masked_on, masked_off, plain):
        assert np.all(np.isfinite(got["avg"])), got["avg"]
    # the per-face entry on the NaN face: no sample, rule on or off
    for got in (faces_on, faces_off):
        assert got["face_pixels"][f] == 10 and not got["count"][f].any() and np.all(got["ret"][f] == -1) and not got["info"][f].any()
        assert np.all(got["surfaces"][f] == p0) and not got["rank"][f].any()
    # the masked capture with the rule switched off against the unmasked capture
    print("masked, rule off: surfaces", masked_off["surfaces"][f], "count", masked_off["count"][f], "stats", masked_off["stats"][f], "rank", masked_off["rank"][f])
    print("unmasked:         surfaces", plain["surfaces"][f], "stats", plain["stats"][f], "rank", plain["rank"][f])
    _same_bytes(masked_off, plain, ("surfaces", "covar", "stats", "rank"), rows=others)
    assert not masked_off["count"][f].any() and np.all(masked_off["surfaces"][f] == p0)  # refused: count 0, p0 stays
    assert not masked_off["stats"][f].any() and not masked_off["covar"][f].any() and not masked_off["rank"][f].any()  # sumsq = R2 = 0
    assert np.all(plain["surfaces"][f] == p0) and np.isnan(plain["stats"][f][:, 0]).all() and not plain["rank"][f].any()  # stopped: NaN sumsq
