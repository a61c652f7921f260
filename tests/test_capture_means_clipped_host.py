"""Sigma-clipped fits in the per-light-means capture, the part that needs no device:

  1. brdf_amd.clip_light_means -- one clip round of the definition as NumPy code -- on hand-made faces: the interval definition, the
     never-returns intersection over two rounds, the fewer-than-3-lights guard, the nothing-dropped settle, the k == 3 sigma, a NaN
     model value dropping its light;
  2. the interval argument, checked: on the brightened rule_capture the intervals keep exactly the samples that per-sample clipping
     (brdf_amd.clip_samples on group_capture_samples, same p, the twin's own sumsq) keeps, over two rounds, in every model;
  3. the entry is exported, declared and bound;
  4. it refuses the three clip arguments and L = 17 under its own name before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import capture_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "brdf_hip_fit_capture_means_clipped_dev"
OFF = dict(v_min=0, v_max=255, cos_min=-2.0)
HAND_P = np.array([0.6, 0.2, 4.0])  # Blinn-Phong
HAND = {0: np.array([0.5, 0.03, 4.0]), 1: HAND_P, 2: np.array([0.6, 0.05, 0.4])}


# ---- hand-made faces ---------------------------------------------------------------------------------------------------------------
def _hand_face(model, L, pixels, seed=7, p=HAND_P, planes=None):
    """one face (nf = 1) of `pixels` pixels in a 1 x pixels map under L lights: every channel shows round(255 f_l(p)) plus a
    deterministic -1 / 0 / +1 pattern; returns (images, pixel_map, face_angles [1,3,L], f [L])"""
    from brdf_amd import synth
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.45, 0.95, size=(1, 3, L)) if planes is None else planes
    with np.errstate(all="ignore"):
        f = synth.model_value(model, p, ang[0, 0], ang[0, 1], ang[0, 2])
    assert np.all((f > 0.08) & (f < 0.75) | np.isnan(f)), f
    base = np.round(255.0 * np.nan_to_num(f, nan=0.4)).astype(np.int64)  # [L]
    noise = (np.arange(pixels)[None, :] + np.arange(L)[:, None]) % 3 - 1  # [L, pixels]
    images = np.zeros((L, 1, pixels, 3), dtype=np.uint8)
    images[:, 0, :, :] = (base[:, None] + noise)[:, :, None]
    return images, np.zeros((1, pixels), dtype=np.int32), ang, f


def _sumsq(images, pm, ang, model, p, lo, hi, rule):
    """the full-sample sum of squares of every fit at p over its current sample set: sum_l c_l (m_l - f_l)^2 + within"""
    import brdf_amd
    from brdf_amd import synth
    lm = brdf_amd.capture_light_means(images, pm, ang, model, v_lo=lo, v_hi=hi, **rule)
    out = np.zeros(len(lm.k))
    for s in range(out.size):
        n = lm.counts[s]
        with np.errstate(all="ignore"):
            f = synth.model_value(model, p[s], lm.angles[s, 0, :n], lm.angles[s, 1, :n], lm.angles[s, 2, :n])
        out[s] = np.sum(lm.w[s, :n] * (lm.x[s, :n] - f) ** 2) + lm.within[s]
    return out, lm


def _brute_interval(f, thr, lo, hi):
    """the definition, level by level: the smallest and the largest v in [lo, hi] with |v / 255.0 - f| <= thr; (1, 0) if there is none"""
    ok = [v for v in range(int(lo), int(hi) + 1) if abs(v / 255.0 - f) <= thr]
    return (ok[0], ok[-1]) if ok else (1, 0)


def test_initial_intervals_are_the_rule():
    import brdf_amd
    ang = np.array([[[0.5, -0.1, 0.5, np.nan], [0.5, 0.5, -0.2, 0.5], [0.5, 0.5, 0.5, 0.5]]])  # light 1 fails plane 0, light 2 plane 1, light 3 is a NaN
    for model, ok in ((0, [1, 0, 1, 0]), (1, [1, 0, 0, 0]), (2, [1, 0, 0, 0])):  # Phong does not read plane 1
        lo, hi = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, v_min=1, v_max=254, cos_min=0.0)
        assert lo.dtype == hi.dtype == np.uint8 and lo.shape == (3, 4)
        assert np.array_equal(lo, np.tile(np.where(ok, 1, 1), (3, 1))) and np.array_equal(hi, np.tile(np.where(ok, 254, 0), (3, 1)))
    lo, hi = brdf_amd.initial_light_intervals(ang, [0], 0, v_min=-5, v_max=300, cos_min=-2.0)  # clamped to 0 ... 255; a NaN is never a sample
    assert list(lo[0]) == [0, 0, 0, 1] and list(hi[0]) == [255, 255, 255, 0]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_a_round_narrows_each_light_to_its_surviving_grey_levels(model):
    import brdf_amd
    p = HAND[model]
    images, pm, ang, f = _hand_face(model, 5, 40, p=p)
    images[0, 0, 3::10, :] += 60   # a highlight under light 0 on four pixels
    images[2, 0, 5::20, :] -= 50   # a shadow under light 2 on two
    pp = np.tile(p, (3, 1))
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    ss, lm = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    assert list(lm.k) == [200] * 3
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=2.5, sigma_min=1e-3, **OFF)
    assert lo.dtype == hi.dtype == np.uint8 and lo.shape == hi.shape == (3, 5) and not settled.any()
    thr = 2.5 * max(np.sqrt(ss[0] / 197.0), 1e-3)
    for s in range(3):
        for l in range(5):
            assert (lo[s, l], hi[s, l]) == _brute_interval(f[l], thr, 0, 255), (s, l)
    base = np.round(255.0 * f).astype(int)
    assert np.all(lo[0] <= base - 1) and np.all(hi[0] >= base + 1)        # the face's own values stay
    assert hi[0, 0] < base[0] + 59 and lo[0, 2] > base[2] - 49             # the planted ones go
    _, after = _sumsq(images, pm, ang, model, pp, lo, hi, OFF)
    assert list(after.k) == [194] * 3 and list(after.counts) == [5] * 3
    # the caller's arrays are not written
    assert np.all(lo0 == 0) and np.all(hi0 == 255)


def test_a_dropped_level_never_returns():
    import brdf_amd
    model = 1
    images, pm, ang, f = _hand_face(model, 5, 40)
    images[0, 0, 3::10, :] += 60
    images[1, 0, 7::10, :] -= 20   # survives round 1 (sigma holds the highlight), not round 2
    pp = np.tile(HAND_P, (3, 1))
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    ss, _ = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    lo1, hi1, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=2.5, sigma_min=1e-3, **OFF)
    assert not settled.any()
    # round 2 at a fit that moved UP by 0.04: its survivors alone would reach above round 1's upper ends
    p2 = pp.copy()
    p2[:, 0] += 0.04 / ang[0, 0].mean()
    from brdf_amd import synth
    f2 = synth.model_value(model, p2[0], ang[0, 0], ang[0, 1], ang[0, 2])
    ss2, lm2 = _sumsq(images, pm, ang, model, p2, lo1, hi1, OFF)
    lo2, hi2, settled2 = brdf_amd.clip_light_means(images, pm, ang, model, p2, ss2, np.zeros(3, dtype=int), lo1, hi1, kappa=1.5, sigma_min=1e-3, **OFF)
    assert not settled2.any()
    thr2 = 1.5 * max(np.sqrt(ss2[0] / (lm2.k[0] - 3.0)), 1e-3)
    beyond = 0
    for l in range(5):
        alone = _brute_interval(f2[l], thr2, 0, 255)
        assert (lo2[0, l], hi2[0, l]) == _brute_interval(f2[l], thr2, lo1[0, l], hi1[0, l])
        assert lo2[0, l] >= lo1[0, l] and hi2[0, l] <= hi1[0, l]
        beyond += alone[1] > hi1[0, l]
    assert beyond >= 3  # the intersection is what kept the upper ends


def test_a_clip_that_leaves_two_lights_is_not_applied():
    import brdf_amd
    model = 1
    images, pm, ang, _ = _hand_face(model, 4, 30)
    ang[0, 1, 3] = -0.5  # light 3 fails the rule: three lights carry samples
    rule = dict(v_min=1, v_max=254, cos_min=0.0)
    images[1, 0, :, :] += 70  # all of light 1 is far off
    pp = np.tile(HAND_P, (3, 1))
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **rule)
    assert list(lo0[0]) == [1, 1, 1, 1] and list(hi0[0]) == [254, 254, 254, 0]
    ss, lm = _sumsq(images, pm, ang, model, pp, lo0, hi0, rule)
    assert list(lm.counts) == [3] * 3
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=1.0, sigma_min=1e-3, **rule)
    assert settled.all() and np.array_equal(lo, lo0) and np.array_equal(hi, hi0)
    # with two far-off pixels instead of the whole light the clip stands
    images[1, 0, 2:, :] -= 70
    ss, _ = _sumsq(images, pm, ang, model, pp, lo0, hi0, rule)
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=2.0, sigma_min=1e-3, **rule)
    assert not settled.any() and hi[0, 1] < hi0[0, 1] and (lo[0, 3], hi[0, 3]) == (1, 0)


def test_a_round_that_drops_no_sample_settles_and_keeps_the_intervals():
    import brdf_amd
    model = 1
    images, pm, ang, _ = _hand_face(model, 5, 40)
    pp = np.tile(HAND_P, (3, 1))
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    ss, _ = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    # the threshold spans a dozen grey levels: levels go, samples do not
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=2.5, sigma_min=0.02, **OFF)
    assert settled.all() and np.array_equal(lo, lo0) and np.array_equal(hi, hi0)
    # ret < 0 and a sumsq that is not finite: settled, whatever the residuals
    images[0, 0, ::4, :] += 60
    ss, _ = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    bad = ss.copy()
    bad[1] = np.inf
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, bad, np.array([-1, 4, 4]), lo0, hi0, kappa=2.5, sigma_min=1e-3, **OFF)
    assert list(settled) == [True, True, False] and np.array_equal(lo[:2], lo0[:2]) and np.array_equal(hi[:2], hi0[:2]) and hi[2, 0] < 255
    # kappa = inf keeps every level and settles every fit
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=np.inf, sigma_min=0.0, **OFF)
    assert settled.all() and np.array_equal(lo, lo0) and np.array_equal(hi, hi0)


def test_three_samples_use_sigma_min():
    import brdf_amd
    model = 1
    pp = np.tile(HAND_P, (3, 1))
    # k == 3: one pixel under three lights.  sumsq / 0 is never formed; the clip to two lights is not applied
    images, pm, ang, _ = _hand_face(model, 3, 1)
    images[2, 0, 0, :] += 3
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    ss, lm = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    assert list(lm.k) == [3] * 3
    with np.errstate(all="raise"):
        lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=2.0, sigma_min=1e-3, **OFF)
    assert settled.all() and np.array_equal(hi, hi0)
    # k == 4: one pixel under four lights.  sigma = max(sqrt(sumsq / 1), sigma_min): at kappa = 0.7 the planted value goes, three lights stay
    images, pm, ang, f = _hand_face(model, 4, 1)
    images[2, 0, 0, :] += 8
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    ss, _ = _sumsq(images, pm, ang, model, pp, lo0, hi0, OFF)
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=0.7, sigma_min=1e-3, **OFF)
    assert not settled.any()
    thr = 0.7 * max(np.sqrt(ss[0] / 1.0), 1e-3)
    assert [(lo[0, l], hi[0, l]) for l in range(4)] == [_brute_interval(f[l], thr, 0, 255) for l in range(4)]
    _, after = _sumsq(images, pm, ang, model, pp, lo, hi, OFF)
    assert list(after.k) == [3] * 3
    # sigma_min above every residual: nothing dropped
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, ss, np.zeros(3, dtype=int), lo0, hi0, kappa=0.7, sigma_min=0.1, **OFF)
    assert settled.all()


def test_a_nan_model_value_drops_its_light():
    import brdf_amd
    model = 0  # Phong: pow(c2, n) of a negative cosine at n = 4.5 is a NaN; the rule switched off lets the light in
    p = np.array([0.5, 0.03, 4.5])
    planes = np.random.default_rng(7).uniform(0.45, 0.95, size=(1, 3, 5))
    planes[0, 2, 1] = -0.6
    images, pm, ang, f = _hand_face(model, 5, 20, p=p, planes=planes)
    assert np.isnan(f[1]) and np.isfinite(np.delete(f, 1)).all()
    pp = np.tile(p, (3, 1))
    lo0, hi0 = brdf_amd.initial_light_intervals(ang, [0, 0, 0], model, **OFF)
    assert (lo0[0, 1], hi0[0, 1]) == (0, 255)
    lo, hi, settled = brdf_amd.clip_light_means(images, pm, ang, model, pp, np.full(3, 0.01), np.zeros(3, dtype=int), lo0, hi0, kappa=3.0,
                                                sigma_min=1e-3, **OFF)
    assert not settled.any() and np.all(lo[:, 1] == 1) and np.all(hi[:, 1] == 0)
    assert np.all(hi[:, [0, 2, 3, 4]] >= lo[:, [0, 2, 3, 4]])
    lm = brdf_amd.capture_light_means(images, pm, ang, model, v_lo=lo, v_hi=hi, **OFF)
    assert list(lm.counts) == [4] * 3 and list(lm.k) == [80] * 3


def test_capture_light_means_without_intervals_is_unchanged():
    import brdf_amd
    cap = P.rule_capture(1)
    plain = brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], 1, **P.RULE)
    lo, hi = brdf_amd.initial_light_intervals(cap["ang"], plain.fit_face, 1, **P.RULE)
    under = brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], 1, v_lo=lo, v_hi=hi, **P.RULE)
    for a, b in zip(plain, under):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(Exception):
        brdf_amd.capture_light_means(cap["images"], cap["pixel_map"], cap["ang"], 1, v_lo=lo, **P.RULE)


# ---- the interval argument, checked -------------------------------------------------------------------------------------------------
def _samples_with_lights(cap, images, model, rule):
    """group_capture_samples' samples with the light and the grey level of each: (fit of sample, light, v), in the packed order"""
    nf, pm = cap["nf"], cap["pixel_map"]
    g, face = P.walk(pm, nf)
    order = np.argsort(face, kind="stable")
    g, face = g[order], face[order]
    vals = P.pixel_values(images, g)  # [P,3,L]
    valid = P.rule_valid(model, vals, cap["ang"][face], **rule)
    L = vals.shape[2]
    fit, light, grey = [], [], []
    for r, f in enumerate(np.unique(face)):
        rows = face == f
        for ch in range(3):
            ok = valid[rows, ch, :]  # [pixels, L]
            fit.append(np.full(int(ok.sum()), 3 * r + ch))
            light.append(np.broadcast_to(np.arange(L), ok.shape)[ok])
            grey.append(vals[rows, ch, :][ok])
    return np.concatenate(fit), np.concatenate(light), np.concatenate(grey)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_intervals_keep_what_per_sample_clipping_keeps(model):
    import brdf_amd
    from brdf_amd import synth
    from tests.test_gpu_capture_faces_clipped import _brightened
    cap = P.rule_capture(model)
    images, big = _brightened(cap, model)
    pm, ang, rule = cap["pixel_map"], cap["ang"], P.RULE
    a, x, off, fit_face, fit_channel, _ = brdf_amd.group_capture_samples(images, pm, ang, model, **rule)
    fit, light, grey = _samples_with_lights(cap, images, model, rule)
    assert np.array_equal(grey / 255.0, x) and np.array_equal(np.bincount(fit, minlength=len(fit_face)), np.diff(off))
    fits = len(fit_face)
    # the renderer's own parameters (tests.capture_problems.face_values): the model is linear in kd and ks
    p = np.array([np.array(synth.TRUTH[model]) * np.array([0.5 * (0.6 + 0.2 * ch)] * 2 + [1.0]) for ch in fit_channel])
    ret = np.where(np.diff(off) >= 3, 5, -1)
    lo, hi = brdf_amd.initial_light_intervals(ang, fit_face, model, **rule)
    keep = np.ones(x.size, dtype=bool)  # the per-sample side's cumulative mask, by the caller's sample position
    active = np.ones(fits, dtype=bool)
    dropped = 0
    for rnd in (1, 2):
        ss, lm = _sumsq(images, pm, ang, model, p, lo, hi, rule)
        assert np.array_equal(lm.k, np.bincount(fit[keep], minlength=fits))  # the two sides hold the same sets
        ret_now = np.where(lm.counts >= 3, ret, -1)  # (three samples under two lights: refused here, fitted there -- settled on both sides)
        nlo, nhi, settled = brdf_amd.clip_light_means(images, pm, ang, model, p, ss, ret_now, lo, hi, kappa=2.5, sigma_min=brdf_amd.SIGMA_MIN_8BIT,
                                                      **rule)
        # per sample: the current sets as a packed batch
        pos = np.flatnonzero(keep)
        cur_off = np.concatenate([[0], np.cumsum(np.bincount(fit[pos], minlength=fits))]).astype(np.int64)
        cur_a = np.concatenate([ang[fit_face[s]][:, light[pos[cur_off[s]:cur_off[s + 1]]]].reshape(-1) for s in range(fits)])
        k_keep, k_settled = brdf_amd.clip_samples(model, cur_a, x[pos], cur_off, p, ss, ret_now, kappa=2.5, sigma_min=brdf_amd.SIGMA_MIN_8BIT)
        # a clip that leaves 3 samples under fewer than 3 lights is applied per sample and not applied here: none in this fixture
        for s in np.flatnonzero(~k_settled):
            assert np.unique(light[pos[cur_off[s]:cur_off[s + 1]]][k_keep[cur_off[s]:cur_off[s + 1]]]).size >= 3, s
        for s in np.flatnonzero(~active):  # a settled fit is never looked at again
            nlo[s], nhi[s], settled[s], k_settled[s] = lo[s], hi[s], True, True
            k_keep[cur_off[s]:cur_off[s + 1]] = True
        assert np.array_equal(settled, k_settled), (rnd, np.flatnonzero(settled != k_settled))
        keep[pos] = k_keep
        by_interval = (grey >= nlo[fit, light]) & (grey <= nhi[fit, light])
        assert np.array_equal(by_interval, keep), (rnd, np.flatnonzero(by_interval != keep)[:10])
        dropped += int((~k_keep).sum())
        lo, hi = nlo, nhi
        active &= ~settled
    assert dropped > 0 and any(not keep[fit == 3 * r + ch].all() for r, f in enumerate(np.unique(fit_face)) if f in big for ch in range(3))


# ---- the entry ------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_declared_and_bound():
    import brdf_amd
    from brdf_amd._lib import ABI
    header = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    lib = C.CDLL(brdf_amd.LIB_PATH)
    assert hasattr(lib, ENTRY) and re.search(r"^int " + ENTRY + r"\(", header, flags=re.M) and ENTRY in ABI
    for name in ("fit_capture_means_clipped", "CaptureMeansClipped", "clip_light_means", "initial_light_intervals"):
        assert hasattr(brdf_amd, name), name
    assert brdf_amd.CaptureMeansClipped._fields[:10] == brdf_amd.CaptureMeans._fields
    assert brdf_amd.CaptureMeansClipped._fields[10:] == ("kept", "rounds", "vlo", "vhi")


def test_the_entry_refuses_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read: every call below is refused before anything touches memory
    ptr = C.c_void_p(buf.ctypes.data)
    dbl = buf.ctypes.data_as(D)
    p0, lb, ub = np.array([0.5, 1.0, 1.0]), np.zeros(3), np.full(3, 100.0)
    nan, inf = float("nan"), float("inf")

    def call(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, nf=10, p=p0, lo=lb, hi=ub, v_min=0, v_max=255, cos_min=-2.0, surfaces=ptr, kappa=2.5,
             sigma_min=0.0, rounds=2):
        d = lambda a: a.ctypes.data_as(D) if isinstance(a, np.ndarray) else a  # noqa: E731
        return lib.brdf_hip_fit_capture_means_clipped_dev(model, images, L, H_, W_, pm, ptr, ptr, ptr, nf, dbl, dbl, 1, d(p), d(lo), d(hi), 100, None,
                                                          v_min, v_max, cos_min, surfaces, None, None, None, None, None, None, None, None, None, None,
                                                          None, None, kappa, sigma_min, rounds, None, None, None, None)

    clip = [dict(kappa=0.0), dict(kappa=-2.0), dict(kappa=nan), dict(kappa=-inf), dict(sigma_min=-0.5), dict(sigma_min=nan), dict(sigma_min=-inf),
            dict(rounds=-1), dict(rounds=17)]
    for kw in clip:
        assert call(**kw) == -1, kw
        assert ENTRY + "()" in brdf_amd.last_error() and "need kappa > 0" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    for kw in (dict(L=17), dict(L=64), dict(L=0)):
        assert call(**kw) == -1, kw
        assert ENTRY + "()" in brdf_amd.last_error() and "need 1 <= L <= 16" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    # what brdf_hip_fit_capture_means_dev refuses, under this entry's name
    for kw in (dict(images=None), dict(pm=None), dict(p=None), dict(surfaces=None), dict(H_=0), dict(nf=0), dict(model=3), dict(v_min=200, v_max=100),
               dict(cos_min=nan), dict(lo=np.array([0.0, 2.0, 0.0]), hi=np.array([1.0, 1.0, 1.0]))):
        assert call(**kw) == -1, kw
        assert ENTRY + "()" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    capfd.readouterr()
