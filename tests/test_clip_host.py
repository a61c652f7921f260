"""Sigma-clipped fits, the part that needs no device: the four entry points are exported and declared, each refuses what the host can
see before any HIP call (never-read buffers, as tests/test_packed_host.py feeds the packed entries), and brdf_amd.clip_samples --
one clip round of the definition as NumPy code -- has the definition's properties."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4
OFFSETS = (0, 16, 16, 21, 40)
SYMBOLS = ("brdf_hip_fit_batch_packed_clipped_dev", "brdf_hip_fit_batch_packed_clipped", "brdf_hip_fit_capture_faces_clipped_dev",
           "brdf_hip_last_clip_stats")


def test_the_four_symbols_are_exported_and_declared():
    import brdf_amd
    header = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    lib = C.CDLL(brdf_amd.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
    from brdf_amd._lib import ABI
    assert set(SYMBOLS) <= set(ABI)
    # the header names what the clip does not cover
    for entry in ("brdf_hip_fit_capture_means_dev", "brdf_hip_fit_capture_masked_dev", "brdf_hip_fit_capture_single_faces_dev"):
        assert re.search(r"Not covered: clipping[^;]*" + entry, header, flags=re.S), entry
    assert lib.brdf_hip_last_clip_stats(0, None, None) == -1 and lib.brdf_hip_last_clip_stats(17, None, None) == -1
    assert isinstance(brdf_amd.last_clip_stats(), list)


def _v(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _d(a):
    from brdf_amd._lib import D
    return a.ctypes.data_as(D) if a is not None else None


def _ll(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong)) if a is not None else None


def test_packed_clipped_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import lib
    total = OFFSETS[-1]
    ang, x, off, p = np.zeros(3 * total), np.zeros(total), np.array(OFFSETS, dtype=np.int64), np.tile([0.5, 1.0, 1.0], S)
    lb, ub = np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 1.0])
    nan, inf = float("nan"), float("inf")

    def dev(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, lo=None, hi=None, ws=0, kappa=2.5, sigma_min=0.001, rounds=3):
        return lib.brdf_hip_fit_batch_packed_clipped_dev(method, model, _v(a), _v(xx), _v(o), s, _v(pp), _d(lo), _d(hi), 10, None, kappa, sigma_min, rounds,
                                                         None, None, None, None, None, None, None, None, ws, None)

    def host(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, lo=None, hi=None, ws=0, kappa=2.5, sigma_min=0.001, rounds=3):
        return lib.brdf_hip_fit_batch_packed_clipped(method, model, _d(a), _d(xx), _ll(o), s, _d(pp), _d(lo), _d(hi), 10, None, kappa, sigma_min, rounds,
                                                     None, None, None, None, None, None, None, None, ws)

    for call, name in ((dev, SYMBOLS[0]), (host, SYMBOLS[1])):
        for kw in (dict(a=None), dict(xx=None), dict(o=None), dict(pp=None)):
            assert call(**kw) == -1 and "null" in brdf_amd.last_error(), (name, kw)
        for kw in (dict(s=0), dict(s=-1), dict(ws=-1)):
            assert call(**kw) == -1 and "need S > 0" in brdf_amd.last_error(), (name, kw)
        for kw in (dict(model=3), dict(model=-1), dict(method=4), dict(method=-1)):
            assert call(**kw) == -1 and "unknown model" in brdf_amd.last_error(), (name, kw)
        assert call(lo=lb, hi=ub) == -1 and "lower bound exceeds" in brdf_amd.last_error(), name
        for kw in (dict(kappa=0.0), dict(kappa=-1.0), dict(kappa=nan), dict(kappa=-inf), dict(sigma_min=-1e-300), dict(sigma_min=nan),
                   dict(sigma_min=-inf), dict(rounds=-1), dict(rounds=17)):
            assert call(**kw) == -1 and "need kappa > 0" in brdf_amd.last_error(), (name, kw)
            assert name + "()" in brdf_amd.last_error(), (name, brdf_amd.last_error())  # the entry's own name
    assert host(o=np.array([0, 16, 12, 21, 40], dtype=np.int64)) == -1 and "offsets decrease at fit 1" in brdf_amd.last_error()
    assert host(o=np.array([0, 16, 16, 21, 21 + 2 ** 31], dtype=np.int64)) == -1 and "more than INT_MAX" in brdf_amd.last_error()
    capfd.readouterr()


def test_capture_faces_clipped_entry_refuses_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read: every call below is refused before anything touches memory
    ptr = C.c_void_p(buf.ctypes.data)
    dbl = buf.ctypes.data_as(D)
    p0, lb, ub = np.array([0.5, 1.0, 1.0]), np.zeros(3), np.full(3, 100.0)
    nan = float("nan")

    def call(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, vertices=ptr, faces=ptr, normals=ptr, nf=10, leds=dbl, view=dbl, p=p0, lo=lb, hi=ub,
             v_min=0, v_max=255, cos_min=-2.0, ws=0, surfaces=ptr, kappa=2.5, sigma_min=0.0, rounds=2):
        d = lambda a: a.ctypes.data_as(D) if isinstance(a, np.ndarray) else a  # noqa: E731
        return lib.brdf_hip_fit_capture_faces_clipped_dev(model, images, L, H_, W_, pm, vertices, faces, normals, nf, leds, view, 1, d(p), d(lo), d(hi),
                                                          100, None, v_min, v_max, cos_min, ws, surfaces, None, None, None, None, None, None, None,
                                                          None, None, None, None, kappa, sigma_min, rounds, None, None)

    refused = [dict(images=None), dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None),
               dict(p=None), dict(surfaces=None), dict(L=0), dict(L=65), dict(L=-1), dict(H_=0), dict(W_=-2), dict(nf=0), dict(nf=-1),
               dict(nf=(2 ** 31 - 1) // 3 + 1), dict(model=3), dict(model=-1), dict(v_min=200, v_max=100), dict(cos_min=nan), dict(ws=-1),
               dict(lo=np.array([0.0, 2.0, 0.0]), hi=np.array([1.0, 1.0, 1.0])),  # what brdf_hip_fit_capture_faces_dev refuses
               dict(kappa=0.0), dict(kappa=nan), dict(kappa=-2.0), dict(sigma_min=-0.5), dict(sigma_min=nan), dict(rounds=-1), dict(rounds=17)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert SYMBOLS[2] + "()" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert "need kappa > 0" in brdf_amd.last_error()
    capfd.readouterr()


# ---- clip_samples: one clip round of the definition ----
def _batch(counts, model=1, seed=5):
    """fits on the model's own values at p (residual 0) -- the tests plant what they need"""
    from brdf_amd import synth
    rng = np.random.default_rng(seed)
    p = np.tile(np.array(synth.TRUTH[model]), (len(counts), 1))
    angles, x, offsets = [], [], [7]  # offsets[0] != 0: the mask is by position offsets[s] - offsets[0] + i
    for s, k in enumerate(counts):
        a = rng.uniform(0.2, 1.0, size=(3, k))
        angles.append(a.reshape(-1))
        x.append(synth.model_value(model, p[s], a[0], a[1], a[2]))
        offsets.append(offsets[-1] + k)
    pad = np.full(7, np.nan)
    return np.concatenate([np.tile(pad, 3)] + angles), np.concatenate([pad] + x), np.array(offsets, dtype=np.int64), p


def _sumsq(model, angles, x, offsets, p):
    from brdf_amd import synth
    out = np.zeros(len(offsets) - 1)
    for s in range(len(out)):
        o, k = offsets[s], offsets[s + 1] - offsets[s]
        a = angles[3 * o:3 * o + 3 * k].reshape(3, k)
        out[s] = np.sum((x[o:o + k] - synth.model_value(model, p[s], a[0], a[1], a[2])) ** 2)
    return out


def test_clip_samples_drops_what_lies_beyond_kappa_sigma():
    import brdf_amd
    for model in (0, 1, 2):
        angles, x, offsets, p = _batch([40, 12], model)
        x[offsets[0] + 5] += 0.3
        x[offsets[0] + 17] -= 0.2
        x[offsets[1] + 3] += 1e-4  # inside sigma_min's band
        ss = _sumsq(model, angles, x, offsets, p)
        keep, settled = brdf_amd.clip_samples(model, angles, x, offsets, p, ss, np.array([5, 5]), kappa=2.5, sigma_min=1e-3)
        want = np.ones(52, dtype=bool)
        want[[5, 17]] = False
        assert keep.dtype == bool and np.array_equal(keep, want) and list(settled) == [False, True]
        # sigma is sqrt(sumsq / (k - 3)) with the outliers in it: 0.059, so a kappa of 4 keeps the smaller one
        keep, settled = brdf_amd.clip_samples(model, angles, x, offsets, p, ss, np.array([5, 5]), kappa=4.0, sigma_min=1e-3)
        want[17] = True
        assert np.array_equal(keep, want) and list(settled) == [False, True]
        # kappa = inf keeps everything and settles every fit
        keep, settled = brdf_amd.clip_samples(model, angles, x, offsets, p, ss, np.array([5, 5]), kappa=np.inf, sigma_min=0.0)
        assert keep.all() and settled.all()


def test_clip_samples_uses_sigma_min_for_three_samples():
    import brdf_amd
    angles, x, offsets, p = _batch([3, 4, 3])
    x[offsets[0] + 1] += 0.01
    x[offsets[1] + 1] += 0.01
    x[offsets[2] + 2] += 0.01
    ss = _sumsq(1, angles, x, offsets, p)
    # k == 3: sumsq / 0 is never formed, sigma = sigma_min -- and the clip to 2 survivors is not applied, the fit is settled
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.zeros(3, dtype=int), kappa=2.0, sigma_min=1e-3)
    assert keep[:3].all() and keep[7:].all() and settled[0] and settled[2]
    # k == 4: sigma = max(sqrt(sumsq / 1), sigma_min) = 0.01 -> |e| = 0.01 <= 2 * 0.01, nothing dropped, settled
    assert keep[3:7].all() and settled[1]
    # with kappa below 1 the k == 4 fit drops its sample and keeps 3: applied
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.zeros(3, dtype=int), kappa=0.5, sigma_min=1e-3)
    assert list(keep[3:7]) == [True, False, True, True] and not settled[1]
    assert keep[:3].all() and settled[0]  # 2 survivors: not applied
    # k == 3 with sigma_min above the residual: nothing dropped
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.zeros(3, dtype=int), kappa=2.0, sigma_min=0.006)
    assert keep.all() and settled.all()


def test_clip_samples_does_not_apply_a_clip_to_fewer_than_three_survivors():
    import brdf_amd
    angles, x, offsets, p = _batch([6, 6])
    x[offsets[0]:offsets[0] + 4] += np.array([0.5, -0.5, 0.5, -0.5])  # 2 survivors at a small kappa
    x[offsets[1]:offsets[1] + 3] += np.array([0.5, -0.5, 0.5])        # 3 survivors
    ss = _sumsq(1, angles, x, offsets, p)
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.array([1, 1]), kappa=0.5, sigma_min=0.0)
    assert keep[:6].all() and settled[0]
    assert list(keep[6:]) == [False, False, False, True, True, True] and not settled[1]


def test_clip_samples_leaves_failed_fits_and_bad_sums_alone_and_drops_nan_residuals():
    import brdf_amd
    angles, x, offsets, p = _batch([10, 10, 10, 10])
    for s in range(4):
        x[offsets[s] + 2] += 0.4
    x[offsets[3] + 7] = np.nan  # a NaN residual fails the comparison
    ss = _sumsq(1, angles, x, offsets, p)
    assert np.isnan(ss[3])
    ss[2] = np.inf
    ss[3] = 0.16  # (what a caller's statistics would not give: the twin looks at the residual itself)
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.array([-1, 3, 3, 3]), kappa=2.0, sigma_min=0.0)
    assert keep[:10].all() and settled[0]       # ret < 0: settled untouched
    assert not keep[12] and keep[10:20].sum() == 9 and not settled[1]
    assert keep[20:30].all() and settled[2]     # a sumsq that is not finite: settled, nothing clipped
    assert not keep[37] and not keep[32] and keep[30:].sum() == 8 and not settled[3]


def test_clip_samples_handles_empty_fits_anywhere_in_the_batch():
    import brdf_amd
    counts = [0, 8, 0, 0, 9, 0]
    angles, x, offsets, p = _batch(counts)
    x[offsets[1] + 1] += 0.3
    x[offsets[4] + 8] += 0.3
    ss = _sumsq(1, angles, x, offsets, p)
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.array([-1, 4, -1, -1, 4, -1]), kappa=2.0, sigma_min=0.0)
    want = np.ones(17, dtype=bool)
    want[[1, 16]] = False
    assert np.array_equal(keep, want) and list(settled) == [True, False, True, True, False, True]
    # empty fits with ret >= 0 (a caller's mistake) are settled as well: k < 3
    keep, settled = brdf_amd.clip_samples(1, angles, x, offsets, p, ss, np.zeros(6, dtype=int), kappa=2.0, sigma_min=0.0)
    assert np.array_equal(keep, want) and list(settled) == [True, False, True, True, False, True]
    # a batch of nothing but empty fits
    keep, settled = brdf_amd.clip_samples(1, np.zeros(0), np.zeros(0), np.zeros(3, dtype=np.int64), np.zeros((2, 3)), np.zeros(2), np.zeros(2, dtype=int),
                                          kappa=2.0, sigma_min=0.0)
    assert keep.size == 0 and settled.all()
