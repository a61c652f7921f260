"""Per-fit sample counts, the part that needs no device: the argument checks of the ragged and masked entry points (every one
of them refuses what the host can see before any HIP call, as tests/test_abi.py checks for the older entries) and
brdf_amd.compact_samples against a plain loop."""
import ctypes as C

import numpy as np
import pytest

S, N = 4, 16


def _arrays():
    return (np.zeros(S * 3 * N), np.zeros(S * N), np.full(S, N, dtype=np.int32), np.tile([0.5, 1.0, 1.0], S), np.zeros(S * 10),
            np.zeros(S, dtype=np.int32))


def _v(a):
    return C.c_void_p(a.ctypes.data)


def _d(a):
    from brdf_amd._lib import D
    return a.ctypes.data_as(D)


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def test_ragged_fit_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import lib
    ang, x, cnt, p, info, ret = _arrays()

    def dev(method=1, model=1, a=ang, xx=x, c=cnt, s=S, n=N, pp=p):
        return lib.brdf_hip_fit_batch_ragged_dev(method, model, _v(a) if a is not None else None, _v(xx) if xx is not None else None,
                                                 _v(c) if c is not None else None, s, n, _v(pp) if pp is not None else None, None, None,
                                                 10, None, _v(info), _v(ret), None)

    def host(method=1, model=1, a=ang, xx=x, c=cnt, s=S, n=N, pp=p):
        return lib.brdf_hip_fit_batch_ragged(method, model, _d(a) if a is not None else None, _d(xx) if xx is not None else None,
                                             _i(c) if c is not None else None, s, n, _d(pp) if pp is not None else None, None, None, 10,
                                             None, _d(info), _i(ret))

    for call in (dev, host):
        for kw in (dict(a=None), dict(xx=None), dict(pp=None), dict(s=0), dict(s=-1), dict(n=0), dict(n=-3)):
            assert call(**kw) == -1, (call.__name__, kw)
            assert "null" in brdf_amd.last_error() or "bad arguments" in brdf_amd.last_error()
        for kw in (dict(model=3), dict(model=-1), dict(method=4), dict(method=-1)):
            assert call(**kw) == -1, (call.__name__, kw)
            assert "unknown model" in brdf_amd.last_error()
    # lb above ub is levmar's own refusal (lmbc_core.c:451-454), seen before anything is launched
    lb, ub = np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 1.0])
    rc = lib.brdf_hip_fit_batch_ragged_dev(1, 1, _v(ang), _v(x), _v(cnt), S, N, _v(p), _d(lb), _d(ub), 10, None, _v(info), _v(ret), None)
    assert rc == -1
    capfd.readouterr()


def test_ragged_stats_entries_refuse_bad_arguments_without_a_device():
    import brdf_amd
    from brdf_amd._lib import lib
    ang, x, cnt, p, _, rank = _arrays()
    covar, stats = np.zeros(S * 9), np.zeros(S * 8)

    def dev(method=1, model=1, a=ang, xx=x, s=S, n=N, pp=p, outs=True):
        return lib.brdf_hip_fit_stats_batch_ragged_dev(method, model, _v(a) if a is not None else None, _v(xx) if xx is not None else None,
                                                       _v(cnt), s, n, _v(pp) if pp is not None else None, None,
                                                       _v(covar) if outs else None, _v(stats) if outs else None, _v(rank) if outs else None,
                                                       None)

    def host(method=1, model=1, a=ang, xx=x, s=S, n=N, pp=p, outs=True):
        return lib.brdf_hip_fit_stats_batch_ragged(method, model, _d(a) if a is not None else None, _d(xx) if xx is not None else None,
                                                   _i(cnt), s, n, _d(pp) if pp is not None else None, None, _d(covar) if outs else None,
                                                   _d(stats) if outs else None, _i(rank) if outs else None)

    for call in (dev, host):
        for kw in (dict(a=None), dict(xx=None), dict(pp=None)):
            assert call(**kw) == -1 and "null" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(s=0), dict(n=0), dict(n=2), dict(n=-1)):  # (the stride itself must allow a covariance: n >= 3)
            assert call(**kw) == -1 and "need S > 0" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(model=3), dict(method=7)):
            assert call(**kw) == -1 and "unknown model" in brdf_amd.last_error(), (call.__name__, kw)
        assert call(outs=False) == -1 and "nothing to compute" in brdf_amd.last_error()
        assert call.__name__ and "ragged" in brdf_amd.last_error()  # the message names the entry point that was called


def test_masked_capture_refuses_bad_arguments_without_a_device():
    import brdf_amd
    from brdf_amd._lib import lib
    L, H, W, nf = 16, 2, 2, 1
    img = np.zeros(L * H * W * 3, dtype=np.uint8)
    pm = np.zeros(H * W, dtype=np.int32)
    vert, faces, nrm = np.zeros(9), np.zeros(3, dtype=np.int32), np.zeros(3)
    leds, view, p0, surf = np.zeros(L * 3), np.zeros(3), np.array([0.5, 1.0, 1.0]), np.zeros(nf * 9)

    def call(model=1, images=img, l=L, h=H, nfaces=nf, v_min=0, v_max=255, cos_min=0.0, pzero=p0):
        return lib.brdf_hip_fit_capture_masked_dev(model, _v(images) if images is not None else None, l, h, W, _v(pm), _v(vert), _v(faces),
                                                   _v(nrm), nfaces, _d(leds), _d(view), 1, _d(pzero) if pzero is not None else None, None, None,
                                                   10, None, _v(surf), None, None, None, None, None, None, v_min, v_max, cos_min, None)

    for kw in (dict(images=None), dict(pzero=None), dict(l=0), dict(l=65), dict(h=0), dict(nfaces=0)):
        assert call(**kw) == -1 and "brdf_hip_fit_capture_masked_dev(): bad arguments" in brdf_amd.last_error(), kw
    for kw in (dict(v_min=200, v_max=100), dict(v_min=1, v_max=0), dict(cos_min=float("nan")), dict(model=3), dict(model=-1)):
        assert call(**kw) == -1 and "bad validity rule" in brdf_amd.last_error(), kw


def _compact_loop(angles, x, valid):
    S_, _, n = angles.shape
    ao, xo, counts = np.full(angles.shape, np.nan), np.full(x.shape, np.nan), np.zeros(S_, dtype=np.int32)
    for s in range(S_):
        w = 0
        for i in range(n):
            if valid[s, i]:
                ao[s, :, w] = angles[s, :, i]
                xo[s, w] = x[s, i]
                w += 1
        counts[s] = w
    return ao, xo, counts


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_compact_samples_against_a_plain_loop(kind):
    import brdf_amd
    rng = np.random.default_rng(7)
    n = 16
    masks = [np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 0, np.arange(n) % 2 == 1, np.arange(n) >= 13, np.arange(n) < 2]
    masks += [rng.random(n) < q for q in (0.2, 0.5, 0.8)]
    valid = np.stack(masks)
    S_ = len(masks)
    angles, x = rng.random((S_, 3, n)), rng.random((S_, n))
    want = _compact_loop(angles, x, valid)
    if kind == "numpy":
        got = brdf_amd.compact_samples(angles, x, valid)
    else:
        import torch
        got = tuple(t.numpy() for t in brdf_amd.compact_samples(torch.from_numpy(angles), torch.from_numpy(x), torch.from_numpy(valid)))
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2])
    assert np.array_equal(got[2][:4], [n, 0, n // 2, n // 2])
    for g, w in zip(got[:2], want[:2]):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True)  # same values in the same places, NaN behind the count
    assert not np.shares_memory(got[0], angles) and np.array_equal(valid, np.stack(masks))  # the inputs are left alone
