"""Packed batches, the part that needs no device: the plan arithmetic (brdf_amd/csrc/packed_plan.h) in a stand-alone C++ program
built here with the sanitizers of the host compiler, the argument checks of the four packed entry points (every one refuses what
the host can see before any HIP call, as tests/test_ragged_host.py checks for the ragged entries) and brdf_amd.pack_samples
against a plain loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4
OFFSETS = (0, 16, 16, 21, 40)


def test_plan_arithmetic_under_the_sanitizers(tmp_path):
    """class of every count at every seam, chunk sizes for 1 byte, one fit's bytes exactly and one byte less than two fits'"""
    exe = tmp_path / "packed_plan_harness"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "packed_plan_harness.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr
    for k, cls in ((0, 0), (16, 0), (17, 1), (64, 1), (65, 2), (256, 2), (257, 3), (1024, 3), (1025, 4), (4096, 4), (4097, 5), (2 ** 31 - 1, 5)):
        assert f"class({k}) = {cls}\n" in run.stdout


def _arrays():
    total = OFFSETS[-1]
    return (np.zeros(3 * total), np.zeros(total), np.array(OFFSETS, dtype=np.int64), np.tile([0.5, 1.0, 1.0], S), np.zeros(S * 10),
            np.zeros(S, dtype=np.int32))


def _v(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _d(a):
    from brdf_amd._lib import D
    return a.ctypes.data_as(D) if a is not None else None


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None


def _ll(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong)) if a is not None else None


def test_packed_fit_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import lib
    ang, x, off, p, info, ret = _arrays()
    lb, ub = np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 1.0])

    def dev(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, lo=None, hi=None, ws=0):
        return lib.brdf_hip_fit_batch_packed_dev(method, model, _v(a), _v(xx), _v(o), s, _v(pp), _d(lo), _d(hi), 10, None, _v(info), _v(ret), ws, None)

    def host(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, lo=None, hi=None, ws=0):
        return lib.brdf_hip_fit_batch_packed(method, model, _d(a), _d(xx), _ll(o), s, _d(pp), _d(lo), _d(hi), 10, None, _d(info), _i(ret), ws)

    for call in (dev, host):
        for kw in (dict(a=None), dict(xx=None), dict(o=None), dict(pp=None)):
            assert call(**kw) == -1 and "null" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(s=0), dict(s=-1), dict(ws=-1)):
            assert call(**kw) == -1 and "need S > 0" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(model=3), dict(model=-1), dict(method=4), dict(method=-1)):
            assert call(**kw) == -1 and "unknown model" in brdf_amd.last_error(), (call.__name__, kw)
        # lb above ub is levmar's own refusal (lmbc_core.c:451-454), seen before anything is launched
        assert call(lo=lb, hi=ub) == -1 and "lower bound exceeds" in brdf_amd.last_error(), call.__name__
        assert "packed" in brdf_amd.last_error()  # the message names the entry point that was called
    # what only the host-pointer entry can see: offsets that decrease, a single count above INT_MAX
    assert host(o=np.array([0, 16, 12, 21, 40], dtype=np.int64)) == -1 and "offsets decrease at fit 1" in brdf_amd.last_error()
    assert host(o=np.array([0, 16, 16, 21, 21 + 2 ** 31], dtype=np.int64)) == -1 and "more than INT_MAX" in brdf_amd.last_error()
    capfd.readouterr()


def test_packed_stats_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import lib
    ang, x, off, p, _, rank = _arrays()
    covar, stats = np.zeros(S * 9), np.zeros(S * 8)

    def dev(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, outs=True, ws=0):
        return lib.brdf_hip_fit_stats_batch_packed_dev(method, model, _v(a), _v(xx), _v(o), s, _v(pp), None, _v(covar) if outs else None,
                                                       _v(stats) if outs else None, _v(rank) if outs else None, ws, None)

    def host(method=1, model=1, a=ang, xx=x, o=off, s=S, pp=p, outs=True, ws=0):
        return lib.brdf_hip_fit_stats_batch_packed(method, model, _d(a), _d(xx), _ll(o), s, _d(pp), None, _d(covar) if outs else None,
                                                   _d(stats) if outs else None, _i(rank) if outs else None, ws)

    for call in (dev, host):
        for kw in (dict(a=None), dict(xx=None), dict(o=None), dict(pp=None)):
            assert call(**kw) == -1 and "null" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(s=0), dict(s=-2), dict(ws=-5)):
            assert call(**kw) == -1 and "need S > 0" in brdf_amd.last_error(), (call.__name__, kw)
        for kw in (dict(model=3), dict(method=7)):
            assert call(**kw) == -1 and "unknown model" in brdf_amd.last_error(), (call.__name__, kw)
        assert call(outs=False) == -1 and "nothing to compute" in brdf_amd.last_error()
        assert "stats_batch_packed" in brdf_amd.last_error()
    assert host(o=np.array([5, 4, 16, 21, 40], dtype=np.int64)) == -1 and "offsets decrease at fit 0" in brdf_amd.last_error()
    assert host(o=np.array([0, 2 ** 31, 2 ** 31, 2 ** 31, 2 ** 31], dtype=np.int64)) == -1 and "more than INT_MAX" in brdf_amd.last_error()
    capfd.readouterr()


def test_last_packed_stats_knows_six_classes():
    import brdf_amd
    from brdf_amd._lib import lib
    assert lib.brdf_hip_last_packed_stats(-1, None, None, None) == -1 and lib.brdf_hip_last_packed_stats(6, None, None, None) == -1
    assert all(lib.brdf_hip_last_packed_stats(c, None, None, None) == 0 for c in range(6))
    assert len(brdf_amd.last_packed_stats()) == 6


def _pack_loop(angles, x, counts):
    S_, _, n = angles.shape
    pa, px, offsets = [], [], [0]
    for s in range(S_):
        k = min(max(int(counts[s]), 0), n)
        for plane in range(3):
            for i in range(k):
                pa.append(angles[s, plane, i])
        for i in range(k):
            px.append(x[s, i])
        offsets.append(offsets[-1] + k)
    return np.array(pa, dtype=np.float64), np.array(px, dtype=np.float64), np.array(offsets, dtype=np.int64)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_pack_samples_against_a_plain_loop(kind):
    import brdf_amd
    rng = np.random.default_rng(11)
    n = 16
    counts = np.array([n, 0, 5, 0, 1, n, 3, 15, 0], dtype=np.int32)  # counts of 0 and of the full stride, at the ends and next to each other
    S_ = len(counts)
    angles, x = rng.random((S_, 3, n)), rng.random((S_, n))
    for s, k in enumerate(counts):  # NaN padding behind every count: it must not travel
        angles[s, :, k:], x[s, k:] = np.nan, np.nan
    want = _pack_loop(angles, x, counts)
    if kind == "numpy":
        got = brdf_amd.pack_samples(angles, x, counts)
    else:
        import torch
        got = tuple(t.numpy() for t in brdf_amd.pack_samples(torch.from_numpy(angles), torch.from_numpy(x), torch.from_numpy(counts)))
    total = int(counts.sum())
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]) and got[2][-1] == total
    assert got[0].dtype == np.float64 and got[0].shape == (3 * total,) and got[1].shape == (total,)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    # fit s's segment is the single-fit layout: planes [3][k] at 3 * offsets[s], measurements at offsets[s]
    for s, k in enumerate(counts):
        o = got[2][s]
        assert np.array_equal(got[0][3 * o:3 * o + 3 * k].reshape(3, k), angles[s, :, :k]) and np.array_equal(got[1][o:o + k], x[s, :k])
    # the round trip of compact_samples -> pack_samples keeps the valid samples, in order
    valid = rng.random((S_, n)) < 0.5
    full_a, full_x = rng.random((S_, 3, n)), rng.random((S_, n))
    ca, cx, cc = brdf_amd.compact_samples(full_a, full_x, valid)
    pa, px, po = brdf_amd.pack_samples(ca, cx, cc)
    assert np.array_equal(px, full_x[valid]) and np.array_equal(np.diff(po), valid.sum(axis=1))
    # a count outside [0, n] is clipped
    assert np.array_equal(brdf_amd.pack_samples(full_a[:2], full_x[:2], np.array([-3, n + 9]))[2], [0, 0, n])
