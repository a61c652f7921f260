"""brdf_hip_fit_batch_multi: one batch over several GPUs through the C ABI.

CPU tests: the ABI (header, export, Python table), the argument checks that come before any HIP call, and a C++ caller
that compiles and links against the header and the library.  GPU tests (one MI355X is enough: a device may be listed more
than once): every fit's p, info, ret and the return value are bit-identical to brdf_hip_fit_batch on one device, the
shards follow dist.shard_range, errors leave the caller's arrays alone, the calling thread's device and counters are not
touched, concurrent callers and the C++ caller get the single-device bits."""
import ctypes as C
import functools
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from brdf_amd import dist, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_ERROR = -1
CALLER = os.path.join(ROOT, "tests", "cpp", "multi_device_caller.cpp")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd


def _ptr(a, ctype=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _devices(devices):
    return (None, 0) if devices is None else ((C.c_int * max(1, len(devices)))(*devices), len(devices))


@functools.lru_cache(maxsize=None)
def _inputs(model, n, S):
    angles, x, _ = synth.make_surfels(model, n, first=0, count=S)
    return angles, x, np.tile(np.array(synth.P0[model]), (S, 1))


def _call(lib, method, model, angles, x, p0, devices=None, multi=True):
    """one raw C call: (return value, p, info, ret)"""
    S, n = x.shape
    p, info, ret = p0.copy(), np.zeros((S, 10)), np.zeros(S, dtype=np.int32)
    lb, ub, opts = np.array(synth.LB), np.array(synth.UB), np.array(synth.OPTS)
    args = [method, model, _ptr(angles), _ptr(x), S, n, _ptr(p), _ptr(lb), _ptr(ub), synth.ITMAX, _ptr(opts), _ptr(info), _ptr(ret, C.c_int)]
    rc = lib.brdf_hip_fit_batch_multi(*args, *_devices(devices)) if multi else lib.brdf_hip_fit_batch(*args)
    return rc, p, info, ret


def _assert_same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _compile_caller(out_dir):
    exe = os.path.join(str(out_dir), "multi_device_caller")
    lib_dir = os.path.join(ROOT, "brdf_amd")
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, CALLER, "-L" + lib_dir, "-lbrdf_hip",
           "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_multi_symbols_are_declared_exported_and_bound():
    import brdf_amd
    from brdf_amd._lib import ABI
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brdf_levmar.h")).read(), flags=re.S)
    lib = C.CDLL(brdf_amd.LIB_PATH)
    for name in ("brdf_hip_fit_batch_multi", "brdf_hip_last_multi_stats"):
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in ABI
    assert brdf_amd.fit_batch_multi and brdf_amd.last_multi_stats


def test_multi_argument_errors_need_no_gpu(capfd):
    """every argument error returns LM_ERROR with a message before any HIP call, and leaves p as it was"""
    import brdf_amd
    from brdf_amd._lib import lib
    S, n = 4, 16
    angles, x, p = np.zeros((S, 3, n)), np.zeros((S, n)), np.full((S, 3), 0.5)
    keep = p.copy()
    one = (C.c_int * 1)(0)
    many = (C.c_int * 65)(*([0] * 65))

    def call(a=angles, xx=x, pp=p, s=S, nn=n, devices=one, ndev=1, method=1, model=1):
        return lib.brdf_hip_fit_batch_multi(method, model, _ptr(a), _ptr(xx), s, nn, _ptr(pp), None, None, 100, None, None, None,
                                            devices, ndev)

    cases = [dict(a=None), dict(xx=None), dict(pp=None), dict(s=0), dict(s=-3), dict(nn=0), dict(nn=-1), dict(ndev=0),
             dict(ndev=-2), dict(devices=many, ndev=65), dict(model=3), dict(method=7)]
    for kw in cases:
        assert call(**kw) == LM_ERROR, kw
        msg = brdf_amd.last_error()
        assert msg.startswith("brdf_hip_fit_batch_multi(): "), (kw, msg)
        assert np.array_equal(p, keep)
    assert call(devices=many, ndev=65) == LM_ERROR and "ndev = 65" in brdf_amd.last_error()
    # a bad call leaves no shards behind; out-of-range shards are refused
    d, f, c, ms = C.c_int(7), C.c_longlong(0), C.c_longlong(0), (C.c_double * 3)()
    assert lib.brdf_hip_last_multi_stats(-1, C.byref(d), C.byref(f), C.byref(c), ms) == LM_ERROR
    assert lib.brdf_hip_last_multi_stats(0, C.byref(d), C.byref(f), C.byref(c), ms) == LM_ERROR
    assert d.value == 7
    assert brdf_amd.last_multi_stats() == []
    with pytest.raises(ValueError):
        brdf_amd.fit_batch_multi(1, 1, angles[:, :2], x, p)
    with pytest.raises(RuntimeError, match="brdf_hip_fit_batch_multi"):
        brdf_amd.fit_batch_multi(1, 1, angles, x, p, devices=[])
    capfd.readouterr()


def test_cpp_caller_compiles_and_links(tmp_path):
    exe = _compile_caller(tmp_path)
    assert os.access(exe, os.X_OK)


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 256, 4096])
@pytest.mark.parametrize("model", [1, 2])  # Blinn-Phong, Ward
@pytest.mark.parametrize("method", [0, 1])
def test_multi_is_bit_identical_to_one_device(gpu, method, model, n):
    """S = 1001 fits (ragged shards) on [0], [0,0], [0,0,0]: p, info, ret and the return value of brdf_hip_fit_batch"""
    _, brdf_amd = gpu
    angles, x, p0 = _inputs(model, n, 1001)
    ref = _call(brdf_amd.lib, method, model, angles, x, p0, multi=False)
    assert ref[0] != LM_ERROR, brdf_amd.last_error()
    for devices in ([0], [0, 0], [0, 0, 0]):
        got = _call(brdf_amd.lib, method, model, angles, x, p0, devices)
        _assert_same(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
def test_multi_large_fits_and_empty_shard(gpu, method):
    """n = 5000 (one fit after the other, each over the whole chip): S = 3 on [0,0], S = 2 on [0,0,0] (an empty shard)"""
    _, brdf_amd = gpu
    model, n = 2, 5000
    for S, devices in ((3, [0, 0]), (2, [0, 0, 0])):
        angles, x, p0 = _inputs(model, n, S)
        ref = _call(brdf_amd.lib, method, model, angles, x, p0, multi=False)
        assert ref[0] != LM_ERROR, brdf_amd.last_error()
        _assert_same(_call(brdf_amd.lib, method, model, angles, x, p0, devices), ref)
        stats = brdf_amd.last_multi_stats()
        assert [(s["first"], s["count"]) for s in stats] == [dist.shard_range(S, k, len(devices)) for k in range(len(devices))]
        assert all(s["device"] == 0 for s in stats)
        assert all(s["fit_ms"] > 0 for s in stats if s["count"] > 0)
        assert all(s["upload_ms"] == s["fit_ms"] == s["download_ms"] == 0 for s in stats if s["count"] == 0)


@pytest.mark.gpu
def test_multi_default_devices_and_shard_stats(gpu):
    """devices=None: every visible device once; the stats follow dist.shard_range and name the listed device"""
    torch, brdf_amd = gpu
    model, n, S, method = 1, 16, 1001, 1
    angles, x, p0 = _inputs(model, n, S)
    ref = _call(brdf_amd.lib, method, model, angles, x, p0, multi=False)
    count = brdf_amd.lib.brdf_hip_device_count()
    assert count == torch.cuda.device_count() >= 1
    _assert_same(_call(brdf_amd.lib, method, model, angles, x, p0, None), ref)
    stats = brdf_amd.last_multi_stats()
    assert [s["device"] for s in stats] == list(range(count))
    assert [(s["first"], s["count"]) for s in stats] == [dist.shard_range(S, k, count) for k in range(count)]
    # the Python wrapper: same bits, p0 untouched
    keep = p0.copy()
    p, info, ret = brdf_amd.fit_batch_multi(method, model, angles, x, p0, devices=[0, 0, 0], lb=synth.LB, ub=synth.UB,
                                            itmax=synth.ITMAX, opts=synth.OPTS)
    assert np.array_equal(p0, keep)
    assert np.array_equal(p, ref[1]) and np.array_equal(info, ref[2]) and np.array_equal(ret, ref[3])
    stats = brdf_amd.last_multi_stats()
    assert [(s["device"], s["first"], s["count"]) for s in stats] == [(0,) + dist.shard_range(S, k, 3) for k in range(3)]
    assert all(s["fit_ms"] > 0 and s["upload_ms"] >= 0 and s["download_ms"] >= 0 for s in stats)


@pytest.mark.gpu
def test_multi_bad_ordinal_leaves_p_untouched(gpu, capfd):
    torch, brdf_amd = gpu
    model, n, S, method = 1, 16, 64, 1
    angles, x, p0 = _inputs(model, n, S)
    bad = torch.cuda.device_count() + 3
    rc, p, info, ret = _call(brdf_amd.lib, method, model, angles, x, p0, [0, bad])
    assert rc == LM_ERROR
    assert f"devices[1] = {bad}" in brdf_amd.last_error()
    assert np.array_equal(p, p0) and not info.any() and not ret.any()
    assert brdf_amd.last_multi_stats() == []
    with pytest.raises(RuntimeError, match=str(bad)):
        brdf_amd.fit_batch_multi(method, model, angles, x, p0, devices=[bad])
    capfd.readouterr()


@pytest.mark.gpu
def test_multi_leaves_the_callers_device_and_counters_alone(gpu):
    """the calling thread's current device and its brdf_hip_last_fit_stats (of a brdf_hip_fit_dev made just before) are
    what they were, also after a multi call whose workers ran single fits of their own (n > 4096)"""
    torch, brdf_amd = gpu
    cur = torch.cuda.device_count() - 1
    torch.cuda.set_device(cur)
    dev = torch.device("cuda", cur)
    a1, x1 = synth.make_single(2, 20000)[:2]
    res = brdf_amd.fit_single(0, 2, torch.from_numpy(a1).to(dev), torch.from_numpy(x1).to(dev), synth.P0[2], itmax=synth.ITMAX,
                              opts=synth.OPTS)
    assert res.ret >= 0
    before = brdf_amd.last_fit_stats()
    angles, x, p0 = _inputs(2, 5000, 3)
    assert _call(brdf_amd.lib, 0, 2, angles, x, p0, [0, 0])[0] != LM_ERROR
    angles, x, p0 = _inputs(1, 256, 1001)
    assert _call(brdf_amd.lib, 1, 1, angles, x, p0, [0])[0] != LM_ERROR
    assert torch.cuda.current_device() == cur
    assert brdf_amd.last_fit_stats() == before
    torch.cuda.set_device(0)


@pytest.mark.gpu
def test_multi_concurrent_callers(gpu):
    """two Python threads (ctypes releases the GIL) call fit_batch_multi at the same time on different inputs"""
    _, brdf_amd = gpu
    jobs = [(1, 1, 16, 0, 3000), (0, 2, 256, 5000, 800)]  # method, model, n, first surfel, S
    inputs = []
    for method, model, n, first, S in jobs:
        angles, x, _ = synth.make_surfels(model, n, first=first, count=S)
        inputs.append((method, model, angles, x, np.tile(np.array(synth.P0[model]), (S, 1))))
    kw = dict(devices=[0, 0], lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS)
    serial = [brdf_amd.fit_batch_multi(*job, **kw) for job in inputs]
    barrier = threading.Barrier(len(inputs))
    out, errors = [None] * len(inputs), []

    def run(i):
        try:
            barrier.wait()
            out[i] = brdf_amd.fit_batch_multi(*inputs[i], **kw)
        except Exception as exc:  # reported below
            errors.append(exc)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(inputs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors and all(not t.is_alive() for t in threads), errors
    for got, ref in zip(out, serial):
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))


@pytest.mark.gpu
def test_multi_two_gpus(gpu):
    torch, brdf_amd = gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (this box has one)")
    model, n, S, method = 2, 256, 1001, 1
    angles, x, p0 = _inputs(model, n, S)
    ref = _call(brdf_amd.lib, method, model, angles, x, p0, multi=False)
    for devices in ([0, 1], [1, 0]):
        _assert_same(_call(brdf_amd.lib, method, model, angles, x, p0, devices), ref)
        assert [s["device"] for s in brdf_amd.last_multi_stats()] == devices


@pytest.mark.gpu
def test_one_thread_moves_between_devices(gpu):
    """One host thread fits on device 0, makes device 1 current (hipSetDevice) and fits there, goes back to device 0 and fits
    again (and once more on device 1): the drop-in dlevmar_bc_dif and brdf_hip_fit_dev at n = 256, brdf_hip_fit_batch_dev at
    n = 16, S = 64.  The thread's staging block, workspaces and batch scratch each belong to the device they were allocated on
    and move when the current device does.  Every later round on a device is bit-identical to the first one there, and the
    thread's brdf_hip_last_error() stays empty.  (A thread of its own: the error text and the workspaces are per thread, so it
    starts from none and gives everything back, on the owning devices, when it ends.)"""
    torch, brdf_amd = gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (this box has one)")
    model = 1
    a1, x1 = synth.make_single(model, 256)[:2]
    a16, x16, p16 = _inputs(model, 16, 64)
    kw = dict(lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS)
    rounds, errors = [], []

    def one_round(d):
        torch.cuda.set_device(d)
        dev = torch.device("cuda", d)
        host = brdf_amd.host_dlevmar(1, model, a1, x1, synth.P0[model], **kw)
        single = brdf_amd.fit_single(1, model, torch.from_numpy(a1).to(dev), torch.from_numpy(x1).to(dev), synth.P0[model], **kw)
        batch = brdf_amd.fit_batch(1, model, torch.from_numpy(a16).to(dev), torch.from_numpy(x16).to(dev), torch.from_numpy(p16).to(dev), **kw)
        torch.cuda.synchronize(dev)
        return [np.array([host.ret, single.ret]), host.p, host.info, single.p, single.info] + [t.cpu().numpy() for t in batch]

    def run():
        try:
            for d in (0, 1, 0, 1):
                rounds.append((d, one_round(d), brdf_amd.last_error()))
        except Exception as exc:  # reported below
            errors.append(exc)

    t = threading.Thread(target=run)
    t.start()
    t.join(timeout=120)
    assert not t.is_alive() and not errors, errors
    first = {}
    for d, got, err in rounds:
        assert err == "", (d, err)
        assert got[0].min() >= 0 and got[-1].min() >= 0, (d, got[0], got[-1])
        ref = first.setdefault(d, got)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)), d
    assert len(rounds) == 4


@pytest.mark.gpu
def test_cpp_caller_runs(gpu, tmp_path):
    """a C++ program: brdf_hip_fit_batch_multi on {0,0} against brdf_hip_fit_batch (memcmp), then a clean exit"""
    exe = _compile_caller(tmp_path)
    for args in ([], ["600", "256", "0", "2"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert "bit-identical" in r.stdout
