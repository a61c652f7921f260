"""Packed batches on the device (brdf_hip_fit_batch_packed_dev, brdf_hip_fit_stats_batch_packed_dev).

The definition is exact -- fit s of a packed batch returns what brdf_hip_fit_batch_dev returns for that fit alone at n = its
count -- so nothing here has a tolerance: ONE packed batch whose counts sit on both sides of every size-class seam, the refusals
(0, 2) and two counts above 4096 (the zero-copy path), fits of neighbouring classes interleaved, must return for every fit of
3 samples or more the BYTES of fit_batch / fit_stats_batch on contiguous copies of the fits of that count, and refuse the others as
levmar refuses n < m.  The same bytes must come back when the batch is reversed, when it starts at offsets[0] = 5 inside a larger
buffer of NaN, and when the workspace holds one fit per chunk; offsets = s * n is the uniform call; the environment switches
still choose the class 0 kernel.  The uniform results are computed once per (model, method) and shared by the tests.

Every test runs under a time limit of its own (the process exits when it runs out), and after a device error nothing else runs."""
import faulthandler

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests.test_gpu_ragged import FAMILIES, OFF, _bc, _check_refused, _items, _ragged_arrays, _same, _t

pytestmark = pytest.mark.gpu

COUNTS = (0, 2, 3, 7, 16, 17, 64, 65, 256, 257, 1024, 1025, 4096, 4097, 5000)
CLASS_OF = {0: 0, 2: 0, 3: 0, 7: 0, 16: 0, 17: 1, 64: 1, 65: 2, 256: 2, 257: 3, 1024: 3, 1025: 4, 4096: 4, 4097: 5, 5000: 5}
# every count next to one of another class: small and large alternate, the two refusals and the two large fits apart
ORDER = (4097, 0, 1025, 3, 257, 16, 65, 2, 17, 4096, 7, 1024, 64, 5000, 256)
CASES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (1, 2), (1, 3)]  # models 0, 1, 2 x methods 0 and 1; methods 2 and 3 on one model
TIME_LIMIT_S = 120


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def own_time_limit_and_no_run_after_a_device_error(gpu):
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)  # a hang ends the process: nothing else is started
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()
    try:
        gpu[0].cuda.synchronize()
    except RuntimeError as exc:  # a device error is sticky: stop the session instead of running the next test into it
        pytest.exit(f"device error after a packed-batch test: {exc}", returncode=3)


def _problem(model):
    """the batch: (count, family, index) per fit -- every family of tests/test_gpu_ragged.py at every count, ORDER repeated family
    after family so that neighbours differ in class -- and each fit's samples"""
    assert sorted(ORDER) == sorted(COUNTS) and all(CLASS_OF[a] != CLASS_OF[b] for a, b in zip(ORDER, ORDER[1:] + ORDER[:1]))
    items = _items(model, ORDER)
    fits, lb, ub = [], None, None
    for k, family, idx in items:
        a, xv, p, lb, ub = E.make(family, model, max(k, 3), idx)
        fits.append((np.ascontiguousarray(a[:, :k]), np.ascontiguousarray(xv[:k]), p))
    return items, fits, lb, ub


def _pack(fits, order, lead=0, tail=0):
    """fits laid back to back in `order`, `lead` samples of NaN in front (offsets[0] = lead) and `tail` behind"""
    nan = np.full(1, np.nan)
    angles = np.concatenate([np.repeat(nan, 3 * lead)] + [fits[s][0].reshape(-1) for s in order] + [np.repeat(nan, 3 * tail)])
    x = np.concatenate([np.repeat(nan, lead)] + [fits[s][1] for s in order] + [np.repeat(nan, tail)])
    offsets = lead + np.concatenate([[0], np.cumsum([fits[s][1].size for s in order])]).astype(np.int64)
    p0 = np.stack([fits[s][2] for s in order])
    return angles, x, offsets, p0


def _kw(method, lb, ub):
    return dict(lb=lb if _bc(method) else None, ub=ub if _bc(method) else None, itmax=synth.ITMAX, opts=synth.OPTS)


def _packed(gpu, method, model, packed, lb, ub, **more):
    """(p, info, ret, covar, stats, rank) of the packed fit and of the packed statistics at its result, and last_packed_stats() of both"""
    torch, brdf_amd, _ = gpu
    angles, x, offsets, p0 = (_t(gpu, a) for a in packed)
    p, info, ret = brdf_amd.fit_batch_packed(method, model, angles, x, offsets, p0, **_kw(method, lb, ub), **more)
    plan_fit = brdf_amd.last_packed_stats()
    st = brdf_amd.fit_stats_batch_packed(method, model, angles, x, offsets, p, opts=synth.OPTS, **more)
    plan_stats = brdf_amd.last_packed_stats()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (p, info, ret, st.covar, st.stats, st.rank)), plan_fit, plan_stats


_reference = {}


def _uniform(gpu, model, method):
    """count -> (fit indices, (p, info, ret, covar, stats, rank) of fit_batch / fit_stats_batch at n = count on contiguous copies of
    the fits of that count), computed once per (model, method) and never changed"""
    if (model, method) in _reference:
        return _reference[model, method]
    torch, brdf_amd, _ = gpu
    items, fits, lb, ub = _problem(model)
    out = {}
    for k in COUNTS:
        rows = [s for s, it in enumerate(items) if it[0] == k]
        assert len(rows) >= 4
        if k < 3:
            continue
        ua, ux, up0 = (np.stack([fits[s][i] for s in rows]) for i in range(3))
        ta, tx = _t(gpu, ua), _t(gpu, ux)
        p, info, ret = brdf_amd.fit_batch(method, model, ta, tx, _t(gpu, up0), **_kw(method, lb, ub))
        st = brdf_amd.fit_stats_batch(method, model, ta, tx, p, opts=synth.OPTS)
        torch.cuda.synchronize()
        out[k] = (rows, tuple(t.cpu().numpy() for t in (p, info, ret, st.covar, st.stats, st.rank)))
        for a in out[k][1]:
            a.setflags(write=False)
    _reference[model, method] = out
    return out


NAMES = ("p", "info", "ret", "covar", "stats", "rank")


def _compare(gpu, model, method, got, order, what):
    """every fit of the batch, laid out in `order`, against the uniform call at its own count, or refused; returns (compared, refused)"""
    items, fits, _, _ = _problem(model)
    ref = _uniform(gpu, model, method)
    where = {s: j for j, s in enumerate(order)}
    compared = refused = 0
    converged = with_covariance = False
    for k in COUNTS:
        if k < 3:
            for s, it in enumerate(items):
                if it[0] == k:
                    j = where[s]
                    _check_refused(k, got[0][j], got[1][j], got[2][j], fits[s][2], got[3][j], got[4][j], got[5][j], what + (k, it))
                    refused += 1
            continue
        rows, want = ref[k]
        at = [where[s] for s in rows]
        for name, g, w in zip(NAMES, got, want):
            assert _same(np.ascontiguousarray(g[at]), w), what + (k, name, g[at], w)
        compared += len(rows)
        converged |= bool(np.any(want[2] >= 0))
        with_covariance |= bool(np.any(want[5] == 3))
    assert converged and with_covariance, what + ("the comparison is one of failures",)  # (as tests/test_gpu_ragged.py asks of a batch)
    assert compared + refused == len(items), what  # no fit is left out
    return compared, refused


def _expected_plan(items, one_per_chunk=False):
    plan = []
    for cls in range(6):
        ks = [it[0] for it in items if CLASS_OF[it[0]] == cls]
        stride = max(ks) if cls == 5 else max(3, max(ks))
        plan.append({"fits": len(ks), "stride": stride, "chunks": len(ks) if (one_per_chunk or cls == 5) else 1})
    return plan


@pytest.mark.parametrize("model,method", CASES)
def test_packed_batch_has_the_bytes_of_the_uniform_call_per_fit(gpu, model, method):
    items, fits, lb, ub = _problem(model)
    order = list(range(len(items)))
    got, plan_fit, plan_stats = _packed(gpu, method, model, _pack(fits, order), lb, ub)
    compared, refused = _compare(gpu, model, method, got, order, ("packed", model, method))
    print(f"packed model {model} method {method}: {compared} fits identical to the uniform call, {refused} refused; plan {plan_fit}")
    assert refused == 2 * len(items) // len(COUNTS) and compared == len(items) - refused
    # one chunk per non-empty class by default, with the fits and strides the counts imply (class 5: one run per fit)
    assert plan_fit == _expected_plan(items) and plan_stats == plan_fit


@pytest.mark.parametrize("model,method", [(1, 1), (1, 0), (2, 1)])
def test_placement_and_chunking_cannot_show(gpu, model, method):
    torch, brdf_amd, _ = gpu
    items, fits, lb, ub = _problem(model)
    S = len(items)
    order = list(range(S))
    what = (model, method)
    # the same fits at other places, among other neighbours
    rev = order[::-1]
    got, _, _ = _packed(gpu, method, model, _pack(fits, rev), lb, ub)
    _compare(gpu, model, method, got, rev, ("reversed",) + what)
    # the batch starts at offsets[0] = 5 inside a larger buffer whose surroundings are NaN: nothing outside it is read
    got, _, _ = _packed(gpu, method, model, _pack(fits, order, lead=5, tail=9), lb, ub)
    _compare(gpu, model, method, got, order, ("offset 5",) + what)
    # one fit per chunk
    got, plan_fit, plan_stats = _packed(gpu, method, model, _pack(fits, order), lb, ub, workspace_bytes=1)
    _compare(gpu, model, method, got, order, ("one fit per chunk",) + what)
    assert plan_fit == _expected_plan(items, one_per_chunk=True) and plan_stats == plan_fit
    assert all(c["chunks"] == c["fits"] > 0 for c in plan_fit)


@pytest.mark.parametrize("n,method", [(16, 1), (16, 0), (256, 1), (256, 0)])
def test_offsets_s_times_n_are_the_uniform_call(gpu, n, method):
    torch, brdf_amd, _ = gpu
    model = 1
    items = _items(model, (n,))
    angles, x, p0, cnt, lb, ub = _ragged_arrays(model, n, items)  # (counts == stride: no padding)
    S = len(items)
    ta, tx = _t(gpu, angles), _t(gpu, x)
    want = brdf_amd.fit_batch(method, model, ta, tx, _t(gpu, p0), **_kw(method, lb, ub))
    offsets = torch.arange(S + 1, dtype=torch.int64, device=tx.device) * n
    got = brdf_amd.fit_batch_packed(method, model, ta.reshape(-1), tx.reshape(-1), offsets, _t(gpu, p0), **_kw(method, lb, ub))
    plan = brdf_amd.last_packed_stats()
    sw = brdf_amd.fit_stats_batch(method, model, ta, tx, want[0], opts=synth.OPTS)
    sg = brdf_amd.fit_stats_batch_packed(method, model, ta.reshape(-1), tx.reshape(-1), offsets, got[0], opts=synth.OPTS)
    torch.cuda.synchronize()
    for g, w in zip(got + (sg.covar, sg.stats, sg.rank), want + (sw.covar, sw.stats, sw.rank)):
        assert _same(g.cpu().numpy(), w.cpu().numpy()), (n, method)
    assert bool((want[2] >= 0).any())
    cls = 0 if n == 16 else 2
    assert [c["fits"] for c in plan] == [S if c == cls else 0 for c in range(6)] and plan[cls] == {"fits": S, "stride": n, "chunks": 1}


def test_switches_still_choose_the_class_0_kernel(gpu, monkeypatch):
    """BRDF_HIP_LANE=0 and BRDF_HIP_ROWS=0: the class 0 fits take the wave-per-fit kernel, in the packed call as in the uniform one"""
    torch, brdf_amd, _ = gpu
    model, method = 1, 1
    items, fits, lb, ub = _problem(model)
    small = [s for s, it in enumerate(items) if CLASS_OF[it[0]] == 0]

    def run():
        angles, x, offsets, p0 = (_t(gpu, a) for a in _pack(fits, small))
        p, info, ret = brdf_amd.fit_batch_packed(method, model, angles, x, offsets, p0, **_kw(method, lb, ub))
        uni = {}
        for k in (3, 7, 16):
            rows = [s for s in small if items[s][0] == k]
            ua, ux, up0 = (_t(gpu, np.stack([fits[s][i] for s in rows])) for i in range(3))
            uni[k] = (rows, brdf_amd.fit_batch(method, model, ua, ux, up0, **_kw(method, lb, ub)))
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (p, info, ret)), {k: (rows, tuple(t.cpu().numpy() for t in r)) for k, (rows, r) in uni.items()}

    default, _ = run()
    for name, value in OFF.items():
        monkeypatch.setenv(name, value)
    got, uni = run()
    where = {s: j for j, s in enumerate(small)}
    for k, (rows, want) in uni.items():
        at = [where[s] for s in rows]
        for g, w in zip(got, want):
            assert _same(np.ascontiguousarray(g[at]), w), (k, g[at], w)
    assert any((want[2] >= 0).any() for _, want in uni.values())  # (the comparison is not one of failures)
    print("the switched-off kernels' bytes differ from the default kernels':", not all(_same(a, b) for a, b in zip(default, got)))


def test_host_pointer_entries_return_the_bytes_of_their_dev_entries(gpu):
    """One fit of every count of COUNTS, Blinn-Phong dlevmar_bc_dif: brdf_hip_fit_batch_packed and brdf_hip_fit_stats_batch_packed
    (host pointers: upload, the _dev entry, one wait, download) return the bytes of brdf_hip_fit_batch_packed_dev and
    brdf_hip_fit_stats_batch_packed_dev, and brdf_hip_fit_batch_ragged (S = 5, stride 16) those of brdf_hip_fit_batch_ragged_dev."""
    import ctypes as C
    torch, brdf_amd, _ = gpu
    from brdf_amd._lib import D, I, lib
    model, method = 1, 1
    fams = [f for f in FAMILIES if model in E.FAMILIES[f]]
    fits, lb, ub = [], None, None
    for j, k in enumerate(COUNTS):
        a, xv, p, lb, ub = E.make(fams[j % len(fams)], model, max(k, 3), 0)
        fits.append((np.ascontiguousarray(a[:, :k]), np.ascontiguousarray(xv[:k]), p))
    S = len(fits)
    packed = _pack(fits, list(range(S)))
    want, _, _ = _packed(gpu, method, model, packed, lb, ub)
    angles, x, offsets, p0 = (np.ascontiguousarray(a) for a in packed)
    lba, uba, opts = (np.ascontiguousarray(v, dtype=np.float64) for v in (lb, ub, synth.OPTS))
    p, info, ret = p0.copy(), np.zeros((S, 10)), np.zeros(S, dtype=np.int32)
    failed = lib.brdf_hip_fit_batch_packed(method, model, angles.ctypes.data_as(D), x.ctypes.data_as(D), offsets.ctypes.data_as(C.POINTER(C.c_longlong)),
                                           S, p.ctypes.data_as(D), lba.ctypes.data_as(D), uba.ctypes.data_as(D), synth.ITMAX, opts.ctypes.data_as(D),
                                           info.ctypes.data_as(D), ret.ctypes.data_as(I), 0)
    assert failed == int((want[2] < 0).sum()) >= 2, brdf_amd.last_error()  # the number of fits with ret < 0 (the two refusals at least)
    covar, stats, rank = np.zeros((S, 3, 3)), np.zeros((S, 8)), np.zeros(S, dtype=np.int32)
    rc = lib.brdf_hip_fit_stats_batch_packed(method, model, angles.ctypes.data_as(D), x.ctypes.data_as(D), offsets.ctypes.data_as(C.POINTER(C.c_longlong)),
                                             S, p.ctypes.data_as(D), opts.ctypes.data_as(D), covar.ctypes.data_as(D), stats.ctypes.data_as(D),
                                             rank.ctypes.data_as(I), 0)
    assert rc == 0, brdf_amd.last_error()
    for name, g, w in zip(NAMES, (p, info, ret, covar, stats, rank), want):
        assert _same(g, w), ("packed", name, g, w)
    assert np.any(want[2] >= 0) and np.any(want[5] == 3)  # (the comparison is not one of failures)
    # the ragged fit pair
    items = [(k, fams[j % len(fams)], 0) for j, k in enumerate((0, 2, 3, 7, 16))]
    ra, rx, rp0, cnt, lb, ub = _ragged_arrays(model, 16, items)
    dev = brdf_amd.fit_batch(method, model, _t(gpu, ra), _t(gpu, rx), _t(gpu, rp0), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, counts=_t(gpu, cnt))
    torch.cuda.synchronize()
    p, info, ret = rp0.copy(), np.zeros((5, 10)), np.zeros(5, dtype=np.int32)
    failed = lib.brdf_hip_fit_batch_ragged(method, model, ra.ctypes.data_as(D), rx.ctypes.data_as(D), cnt.ctypes.data_as(I), 5, 16, p.ctypes.data_as(D),
                                           lba.ctypes.data_as(D), uba.ctypes.data_as(D), synth.ITMAX, opts.ctypes.data_as(D), info.ctypes.data_as(D),
                                           ret.ctypes.data_as(I))
    assert failed == int((ret < 0).sum()) >= 2, brdf_amd.last_error()
    for name, g, w in zip(NAMES, (p, info, ret), dev):
        assert _same(g, w.cpu().numpy()), ("ragged", name, g, w)
    assert np.any(ret >= 0)
