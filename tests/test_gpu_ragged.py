"""Per-fit sample counts on the device (brdf_hip_fit_batch_ragged_dev, brdf_hip_fit_stats_batch_ragged_dev).

The definition is exact -- fit s of a ragged batch is levmar on the first counts[s] samples of its rows -- so the decisive check
needs no tolerance: for a stride, counts from the stride's own size class, every row padded with NaN behind its count, the
ragged call must return the BYTES the uniform entry point returns for n = count on contiguous copies of those fits (p, info,
ret; covar, stats, rank of the two statistics calls at the ragged result).  Counts below 3 must be refused as levmar refuses
n < m; a fit's bytes must not depend on its neighbours or its place; counts = None and counts == stride are the uniform call.
Counts below the stride's size class run in another geometry than the uniform call would pick for them, so there the fits
are judged against the CPU oracle at n = count with the rules of tests/test_gpu_edges.py."""
import collections

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests import oracle_libs as L
from tests.test_gpu_edges import _judge, _tally

pytestmark = pytest.mark.gpu

FAMILIES = ("diffuse_only", "dark", "quantised", "grazing", "nonpositive")  # one box (synth.bounds), every kind of end: on the box,
                                                                          # at round-off, a cosine <= 0 (the exact twin)
OFF = {"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "0"}
# kernel -> (environment, stride, counts, methods): the smallest shapes that reach every kernel and every size-class boundary
BIT_CASES = {
    "lane": ({}, 16, (0, 2, 3, 7, 15, 16), (1, 2)),
    "rows": ({}, 16, (2, 3, 7, 16), (0,)),
    "wave16": (OFF, 16, (3, 16), (1,)),
    "wave1": ({}, 64, (17, 33, 64), (0, 1)),
    "wave4": ({}, 256, (65, 129, 256), (0, 1)),
    "workgroup": ({}, 1024, (257, 1000, 1024), (0, 1)),
    "eight_wave": ({}, 4096, (1025, 3000, 4096), (0, 1)),
    "big_off": ({"BRDF_HIP_BATCH_BIG": "0"}, 4096, (1025, 3000, 4096), (1,)),
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _t(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bc(method):
    return method in (1, 2)


def _items(model, counts):
    """(count, family, index) of a batch, counts interleaved so that every fit has neighbours of other counts"""
    fams = [f for f in FAMILIES if model in E.FAMILIES[f]]
    return [(k, f, j % 2) for j, f in enumerate(fams) for k in counts]


def _ragged_arrays(model, stride, items):
    """rows of `stride` entries, NaN behind each fit's count; a count below 3 takes the first samples of a 3-sample problem"""
    S = len(items)
    angles, x = np.full((S, 3, stride), np.nan), np.full((S, stride), np.nan)
    p0, counts = np.zeros((S, 3)), np.zeros(S, dtype=np.int32)
    lb = ub = None
    for s, (k, family, idx) in enumerate(items):
        a, xv, p, lb_, ub_ = E.make(family, model, max(k, 3), idx)
        angles[s, :, :k], x[s, :k], p0[s], counts[s] = a[:, :k], xv[:k], p, k
        assert lb is None or (np.array_equal(lb, lb_) and np.array_equal(ub, ub_))
        lb, ub = lb_, ub_
    return angles, x, p0, counts, lb, ub


def _fit(gpu, method, model, angles, x, p0, lb, ub, counts=None):
    torch, brdf_amd, _ = gpu
    kw = dict(lb=lb if _bc(method) else None, ub=ub if _bc(method) else None, itmax=synth.ITMAX, opts=synth.OPTS)
    if counts is not None:
        kw["counts"] = _t(gpu, counts)
    p, info, ret = brdf_amd.fit_batch(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, p0), **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


def _stats(gpu, method, model, angles, x, p, counts=None):
    torch, brdf_amd, _ = gpu
    kw = {} if counts is None else {"counts": _t(gpu, counts)}
    st = brdf_amd.fit_stats_batch(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, p), opts=synth.OPTS, **kw)
    torch.cuda.synchronize()
    return st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_refused(k, p, info, ret, p0, covar, stats, rank, what):
    assert ret == -1 and not info.any() and _same(p, p0), what  # levmar's n < m refusal: LM_ERROR, zero info, p as it came
    assert rank == 0 and not covar.any() and not stats[2:].any(), what
    if k == 0:
        assert not stats[:2].any(), what


@pytest.mark.parametrize("kernel", list(BIT_CASES))
def test_ragged_batch_has_the_bytes_of_the_uniform_call(gpu, monkeypatch, kernel):
    env, stride, counts, methods = BIT_CASES[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fits = refused = 0
    for model in (0, 1, 2):
        items = _items(model, counts)
        angles, x, p0, cnt, lb, ub = _ragged_arrays(model, stride, items)
        order = np.arange(len(items))[::-1]  # the same fits at other places, among other neighbours
        for method in methods:
            p, info, ret = _fit(gpu, method, model, angles, x, p0, lb, ub, cnt)
            covar, stats, rank = _stats(gpu, method, model, angles, x, p, cnt)
            p2, info2, ret2 = _fit(gpu, method, model, angles[order], x[order], p0[order], lb, ub, cnt[order])
            assert _same(p2, p[order]) and _same(info2, info[order]) and _same(ret2, ret[order]), (kernel, model, method, "batch composition")
            c2, s2, r2 = _stats(gpu, method, model, angles[order], x[order], p[order], cnt[order])
            assert _same(c2, covar[order]) and _same(s2, stats[order]) and _same(r2, rank[order]), (kernel, model, method, "composition, stats")
            for k in counts:
                rows = np.flatnonzero(cnt == k)
                assert rows.size >= 2
                if k < 3:
                    for s in rows:
                        _check_refused(k, p[s], info[s], ret[s], p0[s], covar[s], stats[s], rank[s], (kernel, model, method, k, items[s]))
                    refused += rows.size
                    continue
                ua, ux = np.ascontiguousarray(angles[rows][:, :, :k]), np.ascontiguousarray(x[rows][:, :k])
                up, uinfo, uret = _fit(gpu, method, model, ua, ux, p0[rows], lb, ub)
                what = (kernel, model, method, k)
                assert _same(p[rows], up), what + ("p", p[rows], up)
                assert _same(info[rows], uinfo), what + ("info", info[rows], uinfo)
                assert _same(ret[rows], uret), what + ("ret", ret[rows], uret)
                ucov, ustats, urank = _stats(gpu, method, model, ua, ux, p[rows])
                assert _same(covar[rows], ucov) and _same(stats[rows], ustats) and _same(rank[rows], urank), what + ("stats",)
                fits += rows.size
            assert np.any(ret >= 0) and np.any(rank == 3), (kernel, model, method)  # (the comparison is not one of failures)
    print(f"ragged {kernel}: {fits} fits identical to the uniform call, {refused} refused for their count")
    assert refused > 0 or min(counts) >= 3


@pytest.mark.parametrize("stride,method,env", [(16, 1, {}), (16, 0, {}), (16, 1, OFF), (64, 1, {}), (1024, 0, {})],
                         ids=["lane", "rows", "wave16", "wave1", "workgroup"])
def test_no_counts_and_full_counts_are_the_uniform_call(gpu, monkeypatch, stride, method, env):
    torch, brdf_amd, _ = gpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = 1
    items = _items(model, (stride,))
    angles, x, p0, cnt, lb, ub = _ragged_arrays(model, stride, items)
    want = _fit(gpu, method, model, angles, x, p0, lb, ub)
    full = _fit(gpu, method, model, angles, x, p0, lb, ub, cnt)
    assert all(_same(a, b) for a, b in zip(full, want))
    kw = dict(lb=lb if _bc(method) else None, ub=ub if _bc(method) else None)
    lba, uba = (np.ascontiguousarray(kw["lb"]), np.ascontiguousarray(kw["ub"])) if _bc(method) else (None, None)
    from brdf_amd._lib import D, lib
    ta, tx, tp = _t(gpu, angles), _t(gpu, x), _t(gpu, p0)
    info = torch.zeros((len(items), 10), dtype=torch.float64, device=tx.device)
    ret = torch.zeros((len(items),), dtype=torch.int32, device=tx.device)
    opts = np.array(synth.OPTS, dtype=np.float64)
    rc = lib.brdf_hip_fit_batch_ragged_dev(method, model, ta.data_ptr(), tx.data_ptr(), None, len(items), stride, tp.data_ptr(),
                                           lba.ctypes.data_as(D) if lba is not None else None, uba.ctypes.data_as(D) if uba is not None else None,
                                           synth.ITMAX, opts.ctypes.data_as(D), info.data_ptr(), ret.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, brdf_amd.last_error()
    none = (tp.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy())
    assert all(_same(a, b) for a, b in zip(none, want))  # d_counts == NULL
    sw = _stats(gpu, method, model, angles, x, want[0])
    sf = _stats(gpu, method, model, angles, x, want[0], cnt)
    assert all(_same(a, b) for a, b in zip(sf, sw))


def test_ragged_fits_above_4096_samples_are_single_fits(gpu):
    """stride 4100: the fits run one after the other through the single-fit regimes with n = count"""
    torch, brdf_amd, _ = gpu
    stride, method = 4100, 1
    for model in (1, 2):
        items = [(k, f, 0) for k, f in ((5, "quantised"), (4097, "diffuse_only"), (4100, "grazing"), (2, "dark"), (4097, "dark"))]
        angles, x, p0, cnt, lb, ub = _ragged_arrays(model, stride, items)
        p, info, ret = _fit(gpu, method, model, angles, x, p0, lb, ub, cnt)
        covar, stats, rank = _stats(gpu, method, model, angles, x, p, cnt)
        for s, (k, family, idx) in enumerate(items):
            what = (model, k, family)
            if k < 3:
                _check_refused(k, p[s], info[s], ret[s], p0[s], covar[s], stats[s], rank[s], what)
                continue
            a, xv = np.ascontiguousarray(angles[s, :, :k]), np.ascontiguousarray(x[s, :k])
            one = brdf_amd.fit_single(method, model, _t(gpu, a), _t(gpu, xv), p0[s], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
            assert one.ret == ret[s] and _same(np.asarray(one.p, dtype=np.float64), p[s]), what + (one.p, p[s])
            assert _same(np.asarray(one.info, dtype=np.float64), info[s]), what + (one.info, info[s])
            uc, us, ur = _stats(gpu, method, model, a[None], xv[None], p[s][None])
            assert _same(uc[0], covar[s]) and _same(us[0], stats[s]) and ur[0] == rank[s], what + ("stats",)
        assert np.sum(ret >= 0) >= 3


# ---- counts below the stride's size class: another geometry than the uniform call's, judged against the oracle ----------------
BELOW_CLASS = {256: ((3, 7, 16, 17, 64), 6), 1024: ((16, 256), 6), 4096: ((256, 1024), 3)}  # stride -> (counts, fits per family)


def below_class_batches(model, counts, per_family):
    """[(lb, ub, [(count, family, index)])]: the families of tests/test_gpu_edges.py at every count, one batch per box"""
    from tests.test_gpu_edges import _batch_groups
    groups = {}
    for k in counts:
        for lb, ub, items in _batch_groups(model, k, per_family):
            groups.setdefault((tuple(lb), tuple(ub)), []).extend((k, f, i) for f, i in items)
    return [(np.array(b[0]), np.array(b[1]), v) for b, v in groups.items()]


@pytest.mark.parametrize("stride", list(BELOW_CLASS))
def test_counts_below_the_size_class_against_the_oracle(gpu, stride):
    counts, per_family = BELOW_CLASS[stride]
    kinds, bad = collections.Counter(), []
    for model in (0, 1, 2):
        for lb, ub, items in below_class_batches(model, counts, per_family):
            angles, x, p0, cnt, _, _ = _ragged_arrays_boxed(model, stride, items)
            for method in (1, 2):
                p, info, ret = _fit(gpu, method, model, angles, x, p0, lb, ub, cnt)
                for s, (k, family, idx) in enumerate(items):
                    ref = L.brdf_fit("orc", method, model, *E.fit_args(family, model, k, idx))
                    _tally(kinds, bad, _judge((int(ret[s]), p[s], info[s]), ref, lb, ub, k, method, model, E.make(family, model, k, idx)[0],
                                              (stride, k, family, model, idx)))
    print(f"ragged stride {stride}, counts {counts}: {dict(kinds)}")
    assert not bad, "\n".join(map(str, bad))
    assert kinds["failed"] >= 2 and kinds["active"] >= 10
    assert kinds["oracle stopped short"] + kinds["flat"] <= 0.05 * sum(kinds.values()) + 2


def _ragged_arrays_boxed(model, stride, items):
    S = len(items)
    angles, x = np.full((S, 3, stride), np.nan), np.full((S, stride), np.nan)
    p0, counts = np.zeros((S, 3)), np.zeros(S, dtype=np.int32)
    for s, (k, family, idx) in enumerate(items):
        a, xv, p, _, _ = E.make(family, model, k, idx)
        angles[s, :, :k], x[s, :k], p0[s], counts[s] = a, xv, p, k
    return angles, x, p0, counts, None, None
