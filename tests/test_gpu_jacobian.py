"""The device's analytic Jacobian against 50-digit derivatives, and dead-lobe fits in every fit regime.

Rows: brdf_amd.model_jacobian (BRDFJac_hip, the exact-path model_jac_kernel) on the grid of tests/jacobian_yardstick.py, every
entry inside the yardstick's bound; dlevmar_chkjac on BRDFFunc_hip / BRDFJac_hip finite where the lobe is dead.

Fits: data with dead-lobe samples (pow(0, n); Ward at cos(N.H) = 0, 5e-320, 1e-200 -- tests/edge_problems.py: make_dead_lobe),
where the Jacobian's third column used to be 0 * inf = NaN and dlevmar_bc_der / dlevmar_der stopped at p0 with reason 5.  Methods
2 and 3, with 1 and 0 as controls, as a single fit (n = 64; n = 5000 resident and as a launch chain), as three channels of a shared
launch, in every batched kernel, in a weighted and in a packed batch.  Per fit: test_gpu_edges' rule against the oracle on the
same inputs (_judge), success with a reason other than 5, ||e||^2 within E_TOL of the reference's own finite-difference optimum
(tests/golden/brdf_dead_lobe_fits.json, which owes nothing to this project's Jacobian), and for Phong / Blinn-Phong the bytes of
the same call under BRDF_HIP_EXACT_POW=1 (a zero cosine sends the fit to the exact model).

Statistics: fit_stats_batch and its packed and weighted twins with the analytic row at a dead-lobe fit's p: rank 3, a finite
covariance, inside tests/stats_yardstick.py's bound.

Every test runs under a time limit of its own (the process exits when it runs out), and after a device error nothing else runs."""
import collections
import ctypes as C
import faulthandler
import functools

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests import jacobian_yardstick as J
from tests import oracle_libs as L
from tests import stats_yardstick as Y
from tests import weighted_yardstick as WY
from tests.test_gpu_edges import E_TOL, FALLBACK_BATCH, METHOD, _identical, _judge

pytestmark = pytest.mark.gpu
TIME_LIMIT_S = 120
METHODS = (2, 3, 1, 0)  # the analytic methods and their finite-difference controls
BATCH = {k: FALLBACK_BATCH[k] + (8,) for k in ("lane", "rows", "wave", "wave4", "workgroup", "eight_wave")}
BATCH["one_by_one"] = FALLBACK_BATCH["one_by_one"] + (2,)  # kernel -> (environment, n, fits)


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
        pytest.exit(f"device error after a Jacobian test: {exc}", returncode=3)


def _t(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bc(method):
    return method in (1, 2)


@functools.lru_cache(maxsize=None)
def _problem(model, n, idx):
    return E.make_dead_lobe(model, n, idx)


@functools.lru_cache(maxsize=None)
def _filler(model, n, idx):
    """an ordinary neighbour for a batch: the `quantised` family (same box as the dead-lobe problems)"""
    return E.make("quantised", model, n, idx)


@functools.lru_cache(maxsize=None)
def _oracle(model, method, n, idx):
    return L.brdf_fit("orc", method, model, *E.dead_lobe_args(model, n, idx))


def _check_dead(got, model, method, n, idx, what, kinds):
    """one device fit (ret, p, info) of the dead-lobe problem (model, n, idx)"""
    angles, x, p0, lb, ub = _problem(model, n, idx)
    ret, p, info = got
    what = (what, METHOD[method], model, n, idx, int(ret), list(p), list(info))
    kind, bad = _judge(got, _oracle(model, method, n, idx), lb, ub, n, method, model, angles, what)
    kinds[kind] += 1
    assert bad is None, bad
    assert ret >= 0 and info[6] != 5 and np.all(np.isfinite(p)) and np.all(np.isfinite(info)), what
    rr, rp, ri = J.dead_lobe_reference(model, method, n, idx)
    assert rr >= 0 and abs(info[1] - ri[1]) <= E_TOL * ri[1], (what, "the reference's finite-difference optimum", ri[1])


def _kw(method, lb, ub):
    return dict(lb=lb if _bc(method) else None, ub=ub if _bc(method) else None, itmax=synth.ITMAX, opts=synth.OPTS)


# ---- rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_device_rows_against_50_digit_derivatives(gpu, model):
    """BRDFJac_hip on the whole grid: judged entries inside (2 K_ULP + 8) u cond sum|terms| + the subnormal floor, dead-lobe entries
    exactly 0, entries not judged NaN / infinite exactly where the IEEE expression is"""
    _, brdf_amd, _ = gpu
    worst, tally = 0.0, {}
    for angles, p in J.grid(model):
        rows = brdf_amd.model_jacobian(model, np.ascontiguousarray(angles), p)
        worst = max(worst, J.check_rows(rows, model, angles, p, ("BRDFJac_hip", model, p), tally))
    print(f"model {model}: worst judged entry of the device row {worst:.2f} u cond sum|terms| (bound {J.REL / J.U:.0f}); entries {tally}")
    assert tally[J.JUDGED] > 1000 and tally[J.DEAD] >= 14


@pytest.mark.parametrize("model", [0, 1, 2])
def test_chkjac_is_finite_on_dead_lobe_rows(gpu, model):
    """dlevmar_chkjac (the product's) on rows whose lobe is dead: err is finite -- a NaN in the row made it NaN -- and says the
    row is right (> 0.5); the rows themselves are (df/dkd, 0, 0)"""
    _, brdf_amd, _ = gpu
    angles, p = J.dead_rows(model)
    planes = [angles]
    if model == 2:
        for c in E.WARD_DEAD_COSINES[1:]:
            a = angles.copy()
            a[1] = c
            planes.append(a)
    for a in planes:
        rows = brdf_amd.model_jacobian(model, a, p)
        assert np.all(np.isfinite(rows)) and np.all(rows[:, 1:] == 0.0) and np.all(rows[:, 0] > 0.0), (model, rows)
        err = brdf_amd.chkjac(model, a, p)
        assert np.all(np.isfinite(err)) and np.all(err > 0.5), (model, err)


# ---- single fits -----------------------------------------------------------------------------------------------------------
def _single(gpu, method, model, n, idx):
    _, brdf_amd, _ = gpu
    angles, x, p0, lb, ub = _problem(model, n, idx)
    return brdf_amd.fit_single(method, model, _t(gpu, angles), _t(gpu, x), p0, want_covar=True, **_kw(method, lb, ub))


@pytest.mark.parametrize("n,resident", [(64, None), (5000, "1"), (5000, "0")], ids=["n64", "n5000_resident", "n5000_launch_chain"])
def test_single_dead_lobe_fits(gpu, monkeypatch, n, resident):
    _, brdf_amd, _ = gpu
    if resident is not None:
        monkeypatch.setenv("BRDF_HIP_RESIDENT", resident)
    kinds = collections.Counter()
    for model in (0, 1, 2):
        for idx in (0, 1):
            for method in METHODS:
                res = _single(gpu, method, model, n, idx)
                _check_dead((res.ret, res.p, res.info), model, method, n, idx, ("single", resident), kinds)
                assert res.covar is not None and np.all(np.isfinite(res.covar)), (model, idx, METHOD[method], res)
                if model != 2:
                    monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
                    exact = _single(gpu, method, model, n, idx)
                    monkeypatch.delenv("BRDF_HIP_EXACT_POW")
                    assert _identical(res, exact), (model, idx, METHOD[method], res, exact)
    print(f"single dead-lobe fits, n = {n}, BRDF_HIP_RESIDENT={resident}: {dict(kinds)}")
    assert kinds["failed"] == 0 and sum(kinds.values()) == 3 * 2 * len(METHODS)


# ---- channels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_three_channels_of_a_shared_launch(gpu, monkeypatch, model):
    """brdf_hip_fit_channels_dev, n = 1000: channel 0 is the dead-lobe problem itself (held to the fixture), channels 1 and 2 the
    same planes with the measurements scaled by 0.8 and 0.6 (held to the oracle); every channel has the bytes of its single fit"""
    _, brdf_amd, _ = gpu
    n, idx = 1000, 0
    angles, x, p0, lb, ub = _problem(model, n, idx)
    xs = np.stack([x, 0.8 * x, 0.6 * x])
    a, xd = _t(gpu, angles), _t(gpu, xs)
    kinds = collections.Counter()
    for method in METHODS:
        shared = brdf_amd.fit_channels(method, model, a, xd, p0, want_covar=True, **_kw(method, lb, ub))
        if _bc(method) and model == 2:  # (the box methods share a launch; a zero cosine of Phong / Blinn-Phong sends it to the exact model)
            assert brdf_amd.last_channels_stats()["shared_launch"], (model, METHOD[method])
        _check_dead((shared[0].ret, shared[0].p, shared[0].info), model, method, n, idx, "channel 0", kinds)
        for c in range(3):
            res = shared[c]
            what = ("channel", c, METHOD[method], model, res)
            alone = brdf_amd.fit_single(method, model, a, xd[c], p0, want_covar=True, **_kw(method, lb, ub))
            assert _identical(res, alone), (what, alone)
            ref = L.brdf_fit("orc", method, model, angles, xs[c], p0, synth.ITMAX, synth.OPTS, lb, ub)
            kind, bad = _judge((res.ret, res.p, res.info), ref, lb, ub, n, method, model, angles, what)
            kinds[kind] += 1
            assert bad is None, bad
            assert res.ret >= 0 and res.info[6] != 5 and np.all(np.isfinite(res.covar)), what
            if model != 2:
                monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
                exact = brdf_amd.fit_single(method, model, a, xd[c], p0, want_covar=True, **_kw(method, lb, ub))
                monkeypatch.delenv("BRDF_HIP_EXACT_POW")
                assert _identical(res, exact), (what, exact)
    assert kinds["failed"] == 0


# ---- batches ---------------------------------------------------------------------------------------------------------------
def _batch_items(model, n, S):
    """S fits: the two dead-lobe problems among ordinary neighbours -> [(is dead, index, (angles, x, p0, lb, ub))]"""
    if S == 2:
        return [(True, i, _problem(model, n, i)) for i in (0, 1)]
    order = [(False, 0), (True, 0), (False, 1), (False, 2), (True, 1), (False, 3), (False, 4), (False, 5)][:S]
    return [(dead, i, _problem(model, n, i) if dead else _filler(model, n, i)) for dead, i in order]


def _run_batch(gpu, method, model, items, weights=None):
    torch, brdf_amd, _ = gpu
    angles, x, p0 = (np.stack([it[2][k] for it in items]) for k in range(3))
    lb, ub = items[0][2][3], items[0][2][4]
    assert all(np.array_equal(it[2][3], lb) and np.array_equal(it[2][4], ub) for it in items)
    if weights is None:
        out = brdf_amd.fit_batch(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, p0), **_kw(method, lb, ub))
    else:
        out = brdf_amd.fit_batch_weighted(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, weights), _t(gpu, p0), **_kw(method, lb, ub))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("kernel", list(BATCH))
def test_batched_kernels_on_dead_lobe_fits(gpu, monkeypatch, kernel):
    """every batched kernel with the two dead-lobe problems among ordinary fits of the same size"""
    env, n, S = BATCH[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kinds = collections.Counter()
    for model in (0, 1, 2):
        items = _batch_items(model, n, S)
        dead = np.array([it[0] for it in items])
        for method in METHODS:
            p, info, ret = _run_batch(gpu, method, model, items)
            for s, (is_dead, idx, prob) in enumerate(items):
                if is_dead:
                    _check_dead((int(ret[s]), p[s], info[s]), model, method, n, idx, kernel, kinds)
                else:
                    ref = L.brdf_fit("orc", method, model, *E.fit_args("quantised", model, n, idx))
                    kind, bad = _judge((int(ret[s]), p[s], info[s]), ref, prob[3], prob[4], n, method, model, prob[0], (kernel, "neighbour", idx))
                    assert bad is None, bad
            if model != 2:
                monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
                pe, ie, re_ = _run_batch(gpu, method, model, items)
                monkeypatch.delenv("BRDF_HIP_EXACT_POW")
                what = (kernel, model, METHOD[method])
                assert np.array_equal(p[dead], pe[dead]) and np.array_equal(info[dead], ie[dead]) and np.array_equal(ret[dead], re_[dead]), what
    print(f"batched kernel {kernel}, dead-lobe fits: {dict(kinds)}")
    assert kinds["failed"] == 0 and sum(kinds.values()) == 3 * 2 * len(METHODS)


# ---- a weighted batch ------------------------------------------------------------------------------------------------------
_FUNC = C.CFUNCTYPE(None, L.D, L.D, C.c_int, C.c_int, C.c_void_p)


def _weights(S, n):
    return np.ascontiguousarray(np.random.default_rng(20).choice([0.5, 1.0, 2.0, 3.0], size=(S, n)))


def _weighted_oracle(method, model, angles, x, w, p0, lb, ub):
    """the oracle's dlevmar_bc_der (method 2) / dlevmar_bc_dif (1) on sqrt(w) f against sqrt(w) x, the Jacobian sqrt(w) times the
    oracle's analytic row"""
    a, xx, sw = L.f64(angles), L.f64(x), np.sqrt(L.f64(w))
    n = xx.size
    ed = Y._Extra(L.ptr(a), model)

    def func(p, hx, m, nn, adata):
        L.orc.orc_brdf_func(p, hx, m, nn, C.c_void_p(adata))
        np.ctypeslib.as_array(hx, shape=(nn,))[:] *= sw

    def jacf(p, jac, m, nn, adata):
        L.orc.orc_brdf_jac(p, jac, m, nn, C.c_void_p(adata))
        np.ctypeslib.as_array(jac, shape=(nn * m,)).reshape(nn, m)[:] *= sw[:, None]

    cf, cj = _FUNC(func), _FUNC(jacf)
    p, info, xs = L.f64(p0).copy(), np.zeros(10), np.ascontiguousarray(sw * xx)
    tail = (L.ptr(p), L.ptr(xs), 3, n, L.ptr(L.f64(lb)), L.ptr(L.f64(ub)), None, synth.ITMAX, L.ptr(L.f64(synth.OPTS)), L.ptr(info), None, None,
            C.byref(ed))
    r = L.orc.orc_dlevmar_bc_der(cf, cj, *tail) if method == 2 else L.orc.orc_dlevmar_bc_dif(cf, *tail)
    return int(r), p, info


@pytest.mark.parametrize("model", [0, 1, 2])
def test_weighted_batch_on_dead_lobe_fits(gpu, monkeypatch, model):
    """brdf_hip_fit_batch_weighted_dev, n = 16, weights in {0.5, 1, 2, 3}: dlevmar_bc_der (and bc_dif as control) against the
    oracle's solver on the weighted problem; ||e||^2 within E_TOL of the weighted finite-difference optimum (the reference's
    dlevmar_bc_dif on sqrt(w) f, tests/weighted_yardstick.py); with unit weights the bytes of the unweighted batch"""
    n, S = 16, 8
    items = _batch_items(model, n, S)
    dead = np.array([it[0] for it in items])
    w = _weights(S, n)
    for method in (2, 1):
        p, info, ret = _run_batch(gpu, method, model, items, weights=w)
        for s, (is_dead, idx, (angles, x, p0, lb, ub)) in enumerate(items):
            ref = _weighted_oracle(method, model, angles, x, w[s], p0, lb, ub)
            what = ("weighted", "dead lobe" if is_dead else "neighbour", idx, int(ret[s]), list(p[s]), list(info[s]))
            # _judge's J'J for a flat direction is the unweighted one: weights in [0.5, 3] change it by at most that factor
            kind, bad = _judge((int(ret[s]), p[s], info[s]), ref, lb, ub, n, method, model, angles, what)
            assert bad is None, bad
            if is_dead:
                assert ret[s] >= 0 and info[s, 6] != 5 and np.all(np.isfinite(p[s])), what
                fr, fp, fi = WY.weighted_fit(model, angles, x, w[s], p0, lb=lb, ub=ub)
                assert fr >= 0 and abs(info[s, 1] - fi[1]) <= E_TOL * fi[1], (what, "weighted finite-difference optimum", fi[1])
        if model != 2:
            monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
            pe, ie, re_ = _run_batch(gpu, method, model, items, weights=w)
            monkeypatch.delenv("BRDF_HIP_EXACT_POW")
            assert np.array_equal(p[dead], pe[dead]) and np.array_equal(info[dead], ie[dead]) and np.array_equal(ret[dead], re_[dead]), (model, method)
        plain = _run_batch(gpu, method, model, items)
        unit = _run_batch(gpu, method, model, items, weights=np.ones((S, n)))
        for u, v in zip(unit, plain):
            assert u.tobytes() == v.tobytes(), (model, METHOD[method])


# ---- a packed batch --------------------------------------------------------------------------------------------------------
PACKED_SIZES = (16, 64, 1024)


def _packed_problem(model):
    """sizes 16, 64 and 1024 interleaved, both dead-lobe problems of each -> ([(n, idx)], angles, x, offsets, p0, lb, ub)"""
    order = [(n, idx) for idx in (0, 1) for n in PACKED_SIZES]
    probs = [_problem(model, n, idx) for n, idx in order]
    angles = np.concatenate([pr[0].reshape(-1) for pr in probs])
    x = np.concatenate([pr[1] for pr in probs])
    offsets = np.concatenate([[0], np.cumsum([pr[1].size for pr in probs])]).astype(np.int64)
    return order, angles, x, offsets, np.stack([pr[2] for pr in probs]), probs[0][3], probs[0][4]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_packed_batch_on_dead_lobe_fits(gpu, monkeypatch, model):
    torch, brdf_amd, _ = gpu
    order, angles, x, offsets, p0, lb, ub = _packed_problem(model)
    kinds = collections.Counter()

    def run(method):
        out = brdf_amd.fit_batch_packed(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, offsets), _t(gpu, p0), **_kw(method, lb, ub))
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in out)

    for method in METHODS:
        p, info, ret = run(method)
        for s, (n, idx) in enumerate(order):
            _check_dead((int(ret[s]), p[s], info[s]), model, method, n, idx, "packed", kinds)
        if model != 2:
            monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
            exact = run(method)
            monkeypatch.delenv("BRDF_HIP_EXACT_POW")
            for u, v in zip((p, info, ret), exact):
                assert np.array_equal(u, v), (model, METHOD[method])
    assert kinds["failed"] == 0


# ---- statistics at a dead-lobe fit -----------------------------------------------------------------------------------------
def _finite_rank3(st, S):
    covar, stats, rank = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in (st.covar, st.stats, st.rank))
    assert np.all(rank == 3) and np.all(np.isfinite(covar)) and np.all(np.isfinite(stats)) and covar.shape == (S, 3, 3), (rank, covar, stats)
    return covar, stats, rank


@pytest.mark.parametrize("model", [0, 1, 2])
def test_fit_statistics_at_dead_lobe_fits(gpu, model):
    """brdf_hip_fit_stats_batch_dev, its packed and its weighted twin with the analytic row (method 2) at the oracle's fitted p of
    the dead-lobe problems: rank 3 and a finite covariance on every fit -- one NaN in a row made J^T J NaN and the rank 0 -- and,
    where cond(J^T J) <= 1e8, C / sigma / rho inside the yardstick's bound"""
    torch, brdf_amd, _ = gpu
    kind = Y.ANALYTIC
    for n in (64, 1024):  # uniform
        probs = [_problem(model, n, i) for i in (0, 1)]
        angles, x = np.stack([pr[0] for pr in probs]), np.stack([pr[1] for pr in probs])
        p = np.stack([_oracle(model, 2, n, i)[1] for i in (0, 1)])
        st = brdf_amd.fit_stats_batch(2, model, _t(gpu, angles), _t(gpu, x), _t(gpu, p), opts=synth.OPTS)
        torch.cuda.synchronize()
        covar, stats, rank = _finite_rank3(st, 2)
        _, compared, _ = Y.compare(kind, model, angles, x, p, covar, stats, rank, label=f"dead lobe n={n}")
        assert compared == 2
    # packed: 16, 64 and 1024 in one call
    order, angles, x, offsets, _, _, _ = _packed_problem(model)
    p = np.stack([_oracle(model, 2, n, i)[1] for n, i in order])
    st = brdf_amd.fit_stats_batch_packed(2, model, _t(gpu, angles), _t(gpu, x), _t(gpu, offsets), _t(gpu, p), opts=synth.OPTS)
    torch.cuda.synchronize()
    covar, stats, rank = _finite_rank3(st, len(order))
    compared = 0
    for s, (n, i) in enumerate(order):
        pr = _problem(model, n, i)
        compared += Y.compare(kind, model, pr[0][None], pr[1][None], p[s:s + 1], covar[s:s + 1], stats[s:s + 1], rank[s:s + 1], max_left_out=1.0,
                              label=f"dead lobe packed n={n}")[1]
    assert compared >= len(order) - 1  # (Phong's 16-sample problem 1 sits at cond 2e8)
    # weighted, n = 16
    n, S = 16, 2
    probs = [_problem(model, n, i) for i in (0, 1)]
    angles, x = np.stack([pr[0] for pr in probs]), np.stack([pr[1] for pr in probs])
    w = _weights(S, n)
    p = np.stack([_weighted_oracle(2, model, pr[0], pr[1], w[s], pr[2], pr[3], pr[4])[1] for s, pr in enumerate(probs)])
    st = brdf_amd.fit_stats_batch_weighted(2, model, _t(gpu, angles), _t(gpu, x), _t(gpu, w), _t(gpu, p), opts=synth.OPTS)
    torch.cuda.synchronize()
    covar, stats, rank = _finite_rank3(st, S)
    _, compared, _ = WY.compare_weighted_stats(kind, model, angles, x, w, p, covar, stats, rank, max_left_out=0.5, label="dead lobe weighted")
    assert compared >= 1
