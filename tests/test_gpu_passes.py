"""Per-pass parity on the device (tests/pass_problems.py): fits cut short by itmax = 1, 2, 3, by a loosened stop rule, by itmax = 0,
with opts = NULL, other tau and delta, in every fit regime -- ret, p, info[0..4] against the oracle within each case's own
tolerance (8 x what the oracle itself moves under re-ordered sums and model values disturbed by the device's documented error;
capped at 1e-8 / 1e-6), info[5..9] exactly.  A Jacobian column that is off, a sample dropped from J'e, a damping update off by a
factor or a speculative evaluation that is counted all show here, where the fixed point (tests/test_gpu_parity.py) hides them.
tests/test_oracle_passes.py judges the same case lists on the CPU first (the reference alone, and the host-driven machines).

The covariance of every single-fit entry is held the same way: max |C_ij - C_ref_ij| / sqrt(C_ref_ii C_ref_jj) within 8 x the oracle's
own spread (capped at 1e-6), in every regime, with dscl, with central differences, at the cut-short fits -- where dlevmar_dif's secant
J'J has the oracle's update history -- and at converged ones; nine zeros exactly where the reference writes nothing defined (itmax = 0,
a stop before the first Jacobian, a singular J'J); untouched where the call is refused.

Every test prints its summary: cases compared, cases the yardstick does not admit, the worst difference / tolerance per field."""
import ctypes as C

import numpy as np
import pytest

from brdf_amd import synth
from tests import pass_problems as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


_ON_DEVICE = {}


def _t(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the problems are read-only)


def _planes(gpu, key):
    """(angles, x) of a problem on the device, uploaded once"""
    if key not in _ON_DEVICE:
        angles, x = P.problem(key)[:2]
        _ON_DEVICE[key] = (_t(gpu, angles), _t(gpu, x))
    return _ON_DEVICE[key]


def _single(gpu, case, want_covar=True):
    _, brdf_amd, _ = gpu
    a, x = _planes(gpu, case.problem)
    lb, ub = P.box(case)
    res = brdf_amd.fit_single(case.method, case.problem[1], a, x, P.problem(case.problem)[2], lb=lb, ub=ub, dscl=P.scaling(case), itmax=case.itmax,
                              opts=case.opts, want_covar=want_covar)
    return (res.ret, res.p, res.info, res.covar) if want_covar else (res.ret, res.p, res.info)


def _same(a, b):
    """ret, p, info -- and the covariance, where both carry one -- byte for byte"""
    return int(a[0]) == int(b[0]) and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in list(zip(a, b))[1:])


# ---- single fits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_pow", ["0", "1"], ids=["fast", "exact_pow"])
@pytest.mark.parametrize("regime", list(P.SINGLE_REGIMES))
def test_single_fits(gpu, monkeypatch, regime, exact_pow):
    """one workgroup (n = 64, 1000, 4096), the resident regime (n = 5000, one launch), the launch chain (n = 5000), a short last
    workgroup (n = 262145); on the default path and with the reference's pow expression"""
    _, brdf_amd, _ = gpu
    monkeypatch.setenv("BRDF_HIP_EXACT_POW", exact_pow)
    monkeypatch.setenv("BRDF_HIP_RESIDENT", "0" if regime == "launch_chain" else "1")
    tally = P.Tally(f"single fits, {regime}, BRDF_HIP_EXACT_POW={exact_pow}")
    chained = 0
    for n in P.SINGLE_REGIMES[regime]:
        for cell, case in P.single_cases(n):
            tally.add(cell, case, _single(gpu, case))
            launches = brdf_amd.last_fit_stats()["launches"]
            if regime in ("resident", "short_last_workgroup"):
                assert launches == 1, (P.describe(case), launches)
            chained += int(launches > 1)
    tally.check()
    assert regime != "launch_chain" or chained >= 0.8 * len(P.single_cases(5000))


# ---- switches whose speculation must not show ---------------------------------------------------------------------------
_DEFAULT_RUNS = {}


@pytest.mark.parametrize("switch,value", [("BRDF_HIP_DIF_CHAIN", "1"), ("BRDF_HIP_DIF_FUSED", "0"), ("BRDF_HIP_SPEC_JAC", "0"), ("BRDF_HIP_PG_MULTI", "1")])
def test_switches_do_not_change_a_byte_of_an_early_end(gpu, monkeypatch, switch, value):
    """chained dlevmar_dif trials, the fused trial-to-trial step, candidates evaluated by the next Jacobian's pass, several
    projected-gradient candidates to a sweep: all evaluate ahead and must throw the sweep away when a stop or the cap fires.  The
    stop-rule and itmax tables and the box-active first passes at n = 5000, resident regime and launch chain: ret, p and info[]
    (the counters included) byte for byte those of the run with the switch at its other value"""
    cases = [c for _, c in P.switch_cases()]
    for regime in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
        monkeypatch.delenv(switch, raising=False)
        if regime not in _DEFAULT_RUNS:
            _DEFAULT_RUNS[regime] = [_single(gpu, c) for c in cases]
        monkeypatch.setenv(switch, value)
        differ = [(P.describe(c), a, b) for c, a in zip(cases, _DEFAULT_RUNS[regime]) for b in [_single(gpu, c)] if not _same(a, b)]
        assert not differ, (switch, regime, len(differ), differ[:5])
    print(f"{switch}={value}: {len(cases)} fits that end early, both regimes, byte-identical to the default (covariance included)")


def test_asking_for_the_covariance_changes_nothing_else(gpu, monkeypatch):
    """want_covar only adds B_FINISH's / D_FINISH's inversion: ret, p and info[] of the same fits, both regimes, byte for byte"""
    cases = [c for _, c in P.switch_cases()]
    for regime in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
        if regime not in _DEFAULT_RUNS:
            _DEFAULT_RUNS[regime] = [_single(gpu, c) for c in cases]
        differ = [(P.describe(c), a, b) for c, a in zip(cases, _DEFAULT_RUNS[regime]) for b in [_single(gpu, c, want_covar=False)] if not _same(a[:3], b)]
        assert not differ, (regime, len(differ), differ[:5])
        assert all(len(a) == 4 and a[3].shape == (3, 3) for a in _DEFAULT_RUNS[regime])
    print(f"want_covar: {len(cases)} fits, both regimes, ret / p / info byte-identical with and without")


# ---- channels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["1", "0"], ids=["shared_launch", "BRDF_HIP_CHANNELS=0"])
def test_channels_that_stop_at_different_iterations(gpu, monkeypatch, shared):
    """three measurement vectors over one set of planes whose fits end at the start point (reason 6), on a small gradient (reason 1)
    and on a small step (reason 2) under one opts -- in one shared launch (dlevmar_bc_dif / bc_der), one after the other (dlevmar_dif
    / der, and BRDF_HIP_CHANNELS=0); then itmax = 2 and itmax = 0.  Every channel, its covariance included, against the oracle, and
    bit for bit its single fit."""
    _, brdf_amd, _ = gpu
    monkeypatch.setenv("BRDF_HIP_CHANNELS", shared)
    tally = P.Tally(f"channels, BRDF_HIP_CHANNELS={shared}")
    for model in P.CHANNEL_TRUTHS:
        a = _planes(gpu, ("channel", model, P.CHANNEL_N, 0))[0]
        xd = _t(gpu, np.stack([P.problem(("channel", model, P.CHANNEL_N, c))[1] for c in range(3)]))
        for method in range(4):
            for row in P.channel_cases(model, method):
                lb, ub = P.box(row[0])
                kw = dict(lb=lb, ub=ub, itmax=row[0].itmax, opts=row[0].opts, want_covar=True)
                res = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], **kw)
                assert brdf_amd.last_channels_stats(3)["shared_launch"] == (shared == "1" and method in (1, 2)), P.describe(row[0])
                for c, case in enumerate(row):
                    got = (res[c].ret, res[c].p, res[c].info, res[c].covar)
                    tally.add(P.METHOD[method], case, got)
                    alone = _single(gpu, case)
                    assert _same(got, alone), (P.describe(case), got, alone)
    tally.check()


# ---- the covariance ---------------------------------------------------------------------------------------------------
REGIMES = (("resident", "1"), ("launch_chain", "0"))


def test_diagonal_scaling_covariance(gpu, monkeypatch):
    """dscl = (3, 1, 0.5) (the kernels fold the scales into the reduced products; B_FINISH multiplies by dscl[i] * dscl[j]): the box
    methods at itmax 1, 2, 3, n = 1000 and 5000, as single fits in both regimes and as three channels of one shared launch"""
    _, brdf_amd, _ = gpu
    for name, resident in REGIMES:
        monkeypatch.setenv("BRDF_HIP_RESIDENT", resident)
        tally = P.Tally(f"diagonal scaling, single fits, {name}")
        for cell, case in P.dscl_cases():
            tally.add(cell, case, _single(gpu, case))
        tally.check()
    monkeypatch.delenv("BRDF_HIP_RESIDENT")
    monkeypatch.setenv("BRDF_HIP_CHANNELS", "1")
    tally = P.Tally("diagonal scaling, three channels")
    for cell, case in P.dscl_cases():
        a, x = _planes(gpu, case.problem)
        lb, ub = P.box(case)
        res = brdf_amd.fit_channels(case.method, case.problem[1], a, x.repeat(3, 1), P.problem(case.problem)[2], lb=lb, ub=ub, dscl=case.dscl,
                                    itmax=case.itmax, opts=case.opts, want_covar=True)
        assert brdf_amd.last_channels_stats(3)["shared_launch"], P.describe(case)
        alone = _single(gpu, case)
        for r in res:
            got = (r.ret, r.p, r.info, r.covar)
            tally.add(cell, case, got)
            assert _same(got, alone), (P.describe(case), got, alone)
    tally.check()


@pytest.mark.parametrize("regime,resident", REGIMES)
def test_converged_covariance(gpu, monkeypatch, regime, resident):
    """fits that run to their own end, four methods x three models at n = 1000 and 5000: the counts differ from run to run, so
    ret >= 0, p, info[1] and the covariance are judged"""
    monkeypatch.setenv("BRDF_HIP_RESIDENT", resident)
    tally = P.Tally(f"converged fits, {regime}")
    for cell, case in P.converged_cases():
        tally.add(cell, case, _single(gpu, case))
    tally.check()


@pytest.mark.parametrize("method", range(4), ids=P.METHOD)
def test_converged_covariance_with_a_short_last_workgroup(gpu, method):
    """the same at n = 262145, one fit per method.  (The fit takes milliseconds; the test's time is the oracle's nine converged runs
    at this size: a few seconds for dlevmar_dif / der, 12 - 16 s for the box methods, whose searches take hundreds of evaluations)"""
    _, brdf_amd, _ = gpu
    tally = P.Tally(f"converged fit, n = 262145, {P.METHOD[method]}")
    for cell, case in P.converged_cases((P.SINGLE_REGIMES["short_last_workgroup"][0],)):
        if case.method == method:
            tally.add(cell, case, _single(gpu, case))
            assert brdf_amd.last_fit_stats()["launches"] == 1, P.describe(case)
    tally.check()


def test_drop_in_entries_return_the_same_covariance(gpu):
    """dlevmar_dif / dlevmar_bc_dif / dlevmar_bc_der / dlevmar_der on host arrays with BRDFFunc_hip / BRDFJac_hip and a covar array,
    n = 1000, itmax = 2: ret, p, info and the nine doubles are those of fit_single on the same inputs (which the tests above hold
    against the oracle)"""
    _, brdf_amd, _ = gpu
    fits = 0
    for model in (0, 1, 2):
        for method in range(4):
            for dscl in (None, P.DSCL) if method in (1, 2) else (None,):
                case = P.Case(("single", model, 1000), method, 2, synth.OPTS, dscl)
                angles, x, p0, _, _ = P.problem(case.problem)
                lb, ub = P.box(case)
                res = brdf_amd.host_dlevmar(method, model, angles, x, p0, lb=lb, ub=ub, dscl=dscl, itmax=2, opts=synth.OPTS, want_covar=True)
                got, alone = (res.ret, res.p, res.info, res.covar), _single(gpu, case)
                assert _same(got, alone) and np.all(np.diag(res.covar) > 0.0), (P.describe(case), got, alone)
                fits += 1
    print(f"drop-in entries: {fits} fits, ret / p / info / covar byte-identical to fit_single")


def test_covariance_where_the_reference_writes_none(gpu, monkeypatch):
    """nine zeros exactly at itmax = 0, at a stop before the first Jacobian (info[8] == 0: the first channel of the channel problems)
    and where J'J is singular (ks = 0 on its lower bound: the exponent's column is zero); a refused call (n < 3, lb > ub) leaves
    the caller's covar as it came"""
    torch, _, _ = gpu
    from brdf_amd._lib import D, ExtraData, lib
    zero = np.zeros((3, 3)).tobytes()
    for name, resident in REGIMES:
        monkeypatch.setenv("BRDF_HIP_RESIDENT", resident)
        tally = P.Tally(f"no covariance in the reference, {name}")
        for cell, case in P.zero_covar_cases():
            got = _single(gpu, case)
            tally.add(cell, case, got)
            assert got[3].tobytes() == zero, (P.describe(case), got)
        tally.check()
    # refused calls, through the C ABI with the caller's own covar memory
    angles, x, p0, lb, ub = P.problem(("single", 1, 1000))
    a_dev, x_dev = _planes(gpu, ("single", 1, 1000))
    flat = np.ascontiguousarray(angles.reshape(-1))
    sentinel = np.arange(1.0, 10.0) * 1.25
    opts = np.array(synth.OPTS)
    func, jacf = C.cast(lib.BRDFFunc_hip, C.c_void_p), C.cast(lib.BRDFJac_hip, C.c_void_p)
    for n, lo, hi in ((2, lb, ub), (1000, np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 100.0]))):
        for method in range(4):
            if n == 1000 and method not in (1, 2):
                continue
            bc = method in (1, 2)
            lo_a, hi_a = (np.array(lo), np.array(hi)) if bc else (None, None)
            for entry in ("brdf_hip_fit_dev", "dlevmar"):
                p, info, covar = np.array(p0), np.zeros(10), sentinel.copy()
                dp = lambda v: None if v is None else v.ctypes.data_as(D)
                if entry == "brdf_hip_fit_dev":
                    ret = lib.brdf_hip_fit_dev(method, 1, C.c_void_p(a_dev.data_ptr()), C.c_void_p(x_dev.data_ptr()), n, dp(p), dp(lo_a), dp(hi_a), None, 2,
                                               dp(opts), dp(info), dp(covar), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                else:
                    ed = ExtraData(dp(flat), 1)
                    if method == 0:
                        ret = lib.dlevmar_dif(func, dp(p), dp(x.copy()), 3, n, 2, dp(opts), dp(info), None, dp(covar), C.byref(ed))
                    elif method == 3:
                        ret = lib.dlevmar_der(func, jacf, dp(p), dp(x.copy()), 3, n, 2, dp(opts), dp(info), None, dp(covar), C.byref(ed))
                    elif method == 2:
                        ret = lib.dlevmar_bc_der(func, jacf, dp(p), dp(x.copy()), 3, n, dp(lo_a), dp(hi_a), None, 2, dp(opts), dp(info), None, dp(covar), C.byref(ed))
                    else:
                        ret = lib.dlevmar_bc_dif(func, dp(p), dp(x.copy()), 3, n, dp(lo_a), dp(hi_a), None, 2, dp(opts), dp(info), None, dp(covar), C.byref(ed))
                assert ret == -1 and covar.tobytes() == sentinel.tobytes() and p.tobytes() == np.array(p0).tobytes(), (entry, n, method, ret, covar, p)


# ---- batches ----------------------------------------------------------------------------------------------------------
def _batch(gpu, method, model, n, keys, itmax, opts, counts=None, stride=None):
    torch, brdf_amd, _ = gpu
    probs = [P.problem(k) for k in keys]
    stride = n if stride is None else stride
    angles, x = np.full((len(keys), 3, stride), np.nan), np.full((len(keys), stride), np.nan)
    for s, pr in enumerate(probs):
        angles[s, :, :pr[1].size], x[s, :pr[1].size] = pr[0], pr[1]
    bc = method in (1, 2)
    kw = {} if counts is None else {"counts": _t(gpu, np.asarray(counts, dtype=np.int32))}
    p, info, ret = brdf_amd.fit_batch(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, np.stack([pr[2] for pr in probs])), lb=probs[0][3] if bc else None,
                                      ub=probs[0][4] if bc else None, itmax=itmax, opts=opts, **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("kernel", list(P.BATCH_KERNELS))
def test_batch_kernels(gpu, monkeypatch, kernel):
    """every batched kernel, one launch per (size, model, method) under ONE opts and itmax = 3 that mixes fits which are over at the
    start point, fits that stop early and fits that reach the cap -- each judged on its own (a neighbour's early end must not leak
    into a fit that goes on); then itmax = 0"""
    env, sizes, methods = P.BATCH_KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tally = P.Tally(f"batch kernel {kernel}")
    for n in sizes:
        for itmax, opts in P.batch_settings(n):
            for model in (0, 1, 2):
                keys = P.batch_items(model, n)
                for method in methods:
                    p, info, ret = _batch(gpu, method, model, n, keys, itmax, opts)
                    for s, key in enumerate(keys):
                        tally.add(P.METHOD[method], P.Case(key, method, itmax, opts), (ret[s], p[s], info[s]))
    tally.check()


# ---- ragged and packed batches: the bytes of the uniform call ------------------------------------------------------------
EARLY_SETTINGS = ((2, synth.OPTS), (synth.ITMAX, (1e-3, 1e-1, 1e-2, 1e-20, 1e-6)), (0, synth.OPTS))
RAGGED = ((16, (3, 7, 16)), (64, (17, 33, 64)), (1024, (257, 1000)))


def test_ragged_and_packed_batches_that_end_early(gpu):
    """itmax = 2, loosened eps1 / eps2 and itmax = 0 through brdf_hip_fit_batch_ragged_dev and brdf_hip_fit_batch_packed_dev: every
    fit has the bytes of the uniform call on its own samples (which the tests above hold against the oracle)"""
    torch, brdf_amd, _ = gpu
    fits = 0
    for model in (1, 2):
        for method in (0, 1):
            lb, ub = synth.bounds(model) if method == 1 else (None, None)
            for itmax, opts in EARLY_SETTINGS:
                uniform = {}

                def alone(k, s):
                    if (k, s) not in uniform:
                        p, info, ret = _batch(gpu, method, model, k, [("surfel", model, k, s)], itmax, opts)
                        uniform[(k, s)] = (ret[0], p[0], info[0])
                    return uniform[(k, s)]

                for stride, counts in RAGGED:
                    items = [(k, 700 + j) for j in range(2) for k in counts]
                    p, info, ret = _batch(gpu, method, model, stride, [("surfel", model, k, s) for k, s in items], itmax, opts,
                                          counts=[k for k, _ in items], stride=stride)
                    for j, (k, s) in enumerate(items):
                        assert _same((ret[j], p[j], info[j]), alone(k, s)), ("ragged", model, method, itmax, stride, k, (ret[j], p[j], info[j]), alone(k, s))
                        fits += 1
                # packed: every size class in one call, a fit above 4096 samples among them
                items = [(k, 700) for k in (3, 16, 33, 257, 1000, 4100, 7, 64)]
                probs = [P.problem(("surfel", model, k, s)) for k, s in items]
                width = max(k for k, _ in items)
                angles, x = np.zeros((len(items), 3, width)), np.zeros((len(items), width))
                for j, pr in enumerate(probs):
                    angles[j, :, :pr[1].size], x[j, :pr[1].size] = pr[0], pr[1]
                pa, px, off = brdf_amd.pack_samples(_t(gpu, angles), _t(gpu, x), _t(gpu, np.array([k for k, _ in items], dtype=np.int32)))
                p, info, ret = brdf_amd.fit_batch_packed(method, model, pa, px, off, _t(gpu, np.stack([pr[2] for pr in probs])), lb=lb, ub=ub,
                                                         itmax=itmax, opts=opts)
                torch.cuda.synchronize()
                p, info, ret = p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
                for j, (k, s) in enumerate(items):
                    assert _same((ret[j], p[j], info[j]), alone(k, s)), ("packed", model, method, itmax, k, (ret[j], p[j], info[j]), alone(k, s))
                    fits += 1
    print(f"ragged and packed: {fits} fits that end early, byte-identical to the uniform call")
