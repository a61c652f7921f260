"""Per-pass parity on the device (tests/pass_problems.py): fits cut short by itmax = 1, 2, 3, by a loosened stop rule, by itmax = 0,
with opts = NULL, other tau and delta, in every fit regime -- ret, p, info[0..4] against the oracle within each case's own
tolerance (8 x what the oracle itself moves under re-ordered sums and model values disturbed by the device's documented error;
capped at 1e-8 / 1e-6), info[5..9] exactly.  A Jacobian column that is off, a sample dropped from J'e, a damping update off by a
factor or a speculative evaluation that is counted all show here, where the fixed point (tests/test_gpu_parity.py) hides them.
tests/test_oracle_passes.py judges the same case lists on the CPU first (the reference alone, and the host-driven machines).

Every test prints its summary: cases compared, cases the yardstick does not admit, the worst difference / tolerance per field."""
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


def _single(gpu, case):
    _, brdf_amd, _ = gpu
    a, x = _planes(gpu, case.problem)
    lb, ub = P.box(case)
    res = brdf_amd.fit_single(case.method, case.problem[1], a, x, P.problem(case.problem)[2], lb=lb, ub=ub, itmax=case.itmax, opts=case.opts)
    return res.ret, res.p, res.info


def _same(a, b):
    return int(a[0]) == int(b[0]) and np.asarray(a[1]).tobytes() == np.asarray(b[1]).tobytes() and np.asarray(a[2]).tobytes() == np.asarray(b[2]).tobytes()


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
    print(f"{switch}={value}: {len(cases)} fits that end early, both regimes, byte-identical to the default")


# ---- channels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["1", "0"], ids=["shared_launch", "BRDF_HIP_CHANNELS=0"])
def test_channels_that_stop_at_different_iterations(gpu, monkeypatch, shared):
    """three measurement vectors over one set of planes whose fits end at the start point (reason 6), on a small gradient (reason 1)
    and on a small step (reason 2) under one opts -- in one shared launch (dlevmar_bc_dif / bc_der), one after the other (dlevmar_dif
    / der, and BRDF_HIP_CHANNELS=0); then itmax = 2 and itmax = 0.  Every channel against the oracle, and bit for bit its single fit."""
    _, brdf_amd, _ = gpu
    monkeypatch.setenv("BRDF_HIP_CHANNELS", shared)
    tally = P.Tally(f"channels, BRDF_HIP_CHANNELS={shared}")
    for model in P.CHANNEL_TRUTHS:
        a = _planes(gpu, ("channel", model, P.CHANNEL_N, 0))[0]
        xd = _t(gpu, np.stack([P.problem(("channel", model, P.CHANNEL_N, c))[1] for c in range(3)]))
        for method in range(4):
            for row in P.channel_cases(model, method):
                lb, ub = P.box(row[0])
                kw = dict(lb=lb, ub=ub, itmax=row[0].itmax, opts=row[0].opts)
                res = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], **kw)
                assert brdf_amd.last_channels_stats(3)["shared_launch"] == (shared == "1" and method in (1, 2)), P.describe(row[0])
                for c, case in enumerate(row):
                    got = (res[c].ret, res[c].p, res[c].info)
                    tally.add(P.METHOD[method], case, got)
                    alone = _single(gpu, case)
                    assert _same(got, alone), (P.describe(case), got, alone)
    tally.check()


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
