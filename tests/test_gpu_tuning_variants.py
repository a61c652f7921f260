"""The kernel variants that only a tuning switch reaches (brdf_amd/csrc/fit_switches.h), run on the device and held to the bytes of the
default: ret, p, info[0..9] -- and the covariance where the entry returns one -- compared with tobytes() / on the device as int64 words.
The switches are read on every call, so they are set in this process.  Every test also reads an observable that shows the variant
ran and was not ignored: brdf_amd.last_batch_launch() (kernel code, waves per SIMD, grid, quorum, maxwait), last_fit_stats() (launches,
passes) or last_channels_stats() (shared_launch, passes).

  1. the lane-per-fit kernels at BRDF_HIP_LANE_WAVES = 2 and 4 (lane_fit.hip, weighted_fit.hip): the edge batches of
     tests/test_gpu_edges.py (also against the oracle), the application's 16-sample workload (test_gpu_parity.py's thresholds), a tiled
     batch of 2 * lanes + 3 fits in which every lane fetches again, and the same with ragged counts that end in a run of refusals;
  2. the lane scheduler at BRDF_HIP_LANE_QUORUM / BRDF_HIP_LANE_MAXWAIT = (1, 6), (64, 0), (64, 1000000), (8, 1) on the same inputs
     (nl == 0 forces a heavy round, so the loop makes progress for any quorum >= 1 and any maxwait >= 0: no other value is used);
  3. partial candidate sets, BRDF_HIP_PG_MULTI / BRDF_HIP_DIF_CHAIN / BRDF_HIP_BATCH_DIF_CHAIN = 2, 3, 5, 7 against 1 and 8: single
     fits (resident regime and launch chain), three channels in one launch, the wave / workgroup / eight-wave batched kernels;
  4. BRDF_HIP_RESIDENT_REPLICAS = 1, 2, 3, 5 against 8: single fits at 17,409 and 262,145 samples, three channels at 262,145;
  5. brdf_hip_fit_channels_dev with x_stride > n (NaN between the channels), shared launch and one channel after the other."""
import collections
import functools

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests import oracle_libs as L
from tests import pass_problems as P
from tests.test_gpu_edges import _batch_groups, _judge, _oracle, _run_batch, _tally, _three_channels

pytestmark = pytest.mark.gpu

LANE, ROWS, WAVE, WORKGROUP, EIGHT_WAVE, BIG512, WEIGHTED_LANE = range(7)  # brdf_hip_last_batch_launch's kernel codes
DEFAULT_PAIR = (24, 6)
PAIRS = ((1, 6), (64, 0), (64, 1000000), (8, 1))
PARTIAL = (1, 2, 3, 5, 7, 8)
REPLICAS = (1, 2, 3, 5, 8)
BOX_ACTIVE = ("tight_box", "start_on_bound", "diffuse_only")
P_TOL = 1e-5  # test_gpu_parity.py's


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: some problems are read-only)


def _env(monkeypatch, **switches):
    """BRDF_HIP_<NAME>=value; None: unset"""
    for name, value in switches.items():
        if value is None:
            monkeypatch.delenv("BRDF_HIP_" + name, raising=False)
        else:
            monkeypatch.setenv("BRDF_HIP_" + name, str(value))


def _lane_env(monkeypatch, waves, pair):
    _env(monkeypatch, LANE_WAVES=waves, LANE_QUORUM=None if pair is None else pair[0], LANE_MAXWAIT=None if pair is None else pair[1])


def _launched(gpu, kernel, waves=None, pair=None):
    """the last batched launch was `kernel` [with `waves` per SIMD and the scheduler pair]; -> its grid"""
    got = gpu[1].last_batch_launch()
    assert got is not None and got["kernel"] == kernel, (got, kernel)
    if waves is not None:
        assert (got["waves_per_simd"], got["quorum"], got["maxwait"]) == (waves,) + tuple(pair or DEFAULT_PAIR), (got, waves, pair)
    return got["grid"]


def _same_host(a, b):
    """tuples of numpy arrays (and ints), byte for byte"""
    return len(a) == len(b) and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


def _words(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_dev(gpu, a, b):
    """tuples of CUDA tensors (p, info: float64; ret: int32), byte for byte"""
    torch = gpu[0]
    return all(torch.equal(_words(u), _words(v)) for u, v in zip(a, b))


# ---- 1 (a) / 2: the edge batches ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_batches():
    """[(model, n, method, lb, ub, items)]: the batches test_batch_kernels_against_the_oracle["lane"] runs"""
    return [(model, n, method, lb, ub, items) for n in (3, 7, 15, 16) for model in (0, 1, 2) for lb, ub, items in _batch_groups(model, n, 6)
            for method in (1, 2)]


_EDGE_DEFAULT = []


def _edge_runs(gpu, monkeypatch, waves, pair):
    """(p, info, ret) of every edge batch with BRDF_HIP_LANE_WAVES=waves and the scheduler pair (None: unset)"""
    _lane_env(monkeypatch, waves, pair)
    out = []
    for model, n, method, lb, ub, items in _edge_batches():
        out.append(_run_batch(gpu, method, model, n, items))
        _launched(gpu, LANE, waves or 1, pair)
    return out


def _edge_default(gpu, monkeypatch):
    if not _EDGE_DEFAULT:
        _EDGE_DEFAULT.extend(_edge_runs(gpu, monkeypatch, None, None))
    return _EDGE_DEFAULT


@pytest.mark.parametrize("waves", [2, 4])
def test_lane_waves_edge_batches(gpu, monkeypatch, waves):
    """lane_fit_kernel<MODEL, FAST, W = 2 | 4> (and its exact twin) -- 256 / 128 registers per lane, the Jacobian loop with one row per
    trip only -- never ran in a test.  Refusals, box-active fits and non-positive cosines at n = 3, 7, 15, 16, dlevmar_bc_dif and
    bc_der: the bytes of W = 1, and against the oracle on test_batch_kernels_against_the_oracle's terms."""
    want = _edge_default(gpu, monkeypatch)
    got = _edge_runs(gpu, monkeypatch, waves, None)
    kinds, bad = collections.Counter(), []
    for (model, n, method, lb, ub, items), g, w in zip(_edge_batches(), got, want):
        assert _same_host(g, w), (waves, model, n, method, items)
        p, info, ret = g
        for s, (family, idx) in enumerate(items):
            _tally(kinds, bad, _judge((int(ret[s]), p[s], info[s]), _oracle(family, model, method, n, idx), lb, ub, n, method, model,
                                      E.make(family, model, n, idx)[0], (f"lane W={waves}", family, model, idx)))
    print(f"lane kernel, BRDF_HIP_LANE_WAVES={waves}: {dict(kinds)}")
    assert not bad, "\n".join(map(str, bad))
    assert kinds["failed"] >= 2 and kinds["oracle stopped short"] + kinds["flat"] <= 0.05 * sum(kinds.values()) + 2


# ---- 1 (b): the application's workload ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workload(model):
    """test_sixteen_sample_fits_fit_by_fit_against_the_oracle's inputs and the oracle's fits of them"""
    n, S = 16, 768
    angles, x, _ = synth.make_surfels(model, n, first=4000, count=S)
    x = np.round(np.clip(x, 0.0, 1.0) * 255.0) / 255.0
    refs = [L.brdf_fit("orc", 1, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB) for s in range(S)]
    return angles, x, refs


def _fit(gpu, method, model, a, x, p0, lb, ub, counts=None, w=None, itmax=synth.ITMAX):
    """fit_batch / fit_batch_weighted on device tensors; p0 is cloned (the call updates it in place).  -> (p, info, ret) on the device"""
    brdf_amd = gpu[1]
    kw = dict(lb=lb, ub=ub, itmax=itmax, opts=synth.OPTS, counts=counts)
    if w is None:
        return brdf_amd.fit_batch(method, model, a, x, p0.clone(), **kw)
    return brdf_amd.fit_batch_weighted(method, model, a, x, w, p0.clone(), **kw)


@pytest.mark.parametrize("model,exact_pow", [(1, "0"), (1, "1"), (0, "0"), (0, "1"), (2, "0")])
def test_lane_waves_application_workload(gpu, monkeypatch, model, exact_pow):
    """768 quantised 16-sample fits, dlevmar_bc_dif, through lane_fit_kernel<.., W = 2 | 4>, fast and exact instances: the bytes of
    W = 1, and (Phong, Blinn-Phong) that test's four thresholds against the oracle -- 0.7 S converge on both sides, 97 % of those
    within 1e-5 on p, 99 % of the objectives within 1e-6, none more than 30 % above."""
    angles, x, refs = _workload(model)
    S = x.shape[0]
    a, xd, p0 = _dev(gpu, angles), _dev(gpu, x), _dev(gpu, np.tile(np.array(synth.P0[model]), (S, 1)))
    _env(monkeypatch, EXACT_POW=exact_pow)
    outs = {}
    for waves in (1, 2, 4):
        _lane_env(monkeypatch, waves, None)
        outs[waves] = tuple(t.cpu().numpy() for t in _fit(gpu, 1, model, a, xd, p0, synth.LB, synth.UB))
        _launched(gpu, LANE, waves, None)
    for waves in (2, 4):
        assert _same_host(outs[waves], outs[1]), (model, exact_pow, waves)
        if model == 2:
            continue
        p, info, ret = outs[waves]
        both = close = near = 0
        worst = 0.0
        for s, (r, p_ref, info_ref) in enumerate(refs):
            assert (ret[s] >= 0) == (r >= 0), (s, ret[s], r)
            if r < 0:
                continue
            excess = (info[s, 1] - info_ref[1]) / max(info_ref[1], 1e-300)
            worst = max(worst, excess)
            near += int(excess <= 1e-6)
            if info_ref[6] != 3 and info[s, 6] != 3:
                both += 1
                close += int(L.rel_err(p[s], p_ref) <= P_TOL)
        print(f"n=16 model {model} exact_pow={exact_pow} W={waves}: {close}/{both} converged fits within 1e-5, {near}/{S} objectives within 1e-6, "
              f"worst objective excess {worst:.3e}")
        assert both >= 0.7 * S and close >= 0.97 * both, (close, both)
        assert near >= 0.99 * S and worst <= 0.3, (near, worst)


# ---- 1 (c), (d) / 2: a batch in which every lane fetches again -----------------------------------------------------------
BASE = 4099           # distinct surfels per model
COUNT_CYCLE = 17      # counts 0 ... 16
TAIL = 130            # the last fits of the ragged batch: all refused (count 2)
# the tiled batches' iteration cap.  A fit of these takes 15 ... 20 iterations where it converges and a third of them run into this
# cap, so both ends of a fit stay in; with synth.ITMAX the 14 % that reach 100 iterations (the exact twin's above all) make a call
# take 0.1 ... 0.7 s, which buys no other path through the rounds, the refill or the queue
TILED_ITMAX = 25
Tiled = collections.namedtuple("Tiled", "S angles x p0 counts w")
_TILED = {}
_TILED_DEFAULT = {}
KINDS = ("uniform", "ragged", "weighted_uniform", "weighted_ragged")


@functools.lru_cache(maxsize=None)
def _base_surfels(model):
    angles, x, _ = synth.make_surfels(model, 16, first=20000, count=BASE)
    x = np.round(np.clip(x, 0.0, 1.0) * 255.0) / 255.0
    if model in (0, 1):  # every seventh fit: one zero cosine in the powered plane -- the exact twin, through the queue (Ward has none)
        angles[::7, E.power_plane(model), 5] = 0.0
    w = np.random.default_rng([11, model]).integers(1, 301, size=(BASE, 16)).astype(np.float64)
    return angles, x, w


def _tiled(gpu, monkeypatch, model):
    """BASE surfels tiled on the device to S = 2 * grid * 64 + 3 fits, grid: what the launch with the most waves per CU (six at
    n = 16, BRDF_HIP_LANE_WAVES=4) starts for a batch that does not cap it"""
    torch, brdf_amd, dev = gpu
    if model not in _TILED:
        angles, x, w = (_dev(gpu, v) for v in _base_surfels(model))
        if "grid" not in _TILED:
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            idx = torch.arange(6 * cus * 64 + 1, device=dev) % BASE
            _lane_env(monkeypatch, 4, None)
            m = 0
            a0, x0 = (_dev(gpu, v) for v in _base_surfels(m)[:2])
            _fit(gpu, 1, m, a0[idx].contiguous(), x0[idx].contiguous(), _dev(gpu, np.array(synth.P0[m])).repeat(idx.numel(), 1), *synth.bounds(m),
                 itmax=1)
            torch.cuda.synchronize()
            _TILED["grid"] = _launched(gpu, LANE, 4, None)
            assert 0 < _TILED["grid"] <= 6 * cus
        S = 2 * _TILED["grid"] * 64 + 3
        s = torch.arange(S, device=dev)
        idx = s % BASE
        counts = (s % COUNT_CYCLE).to(torch.int32)
        counts[S - TAIL:] = 2
        _TILED[model] = Tiled(S, angles[idx].contiguous(), x[idx].contiguous(), _dev(gpu, np.array(synth.P0[model])).repeat(S, 1), counts,
                              w[idx].contiguous())
    return _TILED[model]


def _run_tiled(gpu, monkeypatch, model, kind, waves, pair, unit=False):
    """one call over the tiled batch; asserts the launch record and that lanes fetched again.  -> (p, info, ret) on the device"""
    torch = gpu[0]
    t = _tiled(gpu, monkeypatch, model)
    _lane_env(monkeypatch, waves, pair)
    w = None if not kind.startswith("weighted") else (torch.ones_like(t.w) if unit else t.w)
    out = _fit(gpu, 1, model, t.angles, t.x, t.p0, *synth.bounds(model), counts=t.counts if kind.endswith("ragged") else None, w=w, itmax=TILED_ITMAX)
    torch.cuda.synchronize()
    grid = _launched(gpu, LANE if w is None else WEIGHTED_LANE, waves or 1, pair)
    assert grid * 64 < t.S, (grid, t.S)  # every lane of the launch had a fit and fits were left: lanes did fetch again
    return out


def _tiled_default(gpu, monkeypatch, model, kind):
    if (model, kind) not in _TILED_DEFAULT:
        _TILED_DEFAULT[(model, kind)] = _run_tiled(gpu, monkeypatch, model, kind, None, None)
    return _TILED_DEFAULT[(model, kind)]


def _check_tiling(gpu, monkeypatch, model, kind, out):
    """fit s is fit s % BASE (ragged: s % (BASE * 17), the period of (surfel, count); the refused tail apart)"""
    torch = gpu[0]
    t = _tiled(gpu, monkeypatch, model)
    ragged = kind.endswith("ragged")
    period = BASE * COUNT_CYCLE if ragged else BASE
    upto = t.S - TAIL if ragged else t.S
    assert period < upto
    src = torch.arange(upto, device=out[0].device) % period
    for v in out:
        assert torch.equal(_words(v[:upto]), _words(v[:period][src])), (model, kind)
    p, info, ret = out
    assert bool((ret >= 0).any())
    if ragged:
        refused = t.counts < 3
        assert bool((ret[refused] == -1).all()) and bool((info[refused] == 0.0).all()) and torch.equal(_words(p[refused]), _words(t.p0[refused]))
        assert bool(refused[t.S - TAIL:].all()) and bool((ret[t.counts >= 3] >= 0).any())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", [0, 1, 2])
def test_lane_waves_refill(gpu, monkeypatch, model, kind):
    """The refill loop of lane_fit_kernel / lane_fit_weighted_kernel at W = 1, 2, 4 with more than twice as many fits as lanes (no test
    had a lane fetch a second fit at W > 1, nor the queue run dry inside the refill `while`): 4,099 quantised surfels tiled to
    2 * grid * 64 + 3 fits, every seventh with a zero cosine (the exact twin's queue); `ragged`: counts cycling 0 ... 16 with the last
    130 fits refused (count 2), so that lanes stay in `want` and fetch again while the queue runs dry.  Each W: the bytes of W = 1,
    and fit s those of fit s % 4099 (ragged: of the same surfel with the same count).  Through fit_batch_weighted: a fixed weight
    plane gives the same bytes at every W (and others than unit weights); unit weights give the unweighted call's bytes at every W."""
    want = _tiled_default(gpu, monkeypatch, model, kind)
    _check_tiling(gpu, monkeypatch, model, kind, want)
    for waves in (2, 4):
        assert _same_dev(gpu, _run_tiled(gpu, monkeypatch, model, kind, waves, None), want), (model, kind, waves)
    if kind.startswith("weighted"):
        unweighted = _tiled_default(gpu, monkeypatch, model, kind[len("weighted_"):])
        assert not _same_dev(gpu, want, unweighted)
        for waves in (1, 2, 4):
            assert _same_dev(gpu, _run_tiled(gpu, monkeypatch, model, kind, waves, None, unit=True), unweighted), (model, kind, waves)


SCHEDULES = [(pair, waves) for pair in PAIRS for waves in (1, 2)]
SCHEDULE_IDS = [f"{q}-{m}-W{w}" for (q, m), w in SCHEDULES]


@pytest.mark.parametrize("pair,waves", SCHEDULES, ids=SCHEDULE_IDS)
def test_lane_scheduling_edge_batches(gpu, monkeypatch, pair, waves):
    """heavy = nl == 0 || nh >= quorum || since_heavy >= maxwait (lane_fit.hip) only ever ran as 24 / 6.  No gating (1, 6), every round
    heavy (64, 0), a heavy round only when no lane has light work (64, 1000000: lanes wait longest for their Jacobian, their epilogue
    and their next fit) and (8, 1), at W = 1 and 2, on the edge batches (refusals inside the refill `while`, box-active fits, the
    exact twin): the bytes of the default schedule at W = 1."""
    for g, w, b in zip(_edge_runs(gpu, monkeypatch, waves, pair), _edge_default(gpu, monkeypatch), _edge_batches()):
        assert _same_host(g, w), (pair, waves, b[:3], b[5])


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("pair,waves", SCHEDULES, ids=SCHEDULE_IDS)
def test_lane_scheduling_refill(gpu, monkeypatch, pair, waves, model):
    """the same schedules in lane_fit.hip and weighted_fit.hip where a wave lives through many fits: the tiled batch and the ragged one
    with its run of refusals, weighted and not.  A lane that waits for a heavy round must keep its machine, its LDS samples and its
    count while its neighbours are refilled; a lane refused inside the refill must go on: the bytes of the default schedule at W = 1."""
    for kind in KINDS:
        want = _tiled_default(gpu, monkeypatch, model, kind)
        assert _same_dev(gpu, _run_tiled(gpu, monkeypatch, model, kind, waves, pair), want), (pair, waves, model, kind)


# ---- 3: partial candidate sets ---------------------------------------------------------------------------------------------
def _single(gpu, method, model, a, x, p0, lb, ub, opts):
    """-> ((ret, p, info, covar), passes, launches)"""
    brdf_amd = gpu[1]
    bc = method in (1, 2)
    r = brdf_amd.fit_single(method, model, a, x, p0, lb=lb if bc else None, ub=ub if bc else None, itmax=synth.ITMAX, opts=opts, want_covar=True)
    st = brdf_amd.last_fit_stats()
    return (r.ret, r.p, r.info, r.covar), st["passes"], st["launches"]


SINGLE_REGIMES = (("resident", 4097), ("resident", 17409), ("launch_chain", 5000))


def _across_values(gpu, monkeypatch, switch, regime, rows):
    """rows: [(family, what, run)] with run() -> (result, passes, launches).  Every row under switch = 1, 2, 3, 5, 7, 8: the same
    bytes, one launch in the resident regime, never more passes than one at a time -- and fewer at 8 (and fewer in total at 2, 3, 5,
    7: the guarded code did evaluate several candidates to a sweep) for at least one row per family."""
    fewer = collections.Counter()
    total = collections.Counter()
    for family, what, run in rows:
        got = {}
        for v in PARTIAL:
            _env(monkeypatch, **{switch: v})
            got[v] = run()
            assert (got[v][2] == 1) == (regime == "resident"), (switch, v, what, got[v][2])
            total[v] += got[v][1]
        for v in PARTIAL[1:]:
            assert _same_host(got[v][0], got[1][0]), (switch, v, what, got[v][0], got[1][0])
            assert got[v][1] <= got[1][1], (switch, v, what, got[v][1], got[1][1])
        fewer[family] += int(got[8][1] < got[1][1])
    _env(monkeypatch, **{switch: None})
    print(f"BRDF_HIP_{switch}, {regime}: passes in total {dict(total)}; rows with fewer passes at 8 than at 1: {dict(fewer)}")
    assert all(fewer[f] > 0 for f, _, _ in rows), fewer
    assert all(total[8] <= total[v] < total[1] for v in PARTIAL[1:-1]), total


@pytest.mark.parametrize("regime,n", SINGLE_REGIMES)
def test_pg_multi_partial_sets_single_fits(gpu, monkeypatch, regime, n):
    """BRDF_HIP_PG_MULTI = 2, 3, 5, 7: resident_fit_impl.h's guarded RQ_EVAL_MULTI body (`if (j < u.ncand)`) and the launch chain's
    are then the only multi-candidate code that runs (with 8 they run only where a search happens to be cut short).  The box-active
    families, three models, dlevmar_bc_dif and bc_der, covariance included."""
    _env(monkeypatch, RESIDENT="1" if regime == "resident" else "0")
    rows = []
    for family in BOX_ACTIVE:
        for model in (0, 1, 2):
            angles, x, p0, lb, ub = E.make(family, model, n, 0)
            a, xd = _dev(gpu, angles), _dev(gpu, x)
            for method in (1, 2):
                rows.append((family, (family, model, n, method), functools.partial(_single, gpu, method, model, a, xd, p0, lb, ub, synth.OPTS)))
    _across_values(gpu, monkeypatch, "PG_MULTI", regime, rows)


@pytest.mark.parametrize("regime,n", SINGLE_REGIMES)
def test_dif_chain_partial_sets_single_fits(gpu, monkeypatch, regime, n):
    """BRDF_HIP_DIF_CHAIN = 2, 3, 5, 7: lm_machine.h's ONE_LANE chain builder with `limit` below kMaxCand (the `j >= c.multi` breaks,
    `good >> j`) and the guarded trial sweep.  dlevmar_dif started undamped (tau = 1e-6: its first steps are rejected in a chain) and
    with the default options, three models, covariance included."""
    _env(monkeypatch, RESIDENT="1" if regime == "resident" else "0")
    rows = []
    for name in ("tau=1e-6", "default"):
        opts = synth.OPTS if name == "default" else P.OPTIONS[name]
        for model in (0, 1, 2):
            angles, x, p0, lb, ub = P.problem(("single", model, n))
            a, xd = _dev(gpu, angles), _dev(gpu, x)
            rows.append((name, (name, model, n), functools.partial(_single, gpu, 0, model, a, xd, p0, lb, ub, opts)))
    _across_values(gpu, monkeypatch, "DIF_CHAIN", regime, rows)


@pytest.mark.parametrize("switch,methods", [("PG_MULTI", (1, 2)), ("DIF_CHAIN", (0,))])
def test_partial_sets_do_not_change_a_byte_of_an_early_end(gpu, monkeypatch, switch, methods):
    """fits that end early (tests/pass_problems.py switch_cases(): itmax 0 ... 3, loosened stop rules, box-active first passes, n = 5000;
    for dlevmar_dif also itmax 1 ... 30 from an undamped start) with 2, 3, 5, 7 candidates to a sweep: what was evaluated ahead must be
    thrown away -- the bytes of one at a time and of 8, counters and covariance included, resident regime (one launch) and launch
    chain.  test_gpu_passes.py runs 1 against 8 only."""
    brdf_amd = gpu[1]
    cases = [c for _, c in P.switch_cases() if c.method in methods]
    if switch == "DIF_CHAIN":  # (dlevmar_dif tries one step per iteration, so a chain of rejections spans iterations and the cap can
        # fire inside one; the table's fits meet none: started undamped, a ladder of caps up to the fits' own ~35 iterations does)
        cases += [P.Case(("single", model, 5000), 0, k, P.OPTIONS["tau=1e-6"]) for model in (0, 1, 2) for k in (1, 2, 3, 6, 9, 12, 15, 20, 30)]
    planes = {}
    for c in cases:
        if c.problem not in planes:
            planes[c.problem] = tuple(_dev(gpu, v) for v in P.problem(c.problem)[:2])

    def run(c):
        a, x = planes[c.problem]
        lb, ub = P.box(c)
        r = brdf_amd.fit_single(c.method, c.problem[1], a, x, P.problem(c.problem)[2], lb=lb, ub=ub, itmax=c.itmax, opts=c.opts, want_covar=True)
        st = brdf_amd.last_fit_stats()
        return (r.ret, r.p, r.info, r.covar), st["passes"], st["launches"]

    for regime in ("1", "0"):
        _env(monkeypatch, RESIDENT=regime)
        total = collections.Counter()
        got = {}
        for v in PARTIAL:
            _env(monkeypatch, **{switch: v})
            got[v] = [run(c) for c in cases]
            total[v] = sum(g[1] for g in got[v])
            if regime == "1":
                assert all(g[2] == 1 for g in got[v]), (switch, v, [P.describe(c) for g, c in zip(got[v], cases) if g[2] != 1][:5])
            else:  # (test_single_fits' bar for the launch chain: a fit that is over at once may take one launch)
                assert sum(g[2] > 1 for g in got[v]) >= 0.8 * len(cases), (switch, v)
        _env(monkeypatch, **{switch: None})
        for v in PARTIAL[1:]:
            differ = [(P.describe(c), a[0], b[0]) for c, a, b in zip(cases, got[1], got[v]) if not _same_host(a[0], b[0])]
            assert not differ, (switch, regime, v, len(differ), differ[:5])
        print(f"BRDF_HIP_{switch}, BRDF_HIP_RESIDENT={regime}: {len(cases)} fits that end early, passes in total {dict(total)}")
        assert all(total[8] <= total[v] <= total[1] for v in PARTIAL[1:-1]) and total[8] < total[1], total  # candidates did share sweeps


def test_pg_multi_partial_sets_channels(gpu, monkeypatch):
    """BRDF_HIP_PG_MULTI = 2, 3, 5, 7 in channels_fit_impl.h's shared launch (its own guarded multi-candidate sweep): three channels over
    one set of planes, n = 5000 -- pass_problems.channel_problem (interior fits) and an interior / diffuse-only / dark triple whose
    searches run along the box -- dlevmar_bc_dif and bc_der, covariance included: the bytes of 1 and 8, in one launch."""
    brdf_amd = gpu[1]
    triples = [(model, P.problem(("channel", model, P.CHANNEL_N, 0))[0], np.stack([P.problem(("channel", model, P.CHANNEL_N, c))[1] for c in range(3)]))
               for model in P.CHANNEL_TRUTHS]
    triples += [(model,) + _three_channels(model, 5000) for model in (0, 1, 2)]
    total = collections.Counter()
    for model, angles, xs in triples:
        a, xd = _dev(gpu, angles), _dev(gpu, xs)
        lb, ub = synth.bounds(model)
        for method in (1, 2):
            got = {}
            for v in PARTIAL:
                _env(monkeypatch, PG_MULTI=v)
                res = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
                st = brdf_amd.last_channels_stats(3)
                assert st["shared_launch"], (model, method, v)
                got[v] = [(r.ret, r.p, r.info, r.covar) for r in res]
                total[v] += sum(c["passes"] for c in st["channels"])
            for v in PARTIAL[1:]:
                assert all(_same_host(x, y) for x, y in zip(got[v], got[1])), (model, method, v, got[v], got[1])
    print(f"BRDF_HIP_PG_MULTI, three channels in one launch: passes in total {dict(total)}")
    assert all(total[8] <= total[v] < total[1] for v in PARTIAL[1:-1]), total


BATCH_SIZES = ((64, WAVE), (256, WAVE), (1024, WORKGROUP), (1025, EIGHT_WAVE), (4096, EIGHT_WAVE))


@pytest.mark.parametrize("n,kernel", BATCH_SIZES)
def test_pg_multi_partial_sets_batches(gpu, monkeypatch, n, kernel):
    """BRDF_HIP_PG_MULTI = 2, 3, 5, 7 in batch_fit_kernel's guarded RQ_EVAL_MULTI body (one wave per fit with one and four samples per
    lane, one workgroup per fit) and the eight-wave kernel's: dlevmar_bc_dif on the interleaved edge families -- the bytes of 1 and 8."""
    for model in (0, 1, 2):
        for lb, ub, items in _batch_groups(model, n, 4 if n <= 1024 else 2):
            got = {}
            for v in PARTIAL:
                _env(monkeypatch, PG_MULTI=v)
                got[v] = _run_batch(gpu, 1, model, n, items)
                assert _launched(gpu, kernel) == len(items)
            for v in PARTIAL[1:]:
                assert _same_host(got[v], got[1]), (n, model, v, items)
            assert (got[1][2] >= 0).any()


@pytest.mark.parametrize("n", [1025, 4096])
def test_batch_dif_chain_partial_sets(gpu, monkeypatch, n):
    """BRDF_HIP_BATCH_DIF_CHAIN had no GPU test: the eight-wave batched kernel's dlevmar_dif chains at 1, 2, 3, 5, 7, 8 trial points to
    a sweep, twelve fits per model started undamped (tau = 1e-6) -- the same bytes; and unset with BRDF_HIP_DIF_CHAIN=3, which it
    then inherits."""
    torch, brdf_amd, dev = gpu
    S = 12
    for model in (0, 1, 2):
        angles, x, _ = synth.make_surfels(model, n, first=500, count=S)
        a, xd, p0 = _dev(gpu, angles), _dev(gpu, x), _dev(gpu, np.tile(np.array(synth.P0[model]), (S, 1)))

        def run():
            out = brdf_amd.fit_batch(0, model, a, xd, p0.clone(), itmax=synth.ITMAX, opts=P.OPTIONS["tau=1e-6"])
            torch.cuda.synchronize()
            assert _launched(gpu, EIGHT_WAVE) == S
            return tuple(t.cpu().numpy() for t in out)

        got = {}
        for v in PARTIAL:
            _env(monkeypatch, BATCH_DIF_CHAIN=v, DIF_CHAIN=None)
            got[v] = run()
        _env(monkeypatch, BATCH_DIF_CHAIN=None, DIF_CHAIN=3)
        got["inherited"] = run()
        for v in list(PARTIAL[1:]) + ["inherited"]:
            assert _same_host(got[v], got[1]), (n, model, v)
        ran = got[1][2] >= 0  # (the undamped start sends one Phong fit into a NaN: the oracle's reason 7 too)
        assert ran.sum() >= S - 1 and (got[1][1][ran, 5] > 0).all()


# ---- 4: copies of the exchange's group rows ----------------------------------------------------------------------------------
def _replica_rows(gpu, n):
    rows = []
    for method in range(4):
        for model in ((0, 1, 2) if n < 100000 else (P.SHORT_LAST_MODEL[method],)):
            angles, x, p0, lb, ub = P.problem(("single", model, n))
            a, xd = _dev(gpu, angles), _dev(gpu, x)
            rows.append(((model, n, method, "default"), functools.partial(_single, gpu, method, model, a, xd, p0, lb, ub, synth.OPTS)))
            if method == 0 and n < 100000:  # chains of rejected trials: another row width of the exchange
                rows.append(((model, n, method, "tau=1e-6"), functools.partial(_single, gpu, method, model, a, xd, p0, lb, ub, P.OPTIONS["tau=1e-6"])))
    return rows


@pytest.mark.parametrize("n", [17409, 262145])
def test_resident_replicas_single_fits(gpu, monkeypatch, n):
    """BRDF_HIP_RESIDENT_REPLICAS = 1, 2, 3, 5 (only 8 ever ran): leaders store copies 0 ... replicas-1 of the group rows and every
    workgroup gathers copy blockIdx.x % replicas (resident_fit_impl.h, control_exchange), so a value that is no power of two and the
    value 1 change which lines every workgroup polls.  n = 17,409 (two groups, a leader that is not member 0; four methods x three
    models) and 262,145 (256 workgroups, a short last one; one model per method): the bytes of 8, in ONE launch -- writers and
    readers that disagree would show only as the fallback to the launch chain."""
    _env(monkeypatch, RESIDENT="1")
    for what, run in _replica_rows(gpu, n):
        got = {}
        for v in REPLICAS:
            _env(monkeypatch, RESIDENT_REPLICAS=v)
            got[v] = run()
            assert got[v][2] == 1, (what, v, got[v][2])
        assert got[8][0][0] >= 0, (what, got[8])
        for v in REPLICAS[:-1]:
            assert _same_host(got[v][0], got[8][0]) and got[v][1] == got[8][1], (what, v, got[v], got[8])


def test_resident_replicas_channels(gpu, monkeypatch):
    """the same in channels_fit_impl.h's shared launch: three channels at n = 262,145 (256 workgroups), dlevmar_bc_dif (Blinn-Phong) and
    bc_der (Ward) -- the bytes of 8, in one shared launch"""
    brdf_amd = gpu[1]
    for model, method in ((1, 1), (2, 2)):
        angles, xs = _three_channels(model, 262145)
        a, xd = _dev(gpu, angles), _dev(gpu, xs)
        lb, ub = synth.bounds(model)
        got = {}
        for v in REPLICAS:
            _env(monkeypatch, RESIDENT_REPLICAS=v)
            res = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
            assert brdf_amd.last_channels_stats(3)["shared_launch"], (model, method, v)
            got[v] = [(r.ret, r.p, r.info, r.covar) for r in res]
        assert all(r[0] >= 0 for r in got[8])
        for v in REPLICAS[:-1]:
            assert all(_same_host(x, y) for x, y in zip(got[v], got[8])), (model, method, v, got[v], got[8])


# ---- 5: channels that are not next to each other -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5000, 300])
def test_channels_with_a_stride_between_them(gpu, monkeypatch, n):
    """brdf_hip_fit_channels_dev's x_stride (the Python binding always passed n): channel c at d_x + c * (n + 37), NaN in the gaps --
    the `d_x + c * x_stride` of channels_fit.hip's shared launch and of its one-after-the-other path.  K = 3, dlevmar_bc_dif and
    bc_der, three models: the bytes of the contiguous call, finite results."""
    torch, brdf_amd, dev = gpu
    stride = n + 37
    for model in (0, 1, 2):
        angles, xs = _three_channels(model, n)
        lb, ub = synth.bounds(model)
        a, xd = _dev(gpu, angles), _dev(gpu, xs)
        wide = torch.full((3, stride), float("nan"), dtype=torch.float64, device=dev)
        wide[:, :n] = xd
        for method in (1, 2):
            kw = dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
            for channels in (None, "0"):
                _env(monkeypatch, CHANNELS=channels)
                want = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], **kw)
                assert brdf_amd.last_channels_stats(3)["shared_launch"] == (channels is None)
                got = brdf_amd.fit_channels(method, model, a, wide, synth.P0[model], x_stride=stride, **kw)
                assert brdf_amd.last_channels_stats(3)["shared_launch"] == (channels is None)
                for c in range(3):
                    g, w = got[c], want[c]
                    assert _same_host((g.ret, g.p, g.info, g.covar), (w.ret, w.p, w.info, w.covar)), (n, model, method, channels, c, g, w)
                    assert np.isfinite(g.p).all() and np.isfinite(g.info).all() and np.isfinite(g.covar).all(), (n, model, method, c, g)
