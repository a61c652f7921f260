"""Per-pass parity: the cases, the yardstick and the comparison that tests/test_oracle_passes.py (CPU) and
tests/test_gpu_passes.py (GPU) share.  CPU only.

The fixed point of a fit hides a wrong pass: LM reaches the same minimiser with a Jacobian column that is off, a J'e that
drops a sample or a damping update off by a factor -- by another path.  So a fit is cut short here -- by itmax = 1, 2, 3, by a
loosened stop rule, by itmax = 0 -- and everything it returns is compared with the oracle: ret, p, info[0..4] within the case's
tolerance, info[5..9] (iterations, reason, nfev, njev, nlss) exactly.

A case is (problem, method, itmax, opts[, dscl]).  yardstick(case) says how tightly the oracle alone determines its result: the oracle
is run once as it is, on four seeded permutations of the samples (the difference a tree sum makes) and four times with every
model value -- and, for the analytic methods, every Jacobian entry -- multiplied by 1 + k * 2^-53, k uniform in [-K, K] per
value and per call, K = 8 (the bound test_model_values_match_oracle holds the device's model values to) plus |p2 * log c| for
Phong / Blinn-Phong (the documented error of the fast path's exp(p2 log c), brdf_models.h).  A case is `stable` if ret and
info[5..9] are the same in all nine runs.  Its tolerance is 8 x the spread of the eight re-runs, per field, relative, with a
floor of 64 * 2^-53: the device's tree order is one more draw from the population the permutations sample, and eight times the
maximum of eight draws is the margin.  A case is compared only if it is stable and its tolerance is <= 1e-8 on p, info[0],
info[1] and <= 1e-6 on info[2..4] (conditions, not measurements: a loose yardstick must not hide a wrong pass -- a dropped
sample at n = 5000 is 2e-4, a wrong FD step is percent-sized).  At most 10 % of a test's cases may go uncompared and no
(regime, method) cell may be left with none compared.

Where the reference never forms a Jacobian (info[8] == 0: itmax = 0, or a stop at the start point by eps3) it returns info[2] and
info[4] from memory it never wrote; these two are not compared there.  At itmax = 0 only ret = 0, p == p0, info[0] == info[1],
info[5..9] = 0, 3, 1, 0, 0 are defined.

The covariance (results that carry one: the single-fit entries) is one more field, `covar`: the difference is max over i, j of
|C_ij - C_ref_ij| / sqrt(C_ref_ii * C_ref_jj), the tolerance 8 x the spread of the eight re-runs with the same floor.  It is compared
where the case is stable (a converged case: where all nine runs end with reason 1 or 2), all nine covariances are finite with a
positive diagonal and the tolerance is <= 1e-6 (an n for n - 3 at n = 262145 is 1.1e-5, a missing dscl factor or a damped diagonal
is percent-sized).  Where the reference writes nothing defined -- itmax = 0, info[8] == 0, a J'J that orc_covar finds singular (the
NaN the array was filled with survives) -- the product returns nine zeros, and that is asserted.  At most 10 % of a test's
covariances may be left out and no cell with none judged.  A case may carry dscl (the box methods).  Converged cases
(converged_cases: synth.ITMAX, synth.OPTS) change their counts from run to run: only ret >= 0, p, info[1] and covar are judged.

Measured with the oracle alone (tests/test_oracle_passes.py prints them): cases compared / uncompared, and the largest tolerance
(8 x spread) among the compared ones

    table          compared  uncompared   p        info[0]  info[1]  info[2]  info[3]  info[4]
    first passes      376     38 (9.2 %)  8.6e-09  1.3e-13  9.3e-09  5.6e-07  2.4e-07  4.7e-09
    options           184      8 (4.2 %)  8.7e-09  1.6e-14  9.2e-09  5.0e-07  1.4e-07  1.8e-07
    stop rules        267     14 (5.0 %)  1.0e-08  1.8e-14  9.7e-09  6.3e-07  5.9e-07  2.1e-07
    itmax = 0          12      0          (defined fields only)

    covar: judged  left out     largest tolerance     |  list               judged  left out    largest tolerance
    first passes      374     40 (9.7 %)  6.2e-07     |  diagonal scaling       36      0          6.8e-10
    options           176     16 (8.3 %)  1.3e-07     |  converged fits         22      2 (8.3 %)  2.8e-08
    stop rules        264     17 (6.0 %)  3.0e-07     |  single fits, n = 5000 256      2 (0.8 %)  8.2e-09
    itmax = 0          12      0          (nine zeros)|  channels               72      0          3.0e-10

With 8 units of model-value noise the uncompared cases are nearly all dlevmar_bc_dif (and dlevmar_dif at n = 16): its forward
difference with step 1e-6 turns 8 * 2^-53 on a model value into 1e-9 on a Jacobian entry, and 8 x that is the cap.  The
box-active families alone leave 31 of 270 uncompared (start_on_bound and diffuse_only, where an iterate sits on a corner of the
box and round-off decides which components are free); six of them change their counts.  The GPU case lists: single fits 1.9 - 4.0 %
uncompared, channels 2.8 %, batch kernels 0.3 - 5.6 % (n = 16: 2.8 - 5.6 %).
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import zlib

import numpy as np

from brdf_amd import synth
from tests import edge_problems as E
from tests import oracle_libs as L

U = 2.0 ** -53
FLOOR = 64 * U
MARGIN = 8.0
OWN_UNITS = 8.0  # |model value error| of the device in units of 2^-53 (test_model_values_match_oracle: 4 eps)
CAP_P, CAP_INFO = 1e-8, 1e-6  # a case whose tolerance exceeds these is not compared
MAX_UNCOMPARED = 0.10
MAX_STOP_ITERATIONS = 12
METHOD = ("dif", "bc_dif", "bc_der", "der")
FIELDS = ("p", "info0", "info1", "info2", "info3", "info4")
BOX_FAMILIES = ("tight_box", "high_lb", "start_on_bound", "diffuse_only", "shiny_beyond_box", "ward_mirror")

Case = collections.namedtuple("Case", "problem method itmax opts dscl", defaults=(None,))  # dscl: the box methods' diagonal scaling
# covar: the oracle's 3x3 (NaN where it wrote nothing); covar_rule: "compare", "zeros" (the reference writes nothing defined: the
# product's nine values are 0.0) or "left out"; settled: all nine runs end with reason 1 or 2 (converged_cases)
Yard = collections.namedtuple("Yard", "ret p info stable spread tol comparable covar covar_rule settled")


def _with(i, v):
    o = list(synth.OPTS)
    o[i] = v
    return tuple(o)


FIRST_ITMAX = (1, 2, 3)
OPTIONS = {"none": None, "tau=1": _with(0, 1.0), "tau=1e-6": _with(0, 1e-6), "delta=1e-3": _with(4, 1e-3), "delta=-1e-4": _with(4, -1e-4)}
STOPS = {"eps1=1e-2": _with(1, 1e-2), "eps1=1e-1": _with(1, 1e-1), "eps2=1e-2": _with(2, 1e-2), "eps2=1e-1": _with(2, 1e-1),
         "eps3=1e-1": _with(3, 1e-1), "eps3=1": _with(3, 1.0)}


# ---- problems ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(key):
    """key -> (angles[3,n], x[n], p0[3], lb[3], ub[3]).  ("single", model, n): synth.make_single; ("surfel", model, n, s): surfel s
    of synth.make_surfels; ("near", model, n, s): the surfel's planes with measurements at the model's start point plus its noise
    (a fit that is over before it starts); ("zero_ks", model, n): make_single started with ks = 0; ("channel", model, CHANNEL_N, c): channel_problem; (family, model, n, idx): tests/edge_problems.py.  Box: synth.bounds(model)."""
    kind, model, n = key[:3]
    if kind in E.FAMILIES:
        out = E.make(kind, model, n, key[3])
    elif kind == "channel":
        out = channel_problem(model, key[3])
    else:
        lb, ub = (np.array(b, dtype=np.float64) for b in synth.bounds(model))
        p0 = np.array(synth.P0[model], dtype=np.float64)
        if kind in ("single", "zero_ks"):
            angles, x, _ = synth.make_single(model, n)
            if kind == "zero_ks":
                p0[1] = 0.0
        else:
            a, xs, _ = synth.make_surfels(model, n, first=key[3], count=1)
            angles, x = a[0], xs[0]
            if kind == "near":
                x = x - synth.model_value(model, synth.surfel_truth(model, key[3], 1)[0], *angles) + synth.model_value(model, p0, *angles)
            elif kind != "surfel":
                raise ValueError(key)
        out = (np.ascontiguousarray(angles), np.ascontiguousarray(x), p0, lb, ub)
    for a in out:
        a.setflags(write=False)
    return out


def box(case):
    """(lb, ub) the case's method takes: the problem's for dlevmar_bc_dif / bc_der, none otherwise"""
    _, _, _, lb, ub = problem(case.problem)
    return (lb, ub) if case.method in (1, 2) else (None, None)


def scaling(case):
    """dscl the case's method takes: the case's for dlevmar_bc_dif / bc_der, none otherwise"""
    return case.dscl if case.method in (1, 2) else None


# ---- the oracle, as it is and disturbed -------------------------------------------------------------------------------
class _Extra(C.Structure):
    _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]


_FUNC = C.CFUNCTYPE(None, L.D, L.D, C.c_int, C.c_int, C.c_void_p)


def _noisy_fit(method, model, angles, x, p0, itmax, opts, lb, ub, rng, dscl=None):
    """the oracle's entry point of `method` with callbacks that wrap orc_brdf_func / orc_brdf_jac: every value they return is
    multiplied by 1 + k * 2^-53, |k| <= OWN_UNITS (+ |p2 log c| for Phong / Blinn-Phong)"""
    a = L.f64(angles)
    xx = L.f64(x)
    n = xx.size
    ed = _Extra(L.ptr(a), model)
    c = {0: angles[2], 1: angles[1]}.get(model)
    logc = None if c is None else np.abs(np.log(np.where(c > 0.0, c, 1.0)))

    def bound(p):
        return OWN_UNITS if logc is None else OWN_UNITS + abs(p[2]) * logc

    @_FUNC
    def func(p, hx, m, n_, adata):
        L.orc.orc_brdf_func(p, hx, m, n_, C.byref(ed))
        h = np.ctypeslib.as_array(hx, (n_,))
        h *= 1.0 + rng.uniform(-1.0, 1.0, n_) * bound(p) * U

    @_FUNC
    def jacf(p, jac, m, n_, adata):
        L.orc.orc_brdf_jac(p, jac, m, n_, C.byref(ed))
        j = np.ctypeslib.as_array(jac, (n_, m))
        j *= 1.0 + rng.uniform(-1.0, 1.0, (n_, m)) * (np.asarray(bound(p)) * U).reshape(-1, 1)

    p = L.f64(p0).copy()
    info = np.zeros(10)
    covar = np.full(9, np.nan)  # (NaN: "never written" shows)
    o = L.f64(opts)
    l, u, d = (None if v is None else L.f64(v).copy() for v in (lb, ub, dscl))  # (copies: the reference scales the box in place)
    f, jf, cv = C.cast(func, C.c_void_p), C.cast(jacf, C.c_void_p), L.ptr(covar)
    if method == 0:
        r = L.orc.orc_dlevmar_dif(f, L.ptr(p), L.ptr(xx), 3, n, itmax, L.ptr(o), L.ptr(info), None, cv, None)
    elif method == 3:
        r = L.orc.orc_dlevmar_der(f, jf, L.ptr(p), L.ptr(xx), 3, n, itmax, L.ptr(o), L.ptr(info), None, cv, None)
    elif method == 2:
        r = L.orc.orc_dlevmar_bc_der(f, jf, L.ptr(p), L.ptr(xx), 3, n, L.ptr(l), L.ptr(u), L.ptr(d), itmax, L.ptr(o), L.ptr(info), None, cv, None)
    else:
        r = L.orc.orc_dlevmar_bc_dif(f, L.ptr(p), L.ptr(xx), 3, n, L.ptr(l), L.ptr(u), L.ptr(d), itmax, L.ptr(o), L.ptr(info), None, cv, None)
    return r, p, info, covar.reshape(3, 3)


def _rel(a, b, floor):
    """|a - b| / max(|b|, floor), elementwise; 0 where the two are the same value (inf and NaN included)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), floor)
    d = np.where(same, 0.0, d)
    return float(np.max(np.where(np.isnan(d), np.inf, d)))


def differences(p, info, p_ref, info_ref):
    """per field of FIELDS: the relative difference from the reference values (p: the largest component, |p_ref| floored at 1e-6,
    so that a component at round-off above a bound of 0 is compared on the parameters' scale)"""
    out = {"p": _rel(p, p_ref, 1e-6)}
    for i in range(5):
        out[f"info{i}"] = _rel(info[i], info_ref[i], 1e-300)
    return out


def undefined(info_ref):
    """fields the reference leaves undefined: a fit that ends before its first Jacobian (info[8] == 0: a stop at the start point by
    eps3, like itmax = 0) returns info[2] and info[4] from memory it never wrote -- the oracle's differ from run to run"""
    return ("info2", "info4") if info_ref[8] == 0 else ()


def covar_difference(c, c_ref):
    """max over i, j of |C_ij - C_ref_ij| / sqrt(C_ref_ii * C_ref_jj): the difference on the scale of the reference's standard
    deviations, which removes the parameters' units (inf where either holds a non-finite value or the diagonal is not positive)"""
    c, c_ref = np.asarray(c, dtype=np.float64).reshape(3, 3), np.asarray(c_ref, dtype=np.float64).reshape(3, 3)
    d = np.diag(c_ref)
    if not (np.all(np.isfinite(c)) and np.all(np.isfinite(c_ref)) and np.all(d > 0.0)):
        return np.inf
    s = np.sqrt(d)
    return float(np.max(np.abs(c - c_ref) / np.outer(s, s)))


def _proper(c):
    return bool(np.all(np.isfinite(c)) and np.all(np.diag(c) > 0.0))


def _seed(case):
    """the seed of a case's disturbed runs: that of the four-field Case for a case without dscl"""
    name = f"Case(problem={case.problem!r}, method={case.method!r}, itmax={case.itmax!r}, opts={case.opts!r})"
    return zlib.crc32((name if case.dscl is None else repr(case)).encode())


@functools.lru_cache(maxsize=None)
def yardstick(case) -> Yard:
    angles, x, p0, _, _ = problem(case.problem)
    lb, ub = box(case)
    dscl = scaling(case)
    model = case.problem[1]
    base = L.brdf_fit_covar("orc", case.method, model, angles, x, p0, case.itmax, case.opts, lb, ub, dscl)
    seed = _seed(case)
    runs = []
    for k in range(4):
        perm = np.random.default_rng([seed, k]).permutation(x.size)
        runs.append(L.brdf_fit_covar("orc", case.method, model, angles[:, perm], x[perm], p0, case.itmax, case.opts, lb, ub, dscl))
    for k in range(4):
        runs.append(_noisy_fit(case.method, model, angles, x, p0, case.itmax, case.opts, lb, ub, np.random.default_rng([seed, 4 + k]), dscl))
    stable = all(r[0] == base[0] and np.array_equal(r[2][5:], base[2][5:]) for r in runs)
    spread = {f: 0.0 for f in FIELDS}
    if case.itmax > 0:  # (itmax = 0: info[2], info[4] are undefined, p == p0 -- nothing to measure)
        for r in runs:
            for f, d in differences(r[1], r[2], base[1], base[2]).items():
                spread[f] = max(spread[f], d)
    for f in undefined(base[2]):
        spread[f] = 0.0
    tol = {f: max(MARGIN * s, FLOOR) for f, s in spread.items()}
    comparable = (stable and all(tol[f] <= CAP_P for f in ("p", "info0", "info1")) and all(tol[f] <= CAP_INFO for f in ("info2", "info3", "info4")))
    settled = all(r[0] >= 0 and r[2][6] in (1.0, 2.0) for r in [base] + runs)
    # the covariance: nothing defined at itmax = 0, before the first Jacobian, and where orc_covar found J'J singular (the NaN fill
    # survives); compared where the case is stable (a converged case: settled), all nine are finite with a positive diagonal and
    # 8 x the spread is within the cap
    if case.itmax <= 0 or base[2][8] == 0 or np.all(np.isnan(base[3])):
        rule = "zeros"
    else:
        rule = "left out"
        if (stable or (converged(case) and settled)) and all(_proper(r[3]) for r in [base] + runs):
            spread["covar"] = max(covar_difference(r[3], base[3]) for r in runs)
            tol["covar"] = max(MARGIN * spread["covar"], FLOOR)
            if tol["covar"] <= CAP_INFO:
                rule = "compare"
    return Yard(base[0], base[1], base[2], stable, spread, tol, comparable, base[3], rule, settled)


def converged(case):
    """a case of converged_cases: the fit runs to its own end under synth.ITMAX and synth.OPTS"""
    return case.itmax == synth.ITMAX and case.opts == synth.OPTS


# ---- the comparison ---------------------------------------------------------------------------------------------------
def covar_problem(case, covar):
    """a returned covariance against the oracle's.  -> (rule, ratio, problem): rule is the yardstick's covar_rule; ratio: difference /
    tolerance where it is compared (None otherwise); problem: None, or what is wrong, in words"""
    y = yardstick(case)
    c = np.asarray(covar, dtype=np.float64).reshape(3, 3)
    if y.covar_rule == "zeros":
        if not (np.array_equal(c, np.zeros((3, 3))) and not np.any(np.signbit(c))):
            return "zeros", None, f"covar {c.tolist()} where the reference writes none: nine zeros expected"
        return "zeros", None, None
    if y.covar_rule != "compare":
        return y.covar_rule, None, None
    r = covar_difference(c, y.covar) / y.tol["covar"]
    return "compare", r, None if r <= 1.0 else f"covar: {r:.3g} x its tolerance {y.tol['covar']:.3g} (got {c.tolist()}, oracle {y.covar.tolist()})"


def compare(case, got):
    """one result (ret, p[3], info[10]) or (ret, p[3], info[10], covar[3,3]) against the oracle's.  -> (compared, ratios, problem):
    compared is False for a case the yardstick does not admit; ratios: per field, difference / tolerance; problem: None, or what is
    wrong, in words.  The covariance is judged by its own rule (covar_problem), whether or not the other fields are admitted; a
    "zeros" case is judged where the other fields are."""
    ret, p, info = int(got[0]), np.asarray(got[1], dtype=np.float64), np.asarray(got[2], dtype=np.float64)
    covar = got[3] if len(got) > 3 else None
    if case.itmax <= 0:
        wrong = itmax0_problem(case, (ret, p, info))
        if wrong is None and covar is not None and covar_problem(case, covar)[2]:
            wrong = f"{describe(case)}: {covar_problem(case, covar)[2]}"
        return True, {}, wrong
    y = yardstick(case)
    if converged(case):
        return _compare_converged(case, y, ret, p, info, covar)
    ratios, wrong = {}, []
    if y.comparable:
        ratios = {f: d / y.tol[f] for f, d in differences(p, info, y.p, y.info).items() if f not in undefined(y.info)}
        if ret != y.ret:
            wrong.append(f"ret {ret} != {y.ret}")
        if not np.array_equal(info[5:], y.info[5:]):
            wrong.append(f"info[5..9] {info[5:].tolist()} != {y.info[5:].tolist()}")
        wrong += [f"{f}: {r:.3g} x its tolerance {y.tol[f]:.3g}" for f, r in ratios.items() if not r <= 1.0]
    if covar is not None and (y.comparable or y.covar_rule == "compare"):
        _, r, w = covar_problem(case, covar)
        if r is not None:
            ratios["covar"] = r
        if w:
            wrong.append(w)
    if wrong:
        return y.comparable, ratios, f"{describe(case)}: " + "; ".join(wrong) + f" (got p {p.tolist()} info {info.tolist()}, oracle p {y.p.tolist()} info {y.info.tolist()})"
    return y.comparable, ratios, None


def converged_comparable(y):
    """p of a fit that ran to its own end is as sharp as its stop rule, not as a single pass: the 8 x the spread of the oracle's own p
    reaches 2.4e-8 (Blinn-Phong dlevmar_dif, n = 1000), so the cap on p is CAP_INFO here; info[1] keeps CAP_P"""
    return y.settled and y.tol["p"] <= CAP_INFO and y.tol["info1"] <= CAP_P


def _compare_converged(case, y, ret, p, info, covar):
    """a fit that runs to its own end: the counts differ from run to run, so only ret >= 0, p, info[1] and the covariance are judged"""
    ok = converged_comparable(y)
    ratios, wrong = {}, []
    if ok:
        d = differences(p, info, y.p, y.info)
        ratios = {f: d[f] / y.tol[f] for f in ("p", "info1")}
        if ret < 0:
            wrong.append(f"ret {ret}")
        wrong += [f"{f}: {r:.3g} x its tolerance {y.tol[f]:.3g}" for f, r in ratios.items() if not r <= 1.0]
    if covar is not None and y.covar_rule == "compare":
        _, r, w = covar_problem(case, covar)
        ratios["covar"] = r
        if w:
            wrong.append(w)
    if wrong:
        return ok, ratios, f"{describe(case)}: " + "; ".join(wrong) + f" (got p {p.tolist()} info {info.tolist()}, oracle p {y.p.tolist()} info {y.info.tolist()})"
    return ok, ratios, None


def itmax0_problem(case, got):
    """itmax = 0: the reference returns info[2] and info[4] from memory it never wrote (and info[3] from its initial value); what is
    defined is ret = 0, p == p0 bit for bit (for the box methods: p0 projected on the box), info[0] == info[1] == the oracle's,
    info[5] = 0, info[6] = 3, info[7] = 1, info[8] = info[9] = 0"""
    ret, p, info = got[:3]
    y = yardstick(case)
    wrong = []
    if ret != 0 or y.ret != 0:
        wrong.append(f"ret {ret} (oracle {y.ret})")
    if not np.array_equal(p, y.p):
        wrong.append(f"p {p.tolist()} != {y.p.tolist()}")
    if info[0] != info[1] or _rel(info[0], y.info[0], 1e-300) > 64 * FLOOR:
        wrong.append(f"info[0], info[1] = {info[0]!r}, {info[1]!r}, oracle {y.info[0]!r}")
    if info[5:].tolist() != [0.0, 3.0, 1.0, 0.0, 0.0] or y.info[5:].tolist() != [0.0, 3.0, 1.0, 0.0, 0.0]:
        wrong.append(f"info[5..9] {info[5:].tolist()} (oracle {y.info[5:].tolist()})")
    return None if not wrong else f"{describe(case)}: " + "; ".join(wrong)


def describe(case):
    name = next((k for k, v in {**OPTIONS, **STOPS}.items() if v == case.opts), "default" if case.opts == synth.OPTS else str(case.opts))
    return f"{case.problem} {METHOD[case.method]} itmax={case.itmax} opts:{name}" + ("" if case.dscl is None else f" dscl:{case.dscl}")


def admitted(case):
    """whether the yardstick admits the case's ret, p and info to the comparison"""
    y = yardstick(case)
    return case.itmax <= 0 or (converged_comparable(y) if converged(case) else y.comparable)


def covar_judged(case):
    """whether a returned covariance of the case is judged: compared with the oracle's, or asserted to be nine zeros"""
    y = yardstick(case)
    if y.covar_rule == "zeros":
        return case.itmax <= 0 or y.comparable
    return y.covar_rule == "compare"


class Tally:
    """what a test prints and asserts about its cases: compared / uncompared per cell, the worst ratio per field; for results that
    carry a covariance, the same count for the covariance alone"""

    def __init__(self, name):
        self.name, self.cells, self.worst, self.bad = name, collections.defaultdict(lambda: [0, 0]), {f: 0.0 for f in FIELDS + ("covar",)}, []
        self.covar_cells = collections.defaultdict(lambda: [0, 0])

    def add(self, cell, case, got):
        compared, ratios, wrong = compare(case, got)
        self.cells[cell][0 if compared else 1] += 1
        if len(got) > 3 and got[3] is not None:
            self.covar_cells[cell][0 if covar_judged(case) else 1] += 1
        for f, r in ratios.items():
            self.worst[f] = max(self.worst[f], r)
        if wrong is not None:
            self.bad.append(f"[{cell}] {wrong}")
        return wrong is None

    def summary(self):
        comp, unc = sum(c[0] for c in self.cells.values()), sum(c[1] for c in self.cells.values())
        cov = ""
        if self.covar_cells:
            cov = f"covar: {sum(c[0] for c in self.covar_cells.values())} judged, {sum(c[1] for c in self.covar_cells.values())} left out; "
        return (f"{self.name}: {comp} compared, {unc} uncompared, {len(self.bad)} wrong; {cov}worst difference / tolerance: "
                + ", ".join(f"{f} {r:.2g}" for f, r in self.worst.items() if f != "covar" or self.covar_cells))

    def check(self):
        print(self.summary())
        assert not self.bad, "\n".join(self.bad[:20])
        for what, cells in (("", self.cells), ("covar", self.covar_cells)):
            comp, unc = sum(c[0] for c in cells.values()), sum(c[1] for c in cells.values())
            assert unc <= MAX_UNCOMPARED * (comp + unc), (self.name, what, comp, unc)
            empty = [k for k, c in cells.items() if c[0] == 0]
            assert not empty, (self.name, what, "cells with nothing compared", empty)


# ---- case tables ------------------------------------------------------------------------------------------------------
def fd(method):
    return method in (0, 1)


def option_cases(prob, method, itmax=3):
    return [Case(prob, method, itmax, o) for k, o in OPTIONS.items() if fd(method) or not k.startswith("delta")]


def stop_cases(prob, method):
    """the loosened stop rules at itmax = 100 under which the oracle stops within MAX_STOP_ITERATIONS iterations"""
    out = []
    for o in STOPS.values():
        case = Case(prob, method, synth.ITMAX, o)
        if yardstick(case).info[5] <= MAX_STOP_ITERATIONS:
            out.append(case)
    return out


def first_cases(prob, method):
    return [Case(prob, method, k, synth.OPTS) for k in FIRST_ITMAX]


TABLE_N = (16, 64, 1000, 5000)
BOX_N = (16, 64, 1000)


@functools.lru_cache(maxsize=None)
def tables():
    """table -> [(cell, case)].  first passes: synth.make_single and the six box-active families, itmax 1, 2, 3 (cell: kind of problem
    and method); options; stop rules; itmax = 0 (cell: the method)"""
    t = collections.OrderedDict((k, []) for k in ("first passes", "options", "stop rules", "itmax = 0"))
    for model in (0, 1, 2):
        for n in TABLE_N:
            prob = ("single", model, n)
            for method in range(4):
                t["first passes"] += [("single " + METHOD[method], c) for c in first_cases(prob, method)]
                t["options"] += [(METHOD[method], c) for c in option_cases(prob, method)]
                t["stop rules"] += [(METHOD[method], c) for c in stop_cases(prob, method)]
                if n == 64:
                    t["itmax = 0"].append((METHOD[method], Case(prob, method, 0, synth.OPTS)))
    for family in BOX_FAMILIES:
        for model in E.FAMILIES[family]:
            for n in BOX_N:
                for method in (1, 2):
                    t["first passes"] += [("box " + METHOD[method], c) for c in first_cases((family, model, n, 0), method)]
    return t


def start_point_stops(cases):
    """the cases of `cases` whose oracle run stops at the start point: {reason: [case]}"""
    out = collections.defaultdict(list)
    for c in cases:
        y = yardstick(c)
        if c.itmax > 0 and y.info[5] == 0:
            out[int(y.info[6])].append(c)
    return out


# ---- the cases of tests/test_gpu_passes.py (here, so that the CPU test can judge them before any GPU run) -----------------------
SINGLE_REGIMES = {"one_workgroup": (64, 1000, 4096), "resident": (5000,), "launch_chain": (5000,), "short_last_workgroup": (262145,)}
SHORT_LAST_MODEL = {0: 2, 1: 1, 2: 0, 3: 2}  # n = 262145: one model per method


def box_first_cases(n):
    return [(METHOD[method], c) for family in BOX_FAMILIES for model in E.FAMILIES[family] for method in (1, 2)
            for c in first_cases((family, model, n, 0), method)]


@functools.lru_cache(maxsize=None)
def single_cases(n):
    """[(cell, case)] of the single fits at n samples: first passes and itmax = 0 at every size; the options and the stop rules at
    n = 1000 and 5000; the box-active families at n = 64 and 5000; n = 262145: itmax = 2 and 0, one model per method"""
    out = []
    if n > 100000:
        for method, model in SHORT_LAST_MODEL.items():
            out += [(METHOD[method], Case(("single", model, n), method, k, synth.OPTS)) for k in (2, 0)]
        return out
    for model in (0, 1, 2):
        prob = ("single", model, n)
        for method in range(4):
            cases = first_cases(prob, method) + [Case(prob, method, 0, synth.OPTS)]
            if n in (1000, 5000):
                cases += option_cases(prob, method) + stop_cases(prob, method)
            out += [(METHOD[method], c) for c in cases]
    if n in (64, 5000):
        out += box_first_cases(n)
    return out


@functools.lru_cache(maxsize=None)
def switch_cases(n=5000):
    """[(cell, case)]: the stop-rule and itmax tables at n samples, and the box-active first passes (the projected-gradient search)"""
    out = []
    for model in (0, 1, 2):
        prob = ("single", model, n)
        for method in range(4):
            out += [(METHOD[method], c) for c in first_cases(prob, method) + [Case(prob, method, 0, synth.OPTS)] + stop_cases(prob, method)]
    return out + box_first_cases(n)


# the covariance under diagonal scaling: the box methods, itmax 1, 2, 3.  3.0 is no power of two, so scales folded into the sums show
DSCL = (3.0, 1.0, 0.5)
COVAR_N = (1000, 5000)


@functools.lru_cache(maxsize=None)
def dscl_cases():
    return [(METHOD[method], Case(("single", model, n), method, k, synth.OPTS, DSCL)) for model in (0, 1, 2) for n in COVAR_N for method in (1, 2)
            for k in FIRST_ITMAX]


CONVERGED_LARGE_MODEL = {0: 0, 1: 0, 2: 1, 3: 2}  # n = 262145: per method, the model whose nine oracle runs take the least time


@functools.lru_cache(maxsize=None)
def converged_cases(sizes=COVAR_N):
    """fits that run to their own end (n = 64 stays out: Ward dlevmar_dif ends at itmax there); at n = 262145 one model per method"""
    return [(METHOD[method], Case(("single", model, n), method, synth.ITMAX, synth.OPTS)) for n in sizes for method in range(4)
            for model in ((0, 1, 2) if n < 100000 else (CONVERGED_LARGE_MODEL[method],))]


def singular_cases():
    """a J'J that is singular exactly: Phong / Blinn-Phong started with ks = 0 on lb = 0 -- the column of the exponent is ks * (...)
    = 0 at p and at p + delta, so the Crout LU sees a zero row, orc_covar reports "singular matrix" and leaves covar as it came"""
    return [(METHOD[method], Case(("zero_ks", model, n), method, 1, synth.OPTS)) for model in (0, 1) for n in (1000, 5000) for method in (1, 2)]


@functools.lru_cache(maxsize=None)
def zero_covar_cases():
    """[(cell, case)] where the reference writes no covariance: itmax = 0; a stop at the start point before the first Jacobian (the
    first channel of the channel problems under CHANNEL_OPTS); the singular cases, and the box-active first passes that are singular
    of themselves"""
    rows = [(METHOD[method], Case(("channel", model, CHANNEL_N, 0), method, synth.ITMAX, CHANNEL_OPTS)) for model in CHANNEL_TRUTHS for method in range(4)]
    rows += singular_cases() + [(cell, c) for cell, c in switch_cases() if yardstick(c).covar_rule == "zeros"]
    return [(cell, c) for cell, c in rows if admitted(c)]


# channels: one set of planes (synth.make_single's), three measurement vectors, one opts.  Under CHANNEL_OPTS the first is over at
# the start point (reason 6), the second stops on a small gradient (reason 1), the third on a small step (reason 2), at different
# iterations (dlevmar_bc_dif / bc_der, the methods that share a launch) -- asserted by tests/test_oracle_passes.py
CHANNEL_OPTS = (1e-3, 1e-1, 1e-2, 1e-1, 1e-6)
CHANNEL_N = 5000
CHANNEL_TRUTHS = {1: ((0.35, 0.6, 24.0), (0.6, 0.9, 3.0)), 2: ((0.6, 0.1, 0.3), (0.35, 0.25, 0.15))}
CHANNEL_SETTINGS = ((synth.ITMAX, CHANNEL_OPTS), (2, synth.OPTS), (0, synth.OPTS))


def channel_problem(model, c):
    angles, _, _ = synth.make_single(model, CHANNEL_N)
    rng = np.random.default_rng([77, model, CHANNEL_N, c])
    noise = rng.random(CHANNEL_N) - 0.5
    if c == 0:
        x = synth.model_value(model, synth.P0[model], *angles) + 0.01 * noise
    else:
        x = synth.model_value(model, CHANNEL_TRUTHS[model][c - 1], *angles) + 0.05 * noise
    lb, ub = (np.array(b, dtype=np.float64) for b in synth.bounds(model))
    return np.ascontiguousarray(angles), np.ascontiguousarray(x), np.array(synth.P0[model]), lb, ub


def channel_cases(model, method):
    """[[case of channel 0, 1, 2] per setting]"""
    return [[Case(("channel", model, CHANNEL_N, c), method, itmax, opts) for c in range(3)] for itmax, opts in CHANNEL_SETTINGS]


# batches: kernel -> (environment, sample counts, methods), the kernels of BATCH_KERNELS in tests/test_gpu_edges.py
BATCH_KERNELS = {
    "lane": ({}, (16,), (1, 2)),
    "rows": ({"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "1"}, (16,), (0, 1)),
    "wave16": ({"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "0"}, (16,), (0, 1, 2, 3)),
    "wave": ({}, (64, 256), (0, 1, 2, 3)),
    "workgroup": ({}, (1024,), (0, 1, 2, 3)),
    "eight_wave": ({}, (4096,), (0, 1, 2, 3)),
    "big_off": ({"BRDF_HIP_BATCH_BIG": "0"}, (4096,), (0, 1)),
    "one_by_one": ({}, (4097,), (0, 1, 2, 3)),
}
BATCH_ITMAX = 3


def batch_opts(n):
    """one opts for a whole batch under which, with itmax = BATCH_ITMAX, some fits are over at the start point (the "near" problems:
    ||e||^2 ~ n * 8.3e-6 <= eps3), some stop early on a small gradient or step, and the rest reach the cap"""
    return (1e-3, 1e-1, 1e-1, 2e-5 * n, 1e-6)


def batch_items(model, n):
    """problem keys of one batch: every fourth is over before it starts, among ordinary surfels (twelve fits; six above 4096 samples)"""
    return [("near" if s % 4 == 1 else "surfel", model, n, 500 + s) for s in range(12 if n <= 4096 else 6)]


def batch_settings(n):
    return ((BATCH_ITMAX, batch_opts(n)), (0, synth.OPTS))


def batch_rows(kernel):
    """[(cell, case)] of every fit the kernel's test makes"""
    _, sizes, methods = BATCH_KERNELS[kernel]
    return [(METHOD[m], Case(key, m, itmax, opts)) for n in sizes for itmax, opts in batch_settings(n) for model in (0, 1, 2) for m in methods
            for key in batch_items(model, n)]
