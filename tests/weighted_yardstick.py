"""The yardstick of the weighted-fit tests (test infrastructure only; never the code under test).

A weighted fit is levmar on hx_i = sqrt(w_i) f_i(p) against x'_i = sqrt(w_i) x_i.  The reference side poses exactly that problem to
the compiled reference's dlevmar_bc_dif (oracle/_ref/liblevmar_ref.so) through a ctypes callback that calls orc_brdf_func and
multiplies by sqrt(w); where oracle/_ref was not built, to orc_dlevmar_bc_dif the same way (the two agree bit for bit on weighted
fits).  The statistics side scales stats_yardstick.reference_stats' rows and residuals by sqrt(w) and inverts J^T W J with the
reference's dlevmar_covar."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from brdf_amd import synth
from tests import oracle_libs as L
from tests import stats_yardstick as Y

_FUNC = C.CFUNCTYPE(None, L.D, L.D, C.c_int, C.c_int, C.c_void_p)
_BC_DIF = L.ref.dlevmar_bc_dif if L.ref is not None else L.orc.orc_dlevmar_bc_dif


def quantised_surfels(model: int, count: int, first: int = 4000, n: int = 16):
    """synth.make_surfels with the capture's 8-bit measurements (GetIntensities_FromPixel: value / 255)"""
    angles, x, _ = synth.make_surfels(model, n, first=first, count=count)
    x = np.round(np.clip(x, 0.0, 1.0) * 255.0) / 255.0
    return np.ascontiguousarray(angles), np.ascontiguousarray(x)


def weighted_fit(model: int, angles, x, w, p0, *, lb, ub, itmax=synth.ITMAX, opts=synth.OPTS):
    """One weighted dlevmar_bc_dif fit of the n samples given (angles [3,n], x [n], w [n]) -> (ret, p [3], info [10])."""
    a, xx = L.f64(angles), L.f64(x)
    sw = np.sqrt(L.f64(w))
    n = xx.size
    ed = Y._Extra(L.ptr(a), model)

    def func(p, hx, m, nn, adata):
        L.orc.orc_brdf_func(p, hx, m, nn, C.c_void_p(adata))  # (a bare int would travel as a 32-bit value)
        out = np.ctypeslib.as_array(hx, shape=(nn,))
        out *= sw

    cb = _FUNC(func)
    p, info = L.f64(p0).copy(), np.zeros(10)
    xs = np.ascontiguousarray(sw * xx)
    r = _BC_DIF(cb, L.ptr(p), L.ptr(xs), 3, n, L.ptr(L.f64(lb)), L.ptr(L.f64(ub)), None, itmax, L.ptr(L.f64(opts)), L.ptr(info), None, None,
                C.byref(ed))
    return int(r), p, info


def weighted_fits(model: int, angles, x, w, counts=None):
    """S weighted fits from synth.P0 in synth's box -> (ret [S], p [S,3], info [S,10]); counts: each fit's first counts[s] samples"""
    S, n = x.shape
    lb, ub = synth.bounds(model)
    ret, p, info = np.zeros(S, dtype=np.int32), np.zeros((S, 3)), np.zeros((S, 10))
    for s in range(S):
        k = n if counts is None else int(counts[s])
        ret[s], p[s], info[s] = weighted_fit(model, angles[s][:, :k], x[s][:k], w[s][:k], synth.P0[model], lb=lb, ub=ub)
    return ret, p, info


@functools.lru_cache(maxsize=None)
def reference_case(model: int, S: int = 768):
    """the inputs of the fit-by-fit comparison and the reference's side of it: (angles, x, w, ret, p, info)"""
    angles, x = quantised_surfels(model, S)
    w = np.random.default_rng(100 + model).integers(1, 301, size=x.shape).astype(np.float64)
    return (angles, x, w) + weighted_fits(model, angles, x, w)


def parity_figures(ret, p, info, ret_ref, p_ref, info_ref):
    """test_sixteen_sample_fits_fit_by_fit_against_the_oracle's figures: (fits converged on both sides, of those within 1e-5 on p,
    objectives within 1e-6 of the reference's or better, worst relative objective excess); asserts success on both sides or neither"""
    both = close = near = 0
    worst = 0.0
    for s in range(len(ret)):
        assert (ret[s] >= 0) == (ret_ref[s] >= 0), (s, ret[s], ret_ref[s])
        if ret_ref[s] < 0:
            near += 1
            continue
        excess = (info[s, 1] - info_ref[s, 1]) / max(info_ref[s, 1], 1e-300)
        worst = max(worst, excess)
        near += int(excess <= 1e-6)
        if info_ref[s, 6] != 3 and info[s, 6] != 3:
            both += 1
            close += int(L.rel_err(p[s], p_ref[s]) <= 1e-5)
    return both, close, near, worst


def weighted_reference_stats(kind: int, model: int, angles, x, w, p, nobs=None, extra_ss: float = 0.0, delta: float = 1e-6):
    """stats_yardstick.reference_stats of the weighted problem at p: its J rows and e scaled by sqrt(w), C from the reference's
    dlevmar_covar on J^T W J with nobs observations, SStot about the weighted mean; extra_ss added to sumsq and SStot."""
    ref = Y.reference_stats(kind, model, angles, x, p, delta)
    xx, ww = L.f64(x), L.f64(w)
    sw = np.sqrt(ww)
    n = xx.size
    nobs = n if nobs is None else int(nobs)
    hx = L.model_values(model, angles, p)
    J = ref["J"] * sw[:, None]
    e = sw * (xx - hx)
    with np.errstate(all="ignore"):
        sumsq = float(e @ e) + extra_ss
        A = np.ascontiguousarray(J.T @ J)
        cov, rank = np.zeros((3, 3)), 0
        if np.all(np.isfinite(A)) and np.isfinite(sumsq):
            rank = int(Y._COV(L.ptr(A), L.ptr(cov), C.c_double(sumsq), 3, nobs))
        if not np.all(np.isfinite(cov)) or np.any(np.diag(cov) < 0):
            rank = 0
        if rank and not np.all(np.isfinite(cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov))))):
            rank = 0
        cond = float(np.linalg.cond(A)) if np.all(np.isfinite(A)) else np.inf
        mean = float((ww * xx).sum() / ww.sum())
        sstot = float((ww * (xx - mean) ** 2).sum()) + extra_ss
        r2 = float(1.0 - np.float64(sumsq) / np.float64(sstot))
    shx = sw * hx
    return dict(sumsq=sumsq, sstot=sstot, R2=r2, J=J, A=A, C=cov if rank else np.zeros((3, 3)), rank=rank, cond=cond,
                fmax=float(np.max(np.abs(shx))), d=ref["d"], fnorm=float(np.linalg.norm(shx)), n=n)


def compare_weighted_stats(kind, model, angles, x, w, p, covar, stats, rank, counts=None, nobs=None, extra_ss=None, max_left_out=0.35, label=""):
    """stats_yardstick.compare for the weighted pass: sumsq to E_TOL, R2 through the bound on sumsq, rank, and C / sigma / rho to
    covar_bound on the scaled quantities, on the fits whose reference rank is 3 with cond <= 1e8 (at least 65 % of them)."""
    S = x.shape[0]
    worst, compared = 0.0, 0
    for s in range(S):
        k = x.shape[1] if counts is None else int(counts[s])
        ref = weighted_reference_stats(kind, model, angles[s][:, :k], x[s][:k], w[s][:k], p[s], None if nobs is None else nobs[s],
                                       0.0 if extra_ss is None else float(extra_ss[s]))
        who = (label, model, s)
        assert abs(stats[s, 0] - ref["sumsq"]) <= Y.E_TOL * ref["sumsq"], (who, stats[s, 0], ref["sumsq"])
        ratio = ref["sumsq"] / ref["sstot"]
        tol = Y.MARGIN * (Y.sumsq_bound(ref) + ref["n"] * Y.EPS) * ratio + 4 * Y.EPS * max(1.0, abs(ref["R2"]))
        assert abs(stats[s, 1] - ref["R2"]) <= tol, (who, stats[s, 1], ref["R2"], tol)
        if rank[s] != ref["rank"]:
            assert ref["cond"] > Y.COND_RANK, (who, int(rank[s]), ref["rank"], ref["cond"])
        if rank[s] == 0:
            assert np.all(covar[s] == 0.0) and np.all(stats[s, 2:] == 0.0), who
        if ref["rank"] != 3 or not ref["cond"] <= Y.COND_CUT:
            continue
        compared += 1
        assert rank[s] == 3, who
        bound = Y.covar_bound(kind, ref)
        c2 = float(np.linalg.norm(ref["C"], 2))
        err = float(np.linalg.norm(covar[s] - ref["C"], 2)) / c2
        worst = max(worst, err / bound)
        assert err <= bound, (who, err, bound, ref["cond"])
        sd = stats[s, 2:5]
        assert np.all(np.abs(sd * sd - np.diag(ref["C"])) <= bound * c2 * (1 + 1e-12) + 4 * Y.EPS * np.diag(ref["C"])), (who, sd, np.diag(ref["C"]))
        for kk, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            assert abs(stats[s, 5 + kk] * sd[i] * sd[j] - ref["C"][i, j]) <= bound * c2 * (1 + 1e-12) + 8 * Y.EPS * sd[i] * sd[j], (who, i, j)
    assert compared >= (1.0 - max_left_out) * S, (label, model, compared, S)
    print(f"weighted stats {label} model {model} kind {kind}: {compared}/{S} fits compared on C, worst error / bound = {worst:.3e}")
    return worst, compared, S
