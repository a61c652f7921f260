"""The yardstick of the fit-statistics tests (test infrastructure only): covariance, sigma, rho and R^2 of a BRDF fit at a
given p from the REFERENCE's side -- the compiled reference's dlevmar_fdif_forw_jac_approx / dlevmar_fdif_cent_jac_approx /
dlevmar_covar / dlevmar_R2 (oracle/_ref, misc.c) where it was built, the restated orc_fdif_forward / orc_fdif_central /
orc_covar otherwise, both driven with orc_brdf_func -- and the first-order perturbation bound a device result is held to.
Never the code under test."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from brdf_amd import synth
from tests import oracle_libs as L

EPS = float(np.finfo(np.float64).eps)
K_ULP = 4.0      # device vs host libm on one model value (tests/test_gpu_parity.py::test_model_values_match_oracle)
AN_TOL = 1e-13   # device vs oracle analytic Jacobian entry, times max(1, max|J|) (tests/test_gpu_parity.py:715)
MARGIN = 8.0     # for the second-order terms the first-order bound drops
E_TOL = 1e-8     # the project's bound on ||e||^2
COND_CUT = 1e8   # fits compared on C, sigma, rho: reference rank 3 and cond(J^T J) <= this
COND_RANK = 1e12  # a differing rank is tolerated only beyond this

FORWARD, CENTRAL, ANALYTIC = 0, 1, 2


class _Extra(C.Structure):
    _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]


_CB = C.cast(L.orc.orc_brdf_func, C.c_void_p)
if L.ref is not None:
    _FWD, _CEN, _COV = L.ref.dlevmar_fdif_forw_jac_approx, L.ref.dlevmar_fdif_cent_jac_approx, L.ref.dlevmar_covar
    L.ref.dlevmar_R2.restype = C.c_double
else:
    _FWD, _CEN, _COV = L.orc.orc_fdif_forward, L.orc.orc_fdif_central, L.orc.orc_covar


def jac_kind(method: int, opts) -> int:
    if method in (2, 3):
        return ANALYTIC
    return CENTRAL if (opts is not None and opts[4] < 0) else FORWARD


def reference_stats(kind: int, model: int, angles, x, p, delta: float = 1e-6):
    """One fit at p -> dict(sumsq, sstot, R2, J [n,3], A = J^T J, C [3,3], rank, cond, fmax, d [3])."""
    a, xx, pp = L.f64(angles), L.f64(x), L.f64(p).copy()
    n = xx.size
    ed = _Extra(L.ptr(a), model)
    hx = np.zeros(n)
    L.orc.orc_brdf_func(L.ptr(pp), L.ptr(hx), 3, n, C.byref(ed))
    jac = np.zeros((n, 3))
    d = np.maximum(np.abs(1e-4 * pp), delta)  # misc_core.c:155-158
    if kind == ANALYTIC:
        L.orc.orc_brdf_jac(L.ptr(pp), L.ptr(jac), 3, n, C.byref(ed))
    elif kind == FORWARD:
        _FWD(_CB, L.ptr(pp), L.ptr(hx), L.ptr(np.zeros(n)), C.c_double(delta), L.ptr(jac), 3, n, C.byref(ed))
    else:
        _CEN(_CB, L.ptr(pp), L.ptr(np.zeros(n)), L.ptr(np.zeros(n)), C.c_double(delta), L.ptr(jac), 3, n, C.byref(ed))
    e = xx - hx
    with np.errstate(all="ignore"):
        sumsq = float(e @ e)
        A = jac.T @ jac
        cov = np.zeros((3, 3))
        rank = 0
        if np.all(np.isfinite(A)) and np.isfinite(sumsq) and np.all(np.isfinite(pp)):
            rank = int(_COV(L.ptr(A), L.ptr(cov), C.c_double(sumsq), 3, n))
        if not np.all(np.isfinite(cov)) or np.any(np.diag(cov) < 0):
            rank = 0
        if rank and not np.all(np.isfinite(cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov))))):
            rank = 0
        cond = float(np.linalg.cond(A)) if np.all(np.isfinite(A)) else np.inf
        xavg = xx.sum() / n
        sstot = float(((xx - xavg) ** 2).sum())
        if L.ref is not None:
            r2 = float(L.ref.dlevmar_R2(_CB, L.ptr(pp), L.ptr(xx), 3, n, C.byref(ed)))
        else:
            r2 = float(1.0 - np.float64(sumsq) / np.float64(sstot))
    fmax = float(np.max(np.abs(hx))) if np.all(np.isfinite(hx)) else np.inf
    return dict(sumsq=sumsq, sstot=sstot, R2=r2, J=jac, A=A, C=cov if rank else np.zeros((3, 3)), rank=rank, cond=cond, fmax=fmax,
                d=d, fnorm=float(np.linalg.norm(hx)), n=n)


def sumsq_bound(ref) -> float:
    """relative first-order bound on sumsq = sum e_i^2: each f_i moves by <= K eps |f_i|, so |delta sumsq| <= 2 ||e|| K eps ||f||;
    the reordered sum adds n eps sumsq"""
    if not ref["sumsq"] > 0:
        return np.inf
    return 2.0 * K_ULP * EPS * np.sqrt(ref["sumsq"]) * ref["fnorm"] / ref["sumsq"] + ref["n"] * EPS


def covar_bound(kind: int, ref) -> float:
    """The relative bound ||C_dev - C_ref||_2 / ||C_ref||_2 a device covariance is held to, from the reference's own quantities.

    Budget: a device model value differs from the host's by at most K = 4 ulp.
      * finite-difference row: J_ij = (f(p + d_j e_j) - f(p)) / d_j is a difference of two such values, so
        |delta J_ij| <= 2 K eps max|f| / d_j (forward); a central row divides by 2 d_j: half of it.
      * analytic row: the project's own device-vs-oracle tolerance, 1e-13 max(1, max|J|) per entry.
      * A = J^T J:  ||delta A|| <= 2 ||J||_F ||delta J||_F  +  n eps ||A||   (the second term: the device sums in another order)
      * C = sumsq/(n-3) A^-1:  ||delta C|| / ||C|| <= cond(A) ||delta A|| / ||A||  +  |delta sumsq| / sumsq
    and the whole is multiplied by 8 for the second-order terms."""
    n, J, A = ref["n"], ref["J"], ref["A"]
    if kind == ANALYTIC:
        dj_f = np.sqrt(3.0 * n) * AN_TOL * max(1.0, float(np.max(np.abs(J))))
    else:
        per_col = 2.0 * K_ULP * EPS * ref["fmax"] / ref["d"] * (0.5 if kind == CENTRAL else 1.0)
        dj_f = np.sqrt(n * float(np.sum(per_col ** 2)))
    a2 = float(np.linalg.norm(A, 2))
    d_a = 2.0 * float(np.linalg.norm(J)) * dj_f + n * EPS * a2
    return MARGIN * (ref["cond"] * d_a / a2 + sumsq_bound(ref))


def compare(kind: int, model: int, angles, x, p, covar, stats, rank, delta: float = 1e-6, max_left_out: float = 0.35, label: str = ""):
    """Device outputs of S fits against the yardstick at the same p.  sumsq, R2 and rank on every fit; C, sigma, rho on the fits
    whose reference rank is 3 with cond <= 1e8 (at least 65 % of them).  Returns (worst observed error / bound over C, compared, S)."""
    S = x.shape[0]
    worst, compared = 0.0, 0
    for s in range(S):
        ref = reference_stats(kind, model, angles[s], x[s], p[s], delta)
        who = (label, model, s)
        # sumsq: the project's E_TOL
        if np.isfinite(ref["sumsq"]):
            assert abs(stats[s, 0] - ref["sumsq"]) <= E_TOL * ref["sumsq"], (who, stats[s, 0], ref["sumsq"])
        else:
            assert not np.isfinite(stats[s, 0]) and rank[s] == 0, who
        # R2 = 1 - SSerr / SStot through the bound on SSerr (SStot: a reordered sum of exact terms, n eps)
        if np.isfinite(ref["R2"]):
            ratio = ref["sumsq"] / ref["sstot"]
            tol = MARGIN * (sumsq_bound(ref) + ref["n"] * EPS) * ratio + 4 * EPS * max(1.0, abs(ref["R2"]))
            assert abs(stats[s, 1] - ref["R2"]) <= tol, (who, stats[s, 1], ref["R2"], tol)
        else:
            assert not np.isfinite(stats[s, 1]), who
        if rank[s] != ref["rank"]:
            assert ref["cond"] > COND_RANK, (who, int(rank[s]), ref["rank"], ref["cond"])
        if rank[s] == 0:
            assert np.all(covar[s] == 0.0) and np.all(stats[s, 2:] == 0.0), who
        if ref["rank"] != 3 or not ref["cond"] <= COND_CUT:
            continue
        compared += 1
        assert rank[s] == 3, who
        bound = covar_bound(kind, ref)
        c2 = float(np.linalg.norm(ref["C"], 2))
        err = float(np.linalg.norm(covar[s] - ref["C"], 2)) / c2
        worst = max(worst, err / bound)
        assert err <= bound, (who, err, bound, ref["cond"])
        # sigma and rho through C: sigma_i^2 is C_ii, rho_ij sigma_i sigma_j is C_ij, held to the same ||delta C||
        sd = stats[s, 2:5]
        assert np.all(np.abs(sd * sd - np.diag(ref["C"])) <= bound * c2 * (1 + 1e-12) + 4 * EPS * np.diag(ref["C"])), (who, sd, np.diag(ref["C"]))
        for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            assert abs(stats[s, 5 + k] * sd[i] * sd[j] - ref["C"][i, j]) <= bound * c2 * (1 + 1e-12) + 8 * EPS * sd[i] * sd[j], (who, i, j)
    assert compared >= (1.0 - max_left_out) * S, (label, model, compared, S)
    print(f"fit stats {label} model {model} kind {kind}: {compared}/{S} fits compared on C, worst error / bound = {worst:.3e}")
    return worst, compared, S


@functools.lru_cache(maxsize=None)
def oracle_case(model: int, n: int, first: int, count: int, quantised: bool = False, method: int = 1, single: bool = False):
    """inputs of a case and the ORACLE's fitted p for them: (angles [S,3,n], x [S,n], p [S,3], info [S,10], ret [S])"""
    if single:
        a, x, _ = synth.make_single(model, n)
        angles, x = a[None], x[None]
    else:
        angles, x, _ = synth.make_surfels(model, n, first=first, count=count)
    if quantised:
        x = np.round(np.clip(x, 0.0, 1.0) * 255.0) / 255.0  # the capture's 8-bit measurements
    S = x.shape[0]
    lb, ub = (synth.LB, synth.UB) if (model != 2) else synth.bounds(2)
    p = np.ascontiguousarray(np.tile(np.array(synth.P0[model]), (S, 1)))
    info = np.zeros((S, 10))
    ret = np.zeros(S, dtype=np.int32)
    angles, x = np.ascontiguousarray(angles), np.ascontiguousarray(x)
    L.orc.orc_brdf_fit_batch(method, model, L.ptr(angles), L.ptr(x), C.c_long(S), n, L.ptr(p), synth.ITMAX, L.ptr(L.f64(synth.OPTS)),
                             L.ptr(L.f64(lb)), L.ptr(L.f64(ub)), L.ptr(info), ret.ctypes.data_as(C.POINTER(C.c_int)))
    return angles, x, p, info, ret
