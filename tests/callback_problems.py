"""The host-callback path (brdf_amd/csrc/generic_fit.hip) in every branch of its sums and at the seams between them: the
cases, the yardstick and the comparison that tests/test_oracle_callbacks.py (CPU) and tests/test_gpu_callbacks.py (GPU) share.
CPU only.

The problem is wide_cheb / wide_cheb_jac of oracle/ref_shim.c (ours), called by address from oracle/_ref: any m, any n; for float
sp_wide_cheb / sp_wide_cheb_jac of oracle/sp_wide_cheb.c, by address from oracle/liboracle.so (symbols()).  Truth
default_rng(m).uniform(-1, 1, m), noise 1e-3 (rng.random(n) - 0.5), start [0.1] * m, box +-0.75 (several components end on a
bound).  The yardstick throughout is the compiled reference's own dlevmar_* / slevmar_* on the
same callback, through run(): all four entries, covar always requested, dscl optional, opts per case (None allowed), both precisions.

A.  n m <= 65536: one lane forms the sums in the reference's order (the "small problem" loop below the n m = 1024 switch, the
32-row blocked loop above it), so ret, p, info[0..9] and covar must be the reference's bit for bit.  At itmax = 0 the reference
returns info[2], info[4] and covar from memory it never wrote (info[3] from an initial value); ret, p, info[0], info[1] and
info[5..9] are compared there.

B.  n m > 65536: a 256-lane strided tree.  Fits are cut short by itmax = 1, 2, 3 and held to the rule of tests/pass_problems.py,
taken from the reference alone: the reference as it is and on four seeded permutations of the samples (a Python wrapper around the
C callback returns rows [perm]; x[perm]); tolerance = 8 x the spread of the four, per field, floor 64 * 2^-53; p by its largest
component (|p_ref| floored at 1e-6), info[0..4] relative, covar by relative Frobenius norm; ret and info[5..9] exactly.  A case is
compared only if the five runs agree on ret and info[5..9] and its tolerance is <= 1e-8 on p, info[0], info[1] and <= 1e-6 on
info[2..4] (conditions, not measurements: a row dropped from a sum at n = 21846 is 5e-5, a wrong difference step is percent-sized).
At most 10 % of the cases may go uncompared and no (entry, shape) cell may have none compared.  Every compared case's covar
tolerance is required to be <= 1e-6 as well.

Measured with the reference alone (tests/test_oracle_callbacks.py prints the table): the largest tolerance (8 x spread) per shape
over its 20 cases (four entries forward, dif and bc_dif central, itmax 1, 2, 3; bc_dif and bc_der with dscl at itmax = 2)

    (m, n)       compared  uncompared  p        info[0]  info[1]  info[2]  info[3]  info[4]  covar
    (3, 21846)      20          0       2.9e-13  2.1e-14  4.1e-11  1.8e-10  3.7e-10  4.0e-13  4.1e-11
    (5, 13108)      20          0       1.2e-11  1.5e-14  3.8e-11  4.8e-10  3.8e-10  1.5e-11  3.8e-11
    (16, 4097)      20          0       5.2e-11  1.2e-14  1.2e-11  2.1e-10  6.1e-11  1.1e-11  2.7e-11
    (1, 65537)      17          3       3.8e-13  4.9e-14  1.5e-11  7.1e-08  1.4e-07  6.9e-13  1.5e-11

The three uncompared cases (3.75 % of 80) are bc_dif forward, bc_dif central and bc_der at (1, 65537), itmax = 3: a fit in one unknown
is at its minimum by then, and the permuted runs differ in their evaluation counts.

Fits run to convergence at (5, 13108), forward differences: under permutation the reference's iteration counts are not stable for
dif, bc_dif and bc_der and info[2..4] move by orders of magnitude, so only ret >= 0, p within max(8 x spread, floor) -- required to
be <= 1e-6 -- and info[1] within its tolerance are compared; der is stable and takes the full comparison.

    entry    counts agree  iterations  tolerance p  info[1]  info[2..4]  covar
    dif      no            18          2.5e-09      5.5e-14  8.8e+01     1.1e-11
    der      yes            6          7.1e-15      1.3e-14  9.5e-03     1.5e-14
    bc_dif   no            141         7.9e-08      8.1e-15  2.2e+02     1.7e-10
    bc_der   no            145         7.0e-08      7.1e-15  1.6e+04     1.5e-10

(der's info[2..4] are those of a gradient that cancels at the minimum: they are compared within their own tolerance, without a cap.)

Float in the tree: under permutation the reference's own slevmar_* moves by 1e-4 to 2e-2 per field at these sizes, looser than a
dropped row, so p, info[1..4] and covar of the float tree branch are NOT judged.  info[0] of an itmax = 1 run of each entry at
(3, 21846) is: against ||x - f(p0)||^2 summed in float64 by numpy over the float callback's values, within 8 x the float
reference's own spread on that field under the four permutations (3.5e-6 to 5.5e-6 for the four entries; no floor).
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import zlib

import numpy as np

from tests import oracle_libs as L

U = 2.0 ** -53
FLOOR = 64 * U
MARGIN = 8.0
CAP_P, CAP_INFO, CAP_COVAR, CAP_CONVERGED_P = 1e-8, 1e-6, 1e-6, 1e-6
MAX_UNCOMPARED = 0.10
OPTS = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)  # lmdemo.c:816-817
SOPTS = (1e-3, 1e-7, 1e-7, 1e-12, 1e-4)
ENTRIES = ("dif", "der", "bc_dif", "bc_der")
FIELDS = ("p", "info0", "info1", "info2", "info3", "info4", "covar")
EXACT_LIMIT = 65536  # kGenExactLimit of generic_fit.hip

Case = collections.namedtuple("Case", "entry m n itmax opts dscl real")
Yard = collections.namedtuple("Yard", "ret p info covar stable spread tol comparable")

_REAL = {"d": (np.float64, C.c_double, "d", ""), "s": (np.float32, C.c_float, "s", "sp_")}


def central(opts):
    return opts[:4] + (-opts[4],)


def case(entry, m, n, itmax, cent=False, dscl=False, real="d", opts="default"):
    if opts == "default":
        opts = OPTS if real == "d" else SOPTS
        if cent:
            opts = central(opts)
    return Case(entry, m, n, itmax, opts, dscl, real)


def describe(c):
    o = "NULL" if c.opts is None else ("central" if c.opts[4] < 0 else "forward")
    return f"{c.real}levmar_{c.entry} m={c.m} n={c.n} itmax={c.itmax} {o}" + (" dscl" if c.dscl else "")


def case_id(c):
    return describe(c).replace(" ", "-").replace("=", "")


def _arr(real, v):
    return None if v is None else np.ascontiguousarray(np.asarray(v, dtype=_REAL[real][0]).reshape(-1))


def _ptr(real, a):
    return None if a is None else a.ctypes.data_as(C.POINTER(_REAL[real][1]))


def symbols(real):
    """(wide_cheb, wide_cheb_jac) for `real`: the double ones from oracle/_ref; the float twins from oracle/liboracle.so, which
    every machine builds from the tree (a machine without the reference keeps the oracle/_ref it was given, twins or not)"""
    src, pre = (L.ref, "") if real == "d" else (L.orc, "sp_")
    return getattr(src, pre + "wide_cheb"), getattr(src, pre + "wide_cheb_jac")


def callbacks(real):
    """(func, jacf) of the wide problem, as addresses"""
    f, j = symbols(real)
    return C.cast(f, C.c_void_p), C.cast(j, C.c_void_p)


def values(real, p, n):
    """the callback's values at p: f(p)[n]"""
    p = _arr(real, p).copy()
    hx = np.zeros(n, dtype=_REAL[real][0])
    symbols(real)[0](_ptr(real, p), _ptr(real, hx), p.size, n, None)
    return hx


@functools.lru_cache(maxsize=None)
def problem(m, n, real="d"):
    """-> x[n], p0[m], lb[m], ub[m], dscl[m] (read-only)"""
    rng = np.random.default_rng(m)
    truth = rng.uniform(-1.0, 1.0, m)
    x = values(real, truth, n)
    x = x + (1e-3 * (rng.random(n) - 0.5)).astype(x.dtype)
    out = (x, _arr(real, [0.1] * m), _arr(real, [-0.75] * m), _arr(real, [0.75] * m), _arr(real, [(1.0, 2.0, 50.0)[i % 3] for i in range(m)]))
    for a in out:
        a.setflags(write=False)
    return out


def run(lib, c, func=None, jacf=None, x=None):
    """one case through `lib` (the compiled reference or the product: the same entry names) -> ret, p[m], info[10], covar[m, m].
    func / jacf: other callbacks than oracle/_ref's (addresses); x: other measurements than the problem's."""
    real = c.real
    x0, p0, lb, ub, dscl = problem(c.m, c.n, real)
    f, j = callbacks(real)
    f, j = func or f, jacf or j
    p, xx = p0.copy(), _arr(real, x0 if x is None else x)
    info, covar = np.zeros(10, dtype=p.dtype), np.zeros(c.m * c.m, dtype=p.dtype)
    opts = _arr(real, c.opts)
    ds = dscl if c.dscl else None
    P = functools.partial(_ptr, real)
    fn = getattr(lib, f"{_REAL[real][2]}levmar_{c.entry}")
    if c.entry == "dif":
        r = fn(f, P(p), P(xx), c.m, c.n, c.itmax, P(opts), P(info), None, P(covar), None)
    elif c.entry == "der":
        r = fn(f, j, P(p), P(xx), c.m, c.n, c.itmax, P(opts), P(info), None, P(covar), None)
    elif c.entry == "bc_dif":
        r = fn(f, P(p), P(xx), c.m, c.n, P(lb), P(ub), P(ds), c.itmax, P(opts), P(info), None, P(covar), None)
    elif c.entry == "bc_der":
        r = fn(f, j, P(p), P(xx), c.m, c.n, P(lb), P(ub), P(ds), c.itmax, P(opts), P(info), None, P(covar), None)
    else:
        raise ValueError(c.entry)
    return int(r), p, info, covar.reshape(c.m, c.m)


def run_permuted(c, k):
    """the reference on the samples in another order: rows [perm] of the callbacks' results, x[perm]"""
    real = c.real
    T = C.POINTER(_REAL[real][1])
    perm = np.random.default_rng([zlib.crc32(repr(c).encode()), k]).permutation(c.n)
    f0, j0 = symbols(real)
    tmp, tmpj = np.zeros(c.n, dtype=_REAL[real][0]), np.zeros((c.n, c.m), dtype=_REAL[real][0])

    @C.CFUNCTYPE(None, T, T, C.c_int, C.c_int, C.c_void_p)
    def func(p, hx, m, n, adata):
        f0(p, _ptr(real, tmp), m, n, None)
        np.ctypeslib.as_array(hx, (n,))[:] = tmp[perm]

    @C.CFUNCTYPE(None, T, T, C.c_int, C.c_int, C.c_void_p)
    def jacf(p, jac, m, n, adata):
        j0(p, _ptr(real, tmpj), m, n, None)
        np.ctypeslib.as_array(jac, (n, m))[:] = tmpj[perm]

    return run(L.ref, c, C.cast(func, C.c_void_p), C.cast(jacf, C.c_void_p), problem(c.m, c.n, real)[0][perm])


# ---- the comparison ---------------------------------------------------------------------------------------------------
def _rel(a, b, floor):
    """|a - b| / max(|b|, floor), the largest element; 0 where the two are the same value (inf and NaN included)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), floor)
    d = np.where(same, 0.0, d)
    return float(np.max(np.where(np.isnan(d), np.inf, d)))


def _frob(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if np.array_equal(a, b, equal_nan=True):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.linalg.norm(a - b) / np.linalg.norm(b)
    return float(d) if np.isfinite(d) else np.inf


def differences(got, want):
    """per field of FIELDS: the relative difference of one result (ret, p, info, covar) from another"""
    out = {"p": _rel(got[1], want[1], 1e-6)}
    for i in range(5):
        out[f"info{i}"] = _rel(got[2][i], want[2][i], 1e-300)
    out["covar"] = _frob(got[3], want[3])
    return out


def same_counts(a, b):
    return a[0] == b[0] and np.array_equal(a[2][5:], b[2][5:])


@functools.lru_cache(maxsize=None)
def yardstick(c) -> Yard:
    base = run(L.ref, c)
    runs = [run_permuted(c, k) for k in range(4)]
    stable = all(same_counts(r, base) for r in runs)
    spread = {f: 0.0 for f in FIELDS}
    for r in runs:
        for f, d in differences(r, base).items():
            spread[f] = max(spread[f], d)
    tol = {f: max(MARGIN * s, FLOOR) for f, s in spread.items()}
    comparable = (stable and all(tol[f] <= CAP_P for f in ("p", "info0", "info1")) and all(tol[f] <= CAP_INFO for f in ("info2", "info3", "info4")))
    return Yard(base[0], base[1], base[2], base[3], stable, spread, tol, comparable)


def compare(c, got, fields=FIELDS, counts=True):
    """one result against the reference's within the case's tolerance -> ({field: difference / tolerance}, None or what is wrong)"""
    y = yardstick(c)
    want = (y.ret, y.p, y.info, y.covar)
    ratios = {f: d / y.tol[f] for f, d in differences(got, want).items() if f in fields}
    wrong = []
    if counts and got[0] != y.ret:
        wrong.append(f"ret {got[0]} != {y.ret}")
    if counts and not np.array_equal(got[2][5:], y.info[5:]):
        wrong.append(f"info[5..9] {got[2][5:].tolist()} != {y.info[5:].tolist()}")
    wrong += [f"{f}: {r:.3g} x its tolerance {y.tol[f]:.3g}" for f, r in ratios.items() if not r <= 1.0]
    if wrong:
        return ratios, (f"{describe(c)}: " + "; ".join(wrong) + f" (got p {got[1].tolist()} info {got[2].tolist()}, reference p {y.p.tolist()} "
                        f"info {y.info.tolist()})")
    return ratios, None


def identical(c, got, want):
    """part A: None, or what differs between two results that must be equal bit for bit"""
    wrong = []
    if got[0] != want[0]:
        wrong.append(f"ret {got[0]} != {want[0]}")
    keep = list(range(10)) if c.itmax > 0 else [0, 1, 5, 6, 7, 8, 9]
    if not np.array_equal(got[1], want[1], equal_nan=True):
        wrong.append(f"p {got[1].tolist()} != {want[1].tolist()}")
    if not np.array_equal(got[2][keep], want[2][keep], equal_nan=True):
        wrong.append(f"info {got[2].tolist()} != {want[2].tolist()}")
    if c.itmax > 0 and not np.array_equal(got[3], want[3], equal_nan=True):
        wrong.append(f"covar differs by {_frob(got[3], want[3]):.3g} (relative Frobenius)")
    return None if not wrong else f"{describe(c)}: " + "; ".join(wrong)


class Tally:
    """what a tree test prints and asserts about its cases: compared / uncompared per (entry, shape) cell, the worst ratio per field
    (which cases are compared is decided by the reference alone: the 10 % condition over all shapes is test_oracle_callbacks.py's)"""

    def __init__(self, name):
        self.name, self.cells, self.worst, self.bad = name, collections.defaultdict(lambda: [0, 0]), {f: 0.0 for f in FIELDS}, []

    def add(self, c, got):
        cell = (c.entry, c.m, c.n)
        if not yardstick(c).comparable:
            self.cells[cell][1] += 1
            return
        self.cells[cell][0] += 1
        ratios, wrong = compare(c, got)
        for f, r in ratios.items():
            self.worst[f] = max(self.worst[f], r)
        if wrong is not None:
            self.bad.append(wrong)

    def check(self):
        comp, unc = sum(v[0] for v in self.cells.values()), sum(v[1] for v in self.cells.values())
        print(f"{self.name}: {comp} compared, {unc} uncompared, {len(self.bad)} wrong; worst difference / tolerance: "
              + ", ".join(f"{f} {r:.2g}" for f, r in self.worst.items()))
        assert not self.bad, "\n".join(self.bad[:20])
        empty = [k for k, v in self.cells.items() if v[0] == 0]
        assert not empty, (self.name, "cells with nothing compared", empty)


# ---- A: the reference-order branches ----------------------------------------------------------------------------------
SHAPES_A = ((3, 341), (4, 256), (5, 205), (2, 2049), (1, 1500), (16, 4096), (4, 16384), (3, 21845))
SHAPES_A_FLOAT = ((3, 341), (4, 256), (5, 205), (16, 4096))
ITMAX_FULL, ITMAX_EDGE = 200, 3


def _itmax_a(m, n):
    return ITMAX_FULL if n * m <= 4098 else ITMAX_EDGE


@functools.lru_cache(maxsize=None)
def exact_cases():
    out = []
    for m, n in SHAPES_A:
        out += [case(e, m, n, _itmax_a(m, n)) for e in ENTRIES]
        out += [case(e, m, n, _itmax_a(m, n), cent=True) for e in ("dif", "bc_dif")]
        if n * m > 4098:  # the analytic entry to convergence at the upper edge (6 - 7 iterations)
            out.append(case("der", m, n, ITMAX_FULL))
    # once each: dscl (forward for both bc entries; central, where the `same` comparison of generic_run decides which residual is
    # paired with J'e, on either side of the switch), opts = NULL, itmax = 0
    out += [case(e, 5, 205, ITMAX_FULL, dscl=True) for e in ("bc_dif", "bc_der")]
    out += [case("bc_dif", m, n, ITMAX_FULL, cent=True, dscl=True) for m, n in ((3, 341), (5, 205))]
    out += [case(e, 5, 205, ITMAX_FULL, opts=None) for e in ENTRIES]
    out += [case(e, 4, 256, 0) for e in ENTRIES]
    for m, n in SHAPES_A_FLOAT:
        out += [case(e, m, n, _itmax_a(m, n), real="s") for e in ENTRIES]
    out.append(case("der", 16, 4096, ITMAX_FULL, real="s"))
    out += [case(e, 4, 256, ITMAX_FULL, cent=True, real="s") for e in ("dif", "bc_dif")]
    assert all(c.m * c.n <= EXACT_LIMIT for c in out)
    return tuple(out)


# ---- B: the tree ------------------------------------------------------------------------------------------------------
SHAPES_B = ((3, 21846), (5, 13108), (16, 4097), (1, 65537))
CONVERGED_SHAPE = (5, 13108)
FLOAT_TREE_SHAPE = (3, 21846)


@functools.lru_cache(maxsize=None)
def tree_cases(m, n):
    out = []
    for itmax in (1, 2, 3):
        out += [case(e, m, n, itmax) for e in ENTRIES]
        out += [case(e, m, n, itmax, cent=True) for e in ("dif", "bc_dif")]
    out += [case(e, m, n, 2, dscl=True) for e in ("bc_dif", "bc_der")]
    assert all(c.m * c.n > EXACT_LIMIT for c in out)
    return tuple(out)


def converged_cases():
    return tuple(case(e, *CONVERGED_SHAPE, ITMAX_FULL) for e in ENTRIES)


def compare_converged(c, got):
    """None, or what is wrong with a fit run to convergence: der in full; the others ret >= 0, p and info[1]"""
    y = yardstick(c)
    if c.entry == "der":
        return compare(c, got)[1]
    if got[0] < 0:
        return f"{describe(c)}: ret {got[0]}"
    return compare(c, got, fields=("p", "info1"), counts=False)[1]


def float_tree_cases():
    return tuple(case(e, *FLOAT_TREE_SHAPE, 1, real="s") for e in ENTRIES)


@functools.lru_cache(maxsize=None)
def float_tree_info0(c):
    """-> (||x - f(p0)||^2 in float64 over the float callback's values, 8 x the float reference's spread of info[0] under permutation)"""
    x, p0 = problem(c.m, c.n, "s")[:2]
    e = x.astype(np.float64) - values("s", p0, c.n).astype(np.float64)
    base = run(L.ref, c)
    spread = max(_rel(run_permuted(c, k)[2][0], base[2][0], 1e-300) for k in range(4))
    return float(np.sum(e * e)), MARGIN * spread


# ---- C: the utilities -------------------------------------------------------------------------------------------------
def r2(lib, n, real="d", null_x=False, zero_x=False, m=3):
    """dlevmar_R2 / slevmar_R2 of `lib` on the wide problem at its truth-less start point [0.1] * m"""
    x, p0 = problem(m, n, real)[:2]
    fn = getattr(lib, f"{_REAL[real][2]}levmar_R2")
    fn.restype = _REAL[real][1]
    xx = None if null_x else (np.zeros_like(x) if zero_x else _arr(real, x))
    return fn(callbacks(real)[0], _ptr(real, p0.copy()), _ptr(real, xx), m, n, None)


def chkjac(lib, m, n, jacf=None):
    """dlevmar_chkjac of `lib` at the problem's truth -> err[n]"""
    p = np.random.default_rng(m).uniform(-1.0, 1.0, m)
    err = np.zeros(n)
    f, j = callbacks("d")
    lib.dlevmar_chkjac(f, jacf or j, L.ptr(p), m, n, None, L.ptr(err))
    return err


def scaled_column_jac(column=1, factor=1.01):
    """wide_cheb_jac with one column multiplied by `factor` (keep the returned object alive while it is in use)"""
    @C.CFUNCTYPE(None, L.D, L.D, C.c_int, C.c_int, C.c_void_p)
    def jacf(p, jac, m, n, adata):
        L.ref.wide_cheb_jac(p, jac, m, n, None)
        np.ctypeslib.as_array(jac, (n, m))[:, column] *= factor
    return jacf
