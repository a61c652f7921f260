"""The host-callback path's cases without a GPU (tests/callback_problems.py): with the compiled reference alone, every tree case
meets the yardstick's conditions (the table is printed: pytest -s); the reference-order cases reach the branch they are named for;
the float twins of the wide problem say what the double ones say."""
import ctypes as C

import numpy as np
import pytest

from tests import callback_problems as K
from tests import oracle_libs as L

pytestmark = pytest.mark.skipif(L.ref is None, reason="the wide problem's callbacks and the yardstick live in oracle/_ref")


def _fmt(worst):
    return "  ".join(f"{worst[f]:.1e}" for f in K.FIELDS)


def test_tree_cases_meet_the_yardsticks_conditions():
    """every shape's table row; at most 10 % of all tree cases uncompared, no (entry, shape) cell with none compared, the caps"""
    cells, total = {}, {f: 0.0 for f in K.FIELDS}
    for m, n in K.SHAPES_B:
        worst, count = {f: 0.0 for f in K.FIELDS}, [0, 0]
        for c in K.tree_cases(m, n):
            y = K.yardstick(c)
            assert y.ret >= 0 and y.info[8] >= 1 and y.info[5] <= c.itmax, K.describe(c)
            cells.setdefault((c.entry, c.m, c.n), [0, 0])[0 if y.comparable else 1] += 1
            count[0 if y.comparable else 1] += 1
            if y.comparable:
                for f in K.FIELDS:
                    worst[f] = max(worst[f], y.tol[f])
                    total[f] = max(total[f], y.tol[f])
            else:
                print("    uncompared:", K.describe(c), "counts agree" if y.stable else "counts differ", {f: f"{v:.1e}" for f, v in y.tol.items()})
        print(f"    ({m}, {n})".ljust(17) + f"{count[0]:5d}  {count[1]:9d}       {_fmt(worst)}")
        assert count[0] + count[1] == 20
        # the cases do cut the fit short, and the box is active in them
        assert any(K.yardstick(c).info[6] == 3 for c in K.tree_cases(m, n))
        if m > 1:
            assert any(np.any(np.abs(K.yardstick(c).p) == 0.75) for c in K.tree_cases(m, n) if c.entry.startswith("bc"))
    comp, unc = sum(v[0] for v in cells.values()), sum(v[1] for v in cells.values())
    assert comp + unc == 80 and unc <= K.MAX_UNCOMPARED * (comp + unc), (comp, unc)
    assert all(v[0] > 0 for v in cells.values()), cells
    assert set(cells) == {(e, m, n) for e in K.ENTRIES for m, n in K.SHAPES_B}
    assert all(total[f] <= K.CAP_P for f in ("p", "info0", "info1")) and all(total[f] <= K.CAP_INFO for f in ("info2", "info3", "info4"))
    assert total["covar"] <= K.CAP_COVAR


def test_converged_tree_fits_meet_their_conditions():
    for c in K.converged_cases():
        y = K.yardstick(c)
        print(f"    {K.describe(c)}: stable {y.stable}, iterations {int(y.info[5])}, reason {int(y.info[6])}, tolerance p {y.tol['p']:.1e} "
              f"info[1] {y.tol['info1']:.1e} info[2..4] {max(y.tol[f] for f in ('info2', 'info3', 'info4')):.1e} covar {y.tol['covar']:.1e}")
        assert y.ret >= 0 and y.info[6] != 3, K.describe(c)  # (converged: not stopped by itmax)
        assert y.tol["p"] <= K.CAP_CONVERGED_P and y.tol["info1"] <= K.CAP_P, (K.describe(c), y.tol)
        if c.entry == "der":  # (its info[2..4] are those of a gradient that cancels at the minimum: own tolerance, no cap)
            assert y.stable and y.tol["info0"] <= K.CAP_P and y.tol["covar"] <= K.CAP_COVAR, y.tol
        assert np.sum(np.abs(y.p) == 0.75) >= (1 if c.entry.startswith("bc") else 0)


def test_float_tree_yardstick():
    """info[0] of the float reference itself lies within its own tolerance of the float64 sum, and that tolerance would still
    see a dropped sample"""
    worst = 0.0
    for c in K.float_tree_cases():
        want, tol = K.float_tree_info0(c)
        got = K.run(L.ref, c)
        worst = max(worst, tol)
        assert got[0] >= 0 and abs(got[2][0] - want) <= tol * want, (K.describe(c), got[2][0], want, tol)
        x, p0 = K.problem(c.m, c.n, "s")[:2]
        e2 = (x.astype(np.float64) - K.values("s", p0, c.n).astype(np.float64)) ** 2
        assert np.median(e2) / want > 0.5 / c.n  # (a typical sample's share of the sum ...)
        assert tol < 1e-4  # (... is 4.6e-5 at n = 21846; one at the far end of the interval carries several times that)
    print(f"    float tree info[0]: largest tolerance {worst:.1e}")


def test_reference_order_cases_reach_their_branches():
    """the table of part A: which loop of the kernel each shape reaches, by the arithmetic of generic_fit.hip"""
    small_dif = {(m, n) for m, n in K.SHAPES_A if n * m <= 1024}
    small_rest = {(m, n) for m, n in K.SHAPES_A if n * m < 1024}
    assert small_dif == {(3, 341), (4, 256)} and small_rest == {(3, 341)}
    blocked = [s for s in K.SHAPES_A if s not in small_rest]
    assert {n % 32 for _, n in blocked} >= {0, 1, 13, 21, 28} and {n % 8 for _, n in K.SHAPES_A} >= {0, 1, 4, 5}
    assert max(m * n for m, n in K.SHAPES_A) == K.EXACT_LIMIT and min(m * n for m, n in K.SHAPES_B) == K.EXACT_LIMIT + 1
    assert {m for m, _ in K.SHAPES_A} >= {1, 2, 3, 4, 5, 16} and {m for m, _ in K.SHAPES_B} == {1, 3, 5, 16}
    cases = K.exact_cases()
    assert len(set(cases)) == len(cases)
    for real, shapes in (("d", K.SHAPES_A), ("s", K.SHAPES_A_FLOAT)):
        for m, n in shapes:
            assert {c.entry for c in cases if (c.m, c.n, c.real) == (m, n, real) and c.opts is not None and c.opts[4] > 0} == set(K.ENTRIES)
    assert {c.entry for c in cases if c.dscl} == {"bc_dif", "bc_der"} and any(c.dscl and c.opts[4] < 0 for c in cases)
    assert any(c.opts is None for c in cases) and any(c.itmax == 0 for c in cases)


def test_reference_order_cases_do_what_they_are_meant_to():
    """with the reference alone: fits of n m <= 4098 converge before their cap, the upper-edge ones are cut by it (der also
    converges), the box and dscl are active, central differences change the path"""
    by = {c: K.run(L.ref, c) for c in K.exact_cases() if c.m * c.n <= 4098 or c.real == "d"}
    for c, r in by.items():
        assert r[0] >= 0 or c.itmax == 0, K.describe(c)
        if c.itmax == K.ITMAX_FULL and not c.dscl:  # (with dscl = 50 on a component the box search crawls: those may reach the cap)
            assert r[2][6] != 3 and r[2][5] < c.itmax, (K.describe(c), r[2])
        elif c.itmax == K.ITMAX_EDGE:
            assert r[2][6] == 3 and r[2][5] == c.itmax, (K.describe(c), r[2])
    on_bound = [(m, n) for m, n in K.SHAPES_A if np.any(np.abs(by[K.case("bc_dif", m, n, K._itmax_a(m, n))][1]) == 0.75)]
    print("    a component on a bound at", on_bound)
    assert len(on_bound) >= 4 and {(5, 205), (16, 4096)} <= set(on_bound)
    for m, n in K.SHAPES_A:
        fwd, cen = by[K.case("dif", m, n, K._itmax_a(m, n))], by[K.case("dif", m, n, K._itmax_a(m, n), cent=True)]
        assert not np.array_equal(fwd[2], cen[2])
    plain, scaled = by[K.case("bc_dif", 5, 205, K.ITMAX_FULL)], by[K.case("bc_dif", 5, 205, K.ITMAX_FULL, dscl=True)]
    assert not np.array_equal(plain[2], scaled[2])


def test_float_twins_say_what_the_double_callbacks_say():
    for m, n in ((1, 7), (5, 205), (16, 64)):
        p = np.random.default_rng(m).uniform(-1.0, 1.0, m)
        assert np.max(np.abs(K.values("s", p, n) - K.values("d", p, n))) <= 64 * m * 2.0 ** -24
        jd, js = np.zeros(n * m), np.zeros(n * m, dtype=np.float32)
        L.ref.wide_cheb_jac(L.ptr(p.copy()), L.ptr(jd), m, n, None)
        ps = p.astype(np.float32)
        K.symbols("s")[1](K._ptr("s", ps), K._ptr("s", js), m, n, None)
        assert np.max(np.abs(js - jd)) <= 64 * m * 2.0 ** -24


def test_utilities_reference_side():
    """dlevmar_R2 of the reference equals its three loops restated in numpy order-free within 1e-12; with x == NULL it reads x
    before it tests it (misc_core.c:634-638), so the value of its x == 0 branch is taken from a run on a vector of zeros, which
    performs the same operations on the same values; the reference's chkjac flags nearly every row of a Jacobian whose column 1 is 1 % off"""
    for n in (65536, 65537):
        x, p0 = K.problem(3, n)[:2]
        hx = K.values("d", p0, n)
        want = 1.0 - np.sum((x - hx) ** 2) / np.sum((x - x.mean()) ** 2)
        assert abs(K.r2(L.ref, n) - want) <= 1e-12 * abs(want)
    assert K.r2(L.ref, 100, zero_x=True) == -np.inf
    good = K.chkjac(L.ref, 5, 1000)
    assert good.min() > 0.5
    jf = K.scaled_column_jac()
    bad = K.chkjac(L.ref, 5, 1000, C.cast(jf, C.c_void_p))
    assert np.count_nonzero(bad < 0.5) > 900  # (987: column 1 is T_1(t) = t, so the rows next to t = 0 cannot tell)
