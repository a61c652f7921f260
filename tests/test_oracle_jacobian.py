"""The analytic Jacobian against 50-digit derivatives (tests/jacobian_yardstick.py), and the fits that depend on its dead-lobe
rows against an optimum that does not.

orc_brdf_jac (oracle/brdf_models_oracle.c) and BrdfModel<M>::an_row (brdf_amd/csrc/brdf_models.h) are this project's own
formulas; every other test of dlevmar_bc_der / dlevmar_der compares the device with the oracle or with the reference's solver
driven by that same orc_brdf_jac.  Here each entry of the row is held to the derivative itself, on the edge grid of the model
values and on ordinary samples; and fits whose data hold dead-lobe samples (pow(0, n); Ward at cos(N.H) = 0, subnormal and
1e-200), where column 2 used to be 0 * inf = NaN and one sample stopped the fit at p0 with reason 5, are held to the reference's
own dlevmar_bc_dif / dlevmar_dif optimum on the same data (tests/golden/brdf_dead_lobe_fits.json).

Measured (oracle, worst error of a judged entry in u cond sum|terms|, bound 16): see DESIGN.md section 5."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests import jacobian_yardstick as J
from tests import oracle_libs as L

HERE = os.path.dirname(os.path.abspath(__file__))
DEAD = json.load(open(os.path.join(HERE, "golden", "brdf_dead_lobe_fits.json")))["fits"]
P_TOL = 1e-5
E_TOL = 1e-8
METHOD = ("dif", "bc_dif", "bc_der", "der")


class _Extra(C.Structure):
    _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]


def oracle_rows(model, angles, p):
    a = L.f64(angles)
    n = a.size // 3
    jac = np.full(3 * n, np.nan)
    L.orc.orc_brdf_jac(L.ptr(L.f64(p).copy()), L.ptr(jac), 3, n, C.byref(_Extra(L.ptr(a), model)))
    return jac.reshape(n, 3)


def _hex(v):
    return np.array([float.fromhex(s) for s in v])


@pytest.mark.parametrize("model", [0, 1, 2])
def test_oracle_rows_against_50_digit_derivatives(model):
    """every judged entry of orc_brdf_jac inside (2 K_ULP + 8) u cond sum|terms| + the subnormal floor; dead-lobe entries exactly 0;
    entries not judged NaN / infinite exactly where the IEEE expression is"""
    worst, tally = 0.0, {}
    for angles, p in J.grid(model):
        worst = max(worst, J.check_rows(oracle_rows(model, angles, p), model, angles, p, ("orc_brdf_jac", model, p), tally))
    print(f"model {model}: worst judged entry {worst:.2f} u cond sum|terms| (bound {J.REL / J.U:.0f}); entries {tally}")
    assert tally[J.JUDGED] > 1000 and tally[J.DEAD] >= 14 and (model == 2 or tally[J.NOT_JUDGED] > 0)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_dead_lobe_rows_are_zero_and_finite(model):
    """rows whose lobe factor is exactly 0: columns 1 and 2 are 0 (either sign), column 0 untouched -- at several parameter
    points, Ward's also at the subnormal and the 1e-200 cosine, whose tan^2 overflows"""
    angles, p = J.dead_rows(model)
    points = [p] + ([(0.0, 1.0, 1.0), (0.35, 0.6, 1000.0)] if model in (0, 1) else [(0.0, 1.0, 0.01), (0.35, 0.25, 10.0)])
    planes = [angles]
    if model == 2:
        for c in E.WARD_DEAD_COSINES[1:]:
            a = angles.copy()
            a[1] = c
            planes.append(a)
    for a in planes:
        for q in points:
            rows = oracle_rows(model, a, q)
            assert np.all(np.isfinite(rows)), (model, q, rows)
            assert np.all(rows[:, 1:] == 0.0), (model, q, rows)
            assert np.array_equal(rows[:, 0], a[0] if model != 2 else a[0] / synth.PI)


def test_fixture_covers_every_dead_lobe_case():
    assert [tuple(f[:4]) for f in DEAD] == [(m, meth, n, i) for m, n, i in E.dead_lobe_cases() for meth in (1, 0)]
    for model, n, idx in E.dead_lobe_cases():
        angles = E.make_dead_lobe(model, n, idx)[0]
        k = E.power_plane(model) if model in (0, 1) else 1
        assert np.all(angles >= 0.0) and np.count_nonzero(angles[k] < 1e-150) >= 4
        if model == 2:
            assert set(angles[1][angles[1] < 1e-150]) == set(E.WARD_DEAD_COSINES)
    for f in DEAD:  # the reference's finite-difference fits succeed (one 16-sample Ward fit at itmax): there is an objective to hold
        assert f[4] >= 0 and _hex(f[6])[6] in (1, 2, 3, 6), f  # the analytic ones to


@pytest.mark.skipif(L.ref is None, reason="the reference's levmar lives in oracle/_ref")
def test_dead_lobe_fixture_is_the_live_reference():
    for model, method, n, idx, ret, p, info in DEAD:
        r, rp, ri = L.brdf_fit("ref", method, model, *E.dead_lobe_args(model, n, idx))
        assert r == ret and np.array_equal(rp, _hex(p)) and np.array_equal(ri, _hex(info)), (model, method, n, idx)


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("method", [2, 3])
def test_dead_lobe_fits_reach_the_finite_difference_optimum(method, model):
    """dlevmar_bc_der / dlevmar_der through the oracle and the host-driven product machines on data with dead-lobe samples:
    both succeed, ||e||^2 within E_TOL of the reference's dlevmar_bc_dif / dlevmar_dif optimum, p within P_TOL for n >= 64
    (16 samples determine p only to ~1e-4), and the product's machine equals the oracle bit for bit"""
    worst_e = worst_p = 0.0
    for m, n, idx in E.dead_lobe_cases():
        if m != model:
            continue
        args = E.dead_lobe_args(model, n, idx)
        rr, rp, ri = J.dead_lobe_reference(model, method, n, idx)
        got = L.brdf_fit("orc", method, model, *args)
        hm = L.brdf_fit("hm", method, model, *args)
        what = (METHOD[method], model, n, idx, got, (rr, rp, ri))
        assert got[0] >= 0 and got[2][6] != 5 and rr >= 0, what
        assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2])), what
        assert abs(got[2][1] - ri[1]) <= E_TOL * ri[1], what
        worst_e = max(worst_e, abs(got[2][1] - ri[1]) / ri[1])
        if n >= 64:
            gp, qp = np.array(got[1]), np.array(rp)
            if method == 3 and model == 2:  # unconstrained Ward depends on alpha^2
                gp[2], qp[2] = abs(gp[2]), abs(qp[2])
            assert L.rel_err(gp, qp) <= P_TOL, what
            worst_p = max(worst_p, L.rel_err(gp, qp))
        assert hm[0] == got[0] and np.array_equal(hm[1], got[1]) and np.array_equal(hm[2], got[2]), (what, hm)
    print(f"{METHOD[method]} model {model}: worst objective difference {worst_e:.2e}, worst p difference at n >= 64 {worst_p:.2e}")
