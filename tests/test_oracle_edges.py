"""Edge-of-domain fits (tests/edge_problems.py): the oracle and the host-driven product machines against the REFERENCE's
own results, bit for bit -- live through oracle/_ref where it was built, and through the committed fixture
tests/golden/brdf_edge_fits.json everywhere.  Active bounds, starts on the box, black / saturated / quantised pixels,
grazing and non-positive cosines take the projected step, the line search and the projected-gradient search of
dlevmar_bc_dif with constraints active; the GPU tests compare the device against the oracle on the same problems."""
import json
import os

import numpy as np
import pytest

from tests import edge_problems as E
from tests import oracle_libs as L

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "brdf_edge_fits.json")))
FITS = FIXTURE["fits"]
METHOD = ("dif", "bc_dif", "bc_der", "der")


def _hex(v):
    return np.array([float.fromhex(s) for s in v])


def _defined(info):
    """info[] without the entries levmar leaves undefined.  A fit whose start point already evaluates to NaN stops with reason 7
    before its first Jacobian (njev = 0); info[4] = mu / max(diag J^T J) then divides by the diagonal that the reference restores
    from work memory it never wrote (lmbc_core.c:534, :975-985) -- whatever the heap held.  The product's machines write 0 there
    and report 0/0 = NaN."""
    info = np.array(info, dtype=np.float64)
    if info[6] == 7 and info[8] == 0:
        info[4] = 0.0
    return info


def _same(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1], equal_nan=True)
            and np.array_equal(_defined(a[2]), _defined(b[2]), equal_nan=True))


def test_fixture_covers_every_case():
    assert [tuple(f[:5]) for f in FITS] == E.fixture_cases()
    assert os.path.getsize(os.path.join(HERE, "golden", "brdf_edge_fits.json")) < 512 * 1024


@pytest.mark.parametrize("family,model", E.cases(), ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["orc", "hm"])
def test_edge_fits_equal_the_reference_fixture(which, family, model):
    """every method x n in {5, 16, 64, 1000} x index of the family: ret, p and info[] (iterations, reason, nfev, njev, nlss)
    exactly the reference's"""
    rows = [f for f in FITS if f[0] == family and f[1] == model]
    assert rows
    for _, _, method, n, idx, ret, p, info in rows:
        got = L.brdf_fit(which, method, model, *E.fit_args(family, model, n, idx))
        assert _same(got, (ret, _hex(p), _hex(info))), (which, METHOD[method], n, idx, got, ret, p, info)


@pytest.mark.skipif(L.ref is None, reason="the reference's levmar lives in oracle/_ref")
@pytest.mark.parametrize("family,model", E.cases(), ids=lambda v: str(v))
def test_edge_fits_equal_the_live_reference(family, model):
    """the same fits run through the compiled reference now (the fixture cannot go stale), and a second problem index"""
    for method in E.methods(family):
        for n in E.FIXTURE_N:
            for idx in E.indices(family) + (7,):
                args = E.fit_args(family, model, n, idx)
                ref = L.brdf_fit("ref", method, model, *args)
                for which in ("orc", "hm"):
                    got = L.brdf_fit(which, method, model, *args)
                    assert _same(got, ref), (which, METHOD[method], n, idx, got, ref)


def test_bound_families_end_on_their_bounds():
    """the generator cannot drift back to interior data: every bound family has converged fits with a component exactly
    on its bound (the projection writes the bound's bits), in the fixture and live through the oracle"""
    for family in E.BOUND_FAMILIES:
        on = 0
        for f in FITS:
            if f[0] != family or f[2] not in (1, 2):
                continue
            _, model, method, n, idx, ret, p, info = f
            _, _, _, _, _, lb, ub = E.fit_args(family, model, n, idx)
            on += int(ret >= 0 and len(E.active_set(_hex(p), lb, ub)) > 0)
        assert on >= 4, (family, on)
    # the intended components: ks on lb, n on ub, alpha on lb, all three on the box
    want = {("diffuse_only", 1): (1, "lb"), ("shiny_beyond_box", 0): (2, "ub"), ("shiny_beyond_box", 1): (2, "ub"),
            ("ward_mirror", 2): (2, "lb"), ("tight_box", 0): (0, "ub"), ("high_lb", 1): (0, "lb")}
    for (family, model), comp in want.items():
        r, p, info = L.brdf_fit("orc", 1, model, *E.fit_args(family, model, 1000, 1))
        _, _, _, _, _, lb, ub = E.fit_args(family, model, 1000, 1)
        assert r >= 0 and comp in E.active_set(p, lb, ub), (family, model, p)
    for model in (0, 2):
        r, p, _ = L.brdf_fit("orc", 1, model, *E.fit_args("tight_box", model, 1000, 0))
        assert len(E.active_set(p, *E.fit_args("tight_box", model, 1000, 0)[5:])) == 3
        r, p, _ = L.brdf_fit("orc", 1, model, *E.fit_args("high_lb", model, 1000, 0))
        assert len(E.active_set(p, *E.fit_args("high_lb", model, 1000, 0)[5:])) == 3


def test_nonpositive_cosines_are_in_the_power_plane():
    for model in (0, 1):
        for idx in E.indices("nonpositive"):
            a, x, p0, lb, ub = E.make("nonpositive", model, 64, idx)
            k = E.power_plane(model)
            assert np.any(a[k] == 0.0) and (np.any(a[k] < 0.0) == (idx >= 2)) and np.all(a[[j for j in range(3) if j != k]] > 0.0)
            assert p0[2] == (1.0 if idx % 2 == 0 else 1.5)
            assert np.all(np.isfinite(x))


def test_zero_cosines_do_not_stop_the_analytic_methods():
    """pow(0, n) = 0 is a valid sample: its Jacobian row is (c0, 0, 0), not 0 * log 0 = NaN, so dlevmar_bc_der / dlevmar_der no
    longer stop at p0 with reason 5 ("no further error reduction is possible") -- in the fixture (the reference's solver on
    this project's jacf), through the oracle and through the host-driven product machines.  A negative cosine (index 2, 3)
    still makes the model itself NaN."""
    seen = 0
    for family, model, method, n, idx, ret, p, info in FITS:
        if family != "nonpositive" or method not in (2, 3):
            continue
        angles = E.make(family, model, n, idx)[0]
        if np.any(angles[E.power_plane(model)] < 0.0):
            assert idx >= 2
            continue
        assert idx < 2
        seen += 1
        assert ret >= 0 and _hex(info)[6] != 5 and np.all(np.isfinite(_hex(p))), (METHOD[method], model, n, idx, ret, p, info)
        for which in ("orc", "hm"):
            r, gp, gi = L.brdf_fit(which, method, model, *E.fit_args(family, model, n, idx))
            assert r >= 0 and gi[6] != 5 and np.all(np.isfinite(gp)), (which, METHOD[method], model, n, idx, r, gp, gi)
    assert seen == 2 * 2 * len(E.FIXTURE_N) * 2  # models x methods x sizes x indices: the 32 rows the fix changed


@pytest.mark.parametrize("family,model", [c for c in E.cases() if c[0] != "nonpositive"], ids=lambda v: str(v))
def test_prepared_sample_path_on_edge_families(family, model):
    """hm_fast: the product's FAST model path (cached log c / tan^2 / rsqrt, exp(n log c)) on the host, on every family whose
    cosines are all > 0.  Ward's two paths are the same operations: bit for bit.  Phong / Blinn-Phong: exp(n log c) is not
    pow(c, n), so the rule of test_prepared_sample_path_matches_oracle_within_tolerance holds where the fit is determined
    (n >= 64, both sides stop by a small gradient or step, ||e||^2 above round-off): p within 1e-7 -- 1e-6 for the secant
    (Broyden) updates of dlevmar_dif, which measured 1.9e-7 on quantised Phong -- and ||e||^2 within 1e-10.  Everywhere else
    (n = 5 / 16, itmax, a zero residual where p[2] is noise): both succeed, and the fast path's objective is no worse than
    the oracle's by more than 1e-3 relative."""
    determined = 0
    for method in E.methods(family):
        for n in E.FIXTURE_N:
            for idx in E.indices(family):
                args = E.fit_args(family, model, n, idx)
                assert np.all(args[0] > 0.0)
                a = L.brdf_fit("orc", method, model, *args)
                b = L.brdf_fit("hm_fast", method, model, *args)
                what = (METHOD[method], n, idx, a, b)
                if model == 2:
                    assert _same(a, b), what
                    continue
                assert (a[0] >= 0) == (b[0] >= 0), what
                if n >= 64 and a[2][6] in (1, 2) and b[2][6] in (1, 2) and a[2][1] > 1e-20:
                    determined += 1
                    assert L.rel_err(b[1], a[1]) <= (1e-6 if method == 0 else 1e-7), what
                    assert abs(b[2][1] - a[2][1]) <= 1e-10 * a[2][1], what
                elif a[0] >= 0:
                    assert b[2][1] <= a[2][1] * (1 + 1e-3) + 1e-20, what
    assert model == 2 or family not in ("diffuse_only", "quantised", "grazing", "start_on_bound") or determined > 0
