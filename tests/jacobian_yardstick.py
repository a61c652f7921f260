"""A yardstick for analytic Jacobian rows: the three partial derivatives of a BRDF model per sample, in 50-digit arithmetic.

The analytic Jacobian (brdf_amd/csrc/brdf_models.h: an_row; oracle/brdf_models_oracle.c: orc_brdf_jac) is this project's own --
the reference only differentiates numerically -- so no reference-owned number pins it.  mp_rows() differentiates the model's
expression by hand, once more and independently of both, and evaluates it with mpmath on the exact double inputs (PI is the
reference's double literal, as tests/test_gpu_edges.py: _mp_values does for the model values).  CPU only; the oracle test
(tests/test_oracle_jacobian.py) and the device test (tests/test_gpu_jacobian.py) judge their rows with check_rows().

    Phong        f = kd c0 + A ks c^n,  A = (n + 2)/2 PI        df/dkd = c0   df/dks = A c^n   df/dn = (PI/2) ks c^n + A ks c^n log c
    Blinn-Phong  f = kd c0 + ks c^n                             df/dkd = c0   df/dks = c^n     df/dn = ks c^n log c
    Ward         f = c0 (kd/PI + ks S),  S = k g rinv,          df/dkd = c0/PI  df/dks = c0 S
                 k = 1/(4 PI a^2), g = exp(-t2/a^2)             df/da = c0 ks S (2/a) (t2/a^2) - c0 ks S (2/a)

An entry comes as the list of its terms (two for Phong's and Ward's third column, one everywhere else), because its bound is
relative to sum |terms|, not to the entry: the two terms of a third column cancel (at n log c = -n/(n + 2); at t2 = a^2).

Limits.  A dead lobe -- c == 0 with n > 0, Ward with cos(N.H) == 0 -- has every lobe derivative 0: c^n log c -> 0, and
g (t2/a^2) = exp(-z) z -> 0.  Such an entry is marked DEAD and must be exactly 0.  Two cases are NOT judged: c == 0 with n == 0
(f does not depend on n there and c^n log c has no limit along n -> 0) and a negative powered cosine (pow is real only at
integral n; no derivative exists).

Bound of a judged entry:   |got - sum terms| <= (2 K_ULP + 8) u cond sum|terms| + abs_floor
  * u = 2^-53.  A term is a product of at most two transcendentals (pow or exp, and log), each good to K_ULP ulp
    (tests/stats_yardstick.py: device against host libm), and of at most eight correctly rounded operations: the products and
    quotients that build A or k, rinv and its square root, the final product and the sum of the two terms (at most 7 for
    Phong's second term, 8 for Ward's first).  A term's error is relative to the term; the sum's rounding is relative to
    |sum| <= sum|terms|.
  * cond is 1 for Phong / Blinn-Phong.  Ward's exp takes t2/a^2 with t2 = (1 - c1^2)/c1^2 rounded: its relative error
    (2 + 1/(2 t2)) u (the subtraction 1 - c1^2 cancels) is multiplied by the argument, which is _mp_values' factor
    cond = 1 + (t2/a^2) (1 + 1/(2 t2)).  The same factor covers the first term's explicit t2/a^2: its relative error
    (1 + 1/(2 t2)) u scales a term that is t2/a^2 times the second one.
  * abs_floor is _mp_values' subnormal rule: where the lobe factor is subnormal each rounding loses up to one unit of the
    smallest subnormal, scaled by what multiplies the lobe factor afterwards: (2 + 2 |term / lobe factor|) TINY per term.
"""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np

from brdf_amd import synth
from tests import edge_problems as E
from tests.stats_yardstick import K_ULP
from tests.test_gpu_edges import ALPHAS, COS, TINY, U, _value_grid, _ward_underflow_planes

JUDGED, DEAD, NOT_JUDGED = "judged", "dead", "not judged"
ROUNDINGS = 8
REL = (2 * K_ULP + ROUNDINGS) * U
PHONG_EXPONENTS = (1.0, 2.5, 24.0, 100.0, 1000.0, 0.0)  # 0: not judged at c == 0


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def mp_rows(model: int, angles, p):
    """per sample, three entries (kind, terms, cond, abs_floor): kind JUDGED / DEAD / NOT_JUDGED; terms: the entry's terms as mpf
    (their sum is the derivative; DEAD: zeros; NOT_JUDGED: empty); cond and abs_floor: see the module's docstring"""
    mp = _mp()
    PI = mp.mpf(synth.PI)
    kd, ks, q = (mp.mpf(float(v)) for v in p)
    zero = mp.mpf(0)
    rows = []
    for c0, c1, c2 in zip(*(map(float, np.asarray(angles)[k]) for k in range(3))):
        c0, c1, c2 = mp.mpf(c0), mp.mpf(c1), mp.mpf(c2)
        if model in (0, 1):
            c = c2 if model == 0 else c1
            A = (q + 2) / 2 * PI if model == 0 else mp.mpf(1)
            first = (JUDGED, [c0], 1.0, 2 * TINY)
            if c < 0:
                rows.append([first, (NOT_JUDGED, [], 1.0, 0.0), (NOT_JUDGED, [], 1.0, 0.0)])
                continue
            if c == 0 and q > 0:
                lobe = [zero, zero] if model == 0 else [zero]
                rows.append([first, (DEAD, [zero], 1.0, 0.0), (DEAD, lobe, 1.0, 0.0)])
                continue
            s = mp.mpf(1) if q == 0 else mp.power(c, q)  # (c == 0 with q < 0 does not occur: the box holds n >= 0)
            second = (JUDGED, [A * s], 1.0, (2 + 2 * float(A)) * TINY)
            if c == 0:  # q == 0
                rows.append([first, second, (NOT_JUDGED, [], 1.0, 0.0)])
                continue
            lc = mp.log(c)
            mults = [PI / 2 * ks, A * ks * lc] if model == 0 else [ks * lc]
            floor = sum((2 + 2 * float(abs(m))) * TINY for m in mults)
            rows.append([first, second, (JUDGED, [m * s for m in mults], 1.0, floor)])
        else:
            a2 = q * q
            k = 1 / (4 * PI * a2)
            rinv = 1 / mp.sqrt(c0 * c2)
            first = (JUDGED, [c0 / PI], 1.0, 2 * TINY)
            if c1 == 0:
                rows.append([first, (DEAD, [zero], 1.0, 0.0), (DEAD, [zero, zero], 1.0, 0.0)])
                continue
            t2 = (1 - c1 * c1) / (c1 * c1)
            arg = t2 / a2
            g = mp.exp(-arg)
            cond = 1 + float(min(arg, mp.mpf(1e300))) * (1 + (1 / (2 * float(t2)) if t2 > 0 else 0.0))
            m1 = c0 * k * rinv  # what multiplies g
            m2 = [m1 * ks * (2 / q) * arg, -m1 * ks * (2 / q)]
            rows.append([first, (JUDGED, [m1 * g], cond, (2 + 2 * float(abs(m1))) * TINY),
                         (JUDGED, [m * g for m in m2], cond, sum((2 + 2 * float(min(abs(m), mp.mpf(1e300)))) * TINY for m in m2))])
    return rows


def ieee_rows(model: int, angles, p):
    """the row's expression in plain IEEE double (numpy), with no special case anywhere: where a NOT_JUDGED entry is NaN or
    infinite, this is"""
    a = np.asarray(angles, dtype=np.float64)
    kd, ks, q = (np.float64(v) for v in p)
    with np.errstate(all="ignore"):
        if model in (0, 1):
            c = a[E.power_plane(model)]
            s, lc = np.power(c, q), np.log(c)
            if model == 0:
                A = (q + 2.0) / 2.0 * synth.PI
                return np.stack([a[0], A * s, ((1.0 / 2.0 * synth.PI) * ks) * s + ((A * ks) * s) * lc], axis=1)
            return np.stack([a[0], s, (ks * s) * lc], axis=1)
        a2 = q * q
        ch2 = a[1] * a[1]
        t2 = (1.0 - ch2) / ch2
        spec = ((1.0 / (4.0 * synth.PI * a2)) * np.exp(-(t2 * (1.0 / a2)))) * (1.0 / np.sqrt(a[0] * a[2]))
        return np.stack([a[0] / synth.PI, a[0] * spec, a[0] * ((ks * spec) * ((2.0 / q) * (t2 * (1.0 / a2) - 1.0)))], axis=1)


def check_rows(got, model: int, angles, p, what, tally=None):
    """got [n, 3] against mp_rows: every JUDGED entry inside its bound, every DEAD entry exactly 0, every NOT_JUDGED entry NaN or
    infinite exactly where the IEEE expression is.  Returns the worst error of a judged entry in units of u cond sum|terms|
    (entries whose subnormal floor is more than 1 % of their relative bound are held to the bound but left out of that figure); tally (a dict) counts the kinds."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    ieee = ieee_rows(model, angles, p)
    worst = 0.0
    for i, row in enumerate(mp_rows(model, angles, p)):
        for j, (kind, terms, cond, floor) in enumerate(row):
            g = float(got[i, j])
            if tally is not None:
                tally[kind] = tally.get(kind, 0) + 1
            where = (what, "sample", i, "column", j, [float(np.asarray(angles)[k][i]) for k in range(3)], g)
            if kind == NOT_JUDGED:
                e = float(ieee[i, j])
                assert math.isnan(g) == math.isnan(e) and math.isinf(g) == math.isinf(e), where + (e,)
                continue
            if kind == DEAD:
                assert g == 0.0, where
                continue
            assert math.isfinite(g), where
            total = sum(terms)
            scale = float(sum(abs(t) for t in terms))
            err = float(abs(_mp().mpf(g) - total))
            bound = REL * cond * scale + floor
            assert err <= bound, where + (float(total), err, bound, err / scale / (U * cond) if scale > 0 else None)
            if floor <= 0.01 * REL * cond * scale:
                worst = max(worst, err / scale / (U * cond))
    return worst


def grid(model: int):
    """[(planes [3, N], p)]: the edge grid of the model values (tests/test_gpu_edges.py) with the parameters of this yardstick,
    and 200 seeded ordinary samples in [0.05, 1)"""
    ordinary = np.ascontiguousarray(synth.make_single(model, 200)[0])
    assert ordinary.min() >= 0.05 and ordinary.max() < 1.0
    if model in (0, 1):
        planes = _value_grid(model)
        sets = [(planes, (kd, ks, q)) for kd in (0.0, 0.35) for ks in (0.0, 0.6, 1.0) for q in PHONG_EXPONENTS]
        sets += [(ordinary, (0.35, 0.6, q)) for q in PHONG_EXPONENTS] + [(ordinary, synth.TRUTH[model])]
        return sets
    planes = _value_grid(2)
    sets = [(planes, (kd, ks, al)) for kd in (0.0, 0.35) for ks in (0.0, 0.25, 1.0) for al in ALPHAS]
    sets += [(_ward_underflow_planes(al), (0.0, 1.0, al)) for al in ALPHAS]
    sets += [(ordinary, (0.35, 0.25, al)) for al in ALPHAS] + [(ordinary, synth.TRUTH[2])]
    return sets


def dead_rows(model: int):
    """(planes [3, N], p) whose every row has a dead lobe: the powered cosine 0 over the normal part of the cosine grid"""
    normal = np.array([c for c in COS if c >= 1e-8])
    planes = np.stack([normal, normal, normal])
    planes[E.power_plane(model) if model in (0, 1) else 1] = 0.0
    return np.ascontiguousarray(planes), {0: (0.35, 0.6, 24.0), 1: (0.35, 0.6, 2.5), 2: (0.35, 0.25, 0.1)}[model]


@functools.lru_cache(maxsize=None)
def _dead_lobe_fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brdf_dead_lobe_fits.json")) as fh:
        return json.load(fh)["fits"]


def dead_lobe_reference(model: int, method: int, n: int, index: int):
    """(ret, p, info) of the compiled reference's finite-difference solver on the dead-lobe problem (model, n, index) of
    tests/edge_problems.py, from tests/golden/brdf_dead_lobe_fits.json: dlevmar_bc_dif for the box methods (1, 2), dlevmar_dif
    for the others -- the optimum an analytic-Jacobian fit of the same data is held to"""
    twin = 1 if method in (1, 2) else 0
    row = next(f for f in _dead_lobe_fixture() if tuple(f[:4]) == (model, twin, n, index))
    return row[4], np.array([float.fromhex(v) for v in row[5]]), np.array([float.fromhex(v) for v in row[6]])
