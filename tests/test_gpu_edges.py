"""Edge-of-domain fits on the device, in every fit regime, against the CPU oracle (tests/edge_problems.py): solutions on the
box, starts on it, black / saturated / quantised pixels, grazing and non-positive cosines, fewer than 16 samples.  And the
invariants that must hold bit for bit there: the multi-candidate projected-gradient search (BRDF_HIP_PG_MULTI) and the fast
path's fall-back to the exact model (a cosine <= 0).  Model values at the edge of their domain are checked against a 50-digit
mpmath evaluation of the same expressions.

Per fit, against the oracle on the same inputs and box (at least the bar of test_gpu_parity.py):
  * both succeed or both fail; where they fail, with the same reason (info[6]);
  * both converge (reason 1 / 2) and n >= 64: the same set of components on a bound, each exactly on it (the projection
    writes the bound's bits), the free ones within P_TOL, ||e||^2 within E_TOL;
  * ||e||^2 at round-off (reason 6, ||e||^2 <= opts[3]): the device's no more than the oracle's + opts[3] -- p is noise there;
  * otherwise (n < 64, or the oracle at itmax): the objective, info[1] <= ref * (1 + 1e-3); where the device itself ends at
    itmax on another path, as the suite already allows for 16-sample fits, no more than 30 % above.
Two cases of a converged fit are counted, not failed, because there the data do not determine p to P_TOL:
  * "flat": same active set, ||e||^2 within E_TOL, and the free components differ only along a direction the objective does
    not see -- (p - p_ref)' J'J (p - p_ref) <= FLAT_TOL * ||e||^2 with J the model's Jacobian at the oracle's point.  Measured:
    saturated Ward (dlevmar_dif, x == 1) with ks 1.4e-5 apart at 6e-17 ||e||^2; Ward started on its box with alpha held on
    0.01, where ks ~ 1e-7 barely moves the narrow lobe, at 6e-18 ||e||^2.  A well-determined fit 1e-5 apart in p sits at
    1e-7 ... 1e-5 ||e||^2, so FLAT_TOL = 1e-12 is far inside what P_TOL admits elsewhere;
  * "oracle stopped short": the oracle stopped on a small step (reason 2) at a higher objective than the device reached --
    the reference stalling on a degenerate Jacobian (Ward with ks held on 0 leaves alpha without effect), measured on a dark
    Ward pixel: kd 0.00772 against the optimum 0.0072438 the device found.  Bounded per test.
The GPU sums in trees, the oracle in sequence, so trajectories (nfev, iterations) are not compared there."""
import collections
import ctypes as C
import functools
import math

import numpy as np
import pytest

from brdf_amd import synth
from tests import edge_problems as E
from tests import oracle_libs as L

pytestmark = pytest.mark.gpu
P_TOL = 1e-5
E_TOL = 1e-8
FLAT_TOL = 1e-12
EPS3 = synth.OPTS[3]
METHOD = ("dif", "bc_dif", "bc_der", "der")
U = 2.0 ** -53  # unit roundoff
TINY = 2.0 ** -1074  # smallest subnormal


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _t(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bc(method):
    return method in (1, 2)


@functools.lru_cache(maxsize=None)
def _problem(family, model, n, idx):
    return E.make(family, model, n, idx)


@functools.lru_cache(maxsize=None)
def _oracle(family, model, method, n, idx):
    return L.brdf_fit("orc", method, model, *E.fit_args(family, model, n, idx))


def _single(gpu, method, model, angles, x, p0, lb, ub, **kw):
    _, brdf_amd, _ = gpu
    bc = _bc(method)
    return brdf_amd.fit_single(method, model, _t(gpu, angles), _t(gpu, x), p0, lb=lb if bc else None, ub=ub if bc else None,
                               itmax=synth.ITMAX, opts=synth.OPTS, **kw)


def _identical(a, b):
    """two FitResults, bit for bit"""
    return (a.ret == b.ret and np.array_equal(a.p, b.p, equal_nan=True) and np.array_equal(a.info, b.info, equal_nan=True)
            and (a.covar is None) == (b.covar is None) and (a.covar is None or np.array_equal(a.covar, b.covar, equal_nan=True)))


def _rel(p, p_ref):
    """relative difference; components that are zero to round-off (|p| < 1e-6, e.g. ks = 4e-12 just off its bound) are
    compared on the parameters' unit scale"""
    p, p_ref = np.asarray(p, dtype=np.float64), np.asarray(p_ref, dtype=np.float64)
    return float(np.max(np.abs(p - p_ref) / np.maximum(np.abs(p_ref), 1e-6))) if p.size else 0.0


def _jtj(model, angles, p):
    """J'J of the model's analytic Jacobian (the oracle's) at p over the samples"""
    a = L.f64(angles)
    n = a.size // 3
    jac = np.zeros(3 * n)

    class Extra(C.Structure):
        _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]

    L.orc.orc_brdf_jac(L.ptr(L.f64(p).copy()), L.ptr(jac), 3, n, C.byref(Extra(L.ptr(a), model)))
    jac = jac.reshape(n, 3)
    return jac.T @ jac


def _judge(got, ref, lb, ub, n, method, model, angles, what):
    """one device fit (ret, p, info) against the oracle's on the planes `angles`: (kind of comparison made, None or what
    failed)"""
    gr, gp, gi = got
    rr, rp, ri = ref
    what = (what, METHOD[method], n, (int(gr), [float(v).hex() for v in gp], [float(v) for v in gi]),
            (int(rr), [float(v).hex() for v in rp], [float(v) for v in ri]))
    if (gr >= 0) != (rr >= 0):
        return "failed", ("success differs",) + what
    if rr < 0:
        return "failed", None if gi[6] == ri[6] else ("failure reason differs",) + what
    if ri[6] == 6 or gi[6] == 6:
        return "zero residual", None if gi[1] <= ri[1] * (1 + 1e-3) + EPS3 else ("objective",) + what
    if ri[6] in (1, 2) and gi[6] in (1, 2) and n >= 64:
        gp, rp = np.array(gp), np.array(rp)
        if not _bc(method) and model == 2:  # unconstrained Ward depends on alpha^2
            gp[2], rp[2] = abs(gp[2]), abs(rp[2])
        act_g, act_r = (E.active_set(gp, lb, ub), E.active_set(rp, lb, ub)) if _bc(method) else ((), ())
        free = [j for j in range(3) if j not in dict(act_r)]
        if act_g == act_r and _rel(gp[free], rp[free]) <= P_TOL and abs(gi[1] - ri[1]) <= E_TOL * ri[1]:
            return ("active" if act_r else "compared"), None
        if act_g == act_r and abs(gi[1] - ri[1]) <= E_TOL * ri[1]:
            d = (gp - rp)[free]
            if float(d @ _jtj(model, angles, rp)[np.ix_(free, free)] @ d) <= FLAT_TOL * ri[1]:
                return "flat", None
        if ri[6] == 2 and gi[1] < ri[1] * (1 - E_TOL):
            # the oracle (= the reference) stopped on a small step short of the optimum the device reached: a degenerate
            # Jacobian (ks held on 0 leaves Ward's alpha without effect) -- the device is not wrong there
            return "oracle stopped short", None
        return "compared", ("active set / parameters / objective",) + what
    if gi[6] == 3:  # the device ran out of iterations on another path (the suite exempts these from objective parity)
        return "itmax", None if gi[1] <= ri[1] * 1.3 + 1e-30 else ("objective (itmax)",) + what
    return "objective", None if gi[1] <= ri[1] * (1 + 1e-3) + 1e-30 else ("objective",) + what


def _tally(kinds, bad, judged):
    kind, problem = judged
    kinds[kind] += 1
    if problem is not None:
        bad.append(problem)


# ---- single fits: resident regime, launch chain, diagonal scaling ------------------------------------------------------
def _single_cases():
    """(family, model, method, n, idx): every family x model x method at n = 64 (every index) and n = 5000 (index 0)"""
    out = []
    for family, model in E.cases():
        for method in E.methods(family):
            out += [(family, model, method, 64, i) for i in E.indices(family)]
            out.append((family, model, method, 5000, 0))
    return out


@pytest.mark.parametrize("regime", ["1", "0"], ids=["resident", "launch_chain"])
def test_single_fits_against_the_oracle(gpu, monkeypatch, regime):
    torch, brdf_amd, dev = gpu
    monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
    kinds, bad = collections.Counter(), []
    for family, model, method, n, idx in _single_cases() + [("shiny_beyond_box", 1, 1, 262145, 0)]:
        angles, x, p0, lb, ub = _problem(family, model, n, idx)
        res = _single(gpu, method, model, angles, x, p0, lb, ub)
        _tally(kinds, bad, _judge((res.ret, res.p, res.info), _oracle(family, model, method, n, idx), lb, ub, n, method, model,
                                  angles, (regime, family, model, idx)))
        if family != "nonpositive" and n == 5000:
            assert (brdf_amd.last_fit_stats()["launches"] == 1) == (regime == "1")
    print(f"single fits, BRDF_HIP_RESIDENT={regime}: {dict(kinds)}")
    assert not bad, "\n".join(map(str, bad))
    assert kinds["active"] >= 30 and kinds["failed"] >= 4
    assert kinds["oracle stopped short"] <= 4 and kinds["flat"] <= 0.05 * sum(kinds.values())


def test_diagonal_scaling_with_an_active_bound(gpu, monkeypatch):
    """dscl with a bound that does not round-trip through the scaling: levmar fits in scaled space, so the active component
    is (ub/dscl)*dscl -- the oracle's bits, not the bound's own.  Resident regime and launch chain."""
    model, n = 2, 5000
    ds = 3.0
    ub0 = next(v for v in (0.21, 0.23, 0.3) if (v / ds) * ds != v)  # 0.21 / 3 * 3 = 0.20999999999999996
    angles, x, _ = synth.make_single(model, n)
    lb, ub, dscl = np.array(synth.bounds(model)[0]), np.array([ub0, 100.0, 100.0]), np.array([ds, 1.0, 1.0])
    flat = np.ascontiguousarray(angles.reshape(-1))

    class Extra(C.Structure):
        _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]

    for method in (1, 2):
        p = np.array(synth.P0[model])
        info, opts = np.zeros(10), np.array(synth.OPTS)
        fptr = C.cast(L.orc.orc_brdf_func, C.c_void_p)
        if method == 1:
            r = L.orc.orc_dlevmar_bc_dif(fptr, L.ptr(p), L.ptr(x), 3, n, L.ptr(lb), L.ptr(ub), L.ptr(dscl), synth.ITMAX, L.ptr(opts),
                                         L.ptr(info), None, None, C.byref(Extra(L.ptr(flat), model)))
        else:
            jptr = C.cast(L.orc.orc_brdf_jac, C.c_void_p)
            r = L.orc.orc_dlevmar_bc_der(fptr, jptr, L.ptr(p), L.ptr(x), 3, n, L.ptr(lb), L.ptr(ub), L.ptr(dscl), synth.ITMAX,
                                         L.ptr(opts), L.ptr(info), None, None, C.byref(Extra(L.ptr(flat), model)))
        assert r >= 0 and info[6] in (1, 2) and p[0] == (ub0 / ds) * ds != ub0, (p, info)
        for regime in ("1", "0"):
            monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
            res = _single(gpu, method, model, angles, x, synth.P0[model], lb, ub, dscl=dscl)
            what = (regime, METHOD[method], res.p, p, res.info, info)
            assert res.ret >= 0 and res.info[6] in (1, 2), what
            assert res.p[0] == p[0], what
            assert L.rel_err(res.p[1:], p[1:]) <= P_TOL and abs(res.info[1] - info[1]) <= E_TOL * info[1], what


# ---- channels: one set of planes, three measurement vectors ----------------------------------------------------------
def _three_channels(model, n, zero_cosine=False):
    """interior (synthetic truth), diffuse only (ks ends on 0) and dark, over the planes of synth.make_single"""
    angles, _, _ = synth.make_single(model, n)
    angles = angles.copy()
    if zero_cosine:
        angles[E.power_plane(model), 5] = 0.0
    rng = np.random.default_rng(31 + model)
    noise = 0.01 * (rng.random(n) - 0.5)
    t = np.array(synth.TRUTH[model])
    t[1] = -0.05
    diffuse = synth.model_value(model, t, angles[0], angles[1], angles[2]) + noise
    dark = np.clip(noise, 0.0, None)
    interior = synth.model_value(model, synth.TRUTH[model], angles[0], angles[1], angles[2]) + 0.01 * (rng.random(n) - 0.5)
    return angles, np.stack([interior, diffuse, dark])


@pytest.mark.parametrize("model", [0, 1, 2])
def test_channels_with_active_bounds_equal_single_fits(gpu, monkeypatch, model):
    """brdf_hip_fit_channels_dev with one interior channel, one ending on ks = 0 and a dark one: every channel bit-identical to
    its single fit, in the shared launch and with BRDF_HIP_CHANNELS=0; then with a zero cosine in the powered plane, where the
    whole shared launch falls back to the exact model -- identical to the single fits under BRDF_HIP_EXACT_POW=1"""
    torch, brdf_amd, dev = gpu
    lb, ub = synth.bounds(model)
    on_bound = 0
    for zero_cosine in ((False, True) if model != 2 else (False,)):
        for n in (300, 5000):
            angles, xs = _three_channels(model, n, zero_cosine)
            a, xd = _t(gpu, angles), _t(gpu, xs)
            for method in (1, 2):
                kw = dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
                monkeypatch.delenv("BRDF_HIP_CHANNELS", raising=False)
                shared = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], **kw)
                monkeypatch.setenv("BRDF_HIP_CHANNELS", "0")
                apart = brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], **kw)
                monkeypatch.delenv("BRDF_HIP_CHANNELS")
                for c in range(3):
                    alone = brdf_amd.fit_single(method, model, a, xd[c], synth.P0[model], **kw)
                    what = (zero_cosine, n, METHOD[method], c, shared[c], alone)
                    assert _identical(shared[c], alone) and _identical(apart[c], alone), what
                    ref = L.brdf_fit("orc", method, model, angles, xs[c], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
                    _, problem = _judge((alone.ret, alone.p, alone.info), ref, lb, ub, n, method, model, angles,
                                        ("channel", model, zero_cosine, c))
                    assert problem is None, problem
                    on_bound += int(alone.ret >= 0 and len(E.active_set(alone.p, lb, ub)) > 0)
                    if zero_cosine:
                        monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
                        exact = brdf_amd.fit_single(method, model, a, xd[c], synth.P0[model], **kw)
                        monkeypatch.delenv("BRDF_HIP_EXACT_POW")
                        assert _identical(shared[c], exact), (what, exact)
    assert on_bound >= 2


# ---- batches: every kernel, families interleaved in one launch --------------------------------------------------------
def _batch_groups(model, n, per_family):
    """the families of `model` at n samples, interleaved (index-major), one group per box: [(lb, ub, [(family, idx)])]"""
    groups = {}
    for idx in range(max(per_family, 4)):
        for family, m in E.cases(models=(model,)):
            if idx >= per_family and family != "nonpositive":  # (every kind of non-positive cosine in every batch)
                continue
            _, _, _, lb, ub = _problem(family, model, n, idx)
            groups.setdefault((tuple(lb), tuple(ub)), []).append((family, idx))
    return [(np.array(k[0]), np.array(k[1]), v) for k, v in groups.items()]


def _run_batch(gpu, method, model, n, items):
    torch, brdf_amd, dev = gpu
    probs = [_problem(f, model, n, i) for f, i in items]
    angles = np.stack([p[0] for p in probs])
    x = np.stack([p[1] for p in probs])
    p0 = np.stack([p[2] for p in probs])
    lb, ub = probs[0][3], probs[0][4]
    p, info, ret = brdf_amd.fit_batch(method, model, _t(gpu, angles), _t(gpu, x), _t(gpu, p0), lb=lb if _bc(method) else None,
                                      ub=ub if _bc(method) else None, itmax=synth.ITMAX, opts=synth.OPTS)
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


# kernel -> (environment, sample counts, methods).  n <= 16 bc_dif / bc_der: one lane per fit; BRDF_HIP_LANE=0: one wave per
# fit (BRDF_HIP_ROWS=1: four fits per wavefront); <= 256: wave per fit; <= 1024: workgroup; <= 4096: eight waves
# (BRDF_HIP_BATCH_BIG=0: the 512 x 8 workgroup); > 4096: one fit after the other through the single-fit path
BATCH_KERNELS = {
    "lane": ({}, (3, 7, 15, 16), (1, 2)),
    "rows": ({"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "1"}, (7, 16), (1,)),
    "wave16": ({"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "0"}, (16,), (1,)),
    "wave": ({}, (17, 64, 65, 256), (1, 2)),
    "workgroup": ({}, (257, 1024), (1, 2)),
    "eight_wave": ({}, (1025, 4096), (1, 2)),
    "big_off": ({"BRDF_HIP_BATCH_BIG": "0"}, (4096,), (1,)),
    "one_by_one": ({}, (4097,), (1,)),
}


@pytest.mark.parametrize("kernel", list(BATCH_KERNELS))
def test_batch_kernels_against_the_oracle(gpu, monkeypatch, kernel):
    env, sizes, methods = BATCH_KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kinds, bad = collections.Counter(), []
    for n in sizes:
        per_family = 6 if n <= 1024 else (3 if n <= 4096 else 2)
        for model in (0, 1, 2):
            for lb, ub, items in _batch_groups(model, n, per_family):
                for method in methods:
                    p, info, ret = _run_batch(gpu, method, model, n, items)
                    for s, (family, idx) in enumerate(items):
                        ref = L.brdf_fit("orc", method, model, *E.fit_args(family, model, n, idx))
                        _tally(kinds, bad, _judge((int(ret[s]), p[s], info[s]), ref, lb, ub, n, method, model, _problem(family, model, n, idx)[0],
                                                  (kernel, family, model, idx)))
    print(f"batch kernel {kernel}: {dict(kinds)}")
    assert not bad, "\n".join(map(str, bad))
    assert kinds["failed"] >= 2 and kinds["oracle stopped short"] + kinds["flat"] <= 0.05 * sum(kinds.values()) + 2
    assert kernel in ("lane", "rows", "wave16") or kinds["active"] >= (10 if kernel != "one_by_one" else 5)


def test_lane_kernel_exact_path_replays_the_oracle(gpu, monkeypatch):
    """BRDF_HIP_EXACT_POW=1 on the lane kernel: it sums in the reference's order with the reference's pow expression, so
    what is left is the last bit of pow / exp (ocml vs glibc).  Fraction of the edge fits whose iterations, reason and nfev
    (info[5:8]) are exactly the oracle's."""
    monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
    same = total = 0
    for n in (3, 7, 15, 16):
        for model in (0, 1, 2):
            for lb, ub, items in _batch_groups(model, n, 6):
                _, info, ret = _run_batch(gpu, 1, model, n, items)
                for s, (family, idx) in enumerate(items):
                    ref = L.brdf_fit("orc", 1, model, *E.fit_args(family, model, n, idx))
                    total += 1
                    same += int(np.array_equal(info[s, 5:8], ref[2][5:8]))
    print(f"lane kernel, BRDF_HIP_EXACT_POW=1: {same}/{total} = {same / total:.3f} of the edge fits with info[5:8] identical")
    assert same >= LANE_EXACT_FLOOR * total


LANE_EXACT_FLOOR = 0.65  # measured on the MI355X: 489 / 696 = 0.703


# ---- the capture loop -------------------------------------------------------------------------------------------------
def test_capture_with_black_saturated_and_diffuse_faces(gpu):
    """brdf_hip_fit_capture_dev on a capture where some faces are black, some saturated and one diffuse only (ks = 0 in the
    render): objective parity with the oracle's walk for every (face, channel)"""
    from tests.test_cosines import _objective, make_capture
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture()
    H, W = pixel_map.shape
    touched = np.unique(pixel_map[pixel_map > -1])
    black, saturated, diffuse = set(touched[0::5]), set(touched[1::5]), int(touched[2])
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f in black:
                images[:, H - 1 - y, x, :] = 0
            elif f in saturated:
                images[:, H - 1 - y, x, :] = 255
            elif f == diffuse:
                for ch in range(3):
                    val = L.model_values(1, np.abs(ang[f]), (0.4 + 0.2 * ch, 0.0, 24.0))
                    images[:, H - 1 - y, x, ch] = np.clip(np.round(val * 255.0 * 0.5), 0, 255).astype(np.uint8)
    opts = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
    want, avg_ref, npx_ref = L.fit_capture(1, images, pixel_map, vertices, faces, nrm, leds, view, rv_mode=1, opts=opts)
    tv, tf, tn = (_t(gpu, a) for a in (vertices, faces, nrm))
    got, avg, npx = brdf_amd.fit_capture(1, _t(gpu, images), _t(gpu, pixel_map), tv, tf, tn, leds, view, rv_mode=1, opts=opts)
    got = got.cpu().numpy()
    assert npx == npx_ref
    for f in touched:
        x_, y_ = max((x, y) for y in range(H) for x in range(W) if pixel_map[y, x] == f)
        for ch in range(3):
            I = images[:, H - 1 - y_, x_, ch] / 255.0
            o_got, o_ref = _objective(1, ang[f], I, got[f, ch]), _objective(1, ang[f], I, want[f, ch])
            assert np.all(np.isfinite(got[f, ch])) and np.all(got[f, ch] >= 0.0), (f, ch, got[f, ch])
            assert o_got <= o_ref * (1 + 1e-3) + 1e-20, (f, ch, got[f, ch], want[f, ch], o_got, o_ref)
            if f in black and o_ref <= EPS3:  # x = 0: the fit ends at round-off (unless a negative cosine made it fail)
                assert o_got <= EPS3, (f, ch, got[f, ch], want[f, ch])
    assert np.all(np.isfinite(avg)) and np.all(np.abs(avg - avg_ref) <= 0.05 * np.abs(avg_ref) + 1e-6)


# ---- bit-for-bit invariants: the multi-candidate projected-gradient search --------------------------------------------
def _pg_pair(monkeypatch, run):
    """run() with BRDF_HIP_PG_MULTI=1 and with the default (8)"""
    monkeypatch.setenv("BRDF_HIP_PG_MULTI", "1")
    one = run()
    monkeypatch.delenv("BRDF_HIP_PG_MULTI")
    return one, run()


def test_pg_multi_single_fits_do_not_change_a_bit(gpu, monkeypatch):
    """lm_machine.h (BcMachine::Cold::multi): up to 8 projected-gradient candidates per sweep are judged in the reference's
    order and only the judged ones are counted -- ret, p, info[] and the covariance are those of the one-at-a-time search, in
    the resident regime and the launch chain, on synthetic interior data and on the edge families; never more passes"""
    torch, brdf_amd, dev = gpu
    problems = [("synthetic", model, n, synth.make_single(model, n) + (None,)) for model, n in ((2, 100003), (1, 5000), (0, 5000))]
    for family, model in E.cases(families=E.BOUND_FAMILIES + ("start_on_bound", "quantised", "grazing")):
        problems.append((family, model, 5000, _problem(family, model, 5000, 0)))
    fewer = 0
    for regime in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
        for family, model, n, prob in problems:
            if family == "synthetic":
                angles, x = prob[0], prob[1]
                p0, (lb, ub) = synth.P0[model], synth.bounds(model)
            else:
                angles, x, p0, lb, ub = prob
            for method in (1, 2):
                def run():
                    r = _single(gpu, method, model, angles, x, p0, lb, ub, want_covar=True)
                    return r, brdf_amd.last_fit_stats()["passes"]
                (a, pa), (b, pb) = _pg_pair(monkeypatch, run)
                what = (regime, family, model, METHOD[method], a, b)
                assert _identical(a, b), what
                assert pb <= pa, (what, pa, pb)
                fewer += int(pb < pa and method == 1)
    assert fewer > 0


def test_pg_multi_channels_and_batches_do_not_change_a_bit(gpu, monkeypatch):
    torch, brdf_amd, dev = gpu
    for model in (0, 1, 2):
        lb, ub = synth.bounds(model)
        angles, xs = _three_channels(model, 5000)
        a, xd = _t(gpu, angles), _t(gpu, xs)
        for method in (1, 2):
            one, multi = _pg_pair(monkeypatch, lambda: brdf_amd.fit_channels(method, model, a, xd, synth.P0[model], lb=lb, ub=ub,
                                                                              itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True))
            for c in range(3):
                assert _identical(one[c], multi[c]), (model, METHOD[method], c, one[c], multi[c])
    for n in (16, 64, 1024, 4096):  # lane, wave, workgroup, eight waves
        for model in (0, 1, 2):
            for method in (1, 2):
                groups = _batch_groups(model, n, 2 if n > 1024 else 4)
                for lb, ub, items in groups:
                    one, multi = _pg_pair(monkeypatch, lambda: _run_batch(gpu, method, model, n, items))
                    for u, v in zip(one, multi):
                        assert np.array_equal(u, v, equal_nan=True), (n, model, METHOD[method], items)
                S = 24
                sa, sx, _ = synth.make_surfels(model, n, first=500, count=S)
                p0 = np.tile(np.array(synth.P0[model]), (S, 1))

                def synthetic():
                    p, info, ret = brdf_amd.fit_batch(method, model, _t(gpu, sa), _t(gpu, sx), _t(gpu, p0), lb=lb, ub=ub,
                                                      itmax=synth.ITMAX, opts=synth.OPTS)
                    torch.cuda.synchronize()
                    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
                one, multi = _pg_pair(monkeypatch, synthetic)
                for u, v in zip(one, multi):
                    assert np.array_equal(u, v, equal_nan=True), (n, model, METHOD[method], "synthetic")


# ---- bit-for-bit invariants: the fast path's fall-back to the exact model ---------------------------------------------
FALLBACK_BATCH = {  # kernel -> (environment, n)
    "lane": ({}, 16), "rows": ({"BRDF_HIP_LANE": "0", "BRDF_HIP_ROWS": "1"}, 16), "wave16": ({"BRDF_HIP_LANE": "0"}, 16),
    "wave": ({}, 64), "wave4": ({}, 256), "workgroup": ({}, 1024), "eight_wave": ({}, 4096),
    "big_off": ({"BRDF_HIP_BATCH_BIG": "0"}, 4096), "one_by_one": ({}, 4097),
}


def _bad_replaced(angles, model):
    """the same planes with every cosine <= 0 of the powered plane replaced by a small positive one"""
    a = angles.copy()
    k = E.power_plane(model)
    a[..., k, :] = np.where(a[..., k, :] <= 0.0, 1e-3, a[..., k, :])
    return a


@pytest.mark.parametrize("model", [0, 1])
def test_nonpositive_cosine_single_fits_take_the_exact_path(gpu, monkeypatch, model):
    """a single fit with a cosine <= 0 (Phong's c2, Blinn-Phong's c1; integral and non-integral start) is the exact-path fit,
    bit for bit: the fast attempt is thrown away -- resident regime and launch chain; same outcome as the oracle"""
    torch, brdf_amd, dev = gpu
    differs = 0
    for regime in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
        for n in (64, 5000):
            for idx in E.indices("nonpositive"):
                angles, x, p0, lb, ub = _problem("nonpositive", model, n, idx)
                for method in (1, 2, 0, 3):
                    res = _single(gpu, method, model, angles, x, p0, lb, ub, want_covar=True)
                    monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
                    exact = _single(gpu, method, model, angles, x, p0, lb, ub, want_covar=True)
                    monkeypatch.delenv("BRDF_HIP_EXACT_POW")
                    what = (regime, n, idx, METHOD[method], res, exact)
                    assert _identical(res, exact), what
                    r, _, ri = _oracle("nonpositive", model, method, n, idx)
                    assert (res.ret >= 0) == (r >= 0), (what, r, ri)
                    assert res.info[6] == ri[6] or (res.info[6] in (1, 2) and ri[6] in (1, 2)), (what, r, ri)
                    other = _single(gpu, method, model, _bad_replaced(angles, model), x, p0, lb, ub, want_covar=True)
                    differs += int(not _identical(res, other))
    assert differs >= 16


@pytest.mark.parametrize("kernel", list(FALLBACK_BATCH))
def test_nonpositive_cosine_batch_fits_take_the_exact_path(gpu, monkeypatch, kernel):
    """in one batch, the fits with a cosine <= 0 equal the same batch under BRDF_HIP_EXACT_POW=1, bit for bit; every other fit
    equals the same batch without the bad fits; the bad fits end as the oracle's do (ret sign, info[6])"""
    env, n = FALLBACK_BATCH[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    per = 1 if n > 4096 else 2
    for model in (0, 1):
        items = []
        for idx in range(per * 4):
            items += [("quantised", idx), ("nonpositive", idx), ("diffuse_only", idx)]
        bad = np.array([f == "nonpositive" for f, _ in items])
        for method in ((1, 2) if n <= 4096 else (1,)):
            p, info, ret = _run_batch(gpu, method, model, n, items)
            monkeypatch.setenv("BRDF_HIP_EXACT_POW", "1")
            pe, ie, re_ = _run_batch(gpu, method, model, n, items)
            monkeypatch.delenv("BRDF_HIP_EXACT_POW")
            what = (kernel, model, METHOD[method])
            assert np.array_equal(p[bad], pe[bad], equal_nan=True) and np.array_equal(info[bad], ie[bad], equal_nan=True), what
            assert np.array_equal(ret[bad], re_[bad]), what
            good = [it for it, b in zip(items, bad) if not b]
            pg, ig, rg = _run_batch(gpu, method, model, n, good)
            assert np.array_equal(p[~bad], pg, equal_nan=True) and np.array_equal(info[~bad], ig, equal_nan=True), what
            assert np.array_equal(ret[~bad], rg), what
            for s in np.flatnonzero(bad):
                family, idx = items[s]
                r, _, ri = L.brdf_fit("orc", method, model, *E.fit_args(family, model, n, idx))
                assert (ret[s] >= 0) == (r >= 0), (what, idx, info[s], ri)
                assert info[s, 6] == ri[6] or (info[s, 6] in (1, 2) and ri[6] in (1, 2)), (what, idx, info[s], ri)


# ---- model values at the edge of the domain against a 50-digit evaluation ---------------------------------------------
COS = (1.0, 1.0 - 2.0 ** -53, 0.5, 1e-2, 1e-4, 1e-8, 2.2250738585072014e-308, 5e-320, 0.0)
EXPONENTS = (0.0, 1.0, 2.5, 100.0, 1000.0)
ALPHAS = (0.01, 0.1, 1.0, 10.0)


def _mp_values(model, angles, p):
    """(value, rel_tol, abs_tol) per sample: the model's expression in 50-digit arithmetic on the exact double inputs (PI is
    the reference's double literal); the tolerance is a few ulp -- for Ward times the condition number of exp, 1 + t2/a2,
    and of the rounded t2 = (1 - c1^2)/c1^2 -- plus, where the result is subnormal, one unit of the smallest subnormal per
    rounding, scaled by what multiplies it afterwards"""
    import mpmath
    mpmath.mp.dps = 50
    PI = mpmath.mpf(synth.PI)
    kd, ks, q = (mpmath.mpf(float(v)) for v in p)
    out = []
    for c0, c1, c2 in zip(*(map(float, angles[k]) for k in range(3))):
        c0, c1, c2 = mpmath.mpf(c0), mpmath.mpf(c1), mpmath.mpf(c2)
        if model in (0, 1):
            c = c2 if model == 0 else c1
            s = mpmath.mpf(1) if q == 0 else (mpmath.mpf(0) if c == 0 else mpmath.power(c, q))
            mult = ((q + 2) / 2 * PI) * ks if model == 0 else ks
            out.append((kd * c0 + mult * s, 8 * U, (2 + 2 * float(mult)) * TINY))
        else:
            a2 = q * q
            k = 1 / (4 * PI * a2)
            rinv = 1 / mpmath.sqrt(c0 * c2)
            t2 = mpmath.inf if c1 == 0 else (1 - c1 * c1) / (c1 * c1)
            arg = t2 / a2
            g = mpmath.mpf(0) if arg == mpmath.inf else mpmath.exp(-arg)
            mult = c0 * ks * k * rinv
            # exp's argument is t2/a2 with t2 = (1 - c1^2)/c1^2 rounded: relative error (2 + 1/(2 t2)) u (1 - c1^2 cancels)
            cond = 1 + float(min(arg, 1e300)) * (1 + (1 / (2 * float(t2)) if t2 > 0 else 0.0))
            out.append((c0 * (kd / PI + ks * (k * g) * rinv), 8 * U * cond, (2 + 2 * float(mult)) * TINY))
    return out


def _check_values(got, ieee, ref, what):
    """got: device values; ieee: the same expression in IEEE double (the oracle's restatement): NaN exactly where it is NaN"""
    worst = 0.0
    for i, (g, e, (v, rel, ab)) in enumerate(zip(got, ieee, ref)):
        if math.isnan(e):
            assert math.isnan(g), (what, i, g, e)
            continue
        v = float(v) if v < 1e308 else math.inf
        if v * (1 + ab / TINY) < 2.0 ** -1075:
            assert g == 0.0, (what, i, g, v)
            continue
        err = abs(g - v)
        assert err <= rel * abs(v) + ab, (what, i, g, v, err, rel * abs(v) + ab)
        if abs(v) >= 2.2250738585072014e-308:
            worst = max(worst, err / abs(v) / rel * 8)  # in u, divided by the condition factor
    return worst


def _value_grid(model):
    """planes [3, N]: Phong / Blinn-Phong the full cosine grid in c0 x powered plane; Ward c0 = c2 over the normal part of
    the grid x cos(N.H) over all of it, and cos(N.H) = 1/sqrt(1 + t2) for t2 = alpha^2 * (700 ... 1100, 1e40) (exp_nonpos'
    argument across its underflow select)"""
    if model in (0, 1):
        c0, cp = np.meshgrid(COS, COS, indexing="ij")
        angles = np.full((3, c0.size), 0.5)
        angles[0] = c0.ravel()
        angles[E.power_plane(model)] = cp.ravel()
        return angles
    normal = [c for c in COS if c >= 1e-8]
    c0, c1 = np.meshgrid(normal, COS, indexing="ij")
    angles = np.stack([c0.ravel(), c1.ravel(), c0.ravel()])
    return angles


def _ward_underflow_planes(alpha):
    args = np.array([700.0, 744.0, 745.2, 746.0, 800.0, 1000.0, 1074.0, 1074.9, 1075.0, 1075.1, 1100.0, 2000.0, 1e5, 1e20, 1e40])
    c1 = 1.0 / np.sqrt(1.0 + args * alpha * alpha)
    return np.stack([np.ones_like(c1), c1, np.ones_like(c1)])


@pytest.mark.parametrize("model", [0, 1, 2])
def test_model_values_at_the_domain_edge_against_mpmath(gpu, model):
    """brdf_hip_model_eval_dev (K1) and BRDFFunc_hip on grazing, unit, subnormal and zero cosines, exponents 0 ... 1000 and
    Ward roughness 0.01 ... 10, kd / ks including 0: within a few ulp of the 50-digit value where it is normal, within the
    subnormal unit where it is subnormal, exactly 0 where it rounds to 0, NaN where the reference expression is NaN"""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, lib
    sets = []
    if model in (0, 1):
        angles = _value_grid(model)
        sets += [(angles, (kd, ks, q)) for kd in (0.0, 0.35) for ks in (0.0, 0.6, 1.0) for q in EXPONENTS]
    else:
        angles = _value_grid(2)
        sets += [(angles, (kd, ks, al)) for kd in (0.0, 0.35) for ks in (0.0, 0.25) for al in ALPHAS]
        sets += [(_ward_underflow_planes(al), (0.0, 1.0, al)) for al in (0.01, 1.0)]
    worst = 0.0
    for angles, p in sets:
        angles = np.ascontiguousarray(angles)
        ieee = L.model_values(model, angles, p)
        ref = _mp_values(model, angles, p)
        dev_vals = brdf_amd.model_eval(model, _t(gpu, angles), p).cpu().numpy()
        worst = max(worst, _check_values(dev_vals, ieee, ref, ("model_eval", model, p)))
        flat = np.ascontiguousarray(angles.reshape(-1))
        hx = np.zeros(angles.shape[1])
        pp = np.array(p, dtype=np.float64)
        lib.BRDFFunc_hip(pp.ctypes.data_as(D), hx.ctypes.data_as(D), 3, angles.shape[1], C.byref(ExtraData(flat.ctypes.data_as(D), model)))
        worst = max(worst, _check_values(hx, ieee, ref, ("BRDFFunc_hip", model, p)))
    print(f"model {model}: worst error of a normal value {worst:.2f} u (unit roundoff) against the 50-digit value")


# ---- the fast path's error at kd = 0 ---------------------------------------------------------------------------------
def _start_objective_bound(model, angles, x, p):
    """(sum of squares at p in 50 digits, the relative bound the fast path implies): each f_i carries a relative error of at
    most (max |n log c| + 2) u (exp(n log c) with log c rounded, plus the model's own roundings); e_i = x_i - f_i then carries
    max |f_i / e_i| times that, e_i^2 twice it; the tree sum adds (log2 n + 4) u"""
    import mpmath
    mpmath.mp.dps = 50
    vals = _mp_values(model, angles, p)
    c = angles[E.power_plane(model)]
    tot = mpmath.mpf(0)
    amp = 0.0
    for (f, _, _), xi in zip(vals, x):
        e = mpmath.mpf(float(xi)) - f
        tot += e * e
        amp = max(amp, float(abs(f) / abs(e)))
    return tot, 2 * amp * (float(np.max(np.abs(p[2] * np.log(c)))) + 2) * U + (math.log2(len(x)) + 4) * U


@pytest.mark.parametrize("model", [0, 1])
def test_fast_path_start_objective_at_kd_zero(gpu, monkeypatch, model):
    """info[0] (||e||^2 at the start point) with kd = 0 -- the model value is the specular term alone, so exp(n log c) carries
    up to |n log c| u of relative error in every value, not 'below one ulp of the model value' -- on data where the
    residual does not cancel (x = 0, x = f/2), n = 24 and 100, on the fast path and under BRDF_HIP_EXACT_POW=1, in each
    regime: single (resident, launch chain), channels, batch (lane, wave, workgroup, eight waves)"""
    torch, brdf_amd, dev = gpu
    report = []
    for q in (24.0, 100.0):
        p0 = (0.0, 0.6, q)
        for n in (16, 64, 1024, 4096):
            angles, _, _ = synth.make_single(model, n)
            f = L.model_values(model, angles, p0)
            for xname, x in (("0", np.zeros(n)), ("f/2", 0.5 * f)):
                want, bound = _start_objective_bound(model, angles, x, p0)
                want = float(want)
                for exact in ("0", "1"):
                    monkeypatch.setenv("BRDF_HIP_EXACT_POW", exact)
                    got = []
                    kw = dict(lb=synth.LB, ub=synth.UB, itmax=2, opts=synth.OPTS)
                    for regime in ("1", "0"):
                        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
                        got.append(("single" + regime, brdf_amd.fit_single(1, model, _t(gpu, angles), _t(gpu, x), p0, **kw).info[0]))
                    monkeypatch.delenv("BRDF_HIP_RESIDENT")
                    ch = brdf_amd.fit_channels(1, model, _t(gpu, angles), _t(gpu, np.stack([x, x])), p0, **kw)
                    got.append(("channels", ch[0].info[0]))
                    S = 4
                    p, info, ret = brdf_amd.fit_batch(1, model, _t(gpu, np.stack([angles] * S)), _t(gpu, np.stack([x] * S)),
                                                      _t(gpu, np.tile(np.array(p0), (S, 1))), **kw)
                    torch.cuda.synchronize()
                    got.append(("batch", info.cpu().numpy()[0, 0]))
                    for name, v in got:
                        ratio = abs(v - want) / (bound * want)
                        report.append(ratio)
                        assert ratio <= 1.0, (q, n, xname, exact, name, v, want, bound)
                    monkeypatch.delenv("BRDF_HIP_EXACT_POW")
    print(f"model {model}: info[0] error at kd = 0, as a fraction of the bound: max {max(report):.3f}, mean {np.mean(report):.3f}")
