"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs; against the committed reference fixtures; and, at BASELINE.json's full size, through size-independent
properties.  Tolerances (SURVEY.md section 8d / BASELINE.json north_star): fitted parameters within 1e-5
relative of the CPU levmar path, ||e||^2 within 1e-8 relative.  Here a fit is compared at its fixed point only: the
GPU sums in a tree, the reference sequentially, and accept/reject decisions near convergence are sensitive to the last
bit, so the trajectories of full fits (iteration / nfev counts) differ.  Trajectories ARE compared where the reference
itself determines them -- the first one, two and three iterations, fits that a loosened stop rule ends early, itmax = 0,
opts = NULL and other tau / delta, in every regime: tests/test_gpu_passes.py holds ret, p and info[0..4] to each case's
own tolerance (tests/pass_problems.py) and info[5..9] (iterations, reason, nfev, njev, nlss) exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from brdf_amd import synth
from tests import oracle_libs as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P_TOL = 1e-5
E_TOL = 1e-8


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _dev_fit(gpu, method, model, angles, x, p0=None, **kw):
    torch, brdf_amd, dev = gpu
    a = torch.from_numpy(np.ascontiguousarray(angles)).to(dev)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    kw.setdefault("lb", synth.LB)
    kw.setdefault("ub", synth.UB)
    kw.setdefault("itmax", synth.ITMAX)
    kw.setdefault("opts", synth.OPTS)
    return brdf_amd.fit_single(method, model, a, xd, synth.P0[model] if p0 is None else p0, **kw)


def _check(res, p_ref, info_ref, p_tol=P_TOL, e_tol=E_TOL):
    assert res.ret >= 0
    assert L.rel_err(res.p, p_ref) <= p_tol, (res.p, p_ref)
    assert abs(res.info[1] - info_ref[1]) <= e_tol * info_ref[1], (res.info[1], info_ref[1])
    assert abs(res.info[0] - info_ref[0]) <= 1e-12 * info_ref[0]


@pytest.mark.parametrize("model", [0, 1, 2])
def test_model_values_match_oracle(gpu, model):
    """K1 (BRDFFunc, brdfdata.cpp:969-989) on the device vs the C restatement: identical operation order,
    only libm-vs-ocml pow/exp may differ -> a few ulp"""
    torch, brdf_amd, dev = gpu
    angles, _, _ = synth.make_single(model, 5000)
    for p in (synth.P0[model], synth.TRUTH[model]):
        hx = brdf_amd.model_eval(model, torch.from_numpy(angles).to(dev), p).cpu().numpy()
        ref = L.model_values(model, angles, p)
        assert np.max(np.abs(hx - ref) / np.abs(ref)) <= 4 * np.finfo(np.float64).eps


@pytest.mark.parametrize("n", [64, 1000, 4096, 10000, 100003])
@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("method", [0, 1])
def test_stream_fit_vs_oracle(gpu, method, model, n):
    angles, x, _ = synth.make_single(model, n)
    _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS,
                                    synth.LB, synth.UB)
    _check(_dev_fit(gpu, method, model, angles, x), p_ref, info_ref)


def test_stream_fit_vs_reference_fixture(gpu):
    fits = json.load(open(os.path.join(HERE, "golden", "brdf_fits.json")))["fits"]
    for f in fits:
        if f["n"] < 64:
            continue  # n=16 is ill-conditioned (SURVEY.md section 6 obs. ii): covered by the objective test below
        angles, x, _ = synth.make_single(f["model"], f["n"])
        res = _dev_fit(gpu, f["method"], f["model"], angles, x)
        _check(res, np.array([float.fromhex(s) for s in f["p"]]), np.array([float.fromhex(s) for s in f["info"]]))


@pytest.mark.parametrize("model", [0, 1, 2])
def test_tiny_fits_reach_the_reference_objective(gpu, model):
    """n = 16 (the application's per-surfel size, brdfdata.h:58): parameters are ill-determined, so parity is
    on the objective: the GPU must do at least as well as the reference up to 1e-6 relative"""
    angles, x, _ = synth.make_single(model, 16)
    for method in (0, 1):
        _, _, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS,
                                    synth.LB, synth.UB)
        res = _dev_fit(gpu, method, model, angles, x)
        assert res.ret >= 0 and res.info[1] <= info_ref[1] * (1 + 1e-6)


def test_drop_in_host_entry_points(gpu):
    """dlevmar_dif / dlevmar_bc_dif exactly as brdfdata.cpp:1058/1119 call them: host arrays, callback pointer,
    struct extraData.  Once with the library's BRDFFunc_hip, once with an application callback that was
    registered (its body is never run: the device model replaces it)."""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, MODEL_FUNC, lib
    model, n = 1, 2000
    angles, x, _ = synth.make_single(model, n)
    for method in (0, 1):
        _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS,
                                        synth.LB, synth.UB)
        _check(brdf_amd.host_dlevmar(method, model, angles, x, synth.P0[model], lb=synth.LB, ub=synth.UB,
                                     itmax=synth.ITMAX, opts=synth.OPTS), p_ref, info_ref)
    calls = []

    @MODEL_FUNC
    def app_brdf_func(p_, hx_, m_, n_, adata_):
        calls.append(1)

    fptr = C.cast(app_brdf_func, C.c_void_p)
    assert lib.brdf_hip_register_model(fptr) == 0
    flat = np.ascontiguousarray(angles.reshape(-1))
    p = np.array(synth.P0[model])
    info = np.zeros(10)
    lb, ub, opts = np.array(synth.LB), np.array(synth.UB), np.array(synth.OPTS)
    ed = ExtraData(flat.ctypes.data_as(D), model)
    rc = lib.dlevmar_bc_dif(fptr, p.ctypes.data_as(D), x.ctypes.data_as(D), 3, n, lb.ctypes.data_as(D),
                            ub.ctypes.data_as(D), None, synth.ITMAX, opts.ctypes.data_as(D), info.ctypes.data_as(D),
                            None, None, C.byref(ed))
    lib.brdf_hip_unregister_model(fptr)
    assert rc >= 0 and not calls
    assert L.rel_err(p, p_ref) <= P_TOL


def test_brdffunc_hip_is_a_working_callback(gpu):
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, lib
    for model in (0, 1, 2):
        angles, _, _ = synth.make_single(model, 333)
        flat = np.ascontiguousarray(angles.reshape(-1))
        hx = np.zeros(333)
        p = np.array(synth.TRUTH[model])
        lib.BRDFFunc_hip(p.ctypes.data_as(D), hx.ctypes.data_as(D), 3, 333, C.byref(ExtraData(flat.ctypes.data_as(D), model)))
        ref = L.model_values(model, angles, p)
        assert np.max(np.abs(hx - ref) / np.abs(ref)) <= 4 * np.finfo(np.float64).eps


def test_covariance_matches_oracle(gpu):
    """covar = ||e||^2/(n-m) (J^T J)^-1 (misc_core.c:564-591), requested like lmdemo's Meyer case"""
    model, n = 1, 3000
    angles, x, _ = synth.make_single(model, n)
    flat = np.ascontiguousarray(angles.reshape(-1))

    class Extra(C.Structure):
        _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]

    p = np.array(synth.P0[model])
    info, covar, opts = np.zeros(10), np.zeros(9), np.array(synth.OPTS)
    fptr = C.cast(L.orc.orc_brdf_func, C.c_void_p)
    L.orc.orc_dlevmar_dif(fptr, L.ptr(p), L.ptr(x), 3, n, synth.ITMAX, L.ptr(opts), L.ptr(info), None, L.ptr(covar),
                          C.byref(Extra(L.ptr(flat), model)))
    res = _dev_fit(gpu, 0, model, angles, x, want_covar=True)
    _check(res, p, info)
    # dlevmar_dif: covar comes from the J^T J levmar holds when it stops, i.e. from the SECANT Jacobian (FD refreshes +
    # Broyden updates along the way), which depends on the path taken; the device sums in trees, so accept/reject decisions
    # near convergence -- and with them the update history -- differ from the CPU's: agreement to 1e-3, by construction
    # of the algorithm, while p and ||e||^2 agree to 1e-8 and better
    assert np.max(np.abs(res.covar.reshape(-1) - covar) / np.abs(covar)) <= 1e-3
    # dlevmar_bc_dif differentiates afresh in every iteration: its covariance is a function of the final point only
    pb, infob, covb = np.array(synth.P0[model]), np.zeros(10), np.zeros(9)
    lb, ub = np.array(synth.LB), np.array(synth.UB)
    L.orc.orc_dlevmar_bc_dif(fptr, L.ptr(pb), L.ptr(x), 3, n, L.ptr(lb), L.ptr(ub), None, synth.ITMAX, L.ptr(opts), L.ptr(infob), None,
                             L.ptr(covb), C.byref(Extra(L.ptr(flat), model)))
    resb = _dev_fit(gpu, 1, model, angles, x, want_covar=True)
    _check(resb, pb, infob)
    assert np.max(np.abs(resb.covar.reshape(-1) - covb) / np.abs(covb)) <= 1e-6


def test_r2_through_the_product_abi(gpu):
    """dlevmar_R2 (levmar.h:376, misc_core.c:616-658): host callback once, the three n-sized sums on the device -- in the
    reference's descending order for small n (bit-exact against the same loops in numpy), by a fixed tree beyond"""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, lib
    for model, n in ((1, 500), (2, 200000)):
        angles, x, _ = synth.make_single(model, n)
        flat = np.ascontiguousarray(angles.reshape(-1))
        p = np.array(synth.TRUTH[model])
        ed = ExtraData(flat.ctypes.data_as(D), model)
        r2 = lib.dlevmar_R2(C.cast(lib.BRDFFunc_hip, C.c_void_p), p.ctypes.data_as(D), x.ctypes.data_as(D), 3, n, C.byref(ed))
        hx = brdf_amd.model_eval(model, torch.from_numpy(angles).to(dev), p).cpu().numpy()
        if n <= 65536:
            sx = 0.0
            for v in x[::-1]:
                sx += v
            xavg = sx / n
            sse = sst = 0.0
            for xi, hi in zip(x[::-1], hx[::-1]):
                sse += (xi - hi) * (xi - hi)
                sst += (xi - xavg) * (xi - xavg)
            assert r2 == 1.0 - sse / sst
        else:
            want = 1.0 - np.sum((x - hx) ** 2) / np.sum((x - x.mean()) ** 2)
            assert abs(r2 - want) <= 1e-12 * abs(want)
        assert 0.9 < r2 < 1.0


def test_runs_are_bitwise_reproducible(gpu):
    """fixed launch geometry + fixed reduction tree, no float atomics"""
    angles, x, _ = synth.make_single(2, 50000)
    for method in (0, 1):
        a = _dev_fit(gpu, method, 2, angles, x)
        b = _dev_fit(gpu, method, 2, angles, x)
        assert a.ret == b.ret and np.array_equal(a.p, b.p) and np.array_equal(a.info, b.info)


def test_argument_errors_on_device_path(gpu):
    torch, brdf_amd, dev = gpu
    angles, x, _ = synth.make_single(1, 100)
    res = _dev_fit(gpu, 1, 1, angles, x, lb=(1.0, 0.0, 0.0), ub=(0.5, 100.0, 100.0))  # lb > ub: lmbc_core.c:451
    assert res.ret == -1 and "lower bound" in brdf_amd.last_error()
    res = _dev_fit(gpu, 1, 1, angles, x, p0=(-3.0, 500.0, 1.0))  # infeasible start: projected, then fitted
    _, p_ref, info_ref = L.brdf_fit("orc", 1, 1, angles, x, (-3.0, 500.0, 1.0), synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
    _check(res, p_ref, info_ref)
    res = _dev_fit(gpu, 0, 1, angles[:, :2], x[:2])  # n < m
    assert res.ret == -1


def test_central_differences_and_unbounded_bc(gpu):
    model, n = 2, 5000
    angles, x, _ = synth.make_single(model, n)
    o = list(synth.OPTS)
    o[4] = -1e-6
    for method in (0, 1):
        _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, o, synth.LB, synth.UB)
        _check(_dev_fit(gpu, method, model, angles, x, opts=o), p_ref, info_ref)
    _, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, None, None)
    _check(_dev_fit(gpu, 1, model, angles, x, lb=None, ub=None), p_ref, info_ref)


@pytest.mark.parametrize("model", [2, 1])
@pytest.mark.parametrize("method", [0, 1])
def test_full_size_properties(gpu, method, model):
    """BASELINE.json configs 2/3 (n = 1e6), too slow for the scalar oracle in a unit test, so: (a) the fit
    recovers the generating parameters to within the noise floor, (b) info[1] equals the residual norm
    recomputed independently (K1 kernel + numpy) at the returned p, (c) refitting from the solution is a fixed
    point, (d) the nfev accounting is self-consistent."""
    torch, brdf_amd, dev = gpu
    n = 1_000_000
    angles, x, truth = synth.make_single(model, n)
    a = torch.from_numpy(angles).to(dev)
    xd = torch.from_numpy(x).to(dev)
    res = brdf_amd.fit_single(method, model, a, xd, synth.P0[model], lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX,
                              opts=synth.OPTS)
    assert res.ret >= 0 and res.info[6] in (1, 2, 6)
    assert L.rel_err(res.p, truth) <= 2e-3
    hx = brdf_amd.model_eval(model, a, res.p).cpu().numpy()
    assert abs(float(np.sum((x - hx) ** 2)) - res.info[1]) <= 1e-10 * res.info[1]
    st = brdf_amd.last_fit_stats()
    # levmar's evaluation count against the sweeps the launch made: one sweep per Jacobian, at most one per evaluation
    # (a chain of rejections shares a sweep, a candidate that is taken brings the next iteration's Jacobian with it)
    if method == 0:
        assert st["passes"] <= 1 + res.info[8] + (res.info[7] - 1 - 3 * res.info[8])
    else:
        assert st["passes"] <= res.info[8] + (res.info[7] - 4 * res.info[8])
    again = brdf_amd.fit_single(method, model, a, xd, res.p, lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX,
                                opts=synth.OPTS)
    assert again.ret >= 0 and L.rel_err(again.p, res.p) <= 1e-6 and again.info[1] <= res.info[1] * (1 + 1e-9)


@pytest.mark.parametrize("model,n", [(2, 1_000_000), (1, 1_000_000), (2, 100003), (0, 5000), (1, 300)])
def test_shared_sweeps_do_not_change_a_bit(gpu, monkeypatch, model, n):
    """Fewer sweeps, same arithmetic.  dlevmar_dif evaluates the trial points of a chain of rejections up to eight to a sweep
    (BRDF_HIP_DIF_CHAIN); dlevmar_bc_dif / bc_der evaluate a candidate by the Jacobian pass the next iteration would open with
    (BRDF_HIP_SPEC_JAC).  Every sum that is judged is formed by the same per-lane order and the same trees as in the plain
    passes, so p, info[] (iterations, nfev, njev, nlss) and the covariance must be bit-identical with and without them --
    in the resident regime and in the launch chain."""
    torch, brdf_amd, dev = gpu
    angles, x, _ = synth.make_single(model, n)
    fewer = 0
    for regime in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", regime)
        for method in (0, 1, 2):
            lb, ub = synth.bounds(model) if method == 2 else (synth.LB, synth.UB)
            got = []
            for on in ("8", "1"):
                monkeypatch.setenv("BRDF_HIP_DIF_CHAIN", on)
                monkeypatch.setenv("BRDF_HIP_SPEC_JAC", "1" if on == "8" else "0")
                r = _dev_fit(gpu, method, model, angles, x, lb=lb, ub=ub, want_covar=True)
                got.append((r, brdf_amd.last_fit_stats()["passes"]))
            (a, pa), (b, pb) = got
            what = (regime, method, [float(v).hex() for v in a.info], [float(v).hex() for v in b.info])
            assert a.ret == b.ret and np.array_equal(a.p, b.p), what
            assert np.array_equal(a.info, b.info), what
            assert np.array_equal(a.covar, b.covar), (regime, method, a.covar, b.covar)
            assert pa <= pb
            fewer += pb - pa
    assert fewer > 0


def _channel_measurements(model, angles, n):
    """three measurement vectors over ONE set of planes: the model at three truths + seeded noise (the three colour channels
    of a capture share phi / thetaDash / theta, brdfdata.cpp:1159-1181)"""
    rng = np.random.default_rng(20240 + model)
    truths = {2: ((0.35, 0.25, 0.15), (0.6, 0.1, 0.3), (0.2, 0.4, 0.08)), 1: ((0.35, 0.6, 24.0), (0.5, 0.3, 8.0), (0.2, 0.8, 40.0)),
              0: ((0.35, 0.06, 24.0), (0.5, 0.03, 8.0), (0.2, 0.08, 40.0))}[model]
    return np.stack([L.model_values(model, angles, t) + 0.01 * (rng.random(n) - 0.5) for t in truths])


@pytest.mark.parametrize("model,n", [(2, 1_000_000), (1, 402_928), (2, 262_145), (0, 100_003), (1, 5_000), (2, 300)])
def test_channels_sharing_a_launch_equal_single_fits_bit_for_bit(gpu, model, n):
    """brdf_hip_fit_channels_dev: three dlevmar_bc_dif (and dlevmar_bc_der) fits over one set of planes in ONE resident
    launch -- three control waves, four sweeping waves serving whichever channel has a request out.  Every channel's p,
    info[] and covariance must equal the single-fit resident path's on that channel alone, bit for bit (same sample ->
    lane -> slot mapping, same accumulation order, same trees; only who executes an operation differs); sizes from a
    one-workgroup fit to the full chip, one with a short last workgroup, and the bunny's 402,928 samples."""
    torch, brdf_amd, dev = gpu
    angles, _, _ = synth.make_single(model, n)
    xs = _channel_measurements(model, angles, n)
    a = torch.from_numpy(np.ascontiguousarray(angles)).to(dev)
    xd = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    for method in (1, 2):
        lb, ub = synth.bounds(model) if method == 2 else (synth.LB, synth.UB)
        kw = dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
        for K in (3, 2):
            together = brdf_amd.fit_channels(method, model, a, xd[:K], synth.P0[model], **kw)
            st = brdf_amd.last_channels_stats(K)
            assert st["shared_launch"], st
            for c in range(K):
                alone = brdf_amd.fit_single(method, model, a, xd[c], synth.P0[model], **kw)
                assert brdf_amd.last_fit_stats()["launches"] == 1
                what = (method, K, c, together[c], alone)
                assert together[c].ret == alone.ret and np.array_equal(together[c].p, alone.p), what
                assert np.array_equal(together[c].info, alone.info), what
                assert np.array_equal(together[c].covar, alone.covar), what
                assert st["channels"][c]["passes"] == brdf_amd.last_fit_stats()["passes"]
    # the entry points that keep per-sample state per channel, and more channels than the shared launch takes, run one fit
    # after the other through the same call: same results
    for method, K in ((0, 3), (3, 2)):
        res = brdf_amd.fit_channels(method, model, a, xd[:K], synth.P0[model], itmax=synth.ITMAX, opts=synth.OPTS)
        assert not brdf_amd.last_channels_stats(K)["shared_launch"]
        for c in range(K):
            alone = brdf_amd.fit_single(method, model, a, xd[c], synth.P0[model], itmax=synth.ITMAX, opts=synth.OPTS)
            assert np.array_equal(res[c].p, alone.p) and np.array_equal(res[c].info, alone.info)
    # four channels (the fourth: channel 1's measurements again, not channel 0's): every channel's statistics are its own
    kw = dict(lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS)
    res = brdf_amd.fit_channels(1, model, a, torch.cat([xd, xd[1:2]]), synth.P0[model], **kw)
    st = brdf_amd.last_channels_stats(4)
    assert not st["shared_launch"]
    for c in range(4):
        alone = brdf_amd.fit_single(1, model, a, xd[c if c < 3 else 1], synth.P0[model], **kw)
        assert np.array_equal(res[c].p, alone.p) and np.array_equal(res[c].info, alone.info), c
        if c == 0:
            assert st["channels"][0]["passes"] == brdf_amd.last_fit_stats()["passes"]


def test_channel_launch_drains_when_a_workgroup_never_arrives(gpu, monkeypatch):
    """every wait of the shared-launch kernel is bounded too: with one workgroup withholding its rows (test hook) the control
    waves give up, the sweeping waves see the workgroup's abort word, the launch drains, and the call fits its channels one after the
    other -- through the single-fit regimes, which are sabotaged as well and end in the launch chain: same answers, no hang"""
    torch, brdf_amd, dev = gpu
    monkeypatch.setenv("BRDF_HIP_RESIDENT_SABOTAGE", "3")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_SPIN_MS", "20")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_BACKOFF", "0")
    model, n = 2, 100000
    lb, ub = synth.bounds(model)  # (Ward's roughness kept off 0: the third channel would otherwise end in levmar's NaN stop, here as in the reference)
    angles, _, _ = synth.make_single(model, n)
    xs = _channel_measurements(model, angles, n)
    a = torch.from_numpy(np.ascontiguousarray(angles)).to(dev)
    xd = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    res = brdf_amd.fit_channels(1, model, a, xd, synth.P0[model], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    assert not brdf_amd.last_channels_stats(3)["shared_launch"]
    for c in range(3):
        _, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, xs[c], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
        _check(res[c], p_ref, info_ref)
    monkeypatch.delenv("BRDF_HIP_RESIDENT_SABOTAGE")
    res = brdf_amd.fit_channels(1, model, a, xd, synth.P0[model], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    assert brdf_amd.last_channels_stats(3)["shared_launch"]  # and the shared launch works again afterwards (tables restarted)
    for c in range(3):
        _, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, xs[c], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
        _check(res[c], p_ref, info_ref)


# ---- batched regime ------------------------------------------------------------------------------------
def _batch(gpu, method, model, angles, x, p0):
    torch, brdf_amd, dev = gpu
    a = torch.from_numpy(np.ascontiguousarray(angles)).to(dev)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pd = torch.from_numpy(np.ascontiguousarray(p0)).to(dev)
    p, info, ret = brdf_amd.fit_batch(method, model, a, xd, pd, lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX,
                                      opts=synth.OPTS)
    torch.cuda.synchronize()
    return p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("n", [16, 64, 200, 256, 700, 1024, 3000, 4096])
@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("method", [0, 1])
def test_batch_fit_vs_oracle(gpu, method, model, n):
    """every geometry of the batched kernels (wave-per-fit 64x1 / 64x4, workgroup-per-fit 256x4 / 512x8),
    ragged n included; per-surfel random truth (BASELINE.json configs 4/5 generator)"""
    S = 24
    angles, x, _ = synth.make_surfels(model, n, first=100, count=S)
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    p, info, ret = _batch(gpu, method, model, angles, x, p0)
    worst = 0.0
    for s in range(S):
        r, p_ref, info_ref = L.brdf_fit("orc", method, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS,
                                        synth.LB, synth.UB)
        if n < 64 or r < 0 or info_ref[6] == 3:
            # ill-conditioned tiny fits / fits the reference itself does not finish in itmax: objective parity
            assert ret[s] >= 0 or r < 0
            if r >= 0 and ret[s] >= 0:
                assert info[s, 1] <= info_ref[1] * (1 + 1e-3) + 1e-30
            continue
        assert ret[s] >= 0
        worst = max(worst, L.rel_err(p[s], p_ref))
        assert abs(info[s, 1] - info_ref[1]) <= E_TOL * info_ref[1]
    assert worst <= P_TOL


@pytest.mark.parametrize("n", [16, 200, 1024, 3000])
@pytest.mark.parametrize("method", [2, 3])
def test_batched_analytic_jacobian_entry_points(gpu, method, n):
    """brdf_hip_fit_batch_dev with BRDF_METHOD_BC_DER / BRDF_METHOD_DER (dlevmar_bc_der / dlevmar_der with the models'
    analytic Jacobian, lmbc_core.c:369-1022 / lm_core.c:64-432) in every batched geometry: lane per fit (n <= 16, bc_der),
    wave per fit, workgroup per fit, eight waves per fit -- against the oracle's same entry points"""
    torch, brdf_amd, dev = gpu
    S = 16
    for model in (1, 2):
        lb, ub = synth.bounds(model)
        angles, x, _ = synth.make_surfels(model, n, first=300, count=S)
        a, xd = torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev)
        p0 = torch.from_numpy(np.tile(np.array(synth.P0[model]), (S, 1))).to(dev)
        p, info, ret = brdf_amd.fit_batch(method, model, a, xd, p0, lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
        torch.cuda.synchronize()
        p, info, ret = p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
        compared = 0
        for s in range(S):
            r, p_ref, info_ref = L.brdf_fit("orc", method, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
            assert (ret[s] >= 0) == (r >= 0)
            if r < 0 or n < 64 or info_ref[6] == 3 or info[s, 6] == 3:  # ill-conditioned / unfinished: objective parity
                if r >= 0 and info[s, 6] != 3:
                    assert info[s, 1] <= info_ref[1] * (1 + 1e-3) + 1e-30
                continue
            compared += 1
            assert L.rel_err(p[s], p_ref) <= P_TOL and abs(info[s, 1] - info_ref[1]) <= E_TOL * info_ref[1], (model, s)
        assert n < 64 or compared >= S // 2


def test_batch_of_fits_beyond_one_workgroup(gpu):
    """n > 4096 samples per fit: brdf_hip_fit_batch_dev runs the fits one after the other, each spread over the chip
    (resident regime), instead of refusing -- every method"""
    torch, brdf_amd, dev = gpu
    model, n, S = 2, 6000, 3
    lb, ub = synth.bounds(model)
    angles, x, _ = synth.make_surfels(model, n, first=900, count=S)
    a, xd = torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev)
    for method in (0, 1, 2, 3):
        p0 = torch.from_numpy(np.tile(np.array(synth.P0[model]), (S, 1))).to(dev)
        p, info, ret = brdf_amd.fit_batch(method, model, a, xd, p0, lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
        torch.cuda.synchronize()
        for s in range(S):
            r, p_ref, info_ref = L.brdf_fit("orc", method, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
            assert r >= 0 and ret[s].item() >= 0
            pg, pr = p[s].cpu().numpy(), p_ref.copy()
            if method in (0, 3):  # unconstrained: Ward depends on alpha^2
                pg[2], pr[2] = abs(pg[2]), abs(pr[2])
            assert L.rel_err(pg, pr) <= P_TOL and abs(info[s, 1].item() - info_ref[1]) <= E_TOL * info_ref[1]


@pytest.mark.parametrize("rows", ["0", "1"])
def test_both_kernels_for_sixteen_sample_fits(gpu, monkeypatch, rows):
    """n <= 16 has two kernels (batch_fit.hip): four fits per wavefront (default for dlevmar_dif) and one wave per fit
    (default for dlevmar_bc_dif); BRDF_HIP_ROWS=0 / 1 forces one of them for both entry points.  Objective parity
    against the oracle for each combination."""
    monkeypatch.setenv("BRDF_HIP_ROWS", rows)
    model, n, S = 1, 16, 40
    angles, x, _ = synth.make_surfels(model, n, first=7, count=S)
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    for method in (0, 1):
        p, info, ret = _batch(gpu, method, model, angles, x, p0)
        for s in range(S):
            r, _, info_ref = L.brdf_fit("orc", method, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS,
                                        synth.LB, synth.UB)
            assert ret[s] >= 0 or r < 0
            if r >= 0 and ret[s] >= 0:
                assert info[s, 1] <= info_ref[1] * (1 + 1e-3) + 1e-30


@pytest.mark.parametrize("exact_pow", ["0", "1"])
@pytest.mark.parametrize("model", [1, 0])
def test_sixteen_sample_fits_fit_by_fit_against_the_oracle(gpu, monkeypatch, model, exact_pow):
    """The application's own workload (brdfdata.cpp:1119: 16 lights, dlevmar_bc_dif, once per pixel and channel) on
    8-bit-quantised noisy measurements (GetIntensities_FromPixel, brdfdata.cpp:945-960: value / 255), through the
    lane-per-fit kernel that is the default at this size -- on the default path (exp(n log c)) and with
    BRDF_HIP_EXACT_POW=1 (the reference's pow expression).  The kernel sums in the reference's own order, so what is
    left between it and the CPU reference is the last bit of pow / exp (ocml vs glibc); these fits are ill-conditioned
    (SURVEY.md section 6 ii: 14 % end at itmax), so a last-bit difference CAN send a fit down another path.  What is
    asserted, fit by fit: both succeed or both fail; >= 97 % of the fits that converge on both sides agree to 1e-5 on
    {kd, ks, n}; no fit ends with an objective more than 30 % above the reference's; >= 99 % are within 1e-6 of it or
    better."""
    monkeypatch.setenv("BRDF_HIP_EXACT_POW", exact_pow)
    n, S = 16, 768
    angles, x, _ = synth.make_surfels(model, n, first=4000, count=S)
    x = np.round(np.clip(x, 0.0, 1.0) * 255.0) / 255.0  # the capture's 8-bit measurements
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    p, info, ret = _batch(gpu, 1, model, angles, x, p0)
    both = close = near = same = 0
    worst = 0.0
    for s in range(S):
        r, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
        assert (ret[s] >= 0) == (r >= 0), (s, ret[s], r)
        if r < 0:
            continue
        excess = (info[s, 1] - info_ref[1]) / max(info_ref[1], 1e-300)
        worst = max(worst, excess)
        near += int(excess <= 1e-6)
        same += int(np.array_equal(info[s, 5:8], info_ref[5:8]))
        if info_ref[6] != 3 and info[s, 6] != 3:
            both += 1
            close += int(L.rel_err(p[s], p_ref) <= P_TOL)
    print(f"n=16 model {model} exact_pow={exact_pow}: {close}/{both} converged fits within 1e-5, {near}/{S} objectives within 1e-6, "
          f"{same}/{S} identical (iterations, reason, nfev), worst objective excess {worst:.3e}")
    assert both >= 0.7 * S and close >= 0.97 * both, (close, both)
    assert near >= 0.99 * S and worst <= 0.3, (near, worst)


def test_batch_results_do_not_depend_on_batch_composition(gpu):
    """fits are independent: fitting surfels [0,64) at once or in two halves gives bit-identical outputs
    (this is what makes sharding across GPUs exact)"""
    model, n, S = 2, 256, 64
    angles, x, _ = synth.make_surfels(model, n, first=0, count=S)
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    for method in (0, 1):
        p, info, ret = _batch(gpu, method, model, angles, x, p0)
        pa, ia, ra = _batch(gpu, method, model, angles[:32], x[:32], p0[:32])
        pb, ib, rb = _batch(gpu, method, model, angles[32:], x[32:], p0[32:])
        assert np.array_equal(p, np.concatenate([pa, pb])) and np.array_equal(info, np.concatenate([ia, ib]))
        assert np.array_equal(ret, np.concatenate([ra, rb]))


def test_batches_on_two_streams_do_not_share_scratch(gpu):
    """two asynchronous batches issued back to back from ONE host thread on two different streams: the per-thread
    scratch (exact-path flags, work-queue counters) of the first must not be reset or refilled by the second while the
    first is still running (batch_fit.hip: BatchScratch orders the second call behind the first with an event).  Both
    batches hold fits that need the exact path (a cosine of zero) and use the queue-fed kernels (n = 16)."""
    torch, brdf_amd, dev = gpu
    model, n, S = 1, 16, 6000
    sets = []
    for first in (0, 50000):
        angles, x, _ = synth.make_surfels(model, n, first=first, count=S)
        angles[::7, 1, 5] = 0.0  # every seventh fit takes the exact path
        sets.append((angles, x))
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    for method in (1, 0):
        alone = [_batch(gpu, method, model, a, x, p0) for a, x in sets]
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        dev_in = [(torch.from_numpy(a).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(p0.copy()).to(dev)) for a, x in sets]
        torch.cuda.synchronize()
        outs = []
        for s, (a, x, p) in zip(streams, dev_in):
            with torch.cuda.stream(s):
                outs.append(brdf_amd.fit_batch(method, model, a, x, p, lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS))
        torch.cuda.synchronize()
        for (p, info, ret), (p_ref, info_ref, ret_ref) in zip(outs, alone):
            assert np.array_equal(p.cpu().numpy(), p_ref) and np.array_equal(info.cpu().numpy(), info_ref)
            assert np.array_equal(ret.cpu().numpy(), ret_ref)


def test_batch_nonpositive_cosine_takes_exact_path(gpu):
    """a cosine <= 0 cannot go through the cached-log path: that fit is re-done with the reference's pow()
    (pow(0, n) = 0 is a perfectly valid sample for the reference)"""
    model, n, S = 1, 128, 8
    angles, x, _ = synth.make_surfels(model, n, first=7, count=S)
    angles[3, 1, 5] = 0.0  # cos(N.H) == 0 for one sample of fit 3
    x[3] = synth.model_value(model, synth.TRUTH[model], angles[3, 0], angles[3, 1], angles[3, 2])
    p0 = np.tile(np.array(synth.P0[model]), (S, 1))
    p, info, ret = _batch(gpu, 1, model, angles, x, p0)
    for s in range(S):
        r, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS,
                                        synth.LB, synth.UB)
        assert ret[s] >= 0 and L.rel_err(p[s], p_ref) <= 1e-4  # fit 3 is noise-free: looser, objective ~ 0
    res = _dev_fit(gpu, 1, model, angles[3], x[3])
    assert res.ret >= 0 and L.rel_err(res.p, synth.TRUTH[model]) <= 1e-4


def test_device_generator_matches_host_generator(gpu):
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import lib
    model, n, S, first = 2, 300, 5, 40
    angles, x, truth = synth.make_surfels(model, n, first=first, count=S)
    t = torch.from_numpy(truth).to(dev)
    a = torch.empty((S, 3, n), dtype=torch.float64, device=dev)
    xd = torch.empty((S, n), dtype=torch.float64, device=dev)
    assert lib.brdf_hip_synth_dev(model, synth.SEED, first, S, n, t.data_ptr(), a.data_ptr(), xd.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), angles)  # planes: pure integer hashing + one fma -> identical bits
    assert np.max(np.abs(xd.cpu().numpy() - x)) <= 1e-15  # measurements: device exp vs numpy exp


def test_resident_and_launch_chain_regimes(gpu, monkeypatch):
    """A single fit that fits the chip (n <= #CUs * 4096) can run in ONE launch with its samples resident in
    registers/LDS (resident_fit.hip, passes separated by an in-launch all-gather of tagged granules) or as the launch
    chain (stream_fit.hip, one launch per pass; BRDF_HIP_RESIDENT=0, and any fit too large for the chip).  Same machines,
    same parity bar, both covered."""
    torch, brdf_amd, dev = gpu
    for env in ("1", "0"):
        monkeypatch.setenv("BRDF_HIP_RESIDENT", env)
        for model, n in ((2, 100000), (1, 5000), (0, 300)):
            angles, x, _ = synth.make_single(model, n)
            for method in (0, 1):
                _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS,
                                                synth.LB, synth.UB)
                _check(_dev_fit(gpu, method, model, angles, x), p_ref, info_ref)
                st = brdf_amd.last_fit_stats()
                assert (st["launches"] == 1) == (env == "1"), st


def test_launch_timing_brackets_the_resident_launch(gpu):
    """brdf_hip_set_launch_timing: the event pair the library records on the fit's stream around its resident launch.  The kernel's
    duration contains the device clock from the first pass to the result (the launch's prologue comes on top) and is not far
    above it; off, or for a fit that runs as a chain of launches, the figure is -1; the fit itself does not change."""
    torch, brdf_amd, dev = gpu
    angles, x, _ = synth.make_single(2, 200_000)
    try:
        brdf_amd.set_launch_timing(False)
        plain = _dev_fit(gpu, 1, 2, angles, x)
        assert brdf_amd.last_fit_stats()["kernel_us"] == -1.0
        brdf_amd.set_launch_timing(True)
        for method in (0, 1):
            _dev_fit(gpu, method, 2, angles, x)  # (first use creates the events)
            timed = _dev_fit(gpu, method, 2, angles, x)
            st = brdf_amd.last_fit_stats()
            assert st["launches"] == 1
            assert 0.0 < st["device_us"] <= st["kernel_us"] <= st["device_us"] + 200.0, st
        assert timed.ret == plain.ret and np.array_equal(timed.p, plain.p) and np.array_equal(timed.info, plain.info)
        xs = _channel_measurements(2, angles, 200_000)
        a = torch.from_numpy(np.ascontiguousarray(angles)).to(dev)
        brdf_amd.fit_channels(1, 2, a, torch.from_numpy(xs).to(dev), synth.P0[2], lb=synth.LB, ub=synth.UB, itmax=synth.ITMAX, opts=synth.OPTS)
        st = brdf_amd.last_channels_stats(3)
        assert st["shared_launch"] and max(c["device_us"] for c in st["channels"]) <= st["kernel_us"] <= max(c["device_us"] for c in st["channels"]) + 200.0, st
    finally:
        brdf_amd.set_launch_timing(False)


@pytest.mark.parametrize("method,n,models", [(0, 262145, (2, 1)), (1, 262145, (2, 1)), (2, 262145, (2,)), (3, 262145, (2,)),
                                             (0, 263000, (2, 1)), (1, 263000, (2,)), (2, 263000, (2,)), (3, 263000, (2,)),
                                             (0, 523009, (2,)), (1, 523009, (2,))])
def test_resident_regime_with_a_short_last_workgroup(gpu, method, n, models):
    """A single fit spread over all CUs deals tiles of ceil(n / #CUs) samples, so the LAST workgroup holds up to #CUs - 1
    samples fewer than the others: its slot nk - 2 can be partly empty and its slot nk - 1 entirely (n = 262,145 on 256
    CUs: tile 1025, nk 3, last workgroup 770 samples).  Lanes without a sample must contribute nothing in EVERY slot (a
    round-2 kernel masked the last slot only and summed sample `begin` up to 255 times for a quarter of the sizes in
    (261120, 2^20]).  All four entry points, Ward and Blinn-Phong, against the oracle at the usual 1e-5 / 1e-8."""
    torch, brdf_amd, dev = gpu
    for model in models:
        lb, ub = synth.bounds(model) if method == 2 else (synth.LB, synth.UB)
        angles, x, _ = synth.make_single(model, n)
        _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
        res = _dev_fit(gpu, method, model, angles, x, lb=lb, ub=ub)
        assert brdf_amd.last_fit_stats()["launches"] == 1  # the resident regime did the work
        _check(res, p_ref, info_ref)


def test_resident_regime_falls_back_when_a_workgroup_never_arrives(gpu, monkeypatch, capfd):
    """every spin of the resident kernel is bounded: with one workgroup withholding its partial row (test hook) the
    launch drains, reports `abort`, and the host redoes the fit with the launch chain -- same answer, no hang"""
    torch, brdf_amd, dev = gpu
    monkeypatch.setenv("BRDF_HIP_RESIDENT", "1")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_SABOTAGE", "3")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_SPIN_MS", "20")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_BACKOFF", "0")  # (no stepping aside after an abort: every fit below tries the resident launch)
    model, n = 2, 100000
    angles, x, _ = synth.make_single(model, n)
    for method in (0, 1):
        _, p_ref, info_ref = L.brdf_fit("orc", method, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
        _check(_dev_fit(gpu, method, model, angles, x), p_ref, info_ref)
        assert brdf_amd.last_fit_stats()["launches"] > 1  # the launch chain did the work
    monkeypatch.delenv("BRDF_HIP_RESIDENT_SABOTAGE")
    _check(_dev_fit(gpu, 0, model, angles, x), *L.brdf_fit("orc", 0, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS,
                                                          synth.LB, synth.UB)[1:])
    assert brdf_amd.last_fit_stats()["launches"] == 1  # and the resident regime works again afterwards (tags restarted)
    # after an aborted launch the resident path steps aside for the next fits (default 8, doubling; here 2) instead of
    # burning its spin budget on every call of a process that shares the GPU
    monkeypatch.setenv("BRDF_HIP_RESIDENT_SABOTAGE", "3")
    monkeypatch.setenv("BRDF_HIP_RESIDENT_BACKOFF", "2")
    assert _dev_fit(gpu, 0, model, angles, x).ret >= 0 and brdf_amd.last_fit_stats()["launches"] > 1  # aborted, chain
    monkeypatch.delenv("BRDF_HIP_RESIDENT_SABOTAGE")
    for expect_chain in (True, True, False):
        assert _dev_fit(gpu, 0, model, angles, x).ret >= 0
        assert (brdf_amd.last_fit_stats()["launches"] > 1) == expect_chain


@pytest.mark.parametrize("model", [0, 1, 2])
def test_bc_der_with_the_analytic_device_jacobian(gpu, model, monkeypatch):
    """dlevmar_bc_der with the built-in models' analytic Jacobian, entirely on the device
    (brdf_hip_fit_dev method 2, and the drop-in dlevmar_bc_der(BRDFFunc_hip, BRDFJac_hip, ...)), in both single-fit
    regimes, against the oracle's dlevmar_bc_der (bit-identical to the compiled reference's on the fixtures)"""
    torch, brdf_amd, dev = gpu
    lb, ub = synth.bounds(model)
    for n in (1000, 100003):
        angles, x, _ = synth.make_single(model, n)
        _, p_ref, info_ref = L.brdf_fit("orc", 2, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, lb, ub)
        for env in ("1", "0"):
            monkeypatch.setenv("BRDF_HIP_RESIDENT", env)
            res = _dev_fit(gpu, 2, model, angles, x, lb=lb, ub=ub)
            _check(res, p_ref, info_ref)
            st = brdf_amd.last_fit_stats()  # at most one pass per Jacobian and one per evaluation (candidates evaluated by the
            assert res.info[8] <= st["jac_passes"] and st["passes"] <= res.info[8] + res.info[7]  # next Jacobian's pass share it)
        res = brdf_amd.host_dlevmar(2, model, angles, x, synth.P0[model], lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
        _check(res, p_ref, info_ref)
    # BRDFJac_hip and dlevmar_chkjac through host pointers
    angles, _, _ = synth.make_single(model, 3000)
    p = np.array(synth.TRUTH[model])

    class Extra(C.Structure):
        _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]

    flat = np.ascontiguousarray(angles.reshape(-1))
    jac_ref = np.zeros(9000)
    L.orc.orc_brdf_jac(L.ptr(p.copy()), L.ptr(jac_ref), 3, 3000, C.byref(Extra(L.ptr(flat), model)))
    jac = brdf_amd.model_jacobian(model, angles, p)
    assert np.max(np.abs(jac.reshape(-1) - jac_ref)) <= 1e-13 * max(1.0, np.max(np.abs(jac_ref)))
    err = brdf_amd.chkjac(model, angles, p)
    assert err.min() > 0.5 and err.mean() > 0.99
    if L.ref is not None:
        err_ref = np.zeros(3000)
        L.ref.ref_brdf_chkjac(model, L.ptr(flat), 3000, L.ptr(p.copy()), L.ptr(err_ref))
        # err is a log10 of the rounding noise of a difference quotient: ocml's pow and glibc's differ in the last bits,
        # so the two err vectors agree in what they say (row correct), not digit for digit
        assert err_ref.min() > 0.5 and np.max(np.abs(err - err_ref)) <= 0.1


@pytest.mark.parametrize("model", [0, 1, 2])
def test_der_with_the_analytic_device_jacobian(gpu, model, monkeypatch):
    """dlevmar_der (lm_core.c:64-432) with BRDFJac_hip: the resident regime runs it on the device (DerMachine); the
    drop-in falls back to the host-callback path when the resident regime is not available"""
    torch, brdf_amd, dev = gpu
    for n in (1000, 100003):
        angles, x, _ = synth.make_single(model, n)
        _, p_ref, info_ref = L.brdf_fit("orc", 3, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS)
        res = _dev_fit(gpu, 3, model, angles, x)
        _check(res, p_ref, info_ref)
        assert brdf_amd.last_fit_stats()["launches"] == 1
        res = brdf_amd.host_dlevmar(3, model, angles, x, synth.P0[model], itmax=synth.ITMAX, opts=synth.OPTS)
        _check(res, p_ref, info_ref)
    monkeypatch.setenv("BRDF_HIP_RESIDENT", "0")  # no resident regime: the launch chain runs dlevmar_der too (DerMachine passes)
    for n in (1000, 100003):
        angles, x, _ = synth.make_single(model, n)
        _, p_ref, info_ref = L.brdf_fit("orc", 3, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS)
        _check(brdf_amd.host_dlevmar(3, model, angles, x, synth.P0[model], itmax=synth.ITMAX, opts=synth.OPTS), p_ref, info_ref)
        res = _dev_fit(gpu, 3, model, angles, x)
        _check(res, p_ref, info_ref)
        st = brdf_amd.last_fit_stats()
        assert st["launches"] > 1 and res.info[8] == st["jac_passes"]  # one launch per pass, one pass per Jacobian


def test_diagonal_scaling_and_nan_input(gpu):
    """dscl (lmbc_core.c:536-540, :555-569) and the stop-reason-7 path (non-finite function values ->
    LM_ERROR, lm_core.c:562, :749; lmbc_core.c:534)"""
    torch, brdf_amd, dev = gpu
    model, n = 1, 4000
    angles, x, _ = synth.make_single(model, n)
    dscl = (1.0, 2.0, 50.0)
    flat = np.ascontiguousarray(angles.reshape(-1))

    class Extra(C.Structure):
        _fields_ = [("angles", L.D), ("modelInfo", C.c_int)]

    p = np.array(synth.P0[model])
    info, opts = np.zeros(10), np.array(synth.OPTS)
    lb, ub, ds = np.array(synth.LB), np.array(synth.UB), np.array(dscl)
    fptr = C.cast(L.orc.orc_brdf_func, C.c_void_p)
    r = L.orc.orc_dlevmar_bc_dif(fptr, L.ptr(p), L.ptr(x), 3, n, L.ptr(lb), L.ptr(ub), L.ptr(ds), synth.ITMAX, L.ptr(opts),
                                 L.ptr(info), None, None, C.byref(Extra(L.ptr(flat), model)))
    res = _dev_fit(gpu, 1, model, angles, x, dscl=dscl)
    assert r >= 0
    _check(res, p, info, p_tol=1e-4)
    xb = x.copy()
    xb[17] = np.nan
    for method in (0, 1):
        res = _dev_fit(gpu, method, model, angles, xb)
        assert res.ret == -1 and res.info[6] == 7


# ---- arbitrary host callbacks: the reference's own known answers through the product ABI -------------------
def _product_kat(lib, pr):
    """run one lmdemo problem through libbrdf_hip's dlevmar_dif / dlevmar_bc_dif with the problem function taken,
    by address, from the compiled reference object (a plain host callback the library knows nothing about)"""
    from tests.kat_problems import OPTS
    fp = C.cast(getattr(L.ref, pr["f"]), C.c_void_p)
    p = L.f64(pr["p"]).copy()
    x = L.f64(pr["x"])
    m, n = p.size, x.size
    info, opts = np.zeros(10), L.f64(OPTS)
    covar = np.zeros(m * m) if pr.get("covar") else None
    if pr["kind"] == "dif":
        r = lib.dlevmar_dif(fp, L.ptr(p), L.ptr(x), m, n, pr["itmax"], L.ptr(opts), L.ptr(info), None, L.ptr(covar), None)
    elif pr["kind"] == "der":
        jp = C.cast(getattr(L.ref, pr["j"]), C.c_void_p)
        r = lib.dlevmar_der(fp, jp, L.ptr(p), L.ptr(x), m, n, pr["itmax"], L.ptr(opts), L.ptr(info), None, L.ptr(covar), None)
    elif pr["kind"] == "bc_der":
        lb, ub = L.f64(pr["lb"]), L.f64(pr["ub"])
        jp = C.cast(getattr(L.ref, pr["j"]), C.c_void_p)
        r = lib.dlevmar_bc_der(fp, jp, L.ptr(p), L.ptr(x), m, n, L.ptr(lb), L.ptr(ub), None, pr["itmax"], L.ptr(opts),
                               L.ptr(info), None, L.ptr(covar), None)
    else:
        lb, ub = L.f64(pr["lb"]), L.f64(pr["ub"])
        r = lib.dlevmar_bc_dif(fp, L.ptr(p), L.ptr(x), m, n, L.ptr(lb), L.ptr(ub), None, pr["itmax"], L.ptr(opts),
                               L.ptr(info), None, L.ptr(covar), None)
    return r, p, info, covar


@pytest.mark.skipif(L.ref is None, reason="lmdemo problem functions live in oracle/_ref")
def test_lmdemo_known_answers_through_the_product_abi(gpu, capfd):
    """generic_fit.hip: host callback evaluated on the host, residuals / FD Jacobian fill / J^T J / J^T e / Broyden on
    the device in the reference's summation order (small problems) -> the reference's known answers replay BIT FOR
    BIT through dlevmar_dif / dlevmar_bc_der / dlevmar_bc_dif of libbrdf_hip.so: Wood, Meyer (with covariance), and
    the five box-constrained problems both with their analytic Jacobians (the rows of SURVEY.md section 4) and
    through the finite-difference entry point."""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import lib
    from tests.kat_problems import PROBLEMS
    gold = json.load(open(os.path.join(HERE, "golden", "lmdemo_kat.json")))["kats"]
    ran = 0
    for kat in gold:
        if kat["entry"] not in ("der", "dif", "bc_dif", "bc_der"):
            continue
        r, p, info, covar = _product_kat(lib, PROBLEMS[kat["problem"]])
        hexs = lambda v: np.array([float.fromhex(s) for s in v])  # noqa: E731
        assert r == kat["ret"], (kat["name"], r, kat["ret"])
        assert np.array_equal(p, hexs(kat["p"])), (kat["name"], p)
        assert np.array_equal(info, hexs(kat["info"])), (kat["name"], info)
        if kat["covar"] is not None:
            assert np.array_equal(covar, hexs(kat["covar"]))
        ran += 1
    assert ran == 17  # all twelve no-LAPACK lmdemo problems + the five bc ones through bc_dif
    capfd.readouterr()


@pytest.mark.skipif(L.ref is None, reason="the wide problem's callbacks live in oracle/_ref")
@pytest.mark.parametrize("m", [9, 12, 16])
def test_wide_problems_through_the_product_abi(gpu, m):
    """levmar takes any m (lm_core.c:528-548 sizes its scratch by m); the host-callback path instantiates its machines for
    m = 1..16.  A 12-or-so-parameter Chebyshev fit with a sine in it (oracle/ref_shim.c: wide_cheb, ours) through all four
    entry points of the product ABI against the compiled reference: n m <= 65536, so the sums are formed in the reference's
    order and p, info[] and the covariance must be the reference's bit for bit."""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import lib
    from tests.kat_problems import run_problem
    n = 64
    rng = np.random.default_rng(m)
    truth = rng.uniform(-1.0, 1.0, m)
    x = np.zeros(n)
    L.ref.wide_cheb(L.ptr(truth.copy()), L.ptr(x), m, n, None)
    x += 1e-3 * (rng.random(n) - 0.5)
    base = dict(f="wide_cheb", j="wide_cheb_jac", p=[0.1] * m, x=list(x), itmax=200, covar=True)
    for kind in ("dif", "der", "bc_dif", "bc_der"):
        pr = dict(base, kind=kind, lb=[-0.75] * m, ub=[0.75] * m)
        want = run_problem(L.ref, "", pr)
        got = run_problem(lib, "", pr, ref_lib=L.ref)
        assert got[0] == want[0] >= 0, (kind, brdf_amd.last_error())
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (kind, got[1], want[1])
        if want[3] is not None and kind in ("dif", "der"):
            assert np.array_equal(got[3], want[3])
    p = np.array([0.1] * 17)
    info = np.zeros(10)
    assert lib.dlevmar_dif(C.cast(L.ref.wide_cheb, C.c_void_p), L.ptr(p), L.ptr(np.zeros(40)), 17, 40, 10, None, L.ptr(info), None, None, None) == -1
    assert "m <= 16" in brdf_amd.last_error() or "<= 16" in brdf_amd.last_error()


@pytest.mark.skipif(L.ref is None, reason="the float problem functions live in oracle/_ref")
def test_single_precision_twins_replay_the_reference(gpu, capfd):
    """slevmar_dif / _der / _bc_dif / _bc_der (levmar.h:208-231): the machines and the
    n-sized kernels instantiated with Real = float, as the reference instantiates its *_core.c files (lm.c:43-63).  The
    fixtures are what the compiled reference's own slevmar_* returns on nine float problems (tests/golden/gen_golden.py);
    with the sums formed in the reference's order (n*m <= 65536) the product replays them BIT FOR BIT -- solution,
    info[] (iteration / evaluation / Jacobian / solve counts included) and covariance.  Also the float utilities."""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import F, lib
    from tests.kat_problems import SPROBLEMS, run_sproblem
    gold = {k["name"]: k for k in json.load(open(os.path.join(HERE, "golden", "slevmar_kat.json")))["kats"]}
    assert set(gold) == set(SPROBLEMS)
    f32 = lambda v: np.array([float.fromhex(s) for s in v], dtype=np.float32)  # noqa: E731
    for name, pr in SPROBLEMS.items():
        r, p, info, covar = run_sproblem(lib, pr, ref_lib=L.ref)
        g = gold[name]
        assert r == g["ret"], (name, r, g["ret"])
        assert np.array_equal(p, f32(g["p"])), (name, p, f32(g["p"]))
        assert np.array_equal(info, f32(g["info"])), (name, info, f32(g["info"]))
        if g["covar"] is not None:
            assert np.array_equal(covar, f32(g["covar"]), equal_nan=True), (name, covar)
    capfd.readouterr()
    # utilities: stddev / corcoef / R2 / chkjac / the LU solver, against the reference's own float versions
    cov = np.array([4.0, 1.0, 1.0, 9.0], dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(F)  # noqa: E731
    for fn in ("slevmar_stddev", "slevmar_corcoef", "slevmar_R2"):
        getattr(L.ref, fn).restype = C.c_float
    assert lib.slevmar_stddev(fp(cov), 2, 1) == L.ref.slevmar_stddev(fp(cov), 2, 1) == 3.0
    assert lib.slevmar_corcoef(fp(cov), 2, 0, 1) == L.ref.slevmar_corcoef(fp(cov), 2, 0, 1)
    pm = np.array([2.5, 6.2, 3.5], dtype=np.float32)
    from tests.kat_problems import MEYER_X
    xm = np.array(MEYER_X, dtype=np.float32)
    fm = C.cast(L.ref.sp_meyer, C.c_void_p)
    assert lib.slevmar_R2(fm, fp(pm), fp(xm), 3, 16, None) == L.ref.slevmar_R2(fm, fp(pm.copy()), fp(xm), 3, 16, None)
    ph = np.array([-1.0, 0.5, 0.25], dtype=np.float32)
    e1, e2 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    fh, jh = C.cast(L.ref.sp_helval, C.c_void_p), C.cast(L.ref.sp_helval_jac, C.c_void_p)
    lib.slevmar_chkjac(fh, jh, fp(ph), 3, 3, None, fp(e1))
    L.ref.slevmar_chkjac(fh, jh, fp(ph.copy()), 3, 3, None, fp(e2))
    assert np.all(e1 > 0.5) and np.max(np.abs(e1 - e2)) <= 0.05  # (log10 of float rounding noise: device log10f vs glibc's)
    A = np.array([4, -2, 1, 3, 6, -4, 2, 1, 8], dtype=np.float32)
    B = np.array([12, -25, 32], dtype=np.float32)
    x1, x2 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    assert lib.sAx_eq_b_LU_noLapack(fp(A.copy()), fp(B.copy()), fp(x1), 3) == 1
    assert L.ref.sAx_eq_b_LU_noLapack(fp(A.copy()), fp(B.copy()), fp(x2), 3) == 1
    assert np.array_equal(x1, x2)


def test_unregistered_brdf_callback_takes_the_generic_path(gpu):
    """an application callback that was NOT registered still works (it is called on the host); large n uses the
    deterministic tree, so parity is to tolerance"""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, MODEL_FUNC, lib
    model, n = 1, 30000  # n*m > 65536: tree sums
    angles, x, _ = synth.make_single(model, n)
    flat = np.ascontiguousarray(angles.reshape(-1))
    calls = []

    @MODEL_FUNC
    def app_func(p_, hx_, m_, n_, adata_):
        calls.append(1)
        pp = np.ctypeslib.as_array(p_, shape=(3,))
        out = np.ctypeslib.as_array(hx_, shape=(n_,))
        out[:] = pp[0] * angles[0] + pp[1] * np.power(angles[1], pp[2])

    p = np.array(synth.P0[model])
    info = np.zeros(10)
    lb, ub, opts = np.array(synth.LB), np.array(synth.UB), np.array(synth.OPTS)
    ed = ExtraData(flat.ctypes.data_as(D), model)
    rc = lib.dlevmar_bc_dif(C.cast(app_func, C.c_void_p), p.ctypes.data_as(D), x.ctypes.data_as(D), 3, n,
                            lb.ctypes.data_as(D), ub.ctypes.data_as(D), None, synth.ITMAX, opts.ctypes.data_as(D),
                            info.ctypes.data_as(D), None, None, C.byref(ed))
    _, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
    assert rc >= 0 and len(calls) == info[7]
    assert L.rel_err(p, p_ref) <= 1e-6 and abs(info[1] - info_ref[1]) <= 1e-9 * info_ref[1]


def test_host_batch_entry_point_and_null_measurements(gpu):
    """brdf_hip_fit_batch (host pointers: the CalcBRDFEquation loop as one call, brdfdata.cpp:1195-1220) and
    x == NULL ("a zero vector", lm_core.c:441)"""
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import D, ExtraData, lib
    model, n, S = 1, 16, 40
    angles, x, _ = synth.make_surfels(model, n, first=500, count=S)
    p = np.tile(np.array(synth.P0[model]), (S, 1))
    info = np.zeros((S, 10))
    ret = np.zeros(S, dtype=np.int32)
    lb, ub, opts = np.array(synth.LB), np.array(synth.UB), np.array(synth.OPTS)
    bad = lib.brdf_hip_fit_batch(1, model, angles.ctypes.data_as(D), x.ctypes.data_as(D), S, n, p.ctypes.data_as(D),
                                 lb.ctypes.data_as(D), ub.ctypes.data_as(D), synth.ITMAX, opts.ctypes.data_as(D),
                                 info.ctypes.data_as(D), ret.ctypes.data_as(C.POINTER(C.c_int)))
    assert bad == int((ret < 0).sum())
    for s in range(S):
        r, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles[s], x[s], synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
        if r >= 0 and ret[s] >= 0:
            assert info[s, 1] <= info_ref[1] * (1 + 1e-3) + 1e-30
    # zero measurement vector: the fit drives the model to zero (kd = ks = 0 is feasible)
    flat = np.ascontiguousarray(angles[0].reshape(-1))
    pz = np.array(synth.P0[model])
    infoz = np.zeros(10)
    rc = lib.dlevmar_bc_dif(C.cast(lib.BRDFFunc_hip, C.c_void_p), pz.ctypes.data_as(D), None, 3, n, lb.ctypes.data_as(D),
                            ub.ctypes.data_as(D), None, synth.ITMAX, opts.ctypes.data_as(D), infoz.ctypes.data_as(D), None,
                            None, C.byref(ExtraData(flat.ctypes.data_as(D), model)))
    assert rc >= 0 and infoz[1] <= 1e-12 * infoz[0]


def test_compiled_cpp_call_site_links_and_fits(gpu, tmp_path):
    """tests/cpp/dropin_solve_equation.cpp: the reference's SolveEquation call site (its own struct extraData, its
    own BRDFFunc, dlevmar_bc_dif with NULL work/covar) compiled by g++ and LINKED against libbrdf_hip.so in place
    of liblevmar.a, plus the one registration line.  The application's callback must never run.  The binary holds the
    reference's text, so it is built into oracle/_ref/ (by __graft_entry__.build() where the reference exists)."""
    import subprocess
    exe = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "dropin_solve_equation")
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "cpp"), "dropin_solve_equation"], check=True)
    for model, n in ((1, 16), (1, 5000), (0, 2000)):
        angles, x, _ = synth.make_single(model, n)
        path = tmp_path / f"s{model}_{n}.bin"
        np.concatenate([angles.reshape(-1), x]).tofile(path)
        out = subprocess.run([exe, str(model), str(n), str(path)], capture_output=True, text=True, check=True).stdout
        tok = next(l for l in out.splitlines() if l.startswith("RESULT")).split()
        ret, calls = int(tok[1]), int(tok[2])
        p = np.array([float.fromhex(t) for t in tok[3:6]])
        info = np.array([float.fromhex(t) for t in tok[6:16]])
        r, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, x, synth.P0[model], synth.ITMAX, synth.OPTS, synth.LB, synth.UB)
        assert ret >= 0 and calls == 0
        if n >= 64:
            assert L.rel_err(p, p_ref) <= P_TOL and abs(info[1] - info_ref[1]) <= E_TOL * info_ref[1]
        else:
            assert info[1] <= info_ref[1] * (1 + 1e-6)


@pytest.mark.parametrize("n", [16 * 2500, 16 * 25183])
def test_single_brdf_call_site_configuration(gpu, n):
    """CBRDFdata::SolveEquation_SingleBRDF (brdfdata.cpp:991-1075): ONE fit over all faces x 16 lights with
    p0 = {0,0,0}, itmax = 2000 and opts = {1e-3, 1e-15, 1e-10, 1e-50, delta = 1} (brdfdata.cpp:1002, :1048, :1055-1056),
    bounds [0,100]^3, through dlevmar_bc_dif.  16 x 25,183 = 402,928 is the bunny mesh's face count."""
    model = 1
    angles, x, _ = synth.make_single(model, n)
    p0 = (0.0, 0.0, 0.0)
    opts = (1e-3, 1e-15, 1e-10, 1e-50, 1.0)
    r, p_ref, info_ref = L.brdf_fit("orc", 1, model, angles, x, p0, 2000, opts, synth.LB, synth.UB)
    res = _dev_fit(gpu, 1, model, angles, x, p0=p0, itmax=2000, opts=opts)
    assert r >= 0 and res.ret >= 0
    assert L.rel_err(res.p, p_ref) <= P_TOL, (res.p, p_ref)
    assert abs(res.info[1] - info_ref[1]) <= E_TOL * info_ref[1]


def test_bench_on_two_ranks_reproduces_one_rank_bit_for_bit(gpu):
    """`python bench.py --gpus 2 --workload c5` with real fits: two ranks (here both on this box's one GPU, collectives
    over gloo -- BRDF_BENCH_DEVICE / BRDF_BENCH_BACKEND, the rehearsal switches) shard the surfels, fit their halves with
    the HIP kernels and gather: the digest of all fitted rows equals the one-rank run's.  (RCCL itself needs one GPU per
    rank; the driver's multi-GPU run is the first to use it.)"""
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, BRDF_BENCH_BACKEND="gloo", BRDF_BENCH_DEVICE="0")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    lines = {}
    for gpus in (1, 2):
        for entry in ("dif", "bc_dif"):
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--workload", "c5", "--entry", entry,
                                  "--surfels", "20001", "--steps", "1", "--warmup", "1", "--no-cpu"], capture_output=True, text=True,
                                 env=env, cwd=root, timeout=600)
            assert out.returncode == 0, out.stderr[-2000:]
            js = [l for l in out.stdout.splitlines() if l.startswith("{")]
            assert len(js) == 1, out.stdout
            lines[gpus, entry] = json.loads(js[0])
    for entry in ("dif", "bc_dif"):
        one, two = lines[1, entry], lines[2, entry]
        assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and one["config"]["failed_fits"] == two["config"]["failed_fits"] == 0
        assert one["result_sha256"] == two["result_sha256"] and one["config"]["mean_nfev"] == two["config"]["mean_nfev"]
