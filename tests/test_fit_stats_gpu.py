"""Per-fit covariance, standard errors, correlations and R^2 from the separate statistics pass (fit_stats.hip), on the GPU.

Against the reference: the yardstick (tests/stats_yardstick.py) is the compiled reference's dlevmar_fdif_*_jac_approx /
dlevmar_covar / dlevmar_R2 (or their restatements) at the ORACLE's fitted p -- the same bits handed to both sides -- and
every compared fit gets a first-order perturbation bound computed from the reference's own quantities (covar_bound's
docstring has the derivation); there is no free tolerance.  Structure: bit-reproducible, independent of the batch, the
host-pointer entry, the NULL-able outputs, the capture maps."""
import ctypes as C

import numpy as np
import pytest

from brdf_amd import synth
from tests import oracle_libs as L
from tests import stats_yardstick as Y

pytestmark = pytest.mark.gpu
CENTRAL_OPTS = synth.OPTS[:4] + (-1e-6,)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _stats(gpu, method, model, angles, x, p, opts=synth.OPTS):
    torch, brdf_amd, dev = gpu
    st = brdf_amd.fit_stats_batch(method, model, torch.from_numpy(np.ascontiguousarray(angles)).to(dev),
                                  torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(p)).to(dev), opts=opts)
    torch.cuda.synchronize()
    return st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()


# ---- against the reference evaluated at the same p --------------------------------------------------------------
ROWS = {"n16": (16, 4000, 768, True), "n256": (256, 0, 256, False), "n4096": (4096, 0, 64, False)}


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("model", [1, 0, 2])
@pytest.mark.parametrize("row", list(ROWS))
def test_statistics_against_the_reference_at_the_oracles_p(gpu, row, model, method):
    """dlevmar_bc_dif's forward-difference rows and the analytic rows (the sharp check: its bound is ~ cond * 1e-13) on the
    application's own 16-sample 8-bit fits (the fit-by-fit test's inputs) and on the n = 256 / n = 4096 surfels"""
    n, first, count, quantised = ROWS[row]
    angles, x, p, _, _ = Y.oracle_case(model, n, first, count, quantised)
    covar, stats, rank = _stats(gpu, method, model, angles, x, p)
    Y.compare(Y.jac_kind(method, synth.OPTS), model, angles, x, p, covar, stats, rank, label=f"{row} method {method}")


@pytest.mark.parametrize("model", [0, 1, 2])
def test_dif_and_central_differences_at_n256(gpu, model):
    """BRDF_METHOD_DIF (forward rows at the oracle's dlevmar_dif p: the Jacobian AT p, not levmar's secant one) and central
    differences (opts[4] = -1e-6)"""
    angles, x, p, _, ret = Y.oracle_case(model, 256, 0, 256, False, 0)
    covar, stats, rank = _stats(gpu, 0, model, angles, x, p)
    Y.compare(Y.FORWARD, model, angles, x, p, covar, stats, rank, label="n256 dlevmar_dif")
    angles, x, p, _, _ = Y.oracle_case(model, 256, 0, 256, False)
    covar, stats, rank = _stats(gpu, 1, model, angles, x, p, opts=CENTRAL_OPTS)
    Y.compare(Y.CENTRAL, model, angles, x, p, covar, stats, rank, label="n256 central")
    fwd = _stats(gpu, 1, model, angles, x, p)[0]
    assert not _same_bits(fwd, covar)  # (the sign of opts[4] does select another row)


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("n", [17, 257, 4097])
def test_the_seams_of_the_geometry(gpu, n, model, method):
    """the first size of the wavefront, workgroup and multi-workgroup geometries"""
    angles, x, p, _, _ = Y.oracle_case(model, n, 0, 8, False)
    covar, stats, rank = _stats(gpu, method, model, angles, x, p)
    Y.compare(Y.jac_kind(method, synth.OPTS), model, angles, x, p, covar, stats, rank, label=f"seam n={n} method {method}")


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("n,model", [(1_000_000, 2), (262_145, 1)])
def test_multi_workgroup_fits(gpu, n, model, method):
    """one large fit spread over many workgroups (partial rows + fold), alone and three times in one batch"""
    angles, x, p, _, ret = Y.oracle_case(model, n, 0, 1, False, 1, True)
    assert ret[0] >= 0
    c1, s1, r1 = _stats(gpu, method, model, angles, x, p)
    Y.compare(Y.jac_kind(method, synth.OPTS), model, angles, x, p, c1, s1, r1, label=f"multi n={n} S=1 method {method}")
    a3, x3, p3 = (np.ascontiguousarray(np.repeat(v, 3, axis=0)) for v in (angles, x, p))
    c3, s3, r3 = _stats(gpu, method, model, a3, x3, p3)
    Y.compare(Y.jac_kind(method, synth.OPTS), model, a3, x3, p3, c3, s3, r3, label=f"multi n={n} S=3 method {method}")
    for s in range(3):
        assert _same_bits(c3[s], c1[0]) and _same_bits(s3[s], s1[0]) and r3[s] == r1[0]


# ---- structure ------------------------------------------------------------------------------------------------
GEOMETRIES = [16, 100, 1000, 5000]  # rows, wavefront, workgroup, multi-workgroup


def _truth_case(model, n, S):
    angles, x, truth = synth.make_surfels(model, n, first=100, count=S)
    return angles, x, np.ascontiguousarray(truth * 1.01)  # any p will do here: the pass is a pure function of its inputs


@pytest.mark.parametrize("n", GEOMETRIES)
def test_bit_reproducible_and_independent_of_the_batch(gpu, n):
    """two runs give the same bits; fit s alone gives the bits it gives inside a batch of 1,000"""
    model, S = 2, 1000
    angles, x, p = _truth_case(model, n, S)
    for method in (1, 2):
        a = _stats(gpu, method, model, angles, x, p)
        b = _stats(gpu, method, model, angles, x, p)
        assert all(_same_bits(u, v) for u, v in zip(a, b))
        assert np.any(a[2] == 3) and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
        for s in (0, 1, 15, 16, 517, 999):
            one = _stats(gpu, method, model, angles[s:s + 1], x[s:s + 1], p[s:s + 1])
            assert all(_same_bits(u[s:s + 1], v) for u, v in zip(a, one)), (n, method, s)


@pytest.mark.parametrize("n", [16, 300, 4500])
def test_host_pointer_entry_equals_the_device_entry(gpu, n):
    torch, brdf_amd, dev = gpu
    model, S = 1, 37
    angles, x, p = _truth_case(model, n, S)
    want = _stats(gpu, 1, model, angles, x, p)
    st = brdf_amd.fit_stats_batch(1, model, angles, x, p, opts=synth.OPTS)  # numpy in: brdf_hip_fit_stats_batch
    assert _same_bits(st.covar, want[0]) and _same_bits(st.stats, want[1]) and _same_bits(st.rank, want[2])


def test_every_combination_of_the_nullable_outputs(gpu):
    torch, brdf_amd, dev = gpu
    from brdf_amd._lib import lib
    model, n, S = 0, 16, 129
    angles, x, p = _truth_case(model, n, S)
    want = _stats(gpu, 1, model, angles, x, p)
    ta, tx, tp = (torch.from_numpy(v).to(dev) for v in (angles, x, p))
    opts = np.array(synth.OPTS)
    for mask in range(1, 8):
        covar = torch.full((S, 3, 3), -7.0, dtype=torch.float64, device=dev)
        stats = torch.full((S, 8), -7.0, dtype=torch.float64, device=dev)
        rank = torch.full((S,), -7, dtype=torch.int32, device=dev)
        rc = lib.brdf_hip_fit_stats_batch_dev(1, model, ta.data_ptr(), tx.data_ptr(), S, n, tp.data_ptr(), opts.ctypes.data_as(C.POINTER(C.c_double)),
                                              covar.data_ptr() if mask & 1 else None, stats.data_ptr() if mask & 2 else None,
                                              rank.data_ptr() if mask & 4 else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, brdf_amd.last_error()
        torch.cuda.synchronize()
        got = (covar.cpu().numpy(), stats.cpu().numpy(), rank.cpu().numpy())
        for k in range(3):
            if mask & (1 << k):
                assert _same_bits(got[k], want[k]), (mask, k)
            else:
                assert np.all(got[k] == -7), (mask, k)


@pytest.mark.parametrize("n,model", [(16, 1), (256, 2)])
def test_sumsq_of_the_pass_is_the_fits_own(gpu, n, model):
    """after brdf_amd.fit_batch, fit_stats_batch on its p: stats[:, 0] is info[:, 1] to 1e-8 where the fit succeeded"""
    torch, brdf_amd, dev = gpu
    S = 512
    angles, x, _ = synth.make_surfels(model, n, first=0, count=S)
    lb, ub = synth.bounds(model)
    ta, tx = torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev)
    p0 = torch.tensor(synth.P0[model], dtype=torch.float64, device=dev).repeat(S, 1)
    p, info, ret = brdf_amd.fit_batch(1, model, ta, tx, p0, lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    st = brdf_amd.fit_stats_batch(1, model, ta, tx, p, opts=synth.OPTS)
    torch.cuda.synchronize()
    info, ret, sumsq = info.cpu().numpy(), ret.cpu().numpy(), st.stats.cpu().numpy()[:, 0]
    ok = ret >= 0
    assert ok.sum() >= 0.9 * S
    assert np.all(np.abs(sumsq[ok] - info[ok, 1]) <= 1e-8 * info[ok, 1])


# ---- the capture maps (the mesh and images of tests/test_cosines.py's capture test, rebuilt here) -----------------
def make_mesh(nv=500, nf=900, seed=7):
    rng = np.random.default_rng(seed)
    vertices = rng.uniform(-80.0, 80.0, size=(nv, 3)) + np.array([0.0, -80.0, 60.0])
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    e1 = vertices[faces[:, 1]] - vertices[faces[:, 0]]
    e2 = vertices[faces[:, 2]] - vertices[faces[:, 0]]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    view = np.array([310.0, -75.0, 700.0])
    return vertices, faces, nrm, view


def make_capture(H=23, W=31, nf=40, seed=5):
    vertices, faces, nrm, view = make_mesh(nv=200, nf=nf, seed=seed)
    leds = L.led_table()
    c = vertices[faces].sum(axis=1) / 3.0
    flip = ((leds.mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0
    nrm[flip] *= -1.0
    rng = np.random.default_rng(seed)
    pixel_map = rng.integers(-1, nf - 3, size=(H, W)).astype(np.int32)  # -1 = background; the last faces get no pixel
    pixel_map[rng.random((H, W)) < 0.3] = -1
    ang = np.abs(L.cosines(vertices, faces, nrm, leds, view, rv_mode=1))  # [nf,3,16]
    images = np.zeros((16, H, W, 3), dtype=np.uint8)
    truth = np.array(synth.TRUTH[1])
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f < 0:
                continue
            for ch in range(3):
                val = L.model_values(1, ang[f], truth * (0.6 + 0.2 * ch))
                images[:, H - 1 - y, x, ch] = np.clip(np.round(val * 255.0 * 0.5), 0, 255).astype(np.uint8)
    return vertices, faces, nrm, view, leds, pixel_map, images


def test_capture_maps_hold_the_statistics_of_each_faces_last_pixel(gpu):
    torch, brdf_amd, dev = gpu
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture()
    nf = faces.shape[0]
    opts = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    ti, tp = torch.from_numpy(images).to(dev), torch.from_numpy(pixel_map).to(dev)
    plain, avg0, npx0 = brdf_amd.fit_capture(1, ti, tp, tv, tf, tn, leds, view, rv_mode=1, opts=opts)
    sentinel = brdf_amd.FitStats(torch.full((nf, 3, 3, 3), -7.0, dtype=torch.float64, device=dev),
                                 torch.full((nf, 3, 8), -7.0, dtype=torch.float64, device=dev),
                                 torch.full((nf, 3), -7, dtype=torch.int32, device=dev))
    surf, avg, npx, maps = brdf_amd.fit_capture(1, ti, tp, tv, tf, tn, leds, view, rv_mode=1, opts=opts, want_stats=True, surface_stats=sentinel)
    torch.cuda.synchronize()
    # the fit's own outputs are those of brdf_hip_fit_capture_dev, bit for bit
    assert _same_bits(surf.cpu().numpy(), plain.cpu().numpy()) and _same_bits(avg, avg0) and npx == npx0
    covar, stats, rank = maps.covar.cpu().numpy(), maps.stats.cpu().numpy(), maps.rank.cpu().numpy()
    touched = np.unique(pixel_map[pixel_map > -1])
    untouched = np.setdiff1d(np.arange(nf), touched)
    assert untouched.size > 0
    assert np.all(covar[untouched] == -7.0) and np.all(stats[untouched] == -7.0) and np.all(rank[untouched] == -7)
    # by hand: the numpy walk of the pixel map names each face's last pixel; cosines and the image gather give its samples
    H, W = pixel_map.shape
    surf = surf.cpu().numpy()
    ang = brdf_amd.cosines(tv, tf, tn, leds, view, surfels=torch.from_numpy(touched.astype(np.int32)).to(dev), rv_mode=1).cpu().numpy()
    a_all, x_all, p_all = [], [], []
    for k, f in enumerate(touched):
        x_, y_ = max((x, y) for y in range(H) for x in range(W) if pixel_map[y, x] == f)  # x-major walk: the largest (x, y)
        for ch in range(3):
            a_all.append(ang[k])
            x_all.append(images[:, H - 1 - y_, x_, ch] / 255.0)
            p_all.append(surf[f, ch])
    c_hand, s_hand, r_hand = _stats(gpu, 1, 1, np.array(a_all), np.array(x_all), np.array(p_all), opts=opts)
    assert _same_bits(covar[touched].reshape(-1, 3, 3), c_hand)
    assert _same_bits(stats[touched].reshape(-1, 8), s_hand)
    assert _same_bits(rank[touched].reshape(-1), r_hand)
    print(f"capture maps: {int(np.sum(r_hand == 3))} of {r_hand.size} stored fits have a covariance")
    assert np.any(r_hand == 3)  # (the maps are not all "no covariance")
    # the default return value is what it was
    assert len(brdf_amd.fit_capture(1, ti, tp, tv, tf, tn, leds, view, rv_mode=1, opts=opts)) == 3
