"""The capture loop with a validity rule (brdf_hip_fit_capture_masked_dev) on a capture with black, saturated and back-lit
pixels -- the construction of tests/test_gpu_edges.py::test_capture_with_black_saturated_and_diffuse_faces.

  (a) both conditions off: every output has the bytes of fit_capture with its statistics;
  (b) v_min = 1, v_max = 254, cos_min = 0: the stored fits and the count map have the bytes of the same fits made in Python
      (the oracle's cosine planes, the gathered intensities, the rule, compact_samples, fit_batch(..., counts=...)); the counts
      are the rule's; every stored fit of >= 3 samples is finite and non-negative and reaches the oracle's objective over its
      valid samples (the existing capture test's check: <= ref * (1 + 1e-3) + 1e-20, the oracle fitted at n = count);
  (c) with cos_min = 0 no fit meets a non-positive cosine, so none is left to the exact twin or fails on one: no NaN anywhere."""
import numpy as np
import pytest

from tests import oracle_libs as L

pytestmark = pytest.mark.gpu
OPTS = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
MODEL = 1  # Blinn-Phong reads cos(L.N) and cos(N.H)
P0, LB, UB = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


@pytest.fixture(scope="module")
def capture():
    from tests.test_cosines import make_capture
    vertices, faces, nrm, view, leds, pixel_map, images = make_capture()
    H, W = pixel_map.shape
    touched = np.unique(pixel_map[pixel_map > -1])
    black, saturated = set(touched[0::5]), set(touched[1::5])
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f in black:
                images[:, H - 1 - y, x, :] = 0
            elif f in saturated:
                images[:, H - 1 - y, x, :] = 255
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)  # signed: lights behind a face have cos(L.N) <= 0
    assert (ang[touched][:, 0] <= 0).any() and (images == 0).any() and (images == 255).any()
    return vertices, faces, nrm, view, leds, pixel_map, images, ang, touched


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _masked(gpu, capture, **rule):
    torch, brdf_amd, _ = gpu
    vertices, faces, nrm, view, leds, pixel_map, images, _, _ = capture
    out = brdf_amd.fit_capture_masked(MODEL, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, vertices), _dev(gpu, faces), _dev(gpu, nrm),
                                      leds, view, rv_mode=1, opts=OPTS, **rule)
    torch.cuda.synchronize()
    surf, avg, npx, st, cnt = out
    return surf.cpu().numpy(), avg, npx, st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy(), cnt.cpu().numpy()


def test_rule_switched_off_is_the_unmasked_capture(gpu, capture):
    torch, brdf_amd, _ = gpu
    vertices, faces, nrm, view, leds, pixel_map, images, _, touched = capture
    want = brdf_amd.fit_capture(MODEL, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, vertices), _dev(gpu, faces), _dev(gpu, nrm), leds, view,
                                rv_mode=1, opts=OPTS, want_stats=True)
    torch.cuda.synchronize()
    surf, avg, npx, covar, stats, rank, cnt = _masked(gpu, capture)  # v_min = 0, v_max = 255, cos_min < -1
    assert npx == want[2] and avg.tobytes() == want[1].tobytes()
    assert surf.tobytes() == want[0].cpu().numpy().tobytes()
    assert covar.tobytes() == want[3].covar.cpu().numpy().tobytes() and stats.tobytes() == want[3].stats.cpu().numpy().tobytes()
    assert rank.tobytes() == want[3].rank.cpu().numpy().tobytes()
    untouched = np.setdiff1d(np.arange(faces.shape[0]), touched)
    assert np.all(cnt[touched] == images.shape[0]) and np.all(cnt[untouched] == 0)


def test_masked_capture_is_the_ragged_batch_of_its_valid_samples(gpu, capture):
    torch, brdf_amd, _ = gpu
    vertices, faces, nrm, view, leds, pixel_map, images, ang, touched = capture
    H, W = pixel_map.shape
    Lts = images.shape[0]
    # the reference's walk: x outer, y inner; fit q = 3 * pixel + channel; a face's LAST pixel is the one stored
    pixels = [(x, y) for x in range(W) for y in range(H) if pixel_map[y, x] > -1]
    face = np.array([pixel_map[y, x] for x, y in pixels])
    value = np.stack([images[:, H - 1 - y, x, c] for x, y in pixels for c in range(3)]).astype(np.int64)  # [Q, L]
    planes = np.repeat(ang[face], 3, axis=0)  # [Q, 3, L]
    valid = (value >= 1) & (value <= 254) & (planes[:, 0] > 0.0) & (planes[:, 1] > 0.0)
    a_c, x_c, counts = brdf_amd.compact_samples(planes, value / 255.0, valid)
    assert np.array_equal(counts, valid.sum(axis=1)) and counts.min() < 3 <= counts.max() and (counts < Lts).any()
    p0 = np.tile(np.array(P0), (len(counts), 1))
    p, _, ret = brdf_amd.fit_batch(brdf_amd.METHOD_BC_DIF, MODEL, _dev(gpu, a_c), _dev(gpu, x_c), _dev(gpu, p0), lb=LB, ub=UB, itmax=100,
                                   opts=OPTS, counts=_dev(gpu, counts))
    torch.cuda.synchronize()
    p, ret = p.cpu().numpy(), ret.cpu().numpy()
    last = {int(f): s for s, f in enumerate(face)}  # later pixels overwrite earlier ones
    want_surf, want_cnt = np.zeros((faces.shape[0], 3, 3)), np.zeros((faces.shape[0], 3), dtype=np.int32)
    for f, s in last.items():
        want_surf[f], want_cnt[f] = p[3 * s:3 * s + 3], counts[3 * s:3 * s + 3]

    surf, avg, npx, covar, stats, rank, cnt = _masked(gpu, capture, v_min=1, v_max=254, cos_min=0.0)
    assert npx == len(pixels)
    assert cnt.tobytes() == want_cnt.tobytes()  # ... which are the rule evaluated in numpy (asserted above)
    assert surf.tobytes() == want_surf.tobytes()
    assert not np.isnan(surf).any() and np.all(np.isfinite(avg))  # (c): nothing met a cosine <= 0
    judged = refused = 0
    for f, s in last.items():
        for ch in range(3):
            q = 3 * s + ch
            k = int(counts[q])
            if k < 3:  # refused as levmar refuses n < m: p0 stays, rank 0; the count map is how the caller tells
                assert ret[q] == -1 and np.array_equal(surf[f, ch], P0) and rank[f, ch] == 0 and not covar[f, ch].any(), (f, ch, k)
                refused += 1
                continue
            assert np.all(np.isfinite(surf[f, ch])) and np.all(surf[f, ch] >= 0.0), (f, ch, surf[f, ch])
            a_v, x_v = np.ascontiguousarray(a_c[q, :, :k]), np.ascontiguousarray(x_c[q, :k])
            _, p_ref, _ = L.brdf_fit("orc", 1, MODEL, a_v, x_v, P0, 100, OPTS, LB, UB)
            e_got, e_ref = x_v - L.model_values(MODEL, a_v, surf[f, ch]), x_v - L.model_values(MODEL, a_v, p_ref)
            o_got, o_ref = float(e_got @ e_got), float(e_ref @ e_ref)
            print(f"face {f} channel {ch} count {k}: objective {o_got:.6e} oracle {o_ref:.6e}")
            assert o_got <= o_ref * (1 + 1e-3) + 1e-20, (f, ch, k, surf[f, ch], p_ref, o_got, o_ref)
            # the statistics tail's sumsq runs over the valid samples alone.  Its model values are within 4 ulp of the oracle's (the
            # statistics pass's own parity bound), d <= 4 * 2^-52 * max(1, |f|) each, so the two sums of k squares differ by at most
            # 2 d sqrt(k * sum e^2) + k d^2, and by the rounding of either sum (k + 2 operations each)
            d = 4 * 2.0 ** -52 * max(1.0, float(np.max(np.abs(x_v - e_got))))
            tol = 2 * d * np.sqrt(k * o_got) + k * d * d + 2 * (k + 2) * 2.0 ** -53 * o_got
            assert abs(stats[f, ch, 0] - o_got) <= tol, (f, ch, k, stats[f, ch, 0], o_got, tol)
            judged += 1
    assert judged >= 20 and refused >= 3, (judged, refused)
