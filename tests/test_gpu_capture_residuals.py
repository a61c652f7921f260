"""The carried faces' residuals against M materials (brdf_hip_capture_face_residuals_dev).  Captures: tests/capture_problems.py.

  (1) M = 1 with the single_brdf of fit_capture_single_faces has that call's face_sumsq and face_count BYTES: every model, L = 5, 16, 64;
  (2) M = 2 and M = one more than the kernel's material group: column m has the M = 1 call's bytes for material m, also with the
      materials permuted; two calls give the same bytes; untouched faces keep a sentinel;
  (3) chunk and channel edges: faces of exactly 1024 and 1025 valid samples, a face without a valid sample in one channel only, and
      big_capture(), the scans' multi-block path with a face of five chunks;
  (4) a Ward material with alpha = 0 leaves sums that are not finite and does not disturb its neighbours' bytes;
  (5) against NumPy sums over the oracle's model values on the exact path, to the statistics yardstick's E_TOL."""
import functools

import numpy as np
import pytest

from tests import capture_problems as P
from tests import oracle_libs as L
from tests import stats_yardstick as Y
from tests import test_gpu_capture_single_faces as S

pytestmark = pytest.mark.gpu
SENTINEL = S.SENTINEL
GROUP = 4  # capture_face_major.h: kMaterialGroup


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _residuals(gpu, cap, model, materials, images=None, pixel_map=None, **rule):
    """capture_face_residuals into sentinel maps: (face_sumsq [nf,M,3], face_count [nf,3], face_pixels [nf]) on the host"""
    torch, brdf_amd, dev = gpu
    nf, M = cap["nf"], len(materials)
    out = brdf_amd.FaceResiduals(torch.full((nf, M, 3), float(SENTINEL), dtype=torch.float64, device=dev),
                                 torch.full((nf, 3), SENTINEL, dtype=torch.int32, device=dev), torch.full((nf,), SENTINEL, dtype=torch.int32, device=dev), 0, 0)
    r = brdf_amd.capture_face_residuals(model, S._dev(gpu, cap["images"] if images is None else images),
                                        S._dev(gpu, cap["pixel_map"] if pixel_map is None else pixel_map), S._dev(gpu, cap["vertices"]),
                                        S._dev(gpu, cap["faces"]), S._dev(gpu, cap["nrm"]), cap["leds"], cap["view"], np.asarray(materials, dtype=np.float64),
                                        rv_mode=1, validate=False, out=out, **rule)
    torch.cuda.synchronize()
    return r.face_sumsq.cpu().numpy(), r.face_count.cpu().numpy(), r.face_pixels.cpu().numpy()


def _materials(model, single):
    """GROUP + 1 materials: the single fit's, then others of the model's kind, every channel its own"""
    rng = np.random.default_rng(7 + model)
    from brdf_amd import synth
    truth = np.array(synth.TRUTH[model])
    return np.stack([single] + [truth[None, :] * rng.uniform(0.5, 1.5, size=(3, 3)) for _ in range(GROUP)])


@functools.lru_cache(maxsize=None)
def _single_and_one(gpu, model, lights):
    cap = P.rule_capture(model, lights=lights)
    single = S._single(gpu, cap, model, **P.RULE)
    return cap, single, _residuals(gpu, cap, model, single["single_brdf"][None], **P.RULE)


@pytest.mark.parametrize("lights", [5, 16, 64])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_one_material_has_the_single_capture_bytes(gpu, model, lights):
    cap, single, (sumsq, count, pixels) = _single_and_one(gpu, model, lights)
    assert sumsq[:, 0, :].tobytes() == single["face_sumsq"].tobytes()
    assert count.tobytes() == single["face_count"].tobytes() and pixels.tobytes() == single["face_pixels"].tobytes()
    carried = np.flatnonzero(pixels > 0)
    assert carried.size == 37 and np.all(sumsq[np.setdiff1d(np.arange(cap["nf"]), carried)] == SENTINEL) and count[carried].sum() > 0


@pytest.mark.parametrize("model", [0, 1, 2])
def test_a_column_depends_on_its_material_only(gpu, model):
    cap, single, _ = _single_and_one(gpu, model, 16)
    mats = _materials(model, single["single_brdf"])
    alone = [_residuals(gpu, cap, model, mats[m:m + 1], **P.RULE)[0][:, 0, :] for m in range(GROUP + 1)]
    assert alone[0].tobytes() == single["face_sumsq"].tobytes()
    perm = np.array([3, 0, 4, 2, 1])
    for order in (np.arange(2), np.arange(GROUP + 1), perm, np.array([4, 4, 1])):
        sumsq, count, _ = _residuals(gpu, cap, model, mats[order], **P.RULE)
        assert count.tobytes() == single["face_count"].tobytes()
        for j, m in enumerate(order):
            assert sumsq[:, j, :].tobytes() == alone[m].tobytes(), (list(order), j, m)
    again = _residuals(gpu, cap, model, mats[perm], **P.RULE)
    for a, b in zip(again, _residuals(gpu, cap, model, mats[perm], **P.RULE)):
        assert a.tobytes() == b.tobytes()


def _numpy_check(model, twin, materials, sumsq, count):
    """every carried face and material against the NumPy sum over the oracle's model values: the project's bound on a sum of squares"""
    worst = 0.0
    for c in range(3):
        ang, x, fo = twin.channels[c]
        assert np.array_equal(count[twin.faces, c], np.diff(fo))
        for m in range(len(materials)):
            with np.errstate(all="ignore"):
                e = x - L.model_values(model, ang, materials[m][c]) if x.size else np.zeros(0)
            for r, f in enumerate(twin.faces):
                seg = e[int(fo[r]):int(fo[r + 1])]
                mine = float(sumsq[f, m, c])
                if seg.size == 0:
                    assert mine == 0.0, (f, m, c, mine)
                    continue
                with np.errstate(all="ignore"):
                    ref = float(seg @ seg)
                if not np.isfinite(ref):
                    assert not np.isfinite(mine), (f, m, c, mine, ref)
                    continue
                worst = max(worst, abs(mine - ref) / (Y.E_TOL * ref) if ref > 0 else (0.0 if mine == 0.0 else np.inf))
                assert abs(mine - ref) <= Y.E_TOL * ref, (f, m, c, seg.size, mine, ref)
    print(f"model {model}: worst face residual error / (E_TOL * sum) = {worst:.3e}")


@pytest.mark.parametrize("model", [0, 1, 2])
def test_against_numpy_on_the_exact_path(gpu, model):
    import brdf_amd
    cap, single, _ = _single_and_one(gpu, model, 16)
    mats = _materials(model, single["single_brdf"])
    sumsq, count, _ = _residuals(gpu, cap, model, mats, **P.RULE)
    twin = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    _numpy_check(model, twin, mats, sumsq, count)


@functools.lru_cache(maxsize=None)
def edge_capture():
    """rule_capture(1)'s mesh under a map of its own: three faces whose planes are positive at every light carry 64, 65 and 5 pixels;
    values drawn in [1, 254], then zeros -- which RULE refuses -- leave face A 1024 samples in every channel, face B 1025, 1040 and
    1024, face C none in channel 2 only"""
    cap = dict(P.rule_capture(1))
    rng = np.random.default_rng(3)
    full = np.flatnonzero((cap["ang"] > 0).all(axis=(1, 2)))
    A, B, Cf = (int(f) for f in full[:3])
    others = np.setdiff1d(np.arange(cap["nf"]), [A, B, Cf])
    H, W = cap["pixel_map"].shape
    flat = np.full(H * W, -1, dtype=np.int32)
    place = rng.permutation(H * W)
    flat[place[:64]], flat[place[64:129]], flat[place[129:134]] = A, B, Cf
    flat[place[134:334]] = rng.choice(others, size=200)
    pixel_map = flat.reshape(H, W)
    images = rng.integers(1, 255, size=cap["images"].shape).astype(np.uint8)
    ys, xs = np.nonzero(pixel_map == B)
    images[:15, H - 1 - ys[0], xs[0], 0] = 0   # channel 0 of face B: 1040 - 15 = 1025
    images[:, H - 1 - ys[1], xs[1], 2] = 0     # channel 2 of face B: 1040 - 16 = 1024
    ys, xs = np.nonzero(pixel_map == Cf)
    images[:, H - 1 - ys, xs, 2] = 0           # face C: no valid sample in channel 2
    cap.update(pixel_map=pixel_map, images=images, edge_faces=(A, B, Cf))
    return cap


def test_chunk_and_channel_edges(gpu):
    import brdf_amd
    model = 1
    cap = edge_capture()
    A, B, Cf = cap["edge_faces"]
    single = S._single(gpu, cap, model, **P.RULE)
    mats = _materials(model, single["single_brdf"])
    sumsq, count, pixels = _residuals(gpu, cap, model, mats, **P.RULE)
    assert list(count[A]) == [1024] * 3 and list(count[B]) == [1025, 1040, 1024] and count[Cf, 2] == 0 and min(count[Cf, :2]) == 80
    assert list(pixels[[A, B, Cf]]) == [64, 65, 5]
    assert sumsq[:, 0, :].tobytes() == single["face_sumsq"].tobytes() and count.tobytes() == single["face_count"].tobytes()
    assert not sumsq[Cf, :, 2].any() and np.all(sumsq[Cf, :, :2] > 0)
    for m in range(GROUP + 1):
        assert sumsq[:, m, :].tobytes() == _residuals(gpu, cap, model, mats[m:m + 1], **P.RULE)[0][:, 0, :].tobytes(), m
    twin = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    _numpy_check(model, twin, mats, sumsq, count)


def test_scans_over_many_faces_and_a_face_of_five_chunks(gpu):
    import brdf_amd
    model = 1
    cap = P.big_capture()
    single = S._single(gpu, cap, model, **P.RULE)
    mats = _materials(model, single["single_brdf"])
    sumsq, count, pixels = _residuals(gpu, cap, model, mats, **P.RULE)
    assert sumsq[:, 0, :].tobytes() == single["face_sumsq"].tobytes() and count.tobytes() == single["face_count"].tobytes()
    assert pixels.tobytes() == single["face_pixels"].tobytes() and int((pixels > 0).sum()) == 644
    assert np.all(count[cap["big_face"]] == 4800)  # five residual chunks
    for f in (0, 65535, 65536, cap["nf"] - 1):
        assert pixels[f] > 0 and np.all(sumsq[f] != SENTINEL)
    for m in (1, GROUP):
        assert sumsq[:, m, :].tobytes() == _residuals(gpu, cap, model, mats[m:m + 1], **P.RULE)[0][:, 0, :].tobytes(), m
    twin = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    _numpy_check(model, twin, mats[[0, GROUP]], sumsq[:, [0, GROUP], :], count)


def test_a_ward_material_of_zero_alpha_keeps_to_its_column(gpu):
    model = 2
    cap, single, _ = _single_and_one(gpu, model, 16)
    mats = _materials(model, single["single_brdf"])[:3].copy()
    mats[1, :, 2] = 0.0  # alpha = 0: 1 / alpha^2 is inf, the model value NaN
    sumsq, count, _ = _residuals(gpu, cap, model, mats, **P.RULE)
    sampled = count > 0
    assert sampled.any() and not np.isfinite(sumsq[:, 1, :][sampled]).any()
    carried = np.flatnonzero(count[:, 0] != SENTINEL)
    assert np.all(sumsq[:, 1, :][carried][~sampled[carried]] == 0.0)
    for m in (0, 2):
        assert sumsq[:, m, :].tobytes() == _residuals(gpu, cap, model, mats[m:m + 1], **P.RULE)[0][:, 0, :].tobytes(), m
        assert np.isfinite(sumsq[:, m, :]).all()
