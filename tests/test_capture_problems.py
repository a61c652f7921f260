"""The captures of tests/capture_problems.py hold what tests/test_gpu_capture_shapes.py rests on: a fixture that drifts fails here, on
the CPU, and not silently on the GPU.  And brdf_amd.group_capture_samples -- the per-face entry's definition as code -- equals a plain
triple loop on the big capture too (tests/test_capture_faces_host.py checks it on twelve pixels)."""
import numpy as np
import pytest

from tests import capture_problems as P


@pytest.mark.parametrize("model", [0, 1, 2])
def test_rule_capture_separates_the_planes(model):
    cap = P.rule_capture(model)
    touched = np.unique(cap["pixel_map"][cap["pixel_map"] > -1])
    assert touched.size == 37 and cap["images"].shape == (16, 23, 31, 3)
    cats = P.rule_categories(cap["ang"][touched])
    assert {k: int(m.sum()) for k, m in cats.items()} == P.RULE_COUNTS
    # ... and in this model's images every category decides about candidates whose intensity passes: the planes, not the
    # intensities, make the counts
    g, face = P.walk(cap["pixel_map"], cap["nf"])
    value = P.pixel_values(cap["images"], g)
    shown = ((value >= 1) & (value <= 254)).any(axis=1)  # [P,L]: in some channel
    cats = P.rule_categories(cap["ang"][face])
    for name, mask in cats.items():
        assert int((mask & shown).sum()) >= 1, (model, name)
    # what a wrong plane set would count: the three models differ on this capture
    counts = {m: int(P.rule_valid(m, value, cap["ang"][face], **P.RULE).sum()) for m in (0, 1, 2)}
    assert counts[2] < counts[0] and counts[2] < counts[1] and counts[0] != counts[1], counts


def test_rule_capture_with_a_nan_face():
    cap, sound = P.rule_capture(1, nan_face=True), P.rule_capture(1)
    f = cap["nan_face"]
    assert int((cap["pixel_map"] == f).sum()) == 10 and not (cap["pixel_map_without"] == f).any()
    assert np.isnan(cap["ang"][f]).all() and not np.isnan(np.delete(cap["ang"], f, axis=0)).any()
    assert np.array_equal(np.delete(cap["ang"], f, axis=0), np.delete(sound["ang"], f, axis=0)) and np.array_equal(cap["images"], sound["images"])


def _big_group(model):
    import brdf_amd
    cap = P.big_capture()
    return brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)


def test_big_capture_reaches_the_multi_item_scans():
    cap = P.big_capture()
    nf, pm = cap["nf"], cap["pixel_map"]
    assert pm.shape == (67, 73) and nf == 70001 > 65536 and cap["images"].shape[0] == 16
    g, face = P.walk(pm, nf)
    carried = np.unique(face)
    assert g.size == 4500 and np.array_equal(carried, cap["carried"]) and carried.size == 644 > 85  # more than one scatter block
    assert {0, 65535, 65536, nf - 1} <= set(carried.tolist()) and (carried >= 65536).any()
    assert int((pm == nf).sum()) == 40 and int((pm == -5).sum()) == 40
    assert int((pm == cap["big_face"]).sum()) == 300
    candidates = g.size * 16
    assert (candidates + P.KCT - 1) // P.KCT == 282 > 256  # pack blocks: block_scan3_kernel's threads own two each
    assert (3 * carried.size + P.KCT - 1) // P.KCT == 8  # scatter blocks
    assert (nf + P.KCT - 1) // P.KCT > 1  # face_scan_kernel: 274 faces per thread
    counts = np.diff(_big_group(1)[2])
    assert counts.size == 3 * 644 and (counts < 3).any() and counts.max() > 4096
    classes = np.bincount(np.searchsorted(P.PACKED_BOUNDS, counts), minlength=6)
    print("fits per size class:", classes, "below 3 samples:", int((counts < 3).sum()))
    assert all(classes[c] >= 1 for c in (0, 1, 2, 3, 5)), classes
    for model in (0, 2):
        assert np.diff(_big_group(model)[2]).max() > 4096


def test_wide_captures_pass_the_grid_caps():
    for lights, H, W in ((16, 300, 300), (64, 150, 150)):
        cap = P.wide_capture(lights, H, W)
        assert cap["images"].shape == (lights, H, W, 3) and cap["nf"] == 300 and cap["leds"].shape == (lights, 3)
        assert (cap["pixel_map"] >= 0).all() and np.unique(cap["pixel_map"]).size == 300
        assert 3 * H * W * lights > P.GATHER_CAP == 4194304
    assert 3 * 300 * 300 > 262144  # cosines_rows_kernel: 16 surfels per block, 16384 blocks
    assert (3 * 150 * 150 + 3) // 4 > 16384  # cosines_kernel at 64 lights: 4 surfels per block
    assert np.array_equal(P.leds_for(64)[:16], P.leds_for(16)) and len({tuple(r) for r in P.leds_for(64)}) == 64


@pytest.mark.parametrize("model", [0, 1, 2])
def test_group_capture_samples_on_the_big_capture_against_a_plain_loop(model):
    cap = P.big_capture()
    images, pm, ang, nf = cap["images"], cap["pixel_map"], cap["ang"], cap["nf"]
    lights, H, W = images.shape[:3]
    a, x, off, fit_face, fit_channel, face_pixels = _big_group(model)
    reads = [k for k in range(3) if P.READS[model][k]]
    assert np.array_equal(fit_face, np.repeat(cap["carried"], 3)) and np.array_equal(fit_channel, np.tile([0, 1, 2], 644))
    assert face_pixels.sum() == 4500 and np.array_equal(np.flatnonzero(face_pixels), cap["carried"])
    where = {int(f): [] for f in cap["carried"]}
    for x_ in range(W):  # x outer, y inner
        for y_ in range(H):
            f = int(pm[y_, x_])
            if f in where:
                where[f].append((x_, y_))
    s = 0
    for f in cap["carried"]:
        assert face_pixels[f] == len(where[int(f)])
        for c in range(3):
            kept = [(i, images[i, H - 1 - y_, x_, c] / 255.0) for x_, y_ in where[int(f)] for i in range(lights)
                    if 1 <= images[i, H - 1 - y_, x_, c] <= 254 and all(ang[f, k, i] > 0.0 for k in reads)]
            k = len(kept)
            assert off[s + 1] - off[s] == k, (f, c)
            want_a = np.array([ang[f, plane, i] for plane in range(3) for i, _ in kept])
            assert a[3 * off[s]:3 * off[s + 1]].tobytes() == want_a.tobytes() and x[off[s]:off[s + 1]].tobytes() == np.array([v for _, v in kept]).tobytes()
            s += 1
    assert s == len(fit_face)
