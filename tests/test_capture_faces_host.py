"""The per-face capture (brdf_hip_fit_capture_faces_dev), the part that needs no device: brdf_amd.group_capture_samples -- the
entry's definition as code -- against a plain triple loop, and the entry's refusals, every one before any HIP call (as
tests/test_packed_host.py checks for the packed entries)."""
import ctypes as C

import numpy as np
import pytest

H, W, LIGHTS, NF = 3, 4, 5, 4
ENTRY = "brdf_hip_fit_capture_faces_dev"


def _capture():
    """face 2 on three pixels (walk order (0,1), (2,0), (3,2)), face 0 on one, face 1 on none, one entry >= nf, the rest background"""
    rng = np.random.default_rng(3)
    pixel_map = np.full((H, W), -1, dtype=np.int32)
    pixel_map[2, 3], pixel_map[1, 0], pixel_map[0, 2] = 2, 2, 2
    pixel_map[1, 1] = 0
    pixel_map[2, 0] = NF + 3
    images = rng.integers(1, 255, size=(LIGHTS, H, W, 3)).astype(np.uint8)
    images[0, H - 1 - 1, 0, 0], images[3, H - 1 - 0, 2, 1], images[4, H - 1 - 1, 1, 2] = 0, 255, 0  # on pixels that carry a face
    images[2, H - 1 - 2, 3, :] = (255, 0, 17)
    angles = rng.uniform(0.05, 1.0, size=(NF, 3, LIGHTS))
    angles[2, 0, 1], angles[2, 1, 4], angles[2, 2, 2], angles[0, 1, 0] = -0.3, 0.0, -0.9, np.nan  # plane 2: only Phong and Ward read it
    return images, pixel_map, angles


def _loop(images, pixel_map, angles, model, v_min, v_max, cos_min):
    reads = {0: (0, 2), 1: (0, 1), 2: (0, 1, 2)}[model]
    out_a, out_x, offsets, fit_face, fit_channel, face_pixels = [], [], [0], [], [], np.zeros(NF, dtype=np.int32)
    for f in range(NF):
        pixels = [(x, y) for x in range(W) for y in range(H) if pixel_map[y, x] == f]  # x outer, y inner
        face_pixels[f] = len(pixels)
        if not pixels:
            continue
        for c in range(3):
            kept = []
            for x, y in pixels:
                for i in range(LIGHTS):
                    v = int(images[i, H - 1 - y, x, c])
                    if v_min <= v <= v_max and all(angles[f, k, i] > cos_min for k in reads):
                        kept.append((i, v / 255.0))
            for plane in range(3):
                out_a += [angles[f, plane, i] for i, _ in kept]
            out_x += [v for _, v in kept]
            offsets.append(offsets[-1] + len(kept))
            fit_face.append(f)
            fit_channel.append(c)
    return np.array(out_a), np.array(out_x), np.array(offsets, dtype=np.int64), fit_face, fit_channel, face_pixels


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("rule", [(0, 255, -2.0), (1, 254, 0.0)])
def test_group_capture_samples_against_a_plain_loop(model, rule):
    import brdf_amd
    images, pixel_map, angles = _capture()
    want = _loop(images, pixel_map, angles, model, *rule)
    got = brdf_amd.group_capture_samples(images, pixel_map, angles, model, v_min=rule[0], v_max=rule[1], cos_min=rule[2])
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2])
    assert list(got[3]) == want[3] == [0, 0, 0, 2, 2, 2] and list(got[4]) == want[4] == [0, 1, 2] * 2
    assert got[5].dtype == np.int32 and list(got[5]) == list(want[5]) == [1, 0, 3, 0]
    assert got[0].dtype == got[1].dtype == np.float64
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()  # sample order: pixel walk, light inner
    counts = np.diff(got[2])
    if rule == (0, 255, -2.0):  # the rule switched off keeps every candidate but face 0's NaN cosine (plane 1: not read by Phong)
        assert list(counts) == [LIGHTS - (model != 0)] * 3 + [3 * LIGHTS] * 3
        assert np.array_equal(got[1][got[2][3]:got[2][4]], np.array([images[i, H - 1 - y, x, 0] for x, y in ((0, 1), (2, 0), (3, 2)) for i in range(LIGHTS)]) / 255.0)
    else:  # values 0 and 255 and the cosines <= 0 drop out
        assert counts.max() < 3 * LIGHTS and counts[3:].min() >= 3
        assert model == 0 or not np.isnan(got[0]).any()  # (the NaN stands in plane 1, which Phong does not read: there it travels)
        assert got[1].min() >= 1 / 255.0 and got[1].max() <= 254 / 255.0


def test_group_capture_samples_of_an_empty_capture():
    import brdf_amd
    images, pixel_map, angles = _capture()
    got = brdf_amd.group_capture_samples(images, np.full_like(pixel_map, -1), angles, 1)
    assert got[0].size == got[1].size == got[3].size == got[4].size == 0 and list(got[2]) == [0] and not got[5].any()


def test_capture_faces_entry_refuses_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read: every call below is refused before anything touches memory
    ptr = C.c_void_p(buf.ctypes.data)
    dbl = buf.ctypes.data_as(D)
    p0, lb, ub = np.array([0.5, 1.0, 1.0]), np.zeros(3), np.full(3, 100.0)

    def call(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, vertices=ptr, faces=ptr, normals=ptr, nf=10, leds=dbl, view=dbl, p=p0, lo=lb, hi=ub,
             v_min=0, v_max=255, cos_min=-2.0, ws=0, surfaces=ptr):
        d = lambda a: a.ctypes.data_as(D) if isinstance(a, np.ndarray) else a  # noqa: E731
        return lib.brdf_hip_fit_capture_faces_dev(model, images, L, H_, W_, pm, vertices, faces, normals, nf, leds, view, 1, d(p), d(lo), d(hi), 100,
                                                  None, v_min, v_max, cos_min, ws, surfaces, None, None, None, None, None, None, None, None, None,
                                                  None, None)

    refused = [dict(images=None), dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None),
               dict(p=None), dict(surfaces=None),                                     # null required pointers
               dict(L=0), dict(L=65), dict(L=-1), dict(H_=0), dict(W_=-2), dict(nf=0), dict(nf=-1),
               dict(nf=(2 ** 31 - 1) // 3 + 1),                                       # 3 nf > INT_MAX
               dict(model=3), dict(model=-1), dict(v_min=200, v_max=100), dict(cos_min=float("nan")), dict(ws=-1),
               dict(lo=np.array([0.0, 2.0, 0.0]), hi=np.array([1.0, 1.0, 1.0]))]      # lb > ub: levmar's own refusal
    for kw in refused:
        assert call(**kw) == -1, kw
        assert ENTRY in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert "lower bound exceeds" in brdf_amd.last_error()
    assert call(model=7) == -1 and "unknown model" in brdf_amd.last_error()
    assert call(ws=-9) == -1 and "workspace_bytes" in brdf_amd.last_error()
    assert call(v_min=3, v_max=2) == -1 and "v_min 3 > v_max 2" in brdf_amd.last_error()
    capfd.readouterr()
