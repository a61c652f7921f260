"""The single-BRDF capture over every valid sample (brdf_hip_fit_capture_single_faces_dev), the part that needs no device: the entry's
refusals, every one before any HIP call; brdf_amd.group_capture_single_samples -- the entry's sample sets as code -- against a plain
concatenation of group_capture_samples' fits on the captures of tests/capture_problems.py, with the channel counts the GPU tests rest
on; and the wrapper's validation."""
import ctypes as C

import numpy as np
import pytest

from tests import capture_problems as P

ENTRY = "brdf_hip_fit_capture_single_faces_dev"
RULE_OFF = dict(v_min=0, v_max=255, cos_min=-2.0)
# K_c under RULE on rule_capture(model) at 16 lights; at 5 lights (Ward: 287 ... 289)
K_RULE_16 = {0: (6822, 6822, 6822), 1: (2267, 2258, 2257), 2: (993, 1006, 1013)}
K_RULE_5 = {0: (2106, 2106), 1: (558, 558), 2: (287, 289)}  # (smallest, largest) over the channels


def test_entry_refuses_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read: every call below is refused before anything touches memory
    ptr = C.c_void_p(buf.ctypes.data)
    dbl = buf.ctypes.data_as(D)
    p0, lb, ub = np.array([0.5, 1.0, 1.0]), np.zeros(3), np.full(3, 100.0)
    single = np.zeros(9)

    def call(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, vertices=ptr, faces=ptr, normals=ptr, nf=10, leds=dbl, view=dbl, p=p0, lo=lb, hi=ub,
             v_min=0, v_max=255, cos_min=-2.0, out=single):
        d = lambda a: a.ctypes.data_as(D) if isinstance(a, np.ndarray) else a  # noqa: E731
        return lib.brdf_hip_fit_capture_single_faces_dev(model, images, L, H_, W_, pm, vertices, faces, normals, nf, leds, view, 1, d(p), d(lo), d(hi),
                                                         100, None, v_min, v_max, cos_min, d(out), None, None, None, None, None, None, None, None,
                                                         None, None, None, None)

    refused = [dict(images=None), dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None),
               dict(p=None), dict(out=None),                                          # null required pointers
               dict(L=0), dict(L=65), dict(L=-1), dict(H_=0), dict(W_=-2), dict(nf=0), dict(nf=-1),
               dict(nf=(2 ** 31 - 1) // 3 + 1),                                       # 3 nf > INT_MAX
               dict(model=3), dict(model=-1), dict(v_min=200, v_max=100), dict(cos_min=float("nan")),
               dict(lo=np.array([0.0, 2.0, 0.0]), hi=np.array([1.0, 1.0, 1.0]))]      # lb > ub: levmar's own refusal
    for kw in refused:
        assert call(**kw) == -1, kw
        assert ENTRY in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert "lower bound exceeds" in brdf_amd.last_error()
    assert not single.any()  # a refused call writes nothing
    assert call(model=7) == -1 and "unknown model" in brdf_amd.last_error()
    assert call(v_min=3, v_max=2) == -1 and "v_min 3 > v_max 2" in brdf_amd.last_error()
    assert call(out=None) == -1 and "single_brdf" in brdf_amd.last_error()
    capfd.readouterr()


def _concatenation(cap, model, **rule):
    """channel c's sample set from group_capture_samples' fits, one face behind the other, by a plain loop"""
    import brdf_amd
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **rule)
    out = []
    for c in range(3):
        planes, xs, face_offsets, faces = [[], [], []], [], [0], []
        for s in range(len(fit_face)):
            if fit_channel[s] != c:
                continue
            k = int(off[s + 1] - off[s])
            for j in range(3):
                planes[j] += list(a[3 * off[s] + j * k:3 * off[s] + (j + 1) * k])
            xs += list(x[off[s]:off[s + 1]])
            face_offsets.append(face_offsets[-1] + k)
            faces.append(int(fit_face[s]))
        out.append((np.array(planes, dtype=np.float64).reshape(3, -1), np.array(xs, dtype=np.float64), face_offsets, faces))
    return out, face_pixels


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("ruled", [True, False])
def test_twin_is_the_concatenation_of_the_grouped_fits(model, ruled):
    import brdf_amd
    cap = P.rule_capture(model)
    rule = P.RULE if ruled else RULE_OFF
    want, face_pixels = _concatenation(cap, model, **rule)
    got = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **rule)
    assert got.faces.dtype == np.int32 and got.face_pixels.dtype == np.int32 and np.array_equal(got.face_pixels, face_pixels)
    assert got.faces.size == 37 and int(face_pixels.sum()) == 604 and np.array_equal(got.faces, np.flatnonzero(face_pixels))
    for c in range(3):
        ang, x, face_offsets = got.channels[c]
        assert ang.dtype == x.dtype == np.float64 and face_offsets.dtype == np.int64 and ang.flags.c_contiguous
        assert ang.shape == (3, x.size) and list(face_offsets) == want[c][2] and want[c][3] == list(got.faces)
        assert ang.tobytes() == want[c][0].tobytes() and x.tobytes() == want[c][1].tobytes()
    counts = tuple(int(got.channels[c][1].size) for c in range(3))
    print("model", model, "rule", ruled, "K", counts)
    assert counts == (K_RULE_16[model] if ruled else (9664,) * 3)
    if not ruled:  # every candidate is a sample: the three channels' planes coincide
        assert got.channels[0][0].tobytes() == got.channels[1][0].tobytes() == got.channels[2][0].tobytes()


@pytest.mark.parametrize("model", [0, 1, 2])
def test_counts_at_five_lights(model):
    import brdf_amd
    cap = P.rule_capture(model, lights=5)
    got = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    counts = [int(got.channels[c][1].size) for c in range(3)]
    print("model", model, "five lights, K", counts)
    assert K_RULE_5[model][0] <= min(counts) and max(counts) <= K_RULE_5[model][1]
    off = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model)
    assert [int(off.channels[c][1].size) for c in range(3)] == [604 * 5] * 3


def test_twin_of_an_empty_capture_and_its_validation():
    import brdf_amd
    cap = P.rule_capture(1)
    got = brdf_amd.group_capture_single_samples(cap["images"], np.full_like(cap["pixel_map"], -1), cap["ang"], 1)
    assert got.faces.size == 0 and not got.face_pixels.any()
    for c in range(3):
        assert got.channels[c][0].shape == (3, 0) and got.channels[c][1].size == 0 and list(got.channels[c][2]) == [0]
    with pytest.raises(ValueError):
        brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], 5)
    with pytest.raises(ValueError):
        brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"][:-1], cap["ang"], 1)
    with pytest.raises(ValueError):
        brdf_amd.group_capture_single_samples(cap["images"].astype(np.int32), cap["pixel_map"], cap["ang"], 1)


def test_wrapper_validates_before_it_calls():
    """host tensors, wrong types and wrong shapes never reach the library"""
    import torch
    import brdf_amd
    cap = P.rule_capture(1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731  (host tensors)
    args = [t(cap["images"]), t(cap["pixel_map"]), t(cap["vertices"]), t(cap["faces"]), t(cap["nrm"])]
    with pytest.raises(ValueError):
        brdf_amd.fit_capture_single_faces(1, *args, cap["leds"], cap["view"], p0=P.P0, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS)
    assert brdf_amd.CaptureSingleFaces._fields == ("single_brdf", "info", "ret", "count", "stats", "face_sumsq", "face_count", "face_pixels",
                                                   "n_pixels", "n_faces")
