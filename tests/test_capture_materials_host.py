"""K materials per object -- brdf_hip_capture_face_residuals_dev, brdf_hip_fit_capture_labelled_dev, brdf_hip_fit_capture_materials_dev --
the part that needs no device: the header's declarations; every entry's refusals, each before any HIP call and under the entry's own
name; brdf_amd.group_capture_label_samples -- the labelled fit's sample sets as code -- against group_capture_samples and
group_capture_single_samples; brdf_amd.assign_materials on ties, NaN and all-inf rows; and Lloyd's iteration as NumPy code around the
compiled reference's dlevmar_bc_dif (the oracle's where oracle/_ref was not built) on the planted capture of
tests/materials_problems.py: it settles within 20 rounds with purity 1.0 and ends below the planted truth's sum of squares."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import capture_problems as P
from tests import materials_problems as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUALS, LABELLED, MATERIALS = ("brdf_hip_capture_face_residuals_dev", "brdf_hip_fit_capture_labelled_dev", "brdf_hip_fit_capture_materials_dev")
INT_MAX = 2 ** 31 - 1


def test_header_declares_the_three_entries():
    import brdf_amd
    from brdf_amd._lib import ABI
    text = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in (RESIDUALS, LABELLED, MATERIALS):
        assert f"int {name}(int model, const unsigned char *d_images" in text, name
        assert name in ABI and hasattr(brdf_amd.lib, name)
    for word in ("capture_face_residuals", "fit_capture_labelled", "fit_capture_materials", "group_capture_label_samples", "assign_materials",
                 "seed_materials"):
        assert callable(getattr(brdf_amd, word)), word


def _callers():
    """per entry: a function of keyword overrides that calls it with pointers that are never read"""
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)
    ptr, dbl = C.c_void_p(buf.ctypes.data), buf.ctypes.data_as(D)
    lb, ub = np.zeros(3), np.full(3, 100.0)
    d = lambda a: a.ctypes.data_as(D) if isinstance(a, np.ndarray) else a  # noqa: E731
    base = dict(model=1, images=ptr, L=16, H_=8, W_=8, pm=ptr, vertices=ptr, faces=ptr, normals=ptr, nf=10, leds=dbl, view=dbl, lo=lb, hi=ub, v_min=0,
                v_max=255, cos_min=-2.0, materials=ptr, K=2, labels=ptr, rounds=3, workspace=0)

    def capture(k):
        return (k["model"], k["images"], k["L"], k["H_"], k["W_"], k["pm"], k["vertices"], k["faces"], k["normals"], k["nf"], k["leds"], k["view"], 1)

    def residuals(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_capture_face_residuals_dev(*capture(k), k["v_min"], k["v_max"], k["cos_min"], k["materials"], k["K"], ptr, ptr, None, None,
                                                       None, None)

    def labelled(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_fit_capture_labelled_dev(*capture(k), d(k["lo"]), d(k["hi"]), 100, None, k["v_min"], k["v_max"], k["cos_min"],
                                                     k["workspace"], k["labels"], k["K"], k["materials"], None, None, None, None, None, None, None,
                                                     None, None, None, None)

    def materials(**kw):
        k = {**base, **kw}
        return lib.brdf_hip_fit_capture_materials_dev(*capture(k), d(k["lo"]), d(k["hi"]), 100, None, k["v_min"], k["v_max"], k["cos_min"],
                                                      k["workspace"], k["K"], k["rounds"], k["materials"], k["labels"], None, None, None, None, None,
                                                      None, None, None, None, None, None, None, None, None, None, None)
    return {RESIDUALS: residuals, LABELLED: labelled, MATERIALS: materials}, buf


def test_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    callers, buf = _callers()
    shared = [dict(images=None), dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None),
              dict(materials=None),                                               # null required pointers
              dict(K=0), dict(K=-3), dict(K=INT_MAX // 3 + 1),                    # K < 1, 3 K > INT_MAX
              dict(L=0), dict(L=65), dict(H_=0), dict(W_=-2), dict(nf=0), dict(nf=INT_MAX // 3 + 1), dict(model=3), dict(v_min=200, v_max=100),
              dict(cos_min=float("nan"))]
    fits = [dict(labels=None), dict(workspace=-1), dict(lo=np.array([0.0, 2.0, 0.0]), hi=np.array([1.0, 1.0, 1.0]))]  # lb > ub: levmar's own refusal
    loop = [dict(rounds=-1), dict(rounds=65)]
    for name, call in callers.items():
        cases = shared + (fits if name != RESIDUALS else []) + (loop if name == MATERIALS else [])
        for kw in cases:
            assert call(**kw) == -1, (name, kw)
            assert name + "()" in brdf_amd.last_error(), (name, kw, brdf_amd.last_error())
        assert call(L=65) == -1 and "1 <= L <= 64" in brdf_amd.last_error()
        assert call(K=0) == -1 and ("K = 0" in brdf_amd.last_error() or "M = 0" in brdf_amd.last_error())
        assert call(materials=None) == -1 and "materials" in brdf_amd.last_error()
    assert callers[LABELLED](lo=np.array([0.0, 2.0, 0.0]), hi=np.ones(3)) == -1 and "lower bound exceeds" in brdf_amd.last_error()
    assert callers[MATERIALS](rounds=65) == -1 and "0 <= rounds <= 64" in brdf_amd.last_error()
    assert callers[MATERIALS](labels=None) == -1 and "face_label" in brdf_amd.last_error()
    assert not buf.any()  # a refused call writes nothing
    capfd.readouterr()


@pytest.mark.parametrize("model", [0, 1, 2])
def test_labels_equal_to_the_face_index_reproduce_the_grouped_fits(model):
    import brdf_amd
    cap = P.rule_capture(model)
    nf = cap["nf"]
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    got = brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, np.arange(nf), nf, **P.RULE)
    assert got.offsets.dtype == np.int64 and got.offsets.size == 3 * nf + 1 and got.offsets[-1] == off[-1] and got.x.size == x.size
    assert np.array_equal(got.face_pixels, face_pixels) and np.array_equal(got.label_faces, (face_pixels > 0).astype(np.int32))
    seen = np.zeros(3 * nf, dtype=bool)
    for s in range(len(fit_face)):
        row = int(fit_channel[s]) * nf + int(fit_face[s])
        seen[row] = True
        lo, hi = int(got.offsets[row]), int(got.offsets[row + 1])
        assert hi - lo == off[s + 1] - off[s]
        assert got.x[lo:hi].tobytes() == x[off[s]:off[s + 1]].tobytes() and got.angles[3 * lo:3 * hi].tobytes() == a[3 * off[s]:3 * off[s + 1]].tobytes()
    assert not np.diff(got.offsets)[~seen].any()  # faces no pixel carries: empty fits


@pytest.mark.parametrize("model", [0, 1, 2])
def test_one_label_reproduces_the_single_sample_sets_and_an_outside_label_drops_its_face(model):
    import brdf_amd
    cap = P.rule_capture(model)
    nf = cap["nf"]
    single = brdf_amd.group_capture_single_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)
    got = brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, np.zeros(nf, dtype=np.int32), 1, **P.RULE)
    assert list(got.label_faces) == [single.faces.size] and got.offsets.size == 4
    for c in range(3):
        ang, x, _ = single.channels[c]
        lo, hi = int(got.offsets[c]), int(got.offsets[c + 1])
        assert got.x[lo:hi].tobytes() == x.tobytes() and got.angles[3 * lo:3 * hi].tobytes() == ang.tobytes(), c
    # labels outside [0, K) -- -1, K, a large one -- drop their faces; the others' sets are the two-label split of the same capture
    carried = single.faces
    labels = np.zeros(nf, dtype=np.int32)
    labels[carried[1::2]] = 1
    full = brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, labels, 2, **P.RULE)
    dropped = labels.copy()
    out = carried[[0, 1, 5]]
    dropped[out] = [-1, 2, 10 ** 6]
    part = brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, dropped, 2, **P.RULE)
    assert list(part.label_faces) == [int((labels[carried] == k).sum() - (labels[out] == k).sum()) for k in range(2)]
    per_face = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)[2]
    for c in range(3):
        for k in range(2):
            lost = sum(int(per_face[3 * r + c + 1] - per_face[3 * r + c]) for r in np.flatnonzero(np.isin(carried, out) & (labels[carried] == k)))
            row = c * 2 + k
            assert (full.offsets[row + 1] - full.offsets[row]) - (part.offsets[row + 1] - part.offsets[row]) == lost, (c, k)
    with pytest.raises(ValueError):
        brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, labels[:-1], 2)
    with pytest.raises(ValueError):
        brdf_amd.group_capture_label_samples(cap["images"], cap["pixel_map"], cap["ang"], model, labels, 0)


def test_assignment_ties_nan_and_rows_without_a_finite_cost():
    import brdf_amd
    inf, nan = np.inf, np.nan
    s = np.zeros((7, 3, 3))
    s[0] = [[1, 1, 1], [0.5, 0.5, 0.5], [2, 2, 2]]           # the least cost: 1
    s[1] = [[1, 2, 3], [3, 2, 1], [6, 0, 0]]                 # a three-way tie: the lowest k
    s[2] = [[nan, 0, 0], [4, 4, 4], [inf, 0, 0]]             # NaN and inf count as +inf: 1
    s[3] = [[nan, 1, 1], [1, inf, 1], [1, 1, -inf]]          # no finite cost: the label stays
    s[4] = [[1e308, 1e308, 1], [5, 5, 5], [7, 7, 7]]         # a sum that overflows is +inf: 1
    s[5] = [[0.1, 0.2, 0.3], [0.3, 0.2, 0.1], [9, 9, 9]]     # (0.1 + 0.2) + 0.3 > (0.3 + 0.2) + 0.1 in doubles: the order of the sum decides
    s[6] = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]                 # not carried: never assigned
    labels = np.array([-1, 2, 0, 2, -1, -1, -1], dtype=np.int32)
    carried = np.array([True] * 6 + [False])
    new, changed = brdf_amd.assign_materials(s, labels, carried=carried)
    assert (0.1 + 0.2) + 0.3 > (0.3 + 0.2) + 0.1
    assert new.dtype == np.int32 and list(new) == [1, 0, 1, 2, 1, 1, -1] and changed == 5
    again, changed = brdf_amd.assign_materials(s, new, carried=carried)
    assert list(again) == list(new) and changed == 0
    everyone, changed = brdf_amd.assign_materials(s, labels)  # without `carried` every row is a face
    assert list(everyone) == [1, 0, 1, 2, 1, 1, 0] and changed == 6
    with pytest.raises(ValueError):
        brdf_amd.assign_materials(s[:, :, :2], labels)


def test_lloyd_around_the_cpu_solver_recovers_the_planted_materials():
    cap = M.planted_capture()
    which = M.solver()
    sets, carried = M.face_samples()
    assert cap["nf"] == 80 and carried.size == 80 and cap["sizes"].min() >= 3 and cap["sizes"].max() <= 29
    assert sorted(np.bincount(cap["planted"])) == [20] * 4
    seeds, chosen = M.host_seeds(which, M.K_PLANTED)
    got = M.host_loop(which, seeds, 20)
    truth = M.face_sumsq(sets, carried, cap["nf"], cap["truth"])
    truth_total = float(sum(truth[f, cap["planted"][f]].sum() for f in carried))
    single_total = float(M.face_sumsq(sets, carried, cap["nf"], seeds[:1])[:, 0].sum())
    total = float(got["face_sumsq"].sum())
    print(f"solver {which}: seeds from faces {chosen} (planted {list(cap['planted'][chosen])}), changed {got['changed']}, rounds {got['rounds_used']}, "
          f"purity {M.purity(got['labels'], cap['planted'], M.K_PLANTED)}, sum of squares single {single_total:.4f} -> {total:.4f}, "
          f"planted truth {truth_total:.4f}")
    assert got["settled"] and got["rounds_used"] <= 20 and got["changed"][-1] == 0
    assert M.purity(got["labels"], cap["planted"], M.K_PLANTED) == 1.0
    assert total < truth_total < single_total
    short = M.host_loop(which, seeds, 0)  # rounds = 0: the seeds and one assignment
    assert short["rounds_used"] == 0 and not short["settled"] and short["changed"] == [80] and short["materials"].tobytes() == seeds.tobytes()
