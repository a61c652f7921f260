"""One fit per (label, channel) (brdf_hip_fit_capture_labelled_dev).  Captures: tests/capture_problems.py.

  (1) every map has the bytes of fit_batch_packed + fit_stats_batch_packed on the twin's batch (group_capture_label_samples, rows
      channel * K + label) from the same starting points: shuffled labels, an empty label, a label of fewer than 3 samples, labels
      outside [0, K), K = 1, a label above 4096 samples next to labels of at most 16 in one call, distinct starts per (label, channel);
      two calls give the same bytes;
  (2) label[f] = f, K = nf and every start p0: fit_capture_faces' bytes in every map both have;
  (3) K = 1 against fit_capture_single_faces: the counts are equal; whether p has the same bytes is printed (DESIGN.md records it: the
      packed call's large-fit path is the definition here, the single-fit entry's regime choice there);
  (4) big_capture(): 70,001 faces, 644 carried, the sort and the scans over many faces."""
import numpy as np
import pytest

from tests import capture_problems as P
from tests import test_gpu_capture_single_faces as S

pytestmark = pytest.mark.gpu
MAPS = ("materials", "info", "ret", "covar", "stats", "rank", "count", "label_faces", "face_pixels")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def _labelled(gpu, cap, model, labels, starts, images=None, **rule):
    """fit_capture_labelled, everything on the host: a dict of numpy arrays"""
    torch, brdf_amd, _ = gpu
    r = brdf_amd.fit_capture_labelled(model, S._dev(gpu, cap["images"] if images is None else images), S._dev(gpu, cap["pixel_map"]),
                                      S._dev(gpu, cap["vertices"]), S._dev(gpu, cap["faces"]), S._dev(gpu, cap["nrm"]), cap["leds"], cap["view"],
                                      np.asarray(labels, dtype=np.int32), np.array(starts, dtype=np.float64), rv_mode=1, lb=P.LB, ub=P.UB, itmax=100,
                                      opts=P.OPTS, validate=False, **rule)
    torch.cuda.synchronize()
    return dict(materials=r.materials.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), covar=r.stats.covar.cpu().numpy(),
                stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy(), count=r.count.cpu().numpy(), label_faces=r.label_faces.cpu().numpy(),
                face_pixels=r.face_pixels.cpu().numpy(), n_pixels=r.n_pixels, n_faces=r.n_faces)


def _definition(gpu, cap, model, labels, starts, images=None, **rule):
    """the two packed calls on the twin's batch, laid out as the entry's maps"""
    torch, brdf_amd, _ = gpu
    K = len(starts)
    twin = brdf_amd.group_capture_label_samples(cap["images"] if images is None else images, cap["pixel_map"], cap["ang"], model, labels, K, **rule)
    rows = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).transpose(1, 0, 2).reshape(3 * K, 3))  # row c * K + k
    a = S._dev(gpu, twin.angles if twin.angles.size else np.zeros(3))
    x = S._dev(gpu, twin.x if twin.x.size else np.zeros(1))
    off = S._dev(gpu, twin.offsets)
    p, info, ret = brdf_amd.fit_batch_packed(brdf_amd.METHOD_BC_DIF, model, a, x, off, S._dev(gpu, rows), lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS,
                                             validate=False)
    st = brdf_amd.fit_stats_batch_packed(brdf_amd.METHOD_BC_DIF, model, a, x, off, p, opts=P.OPTS, validate=False)
    torch.cuda.synchronize()
    back = lambda t, *tail: np.ascontiguousarray(t.cpu().numpy().reshape(3, K, *tail).swapaxes(0, 1))  # noqa: E731
    return dict(materials=back(p, 3), info=back(info, 10), ret=back(ret), covar=back(st.covar, 3, 3), stats=back(st.stats, 8), rank=back(st.rank),
                count=np.ascontiguousarray(np.diff(twin.offsets).astype(np.int32).reshape(3, K).T), label_faces=twin.label_faces,
                face_pixels=twin.face_pixels), twin


def _same(got, want, names=MAPS):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, want[name].dtype, got[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


def _starts(K, seed=0):
    """distinct starting points per (label, channel), inside the box"""
    return np.array(P.P0)[None, None, :] * np.random.default_rng(100 + seed).uniform(0.6, 1.4, size=(K, 3, 3))


def _carried(cap):
    return np.flatnonzero(np.bincount(cap["pixel_map"][(cap["pixel_map"] >= 0) & (cap["pixel_map"] < cap["nf"])], minlength=cap["nf"]))


@pytest.mark.parametrize("model", [0, 1, 2])
def test_shuffled_labels_an_empty_label_a_short_label_and_labels_outside(gpu, model):
    cap = P.rule_capture(model)
    carried = _carried(cap)
    rng = np.random.default_rng(50 + model)
    K = 5
    labels = np.full(cap["nf"], 3, dtype=np.int32)  # (faces no pixel carries: their label does not matter)
    labels[carried] = rng.integers(0, 3, size=carried.size)  # label 3 stays empty
    one_pixel = int(carried[np.flatnonzero(np.bincount(cap["pixel_map"][cap["pixel_map"] >= 0], minlength=cap["nf"])[carried] == 1)[0]])
    labels[one_pixel] = 4  # label 4: this face alone, two values left in every channel
    images = cap["images"].copy()
    ys, xs = np.nonzero(cap["pixel_map"] == one_pixel)
    H = images.shape[1]
    images[2:, H - 1 - ys[0], xs[0], :] = 0
    outside = carried[carried != one_pixel][[1, 7, 12]]
    labels[outside] = [-1, K, 10 ** 6]
    starts = _starts(K, model)
    got = _labelled(gpu, cap, model, labels, starts, images=images, **P.RULE)
    want, twin = _definition(gpu, cap, model, labels, starts, images=images, **P.RULE)
    print("model", model, "counts", got["count"].T.tolist(), "ret", got["ret"].T.tolist(), "faces", got["label_faces"].tolist())
    _same(got, want)
    assert got["label_faces"][3] == 0 and got["label_faces"][4] == 1 and got["label_faces"].sum() == carried.size - 3
    assert got["n_faces"] == carried.size and got["n_pixels"] == 604
    for k in (3, 4):  # the packed call's refusal: ret -1, zero info, the start untouched, rank 0
        assert np.all(got["count"][k] < 3) and (k == 4 or not got["count"][k].any())
        assert np.all(got["ret"][k] == -1) and not got["info"][k].any() and got["materials"][k].tobytes() == starts[k].tobytes() and not got["rank"][k].any()
    assert np.all(got["count"][:3].sum(axis=0) > 0)
    _same(_labelled(gpu, cap, model, labels, starts, images=images, **P.RULE), got)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_one_label_and_the_single_capture(gpu, model):
    cap = P.rule_capture(model)
    labels = np.zeros(cap["nf"], dtype=np.int32)
    starts = np.tile(np.array(P.P0), (1, 3, 1))
    got = _labelled(gpu, cap, model, labels, starts, **P.RULE)
    want, _ = _definition(gpu, cap, model, labels, starts, **P.RULE)
    _same(got, want)
    single = S._single(gpu, cap, model, **P.RULE)
    assert list(got["count"][0]) == [int(k) for k in single["count"]] and got["label_faces"][0] == single["n_faces"]
    print(f"model {model}: K = 1 against fit_capture_single_faces: counts {got['count'][0].tolist()}, p the same bytes "
          f"{got['materials'][0].tobytes() == single['single_brdf'].tobytes()}, ret {got['ret'][0].tolist()} / {single['ret'].tolist()}, "
          f"largest relative difference of p {np.max(np.abs(got['materials'][0] - single['single_brdf']) / np.maximum(np.abs(single['single_brdf']), 1e-12)):.3e}")


def test_a_label_above_4096_samples_next_to_labels_of_sixteen(gpu):
    import brdf_amd
    model = 0
    cap = P.rule_capture(model)
    carried = _carried(cap)
    per_face = np.diff(brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], model, **P.RULE)[2]).reshape(-1, 3)
    small = [int(carried[r]) for r in np.flatnonzero((per_face.max(axis=1) <= 16) & (per_face.min(axis=1) >= 3))[:2]]
    assert len(small) == 2
    labels = np.zeros(cap["nf"], dtype=np.int32)
    labels[small] = [1, 2]
    starts = _starts(3, 9)
    got = _labelled(gpu, cap, model, labels, starts, **P.RULE)
    want, _ = _definition(gpu, cap, model, labels, starts, **P.RULE)
    print("counts", got["count"].T.tolist(), "ret", got["ret"].T.tolist(), "packed classes", brdf_amd.last_packed_stats())
    assert np.all(got["count"][0] > 4096) and np.all(got["count"][1:] <= 16) and np.all(got["count"][1:] >= 3)
    _same(got, want)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_a_label_per_face_gives_the_per_face_capture(gpu, model):
    torch, brdf_amd, _ = gpu
    cap = P.rule_capture(model)
    nf = cap["nf"]
    carried = _carried(cap)
    got = _labelled(gpu, cap, model, np.arange(nf), np.tile(np.array(P.P0), (nf, 3, 1)), **P.RULE)
    r = brdf_amd.fit_capture_faces(model, S._dev(gpu, cap["images"]), S._dev(gpu, cap["pixel_map"]), S._dev(gpu, cap["vertices"]), S._dev(gpu, cap["faces"]),
                                   S._dev(gpu, cap["nrm"]), cap["leds"], cap["view"], rv_mode=1, p0=P.P0, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS,
                                   validate=False, **P.RULE)
    torch.cuda.synchronize()
    faces = dict(materials=r.surfaces, info=r.info, ret=r.ret, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank, count=r.count)
    for name, t in faces.items():
        assert got[name][carried].tobytes() == t.cpu().numpy()[carried].tobytes(), name
    assert got["face_pixels"].tobytes() == r.face_pixels.cpu().numpy().tobytes() and (got["n_pixels"], got["n_faces"]) == (r.n_pixels, r.n_faces)
    rest = np.setdiff1d(np.arange(nf), carried)  # no pixel carries them: empty fits, refused
    assert rest.size and np.all(got["ret"][rest] == -1) and not got["count"][rest].any() and np.all(got["materials"][rest] == np.array(P.P0))
    assert list(got["label_faces"]) == [int(f in carried) for f in range(nf)]


def test_many_faces(gpu):
    model = 1
    cap = P.big_capture()
    carried = cap["carried"]
    rng = np.random.default_rng(77)
    K = 7
    labels = np.full(cap["nf"], -1, dtype=np.int32)
    labels[carried] = rng.integers(-1, K, size=carried.size)  # (-1: some carried faces take no part)
    starts = _starts(K, 3)
    got = _labelled(gpu, cap, model, labels, starts, **P.RULE)
    want, _ = _definition(gpu, cap, model, labels, starts, **P.RULE)
    print("counts", got["count"].T.tolist(), "faces", got["label_faces"].tolist())
    _same(got, want)
    assert got["label_faces"].sum() == int((labels[carried] >= 0).sum()) and got["n_faces"] == 644
