"""The per-face capture (brdf_hip_fit_capture_faces_dev): one fit per (face, channel) over the samples of ALL the face's pixels.

The capture: the mesh and the renderer of tests/test_cosines.py (make_mesh, the loop of make_capture), 23 x 31 pixels, 40 faces, 16
lights, the signed planes of rv_mode = 1.  Six faces carry 300, 100, 40, 10, 3 and 1 pixels, scattered by a seeded permutation --
4800, 1600, 640, 160, 48 and 16 candidate samples, one face per size class of the packed batch --, about 150 further pixels go to
random other faces, the last faces get no pixel, the rest is background.  Every pixel has its own gain in [0.8, 1.2] before the
quantisation: a face's pixels differ, so a wrong order or membership shows in the bytes.

  (a) the definition: with v_min = 1, v_max = 254, cos_min = 0 every map has the bytes of fit_batch_packed + fit_stats_batch_packed on
      group_capture_samples (the oracle's cosine planes); all six size classes hold fits; untouched faces keep a sentinel; avg;
  (b) a map on which every carried face has one pixel, rule off: the bytes of fit_capture(want_stats=True);
  (c) on the capture with every fifth touched face blackened and every fifth saturated: every carried (face, channel) is refused by
      its count or reaches the CPU checker's objective over its own samples (<= ref * (1 + 1e-3) + 1e-20, the capture tests' bar);
  (d) two calls, a workspace that forces several chunks per class, L = 5 and an all-background map."""
import numpy as np
import pytest

from tests import oracle_libs as L

pytestmark = pytest.mark.gpu
OPTS = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
MODEL = 1  # Blinn-Phong reads cos(L.N) and cos(N.H)
P0, LB, UB = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0)
H, W, NF, LIGHTS = 23, 31, 40, 16
SIZES = (300, 100, 40, 10, 3, 1)  # pixels of the six class faces: one per packed size class at 16 lights
RULE = dict(v_min=1, v_max=254, cos_min=0.0)
SENTINEL = -7


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


def make_faces_capture():
    from brdf_amd import synth
    from tests.test_cosines import make_mesh
    vertices, faces, nrm, view = make_mesh(nv=200, nf=NF, seed=5)
    leds = L.led_table()
    c = vertices[faces].sum(axis=1) / 3.0
    flip = ((leds.mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0
    nrm[flip] *= -1.0
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)  # signed: lights behind a face have cos(L.N) <= 0
    # the six class faces: lit by every light, so that the rule leaves their size class alone, and none of them among every fifth
    # touched face (faces 0, 5, 10, ... and 1, 6, 11, ...: the ones test (c) blackens and saturates; every face below NF - 3 is touched)
    lit = [f for f in range(NF - 3) if f % 5 > 1 and (ang[f, :2] > 0.0).all()]
    assert len(lit) >= len(SIZES), lit
    class_faces = lit[:len(SIZES)]
    rng = np.random.default_rng(17)
    perm = rng.permutation(H * W)
    flat = np.full(H * W, -1, dtype=np.int32)
    at = 0
    for f, k in zip(class_faces, SIZES):
        flat[perm[at:at + k]] = f
        at += k
    others = np.setdiff1d(np.arange(NF - 3), class_faces)  # the last faces get no pixel
    flat[perm[at:at + 150]] = np.concatenate([others, rng.choice(others, size=150 - others.size)])
    pixel_map = flat.reshape(H, W)
    gain = rng.uniform(0.8, 1.2, size=(H, W))
    images = np.zeros((LIGHTS, H, W, 3), dtype=np.uint8)
    truth = np.array(synth.TRUTH[1])
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f < 0:
                continue
            for ch in range(3):
                val = L.model_values(1, np.abs(ang[f]), truth * (0.6 + 0.2 * ch))
                images[:, H - 1 - y, x, ch] = np.clip(np.round(val * 255.0 * 0.5 * gain[y, x]), 0, 255).astype(np.uint8)
    return dict(vertices=vertices, faces=faces, nrm=nrm, view=view, leds=leds, pixel_map=pixel_map, images=images, ang=ang,
                class_faces=class_faces)


@pytest.fixture(scope="module")
def capture():
    cap = make_faces_capture()
    for f, k in zip(cap["class_faces"], SIZES):
        assert int((cap["pixel_map"] == f).sum()) == k
    touched = np.unique(cap["pixel_map"][cap["pixel_map"] > -1])
    assert np.array_equal(touched, np.arange(NF - 3))
    return cap


@pytest.fixture(scope="module")
def masked_capture(capture):
    """the capture with every fifth touched face black and every fifth saturated, as tests/test_gpu_capture_masked.py's fixture"""
    cap = dict(capture)
    images, pixel_map = capture["images"].copy(), capture["pixel_map"]
    touched = np.unique(pixel_map[pixel_map > -1])
    black, saturated = set(touched[0::5]), set(touched[1::5])
    assert not (black | saturated) & set(capture["class_faces"])
    for y in range(H):
        for x in range(W):
            f = pixel_map[y, x]
            if f in black:
                images[:, H - 1 - y, x, :] = 0
            elif f in saturated:
                images[:, H - 1 - y, x, :] = 255
    cap["images"] = images
    return cap


def _dev(gpu, a):
    torch, _, dev = gpu
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sentinel_maps(gpu):
    torch, brdf_amd, dev = gpu

    def full(*shape, dtype=torch.float64):
        return torch.full((NF, *shape), SENTINEL, dtype=dtype, device=dev)
    return brdf_amd.CaptureFaces(full(3, 3), full(3, 10), full(3, dtype=torch.int32),
                                 brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=torch.int32)), full(3, dtype=torch.int32),
                                 full(dtype=torch.int32), None, 0, 0)


def _faces(gpu, cap, images=None, pixel_map=None, leds=None, out=None, **kw):
    """fit_capture_faces on the capture, everything on the host: a dict of numpy arrays"""
    torch, brdf_amd, _ = gpu
    images = cap["images"] if images is None else images
    pixel_map = cap["pixel_map"] if pixel_map is None else pixel_map
    leds = cap["leds"] if leds is None else leds
    r = brdf_amd.fit_capture_faces(MODEL, _dev(gpu, images), _dev(gpu, pixel_map), _dev(gpu, cap["vertices"]), _dev(gpu, cap["faces"]),
                                   _dev(gpu, cap["nrm"]), leds, cap["view"], rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, out=out, **kw)
    torch.cuda.synchronize()
    return dict(surfaces=r.surfaces.cpu().numpy(), info=r.info.cpu().numpy(), ret=r.ret.cpu().numpy(), covar=r.stats.covar.cpu().numpy(),
                stats=r.stats.stats.cpu().numpy(), rank=r.stats.rank.cpu().numpy(), count=r.count.cpu().numpy(),
                face_pixels=r.face_pixels.cpu().numpy(), avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)


MAPS = ("surfaces", "info", "ret", "count", "face_pixels", "covar", "stats", "rank")


def _packed(gpu, images, pixel_map, ang, fill=0, **rule):
    """the definition: group_capture_samples -> fit_batch_packed + fit_stats_batch_packed, laid out as the entry's maps"""
    torch, brdf_amd, _ = gpu
    a, x, off, fit_face, fit_channel, face_pixels = brdf_amd.group_capture_samples(images, pixel_map, ang, MODEL, **rule)
    S = len(fit_face)
    da, dx, do = _dev(gpu, a), _dev(gpu, x), _dev(gpu, off)
    p, info, ret = brdf_amd.fit_batch_packed(brdf_amd.METHOD_BC_DIF, MODEL, da, dx, do, _dev(gpu, np.tile(np.array(P0), (S, 1))), lb=LB, ub=UB,
                                             itmax=100, opts=OPTS)
    classes = brdf_amd.last_packed_stats()
    st = brdf_amd.fit_stats_batch_packed(brdf_amd.METHOD_BC_DIF, MODEL, da, dx, do, p, opts=OPTS)
    torch.cuda.synchronize()
    want = dict(surfaces=np.full((NF, 3, 3), fill, dtype=np.float64), info=np.full((NF, 3, 10), fill, dtype=np.float64),
                ret=np.full((NF, 3), fill, dtype=np.int32), count=np.full((NF, 3), fill, dtype=np.int32), face_pixels=face_pixels,
                covar=np.full((NF, 3, 3, 3), fill, dtype=np.float64), stats=np.full((NF, 3, 8), fill, dtype=np.float64),
                rank=np.full((NF, 3), fill, dtype=np.int32))
    at = (fit_face, fit_channel)
    want["surfaces"][at], want["info"][at], want["ret"][at] = p.cpu().numpy(), info.cpu().numpy(), ret.cpu().numpy()
    want["count"][at] = np.diff(off)
    want["covar"][at], want["stats"][at], want["rank"][at] = st.covar.cpu().numpy(), st.stats.cpu().numpy(), st.rank.cpu().numpy()
    return want, dict(a=a, x=x, off=off, fit_face=fit_face, fit_channel=fit_channel, classes=classes)


def test_definition_is_the_packed_batch_of_the_grouped_samples(gpu, capture):
    torch, brdf_amd, _ = gpu
    want, group = _packed(gpu, capture["images"], capture["pixel_map"], capture["ang"], fill=SENTINEL, **RULE)
    assert all(c["fits"] > 0 for c in group["classes"]), group["classes"]  # the reference side covers all six size classes ...
    got = _faces(gpu, capture, out=_sentinel_maps(gpu), **RULE)
    classes = brdf_amd.last_packed_stats()
    print("size classes of the entry's packed call:", classes)
    assert all(c["fits"] > 0 for c in classes), classes  # ... and so does the entry's own packed call
    for name in MAPS:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    untouched = np.setdiff1d(np.arange(NF), np.unique(group["fit_face"]))
    assert untouched.size >= 3
    for name in MAPS:
        if name != "face_pixels":  # (written for every face: 0 where none)
            assert np.all(got[name][untouched] == SENTINEL), name
    assert np.all(got["face_pixels"][untouched] == 0)
    assert got["n_faces"] == NF - 3 and got["n_pixels"] == int((capture["pixel_map"] > -1).sum()) == int(got["face_pixels"].sum())
    carried = np.unique(group["fit_face"])
    # at most 120 addends: any order of the sum is within 120 * 2^-53 relative of any other (all addends are >= 0: the box)
    ref = got["surfaces"][carried].reshape(-1, 3).sum(axis=0) / (NF * 3)
    assert np.all(np.abs(got["avg"] - ref) <= 1e-12 * np.abs(ref)), (got["avg"], ref)


def test_one_pixel_per_face_is_the_last_pixel_capture(gpu, capture):
    torch, brdf_amd, _ = gpu
    pixel_map = np.full((H, W), -1, dtype=np.int32)
    flat = pixel_map.reshape(-1)
    for f in range(NF - 3):  # the face's first pixel in row-major order: every carried face appears exactly once
        flat[np.flatnonzero(capture["pixel_map"].reshape(-1) == f)[0]] = f
    want = brdf_amd.fit_capture(MODEL, _dev(gpu, capture["images"]), _dev(gpu, pixel_map), _dev(gpu, capture["vertices"]), _dev(gpu, capture["faces"]),
                                _dev(gpu, capture["nrm"]), capture["leds"], capture["view"], rv_mode=1, p0=P0, lb=LB, ub=UB, opts=OPTS, want_stats=True)
    torch.cuda.synchronize()
    got = _faces(gpu, capture, pixel_map=pixel_map)  # the rule switched off
    assert got["n_pixels"] == got["n_faces"] == want[2] == NF - 3
    assert got["surfaces"].tobytes() == want[0].cpu().numpy().tobytes()
    assert got["covar"].tobytes() == want[3].covar.cpu().numpy().tobytes() and got["stats"].tobytes() == want[3].stats.cpu().numpy().tobytes()
    assert got["rank"].tobytes() == want[3].rank.cpu().numpy().tobytes()
    assert np.all(got["count"][:NF - 3] == LIGHTS) and np.all(got["face_pixels"][:NF - 3] == 1) and not got["count"][NF - 3:].any()


def test_grouped_fits_reach_the_cpu_checkers_objective(gpu, masked_capture):
    """every fit's objective and the checker's are printed; the bar is the existing capture tests'"""
    torch, brdf_amd, _ = gpu
    cap = masked_capture
    a, x, off, fit_face, fit_channel, _ = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    got = _faces(gpu, cap, **RULE)
    judged, refused = [0] * 6, 0
    bounds = (16, 64, 256, 1024, 4096)
    for s, (f, ch) in enumerate(zip(fit_face, fit_channel)):
        k = int(off[s + 1] - off[s])
        assert got["count"][f, ch] == k
        if k < 3:  # levmar's n < m refusal
            assert got["ret"][f, ch] == -1 and np.array_equal(got["surfaces"][f, ch], P0) and not got["info"][f, ch].any() and got["rank"][f, ch] == 0
            refused += 1
            continue
        p = got["surfaces"][f, ch]
        assert np.all(np.isfinite(p)) and np.all(p >= np.array(LB)) and np.all(p <= np.array(UB)), (f, ch, k, p)
        a_v, x_v = np.ascontiguousarray(a[3 * off[s]:3 * off[s + 1]].reshape(3, k)), np.ascontiguousarray(x[off[s]:off[s + 1]])
        _, p_ref, _ = L.brdf_fit("orc", 1, MODEL, a_v, x_v, P0, 100, OPTS, LB, UB)
        e_got, e_ref = x_v - L.model_values(MODEL, a_v, p), x_v - L.model_values(MODEL, a_v, p_ref)
        o_got, o_ref = float(e_got @ e_got), float(e_ref @ e_ref)
        print(f"face {f} channel {ch} count {k}: objective {o_got:.6e} oracle {o_ref:.6e}")
        assert o_got <= o_ref * (1 + 1e-3) + 1e-20, (f, ch, k, p, p_ref, o_got, o_ref)
        judged[sum(k > b for b in bounds)] += 1
    print("judged per size class:", judged, "refused:", refused)
    assert all(j >= 1 for j in judged) and refused >= 1, (judged, refused)
    assert sum(judged) + refused == len(fit_face) == 3 * (NF - 3)  # no carried (face, channel) was skipped


def test_nothing_but_the_definition_shows(gpu, capture):
    torch, brdf_amd, _ = gpu
    first = _faces(gpu, capture, **RULE)
    again = _faces(gpu, capture, **RULE)
    # a workspace of one byte holds one fit: as many chunks as fits in every class
    small = _faces(gpu, capture, workspace_bytes=1, **RULE)
    chunks = brdf_amd.last_packed_stats()
    assert all(c["chunks"] == c["fits"] for c in chunks) and sum(c["fits"] > 1 for c in chunks[:5]) >= 3, chunks
    for other in (again, small):
        for name in MAPS + ("avg",):
            assert other[name].tobytes() == first[name].tobytes(), name
        assert (other["n_pixels"], other["n_faces"]) == (first["n_pixels"], first["n_faces"])
    # L = 5: the first five images; t / L with L no divisor of the wavefront
    five = _faces(gpu, capture, images=capture["images"][:5], leds=capture["leds"][:5], **RULE)
    ang5 = L.cosines(capture["vertices"], capture["faces"], capture["nrm"], capture["leds"][:5], capture["view"], rv_mode=1)
    want, _ = _packed(gpu, capture["images"][:5], capture["pixel_map"], ang5, **RULE)
    for name in MAPS:
        assert five[name].tobytes() == want[name].tobytes(), name
    # an all-background map: returns 0 with zeros, writes nothing but the pixel counts
    empty = _faces(gpu, capture, pixel_map=np.full((H, W), -1, dtype=np.int32), out=_sentinel_maps(gpu), **RULE)
    assert empty["n_pixels"] == empty["n_faces"] == 0 and not empty["avg"].any() and not empty["face_pixels"].any()
    for name in MAPS:
        if name != "face_pixels":
            assert np.all(empty[name] == SENTINEL), name
