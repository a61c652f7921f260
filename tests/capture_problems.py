"""Captures for the kernels on either side of the fit -- cosines, pixel compaction, face grouping, validity rule, pack and scatter
(cosines.hip, capture_fit.hip, capture_faces.hip) -- at the shapes the 23 x 31, 40-face Blinn-Phong fixture never reaches.  Pure
NumPy plus the C oracle's cosine planes, no device; tests/test_capture_problems.py asserts on the CPU what the GPU tests rest on.

  rule_capture(model)    the mesh, renderer and map of tests/test_gpu_capture_faces.py::make_faces_capture seen from (0, -80, -600):
                         over its 37 touched faces x 16 lights the rule `1, 254, 0.0` rejects 119 candidates by plane 1 alone, 112 by
                         plane 2 alone, 110 by both, 14 by plane 0, and 237 pass: which planes a model reads shows in every count.
                         nan_face=True: one carried face has a NaN normal, so all its cosines are NaN.  lights: the same capture
                         under leds_for(lights).
  big_capture()          67 x 73 pixels, 70,001 faces, 644 of them carried (0, 65,535, 65,536 and nf - 1 among them) by 4,500 pixels,
                         one face by 300; 40 pixels name face nf and 40 face -5 (background).  72,000 candidates per channel are 282
                         pack blocks, 1,932 fits are 8 scatter blocks: every one-workgroup scan has threads that own two items.
  wide_capture(L, H, W)  every pixel carries one of 300 faces: at (16, 300, 300) and (64, 150, 150) the gather, the rows kernel and
                         the one-lane-per-(surfel, light) kernel all wrap their grid-stride loops.

The captures are cached: callers must not write into what they get."""
import functools

import numpy as np

from tests import oracle_libs as L

OPTS = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)
P0, LB, UB = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0)
RULE = dict(v_min=1, v_max=254, cos_min=0.0)
RULE_VIEW = np.array([0.0, -80.0, -600.0])
RULE_COUNTS = dict(plane1=119, plane2=112, both=110, plane0=14, passed=237)  # over the touched faces x 16 lights
READS = {0: (True, False, True), 1: (True, True, False), 2: (True, True, True)}  # the planes a model reads (brdf_models.h)
KCT = 256  # the capture kernels' workgroup (capture_compact.h: kCT)
GATHER_CAP = 256 * 64 * KCT  # elements one trip of gather_kernel's grid covers
PACKED_BOUNDS = (16, 64, 256, 1024, 4096)


def leds_for(lights):
    """the rig's first `lights` LEDs; above 16: the rig plus positions drawn near its LEDs"""
    table = L.led_table()
    if lights <= 16:
        return np.ascontiguousarray(table[:lights])
    rng = np.random.default_rng(lights)
    extra = table[rng.integers(0, 16, size=lights - 16)] + rng.uniform(-15.0, 15.0, size=(lights - 16, 3))
    return np.ascontiguousarray(np.concatenate([table, extra]))


def face_values(model, ang):
    """what the renderer of the existing fixtures draws for faces with planes ang [F,3,L], before gain and quantisation: [F,3,L] per
    channel, the model at |cosines| with truth * (0.6 + 0.2 channel), times 255 / 2"""
    from brdf_amd import synth
    a = np.abs(ang)
    out = np.empty((ang.shape[0], 3, ang.shape[2]))
    with np.errstate(all="ignore"):
        for ch in range(3):
            out[:, ch, :] = synth.model_value(model, np.array(synth.TRUTH[model]) * (0.6 + 0.2 * ch), a[:, 0], a[:, 1], a[:, 2])
    return out * (255.0 * 0.5)


def paint(values, row_of_pixel, gain):
    """images [L,H,W,3]: pixel (y, x) with row_of_pixel[y, x] = r >= 0 shows values[r] * gain[y, x], rounded and clipped to 8 bits,
    in image row H-1-y; the other pixels stay black"""
    H, W = row_of_pixel.shape
    images = np.zeros((values.shape[2], H, W, 3), dtype=np.uint8)
    ys, xs = np.nonzero(row_of_pixel >= 0)
    v = values[row_of_pixel[ys, xs]] * gain[ys, xs, None, None]  # [P,3,L]
    v = np.clip(np.round(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255).astype(np.uint8)
    images[:, H - 1 - ys, xs, :] = v.transpose(2, 0, 1)
    return images


def walk(pixel_map, nf):
    """the reference's walk (x outer, y inner) over the pixels that carry a face: (g = x * H + y of each, its face), in walk order"""
    flat = np.asarray(pixel_map).T.reshape(-1)
    g = np.flatnonzero((flat > -1) & (flat < nf))
    return g, flat[g].astype(np.int64)


def pixel_values(images, g):
    """the 8-bit intensities of the pixels g = x * H + y: [P,3,L] (channel, light)"""
    H = images.shape[1]
    return images[:, H - 1 - g % H, g // H, :].astype(np.int64).transpose(1, 2, 0)


def rule_valid(model, values, planes, v_min=0, v_max=255, cos_min=-2.0):
    """the validity rule in NumPy: values [P,3,L] (channel, light), planes [P,3,L] (plane, light) -> valid [P,3,L] (channel, light).
    A NaN cosine compares false: not valid."""
    cos_ok = np.ones(planes.shape[0::2], dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in range(3):
            if READS[model][k]:
                cos_ok &= planes[:, k, :] > cos_min
    return (values >= v_min) & (values <= v_max) & cos_ok[:, None, :]


def last_pixels(pixel_map, nf):
    """(faces that some pixel carries, ascending; the place in the walk of each one's LAST pixel)"""
    _, face = walk(pixel_map, nf)
    last = np.full(nf, -1, dtype=np.int64)
    last[face] = np.arange(face.size)  # (ascending places: the last assignment stays)
    carried = np.flatnonzero(last >= 0)
    return carried, last[carried]


@functools.lru_cache(maxsize=None)
def _faces_base():
    from tests.test_gpu_capture_faces import make_faces_capture
    return make_faces_capture()


@functools.lru_cache(maxsize=None)
def rule_capture(model, nan_face=False, lights=16):
    base = _faces_base()
    vertices, faces, nrm, leds, pixel_map = base["vertices"], base["faces"], base["nrm"], leds_for(lights), base["pixel_map"]
    ang = L.cosines(vertices, faces, nrm, leds, RULE_VIEW, rv_mode=1)  # signed planes
    gain = np.random.default_rng(23).uniform(0.8, 1.2, size=pixel_map.shape)
    images = paint(face_values(model, ang), pixel_map, gain)
    cap = dict(vertices=vertices, faces=faces, nrm=nrm, view=RULE_VIEW, leds=leds, pixel_map=pixel_map, images=images, ang=ang, model=model,
               nf=faces.shape[0])
    if nan_face:  # the images are those of the sound mesh: only the geometry of one face is lost
        f = base["class_faces"][3]  # ten pixels
        nrm = nrm.copy()
        nrm[f] = np.nan
        without = pixel_map.copy()
        without[pixel_map == f] = -1
        cap.update(nrm=nrm, ang=L.cosines(vertices, faces, nrm, leds, RULE_VIEW, rv_mode=1), nan_face=f, pixel_map_without=without)
    return cap


def rule_categories(ang):
    """how the rule `cos_min = 0` sees candidates with planes ang [F,3,L]: five disjoint masks [F,L]"""
    ok = ang > 0.0
    p0 = ~ok[:, 0]
    return dict(plane0=p0, plane1=~p0 & ~ok[:, 1] & ok[:, 2], plane2=~p0 & ok[:, 1] & ~ok[:, 2], both=~p0 & ~ok[:, 1] & ~ok[:, 2],
                passed=ok[:, 0] & ok[:, 1] & ok[:, 2])


@functools.lru_cache(maxsize=None)
def big_capture():
    H, W, nf, nv, lights, n_carried, n_pixels, big = 67, 73, 70001, 4000, 16, 644, 4500, 300
    rng = np.random.default_rng(41)
    vertices = rng.uniform(-80.0, 80.0, size=(nv, 3)) + np.array([0.0, -80.0, 60.0])
    i0 = rng.integers(0, nv, size=nf)
    i1 = (i0 + rng.integers(1, nv, size=nf)) % nv
    i2 = rng.integers(0, nv - 2, size=nf)  # the third index among the nv - 2 that are left
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    faces = np.stack([i0, i1, i2], axis=1).astype(np.int32)
    nrm = np.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)  # as they come: about half the faces look away from the rig
    view, leds = np.array([310.0, -75.0, 700.0]), L.led_table()
    must = np.array([0, 65535, 65536, nf - 1])
    carried = np.sort(np.concatenate([must, rng.choice(np.setdiff1d(np.arange(nf), must), size=n_carried - must.size, replace=False)]))
    ang_c = L.cosines(vertices, faces, nrm, leds, view, surfels=carried.astype(np.int32), rv_mode=1)
    values = face_values(1, ang_c)
    # the face of 300 pixels: every plane positive at every light and every value inside [1, 254] at any gain, so that under the rule
    # all 4800 candidates are samples in every model
    bright = np.flatnonzero((ang_c > 0.0).all(axis=(1, 2)) & (values.min(axis=(1, 2)) * 0.8 >= 1.5) & (values.max(axis=(1, 2)) * 1.2 <= 253.5))
    big_row = int(bright[0])
    sizes = np.ones(n_carried, dtype=np.int64)
    sizes[big_row] = big
    rest = np.flatnonzero(np.arange(n_carried) != big_row)
    weight = rng.pareto(1.2, size=rest.size) + 0.05  # a few faces of tens of pixels among many of one or two
    sizes[rest] += rng.multinomial(n_pixels - big - rest.size, weight / weight.sum())
    perm = rng.permutation(H * W)
    flat = np.full(H * W, -1, dtype=np.int32)
    flat[perm[:n_pixels]] = np.repeat(carried, sizes)
    flat[perm[n_pixels:n_pixels + 40]] = nf  # outside [-1, nf): background to the kernels, refused by the wrappers' validation
    flat[perm[n_pixels + 40:n_pixels + 80]] = -5
    pixel_map = flat.reshape(H, W)
    gain = rng.uniform(0.8, 1.2, size=(H, W))
    inside = (pixel_map > -1) & (pixel_map < nf)
    row_of_pixel = np.where(inside, np.searchsorted(carried, np.where(inside, pixel_map, 0)), -1)
    images = paint(values, row_of_pixel, gain)
    ang = np.zeros((nf, 3, lights))  # the host twin reads the carried faces' rows only
    ang[carried] = ang_c
    return dict(vertices=vertices, faces=faces, nrm=nrm, view=view, leds=leds, pixel_map=pixel_map, images=images, ang=ang, nf=nf,
                carried=carried, sizes=sizes, big_face=int(carried[big_row]))


@functools.lru_cache(maxsize=None)
def wide_capture(lights, H, W):
    from tests.test_cosines import make_mesh
    nf = 300
    vertices, faces, nrm, view = make_mesh(nv=200, nf=nf, seed=29)
    leds = leds_for(lights)
    c = vertices[faces].sum(axis=1) / 3.0
    nrm[((leds[:16].mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0] *= -1.0
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)
    rng = np.random.default_rng(1000 * lights + H)
    pixel_map = rng.integers(0, nf, size=(H, W)).astype(np.int32)
    gain = rng.uniform(0.8, 1.2, size=(H, W))
    images = paint(face_values(1, ang), pixel_map.astype(np.int64), gain)  # per face, indexed by the map
    return dict(vertices=vertices, faces=faces, nrm=nrm, view=view, leds=leds, pixel_map=pixel_map, images=images, ang=ang, nf=nf)
