"""K materials per object (brdf_hip_fit_capture_materials_dev): the planted capture the host and the GPU tests share, and Lloyd's
iteration as NumPy code around a CPU solver.  Pure NumPy plus the oracle's cosines and model values, no device.

  planted_capture()   Blinn-Phong, 80 faces of 3 ... 29 pixels under 16 lights, 4 planted materials (kd, ks in U[0.1, 0.9], n in
                      U[2, 62] per channel, synth's truth ranges, at the renderers' gain 1/2), sigma = 0.02 noise, 8 bits.  The
                      lights are a 4 x 4 grid 900 wide above the object and every face's normal leans towards the half vector of one
                      of them, so that a face's 16 cosines cross its lobe: under the project's rig, a panel 160 wide 600 away, they
                      span a few degrees and a per-face fit -- the seeds -- is not determined.
  host_seeds(...)     the seeding rule of brdf_amd.seed_materials with a CPU solver: seed 0 the single fit, seed j the per-face fit of
                      the face with the largest per-sample residual against its nearest current seed, a face once at most
  host_loop(...)      assign / settle or stop / refit, exactly as the device entry defines them, the fits by the compiled reference's
                      dlevmar_bc_dif ("ref") or the oracle's ("orc")

The captures are cached: callers must not write into what they get."""
import functools

import numpy as np

from tests import capture_problems as P
from tests import oracle_libs as L

MODEL = 1
K_PLANTED = 4
RULE = P.RULE
MIN_COUNT = 16


def solver():
    """the compiled reference where it was built, the oracle's restatement otherwise"""
    return "ref" if L.ref is not None else "orc"


@functools.lru_cache(maxsize=None)
def planted_capture(nf=80, K=K_PLANTED, lights=16, seed=14):
    from brdf_amd import synth
    from tests.test_cosines import make_mesh
    rng = np.random.default_rng(seed)
    vertices, faces, _, view = make_mesh(nv=60, nf=nf, seed=seed)
    side = int(round(np.sqrt(lights)))
    assert side * side == lights
    gx, gy = np.meshgrid(np.linspace(-450.0, 450.0, side), np.linspace(-450.0, 450.0, side))
    leds = np.ascontiguousarray(np.stack([gx.reshape(-1) - 10.0, gy.reshape(-1) - 87.0, np.full(lights, 560.0)], axis=1))  # a wide rig
    c = vertices[faces].sum(axis=1) / 3.0
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    half = unit(unit(leds[rng.integers(0, lights, size=nf)] - c) + unit(view[None, :] - c))
    nrm = unit(half + rng.normal(0.0, 0.12, size=(nf, 3)))
    ang = L.cosines(vertices, faces, nrm, leds, view, rv_mode=1)
    truth = np.stack([rng.uniform(0.1, 0.9, size=(K, 3)), rng.uniform(0.1, 0.9, size=(K, 3)), rng.uniform(2.0, 62.0, size=(K, 3))], axis=2)
    truth[:, :, :2] *= 0.5  # the renderers' gain: every value stays below 1
    planted = rng.permutation(np.arange(nf) % K).astype(np.int32)
    sizes = rng.integers(3, 30, size=nf)
    H, W = 48, 64
    flat = np.full(H * W, -1, dtype=np.int32)
    flat[rng.permutation(H * W)[:int(sizes.sum())]] = np.repeat(np.arange(nf, dtype=np.int32), sizes)
    pixel_map = flat.reshape(H, W)
    a = np.abs(ang)
    clean = np.empty((nf, 3, lights))
    with np.errstate(all="ignore"):
        for ch in range(3):
            p = truth[planted, ch]  # [nf,3]
            clean[:, ch, :] = synth.model_value(MODEL, (p[:, 0:1], p[:, 1:2], p[:, 2:3]), a[:, 0], a[:, 1], a[:, 2])
    images = np.zeros((lights, H, W, 3), dtype=np.uint8)
    ys, xs = np.nonzero(pixel_map >= 0)
    v = clean[pixel_map[ys, xs]] + rng.normal(0.0, 0.02, size=(ys.size, 3, lights))
    images[:, H - 1 - ys, xs, :] = np.clip(np.round(255.0 * v), 0, 255).astype(np.uint8).transpose(2, 0, 1)
    return dict(vertices=vertices, faces=faces, nrm=nrm, view=view, leds=leds, pixel_map=pixel_map, images=images, ang=ang, nf=nf, model=MODEL,
                truth=truth, planted=planted, sizes=sizes)


@functools.lru_cache(maxsize=None)
def face_samples(nf=80):
    """(per carried face and channel (planes [3,k], x [k]), the carried faces) of planted_capture under RULE"""
    import brdf_amd
    cap = planted_capture(nf=nf)
    a, x, off, fit_face, _, _ = brdf_amd.group_capture_samples(cap["images"], cap["pixel_map"], cap["ang"], MODEL, **RULE)
    sets = {}
    for s in range(len(fit_face)):
        k = int(off[s + 1] - off[s])
        sets[(int(fit_face[s]), s % 3)] = (a[3 * off[s]:3 * off[s + 1]].reshape(3, k), x[off[s]:off[s + 1]])
    return sets, np.unique(fit_face).astype(np.int64)


def label_set(sets, faces, c):
    """the sample set of the faces `faces` (ascending) in channel c, one face behind the other"""
    planes = [np.zeros((3, 0))] + [sets[(int(f), c)][0] for f in faces]
    xs = [np.zeros(0)] + [sets[(int(f), c)][1] for f in faces]
    return np.ascontiguousarray(np.concatenate(planes, axis=1)), np.ascontiguousarray(np.concatenate(xs))


def face_sumsq(sets, carried, nf, materials):
    """[nf,K,3]: every carried face's sum of squared residuals against every material, by the oracle's model values"""
    K = materials.shape[0]
    out = np.zeros((nf, K, 3))
    with np.errstate(all="ignore"):
        for c in range(3):
            planes, x = label_set(sets, carried, c)
            starts = np.cumsum([0] + [sets[(int(f), c)][1].size for f in carried])
            for k in range(K):
                e = x - L.model_values(MODEL, planes, materials[k, c])
                for r, f in enumerate(carried):
                    seg = e[starts[r]:starts[r + 1]]
                    out[f, k, c] = float(seg @ seg)
    return out


def host_fit(which, planes, x, p0, itmax=100, sign=None):
    """(ret, p, info): the solver's dlevmar_bc_dif; fewer than 3 samples: refused, p0 kept.  sign [k] of -1 / +1: every model value
    the solver sees is moved by that many ulp (the reference's "+-1 ulp twin": what a last-bit difference in the model does to a fit)"""
    if x.size < 3:
        return -1, np.array(p0, dtype=np.float64), np.zeros(10)
    if sign is None:
        return L.brdf_fit(which, 1, MODEL, planes, x, p0, itmax, P.OPTS, P.LB, P.UB)
    import ctypes as C
    from tests import stats_yardstick as Y
    from tests import weighted_yardstick as WY
    a, xx = L.f64(planes), L.f64(x)
    ed = Y._Extra(L.ptr(a), MODEL)

    def func(pp, hx, m, nn, adata):
        L.orc.orc_brdf_func(pp, hx, m, nn, C.c_void_p(adata))
        out = np.ctypeslib.as_array(hx, shape=(nn,))
        out[:] = np.nextafter(out, sign * np.inf)

    cb = WY._FUNC(func)
    p, info = L.f64(p0).copy(), np.zeros(10)
    r = WY._BC_DIF(cb, L.ptr(p), L.ptr(xx), 3, xx.size, L.ptr(L.f64(P.LB)), L.ptr(L.f64(P.UB)), None, itmax, L.ptr(L.f64(P.OPTS)), L.ptr(info), None,
                   None, C.byref(ed))
    return int(r), p, info


def host_seeds(which, K, nf=80, min_count=MIN_COUNT):
    """brdf_amd.seed_materials' rule with the CPU solver: ([K,3,3] seeds, the faces seeds 1 ... K-1 come from).  A face's three fits run
    when its turn comes -- the faces are tried by descending residual, the lowest index first among equals --, which picks the face the
    rule names without fitting every face"""
    sets, carried = face_samples(nf)
    seeds = [np.stack([host_fit(which, *label_set(sets, carried, c), P.P0)[1] for c in range(3)])]
    fits = {}
    counted = [int(f) for f in carried if all(sets[(int(f), c)][1].size >= min_count for c in range(3))]
    chosen = []
    for _ in range(1, K):
        s = face_sumsq(sets, carried, nf, np.stack(seeds))
        cost = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
        cost = np.where(np.isfinite(cost), cost, np.inf).min(axis=1)
        per = {f: cost[f] / sum(sets[(f, c)][1].size for c in range(3)) for f in counted if np.isfinite(cost[f])}
        for f in sorted((f for f in per if f not in chosen), key=lambda f: (-per[f], f)):
            if f not in fits:
                fits[f] = [host_fit(which, *sets[(f, c)], P.P0) for c in range(3)]
            if all(r[0] >= 0 for r in fits[f]):
                chosen.append(f)
                seeds.append(np.stack([fits[f][c][1] for c in range(3)]))
                break
        else:
            raise AssertionError("no eligible face")
    return np.stack(seeds), chosen


def host_loop(which, seeds, rounds, nf=80, twin_seed=None):
    """Lloyd's iteration as the device entry defines it; twin_seed: the seed of the +-1 ulp perturbation of every fit's model values
    (host_fit).  Returns dict(materials [K,3,3], labels [nf], changed (per assignment),
    rounds_used, settled, info [K,3,10], ret [K,3], face_sumsq [nf,3]: against the face's own material)"""
    import brdf_amd
    sets, carried = face_samples(nf)
    is_carried = np.zeros(nf, dtype=bool)
    is_carried[carried] = True
    materials = np.array(seeds, dtype=np.float64)
    K = materials.shape[0]
    labels = np.full(nf, -1, dtype=np.int32)
    info, ret = np.zeros((K, 3, 10)), np.full((K, 3), -1, dtype=np.int32)
    changed, refits, settled = [], 0, False
    rng = None if twin_seed is None else np.random.default_rng(twin_seed)
    while True:
        labels, n = brdf_amd.assign_materials(face_sumsq(sets, carried, nf, materials), labels, carried=is_carried)
        changed.append(n)
        if n == 0:
            settled = True
            break
        if refits == rounds:
            break
        for k in range(K):
            faces = carried[labels[carried] == k]
            for c in range(3):
                planes, x = label_set(sets, faces, c)
                sign = None if rng is None else np.where(rng.random(x.size) < 0.5, -1.0, 1.0)
                ret[k, c], materials[k, c], info[k, c] = host_fit(which, planes, x, materials[k, c], sign=sign)
        refits += 1
        if refits == rounds:
            break
    s = face_sumsq(sets, carried, nf, materials)
    own = np.zeros((nf, 3))
    for f in carried:
        own[f] = s[f, labels[f]] if labels[f] >= 0 else np.inf
    return dict(materials=materials, labels=labels, changed=changed, rounds_used=refits, settled=settled, info=info, ret=ret, face_sumsq=own)


def purity(labels, planted, K):
    """the share of faces whose label's majority planted material is theirs"""
    labels, planted = np.asarray(labels), np.asarray(planted)
    hit = 0
    for k in range(K):
        mine = planted[labels == k]
        if mine.size:
            hit += int(np.bincount(mine).max())
    return hit / float(labels.size)
