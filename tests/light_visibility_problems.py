"""Scenes for the cast-shadow tests (tests/test_light_visibility_host.py, tests/test_gpu_light_visibility.py).  Pure NumPy.

The hand-written scenes stand on a floor of two triangles over [0, 6]^2 at z = 0 whose centres, (4, 2, 0) and (2, 4, 0), are exact in
binary; with the light at (3, 3, 8) the ray of face 0 is (4, 2, 0) + t (-1, 1, 8) and passes (3.5, 2.5) at z = 4, that of face 1 passes
(2.5, 3.5).  Every coordinate is dyadic, so every operation of the hit test on these rays is exact and a ray through an edge gives
U = 0, V = 0 or U + V = A exactly."""
import numpy as np

FLOOR_V = [(0.0, 0.0, 0.0), (6.0, 0.0, 0.0), (6.0, 6.0, 0.0), (0.0, 6.0, 0.0)]
FLOOR_F = [(0, 1, 2), (0, 2, 3)]
LIGHT = (3.0, 3.0, 8.0)


def floor_with(triangle, faces=None):
    """the floor and one more face, the blocker: (vertices [7,3], faces [3,3] int32)"""
    return np.array(FLOOR_V + list(triangle), dtype=np.float64), np.array(FLOOR_F + [faces or (4, 5, 6)], dtype=np.int32)


def grid(n=4):
    """n x n unit quads at z = 0, two triangles each, counter-clockwise seen from above: (vertices, faces)"""
    v = np.array([(float(i), float(j), 0.0) for j in range(n + 1) for i in range(n + 1)])
    at = lambda i, j: j * (n + 1) + i
    f = [t for j in range(n) for i in range(n) for t in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    return v, np.array(f, dtype=np.int32)


def hand_scenes():
    """name -> (vertices, faces, leds, with_normals, expected lit word per face as a Python int (bit l = light l), expected stats)"""
    nan = float("nan")
    gv, gf = grid(4)
    tilted = np.array([(0.0, 0.0, 0.0), (3.0, 1.0, 2.0), (1.0, 3.0, 1.0)])  # normal (-5, -1, 8)
    far = [(-20.0 - l, 2.0, 8.0) for l in range(63)]  # from these the blocker is nowhere near a floor centre's ray
    s = {
        # the ray of face 0 passes the blocker's interior at (3.5, 2.5, 4), that of face 1 misses it; nothing is above the blocker
        "blocker": (*floor_with([(3.0, 2.0, 4.0), (5.0, 2.0, 4.0), (3.0, 4.0, 4.0)]), [LIGHT], False, [0, 1, 1], [3, 0, 0, 2, 1]),
        # the same triangle where face 0's ray arrives at t = 1.5, beyond the light
        "beyond_the_light": (*floor_with([(2.0, 3.0, 12.0), (4.0, 3.0, 12.0), (2.0, 5.0, 12.0)]), [LIGHT], False, [1, 1, 1], [3, 0, 0, 3, 0]),
        # ... and at t = -0.5, behind the origin: the floor is lit; the blocker, now under the floor, is shadowed by face 0
        "behind_the_origin": (*floor_with([(4.0, 1.0, -4.0), (6.0, 1.0, -4.0), (4.0, 3.0, -4.0)]), [LIGHT], False, [1, 1, 0], [3, 0, 0, 2, 1]),
        # (3.5, 2.5) on the blocker's edge v0-v2 (U = 0), at its corner v0 (U = V = 0), on its hypotenuse (U + V = A; face 1's ray
        # meets the corner v2 of that one): edges are inclusive
        "edge": (*floor_with([(3.5, 2.0, 4.0), (5.5, 2.0, 4.0), (3.5, 4.0, 4.0)]), [LIGHT], False, [0, 1, 1], [3, 0, 0, 2, 1]),
        "corner": (*floor_with([(3.5, 2.5, 4.0), (5.5, 2.5, 4.0), (3.5, 4.5, 4.0)]), [LIGHT], False, [0, 1, 1], [3, 0, 0, 2, 1]),
        "hypotenuse": (*floor_with([(2.5, 1.5, 4.0), (4.5, 1.5, 4.0), (2.5, 3.5, 4.0)]), [LIGHT], False, [0, 0, 1], [3, 0, 0, 1, 2]),
        # the light straight above face 0's centre and a blocker in the plane x = 4 that holds the ray: a = 0, a miss
        "parallel": (*floor_with([(4.0, 1.0, 2.0), (4.0, 3.0, 2.0), (4.0, 2.0, 6.0)]), [(4.0, 2.0, 8.0)], False, [1, 1, 1], [3, 0, 0, 3, 0]),
        # coplanar neighbours: T = 0 exactly
        "grid_above": (gv, gf, [(1.25, 2.5, 5.0)], True, [1] * 32, [32, 0, 0, 32, 0]),
        "grid_below_with_normals": (gv, gf, [(1.25, 2.5, -5.0)], True, [0] * 32, [32, 0, 32, 0, 0]),
        "grid_below_without_normals": (gv, gf, [(1.25, 2.5, -5.0)], False, [1] * 32, [32, 0, 0, 32, 0]),
        # three times the point (3.5, 2.5, 4) on face 0's ray: e1 = e2 = 0, A = 0
        "degenerate_occluder": (*floor_with([(3.5, 2.5, 4.0)] * 3), [LIGHT], False, [1, 1, 1], [3, 0, 0, 3, 0]),
        # the blocker of the first scene made invalid: lit = 0, and it occludes nothing
        "nan_vertex": (*floor_with([(3.0, 2.0, 4.0), (5.0, nan, 4.0), (3.0, 4.0, 4.0)]), [LIGHT], False, [1, 1, 0], [2, 1, 0, 2, 0]),
        "bad_index": (*floor_with([(3.0, 2.0, 4.0), (5.0, 2.0, 4.0), (3.0, 4.0, 4.0)], faces=(4, 5, 7)), [LIGHT], False, [1, 1, 0], [2, 1, 0, 2, 0]),
        # two copies of one tilted face, the light on the side of its normal: each centre lies in the other's plane, T is rounding noise
        "coincident": (tilted, np.array([(0, 1, 2), (0, 1, 2)], dtype=np.int32), [(-3.0, 0.5, 9.0)], True, [1, 1], [2, 0, 0, 2, 0]),
        # 64 lights, the last one the first scene's: only bit 63 of face 0 is clear
        "sixty_four_lights": (*floor_with([(3.0, 2.0, 4.0), (5.0, 2.0, 4.0), (3.0, 4.0, 4.0)]), far + [LIGHT], False,
                              [2 ** 63 - 1, 2 ** 64 - 1, 2 ** 64 - 1], [3, 0, 0, 191, 1]),
    }
    return s


def words(expected):
    """Python ints (unsigned bit patterns) -> the int64 array that carries them"""
    return np.array(expected, dtype=np.uint64).view(np.int64)


def scene_normals(vertices, faces):
    import brdf_amd
    return brdf_amd.face_normals_host(vertices, faces)


# ---- the random scene ------------------------------------------------------------------------------------------------------------------
def random_scene(nf, L=16, seed=7):
    """A jittered floor grid over [-1, 1]^2 near z = 0 with floating blocker quads above it: exactly nf faces, about a fifth of them
    blockers (none below 10 faces), all counter-clockwise seen from above; L lights, four of five above the scene and every fifth below
    it.  The quads' side shrinks with their number so that about half of the floor lies in some shadow.  (vertices, faces, leds)"""
    rng = np.random.default_rng(seed)
    n_block = 2 * (nf // 10)
    n_floor = nf - n_block
    g = max(1, int(np.ceil(np.sqrt(n_floor / 2.0))))
    x = np.linspace(-1.0, 1.0, g + 1)
    gx, gy = np.meshgrid(x, x)
    v = np.stack([gx, gy, np.zeros_like(gx)], axis=2).reshape(-1, 3)
    v += rng.uniform(-1.0, 1.0, size=v.shape) * [0.5 / g, 0.5 / g, 0.02]
    at = lambda i, j: j * (g + 1) + i
    f = [t for j in range(g) for i in range(g) for t in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))][:n_floor]
    quads = n_block // 2
    if quads:
        side = np.sqrt(2.8 / quads)
        c = np.concatenate([rng.uniform(-1.0, 1.0, size=(quads, 2)), rng.uniform(0.3, 0.8, size=(quads, 1))], axis=1)
        corners = np.array([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)]) * side
        qv = (c[:, None, :] + corners[None] + rng.uniform(-0.05, 0.05, size=(quads, 4, 3)) * side).reshape(-1, 3)
        base = v.shape[0] + 4 * np.arange(quads)
        f += [t for b in base for t in ((b, b + 1, b + 2), (b, b + 2, b + 3))]
        v = np.concatenate([v, qv])
    ang = rng.uniform(0.0, 2.0 * np.pi, size=L)
    r = rng.uniform(0.2, 1.5, size=L)
    z = np.where(np.arange(L) % 5 == 4, -2.0, rng.uniform(2.0, 3.0, size=L))
    leds = np.stack([r * np.cos(ang), r * np.sin(ang), z], axis=1)
    faces = np.array(f, dtype=np.int32).reshape(-1, 3)
    assert faces.shape[0] == nf
    return v, faces, leds


def shadowed_share(stats):
    """the shadowed share of the pairs that do not face away"""
    return stats[4] / float(stats[3] + stats[4])


def spoil(vertices, faces):
    """the scene with a NaN vertex, an infinite one and two faces with an index outside [0, nv): invalid faces among valid ones"""
    v, f = vertices.copy(), faces.copy()
    v[f[3, 1], 2] = np.nan
    v[f[f.shape[0] - 2, 0], 0] = np.inf
    f[5, 2] = v.shape[0]
    f[f.shape[0] // 2, 0] = -1
    return v, f


# ---- painting ----------------------------------------------------------------------------------------------------------------------------
def paint_case(L, H, W, nf, seed=3):
    """random images [L,H,W,3], a map with entries from -2 to nf + 1 and random words: (images, pixel_map int32, face_lit int64)"""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(L, H, W, 3), dtype=np.uint8)
    pm = rng.integers(-2, nf + 2, size=(H, W)).astype(np.int32)
    lit = rng.integers(0, 2 ** 64, size=nf, dtype=np.uint64).view(np.int64)  # all 64 bits
    return images, pm, lit
