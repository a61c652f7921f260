"""Meshes and cameras for the pixel-map tests (tests/test_pixel_map_host.py, tests/test_gpu_pixel_map.py).  Pure NumPy.

The hand-written cases live in window space: identity model_view and projection, an 8 x 8 viewport, dyadic coordinates -- every
operation of the projection and of the edge functions is exact, so the expected maps can be written down."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL_DIR = os.path.join(ROOT, "tests", "golden", "cal")
IDENTITY = np.eye(4).reshape(-1)
N = 8  # the hand-written cases' viewport is N x N
VIEWPORT = (0.0, 0.0, float(N), float(N))


def from_window(points):
    """[n,3] window coordinates (x, y in pixels of the N x N viewport, z in [0, 1]) -> the object coordinates that project there under
    identity matrices: win = (v * 0.5 + 0.5) * N, exact for dyadic values"""
    w = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.stack([w[:, 0] / (N / 2) - 1.0, w[:, 1] / (N / 2) - 1.0, 2.0 * w[:, 2] - 1.0], axis=1)


def window_mesh(triangles):
    """triangles: per face three window-space points (x, y, z) -> (vertices [3 nf, 3], faces [nf, 3] int32), no vertex shared"""
    t = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    return from_window(t.reshape(-1, 3)), np.arange(3 * t.shape[0], dtype=np.int32).reshape(-1, 3)


def tri(ax, ay, bx, by, cx, cy, z=0.5):
    return [(ax, ay, z), (bx, by, z), (cx, cy, z)]


# name -> (triangles in window space, keyword arguments, expected map as a function of (col, row) or None where the test says more)
def hand_cases():
    big = tri(1, 1, 7, 1, 1, 7)             # centres with col, row >= 1 and col + row <= 7; col + row = 7 lies ON the hypotenuse
    edge = tri(0.5, 0.5, 4.5, 0.5, 0.5, 4.5)  # both legs run through centres: col + row <= 4
    quad = [tri(1, 1, 7, 1, 7, 7), tri(1, 1, 7, 7, 1, 7)]  # the diagonal's centres are on the shared edge: equal depth, face 0
    inside = lambda c, r: 1 <= c <= 6 and 1 <= r <= 6
    return {
        "one_triangle": ([big], {}, lambda c, r: 0 if c >= 1 and r >= 1 and c + r <= 7 else -1),
        "centres_on_edges": ([edge], {}, lambda c, r: 0 if c + r <= 4 else -1),
        "quad": (quad, {}, lambda c, r: (0 if r <= c else 1) if inside(c, r) else -1),
        "nearer_over_farther": ([tri(1, 1, 7, 1, 1, 7, z=0.75), tri(1, 1, 7, 1, 1, 7, z=0.25)], {},
                                lambda c, r: 1 if c >= 1 and r >= 1 and c + r <= 7 else -1),
        "identical": ([big, big], {}, lambda c, r: 0 if c >= 1 and r >= 1 and c + r <= 7 else -1),
        "clockwise_kept": ([tri(1, 1, 1, 7, 7, 1)], dict(cull=0), lambda c, r: 0 if c >= 1 and r >= 1 and c + r <= 7 else -1),
        "clockwise_culled": ([tri(1, 1, 1, 7, 7, 1)], dict(cull=1), lambda c, r: -1),
        "counter_clockwise_under_cull": ([big], dict(cull=1), lambda c, r: 0 if c >= 1 and r >= 1 and c + r <= 7 else -1),
    }


def expected_map(rule):
    return np.array([[rule(c, r) for c in range(N)] for r in range(N)], dtype=np.int32)


def point_face(x, y, z=0.5):
    """a face whose three vertices are one point: mode 0's centroid ((a + b) + c) / 3.0 is that point, exactly"""
    return [(x, y, z)] * 3


def centroid_case():
    """mode 0: faces 0, 1, 2 share pixel (2, 3); face 3 has winX in (-1, 0): rejected; face 4 has (int)winX = N: refused and counted;
    face 5 alone in pixel (7, 0); face 6 has (int)winY = N: refused"""
    tris = [point_face(2.25, 3.5, 0.25), point_face(2.5, 3.25, 0.5), point_face(2.75, 3.75, 0.75), point_face(-0.5, 3.0), point_face(8.0, 3.0),
            point_face(7.5, 0.5, 0.125), point_face(1.0, 8.5)]
    want = np.full((N, N), -1, dtype=np.int32)
    want[3, 2], want[0, 7] = 2, 5
    depth = np.full((N, N), 2.0)
    depth[3, 2], depth[0, 7] = 0.75, 0.125
    stats = np.array([4, 0, 0, 0, 1, 0, 2, 2])
    return tris, want, depth, stats


# ---- the shapes the hand-written cases do not reach -------------------------------------------------------------------------------------
def perspective_scene(n_small=70001, seed=11):
    """A full-viewport pair of triangles behind n_small small random faces, seen through gl_frustum / gl_look_at: (vertices, faces,
    model_view, projection).  Some small faces reach past the viewport's border, a few are degenerate (a repeated vertex)."""
    import brdf_amd
    rng = np.random.default_rng(seed)
    mv = brdf_amd.gl_look_at((0.3, -0.2, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    pr = brdf_amd.gl_frustum(-0.5, 0.5, -0.5, 0.5, 1.0, 20.0)
    back = np.array([[-8.0, -8.0, -3.0], [8.0, -8.0, -3.0], [8.0, 8.0, -3.0], [-8.0, 8.0, -3.0]])
    centre = rng.uniform(-3.2, 3.2, size=(n_small, 1, 3)) * [1.0, 1.0, 0.3]
    small = (centre + rng.uniform(-0.04, 0.04, size=(n_small, 3, 3))).reshape(-1, 3)
    vertices = np.concatenate([back, small])
    faces = np.concatenate([[[0, 1, 2], [0, 2, 3]], 4 + np.arange(3 * n_small).reshape(-1, 3)]).astype(np.int32)
    faces[5::1000, 2] = faces[5::1000, 1]  # degenerate: zero area
    return vertices, faces, mv, pr


def trouble_mesh():
    """In the N x N window (identity matrices): 0 partly outside, 1 wholly outside, 2 beyond z = 1, 3 a NaN vertex, 4 an index outside
    [0, nv), 5 plain and behind 0 where they overlap; then, for a perspective camera, see test: behind the eye"""
    tris = [tri(-3, 2, 5, 2, 1, 6, z=0.25), tri(9, 9, 12, 9, 9, 12), tri(1, 1, 3, 1, 1, 3, z=1.5), tri(4, 4, 6, 4, 4, 6), tri(0, 0, 1, 0, 0, 1),
            tri(0, 0, 8, 0, 0, 8, z=0.5)]
    vertices, faces = window_mesh(tris)
    vertices[3 * 3 + 1, 1] = np.nan
    faces[4, 2] = vertices.shape[0] + 7
    return vertices, faces


def sphere(rings=32, segments=32, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a latitude-longitude sphere: 2 * segments * (rings - 1) faces, wound counter-clockwise seen from outside"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, rings):
        t = np.pi * i / rings
        v += [(np.sin(t) * np.cos(2 * np.pi * j / segments), np.sin(t) * np.sin(2 * np.pi * j / segments), np.cos(t)) for j in range(segments)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * segments + j % segments
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(segments)]
    for i in range(1, rings - 1):
        for j in range(segments):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    f += [(len(v) - 1, ring(rings - 1, j + 1), ring(rings - 1, j)) for j in range(segments)]
    return np.asarray(v) * radius + np.asarray(centre), np.asarray(f, dtype=np.int32)


def cal_files():
    return sorted(f for f in os.listdir(CAL_DIR) if f.endswith(".cal"))


def read_cal(name):
    import brdf_amd
    with open(os.path.join(CAL_DIR, name)) as fh:
        return brdf_amd.parse_cal(fh.read())
