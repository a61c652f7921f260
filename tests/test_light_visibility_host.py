"""Cast shadows (brdf_amd/shadow.py, brdf_amd/csrc/light_visibility.hip), the part that needs no device: the header's declarations;
every refusal of the two entries, each before any HIP call and under the entry's own name; the visibility twin light_visibility_host on
hand-written scenes whose lit bits are worked out by hand (tests/light_visibility_problems.py: dyadic coordinates, exact rays); the
paint twin apply_visibility_host on a 3 x 4 map; and a condition on the random scene the device tests compare bytes on: its shadowed
share lies between 10 % and 90 %, so an all-lit or all-dark answer could not pass them."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import light_visibility_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIS, APPLY = "brdf_hip_light_visibility_dev", "brdf_hip_capture_apply_visibility_dev"
INT_MAX = 2 ** 31 - 1


def test_header_declares_the_two_entries_and_the_package_exports_the_module():
    import brdf_amd
    from brdf_amd._lib import ABI
    text = open(os.path.join(ROOT, "include", "brdf_levmar.h")).read()
    for name in (VIS, APPLY):
        assert f"int {name}(" in text and name in ABI and hasattr(brdf_amd.lib, name)
    for word in ("light_visibility", "light_visibility_host", "apply_visibility", "apply_visibility_host", "lit_matrix"):
        assert callable(getattr(brdf_amd, word)) and getattr(brdf_amd, word) is getattr(brdf_amd.shadow, word)


def test_entries_refuse_bad_arguments_without_a_device(capfd):
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read as device memory: every call below is refused before any HIP call
    ptr = C.c_void_p(buf.ctypes.data)
    stats = np.full(5, -7, dtype=np.int64)
    leds = np.arange(48, dtype=np.float64)

    def vis(vertices=ptr, nv=12, faces=ptr, nf=4, normals=None, leds_=leds, L=16, t_min=1e-9, lit=ptr):
        return lib.brdf_hip_light_visibility_dev(vertices, nv, faces, nf, normals, None if leds_ is None else leds_.ctypes.data_as(D), L, t_min, lit,
                                                 stats.ctypes.data_as(C.POINTER(C.c_longlong)), None)

    def with_entry(i, v):
        a = leds.copy()
        a[i] = v
        return a
    for kw in (dict(vertices=None), dict(faces=None), dict(leds_=None), dict(lit=None), dict(L=0), dict(L=65), dict(L=-1), dict(nf=0), dict(nf=-5),
               dict(nv=0), dict(nf=INT_MAX + 1), dict(nv=INT_MAX + 1), dict(leds_=with_entry(0, np.nan)), dict(leds_=with_entry(47, np.inf)),
               dict(leds_=with_entry(20, -np.inf)), dict(t_min=-1e-12), dict(t_min=0.5), dict(t_min=np.nan), dict(t_min=np.inf)):
        assert vis(**kw) == -1, kw
        assert VIS + "()" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert vis(L=65) == -1 and "L = 65" in brdf_amd.last_error()
    assert vis(t_min=0.5) == -1 and "t_min = 0.5" in brdf_amd.last_error()
    assert vis(leds_=with_entry(47, np.inf)) == -1 and "leds[15][2] = inf" in brdf_amd.last_error()

    base = C.c_void_p(buf.ctypes.data)

    def apply(images=base, L=2, H=2, W=4, pm=ptr, lit=ptr, nf=4, level=0, out=base, shadowed=ptr):
        return lib.brdf_hip_capture_apply_visibility_dev(images, L, H, W, pm, lit, nf, level, out, shadowed, None)
    at = lambda off: C.c_void_p(buf.ctypes.data + off)
    for kw in (dict(images=None), dict(pm=None), dict(lit=None), dict(out=None), dict(L=0), dict(L=65), dict(H=0), dict(W=0), dict(W=-1), dict(nf=0),
               dict(H=65536, W=32768), dict(level=-1), dict(level=256), dict(out=at(1)), dict(out=at(47)), dict(images=at(47)), dict(images=at(16), out=at(8))):
        assert apply(**kw) == -1, kw
        assert APPLY + "()" in brdf_amd.last_error(), (kw, brdf_amd.last_error())
    assert apply(out=at(47)) == -1 and "overlaps" in brdf_amd.last_error()  # 2 x 2 x 4 x 3 = 48 bytes: the last byte is shared
    assert apply(level=256) == -1 and "level = 256" in brdf_amd.last_error()
    assert not buf.any() and np.all(stats == -7)  # a refused call writes nothing
    capfd.readouterr()


def test_twins_refuse_what_the_entries_refuse():
    import brdf_amd
    v, f = P.floor_with([(3.0, 2.0, 4.0), (5.0, 2.0, 4.0), (3.0, 4.0, 4.0)])
    for kw in (dict(leds=np.zeros((0, 3))), dict(leds=np.zeros((65, 3))), dict(leds=[(0.0, np.nan, 1.0)]), dict(t_min=-1e-9), dict(t_min=0.5),
               dict(t_min=float("nan")), dict(normals=np.zeros((2, 3)))):
        args = dict(leds=[P.LIGHT])
        args.update(kw)
        with pytest.raises(ValueError):
            brdf_amd.light_visibility_host(v, f, **args)
    images, pm, lit = P.paint_case(2, 3, 4, 5)
    for call in (lambda: brdf_amd.apply_visibility_host(images, pm, lit, level=256), lambda: brdf_amd.apply_visibility_host(images, pm, lit, level=-1),
                 lambda: brdf_amd.apply_visibility_host(images, pm[:2], lit), lambda: brdf_amd.apply_visibility_host(images.astype(np.int32), pm, lit),
                 lambda: brdf_amd.apply_visibility_host(images, pm, lit, out=np.zeros((2, 3, 4, 2), dtype=np.uint8)),
                 lambda: brdf_amd.lit_matrix(lit, 0), lambda: brdf_amd.lit_matrix(lit, 65)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("name", sorted(P.hand_scenes()))
def test_hand_written_scenes(name):
    import brdf_amd
    v, f, leds, with_normals, expected, stats = P.hand_scenes()[name]
    got = brdf_amd.light_visibility_host(v, f, leds, normals=P.scene_normals(v, f) if with_normals else None)
    assert got.face_lit.dtype == np.int64 and got.stats.dtype == np.int64
    assert got.face_lit.tolist() == P.words(expected).tolist(), (name, [hex(w) for w in got.face_lit.view(np.uint64).tolist()])
    assert got.stats.tolist() == stats, (name, got.stats)
    L = len(leds)
    m = brdf_amd.lit_matrix(got.face_lit, L)
    assert m.shape == (len(expected), L) and m.dtype == bool
    assert [sum(int(b) << l for l, b in enumerate(row)) for row in m] == expected


def test_the_ray_arithmetic_of_the_hand_written_scenes_is_exact():
    """what the scenes' comments claim: face 0's centre is (4, 2, 0) exactly, and on the edge, corner and hypotenuse scenes the hit test
    sees U = 0, V = 0 or U + V = A exactly"""
    from brdf_amd.shadow import _cross3, _dot3
    scenes = P.hand_scenes()
    want = {"edge": lambda U, V, A: U == 0.0 and V > 0.0, "corner": lambda U, V, A: U == 0.0 and V == 0.0,
            "hypotenuse": lambda U, V, A: U > 0.0 and V > 0.0 and U + V == A}
    for name, rule in want.items():
        v, f = scenes[name][:2]
        a, b, c = (v[f[0, k]] for k in range(3))
        o = ((a + b) + c) / 3.0
        assert o.tolist() == [4.0, 2.0, 0.0]
        v0, e1, e2 = v[f[2, 0]], v[f[2, 1]] - v[f[2, 0]], v[f[2, 2]] - v[f[2, 0]]
        d, s = np.array(P.LIGHT) - o, o - v0
        h, q = _cross3(d, e2), _cross3(s, e1)
        A, U, V, T = _dot3(e1, h), _dot3(s, h), _dot3(d, q), _dot3(e2, q)
        if A < 0.0:
            A, U, V, T = -A, -U, -V, -T
        assert rule(U, V, A) and T == 0.5 * A, (name, U, V, T, A)  # the blockers hang at z = 4, half way to the light at z = 8


def test_t_min_decides_a_hit_at_the_ends_of_the_ray():
    """an occluder through the light itself (T = A) or through the origin (T = 0) never hits; one at a quarter of the way hits unless
    t_min reaches past it"""
    import brdf_amd
    v, f = P.floor_with([(2.0, 2.0, 2.0), (6.0, 2.0, 2.0), (2.0, 6.0, 2.0)])  # face 0's ray passes (3.75, 2.25, 2) at t = 0.25
    for t_min, lit in ((0.0, 0), (1e-9, 0), (0.25, 1), (0.375, 1), (0.125, 0)):
        assert brdf_amd.light_visibility_host(v, f, [P.LIGHT], t_min=t_min).face_lit[0] == lit, t_min
    through_light, _ = P.floor_with([(2.0, 2.0, 8.0), (6.0, 2.0, 8.0), (2.0, 6.0, 8.0)])
    assert brdf_amd.light_visibility_host(through_light, f, [P.LIGHT], t_min=0.0).face_lit[:2].tolist() == [1, 1]
    through_origin, _ = P.floor_with([(3.0, 1.0, 0.0), (6.0, 1.0, 0.0), (3.0, 4.0, 0.0)])  # in the floor's plane, over face 0's centre
    assert brdf_amd.light_visibility_host(through_origin, f, [P.LIGHT], t_min=0.0).face_lit[:2].tolist() == [1, 1]


def test_paint_twin_on_a_three_by_four_map():
    import brdf_amd
    L, H, W, nf = 3, 3, 4, 3
    lit = P.words([0b111, 0b010, 0b000])  # face 0 sees every light, face 1 light 1 only, face 2 none
    pm = np.array([[0, 1, 2, -1], [3, 1, 0, 2], [-1, -1, 2, 1]], dtype=np.int32)  # 3 is beyond nf: background, like -1
    images = (np.arange(L * H * W * 3, dtype=np.int64) % 251 + 1).astype(np.uint8).reshape(L, H, W, 3)
    dark_faces = {0: (1, 2), 1: (2,), 2: (1, 2)}  # per light: the faces that do not see it
    for level in (0, 200):
        got = brdf_amd.apply_visibility_host(images, pm, lit, level=level)
        want = images.copy()
        for l in range(L):
            for y in range(H):
                for x in range(W):
                    if pm[y, x] in dark_faces[l]:
                        want[l, H - 1 - y, x, :] = level  # map row y is image row H - 1 - y
        assert got.images is not images and np.array_equal(got.images, want)
        assert got.shadowed.dtype == np.int64 and got.shadowed.tolist() == [6, 3, 6]  # three pixels carry face 1, three face 2
        assert (got.images != images).any(axis=3).sum() == 15
    other = np.full_like(images, 9)
    assert brdf_amd.apply_visibility_host(images, pm, lit, level=200, out=other).images is other and np.array_equal(other, want)
    work = images.copy()
    in_place = brdf_amd.apply_visibility_host(work, pm, lit, level=200, out=work)
    assert in_place.images is work and np.array_equal(work, want)
    assert np.array_equal(brdf_amd.apply_visibility_host(images, pm, P.words([2 ** 64 - 1] * 3)).images, images)  # all lit: nothing painted


@pytest.mark.parametrize("nf,L", [(257, 16), (1025, 16), (257, 64)])
def test_random_scene_is_neither_all_lit_nor_all_dark(nf, L):
    """the scene of tests/test_gpu_light_visibility.py: between 10 % and 90 % of the pairs that do not face away are shadowed, with and
    without normals; and with normals the lights below the floor make pairs that face away"""
    import brdf_amd
    v, f, leds = P.random_scene(nf, L)
    bare = brdf_amd.light_visibility_host(v, f, leds)
    assert bare.stats[0] == nf and bare.stats[2] == 0 and bare.stats[3] + bare.stats[4] == nf * L
    assert 0.10 <= P.shadowed_share(bare.stats) <= 0.90, bare.stats
    if nf == 257:
        normals = brdf_amd.light_visibility_host(v, f, leds, normals=P.scene_normals(v, f))
        assert normals.stats[2] >= nf * (L // 5) // 2 and normals.stats[2:].sum() == nf * L
        assert 0.10 <= P.shadowed_share(normals.stats) <= 0.90, normals.stats
        assert np.array_equal(normals.face_lit & ~bare.face_lit, np.zeros(nf, dtype=np.int64))  # normals only clear bits
