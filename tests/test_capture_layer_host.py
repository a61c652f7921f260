"""The capture layer's refusals, word for word what the commit before the capture-layer refactor said, and the coverage of the two
fixtures scripts/gen_capture_layer_golden.py wrote at that commit.  No device: every call below is refused before any HIP call.

The refused argument sets are those of the host tests of the seven entries -- tests/test_capture_faces_host.py,
tests/test_capture_single_faces_host.py, tests/test_ragged_host.py (masked), tests/test_fit_stats.py (capture_stats) and
tests/test_weighted_host.py (means) -- and, for the two entries without such a test, a null pointer and L out of range."""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capture_refusals_parent.json")

_NULLS = [dict(images=None), dict(pm=None), dict(vertices=None), dict(faces=None), dict(normals=None), dict(leds=None), dict(view=None), dict(p0=None),
          dict(out=None)]
_SHAPES = [dict(L=0), dict(L=65), dict(L=-1), dict(H=0), dict(W=-2), dict(nf=0), dict(nf=-1), dict(nf=(2 ** 31 - 1) // 3 + 1)]
_RULES = [dict(model=3), dict(model=-1), dict(model=7), dict(v_min=200, v_max=100), dict(v_min=3, v_max=2), dict(cos_min=float("nan"))]
_BOX = [dict(lb=(0.0, 2.0, 0.0), ub=(1.0, 1.0, 1.0))]
# entry -> (what the calls share besides BASE, the refused argument sets)
REFUSED = {
    "faces": ({}, _NULLS + _SHAPES + _RULES + [dict(ws=-1), dict(ws=-9)] + _BOX),
    "single_faces": ({}, _NULLS + _SHAPES + _RULES + _BOX),
    "masked": (dict(H=2, W=2, nf=1, lb=None, ub=None, cos_min=0.0, itmax=10),
               [dict(images=None), dict(p0=None), dict(L=0), dict(L=65), dict(H=0), dict(nf=0), dict(v_min=200, v_max=100), dict(v_min=1, v_max=0),
                dict(cos_min=float("nan")), dict(model=3), dict(model=-1)]),
    "stats": (dict(H=4, W=4, nf=5, lb=None, ub=None), [dict(L=2), dict(images=None), dict(L=65), dict(nf=(2 ** 31 - 1) // 3 + 1)]),
    "means": (dict(H=4, W=4, nf=5), [dict(L=17), dict(L=64), dict(L=0), dict(v_min=200, v_max=100), dict(ub=(1.0, -1.0, 1.0)), dict(images=None)]),
    "capture": ({}, [dict(images=None), dict(out=None), dict(L=0), dict(L=65), dict(H=0), dict(nf=0)]),
    "single": ({}, [dict(images=None), dict(out=None), dict(L=0), dict(L=65), dict(W=0), dict(nf=-3)]),
}
BASE = dict(model=1, L=16, H=8, W=8, nf=10, p0=(0.5, 1.0, 1.0), lb=(0.0, 0.0, 0.0), ub=(100.0, 100.0, 100.0), itmax=100, v_min=0, v_max=255, cos_min=-2.0,
            ws=0)
POINTERS = ("images", "pm", "vertices", "faces", "normals", "leds", "view", "out")


def name_of(entry, change):
    return entry + "(" + ", ".join(f"{k}={v}" for k, v in change.items()) + ")"


def refusal(entry, change):
    """(return code, brdf_amd.last_error()) of one refused call"""
    import brdf_amd
    from brdf_amd._lib import D, lib
    buf = np.zeros(64)  # never read: the call is refused before anything touches memory
    k = dict(BASE, **{name: C.c_void_p(buf.ctypes.data) for name in POINTERS})
    k.update(REFUSED[entry][0])
    k.update(change)
    keep = {name: None if k[name] is None else np.array(k[name], dtype=np.float64) for name in ("p0", "lb", "ub")}
    d = lambda name: None if keep[name] is None else keep[name].ctypes.data_as(D)  # noqa: E731
    dbl = lambda name: None if k[name] is None else C.cast(k[name], D)  # noqa: E731
    head = (k["model"], k["images"], k["L"], k["H"], k["W"], k["pm"], k["vertices"], k["faces"], k["normals"], k["nf"], dbl("leds"), dbl("view"), 1,
            d("p0"), d("lb"), d("ub"), k["itmax"], None)
    rule = (k["v_min"], k["v_max"], k["cos_min"])
    out = k["out"]
    tail = {"capture": (out, None, None, None),
            "stats": (out, None, None, None, None, out, None),
            "masked": (out, None, None, None, None, None, None, *rule, None),
            "faces": (*rule, k["ws"], out) + (None,) * 11,
            "means": (*rule, out) + (None,) * 12,
            "single": (dbl("out"), None, None, None),
            "single_faces": (*rule, dbl("out")) + (None,) * 12}[entry]
    from tests.test_gpu_capture_layer import SYMBOL
    rc = getattr(lib, SYMBOL[entry])(*head, *tail)
    return rc, brdf_amd.last_error()


def all_refusals():
    return {name_of(entry, change): refusal(entry, change) for entry, (_, changes) in REFUSED.items() for change in changes}


def test_refusal_texts_are_the_parents(capfd):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = all_refusals()
    assert sorted(got) == sorted(want) and len(got) == sum(len(changes) for _, changes in REFUSED.values())
    from tests.test_gpu_capture_layer import SYMBOL
    for name, (rc, text) in got.items():
        assert rc == -1 and text == want[name], (name, text, want[name])
        assert SYMBOL[name.split("(")[0]] + "()" in text, (name, text)  # every refusal names the entry that was called
    capfd.readouterr()


def test_the_gpu_fixture_covers_every_case_and_every_entry():
    from tests import test_gpu_capture_layer as T
    with open(T.GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == sorted(T.case_names())
    for name in T.case_names():
        ruled = name.endswith("/rule")
        assert sorted(g[name]) == sorted(T.RULED if ruled else T.UNRULED + T.RULED), name
        for entry, rec in g[name].items():
            if name.startswith("empty") and entry == "single":  # the one refusal: "no pixel carries a face"
                assert rec["rc"] == -1 and "no pixel carries a face" in rec["error"]
            elif entry == "single" and rec["rc"] < 0:  # levmar's own failure, no text: this entry has no rule, a NaN or a cosine <= 0 is a sample
                assert rec == {"rc": -1, "error": ""} and ("/nan/" in name or "/m2/" in name), (name, rec)
            else:
                assert rec["rc"] >= 0 and "error" not in rec and ("surfaces" in rec["sha256"] or "single_brdf" in rec["sha256"]), (name, entry, rec)
    big = g["big/m1/rule"]
    assert big["faces"]["n_pixels"] == big["means"]["n_pixels"] == big["single_faces"]["n_pixels"] == 4500
    assert big["faces"]["n_faces"] == big["means"]["n_faces"] == big["single_faces"]["n_faces"] == 644
    assert g["empty/m1/off"]["faces"]["n_pixels"] == 0 and g["empty/m1/off"]["single_faces"]["rc"] == 3
