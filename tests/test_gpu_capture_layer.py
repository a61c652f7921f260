"""The seven capture entries against what the commit before the capture-layer refactor computed, byte for byte.

The refactor moved the capture's host code and its grouping, scan and scatter kernels into shared text and must not move a bit of a
result.  tests/golden/capture_layer_parent.json holds, for every call below, the return code, the host scalars and the sha256 of every
output array as that parent commit's library returned them on an MI355X (scripts/gen_capture_layer_golden.py wrote it, from this
file's case list, after two runs that agreed: the capture has integer atomics and fixed-order sums only); the test asserts the same.

Captures (tests/capture_problems.py), the smallest that reach every path of the layer:
    rule_capture(model)   23 x 31 pixels, 37 carried faces, 604 pixels: every model at 16 and at 5 lights, the rule off and RULE, the
                          sound mesh and the one with a face of NaN cosines
    an all-background map the empty capture
    big_capture()         67 x 73 pixels, 70,001 faces, 282 pack blocks, 8 scatter blocks: multi-block compaction, every one-workgroup
                          scan with two items per thread, multi-block scatter, one face of 300 pixels among faces of one
Every optional map is asked for, and every map starts from a sentinel, so a write to a row that is not the call's shows as well.  The
entries without a validity rule (capture, capture_stats, capture_single) run in the cases with the rule off."""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest

from tests import capture_problems as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capture_layer_parent.json")
SENTINEL = -7
RULE_OFF = dict(v_min=0, v_max=255, cos_min=-2.0)
RULED = ("masked", "faces", "means", "single_faces")  # the entries that take a validity rule
UNRULED = ("capture", "stats", "single")
SYMBOL = {"capture": "brdf_hip_fit_capture_dev", "stats": "brdf_hip_fit_capture_stats_dev", "masked": "brdf_hip_fit_capture_masked_dev",
          "faces": "brdf_hip_fit_capture_faces_dev", "means": "brdf_hip_fit_capture_means_dev", "single": "brdf_hip_fit_capture_single_dev",
          "single_faces": "brdf_hip_fit_capture_single_faces_dev"}


def case_names():
    out = [f"rule/m{model}/L{lights}/{'nan' if nan else 'sound'}/{'rule' if ruled else 'off'}"
           for model in (0, 1, 2) for lights in (16, 5) for nan in (False, True) for ruled in (False, True)]
    return out + ["empty/m1/off", "big/m1/off", "big/m1/rule"]


def case_of(name):
    """(capture, pixel map, model, rule, the entries to call)"""
    parts = name.split("/")
    ruled = parts[-1] == "rule"
    model = int(parts[1][1:])
    if parts[0] == "rule":
        cap = P.rule_capture(model, nan_face=parts[3] == "nan", lights=int(parts[2][1:]))
    elif parts[0] == "empty":
        cap = P.rule_capture(model)
    else:
        cap = P.big_capture()
    pixel_map = np.full_like(cap["pixel_map"], -1) if parts[0] == "empty" else cap["pixel_map"]
    return cap, pixel_map, model, (P.RULE if ruled else RULE_OFF), (RULED if ruled else UNRULED + RULED)


def _sha(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@contextlib.contextmanager
def _recorded(symbol):
    """the C entry's own return code: the wrappers turn it into an exception or drop it"""
    from brdf_amd._lib import lib
    fn = getattr(lib, symbol)
    seen = {}

    def proxy(*args):
        seen["rc"] = fn(*args)
        return seen["rc"]
    setattr(lib, symbol, proxy)
    try:
        yield seen
    finally:
        setattr(lib, symbol, fn)


MARK = "brdf_hip_fit_capture_dev(): bad arguments"


def _mark_error():
    """The library keeps a thread's last error text until the next one: a refused call (no device is touched) leaves a known text, so
    that a failing call that words no error of its own -- a fit that levmar itself gives up -- is told from one that does."""
    import brdf_amd
    from brdf_amd._lib import lib
    assert lib.brdf_hip_fit_capture_dev(0, None, 0, 0, 0, None, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, None) == -1
    assert brdf_amd.last_error() == MARK


def _call_entry(gpu, entry, dev_args, cap, model, rule):
    """one call through the Python wrapper, every map from the sentinel: {name: array or scalar}"""
    torch, brdf_amd, dev = gpu
    nf = cap["nf"]
    full = lambda *shape, dtype=torch.float64: torch.full((nf, *shape), SENTINEL, dtype=dtype, device=dev)  # noqa: E731
    i32 = torch.int32
    stats = lambda: brdf_amd.FitStats(full(3, 3, 3), full(3, 8), full(3, dtype=i32))  # noqa: E731
    common = dict(rv_mode=1, p0=P.P0, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS, validate=False)
    args = (model, *dev_args, cap["leds"], cap["view"])
    if entry in ("capture", "stats", "masked"):
        kw = dict(common, brdf_surfaces=full(3, 3))
        if entry == "capture":
            r = brdf_amd.fit_capture(*args, **kw)
        elif entry == "stats":
            r = brdf_amd.fit_capture(*args, want_stats=True, surface_stats=stats(), **kw)
        else:
            r = brdf_amd.fit_capture_masked(*args, surface_count=full(3, dtype=i32), surface_stats=stats(), **rule, **kw)
        out = dict(surfaces=r[0], avg=r[1], n_pixels=r[2])
        if entry != "capture":
            out.update(covar=r[3].covar, stats=r[3].stats, rank=r[3].rank)
        if entry == "masked":
            out.update(count=r[4])
        return out
    if entry == "faces":
        r = brdf_amd.fit_capture_faces(*args, **rule, **common, out=brdf_amd.CaptureFaces(full(3, 3), full(3, 10), full(3, dtype=i32), stats(), full(3, dtype=i32),
                                                                                       full(dtype=i32), None, 0, 0))
        return dict(surfaces=r.surfaces, info=r.info, ret=r.ret, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank, count=r.count,
                    face_pixels=r.face_pixels, avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)
    if entry == "means":
        r = brdf_amd.fit_capture_means(*args, **rule, **common, out=brdf_amd.CaptureMeans(full(3, 3), full(3, 10), full(3, dtype=i32), stats(), full(3, dtype=i32),
                                                                                       full(3, dtype=i32), full(dtype=i32), None, 0, 0))
        return dict(surfaces=r.surfaces, info=r.info, ret=r.ret, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank, count=r.count,
                    lights=r.lights, face_pixels=r.face_pixels, avg=r.avg, n_pixels=r.n_pixels, n_faces=r.n_faces)
    if entry == "single":
        r = brdf_amd.fit_capture_single(*args, **common)
        return dict(single_brdf=r[0], info=r[1], n_faces=r[2])
    assert entry == "single_faces"
    r = brdf_amd.fit_capture_single_faces(*args, **rule, **common, out=brdf_amd.CaptureSingleFaces(None, None, None, None, None, full(3), full(3, dtype=i32),
                                                                                                  full(dtype=i32), 0, 0))
    return dict(single_brdf=r.single_brdf, info=r.info, ret=r.ret, count=r.count, covar=r.stats.covar, stats=r.stats.stats, rank=r.stats.rank,
                face_sumsq=r.face_sumsq, face_count=r.face_count, face_pixels=r.face_pixels, n_pixels=r.n_pixels, n_faces=r.n_faces)


def run_case(gpu, name):
    """{entry: {"rc", "error" (a refused call's text) or the scalars and "sha256" of every output array}} of one case"""
    torch, brdf_amd, dev = gpu
    cap, pixel_map, model, rule, entries = case_of(name)
    dev_args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cap["images"], pixel_map, cap["vertices"], cap["faces"], cap["nrm"]))
    res = {}
    for entry in entries:
        rec = {}
        _mark_error()
        with _recorded(SYMBOL[entry]) as seen:
            try:
                out = _call_entry(gpu, entry, dev_args, cap, model, rule)
            except RuntimeError:
                out = None
                rec["error"] = brdf_amd.last_error() if brdf_amd.last_error() != MARK else ""
        torch.cuda.synchronize()
        rec["rc"] = int(seen["rc"])
        for key, value in (out or {}).items():
            if isinstance(value, int):
                rec[key] = value
            elif key == "avg":
                rec[key] = np.asarray(value, dtype=np.float64).tobytes().hex()
            else:
                rec.setdefault("sha256", {})[key] = _sha(_host(value))
        res[entry] = rec
    return res


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", case_names())
def test_capture_entries_return_the_parents_bytes(gpu, golden, name):
    got, want = run_case(gpu, name), golden[name]
    assert sorted(got) == sorted(want)
    wrong = [(entry, got[entry], want[entry]) for entry in got if got[entry] != want[entry]]
    assert not wrong, wrong
