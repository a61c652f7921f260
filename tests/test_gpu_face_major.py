"""The entries over the face-major samples against what the commit before capture_face_major.hip computed, byte for byte.

That commit held the face-major pack, the chunk scan, the residual chunk kernel and the fold twice, once in capture_single_faces.hip and
once in capture_materials.hip; now both entries run one text, and that the two agree (tests/test_gpu_capture_residuals.py) no longer
pins either.  tests/golden/face_major_parent.json holds, for every call below, the return code, the host scalars and the sha256 of every
output array as that parent commit's library returned them on an MI355X (scripts/gen_face_major_golden.py wrote it, from this file's
case list, after two runs that agreed: integer atomics and fixed-order sums only); the test asserts the same.

Cases, the smallest that reach a path tests/golden/capture_layer_parent.json does not:
    single/m*/L64      fit_capture_single_faces on rule_capture(model, lights=64), every model (that fixture stops at 16 lights)
    edge/single, edge/residuals5
                       test_gpu_capture_residuals.edge_capture(): faces of 1024 and 1025 samples, a face empty in one channel;
                       capture_face_residuals with one material more than the kernel's group
    big/residuals5     the same on big_capture(): the scans over many faces, a face of five chunks
    planted/labelled, planted/materials
                       fit_capture_labelled on the planted labels and fit_capture_materials (3 rounds) on the planted capture of
                       tests/materials_problems.py, every optional map
Every map starts from a sentinel, so a write to a row that is not the call's shows as well.  single/m2/L64 returns 3: on this
capture's planes no Ward fit at 64 lights ends with ret >= 0, so that case pins the pack and the residual kernels' bytes at the points
the fits leave, not a converged Ward fit (the older fixture's 16-light cases hold those).  "_made_by" in the fixture names the library
that wrote it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import capture_problems as P
from tests import materials_problems as M
from tests import test_gpu_capture_layer as T
from tests import test_gpu_capture_residuals as R
from tests import test_gpu_capture_single_faces as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(T.ROOT, "tests", "golden", "face_major_parent.json")
SENTINEL = S.SENTINEL


def case_names():
    return [f"single/m{model}/L64" for model in (0, 1, 2)] + ["edge/single", "edge/residuals5", "big/residuals5", "planted/labelled", "planted/materials"]


def _five(model):
    """GROUP + 1 materials that depend on no fit: the model's truth, then R._materials' others"""
    from brdf_amd import synth
    return R._materials(model, np.tile(np.array(synth.TRUTH[model]), (3, 1)))


def _labelled_entry(gpu, cap, materials, labels, rounds=None):
    """brdf_hip_fit_capture_labelled_dev (rounds None) or brdf_hip_fit_capture_materials_dev itself, every map from the sentinel:
    (the return code, {name: array or scalar})"""
    torch, brdf_amd, dev = gpu
    from brdf_amd import fit as F
    nf, K = cap["nf"], len(materials)
    args, keep, _ = F._capture_args(M.MODEL, *(S._dev(gpu, cap[k]) for k in ("images", "pixel_map", "vertices", "faces", "nrm")), cap["leds"], cap["view"], 1,
                                    None, P.LB, P.UB, 100, P.OPTS, False)
    full = lambda *shape, dtype=torch.float64: torch.full(shape, SENTINEL, dtype=dtype, device=dev)  # noqa: E731
    i32 = torch.int32
    out = dict(materials=S._dev(gpu, np.array(materials, dtype=np.float64)), info=full(K, 3, 10), ret=full(K, 3, dtype=i32), covar=full(K, 3, 3, 3),
               stats=full(K, 3, 8), rank=full(K, 3, dtype=i32), count=full(K, 3, dtype=i32), label_faces=full(K, dtype=i32), face_pixels=full(nf, dtype=i32))
    fits = tuple(out[k].data_ptr() for k in ("info", "ret", "covar", "stats", "rank", "count", "label_faces", "face_pixels"))
    rule = (M.RULE["v_min"], M.RULE["v_max"], M.RULE["cos_min"], 0)  # the rule, workspace_bytes
    npx, nfc = C.c_longlong(-1), C.c_longlong(-1)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    with torch.cuda.device(dev):
        if rounds is None:
            out["labels"] = S._dev(gpu, np.asarray(labels, dtype=np.int32))
            rc = brdf_amd.lib.brdf_hip_fit_capture_labelled_dev(*args[:13], *args[14:18], *rule, out["labels"].data_ptr(), K, out["materials"].data_ptr(),
                                                                *fits, C.byref(npx), C.byref(nfc), stream())
        else:
            out.update(labels=full(nf, dtype=i32), face_sumsq=full(nf, 3), face_count=full(nf, 3, dtype=i32))
            used, settled = C.c_int(-1), C.c_int(-1)
            changed = np.full(rounds + 1, SENTINEL, dtype=np.int64)
            rc = brdf_amd.lib.brdf_hip_fit_capture_materials_dev(*args[:13], *args[14:18], *rule, K, rounds, out["materials"].data_ptr(),
                                                                 out["labels"].data_ptr(), out["face_sumsq"].data_ptr(), out["face_count"].data_ptr(), *fits,
                                                                 C.byref(used), C.byref(settled), changed.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                                 C.byref(npx), C.byref(nfc), stream())
            out.update(rounds_used=used.value, settled=settled.value, changed=changed)
    torch.cuda.synchronize()
    out.update(n_pixels=npx.value, n_faces=nfc.value)
    return int(rc), out


def run_case(gpu, name):
    """{"rc", the host scalars, "sha256": {output array: its hash}} of one case"""
    torch, brdf_amd, _ = gpu
    kind, what = name.split("/")[:2]
    if kind == "planted":
        cap = M.planted_capture()
        if what == "labelled":
            rc, out = _labelled_entry(gpu, cap, np.tile(np.array(P.P0), (M.K_PLANTED, 3, 1)), cap["planted"])
        else:
            rc, out = _labelled_entry(gpu, cap, 1.1 * cap["truth"], None, rounds=3)
    elif what == "residuals5":
        cap = R.edge_capture() if kind == "edge" else P.big_capture()
        with T._recorded("brdf_hip_capture_face_residuals_dev") as seen:
            out = dict(zip(("face_sumsq", "face_count", "face_pixels"), R._residuals(gpu, cap, 1, _five(1), **P.RULE)))
        rc = int(seen["rc"])
    else:
        model = int(what[1:]) if kind == "single" else 1
        cap = P.rule_capture(model, lights=64) if kind == "single" else R.edge_capture()
        with T._recorded("brdf_hip_fit_capture_single_faces_dev") as seen:
            out = S._single(gpu, cap, model, **P.RULE)
        rc = int(seen["rc"])
    rec = {"rc": rc}
    for key, value in out.items():
        if isinstance(value, (int, bool)):
            rec[key] = int(value)
        else:
            rec.setdefault("sha256", {})[key] = T._sha(T._host(value))
    return rec


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
def test_face_major_entries_return_the_parents_bytes(gpu, golden, name):
    got, want = run_case(gpu, name), golden[name]
    assert got == want, (got, want)
