"""K materials per object (brdf_hip_fit_capture_materials_dev) on the planted capture of tests/materials_problems.py.

  (1) every output has the bytes of a host-driven replay of the definition: capture_face_residuals and fit_capture_labelled on the
      device, assign_materials on the host ON THE DEVICE'S BYTES, so that no near-tie can separate the two -- with rounds = 0, 1, 2 (a
      run that exhausts its rounds unsettled) and enough to settle; two identical seeds, where the lowest k takes everything and the
      other label is empty and keeps its material; the four seeds of the seeding rule;
  (2) the planted capture through seed_materials and the entry: purity 1.0, settled, `changed` ends in 0, below the planted truth's sum
      of squares as the CPU loop is;
  (3) against the same loop around the compiled reference (the oracle's restatement where oracle/_ref was not built) from the same
      seeds: the labels are the same; p agrees to 1e-5 wherever the reference agrees with its own +-1 ulp twin; every objective is
      within 1e-6 of the reference's or lower (tests/weighted_yardstick.py: parity_figures).  Figures: DESIGN.md section 2."""
import functools

import numpy as np
import pytest

from tests import capture_problems as P
from tests import materials_problems as M
from tests import oracle_libs as L
from tests import test_gpu_capture_single_faces as S
from tests import weighted_yardstick as WY

pytestmark = pytest.mark.gpu
OUTPUTS = ("materials", "labels", "face_sumsq", "face_count", "info", "ret", "covar", "stats", "rank", "count", "label_faces", "face_pixels")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import brdf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch, brdf_amd, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _capture(gpu):
    cap = M.planted_capture()
    return cap, tuple(S._dev(gpu, cap[k]) for k in ("images", "pixel_map", "vertices", "faces", "nrm")) + (cap["leds"], cap["view"])


KW = dict(rv_mode=1, lb=P.LB, ub=P.UB, itmax=100, opts=P.OPTS, validate=False, **M.RULE)


def _entry(gpu, seeds, rounds):
    torch, brdf_amd, _ = gpu
    _, args = _capture(gpu)
    r = brdf_amd.fit_capture_materials(M.MODEL, *args, np.array(seeds, dtype=np.float64), rounds=rounds, **KW)
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(materials=h(r.materials), labels=h(r.labels), face_sumsq=h(r.face_sumsq), face_count=h(r.face_count), info=h(r.info), ret=h(r.ret),
                covar=h(r.stats.covar), stats=h(r.stats.stats), rank=h(r.stats.rank), count=h(r.count), label_faces=h(r.label_faces),
                face_pixels=h(r.face_pixels), rounds_used=r.rounds_used, settled=r.settled, changed=[int(n) for n in r.changed], n_pixels=r.n_pixels,
                n_faces=r.n_faces)


def _replay(gpu, seeds, rounds):
    """the definition, driven from the host: the device's residuals and labelled fits, the host's assignment on the device's bytes"""
    torch, brdf_amd, dev = gpu
    cap, args = _capture(gpu)
    nf, K = cap["nf"], len(seeds)
    rule = {k: KW[k] for k in ("v_min", "v_max", "cos_min", "rv_mode", "validate")}
    materials = torch.from_numpy(np.array(seeds, dtype=np.float64)).to(dev)
    labels = np.full(nf, -1, dtype=np.int32)
    want = dict(info=np.zeros((K, 3, 10)), ret=np.full((K, 3), -1, dtype=np.int32), covar=np.zeros((K, 3, 3, 3)), stats=np.zeros((K, 3, 8)),
                rank=np.zeros((K, 3), dtype=np.int32), count=np.zeros((K, 3), dtype=np.int32), label_faces=np.zeros(K, dtype=np.int32))
    changed, refits, settled = [], 0, False
    while True:
        res = brdf_amd.capture_face_residuals(M.MODEL, *args, materials, **rule)
        carried = res.face_pixels.cpu().numpy() > 0
        labels, n = brdf_amd.assign_materials(res.face_sumsq.cpu().numpy(), labels, carried=carried)
        changed.append(n)
        if n == 0:
            settled = True
            break
        if refits == rounds:
            break
        fit = brdf_amd.fit_capture_labelled(M.MODEL, *args, labels, materials, **KW)  # (writes the materials)
        for name, t in (("info", fit.info), ("ret", fit.ret), ("covar", fit.stats.covar), ("stats", fit.stats.stats), ("rank", fit.stats.rank),
                        ("count", fit.count), ("label_faces", fit.label_faces)):
            want[name] = t.cpu().numpy()
        refits += 1
        if refits == rounds:
            break
    res = brdf_amd.capture_face_residuals(M.MODEL, *args, materials, **rule)
    s = res.face_sumsq.cpu().numpy()
    own = np.zeros((nf, 3))
    for f in np.flatnonzero(carried):
        own[f] = s[f, labels[f]] if labels[f] >= 0 else np.inf
    want.update(materials=materials.cpu().numpy(), labels=labels, face_sumsq=own, face_count=res.face_count.cpu().numpy(),
                face_pixels=res.face_pixels.cpu().numpy(), rounds_used=refits, settled=settled, changed=changed)
    return want


def _same(got, want):
    for name in OUTPUTS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, want[name].dtype)
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])
    assert (got["rounds_used"], got["settled"], got["changed"]) == (want["rounds_used"], want["settled"], want["changed"]), (got["changed"], want["changed"])


@functools.lru_cache(maxsize=None)
def _host_seeds():
    return M.host_seeds(M.solver(), M.K_PLANTED)[0]


@pytest.mark.parametrize("rounds", [0, 1, 2, 20])
def test_replay_with_two_materials(gpu, rounds):
    seeds = _host_seeds()[:2]
    got, want = _entry(gpu, seeds, rounds), _replay(gpu, seeds, rounds)
    print("rounds", rounds, "used", got["rounds_used"], "settled", got["settled"], "changed", got["changed"], "faces", got["label_faces"].tolist())
    _same(got, want)
    assert got["n_faces"] == 80 and got["n_pixels"] == int(M.planted_capture()["sizes"].sum())
    if rounds == 0:  # the seeds and one assignment; no refit ran
        assert got["materials"].tobytes() == np.array(seeds).tobytes() and got["changed"] == [80] and not got["settled"]
        assert np.all(got["ret"] == -1) and not got["info"].any() and not got["count"].any() and not got["label_faces"].any()
    elif rounds < 20:  # exhausted unsettled: `rounds` refits, `rounds` assignments, the last one moved labels
        assert got["rounds_used"] == rounds and not got["settled"] and len(got["changed"]) == rounds and got["changed"][-1] > 0
    else:
        assert got["settled"] and 2 < got["rounds_used"] < 20 and got["changed"][-1] == 0 and len(got["changed"]) == got["rounds_used"] + 1
    assert np.all(got["labels"] >= 0) and got["label_faces"].sum() in (0, 80)
    assert np.isfinite(got["face_sumsq"]).all() and (rounds == 0 or got["face_count"].sum() == got["count"].sum())


def test_replay_with_two_identical_seeds(gpu):
    seeds = _host_seeds()[[1, 1, 2, 3]]
    first = _entry(gpu, seeds, 1)
    _same(first, _replay(gpu, seeds, 1))
    assert first["label_faces"][1] == 0 and first["label_faces"][0] > 0 and not np.any(first["labels"] == 1)  # the lowest k takes everything
    assert first["materials"][1].tobytes() == seeds[1].tobytes() and np.all(first["ret"][1] == -1) and not first["count"][1].any()
    got = _entry(gpu, seeds, 20)
    print("identical seeds: used", got["rounds_used"], "settled", got["settled"], "changed", got["changed"], "faces", got["label_faces"].tolist())
    _same(got, _replay(gpu, seeds, 20))
    assert got["settled"]


def _truth_total():
    cap = M.planted_capture()
    sets, carried = M.face_samples()
    truth = M.face_sumsq(sets, carried, cap["nf"], cap["truth"])
    return float(sum(truth[f, cap["planted"][f]].sum() for f in carried))


def test_the_planted_capture_through_the_seeding_rule_and_the_entry(gpu):
    torch, brdf_amd, _ = gpu
    cap, args = _capture(gpu)
    seeds = brdf_amd.seed_materials(M.K_PLANTED, M.MODEL, *args, min_count=M.MIN_COUNT, p0=P.P0, **KW)
    assert seeds.shape == (4, 3, 3) and np.isfinite(seeds).all()
    host = _host_seeds()
    print("seeds against the CPU rule's, largest relative difference per seed:", [f"{L.rel_err(seeds[k].reshape(-1), host[k].reshape(-1)):.2e}" for k in range(4)])
    got = _entry(gpu, seeds, 20)
    _same(got, _replay(gpu, seeds, 20))
    total, truth = float(got["face_sumsq"].sum()), _truth_total()
    print(f"used {got['rounds_used']} settled {got['settled']} changed {got['changed']} purity {M.purity(got['labels'], cap['planted'], 4)} "
          f"sum of squares {total:.6f} planted truth {truth:.6f} ret {got['ret'].T.tolist()}")
    assert got["settled"] and got["changed"][-1] == 0 and got["rounds_used"] <= 20
    assert M.purity(got["labels"], cap["planted"], M.K_PLANTED) == 1.0
    assert total < truth


def test_against_the_loop_around_the_reference(gpu):
    which = M.solver()
    seeds = _host_seeds()
    got = _entry(gpu, seeds, 20)
    ref = M.host_loop(which, seeds, 20)
    twin = M.host_loop(which, seeds, 20, twin_seed=12345)
    assert np.array_equal(got["labels"], ref["labels"]) and got["changed"] == ref["changed"] and got["settled"] == ref["settled"]
    flat = lambda a, *tail: a.reshape(-1, *tail)  # noqa: E731
    both, close, near, worst = WY.parity_figures(flat(got["ret"]), flat(got["materials"], 3), flat(got["info"], 10), flat(ref["ret"]),
                                                 flat(ref["materials"], 3), flat(ref["info"], 10))
    agree = np.array_equal(ref["labels"], twin["labels"])
    steady = [(k, c) for k in range(4) for c in range(3) if agree and L.rel_err(ref["materials"][k, c], twin["materials"][k, c]) <= 1e-5]
    held = [(k, c) for k, c in steady if L.rel_err(got["materials"][k, c], ref["materials"][k, c]) <= 1e-5]
    print(f"solver {which}: labels equal, changed {got['changed']}; of 12 fits the reference agrees with its +-1 ulp twin on {len(steady)}, the entry with "
          f"the reference on {len(held)} of those; parity_figures: converged on both sides {both}, within 1e-5 on p {close}, objectives within 1e-6 or "
          f"lower {near}, worst excess {worst:.3e}")
    assert held == steady, (steady, held)
    assert near == 12, (near, worst)
