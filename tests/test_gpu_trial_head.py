"""The resident single-fit dlevmar_dif kernels against what the commit before the trial-head change computed, byte for byte.

The change shortens the serial code in front of the control wave's sweep: on an accepted step its f(p) and f(p + Dp) planes, parked
in LDS, trade names (a wave-uniform offset on the two fields' addresses) instead of being copied slot by slot.  No operand,
operation or summation order moves, so no bit of a result may.  tests/golden/trial_head_parent.json holds p, info[], the covariance,
the return code, the pass count and the number of fused steps of every case below as the parent commit's library returned them
on an MI355X (scripts/gen_trial_head_golden.py wrote it, from this file's case list); the test asserts the same bytes.

Sizes, by occupied sample slots per lane of a workgroup (512 lanes, up to 8 slots; `full` slots hold a sample in every lane) -- the
control wave's rolled loop takes two slots per trip and masks the slots that are not full:
    4,096    one workgroup, 8 full slots, no exchange
    4,097    5 workgroups of 820 (the last 817): 2 slots, 1 full -- one trip, its second slot with dead lanes
    262,145  256 workgroups of 1025 (the last 770): 3 slots, 2 full -- a trip and a half; the last workgroup's third slot is empty
    600,001  256 workgroups of 2344: 5 slots, 4 full -- two trips and a partly empty fifth slot
    917,505  256 workgroups of 3585: 8 slots, 7 full, a single sample in the last -- the smallest size with all eight slots in use
Options: the default fits accept most steps (every acceptance is a flip, and the planes are read flipped and unflipped by trial,
Jacobian and chain passes alike) and adopt the Broyden update behind most rejections; tau = 1e-6 starts undamped, so the first
steps are rejected in a chain (several trial points to a sweep) before the first flip.  BRDF_HIP_DIF_FUSED = 0 sends every step
through the generic path.  One dlevmar_bc_dif fit shows that a kernel the change does not touch returns the parent's bytes too.

BRDF_HIP_DIF_FUSED is read from the environment, so each setting runs in a fresh child process (this file, `--worker`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trial_head_parent.json")
SIZES = (4096, 4097, 262145, 600001, 917505)
OPTS = ("default", "tau=1e-6")
MODELS = (0, 1, 2)
METHODS = ("dif", "bc_dif")
BC_CASE = (("single", 2, 4097), 1, "default")
SETTINGS = {"fused": {"BRDF_HIP_DIF_FUSED": "1"}, "generic": {"BRDF_HIP_DIF_FUSED": "0"}}


def case_keys(setting):
    """[(problem key of tests/pass_problems.py, method, name of the opts)]; the dlevmar_bc_dif case runs under `fused` only"""
    out = [(("single", model, n), 0, opts) for model in MODELS for n in SIZES for opts in OPTS]
    return out + ([BC_CASE] if setting == "fused" else [])


def name_of(key):
    problem, method, opts = key
    return "/".join(str(v) for v in problem) + f"/{METHODS[method]}/{opts}"


def _worker(setting, path):
    import torch

    import brdf_amd
    from brdf_amd import synth
    from tests import pass_problems as P

    dev = torch.device("cuda:0")
    hexs = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes().hex()
    opts_of = dict(P.OPTIONS, default=synth.OPTS)
    out = {}
    on_dev = {}
    for key in case_keys(setting):
        problem, method, opts = key
        angles, x, p0, lb, ub = P.problem(problem)
        if problem not in on_dev:
            on_dev[problem] = (torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev))
        box = {"lb": lb, "ub": ub} if method == 1 else {}
        res = brdf_amd.fit_single(method, problem[1], *on_dev[problem], p0, itmax=synth.ITMAX, opts=opts_of[opts], want_covar=True, **box)
        st = brdf_amd.last_fit_stats()
        out[name_of(key)] = {"ret": int(res.ret), "p": hexs(res.p), "info": hexs(res.info), "covar": hexs(res.covar), "passes": int(st["passes"]),
                             "jac_passes": int(st["jac_passes"]), "fused_steps": int(st["fused_steps"]), "launches": int(st["launches"])}
    with open(path, "w") as f:
        json.dump(out, f)


def run_settings(directory):
    """{setting: {case name: record}} from one child process per setting, side by side"""
    procs = {}
    for name, extra in SETTINGS.items():
        env = dict(os.environ, **extra)
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        env.pop("BRDF_HIP_RESIDENT", None)
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", name, os.path.join(str(directory), f"{name}.json")],
                                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for name, pr in procs.items():
        log, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, log[-3000:])
        with open(os.path.join(str(directory), f"{name}.json")) as f:
            res[name] = json.load(f)
    return res


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return run_settings(tmp_path_factory.mktemp("trial_head"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(runs, golden, setting, keys):
    wrong = []
    for key in keys:
        name = name_of(key)
        got, want = runs[setting][name], golden[setting][name]
        assert got["launches"] == 1, (name, got)  # the resident kernel ran, and did not fall back
        for field in ("ret", "p", "info", "covar", "passes", "jac_passes", "fused_steps"):
            if got[field] != want[field]:
                wrong.append((name, field, got[field], want[field]))
    print(f"{setting}: {len(keys)} fits, {len(wrong)} fields differ")
    assert not wrong, wrong[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("setting", tuple(SETTINGS))
def test_dif_fits_return_the_parents_bytes(runs, golden, setting, model):
    keys = [k for k in case_keys(setting) if k[1] == 0 and k[0][1] == model]
    assert len(keys) == len(SIZES) * len(OPTS)
    _compare(runs, golden, setting, keys)


@pytest.mark.gpu
def test_bc_dif_fit_returns_the_parents_bytes(runs, golden):
    _compare(runs, golden, "fused", [BC_CASE])


def test_the_fixture_covers_every_case_and_both_step_paths():
    with open(GOLDEN) as f:
        g = json.load(f)
    for setting in SETTINGS:
        assert sorted(g[setting]) == sorted(name_of(k) for k in case_keys(setting))
        assert all(r["launches"] == 1 and r["ret"] >= 0 for r in g[setting].values())
    dif = {k: r for k, r in g["fused"].items() if "/dif/" in k}
    assert all(r["fused_steps"] > 0 for k, r in dif.items() if k.endswith("default"))
    assert all(r["fused_steps"] == 0 for r in g["generic"].values())
    # the two settings walk the same fit: a fused step leaves what the generic step leaves
    assert all(g["generic"][k]["p"] == r["p"] and g["generic"][k]["passes"] == r["passes"] for k, r in dif.items())
    # an undamped start is another walk (its first steps are rejected in a chain): for every model some size shows it in the pass count
    for model in MODELS:
        assert any(dif[k.replace("default", "tau=1e-6")]["passes"] != r["passes"] for k, r in dif.items()
                   if k.endswith("default") and k.startswith(f"single/{model}/"))


if __name__ == "__main__":
    assert sys.argv[1] == "--worker"
    _worker(sys.argv[2], sys.argv[3])
