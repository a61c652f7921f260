"""The resident single-fit kernels against what the commit before the plumbing change computed, byte for byte.

The change moved work inside a workgroup -- which wave stores a partial sum's exchange cell, where the fused step's next uniforms
come from -- and must not move a bit of a result.  tests/golden/resident_plumbing_parent.json holds p, info[], the covariance, the return
code, the pass count and the number of fused steps of every case below as that parent commit's library returned them on an
MI355X (scripts/gen_resident_plumbing_golden.py wrote it, from this file's case list); the test asserts the same bytes.

Sizes: the smallest that reach each case of the exchange (4096 samples per workgroup, 16 workgroups per group)
    4,096    one workgroup: no exchange, the path the change leaves alone
    4,097    five workgroups of 820 samples, the last of 817: one short group
    17,409   18 workgroups: two groups, the second with two members and a leader that is not its member 0
    262,145  256 workgroups, 770 samples in the last one
Requests: the default fits walk through init / FD or analytic Jacobian / trial / plain evaluation (with its max slot for the box
methods); tau = 1e-6 starts dlevmar_dif undamped, so its first steps are rejected in a chain (several trial points to a sweep);
the box-active families send dlevmar_bc_dif / bc_der through the projected-gradient search with several candidates to a sweep;
delta = -1e-4 takes central differences.  So every row width of the reduction -- 1, 8, 9, 10 sums and a row with a max -- is
published at least once at every multi-workgroup size.

BRDF_HIP_DIF_FUSED is read from the environment, so each setting runs in a fresh child process (this file, `--worker`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resident_plumbing_parent.json")
SIZES = (4097, 17409, 262145, 4096)
EXTRA_N = (4097, 17409)  # the sizes of the box-active and option cases
METHODS = ("dif", "bc_dif", "bc_der", "der")
BOX_ACTIVE = ("tight_box", "start_on_bound", "diffuse_only")
SETTINGS = {"fused": {"BRDF_HIP_DIF_FUSED": "1"}, "generic": {"BRDF_HIP_DIF_FUSED": "0"}}


def case_keys(setting):
    """[(problem key of tests/pass_problems.py, method, name of the opts)]; the `generic` setting: the dlevmar_dif cases only"""
    out = []
    for method in range(4):
        for model in (0, 1, 2):
            out += [(("single", model, n), method, "default") for n in SIZES]
            for n in EXTRA_N:
                if method in (0, 1):
                    out += [(("single", model, n), method, "tau=1e-6"), (("single", model, n), method, "delta=-1e-4")]
                if method in (1, 2):
                    out += [((family, model, n, 0), method, "default") for family in BOX_ACTIVE]
    return [c for c in out if setting == "fused" or c[1] == 0]


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
    for key in case_keys(setting):
        problem, method, opts = key
        angles, x, p0, lb, ub = P.problem(problem)
        box = {"lb": lb, "ub": ub} if method in (1, 2) else {}
        res = brdf_amd.fit_single(method, problem[1], torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev), p0, itmax=synth.ITMAX,
                                  opts=opts_of[opts], want_covar=True, **box)
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
    return run_settings(tmp_path_factory.mktemp("resident_plumbing"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("method", range(4), ids=METHODS)
@pytest.mark.parametrize("setting", tuple(SETTINGS))
def test_resident_fits_return_the_parents_bytes(runs, golden, setting, method):
    keys = [k for k in case_keys(setting) if k[1] == method]
    if setting == "generic":
        assert bool(keys) == (method == 0)  # (the switch reaches dlevmar_dif only: nothing to run for the others)
    wrong = []
    for key in keys:
        name = name_of(key)
        got, want = runs[setting][name], golden[setting][name]
        assert got["launches"] == 1, (name, got)  # the resident kernel ran, and did not fall back
        for field in ("ret", "p", "info", "covar", "passes", "jac_passes", "fused_steps"):
            if got[field] != want[field]:
                wrong.append((name, field, got[field], want[field]))
    print(f"{setting} {METHODS[method]}: {len(keys)} fits, {len(wrong)} fields differ")
    assert not wrong, wrong[:10]


def test_the_fixture_covers_every_case_and_every_row_width():
    with open(GOLDEN) as f:
        g = json.load(f)
    for setting in SETTINGS:
        assert sorted(g[setting]) == sorted(name_of(k) for k in case_keys(setting))
        assert all(r["launches"] == 1 and r["ret"] >= 0 for r in g[setting].values())
    dif = {k: r for k, r in g["fused"].items() if "/dif/" in k}
    assert all(r["fused_steps"] > 0 for k, r in dif.items() if k.endswith("default"))
    assert all(r["fused_steps"] == 0 for r in g["generic"].values())
    # a chain of rejections costs passes that are neither a Jacobian nor an accepted trial: the undamped start takes more of them
    assert any(dif[k.replace("default", "tau=1e-6")]["passes"] != r["passes"] for k, r in dif.items() if k.endswith("default") and "/17409/" in k)


if __name__ == "__main__":
    assert sys.argv[1] == "--worker"
    _worker(sys.argv[2], sys.argv[3])
