"""The resident dlevmar_dif kernels with and without the fused trial -> trial step (BRDF_HIP_DIF_FUSED, lm_machine.h:
DifMachine::fused_trial_step): the switch changes how the control wave walks through a step, never a bit of a result.

The switch is read from the environment, so every setting runs in a fresh child process (this file, `--worker`), which
fits every case below and writes the raw bytes of its results as JSON; the three children run side by side and the tests
compare what they wrote."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_N = (1000, 5000, 20000, 262145)  # one workgroup, no exchange | five workgroups, one partial group | two groups | full grid, short last workgroup
MODELS = (0, 1, 2)
BATCH_MODELS = (2, 1)  # Ward, Blinn-Phong
BATCH_S, BATCH_N = 32, 2048


def _worker(path):
    import torch

    import brdf_amd
    from brdf_amd import synth

    dev = torch.device("cuda:0")
    out = {}
    hexs = lambda a: np.ascontiguousarray(a).tobytes().hex()
    for model in MODELS:
        for n in SINGLE_N:
            angles, x, _ = synth.make_single(model, n)
            res = brdf_amd.fit_single(brdf_amd.METHOD_DIF, model, torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev),
                                      synth.P0[model], itmax=synth.ITMAX, opts=synth.OPTS, want_covar=True)
            st = brdf_amd.last_fit_stats()
            out[f"single/{model}/{n}"] = {"ret": int(res.ret), "p": hexs(res.p), "info": hexs(res.info), "covar": hexs(res.covar),
                                          "passes": int(st["passes"]), "fused_steps": int(st["fused_steps"]), "launches": int(st["launches"])}
    for model in BATCH_MODELS:
        angles, x, _ = synth.make_surfels(model, BATCH_N, first=0, count=BATCH_S)
        p0 = torch.from_numpy(np.tile(np.array(synth.P0[model]), (BATCH_S, 1))).to(dev)
        p, info, ret = brdf_amd.fit_batch(brdf_amd.METHOD_DIF, model, torch.from_numpy(angles).to(dev), torch.from_numpy(x).to(dev), p0,
                                          itmax=synth.ITMAX, opts=synth.OPTS)
        torch.cuda.synchronize()
        out[f"batch/{model}"] = {"p": hexs(p.cpu().numpy()), "info": hexs(info.cpu().numpy()), "ret": hexs(ret.cpu().numpy()),
                                 "min_ret": int(ret.min().item())}
    with open(path, "w") as f:
        json.dump(out, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dif_fused_gpu")
    settings = {"on": {"BRDF_HIP_DIF_FUSED": "1"}, "off": {"BRDF_HIP_DIF_FUSED": "0"}, "chain": {"BRDF_HIP_RESIDENT": "0"}}
    procs = {}
    for name, extra in settings.items():
        env = dict(os.environ, **extra)
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        if name != "chain":
            env.pop("BRDF_HIP_RESIDENT", None)
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(d / f"{name}.json")], env=env, cwd=ROOT,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for name, pr in procs.items():
        log, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, log[-3000:])
        with open(d / f"{name}.json") as f:
            res[name] = json.load(f)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", SINGLE_N)
@pytest.mark.parametrize("model", MODELS)
def test_single_fits_identical_with_and_without_the_fused_step(runs, model, n):
    on, off = runs["on"][f"single/{model}/{n}"], runs["off"][f"single/{model}/{n}"]
    print(f"model {model} n {n}: passes {on['passes']}, fused steps {on['fused_steps']} (off: {off['fused_steps']}), ret {on['ret']}")
    assert on["ret"] >= 0 and on["launches"] == 1 and off["launches"] == 1  # the resident kernel ran
    for key in ("ret", "p", "info", "covar", "passes"):
        assert on[key] == off[key], key
    assert 2 * on["fused_steps"] >= on["passes"], (on["fused_steps"], on["passes"])  # the path is taken
    assert off["fused_steps"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("model", BATCH_MODELS)
def test_batched_resident_body_identical_with_and_without_the_fused_step(runs, model):
    on, off = runs["on"][f"batch/{model}"], runs["off"][f"batch/{model}"]
    assert on["min_ret"] >= 0
    for key in ("p", "info", "ret"):
        assert on[key] == off[key], key


@pytest.mark.gpu
def test_launch_chain_never_sees_the_switch(runs):
    # BRDF_HIP_RESIDENT=0: one launch per pass, the generic step only.  A smoke check: the two regimes sum in different trees, so
    # bits differ; each is within 1e-5 relative of the CPU path (tests/test_gpu_parity.py: P_TOL), hence within 2e-5 of the other
    for model in MODELS:
        for n in SINGLE_N:
            ch, on = runs["chain"][f"single/{model}/{n}"], runs["on"][f"single/{model}/{n}"]
            assert ch["ret"] >= 0 and ch["fused_steps"] == 0 and ch["launches"] > 1
            p_ch, p_on = np.frombuffer(bytes.fromhex(ch["p"])), np.frombuffer(bytes.fromhex(on["p"]))
            assert np.max(np.abs(p_ch - p_on) / np.abs(p_on)) <= 2e-5, (model, n, p_ch, p_on)


if __name__ == "__main__":
    assert sys.argv[1] == "--worker"
    _worker(sys.argv[2])
