"""Writes the two fixtures of the capture-layer tests from the library of the checked-out commit.  Run at the commit the tests compare
against:

    python scripts/gen_capture_layer_golden.py refusals [output file]   # no device: tests/golden/capture_refusals_parent.json
    python scripts/gen_capture_layer_golden.py gpu [output file]        # on the GPU: tests/golden/capture_layer_parent.json

`gpu` runs every case of tests/test_gpu_capture_layer.py twice and fails if the two runs differ.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write(out, res):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


def refusals(out):
    from tests import test_capture_layer_host as T
    res = {}
    for name, (rc, text) in T.all_refusals().items():
        assert rc == -1 and text, (name, rc, text)
        res[name] = text
    write(out or T.GOLDEN, res)


def gpu(out):
    import torch

    import brdf_amd
    from tests import test_gpu_capture_layer as T
    assert torch.cuda.is_available(), "the gpu half needs the MI355X"
    handle = (torch, brdf_amd, torch.device("cuda:0"))
    res = {}
    for name in T.case_names():
        first, second = T.run_case(handle, name), T.run_case(handle, name)
        assert first == second, (name, first, second)  # integer atomics and fixed-order sums only: two runs cannot differ
        res[name] = first
        print(name, {entry: rec["rc"] for entry, rec in first.items()}, flush=True)
    write(out or T.GOLDEN, res)


if __name__ == "__main__":
    half = sys.argv[1] if len(sys.argv) > 1 else ""
    assert half in ("refusals", "gpu"), __doc__
    {"refusals": refusals, "gpu": gpu}[half](sys.argv[2] if len(sys.argv) > 2 else None)
