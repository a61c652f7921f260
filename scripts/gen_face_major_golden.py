"""Writes tests/golden/face_major_parent.json from the library of the checked-out commit (or the one BRDF_HIP_LIB names).  Run on the
GPU with the library of the commit the test compares against:

    python scripts/gen_face_major_golden.py [output file]

Runs every case of tests/test_gpu_face_major.py twice and fails if the two runs differ.  "_made_by" in the file names the library
(its path and sha256) and the commit that was checked out.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch

    import brdf_amd
    from scripts.gen_capture_layer_golden import write
    from tests import test_gpu_face_major as T
    assert torch.cuda.is_available(), "needs the MI355X"
    print("library", brdf_amd.LIB_PATH, flush=True)
    handle = (torch, brdf_amd, torch.device("cuda:0"))
    res = {}
    for name in T.case_names():
        first, second = T.run_case(handle, name), T.run_case(handle, name)
        assert first == second, (name, first, second)  # integer atomics and fixed-order sums only: two runs cannot differ
        res[name] = first
        print(name, {k: v for k, v in first.items() if k != "sha256"}, flush=True)
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    with open(brdf_amd.LIB_PATH, "rb") as f:
        res["_made_by"] = {"library_sha256": hashlib.sha256(f.read()).hexdigest(), "library": os.path.relpath(brdf_amd.LIB_PATH, ROOT),
                           "checked_out_commit": head, "note": "the library was built from the commit before capture_face_major.hip"}
    write(out or T.GOLDEN, res)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
