"""Writes tests/golden/trial_head_parent.json: what the library of the checked-out commit (or the one BRDF_HIP_LIB names) returns
for every case of tests/test_gpu_trial_head.py, as hex bytes.  Run once on the GPU with the library of the commit the test
compares against:

    python scripts/gen_trial_head_golden.py [output file]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_trial_head as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
with tempfile.TemporaryDirectory() as d:
    res = T.run_settings(d)
bad = [(s, k) for s, recs in res.items() for k, r in recs.items() if r["launches"] != 1 or r["ret"] < 0]
assert not bad, bad  # every case must be a resident fit that succeeds
for setting, recs in res.items():
    print(setting, len(recs), "fits; passes", min(r["passes"] for r in recs.values()), "..", max(r["passes"] for r in recs.values()), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", out, os.path.getsize(out), "bytes")
