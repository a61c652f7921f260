"""brdf_hip_fit_batch_multi against brdf_hip_fit_batch: wall time, per-shard upload / fit / download, throughput and a hash of
the results, for several device lists.  Inputs are made on device 0 by brdf_hip_synth_dev (faster than numpy at the
configs[3] / configs[4] sizes) and copied to host memory, as a C caller would hold them.

usage: python scripts/gpu_multi_scaling.py --surfels 65536 --n 4096 --method dif --model ward [--devices 0,0 --devices 0,1 ...]
       [--repeat R] [--out FILE]
Without --devices: 1, 2, 4 and 8 distinct GPUs where this process sees them, and [0], [0,0], [0,0,0,0].  One JSON line per
timed call; --out also writes them as one JSON document.  A device list timed on one GPU says nothing about several GPUs."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brdf_amd
from brdf_amd import synth
from brdf_amd._lib import lib

METHODS = {"dif": 0, "bc_dif": 1, "bc_der": 2, "der": 3}
MODELS = {"phong": 0, "blinn_phong": 1, "ward": 2}


def ptr(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=int, required=True)
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--method", choices=sorted(METHODS), default="dif")
    ap.add_argument("--model", choices=sorted(MODELS), default="ward")
    ap.add_argument("--devices", action="append", default=None, help="comma-separated HIP ordinals; repeat for several lists")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    S, n, method, model = args.surfels, args.n, METHODS[args.method], MODELS[args.model]
    visible = lib.brdf_hip_device_count()
    if args.devices:
        lists = [[int(d) for d in s.split(",")] for s in args.devices]
    else:
        lists = [list(range(g)) for g in (1, 2, 4, 8) if g <= visible]
        lists += [l for l in ([0], [0, 0], [0, 0, 0, 0]) if l not in lists]

    # inputs: device 0 -> host
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    truth = torch.from_numpy(synth.surfel_truth(model, 0, S)).to(dev)
    a_d = torch.empty((S, 3, n), dtype=torch.float64, device=dev)
    x_d = torch.empty((S, n), dtype=torch.float64, device=dev)
    assert lib.brdf_hip_synth_dev(model, synth.SEED, 0, S, n, truth.data_ptr(), a_d.data_ptr(), x_d.data_ptr(), None) == 0
    angles, x = a_d.cpu().numpy(), x_d.cpu().numpy()
    del a_d, x_d, truth
    torch.cuda.empty_cache()
    synth_s = time.perf_counter() - t0
    p0 = np.tile(np.array(synth.P0[model], dtype=np.float64), (S, 1))
    lb, ub = (np.array(v, dtype=np.float64) for v in synth.bounds(model))
    opts = np.array(synth.OPTS, dtype=np.float64)

    def run(devices):
        p, info, ret = p0.copy(), np.zeros((S, 10)), np.zeros(S, dtype=np.int32)
        common = (method, model, ptr(angles), ptr(x), S, n, ptr(p), ptr(lb), ptr(ub), synth.ITMAX, ptr(opts), ptr(info), ptr(ret, C.c_int))
        t = time.perf_counter()
        if devices is None:
            rc = lib.brdf_hip_fit_batch(*common)
        else:
            rc = lib.brdf_hip_fit_batch_multi(*common, (C.c_int * len(devices))(*devices), len(devices))
        wall = time.perf_counter() - t
        if rc < 0:
            raise SystemExit(f"{'brdf_hip_fit_batch' if devices is None else devices}: {brdf_amd.last_error()}")
        return rc, wall, p, info, ret

    # warm-up: code objects, contexts and the runtime's own first-call costs on every device that is used, outside the timing
    small = min(S, 64)
    for d in sorted({d for l in lists for d in l}):
        p, info, ret = p0[:small].copy(), np.zeros((small, 10)), np.zeros(small, dtype=np.int32)
        lib.brdf_hip_fit_batch_multi(method, model, ptr(angles), ptr(x), small, n, ptr(p), ptr(lb), ptr(ub), synth.ITMAX, ptr(opts),
                                     ptr(info), ptr(ret, C.c_int), (C.c_int * 1)(d), 1)
    p, info, ret = p0[:small].copy(), np.zeros((small, 10)), np.zeros(small, dtype=np.int32)
    lib.brdf_hip_fit_batch(method, model, ptr(angles), ptr(x), small, n, ptr(p), ptr(lb), ptr(ub), synth.ITMAX, ptr(opts), ptr(info),
                           ptr(ret, C.c_int))

    records = []
    single_sha = None
    for rep in range(args.repeat):
        for devices in [None] + lists:
            rc, wall, p, info, ret = run(devices)
            sha = hashlib.sha256(p.tobytes() + info.tobytes() + ret.tobytes()).hexdigest()
            if devices is None:
                single_sha = sha
            rec = {"entry": "brdf_hip_fit_batch" if devices is None else "brdf_hip_fit_batch_multi", "devices": devices,
                   "distinct_devices": 1 if devices is None else len(set(devices)), "rep": rep, "surfels": S, "n": n,
                   "method": args.method, "model": args.model, "wall_ms": wall * 1e3, "failed_fits": rc,
                   "fits_per_s": S / wall, "residual_evals_per_s": float(info[:, 7].sum()) * n / wall,
                   "mean_nfev": float(info[:, 7].mean()), "result_sha256": sha, "same_as_brdf_hip_fit_batch": sha == single_sha}
            if devices is not None:
                rec["shards"] = [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in s.items()} for s in brdf_amd.last_multi_stats()]
            print(json.dumps(rec), flush=True)
            records.append(rec)
    if args.out:
        doc = {"visible_devices": visible, "device_name": torch.cuda.get_device_name(0), "synth_and_copy_to_host_s": synth_s,
               "host_bytes_of_inputs": int(angles.nbytes + x.nbytes), "runs": records}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
