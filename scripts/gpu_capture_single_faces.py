"""The single-BRDF capture over every valid sample (brdf_hip_fit_capture_single_faces_dev) next to the last-pixel single-BRDF capture
(brdf_hip_fit_capture_single_dev, unchanged since the parent commit), on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py (scripts/gpu_capture_faces.py's make_capture).  Per rule -- off,
and v_min = 1, v_max = 254, cos_min = 0 -- four calls alternate on the same inputs, all of them synchronising, so the device-synchronised
wall time of a call is its cost:
    full        the new entry with the statistics and the face maps
    fit only    the new entry without statistics and without face maps
    pack only   the new entry with itmax = 0, without statistics and face maps: grouping + packing and three fits that stop at once,
                an UPPER bound of the grouping and packing
    last pixel  fit_capture_single with the same start, box, itmax and opts (it knows no rule: the same call under both)
The two entries fit different sample sets (every valid sample against 16 per carried face): there is no pass/fail threshold.  Reported
per rule: the medians of --reps calls, K_c, the regime of each channel's fit (resident up to 2^20 samples, the launch chain above; the
last channel's launch count is read back as a check), the channels' results of both entries.  Writes profiles/capture_single_faces.json
(or --out).

    python scripts/gpu_capture_single_faces.py [--out FILE] [--reps 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_capture_faces import OPTS, make_capture, wall  # noqa: E402

P0, LB, UB, ITMAX = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0), 100
RESIDENT_MAX = 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_single_faces.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    from brdf_amd import fit as F
    dev = torch.device("cuda:0")
    mesh = make_capture(torch, brdf_amd, dev)
    out = []
    for name, rule in (("rule off", dict(v_min=0, v_max=255, cos_min=-2.0)), ("v_min 1, v_max 254, cos_min 0", dict(v_min=1, v_max=254, cos_min=0.0))):
        def full():
            return brdf_amd.fit_capture_single_faces(1, *mesh, rv_mode=1, p0=P0, lb=LB, ub=UB, itmax=ITMAX, opts=OPTS, validate=False, **rule)

        def bare(itmax):
            """the C entry without statistics and without face maps"""
            a, _, _ = F._capture_args(1, *mesh, 1, P0, LB, UB, itmax, OPTS, False)
            single = np.zeros((3, 3))
            rc = brdf_amd.lib.brdf_hip_fit_capture_single_faces_dev(*a, rule["v_min"], rule["v_max"], rule["cos_min"], F._dptr(single), None, None, None,
                                                                    None, None, None, None, None, None, None, None,
                                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc >= 0, brdf_amd.last_error()
            return single

        def last_pixel():
            return brdf_amd.fit_capture_single(1, *mesh, rv_mode=1, p0=P0, lb=LB, ub=UB, itmax=ITMAX, opts=OPTS, validate=False)

        r = full()  # warm-up
        last = brdf_amd.last_fit_stats()
        old = last_pixel()
        bare(ITMAX), bare(0)
        t_full, t_fit, t_pack, t_old = [], [], [], []
        for _ in range(args.reps):  # alternating
            t_full.append(wall(torch, full)[0])
            t_fit.append(wall(torch, lambda: bare(ITMAX))[0])
            t_pack.append(wall(torch, lambda: bare(0))[0])
            t_old.append(wall(torch, last_pixel)[0])
        med = statistics.median
        face_sumsq = r.face_sumsq.cpu().numpy()
        entry = dict(rule=name, image=[1024, 1024], lights=16, pixels=r.n_pixels, faces=r.n_faces, samples_per_channel=[int(k) for k in r.count],
                     regime_per_channel=["resident" if k <= RESIDENT_MAX else "launch chain" for k in r.count],
                     launches_of_the_last_channels_fit=int(last["launches"]), passes_of_the_last_channels_fit=int(last["passes"]),
                     samples_of_the_last_pixel_fit=16 * int(old[2]),
                     timing="device-synchronised wall time of one call, median; the calls alternate", reps=args.reps,
                     full_s=med(t_full), full_s_min=min(t_full), full_s_max=max(t_full),
                     fit_only_s=med(t_fit), fit_only_s_min=min(t_fit), fit_only_s_max=max(t_fit),
                     group_and_pack_s_upper_bound=med(t_pack), group_and_pack_s_min=min(t_pack), group_and_pack_s_max=max(t_pack),
                     last_pixel_s=med(t_old), last_pixel_s_min=min(t_old), last_pixel_s_max=max(t_old),
                     statistics_and_face_maps_s=med(t_full) - med(t_fit), full_over_last_pixel=med(t_full) / med(t_old),
                     group_and_pack_share_of_full=med(t_pack) / med(t_full),
                     ret=[int(v) for v in r.ret], reason=[float(v) for v in r.info[:, 6]], iterations=[float(v) for v in r.info[:, 5]],
                     single_brdf=[[float(v) for v in row] for row in r.single_brdf], sumsq=[float(v) for v in r.stats.stats[:, 0]],
                     r2=[float(v) for v in r.stats.stats[:, 1]], face_map_sum=[float(v) for v in face_sumsq.sum(axis=0)],
                     single_brdf_last_pixel=[[float(v) for v in row] for row in old[0]], reason_last_pixel=[float(v) for v in old[1][:, 6]])
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
