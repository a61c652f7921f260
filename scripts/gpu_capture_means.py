"""The per-face capture over per-light means (brdf_hip_fit_capture_means_dev) next to the per-face capture over all samples
(brdf_hip_fit_capture_faces_dev) and the last-pixel-wins capture (brdf_hip_fit_capture_masked_dev), on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py (scripts/gpu_capture_faces.py's make_capture).  The three calls
run on the same inputs with the same rule -- off, and v_min = 1, v_max = 254, cos_min = 0 --, alternating; all three synchronise, so
the device-synchronised wall time of a call is its cost.  Reported per rule: the median of --reps calls each, the ratio means / faces,
the share of the grouping, accumulation and packing in the means call (a call with itmax = 0 and without statistics: an UPPER bound, it
still launches the fit kernel once), and the largest relative difference of p between the means and the faces capture over the fits that
converged in both (the two fits have the same minimiser).  Writes profiles/capture_means.json (or --out).

    python scripts/gpu_capture_means.py [--out FILE] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_capture_faces import OPTS, make_capture, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_means.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    mesh = make_capture(torch, brdf_amd, dev)
    out = []
    for name, rule in (("rule off", dict()), ("v_min 1, v_max 254, cos_min 0", dict(v_min=1, v_max=254, cos_min=0.0))):
        def means(**kw):
            return brdf_amd.fit_capture_means(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule, **kw)

        def faces():
            return brdf_amd.fit_capture_faces(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule)

        def masked():
            return brdf_amd.fit_capture_masked(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule)

        def accumulate_only():
            return brdf_amd.fit_capture_means(1, *mesh, rv_mode=1, opts=OPTS, validate=False, itmax=0, want_stats=False, **rule)

        rm, rf, _, _ = means(), faces(), masked(), accumulate_only()  # warm-up
        t_means, t_faces, t_masked, t_acc = [], [], [], []
        for _ in range(args.reps):  # alternating
            t_means.append(wall(torch, means)[0])
            t_faces.append(wall(torch, faces)[0])
            t_masked.append(wall(torch, masked)[0])
            t_acc.append(wall(torch, accumulate_only)[0])
        carried = rm.face_pixels.cpu().numpy() > 0
        info_m, info_f = rm.info.cpu().numpy()[carried], rf.info.cpu().numpy()[carried]
        ret_m, ret_f = rm.ret.cpu().numpy()[carried], rf.ret.cpu().numpy()[carried]
        p_m, p_f = rm.surfaces.cpu().numpy()[carried], rf.surfaces.cpu().numpy()[carried]
        both = (ret_m >= 0) & (ret_f >= 0) & (info_m[..., 6] != 3) & (info_f[..., 6] != 3)  # reason 3: stopped by itmax
        rel = np.max(np.abs(p_m - p_f) / np.maximum(np.abs(p_f), 1e-12), axis=-1)
        # the full-sample objective of both: stats[0] of the means capture is info[1] + within, info[1] of the faces capture is its own
        obj_m, obj_f = rm.stats.stats.cpu().numpy()[carried][..., 0], info_f[..., 1]
        ok = (ret_m >= 0) & (ret_f >= 0)
        med = statistics.median
        entry = dict(rule=name, image=[1024, 1024], lights=16, pixels=rm.n_pixels, faces=rm.n_faces, fits=3 * rm.n_faces,
                     samples=int(rm.count.cpu().numpy()[carried].sum()), fits_refused_means=int((ret_m < 0).sum()), fits_refused_faces=int((ret_f < 0).sum()),
                     timing="device-synchronised wall time of one call, median; the calls alternate", reps=args.reps,
                     means_s=med(t_means), means_s_min=min(t_means), means_s_max=max(t_means),
                     faces_s=med(t_faces), faces_s_min=min(t_faces), faces_s_max=max(t_faces),
                     masked_s=med(t_masked), masked_s_min=min(t_masked), masked_s_max=max(t_masked),
                     accumulate_and_pack_s_upper_bound=med(t_acc), accumulate_and_pack_s_min=min(t_acc), accumulate_and_pack_s_max=max(t_acc),
                     means_over_faces=med(t_means) / med(t_faces), means_over_masked=med(t_means) / med(t_masked),
                     accumulate_and_pack_share_of_means=med(t_acc) / med(t_means),
                     fits_converged_in_both=int(both.sum()), largest_relative_difference_of_p_converged_in_both=float(rel[both].max()) if both.any() else None,
                     fits_within_1e_5_on_p_converged_in_both=int((rel[both] <= 1e-5).sum()),
                     means_objective_above_faces_by_more_than_1e_6=int((obj_m[ok] > obj_f[ok] * (1 + 1e-6)).sum()),
                     faces_objective_above_means_by_more_than_1e_6=int((obj_f[ok] > obj_m[ok] * (1 + 1e-6)).sum()),
                     avg_means=[float(v) for v in rm.avg], avg_faces=[float(v) for v in rf.avg])
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
