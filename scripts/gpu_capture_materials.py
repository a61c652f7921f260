"""K materials per object (brdf_hip_fit_capture_materials_dev) next to the single-BRDF capture over every valid sample
(brdf_hip_fit_capture_single_faces_dev, unchanged since the parent commit), on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py (scripts/gpu_capture_faces.py's make_capture) under the rule
v_min = 1, v_max = 254, cos_min = 0.  Per K in 1, 4, 16, with the seeds of brdf_amd.seed_materials, four calls alternate on the same
inputs, all of them synchronising, so the device-synchronised wall time of a call is its cost:
    materials   fit_capture_materials at rounds = 5, with the statistics
    residuals   fit_capture_materials at rounds = 0: grouping, the face-major placing, ONE residual pass against K materials, the
                assignment and the last residual pass -- two passes in all
    regroup     fit_capture_labelled with itmax = 0 and without statistics on the labels `materials` returned: grouping, the label-major
                regrouping and 3 K fits that stop at once, an UPPER bound of the regrouping
    single      fit_capture_single_faces with the statistics and the face maps
The new entries answer another question than the single fit: there is no pass/fail threshold.  Reported per K: the medians of --reps
calls, the rounds used, the changed faces per assignment, the faces per label, the total sum of squares against the faces' own
materials and the single fit's.  Writes profiles/capture_materials.json (or --out).

    python scripts/gpu_capture_materials.py [--out FILE] [--reps 5]
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

P0, LB, UB, ITMAX, ROUNDS = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0), 100, 5
RULE = dict(v_min=1, v_max=254, cos_min=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_materials.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 4, 16])
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    mesh = make_capture(torch, brdf_amd, dev)
    kw = dict(rv_mode=1, lb=LB, ub=UB, itmax=ITMAX, opts=OPTS, validate=False, **RULE)

    def single():
        return brdf_amd.fit_capture_single_faces(1, *mesh, p0=P0, **kw)

    t_seed, face_fits = wall(torch, lambda: brdf_amd.fit_capture_faces(1, *mesh, p0=P0, want_stats=False, **kw))
    s = single()
    single_total = float(s.face_sumsq.sum())
    out = []
    for K in args.K:
        t_seeds, seeds = wall(torch, lambda: brdf_amd.seed_materials(K, 1, *mesh, face_fits=face_fits, p0=P0, **kw))

        def materials(rounds=ROUNDS):
            return brdf_amd.fit_capture_materials(1, *mesh, seeds, rounds=rounds, want_stats=rounds > 0, **kw)

        r = materials()  # warm-up
        labels = r.labels.clone()

        def regroup():
            return brdf_amd.fit_capture_labelled(1, *mesh, labels, r.materials.clone(), want_stats=False, **{**kw, "itmax": 0})

        materials(0), regroup()
        t_mat, t_res, t_reg, t_single = [], [], [], []
        for _ in range(args.reps):  # alternating
            t_mat.append(wall(torch, materials)[0])
            t_res.append(wall(torch, lambda: materials(0))[0])
            t_reg.append(wall(torch, regroup)[0])
            t_single.append(wall(torch, single)[0])
        med = statistics.median
        finite = torch.isfinite(r.face_sumsq)
        entry = dict(K=K, rounds=ROUNDS, image=[1024, 1024], lights=16, rule="v_min 1, v_max 254, cos_min 0", pixels=r.n_pixels, faces=r.n_faces,
                     samples_per_channel=[int(k) for k in s.count], timing="device-synchronised wall time of one call, median; the calls alternate",
                     reps=args.reps, seeding_s=t_seeds, per_face_fits_for_the_seeds_s=t_seed,
                     materials_s=med(t_mat), materials_s_min=min(t_mat), materials_s_max=max(t_mat),
                     residuals_rounds_0_s=med(t_res), residuals_rounds_0_s_min=min(t_res), residuals_rounds_0_s_max=max(t_res),
                     regroup_itmax_0_s_upper_bound=med(t_reg), regroup_itmax_0_s_min=min(t_reg), regroup_itmax_0_s_max=max(t_reg),
                     single_s=med(t_single), single_s_min=min(t_single), single_s_max=max(t_single), materials_over_single=med(t_mat) / med(t_single),
                     rounds_used=r.rounds_used, settled=r.settled, changed_per_assignment=[int(n) for n in r.changed],
                     faces_per_label=[int(n) for n in r.label_faces.cpu().numpy()], unassigned_carried_faces=int(((r.labels < 0) & (r.face_pixels > 0)).sum()),
                     total_sumsq=float(r.face_sumsq[finite].sum()), total_sumsq_single=single_total,
                     ret=r.ret.cpu().numpy().tolist(), reason=r.info[:, :, 6].cpu().numpy().tolist(),
                     materials=np.round(r.materials.cpu().numpy(), 6).tolist())
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
