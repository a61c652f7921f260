"""The per-light-means capture with sigma-clipped fits (brdf_hip_fit_capture_means_clipped_dev) next to fit_capture_means (what the
capture did before) and next to fit_capture_faces_clipped (the other clipped capture), on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py, as scripts/gpu_capture_faces.py builds it.  With the rule off
and with v_min = 1, v_max = 254, cos_min = 0, the calls alternate: fit_capture_means, the clipped entry at rounds = 0 (the same bytes;
whether its median lies inside fit_capture_means' min ... max of this job is reported), the clipped entry at rounds = 3, kappa = 2.5,
sigma_min = 1 / (255 sqrt 12), and fit_capture_faces_clipped at the same settings.  All calls synchronise, so the device-synchronised
wall time of a call is its cost.  One process.

Per clip round the job reports the fits that were clipped and refitted and the samples dropped (brdf_amd.last_clip_stats).  The cost
of the clip rounds without their refits comes from two calls with itmax = 0 and without statistics maps, at rounds = 3 and at
rounds = 0: every fit stops at once, so the difference is the rounds' statistics calls, interval and accumulate passes and refit
launches.  Over the fits that converge in both clipped captures: how many agree on kept and, of those, to 1e-5 on p -- a figure, not a
bar: the two captures refit from fits that differ in the last bits.  Writes profiles/capture_means_clipped.json (or --out).

    timeout -k 10 900 python scripts/gpu_capture_means_clipped.py [--out FILE] [--reps 5]
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

KAPPA, ROUNDS = 2.5, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_means_clipped.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    mesh = make_capture(torch, brdf_amd, dev)
    out = []
    for name, rule in (("rule off", dict()), ("v_min 1, v_max 254, cos_min 0", dict(v_min=1, v_max=254, cos_min=0.0))):
        def means():
            return brdf_amd.fit_capture_means(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule)

        def clipped(rounds, **kw):
            return brdf_amd.fit_capture_means_clipped(1, *mesh, kappa=KAPPA, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=rounds, rv_mode=1, opts=OPTS,
                                                      validate=False, **rule, **kw)

        def faces_clipped():
            return brdf_amd.fit_capture_faces_clipped(1, *mesh, kappa=KAPPA, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=ROUNDS, rv_mode=1, opts=OPTS,
                                                      validate=False, **rule)

        plain, c0, fc = means(), clipped(0), faces_clipped()  # warm-up
        faces_rounds = brdf_amd.last_clip_stats()
        c3 = clipped(ROUNDS)
        rounds = brdf_amd.last_clip_stats()
        clipped(ROUNDS, itmax=0, want_stats=False)
        rounds_itmax0 = brdf_amd.last_clip_stats()  # (at p0 every fit: the rounds that ran there)
        clipped(0, itmax=0, want_stats=False)
        same = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()  # (bytes: a NaN equals itself)
                   for a, b in ((plain.surfaces, c0.surfaces), (plain.info, c0.info), (plain.ret, c0.ret), (plain.count, c0.count), (plain.lights, c0.lights),
                                (plain.stats.covar, c0.stats.covar), (plain.stats.stats, c0.stats.stats), (plain.stats.rank, c0.stats.rank)))
        t = {k: [] for k in ("means", "rounds0", "rounds3", "faces_clipped", "passes3", "passes0")}
        for _ in range(args.reps):  # alternating
            t["means"].append(wall(torch, means)[0])
            t["rounds0"].append(wall(torch, lambda: clipped(0))[0])
            t["rounds3"].append(wall(torch, lambda: clipped(ROUNDS))[0])
            t["faces_clipped"].append(wall(torch, faces_clipped)[0])
            t["passes3"].append(wall(torch, lambda: clipped(ROUNDS, itmax=0, want_stats=False))[0])
            t["passes0"].append(wall(torch, lambda: clipped(0, itmax=0, want_stats=False))[0])
        med = {k: statistics.median(v) for k, v in t.items()}
        carried = plain.face_pixels.cpu().numpy() > 0
        count, kept = c3.count.cpu().numpy()[carried], c3.kept.cpu().numpy()[carried]
        # the two clipped captures, over the fits that converge in both
        f_kept, f_ret, f_p = fc.kept.cpu().numpy()[carried], fc.ret.cpu().numpy()[carried], fc.surfaces.cpu().numpy()[carried]
        m_ret, m_p = c3.ret.cpu().numpy()[carried], c3.surfaces.cpu().numpy()[carried]
        both = (f_ret >= 0) & (m_ret >= 0)
        same_kept = both & (f_kept == kept)
        rel = np.max(np.abs(m_p - f_p), axis=-1) / np.maximum(np.max(np.abs(f_p), axis=-1), 1e-300)
        entry = dict(rule=name, image=[1024, 1024], lights=16, pixels=plain.n_pixels, faces=plain.n_faces, fits=3 * plain.n_faces,
                     samples=int(count.sum()), kappa=KAPPA, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=ROUNDS,
                     timing="device-synchronised wall time of one call, median; the calls alternate", reps=args.reps,
                     means_s=med["means"], means_s_min=min(t["means"]), means_s_max=max(t["means"]),
                     rounds0_s=med["rounds0"], rounds0_s_min=min(t["rounds0"]), rounds0_s_max=max(t["rounds0"]),
                     rounds0_inside_means_min_max=bool(min(t["means"]) <= med["rounds0"] <= max(t["means"])), rounds0_same_bytes=bool(same),
                     rounds3_s=med["rounds3"], rounds3_s_min=min(t["rounds3"]), rounds3_s_max=max(t["rounds3"]),
                     rounds3_over_means=med["rounds3"] / med["means"],
                     faces_clipped_s=med["faces_clipped"], faces_clipped_s_min=min(t["faces_clipped"]), faces_clipped_s_max=max(t["faces_clipped"]),
                     faces_clipped_over_rounds3=med["faces_clipped"] / med["rounds3"],
                     per_round=[dict(round=i + 1, fits_clipped_and_refitted=r["active"], samples_dropped=r["clipped"]) for i, r in enumerate(rounds)],
                     faces_clipped_per_round=[dict(round=i + 1, fits_clipped_and_refitted=r["active"], samples_dropped=r["clipped"])
                                              for i, r in enumerate(faces_rounds)],
                     samples_kept=int(kept.sum()), fits_with_a_dropped_sample=int((kept < count).sum()),
                     clip_rounds_without_refits_s=med["passes3"] - med["passes0"], itmax0_rounds3_s=med["passes3"], itmax0_rounds0_s=med["passes0"],
                     itmax0_per_round=[dict(round=i + 1, fits_clipped_and_refitted=r["active"], samples_dropped=r["clipped"]) for i, r in enumerate(rounds_itmax0)],
                     fits_converged_in_both_clipped_captures=int(both.sum()), of_those_same_kept=int(same_kept.sum()),
                     of_those_p_within_1e_5=int((rel[same_kept] <= 1e-5).sum()))
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    assert all(e["rounds0_same_bytes"] for e in out), "rounds = 0 differs from fit_capture_means"


if __name__ == "__main__":
    main()
