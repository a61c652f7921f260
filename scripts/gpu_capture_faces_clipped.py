"""The per-face capture with sigma-clipped fits (brdf_hip_fit_capture_faces_clipped_dev) next to fit_capture_faces, on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py, as scripts/gpu_capture_faces.py builds it.  With the rule off
and with v_min = 1, v_max = 254, cos_min = 0, three calls alternate: fit_capture_faces, the clipped entry at rounds = 0 (the same
launches: its median has to lie inside fit_capture_faces' min ... max of this job) and the clipped entry at rounds = 3, kappa = 2.5,
sigma_min = 1 / (255 sqrt 12).  All calls synchronise, so the device-synchronised wall time of a call is its cost.

Per clip round the job reports the fits that were clipped and refitted and the samples dropped (brdf_amd.last_clip_stats).  The cost
of the clip rounds without their refits is bounded from above by two calls with itmax = 0 and without statistics maps, at rounds = 3 and
at rounds = 0: every fit stops at once, so the difference is the rounds' statistics calls, clip passes and refit launches.  The cost
of the clip rounds is reported, not bounded.  Writes profiles/capture_faces_clipped.json (or --out).

    python scripts/gpu_capture_faces_clipped.py [--out FILE] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_capture_faces import OPTS, make_capture, wall  # noqa: E402

KAPPA, ROUNDS = 2.5, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_faces_clipped.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    mesh = make_capture(torch, brdf_amd, dev)
    out = []
    for name, rule in (("rule off", dict()), ("v_min 1, v_max 254, cos_min 0", dict(v_min=1, v_max=254, cos_min=0.0))):
        def faces():
            return brdf_amd.fit_capture_faces(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule)

        def clipped(rounds, **kw):
            return brdf_amd.fit_capture_faces_clipped(1, *mesh, kappa=KAPPA, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=rounds, rv_mode=1, opts=OPTS,
                                                      validate=False, **rule, **kw)

        plain, c0, c3 = faces(), clipped(0), clipped(ROUNDS)  # warm-up
        rounds = brdf_amd.last_clip_stats()
        clipped(ROUNDS, itmax=0, want_stats=False), clipped(0, itmax=0, want_stats=False)
        same = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()  # (bytes: a NaN equals itself)
                   for a, b in ((plain.surfaces, c0.surfaces), (plain.info, c0.info), (plain.ret, c0.ret), (plain.count, c0.count),
                                (plain.stats.covar, c0.stats.covar), (plain.stats.stats, c0.stats.stats), (plain.stats.rank, c0.stats.rank)))
        t = {k: [] for k in ("faces", "rounds0", "rounds3", "passes3", "passes0")}
        for _ in range(args.reps):  # alternating
            t["faces"].append(wall(torch, faces)[0])
            t["rounds0"].append(wall(torch, lambda: clipped(0))[0])
            t["rounds3"].append(wall(torch, lambda: clipped(ROUNDS))[0])
            t["passes3"].append(wall(torch, lambda: clipped(ROUNDS, itmax=0, want_stats=False))[0])
            t["passes0"].append(wall(torch, lambda: clipped(0, itmax=0, want_stats=False))[0])
        med = {k: statistics.median(v) for k, v in t.items()}
        carried = plain.face_pixels.cpu().numpy() > 0
        count, kept = c3.count.cpu().numpy()[carried], c3.kept.cpu().numpy()[carried]
        entry = dict(rule=name, image=[1024, 1024], lights=16, pixels=plain.n_pixels, faces=plain.n_faces, fits=3 * plain.n_faces,
                     samples=int(count.sum()), kappa=KAPPA, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=ROUNDS,
                     timing="device-synchronised wall time of one call, median; the calls alternate", reps=args.reps,
                     faces_s=med["faces"], faces_s_min=min(t["faces"]), faces_s_max=max(t["faces"]),
                     rounds0_s=med["rounds0"], rounds0_s_min=min(t["rounds0"]), rounds0_s_max=max(t["rounds0"]),
                     rounds0_inside_faces_min_max=bool(min(t["faces"]) <= med["rounds0"] <= max(t["faces"])), rounds0_same_bytes=bool(same),
                     rounds3_s=med["rounds3"], rounds3_s_min=min(t["rounds3"]), rounds3_s_max=max(t["rounds3"]),
                     rounds3_over_faces=med["rounds3"] / med["faces"],
                     per_round=[dict(round=i + 1, fits_clipped_and_refitted=r["active"], samples_dropped=r["clipped"]) for i, r in enumerate(rounds)],
                     samples_kept=int(kept.sum()), fits_with_a_dropped_sample=int((kept < count).sum()),
                     clip_rounds_without_refits_s_upper_bound=med["passes3"] - med["passes0"], itmax0_rounds3_s=med["passes3"], itmax0_rounds0_s=med["passes0"])
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    assert all(e["rounds0_same_bytes"] for e in out), "rounds = 0 differs from fit_capture_faces"
    assert all(e["rounds0_inside_faces_min_max"] for e in out), "the median of rounds = 0 lies outside fit_capture_faces' min ... max"


if __name__ == "__main__":
    main()
