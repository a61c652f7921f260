"""Cast shadows on the GPU (brdf_hip_light_visibility_dev, brdf_hip_capture_apply_visibility_dev): what the two calls cost, next to a
capture fit and next to a copy of the images' bytes.

  visibility  the 40,000-triangle jittered grid of scripts/gpu_pixel_map.py with --blockers floating quads above it (two triangles
              each), under the 16 lights of led_table re-posed over the grid: scaled so that the rig spans the grid, its centre over
              the grid's, 1.5 above it.  With and without normals.  The arithmetic a call issues is counted from the definition:
              17 operations per (origin, occluder) and 24 per (origin, occluder, light), comparisons and selects not counted, early
              stops ignored -- an upper bound of the work done, so the rate derived from it is an upper bound too.
  painting    16 images of 1024 x 1024 (50.3 MB), in place and out of place, against a device-to-device copy of the same bytes.
  timings     the calls alternate on the same inputs in one process, all of them synchronising, so the device-synchronised wall time
              of a call is its cost; medians of --reps.  `means` is fit_capture_means on the synthetic 1024 x 1024 capture of
              scripts/gpu_capture_faces.py.  The ratios are reported; there is no threshold.
Not measured: kernel times by rocprofv3 (these are wall times of whole calls), other mesh sizes and light counts, the split's and the
early stop's separate effects.
Writes profiles/light_visibility.json (or --out).

    python scripts/gpu_light_visibility.py [--out FILE] [--reps 5] [--blockers 200]
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
from gpu_pixel_map import make_mesh  # noqa: E402

H = W = 1024
FP64_VECTOR_PEAK = 78.6e12  # the MI355X data sheet's vector fp64 peak, counted with fused multiply-adds


def add_blockers(v, f, quads, seed=9):
    """the mesh with `quads` floating quads over it: side 0.15, 0.2 to 0.6 above the grid, counter-clockwise seen from above"""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform(-1.0, 1.0, size=(quads, 2)), rng.uniform(0.2, 0.6, size=(quads, 1))], axis=1)
    corners = np.array([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)]) * 0.15
    qv = (c[:, None, :] + corners[None]).reshape(-1, 3)
    base = v.shape[0] + 4 * np.arange(quads)
    qf = np.stack([np.stack([base, base + 1, base + 2], axis=1), np.stack([base, base + 2, base + 3], axis=1)], axis=1).reshape(-1, 3)
    return np.concatenate([v, qv]), np.concatenate([f, qf]).astype(np.int32)


def pose_rig(leds):
    """led_table's 16 positions, re-posed over the grid: centred, scaled to span 2 in x and y, lifted to z >= 1.5"""
    p = leds - leds.mean(axis=0)
    p = p * (2.0 / max(np.ptp(p[:, 0]), np.ptp(p[:, 1])))
    p[:, 2] = 1.5 + np.abs(p[:, 2])
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_visibility.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blockers", type=int, default=200)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    med = statistics.median
    v, f, _, _ = make_mesh()
    v, f = add_blockers(v, f, args.blockers)
    leds = pose_rig(brdf_amd.led_table())
    tv, tf = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (v, f))
    tn = brdf_amd.face_normals(tv, tf, validate=False)
    img, pm, cv, cf, cn, cleds, view = make_capture(torch, brdf_amd, dev)
    nf, L = int(f.shape[0]), int(leds.shape[0])
    words = brdf_amd.light_visibility(cv, cf, cleds, validate=False).face_lit  # (the capture's own random mesh: any words will do for the paint pass)
    work, apart = img.clone(), torch.empty_like(img)

    calls = dict(visibility=lambda: brdf_amd.light_visibility(tv, tf, leds, validate=False),
                 visibility_normals=lambda: brdf_amd.light_visibility(tv, tf, leds, normals=tn, validate=False),
                 paint_in_place=lambda: brdf_amd.apply_visibility(work, pm, words, level=0, out=work),
                 paint_apart=lambda: brdf_amd.apply_visibility(img, pm, words, level=0, out=apart),
                 copy=lambda: apart.copy_(img),
                 means=lambda: brdf_amd.fit_capture_means(1, img, pm, cv, cf, cn, cleds, view, rv_mode=1, p0=(0.5, 1.0, 1.0), opts=OPTS, validate=False,
                                                          v_min=1, v_max=254, cos_min=0.0))
    out = {k: fn() for k, fn in calls.items()}  # warm-up
    t = {k: [] for k in calls}
    for _ in range(args.reps):  # alternating
        for k, fn in calls.items():
            t[k].append(wall(torch, fn)[0])
    names = brdf_amd.shadow.STAT_NAMES
    ops = float(nf) * nf * (17.0 + 24.0 * L)
    result = dict(faces=nf, blocker_quads=args.blockers, lights=L, images=[L, H, W, 3], image_bytes=int(img.numel()), reps=args.reps,
                  timing="device-synchronised wall time of one call, median; the calls alternate in one process",
                  **{f"{k}_s": med(x) for k, x in t.items()}, **{f"{k}_s_min": min(x) for k, x in t.items()}, **{f"{k}_s_max": max(x) for k, x in t.items()},
                  stats=dict(zip(names, out["visibility"].stats.tolist())), stats_normals=dict(zip(names, out["visibility_normals"].stats.tolist())),
                  fp64_operations_upper_bound=ops, fp64_rate_upper_bound=ops / med(t["visibility"]),
                  fp64_rate_over_vector_peak=ops / med(t["visibility"]) / FP64_VECTOR_PEAK, fp64_vector_peak_assumed=FP64_VECTOR_PEAK,
                  visibility_over_means=med(t["visibility"]) / med(t["means"]), visibility_normals_over_visibility=med(t["visibility_normals"]) / med(t["visibility"]),
                  paint_in_place_over_copy=med(t["paint_in_place"]) / med(t["copy"]), paint_apart_over_copy=med(t["paint_apart"]) / med(t["copy"]),
                  painted_pixels=int(out["paint_apart"].shadowed.sum()),
                  not_measured="kernel times by rocprofv3 (these are wall times of whole calls); other mesh sizes and light counts; the split's and "
                               "the early stop's separate effects")
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
