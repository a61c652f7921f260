"""Rendering a fitted capture (brdf_hip_capture_render_dev, brdf_hip_capture_render_residuals_dev) on the GPU: what the two passes cost
next to a copy of the same image bytes, and how the capture layer's fits predict lights they were not fitted to.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py (scripts/gpu_capture_faces.py's make_capture), Blinn-Phong,
under the rule v_min = 1, v_max = 254, cos_min = 0.

  timings    six calls alternate on the same inputs in one process, all of them synchronising, so the device-synchronised wall time
             of a call is its cost; medians of --reps:
                 render      capture_render at 16 lights: value table and images, into a tensor it is given; also with the value table
                             alone (cosines of all faces, the table, the call's allocations and its wait) and the images alone
                 residuals   capture_render_residuals at 16 lights with all maps, into the tensors of an earlier result
                 copy        a device-to-device copy of the same 16 x 1024 x 1024 x 3 image bytes: the yardstick for the store stream
                             of `render` and the load stream of `residuals`
                 means       fit_capture_means on the same capture
             The ratios are reported; there is no threshold.
  held out   the fits see lights FITTED (12 of the rig's 16) and are evaluated -- capture_render_residuals' psnr() under the same rule --
             on those and on the other four: fit_capture_faces, fit_capture_means_clipped (rounds 3, kappa 2.5), fit_capture_single_faces
             and fit_capture_materials at K = 4 and K = 16 (seed_materials' seeds, rounds 5), the last three through
             surfaces_from_materials.
Not measured: Phong and Ward at this size, kernel times by rocprofv3 (wall times of whole calls only), other image sizes.
Writes profiles/capture_render.json (or --out).

    python scripts/gpu_capture_render.py [--out FILE] [--reps 5]
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

P0, LB, UB, ITMAX = (0.5, 1.0, 1.0), (0.0, 0.0, 0.0), (100.0, 100.0, 100.0), 100
RULE = dict(v_min=1, v_max=254, cos_min=0.0)
HELD = (2, 5, 11, 12)  # one light of each row of the rig, in four different columns
FITTED = tuple(i for i in range(16) if i not in HELD)
MODEL = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_render.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[4, 16])
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    img, pm, tv, tf, tn, leds, view = make_capture(torch, brdf_amd, dev)
    leds = np.ascontiguousarray(leds)
    mesh = (tv, tf, tn)
    kw = dict(rv_mode=1, lb=LB, ub=UB, itmax=ITMAX, opts=OPTS, validate=False, **RULE)
    med = statistics.median

    # ---- timings: all 16 lights, the per-face fit's surfaces ----
    full = (img, pm, *mesh, leds, view)
    faces16 = brdf_amd.fit_capture_faces(MODEL, *full, p0=P0, want_stats=False, **kw)
    rendered = torch.zeros_like(img)
    copy_to = torch.empty_like(img)

    def render():
        return brdf_amd.capture_render(MODEL, pm, *mesh, leds, view, faces16.surfaces, rv_mode=1, rendered=rendered, validate=False)

    res = brdf_amd.capture_render_residuals(MODEL, *full, faces16.surfaces, rv_mode=1, validate=False, **RULE)

    def residuals():
        return brdf_amd.capture_render_residuals(MODEL, *full, faces16.surfaces, rv_mode=1, validate=False, out=res, **RULE)

    def copy():
        return copy_to.copy_(img)

    def means():
        return brdf_amd.fit_capture_means(MODEL, *full, p0=P0, **kw)

    def values_only():
        return brdf_amd.capture_render(MODEL, pm, *mesh, leds, view, faces16.surfaces, rv_mode=1, want_images=False, validate=False)

    def images_only():
        return brdf_amd.capture_render(MODEL, pm, *mesh, leds, view, faces16.surfaces, rv_mode=1, want_values=False, rendered=rendered, validate=False)

    calls = dict(render=render, residuals=residuals, copy=copy, means=means, values_only=values_only, images_only=images_only)
    for fn in calls.values():  # warm-up
        fn()
    t = {k: [] for k in calls}
    for _ in range(args.reps):  # alternating
        for k, fn in calls.items():
            t[k].append(wall(torch, fn)[0])
    image_bytes = int(img.numel())
    timing = dict(image=[1024, 1024], lights=16, image_bytes=image_bytes, pixels=res.n_pixels, faces=int(tf.shape[0]), reps=args.reps,
                  timing="device-synchronised wall time of one call, median; the calls alternate in one process",
                  **{f"{k}_s": med(v) for k, v in t.items()}, **{f"{k}_s_min": min(v) for k, v in t.items()}, **{f"{k}_s_max": max(v) for k, v in t.items()},
                  render_over_copy=med(t["render"]) / med(t["copy"]), residuals_over_copy=med(t["residuals"]) / med(t["copy"]),
                  render_over_means=med(t["render"]) / med(t["means"]), residuals_over_means=med(t["residuals"]) / med(t["means"]),
                  render_gb_per_s=image_bytes / med(t["render"]) / 1e9, residuals_gb_per_s=image_bytes / med(t["residuals"]) / 1e9,
                  copy_gb_per_s_each_way=image_bytes / med(t["copy"]) / 1e9,
                  psnr_db_all_16_lights_fit_capture_faces=res.psnr()[1],
                  not_measured="Phong and Ward at this size; kernel times by rocprofv3 (these are wall times of whole calls: cosines, value table, "
                               "grouping and sort included); other image sizes")
    print(json.dumps(timing), flush=True)

    # ---- held-out lights ----
    fit_idx, held_idx = list(FITTED), list(HELD)
    part = (img[fit_idx].contiguous(), pm, *mesh, leds[fit_idx], view)
    held = (img[held_idx].contiguous(), pm, *mesh, leds[held_idx], view)

    def psnr(surfaces):
        on = brdf_amd.capture_render_residuals(MODEL, *part, surfaces, rv_mode=1, validate=False, **RULE)
        off = brdf_amd.capture_render_residuals(MODEL, *held, surfaces, rv_mode=1, validate=False, **RULE)
        return dict(fitted_lights_db=on.psnr()[1], held_out_lights_db=off.psnr()[1], compared_fitted=int(on.light_count.sum()),
                    compared_held_out=int(off.light_count.sum()), held_out_per_light_db=np.round(off.psnr()[0], 3).tolist(),
                    held_out_max_abs=int(off.abs_max.max()))

    zeros = torch.zeros(int(tf.shape[0]), dtype=torch.int32, device=dev)
    fits = {}
    face_fits = brdf_amd.fit_capture_faces(MODEL, *part, p0=P0, want_stats=False, **kw)
    fits["fit_capture_faces"] = psnr(face_fits.surfaces)
    clipped = brdf_amd.fit_capture_means_clipped(MODEL, *part, kappa=2.5, sigma_min=brdf_amd.SIGMA_MIN_8BIT, rounds=3, p0=P0, want_stats=False, **kw)
    fits["fit_capture_means_clipped"] = psnr(clipped.surfaces)
    single = brdf_amd.fit_capture_single_faces(MODEL, *part, p0=P0, want_stats=False, **kw)
    fits["fit_capture_single_faces"] = psnr(brdf_amd.surfaces_from_materials(zeros, single.single_brdf[None]))
    for K in args.K:
        seeds = brdf_amd.seed_materials(K, MODEL, *part, face_fits=face_fits, p0=P0, **kw)
        mats = brdf_amd.fit_capture_materials(MODEL, *part, seeds, rounds=5, want_stats=False, **kw)
        entry = psnr(brdf_amd.surfaces_from_materials(mats.labels, mats.materials, P0))
        entry.update(rounds_used=mats.rounds_used, settled=mats.settled, unassigned_carried_faces=int(((mats.labels < 0) & (mats.face_pixels > 0)).sum()))
        fits[f"fit_capture_materials_K{K}"] = entry
    held_out = dict(fitted_lights=fit_idx, held_out_lights=held_idx, rule="v_min 1, v_max 254, cos_min 0", model="Blinn-Phong",
                    psnr="10 log10(255^2 count / sum d^2) over the compared candidates of all lights and channels", fits=fits)
    print(json.dumps(held_out), flush=True)
    with open(args.out, "w") as fh:
        json.dump(dict(timings=timing, held_out=held_out), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
