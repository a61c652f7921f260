"""The per-face capture (brdf_hip_fit_capture_faces_dev) next to the last-pixel-wins capture, on the GPU.

The capture is the synthetic 1024 x 1024 one of tests/measure_capture.py (seed 2: 16 images, 40 000 faces, ~70 % of the pixels on the
mesh, ~18 pixels per face).  fit_capture_faces, with the rule off and with v_min = 1, v_max = 254, cos_min = 0, is timed against
fit_capture_masked on the same inputs with the same rule, the two calls alternating; both calls synchronise, so the device-synchronised
wall time of a call is its cost.  The two compute different things (F x 3 grouped fits against pixels x 3 sixteen-sample fits of which
F x 3 are kept): there is no pass/fail threshold.

The group / pack work is reported apart from the fit: a call on the same capture with itmax = 0 and without statistics runs the
compaction, the sort, the cosines, the three candidate passes, the packed plan and a fit launch that stops at once; its time is an
UPPER bound of the grouping and packing.  Writes profiles/capture_faces.json (or --out).

    python scripts/gpu_capture_faces.py [--out FILE] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = (1e-3, 1e-15, 1e-15, 1e-20, 1e-6)


def make_capture(torch, brdf_amd, dev):
    """tests/measure_capture.py's capture, statement for statement"""
    from brdf_amd import synth
    rng = np.random.default_rng(2)
    H = W = 1024
    nv, nf = 20000, 40000
    vertices = rng.uniform(-80, 80, size=(nv, 3)) + np.array([0.0, -80.0, 60.0])
    faces = np.stack([rng.integers(0, nv, size=nf), rng.integers(0, nv, size=nf), rng.integers(0, nv, size=nf)], axis=1).astype(np.int32)
    e1 = vertices[faces[:, 1]] - vertices[faces[:, 0]]
    e2 = vertices[faces[:, 2]] - vertices[faces[:, 0]]
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    leds = brdf_amd.led_table()
    view = np.array([310.0, -75.0, 700.0])
    c = vertices[faces].sum(axis=1) / 3.0
    nrm[((leds.mean(axis=0)[None, :] - c) * nrm).sum(axis=1) < 0] *= -1.0
    pixel_map = rng.integers(0, nf, size=(H, W)).astype(np.int32)
    pixel_map[rng.random((H, W)) < 0.3] = -1
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (vertices, faces, nrm))
    ang = torch.abs(brdf_amd.cosines(tv, tf, tn, leds, view, rv_mode=1))
    pm = torch.from_numpy(pixel_map).to(dev)
    a_px = ang[pm.clamp(min=0).long()]
    kd, ks, n = synth.TRUTH[1]
    val = kd * a_px[:, :, 0, :] + ks * torch.pow(a_px[:, :, 1, :], n)
    img = torch.zeros((16, H, W, 3), dtype=torch.uint8, device=dev)
    for ch in range(3):
        q = torch.clamp(torch.round(val * (0.6 + 0.2 * ch) * 127.0), 0, 255).to(torch.uint8)
        img[:, :, :, ch] = torch.flip(q.permute(2, 0, 1), dims=[1])
    return img, pm, tv, tf, tn, leds, view


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_faces.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    img, pm, tv, tf, tn, leds, view = make_capture(torch, brdf_amd, dev)
    mesh = (img, pm, tv, tf, tn, leds, view)
    out = []
    for name, rule in (("rule off", dict()), ("v_min 1, v_max 254, cos_min 0", dict(v_min=1, v_max=254, cos_min=0.0))):
        def faces(**kw):
            return brdf_amd.fit_capture_faces(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule, **kw)

        def masked():
            return brdf_amd.fit_capture_masked(1, *mesh, rv_mode=1, opts=OPTS, validate=False, **rule)

        def pack_only():
            return brdf_amd.fit_capture_faces(1, *mesh, rv_mode=1, opts=OPTS, validate=False, itmax=0, want_stats=False, **rule)

        r, _, _ = faces(), masked(), pack_only()  # warm-up
        classes = brdf_amd.last_packed_stats()
        t_faces, t_masked, t_pack = [], [], []
        for _ in range(args.reps):  # alternating
            t_faces.append(wall(torch, faces)[0])
            t_masked.append(wall(torch, masked)[0])
            t_pack.append(wall(torch, pack_only)[0])
        count = r.count.cpu().numpy()
        carried = r.face_pixels.cpu().numpy() > 0
        entry = dict(rule=name, image=[1024, 1024], lights=16, pixels=r.n_pixels, faces=r.n_faces, grouped_fits=3 * r.n_faces,
                     per_pixel_fits_of_the_masked_capture=3 * r.n_pixels, samples=int(count[carried].sum()),
                     fits_refused=int((r.ret.cpu().numpy()[carried] < 0).sum()), size_classes_of_the_statistics_call=classes,
                     timing="device-synchronised wall time of one call, median; the calls alternate", reps=args.reps,
                     faces_s=statistics.median(t_faces), faces_s_min=min(t_faces), faces_s_max=max(t_faces),
                     masked_s=statistics.median(t_masked), masked_s_min=min(t_masked), masked_s_max=max(t_masked),
                     group_and_pack_s_upper_bound=statistics.median(t_pack), group_and_pack_s_min=min(t_pack), group_and_pack_s_max=max(t_pack),
                     faces_over_masked=statistics.median(t_faces) / statistics.median(t_masked),
                     group_and_pack_share_of_faces=statistics.median(t_pack) / statistics.median(t_faces), avg=[float(v) for v in r.avg])
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
