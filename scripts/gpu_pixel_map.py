"""Pixel maps and face normals on the GPU (brdf_hip_pixel_map_dev, brdf_hip_face_normals_dev): what the calls cost next to a copy of
the map's bytes and next to a capture fit of the same image size, and how much of the candidate walk is wasted.

The mesh is a jittered 200 x 100 grid of quads (40,000 triangles) that fills a 1024 x 1024 viewport through a perspective camera
(gl_look_at from (0, 0, 3), gl_frustum); `backdrop` is the same mesh with two triangles behind it that cover the whole viewport -- the
load-balance case: two faces with 2 x 1024 x 1024 candidates next to 40,000 faces with a few dozen each.

  timings    the calls alternate on the same inputs in one process, all of them synchronising, so the device-synchronised wall time
             of a call is its cost; medians of --reps:
                 map          pixel_map, mode 1, the map and face_pixels
                 map_depth    the same with the depth map
                 backdrop     mode 1 on the mesh with the backdrop
                 centroids    mode 0 on the mesh
                 normals      face_normals on the mesh
                 copy         a device-to-device copy of the map's 4 MiB: the yardstick for the stores
                 means        fit_capture_means on the synthetic 1024 x 1024 capture of scripts/gpu_capture_faces.py
             The ratios are reported; there is no threshold.
  candidates candidates visited per owned pixel, for the mesh and for the mesh with the backdrop (stats[5] / stats[6]).
Not measured: kernel times by rocprofv3 (these are wall times of whole calls: allocation, memsets, five launches and the wait), other
viewport and mesh sizes, meshes with long thin triangles (whose boxes are mostly empty).
Writes profiles/pixel_map.json (or --out).

    python scripts/gpu_pixel_map.py [--out FILE] [--reps 5]
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

H = W = 1024


def make_mesh(nx=200, ny=100, seed=4):
    """(vertices, faces, vertices and faces with the backdrop in front of the list): a jittered grid over [-1.02, 1.02]^2 near z = 0"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(-1.02, 1.02, nx + 1), np.linspace(-1.02, 1.02, ny + 1))
    v = np.stack([gx, gy, np.zeros_like(gx)], axis=2).reshape(-1, 3)
    v += rng.uniform(-1.0, 1.0, size=v.shape) * [0.3 * 2.04 / nx, 0.3 * 2.04 / ny, 0.05]
    at = lambda i, j: j * (nx + 1) + i
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    i, j = i.reshape(-1), j.reshape(-1)
    f = np.concatenate([np.stack([at(i, j), at(i + 1, j), at(i + 1, j + 1)], axis=1), np.stack([at(i, j), at(i + 1, j + 1), at(i, j + 1)], axis=1)]).astype(np.int32)
    back = np.array([[-4.0, -4.0, -1.0], [4.0, -4.0, -1.0], [4.0, 4.0, -1.0], [-4.0, 4.0, -1.0]])
    vb = np.concatenate([back, v])
    fb = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), f + 4]).astype(np.int32)
    return v, f, vb, fb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_map.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    med = statistics.median
    v, f, vb, fb = make_mesh()
    tv, tf, tvb, tfb = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (v, f, vb, fb))
    mv = brdf_amd.gl_look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    pr = brdf_amd.gl_frustum(-1.0 / 3, 1.0 / 3, -1.0 / 3, 1.0 / 3, 1.0, 10.0)
    cam = (mv, pr, (0.0, 0.0, float(W), float(H)), H, W)
    img, pm, cv, cf, cn, leds, view = make_capture(torch, brdf_amd, dev)
    copy_from = brdf_amd.pixel_map(tv, tf, *cam, validate=False).pixel_map
    copy_to = torch.empty_like(copy_from)

    calls = dict(map=lambda: brdf_amd.pixel_map(tv, tf, *cam, validate=False),
                 map_depth=lambda: brdf_amd.pixel_map(tv, tf, *cam, want_depth=True, validate=False),
                 backdrop=lambda: brdf_amd.pixel_map(tvb, tfb, *cam, validate=False),
                 centroids=lambda: brdf_amd.pixel_map(tv, tf, *cam, mode=0, validate=False),
                 normals=lambda: brdf_amd.face_normals(tv, tf, validate=False),
                 copy=lambda: copy_to.copy_(copy_from),
                 means=lambda: brdf_amd.fit_capture_means(1, img, pm, cv, cf, cn, leds, view, rv_mode=1, p0=(0.5, 1.0, 1.0), opts=OPTS, validate=False,
                                                          v_min=1, v_max=254, cos_min=0.0))
    out = {k: fn() for k, fn in calls.items()}  # warm-up
    t = {k: [] for k in calls}
    for _ in range(args.reps):  # alternating
        for k, fn in calls.items():
            t[k].append(wall(torch, fn)[0])
    # the twin on the same inputs: the bytes, once
    twin = brdf_amd.pixel_map_host(vb, fb, *cam)
    same = bool(np.array_equal(out["backdrop"].pixel_map.cpu().numpy(), twin.pixel_map) and out["backdrop"].stats.tolist() == twin.stats.tolist())
    names = brdf_amd.raster.STAT_NAMES
    result = dict(viewport=[H, W], faces=int(f.shape[0]), map_bytes=4 * H * W, reps=args.reps,
                  timing="device-synchronised wall time of one call, median; the calls alternate in one process",
                  **{f"{k}_s": med(x) for k, x in t.items()}, **{f"{k}_s_min": min(x) for k, x in t.items()}, **{f"{k}_s_max": max(x) for k, x in t.items()},
                  map_over_copy=med(t["map"]) / med(t["copy"]), backdrop_over_map=med(t["backdrop"]) / med(t["map"]),
                  map_over_means=med(t["map"]) / med(t["means"]), centroids_over_copy=med(t["centroids"]) / med(t["copy"]),
                  normals_over_copy=med(t["normals"]) / med(t["copy"]),
                  stats_mesh=dict(zip(names, out["map"].stats.tolist())), stats_backdrop=dict(zip(names, out["backdrop"].stats.tolist())),
                  stats_centroids=dict(zip(names, out["centroids"].stats.tolist())),
                  candidates_per_owned_pixel_mesh=out["map"].stats[5] / out["map"].stats[6],
                  candidates_per_owned_pixel_backdrop=out["backdrop"].stats[5] / out["backdrop"].stats[6],
                  candidates_per_second_backdrop=out["backdrop"].stats[5] / med(t["backdrop"]),
                  backdrop_bytes_equal_twin=same,
                  not_measured="kernel times by rocprofv3 (these are wall times of whole calls: allocation, memsets, five launches, the wait); "
                               "other viewport and mesh sizes; long thin triangles")
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
