"""Packed batches (brdf_hip_fit_batch_packed_dev) next to the calls they are defined by, on the GPU.

Everything is timed in this process after a warm-up, by a HIP event pair around one call, median of LAUNCHES calls.  Writes
profiles/packed_batch.json (or --out):

  equal counts   2^20 x 16 and 2^18 x 256, Blinn-Phong dlevmar_bc_dif: the packed call (offsets = s * n) against the uniform call on
                 the same arrays, their ratio, and the difference of the two medians -- plan, gather and scatter together -- set
                 against the bytes the gather and the scatter move (samples read and written once more, p / info / ret twice): bytes/s
                 of that difference and its share of the 8 TB/s HBM peak.  The difference also holds the plan's three launches, the
                 readback and the workspace allocation, so this is a LOWER bound of the two kernels' own rate.
  a mixed batch  counts drawn from a fixed seeded mixture over the five classes plus a handful above 4096, three ways: the packed
                 call; the ragged call at stride = the largest count <= 4096 with the large fits as single-fit batches; hand-made
                 per-class ragged calls (the padded copies are built outside the timed region) with the same large fits.  Each run's
                 last_packed_stats() is recorded, and that all three return the same bytes.

    python scripts/measure_packed.py [--out FILE] [--launches 20] [--mixed-fits 16384]
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

HBM_PEAK = 8.0e12  # bytes/s, the figure DESIGN.md uses
BOUNDS = (16, 64, 256, 1024, 4096)
MIXTURE = (0.60, 0.20, 0.12, 0.05, 0.03)  # share of the fits per class 0..4
LARGE = (4097, 5000, 6000, 8192)          # the handful above 4096
SEED = 20240607


def timed(torch, fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def synth_batch(torch, brdf_amd, model, S, n, dev, first=0):
    from brdf_amd import synth
    from brdf_amd._lib import lib
    truth = torch.from_numpy(np.ascontiguousarray(synth.surfel_truth(model, first, S))).to(dev)
    angles = torch.empty((S, 3, n), dtype=torch.float64, device=dev)
    x = torch.empty((S, n), dtype=torch.float64, device=dev)
    rc = lib.brdf_hip_synth_dev(model, synth.SEED, first, S, n, truth.data_ptr(), angles.data_ptr(), x.data_ptr(), None)
    assert rc == 0, brdf_amd.last_error()
    return angles, x


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def equal_counts(torch, brdf_amd, dev, S, n, launches):
    from brdf_amd import synth
    model, method = brdf_amd.MODEL_BLINN_PHONG, brdf_amd.METHOD_BC_DIF
    angles, x = synth_batch(torch, brdf_amd, model, S, n, dev)
    lb, ub = synth.bounds(model)
    p0 = torch.tensor(synth.P0[model], dtype=torch.float64, device=dev).repeat(S, 1)
    offsets = torch.arange(S + 1, dtype=torch.int64, device=dev) * n
    fa, fx = angles.reshape(-1), x.reshape(-1)
    kw = dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)

    def uniform():
        return brdf_amd.fit_batch(method, model, angles, x, p0.clone(), **kw)

    def packed():
        return brdf_amd.fit_batch_packed(method, model, fa, fx, offsets, p0.clone(), validate=False, **kw)

    u, p = uniform(), packed()  # warm-up; the two calls must agree to the bit
    torch.cuda.synchronize()
    identical = all(same(a, b) for a, b in zip(u, p))
    plan = brdf_amd.last_packed_stats()
    uni_ms, uni_min, uni_max = timed(torch, uniform, launches)
    pk_ms, pk_min, pk_max = timed(torch, packed, launches)
    moved = 2 * 32 * n * S + 2 * (24 + 4) * S + 2 * (24 + 80 + 4) * S  # gather: samples, p, count read + written; scatter: p, info, ret
    extra_ms = pk_ms - uni_ms
    entry = dict(workload=f"{S} x {n} Blinn-Phong dlevmar_bc_dif", S=S, n=n, launches=launches, timing="HIP event pair around one call, median",
                 uniform_ms=uni_ms, uniform_ms_min=uni_min, uniform_ms_max=uni_max, packed_ms=pk_ms, packed_ms_min=pk_min, packed_ms_max=pk_max,
                 packed_over_uniform=pk_ms / uni_ms, bytes_identical=identical, plan=plan, gather_scatter_bytes=moved,
                 packed_minus_uniform_ms=extra_ms)
    if extra_ms > 0:
        entry["gather_scatter_bytes_per_s_lower_bound"] = moved / (extra_ms * 1e-3)
        entry["hbm_peak_share_lower_bound"] = moved / (extra_ms * 1e-3) / HBM_PEAK
    return entry


def mixed(torch, brdf_amd, dev, S, launches):
    from brdf_amd import synth
    model, method = brdf_amd.MODEL_BLINN_PHONG, brdf_amd.METHOD_BC_DIF
    rng = np.random.default_rng(SEED)
    cls = rng.choice(5, size=S, p=MIXTURE)
    lo = np.array([3, 17, 65, 257, 1025])[cls]
    counts_np = rng.integers(lo, np.array(BOUNDS)[cls] + 1).astype(np.int32)
    stride = int(counts_np.max())
    lb, ub = synth.bounds(model)
    kw = dict(lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)
    angles, x = synth_batch(torch, brdf_amd, model, S, stride, dev)
    counts = torch.from_numpy(counts_np).to(dev)
    big = [synth_batch(torch, brdf_amd, model, 1, k, dev, first=S + i) for i, k in enumerate(LARGE)]
    pa, px, po = brdf_amd.pack_samples(angles, x, counts)
    # the packed batch: the S small fits, then the large ones
    pa = torch.cat([pa] + [a.reshape(-1) for a, _ in big])
    px = torch.cat([px] + [v.reshape(-1) for _, v in big])
    po = torch.cat([po, po[-1] + torch.cumsum(torch.tensor(LARGE, dtype=torch.int64, device=dev), 0)])
    total = S + len(LARGE)
    p0 = torch.tensor(synth.P0[model], dtype=torch.float64, device=dev).repeat(total, 1)

    def packed():
        return brdf_amd.fit_batch_packed(method, model, pa, px, po, p0.clone(), validate=False, **kw)

    def large_fits():
        return [brdf_amd.fit_batch(method, model, a, v, p0[:1].clone(), **kw) for a, v in big]

    def ragged():
        return brdf_amd.fit_batch(method, model, angles, x, p0[:S].clone(), counts=counts, **kw), large_fits()

    by_class = []
    for c in range(5):
        idx = torch.nonzero(torch.from_numpy(cls == c).to(dev)).reshape(-1)
        if idx.numel():
            n_c = int(counts[idx].max())
            by_class.append((idx, angles[idx][:, :, :n_c].contiguous(), x[idx][:, :n_c].contiguous(), counts[idx].contiguous()))

    def per_class():
        return [brdf_amd.fit_batch(method, model, a, v, p0[:idx.numel()].clone(), counts=k, **kw) for idx, a, v, k in by_class], large_fits()

    out_p, out_r, out_c = packed(), ragged(), per_class()  # warm-up
    torch.cuda.synchronize()
    plan = brdf_amd.last_packed_stats()
    # the hand-made per-class calls are what the packed call is defined by: same bytes, fit by fit
    identical = True
    for (idx, _, _, _), res in zip(by_class, out_c[0]):
        identical &= all(same(full[idx], part) for full, part in zip(out_p, res))
    for i, res in enumerate(out_c[1]):
        identical &= all(same(full[S + i:S + i + 1], part) for full, part in zip(out_p, res))
    reps = max(5, launches // 4)  # (the stride-4096 ragged call runs every fit in an eight-wave workgroup: seconds per call)
    pk = timed(torch, packed, launches)
    rg = timed(torch, ragged, reps)
    pc = timed(torch, per_class, launches)
    hist = {f"class {c}": int((cls == c).sum()) for c in range(5)}
    hist["class 5"] = len(LARGE)
    return dict(workload=f"mixed batch: {S} fits over five classes + {len(LARGE)} above 4096, Blinn-Phong dlevmar_bc_dif", seed=SEED, mixture=MIXTURE,
                fits_per_class=hist, samples=int(po[-1]), padded_samples_of_the_ragged_call=S * stride, ragged_stride=stride,
                timing="HIP event pair around one call, median", launches=dict(packed=launches, ragged=reps, per_class=launches),
                packed_ms=pk[0], packed_ms_min=pk[1], packed_ms_max=pk[2], ragged_one_stride_ms=rg[0], ragged_one_stride_ms_min=rg[1],
                ragged_one_stride_ms_max=rg[2], per_class_by_hand_ms=pc[0], per_class_by_hand_ms_min=pc[1], per_class_by_hand_ms_max=pc[2],
                per_class_copies_timed=False, packed_bytes_identical_to_per_class_calls=bool(identical), plan=plan,
                fits_failed=int((out_p[2] < 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_batch.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--mixed-fits", type=int, default=1 << 14)
    args = ap.parse_args()
    import torch
    import brdf_amd
    dev = torch.device("cuda:0")
    out = []
    for S, n in ((1 << 20, 16), (1 << 18, 256)):
        out.append(equal_counts(torch, brdf_amd, dev, S, n, args.launches))
        print(json.dumps(out[-1]), flush=True)
        torch.cuda.empty_cache()
    out.append(mixed(torch, brdf_amd, dev, args.mixed_fits, args.launches))
    print(json.dumps(out[-1]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
