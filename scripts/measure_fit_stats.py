"""Time of the statistics pass (brdf_hip_fit_stats_batch_dev) next to the fit it follows, on the GPU.

Inputs are generated on the device (brdf_hip_synth_dev) and fitted with brdf_hip_fit_batch_dev; the pass runs at the fitted
p.  Both are timed in this process after a warm-up, by HIP event pairs around one call each, median of LAUNCHES calls.
Writes profiles/fit_stats_pass.json (or --out): per workload the algorithmic bytes of the pass -- (24|32) n S read (two or
three planes and x) + 24 S read (p) + 140 S written (covar, stats, rank) --, its time, the achieved bytes/s and their share
of the 8 TB/s HBM peak, an estimate of its fp64 issue share, which of the two bounds it, and pass time / fit time; for the two pow
models also the A/B against the prepared-sample variant of the pass (BRDF_HIP_STATS_FAST=1).

    python scripts/measure_fit_stats.py [--out FILE] [--launches 20] [--only 0,1,2,3,4]
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

HBM_PEAK = 8.0e12        # bytes/s
FP64_LANE_RATE = 256 * 4 * 16 * 2.4e9  # fp64 VALU lane-instructions/s: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz
# VALU instructions per sample of the pass with a forward-difference row, counted in the gfx950 ISA of each geometry's kernel
# (static counts; [model] exact path, and the prepared-sample A/B variant for the two pow models):
#   rows   everything a lane executes up to the barrier -- one sample per lane, the fit's uniforms and the DPP trees included
#   wave   the same divided by the 4 samples a lane holds at n = 256
#   block  the body of the sample loop of fit_stats_block_kernel / fit_stats_partial_kernel
# Every VALU instruction is charged the fp64 rate (4 cycles per wavefront), so the share is an upper estimate of the issue time in use.
INSTR_PER_SAMPLE = {"rows": {0: 718, 1: 709, 2: 500}, "wave": {0: 535, 1: 527, 2: 261}, "block": {0: 407, 1: 407, 2: 128}}
INSTR_PER_SAMPLE_FAST = {"rows": {0: 487, 1: 478}, "wave": {0: 295, 1: 292}, "block": {0: 165, 1: 165}}


def geometry(n):
    return "rows" if n <= 16 else "wave" if n <= 256 else "block"


WORKLOADS = [
    dict(name="2^20 x 16 Blinn-Phong dlevmar_bc_dif", model=1, S=1 << 20, n=16),
    dict(name="BASELINE configs[4]: 2^20 x 256 Ward dlevmar_bc_dif", model=2, S=1 << 20, n=256),
    dict(name="BASELINE configs[3]: 65,536 x 4,096 Ward dlevmar_bc_dif", model=2, S=1 << 16, n=4096),
    dict(name="one 1,000,000-sample Ward fit, dlevmar_bc_dif", model=2, S=1, n=1_000_000),
    # not one of the four lines: the second size of the exact / prepared-sample A/B (Ward's two paths are the same operations)
    dict(name="A/B only: 2^18 x 256 Blinn-Phong dlevmar_bc_dif", model=1, S=1 << 18, n=256),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_stats_pass.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--only", default="0,1,2,3,4")
    args = ap.parse_args()
    import torch
    import brdf_amd
    from brdf_amd import synth
    from brdf_amd._lib import lib
    dev = torch.device("cuda:0")
    launches = max(20, args.launches)
    method = brdf_amd.METHOD_BC_DIF
    out = []
    for k in (int(v) for v in args.only.split(",")):
        w = WORKLOADS[k]
        model, S, n = w["model"], w["S"], w["n"]
        if S == 1:
            a_np, x_np, _ = synth.make_single(model, n)
            angles, x = torch.from_numpy(a_np[None]).to(dev), torch.from_numpy(x_np[None]).to(dev)
        else:
            truth = torch.from_numpy(np.ascontiguousarray(synth.surfel_truth(model, 0, S))).to(dev)
            angles = torch.empty((S, 3, n), dtype=torch.float64, device=dev)
            x = torch.empty((S, n), dtype=torch.float64, device=dev)
            rc = lib.brdf_hip_synth_dev(model, synth.SEED, 0, S, n, truth.data_ptr(), angles.data_ptr(), x.data_ptr(), None)
            assert rc == 0, brdf_amd.last_error()
        lb, ub = synth.bounds(model)
        p0 = torch.tensor(synth.P0[model], dtype=torch.float64, device=dev).repeat(S, 1)
        torch.cuda.synchronize()

        def fit():
            return brdf_amd.fit_batch(method, model, angles, x, p0.clone(), lb=lb, ub=ub, itmax=synth.ITMAX, opts=synth.OPTS)

        def timed(fn, reps):
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms), min(ms)

        p, info, ret = fit()  # warm-up of the fit; its p is the point of the pass
        torch.cuda.synchronize()
        p = p.clone()
        covar = torch.zeros((S, 3, 3), dtype=torch.float64, device=dev)
        stats = torch.zeros((S, 8), dtype=torch.float64, device=dev)
        rank = torch.zeros((S,), dtype=torch.int32, device=dev)
        opts = np.array(synth.OPTS)
        stream = torch.cuda.current_stream().cuda_stream

        def stats_pass():
            rc = lib.brdf_hip_fit_stats_batch_dev(method, model, angles.data_ptr(), x.data_ptr(), S, n, p.data_ptr(),
                                                  opts.ctypes.data_as(brdf_amd._lib.D), covar.data_ptr(), stats.data_ptr(), rank.data_ptr(), stream)
            assert rc == 0, brdf_amd.last_error()

        for _ in range(3):
            stats_pass()
        torch.cuda.synchronize()
        # the fit's input p0 is cloned inside the timed region (a 24 S byte copy: noise next to the fit)
        fit_ms, fit_min = timed(fit, launches if S * n < (1 << 27) else 20)
        pass_ms, pass_min = timed(stats_pass, launches)
        fast_ms = None
        if model != 2:  # the A/B: the same pass with exp(n log c) for pow(c, n) (BRDF_HIP_STATS_FAST=1; no fallback, not the default)
            os.environ["BRDF_HIP_STATS_FAST"] = "1"
            exact_stats = stats.clone()
            for _ in range(3):
                stats_pass()
            fast_ms, _ = timed(stats_pass, launches)
            torch.cuda.synchronize()
            ok = (rank == 3)
            sd_shift = float(((stats[ok, 2:5] - exact_stats[ok, 2:5]).abs() / exact_stats[ok, 2:5].abs()).max()) if bool(ok.any()) else None
            os.environ["BRDF_HIP_STATS_FAST"] = "0"
            stats_pass()  # the recorded outputs are the exact path's
            torch.cuda.synchronize()
        planes = 3 if model == 2 else 2
        nbytes = 8 * (planes + 1) * n * S + 24 * S + 140 * S
        bw = nbytes / (pass_ms * 1e-3)
        geo = geometry(n)
        fp64_share = INSTR_PER_SAMPLE[geo][model] * n * S / (pass_ms * 1e-3) / FP64_LANE_RATE
        hbm_share = bw / HBM_PEAK
        rk = rank.cpu().numpy()
        entry = dict(workload=w["name"], model=model, S=S, n=n, method="dlevmar_bc_dif", launches=launches, algorithmic_bytes=nbytes,
                     pass_ms=pass_ms, pass_ms_min=pass_min, fit_ms=fit_ms, fit_ms_min=fit_min, bytes_per_s=bw, hbm_peak_share=hbm_share,
                     fp64_issue_share_estimate=fp64_share, bound_by="HBM" if hbm_share >= fp64_share else "fp64 issue",
                     pass_over_fit=pass_ms / fit_ms, pass_faster_than_fit=bool(pass_ms < fit_ms), fits_failed=int((ret.cpu().numpy() < 0).sum()),
                     rank3=int((rk == 3).sum()), timing="HIP event pair around one call, median", geometry=geo,
                     valu_instr_per_sample=INSTR_PER_SAMPLE[geo][model])
        if fast_ms is not None:
            entry["ab_prepared_sample"] = dict(pass_ms=fast_ms, exact_over_prepared=pass_ms / fast_ms, valu_instr_per_sample=INSTR_PER_SAMPLE_FAST[geo][model],
                                               fp64_issue_share_estimate=INSTR_PER_SAMPLE_FAST[geo][model] * n * S / (fast_ms * 1e-3) / FP64_LANE_RATE,
                                               hbm_peak_share=nbytes / (fast_ms * 1e-3) / HBM_PEAK, max_relative_shift_of_sd_on_rank3_fits=sd_shift)
        print(json.dumps(entry), flush=True)
        out.append(entry)
        del angles, x, covar, stats, rank, p, p0
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    assert all(e["pass_faster_than_fit"] for e in out), "a statistics pass slower than the fit it follows is a bug"


if __name__ == "__main__":
    main()
