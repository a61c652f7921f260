// capture_faces.hip -- brdf_hip_fit_capture_faces_dev: ONE fit per (face, channel) over the samples of ALL the face's pixels, where
// the capture loop of capture_fit.hip fits every pixel and keeps the face's last one.  No fit or statistics kernel of its own: the
// capture becomes a packed batch (packed_fit.h) on the device, the packed calls fit it, a scatter fills the [nf][3] maps.
//
// (compact, group, cosines and scatter are capture_group.hip's, shared with capture_means.hip and capture_single_faces.hip)
//   pack      the candidates of a channel are ONE flat array, t = sorted pixel * L + light, and a channel's measurements are one
//             stream compaction of it (ballot + popcount, block counts, scan: count / place once more).  A fit's offset is the
//             prefix at its face's first candidate, so no wave belongs to a face and a face of 10^5 pixels costs what 10^5 faces of
//             one pixel cost.  Fit s = channel * F + face rank: the offsets ascend with s.  A third pass over the same candidates
//             writes the plane triples, which need the fits' counts.
//   fit       packed_fit_run (dlevmar_bc_dif), packed_stats_run where a statistics map is asked for; in the clipped entry
//             (brdf_hip_fit_capture_faces_clipped_dev: CaptureFacesArgs::clip) clip_fit_run in their place, and two more maps
//
// The three candidate passes evaluate the same rule on the same bytes, so the places of pass 2 and 3 are the counts of pass 1.
#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "clip_fit.h"
#include "fit_stats.h"
#include "packed_fit.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_faces_dev", *kWhoClipped = "brdf_hip_fit_capture_faces_clipped_dev";

// ---- count and pack ------------------------------------------------------------------------------------------------------------
struct PackCtx {
  CandidateCtx cand;
  int *block_count;             // [blocks][3]                                                    (pass 0 writes)
  const long long *block_off;   // [blocks][3]: the place of the block's first valid candidate    (block_scan3_kernel<true>)
  long long *offsets;           // [3 F + 1]                                                      (pass 1 writes, pass 2 reads)
  double *angles, *x, *p;       // the packed batch
  double p0[kM];
};

// Candidate t = (sorted pixel, light) of all three channels (capture_compact.h: read_candidate).
//   PASS 0  the block's number of valid candidates per channel
//   PASS 1  measurements to their places; at a face's first candidate the fit's offset (the prefix there) and its starting point
//   PASS 2  the plane triples, three planes of the fit's count each
template <int PASS>
__global__ __launch_bounds__(kCT) void pack_kernel(PackCtx c) {
  __shared__ int wave_cnt[kWaves][3];
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const Candidate k = read_candidate(c.cand, t);
  ChannelPlaces pl = {wave_cnt};
  pl.place(k.valid);
  if (PASS == 0) {
    if (threadIdx.x < 3) c.block_count[(size_t)blockIdx.x * 3 + threadIdx.x] = pl.count(threadIdx.x);
    return;
  }
  if (t >= c.cand.T) return;
  const bool first_of_face = k.i == 0 && k.s == c.cand.face_first[k.r];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long long at = pl.at(ch, c.block_off[(size_t)blockIdx.x * 3 + ch]);
    const size_t fit = (size_t)ch * c.cand.F + k.r;
    if (PASS == 1) {
      if (k.valid[ch]) c.x[at] = k.v[ch] / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
      if (first_of_face) {
        c.offsets[fit] = at;
        for (int j = 0; j < kM; ++j) c.p[fit * kM + j] = c.p0[j];
      }
    } else if (k.valid[ch]) {
      const long long o = c.offsets[fit], n = c.offsets[fit + 1] - o;
      double *dst = c.angles + 3 * o + (at - o);
      dst[0] = k.c0;
      dst[n] = k.c1;
      dst[2 * n] = k.c2;
    }
  }
}

}  // namespace

int capture_faces_run(const CaptureFacesArgs &a) {
  const char *who = a.clip ? kWhoClipped : kWho;
  if (a.workspace_bytes < 0) {  // what the entry refuses before any HIP call
    set_error("%s(): workspace_bytes = %lld: need workspace_bytes >= 0", who, a.workspace_bytes);
    return kLmError;
  }
  if (capture_args_check(who, a.g, a.d_brdf_surfaces, "brdf_surfaces") != 0) return kLmError;
  if (a.clip && clip_spec_check(ClipSpec{a.clip->kappa, a.clip->sigma_min, a.clip->rounds}, who) != 0) return kLmError;
  (void)hipGetLastError();
  const CaptureArgs &cap = a.g.cap;
  hipStream_t stream = cap.stream;
  if (a.avg) a.avg[0] = a.avg[1] = a.avg[2] = 0.0;
  if (a.g.n_pixels) *a.g.n_pixels = 0;
  if (a.g.n_faces) *a.g.n_faces = 0;

  // ---- compact, group, cosines (capture_group.hip) ----
  CaptureGroup g;
  if (capture_group_run(who, a.g, g) != 0) return kLmError;
  if (g.S == 0) return 0;  // an empty capture: nothing is written but the pixel counts

  // ---- count and pack ----
  PackCtx pc = {};
  pc.cand = capture_candidates(a.g, g);
  const long long T = pc.cand.T;  // candidates of one channel
  const int pb = (int)((T + kCT - 1) / kCT), fits = (int)(3 * g.F);
  DevBuf pack_count, pack_off, offsets, p, ends;
  DevBuf clip_maps;  // the clip rounds' kept and rounds_used, rows channel * F + face rank (rounds = 0: the counts and 0, no array)
  if (!take(pack_count, sizeof(int) * 3 * (size_t)pb, "the candidate blocks' counts", who) ||
      !take(pack_off, sizeof(long long) * 3 * (size_t)pb, "the candidate blocks' offsets", who) ||
      !take(offsets, sizeof(long long) * ((size_t)fits + 1), "the fits' offsets", who) ||
      !take(p, sizeof(double) * kM * (size_t)fits, "the fits' parameters", who) || !take(ends, sizeof(long long) * 3, "the channels' ends", who) ||
      (a.clip && a.clip->rounds > 0 && !take(clip_maps, sizeof(int) * 2 * (size_t)fits, "the fits' kept counts and rounds", who)))
    return kLmError;
  pc.block_count = pack_count.as<int>();
  pc.block_off = pack_off.as<long long>();
  pc.offsets = offsets.as<long long>();
  pc.p = p.as<double>();
  for (int k = 0; k < kM; ++k) pc.p0[k] = cap.p0[k];
  hipLaunchKernelGGL(pack_kernel<0>, dim3(pb), dim3(kCT), 0, stream, pc);
  // channel after channel: the last channel's end is offsets[3 F], the valid candidates of all three channels
  hipLaunchKernelGGL(block_scan3_kernel<true>, dim3(1), dim3(kCT), 0, stream, pack_count.as<int>(), (long long)pb, pack_off.as<long long>(),
                     offsets.as<long long>() + fits, 0LL, ends.as<long long>());
  CAPTURE_OK(who, hipGetLastError());
  long long end[3] = {0, 0, 0};
  CAPTURE_OK(who, hipMemcpyAsync(end, ends.ptr, sizeof end, hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  const long long total = end[2];
  if (total < 0 || total > 3 * T) {
    set_error("%s(): the count finds %lld valid samples among %lld candidates", who, total, 3 * T);
    return kLmError;
  }
  DevBuf angles, x;  // 32 bytes per valid sample
  if (!take(angles, sizeof(double) * 3 * (size_t)total, "the packed planes", who) || !take(x, sizeof(double) * (size_t)total, "the packed measurements", who))
    return kLmError;
  pc.angles = angles.as<double>();
  pc.x = x.as<double>();
  hipLaunchKernelGGL(pack_kernel<1>, dim3(pb), dim3(kCT), 0, stream, pc);
  hipLaunchKernelGGL(pack_kernel<2>, dim3(pb), dim3(kCT), 0, stream, pc);
  CAPTURE_OK(who, hipGetLastError());

  // ---- fit ----
  const bool want_stats = a.d_surface_covar || a.d_surface_stats || a.d_surface_rank;
  FitResultBufs res;
  if (!take_fit_results(res, a, fits, who)) return kLmError;
  const PackedFitArgs pf = {BRDF_METHOD_BC_DIF, cap.model, angles.as<double>(), x.as<double>(), offsets.as<long long>(), fits, p.as<double>(), cap.lb, cap.ub,
                            cap.itmax, cap.opts, res.info.as<double>(), res.ret.as<int>(), a.workspace_bytes, stream};
  if (a.clip) {
    const ClipFitArgs cf = {pf, {a.clip->kappa, a.clip->sigma_min, a.clip->rounds}, res.covar.as<double>(), res.stats.as<double>(), res.rank.as<int>(),
                            clip_maps.as<int>(), clip_maps.ptr ? clip_maps.as<int>() + fits : nullptr, nullptr};
    if (clip_fit_run(cf, who) != 0) return kLmError;
    if (clip_scatter_maps(who, g.face_list.as<int>(), (int)g.F, cf.d_kept, cf.d_rounds_used, offsets.as<long long>(), a.clip->d_surface_kept, a.clip->d_surface_rounds, stream) != 0)
      return kLmError;
  } else if (packed_fit_run(pf, who) != 0) {
    return kLmError;
  }
  if (want_stats && !a.clip) {
    const PackedStatsArgs ps = {BRDF_METHOD_BC_DIF, cap.model, pf.d_angles, pf.d_x, pf.d_offsets, fits, pf.d_p, cap.opts, res.covar.as<double>(),
                                res.stats.as<double>(), res.rank.as<int>(), a.workspace_bytes, stream};
    if (packed_stats_run(ps, who) != 0) return kLmError;
  }

  // ---- scatter (capture_group.hip) ----
  const ScatterArgs sc = {&a, &g, p.as<double>(), &res, offsets.as<long long>(), nullptr, nullptr, nullptr};
  return capture_scatter_run(who, sc);
}

}  // namespace brdf
