// capture_means_clip.h -- what capture_means.hip and capture_means_clip.hip share: the means capture's device state and the clip
// rounds' host interface.
//
// Sigma clipping for per-light means (include/brdf_levmar.h says the same, and brdf_amd.clip_light_means is one round of it as NumPy
// code).  All pixels of a face share the face's cosines, so whether a sample survives a round depends on (fit, light, grey level v)
// alone: the survivors under one light are an interval of grey levels, "a dropped sample never returns" is an intersection of
// intervals, and the whole clip state is two bytes per (fit, light).
//   intervals  [lo_l, hi_l] per (fit, light): [v_min, v_max] clamped to 0 ... 255 where the light's cosines pass the rule, empty
//              (lo = 1, hi = 0) where they fail.  The fit's current sample set: the valid candidates with lo_l <= v <= hi_l.
//   round 0    brdf_hip_fit_capture_means_dev's fit, with its bytes
//   settled    a fit that is refused (fewer than 3 lights with a sample) or ends with ret < 0 keeps its outputs and its samples
//   round r = 1 ... rounds, for every fit that is not settled, at its current p:
//              sumsq = stats[0] of the weighted statistics pass on the current rows with extra_ss = within and nobs = k (the
//              full-sample sum of squares); not finite: settled, nothing clipped
//              sigma = fmax(sqrt(sumsq / (k - 3)), sigma_min) for k > 3, sigma_min for k == 3
//              grey level v under light l survives iff fabs(v / 255.0 - f_l(p)) <= kappa * sigma (f on the exact path; a NaN fails)
//              the new interval of a light: from the smallest to the largest surviving v inside the old one; empty if none survives
//              no sample dropped: settled.  Fewer than 3 lights keep a sample: the clip is NOT applied, the intervals stay, settled.
//              otherwise the intervals are adopted, count, sum v, sum v^2, means, weights, within, k and lights are formed again from
//              the survivors, the fit runs again from its current p -- the weighted fit's bytes on those rows from that p -- and
//              rounds_used = r.  The loop ends early when every fit is settled.
//   statistics the weighted statistics pass's bytes at the returned p over the returned rows, with their within and k
#pragma once

#include "capture_group.h"

namespace brdf {

// the means capture's device state (capture_means.hip allocates and fills it; its kernels take a type of their own derived from this
// one, so they keep their names)
struct MeansState {
  CandidateCtx cand;
  // accumulators, word (channel * F + rank) * L + light
  int *cnt;
  unsigned long long *s1, *s2;
  // the weighted batch: rows of stride L
  double *angles, *x, *w, *within, *p;
  int *lights, *nobs;
  double p0[kM];
};

// The clip rounds of brdf_hip_fit_capture_means_clipped_dev, between round 0's fit and the scatter of capture_means.hip.
struct MeansClipArgs {
  const char *who;
  MeansState ctx;        // after round 0: the sums, the rows and p of every fit (all of them are written again by a round that clips)
  const CaptureArgs *cap;
  int fits;             // 3 F
  double kappa, sigma_min;
  int rounds;
  double *d_info;       // [fits][10] or null
  int *d_ret;           // [fits], required with rounds > 0
  double *d_covar, *d_stats;  // [fits][9], [fits][kStatsSz] or null: written by every round's statistics call and by the last one
  int *d_rank;                // [fits] or null
  int *d_rounds_used;         // [fits], zeroed by the caller
  unsigned char *d_vlo, *d_vhi;  // [fits][L], by the capture's light index: the initial intervals on entry (means_clip_intervals)
};
// the initial intervals of every fit: enqueues
int means_clip_intervals(const char *who, const CandidateCtx &cand, unsigned char *d_vlo, unsigned char *d_vhi, hipStream_t stream);
// Runs the rounds; waits for the stream once per round, to learn whether any fit is still active.  *stats_fresh: the statistics maps
// hold the statistics at the returned p over the returned rows (false: a round refitted after the last statistics call, or no round
// ran).  Records the rounds where brdf_hip_last_clip_stats finds them.
int means_clip_run(const MeansClipArgs &a, bool *stats_fresh);
// rows (carried face, channel) of the two [nf][3][L] interval maps <- rows channel * F + face rank (either map may be null); enqueues
int means_clip_scatter(const char *who, const int *d_face_list, int F, int L, const unsigned char *d_vlo, const unsigned char *d_vhi,
                       unsigned char *d_surface_vlo, unsigned char *d_surface_vhi, hipStream_t stream);

}  // namespace brdf
