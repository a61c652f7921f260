// clip_fit.h -- sigma-clipped packed batches (clip_fit.hip): fit, drop the samples further than kappa sigma from the fit, fit the
// survivors again, until nothing more is dropped.  No fit or statistics kernel of its own: the fits are packed_fit_run's and the
// statistics packed_stats_run's, unchanged; the unit adds the clip pass between them -- the exact-path residual of every sample
// against its fit's threshold and the stream compaction of the survivors into a new packed batch.
//
// The definition (include/brdf_levmar.h says the same, and brdf_amd.clip_samples is one round of it as NumPy code):
//   round 0   every fit from d_p on all of its samples: packed_fit_run's bytes
//   settled   a fit that is refused (k < 3) or ends with ret < 0 keeps those outputs and all of its samples
//   round r = 1 ... rounds, for every fit that is not settled, with its k current samples at its current p:
//             sumsq = stats[0] of packed_stats_run on the current sample set at p; not finite: settled, nothing clipped
//             sigma = fmax(sqrt(sumsq / (k - 3)), sigma_min) for k > 3, sigma_min for k == 3
//             sample i survives iff fabs(x_i - f_i(p)) <= kappa * sigma (f on the exact path; a NaN residual fails)
//             nothing dropped: settled.  Fewer than 3 survivors: the clip is NOT applied, settled.
//             otherwise the survivors, in their order, are the fit's sample set from now on (a dropped sample never returns), the
//             fit runs again from its current p -- packed_fit_run's bytes on the survivors from that p -- and rounds_used = r
//             the loop ends early when every fit is settled
//   statistics  packed_stats_run's bytes at the returned p over the returned sample set
#pragma once

#include "packed_fit.h"

namespace brdf {

constexpr int kClipMaxRounds = 16;

struct ClipSpec {
  double kappa, sigma_min;
  int rounds;
};
// what the clipped entries refuse of the three arguments, before any HIP call: a kappa that is not > 0 (+inf is allowed), a sigma_min
// that is negative or not a number, rounds outside [0, kClipMaxRounds]
int clip_spec_check(const ClipSpec &c, const char *who);

struct ClipFitArgs {
  PackedFitArgs fit;  // the packed call's arguments: d_p in/out, d_info and d_ret may be null
  ClipSpec clip;
  double *d_covar, *d_stats;  // [S][9], [S][kStatsSz] or null
  int *d_rank;                // [S] or null
  int *d_kept;                // [S] or null: the samples of the fit's returned set
  int *d_rounds_used;         // [S] or null
  unsigned char *d_mask;      // [offsets[S] - offsets[0]] or null: 1 = in the returned set, by the caller's sample position
};
int clip_fit_check(const ClipFitArgs &a, const char *who);  // no HIP call
// Waits for the stream as the packed calls do -- once per fit and per statistics call -- once for the batch's extent (where a clip round
// or the mask needs it) and once per clip round, to learn whether any fit is still active.
int clip_fit_run(const ClipFitArgs &a, const char *who);

// the calling thread's last clipped call: the clip rounds it ran and, per round, the fits that were refitted and the samples dropped
struct ClipLastStats {
  int rounds;
  long long active[kClipMaxRounds], clipped[kClipMaxRounds];
};
ClipLastStats clip_last_stats();
void clip_last_stats_set(const ClipLastStats &s);  // (capture_means_clip.hip records its rounds here)

// rows (carried face, channel) of two [nf][3] int maps <- rows channel * F + face rank of the batch (either map may be null); enqueues.
// d_kept null: the fits' counts by d_offsets; d_rounds null: 0 -- what a call with rounds = 0 returns, without its two arrays
int clip_scatter_maps(const char *who, const int *d_face_list, int F, const int *d_kept, const int *d_rounds, const long long *d_offsets,
                      int *d_surface_kept, int *d_surface_rounds, hipStream_t stream);

}  // namespace brdf
