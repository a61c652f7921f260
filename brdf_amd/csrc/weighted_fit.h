// weighted_fit.h -- per-sample weights in ONE size class, the application's own: n <= 16 samples per fit (kLaneMaxN), dlevmar_bc_dif /
// dlevmar_bc_der.  Fit s is levmar on the weighted problem hx_i = sqrt(w_i) f_i(p), x'_i = sqrt(w_i) x_i over the first counts[s]
// samples of its rows -- what a levmar caller does today by scaling inside the callback.  The fit is the lane-per-fit kernel with one
// more LDS plane (weighted_fit.hip); the statistics are a 16-lane-row pass of their own (fit_stats.hip,
// fit_stats_weighted.inc); capture_means.hip spends both on the per-face capture.  No existing kernel or argument block is involved.
#pragma once

#include "batch_fit.h"
#include "fit_stats.h"
#include "stream_fit.h"

namespace brdf {

struct WeightedFitArgs {
  BatchFitArgs fit;   // the ragged batch call's arguments (fit.d_counts may be null: every fit has n samples)
  const double *d_w;  // [S][n], the layout of fit.d_x
};
// argument check (no HIP call) and enqueue; `who` names the entry point in error texts.  Asynchronous on a.fit.stream.
int weighted_fit_check(const WeightedFitArgs &a, const char *who);
int weighted_fit_enqueue(const WeightedFitArgs &a, const char *who);

// the weighted lane kernels' argument block (a type of its own: the unweighted kernels keep theirs)
struct WeightedBatchCtx : RaggedBatchCtx {
  const double *w;  // [S][n]
};

// Statistics of the weighted problem at p: sumsq = sum w e^2 (+ extra_ss), J^T W J, mean = sum w x / sum w, SStot = sum w (x - mean)^2
// (+ extra_ss), covar = sumsq / (nobs - 3) * inverse(J^T W J); sd, rho, R2 from these as in the unweighted pass.
struct WeightedStatsArgs {
  FitStatsArgs stats;        // the ragged statistics call's arguments (d_src / rows unused; d_counts may be null)
  const double *d_w;         // [S][n]
  const double *d_extra_ss;  // [S] or null: a sum of squares that does not depend on p, added to sumsq and to SStot
  const int *d_nobs;         // [S] or null: the observation count of the degrees of freedom (null: the fit's count)
};
int weighted_stats_check(const WeightedStatsArgs &a, const char *who);
int weighted_stats_enqueue(const WeightedStatsArgs &a, const char *who);

}  // namespace brdf
