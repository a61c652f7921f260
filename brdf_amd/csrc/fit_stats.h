// fit_stats.h -- per-fit covariance, standard errors, correlations and R^2 at a fitted point: ONE evaluation pass over the
// samples of each fit, in kernels of its own (fit_stats.hip).  The fit kernels are not involved: the pass is a pure
// function of (angles, x, p, method, opts[4]) and does not care who fitted p.
#pragma once

#include "batch_fit.h"
#include "device_common.h"

namespace brdf {

constexpr int kStatsSz = 8;  // BRDF_STATS_SZ: sumsq, R2, sd[0..2], rho01, rho02, rho12

struct FitStatsArgs {
  int method, model;
  const double *d_angles, *d_x;  // [S][3][n], [S][n]
  int S, n;
  const double *d_p;   // [S][3]: the point the statistics are taken at
  const double *opts;  // host, 5 or null: only opts[4] (the difference step and its sign) is read
  double *d_covar;     // [rows][9] or null
  double *d_stats;     // [rows][kStatsSz] or null
  int *d_rank;         // [rows] or null
  // output row r reads fit d_src[r] (a negative entry leaves row r untouched); null: rows = S, row r reads fit r
  const int *d_src = nullptr;
  int rows = 0;
  hipStream_t stream = nullptr;
  // ragged batch (device, [S], or null): fit s has samples [0, d_counts[s]) of its rows, n is the row stride and the largest count.
  // Degrees of freedom d_counts[s] - 3; a count below 3 or outside [0, n]: rank 0, zero covar / sd / rho, sumsq and R2 over the samples
  // there are (both 0 for none).  n > 4096: synchronises the stream (the counts travel to the host; one uniform pass per fit).
  const int *d_counts = nullptr;
};

// argument check (no HIP call) and enqueue; `who` names the entry point in error texts.  Asynchronous on a.stream.
int fit_stats_check(const FitStatsArgs &a, const char *who);
int fit_stats_enqueue(const FitStatsArgs &a, const char *who);
// a fit above 4096 samples whose planes lie next to each other at `planes` (b.k apart): the uniform pass with S = 1, n = b.k at row b.row
// of a's p, straight into row b.row of a's covar / stats / rank; method, model, opts and stream are a's
int big_fit_stats_enqueue(const FitStatsArgs &a, const BigFit &b, const double *planes, const char *who);

}  // namespace brdf
