// packed_fit.h -- packed batches: S fits of any size laid back to back (CSR offsets), bucketed by size class inside the library
// (packed_fit.hip).  No fit or statistics kernel of its own: a plan (classify, stable partition by class), per class a segmented
// gather into padded rows, the existing ragged launches (batch_fit_enqueue / fit_stats_enqueue with per-fit counts) and a scatter;
// fits above 4096 samples run where they lie through the single-fit path.
#pragma once

#include "device_common.h"
#include "packed_plan.h"

namespace brdf {

struct PackedFitArgs {
  int method, model;             // BRDF_METHOD_* of include/brdf_levmar.h
  const double *d_angles, *d_x;  // fit s: planes [3][k_s] at d_angles + 3 offsets[s], measurements at d_x + offsets[s]
  const long long *d_offsets;    // device, [S + 1], non-decreasing; k_s = offsets[s + 1] - offsets[s]
  int S;
  double *d_p;  // [S][3] in/out
  const double *lb, *ub;
  int itmax;
  const double *opts;
  double *d_info;  // [S][10] or null
  int *d_ret;      // [S] or null
  long long workspace_bytes;  // bound of the padded rows of one chunk; 0: kPackedDefaultWorkspace
  hipStream_t stream;
};
// Argument check (no HIP call), then the plan and the launches.  Waits for the stream ONCE, to read the plan back (and again around the
// fits above 4096 samples, which are synchronous as in the uniform call).
int packed_fit_check(const PackedFitArgs &a, const char *who);
int packed_fit_run(const PackedFitArgs &a, const char *who);

struct PackedStatsArgs {
  int method, model;
  const double *d_angles, *d_x;
  const long long *d_offsets;
  int S;
  const double *d_p;  // [S][3], read only
  const double *opts;
  double *d_covar;  // [S][9] or null
  double *d_stats;  // [S][kStatsSz] or null
  int *d_rank;      // [S] or null
  long long workspace_bytes;
  hipStream_t stream;
};
int packed_stats_check(const PackedStatsArgs &a, const char *who);
int packed_stats_run(const PackedStatsArgs &a, const char *who);

// the calling thread's last packed call, per class: fits, the row stride its launches used (0 for an empty class; class 5: the largest
// count) and the number of chunks (class 5: one run per fit)
struct PackedLastStats {
  long long fits[kPackedClasses];
  int stride[kPackedClasses];
  int chunks[kPackedClasses];
};
PackedLastStats packed_last_stats();

}  // namespace brdf
