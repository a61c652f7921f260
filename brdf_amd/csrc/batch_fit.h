// batch_fit.h -- "batched" regime: S independent fits, one workgroup (or one wavefront) per fit, the
// whole LM loop inside the kernel.  Replaces the serial pixel x channel loop of
// CBRDFdata::CalcBRDFEquation (brdfdata.cpp:1195-1220), each iteration of which is one
// dlevmar_bc_dif call (brdfdata.cpp:1119).
#pragma once

#include <type_traits>

#include "device_common.h"

namespace brdf {

struct BatchFitArgs {
  int method, model;  // method: BRDF_METHOD_* of include/brdf_levmar.h (0 dif, 1 bc_dif, 2 bc_der, 3 der)
  const double *d_angles, *d_x;
  int S, n;
  double *d_p;
  const double *lb, *ub;
  int itmax;
  const double *opts;
  double *d_info;
  int *d_ret;
  hipStream_t stream;
  // ragged batch (device, [S], or null): fit s uses samples [0, d_counts[s]) of its rows; n stays the row stride
  const int *d_counts = nullptr;
};
// argument check (no HIP call) and enqueue; `who` names the entry point in error texts.  Asynchronous on a.stream up to 4096 samples per fit.
int batch_fit_check(const BatchFitArgs &a, const char *who);
int batch_fit_enqueue(const BatchFitArgs &a, const char *who);

// A fit above 4096 samples no longer fits a workgroup: the batched entries run such fits one after the other through the single-fit
// path, each spread over the chip.
struct BigFit {
  const double *d_angles, *d_x;  // three planes `stride` apart, the measurements
  int k, stride;                 // the fit's own sample count; k == stride: the planes already lie as a single fit reads them
  long long row;                 // the fit's row of the caller's arrays
};
// fits[0, count) from host p[rows][3] into host p, info[rows][10] and ret[rows]; method, model, box, itmax, opts and stream are a's.  A
// count below 3 or above the stride is levmar's n < m refusal (lm_core.c:502, lmbc_core.c:440) without a launch: ret -1, info and p as
// they are.  The caller waits for a.stream before the host arrays go away.
int big_fits_run(const BatchFitArgs &a, const BigFit *fits, int count, double *p, double *info, int *ret);

constexpr int kNeedsExact = -2;  // flag value: this fit has a cosine <= 0 and must take the exact model path

struct BatchCtx {
  const double *angles;  // [S][3][n]
  const double *x;       // [S][n]
  double *p;             // [S][3] in/out
  double *info;          // [S][10] or null
  int *ret;              // [S] or null
  int *flags;            // [S] internal: kNeedsExact marks fits handed to the exact kernel
  int S, n, itmax;
  int has_opts, has_lb, has_ub;
  int multi;  // bc_dif: projected-gradient candidates per sweep (workgroup/wave-per-fit kernels)
  int lane_quorum, lane_maxwait;  // lane_fit.hip: lanes waiting for / rounds between two heavy rounds
  int analytic;  // RQ_JAC rows from the model's analytic Jacobian (dlevmar_bc_der / dlevmar_der) instead of finite differences
  int chain;     // dlevmar_dif: trial points per sweep in a chain of rejections (eight-wave kernel; 1 = one at a time)
  int spec_jac;  // dlevmar_bc_dif: candidates evaluated by Jacobian passes (off in the batched kernels: they are bound by arithmetic)
  int dif_fused; // dlevmar_dif, eight-wave kernel: the step behind a trial pass tries DifMachine::fused_trial_step first
  double opts[5], lb[kM], ub[kM];
};

// what the RAGGED kernel instances take instead: n is the row stride there, counts[S] the fits' own sample counts.  (A type of its
// own: the uniform kernels' argument block, and with it their code, stays what it was.)
struct RaggedBatchCtx : BatchCtx {
  const int *counts;
};
template <bool RAGGED>
using BatchCtxOf = typename std::conditional<RAGGED, RaggedBatchCtx, BatchCtx>::type;
inline RaggedBatchCtx ragged_ctx(const BatchCtx &c, const int *counts) {
  RaggedBatchCtx r;
  static_cast<BatchCtx &>(r) = c;
  r.counts = counts;
  return r;
}

// a ragged fit's own sample count: the fit's entry of counts[], or 0 -- levmar's n < m refusal -- where the entry is outside [0, stride]
__device__ __forceinline__ int ragged_count(const int *counts, long long fit, int stride) {
  const int k = counts[fit];
  return (k < 0 || k > stride) ? 0 : k;
}

// 1024 < n <= 4096 samples per fit: one workgroup per fit, control wave + seven sample waves (resident_fit.hip).
// fast = false: only the fits whose flag is kNeedsExact are fitted (exact model path)
// counts (device, [S], or null): per-fit sample counts -- the RAGGED instances
int resident_batch_enqueue(int model, int method, bool fast, const BatchCtx &c, const int *counts, hipStream_t stream);


// n <= kLaneMaxN, dlevmar_bc_dif: one lane per fit (lane_fit.hip).  queue: two zeroed ints
constexpr int kLaneMaxN = 16;
int lane_fit_enqueue(int model, bool fast, const BatchCtx &c, const int *counts, int *queue, hipStream_t stream);

int synth_enqueue(int model, unsigned long long seed, long long first, int count, int n, const double *d_truth,
                  double *d_angles, double *d_x, hipStream_t stream);

}  // namespace brdf
