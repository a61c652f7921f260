// fit_stats_weighted.inc -- the statistics pass of the weighted problem (weighted_fit.h), n <= 16: included by fit_stats.hip behind the
// unweighted kernels, whose text, argument block and instances stay what they were.
//
// One 16-lane DPP row per fit, fit_stats_ragged_rows_kernel's geometry and reduction trees.  Per sample, with sw = sqrt(w): the model
// value and the Jacobian row as the fit's method forms them, both times sw (the weighted fit's own roundings); e = sw x - sw f.
//   per fit   sum e^2 = sum w e^2, the six sums of J^T W J, sum w x, sum w;  then, with mean = sum w x / sum w, sum w (x - mean)^2
//   finish    finish_fit: covar = sumsq / (nobs - 3) * inverse(J^T W J), sigma, rho, R^2 = 1 - sumsq / SStot
// extra[q] (optional) is added to sumsq and to SStot first: a sum of squares that does not depend on p, such as the spread of the
// observations inside the groups whose means are being fitted.  nobs[q] (optional) replaces the fit's count in the degrees of freedom.
// With unit weights and neither array every added operation is exact and sum w is the count: the ragged pass's bytes.
struct WeightedStatsCtx {
  const double *angles, *x, *w, *p, *extra;
  const int *counts, *nobs;
  double *covar, *stats;
  int *rank;
  long long rows;
  int n;
  double delta;
};

__device__ __forceinline__ int weighted_stats_count(const WeightedStatsCtx &c, long long q) {
  if (!c.counts) return c.n;
  const int k = c.counts[q];
  return (k < 0 || k > c.n) ? 0 : k;
}

template <int MODEL, int JAC, bool FAST>
__global__ __launch_bounds__(kRowsThreads) void fit_stats_weighted_rows_kernel(WeightedStatsCtx c) {
  using Mdl = BrdfModel<MODEL>;
  constexpr int kNW = kNS + 1;  // [e^2, J^T W J lower (6), w x, w]
  __shared__ double sh[kRowsFits][kRow];
  const int slot = threadIdx.x >> 4, i = threadIdx.x & 15, lane = threadIdx.x & (kWave - 1);
  const long long r0 = (long long)blockIdx.x * kRowsFits + slot;
  const long long q = r0 < c.rows ? r0 : -1;
  const int nq = q >= 0 ? weighted_stats_count(c, q) : 0;
  const bool ok = q >= 0 && i < nq;
  double acc[kNW], xv = 0.0, wv = 0.0;
#pragma unroll
  for (int k = 0; k < kNW; ++k) acc[k] = 0.0;
  if (ok) {
    JacUniforms u;
    build_uniforms<MODEL, JAC>(c.p + 3 * q, c.delta, u);
    const double *a = c.angles + (size_t)q * 3 * c.n;
    const double c0 = a[i];
    const double c1 = Mdl::uses_c1 ? a[(size_t)c.n + i] : 1.0;
    const double c2 = Mdl::uses_c2 ? a[2 * (size_t)c.n + i] : 1.0;
    xv = c.x[(size_t)q * c.n + i];
    wv = c.w[(size_t)q * c.n + i];
    const double sw = sqrt(wv);
    const Prep pq = Mdl::template prepare<FAST>(c0, c1, c2);
    double f0, j[kM];
    if (JAC == JAC_ANALYTIC)
      model_an_row<MODEL, FAST>(u, c0, pq, f0, j);
    else
      model_fd_row_t<MODEL, FAST, JAC == JAC_CENTRAL>(u, c0, pq, true, f0, 0.0, false, j);
    f0 = sw * f0;
#pragma unroll
    for (int k = 0; k < kM; ++k) j[k] = sw * j[k];
    const double e = sw * xv - f0;
    acc[0] += e * e;
    acc[1] += j[0] * j[0];
    acc[2] += j[0] * j[1];
    acc[3] += j[1] * j[1];
    acc[4] += j[0] * j[2];
    acc[5] += j[1] * j[2];
    acc[6] += j[2] * j[2];
    acc[7] += wv * xv;
    acc[8] += wv;
  }
#pragma unroll
  for (int k = 0; k < kNW; ++k) acc[k] = row_reduce_to_last<OpSum>(acc[k]);  // lanes beyond the count add +0.0
  const double mean = __shfl(acc[kNS - 1], lane | 15) / __shfl(acc[kNS], lane | 15);
  const double dx = ok ? xv - mean : 0.0;
  const double st = row_reduce_to_last<OpSum>(wv * (dx * dx));
  if (i == 15) {
    double extra = 0.0;
    if (c.extra && q >= 0) extra = c.extra[q];
#pragma unroll
    for (int k = 0; k < kNS; ++k) sh[slot][k] = acc[k];
    sh[slot][kNS] = st;
    if (c.extra) {
      sh[slot][0] = acc[0] + extra;
      sh[slot][kNS] = st + extra;
    }
  }
  __syncthreads();
  if (threadIdx.x < kRowsFits) {
    const long long r = (long long)blockIdx.x * kRowsFits + threadIdx.x;
    if (r < c.rows) {
      StatsCtx fc;  // what finish_fit reads: the point and the three outputs
      fc.p = c.p;
      fc.covar = c.covar;
      fc.stats = c.stats;
      fc.rank = c.rank;
      // the degrees of freedom are nobs - 3 where the fit has its three samples; below that the count itself says rank 0
      const int cnt = weighted_stats_count(c, r);
      const int nobs = (c.nobs && cnt >= kM) ? c.nobs[r] : cnt;
      finish_fit<true>(fc, r, r, sh[threadIdx.x], nobs);
    }
  }
}
