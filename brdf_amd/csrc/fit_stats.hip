// fit_stats.hip -- covariance, standard errors, correlations and R^2 of S fits at their fitted points.
//
// What levmar hands back with a single fit -- covar = sumsq/(n-3) * (J^T J)^-1 (misc_core.c:564-591) and, through its
// utilities, sigma_i, rho_ij (:598-611) and R^2 (:616-658) -- for the batched and capture entry points, which return p and
// info only.  The statistics are NOT taken from the fit kernels (their register budgets and result bits stay as they are):
// they come from one evaluation pass at the fitted p,
//
//   per sample   f(p) and the Jacobian row as the fit's method forms it: a forward / central difference row with levmar's
//                steps (fd_steps, quotient as a multiplication by 1/d: model_fd_row_t) or the analytic row (model_an_row),
//                on the EXACT model path (the reference's own pow expression);  e = x - f
//   per fit      sum e^2, the six sums of J^T J, sum x;  then, with the mean known, sum (x - mean)^2   (two phases, as
//                dlevmar_R2 is two loops)
//   finish       one lane per fit: unpack_lower, lu_covar<3> (the fitter's own Crout LU), sigma, rho, R^2
//
// Every sum is a fixed tree (device_common.h) or a fixed serial fold: no float atomics, so two runs give the same bits and
// a fit's result depends on (n, its own data) only -- never on S or on its position in the batch.
//
// Geometry by fit size, the batched fitter's own split:
//   n <= 16      fit_stats_rows_kernel     one 16-lane DPP row per fit (a fit's samples are contiguous: 512 B for Ward)
//   n <= 256     fit_stats_wave_kernel     one wavefront per fit, up to 4 samples per lane
//   n <= 4096    fit_stats_block_kernel    one 256-thread workgroup per fit
//   n  > 4096    fit_stats_partial_kernel  several workgroups per fit publish a partial row each (8 sums);
//                fit_stats_spread_kernel   every workgroup folds the sum-x column by one fixed tree (same bits in all of
//                                          them), sweeps its chunk of x for sum (x - mean)^2 and adds it to its row;
//                fit_stats_fold_kernel     one workgroup per fit folds the rows, a fixed tree per column, and finishes.
//                The launch chain's partial-row scheme: kernel boundaries order the phases, nothing spins.
// In the first three the per-fit sums are parked in LDS and the first lanes of the workgroup finish one fit each, so the
// serial 3 x 3 LU runs in a few dense wavefronts instead of one lane of every wavefront.
#include <cstdio>
#include <vector>

#include "../../include/brdf_levmar.h"
#include "fit_stats.h"
#include "fit_host.h"
#include "packed_plan.h"
#include "weighted_fit.h"

namespace brdf {

namespace {

constexpr int kNS = 8;         // reduced in the first phase: [e^2, J^T J lower (6), x]
constexpr int kRow = kNS + 1;  // + sum (x - mean)^2
constexpr int kRowsThreads = 512, kRowsFits = kRowsThreads / 16;
constexpr int kWaveThreads = 256, kWaveFits = kWaveThreads / kWave, kWaveMaxN = 256, kWavePer = kWaveMaxN / kWave;
constexpr int kBlockThreads = 256, kBlockMaxN = 4096;
// (a packed batch's size classes, packed_plan.h, step wherever these kernels change: rows | wave | workgroup | chunked)
static_assert(packed_class(16) + 1 == packed_class(17) && packed_class(kWaveMaxN) + 1 == packed_class(kWaveMaxN + 1) &&
                  packed_class(kBlockMaxN) + 1 == packed_class(kBlockMaxN + 1) && packed_class(kBlockMaxN + 1) == kPackedLargeClass,
              "packed_plan.h: the statistics kernels' bounds are size-class bounds");
constexpr int kMaxPartials = kBlockThreads;  // workgroups per fit at most (n > 4096): the folds hold one partial row per thread

constexpr int kMaxSamples = 0x7fffffff - 2 * kMaxPartials * kBlockThreads;  // largest n: no index of a sweep overflows

enum JacKind : int { JAC_FORWARD = 0, JAC_CENTRAL = 1, JAC_ANALYTIC = 2 };

struct StatsCtx {
  const double *angles, *x, *p;
  const int *src;
  double *covar, *stats;
  int *rank;
  double *partials;  // [rows][nb][kRow]   (n > 4096)
  long long rows;
  int n, chunk, nb;
  double delta;  // |opts[4]|, or LM_DIFF_DELTA
  const int *counts;  // [S] or null: per-fit sample counts (RAGGED kernel instances; n is the row stride there)
};

// a ragged fit's own sample count: 0 where the entry is outside [0, stride] (nothing of the row is read then)
__device__ __forceinline__ int stats_count(const StatsCtx &c, long long q) {
  const int k = c.counts[q];
  return (k < 0 || k > c.n) ? 0 : k;
}

__device__ __forceinline__ long long fit_of_row(const StatsCtx &c, long long r) {
  if (r >= c.rows) return -1;
  return c.src ? (long long)c.src[r] : r;
}

// the uniforms of one fit's pass: PassUniforms::build's arithmetic for an RQ_JAC request at p
template <int MODEL, int JAC>
__device__ __forceinline__ void build_uniforms(const double *pg, double delta, JacUniforms &u) {
  using Mdl = BrdfModel<MODEL>;
  const double p[kM] = {pg[0], pg[1], pg[2]};
  u.l0 = Mdl::lin(p);
  u.n0 = Mdl::nl(p);
  u.central = JAC == JAC_CENTRAL;
  u.analytic = JAC == JAC_ANALYTIC;
  if (JAC == JAC_ANALYTIC) {
    Mdl::an_scalars(p, u.an);
    return;
  }
  double d[kM];
  fd_steps<kM>(p, delta, d);
#pragma unroll
  for (int j = 0; j < kM; ++j) {
    double pp[kM] = {p[0], p[1], p[2]};
    pp[j] = p[j] + d[j];  // misc_core.c:161 / :202
    u.lp[j] = Mdl::lin(pp);
    if (j == kM - 1) u.np2 = Mdl::nl(pp);
    if (JAC == JAC_CENTRAL) {
      double pm[kM] = {p[0], p[1], p[2]};
      pm[j] = p[j] - d[j];  // misc_core.c:199
      u.lm[j] = Mdl::lin(pm);
      if (j == kM - 1) u.nm2 = Mdl::nl(pm);
    }
    u.dinv[j] = (JAC == JAC_CENTRAL ? 0.5 : 1.0) / d[j];
  }
}

// sample i of a fit whose planes start at `a` (plane stride n): its terms added to acc[kNS]; returns x_i
template <int MODEL, int JAC, bool FAST>
__device__ __forceinline__ double sample_acc(const JacUniforms &u, const double *a, const double *x, int n, int i, double *acc) {
  using Mdl = BrdfModel<MODEL>;
  const double c0 = a[i];
  const double c1 = Mdl::uses_c1 ? a[(size_t)n + i] : 1.0;
  const double c2 = Mdl::uses_c2 ? a[2 * (size_t)n + i] : 1.0;
  const double xv = x[i];
  const Prep q = Mdl::template prepare<FAST>(c0, c1, c2);
  double f0, j[kM];
  if (JAC == JAC_ANALYTIC)
    model_an_row<MODEL, FAST>(u, c0, q, f0, j);
  else
    model_fd_row_t<MODEL, FAST, JAC == JAC_CENTRAL>(u, c0, q, true, f0, 0.0, false, j);
  const double e = xv - f0;
  acc[0] += e * e;
  acc[1] += j[0] * j[0];
  acc[2] += j[0] * j[1];
  acc[3] += j[1] * j[1];
  acc[4] += j[0] * j[2];
  acc[5] += j[1] * j[2];
  acc[6] += j[2] * j[2];
  acc[7] += xv;
  return xv;
}

// one lane per fit: row = [sum e^2, J^T J lower (6), sum x, sum (x - mean)^2] -> the fit's outputs
// RAGGED: n is the fit's own count -- below kM there are no degrees of freedom (rank 0), and of no samples both sumsq and R2 are 0
template <bool RAGGED = false>
__device__ __forceinline__ void finish_fit(const StatsCtx &c, long long r, long long q, const double *row, int n) {
  double jtj[kM * kM], cv[kM * kM], sd[kM], rho[kM];
  const double sumsq = row[0], sstot = row[kNS];
  unpack_lower<kM>(row + 1, jtj);
#pragma unroll
  for (int k = 0; k < kM * kM; ++k) cv[k] = 0.0;
  int rank = lu_covar<kM>(jtj, cv, sumsq, n);
#pragma unroll
  for (int i = 0; i < kM; ++i) sd[i] = sqrt(cv[i * kM + i]);  // misc_core.c:600
  rho[0] = cv[0 * kM + 1] / sqrt(cv[0 * kM + 0] * cv[1 * kM + 1]);  // misc_core.c:610
  rho[1] = cv[0 * kM + 2] / sqrt(cv[0 * kM + 0] * cv[2 * kM + 2]);
  rho[2] = cv[1 * kM + 2] / sqrt(cv[1 * kM + 1] * cv[2 * kM + 2]);
  bool finite = true;
#pragma unroll
  for (int k = 0; k < kRow; ++k) finite = finite && lm_finite(row[k]);
#pragma unroll
  for (int k = 0; k < kM; ++k) finite = finite && lm_finite(c.p[3 * q + k]) && lm_finite(sd[k]) && lm_finite(rho[k]);
#pragma unroll
  for (int k = 0; k < kM * kM; ++k) finite = finite && lm_finite(cv[k]);
  if (!finite) rank = 0;
  if (RAGGED && n < kM) rank = 0;
  if (rank == 0) {  // what a single fit's covar shows when levmar could not invert J^T J
#pragma unroll
    for (int k = 0; k < kM * kM; ++k) cv[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kM; ++k) sd[k] = rho[k] = 0.0;
  }
  if (c.covar) {
#pragma unroll
    for (int k = 0; k < kM * kM; ++k) c.covar[r * (kM * kM) + k] = cv[k];
  }
  if (c.stats) {
    double *o = c.stats + r * kStatsSz;
    o[0] = sumsq;
    o[1] = (RAGGED && n <= 0) ? 0.0 : 1.0 - sumsq / sstot;  // misc_core.c:657 (the IEEE result when SStot = 0)
    o[2] = sd[0];
    o[3] = sd[1];
    o[4] = sd[2];
    o[5] = rho[0];
    o[6] = rho[1];
    o[7] = rho[2];
  }
  if (c.rank) c.rank[r] = rank;
}


// ---- helpers of the wavefront / workgroup kernels ------------------------------------------------------------------------
__device__ __forceinline__ double wave_last(double v) {  // lane 63's value, in scalar registers
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), kWave - 1);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), kWave - 1);
  return __hiloint2double(hi, lo);
}


// ---- a workgroup's share [first, last) of one fit: the eight sums into out[0..kNS) (LDS, visible to all on return) ---
template <int MODEL, int JAC, bool FAST>
__device__ __forceinline__ void block_sums(const StatsCtx &c, long long q, int first, int last, double *buf, double *out) {
  JacUniforms u;
  build_uniforms<MODEL, JAC>(c.p + 3 * q, c.delta, u);
  u = scalar_copy(u);
  const double *a = c.angles + (size_t)q * 3 * c.n, *x = c.x + (size_t)q * c.n;
  double acc[kNS];
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = 0.0;
  for (int i = first + (int)threadIdx.x; i < last; i += kBlockThreads) (void)sample_acc<MODEL, JAC, FAST>(u, a, x, c.n, i, acc);
  block_reduce<kNS, kBlockThreads>(acc, 0.0, buf, out);
}

// ... and sum (x - mean)^2 over the same share into out[0]
__device__ __forceinline__ void block_spread(const StatsCtx &c, long long q, int first, int last, double mean, double *buf, double *out) {
  const double *x = c.x + (size_t)q * c.n;
  double st[1] = {0.0};
  for (int i = first + (int)threadIdx.x; i < last; i += kBlockThreads) {
    const double dx = x[i] - mean;
    st[0] += dx * dx;
  }
  block_reduce<1, kBlockThreads>(st, 0.0, buf, out);
}


// ---- n <= 16 / 256 / 4096: a 16-lane row / a wavefront / a workgroup per fit; uniform, and with per-fit sample counts -------------
#define FIT_STATS_KERNEL(kind) fit_stats_##kind##_kernel
#define FIT_STATS_RAGGED false
#include "fit_stats_kernels.inc"
#undef FIT_STATS_KERNEL
#undef FIT_STATS_RAGGED
#define FIT_STATS_KERNEL(kind) fit_stats_ragged_##kind##_kernel
#define FIT_STATS_RAGGED true
#include "fit_stats_kernels.inc"
#undef FIT_STATS_KERNEL
#undef FIT_STATS_RAGGED

// ---- n > 4096: several workgroups per fit, partial rows, a folding kernel --------------------------------------
template <int MODEL, int JAC, bool FAST>
__global__ __launch_bounds__(kBlockThreads) void fit_stats_partial_kernel(StatsCtx c) {
  __shared__ double buf[reduce_buf_doubles<kBlockThreads>()];
  __shared__ double out[kSlots];
  const long long r = blockIdx.x / c.nb, q = fit_of_row(c, r);
  const int b = (int)(blockIdx.x - r * c.nb);
  if (q < 0) return;
  const long long first = (long long)b * c.chunk, last = first + c.chunk;
  block_sums<MODEL, JAC, FAST>(c, q, (int)first, (int)(last < c.n ? last : c.n), buf, out);
  if (threadIdx.x < kNS) c.partials[((size_t)r * c.nb + b) * kRow + threadIdx.x] = out[threadIdx.x];
}

__global__ __launch_bounds__(kBlockThreads) void fit_stats_spread_kernel(StatsCtx c) {
  __shared__ double buf[reduce_buf_doubles<kBlockThreads>()];
  __shared__ double out[kSlots];
  const long long r = blockIdx.x / c.nb, q = fit_of_row(c, r);
  const int b = (int)(blockIdx.x - r * c.nb);
  if (q < 0) return;
  const double *rows = c.partials + (size_t)r * c.nb * kRow;
  // the sum-x column, one row per thread (nb <= kBlockThreads), folded by the same tree in every workgroup: the same mean everywhere
  double sx[1] = {(int)threadIdx.x < c.nb ? rows[(size_t)threadIdx.x * kRow + kNS - 1] : 0.0};
  block_reduce<1, kBlockThreads>(sx, 0.0, buf, out);
  const double mean = out[0] / (double)c.n;
  const long long first = (long long)b * c.chunk, last = first + c.chunk;
  block_spread(c, q, (int)first, (int)(last < c.n ? last : c.n), mean, buf, out);
  if (threadIdx.x == 0) c.partials[((size_t)r * c.nb + b) * kRow + kNS] = out[0];
}

// one workgroup per fit: thread b holds partial row b, one fixed tree per column, thread 0 finishes
__global__ __launch_bounds__(kBlockThreads) void fit_stats_fold_kernel(StatsCtx c) {
  __shared__ double buf[reduce_buf_doubles<kBlockThreads>()];
  __shared__ double out[kSlots];
  const long long r = blockIdx.x, q = fit_of_row(c, r);
  if (q < 0) return;
  const double *rows = c.partials + (size_t)r * c.nb * kRow;
  double v[kRow];
#pragma unroll
  for (int k = 0; k < kRow; ++k) v[k] = (int)threadIdx.x < c.nb ? rows[(size_t)threadIdx.x * kRow + k] : 0.0;
  block_reduce<kRow, kBlockThreads>(v, 0.0, buf, out);
  if (threadIdx.x == 0) {
    double row[kRow];
#pragma unroll
    for (int k = 0; k < kRow; ++k) row[k] = out[k];
    finish_fit(c, r, q, row, c.n);
  }
}

// ---- the weighted problem, n <= 16 (weighted_fit.h): a kernel, an argument block and a table of their own -------------------
#include "fit_stats_weighted.inc"

typedef void (*StatsKernel)(StatsCtx);
// fast: the prepared-sample variant (exp(n log c) for pow(c, n)), an A/B switch only -- see stats_fast_path().  Ward's two paths
// perform the same operations (brdf_models.h), so its `fast` entries are the exact kernels.
template <template <int, int, bool> class K>
StatsKernel pick1(int model, int jac, bool fast) {
  static const StatsKernel t[2][MODEL_COUNT][3] = {{{K<0, 0, false>::fn, K<0, 1, false>::fn, K<0, 2, false>::fn},
                                                   {K<1, 0, false>::fn, K<1, 1, false>::fn, K<1, 2, false>::fn},
                                                   {K<2, 0, false>::fn, K<2, 1, false>::fn, K<2, 2, false>::fn}},
                                                  {{K<0, 0, true>::fn, K<0, 1, true>::fn, K<0, 2, true>::fn},
                                                   {K<1, 0, true>::fn, K<1, 1, true>::fn, K<1, 2, true>::fn},
                                                   {K<2, 0, false>::fn, K<2, 1, false>::fn, K<2, 2, false>::fn}}};
  return t[fast ? 1 : 0][model][jac];
}
template <int M, int J, bool F>
struct RowsK {
  static constexpr StatsKernel fn = fit_stats_rows_kernel<M, J, F>;
};
template <int M, int J, bool F>
struct WaveK {
  static constexpr StatsKernel fn = fit_stats_wave_kernel<M, J, F>;
};
template <int M, int J, bool F>
struct BlockK {
  static constexpr StatsKernel fn = fit_stats_block_kernel<M, J, F>;
};
template <int M, int J, bool F>
struct RowsRaggedK {
  static constexpr StatsKernel fn = fit_stats_ragged_rows_kernel<M, J, F>;
};
template <int M, int J, bool F>
struct WaveRaggedK {
  static constexpr StatsKernel fn = fit_stats_ragged_wave_kernel<M, J, F>;
};
template <int M, int J, bool F>
struct BlockRaggedK {
  static constexpr StatsKernel fn = fit_stats_ragged_block_kernel<M, J, F>;
};
// the uniform instance, or with per-fit counts the RAGGED one
template <template <int, int, bool> class K, template <int, int, bool> class KR>
StatsKernel pick(int model, int jac, bool fast, bool ragged) {
  return ragged ? pick1<KR>(model, jac, fast) : pick1<K>(model, jac, fast);
}
template <int M, int J, bool F>
struct PartialK {
  static constexpr StatsKernel fn = fit_stats_partial_kernel<M, J, F>;
};

typedef void (*WeightedStatsKernel)(WeightedStatsCtx);
WeightedStatsKernel pick_weighted(int model, int jac, bool fast) {  // (pick1's table: Ward's `fast` entries are the exact kernels)
#define WK(M, J, F) fit_stats_weighted_rows_kernel<M, J, F>
  static const WeightedStatsKernel t[2][MODEL_COUNT][3] = {{{WK(0, 0, false), WK(0, 1, false), WK(0, 2, false)},
                                                           {WK(1, 0, false), WK(1, 1, false), WK(1, 2, false)},
                                                           {WK(2, 0, false), WK(2, 1, false), WK(2, 2, false)}},
                                                          {{WK(0, 0, true), WK(0, 1, true), WK(0, 2, true)},
                                                           {WK(1, 0, true), WK(1, 1, true), WK(1, 2, true)},
                                                           {WK(2, 0, false), WK(2, 1, false), WK(2, 2, false)}}};
#undef WK
  return t[fast ? 1 : 0][model][jac];
}

// BRDF_HIP_STATS_FAST=1: the A/B variant DESIGN.md section 2 measures (the pass is bound by fp64 issue, and pow is most of it).  It is
// NOT the default and has no exact fallback: exp(n log c) is off pow(c, n) by up to |n log c| ulp of the specular term, which the
// statistics' parity bound (4 ulp of a model value) does not cover, and a cosine <= 0 turns the fit's sums into NaN (rank 0).
bool stats_fast_path() { return switch_on(kSwStatsFast); }

#define STATS_OK(call)                                                        \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", who, #call, hipGetErrorString(e_));    \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

}  // namespace

int fit_stats_check(const FitStatsArgs &a, const char *who) {
  MethodSpec ms;
  if (!known_model_method(a.model, a.method, &ms, who)) return kLmError;
  if (!a.d_angles || !a.d_x || !a.d_p) {
    set_error("%s(): null angles, x or p", who);
    return kLmError;
  }
  if (a.S <= 0 || a.n < kM || a.n > kMaxSamples) {  // (the sample loops step an int index by a workgroup's width)
    set_error("%s(): S = %d, n = %d: need S > 0 and %d <= n <= %d samples per fit", who, a.S, a.n, kM, kMaxSamples);
    return kLmError;
  }
  if (!a.d_covar && !a.d_stats && !a.d_rank) {
    set_error("%s(): covar, stats and rank are all NULL: nothing to compute", who);
    return kLmError;
  }
  return 0;
}

namespace {
int stats_launches(const FitStatsArgs &a, const char *who, bool refused_large);

// one fit of the batch: S = 1, its row of p and of the outputs (angles, x, n and the counts are the caller's to set)
FitStatsArgs row_of(const FitStatsArgs &a, long long row) {
  FitStatsArgs f = a;
  f.S = 1;
  f.d_p = a.d_p + row * kM;
  f.d_covar = a.d_covar ? a.d_covar + row * kM * kM : nullptr;
  f.d_stats = a.d_stats ? a.d_stats + row * kStatsSz : nullptr;
  f.d_rank = a.d_rank ? a.d_rank + row : nullptr;
  return f;
}
}  // namespace

int big_fit_stats_enqueue(const FitStatsArgs &a, const BigFit &b, const double *planes, const char *who) {
  FitStatsArgs f = row_of(a, b.row);
  f.d_angles = planes;
  f.d_x = b.d_x;
  f.n = b.k;
  f.d_counts = nullptr;
  return fit_stats_enqueue(f, who);
}

// ragged statistics of fits with a stride above 4096: one after the other.  A fit of k >= 3 samples is the uniform pass on its three
// plane prefixes packed next to each other; a refused one (k < 3) takes the ragged workgroup kernel, which reads the first k samples
// of the row where it lies.
namespace {
int stats_of_large_ragged(const FitStatsArgs &a, const char *who) {
  if (a.d_src) {
    set_error("%s(): row indirection with per-fit counts is limited to n <= %d", who, kBlockMaxN);
    return kLmError;
  }
  std::vector<int> counts((size_t)a.S);
  STATS_OK(hipMemcpyAsync(counts.data(), a.d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost, a.stream));
  STATS_OK(hipStreamSynchronize(a.stream));
  DeviceBlock<double> pack;
  for (int s = 0; s < a.S; ++s) {
    const int k = (counts[s] < 0 || counts[s] > a.n) ? 0 : counts[s];
    const BigFit b = {a.d_angles + (size_t)s * 3 * a.n, a.d_x + (size_t)s * a.n, k, a.n, s};
    if (k >= kM) {
      if (pack_plane_prefixes(b, pack, a.stream) != 0 || big_fit_stats_enqueue(a, b, pack.ptr, who) != 0) return kLmError;
    } else {
      FitStatsArgs f = row_of(a, s);
      f.d_angles = b.d_angles;
      f.d_x = b.d_x;
      f.d_counts = a.d_counts + s;
      if (stats_launches(f, who, true) != 0) return kLmError;
    }
  }
  STATS_OK(hipStreamSynchronize(a.stream));  // (the packed planes are about to go away)
  return 0;
}
}  // namespace

int fit_stats_enqueue(const FitStatsArgs &a, const char *who) {
  if (fit_stats_check(a, who) != 0) return kLmError;
  if (a.d_counts && a.n > kBlockMaxN) return stats_of_large_ragged(a, who);
  return stats_launches(a, who, false);
}

namespace {
// refused_large: one fit of fewer than kM samples in rows of a stride above 4096 -- the workgroup kernel, whatever the stride
int stats_launches(const FitStatsArgs &a, const char *who, bool refused_large) {
  StatsCtx c;
  c.angles = a.d_angles;
  c.x = a.d_x;
  c.p = a.d_p;
  c.src = a.d_src;
  c.covar = a.d_covar;
  c.stats = a.d_stats;
  c.rank = a.d_rank;
  c.partials = nullptr;
  c.rows = a.d_src ? a.rows : a.S;
  c.n = a.n;
  c.counts = a.d_counts;
  const bool ragged = a.d_counts != nullptr;
  c.chunk = c.nb = 0;
  // "opts==NULL": forward differences with LM_DIFF_DELTA (lmbc_core.c:1088); opts[4] < 0: central, step |opts[4]| (lm_core.c:515-519)
  const double d4 = a.opts ? a.opts[4] : LM_DIFF_DELTA;
  c.delta = d4 < 0.0 ? -d4 : d4;
  const bool fast = stats_fast_path();
  MethodSpec ms;
  (void)method_spec(a.method, &ms);
  const int jac = ms.analytic ? JAC_ANALYTIC : (d4 < 0.0 ? JAC_CENTRAL : JAC_FORWARD);
  if (c.rows <= 0) return 0;
  (void)hipGetLastError();
  if (a.n <= 16) {
    const long long blocks = (c.rows + kRowsFits - 1) / kRowsFits;
    hipLaunchKernelGGL((pick<RowsK, RowsRaggedK>(a.model, jac, fast, ragged)), dim3((unsigned)blocks), dim3(kRowsThreads), 0, a.stream, c);
  } else if (a.n <= kWaveMaxN) {
    const long long blocks = (c.rows + kWaveFits - 1) / kWaveFits;
    hipLaunchKernelGGL((pick<WaveK, WaveRaggedK>(a.model, jac, fast, ragged)), dim3((unsigned)blocks), dim3(kWaveThreads), 0, a.stream, c);
  } else if (a.n <= kBlockMaxN || refused_large) {
    hipLaunchKernelGGL((pick<BlockK, BlockRaggedK>(a.model, jac, fast, ragged)), dim3((unsigned)c.rows), dim3(kBlockThreads), 0, a.stream, c);
  } else {
    // chunks of a whole number of sweeps of the workgroup, at least 4096 samples, at most kMaxPartials of them per fit
    long long chunk = ((long long)a.n + kMaxPartials - 1) / kMaxPartials;
    if (chunk < kBlockMaxN) chunk = kBlockMaxN;
    chunk = (chunk + kBlockThreads - 1) / kBlockThreads * kBlockThreads;
    c.chunk = (int)chunk;
    c.nb = (int)(((long long)a.n + chunk - 1) / chunk);
    if (c.rows * c.nb > 0x7fffffffLL) {
      set_error("%s(): %lld fits of %d samples need more than 2^31-1 workgroups; split the batch", who, c.rows, a.n);
      return kLmError;
    }
    void *part = nullptr;
    STATS_OK(hipMallocAsync(&part, sizeof(double) * kRow * (size_t)c.rows * c.nb, a.stream));
    c.partials = static_cast<double *>(part);
    const unsigned grid = (unsigned)(c.rows * c.nb);
    hipLaunchKernelGGL(pick1<PartialK>(a.model, jac, fast), dim3(grid), dim3(kBlockThreads), 0, a.stream, c);
    hipLaunchKernelGGL(fit_stats_spread_kernel, dim3(grid), dim3(kBlockThreads), 0, a.stream, c);
    hipLaunchKernelGGL(fit_stats_fold_kernel, dim3((unsigned)c.rows), dim3(kBlockThreads), 0, a.stream, c);
    const hipError_t le = hipGetLastError();
    STATS_OK(hipFreeAsync(part, a.stream));
    STATS_OK(le);
    return 0;
  }
  STATS_OK(hipGetLastError());
  return 0;
}
}  // namespace

// ---- the weighted problem (weighted_fit.h) -------------------------------------------------------------------------------------
int weighted_stats_check(const WeightedStatsArgs &a, const char *who) {
  if (fit_stats_check(a.stats, who) != 0) return kLmError;
  if (a.stats.method != BRDF_METHOD_BC_DIF && a.stats.method != BRDF_METHOD_BC_DER) {
    set_error("%s(): weights are limited to BRDF_METHOD_BC_DIF and BRDF_METHOD_BC_DER (got method %d)", who, a.stats.method);
    return kLmError;
  }
  if (a.stats.n > 16) {
    set_error("%s(): weights are limited to n <= 16 samples per fit (got n = %d)", who, a.stats.n);
    return kLmError;
  }
  if (!a.d_w) {
    set_error("%s(): null weights", who);
    return kLmError;
  }
  return 0;
}

int weighted_stats_enqueue(const WeightedStatsArgs &wa, const char *who) {
  if (weighted_stats_check(wa, who) != 0) return kLmError;
  const FitStatsArgs &a = wa.stats;
  WeightedStatsCtx c;
  c.angles = a.d_angles;
  c.x = a.d_x;
  c.w = wa.d_w;
  c.p = a.d_p;
  c.extra = wa.d_extra_ss;
  c.counts = a.d_counts;
  c.nobs = wa.d_nobs;
  c.covar = a.d_covar;
  c.stats = a.d_stats;
  c.rank = a.d_rank;
  c.rows = a.S;
  c.n = a.n;
  const double d4 = a.opts ? a.opts[4] : LM_DIFF_DELTA;  // (stats_launches' reading of opts[4])
  c.delta = d4 < 0.0 ? -d4 : d4;
  MethodSpec ms;
  (void)method_spec(a.method, &ms);
  const int jac = ms.analytic ? JAC_ANALYTIC : (d4 < 0.0 ? JAC_CENTRAL : JAC_FORWARD);
  (void)hipGetLastError();
  const long long blocks = (c.rows + kRowsFits - 1) / kRowsFits;
  hipLaunchKernelGGL(pick_weighted(a.model, jac, stats_fast_path()), dim3((unsigned)blocks), dim3(kRowsThreads), 0, a.stream, c);
  STATS_OK(hipGetLastError());
  return 0;
}

}  // namespace brdf
