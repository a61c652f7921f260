// capture_means_clip.hip -- the clip rounds of brdf_hip_fit_capture_means_clipped_dev (capture_means_clip.h holds the definition).
//
// The clip state is two bytes per (fit, light): the interval [lo, hi] of grey levels that are still in the fit's sample set.  A round
// narrows a TENTATIVE copy, accumulates the integer sums again under it, and adopts it per fit only where the guard lets the clip
// stand.  No per-candidate array, no float atomics: the property capture_means.hip states in its header.
//
//   sigma       per fit: the threshold kappa * sigma from the statistics pass's sumsq, the settled flag
//   interval    per (fit, light): f_l(p) ONCE on the exact path, then the interval shrinks from both ends while its end fails
//               fabs(v / 255.0 - f) <= threshold -- the comparison is monotone on either side of f, so what is left is the smallest to
//               the largest surviving grey level.  A settled fit's tentative interval is its own.
//   accumulate  capture_means.hip's accumulate with `valid && lo <= v <= hi`: LDS integer atomics, then one global integer atomic per
//               touched word.  Every candidate, every round: a settled fit's sums come out as they were.
//   guard       per fit: nothing dropped or fewer than 3 lights keep a sample -> settled, nothing is adopted.  Otherwise the
//               intervals are adopted and rounds_used = r; two integer counters tell the host the fits to refit and the samples dropped.
//   pack        per fit: the rows of the fits the guard let through, again from the sums (means_pack_rows: round 0's arithmetic)
//   scan        capture_compact.h's, one workgroup: the clipped fits' places in a dense batch, in fit order
//   gather      per (fit, light): the clipped fits' rows, counts and p into the dense batch -- a settled fit is never fitted again
//   fit         weighted_fit_enqueue on the dense batch, from the current p
//   take        per fit: p, info and ret of the clipped fits back to their rows
#include <cmath>
#include <type_traits>

#include "../../include/brdf_levmar.h"
#include "capture_means_clip.h"
#include "brdf_models.h"
#include "clip_fit.h"
#include "fit_stats.h"
#include "weighted_fit.h"

namespace brdf {

namespace {

constexpr int kSettled = 1, kClipped = 2;  // a fit's state: settled for good; clipped in this round (its refit is taken)
constexpr int kMeansMaxL = 16;
constexpr int kLocalWords = 3 * (kCT + 2 * kMeansMaxL);  // capture_means.hip's: a workgroup's face ranks, 3 L words each

// the uniforms of f(p) of one fit, as model_value reads them
struct FitUniforms {
  Lin l0;
  Nl n0;
};

struct ClipCtx {
  MeansState m;
  int fits, round;
  double kappa, sigma_min;
  const double *stats;  // [fits][kStatsSz]
  double *info;         // [fits][10] or null
  int *ret;             // [fits]
  double *thr;          // [fits]
  int *state, *rounds_used;           // [fits]
  unsigned char *lo, *hi, *tlo, *thi;  // [fits][L]: the intervals, and this round's tentative ones
  unsigned long long *head;  // of this round: {fits clipped, samples dropped}
  int *flag;                 // [F][3]: 1 = fit channel * F + rank was clipped in this round
  const long long *dense_of;  // [F][3]: its place in the dense batch
  // the dense batch of the fits clipped in this round: rows of stride L
  double *da, *dx, *dw, *dp, *dinfo;
  int *dlights, *dret;
};

// ---- the initial intervals ----------------------------------------------------------------------------------------------------
// one lane per (fit, light): the rule's grey levels where the light's cosines pass it (capture_compact.h: read_candidate), empty otherwise
__global__ __launch_bounds__(kCT) void means_clip_init_kernel(CandidateCtx c, unsigned char *__restrict__ lo, unsigned char *__restrict__ hi) {
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t >= 3LL * c.F * c.L) return;
  const int i = (int)(t % c.L), r = (int)((t / c.L) % c.F);
  const double *a = c.angles_f + (size_t)r * 3 * c.L + i;
  const bool cos_ok = a[0] > c.cos_min && (!c.use1 || a[c.L] > c.cos_min) && (!c.use2 || a[2 * c.L] > c.cos_min);  // (a NaN is not valid)
  const int v0 = c.v_min < 0 ? 0 : (c.v_min > 255 ? 255 : c.v_min), v1 = c.v_max < 0 ? 0 : (c.v_max > 255 ? 255 : c.v_max);
  lo[t] = cos_ok ? (unsigned char)v0 : 1;
  hi[t] = cos_ok ? (unsigned char)v1 : 0;
}

// ---- a clip round -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCT) void means_clip_sigma_kernel(ClipCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= c.fits) return;
  bool settled = (c.state[s] & kSettled) != 0;
  if (!settled) {
    const int k = c.m.nobs[s];
    const double sumsq = c.stats[(size_t)s * kStatsSz];
    if (c.ret[s] < 0 || c.m.lights[s] < 3 || !isfinite(sumsq)) {
      settled = true;
    } else {
      const double sigma = k > 3 ? fmax(sqrt(sumsq / (double)(k - 3)), c.sigma_min) : c.sigma_min;
      c.thr[s] = c.kappa * sigma;
    }
  }
  c.state[s] = settled ? kSettled : 0;
}

// one lane per (fit, light)
template <int MODEL>
__global__ __launch_bounds__(kCT) void means_clip_interval_kernel(ClipCtx c) {
  using Mdl = BrdfModel<MODEL>;
  const int L = c.m.cand.L;
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t >= (long long)c.fits * L) return;
  const long long s = t / L;
  const int i = (int)(t - s * L), r = (int)(s % c.m.cand.F);
  int lo = c.lo[t], hi = c.hi[t];
  if (!(c.state[s] & kSettled) && lo <= hi) {
    const double *__restrict__ a = c.m.cand.angles_f + (size_t)r * 3 * L + i;
    const double c0 = a[0];
    const double c1 = Mdl::uses_c1 ? a[L] : 1.0;
    const double c2 = Mdl::uses_c2 ? a[2 * L] : 1.0;
    const double *p = c.m.p + (size_t)s * kM;
    const FitUniforms u = {Mdl::lin(p), Mdl::nl(p)};
    const double f = model_value<MODEL, false>(u, c0, Mdl::template prepare<false>(c0, c1, c2));
    const double thr = c.thr[s];
    // (a NaN residual, or a NaN threshold, fails: the interval comes out empty)
    while (lo <= hi && !(fabs(lo / 255.0 - f) <= thr)) ++lo;
    while (hi >= lo && !(fabs(hi / 255.0 - f) <= thr)) --hi;
    if (lo > hi) {
      lo = 1;
      hi = 0;
    }
  }
  c.tlo[t] = (unsigned char)lo;
  c.thi[t] = (unsigned char)hi;
}

// means_accumulate_kernel (capture_means.hip) under the tentative intervals
__global__ __launch_bounds__(kCT) void means_clip_accumulate_kernel(ClipCtx c) {
  __shared__ int l_cnt[kLocalWords];
  __shared__ unsigned long long l_s1[kLocalWords], l_s2[kLocalWords];
  const CandidateCtx &cand = c.m.cand;
  const int L = cand.L, F = cand.F;
  const long long t0 = (long long)blockIdx.x * kCT, t = t0 + threadIdx.x;
  const int r0 = cand.rank_of_face[cand.face_sorted[t0 / L]];  // the lowest rank of the workgroup: ranks ascend with the sorted pixels
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    l_cnt[e] = 0;
    l_s1[e] = 0ull;
    l_s2[e] = 0ull;
  }
  __syncthreads();
  const Candidate k = read_candidate(cand, t);
  const int lr = k.r - r0;  // 0 <= lr <= kCT / L + 1
  if (lr >= 0 && (lr * 3 + 2) * L + k.i < kLocalWords) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (!k.valid[ch]) continue;
      const size_t word = ((size_t)ch * F + k.r) * L + k.i;
      const int v = k.v[ch], e = (lr * 3 + ch) * L + k.i;
      if (v < (int)c.tlo[word] || v > (int)c.thi[word]) continue;
      atomicAdd(&l_cnt[e], 1);
      atomicAdd(&l_s1[e], (unsigned long long)v);
      atomicAdd(&l_s2[e], (unsigned long long)(v * v));
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    const int n = l_cnt[e];
    if (n == 0) continue;
    const int i = e % L, ch = (e / L) % 3, r = r0 + e / (3 * L);
    const size_t word = ((size_t)ch * F + r) * L + i;
    atomicAdd(&c.m.cnt[word], n);
    atomicAdd(&c.m.s1[word], l_s1[e]);
    atomicAdd(&c.m.s2[word], l_s2[e]);
  }
}

// means_pack_kernel's pack (capture_means.hip), statement by statement, without its reset of p: a round forms a fit's rows again with
// the arithmetic of round 0.  (A copy: that kernel keeps its text, so that its code does not move.)
__device__ __forceinline__ void means_pack_rows(const MeansState &c, long long s) {
  const int r = (int)(s % c.cand.F), L = c.cand.L;
  const double *a = c.cand.angles_f + (size_t)r * 3 * L;
  double *ao = c.angles + (size_t)s * 3 * L, *xo = c.x + (size_t)s * L, *wo = c.w + (size_t)s * L;
  int n = 0;
  long long k = 0;
  double within = 0.0;
  for (int i = 0; i < L; ++i) {
    const long long cn = c.cnt[(size_t)s * L + i];
    if (cn <= 0) continue;
    const long long s1 = (long long)c.s1[(size_t)s * L + i], s2 = (long long)c.s2[(size_t)s * L + i];
    ao[n] = a[i];
    ao[L + n] = a[L + i];
    ao[2 * L + n] = a[2 * L + i];
    xo[n] = (double)s1 / (255.0 * (double)cn);
    wo[n] = (double)cn;
    within += (double)(cn * s2 - s1 * s1) / (65025.0 * (double)cn);
    k += cn;
    ++n;
  }
  c.lights[s] = n;
  c.nobs[s] = (int)k;
  c.within[s] = within;
}

// One lane per fit s = channel * F + rank.  Decided BEFORE anything is adopted: the sums under the tentative intervals tell what the
// clip would leave.
__global__ __launch_bounds__(kCT) void means_clip_guard_kernel(ClipCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= c.fits) return;
  const int F = c.m.cand.F, L = c.m.cand.L;
  const int r = (int)(s % F), ch = (int)(s / F);
  c.flag[r * 3 + ch] = 0;
  if (c.state[s] & kSettled) return;
  int n = 0;
  long long k = 0;
  for (int i = 0; i < L; ++i) {
    const int cn = c.m.cnt[(size_t)s * L + i];
    k += cn;
    n += cn > 0;
  }
  const long long k0 = c.m.nobs[s];
  if (k >= k0 || n < 3) {  // nothing dropped; or a clip that leaves fewer than 3 lights, which is not applied
    c.state[s] = kSettled;
    return;
  }
  for (int i = 0; i < L; ++i) {
    c.lo[(size_t)s * L + i] = c.tlo[(size_t)s * L + i];
    c.hi[(size_t)s * L + i] = c.thi[(size_t)s * L + i];
  }
  c.state[s] = kClipped;
  c.rounds_used[s] = c.round;
  c.flag[r * 3 + ch] = 1;
  atomicAdd(&c.head[0], 1ull);
  atomicAdd(&c.head[1], (unsigned long long)(k0 - k));
}

// one lane per fit: the rows of the fits clipped in this round, from the sums under their new intervals
__global__ __launch_bounds__(kCT) void means_clip_pack_kernel(ClipCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s < c.fits && (c.state[s] & kClipped)) means_pack_rows(c.m, s);
}

// one lane per (fit, light): the rows of the fits clipped in this round, to their places in the dense batch
__global__ __launch_bounds__(kCT) void means_clip_gather_kernel(ClipCtx c) {
  const int L = c.m.cand.L, F = c.m.cand.F;
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t >= (long long)c.fits * L) return;
  const long long s = t / L;
  if (!(c.state[s] & kClipped)) return;
  const int i = (int)(t - s * L);
  const long long d = c.dense_of[(s % F) * 3 + s / F];
  if (d < 0 || d >= c.fits) return;  // (cannot happen: the places count the flags)
  const double *a = c.m.angles + (size_t)s * 3 * L + i;
  double *ao = c.da + (size_t)d * 3 * L + i;
  ao[0] = a[0];
  ao[L] = a[L];
  ao[2 * L] = a[2 * L];
  c.dx[d * L + i] = c.m.x[s * L + i];
  c.dw[d * L + i] = c.m.w[s * L + i];
  if (i == 0) {
    c.dlights[d] = c.m.lights[s];
    for (int j = 0; j < kM; ++j) c.dp[d * kM + j] = c.m.p[s * kM + j];
  }
}

// the refit's results of the fits clipped in this round
__global__ __launch_bounds__(kCT) void means_clip_take_kernel(ClipCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= c.fits || !(c.state[s] & kClipped)) return;
  const int F = c.m.cand.F;
  const long long d = c.dense_of[(s % F) * 3 + s / F];
  if (d < 0 || d >= c.fits) return;
  for (int j = 0; j < kM; ++j) c.m.p[s * kM + j] = c.dp[d * kM + j];
  if (c.info)
    for (int j = 0; j < kInfoSz; ++j) c.info[s * kInfoSz + j] = c.dinfo[d * kInfoSz + j];
  c.ret[s] = c.dret[d];
}

__global__ __launch_bounds__(kCT) void means_clip_scatter_kernel(const int *__restrict__ face_list, int F, int L, const unsigned char *__restrict__ lo,
                                                                 const unsigned char *__restrict__ hi, unsigned char *__restrict__ s_lo,
                                                                 unsigned char *__restrict__ s_hi) {
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t >= 3LL * F * L) return;
  const long long s = t / L;
  const int i = (int)(t - s * L), r = (int)(s % F), ch = (int)(s / F);
  const size_t dst = ((size_t)face_list[r] * 3 + ch) * L + i;
  if (s_lo) s_lo[dst] = lo[t];
  if (s_hi) s_hi[dst] = hi[t];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// one allocation, carved into aligned pieces
struct Arena {
  DevBuf buf;
  size_t used = 0;
  size_t reserve(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) / 256 * 256;
    return at;
  }
  template <class T>
  T *at(size_t off) const { return reinterpret_cast<T *>(buf.as<char>() + off); }
};

unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

template <class Launch>
void launch_by_model(int model, Launch launch) {
  if (model == MODEL_PHONG) launch(std::integral_constant<int, MODEL_PHONG>());
  else if (model == MODEL_BLINN_PHONG) launch(std::integral_constant<int, MODEL_BLINN_PHONG>());
  else launch(std::integral_constant<int, MODEL_WARD>());
}

}  // namespace

int means_clip_intervals(const char *who, const CandidateCtx &cand, unsigned char *d_vlo, unsigned char *d_vhi, hipStream_t stream) {
  hipLaunchKernelGGL(means_clip_init_kernel, dim3(blocks_of(3LL * cand.F * cand.L)), dim3(kCT), 0, stream, cand, d_vlo, d_vhi);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int means_clip_scatter(const char *who, const int *d_face_list, int F, int L, const unsigned char *d_vlo, const unsigned char *d_vhi,
                       unsigned char *d_surface_vlo, unsigned char *d_surface_vhi, hipStream_t stream) {
  if (!d_surface_vlo && !d_surface_vhi) return 0;
  hipLaunchKernelGGL(means_clip_scatter_kernel, dim3(blocks_of(3LL * F * L)), dim3(kCT), 0, stream, d_face_list, F, L, d_vlo, d_vhi, d_surface_vlo,
                     d_surface_vhi);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int means_clip_run(const MeansClipArgs &a, bool *stats_fresh) {
  const char *who = a.who;
  const CaptureArgs &cap = *a.cap;
  hipStream_t stream = cap.stream;
  const int fits = a.fits, L = cap.L, F = a.ctx.cand.F;
  *stats_fresh = false;
  ClipLastStats last = {};
  clip_last_stats_set(last);
  if (a.rounds <= 0 || L < kM) return 0;  // (L < 3: every fit is refused, and settled)

  const size_t words = (size_t)fits * L;
  Arena ar;
  const size_t o_stats = ar.reserve(a.d_stats ? 0 : sizeof(double) * kStatsSz * fits), o_thr = ar.reserve(sizeof(double) * fits),
               o_da = ar.reserve(sizeof(double) * 3 * words), o_dx = ar.reserve(sizeof(double) * words), o_dw = ar.reserve(sizeof(double) * words),
               o_dp = ar.reserve(sizeof(double) * kM * fits), o_dinfo = ar.reserve(sizeof(double) * kInfoSz * fits),
               o_dense = ar.reserve(sizeof(long long) * fits), o_ends = ar.reserve(sizeof(long long) * 4),
               o_head = ar.reserve(sizeof(unsigned long long) * 2), o_state = ar.reserve(sizeof(int) * fits), o_flag = ar.reserve(sizeof(int) * fits),
               o_dlights = ar.reserve(sizeof(int) * fits), o_dret = ar.reserve(sizeof(int) * fits), o_tlo = ar.reserve(words), o_thi = ar.reserve(words);
  if (!take(ar.buf, ar.used, "the clip rounds' state", who)) return kLmError;
  double *stats = a.d_stats ? a.d_stats : ar.at<double>(o_stats);
  ClipCtx c = {};
  c.m = a.ctx;
  c.fits = fits;
  c.kappa = a.kappa;
  c.sigma_min = a.sigma_min;
  c.stats = stats;
  c.info = a.d_info;
  c.ret = a.d_ret;
  c.thr = ar.at<double>(o_thr);
  c.state = ar.at<int>(o_state);
  c.rounds_used = a.d_rounds_used;
  c.lo = a.d_vlo;
  c.hi = a.d_vhi;
  c.tlo = ar.at<unsigned char>(o_tlo);
  c.thi = ar.at<unsigned char>(o_thi);
  c.head = ar.at<unsigned long long>(o_head);
  c.flag = ar.at<int>(o_flag);
  c.dense_of = ar.at<long long>(o_dense);
  c.da = ar.at<double>(o_da);
  c.dx = ar.at<double>(o_dx);
  c.dw = ar.at<double>(o_dw);
  c.dp = ar.at<double>(o_dp);
  c.dinfo = ar.at<double>(o_dinfo);
  c.dlights = ar.at<int>(o_dlights);
  c.dret = ar.at<int>(o_dret);
  CAPTURE_OK(who, hipMemsetAsync(c.state, 0, sizeof(int) * fits, stream));

  const unsigned fb = blocks_of(fits), wb = blocks_of((long long)words), ab = blocks_of(a.ctx.cand.T);
  for (int r = 1; r <= a.rounds; ++r) {
    // sumsq of every fit at its p over its current rows.  With the caller's maps where they are asked for: should this round settle
    // every fit, they already hold the returned statistics.
    const WeightedStatsArgs ws = {{BRDF_METHOD_BC_DIF, cap.model, c.m.angles, c.m.x, fits, L, c.m.p, cap.opts, a.d_covar, stats, a.d_rank, nullptr, 0, stream,
                                   c.m.lights},
                                  c.m.w, c.m.within, c.m.nobs};
    if (weighted_stats_enqueue(ws, who) != 0) return kLmError;
    *stats_fresh = true;
    c.round = r;
    CAPTURE_OK(who, hipMemsetAsync(c.head, 0, sizeof(unsigned long long) * 2, stream));
    CAPTURE_OK(who, hipMemsetAsync(c.m.cnt, 0, sizeof(int) * words, stream));
    CAPTURE_OK(who, hipMemsetAsync(c.m.s1, 0, sizeof(long long) * words, stream));
    CAPTURE_OK(who, hipMemsetAsync(c.m.s2, 0, sizeof(long long) * words, stream));
    hipLaunchKernelGGL(means_clip_sigma_kernel, dim3(fb), dim3(kCT), 0, stream, c);
    launch_by_model(cap.model,
                    [&](auto m) { hipLaunchKernelGGL(means_clip_interval_kernel<decltype(m)::value>, dim3(wb), dim3(kCT), 0, stream, c); });
    hipLaunchKernelGGL(means_clip_accumulate_kernel, dim3(ab), dim3(kCT), 0, stream, c);
    hipLaunchKernelGGL(means_clip_guard_kernel, dim3(fb), dim3(kCT), 0, stream, c);
    hipLaunchKernelGGL(means_clip_pack_kernel, dim3(fb), dim3(kCT), 0, stream, c);
    // channel after channel: the clipped fits' places ascend with s = channel * F + rank
    long long *ends = ar.at<long long>(o_ends);
    hipLaunchKernelGGL(block_scan3_kernel<true>, dim3(1), dim3(kCT), 0, stream, c.flag, (long long)F, const_cast<long long *>(c.dense_of), ends, 0LL, ends + 1);
    CAPTURE_OK(who, hipGetLastError());
    unsigned long long head[2] = {0, 0};
    CAPTURE_OK(who, hipMemcpyAsync(head, c.head, sizeof head, hipMemcpyDeviceToHost, stream));
    CAPTURE_OK(who, hipStreamSynchronize(stream));  // the round's one readback: is any fit still active?
    last.rounds = r;
    last.active[r - 1] = (long long)head[0];
    last.clipped[r - 1] = (long long)head[1];
    clip_last_stats_set(last);
    if (head[0] == 0) break;
    if (head[0] > (unsigned long long)fits) {
      set_error("%s(): clip round %d refits %llu fits of %d", who, r, head[0], fits);
      return kLmError;
    }

    // The refit: the clipped fits' rows, dense, from their current p; the clipped ones are taken.
    const int A = (int)head[0];
    hipLaunchKernelGGL(means_clip_gather_kernel, dim3(wb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    const WeightedFitArgs wf = {{BRDF_METHOD_BC_DIF, cap.model, c.da, c.dx, A, L, c.dp, cap.lb, cap.ub, cap.itmax, cap.opts, a.d_info ? c.dinfo : nullptr, c.dret,
                                 stream, c.dlights},
                                c.dw};
    if (weighted_fit_enqueue(wf, who) != 0) return kLmError;
    hipLaunchKernelGGL(means_clip_take_kernel, dim3(fb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    *stats_fresh = false;
  }
  CAPTURE_OK(who, hipStreamSynchronize(stream));  // (the arena is about to go away)
  return 0;
}

}  // namespace brdf
