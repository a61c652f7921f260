// capture_means.hip -- brdf_hip_fit_capture_means_dev: the per-face capture of capture_faces.hip as a WEIGHTED fit of per-light means.
//
// All pixels of a face share the face's cosine triples, so the model values f_l(p) are the same for every pixel of the face.  With
// c_l valid values v_pl under light l, their mean m_l = sum_p v_pl / (255 c_l) and the spread inside the lights
// within = sum_l sum_p (v_pl / 255 - m_l)^2:
//
//   sum_{p,l} (v_pl / 255 - f_l(p))^2  =  sum_l c_l (m_l - f_l(p))^2  +  within
//
// `within` does not depend on p: the fit of all the face's samples and the fit of at most L means weighted by c_l have the same
// minimiser and the same J^T J.  The weighted fit has n <= 16 -- the lane-per-fit kernel's size (weighted_fit.hip) -- whatever the face's
// number of pixels, and no per-candidate array is ever written.
//
//   group       capture_group.hip: compaction, sort by face, carried faces, their cosines -- capture_faces.hip's, shared
//   accumulate  one lane per candidate (sorted pixel, light), all three channels: per (fit, light) the count c, S1 = sum v and S2 = sum v^2
//               as INTEGERS.  LDS integer atomics inside the workgroup (a workgroup's candidates belong to consecutive face ranks), then
//               one global integer atomic per word that got a sample.  Integer adds: their order cannot show; no float atomics.
//   pack        one lane per fit s = channel * F + face rank: the lights with c > 0, ascending, into rows of stride L -- the face's
//               cosines there, x = S1 / (255 c), w = c --, their number, k = sum c, and
//               within = sum_l (c S2 - S1^2) / (65025 c): the numerator exactly in 64-bit integers, one division per light
//   fit, stats  weighted_fit_enqueue (dlevmar_bc_dif), weighted_stats_enqueue with extra_ss = within and nobs = k: sumsq, the
//               covariance, sigma, rho and R^2 are those of the fit of all k samples
//   scatter     rows (face, channel) in ascending order, block sums of p in a fixed order: capture_group.hip's, with the lights map
// brdf_hip_fit_capture_means_clipped_dev (CaptureMeansArgs::clip) runs the clip rounds of capture_means_clip.hip between the fit and the
// statistics, and scatters four more maps.
#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "capture_means_clip.h"
#include "clip_fit.h"
#include "fit_stats.h"
#include "weighted_fit.h"

namespace brdf {

namespace {

constexpr const char *kWhoPlain = "brdf_hip_fit_capture_means_dev", *kWhoClipped = "brdf_hip_fit_capture_means_clipped_dev";
constexpr int kMeansMaxL = 16;
// a workgroup's kCT candidates touch at most kCT / L + 2 sorted pixels, so at most that many face ranks, each with 3 L words
constexpr int kLocalWords = 3 * (kCT + 2 * kMeansMaxL);
// c S2 - S1^2 <= (255 c)^2 must fit a signed 64-bit integer
constexpr long long kMeansMaxPixels = 11000000;

struct MeansCtx : MeansState {};  // (capture_means_clip.h)

__global__ __launch_bounds__(kCT) void means_accumulate_kernel(MeansCtx c) {
  __shared__ int l_cnt[kLocalWords];
  __shared__ unsigned long long l_s1[kLocalWords], l_s2[kLocalWords];
  const int L = c.cand.L, F = c.cand.F;
  const long long t0 = (long long)blockIdx.x * kCT, t = t0 + threadIdx.x;
  const int r0 = c.cand.rank_of_face[c.cand.face_sorted[t0 / L]];  // the lowest rank of the workgroup: ranks ascend with the sorted pixels
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    l_cnt[e] = 0;
    l_s1[e] = 0ull;
    l_s2[e] = 0ull;
  }
  __syncthreads();
  const Candidate k = read_candidate(c.cand, t);
  const int lr = k.r - r0;  // 0 <= lr <= kCT / L + 1
  if (lr >= 0 && (lr * 3 + 2) * L + k.i < kLocalWords) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (k.valid[ch]) {
        const int v = k.v[ch], e = (lr * 3 + ch) * L + k.i;
        atomicAdd(&l_cnt[e], 1);
        atomicAdd(&l_s1[e], (unsigned long long)v);
        atomicAdd(&l_s2[e], (unsigned long long)(v * v));
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    const int n = l_cnt[e];
    if (n == 0) continue;
    const int i = e % L, ch = (e / L) % 3, r = r0 + e / (3 * L);
    const size_t word = ((size_t)ch * F + r) * L + i;
    atomicAdd(&c.cnt[word], n);
    atomicAdd(&c.s1[word], l_s1[e]);
    atomicAdd(&c.s2[word], l_s2[e]);
  }
}

// one lane per fit s = channel * F + rank
__global__ __launch_bounds__(kCT) void means_pack_kernel(MeansCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= 3LL * c.cand.F) return;
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
  for (int j = 0; j < kM; ++j) c.p[(size_t)s * kM + j] = c.p0[j];
}

}  // namespace

int capture_means_run(const CaptureMeansArgs &ma) {
  const CaptureFacesArgs &a = ma.faces;
  const CaptureArgs &cap = a.g.cap;
  const CaptureClip *clip = ma.clip ? &ma.clip->clip : nullptr;
  const char *kWho = clip ? kWhoClipped : kWhoPlain;
  // what the entry refuses before any HIP call
  if (capture_args_check(kWho, a.g, a.d_brdf_surfaces, "brdf_surfaces", kMeansMaxL,
                         " (the weighted fit's size class; brdf_hip_fit_capture_faces_dev takes L <= 64)") != 0)
    return kLmError;
  if (clip && clip_spec_check(ClipSpec{clip->kappa, clip->sigma_min, clip->rounds}, kWho) != 0) return kLmError;
  (void)hipGetLastError();
  hipStream_t stream = cap.stream;
  const int L = cap.L;
  if (a.avg) a.avg[0] = a.avg[1] = a.avg[2] = 0.0;
  if (a.g.n_pixels) *a.g.n_pixels = 0;
  if (a.g.n_faces) *a.g.n_faces = 0;

  // ---- compact, group, cosines (capture_group.hip) ----
  CaptureGroup g;
  if (capture_group_run(kWho, a.g, g) != 0) return kLmError;
  if (g.S == 0) return 0;  // an empty capture: nothing is written but the pixel counts
  if (g.max_pixels > kMeansMaxPixels) {
    set_error("%s(): a face has %lld pixels, more than the %lld whose sums of squares fit 64-bit integers", kWho, g.max_pixels, kMeansMaxPixels);
    return kLmError;
  }

  // ---- accumulate and pack ----
  const int fits = (int)(3 * g.F);
  const size_t words = (size_t)fits * L;
  DevBuf cnt, s1, s2, angles, x, w, within, p, lights, nobs;
  if (!take(cnt, sizeof(int) * words, "the lights' counts", kWho) || !take(s1, sizeof(long long) * words, "the lights' sums", kWho) ||
      !take(s2, sizeof(long long) * words, "the lights' sums of squares", kWho) || !take(angles, sizeof(double) * 3 * words, "the fits' planes", kWho) ||
      !take(x, sizeof(double) * words, "the fits' means", kWho) || !take(w, sizeof(double) * words, "the fits' weights", kWho) ||
      !take(within, sizeof(double) * (size_t)fits, "the fits' inner sums of squares", kWho) ||
      !take(p, sizeof(double) * kM * (size_t)fits, "the fits' parameters", kWho) || !take(lights, sizeof(int) * (size_t)fits, "the fits' light counts", kWho) ||
      !take(nobs, sizeof(int) * (size_t)fits, "the fits' sample counts", kWho))
    return kLmError;
  CAPTURE_OK(kWho, hipMemsetAsync(cnt.ptr, 0, sizeof(int) * words, stream));
  CAPTURE_OK(kWho, hipMemsetAsync(s1.ptr, 0, sizeof(long long) * words, stream));
  CAPTURE_OK(kWho, hipMemsetAsync(s2.ptr, 0, sizeof(long long) * words, stream));
  MeansCtx mc = {};
  mc.cand = capture_candidates(a.g, g);
  mc.cnt = cnt.as<int>();
  mc.s1 = s1.as<unsigned long long>();
  mc.s2 = s2.as<unsigned long long>();
  mc.angles = angles.as<double>();
  mc.x = x.as<double>();
  mc.w = w.as<double>();
  mc.within = within.as<double>();
  mc.p = p.as<double>();
  mc.lights = lights.as<int>();
  mc.nobs = nobs.as<int>();
  for (int k = 0; k < kM; ++k) mc.p0[k] = cap.p0[k];
  const int ab = (int)((mc.cand.T + kCT - 1) / kCT), fb = (fits + kCT - 1) / kCT;
  hipLaunchKernelGGL(means_accumulate_kernel, dim3(ab), dim3(kCT), 0, stream, mc);
  hipLaunchKernelGGL(means_pack_kernel, dim3(fb), dim3(kCT), 0, stream, mc);
  CAPTURE_OK(kWho, hipGetLastError());

  // ---- fit and statistics: the weighted problem, n = L ----
  const bool want_stats = a.d_surface_covar || a.d_surface_stats || a.d_surface_rank;
  FitResultBufs res;
  if (!take_fit_results(res, a, fits, kWho)) return kLmError;
  // (the clip rounds read every fit's ret)
  const bool rounds = clip && clip->rounds > 0;
  DevBuf own_ret;
  if (rounds && !res.ret.ptr && !take(own_ret, sizeof(int) * (size_t)fits, "the fits' ret", kWho)) return kLmError;
  int *ret = res.ret.ptr ? res.ret.as<int>() : own_ret.as<int>();
  const WeightedFitArgs wf = {{BRDF_METHOD_BC_DIF, cap.model, angles.as<double>(), x.as<double>(), fits, L, p.as<double>(), cap.lb, cap.ub, cap.itmax, cap.opts,
                               res.info.as<double>(), ret, stream, lights.as<int>()},
                              w.as<double>()};
  if (weighted_fit_enqueue(wf, kWho) != 0) return kLmError;

  // ---- the clip rounds (capture_means_clip.hip): the intervals, the counts of round 0, rounds_used ----
  DevBuf vlo, vhi, nobs0, rounds_used;
  bool stats_fresh = false;
  if (clip) {
    if (!take(vlo, words, "the lights' lowest grey levels", kWho) || !take(vhi, words, "the lights' highest grey levels", kWho)) return kLmError;
    if (means_clip_intervals(kWho, mc.cand, vlo.as<unsigned char>(), vhi.as<unsigned char>(), stream) != 0) return kLmError;
  }
  if (rounds) {
    if (!take(nobs0, sizeof(int) * (size_t)fits, "the fits' unclipped sample counts", kWho) ||
        !take(rounds_used, sizeof(int) * (size_t)fits, "the fits' rounds", kWho))
      return kLmError;
    CAPTURE_OK(kWho, hipMemcpyAsync(nobs0.ptr, nobs.ptr, sizeof(int) * (size_t)fits, hipMemcpyDeviceToDevice, stream));
    CAPTURE_OK(kWho, hipMemsetAsync(rounds_used.ptr, 0, sizeof(int) * (size_t)fits, stream));
    const MeansClipArgs ca = {kWho, mc, &cap, fits, clip->kappa, clip->sigma_min, clip->rounds, res.info.as<double>(), ret, res.covar.as<double>(),
                              res.stats.as<double>(), res.rank.as<int>(), rounds_used.as<int>(), vlo.as<unsigned char>(), vhi.as<unsigned char>()};
    if (means_clip_run(ca, &stats_fresh) != 0) return kLmError;
  } else if (clip) {
    clip_last_stats_set(ClipLastStats{});
  }

  // ---- the statistics at the returned p over the returned rows ----
  if (want_stats && L >= kM && !stats_fresh) {
    const WeightedStatsArgs ws = {{BRDF_METHOD_BC_DIF, cap.model, angles.as<double>(), x.as<double>(), fits, L, p.as<double>(), cap.opts, res.covar.as<double>(),
                                   res.stats.as<double>(), res.rank.as<int>(), nullptr, 0, stream, lights.as<int>()},
                                  w.as<double>(), within.as<double>(), nobs.as<int>()};
    if (weighted_stats_enqueue(ws, kWho) != 0) return kLmError;
  } else if (want_stats && L < kM) {  // fewer than three lights: every fit is refused, there is nothing to take statistics of
    if (res.covar.ptr) CAPTURE_OK(kWho, hipMemsetAsync(res.covar.ptr, 0, sizeof(double) * kM * kM * (size_t)fits, stream));
    if (res.stats.ptr) CAPTURE_OK(kWho, hipMemsetAsync(res.stats.ptr, 0, sizeof(double) * kStatsSz * (size_t)fits, stream));
    if (res.rank.ptr) CAPTURE_OK(kWho, hipMemsetAsync(res.rank.ptr, 0, sizeof(int) * (size_t)fits, stream));
  }

  // ---- scatter (capture_group.hip); `count` stays the unclipped sample count, `lights` is the returned set's ----
  if (clip) {
    if (clip_scatter_maps(kWho, g.face_list.as<int>(), (int)g.F, nobs.as<int>(), rounds_used.as<int>(), nullptr, clip->d_surface_kept, clip->d_surface_rounds,
                          stream) != 0 ||
        means_clip_scatter(kWho, g.face_list.as<int>(), (int)g.F, L, vlo.as<unsigned char>(), vhi.as<unsigned char>(), ma.clip->d_surface_vlo,
                           ma.clip->d_surface_vhi, stream) != 0)
      return kLmError;
  }
  const ScatterArgs sc = {&a, &g, p.as<double>(), &res, nullptr, rounds ? nobs0.as<int>() : nobs.as<int>(), lights.as<int>(), ma.d_surface_lights};
  return capture_scatter_run(kWho, sc);
}

}  // namespace brdf
