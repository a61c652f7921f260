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
//   group       capture_group.h: compaction, sort by face, carried faces, their cosines -- capture_faces.hip's, shared
//   accumulate  one lane per candidate (sorted pixel, light), all three channels: per (fit, light) the count c, S1 = sum v and S2 = sum v^2
//               as INTEGERS.  LDS integer atomics inside the workgroup (a workgroup's candidates belong to consecutive face ranks), then
//               one global integer atomic per word that got a sample.  Integer adds: their order cannot show; no float atomics.
//   pack        one lane per fit s = channel * F + face rank: the lights with c > 0, ascending, into rows of stride L -- the face's
//               cosines there, x = S1 / (255 c), w = c --, their number, k = sum c, and
//               within = sum_l (c S2 - S1^2) / (65025 c): the numerator exactly in 64-bit integers, one division per light
//   fit, stats  weighted_fit_enqueue (dlevmar_bc_dif), weighted_stats_enqueue with extra_ss = within and nobs = k: sumsq, the
//               covariance, sigma, rho and R^2 are those of the fit of all k samples
//   scatter     rows (face, channel) in ascending order, block sums of p in a fixed order: capture_faces.hip's scheme
#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "fit_stats.h"
#include "weighted_fit.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_means_dev";
constexpr int kMeansMaxL = 16;
// a workgroup's kCT candidates touch at most kCT / L + 2 sorted pixels, so at most that many face ranks, each with 3 L words
constexpr int kLocalWords = 3 * (kCT + 2 * kMeansMaxL);
// c S2 - S1^2 <= (255 c)^2 must fit a signed 64-bit integer
constexpr long long kMeansMaxPixels = 11000000;

struct MeansCtx {
  const unsigned char *images;
  int L, H, W;
  const long long *pixel_sorted;  // [S]
  const unsigned *face_sorted;    // [S]
  const int *rank_of_face;        // [nf]
  const double *angles_f;         // [F][3][L]
  long long T;                    // candidates of one channel: S * L
  int F;
  int v_min, v_max;
  double cos_min;
  int use1, use2;
  // accumulators, word (channel * F + rank) * L + light
  int *cnt;
  unsigned long long *s1, *s2;
  // the weighted batch: rows of stride L
  double *angles, *x, *w, *within, *p;
  int *lights, *nobs;
  double p0[kM];
};

__global__ __launch_bounds__(kCT) void means_accumulate_kernel(MeansCtx c) {
  __shared__ int l_cnt[kLocalWords];
  __shared__ unsigned long long l_s1[kLocalWords], l_s2[kLocalWords];
  const long long t0 = (long long)blockIdx.x * kCT, t = t0 + threadIdx.x;
  const int r0 = c.rank_of_face[c.face_sorted[t0 / c.L]];  // the lowest rank of the workgroup: ranks ascend with the sorted pixels
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    l_cnt[e] = 0;
    l_s1[e] = 0ull;
    l_s2[e] = 0ull;
  }
  __syncthreads();
  if (t < c.T) {
    const long long s = t / c.L;
    const int i = (int)(t - s * c.L);
    const int r = c.rank_of_face[c.face_sorted[s]];
    const long long g = c.pixel_sorted[s];
    const int px = (int)(g / c.H), py = (int)(g % c.H);
    const unsigned char *pxl = c.images + (((size_t)i * c.H + (size_t)(c.H - 1 - py)) * c.W + px) * 3;
    const double *a = c.angles_f + (size_t)r * 3 * c.L + i;
    const double c0 = a[0], c1 = a[c.L], c2 = a[2 * c.L];
    const bool cos_ok = c0 > c.cos_min && (!c.use1 || c1 > c.cos_min) && (!c.use2 || c2 > c.cos_min);  // (a NaN is not valid)
    const int lr = r - r0;  // 0 <= lr <= kCT / L + 1
    if (cos_ok && lr >= 0 && (lr * 3 + 2) * c.L + i < kLocalWords) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int v = pxl[ch];
        if (v >= c.v_min && v <= c.v_max) {
          const int e = (lr * 3 + ch) * c.L + i;
          atomicAdd(&l_cnt[e], 1);
          atomicAdd(&l_s1[e], (unsigned long long)v);
          atomicAdd(&l_s2[e], (unsigned long long)(v * v));
        }
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLocalWords; e += kCT) {
    const int n = l_cnt[e];
    if (n == 0) continue;
    const int i = e % c.L, ch = (e / c.L) % 3, r = r0 + e / (3 * c.L);
    const size_t word = ((size_t)ch * c.F + r) * c.L + i;
    atomicAdd(&c.cnt[word], n);
    atomicAdd(&c.s1[word], l_s1[e]);
    atomicAdd(&c.s2[word], l_s2[e]);
  }
}

// one lane per fit s = channel * F + rank
__global__ __launch_bounds__(kCT) void means_pack_kernel(MeansCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= 3LL * c.F) return;
  const int r = (int)(s % c.F), L = c.L;
  const double *a = c.angles_f + (size_t)r * 3 * L;
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

struct MeansScatterCtx {
  int F;
  const int *face_list;
  const double *p, *info, *covar, *stats;  // the batch's results, rows channel * F + face rank; null: not computed
  const int *ret, *rank, *nobs, *lights;
  double *surfaces, *s_info, *s_covar, *s_stats;  // the [nf][3] maps; null (all but surfaces): not wanted
  int *s_ret, *s_rank, *s_count, *s_lights;
  double *block_sums;  // [blocks][3]
};

// One thread per (carried face, channel), in ascending order of the destination rows; per-block partial sums of kd, ks, n in a fixed
// order (face_scatter_kernel's scheme in capture_faces.hip)
__global__ __launch_bounds__(kCT) void means_scatter_kernel(MeansScatterCtx c) {
  __shared__ double red[3][kCT];
  const long long q = (long long)blockIdx.x * kCT + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (q < 3LL * c.F) {
    const int r = (int)(q / 3), ch = (int)(q - 3LL * r);
    const size_t src = (size_t)ch * c.F + r, dst = (size_t)c.face_list[r] * 3 + ch;
    for (int k = 0; k < kM; ++k) c.surfaces[dst * kM + k] = v[k] = c.p[src * kM + k];
    if (c.s_info)
      for (int k = 0; k < kInfoSz; ++k) c.s_info[dst * kInfoSz + k] = c.info[src * kInfoSz + k];
    if (c.s_ret) c.s_ret[dst] = c.ret[src];
    if (c.s_covar)
      for (int k = 0; k < kM * kM; ++k) c.s_covar[dst * kM * kM + k] = c.covar[src * kM * kM + k];
    if (c.s_stats)
      for (int k = 0; k < kStatsSz; ++k) c.s_stats[dst * kStatsSz + k] = c.stats[src * kStatsSz + k];
    if (c.s_rank) c.s_rank[dst] = c.rank[src];
    if (c.s_count) c.s_count[dst] = c.nobs[src];
    if (c.s_lights) c.s_lights[dst] = c.lights[src];
  }
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = kCT / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) c.block_sums[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

#define MEANS_OK(call)                                                        \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", kWho, #call, hipGetErrorString(e_));   \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

bool take(DevBuf &b, size_t bytes, const char *what) { return take(b, bytes, what, kWho); }

// what the entry refuses before any HIP call
int capture_means_check(const CaptureFacesArgs &a) {
  return capture_args_check(kWho, a, kMeansMaxL, " (the weighted fit's size class; brdf_hip_fit_capture_faces_dev takes L <= 64)");
}

}  // namespace

int capture_means_run(const CaptureMeansArgs &ma) {
  const CaptureFacesArgs &a = ma.faces;
  if (capture_means_check(a) != 0) return kLmError;
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int L = a.L, nf = a.nf;
  if (a.avg) a.avg[0] = a.avg[1] = a.avg[2] = 0.0;
  if (a.n_pixels) *a.n_pixels = 0;
  if (a.n_faces) *a.n_faces = 0;

  // ---- compact, group, cosines (capture_group.h) ----
  CaptureGroup g;
  if (capture_group_run(kWho, a, g) != 0) return kLmError;
  if (g.S == 0) return 0;  // an empty capture: nothing is written but the pixel counts
  const long long F = g.F, T = g.S * L;
  if (g.max_pixels > kMeansMaxPixels) {
    set_error("%s(): a face has %lld pixels, more than the %lld whose sums of squares fit 64-bit integers", kWho, g.max_pixels, kMeansMaxPixels);
    return kLmError;
  }

  // ---- accumulate and pack ----
  const int fits = (int)(3 * F);
  const size_t words = (size_t)fits * L;
  DevBuf cnt, s1, s2, angles, x, w, within, p, lights, nobs;
  if (!take(cnt, sizeof(int) * words, "the lights' counts") || !take(s1, sizeof(long long) * words, "the lights' sums") ||
      !take(s2, sizeof(long long) * words, "the lights' sums of squares") || !take(angles, sizeof(double) * 3 * words, "the fits' planes") ||
      !take(x, sizeof(double) * words, "the fits' means") || !take(w, sizeof(double) * words, "the fits' weights") ||
      !take(within, sizeof(double) * (size_t)fits, "the fits' inner sums of squares") || !take(p, sizeof(double) * kM * (size_t)fits, "the fits' parameters") ||
      !take(lights, sizeof(int) * (size_t)fits, "the fits' light counts") || !take(nobs, sizeof(int) * (size_t)fits, "the fits' sample counts"))
    return kLmError;
  MEANS_OK(hipMemsetAsync(cnt.ptr, 0, sizeof(int) * words, stream));
  MEANS_OK(hipMemsetAsync(s1.ptr, 0, sizeof(long long) * words, stream));
  MEANS_OK(hipMemsetAsync(s2.ptr, 0, sizeof(long long) * words, stream));
  MeansCtx mc = {};
  mc.images = a.d_images;
  mc.L = L;
  mc.H = a.H;
  mc.W = a.W;
  mc.pixel_sorted = g.pixel_sorted.as<long long>();
  mc.face_sorted = g.face_sorted.as<unsigned>();
  mc.rank_of_face = g.rank_of_face.as<int>();
  mc.angles_f = g.angles_f.as<double>();
  mc.T = T;
  mc.F = (int)F;
  mc.v_min = a.v_min;
  mc.v_max = a.v_max;
  mc.cos_min = a.cos_min;
  mc.use1 = a.model != MODEL_PHONG;
  mc.use2 = a.model != MODEL_BLINN_PHONG;
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
  for (int k = 0; k < kM; ++k) mc.p0[k] = a.p0[k];
  const int ab = (int)((T + kCT - 1) / kCT), fb = (fits + kCT - 1) / kCT;
  hipLaunchKernelGGL(means_accumulate_kernel, dim3(ab), dim3(kCT), 0, stream, mc);
  hipLaunchKernelGGL(means_pack_kernel, dim3(fb), dim3(kCT), 0, stream, mc);
  MEANS_OK(hipGetLastError());

  // ---- fit and statistics: the weighted problem, n = L ----
  const bool want_stats = a.d_surface_covar || a.d_surface_stats || a.d_surface_rank;
  DevBuf info, ret, covar, stats, rank;
  if ((a.d_surface_info && !take(info, sizeof(double) * kInfoSz * (size_t)fits, "the fits' info")) ||
      (a.d_surface_ret && !take(ret, sizeof(int) * (size_t)fits, "the fits' ret")) ||
      (a.d_surface_covar && !take(covar, sizeof(double) * kM * kM * (size_t)fits, "the fits' covariances")) ||
      (a.d_surface_stats && !take(stats, sizeof(double) * kStatsSz * (size_t)fits, "the fits' statistics")) ||
      (a.d_surface_rank && !take(rank, sizeof(int) * (size_t)fits, "the fits' ranks")))
    return kLmError;
  const WeightedFitArgs wf = {{BRDF_METHOD_BC_DIF, a.model, angles.as<double>(), x.as<double>(), fits, L, p.as<double>(), a.lb, a.ub, a.itmax, a.opts,
                               info.as<double>(), ret.as<int>(), stream, lights.as<int>()},
                              w.as<double>()};
  if (weighted_fit_enqueue(wf, kWho) != 0) return kLmError;
  if (want_stats && L >= kM) {
    const WeightedStatsArgs ws = {{BRDF_METHOD_BC_DIF, a.model, angles.as<double>(), x.as<double>(), fits, L, p.as<double>(), a.opts, covar.as<double>(),
                                   stats.as<double>(), rank.as<int>(), nullptr, 0, stream, lights.as<int>()},
                                  w.as<double>(), within.as<double>(), nobs.as<int>()};
    if (weighted_stats_enqueue(ws, kWho) != 0) return kLmError;
  } else if (want_stats) {  // fewer than three lights: every fit is refused, there is nothing to take statistics of
    if (covar.ptr) MEANS_OK(hipMemsetAsync(covar.ptr, 0, sizeof(double) * kM * kM * (size_t)fits, stream));
    if (stats.ptr) MEANS_OK(hipMemsetAsync(stats.ptr, 0, sizeof(double) * kStatsSz * (size_t)fits, stream));
    if (rank.ptr) MEANS_OK(hipMemsetAsync(rank.ptr, 0, sizeof(int) * (size_t)fits, stream));
  }

  // ---- scatter ----
  const int sb = (fits + kCT - 1) / kCT;
  DevBuf sums;
  if (!take(sums, sizeof(double) * 3 * (size_t)sb, "the block sums")) return kLmError;
  const MeansScatterCtx sc = {(int)F, g.face_list.as<int>(), p.as<double>(), info.as<double>(), covar.as<double>(), stats.as<double>(), ret.as<int>(),
                              rank.as<int>(), nobs.as<int>(), lights.as<int>(), a.d_brdf_surfaces, a.d_surface_info, a.d_surface_covar, a.d_surface_stats,
                              a.d_surface_ret, a.d_surface_rank, a.d_surface_count, ma.d_surface_lights, sums.as<double>()};
  hipLaunchKernelGGL(means_scatter_kernel, dim3(sb), dim3(kCT), 0, stream, sc);
  MEANS_OK(hipGetLastError());
  std::vector<double> h_sums((size_t)3 * sb);
  MEANS_OK(hipMemcpyAsync(h_sums.data(), sums.ptr, sizeof(double) * 3 * sb, hipMemcpyDeviceToHost, stream));
  MEANS_OK(hipStreamSynchronize(stream));
  if (a.avg) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < sb; ++b)
      for (int k = 0; k < 3; ++k) t[k] += h_sums[(size_t)3 * b + k];
    for (int k = 0; k < 3; ++k) a.avg[k] = t[k] / ((double)nf * 3);
  }
  return 0;
}

}  // namespace brdf
