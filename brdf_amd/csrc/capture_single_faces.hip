// capture_single_faces.hip -- brdf_hip_fit_capture_single_faces_dev: ONE fit per colour channel for the whole object over the valid
// samples of EVERY pixel of every carried face, where capture_fit.hip's single-BRDF fit takes each face's last pixel and knows no
// validity rule; and, per carried face and channel, the sum of squared residuals against that one fit: where on the object the
// one-material assumption fails.  No kernel of its own: capture_face_major.hip packs and takes the residuals, stream_fit_run fits,
// fit_stats.hip takes the statistics.
//
// (compact, group and cosines are capture_group.hip's, shared with capture_faces.hip and capture_means.hip)
//   pack      face_major_run with the data (capture_face_major.hip, shared with capture_materials.hip): the single-fit layout --
//             planes [3][K_c], x [K_c] per channel -- and where a face's samples start in the channel, seg[c][F + 1]
//   fit       stream_fit_run (dlevmar_bc_dif) per channel with K_c >= 3; fit_stats_enqueue at the fitted point
//   residuals residuals_prepare / residuals_enqueue (capture_face_major.hip) at M = 1: the three fitted points, [3][3], are a table of
//             ONE material.  A face's value depends on its samples, their order and p only; no float atomics.
#include <algorithm>
#include <string>

#include "../../include/brdf_levmar.h"
#include "capture_face_major.h"
#include "fit_stats.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_single_faces_dev";

// levmar's n < m refusal of channel c: ret = LM_ERROR, zero info, p0
void refuse_channel(const CaptureSingleFacesArgs &sa, int c) {
  for (int k = 0; k < kM; ++k) sa.single_brdf[c * kM + k] = sa.g.cap.p0[k];
  if (sa.info)
    for (int k = 0; k < kInfoSz; ++k) sa.info[c * kInfoSz + k] = 0.0;
  if (sa.ret) sa.ret[c] = kLmError;
}

}  // namespace

int capture_single_faces_run(const CaptureSingleFacesArgs &sa) {
  if (capture_args_check(kWho, sa.g, sa.single_brdf, "single_brdf") != 0) return kLmError;  // before any HIP call
  const CaptureArgs &a = sa.g.cap;
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  if (sa.g.n_pixels) *sa.g.n_pixels = 0;
  if (sa.g.n_faces) *sa.g.n_faces = 0;
  if (sa.count) sa.count[0] = sa.count[1] = sa.count[2] = 0;
  const bool want_stats = sa.covar || sa.stats || sa.rank;
  const bool want_faces = sa.d_face_sumsq || sa.d_face_count;

  // ---- compact, group, cosines; count, scan, place: 32 bytes per valid sample (capture_face_major.hip) ----
  FaceMajor fm;
  if (face_major_run(kWho, sa.g, fm, true) != 0) return kLmError;
  if (fm.g.S == 0) {  // an empty capture: every channel is refused, nothing is written on the device but the pixel counts
    for (int c = 0; c < 3; ++c) refuse_channel(sa, c);
    if (sa.covar) std::fill(sa.covar, sa.covar + 3 * kM * kM, 0.0);  // (the ragged statistics of no sample)
    if (sa.stats) std::fill(sa.stats, sa.stats + 3 * kStatsSz, 0.0);
    if (sa.rank) sa.rank[0] = sa.rank[1] = sa.rank[2] = 0;
    return 3;
  }
  const FacePackCtx &pc = fm.pc;
  const long long *K = fm.K;
  if (sa.count)
    for (int c = 0; c < 3; ++c) sa.count[c] = K[c];

  // ---- fit: "do the calculation once for each color-channel", brdfdata.cpp:1161, one dlevmar_bc_dif (:1058) each ----
  int failed = 0;
  double p3[3 * kM];
  for (int c = 0; c < 3; ++c) {
    double *p = p3 + c * kM;
    for (int k = 0; k < kM; ++k) p[k] = a.p0[k];
    if (K[c] < kM) {  // lm_core.c:502-505, lmbc_core.c:440-443
      refuse_channel(sa, c);
      ++failed;
      continue;
    }
    double info[kInfoSz] = {0.0};
    const int ret = stream_fit_run(stream_fit_args({kBcMachine, false}, a.model, pc.ang[c], pc.x[c], (int)K[c], p, a.lb, a.ub, nullptr, a.itmax, a.opts,
                                                   info, nullptr, stream));
    if (ret < 0 && info[6] == 0.0) {  // no stop reason: not levmar's failure but the call's
      const std::string why = get_error();
      set_error("%s(): the fit of channel %d (%lld samples) could not run: %s", kWho, c, K[c], why.c_str());
      return kLmError;
    }
    for (int k = 0; k < kM; ++k) sa.single_brdf[c * kM + k] = p[k];
    if (sa.info)
      for (int k = 0; k < kInfoSz; ++k) sa.info[c * kInfoSz + k] = info[k];
    if (sa.ret) sa.ret[c] = ret;
    failed += ret < 0;
  }

  // ---- the fitted points on the device, [3][3]: the statistics' p and the residuals' table of ONE material ----
  const int h_cnt[3] = {(int)K[0], (int)K[1], (int)K[2]};  // (read by a copy the stream may still hold: lives until the last wait)
  DevBuf small;  // p [3][3]; for the statistics covar [3][9], stats [3][kStatsSz], three staged rows of 12 doubles; rank [3], counts [3]
  constexpr int kSmallD = 3 * kM + 3 * kM * kM + 3 * kStatsSz + 3 * 12;
  const size_t small_bytes = want_stats ? sizeof(double) * kSmallD + sizeof(int) * 6 : sizeof p3;
  double *d_p = nullptr;
  if (want_stats || want_faces) {
    if (!take(small, small_bytes, "the channels' statistics", kWho)) return kLmError;  // (the fitted points alone for the face maps)
    d_p = small.as<double>();
    CAPTURE_OK(kWho, hipMemsetAsync(small.ptr, 0, small_bytes, stream));
    CAPTURE_OK(kWho, hipMemcpyAsync(d_p, p3, sizeof p3, hipMemcpyHostToDevice, stream));
  }

  // ---- statistics at the fitted points: the uniform pass at n = K_c; below 3 samples the ragged one on a row of stride 3 ----
  if (want_stats) {
    double *d_covar = d_p + 3 * kM, *d_stats = d_covar + 3 * kM * kM, *d_stage = d_stats + 3 * kStatsSz;
    int *d_rank = reinterpret_cast<int *>(d_stage + 3 * 12), *d_cnt = d_rank + 3;
    CAPTURE_OK(kWho, hipMemcpyAsync(d_cnt, h_cnt, sizeof h_cnt, hipMemcpyHostToDevice, stream));
    for (int c = 0; c < 3; ++c) {
      FitStatsArgs f = {BRDF_METHOD_BC_DIF, a.model, pc.ang[c], pc.x[c], 1, (int)K[c], d_p + c * kM, a.opts, d_covar + c * kM * kM, d_stats + c * kStatsSz,
                        d_rank + c, nullptr, 0, stream, nullptr};
      if (K[c] < kM) {
        double *row = d_stage + c * 12;  // planes [3][3], x [3]: the channel's K_c samples at the front of each
        for (int k = 0; k < 3 && K[c] > 0; ++k)
          CAPTURE_OK(kWho, hipMemcpyAsync(row + 3 * k, pc.ang[c] + k * K[c], sizeof(double) * K[c], hipMemcpyDeviceToDevice, stream));
        if (K[c] > 0) CAPTURE_OK(kWho, hipMemcpyAsync(row + 9, pc.x[c], sizeof(double) * K[c], hipMemcpyDeviceToDevice, stream));
        f.d_angles = row;
        f.d_x = row + 9;
        f.n = kM;
        f.d_counts = d_cnt + c;
      }
      if (fit_stats_enqueue(f, kWho) != 0) return kLmError;
    }
    if (sa.covar) CAPTURE_OK(kWho, hipMemcpyAsync(sa.covar, d_covar, sizeof(double) * 3 * kM * kM, hipMemcpyDeviceToHost, stream));
    if (sa.stats) CAPTURE_OK(kWho, hipMemcpyAsync(sa.stats, d_stats, sizeof(double) * 3 * kStatsSz, hipMemcpyDeviceToHost, stream));
    if (sa.rank) CAPTURE_OK(kWho, hipMemcpyAsync(sa.rank, d_rank, sizeof(int) * 3, hipMemcpyDeviceToHost, stream));
  }

  // ---- residuals of every carried face against its channel's fit (capture_face_major.hip, M = 1) ----
  Residuals rs;
  if (want_faces && (residuals_prepare(kWho, fm, 1, stream, rs) != 0 ||
                     residuals_enqueue(kWho, fm, rs, a.model, d_p, stream, sa.d_face_sumsq, false, sa.d_face_count) != 0))
    return kLmError;
  CAPTURE_OK(kWho, hipStreamSynchronize(stream));
  return failed;
}

}  // namespace brdf
