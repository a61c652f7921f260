// capture_materials.hip -- K materials per object, between one fit per face (capture_faces.hip) and one per object
// (capture_single_faces.hip):
//   brdf_hip_capture_face_residuals_dev  the carried faces' sums of squared residuals against M candidate materials, one read of a
//                                        chunk's samples per group of kMaterialGroup materials
//   brdf_hip_fit_capture_labelled_dev    one fit per (label, channel) over the samples of the faces that carry the label
//   brdf_hip_fit_capture_materials_dev   Lloyd's iteration around the two: assign every face to the material of least residual, refit
//                                        every material over its faces, until no label moves
// No fit or statistics kernel of its own: the labelled fits are ONE packed batch (packed_fit.h), rows channel * K + label.
//
// (compact, group and cosines are capture_group.hip's; the candidate reader, the channel compaction and the scan are capture_compact.h's;
// the face-major samples -- seg[c][F + 1] alone for the labelled fits, with the planes and measurements where residuals are taken --
// and the residuals' summation per material are capture_face_major.hip's, shared with capture_single_faces.hip)
//   label-major a stable sort of the carried faces by label (rocPRIM's radix sort: K has no bound a per-block histogram could hold),
//               one scan of the faces' sample counts in that order, channel after channel -- a fit's offset is the prefix at its first
//               face, a face's samples stay contiguous and in order -- and a placing pass over the candidates.  Integers only.
// Every candidate pass evaluates the same rule on the same bytes, so the places of the later passes are the counts of pass 0.  Phases
// are ordered by kernel boundaries; the only atomic is the integer count of the faces whose label changed.
#include <algorithm>
#include <climits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/brdf_levmar.h"
#include "capture_face_major.h"
#include "capture_materials.h"
#include "fit_stats.h"
#include "packed_fit.h"

namespace brdf {

namespace {

constexpr const char *kWhoResiduals = "brdf_hip_capture_face_residuals_dev", *kWhoLabelled = "brdf_hip_fit_capture_labelled_dev",
                     *kWhoMaterials = "brdf_hip_fit_capture_materials_dev";

// ---- label-major ----------------------------------------------------------------------------------------------------------------
// carried face r: its label (-1 outside [0, K)), the sort's key (K for those: behind every label) and its rank as the sort's value
__global__ __launch_bounds__(kCT) void label_key_kernel(const int *__restrict__ face_list, const int *__restrict__ face_label, int F, int K,
                                                        int *__restrict__ label_r, unsigned *__restrict__ key, int *__restrict__ rank) {
  const long long r = (long long)blockIdx.x * kCT + threadIdx.x;
  if (r >= F) return;
  const int l = face_label[face_list[r]];
  const bool ok = l >= 0 && l < K;
  label_r[r] = ok ? l : -1;
  key[r] = ok ? (unsigned)l : (unsigned)K;
  rank[r] = (int)r;
}

// One workgroup over the carried faces in label order (order[j]: the rank of the j-th), channel after channel: pos[c][j] = the samples
// in front of the j-th face's in the batch, pos[c][F] the channel's end; dst[c][rank] = the same by rank, -1 where the face has no label
__global__ __launch_bounds__(kCT) void label_scan_kernel(const long long *__restrict__ seg_all, const unsigned *__restrict__ key_sorted,
                                                         const int *__restrict__ order, int F, int K, long long *__restrict__ pos,
                                                         long long *__restrict__ dst) {
  __shared__ long long part[kCT];
  __shared__ long long base;
  const int t = threadIdx.x;
  const long long per = ((long long)F + kCT - 1) / kCT;
  const long long j0 = t * per < F ? t * per : F, j1 = j0 + per < F ? j0 + per : F;
  if (t == 0) base = 0;
  __syncthreads();
  for (int ch = 0; ch < 3; ++ch) {
    const long long *seg = seg_all + (size_t)ch * (F + 1);
    long long sum = 0;
    for (long long j = j0; j < j1; ++j)
      if (key_sorted[j] < (unsigned)K) sum += seg[order[j] + 1] - seg[order[j]];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
      long long run = base;
      for (int i = 0; i < kCT; ++i) {
        const long long v = part[i];
        part[i] = run;
        run += v;
      }
      pos[(size_t)ch * (F + 1) + F] = run;
      base = run;
    }
    __syncthreads();
    sum = part[t];
    for (long long j = j0; j < j1; ++j) {
      const int r = order[j];
      const bool has = key_sorted[j] < (unsigned)K;
      pos[(size_t)ch * (F + 1) + j] = sum;
      dst[(size_t)ch * F + r] = has ? sum : -1;
      if (has) sum += seg[r + 1] - seg[r];
    }
    __syncthreads();
  }
}

// Thread k <= K: label k's faces are [lower(k), lower(k + 1)) of the label order, fit (c, k) starts at pos[c][lower(k)]
__global__ __launch_bounds__(kCT) void label_offsets_kernel(const unsigned *__restrict__ key_sorted, const long long *__restrict__ pos, int F, int K,
                                                            long long *__restrict__ offsets, int *__restrict__ label_faces) {
  const long long k = (long long)blockIdx.x * kCT + threadIdx.x;
  if (k > K) return;
  if (k == K) {
    offsets[(size_t)3 * K] = pos[(size_t)2 * (F + 1) + F];
    return;
  }
  long long bound[2];
  for (int e = 0; e < 2; ++e) {  // the first j with key_sorted[j] >= k + e
    long long lo = 0, hi = F;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (key_sorted[mid] < (unsigned)(k + e)) lo = mid + 1; else hi = mid;
    }
    bound[e] = lo;
  }
  if (label_faces) label_faces[k] = (int)(bound[1] - bound[0]);
  for (int ch = 0; ch < 3; ++ch) offsets[(size_t)ch * K + k] = pos[(size_t)ch * (F + 1) + bound[0]];
}

struct LabelPlaceCtx {
  CandidateCtx cand;
  const long long *block_off;  // [blocks][3]: face_pack_kernel's
  const long long *seg;        // [3][F + 1]
  const long long *dst;        // [3][F]
  const int *label_r;          // [F]
  const long long *offsets;    // [3 K + 1]
  int K;
  double *angles, *x;  // the packed batch
};

// Candidate t once more: a valid one of a labelled face goes where its face's samples start in the batch, plus its place in the face
__global__ __launch_bounds__(kCT) void label_place_kernel(LabelPlaceCtx c) {
  __shared__ int wave_cnt[kWaves][3];
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const Candidate k = read_candidate(c.cand, t);
  ChannelPlaces pl = {wave_cnt};
  pl.place(k.valid);
  if (t >= c.cand.T) return;
  const int label = c.label_r[k.r];
  if (label < 0) return;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if (!k.valid[ch]) continue;
    const long long at = pl.at(ch, c.block_off[(size_t)blockIdx.x * 3 + ch]);
    const long long d = c.dst[(size_t)ch * c.cand.F + k.r] + (at - c.seg[(size_t)ch * (c.cand.F + 1) + k.r]);
    const size_t fit = (size_t)ch * c.K + label;
    const long long o = c.offsets[fit], n = c.offsets[fit + 1] - o;  // (o <= d < o + n: the scan counted this sample)
    c.x[d] = k.v[ch] / 255.0;
    double *dp = c.angles + 3 * o + (d - o);
    dp[0] = k.c0;
    dp[n] = k.c1;
    dp[2 * n] = k.c2;
  }
}

// the batch's rows channel * K + label <-> the caller's rows [label][channel]
struct LabelRowsCtx {
  int K;
  const long long *offsets;
  double *p;  // [3 K][3]
  const double *info, *covar, *stats;
  const int *ret, *rank;
  double *materials, *o_info, *o_covar, *o_stats;
  int *o_ret, *o_rank, *o_count;
};
template <bool IN>
__global__ __launch_bounds__(kCT) void label_rows_kernel(LabelRowsCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= 3LL * c.K) return;
  const long long ch = s / c.K, k = s - ch * c.K;
  const size_t row = (size_t)k * 3 + ch;
  if (IN) {
    for (int j = 0; j < kM; ++j) c.p[s * kM + j] = c.materials[row * kM + j];
    return;
  }
  if (c.materials)
    for (int j = 0; j < kM; ++j) c.materials[row * kM + j] = c.p[s * kM + j];
  if (c.o_info && c.info)
    for (int j = 0; j < kInfoSz; ++j) c.o_info[row * kInfoSz + j] = c.info[s * kInfoSz + j];
  if (c.o_covar && c.covar)
    for (int j = 0; j < kM * kM; ++j) c.o_covar[row * kM * kM + j] = c.covar[s * kM * kM + j];
  if (c.o_stats && c.stats)
    for (int j = 0; j < kStatsSz; ++j) c.o_stats[row * kStatsSz + j] = c.stats[s * kStatsSz + j];
  if (c.o_ret && c.ret) c.o_ret[row] = c.ret[s];
  if (c.o_rank && c.rank) c.o_rank[row] = c.rank[s];
  if (c.o_count) c.o_count[row] = (int)(c.offsets[s + 1] - c.offsets[s]);
}

// ---- the loop's own kernels ----------------------------------------------------------------------------------------------------
// One thread per carried face: cost[k] = (s[k][0] + s[k][1]) + s[k][2], a cost that is not finite is +inf, the least cost wins, the
// lowest k on a tie; every cost +inf: the label stays.  *changed counts the faces whose label moved (integer atomic).
__global__ __launch_bounds__(kCT) void assign_kernel(const int *__restrict__ face_list, int F, int K, const double *__restrict__ sumsq_r,
                                                     int *__restrict__ face_label, int *__restrict__ changed) {
  const long long r = (long long)blockIdx.x * kCT + threadIdx.x;
  if (r >= F) return;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  int best = -1;
  double least = inf;
  for (int k = 0; k < K; ++k) {
    const double *s = sumsq_r + ((size_t)r * K + k) * 3;
    double cost = (s[0] + s[1]) + s[2];
    if (!(fabs(cost) < inf)) cost = inf;
    if (cost < least) {
      least = cost;
      best = k;
    }
  }
  const int f = face_list[r];
  if (best >= 0 && best != face_label[f]) {
    face_label[f] = best;
    atomicAdd(changed, 1);
  }
}

// face_sumsq[f][c] = the face's residual against its own material; +inf where it has none
__global__ __launch_bounds__(kCT) void own_residual_kernel(const int *__restrict__ face_list, int F, int K, const double *__restrict__ sumsq_r,
                                                           const int *__restrict__ face_label, double *__restrict__ face_sumsq) {
  const long long r = (long long)blockIdx.x * kCT + threadIdx.x;
  if (r >= F) return;
  const int f = face_list[r], l = face_label[f];
  for (int ch = 0; ch < 3; ++ch)
    face_sumsq[(size_t)f * 3 + ch] = (l >= 0 && l < K) ? sumsq_r[((size_t)r * K + l) * 3 + ch] : __longlong_as_double(0x7ff0000000000000LL);
}

// ---- host: the three phases -----------------------------------------------------------------------------------------------------
struct Labelled {
  int K = 0, fits = 0;
  unsigned end_bit = 1;
  size_t tmp_bytes = 0;
  DevBuf key, rank, key_sorted, order, sort_tmp, label_r, pos, dst, offsets, angles, x, p, info, ret, covar, stats, srank;
};

// what a regrouping and its fits need: 24 bytes per carried face and channel, 32 bytes per valid sample, the batch's rows
int labelled_prepare(const char *who, const FaceMajor &fm, const CaptureLabelledArgs &a, Labelled &lb) {
  const size_t F = (size_t)fm.F, fits = 3 * (size_t)a.K;
  lb.K = a.K;
  lb.fits = (int)fits;
  while ((1LL << lb.end_bit) <= a.K) ++lb.end_bit;  // the keys reach K
  const size_t total = std::max<size_t>((size_t)(fm.K[0] + fm.K[1] + fm.K[2]), 1);  // (at most: unlabelled faces leave theirs out)
  if (!take(lb.key, sizeof(unsigned) * F, "the faces' keys", who) || !take(lb.rank, sizeof(int) * F, "the faces' ranks", who) ||
      !take(lb.key_sorted, sizeof(unsigned) * F, "the sorted keys", who) || !take(lb.order, sizeof(int) * F, "the faces by label", who) ||
      !take(lb.label_r, sizeof(int) * F, "the carried faces' labels", who) || !take(lb.pos, sizeof(long long) * 3 * (F + 1), "the faces' places", who) ||
      !take(lb.dst, sizeof(long long) * 3 * F, "the faces' places by rank", who) || !take(lb.offsets, sizeof(long long) * (fits + 1), "the fits' offsets", who) ||
      !take(lb.angles, sizeof(double) * 3 * total, "the packed planes", who) || !take(lb.x, sizeof(double) * total, "the packed measurements", who) ||
      !take(lb.p, sizeof(double) * kM * fits, "the fits' parameters", who) || (a.d_info && !take(lb.info, sizeof(double) * kInfoSz * fits, "the fits' info", who)) ||
      (a.d_ret && !take(lb.ret, sizeof(int) * fits, "the fits' ret", who)) ||
      (a.d_covar && !take(lb.covar, sizeof(double) * kM * kM * fits, "the fits' covariances", who)) ||
      (a.d_stats && !take(lb.stats, sizeof(double) * kStatsSz * fits, "the fits' statistics", who)) ||
      (a.d_rank && !take(lb.srank, sizeof(int) * fits, "the fits' ranks", who)))
    return kLmError;
  CAPTURE_OK(who, rocprim::radix_sort_pairs(nullptr, lb.tmp_bytes, lb.key.as<unsigned>(), lb.key_sorted.as<unsigned>(), lb.rank.as<int>(), lb.order.as<int>(), F,
                                            0u, lb.end_bit, a.g.cap.stream));
  if (!take(lb.sort_tmp, std::max<size_t>(lb.tmp_bytes, 1), "the sort of the faces by label", who)) return kLmError;
  return 0;
}

LabelRowsCtx label_rows(const CaptureLabelledArgs &a, const Labelled &lb) {
  LabelRowsCtx rc = {};
  rc.K = lb.K;
  rc.offsets = lb.offsets.as<long long>();
  rc.p = lb.p.as<double>();
  return rc;
}

// the batch of the labels a.d_face_label holds, from the materials a.d_materials holds: enqueued, no wait
int labelled_regroup(const char *who, const FaceMajor &fm, const CaptureLabelledArgs &a, Labelled &lb) {
  hipStream_t stream = a.g.cap.stream;
  const int F = (int)fm.F;
  hipLaunchKernelGGL(label_key_kernel, dim3(blocks_of(F)), dim3(kCT), 0, stream, fm.g.face_list.as<int>(), a.d_face_label, F, lb.K, lb.label_r.as<int>(),
                     lb.key.as<unsigned>(), lb.rank.as<int>());
  CAPTURE_OK(who, hipGetLastError());
  size_t tmp = lb.tmp_bytes;
  CAPTURE_OK(who, rocprim::radix_sort_pairs(lb.sort_tmp.ptr, tmp, lb.key.as<unsigned>(), lb.key_sorted.as<unsigned>(), lb.rank.as<int>(), lb.order.as<int>(),
                                            (size_t)F, 0u, lb.end_bit, stream));
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kCT), 0, stream, fm.seg.as<long long>(), lb.key_sorted.as<unsigned>(), lb.order.as<int>(), F, lb.K,
                     lb.pos.as<long long>(), lb.dst.as<long long>());
  hipLaunchKernelGGL(label_offsets_kernel, dim3(blocks_of((long long)lb.K + 1)), dim3(kCT), 0, stream, lb.key_sorted.as<unsigned>(), lb.pos.as<long long>(), F,
                     lb.K, lb.offsets.as<long long>(), a.d_label_faces);
  LabelPlaceCtx pc = {};
  pc.cand = fm.pc.cand;
  pc.block_off = fm.pack_off.as<long long>();
  pc.seg = fm.seg.as<long long>();
  pc.dst = lb.dst.as<long long>();
  pc.label_r = lb.label_r.as<int>();
  pc.offsets = lb.offsets.as<long long>();
  pc.K = lb.K;
  pc.angles = lb.angles.as<double>();
  pc.x = lb.x.as<double>();
  hipLaunchKernelGGL(label_place_kernel, dim3(fm.pb), dim3(kCT), 0, stream, pc);
  LabelRowsCtx rc = label_rows(a, lb);
  rc.materials = a.d_materials;
  hipLaunchKernelGGL(label_rows_kernel<true>, dim3(blocks_of(3LL * lb.K)), dim3(kCT), 0, stream, rc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

// packed_fit_run on the batch; materials, info, ret and count to the caller's rows
int labelled_fit(const char *who, const CaptureLabelledArgs &a, Labelled &lb) {
  const CaptureArgs &cap = a.g.cap;
  const PackedFitArgs pf = {BRDF_METHOD_BC_DIF, cap.model, lb.angles.as<double>(), lb.x.as<double>(), lb.offsets.as<long long>(), lb.fits, lb.p.as<double>(),
                            cap.lb, cap.ub, cap.itmax, cap.opts, lb.info.as<double>(), lb.ret.as<int>(), a.workspace_bytes, cap.stream};
  if (packed_fit_run(pf, who) != 0) return kLmError;
  LabelRowsCtx rc = label_rows(a, lb);
  rc.materials = a.d_materials;
  rc.info = lb.info.as<double>();
  rc.ret = lb.ret.as<int>();
  rc.o_info = a.d_info;
  rc.o_ret = a.d_ret;
  rc.o_count = a.d_count;
  hipLaunchKernelGGL(label_rows_kernel<false>, dim3(blocks_of(3LL * lb.K)), dim3(kCT), 0, cap.stream, rc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

// packed_stats_run on the batch at its fitted points, where a statistics map is asked for
int labelled_stats(const char *who, const CaptureLabelledArgs &a, Labelled &lb) {
  if (!a.d_covar && !a.d_stats && !a.d_rank) return 0;
  const CaptureArgs &cap = a.g.cap;
  const PackedStatsArgs ps = {BRDF_METHOD_BC_DIF, cap.model, lb.angles.as<double>(), lb.x.as<double>(), lb.offsets.as<long long>(), lb.fits, lb.p.as<double>(),
                              cap.opts, lb.covar.as<double>(), lb.stats.as<double>(), lb.srank.as<int>(), a.workspace_bytes, cap.stream};
  if (packed_stats_run(ps, who) != 0) return kLmError;
  LabelRowsCtx rc = label_rows(a, lb);
  rc.covar = lb.covar.as<double>();
  rc.stats = lb.stats.as<double>();
  rc.rank = lb.srank.as<int>();
  rc.o_covar = a.d_covar;
  rc.o_stats = a.d_stats;
  rc.o_rank = a.d_rank;
  hipLaunchKernelGGL(label_rows_kernel<false>, dim3(blocks_of(3LL * lb.K)), dim3(kCT), 0, cap.stream, rc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

// the maps of fits that did not run: levmar's refusal in every row (ret LM_ERROR, zero info, rank 0), zero statistics and counts
int refuse_rows(const char *who, const CaptureLabelledArgs &a) {
  hipStream_t stream = a.g.cap.stream;
  const size_t rows = 3 * (size_t)a.K;
  if (a.d_info) CAPTURE_OK(who, hipMemsetAsync(a.d_info, 0, sizeof(double) * kInfoSz * rows, stream));
  if (a.d_ret) CAPTURE_OK(who, hipMemsetAsync(a.d_ret, 0xff, sizeof(int) * rows, stream));
  if (a.d_covar) CAPTURE_OK(who, hipMemsetAsync(a.d_covar, 0, sizeof(double) * kM * kM * rows, stream));
  if (a.d_stats) CAPTURE_OK(who, hipMemsetAsync(a.d_stats, 0, sizeof(double) * kStatsSz * rows, stream));
  if (a.d_rank) CAPTURE_OK(who, hipMemsetAsync(a.d_rank, 0, sizeof(int) * rows, stream));
  if (a.d_count) CAPTURE_OK(who, hipMemsetAsync(a.d_count, 0, sizeof(int) * rows, stream));
  if (a.d_label_faces) CAPTURE_OK(who, hipMemsetAsync(a.d_label_faces, 0, sizeof(int) * (size_t)a.K, stream));
  return 0;
}

const double kNoStart[kM] = {0.0, 0.0, 0.0};  // capture_args_check wants a p0; these entries read none

// what the labelled entries refuse besides capture_args_check's list
int labelled_args_check(const char *who, const CaptureLabelledArgs &a) {
  if (!a.d_face_label || !a.d_materials) {
    set_error("%s(): null face_label or materials", who);
    return kLmError;
  }
  if (a.K < 1 || a.K > INT_MAX / 3 || a.workspace_bytes < 0) {
    set_error("%s(): K = %d, workspace_bytes = %lld: need K >= 1, 3 K <= INT_MAX and workspace_bytes >= 0", who, a.K, a.workspace_bytes);
    return kLmError;
  }
  return 0;
}

}  // namespace

int capture_face_residuals_run(const CaptureResidualsArgs &ra) {
  const char *who = kWhoResiduals;
  CaptureGrouped ga = ra.g;
  ga.cap.p0 = kNoStart;
  ga.cap.lb = ga.cap.ub = nullptr;
  if (capture_args_check(who, ga, ra.d_materials, "materials") != 0) return kLmError;  // before any HIP call
  if (ra.M < 1 || ra.M > INT_MAX / 3) {
    set_error("%s(): M = %d: need M >= 1 and 3 M <= INT_MAX", who, ra.M);
    return kLmError;
  }
  (void)hipGetLastError();
  hipStream_t stream = ga.cap.stream;
  if (ga.n_pixels) *ga.n_pixels = 0;
  if (ga.n_faces) *ga.n_faces = 0;
  FaceMajor fm;
  if (face_major_run(who, ga, fm, true) != 0) return kLmError;
  if (fm.g.S == 0 || (!ra.d_face_sumsq && !ra.d_face_count)) return 0;  // an empty capture: nothing is written but the pixel counts
  Residuals rs;
  if (residuals_prepare(who, fm, ra.M, stream, rs) != 0 ||
      residuals_enqueue(who, fm, rs, ga.cap.model, ra.d_materials, stream, ra.d_face_sumsq, false, ra.d_face_count) != 0)
    return kLmError;
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  return 0;
}

int capture_labelled_run(const CaptureLabelledArgs &la) {
  const char *who = kWhoLabelled;
  CaptureLabelledArgs a = la;
  a.g.cap.p0 = kNoStart;
  if (labelled_args_check(who, a) != 0 || capture_args_check(who, a.g, a.d_materials, "materials") != 0) return kLmError;  // before any HIP call
  (void)hipGetLastError();
  hipStream_t stream = a.g.cap.stream;
  if (a.g.n_pixels) *a.g.n_pixels = 0;
  if (a.g.n_faces) *a.g.n_faces = 0;
  FaceMajor fm;
  if (face_major_run(who, a.g, fm, false) != 0) return kLmError;
  if (fm.g.S == 0) {  // an empty capture: every fit is refused, the materials stay
    if (refuse_rows(who, a) != 0) return kLmError;
    CAPTURE_OK(who, hipStreamSynchronize(stream));
    return 0;
  }
  Labelled lb;
  if (labelled_prepare(who, fm, a, lb) != 0 || labelled_regroup(who, fm, a, lb) != 0 || labelled_fit(who, a, lb) != 0 || labelled_stats(who, a, lb) != 0)
    return kLmError;
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  return 0;
}

int capture_materials_run(const CaptureMaterialsArgs &ma) {
  const char *who = kWhoMaterials;
  CaptureLabelledArgs a = ma.fit;
  a.g.cap.p0 = kNoStart;
  if (labelled_args_check(who, a) != 0) return kLmError;  // before any HIP call
  if (ma.rounds < 0 || ma.rounds > kMaterialRoundsMax) {
    set_error("%s(): rounds = %d: need 0 <= rounds <= %d", who, ma.rounds, kMaterialRoundsMax);
    return kLmError;
  }
  if (capture_args_check(who, a.g, a.d_materials, "materials") != 0) return kLmError;
  (void)hipGetLastError();
  hipStream_t stream = a.g.cap.stream;
  const int K = a.K;
  if (a.g.n_pixels) *a.g.n_pixels = 0;
  if (a.g.n_faces) *a.g.n_faces = 0;
  if (ma.rounds_used) *ma.rounds_used = 0;
  if (ma.settled) *ma.settled = 0;
  if (ma.changed)
    for (int i = 0; i <= ma.rounds; ++i) ma.changed[i] = -1;
  CAPTURE_OK(who, hipMemsetAsync(a.d_face_label, 0xff, sizeof(int) * (size_t)a.g.cap.nf, stream));  // every label -1
  if (refuse_rows(who, a) != 0) return kLmError;                                                       // until a refit ran
  FaceMajor fm;
  if (face_major_run(who, a.g, fm, true) != 0) return kLmError;
  if (fm.g.S == 0) {  // an empty capture: no face to assign
    if (ma.changed) ma.changed[0] = 0;
    if (ma.settled) *ma.settled = 1;
    CAPTURE_OK(who, hipStreamSynchronize(stream));
    return 0;
  }
  const long long F = fm.F;
  Residuals rs;
  Labelled lb;
  DevBuf sumsq_r, changed;  // [F][K][3]; one int
  if (residuals_prepare(who, fm, K, stream, rs) != 0 || !take(sumsq_r, sizeof(double) * 3 * (size_t)F * (size_t)K, "the faces' residuals", who) ||
      !take(changed, sizeof(int), "the changed labels' count", who))
    return kLmError;
  // the statistics wait for the last refit: the refits themselves take none
  CaptureLabelledArgs fit_only = a;
  fit_only.d_covar = fit_only.d_stats = nullptr;
  fit_only.d_rank = nullptr;
  int refits = 0, assignments = 0;
  bool settled = false;
  for (;;) {
    // ---- assign ----
    int n = 0;
    CAPTURE_OK(who, hipMemsetAsync(changed.ptr, 0, sizeof(int), stream));
    if (residuals_enqueue(who, fm, rs, a.g.cap.model, a.d_materials, stream, sumsq_r.as<double>(), true, nullptr) != 0) return kLmError;
    hipLaunchKernelGGL(assign_kernel, dim3(blocks_of(F)), dim3(kCT), 0, stream, fm.g.face_list.as<int>(), (int)F, K, sumsq_r.as<double>(), a.d_face_label,
                       changed.as<int>());
    CAPTURE_OK(who, hipGetLastError());
    CAPTURE_OK(who, hipMemcpyAsync(&n, changed.ptr, sizeof n, hipMemcpyDeviceToHost, stream));
    CAPTURE_OK(who, hipStreamSynchronize(stream));  // the round's one wait besides the packed call's
    if (ma.changed) ma.changed[assignments] = n;
    ++assignments;
    // ---- settle or stop ----
    if (n == 0) {
      settled = true;
      break;
    }
    if (refits == ma.rounds) break;
    // ---- refit ----
    if (refits == 0 && labelled_prepare(who, fm, a, lb) != 0) return kLmError;
    if (labelled_regroup(who, fm, fit_only, lb) != 0 || labelled_fit(who, fit_only, lb) != 0) return kLmError;
    if (++refits == ma.rounds) break;  // the labels are not assigned again: the materials are the fits on the returned labels
  }
  if (refits > 0 && labelled_stats(who, a, lb) != 0) return kLmError;  // (the batch is still the last refit's)
  // ---- the returned materials' residuals ----
  if (ma.d_face_sumsq || ma.d_face_count) {
    if (residuals_enqueue(who, fm, rs, a.g.cap.model, a.d_materials, stream, ma.d_face_sumsq ? sumsq_r.as<double>() : nullptr, true, ma.d_face_count) != 0)
      return kLmError;
    if (ma.d_face_sumsq)
      hipLaunchKernelGGL(own_residual_kernel, dim3(blocks_of(F)), dim3(kCT), 0, stream, fm.g.face_list.as<int>(), (int)F, K, sumsq_r.as<double>(),
                         a.d_face_label, ma.d_face_sumsq);
    CAPTURE_OK(who, hipGetLastError());
  }
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  if (ma.rounds_used) *ma.rounds_used = refits;
  if (ma.settled) *ma.settled = settled ? 1 : 0;
  return 0;
}

}  // namespace brdf
