// capture_single_faces.hip -- brdf_hip_fit_capture_single_faces_dev: ONE fit per colour channel for the whole object over the valid
// samples of EVERY pixel of every carried face, where capture_fit.hip's single-BRDF fit takes each face's last pixel and knows no
// validity rule; and, per carried face and channel, the sum of squared residuals against that one fit: where on the object the
// one-material assumption fails.  No fit or statistics kernel of its own: stream_fit_run fits, fit_stats.hip takes the statistics.
//
// (compact, group and cosines are capture_group.hip's, shared with capture_faces.hip and capture_means.hip; the candidate reader, the
// channel compaction and the scan are capture_compact.h's, shared with capture_faces.hip)
//   pack      the candidates of a channel are ONE flat array, t = sorted pixel * L + light (capture_faces.hip's), and a channel's
//             samples are one stream compaction of it: ballot + popcount and block counts (pass 0), one scan, place (pass 1).  The
//             channel totals K_c are the scan's, so ONE placing pass writes the single-fit layout -- planes [3][K_c], x [K_c] --
//             and, at a face's first candidate, where the face's samples start in the channel: seg[c][F + 1].
//   fit       stream_fit_run (dlevmar_bc_dif) per channel with K_c >= 3; fit_stats_enqueue at the fitted point
//   residuals a face's samples are cut into chunks of kRC counted from the face's OWN first sample; one wavefront per chunk: a lane
//             adds its samples in ascending order, one DPP tree over the lanes; one thread per face adds the chunks' partial sums in
//             ascending order.  A face's value depends on its samples, their order and p only; no float atomics.  The chunk of a
//             wavefront comes from one scan of the faces' chunk counts and a binary search in it.
//
// The two candidate passes evaluate the same rule on the same bytes, so the places of pass 1 are the counts of pass 0.
#include <algorithm>
#include <climits>
#include <string>

#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "fit_stats.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_single_faces_dev";
constexpr int kRC = 1024;    // samples of a residual chunk: 16 per lane of its wavefront
constexpr int kAlign = 32;   // doubles: every channel's planes and measurements start on a 256-byte boundary

// ---- count and place -------------------------------------------------------------------------------------------------------------
struct SinglePackCtx {
  CandidateCtx cand;
  int *block_count;            // [blocks][3]                                                              (pass 0 writes)
  const long long *block_off;  // [blocks][3]: the place IN ITS CHANNEL of the block's first valid candidate  (block_scan3_kernel<false>)
  long long *seg;              // [3][F + 1]: where a face's samples start in the channel                   (pass 1 writes [c][0, F))
  double *ang[3], *x[3];       // the channels' planes [3][K_c] and measurements [K_c]
  long long K[3];
};

// Candidate t = (sorted pixel, light) of all three channels (capture_compact.h: read_candidate).
//   PASS 0  the block's number of valid candidates per channel
//   PASS 1  the plane triple and the measurement to their place; at a face's first candidate the face's offset (the prefix there)
template <int PASS>
__global__ __launch_bounds__(kCT) void single_pack_faces_kernel(SinglePackCtx c) {
  __shared__ int wave_cnt[kWaves][3];
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const Candidate k = read_candidate(c.cand, t);
  ChannelPlaces pl = {wave_cnt};
  pl.place(k.valid);
  if (PASS == 0) {
    if (threadIdx.x < 3) c.block_count[(size_t)blockIdx.x * 3 + threadIdx.x] = pl.count(threadIdx.x);
    return;
  }
  if (t >= c.cand.T) return;
  const bool first_of_face = k.i == 0 && k.s == c.cand.face_first[k.r];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long long at = pl.at(ch, c.block_off[(size_t)blockIdx.x * 3 + ch]);
    if (first_of_face) c.seg[(size_t)ch * (c.cand.F + 1) + k.r] = at;
    if (k.valid[ch]) {  // (at < K[ch]: the rule of pass 0 on the same bytes)
      const long long n = c.K[ch];
      double *dst = c.ang[ch] + at;
      dst[0] = k.c0;
      dst[n] = k.c1;
      dst[2 * n] = k.c2;
      c.x[ch][at] = k.v[ch] / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
    }
  }
}

// ---- residuals --------------------------------------------------------------------------------------------------------------------
// One workgroup per channel (blockIdx.x) over the carried faces: chunk_first[c][r] = the chunks of the faces below rank r, [c][F]: all
__global__ __launch_bounds__(kCT) void resid_scan_kernel(const long long *__restrict__ seg_all, int F, long long *__restrict__ chunk_first_all) {
  __shared__ long long part[kCT];
  const long long *seg = seg_all + (size_t)blockIdx.x * (F + 1);
  long long *chunk_first = chunk_first_all + (size_t)blockIdx.x * (F + 1);
  const int t = threadIdx.x;
  const long long per = ((long long)F + kCT - 1) / kCT;
  const long long r0 = t * per < F ? t * per : F, r1 = r0 + per < F ? r0 + per : F;
  long long sum = 0;
  for (long long r = r0; r < r1; ++r) sum += (seg[r + 1] - seg[r] + kRC - 1) / kRC;
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < kCT; ++i) {
      const long long v = part[i];
      part[i] = run;
      run += v;
    }
    chunk_first[F] = run;
  }
  __syncthreads();
  sum = part[t];
  for (long long r = r0; r < r1; ++r) {
    chunk_first[r] = sum;
    sum += (seg[r + 1] - seg[r] + kRC - 1) / kRC;
  }
}

struct ResidCtx {
  const double *ang, *x;  // one channel: planes [3][K], measurements [K]
  long long K;
  const long long *seg, *chunk_first;  // [F + 1] each, the channel's
  int F;
  long long max_chunks;  // what `partial` holds
  double p[kM];
  double *partial;  // [chunks]
};

// One wavefront per chunk: sum (x - f(p))^2 over the chunk's samples, f on the EXACT model path (the reference's own pow expression),
// as fit_stats.hip's e = x - f.  Lane l adds samples l, l + 64, ... of the chunk in that order; one DPP tree over the lanes.
template <int MODEL>
__global__ __launch_bounds__(kCT) void resid_chunk_kernel(ResidCtx c) {
  using Mdl = BrdfModel<MODEL>;
  const int lane = threadIdx.x & (kWave - 1);
  const long long w = (long long)blockIdx.x * kWaves + threadIdx.x / kWave;
  long long nchunks = c.chunk_first[c.F];
  if (nchunks > c.max_chunks) nchunks = c.max_chunks;  // (cannot be: sum ceil(k / kRC) <= K / kRC + F)
  if (w >= nchunks) return;                            // wave-uniform
  long long lo = 0, hi = c.F;  // chunk_first[lo] <= w < chunk_first[hi]: the last of equal entries is the face that has the chunk
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (c.chunk_first[mid] <= w) lo = mid; else hi = mid;
  }
  const long long first = c.seg[lo] + (w - c.chunk_first[lo]) * kRC, end = c.seg[lo + 1];
  const long long last = first + kRC < end ? first + kRC : end;
  const double p[kM] = {c.p[0], c.p[1], c.p[2]};
  EvalUniforms u;
  u.l0 = Mdl::lin(p);
  u.n0 = Mdl::nl(p);
  u.scal = 1.0;
  u = scalar_copy(u);
  const double *a0 = c.ang, *a1 = c.ang + c.K, *a2 = c.ang + 2 * c.K;
  double acc = 0.0;
  for (long long i = first + lane; i < last; i += kWave) {
    const double c0 = a0[i];
    const double c1 = Mdl::uses_c1 ? a1[i] : 1.0;
    const double c2 = Mdl::uses_c2 ? a2[i] : 1.0;
    const Prep q = Mdl::template prepare<false>(c0, c1, c2);
    const double e = c.x[i] - model_value<MODEL, false>(u, c0, q);
    acc += e * e;
  }
  acc = wave_reduce_to_last<OpSum>(acc);
  if (lane == kWave - 1) c.partial[w] = acc;
}

struct ResidFoldCtx {
  int F;
  const int *face_list;                // [F]
  const long long *seg, *chunk_first;  // [3][F + 1]
  const double *partial[3];
  double *sumsq;  // [nf][3] or null
  int *count;     // [nf][3] or null
};

// One thread per carried face: the chunks' partial sums in ascending order, channel after channel
__global__ __launch_bounds__(kCT) void resid_fold_kernel(ResidFoldCtx c) {
  const long long r = (long long)blockIdx.x * kCT + threadIdx.x;
  if (r >= c.F) return;
  const size_t dst = (size_t)c.face_list[r] * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long long *seg = c.seg + (size_t)ch * (c.F + 1), *cf = c.chunk_first + (size_t)ch * (c.F + 1);
    double s = 0.0;
    for (long long j = cf[r]; j < cf[r + 1]; ++j) s += c.partial[ch][j];
    if (c.sumsq) c.sumsq[dst + ch] = s;
    if (c.count) c.count[dst + ch] = (int)(seg[r + 1] - seg[r]);
  }
}

typedef void (*ResidKernel)(ResidCtx);
ResidKernel resid_kernel_of(int model) {
  static const ResidKernel t[MODEL_COUNT] = {resid_chunk_kernel<0>, resid_chunk_kernel<1>, resid_chunk_kernel<2>};
  return t[model];
}

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

  // ---- compact, group, cosines (capture_group.hip) ----
  CaptureGroup g;
  if (capture_group_run(kWho, sa.g, g) != 0) return kLmError;
  if (g.S == 0) {  // an empty capture: every channel is refused, nothing is written on the device but the pixel counts
    for (int c = 0; c < 3; ++c) refuse_channel(sa, c);
    if (sa.covar) std::fill(sa.covar, sa.covar + 3 * kM * kM, 0.0);  // (the ragged statistics of no sample)
    if (sa.stats) std::fill(sa.stats, sa.stats + 3 * kStatsSz, 0.0);
    if (sa.rank) sa.rank[0] = sa.rank[1] = sa.rank[2] = 0;
    return 3;
  }
  const long long F = g.F;

  // ---- count, scan ----
  SinglePackCtx pc = {};
  pc.cand = capture_candidates(sa.g, g);
  const long long T = pc.cand.T;  // candidates of one channel
  const int pb = (int)((T + kCT - 1) / kCT);
  DevBuf pack_count, pack_off, seg, totals;
  if (!take(pack_count, sizeof(int) * 3 * (size_t)pb, "the candidate blocks' counts", kWho) ||
      !take(pack_off, sizeof(long long) * 3 * (size_t)pb, "the candidate blocks' offsets", kWho) ||
      !take(seg, sizeof(long long) * 3 * ((size_t)F + 1), "the faces' offsets", kWho) || !take(totals, sizeof(long long) * 3, "the channels' totals", kWho))
    return kLmError;
  pc.block_count = pack_count.as<int>();
  pc.block_off = pack_off.as<long long>();
  pc.seg = seg.as<long long>();
  hipLaunchKernelGGL(single_pack_faces_kernel<0>, dim3(pb), dim3(kCT), 0, stream, pc);
  // every channel from 0: its end is K_c, also the end of the channel's face offsets, seg[c][F]
  hipLaunchKernelGGL(block_scan3_kernel<false>, dim3(1), dim3(kCT), 0, stream, pack_count.as<int>(), (long long)pb, pack_off.as<long long>(),
                     seg.as<long long>() + F, F + 1, totals.as<long long>());
  CAPTURE_OK(kWho, hipGetLastError());
  long long K[3] = {0, 0, 0};
  CAPTURE_OK(kWho, hipMemcpyAsync(K, totals.ptr, sizeof K, hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(kWho, hipStreamSynchronize(stream));
  for (int c = 0; c < 3; ++c) {
    if (K[c] < 0 || K[c] > T) {
      set_error("%s(): the count finds %lld valid samples among %lld candidates of channel %d", kWho, K[c], T, c);
      return kLmError;
    }
    if (K[c] > INT_MAX) {  // a fit's count is an int
      set_error("%s(): channel %d has %lld samples, more than INT_MAX", kWho, c, K[c]);
      return kLmError;
    }
    if (sa.count) sa.count[c] = K[c];
  }

  // ---- place: 32 bytes per valid sample ----
  size_t start[3], doubles = 0;  // a channel's planes, then its measurements
  for (int c = 0; c < 3; ++c) {
    start[c] = doubles;
    doubles += (4 * (size_t)K[c] + kAlign - 1) / kAlign * kAlign;
  }
  DevBuf packed;
  if (!take(packed, sizeof(double) * doubles, "the channels' planes and measurements", kWho)) return kLmError;
  for (int c = 0; c < 3; ++c) {
    pc.ang[c] = packed.as<double>() + start[c];
    pc.x[c] = pc.ang[c] + 3 * (size_t)K[c];
    pc.K[c] = K[c];
  }
  hipLaunchKernelGGL(single_pack_faces_kernel<1>, dim3(pb), dim3(kCT), 0, stream, pc);
  CAPTURE_OK(kWho, hipGetLastError());

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

  // ---- statistics at the fitted points: the uniform pass at n = K_c; below 3 samples the ragged one on a row of stride 3 ----
  const int h_cnt[3] = {(int)K[0], (int)K[1], (int)K[2]};  // (read by a copy the stream may still hold: lives until the last wait)
  DevBuf small;  // p [3][3], covar [3][9], stats [3][kStatsSz], three staged rows of 12 doubles; rank [3], counts [3]
  constexpr int kSmallD = 3 * kM + 3 * kM * kM + 3 * kStatsSz + 3 * 12;
  if (want_stats) {
    if (!take(small, sizeof(double) * kSmallD + sizeof(int) * 6, "the channels' statistics", kWho)) return kLmError;
    double *d_p = small.as<double>(), *d_covar = d_p + 3 * kM, *d_stats = d_covar + 3 * kM * kM, *d_stage = d_stats + 3 * kStatsSz;
    int *d_rank = reinterpret_cast<int *>(d_stage + 3 * 12), *d_cnt = d_rank + 3;
    CAPTURE_OK(kWho, hipMemsetAsync(small.ptr, 0, sizeof(double) * kSmallD + sizeof(int) * 6, stream));
    CAPTURE_OK(kWho, hipMemcpyAsync(d_p, p3, sizeof p3, hipMemcpyHostToDevice, stream));
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

  // ---- residuals of every carried face against its channel's fit ----
  DevBuf chunk_first, partial;
  if (want_faces) {
    long long max_chunks[3];
    size_t pstart[3], pdoubles = 0;
    for (int c = 0; c < 3; ++c) {
      max_chunks[c] = K[c] / kRC + F;  // sum over the faces of ceil(k / kRC)
      pstart[c] = pdoubles;
      pdoubles += (size_t)max_chunks[c];
      if ((max_chunks[c] + kWaves - 1) / kWaves > INT_MAX) {
        set_error("%s(): %lld residual chunks of channel %d are more than one launch walks", kWho, max_chunks[c], c);
        return kLmError;
      }
    }
    if (!take(chunk_first, sizeof(long long) * 3 * ((size_t)F + 1), "the faces' first chunks", kWho) ||
        !take(partial, sizeof(double) * pdoubles, "the chunks' partial sums", kWho))
      return kLmError;
    hipLaunchKernelGGL(resid_scan_kernel, dim3(3), dim3(kCT), 0, stream, seg.as<long long>(), (int)F, chunk_first.as<long long>());
    ResidFoldCtx fc = {};
    fc.F = (int)F;
    fc.face_list = g.face_list.as<int>();
    fc.seg = seg.as<long long>();
    fc.chunk_first = chunk_first.as<long long>();
    fc.sumsq = sa.d_face_sumsq;
    fc.count = sa.d_face_count;
    for (int c = 0; c < 3; ++c) {
      ResidCtx rc = {};
      rc.ang = pc.ang[c];
      rc.x = pc.x[c];
      rc.K = K[c];
      rc.seg = seg.as<long long>() + (size_t)c * (F + 1);
      rc.chunk_first = chunk_first.as<long long>() + (size_t)c * (F + 1);
      rc.F = (int)F;
      rc.max_chunks = max_chunks[c];
      for (int k = 0; k < kM; ++k) rc.p[k] = sa.single_brdf[c * kM + k];
      rc.partial = partial.as<double>() + pstart[c];
      fc.partial[c] = rc.partial;
      const unsigned grid = (unsigned)((max_chunks[c] + kWaves - 1) / kWaves);
      hipLaunchKernelGGL(resid_kernel_of(a.model), dim3(grid), dim3(kCT), 0, stream, rc);
    }
    hipLaunchKernelGGL(resid_fold_kernel, dim3((unsigned)((F + kCT - 1) / kCT)), dim3(kCT), 0, stream, fc);
    CAPTURE_OK(kWho, hipGetLastError());
  }
  CAPTURE_OK(kWho, hipStreamSynchronize(stream));
  return failed;
}

}  // namespace brdf
