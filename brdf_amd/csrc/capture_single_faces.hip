// capture_single_faces.hip -- brdf_hip_fit_capture_single_faces_dev: ONE fit per colour channel for the whole object over the valid
// samples of EVERY pixel of every carried face, where capture_fit.hip's single-BRDF fit takes each face's last pixel and knows no
// validity rule; and, per carried face and channel, the sum of squared residuals against that one fit: where on the object the
// one-material assumption fails.  No fit or statistics kernel of its own: stream_fit_run fits, fit_stats.hip takes the statistics.
//
// (compact, group and cosines are capture_group.h's, shared with capture_faces.hip and capture_means.hip)
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
// The kernels here are copies, not shared text: capture_faces.hip's instances keep their registers (weighted_fit.hip tells why).
// The two candidate passes evaluate the same rule on the same bytes, so the places of pass 1 are the counts of pass 0.
#include <algorithm>
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
  const unsigned char *images;
  int L, H, W;
  const long long *pixel_sorted;  // [S]: x-major pixel index, grouped by face
  const unsigned *face_sorted;    // [S]
  const int *rank_of_face;        // [nf]
  const long long *face_first;    // [F + 1]
  const double *angles_f;         // [F][3][L]
  long long T;                    // candidates of one channel: S * L
  int F;
  int v_min, v_max;
  double cos_min;
  int use1, use2;  // the planes the model reads besides the first (brdf_models.h: uses_c1, uses_c2)
  int *block_count;            // [blocks][3]                                                              (pass 0 writes)
  const long long *block_off;  // [blocks][3]: the place IN ITS CHANNEL of the block's first valid candidate  (single_scan_kernel)
  long long *seg;              // [3][F + 1]: where a face's samples start in the channel                   (pass 1 writes [c][0, F))
  double *ang[3], *x[3];       // the channels' planes [3][K_c] and measurements [K_c]
  long long K[3];
};

// Candidate t = (sorted pixel, light) of all three channels: the pixel's B, G, R bytes are one read, the cosine test is the face's.
//   PASS 0  the block's number of valid candidates per channel
//   PASS 1  the plane triple and the measurement to their place; at a face's first candidate the face's offset (the prefix there)
template <int PASS>
__global__ __launch_bounds__(kCT) void single_pack_faces_kernel(SinglePackCtx c) {
  __shared__ int wave_cnt[kWaves][3];
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  bool valid[3] = {false, false, false};
  int v[3] = {0, 0, 0}, i = 0, r = 0;
  long long s = 0;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (t < c.T) {
    s = t / c.L;
    i = (int)(t - s * c.L);
    r = c.rank_of_face[c.face_sorted[s]];
    const long long g = c.pixel_sorted[s];
    const int px = (int)(g / c.H), py = (int)(g % c.H);
    const unsigned char *pxl = c.images + (((size_t)i * c.H + (size_t)(c.H - 1 - py)) * c.W + px) * 3;
    const double *a = c.angles_f + (size_t)r * 3 * c.L + i;
    c0 = a[0];
    c1 = a[c.L];
    c2 = a[2 * c.L];
    const bool cos_ok = c0 > c.cos_min && (!c.use1 || c1 > c.cos_min) && (!c.use2 || c2 > c.cos_min);  // (a NaN is not valid)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      v[ch] = pxl[ch];
      valid[ch] = cos_ok && v[ch] >= c.v_min && v[ch] <= c.v_max;
    }
  }
  int before[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned long long m = __ballot(valid[ch]);
    before[ch] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave][ch] = __popcll(m);
  }
  __syncthreads();
  if (PASS == 0) {
    if (threadIdx.x < 3) {
      int n = 0;
      for (int w = 0; w < kWaves; ++w) n += wave_cnt[w][threadIdx.x];
      c.block_count[(size_t)blockIdx.x * 3 + threadIdx.x] = n;
    }
    return;
  }
  if (t >= c.T) return;
  const bool first_of_face = i == 0 && s == c.face_first[r];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    long long at = c.block_off[(size_t)blockIdx.x * 3 + ch] + before[ch];
    for (int w = 0; w < wave; ++w) at += wave_cnt[w][ch];
    if (first_of_face) c.seg[(size_t)ch * (c.F + 1) + r] = at;
    if (valid[ch]) {  // (at < K[ch]: the rule of pass 0 on the same bytes)
      const long long k = c.K[ch];
      double *dst = c.ang[ch] + at;
      dst[0] = c0;
      dst[k] = c1;
      dst[2 * k] = c2;
      c.x[ch][at] = v[ch] / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
    }
  }
}

// the scan between the two passes, one workgroup: block_count[b][ch] -> block_off[b][ch], every channel from 0; totals[ch] = K_ch, also
// the end of the channel's face offsets, seg[ch][F]
__global__ __launch_bounds__(kCT) void single_scan_kernel(const int *__restrict__ block_count, long long nb, long long *__restrict__ block_off,
                                                          long long *__restrict__ seg, int F, long long *__restrict__ totals) {
  __shared__ long long part[kCT][3];
  const int t = threadIdx.x;
  const long long per = (nb + kCT - 1) / kCT;
  const long long b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
  long long sum[3] = {0, 0, 0};
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sum[ch] += block_count[b * 3 + ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) part[t][ch] = sum[ch];
  __syncthreads();
  if (t < 3) {
    long long run = 0;
    for (int i = 0; i < kCT; ++i) {
      const long long v = part[i][t];
      part[i][t] = run;
      run += v;
    }
    totals[t] = run;
    seg[(size_t)t * (F + 1) + F] = run;
  }
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) sum[ch] = part[t][ch];
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      block_off[b * 3 + ch] = sum[ch];
      sum[ch] += block_count[b * 3 + ch];
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

#define SINGLE_OK(call)                                                       \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", kWho, #call, hipGetErrorString(e_));   \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

// `bytes` of device memory for `what`; a failure names the bytes asked for
bool take(DevBuf &b, size_t bytes, const char *what) { return take(b, bytes, what, kWho); }

// what the entry refuses before any HIP call
int capture_single_faces_check(const CaptureSingleFacesArgs &sa) {
  const CaptureFacesArgs &a = sa.cap;
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !sa.single_brdf) {
    set_error("%s(): null images, pixel map, mesh, leds, view origin, p0 or single_brdf", kWho);
    return kLmError;
  }
  if (a.L < 1 || a.L > 64 || a.H <= 0 || a.W <= 0 || a.nf <= 0 || a.nf > INT_MAX / 3) {
    set_error("%s(): L = %d, H = %d, W = %d, nf = %d: need 1 <= L <= 64, H, W, nf > 0 and 3 nf <= INT_MAX", kWho, a.L, a.H, a.W, a.nf);
    return kLmError;
  }
  MethodSpec ms;
  if (!known_model_method(a.model, BRDF_METHOD_BC_DIF, &ms, kWho)) return kLmError;
  if (a.v_min > a.v_max || a.cos_min != a.cos_min) {
    set_error("%s(): bad validity rule (v_min %d > v_max %d, or cos_min not a number)", kWho, a.v_min, a.v_max);
    return kLmError;
  }
  return box_refused(ms, a.lb, a.ub, kWho) ? kLmError : 0;
}

// levmar's n < m refusal of channel c: ret = LM_ERROR, zero info, p0
void refuse_channel(const CaptureSingleFacesArgs &sa, int c) {
  for (int k = 0; k < kM; ++k) sa.single_brdf[c * kM + k] = sa.cap.p0[k];
  if (sa.info)
    for (int k = 0; k < kInfoSz; ++k) sa.info[c * kInfoSz + k] = 0.0;
  if (sa.ret) sa.ret[c] = kLmError;
}

}  // namespace

int capture_single_faces_run(const CaptureSingleFacesArgs &sa) {
  if (capture_single_faces_check(sa) != 0) return kLmError;
  const CaptureFacesArgs &a = sa.cap;
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int L = a.L, H = a.H, W = a.W;
  if (a.n_pixels) *a.n_pixels = 0;
  if (a.n_faces) *a.n_faces = 0;
  if (sa.count) sa.count[0] = sa.count[1] = sa.count[2] = 0;
  const bool want_stats = sa.covar || sa.stats || sa.rank;
  const bool want_faces = sa.d_face_sumsq || sa.d_face_count;

  // ---- compact, group, cosines (capture_group.h) ----
  CaptureGroup g;
  if (capture_group_run(kWho, a, g) != 0) return kLmError;
  if (g.S == 0) {  // an empty capture: every channel is refused, nothing is written on the device but the pixel counts
    for (int c = 0; c < 3; ++c) refuse_channel(sa, c);
    if (sa.covar) std::fill(sa.covar, sa.covar + 3 * kM * kM, 0.0);  // (the ragged statistics of no sample)
    if (sa.stats) std::fill(sa.stats, sa.stats + 3 * kStatsSz, 0.0);
    if (sa.rank) sa.rank[0] = sa.rank[1] = sa.rank[2] = 0;
    return 3;
  }
  const long long S = g.S, F = g.F, T = S * L;  // T: candidates of one channel

  // ---- count, scan ----
  const int pb = (int)((T + kCT - 1) / kCT);
  DevBuf pack_count, pack_off, seg;
  if (!take(pack_count, sizeof(int) * 3 * (size_t)pb, "the candidate blocks' counts") ||
      !take(pack_off, sizeof(long long) * 3 * (size_t)pb, "the candidate blocks' offsets") ||
      !take(seg, sizeof(long long) * 3 * ((size_t)F + 1), "the faces' offsets"))
    return kLmError;
  SinglePackCtx pc = {};
  pc.images = a.d_images;
  pc.L = L;
  pc.H = H;
  pc.W = W;
  pc.pixel_sorted = g.pixel_sorted.as<long long>();
  pc.face_sorted = g.face_sorted.as<unsigned>();
  pc.rank_of_face = g.rank_of_face.as<int>();
  pc.face_first = g.face_first.as<long long>();
  pc.angles_f = g.angles_f.as<double>();
  pc.T = T;
  pc.F = (int)F;
  pc.v_min = a.v_min;
  pc.v_max = a.v_max;
  pc.cos_min = a.cos_min;
  pc.use1 = a.model != MODEL_PHONG;
  pc.use2 = a.model != MODEL_BLINN_PHONG;
  pc.block_count = pack_count.as<int>();
  pc.block_off = pack_off.as<long long>();
  pc.seg = seg.as<long long>();
  hipLaunchKernelGGL(single_pack_faces_kernel<0>, dim3(pb), dim3(kCT), 0, stream, pc);
  hipLaunchKernelGGL(single_scan_kernel, dim3(1), dim3(kCT), 0, stream, pack_count.as<int>(), (long long)pb, pack_off.as<long long>(), seg.as<long long>(),
                     (int)F, g.head.as<long long>());
  SINGLE_OK(hipGetLastError());
  long long K[3] = {0, 0, 0};
  SINGLE_OK(hipMemcpyAsync(K, g.head.ptr, sizeof K, hipMemcpyDeviceToHost, stream));
  SINGLE_OK(hipStreamSynchronize(stream));
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
  if (!take(packed, sizeof(double) * doubles, "the channels' planes and measurements")) return kLmError;
  for (int c = 0; c < 3; ++c) {
    pc.ang[c] = packed.as<double>() + start[c];
    pc.x[c] = pc.ang[c] + 3 * (size_t)K[c];
    pc.K[c] = K[c];
  }
  hipLaunchKernelGGL(single_pack_faces_kernel<1>, dim3(pb), dim3(kCT), 0, stream, pc);
  SINGLE_OK(hipGetLastError());

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
    if (!take(small, sizeof(double) * kSmallD + sizeof(int) * 6, "the channels' statistics")) return kLmError;
    double *d_p = small.as<double>(), *d_covar = d_p + 3 * kM, *d_stats = d_covar + 3 * kM * kM, *d_stage = d_stats + 3 * kStatsSz;
    int *d_rank = reinterpret_cast<int *>(d_stage + 3 * 12), *d_cnt = d_rank + 3;
    SINGLE_OK(hipMemsetAsync(small.ptr, 0, sizeof(double) * kSmallD + sizeof(int) * 6, stream));
    SINGLE_OK(hipMemcpyAsync(d_p, p3, sizeof p3, hipMemcpyHostToDevice, stream));
    SINGLE_OK(hipMemcpyAsync(d_cnt, h_cnt, sizeof h_cnt, hipMemcpyHostToDevice, stream));
    for (int c = 0; c < 3; ++c) {
      FitStatsArgs f = {BRDF_METHOD_BC_DIF, a.model, pc.ang[c], pc.x[c], 1, (int)K[c], d_p + c * kM, a.opts, d_covar + c * kM * kM, d_stats + c * kStatsSz,
                        d_rank + c, nullptr, 0, stream, nullptr};
      if (K[c] < kM) {
        double *row = d_stage + c * 12;  // planes [3][3], x [3]: the channel's K_c samples at the front of each
        for (int k = 0; k < 3 && K[c] > 0; ++k)
          SINGLE_OK(hipMemcpyAsync(row + 3 * k, pc.ang[c] + k * K[c], sizeof(double) * K[c], hipMemcpyDeviceToDevice, stream));
        if (K[c] > 0) SINGLE_OK(hipMemcpyAsync(row + 9, pc.x[c], sizeof(double) * K[c], hipMemcpyDeviceToDevice, stream));
        f.d_angles = row;
        f.d_x = row + 9;
        f.n = kM;
        f.d_counts = d_cnt + c;
      }
      if (fit_stats_enqueue(f, kWho) != 0) return kLmError;
    }
    if (sa.covar) SINGLE_OK(hipMemcpyAsync(sa.covar, d_covar, sizeof(double) * 3 * kM * kM, hipMemcpyDeviceToHost, stream));
    if (sa.stats) SINGLE_OK(hipMemcpyAsync(sa.stats, d_stats, sizeof(double) * 3 * kStatsSz, hipMemcpyDeviceToHost, stream));
    if (sa.rank) SINGLE_OK(hipMemcpyAsync(sa.rank, d_rank, sizeof(int) * 3, hipMemcpyDeviceToHost, stream));
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
    if (!take(chunk_first, sizeof(long long) * 3 * ((size_t)F + 1), "the faces' first chunks") ||
        !take(partial, sizeof(double) * pdoubles, "the chunks' partial sums"))
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
    SINGLE_OK(hipGetLastError());
  }
  SINGLE_OK(hipStreamSynchronize(stream));
  return failed;
}

}  // namespace brdf
