// capture_faces.hip -- brdf_hip_fit_capture_faces_dev: ONE fit per (face, channel) over the samples of ALL the face's pixels, where
// the capture loop of capture_fit.hip fits every pixel and keeps the face's last one.  No fit or statistics kernel of its own: the
// capture becomes a packed batch (packed_fit.h) on the device, the packed calls fit it, a scatter fills the [nf][3] maps.
//
// (compact, group and cosines are capture_group.h's, shared with capture_means.hip)
//   compact   the pixels that carry a face, in the reference's x-major walk (the two-pass compaction of capture_fit.hip), and the
//             number of pixels of every face (integer adds: their order cannot show)
//   group     a stable radix sort of the compacted pixels by face (rocPRIM; walk order kept inside a face); one scan over the faces
//             gives the carried faces in ascending order, each with its first sorted pixel
//   cosines   angles_f[F][3][L] of the F carried faces (cosines.hip): all pixels of a face share them
//   pack      the candidates of a channel are ONE flat array, t = sorted pixel * L + light, and a channel's measurements are one
//             stream compaction of it (ballot + popcount, block counts, scan: count / place once more).  A fit's offset is the
//             prefix at its face's first candidate, so no wave belongs to a face and a face of 10^5 pixels costs what 10^5 faces of
//             one pixel cost.  Fit s = channel * F + face rank: the offsets ascend with s.  A third pass over the same candidates
//             writes the plane triples, which need the fits' counts.
//   fit       packed_fit_run (dlevmar_bc_dif), packed_stats_run where a statistics map is asked for
//   scatter   rows (face, channel) in ascending order: p, info, ret, the statistics, the counts; block sums of p in a fixed order
//
// The three candidate passes evaluate the same rule on the same bytes, so the places of pass 2 and 3 are the counts of pass 1.
#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "fit_stats.h"
#include "packed_fit.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_faces_dev";

// ---- count and pack ------------------------------------------------------------------------------------------------------------
struct PackCtx {
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
  int *block_count;             // [blocks][3]                                                    (pass 0 writes)
  const long long *block_off;   // [blocks][3]: the place of the block's first valid candidate    (pack_scan_kernel)
  long long *offsets;           // [3 F + 1]                                                      (pass 1 writes, pass 2 reads)
  double *angles, *x, *p;       // the packed batch
  double p0[kM];
};

// Candidate t = (sorted pixel, light) of all three channels: the pixel's B, G, R bytes are one read, the cosine test is the face's.
//   PASS 0  the block's number of valid candidates per channel
//   PASS 1  measurements to their places; at a face's first candidate the fit's offset (the prefix there) and its starting point
//   PASS 2  the plane triples, three planes of the fit's count each
template <int PASS>
__global__ __launch_bounds__(kCT) void pack_kernel(PackCtx c) {
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
    const size_t fit = (size_t)ch * c.F + r;
    if (PASS == 1) {
      if (valid[ch]) c.x[at] = v[ch] / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
      if (first_of_face) {
        c.offsets[fit] = at;
        for (int k = 0; k < kM; ++k) c.p[fit * kM + k] = c.p0[k];
      }
    } else if (valid[ch]) {
      const long long o = c.offsets[fit], k = c.offsets[fit + 1] - o;
      double *dst = c.angles + 3 * o + (at - o);
      dst[0] = c0;
      dst[k] = c1;
      dst[2 * k] = c2;
    }
  }
}

// the scan between pass 0 and pass 1, one workgroup: block_count[b][ch] -> block_off[b][ch], channel after channel (channel ch
// starts where the channels below it end); offsets[3 F] and *total: the valid candidates of all three channels
__global__ __launch_bounds__(kCT) void pack_scan_kernel(const int *__restrict__ block_count, long long nb, long long *__restrict__ block_off,
                                                        long long *__restrict__ offsets_end, long long *__restrict__ total) {
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
  if (t == 0) {
    long long run = 0;
    for (int ch = 0; ch < 3; ++ch) {
      for (int i = 0; i < kCT; ++i) {
        const long long v = part[i][ch];
        part[i][ch] = run;
        run += v;
      }
    }
    *offsets_end = run;
    *total = run;
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

// ---- scatter -------------------------------------------------------------------------------------------------------------------
struct FaceScatterCtx {
  int F;
  const int *face_list;
  const long long *offsets;
  const double *p, *info, *covar, *stats;  // the batch's results, rows channel * F + face rank; null: not computed
  const int *ret, *rank;
  double *surfaces, *s_info, *s_covar, *s_stats;  // the [nf][3] maps; null (all but surfaces): not wanted
  int *s_ret, *s_rank, *s_count;
  double *block_sums;  // [blocks][3]
};

// One thread per (carried face, channel), in ascending order of the destination rows; per-block partial sums of kd, ks, n in a fixed
// order (store_kernel's reduction in capture_fit.hip)
__global__ __launch_bounds__(kCT) void face_scatter_kernel(FaceScatterCtx c) {
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
    if (c.s_count) c.s_count[dst] = (int)(c.offsets[src + 1] - c.offsets[src]);
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

#define FACES_OK(call)                                                        \
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
int capture_faces_check(const CaptureFacesArgs &a) {
  if (a.workspace_bytes < 0) {
    set_error("%s(): workspace_bytes = %lld: need workspace_bytes >= 0", kWho, a.workspace_bytes);
    return kLmError;
  }
  return capture_args_check(kWho, a, 64, "");
}

}  // namespace

int capture_faces_run(const CaptureFacesArgs &a) {
  if (capture_faces_check(a) != 0) return kLmError;
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int L = a.L, H = a.H, W = a.W, nf = a.nf;
  if (a.avg) a.avg[0] = a.avg[1] = a.avg[2] = 0.0;
  if (a.n_pixels) *a.n_pixels = 0;
  if (a.n_faces) *a.n_faces = 0;

  // ---- compact, group, cosines (capture_group.h) ----
  CaptureGroup g;
  if (capture_group_run(kWho, a, g) != 0) return kLmError;
  if (g.S == 0) return 0;  // an empty capture: nothing is written but the pixel counts
  const long long S = g.S, F = g.F, T = S * L;  // T: candidates of one channel
  DevBuf &pixel_sorted = g.pixel_sorted, &face_sorted = g.face_sorted, &face_list = g.face_list, &face_first = g.face_first,
         &rank_of_face = g.rank_of_face, &head = g.head, &angles_f = g.angles_f;

  // ---- count and pack ----
  const int pb = (int)((T + kCT - 1) / kCT), fits = (int)(3 * F);
  DevBuf pack_count, pack_off, offsets, p;
  if (!take(pack_count, sizeof(int) * 3 * (size_t)pb, "the candidate blocks' counts") ||
      !take(pack_off, sizeof(long long) * 3 * (size_t)pb, "the candidate blocks' offsets") ||
      !take(offsets, sizeof(long long) * ((size_t)fits + 1), "the fits' offsets") || !take(p, sizeof(double) * kM * (size_t)fits, "the fits' parameters"))
    return kLmError;
  PackCtx pc = {};
  pc.images = a.d_images;
  pc.L = L;
  pc.H = H;
  pc.W = W;
  pc.pixel_sorted = pixel_sorted.as<long long>();
  pc.face_sorted = face_sorted.as<unsigned>();
  pc.rank_of_face = rank_of_face.as<int>();
  pc.face_first = face_first.as<long long>();
  pc.angles_f = angles_f.as<double>();
  pc.T = T;
  pc.F = (int)F;
  pc.v_min = a.v_min;
  pc.v_max = a.v_max;
  pc.cos_min = a.cos_min;
  pc.use1 = a.model != MODEL_PHONG;
  pc.use2 = a.model != MODEL_BLINN_PHONG;
  pc.block_count = pack_count.as<int>();
  pc.block_off = pack_off.as<long long>();
  pc.offsets = offsets.as<long long>();
  pc.p = p.as<double>();
  for (int k = 0; k < kM; ++k) pc.p0[k] = a.p0[k];
  hipLaunchKernelGGL(pack_kernel<0>, dim3(pb), dim3(kCT), 0, stream, pc);
  hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(kCT), 0, stream, pack_count.as<int>(), (long long)pb, pack_off.as<long long>(),
                     offsets.as<long long>() + fits, head.as<long long>() + 2);
  FACES_OK(hipGetLastError());
  long long total = 0;
  FACES_OK(hipMemcpyAsync(&total, head.as<long long>() + 2, sizeof total, hipMemcpyDeviceToHost, stream));
  FACES_OK(hipStreamSynchronize(stream));
  if (total < 0 || total > 3 * T) {
    set_error("%s(): the count finds %lld valid samples among %lld candidates", kWho, total, 3 * T);
    return kLmError;
  }
  DevBuf angles, x;  // 32 bytes per valid sample
  if (!take(angles, sizeof(double) * 3 * (size_t)total, "the packed planes") || !take(x, sizeof(double) * (size_t)total, "the packed measurements"))
    return kLmError;
  pc.angles = angles.as<double>();
  pc.x = x.as<double>();
  hipLaunchKernelGGL(pack_kernel<1>, dim3(pb), dim3(kCT), 0, stream, pc);
  hipLaunchKernelGGL(pack_kernel<2>, dim3(pb), dim3(kCT), 0, stream, pc);
  FACES_OK(hipGetLastError());

  // ---- fit ----
  const bool want_stats = a.d_surface_covar || a.d_surface_stats || a.d_surface_rank;
  DevBuf info, ret, covar, stats, rank;
  if ((a.d_surface_info && !take(info, sizeof(double) * kInfoSz * (size_t)fits, "the fits' info")) ||
      (a.d_surface_ret && !take(ret, sizeof(int) * (size_t)fits, "the fits' ret")) ||
      (a.d_surface_covar && !take(covar, sizeof(double) * kM * kM * (size_t)fits, "the fits' covariances")) ||
      (a.d_surface_stats && !take(stats, sizeof(double) * kStatsSz * (size_t)fits, "the fits' statistics")) ||
      (a.d_surface_rank && !take(rank, sizeof(int) * (size_t)fits, "the fits' ranks")))
    return kLmError;
  const PackedFitArgs pf = {BRDF_METHOD_BC_DIF, a.model, angles.as<double>(), x.as<double>(), offsets.as<long long>(), fits, p.as<double>(), a.lb, a.ub,
                            a.itmax, a.opts, info.as<double>(), ret.as<int>(), a.workspace_bytes, stream};
  if (packed_fit_run(pf, kWho) != 0) return kLmError;
  if (want_stats) {
    const PackedStatsArgs ps = {BRDF_METHOD_BC_DIF, a.model, pf.d_angles, pf.d_x, pf.d_offsets, fits, pf.d_p, a.opts, covar.as<double>(), stats.as<double>(),
                                rank.as<int>(), a.workspace_bytes, stream};
    if (packed_stats_run(ps, kWho) != 0) return kLmError;
  }

  // ---- scatter ----
  const int sb = (fits + kCT - 1) / kCT;
  DevBuf sums;
  if (!take(sums, sizeof(double) * 3 * (size_t)sb, "the block sums")) return kLmError;
  const FaceScatterCtx sc = {(int)F, face_list.as<int>(), offsets.as<long long>(), p.as<double>(), info.as<double>(), covar.as<double>(), stats.as<double>(),
                             ret.as<int>(), rank.as<int>(), a.d_brdf_surfaces, a.d_surface_info, a.d_surface_covar, a.d_surface_stats, a.d_surface_ret,
                             a.d_surface_rank, a.d_surface_count, sums.as<double>()};
  hipLaunchKernelGGL(face_scatter_kernel, dim3(sb), dim3(kCT), 0, stream, sc);
  FACES_OK(hipGetLastError());
  std::vector<double> h_sums((size_t)3 * sb);
  FACES_OK(hipMemcpyAsync(h_sums.data(), sums.ptr, sizeof(double) * 3 * sb, hipMemcpyDeviceToHost, stream));
  FACES_OK(hipStreamSynchronize(stream));
  if (a.avg) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < sb; ++b)
      for (int k = 0; k < 3; ++k) t[k] += h_sums[(size_t)3 * b + k];
    for (int k = 0; k < 3; ++k) a.avg[k] = t[k] / ((double)nf * 3);
  }
  return 0;
}

}  // namespace brdf
