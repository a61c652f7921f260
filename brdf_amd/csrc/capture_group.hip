// capture_group.hip -- the host layer the capture entries share (capture_group.h), its kernels, and the library's only use of rocPRIM.
//
//   compact   the pixels that carry a face, in the reference's x-major walk: a deterministic two-pass compaction (count per block,
//             prefix on the host, place), and one statistic per face by an integer atomic -- its last pixel (the capture loop,
//             capture_fit.hip) or its number of pixels (the grouping).  Integer atomics: their order cannot show.
//   group     a stable radix sort of the compacted pixels by face (rocPRIM; walk order kept inside a face); one scan over the faces
//             gives the carried faces in ascending order, each with its first sorted pixel
//   cosines   angles_f[F][3][L] of the F carried faces (cosines.hip): all pixels of a face share them
//   scatter   rows (face, channel) of the [nf][3] maps in ascending order: p, info, ret, the statistics, the counts; block sums of p
//             in a fixed order, added on the host in block order
#include <algorithm>
#include <climits>
#include <cstring>  // (in front of rocPRIM, whose headers use memset without it)
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "capture_group.h"
#include "fit_stats.h"

namespace brdf {

namespace {

// pass 1 of the pixel compaction
__global__ __launch_bounds__(kCT) void count_kernel(const int *pm, int H, int W, int nf, int *block_count) {
  __shared__ int wave_cnt[kWaves];
  const long long g = (long long)blockIdx.x * kCT + threadIdx.x;
  const int f = (g < (long long)H * W) ? face_of(pm, H, W, g) : -1;
  const bool valid = f > -1 && f < nf;
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & (kWave - 1)) == 0) wave_cnt[threadIdx.x / kWave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// pass 2: a carried pixel's place in the walk, and its face's statistic
template <FaceStat STAT>
__global__ __launch_bounds__(kCT) void compact_kernel(const int *pm, int H, int W, int nf, const long long *block_offset, long long *pixel_of,
                                                      unsigned *face_of_surfel, void *face_stat) {
  __shared__ int wave_cnt[kWaves];
  const long long g = (long long)blockIdx.x * kCT + threadIdx.x;
  const int f = (g < (long long)H * W) ? face_of(pm, H, W, g) : -1;
  const bool valid = f > -1 && f < nf;
  const unsigned long long m = __ballot(valid);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  if (!valid) return;
  long long s = block_offset[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) s += wave_cnt[w];
  pixel_of[s] = g;
  face_of_surfel[s] = (unsigned)f;
  if (STAT == FaceStat::kLastPixel)
    atomicMax(static_cast<unsigned long long *>(face_stat) + f, (unsigned long long)(s + 1));  // 0 = no pixel
  else
    atomicAdd(static_cast<int *>(face_stat) + f, 1);
}

// One workgroup over the faces: the carried faces in ascending order (face_list[F]), where each one's pixels start among the sorted
// pixels (face_first[F + 1]) and its rank (rank_of_face[nf], -1 for a face no pixel carries); head = {F, the largest pixel count}.
__global__ __launch_bounds__(kCT) void face_scan_kernel(const int *__restrict__ face_pixels, int nf, int *__restrict__ face_list,
                                                        long long *__restrict__ face_first, int *__restrict__ rank_of_face,
                                                        long long *__restrict__ head) {
  __shared__ long long part_px[kCT];
  __shared__ int part_f[kCT], part_mx[kCT];
  const int t = threadIdx.x;
  const long long per = ((long long)nf + kCT - 1) / kCT;
  const long long b0 = t * per < nf ? t * per : nf, b1 = b0 + per < nf ? b0 + per : nf;
  long long px = 0;
  int fc = 0, mx = 0;
  for (long long f = b0; f < b1; ++f) {
    const int k = face_pixels[f];
    px += k;
    fc += k > 0;
    mx = k > mx ? k : mx;
  }
  part_px[t] = px;
  part_f[t] = fc;
  part_mx[t] = mx;
  __syncthreads();
  if (t == 0) {
    long long run_px = 0;
    int run_f = 0, all_mx = 0;
    for (int i = 0; i < kCT; ++i) {
      const long long v = part_px[i];
      const int c = part_f[i];
      part_px[i] = run_px;
      part_f[i] = run_f;
      run_px += v;
      run_f += c;
      all_mx = part_mx[i] > all_mx ? part_mx[i] : all_mx;
    }
    head[0] = run_f;
    head[1] = all_mx;
    face_first[run_f] = run_px;
  }
  __syncthreads();
  px = part_px[t];
  fc = part_f[t];
  for (long long f = b0; f < b1; ++f) {
    const int k = face_pixels[f];
    rank_of_face[f] = k > 0 ? fc : -1;
    if (k > 0) {
      face_list[fc] = (int)f;
      face_first[fc] = px;
      ++fc;
      px += k;
    }
  }
}

struct ScatterCtx {
  int F;
  const int *face_list;
  const long long *offsets;  // the fits' counts: offsets[s + 1] - offsets[s], or (null) nobs[s]
  const int *nobs;
  const double *p, *info, *covar, *stats;  // the batch's results, rows channel * F + face rank; null: not computed
  const int *ret, *rank, *lights;
  double *surfaces, *s_info, *s_covar, *s_stats;  // the [nf][3] maps; null (all but surfaces): not wanted
  int *s_ret, *s_rank, *s_count, *s_lights;
  double *block_sums;  // [blocks][3]
};

// One thread per (carried face, channel), in ascending order of the destination rows; per-block partial sums of kd, ks, n
__global__ __launch_bounds__(kCT) void scatter_kernel(ScatterCtx c) {
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
    if (c.s_count) c.s_count[dst] = c.offsets ? (int)(c.offsets[src + 1] - c.offsets[src]) : c.nobs[src];
    if (c.s_lights) c.s_lights[dst] = c.lights[src];
  }
  block_sums3(v, c.block_sums);
}

}  // namespace

bool take(DevBuf &b, size_t bytes, const char *what, const char *who) {
  const hipError_t e = b.ensure(bytes);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  set_error("%s(): cannot allocate %zu bytes for %s: %s", who, bytes, what, hipGetErrorString(e));
  return false;
}

int capture_compact_run(const char *who, const CaptureArgs &a, PixelCompaction &c) {
  const long long npx = (long long)a.H * a.W;
  if ((npx + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): H x W = %lld pixels are more than one launch walks", who, npx);
    return kLmError;
  }
  const int nb = (int)((npx + kCT - 1) / kCT);
  if (!take(c.counts, sizeof(int) * nb, "the pixel blocks' counts", who) || !take(c.block_off, sizeof(long long) * nb, "the pixel blocks' offsets", who))
    return kLmError;
  hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kCT), 0, a.stream, a.d_pixel_map, a.H, a.W, a.nf, c.counts.as<int>());
  CAPTURE_OK(who, hipGetLastError());
  std::vector<int> h_counts(nb);
  CAPTURE_OK(who, hipMemcpyAsync(h_counts.data(), c.counts.ptr, sizeof(int) * nb, hipMemcpyDeviceToHost, a.stream));
  CAPTURE_OK(who, hipStreamSynchronize(a.stream));
  c.h_off.resize(nb);
  long long S = 0;
  for (int b = 0; b < nb; ++b) {
    c.h_off[b] = S;
    S += h_counts[b];
  }
  c.S = S;
  if (S == 0 || S > c.max_S) return 0;
  CAPTURE_OK(who, hipMemcpyAsync(c.block_off.ptr, c.h_off.data(), sizeof(long long) * nb, hipMemcpyHostToDevice, a.stream));
  if (!take(c.pixel_of, sizeof(long long) * S, "the carried pixels", who) || !take(c.face_s, sizeof(unsigned) * S, "the carried pixels' faces", who))
    return kLmError;
  const auto kernel = c.stat == FaceStat::kLastPixel ? compact_kernel<FaceStat::kLastPixel> : compact_kernel<FaceStat::kPixelCount>;
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(kCT), 0, a.stream, a.d_pixel_map, a.H, a.W, a.nf, c.block_off.as<long long>(), c.pixel_of.as<long long>(),
                     c.face_s.as<unsigned>(), c.d_face_stat);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int capture_average(const char *who, const CaptureArgs &a, const double *d_block_sums, int blocks, double *avg) {
  std::vector<double> h_sums((size_t)3 * blocks);
  CAPTURE_OK(who, hipMemcpyAsync(h_sums.data(), d_block_sums, sizeof(double) * 3 * blocks, hipMemcpyDeviceToHost, a.stream));
  CAPTURE_OK(who, hipStreamSynchronize(a.stream));
  if (!avg) return 0;
  double t[3] = {0.0, 0.0, 0.0};
  for (int b = 0; b < blocks; ++b)
    for (int k = 0; k < 3; ++k) t[k] += h_sums[(size_t)3 * b + k];
  for (int k = 0; k < 3; ++k) avg[k] = t[k] / ((double)a.nf * 3);
  return 0;
}

int capture_args_check(const char *who, const CaptureGrouped &ga, const void *out, const char *out_name, int max_L, const char *l_note) {
  const CaptureArgs &a = ga.cap;
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !out) {
    set_error("%s(): null images, pixel map, mesh, leds, view origin, p0 or %s", who, out_name);
    return kLmError;
  }
  if (a.L < 1 || a.L > max_L || a.H <= 0 || a.W <= 0 || a.nf <= 0 || a.nf > INT_MAX / 3) {
    set_error("%s(): L = %d, H = %d, W = %d, nf = %d: need 1 <= L <= %d%s, H, W, nf > 0 and 3 nf <= INT_MAX", who, a.L, a.H, a.W, a.nf, max_L, l_note);
    return kLmError;
  }
  MethodSpec ms;
  if (!known_model_method(a.model, BRDF_METHOD_BC_DIF, &ms, who)) return kLmError;
  if (ga.v_min > ga.v_max || ga.cos_min != ga.cos_min) {
    set_error("%s(): bad validity rule (v_min %d > v_max %d, or cos_min not a number)", who, ga.v_min, ga.v_max);
    return kLmError;
  }
  return box_refused(ms, a.lb, a.ub, who) ? kLmError : 0;
}

int capture_group_run(const char *who, const CaptureGrouped &ga, CaptureGroup &g) {
  const CaptureArgs &a = ga.cap;
  hipStream_t stream = a.stream;
  const int L = a.L, nf = a.nf;
  // ---- compact: the pixels that carry a face, in walk order, and every face's number of pixels ----
  if (!take(g.face_pixels, sizeof(int) * (size_t)nf, "the faces' pixel counts", who)) return kLmError;
  CAPTURE_OK(who, hipMemsetAsync(g.face_pixels.ptr, 0, sizeof(int) * (size_t)nf, stream));
  g.walk.stat = FaceStat::kPixelCount;
  g.walk.d_face_stat = g.face_pixels.ptr;
  g.walk.max_S = std::min<long long>(INT_MAX, (long long)INT_MAX * kCT / L);  // S and the candidate blocks of a channel, ceil(S L / kCT), are ints
  if (capture_compact_run(who, a, g.walk) != 0) return kLmError;
  const long long S = g.walk.S;
  if (S == 0) {  // an empty capture: nothing is written but the pixel counts
    if (ga.d_face_pixels) CAPTURE_OK(who, hipMemcpyAsync(ga.d_face_pixels, g.face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
    CAPTURE_OK(who, hipStreamSynchronize(stream));
    return 0;
  }
  if (S > g.walk.max_S) {
    set_error("%s(): %lld pixels carry a face, %lld candidates per channel: more than one launch walks", who, S, S * L);
    return kLmError;
  }

  // ---- group: a stable sort by face keeps the walk order inside a face; the carried faces and where their pixels start ----
  if (!take(g.pixel_sorted, sizeof(long long) * S, "the grouped pixels", who) || !take(g.face_sorted, sizeof(unsigned) * S, "the grouped pixels' faces", who))
    return kLmError;
  unsigned end_bit = 1;
  while ((1LL << end_bit) < nf) ++end_bit;
  size_t tmp_bytes = 0;
  CAPTURE_OK(who, rocprim::radix_sort_pairs(nullptr, tmp_bytes, g.walk.face_s.as<unsigned>(), g.face_sorted.as<unsigned>(), g.walk.pixel_of.as<long long>(),
                                            g.pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  if (!take(g.sort_tmp, tmp_bytes, "the sort of the pixels by face", who)) return kLmError;
  CAPTURE_OK(who, rocprim::radix_sort_pairs(g.sort_tmp.ptr, tmp_bytes, g.walk.face_s.as<unsigned>(), g.face_sorted.as<unsigned>(),
                                            g.walk.pixel_of.as<long long>(), g.pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  if (!take(g.face_list, sizeof(int) * (size_t)nf, "the carried faces", who) ||
      !take(g.face_first, sizeof(long long) * ((size_t)nf + 1), "the faces' first pixels", who) ||
      !take(g.rank_of_face, sizeof(int) * (size_t)nf, "the faces' ranks", who) || !take(g.head, sizeof(long long) * 2, "the counts the host reads", who))
    return kLmError;
  hipLaunchKernelGGL(face_scan_kernel, dim3(1), dim3(kCT), 0, stream, g.face_pixels.as<int>(), nf, g.face_list.as<int>(), g.face_first.as<long long>(),
                     g.rank_of_face.as<int>(), g.head.as<long long>());
  CAPTURE_OK(who, hipGetLastError());
  if (ga.d_face_pixels) CAPTURE_OK(who, hipMemcpyAsync(ga.d_face_pixels, g.face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
  long long h_head[2] = {0, 0};
  CAPTURE_OK(who, hipMemcpyAsync(h_head, g.head.ptr, sizeof h_head, hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  const long long F = h_head[0];
  if (F < 1 || F > nf) {
    set_error("%s(): the grouping finds %lld carried faces of %d", who, F, nf);
    return kLmError;
  }
  if (h_head[1] * L > INT_MAX) {  // one fit's candidates: a fit's count is an int
    set_error("%s(): a face has %lld pixels, %lld candidate samples per fit: more than INT_MAX", who, h_head[1], h_head[1] * L);
    return kLmError;
  }
  if (ga.n_pixels) *ga.n_pixels = S;
  if (ga.n_faces) *ga.n_faces = F;

  // ---- cosines of the carried faces ----
  if (!take(g.angles_f, sizeof(double) * 3 * (size_t)F * L, "the carried faces' cosines", who)) return kLmError;
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, g.face_list.as<int>(), F, a.leds, L, a.view, a.rv_mode, g.angles_f.as<double>(), stream) != 0)
    return kLmError;
  g.S = S;
  g.F = F;
  g.max_pixels = h_head[1];
  return 0;
}

CandidateCtx capture_candidates(const CaptureGrouped &ga, const CaptureGroup &g) {
  const CaptureArgs &a = ga.cap;
  CandidateCtx c = {};
  c.images = a.d_images;
  c.L = a.L;
  c.H = a.H;
  c.W = a.W;
  c.pixel_sorted = g.pixel_sorted.as<long long>();
  c.face_sorted = g.face_sorted.as<unsigned>();
  c.rank_of_face = g.rank_of_face.as<int>();
  c.face_first = g.face_first.as<long long>();
  c.angles_f = g.angles_f.as<double>();
  c.T = g.S * a.L;
  c.F = (int)g.F;
  c.v_min = ga.v_min;
  c.v_max = ga.v_max;
  c.cos_min = ga.cos_min;
  c.use1 = a.model != MODEL_PHONG;
  c.use2 = a.model != MODEL_BLINN_PHONG;
  return c;
}

bool take_fit_results(FitResultBufs &b, const CaptureFacesArgs &a, size_t fits, const char *who) {
  return (!a.d_surface_info || take(b.info, sizeof(double) * kInfoSz * fits, "the fits' info", who)) &&
         (!a.d_surface_ret || take(b.ret, sizeof(int) * fits, "the fits' ret", who)) &&
         (!a.d_surface_covar || take(b.covar, sizeof(double) * kM * kM * fits, "the fits' covariances", who)) &&
         (!a.d_surface_stats || take(b.stats, sizeof(double) * kStatsSz * fits, "the fits' statistics", who)) &&
         (!a.d_surface_rank || take(b.rank, sizeof(int) * fits, "the fits' ranks", who));
}

int capture_scatter_run(const char *who, const ScatterArgs &s) {
  const CaptureFacesArgs &a = *s.a;
  const int fits = (int)(3 * s.g->F), sb = (fits + kCT - 1) / kCT;
  DevBuf sums;
  if (!take(sums, sizeof(double) * 3 * (size_t)sb, "the block sums", who)) return kLmError;
  const FitResultBufs &r = *s.res;
  const ScatterCtx sc = {(int)s.g->F, s.g->face_list.as<int>(), s.offsets, s.nobs, s.p, r.info.as<double>(), r.covar.as<double>(), r.stats.as<double>(),
                         r.ret.as<int>(), r.rank.as<int>(), s.lights, a.d_brdf_surfaces, a.d_surface_info, a.d_surface_covar, a.d_surface_stats,
                         a.d_surface_ret, a.d_surface_rank, a.d_surface_count, s.s_lights, sums.as<double>()};
  hipLaunchKernelGGL(scatter_kernel, dim3(sb), dim3(kCT), 0, a.g.cap.stream, sc);
  CAPTURE_OK(who, hipGetLastError());
  return capture_average(who, a.g.cap, sums.as<double>(), sb, a.avg);
}

}  // namespace brdf
