// capture_faces.hip -- brdf_hip_fit_capture_faces_dev: ONE fit per (face, channel) over the samples of ALL the face's pixels, where
// the capture loop of capture_fit.hip fits every pixel and keeps the face's last one.  No fit or statistics kernel of its own: the
// capture becomes a packed batch (packed_fit.h) on the device, the packed calls fit it, a scatter fills the [nf][3] maps.
//
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
#include <climits>
#include <cstring>  // (in front of rocPRIM, whose headers use memset without it)
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/brdf_levmar.h"
#include "capture_compact.h"
#include "fit_host.h"
#include "fit_stats.h"
#include "packed_fit.h"

namespace brdf {

namespace {

constexpr const char *kWho = "brdf_hip_fit_capture_faces_dev";
constexpr int kWaves = kCT / kWave;

// pass 2 of the pixel compaction, as capture_fit.hip's compact_kernel; instead of a face's last pixel it counts the face's pixels
__global__ __launch_bounds__(kCT) void compact_faces_kernel(const int *pm, int H, int W, int nf, const long long *block_offset,
                                                            long long *pixel_of, unsigned *face_of_surfel, int *face_pixels) {
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
  atomicAdd(face_pixels + f, 1);
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

using DevBuf = DeviceBlock<char>;  // scoped: bytes

#define FACES_OK(call)                                                        \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", kWho, #call, hipGetErrorString(e_));   \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

// `bytes` of device memory for `what`; a failure names the bytes asked for
bool take(DevBuf &b, size_t bytes, const char *what) {
  const hipError_t e = b.ensure(bytes);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  set_error("%s(): cannot allocate %zu bytes for %s: %s", kWho, bytes, what, hipGetErrorString(e));
  return false;
}

// what the entry refuses before any HIP call
int capture_faces_check(const CaptureFacesArgs &a) {
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !a.d_brdf_surfaces) {
    set_error("%s(): null images, pixel map, mesh, leds, view origin, p0 or brdf_surfaces", kWho);
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
  if (a.workspace_bytes < 0) {
    set_error("%s(): workspace_bytes = %lld: need workspace_bytes >= 0", kWho, a.workspace_bytes);
    return kLmError;
  }
  if (box_refused(ms, a.lb, a.ub, kWho)) return kLmError;
  return 0;
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

  // ---- compact: the pixels that carry a face, in walk order ----
  const long long npx = (long long)H * W;
  if ((npx + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): H x W = %lld pixels are more than one launch walks", kWho, npx);
    return kLmError;
  }
  const int nb = (int)((npx + kCT - 1) / kCT);
  DevBuf counts, block_off, face_pixels;
  if (!take(counts, sizeof(int) * nb, "the pixel blocks' counts") || !take(block_off, sizeof(long long) * nb, "the pixel blocks' offsets") ||
      !take(face_pixels, sizeof(int) * (size_t)nf, "the faces' pixel counts"))
    return kLmError;
  FACES_OK(hipMemsetAsync(face_pixels.ptr, 0, sizeof(int) * (size_t)nf, stream));
  hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kCT), 0, stream, a.d_pixel_map, H, W, nf, counts.as<int>());
  FACES_OK(hipGetLastError());
  std::vector<int> h_counts(nb);
  FACES_OK(hipMemcpyAsync(h_counts.data(), counts.ptr, sizeof(int) * nb, hipMemcpyDeviceToHost, stream));
  FACES_OK(hipStreamSynchronize(stream));
  std::vector<long long> h_off(nb);
  long long S = 0;
  for (int b = 0; b < nb; ++b) {
    h_off[b] = S;
    S += h_counts[b];
  }
  if (S == 0) {  // an empty capture: nothing is written but the pixel counts
    if (a.d_face_pixels) FACES_OK(hipMemcpyAsync(a.d_face_pixels, face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
    FACES_OK(hipStreamSynchronize(stream));
    return 0;
  }
  const long long T = S * L;  // candidates of one channel
  if (S > INT_MAX || (T + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): %lld pixels carry a face, %lld candidates per channel: more than one launch walks", kWho, S, T);
    return kLmError;
  }
  FACES_OK(hipMemcpyAsync(block_off.ptr, h_off.data(), sizeof(long long) * nb, hipMemcpyHostToDevice, stream));
  DevBuf pixel_of, face_s, pixel_sorted, face_sorted, sort_tmp;
  if (!take(pixel_of, sizeof(long long) * S, "the carried pixels") || !take(face_s, sizeof(unsigned) * S, "the carried pixels' faces") ||
      !take(pixel_sorted, sizeof(long long) * S, "the grouped pixels") || !take(face_sorted, sizeof(unsigned) * S, "the grouped pixels' faces"))
    return kLmError;
  hipLaunchKernelGGL(compact_faces_kernel, dim3(nb), dim3(kCT), 0, stream, a.d_pixel_map, H, W, nf, block_off.as<long long>(),
                     pixel_of.as<long long>(), face_s.as<unsigned>(), face_pixels.as<int>());
  FACES_OK(hipGetLastError());

  // ---- group: a stable sort by face keeps the walk order inside a face; the carried faces and where their pixels start ----
  unsigned end_bit = 1;
  while ((1LL << end_bit) < nf) ++end_bit;
  size_t tmp_bytes = 0;
  FACES_OK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, face_s.as<unsigned>(), face_sorted.as<unsigned>(), pixel_of.as<long long>(),
                                     pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  if (!take(sort_tmp, tmp_bytes, "the sort of the pixels by face")) return kLmError;
  FACES_OK(rocprim::radix_sort_pairs(sort_tmp.ptr, tmp_bytes, face_s.as<unsigned>(), face_sorted.as<unsigned>(), pixel_of.as<long long>(),
                                     pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  DevBuf face_list, face_first, rank_of_face, head;
  if (!take(face_list, sizeof(int) * (size_t)nf, "the carried faces") || !take(face_first, sizeof(long long) * ((size_t)nf + 1), "the faces' first pixels") ||
      !take(rank_of_face, sizeof(int) * (size_t)nf, "the faces' ranks") || !take(head, sizeof(long long) * 3, "the counts the host reads"))
    return kLmError;
  hipLaunchKernelGGL(face_scan_kernel, dim3(1), dim3(kCT), 0, stream, face_pixels.as<int>(), nf, face_list.as<int>(), face_first.as<long long>(),
                     rank_of_face.as<int>(), head.as<long long>());
  FACES_OK(hipGetLastError());
  if (a.d_face_pixels) FACES_OK(hipMemcpyAsync(a.d_face_pixels, face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
  long long h_head[2] = {0, 0};
  FACES_OK(hipMemcpyAsync(h_head, head.ptr, sizeof h_head, hipMemcpyDeviceToHost, stream));
  FACES_OK(hipStreamSynchronize(stream));
  const long long F = h_head[0];
  if (F < 1 || F > nf) {
    set_error("%s(): the grouping finds %lld carried faces of %d", kWho, F, nf);
    return kLmError;
  }
  if (h_head[1] * L > INT_MAX) {  // one fit's candidates: a fit's count is an int
    set_error("%s(): a face has %lld pixels, %lld candidate samples per fit: more than INT_MAX", kWho, h_head[1], h_head[1] * L);
    return kLmError;
  }
  if (a.n_pixels) *a.n_pixels = S;
  if (a.n_faces) *a.n_faces = F;

  // ---- cosines of the carried faces ----
  DevBuf angles_f;
  if (!take(angles_f, sizeof(double) * 3 * (size_t)F * L, "the carried faces' cosines")) return kLmError;
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, face_list.as<int>(), F, a.leds, L, a.view, a.rv_mode, angles_f.as<double>(), stream) != 0)
    return kLmError;

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
