// capture_group.h -- the grouping the per-face captures share (capture_faces.hip, capture_means.hip): the pixels that carry a face,
// grouped by face, and the carried faces' cosines.
//
//   compact   the pixels that carry a face, in the reference's x-major walk (the two-pass compaction of capture_fit.hip), and the
//             number of pixels of every face (integer adds: their order cannot show)
//   group     a stable radix sort of the compacted pixels by face (rocPRIM; walk order kept inside a face); one scan over the faces
//             gives the carried faces in ascending order, each with its first sorted pixel
//   cosines   angles_f[F][3][L] of the F carried faces (cosines.hip): all pixels of a face share them
// Host code and two kernels, in an unnamed namespace: each of the two translation units has its own copy.
#pragma once

#include <climits>
#include <cstring>  // (in front of rocPRIM, whose headers use memset without it)
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "capture_compact.h"
#include "fit_host.h"

namespace brdf {

namespace {

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

using DevBuf = DeviceBlock<char>;  // scoped: bytes

#define GROUP_OK(call)                                                        \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", who, #call, hipGetErrorString(e_));    \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

// `bytes` of device memory for `what`; a failure names the entry `who` and the bytes asked for
bool take(DevBuf &b, size_t bytes, const char *what, const char *who) {
  const hipError_t e = b.ensure(bytes);
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  set_error("%s(): cannot allocate %zu bytes for %s: %s", who, bytes, what, hipGetErrorString(e));
  return false;
}

// What the per-face captures refuse before any HIP call, under the entry's name `who`: a null required pointer, L outside [1, max_L]
// (`l_note`: what the text says about the bound), H, W or nf <= 0, 3 nf > INT_MAX, an unknown model, a bad validity rule, lb > ub.
int capture_args_check(const char *who, const CaptureFacesArgs &a, int max_L, const char *l_note) {
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !a.d_brdf_surfaces) {
    set_error("%s(): null images, pixel map, mesh, leds, view origin, p0 or brdf_surfaces", who);
    return kLmError;
  }
  if (a.L < 1 || a.L > max_L || a.H <= 0 || a.W <= 0 || a.nf <= 0 || a.nf > INT_MAX / 3) {
    set_error("%s(): L = %d, H = %d, W = %d, nf = %d: need 1 <= L <= %d%s, H, W, nf > 0 and 3 nf <= INT_MAX", who, a.L, a.H, a.W, a.nf, max_L, l_note);
    return kLmError;
  }
  MethodSpec ms;
  if (!known_model_method(a.model, BRDF_METHOD_BC_DIF, &ms, who)) return kLmError;
  if (a.v_min > a.v_max || a.cos_min != a.cos_min) {
    set_error("%s(): bad validity rule (v_min %d > v_max %d, or cos_min not a number)", who, a.v_min, a.v_max);
    return kLmError;
  }
  return box_refused(ms, a.lb, a.ub, who) ? kLmError : 0;
}

// what capture_group_run leaves: S carried pixels grouped by face, F carried faces (S == 0: an empty capture, nothing else is set)
struct CaptureGroup {
  long long S = 0, F = 0, max_pixels = 0;  // max_pixels: the pixels of the largest face
  DevBuf counts, block_off, face_pixels;   // the pixel blocks' counts and offsets; [nf]: the faces' pixel counts
  DevBuf pixel_of, face_s, sort_tmp;       // the carried pixels in walk order, their faces, the sort's scratch
  DevBuf pixel_sorted, face_sorted;        // [S] long long: x-major pixel index, grouped by face; [S] unsigned: its face
  DevBuf face_list, face_first, rank_of_face;  // [F] int ascending; [F + 1] long long; [nf] int (-1: no pixel carries the face)
  DevBuf head;                             // 3 long long: {F, max_pixels, one more word for the caller}
  DevBuf angles_f;                         // [F][3][L] double
};

// Groups the capture `a` for the entry `who` and waits for a.stream.  Writes a.d_face_pixels (where asked for) and the host scalars
// n_pixels and n_faces.  0, or kLmError with the error text; g.S == 0 on return 0: no pixel carries a face, the caller is done.
int capture_group_run(const char *who, const CaptureFacesArgs &a, CaptureGroup &g) {
  hipStream_t stream = a.stream;
  const int L = a.L, H = a.H, W = a.W, nf = a.nf;
  // ---- compact: the pixels that carry a face, in walk order ----
  const long long npx = (long long)H * W;
  if ((npx + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): H x W = %lld pixels are more than one launch walks", who, npx);
    return kLmError;
  }
  const int nb = (int)((npx + kCT - 1) / kCT);
  if (!take(g.counts, sizeof(int) * nb, "the pixel blocks' counts", who) || !take(g.block_off, sizeof(long long) * nb, "the pixel blocks' offsets", who) ||
      !take(g.face_pixels, sizeof(int) * (size_t)nf, "the faces' pixel counts", who))
    return kLmError;
  GROUP_OK(hipMemsetAsync(g.face_pixels.ptr, 0, sizeof(int) * (size_t)nf, stream));
  hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(kCT), 0, stream, a.d_pixel_map, H, W, nf, g.counts.as<int>());
  GROUP_OK(hipGetLastError());
  std::vector<int> h_counts(nb);
  GROUP_OK(hipMemcpyAsync(h_counts.data(), g.counts.ptr, sizeof(int) * nb, hipMemcpyDeviceToHost, stream));
  GROUP_OK(hipStreamSynchronize(stream));
  std::vector<long long> h_off(nb);
  long long S = 0;
  for (int b = 0; b < nb; ++b) {
    h_off[b] = S;
    S += h_counts[b];
  }
  if (S == 0) {  // an empty capture: nothing is written but the pixel counts
    if (a.d_face_pixels) GROUP_OK(hipMemcpyAsync(a.d_face_pixels, g.face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
    GROUP_OK(hipStreamSynchronize(stream));
    return 0;
  }
  const long long T = S * L;  // candidates of one channel
  if (S > INT_MAX || (T + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): %lld pixels carry a face, %lld candidates per channel: more than one launch walks", who, S, T);
    return kLmError;
  }
  GROUP_OK(hipMemcpyAsync(g.block_off.ptr, h_off.data(), sizeof(long long) * nb, hipMemcpyHostToDevice, stream));
  if (!take(g.pixel_of, sizeof(long long) * S, "the carried pixels", who) || !take(g.face_s, sizeof(unsigned) * S, "the carried pixels' faces", who) ||
      !take(g.pixel_sorted, sizeof(long long) * S, "the grouped pixels", who) || !take(g.face_sorted, sizeof(unsigned) * S, "the grouped pixels' faces", who))
    return kLmError;
  hipLaunchKernelGGL(compact_faces_kernel, dim3(nb), dim3(kCT), 0, stream, a.d_pixel_map, H, W, nf, g.block_off.as<long long>(),
                     g.pixel_of.as<long long>(), g.face_s.as<unsigned>(), g.face_pixels.as<int>());
  GROUP_OK(hipGetLastError());

  // ---- group: a stable sort by face keeps the walk order inside a face; the carried faces and where their pixels start ----
  unsigned end_bit = 1;
  while ((1LL << end_bit) < nf) ++end_bit;
  size_t tmp_bytes = 0;
  GROUP_OK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, g.face_s.as<unsigned>(), g.face_sorted.as<unsigned>(), g.pixel_of.as<long long>(),
                                     g.pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  if (!take(g.sort_tmp, tmp_bytes, "the sort of the pixels by face", who)) return kLmError;
  GROUP_OK(rocprim::radix_sort_pairs(g.sort_tmp.ptr, tmp_bytes, g.face_s.as<unsigned>(), g.face_sorted.as<unsigned>(), g.pixel_of.as<long long>(),
                                     g.pixel_sorted.as<long long>(), (size_t)S, 0u, end_bit, stream));
  if (!take(g.face_list, sizeof(int) * (size_t)nf, "the carried faces", who) ||
      !take(g.face_first, sizeof(long long) * ((size_t)nf + 1), "the faces' first pixels", who) ||
      !take(g.rank_of_face, sizeof(int) * (size_t)nf, "the faces' ranks", who) || !take(g.head, sizeof(long long) * 3, "the counts the host reads", who))
    return kLmError;
  hipLaunchKernelGGL(face_scan_kernel, dim3(1), dim3(kCT), 0, stream, g.face_pixels.as<int>(), nf, g.face_list.as<int>(), g.face_first.as<long long>(),
                     g.rank_of_face.as<int>(), g.head.as<long long>());
  GROUP_OK(hipGetLastError());
  if (a.d_face_pixels) GROUP_OK(hipMemcpyAsync(a.d_face_pixels, g.face_pixels.ptr, sizeof(int) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
  long long h_head[2] = {0, 0};
  GROUP_OK(hipMemcpyAsync(h_head, g.head.ptr, sizeof h_head, hipMemcpyDeviceToHost, stream));
  GROUP_OK(hipStreamSynchronize(stream));
  const long long F = h_head[0];
  if (F < 1 || F > nf) {
    set_error("%s(): the grouping finds %lld carried faces of %d", who, F, nf);
    return kLmError;
  }
  if (h_head[1] * L > INT_MAX) {  // one fit's candidates: a fit's count is an int
    set_error("%s(): a face has %lld pixels, %lld candidate samples per fit: more than INT_MAX", who, h_head[1], h_head[1] * L);
    return kLmError;
  }
  if (a.n_pixels) *a.n_pixels = S;
  if (a.n_faces) *a.n_faces = F;

  // ---- cosines of the carried faces ----
  if (!take(g.angles_f, sizeof(double) * 3 * (size_t)F * L, "the carried faces' cosines", who)) return kLmError;
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, g.face_list.as<int>(), F, a.leds, L, a.view, a.rv_mode, g.angles_f.as<double>(), stream) != 0)
    return kLmError;
  g.S = S;
  g.F = F;
  g.max_pixels = h_head[1];
  return 0;
}

#undef GROUP_OK

}  // namespace

}  // namespace brdf
