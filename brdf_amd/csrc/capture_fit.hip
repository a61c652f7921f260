// capture_fit.hip -- the pixel loop of CBRDFdata::CalcBRDFEquation (brdfdata.cpp:1188-1227) as a handful of launches
// (SURVEY.md section 8, row f2).
//
// The reference walks the image x-major (x outer, y inner), and for every pixel whose pixel-map entry names a face:
// rebuilds the three cosine planes of that face (:1203-1205), and for each colour channel (B, G, R) gathers the 16
// intensities of the pixel (GetIntensities_FromPixel, :945-960: row height-1-y, value / 255.0), fits them with
// dlevmar_bc_dif (SolveEquation, :1077-1136) and stores {kd, ks, n} in brdf_surfaces(face, channel)
// (SaveValuesToSurface, :368-377) -- a later pixel of the same face overwrites an earlier one.  Here:
//
//   compact   the pixels that carry a face, in the reference's own x-major order (deterministic two-pass compaction),
//             and the LAST such pixel of every face (atomicMax of the compacted index)
//   gather    x[3S][L] = image_i(H-1-y, x)[c] / 255.0 for the 3 S (pixel, channel) fits
//   cosines   angles[3S][3][L] through cosines.hip (a pixel's three channels share a face)
//   fit       ONE batched dlevmar_bc_dif launch over the 3 S fits (batch_fit.hip)
//   store     brdf_surfaces[face][channel] <- the fit of the face's last pixel; sums of kd, ks, n over all fits
//
// Everything stays in HBM between the steps; the host sees S and the three averages.
#include <vector>

#include "../../include/brdf_levmar.h"
#include "capture_group.h"
#include "fit_stats.h"

namespace brdf {

namespace {

// (the compaction and the face's last pixel: capture_group.hip, FaceStat::kLastPixel)
// fit id q = 3 s + c: the three channels of pixel s are consecutive, as in the reference's loop nest
__global__ __launch_bounds__(kCT) void gather_kernel(const unsigned char *images, int L, int H, int W, const long long *pixel_of,
                                                     const int *face_of_surfel, long long S, const double *p0, double *x,
                                                     int *faces3, double *p) {
  const long long total = 3 * S * L;
  for (long long t = (long long)blockIdx.x * kCT + threadIdx.x; t < total; t += (long long)gridDim.x * kCT) {
    const long long q = t / L;
    const int i = (int)(t - q * L);
    const long long s = q / 3;
    const int c = (int)(q - 3 * s);
    const long long g = pixel_of[s];
    const int px = (int)(g / H), py = (int)(g % H);
    const unsigned char v = images[(((size_t)i * H + (size_t)(H - 1 - py)) * W + px) * 3 + c];
    x[q * L + i] = v / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
    if (i == 0) {
      faces3[q] = face_of_surfel[s];
      p[3 * q + 0] = p0[0];
      p[3 * q + 1] = p0[1];
      p[3 * q + 2] = p0[2];
    }
  }
}

// brdf_surfaces(face, channel) <- the last pixel's fit; per-block partial sums of kd, ks, n in a fixed order
__global__ __launch_bounds__(kCT) void store_kernel(const double *p, const int *face_of_surfel, const long long *last_of_face,
                                                    long long S, double *brdf_surfaces, double *block_sums) {
  const long long q = (long long)blockIdx.x * kCT + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (q < 3 * S) {
    const long long s = q / 3;
    const int c = (int)(q - 3 * s);
    const int f = face_of_surfel[s];
    v[0] = p[3 * q];
    v[1] = p[3 * q + 1];
    v[2] = p[3 * q + 2];
    if (last_of_face[f] == s + 1) {
      double *dst = brdf_surfaces + ((size_t)f * 3 + c) * 3;
      dst[0] = v[0];
      dst[1] = v[1];
      dst[2] = v[2];
    }
  }
  block_sums3(v, block_sums);
}

// the optional statistics tail: row (face, channel) of the three maps reads the fit store_kernel's rule picks for it -- channel c
// of the face's LAST pixel -- or nothing (-1) where no pixel carries the face
__global__ __launch_bounds__(kCT) void stats_rows_kernel(const long long *last_of_face, int nf, int *src_of_row) {
  const int r = blockIdx.x * kCT + threadIdx.x;
  if (r >= 3 * nf) return;
  const int f = r / 3;
  const long long last = last_of_face[f];
  src_of_row[r] = last ? (int)(3 * (last - 1) + (r - 3 * f)) : -1;
}

// ---- the validity rule of brdf_hip_fit_capture_masked_dev --------------------------------------------------------------------
// sample i of a fit is valid iff v_min <= its 8-bit intensity <= v_max and every cosine plane the model reads is > cos_min (a NaN
// cosine is not).  x holds intensity / 255.0 (gather_kernel): rint(x * 255) is the intensity again, the product being within an ulp
// of 255 of it.
__device__ __forceinline__ bool sample_valid(double c0, double c1, double c2, double xv, int v_min, int v_max, double cos_min, int use1,
                                             int use2) {
  const int v = __double2int_rn(xv * 255.0);
  return v >= v_min && v <= v_max && c0 > cos_min && (!use1 || c1 > cos_min) && (!use2 || c2 > cos_min);
}

// L = 16: a fit is one 16-lane row of a wave.  Every lane reads its four values; a ballot and the popcount of the row's lower lanes
// give a valid sample its place at the front of the row (stable in light order); then the lanes write.  A row is read and written by
// its own sixteen lanes only, and a wave's loads of a plane have all returned before its stores to that plane issue: in place is safe.
__global__ __launch_bounds__(kCT) void mask_rows16_kernel(double *angles, double *x, long long Q, int v_min, int v_max, double cos_min,
                                                          int use1, int use2, int *counts) {
  const long long q = ((long long)blockIdx.x * kCT + threadIdx.x) >> 4;
  const int i = threadIdx.x & 15, lane = threadIdx.x & 63;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, vx = 0.0;
  bool valid = false;
  double *a = angles + (size_t)(q < Q ? q : 0) * 48, *xr = x + (size_t)(q < Q ? q : 0) * 16;
  if (q < Q) {
    v0 = a[i];
    v1 = a[16 + i];
    v2 = a[32 + i];
    vx = xr[i];
    valid = sample_valid(v0, v1, v2, vx, v_min, v_max, cos_min, use1, use2);
  }
  const unsigned long long m = __ballot(valid);
  const unsigned row = (unsigned)(m >> (lane & 48)) & 0xffffu;
  if (valid) {
    const int d = __popc(row & ((1u << i) - 1u));
    a[d] = v0;
    a[16 + d] = v1;
    a[32 + d] = v2;
    xr[d] = vx;
  }
  if (q < Q && i == 0) counts[q] = __popc(row);
}

// any other L <= 64: one thread per fit, a serial walk (the write index never passes the read index)
__global__ __launch_bounds__(kCT) void mask_serial_kernel(double *angles, double *x, long long Q, int L, int v_min, int v_max,
                                                          double cos_min, int use1, int use2, int *counts) {
  const long long q = (long long)blockIdx.x * kCT + threadIdx.x;
  if (q >= Q) return;
  double *a = angles + (size_t)q * 3 * L, *xr = x + (size_t)q * L;
  int w = 0;
  for (int i = 0; i < L; ++i) {
    const double v0 = a[i], v1 = a[L + i], v2 = a[2 * L + i], vx = xr[i];
    if (!sample_valid(v0, v1, v2, vx, v_min, v_max, cos_min, use1, use2)) continue;
    a[w] = v0;
    a[L + w] = v1;
    a[2 * L + w] = v2;
    xr[w] = vx;
    ++w;
  }
  counts[q] = w;
}

// surface_count(face, channel) <- the sample count of the fit store_kernel's rule stores for it
__global__ __launch_bounds__(kCT) void count_map_kernel(const long long *last_of_face, int nf, const int *counts, int *surface_count) {
  const int r = blockIdx.x * kCT + threadIdx.x;
  if (r >= 3 * nf) return;
  const int f = r / 3;
  const long long last = last_of_face[f];
  if (last) surface_count[r] = counts[3 * (last - 1) + (r - 3 * f)];
}

// ---- single-BRDF variant (CalcBRDFEquation_SingleBRDF, brdfdata.cpp:1138-1186) --------------------------------
__global__ __launch_bounds__(kCT) void face_count_kernel(const long long *last_of_face, int nf, int *block_count) {
  __shared__ int wave_cnt[kCT / 64];
  const int f = blockIdx.x * kCT + threadIdx.x;
  const bool valid = f < nf && last_of_face[f] != 0;
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// the faces some pixel carries, in face order, each with the x-major index of its LAST pixel
__global__ __launch_bounds__(kCT) void face_compact_kernel(const long long *last_of_face, const long long *pixel_of, int nf,
                                                           const long long *block_offset, int *face_list, long long *pixel_list) {
  __shared__ int wave_cnt[kCT / 64];
  const int f = blockIdx.x * kCT + threadIdx.x;
  const bool valid = f < nf && last_of_face[f] != 0;
  const unsigned long long m = __ballot(valid);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  if (!valid) return;
  long long r = block_offset[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) r += wave_cnt[w];
  face_list[r] = f;
  pixel_list[r] = pixel_of[last_of_face[f] - 1];
}

// one fit over all F faces x L lights: planes[3][F*L] (face-major inside a plane, "x[i*m_numImages+j] = I(i,j)",
// brdfdata.cpp:1016) from the per-face planes of cosines.hip, and the measurements of the three channels x3[3][F*L]
__global__ __launch_bounds__(kCT) void single_pack_kernel(const unsigned char *images, int L, int H, int W, const long long *pixel_list,
                                                          const double *angles_f, long long F, double *planes, double *x3) {
  const long long n = F * L;
  for (long long t = (long long)blockIdx.x * kCT + threadIdx.x; t < n; t += (long long)gridDim.x * kCT) {
    const long long r = t / L;
    const int i = (int)(t - r * L);
    const long long g = pixel_list[r];
    const int px = (int)(g / H), py = (int)(g % H);
#pragma unroll
    for (int k = 0; k < 3; ++k) planes[k * n + t] = angles_f[(r * 3 + k) * L + i];
    const unsigned char *pxl = images + (((size_t)i * H + (size_t)(H - 1 - py)) * W + px) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) x3[c * n + t] = pxl[c] / 255.0;
  }
}

}  // namespace

int capture_fit_run(const CaptureFitArgs &fa) {
  const CaptureArgs &a = fa.cap;
  const CaptureMask *mask = fa.mask;
  const int model = a.model, L = a.L, nf = a.nf;
  hipStream_t stream = a.stream;
  const bool want_stats = fa.d_surface_covar || fa.d_surface_stats || fa.d_surface_rank;
  const char *who = mask ? "brdf_hip_fit_capture_masked_dev" : (want_stats ? "brdf_hip_fit_capture_stats_dev" : "brdf_hip_fit_capture_dev");
  if (mask && (mask->v_min > mask->v_max || mask->cos_min != mask->cos_min || model < 0 || model >= MODEL_COUNT)) {
    set_error("%s(): bad validity rule (v_min %d > v_max %d, or cos_min not a number) or unknown model %d", who, mask->v_min, mask->v_max, model);
    return kLmError;
  }
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !fa.d_brdf_surfaces ||
      L <= 0 || L > 64 || a.H <= 0 || a.W <= 0 || nf <= 0) {
    set_error("%s(): bad arguments", who);
    return kLmError;
  }
  if (want_stats && (L < kM || nf > 0x7fffffff / 3)) {  // before anything runs: a covariance needs n >= 3 samples; the maps have 3 nf rows
    set_error("%s(): L = %d, nf = %d: the statistics maps need L >= %d images and 3 nf <= 2^31-1", who, L, nf, kM);
    return kLmError;
  }
  (void)hipGetLastError();
  DevBuf last;
  CAPTURE_OK(who, last.ensure(sizeof(long long) * nf));
  CAPTURE_OK(who, hipMemsetAsync(last.ptr, 0, sizeof(long long) * nf, stream));
  PixelCompaction walk;
  walk.stat = FaceStat::kLastPixel;
  walk.d_face_stat = last.ptr;
  walk.max_S = 0x7fffffffLL / 3;  // 3 S fits
  if (capture_compact_run(who, a, walk) != 0) return kLmError;
  const long long S = walk.S;
  if (fa.n_pixels) *fa.n_pixels = S;
  if (fa.avg) fa.avg[0] = fa.avg[1] = fa.avg[2] = 0.0;
  if (S == 0) return 0;
  if (S > walk.max_S) {
    set_error("%s(): %lld pixels carry a face; the batched fitter takes at most 2^31-1 fits per call", who, S);
    return kLmError;
  }
  DevBuf &pixel_of = walk.pixel_of, &face_s = walk.face_s;
  DevBuf faces3, x, p, angles, ret, p0d, sums;
  CAPTURE_OK(who, faces3.ensure(sizeof(int) * 3 * S));
  CAPTURE_OK(who, x.ensure(sizeof(double) * 3 * S * L));
  CAPTURE_OK(who, p.ensure(sizeof(double) * 9 * S));
  CAPTURE_OK(who, angles.ensure(sizeof(double) * 9 * S * L));
  CAPTURE_OK(who, ret.ensure(sizeof(int) * 3 * S));
  CAPTURE_OK(who, p0d.ensure(sizeof(double) * 3));
  CAPTURE_OK(who, hipMemcpyAsync(p0d.ptr, a.p0, sizeof(double) * 3, hipMemcpyHostToDevice, stream));
  long long gb = (3 * S * L + kCT - 1) / kCT;
  if (gb > 256 * 64) gb = 256 * 64;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)gb), dim3(kCT), 0, stream, a.d_images, L, a.H, a.W, pixel_of.as<long long>(),
                     face_s.as<int>(), S, p0d.as<double>(), x.as<double>(), faces3.as<int>(), p.as<double>());
  CAPTURE_OK(who, hipGetLastError());
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, faces3.as<int>(), 3 * S, a.leds, L, a.view, a.rv_mode, angles.as<double>(), stream) != 0)
    return kLmError;
  DevBuf fit_counts;
  if (mask) {  // valid samples to the front of every fit's rows, in place; the fits below are ragged
    const long long Q = 3 * S;
    const int use1 = model != MODEL_PHONG, use2 = model != MODEL_BLINN_PHONG;  // the planes the model reads (brdf_models.h: uses_c1, uses_c2)
    CAPTURE_OK(who, fit_counts.ensure(sizeof(int) * Q));
    if (L == 16)
      hipLaunchKernelGGL(mask_rows16_kernel, dim3((unsigned)((Q * 16 + kCT - 1) / kCT)), dim3(kCT), 0, stream, angles.as<double>(), x.as<double>(), Q,
                         mask->v_min, mask->v_max, mask->cos_min, use1, use2, fit_counts.as<int>());
    else
      hipLaunchKernelGGL(mask_serial_kernel, dim3((unsigned)((Q + kCT - 1) / kCT)), dim3(kCT), 0, stream, angles.as<double>(), x.as<double>(), Q, L,
                         mask->v_min, mask->v_max, mask->cos_min, use1, use2, fit_counts.as<int>());
    CAPTURE_OK(who, hipGetLastError());
  }
  // dlevmar_bc_dif: brdfdata.cpp:1119; no info; with a mask the fits are ragged
  const BatchFitArgs b = {BRDF_METHOD_BC_DIF, model, angles.as<double>(), x.as<double>(), (int)(3 * S), L, p.as<double>(), a.lb, a.ub, a.itmax, a.opts,
                          nullptr, ret.as<int>(), stream, mask ? fit_counts.as<int>() : nullptr};
  if (batch_fit_enqueue(b, who) != 0) return kLmError;
  const int sb = (int)((3 * S + kCT - 1) / kCT);
  CAPTURE_OK(who, sums.ensure(sizeof(double) * 3 * sb));
  hipLaunchKernelGGL(store_kernel, dim3(sb), dim3(kCT), 0, stream, p.as<double>(), face_s.as<int>(), last.as<long long>(), S,
                     fa.d_brdf_surfaces, sums.as<double>());
  CAPTURE_OK(who, hipGetLastError());
  if (mask && mask->d_surface_count) {
    hipLaunchKernelGGL(count_map_kernel, dim3((3 * nf + kCT - 1) / kCT), dim3(kCT), 0, stream, last.as<long long>(), nf, fit_counts.as<int>(),
                       mask->d_surface_count);
    CAPTURE_OK(who, hipGetLastError());
  }
  DevBuf src_of_row;
  if (want_stats) {  // the staged angles / x / p are still in HBM: one pass over the stored fits
    CAPTURE_OK(who, src_of_row.ensure(sizeof(int) * 3 * (size_t)nf));
    hipLaunchKernelGGL(stats_rows_kernel, dim3((3 * nf + kCT - 1) / kCT), dim3(kCT), 0, stream, last.as<long long>(), nf, src_of_row.as<int>());
    CAPTURE_OK(who, hipGetLastError());
    const FitStatsArgs fs = {b.method, model, b.d_angles, b.d_x, b.S, L, b.d_p, a.opts, fa.d_surface_covar, fa.d_surface_stats, fa.d_surface_rank,
                             src_of_row.as<int>(), 3 * nf, stream, b.d_counts};
    if (fit_stats_enqueue(fs, who) != 0) return kLmError;
  }
  return capture_average(who, a, sums.as<double>(), sb, fa.avg);
}


// CalcBRDFEquation_SingleBRDF (brdfdata.cpp:1138-1186) + SolveEquation_SingleBRDF (:992-1062): ONE parameter triple per
// colour channel, fitted to the 16 samples of EVERY face the pixel map shows (n = 16 x faces; bunny: 402,928).  The
// reference fills phi/thetaDash/theta/I only for the faces some pixel carries and leaves the other rows of its
// matrices uninitialised, then pairs x (face-major) with planes read through a column-major linear index (:1031): both
// slips are not reproduced -- the fit sees exactly the carried faces, samples and measurements paired.
int capture_fit_single_run(const CaptureSingleArgs &sa) {
  static const char *const who = "brdf_hip_fit_capture_single_dev";
  const CaptureArgs &a = sa.cap;
  const int L = a.L, nf = a.nf;
  hipStream_t stream = a.stream;
  if (!a.d_images || !a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !a.p0 || !sa.single_brdf || L <= 0 ||
      L > 64 || a.H <= 0 || a.W <= 0 || nf <= 0) {
    set_error("%s(): bad arguments", who);
    return kLmError;
  }
  (void)hipGetLastError();
  const int fb = (nf + kCT - 1) / kCT;
  DevBuf last, fcounts, foffsets;
  CAPTURE_OK(who, last.ensure(sizeof(long long) * nf));
  CAPTURE_OK(who, fcounts.ensure(sizeof(int) * fb));
  CAPTURE_OK(who, foffsets.ensure(sizeof(long long) * fb));
  CAPTURE_OK(who, hipMemsetAsync(last.ptr, 0, sizeof(long long) * nf, stream));
  PixelCompaction walk;
  walk.stat = FaceStat::kLastPixel;
  walk.d_face_stat = last.ptr;
  walk.max_S = (long long)a.H * a.W;  // no limit of this entry's own
  if (capture_compact_run(who, a, walk) != 0) return kLmError;
  if (sa.n_faces_used) *sa.n_faces_used = 0;
  if (walk.S == 0) {
    set_error("%s(): no pixel carries a face", who);
    return kLmError;
  }
  hipLaunchKernelGGL(face_count_kernel, dim3(fb), dim3(kCT), 0, stream, last.as<long long>(), nf, fcounts.as<int>());
  std::vector<int> h_fc(fb);
  CAPTURE_OK(who, hipMemcpyAsync(h_fc.data(), fcounts.ptr, sizeof(int) * fb, hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  std::vector<long long> h_fo(fb);
  long long F = 0;
  for (int b = 0; b < fb; ++b) {
    h_fo[b] = F;
    F += h_fc[b];
  }
  if (sa.n_faces_used) *sa.n_faces_used = F;
  const long long n = F * L;
  if (n > 0x7fffffffLL) {
    set_error("%s(): %lld samples exceed one fit's index range", who, n);
    return kLmError;
  }
  CAPTURE_OK(who, hipMemcpyAsync(foffsets.ptr, h_fo.data(), sizeof(long long) * fb, hipMemcpyHostToDevice, stream));
  DevBuf face_list, pixel_list, angles_f, planes, x3;
  CAPTURE_OK(who, face_list.ensure(sizeof(int) * F));
  CAPTURE_OK(who, pixel_list.ensure(sizeof(long long) * F));
  CAPTURE_OK(who, angles_f.ensure(sizeof(double) * 3 * n));
  CAPTURE_OK(who, planes.ensure(sizeof(double) * 3 * n));
  CAPTURE_OK(who, x3.ensure(sizeof(double) * 3 * n));
  hipLaunchKernelGGL(face_compact_kernel, dim3(fb), dim3(kCT), 0, stream, last.as<long long>(), walk.pixel_of.as<long long>(), nf,
                     foffsets.as<long long>(), face_list.as<int>(), pixel_list.as<long long>());
  CAPTURE_OK(who, hipGetLastError());
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, face_list.as<int>(), F, a.leds, L, a.view, a.rv_mode, angles_f.as<double>(), stream) != 0)
    return kLmError;
  long long gb = (n + kCT - 1) / kCT;
  if (gb > 256 * 64) gb = 256 * 64;
  hipLaunchKernelGGL(single_pack_kernel, dim3((unsigned)gb), dim3(kCT), 0, stream, a.d_images, L, a.H, a.W, pixel_list.as<long long>(),
                     angles_f.as<double>(), F, planes.as<double>(), x3.as<double>());
  CAPTURE_OK(who, hipGetLastError());
  // "do the calculation once for each color-channel", brdfdata.cpp:1161: three dlevmar_bc_dif fits (:1058) over the SAME planes --
  // one shared resident launch where the fit fits the chip (channels_fit_impl.h), one fit after the other otherwise
  double p3[9];
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 3; ++k) p3[3 * c + k] = a.p0[k];
  const int worst = channels_fit_run(BRDF_METHOD_BC_DIF, a.model, planes.as<double>(), x3.as<double>(), n, (int)n, 3, p3, a.lb, a.ub, nullptr, a.itmax,
                                     a.opts, sa.info, nullptr, stream);
  for (int k = 0; k < 9; ++k) sa.single_brdf[k] = p3[k];
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  return worst;
}

}  // namespace brdf
