// capture_render.hip -- parameters back into images: what the reference program shades the mesh with, in the captures' own layout.
//   brdf_hip_capture_render_dev            the model at the fitted surfaces under ANY lights: the value table and 8-bit BGR images
//   brdf_hip_capture_render_residuals_dev  captures minus rendered grey levels as integer maps: per light, per (face, light), per pixel
//   brdf_hip_surfaces_from_materials_dev   surfaces[f] = materials[label[f]]: labelled and single-BRDF results as surfaces
// No fit or statistics kernel.  All pixels of a face share the face's cosines, so a prediction depends on (face, channel, light) alone:
//
//   values     cosines.hip's planes of ALL nf faces under the call's lights, then one lane per (face, channel, light): the model on
//              the exact path -- model_eval_kernel's operations on the same operands, so brdf_hip_model_eval_dev's bytes -- and its
//              grey level q = clamp((int)(255 v + 0.5)) into a byte table grey[nf][3][L] that both passes gather through L2.
//   render     a pure store stream: an image's bytes between its first and last 16-byte boundary go out as 16-byte stores, one chunk
//              per lane and consecutive lanes on consecutive chunks; the image's two ends, and chunks that hold a pixel the call
//              leaves untouched (background -1), go out byte by byte.  (Rows of 3 W bytes need not be dword-aligned; an image is
//              H rows back to back, so only its ends are ragged.)  A chunk walks its 5 to 7 pixels along the image row: one read of
//              the pixel map per pixel, one byte of the table per channel.
//   residuals  capture_group.hip's grouping (pixels sorted by face) and capture_compact.h's candidate reader, tiles of kCT / L WHOLE
//              pixels: a tile's (face, channel, light) words -- count, sum d, sum d^2 -- are LDS integer atomics, a pixel's L
//              candidates meet in one LDS word per channel (atomicMax of |d| << 8 | 255 - light: the largest |d|, the lowest light on
//              a tie) and are written by the tile itself, the touched face words go out as one global integer atomic each, and on
//              the way into the workgroup's per-light words, which go out once per workgroup.  The images are read once.  Integer
//              adds: their order cannot show; no float atomics.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/brdf_levmar.h"
#include "capture_group.h"

namespace brdf {

namespace {

constexpr const char *kWhoRender = "brdf_hip_capture_render_dev", *kWhoResiduals = "brdf_hip_capture_render_residuals_dev",
                     *kWhoSurfaces = "brdf_hip_surfaces_from_materials_dev";
constexpr int kRenderMaxL = 64;
constexpr int kChunk = 16;                  // bytes of a render store
constexpr int kTileWords = 3 * kCT;         // a tile holds kCT / L whole pixels, so at most that many faces with 3 L words each
constexpr int kLightWords = 3 * kRenderMaxL;
constexpr unsigned kMaxBlocks = 256 * 8;    // the grid of the passes that stride

// t = 255.0 * v + 0.5;  q = !(t >= 0) ? 0 : (t >= 256.0 ? 255 : (int)t): a NaN gives 0   (-ffp-contract=off: a product, then a sum)
__device__ __forceinline__ int grey_level(double v) {
  const double t = 255.0 * v + 0.5;
  return !(t >= 0.0) ? 0 : (t >= 256.0 ? 255 : (int)t);
}

// ---- values -----------------------------------------------------------------------------------------------------------------------
struct ValueCtx {
  const double *angles;    // [nf][3][L]
  const double *surfaces;  // [nf][3][3]
  long long words;         // 3 nf L
  int L;
  double *values;          // [nf][3][L] or null
  unsigned char *grey;     // [nf][3][L]
};

// One lane per (face, channel, light): model_eval_kernel's value (stream_fit.hip) at surfaces[face][channel] on the face's triple
template <int MODEL>
__global__ __launch_bounds__(kCT) void face_values_kernel(ValueCtx c) {
  using Mdl = BrdfModel<MODEL>;
  const long long e = (long long)blockIdx.x * kCT + threadIdx.x;
  if (e >= c.words) return;
  const long long row = e / c.L, f = row / 3;
  const int l = (int)(e - row * c.L);
  const double *pm = c.surfaces + (size_t)row * kM;
  const double p[kM] = {pm[0], pm[1], pm[2]};
  EvalUniforms u;
  u.l0 = Mdl::lin(p);
  u.n0 = Mdl::nl(p);
  u.scal = 1.0;
  const double *a = c.angles + (size_t)f * 3 * c.L + l;
  const double c0 = a[0];
  const double c1 = Mdl::uses_c1 ? a[c.L] : 0.0;
  const double c2 = Mdl::uses_c2 ? a[2 * c.L] : 0.0;
  const double v = model_value<MODEL, false>(u, c0, Mdl::template prepare<false>(c0, c1, c2));
  if (c.values) c.values[e] = v;
  c.grey[e] = (unsigned char)grey_level(v);
}

typedef void (*ValueKernel)(ValueCtx);
ValueKernel value_kernel_of(int model) {
  static const ValueKernel t[MODEL_COUNT] = {face_values_kernel<0>, face_values_kernel<1>, face_values_kernel<2>};
  return t[model];
}

// ---- render -----------------------------------------------------------------------------------------------------------------------
struct RenderCtx {
  const int *pm;              // [H][W]
  const unsigned char *grey;  // [nf][3][L]
  unsigned char *out;         // [L][H][W][3]
  int H, W, nf, L, background;
  long long img_bytes;  // 3 H W
  long long chunks;     // of one image: its ragged head, then the 16-byte chunks from its first boundary on
};

// blockIdx.y: the light.  Chunk 0 is the image's bytes in front of its first 16-byte boundary, chunk k > 0 the 16 bytes from
// boundary k - 1 on, cut at the image's end.
__global__ __launch_bounds__(kCT) void render_kernel(RenderCtx c) {
  const int l = blockIdx.y;
  unsigned char *img = c.out + (size_t)l * c.img_bytes;
  const long long to_boundary = (long long)((kChunk - (reinterpret_cast<uintptr_t>(img) & (kChunk - 1))) & (kChunk - 1));
  const long long head = to_boundary < c.img_bytes ? to_boundary : c.img_bytes;
  for (long long k = (long long)blockIdx.x * kCT + threadIdx.x; k < c.chunks; k += (long long)gridDim.x * kCT) {
    const long long b0 = k == 0 ? 0 : head + kChunk * (k - 1);
    long long b1 = k == 0 ? head : b0 + kChunk;
    if (b1 > c.img_bytes) b1 = c.img_bytes;
    if (b0 >= b1) continue;
    const int n = (int)(b1 - b0);
    const long long px = b0 / 3;
    int ch = (int)(b0 - 3 * px), row = (int)(px / c.W), x = (int)(px - (long long)row * c.W);
    int face = c.pm[(size_t)(c.H - 1 - row) * c.W + x];  // image row `row` is map row H - 1 - row
    unsigned w[4] = {0u, 0u, 0u, 0u}, untouched = 0u;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      if (j < n) {
        int q = c.background;
        if (face >= 0 && face < c.nf) q = c.grey[((size_t)face * 3 + ch) * c.L + l];
        if (q < 0) {
          untouched |= 1u << j;
          q = 0;
        }
        w[j >> 2] |= (unsigned)q << (8 * (j & 3));
        if (++ch == 3) {
          ch = 0;
          if (++x == c.W) {
            x = 0;
            ++row;
          }
          if (j + 1 < n) face = c.pm[(size_t)(c.H - 1 - row) * c.W + x];  // (the next byte is the image's: row < H)
        }
      }
    }
    if (n == kChunk && untouched == 0u) {
      *reinterpret_cast<uint4 *>(img + b0) = make_uint4(w[0], w[1], w[2], w[3]);  // (img + b0 is on a boundary: k > 0)
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; ++j)
        if (j < n && !((untouched >> j) & 1u)) img[b0 + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

// ---- residuals --------------------------------------------------------------------------------------------------------------------
struct ResidCtx {
  CandidateCtx cand;
  const unsigned char *grey;  // [nf][3][L]
  unsigned long long *light_acc;  // [3][L][3]: count, sum d, sum d^2 per light and channel (two's complement: the sums are signed)
  int *fl_count;                          // [nf][3][L]  (FACE: all three)
  unsigned long long *fl_sum, *fl_sumsq;  // [nf][3][L]
  unsigned char *abs_max, *worst;         // [H][W][3]   (PIXEL: both)
};

// Lane j of a tile: local pixel j / L, light j % L (lanes behind ppt * L idle).  A workgroup strides over the tiles and keeps its
// per-light words for all of them.  FACE, PIXEL: the call wants face maps, pixel maps -- every map of the kind is there then (the host
// lends what the caller left out): each uniform test of a pointer inside the loop is a pair of scalar registers the pass has not got.
template <bool FACE, bool PIXEL>
__global__ __launch_bounds__(kCT) void render_resid_kernel(ResidCtx c) {
  __shared__ int f_cnt[kTileWords], f_s1[kTileWords];  // a tile's sums fit 32 bits: at most kCT candidates, |d| <= 255
  __shared__ unsigned f_s2[kTileWords], p_key[kTileWords], f_face[kCT];  // (f_face: the face of the tile's local rank)
  __shared__ unsigned long long l_cnt[kLightWords], l_s1[kLightWords], l_s2[kLightWords];
  const int L = c.cand.L, H = c.cand.H, W = c.cand.W;
  const int ppt = kCT / L;  // the whole pixels of a tile
  const int S = (int)(c.cand.T / L), tiles = (int)(((long long)S + ppt - 1) / ppt);  // (the grouping refuses more than INT_MAX carried pixels)
  const int lp = (int)threadIdx.x / L, i = (int)threadIdx.x - lp * L;
  const int face_words = 3 * ppt * L;  // <= kTileWords
  for (int e = threadIdx.x; e < kLightWords; e += kCT) {
    l_cnt[e] = 0ull;
    l_s1[e] = 0ull;
    l_s2[e] = 0ull;
  }
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int e = threadIdx.x; e < kTileWords; e += kCT) {
      f_cnt[e] = 0;
      f_s1[e] = 0;
      f_s2[e] = 0u;
      p_key[e] = 0u;
    }
    __syncthreads();
    const int s0 = tile * ppt, s = s0 + lp;  // (s0 < S: tiles = ceil(S / ppt))
    const int r0 = c.cand.rank_of_face[c.cand.face_sorted[s0]];  // the tile's lowest rank: ranks ascend with the sorted pixels
    const bool live = lp < ppt && s < S;
    const Candidate k = read_candidate(c.cand, live ? (long long)s * L + i : c.cand.T);
    if (live) {
      const size_t face = c.cand.face_sorted[s];
      const unsigned lr = (unsigned)(k.r - r0);  // < ppt
      if (i == 0 && lr < (unsigned)ppt) f_face[lr] = (unsigned)face;  // (the face's pixels all write the same)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (k.valid[ch] && lr < (unsigned)ppt) {
          const int d = k.v[ch] - (int)c.grey[(face * 3 + ch) * L + i];
          const int e = ((int)lr * 3 + ch) * L + i;
          atomicAdd(&f_cnt[e], 1);
          atomicAdd(&f_s1[e], d);
          atomicAdd(&f_s2[e], (unsigned)(d * d));
          atomicMax(&p_key[lp * 3 + ch], ((unsigned)(d < 0 ? -d : d) << 8) | (unsigned)(255 - i));  // (> 0: i <= 63)
        }
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < face_words; e += kCT) {
      const int n = f_cnt[e];
      if (n == 0) continue;
      const int li = e % L, ch = (e / L) % 3;
      const unsigned long long s1 = (unsigned long long)(long long)f_s1[e], s2 = f_s2[e];
      const size_t word = ((size_t)f_face[e / (3 * L)] * 3 + ch) * L + li;
      if (FACE) {
        atomicAdd(&c.fl_count[word], n);
        atomicAdd(&c.fl_sum[word], s1);
        atomicAdd(&c.fl_sumsq[word], s2);
      }
      atomicAdd(&l_cnt[li * 3 + ch], (unsigned long long)n);
      atomicAdd(&l_s1[li * 3 + ch], s1);
      atomicAdd(&l_s2[li * 3 + ch], s2);
    }
    if (PIXEL && live && i == 0) {  // the pixel's first lane writes its three channels
      const long long g = c.cand.pixel_sorted[s];
      const int px = (int)(g / H), py = (int)(g % H);
      const size_t o = ((size_t)py * W + px) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const unsigned key = p_key[lp * 3 + ch];  // 0: nothing compared -> 0 and 255
        c.abs_max[o + ch] = (unsigned char)(key >> 8);
        c.worst[o + ch] = (unsigned char)(255u - (key & 255u));
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < 3 * L; e += kCT) {
    if (l_cnt[e] == 0ull) continue;
    atomicAdd(&c.light_acc[e], l_cnt[e]);
    atomicAdd(&c.light_acc[3 * L + e], l_s1[e]);
    atomicAdd(&c.light_acc[6 * L + e], l_s2[e]);
  }
}

// ---- surfaces from materials ----------------------------------------------------------------------------------------------------------
struct FillRow {
  double v[kM];
};
// One lane per double of surfaces[nf][3][3]
__global__ __launch_bounds__(kCT) void surfaces_from_materials_kernel(const int *__restrict__ label, long long words, const double *__restrict__ materials,
                                                                      int K, FillRow fill, double *__restrict__ surfaces) {
  const long long e = (long long)blockIdx.x * kCT + threadIdx.x;
  if (e >= words) return;
  const long long f = e / 9;
  const int j = (int)(e - 9 * f), k = label[f];
  surfaces[e] = (k >= 0 && k < K) ? materials[(size_t)k * 9 + j] : fill.v[j % kM];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
inline unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

// what the two rendering entries refuse besides their own pointers
int render_args_check(const char *who, const CaptureArgs &a) {
  if (a.L < 1 || a.L > kRenderMaxL || a.H <= 0 || a.W <= 0 || a.nf <= 0 || a.nf > INT_MAX / 3) {
    set_error("%s(): Lr = %d, H = %d, W = %d, nf = %d: need 1 <= Lr <= %d, H, W, nf > 0 and 3 nf <= INT_MAX", who, a.L, a.H, a.W, a.nf, kRenderMaxL);
    return kLmError;
  }
  MethodSpec ms;
  if (!known_model_method(a.model, BRDF_METHOD_BC_DIF, &ms, who)) return kLmError;
  if (a.rv_mode != 0 && a.rv_mode != 1) {
    set_error("%s(): rv_mode = %d: need 0 or 1", who, a.rv_mode);
    return kLmError;
  }
  return 0;
}

struct ValueTables {
  DevBuf angles, grey;  // [nf][3][L] double, unsigned char
};

// the cosines of all nf faces under the call's lights, the values (where asked for) and the grey levels: enqueued, no wait
int values_enqueue(const char *who, const CaptureArgs &a, const double *d_surfaces, double *d_face_values, ValueTables &vt) {
  const long long words = 3LL * a.nf * a.L;
  if (!take(vt.angles, sizeof(double) * (size_t)words, "the faces' cosines", who) || !take(vt.grey, (size_t)words, "the faces' grey levels", who)) return kLmError;
  if (cosines_run(a.d_vertices, a.d_faces, a.d_normals, nullptr, a.nf, a.leds, a.L, a.view, a.rv_mode, vt.angles.as<double>(), a.stream) != 0) return kLmError;
  const ValueCtx vc = {vt.angles.as<double>(), d_surfaces, words, a.L, d_face_values, vt.grey.as<unsigned char>()};
  hipLaunchKernelGGL(value_kernel_of(a.model), dim3(blocks_of(words)), dim3(kCT), 0, a.stream, vc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

const double kNoStart[kM] = {0.0, 0.0, 0.0};  // capture_args_check wants a p0; these entries read none

}  // namespace

int capture_render_run(const CaptureRenderArgs &ra) {
  const char *who = kWhoRender;
  const CaptureArgs &a = ra.cap;
  // ---- refused before any HIP call ----
  if (!a.d_pixel_map || !a.d_vertices || !a.d_faces || !a.d_normals || !a.leds || !a.view || !ra.d_brdf_surfaces) {
    set_error("%s(): null pixel map, mesh, leds, view origin or brdf_surfaces", who);
    return kLmError;
  }
  if (!ra.d_face_values && !ra.d_rendered) {
    set_error("%s(): face_values and rendered are both null: nothing to write", who);
    return kLmError;
  }
  if (render_args_check(who, a) != 0) return kLmError;
  if (ra.background < -1 || ra.background > 255) {
    set_error("%s(): background = %d: need -1 (leave untouched) or a grey level 0 ... 255", who, ra.background);
    return kLmError;
  }
  (void)hipGetLastError();
  ValueTables vt;
  if (values_enqueue(who, a, ra.d_brdf_surfaces, ra.d_face_values, vt) != 0) return kLmError;
  if (ra.d_rendered) {
    RenderCtx rc = {};
    rc.pm = a.d_pixel_map;
    rc.grey = vt.grey.as<unsigned char>();
    rc.out = ra.d_rendered;
    rc.H = a.H;
    rc.W = a.W;
    rc.nf = a.nf;
    rc.L = a.L;
    rc.background = ra.background;
    rc.img_bytes = 3LL * a.H * a.W;
    rc.chunks = rc.img_bytes / kChunk + 2;  // the head, the whole chunks, the tail
    const unsigned bx = std::min(blocks_of(rc.chunks), kMaxBlocks);
    hipLaunchKernelGGL(render_kernel, dim3(bx, (unsigned)a.L), dim3(kCT), 0, a.stream, rc);
    CAPTURE_OK(who, hipGetLastError());
  }
  CAPTURE_OK(who, hipStreamSynchronize(a.stream));
  return 0;
}

int capture_render_residuals_run(const CaptureRenderResidualsArgs &ra) {
  const char *who = kWhoResiduals;
  CaptureGrouped ga = ra.g;
  ga.cap.p0 = kNoStart;
  ga.cap.lb = ga.cap.ub = nullptr;
  ga.d_face_pixels = nullptr;
  ga.n_faces = nullptr;
  const CaptureArgs &a = ga.cap;
  // ---- refused before any HIP call ----
  if (capture_args_check(who, ga, ra.d_brdf_surfaces, "brdf_surfaces", kRenderMaxL) != 0 || render_args_check(who, a) != 0) return kLmError;
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int L = a.L;
  if (ga.n_pixels) *ga.n_pixels = 0;
  // ---- every map's value where nothing is compared ----
  const size_t light_words = 3 * (size_t)L, face_words = 3 * (size_t)a.nf * L, map_bytes = 3 * (size_t)a.H * a.W;
  long long *const light_out[3] = {ra.d_light_count, ra.d_light_sum, ra.d_light_sumsq};
  DevBuf light_acc;  // the three per-light maps behind ONE pointer: the pass holds enough of them
  if (!take(light_acc, sizeof(long long) * 3 * light_words, "the lights' sums", who)) return kLmError;
  CAPTURE_OK(who, hipMemsetAsync(light_acc.ptr, 0, sizeof(long long) * 3 * light_words, stream));
  for (long long *out : light_out)
    if (out) CAPTURE_OK(who, hipMemsetAsync(out, 0, sizeof(long long) * light_words, stream));
  if (ra.d_face_light_count) CAPTURE_OK(who, hipMemsetAsync(ra.d_face_light_count, 0, sizeof(int) * face_words, stream));
  if (ra.d_face_light_sum) CAPTURE_OK(who, hipMemsetAsync(ra.d_face_light_sum, 0, sizeof(long long) * face_words, stream));
  if (ra.d_face_light_sumsq) CAPTURE_OK(who, hipMemsetAsync(ra.d_face_light_sumsq, 0, sizeof(long long) * face_words, stream));
  if (ra.d_abs_max) CAPTURE_OK(who, hipMemsetAsync(ra.d_abs_max, 0, map_bytes, stream));
  if (ra.d_worst_light) CAPTURE_OK(who, hipMemsetAsync(ra.d_worst_light, 0xff, map_bytes, stream));
  // ---- values, grouping ----
  ValueTables vt;
  if (values_enqueue(who, a, ra.d_brdf_surfaces, ra.d_face_values, vt) != 0) return kLmError;
  CaptureGroup g;
  if (capture_group_run(who, ga, g) != 0) return kLmError;
  const bool any_map = ra.d_light_count || ra.d_light_sum || ra.d_light_sumsq || ra.d_face_light_count || ra.d_face_light_sum || ra.d_face_light_sumsq ||
                       ra.d_abs_max || ra.d_worst_light;
  if (g.S == 0 || !any_map) {  // an empty capture: every map holds what the memsets left
    CAPTURE_OK(who, hipStreamSynchronize(stream));
    return 0;
  }
  // ---- the one pass over the images ----
  ResidCtx rc = {};
  rc.cand = capture_candidates(ga, g);
  rc.grey = vt.grey.as<unsigned char>();
  const long long tiles = (g.S + kCT / L - 1) / (kCT / L);  // of kCT / L whole pixels
  rc.light_acc = light_acc.as<unsigned long long>();
  // a kind of map the call wants comes whole: what the caller left out of it is lent (and thrown away)
  const bool face_maps = ra.d_face_light_count || ra.d_face_light_sum || ra.d_face_light_sumsq, pixel_maps = ra.d_abs_max || ra.d_worst_light;
  DevBuf lent[5];
  void *maps[5] = {ra.d_face_light_count, ra.d_face_light_sum, ra.d_face_light_sumsq, ra.d_abs_max, ra.d_worst_light};
  const size_t map_size[5] = {sizeof(int) * face_words, sizeof(long long) * face_words, sizeof(long long) * face_words, map_bytes, map_bytes};
  for (int m = 0; m < 5; ++m) {
    if (maps[m] || !(m < 3 ? face_maps : pixel_maps)) continue;
    if (!take(lent[m], map_size[m], "a map the call left out", who)) return kLmError;
    maps[m] = lent[m].ptr;
  }
  rc.fl_count = static_cast<int *>(maps[0]);
  rc.fl_sum = static_cast<unsigned long long *>(maps[1]);
  rc.fl_sumsq = static_cast<unsigned long long *>(maps[2]);
  rc.abs_max = static_cast<unsigned char *>(maps[3]);
  rc.worst = static_cast<unsigned char *>(maps[4]);
  const auto kernel = face_maps ? (pixel_maps ? render_resid_kernel<true, true> : render_resid_kernel<true, false>)
                                : (pixel_maps ? render_resid_kernel<false, true> : render_resid_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<long long>(tiles, kMaxBlocks)), dim3(kCT), 0, stream, rc);
  CAPTURE_OK(who, hipGetLastError());
  for (int m = 0; m < 3; ++m)
    if (light_out[m])
      CAPTURE_OK(who, hipMemcpyAsync(light_out[m], light_acc.as<long long>() + m * light_words, sizeof(long long) * light_words, hipMemcpyDeviceToDevice, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  return 0;
}

int surfaces_from_materials_run(const SurfacesFromMaterialsArgs &a) {
  const char *who = kWhoSurfaces;
  if (!a.d_face_label || !a.d_materials || !a.fill || !a.d_brdf_surfaces) {
    set_error("%s(): null face_label, materials, fill or brdf_surfaces", who);
    return kLmError;
  }
  if (a.nf <= 0 || a.nf > INT_MAX / 3 || a.K < 1) {
    set_error("%s(): nf = %d, K = %d: need nf > 0, 3 nf <= INT_MAX and K >= 1", who, a.nf, a.K);
    return kLmError;
  }
  (void)hipGetLastError();
  const FillRow fill = {{a.fill[0], a.fill[1], a.fill[2]}};
  const long long words = 9LL * a.nf;
  hipLaunchKernelGGL(surfaces_from_materials_kernel, dim3(blocks_of(words)), dim3(kCT), 0, a.stream, a.d_face_label, words, a.d_materials, a.K, fill,
                     a.d_brdf_surfaces);
  CAPTURE_OK(who, hipGetLastError());
  CAPTURE_OK(who, hipStreamSynchronize(a.stream));
  return 0;
}

}  // namespace brdf
