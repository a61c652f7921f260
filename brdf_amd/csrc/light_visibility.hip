// light_visibility.hip -- cast shadows (light_visibility.h): per face one 64-bit word, bit l set iff light l is visible from the face's
// centre, and that word painted into the captures' images.  The reference stops short of this: its voxel-grid shadow code in
// brdfdata.cpp is commented out.  Brute force on purpose, nf^2 L ray-triangle tests and no acceleration structure: the answer depends on
// mesh and rig alone, so a capture session computes it once.
//
// Visibility, three launches and one wait:
//   prepare   one lane per face: the occluder record (v0, e1, e2; NaN for an invalid face, so that A > 0 fails by itself), the origin
//             ((a + b) + c) / 3.0, and the word of the lights the face does not face away from -- which is also what the face's result
//             starts from (0 for an invalid face)
//   cast      blockIdx.x: 256 origins, one per lane; blockIdx.y: a group of kLights lights whose directions d = P - o the lane holds in
//             registers; blockIdx.z: a contiguous range of occluders, so that a small mesh still fills the machine.  The occluders
//             stream through LDS in tiles of kTile records; every lane of a wave reads the same record, and identical LDS addresses
//             broadcast without a bank conflict.  s = o - v0, q = s x e1 and T = e2 . q depend on (origin, occluder) alone and are paid
//             once per occluder; h = d x e2, a, U and V once per light.  A lane ends with the bits of its group that some occluder of its
//             range hides and clears them with one atomicAnd.  A wave whose lanes have no light left skips the tile's arithmetic, a
//             workgroup without one leaves the loop: either only skips tests whose bits are already clear.
//   finish    one lane per face: the lit and the shadowed pairs, counted
// AND is commutative and idempotent, so neither the split nor the early stop nor the order of the workgroups can change a bit: two calls
// give the same bytes whatever the grid.  Integer atomics only.  Workspace: 112 B per face.
//
// Painting is one pass over the images: a lane takes four pixels (12 bytes) of one image, reads their map entries and the faces' words,
// and moves the bytes as three dwords where the image's base allows it, byte by byte otherwise and at the image's end.  In place it
// writes painted bytes only.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "capture_group.h"
#include "light_visibility.h"

namespace brdf {

namespace {

constexpr int kLights = 8;              // the lights a lane holds in registers: 24 doubles
constexpr int kTile = 128;              // occluder records of an LDS tile: 9 KiB
constexpr int kRec = 9;                 // doubles of an occluder record: v0, e1, e2
constexpr int kSplitTiles = 4;          // the least tiles of an occluder range
constexpr long long kWantBlocks = 256 * 8;  // workgroups that fill the machine: 8 per CU
constexpr int kApplyPixels = 4;         // the pixels a lane of the paint pass takes: 12 bytes, three dwords
constexpr unsigned kApplyGrid = 256 * 8;
const char *const kWhoVis = "brdf_hip_light_visibility_dev", *const kWhoApply = "brdf_hip_capture_apply_visibility_dev";

enum Stat { kValid, kInvalid, kAway, kLit, kShadowed };

struct Rig {
  double p[kVisibilityMaxL][3];  // the lights, by value: a uniform index reads them through scalar registers
};

__device__ __forceinline__ double dot3(const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ __forceinline__ void cross3(const double *x, const double *y, double *out) {
  out[0] = x[1] * y[2] - x[2] * y[1];
  out[1] = x[2] * y[0] - x[0] * y[2];
  out[2] = x[0] * y[1] - x[1] * y[0];
}

struct VisCtx {
  const double *vertices;
  const int *faces;
  const double *normals;  // or null
  int nv, nf, L;
  int split_tiles;        // the tiles of an occluder range
  double t_min, one_minus;  // 1.0 - t_min
  double *occ;                      // [nf][kRec]
  double *org;                      // [nf][3]
  unsigned long long *toward;       // [nf]: the lights the face does not face away from; 0 for an invalid face
  unsigned long long *lit;          // [nf]: the result
  unsigned long long *stats;        // [kVisibilityStats]
};

__global__ __launch_bounds__(kCT) void prepare_kernel(VisCtx c, Rig rig) {
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  int valid = -1;  // (-1: no face)
  unsigned long long toward = 0;
  if (f < c.nf) {
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = c.faces[3 * (size_t)f + k];
    double rec[kRec], o[3] = {NAN, NAN, NAN};
#pragma unroll
    for (int k = 0; k < kRec; ++k) rec[k] = NAN;
    valid = v[0] >= 0 && v[0] < c.nv && v[1] >= 0 && v[1] < c.nv && v[2] >= 0 && v[2] < c.nv;
    if (valid) {
      double p[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          p[i][k] = c.vertices[3 * (size_t)v[i] + k];
          valid = valid && isfinite(p[i][k]);
        }
      if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          rec[k] = p[0][k];
          rec[3 + k] = p[1][k] - p[0][k];
          rec[6 + k] = p[2][k] - p[0][k];
          o[k] = ((p[0][k] + p[1][k]) + p[2][k]) / 3.0;
        }
        double n[3] = {0.0, 0.0, 0.0};
        if (c.normals)
#pragma unroll
          for (int k = 0; k < 3; ++k) n[k] = c.normals[3 * (size_t)f + k];
        for (int l = 0; l < c.L; ++l) {
          const double d[3] = {rig.p[l][0] - o[0], rig.p[l][1] - o[1], rig.p[l][2] - o[2]};
          if (!c.normals || dot3(n, d) > 0.0) toward |= 1ull << l;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kRec; ++k) c.occ[kRec * (size_t)f + k] = rec[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c.org[3 * (size_t)f + k] = o[k];
    c.toward[f] = toward;
    c.lit[f] = toward;
  }
  // every lane of the workgroup is here again: the wave's counts
  unsigned long long away = 0;
  for (int l = 0; l < c.L; ++l) away += (unsigned long long)__popcll(__ballot(valid == 1 && !((toward >> l) & 1ull)));
  const unsigned long long ok = __ballot(valid == 1), bad = __ballot(valid == 0);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (ok) atomicAdd(&c.stats[kValid], (unsigned long long)__popcll(ok));
    if (bad) atomicAdd(&c.stats[kInvalid], (unsigned long long)__popcll(bad));
    if (away) atomicAdd(&c.stats[kAway], away);
  }
}

__global__ __launch_bounds__(kCT) void cast_kernel(VisCtx c, Rig rig) {
  __shared__ double tile[kTile * kRec];
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  const int l0 = blockIdx.y * kLights;
  double o[3] = {0.0, 0.0, 0.0};
  unsigned mine = 0;  // the group's lights this lane has to decide: bit k is light l0 + k
  if (f < c.nf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = c.org[3 * (size_t)f + k];
    mine = (unsigned)(c.toward[f] >> l0) & ((1u << kLights) - 1u);
  }
  double d[kLights][3];
#pragma unroll
  for (int k = 0; k < kLights; ++k) {
    const int l = l0 + k < c.L ? l0 + k : c.L - 1;  // (a light beyond L is none of `mine`: what it hits is dropped)
#pragma unroll
    for (int j = 0; j < 3; ++j) d[k][j] = rig.p[l][j] - o[j];
  }
  unsigned shadow = 0;
  const long long range = (long long)c.split_tiles * kTile, g0 = (long long)blockIdx.z * range, g1 = g0 + range < c.nf ? g0 + range : c.nf;
  for (long long base = g0; base < g1; base += kTile) {
    // (the barrier that lets the tile be overwritten, and the workgroup's early stop)
    if (!__syncthreads_or((mine & ~shadow) != 0u)) break;
    const int count = g1 - base < kTile ? (int)(g1 - base) : kTile;
    for (int i = threadIdx.x; i < count * kRec; i += kCT) tile[i] = c.occ[kRec * (size_t)base + i];
    __syncthreads();
    if (__ballot((mine & ~shadow) != 0u) == 0ull) continue;  // the wave's early stop
    for (int j = 0; j < count; ++j) {
      const double *r = tile + kRec * j;  // the same address in every lane: a broadcast
      const double v0[3] = {r[0], r[1], r[2]}, e1[3] = {r[3], r[4], r[5]}, e2[3] = {r[6], r[7], r[8]};
      const double s[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
      double q[3];
      cross3(s, e1, q);
      const double T = dot3(e2, q);
      const bool other = base + j != f;
#pragma unroll
      for (int k = 0; k < kLights; ++k) {
        double h[3];
        cross3(d[k], e2, h);
        const double a = dot3(e1, h), U = dot3(s, h), V = dot3(d[k], q);
        const bool neg = a < 0.0;
        const double A = fabs(a), Un = neg ? -U : U, Vn = neg ? -V : V, Tn = neg ? -T : T;
        const bool hit = A > 0.0 && Un >= 0.0 && Vn >= 0.0 && Un + Vn <= A && Tn > c.t_min * A && Tn < c.one_minus * A;
        shadow |= (unsigned)(hit && other) << k;
      }
    }
  }
  shadow &= mine;
  if (shadow) atomicAnd(&c.lit[f], ~((unsigned long long)shadow << l0));  // (mine != 0: f < nf)
}

__global__ __launch_bounds__(kCT) void finish_kernel(VisCtx c) {
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  unsigned long long lit = 0, toward = 0;
  if (f < c.nf) {
    lit = c.lit[f];
    toward = c.toward[f];
  }
  // the wave's sums of two small counts, by ballots of their bits (a count is at most 64: seven bits)
  unsigned long long n_lit = 0, n_dark = 0;
  const int a = __popcll(lit), b = __popcll(toward & ~lit);
#pragma unroll
  for (int bit = 0; bit < 7; ++bit) {
    n_lit += (unsigned long long)__popcll(__ballot((a >> bit) & 1)) << bit;
    n_dark += (unsigned long long)__popcll(__ballot((b >> bit) & 1)) << bit;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (n_lit) atomicAdd(&c.stats[kLit], n_lit);
    if (n_dark) atomicAdd(&c.stats[kShadowed], n_dark);
  }
}

// ---- painting ----------------------------------------------------------------------------------------------------------------------------
struct ApplyCtx {
  const unsigned char *in;  // [L][H][W][3]
  unsigned char *out;       // the same, or apart from it
  const int *pm;            // [H][W]
  const unsigned long long *lit;  // [nf]
  int H, W, nf;
  unsigned level;
  long long pixels;               // H W
  unsigned long long *shadowed;   // [L] or null, zeroed
};

// byte b of the 12 in w[3]
__device__ __forceinline__ void put_byte(unsigned *w, int b, unsigned v) { w[b >> 2] = (w[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (v << (8 * (b & 3))); }

// blockIdx.y: the light.  IN_PLACE: out == in, and only painted bytes are written.
template <bool IN_PLACE>
__global__ __launch_bounds__(kCT) void apply_kernel(ApplyCtx c) {
  __shared__ unsigned block_painted;
  const int l = blockIdx.y;
  const size_t image = (size_t)l * 3 * (size_t)c.pixels;
  const unsigned char *src = c.in + image;
  unsigned char *dst = c.out + image;
  const bool src_words = (reinterpret_cast<uintptr_t>(src) & 3u) == 0, dst_words = (reinterpret_cast<uintptr_t>(dst) & 3u) == 0;  // (12 k keeps it)
  const unsigned fill = c.level * 0x01010101u;
  if (threadIdx.x == 0) block_painted = 0;
  __syncthreads();
  unsigned painted = 0;
  for (long long k = (long long)blockIdx.x * kCT + threadIdx.x; kApplyPixels * k < c.pixels; k += (long long)gridDim.x * kCT) {
    const long long p0 = kApplyPixels * k;
    const int n = c.pixels - p0 < kApplyPixels ? (int)(c.pixels - p0) : kApplyPixels;
    int row = (int)(p0 / c.W), x = (int)(p0 - (long long)row * c.W);
    unsigned dark = 0;
#pragma unroll
    for (int j = 0; j < kApplyPixels; ++j) {
      if (j < n) {
        const int face = c.pm[(size_t)(c.H - 1 - row) * c.W + x];  // image row `row` is map row H - 1 - row
        if (face >= 0 && face < c.nf && !((c.lit[face] >> l) & 1ull)) dark |= 1u << j;
        if (++x == c.W) {
          x = 0;
          ++row;
        }
      }
    }
    painted += (unsigned)__popc(dark);
    const size_t b0 = 3 * (size_t)p0;
    if (IN_PLACE) {
      if (dark == (1u << kApplyPixels) - 1u && dst_words) {
        unsigned *w = reinterpret_cast<unsigned *>(dst + b0);
        w[0] = fill;
        w[1] = fill;
        w[2] = fill;
      } else {
#pragma unroll
        for (int b = 0; b < 3 * kApplyPixels; ++b)
          if ((dark >> (b / 3)) & 1u) dst[b0 + b] = (unsigned char)c.level;
      }
    } else {
      unsigned w[3] = {0u, 0u, 0u};
      if (n == kApplyPixels && src_words) {
        const unsigned *s = reinterpret_cast<const unsigned *>(src + b0);
        w[0] = s[0];
        w[1] = s[1];
        w[2] = s[2];
      } else {
#pragma unroll
        for (int b = 0; b < 3 * kApplyPixels; ++b)
          if (b < 3 * n) put_byte(w, b, src[b0 + b]);
      }
#pragma unroll
      for (int b = 0; b < 3 * kApplyPixels; ++b)
        if ((dark >> (b / 3)) & 1u) put_byte(w, b, c.level);
      if (n == kApplyPixels && dst_words) {
        unsigned *t = reinterpret_cast<unsigned *>(dst + b0);
        t[0] = w[0];
        t[1] = w[1];
        t[2] = w[2];
      } else {
#pragma unroll
        for (int b = 0; b < 3 * kApplyPixels; ++b)
          if (b < 3 * n) dst[b0 + b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
      }
    }
  }
  if (c.shadowed) {  // (uniform)
    if (painted) atomicAdd(&block_painted, painted);  // (a workgroup's share of at most 2^31 pixels: no overflow)
    __syncthreads();
    if (threadIdx.x == 0 && block_painted) atomicAdd(&c.shadowed[l], (unsigned long long)block_painted);
  }
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

}  // namespace

int light_visibility_run(const LightVisibilityArgs &a) {
  const char *who = kWhoVis;
  // ---- refused before any HIP call ----
  if (!a.d_vertices || !a.d_faces || !a.leds || !a.d_face_lit) {
    set_error("%s(): null vertices, faces, leds or face_lit", who);
    return kLmError;
  }
  if (a.L < 1 || a.L > kVisibilityMaxL) {
    set_error("%s(): L = %d: need 1 <= L <= %d (one bit of a 64-bit word per light)", who, a.L, kVisibilityMaxL);
    return kLmError;
  }
  if (a.nv < 1 || a.nv > INT_MAX || a.nf < 1 || a.nf > INT_MAX) {
    set_error("%s(): nv = %lld, nf = %lld: need 1 <= nv, nf <= INT_MAX", who, a.nv, a.nf);
    return kLmError;
  }
  if (!(a.t_min >= 0.0 && a.t_min < 0.5)) {
    set_error("%s(): t_min = %g: need 0 <= t_min < 0.5", who, a.t_min);
    return kLmError;
  }
  Rig rig = {};
  for (int l = 0; l < a.L; ++l)
    for (int k = 0; k < 3; ++k) {
      rig.p[l][k] = a.leds[3 * l + k];
      if (!std::isfinite(rig.p[l][k])) {
        set_error("%s(): leds[%d][%d] = %g: need finite light positions", who, l, k, rig.p[l][k]);
        return kLmError;
      }
    }
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int nf = (int)a.nf;
  // one allocation: the counters, the occluder records, the origins, the words of the lights faced
  const size_t at_stats = 0, at_occ = 256, at_org = at_occ + sizeof(double) * kRec * (size_t)nf, at_toward = at_org + sizeof(double) * 3 * (size_t)nf;
  DevBuf ws;
  if (!take(ws, at_toward + sizeof(long long) * (size_t)nf, "the workspace", who)) return kLmError;
  unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(ws.ptr + at_stats);
  CAPTURE_OK(who, hipMemsetAsync(d_stats, 0, sizeof(long long) * kVisibilityStats, stream));
  // the grid of the cast: origins x light groups x occluder ranges, the ranges as many as fill the machine and no shorter than kSplitTiles
  const long long nb = blocks_of(nf), groups = (a.L + kLights - 1) / kLights, tiles = ((long long)nf + kTile - 1) / kTile;
  const long long want = (kWantBlocks + nb * groups - 1) / (nb * groups);
  const long long split_tiles = std::max<long long>(kSplitTiles, (tiles + want - 1) / want), splits = (tiles + split_tiles - 1) / split_tiles;
  const VisCtx c = {a.d_vertices, a.d_faces, a.d_normals, (int)a.nv, nf, a.L, (int)split_tiles, a.t_min, 1.0 - a.t_min,
                    reinterpret_cast<double *>(ws.ptr + at_occ), reinterpret_cast<double *>(ws.ptr + at_org),
                    reinterpret_cast<unsigned long long *>(ws.ptr + at_toward), a.d_face_lit, d_stats};
  hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)nb), dim3(kCT), 0, stream, c, rig);
  CAPTURE_OK(who, hipGetLastError());
  hipLaunchKernelGGL(cast_kernel, dim3((unsigned)nb, (unsigned)groups, (unsigned)splits), dim3(kCT), 0, stream, c, rig);
  CAPTURE_OK(who, hipGetLastError());
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)nb), dim3(kCT), 0, stream, c);
  CAPTURE_OK(who, hipGetLastError());
  long long h_stats[kVisibilityStats];
  CAPTURE_OK(who, hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  if (a.stats)
    for (int k = 0; k < kVisibilityStats; ++k) a.stats[k] = h_stats[k];
  return 0;
}

int apply_visibility_run(const ApplyVisibilityArgs &a) {
  const char *who = kWhoApply;
  // ---- refused before any HIP call ----
  if (!a.d_images || !a.d_pixel_map || !a.d_face_lit || !a.d_out) {
    set_error("%s(): null images, pixel_map, face_lit or out", who);
    return kLmError;
  }
  if (a.L < 1 || a.L > kVisibilityMaxL) {
    set_error("%s(): L = %d: need 1 <= L <= %d (bit l of a face's word is image l)", who, a.L, kVisibilityMaxL);
    return kLmError;
  }
  if (a.H < 1 || a.W < 1 || (long long)a.H * a.W > INT_MAX || a.nf < 1) {
    set_error("%s(): H = %d, W = %d, nf = %d: need H, W, nf >= 1 and H W <= INT_MAX", who, a.H, a.W, a.nf);
    return kLmError;
  }
  if (a.level < 0 || a.level > 255) {
    set_error("%s(): level = %d: need 0 ... 255", who, a.level);
    return kLmError;
  }
  const long long pixels = (long long)a.H * a.W;
  const uintptr_t in = reinterpret_cast<uintptr_t>(a.d_images), out = reinterpret_cast<uintptr_t>(a.d_out), bytes = (uintptr_t)3 * pixels * a.L;
  if (in != out && in < out + bytes && out < in + bytes) {
    set_error("%s(): out overlaps images in part: need out == images (in place) or a buffer apart from it", who);
    return kLmError;
  }
  (void)hipGetLastError();
  if (a.d_shadowed) CAPTURE_OK(who, hipMemsetAsync(a.d_shadowed, 0, sizeof(long long) * (size_t)a.L, a.stream));
  const ApplyCtx c = {a.d_images, a.d_out, a.d_pixel_map, a.d_face_lit, a.H, a.W, a.nf, (unsigned)a.level, pixels, a.d_shadowed};
  const unsigned grid = std::min(blocks_of((pixels + kApplyPixels - 1) / kApplyPixels), kApplyGrid);
  if (in == out) hipLaunchKernelGGL(apply_kernel<true>, dim3(grid, (unsigned)a.L), dim3(kCT), 0, a.stream, c);
  else hipLaunchKernelGGL(apply_kernel<false>, dim3(grid, (unsigned)a.L), dim3(kCT), 0, a.stream, c);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

}  // namespace brdf
