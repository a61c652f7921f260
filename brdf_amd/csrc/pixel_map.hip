// pixel_map.hip -- mesh + camera -> face normals and the pixel-to-face map, the two inputs every capture entry takes (pixel_map.h).
//
// Replaces CBRDFdata::CalcFaceNormals (brdfdata.cpp:314-330, Eigen on the host) and CBRDFdata::CalcPixel2SurfaceMapping (:629-681,
// gluProject under a live GL context, one pixel per face).  Mode 0 is that map; mode 1 is the map the capture layer assumes: a face
// owns every pixel whose centre it covers, and where faces overlap the nearest one, the lowest index among equals.
//
// Mode 1, four launches and one wait:
//   setup     one lane per face: project the three vertices, drop what cannot be drawn, write a 96-byte record (window-space vertices,
//             area, clamped box) and the box's pixel count; the workgroup scans its 256 counts (exclusive, 64-bit) and writes its total
//   scan      one workgroup: the totals -> the workgroups' offsets and T, the number of candidates (face, box pixel)
//   depth     one lane per candidate in a grid-stride loop over T: two binary searches (offsets, then the 256 counts of a workgroup)
//             name the face, the remainder names the box pixel; a covered pixel gets atomicMin of z's bit pattern (a double in [0, 1]
//             orders as its unsigned bits) on a 64-bit map
//   owner     the same walk and the same device function, so the same bits: where z equals the stored minimum, atomicMin of the face
//             index on the output map (unsigned, initialised to all ones = -1)
//   finish    one lane per pixel: depth, face_pixels and the owned count, integer atomics
// Nothing depends on the order in which lanes run: two calls give the same bytes whatever the grid.  Work per lane is one box pixel,
// whatever the sizes of the triangles: a two-triangle backdrop spreads over as many lanes as it has pixels.
// Workspace: 96 B + 8 B per face, 8 B per pixel, 8 B per 256 faces: O(nf + H W).
#include <climits>
#include <cmath>

#include "capture_group.h"
#include "pixel_map.h"

namespace brdf {

namespace {

constexpr unsigned kGridCap = 256 * 8;  // workgroups of the candidate walks: 8 per CU keep every SIMD at 8 waves
const char *const kWhoMap = "brdf_hip_pixel_map_dev", *const kWhoNormals = "brdf_hip_face_normals_dev";

enum Stat { kRasterised, kUnprojectable, kDegenerate, kCulled, kOutside, kCandidates, kOwned, kRefused };

struct Camera {
  double mv[16], pr[16], vp[4];
};

struct Win {
  double x, y, z, w;
  bool ok;  // w != 0 and everything finite
};

__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// gluProject: model_view, projection (column-major), perspective division, viewport
__device__ __forceinline__ Win project(const Camera &c, double x, double y, double z) {
  double e[4], q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = ((x * c.mv[i] + y * c.mv[4 + i]) + z * c.mv[8 + i]) + c.mv[12 + i];  // in3 = 1
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = ((e[0] * c.pr[i] + e[1] * c.pr[4 + i]) + e[2] * c.pr[8 + i]) + e[3] * c.pr[12 + i];
  Win w;
  w.w = q[3];
  w.ok = q[3] != 0.0 && finite3(q[0], q[1], q[2]) && isfinite(q[3]);
  const double d = w.ok ? q[3] : 1.0;
  w.x = (q[0] / d * 0.5 + 0.5) * c.vp[2] + c.vp[0];
  w.y = (q[1] / d * 0.5 + 0.5) * c.vp[3] + c.vp[1];
  w.z = q[2] / d * 0.5 + 0.5;
  w.ok = w.ok && finite3(w.x, w.y, w.z);
  return w;
}

// a face's three vertex indices; false: one of them is outside [0, nv)
__device__ __forceinline__ bool face_indices(const int *faces, long long f, int nv, int v[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = faces[3 * (size_t)f + k];
  return v[0] >= 0 && v[0] < nv && v[1] >= 0 && v[1] < nv && v[2] >= 0 && v[2] < nv;
}

// stats[k] += the number of the workgroup's lanes whose status is k, k < n; every lane of the workgroup calls
__device__ __forceinline__ void count_status(unsigned long long *stats, int status, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int k = 0; k < n; ++k) {
    const unsigned long long m = __ballot(status == k);
    if (lane == 0 && m) atomicAdd(&stats[k], (unsigned long long)__popcll(m));
  }
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCT) void face_normals_kernel(const double *__restrict__ vertices, int nv, const int *__restrict__ faces, int nf,
                                                           double *__restrict__ normals) {
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  if (f >= nf) return;
  int v[3];
  double n[3] = {NAN, NAN, NAN};
  if (face_indices(faces, f, nv, v)) {
    const double *a = vertices + 3 * (size_t)v[0], *b = vertices + 3 * (size_t)v[1], *c = vertices + 3 * (size_t)v[2];
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double z = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (z > 0.0) {  // Eigen's normalize(); true divisions: a -0 component stays -0, as in the twin
      const double s = sqrt(z);
      n[0] /= s;
      n[1] /= s;
      n[2] /= s;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) normals[3 * (size_t)f + k] = n[k];
}

// ---- mode 0: one pixel per centroid ---------------------------------------------------------------------------------------------------
struct CentroidCtx {
  const double *vertices;
  const int *faces;
  int nv, nf, H, W;
  Camera cam;
  int *map;         // [H][W], initialised to -1
  double *face_z;   // [nf]: the centroid's window z
  unsigned long long *stats;
};

__global__ __launch_bounds__(kCT) void centroid_kernel(CentroidCtx c) {
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  int status = -1, v[3];
  if (f < c.nf) {
    status = kUnprojectable;
    if (face_indices(c.faces, f, c.nv, v)) {
      double m[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) m[k] = ((c.vertices[3 * (size_t)v[0] + k] + c.vertices[3 * (size_t)v[1] + k]) + c.vertices[3 * (size_t)v[2] + k]) / 3.0;
      const Win w = project(c.cam, m[0], m[1], m[2]);
      if (w.ok) {
        c.face_z[f] = w.z;
        if (!(w.y >= 0.0 && w.x >= 0.0)) {
          status = kOutside;
        } else if (w.x >= (double)c.W || w.y >= (double)c.H) {  // (int)winX >= W: the reference writes out of bounds here
          status = kRefused;
        } else {
          status = kRasterised;
          atomicMax(&c.map[(size_t)(int)w.y * c.W + (int)w.x], (int)f);  // the serial loop's last face wins
        }
      }
    }
  }
  count_status(c.stats, status, kPixelMapStats);
}

// ---- mode 1 ------------------------------------------------------------------------------------------------------------------------------
struct FaceRec {
  double ax, ay, az, bx, by, bz, cx, cy, cz, A;  // window space
  int x0, y0, bw, pad;                           // the clamped box's first column and row, its width
};

struct RasterCtx {
  const double *vertices;
  const int *faces;
  int nv, nf, H, W, cull;
  long long nb;  // workgroups of the setup: ceil(nf / kCT)
  Camera cam;
  FaceRec *rec;                   // [nf]
  long long *local;               // [nf]: the box pixels of the faces before this one in its workgroup
  long long *block_off;           // [nb + 1]: in: the workgroups' totals; out: their offsets, [nb] = T
  unsigned long long *zmap;       // [H][W]: the least z's bits, initialised to all ones
  unsigned *map;                  // [H][W]: the owner, initialised to all ones
  unsigned long long *stats;
};

__global__ __launch_bounds__(kCT) void setup_kernel(RasterCtx c) {
  __shared__ long long scan[2][kCT];
  const long long f = (long long)blockIdx.x * kCT + threadIdx.x;
  int status = -1, v[3];
  long long pixels = 0;
  if (f < c.nf) {
    status = kUnprojectable;
    if (face_indices(c.faces, f, c.nv, v)) {
      const double *pa = c.vertices + 3 * (size_t)v[0], *pb = c.vertices + 3 * (size_t)v[1], *pc = c.vertices + 3 * (size_t)v[2];
      const Win a = project(c.cam, pa[0], pa[1], pa[2]), b = project(c.cam, pb[0], pb[1], pb[2]), d = project(c.cam, pc[0], pc[1], pc[2]);
      if (a.ok && b.ok && d.ok && a.w > 0.0 && b.w > 0.0 && d.w > 0.0) {
        const double A = (b.x - a.x) * (d.y - a.y) - (b.y - a.y) * (d.x - a.x);
        const double minx = fmin(fmin(a.x, b.x), d.x), maxx = fmax(fmax(a.x, b.x), d.x);
        const double miny = fmin(fmin(a.y, b.y), d.y), maxy = fmax(fmax(a.y, b.y), d.y);
        if (A == 0.0 || !isfinite(A)) {
          status = kDegenerate;
        } else if (c.cull && A < 0.0) {
          status = kCulled;
        } else if (maxx < 0.0 || minx > (double)c.W || maxy < 0.0 || miny > (double)c.H) {
          status = kOutside;
        } else {
          status = kRasterised;
          // the pixels whose centres the box holds: col + 0.5 in [minx, maxx], clamped to the viewport
          const double x0 = fmax(ceil(minx - 0.5), 0.0), x1 = fmin(floor(maxx - 0.5), (double)(c.W - 1));
          const double y0 = fmax(ceil(miny - 0.5), 0.0), y1 = fmin(floor(maxy - 0.5), (double)(c.H - 1));
          FaceRec r = {a.x, a.y, a.z, b.x, b.y, b.z, d.x, d.y, d.z, A, 0, 0, 0, 0};
          if (x0 <= x1 && y0 <= y1) {  // (a face between the centres holds none)
            r.x0 = (int)x0;
            r.y0 = (int)y0;
            r.bw = (int)x1 - r.x0 + 1;
            pixels = (long long)r.bw * ((int)y1 - r.y0 + 1);
          }
          c.rec[f] = r;
        }
      }
    }
  }
  count_status(c.stats, status, kOutside + 1);
  // exclusive scan of the workgroup's counts
  int cur = 0;
  scan[0][threadIdx.x] = pixels;
  __syncthreads();
  for (int step = 1; step < kCT; step <<= 1) {
    const long long mine = scan[cur][threadIdx.x] + ((int)threadIdx.x >= step ? scan[cur][threadIdx.x - step] : 0);
    scan[cur ^ 1][threadIdx.x] = mine;
    cur ^= 1;
    __syncthreads();
  }
  if (f < c.nf) c.local[f] = scan[cur][threadIdx.x] - pixels;
  if (threadIdx.x == kCT - 1) c.block_off[blockIdx.x] = scan[cur][kCT - 1];
}

// One workgroup: totals[nb] -> offsets[nb + 1] in place, the shape of capture_compact.h's block_scan3_kernel with one 64-bit column (a
// workgroup's total of box pixels does not fit the int that kernel reads).  stats[kCandidates] = T.
__global__ __launch_bounds__(kCT) void offsets_kernel(long long *__restrict__ block_off, long long nb, unsigned long long *__restrict__ stats) {
  __shared__ long long part[kCT];
  const int t = threadIdx.x;
  const long long per = (nb + kCT - 1) / kCT;
  const long long b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
  long long sum = 0;
  for (long long b = b0; b < b1; ++b) sum += block_off[b];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < kCT; ++i) {
      const long long v = part[i];
      part[i] = run;
      run += v;
    }
    block_off[nb] = run;
    stats[kCandidates] = (unsigned long long)run;
  }
  __syncthreads();
  sum = part[t];
  for (long long b = b0; b < b1; ++b) {
    const long long v = block_off[b];
    block_off[b] = sum;
    sum += v;
  }
}

// the largest i in [lo, hi) with a[i] <= key (a ascending, a[lo] <= key)
__device__ __forceinline__ long long last_not_above(const long long *__restrict__ a, long long lo, long long hi, long long key) {
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

// candidate t -> its face and box pixel; true: the face covers the pixel's centre with a depth in [0, 1]
__device__ __forceinline__ bool candidate(const RasterCtx &c, long long t, long long &f, size_t &pixel, unsigned long long &zbits) {
  const long long b = last_not_above(c.block_off, 0, c.nb, t);
  const long long rest = t - c.block_off[b], f0 = b * kCT, f1 = f0 + kCT < c.nf ? f0 + kCT : c.nf;
  f = last_not_above(c.local, f0, f1, rest);  // (faces without pixels share their successor's entry: the last of a run has them)
  const FaceRec r = c.rec[f];
  const unsigned k = (unsigned)(rest - c.local[f]);
  const int row = r.y0 + (int)(k / (unsigned)r.bw), col = r.x0 + (int)(k % (unsigned)r.bw);
  pixel = (size_t)row * c.W + col;
  const double px = col + 0.5, py = row + 0.5;
  const double E0 = (r.bx - px) * (r.cy - py) - (r.by - py) * (r.cx - px);
  const double E1 = (r.cx - px) * (r.ay - py) - (r.cy - py) * (r.ax - px);
  const double E2 = (r.ax - px) * (r.by - py) - (r.ay - py) * (r.bx - px);
  const double s = r.A > 0.0 ? 1.0 : -1.0;
  if (!(s * E0 >= 0.0 && s * E1 >= 0.0 && s * E2 >= 0.0)) return false;
  double z = ((E0 * r.az + E1 * r.bz) + E2 * r.cz) / r.A;
  if (!(z >= 0.0 && z <= 1.0)) return false;
  if (z == 0.0) z = 0.0;  // -0 orders above every depth as bits
  zbits = (unsigned long long)__double_as_longlong(z);
  return true;
}

template <bool OWNER>
__global__ __launch_bounds__(kCT) void candidates_kernel(RasterCtx c) {
  const long long T = c.block_off[c.nb];
  for (long long t = (long long)blockIdx.x * kCT + threadIdx.x; t < T; t += (long long)gridDim.x * kCT) {
    long long f;
    size_t pixel;
    unsigned long long zbits;
    if (!candidate(c, t, f, pixel, zbits)) continue;
    if (!OWNER) atomicMin(&c.zmap[pixel], zbits);
    else if (c.zmap[pixel] == zbits) atomicMin(&c.map[pixel], (unsigned)f);
  }
}

// ---- both modes: depth, face_pixels, the owned count ------------------------------------------------------------------------------------
struct FinishCtx {
  const int *map;
  long long pixels;
  int nf;
  const unsigned long long *zmap;  // mode 1
  const double *face_z;            // mode 0
  double *depth;                   // or null
  int *face_pixels;                // or null, zeroed
  unsigned long long *stats;
};

__global__ __launch_bounds__(kCT) void finish_kernel(FinishCtx c) {
  const long long i = (long long)blockIdx.x * kCT + threadIdx.x;
  int f = -1;
  if (i < c.pixels) {
    f = c.map[i];
    if (c.depth) c.depth[i] = f < 0 ? 2.0 : (c.zmap ? __longlong_as_double((long long)c.zmap[i]) : c.face_z[f]);
    if (f >= 0 && c.face_pixels) atomicAdd(&c.face_pixels[f], 1);
  }
  const unsigned long long m = __ballot(f >= 0);
  if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(&c.stats[kOwned], (unsigned long long)__popcll(m));
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

bool mesh_refused(const char *who, const void *d_vertices, long long nv, const void *d_faces, long long nf) {
  if (!d_vertices || !d_faces) {
    set_error("%s(): null vertices or faces", who);
    return true;
  }
  if (nv < 1 || nv > INT_MAX || nf < 1 || nf > INT_MAX) {
    set_error("%s(): nv = %lld, nf = %lld: need 1 <= nv, nf <= INT_MAX", who, nv, nf);
    return true;
  }
  return false;
}

}  // namespace

int face_normals_run(const double *d_vertices, long long nv, const int *d_faces, long long nf, double *d_normals, hipStream_t stream) {
  const char *who = kWhoNormals;
  if (mesh_refused(who, d_vertices, nv, d_faces, nf)) return kLmError;
  if (!d_normals) {
    set_error("%s(): null normals", who);
    return kLmError;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(face_normals_kernel, dim3(blocks_of(nf)), dim3(kCT), 0, stream, d_vertices, (int)nv, d_faces, (int)nf, d_normals);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int pixel_map_run(const PixelMapArgs &a) {
  const char *who = kWhoMap;
  // ---- refused before any HIP call ----
  if (mesh_refused(who, a.d_vertices, a.nv, a.d_faces, a.nf)) return kLmError;
  if (!a.model_view || !a.projection || !a.viewport || !a.d_pixel_map) {
    set_error("%s(): null model_view, projection, viewport or pixel_map", who);
    return kLmError;
  }
  if (a.H < 1 || a.W < 1 || (long long)a.H * a.W > INT_MAX) {
    set_error("%s(): H = %d, W = %d: need H, W >= 1 and H W <= INT_MAX", who, a.H, a.W);
    return kLmError;
  }
  if ((a.mode != 0 && a.mode != 1) || (a.cull != 0 && a.cull != 1)) {
    set_error("%s(): mode = %d, cull = %d: need 0 or 1 each", who, a.mode, a.cull);
    return kLmError;
  }
  Camera cam;
  for (int i = 0; i < 16; ++i) {
    cam.mv[i] = a.model_view[i];
    cam.pr[i] = a.projection[i];
    if (!std::isfinite(cam.mv[i]) || !std::isfinite(cam.pr[i])) {
      set_error("%s(): model_view[%d] = %g, projection[%d] = %g: need finite matrices", who, i, cam.mv[i], i, cam.pr[i]);
      return kLmError;
    }
  }
  for (int i = 0; i < 4; ++i) {
    cam.vp[i] = a.viewport[i];
    if (!std::isfinite(cam.vp[i]) || (i >= 2 && cam.vp[i] <= 0.0)) {
      set_error("%s(): viewport[%d] = %g: need a finite viewport of positive width and height", who, i, cam.vp[i]);
      return kLmError;
    }
  }
  (void)hipGetLastError();
  hipStream_t stream = a.stream;
  const int nf = (int)a.nf;
  const long long pixels = (long long)a.H * a.W, nb = blocks_of(nf);
  // one allocation: the counters, then mode 0's centroid depths or mode 1's depth map, records and offsets
  const size_t at_stats = 0, at_a = 256, at_rec = at_a + sizeof(long long) * (size_t)pixels, at_local = at_rec + sizeof(FaceRec) * (size_t)nf,
               at_off = at_local + sizeof(long long) * (size_t)nf;
  const size_t bytes = a.mode == 0 ? at_a + sizeof(double) * (size_t)nf : at_off + sizeof(long long) * (size_t)(nb + 1);
  DevBuf ws;
  if (!take(ws, bytes, "the workspace", who)) return kLmError;
  unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(ws.ptr + at_stats);
  CAPTURE_OK(who, hipMemsetAsync(d_stats, 0, sizeof(long long) * kPixelMapStats, stream));
  CAPTURE_OK(who, hipMemsetAsync(a.d_pixel_map, 0xff, sizeof(int) * (size_t)pixels, stream));
  if (a.d_face_pixels) CAPTURE_OK(who, hipMemsetAsync(a.d_face_pixels, 0, sizeof(int) * (size_t)nf, stream));
  FinishCtx fc = {a.d_pixel_map, pixels, nf, nullptr, nullptr, a.d_depth, a.d_face_pixels, d_stats};
  if (a.mode == 0) {
    double *face_z = reinterpret_cast<double *>(ws.ptr + at_a);
    const CentroidCtx c = {a.d_vertices, a.d_faces, (int)a.nv, nf, a.H, a.W, cam, a.d_pixel_map, face_z, d_stats};
    hipLaunchKernelGGL(centroid_kernel, dim3((unsigned)nb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    fc.face_z = face_z;
  } else {
    unsigned long long *zmap = reinterpret_cast<unsigned long long *>(ws.ptr + at_a);
    CAPTURE_OK(who, hipMemsetAsync(zmap, 0xff, sizeof(long long) * (size_t)pixels, stream));
    const RasterCtx c = {a.d_vertices, a.d_faces, (int)a.nv, nf, a.H, a.W, a.cull, nb, cam, reinterpret_cast<FaceRec *>(ws.ptr + at_rec),
                         reinterpret_cast<long long *>(ws.ptr + at_local), reinterpret_cast<long long *>(ws.ptr + at_off), zmap,
                         reinterpret_cast<unsigned *>(a.d_pixel_map), d_stats};
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)nb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(kCT), 0, stream, c.block_off, nb, d_stats);
    CAPTURE_OK(who, hipGetLastError());
    // T is the device's to know: the grid is sized by its upper bound nf H W, the loop by T
    const double bound = (double)nf * (double)pixels / kCT + 1.0;
    const unsigned grid = bound < (double)kGridCap ? (unsigned)bound : kGridCap;
    hipLaunchKernelGGL(candidates_kernel<false>, dim3(grid), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    hipLaunchKernelGGL(candidates_kernel<true>, dim3(grid), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    fc.zmap = zmap;
  }
  hipLaunchKernelGGL(finish_kernel, dim3(blocks_of(pixels)), dim3(kCT), 0, stream, fc);
  CAPTURE_OK(who, hipGetLastError());
  long long h_stats[kPixelMapStats];
  CAPTURE_OK(who, hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  if (a.stats)
    for (int k = 0; k < kPixelMapStats; ++k) a.stats[k] = h_stats[k];
  return 0;
}

}  // namespace brdf
