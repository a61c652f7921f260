// capture_face_major.hip -- the face-major samples of a grouped capture and the carried faces' residuals over them, ONE text under
// brdf_hip_fit_capture_single_faces_dev (capture_single_faces.hip, M = 1) and the three materials entries (capture_materials.hip).
//
// (compact, group and cosines are capture_group.hip's; the candidate reader, the channel compaction and the scan are capture_compact.h's)
//   face-major  the candidates of a channel are ONE flat array, t = sorted pixel * L + light (capture_faces.hip's), and a channel's
//               samples are one stream compaction of it: ballot + popcount and block counts (pass 0), one scan, then the faces'
//               offsets seg[c][F + 1] alone (pass 1) or with the planes [3][K_c] and measurements [K_c] (pass 2).  The channel totals
//               K_c are the scan's, so ONE placing pass writes the single-fit layout.
//   residuals   a face's samples are cut into chunks of kRC counted from the face's OWN first sample; one wavefront per chunk: lane l
//               adds samples l, l + 64, ... in ascending order, one DPP tree over the lanes per material; one thread per
//               (face, material) adds the chunks' partial sums in ascending order.  Column m depends on the face's samples, their
//               order and materials[m] only: not on M, not on where m stands.  No float atomics.  The chunk of a wavefront comes from
//               one scan of the faces' chunk counts and a binary search in it.
// Every candidate pass evaluates the same rule on the same bytes, so the places of the later passes are the counts of pass 0.
#include <algorithm>
#include <climits>

#include "capture_face_major.h"

namespace brdf {

namespace {

constexpr int kRC = 1024;   // samples of a residual chunk: 16 per lane of its wavefront
constexpr int kAlign = 32;  // doubles: every channel's planes and measurements start on a 256-byte boundary
constexpr int kMG = kMaterialGroup;

// ---- face-major: count, offsets, place ----------------------------------------------------------------------------------------
// Candidate t = (sorted pixel, light) of all three channels (capture_compact.h: read_candidate).
//   PASS 0  the block's number of valid candidates per channel
//   PASS 1  at a face's first candidate the face's offset (the prefix there)
//   PASS 2  that, and the plane triple and the measurement to their place
template <int PASS>
__global__ __launch_bounds__(kCT) void face_pack_kernel(FacePackCtx c) {
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
    if (PASS == 2 && k.valid[ch]) {  // (at < K[ch]: the rule of pass 0 on the same bytes)
      const long long n = c.K[ch];
      double *dst = c.ang[ch] + at;
      dst[0] = k.c0;
      dst[n] = k.c1;
      dst[2 * n] = k.c2;
      c.x[ch][at] = k.v[ch] / 255.0;  // "intensity.val[colorChannel]/255.0", brdfdata.cpp:956
    }
  }
}

// ---- residuals ------------------------------------------------------------------------------------------------------------------
// One workgroup per channel (blockIdx.x) over the carried faces: chunk_first[c][r] = the chunks of the faces below rank r, [c][F]: all
__global__ __launch_bounds__(kCT) void chunk_scan_kernel(const long long *__restrict__ seg_all, int F, long long *__restrict__ chunk_first_all) {
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

struct MaterialResidCtx {
  const double *ang, *x;  // one channel: planes [3][K], measurements [K]
  long long K;
  const long long *seg, *chunk_first;  // [F + 1] each, the channel's
  int F, ch, M;
  long long max_chunks;     // `partial` holds max_chunks * M
  const double *materials;  // [M][3][3]
  double *partial;          // [chunks][M]
};

// One wavefront per chunk: sum (x - f(materials[m][ch]))^2 over the chunk's samples for every m, f on the EXACT model path (the
// reference's own pow expression), as fit_stats.hip's e = x - f.  The materials are taken G at a time: their uniforms in scalar
// registers, one accumulator each per lane, the chunk's samples read once per group.  Per material, lane l adds samples l, l + 64, ...
// of the chunk in that order and one DPP tree folds the lanes: the group size moves no bit of a sum.  G = kMaterialGroup, and G = 1
// for a table of one material (the single-BRDF capture: one accumulator's registers, a wave more per SIMD).
template <int MODEL, int G>
__global__ __launch_bounds__(kCT) void material_resid_kernel(MaterialResidCtx c) {
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
  const double *a0 = c.ang, *a1 = c.ang + c.K, *a2 = c.ang + 2 * c.K;
  for (int m0 = 0; m0 < c.M; m0 += G) {  // wave-uniform
    const int gm = c.M - m0 < G ? c.M - m0 : G;
    EvalUniforms u[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const double *pm = c.materials + ((size_t)(m0 + (j < gm ? j : 0)) * 3 + c.ch) * kM;  // (behind the group's end: its first, unused)
      const double p[kM] = {pm[0], pm[1], pm[2]};
      u[j].l0 = Mdl::lin(p);
      u[j].n0 = Mdl::nl(p);
      u[j].scal = 1.0;
      u[j] = scalar_copy(u[j]);
    }
    double acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.0;
    for (long long i = first + lane; i < last; i += kWave) {
      const double c0 = a0[i];
      const double c1 = Mdl::uses_c1 ? a1[i] : 1.0;
      const double c2 = Mdl::uses_c2 ? a2[i] : 1.0;
      const double xi = c.x[i];
      const Prep q = Mdl::template prepare<false>(c0, c1, c2);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (j < gm) {
          const double e = xi - model_value<MODEL, false>(u[j], c0, q);
          acc[j] += e * e;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (j < gm) {
        const double s = wave_reduce_to_last<OpSum>(acc[j]);
        if (lane == kWave - 1) c.partial[(size_t)w * c.M + m0 + j] = s;
      }
    }
  }
}

struct MaterialFoldCtx {
  int F, M;
  const int *face_list;                // [F]
  const long long *seg, *chunk_first;  // [3][F + 1]
  const double *partial[3];            // [chunks][M]
  double *sumsq;   // rows of [M][3], or null
  int by_rank;     // sumsq's row: the face's rank (the loop's own map), otherwise the face
  int *count;      // [nf][3] or null
};

// One thread per (carried face, material): the chunks' partial sums in ascending order, channel after channel
__global__ __launch_bounds__(kCT) void material_fold_kernel(MaterialFoldCtx c) {
  const long long idx = (long long)blockIdx.x * kCT + threadIdx.x;
  if (idx >= (long long)c.F * c.M) return;
  const long long r = idx / c.M;
  const int m = (int)(idx - r * c.M);
  const size_t face = (size_t)c.face_list[r], row = c.by_rank ? (size_t)r : face;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long long *seg = c.seg + (size_t)ch * (c.F + 1), *cf = c.chunk_first + (size_t)ch * (c.F + 1);
    double s = 0.0;
    for (long long j = cf[r]; j < cf[r + 1]; ++j) s += c.partial[ch][(size_t)j * c.M + m];
    if (c.sumsq) c.sumsq[(row * c.M + m) * 3 + ch] = s;
    if (c.count && m == 0) c.count[face * 3 + ch] = (int)(seg[r + 1] - seg[r]);
  }
}

typedef void (*ResidKernel)(MaterialResidCtx);
ResidKernel resid_kernel_of(int model, int M) {
  static const ResidKernel t[2][MODEL_COUNT] = {{material_resid_kernel<0, kMG>, material_resid_kernel<1, kMG>, material_resid_kernel<2, kMG>},
                                                {material_resid_kernel<0, 1>, material_resid_kernel<1, 1>, material_resid_kernel<2, 1>}};
  return t[M == 1][model];
}

}  // namespace

int face_major_run(const char *who, const CaptureGrouped &ga, FaceMajor &fm, bool with_data) {
  hipStream_t stream = ga.cap.stream;
  if (capture_group_run(who, ga, fm.g) != 0) return kLmError;
  if (fm.g.S == 0) return 0;
  const long long F = fm.F = fm.g.F;
  FacePackCtx &pc = fm.pc;
  pc.cand = capture_candidates(ga, fm.g);
  const long long T = fm.T = pc.cand.T;
  const int pb = fm.pb = (int)((T + kCT - 1) / kCT);
  if (!take(fm.pack_count, sizeof(int) * 3 * (size_t)pb, "the candidate blocks' counts", who) ||
      !take(fm.pack_off, sizeof(long long) * 3 * (size_t)pb, "the candidate blocks' offsets", who) ||
      !take(fm.seg, sizeof(long long) * 3 * ((size_t)F + 1), "the faces' offsets", who) ||
      !take(fm.totals, sizeof(long long) * 3, "the channels' totals", who))
    return kLmError;
  pc.block_count = fm.pack_count.as<int>();
  pc.block_off = fm.pack_off.as<long long>();
  pc.seg = fm.seg.as<long long>();
  hipLaunchKernelGGL(face_pack_kernel<0>, dim3(pb), dim3(kCT), 0, stream, pc);
  // every channel from 0: its end is K_c, also the end of the channel's face offsets, seg[c][F]
  hipLaunchKernelGGL(block_scan3_kernel<false>, dim3(1), dim3(kCT), 0, stream, fm.pack_count.as<int>(), (long long)pb, fm.pack_off.as<long long>(),
                     fm.seg.as<long long>() + F, F + 1, fm.totals.as<long long>());
  CAPTURE_OK(who, hipGetLastError());
  if (!with_data) hipLaunchKernelGGL(face_pack_kernel<1>, dim3(pb), dim3(kCT), 0, stream, pc);  // (needs no K_c: in the wait's shadow)
  CAPTURE_OK(who, hipMemcpyAsync(fm.K, fm.totals.ptr, sizeof fm.K, hipMemcpyDeviceToHost, stream));
  CAPTURE_OK(who, hipStreamSynchronize(stream));
  for (int c = 0; c < 3; ++c) {
    if (fm.K[c] < 0 || fm.K[c] > T) {
      set_error("%s(): the count finds %lld valid samples among %lld candidates of channel %d", who, fm.K[c], T, c);
      return kLmError;
    }
    if (fm.K[c] > INT_MAX) {  // a fit's count is an int
      set_error("%s(): channel %d has %lld samples, more than INT_MAX", who, c, fm.K[c]);
      return kLmError;
    }
  }
  if (!with_data) return 0;
  size_t start[3], doubles = 0;  // a channel's planes, then its measurements
  for (int c = 0; c < 3; ++c) {
    start[c] = doubles;
    doubles += (4 * (size_t)fm.K[c] + kAlign - 1) / kAlign * kAlign;
  }
  if (!take(fm.packed, sizeof(double) * std::max<size_t>(doubles, 1), "the channels' planes and measurements", who)) return kLmError;
  for (int c = 0; c < 3; ++c) {
    pc.ang[c] = fm.packed.as<double>() + start[c];
    pc.x[c] = pc.ang[c] + 3 * (size_t)fm.K[c];
    pc.K[c] = fm.K[c];
  }
  hipLaunchKernelGGL(face_pack_kernel<2>, dim3(pb), dim3(kCT), 0, stream, pc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int residuals_prepare(const char *who, const FaceMajor &fm, int M, hipStream_t stream, Residuals &rs) {
  rs.M = M;
  size_t pdoubles = 0;
  for (int c = 0; c < 3; ++c) {
    rs.max_chunks[c] = fm.K[c] / kRC + fm.F;  // sum over the faces of ceil(k / kRC)
    rs.pstart[c] = pdoubles;
    pdoubles += (size_t)rs.max_chunks[c] * (size_t)M;
    if ((rs.max_chunks[c] + kWaves - 1) / kWaves > INT_MAX) {
      set_error("%s(): %lld residual chunks of channel %d are more than one launch walks", who, rs.max_chunks[c], c);
      return kLmError;
    }
  }
  if ((fm.F * M + kCT - 1) / kCT > INT_MAX) {
    set_error("%s(): %lld carried faces times %d materials are more than one launch walks", who, fm.F, M);
    return kLmError;
  }
  if (!take(rs.chunk_first, sizeof(long long) * 3 * ((size_t)fm.F + 1), "the faces' first chunks", who) ||
      !take(rs.partial, sizeof(double) * pdoubles, "the chunks' partial sums", who))
    return kLmError;
  hipLaunchKernelGGL(chunk_scan_kernel, dim3(3), dim3(kCT), 0, stream, fm.seg.as<long long>(), (int)fm.F, rs.chunk_first.as<long long>());
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int residuals_enqueue(const char *who, const FaceMajor &fm, const Residuals &rs, int model, const double *d_materials, hipStream_t stream,
                      double *sumsq, bool by_rank, int *count) {
  const long long F = fm.F;
  MaterialFoldCtx fc = {};
  fc.F = (int)F;
  fc.M = rs.M;
  fc.face_list = fm.g.face_list.as<int>();
  fc.seg = fm.seg.as<long long>();
  fc.chunk_first = rs.chunk_first.as<long long>();
  fc.sumsq = sumsq;
  fc.by_rank = by_rank ? 1 : 0;
  fc.count = count;
  for (int c = 0; c < 3; ++c) {
    MaterialResidCtx rc = {};
    rc.ang = fm.pc.ang[c];
    rc.x = fm.pc.x[c];
    rc.K = fm.K[c];
    rc.seg = fm.seg.as<long long>() + (size_t)c * (F + 1);
    rc.chunk_first = rs.chunk_first.as<long long>() + (size_t)c * (F + 1);
    rc.F = (int)F;
    rc.ch = c;
    rc.M = rs.M;
    rc.max_chunks = rs.max_chunks[c];
    rc.materials = d_materials;
    rc.partial = rs.partial.as<double>() + rs.pstart[c];
    fc.partial[c] = rc.partial;
    if (sumsq) hipLaunchKernelGGL(resid_kernel_of(model, rs.M), dim3(blocks_of(rs.max_chunks[c] * kWave)), dim3(kCT), 0, stream, rc);
  }
  hipLaunchKernelGGL(material_fold_kernel, dim3(blocks_of(F * rs.M)), dim3(kCT), 0, stream, fc);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

}  // namespace brdf
