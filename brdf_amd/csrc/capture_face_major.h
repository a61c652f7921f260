// capture_face_major.h -- the face-major samples of a grouped capture and the carried faces' residuals over them
// (capture_face_major.hip), shared by capture_single_faces.hip and capture_materials.hip.  Declarations only: the kernels are
// capture_face_major.hip's.
//   face-major  the candidates of a channel are ONE flat array, t = sorted pixel * L + light (capture_faces.hip's), and a channel's
//               samples are one stream compaction of it: the planes [3][K_c] and measurements x [K_c] per channel, and where a face's
//               samples start in the channel, seg[c][F + 1]
//   residuals   a face's samples in chunks of 1024 counted from the face's OWN first sample, chunk_first[c][F + 1]; per material one
//               sum of squared residuals per (carried face, channel)
#pragma once

#include "capture_group.h"

namespace brdf {

constexpr int kMaterialGroup = 4;  // materials a residual chunk evaluates per read of its samples

inline unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

struct FacePackCtx {
  CandidateCtx cand;
  int *block_count;            // [blocks][3]                                                              (pass 0 writes)
  const long long *block_off;  // [blocks][3]: the place IN ITS CHANNEL of the block's first valid candidate  (block_scan3_kernel<false>)
  long long *seg;              // [3][F + 1]: where a face's samples start in the channel                   (pass 1, 2 write [c][0, F))
  double *ang[3], *x[3];       // the channels' planes [3][K_c] and measurements [K_c]                      (pass 2 writes)
  long long K[3];
};

struct FaceMajor {
  CaptureGroup g;
  FacePackCtx pc = {};
  int pb = 0;
  long long F = 0, T = 0, K[3] = {0, 0, 0};
  DevBuf pack_count, pack_off, seg, totals, packed;
};

// group, count, scan, place.  with_data: the planes and measurements too (32 bytes per valid sample).  fm.g.S == 0: an empty capture
int face_major_run(const char *who, const CaptureGrouped &ga, FaceMajor &fm, bool with_data);

struct Residuals {
  int M = 0;
  long long max_chunks[3] = {0, 0, 0};
  size_t pstart[3] = {0, 0, 0};
  DevBuf chunk_first, partial;
};

// the chunks of the face-major samples and room for M partial sums each: 8 M bytes per chunk
int residuals_prepare(const char *who, const FaceMajor &fm, int M, hipStream_t stream, Residuals &rs);

// one residual pass against d_materials [M][3][3]: sumsq rows by face ([nf][M][3]) or by rank ([F][M][3]), count [nf][3]; each or null
int residuals_enqueue(const char *who, const FaceMajor &fm, const Residuals &rs, int model, const double *d_materials, hipStream_t stream,
                      double *sumsq, bool by_rank, int *count);

}  // namespace brdf
