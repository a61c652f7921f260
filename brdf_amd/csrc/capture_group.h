// capture_group.h -- the host layer the capture entries share (capture_group.hip): the pixel compaction of all of them; the grouping by
// face of the per-face entries (capture_faces.hip, capture_means.hip, capture_single_faces.hip), their argument check, their candidates,
// their result buffers and their scatter.  Declarations only: the kernels and rocPRIM's sort are capture_group.hip's.
#pragma once

#include "capture_compact.h"
#include "capture_fit.h"
#include "fit_host.h"

namespace brdf {

using DevBuf = DeviceBlock<char>;  // scoped: bytes

// a failed HIP call becomes the error text of the entry `who` and kLmError
#define CAPTURE_OK(who, call)                                                 \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) {                                                   \
      set_error("%s(): %s failed: %s", who, #call, hipGetErrorString(e_));    \
      return kLmError;                                                        \
    }                                                                         \
  } while (0)

// `bytes` of device memory for `what`; a failure names the entry `who` and the bytes asked for
bool take(DevBuf &b, size_t bytes, const char *what, const char *who);

// ---- the pixel compaction ------------------------------------------------------------------------------------------------------
// The pixels that carry a face, in the reference's x-major walk: count per block, prefix on the host, place (deterministic).  With a
// pixel's place, one statistic of its face, by an integer atomic (the order cannot show):
enum class FaceStat {
  kLastPixel,   // long long [nf]: 1 + the place of the face's last pixel (atomicMax; 0: no pixel)
  kPixelCount,  // int [nf]: the face's pixels (atomicAdd)
};
struct PixelCompaction {
  FaceStat stat;             // the caller's: which statistic,
  void *d_face_stat;         //   where (zeroed by the caller on the stream),
  long long max_S;           //   and the most pixels the caller takes: its own refusal follows where S is larger
  long long S = 0;           // the pixels that carry a face
  DevBuf counts, block_off;  // the pixel blocks' counts and offsets
  std::vector<long long> h_off;  // (the offsets on the host: read by a copy the stream may still hold)
  DevBuf pixel_of, face_s;   // [S] long long: x-major index, in walk order; [S] int: its face.  Set where 0 < S <= max_S
};
// Counts, waits for a.stream and -- where 0 < S <= max_S -- places.  0, or kLmError with the error text: a HIP failure, or an
// H x W that one launch cannot walk.
int capture_compact_run(const char *who, const CaptureArgs &a, PixelCompaction &c);

// avg[k] = (the sum of d_block_sums[b][k] in ascending b) / (3 nf): "avg_kd/(m_faces.rows()*3)", brdfdata.cpp:1224-1226.  Waits for
// a.stream; avg: or null
int capture_average(const char *who, const CaptureArgs &a, const double *d_block_sums, int blocks, double *avg);

// ---- the grouping by face ---------------------------------------------------------------------------------------------------
// What the per-face captures refuse before any HIP call, under the entry's name `who`: a null required pointer (`out`, the entry's
// required output, is called `out_name`), L outside [1, max_L] (`l_note`: what the text says about the bound), H, W or nf <= 0,
// 3 nf > INT_MAX, an unknown model, a bad validity rule, lb > ub.
int capture_args_check(const char *who, const CaptureGrouped &a, const void *out, const char *out_name, int max_L = 64, const char *l_note = "");

// what capture_group_run leaves: S carried pixels grouped by face, F carried faces (S == 0: an empty capture, nothing else is set)
struct CaptureGroup {
  long long S = 0, F = 0, max_pixels = 0;  // max_pixels: the pixels of the largest face
  PixelCompaction walk;                    // the carried pixels in walk order
  DevBuf face_pixels, sort_tmp;            // [nf]: the faces' pixel counts; the sort's scratch
  DevBuf pixel_sorted, face_sorted;        // [S] long long: x-major pixel index, grouped by face; [S] unsigned: its face
  DevBuf face_list, face_first, rank_of_face;  // [F] int ascending; [F + 1] long long; [nf] int (-1: no pixel carries the face)
  DevBuf head;                             // 2 long long: {F, max_pixels}
  DevBuf angles_f;                         // [F][3][L] double
};
// Groups the capture `a` for the entry `who` and waits for the stream.  Writes a.d_face_pixels (where asked for) and the host scalars
// n_pixels and n_faces.  0, or kLmError with the error text; g.S == 0 on return 0: no pixel carries a face, the caller is done.
int capture_group_run(const char *who, const CaptureGrouped &a, CaptureGroup &g);
// the candidates of the grouped capture (capture_compact.h)
CandidateCtx capture_candidates(const CaptureGrouped &a, const CaptureGroup &g);

// ---- results and scatter ------------------------------------------------------------------------------------------------------
// the batch's optional per-fit results, rows channel * F + face rank: allocated where the call asks for the map
struct FitResultBufs {
  DevBuf info, ret, covar, stats, rank;
};
bool take_fit_results(FitResultBufs &b, const CaptureFacesArgs &a, size_t fits, const char *who);

// rows (carried face, channel) of the [nf][3] maps <- the batch's rows channel * F + face rank; avg from block sums of p in a fixed order
struct ScatterArgs {
  const CaptureFacesArgs *a;  // the maps
  const CaptureGroup *g;
  const double *p;            // [3 F][3]
  const FitResultBufs *res;
  const long long *offsets;   // [3 F + 1]: the count of fit s is offsets[s + 1] - offsets[s]; or null: nobs[s]
  const int *nobs;
  const int *lights;          // the source of s_lights
  int *s_lights;              // [nf][3] or null
};
int capture_scatter_run(const char *who, const ScatterArgs &s);  // waits for the stream

}  // namespace brdf
