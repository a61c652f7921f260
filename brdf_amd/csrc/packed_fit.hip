// packed_fit.hip -- packed batches (packed_fit.h): fits of any size in one call, bucketed by size class inside the library.
//
//   plan      count and class of every fit (packed_plan.h), per-class fit counts and largest counts; a stable partition of the fit
//             indices by class, ascending inside a class (a uniform batch maps to the identity): count / scan / place, the two-pass
//             compaction capture_fit.hip uses for pixels.  The host reads six counts and six maxima back -- the call's one wait.
//   class 0..4  in chunks of what the workspace holds: a segmented gather into padded rows of the class's largest count (padding left
//             unwritten: the ragged kernels never read it), the EXISTING ragged launch (batch_fit_enqueue / fit_stats_enqueue with
//             d_counts), a scatter of the results to the caller's rows.  The stride is never above the class bound, so the class's own
//             kernel is chosen, and inside its class a ragged fit has the bytes of the uniform call at n = count.
//   class 5   zero copy: a fit's segment already is the single-fit layout; stream_fit_run with n = k_s on the caller's memory (the
//             loop of the uniform call above 4096 samples, big_fits_run), one download of the starting points before the loop, one upload of the results after it.
//
// The phases are ordered by kernel boundaries only.  Atomics: integer adds and maxima on counters whose order cannot show.
#include <climits>
#include <vector>

#include "../../include/brdf_levmar.h"
#include "fit_host.h"
#include "fit_stats.h"
#include "packed_fit.h"

namespace brdf {

namespace {

constexpr int kPT = 256;
constexpr int kScatterLanes = 32;  // lanes per fit of the scatter: two double rows (3 + 10 or 9 + 8 values) and one int

thread_local PackedLastStats g_last = {};

// a fit's own count: the difference of its offsets, or 0 -- levmar's n < m refusal -- where they decrease or differ by more than an int
__device__ __forceinline__ int packed_count(const long long *__restrict__ off, long long s) {
  const long long k = off[s + 1] - off[s];
  return (k < 0 || k > 0x7fffffffLL) ? 0 : (int)k;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// pass 1: per block, the number of fits of every class; per class, the largest count
__global__ __launch_bounds__(kPT) void packed_count_kernel(const long long *__restrict__ off, int S, int *__restrict__ block_hist,
                                                           int *__restrict__ class_max) {
  __shared__ int hist[kPackedClasses], mx[kPackedClasses];
  if (threadIdx.x < kPackedClasses) hist[threadIdx.x] = mx[threadIdx.x] = 0;
  __syncthreads();
  const long long s = (long long)blockIdx.x * kPT + threadIdx.x;
  if (s < S) {
    const int k = packed_count(off, s), c = packed_class(k);
    atomicAdd(&hist[c], 1);
    atomicMax(&mx[c], k);
  }
  __syncthreads();
  if (threadIdx.x < kPackedClasses) {
    block_hist[(size_t)blockIdx.x * kPackedClasses + threadIdx.x] = hist[threadIdx.x];
    if (mx[threadIdx.x] > 0) atomicMax(&class_max[threadIdx.x], mx[threadIdx.x]);
  }
}

// the scan between the passes, one workgroup: block_hist[b][c] becomes the place of block b's first fit of class c in perm[] (class c
// starts where the classes below it end); plan[0..5] the classes' fit counts, plan[6..11] their largest counts
__global__ __launch_bounds__(kPT) void packed_scan_kernel(int *__restrict__ block_hist, int nb, const int *__restrict__ class_max,
                                                          long long *__restrict__ plan) {
  __shared__ long long part[kPT][kPackedClasses];
  __shared__ long long base[kPackedClasses];
  const int t = threadIdx.x, per = (nb + kPT - 1) / kPT;
  const long long b0 = (long long)t * per, b1 = b0 + per < nb ? b0 + per : nb;
  long long sum[kPackedClasses];
#pragma unroll
  for (int c = 0; c < kPackedClasses; ++c) sum[c] = 0;
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int c = 0; c < kPackedClasses; ++c) sum[c] += block_hist[b * kPackedClasses + c];
  }
#pragma unroll
  for (int c = 0; c < kPackedClasses; ++c) part[t][c] = sum[c];
  __syncthreads();
  if (t < kPackedClasses) {  // thread c: the exclusive scan of class c over the threads' ranges
    long long run = 0;
    for (int i = 0; i < kPT; ++i) {
      const long long v = part[i][t];
      part[i][t] = run;
      run += v;
    }
    base[t] = run;  // (the class's total, for now)
    plan[t] = run;
    plan[kPackedClasses + t] = class_max[t];
  }
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int c = 0; c < kPackedClasses; ++c) {
      const long long v = base[c];
      base[c] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kPackedClasses; ++c) sum[c] = base[c] + part[t][c];
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int c = 0; c < kPackedClasses; ++c) {
      const int v = block_hist[b * kPackedClasses + c];
      block_hist[b * kPackedClasses + c] = (int)sum[c];
      sum[c] += v;
    }
  }
}

// pass 2: fit s takes the next place of its class, in ascending s (ballots inside a wave, the waves of a block in order)
__global__ __launch_bounds__(kPT) void packed_place_kernel(const long long *__restrict__ off, int S, const int *__restrict__ block_off,
                                                           int *__restrict__ perm) {
  __shared__ int wave_cnt[kPT / kWave][kPackedClasses];
  const long long s = (long long)blockIdx.x * kPT + threadIdx.x;
  const int cls = s < S ? packed_class(packed_count(off, s)) : -1;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int rank = 0;
#pragma unroll
  for (int c = 0; c < kPackedClasses; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (lane == 0) wave_cnt[wave][c] = __popcll(m);
    if (cls == c) rank = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (cls < 0) return;
  int at = block_off[(size_t)blockIdx.x * kPackedClasses + cls] + rank;
  for (int w = 0; w < wave; ++w) at += wave_cnt[w][cls];
  perm[at] = (int)s;
}

// ---- gather and scatter ------------------------------------------------------------------------------------------------------
struct GatherCtx {
  const double *angles, *x, *p;
  const long long *off;
  const int *perm;  // the chunk's fits: chunk fit j is fit perm[j]
  int fits, stride;
  double *wa, *wx, *wp;  // [fits][3][stride], [fits][stride], [fits][3]
  int *wc;               // [fits]
};

// Chunk fit j's segment -> its padded rows.  LANES consecutive lanes per fit read consecutive doubles of each of the four streams
// (three planes, the measurements): one 16-lane row per fit in class 0, as mask_rows16_kernel lays fits out; one wavefront per fit
// up to 256 samples; one workgroup per fit above.  A segment starts on an 8-byte boundary, not more: plain double loads.  Entries at
// and behind the count are not written.
template <int LANES>
__global__ __launch_bounds__(kPT) void packed_gather_kernel(GatherCtx c) {
  const long long j = ((long long)blockIdx.x * kPT + threadIdx.x) / LANES;
  const int i0 = threadIdx.x % LANES;
  if (j >= c.fits) return;
  const long long s = c.perm[j], o = c.off[s];
  int k = packed_count(c.off, s);
  if (k > c.stride) k = 0;  // (cannot happen: the stride is the class's largest count.  Nothing is ever written past a row.)
  const double *__restrict__ a = c.angles + 3 * o;
  const double *__restrict__ xs = c.x + o;
  double *__restrict__ wa = c.wa + (size_t)j * 3 * c.stride;
  double *__restrict__ wx = c.wx + (size_t)j * c.stride;
  for (int i = i0; i < k; i += LANES) {
    const double v0 = a[i], v1 = a[(size_t)k + i], v2 = a[2 * (size_t)k + i], vx = xs[i];
    wa[i] = v0;
    wa[c.stride + i] = v1;
    wa[2 * (size_t)c.stride + i] = v2;
    wx[i] = vx;
  }
  if (i0 < kM) c.wp[(size_t)j * kM + i0] = c.p[(size_t)s * kM + i0];
  if (i0 == 0) c.wc[j] = k;
}

struct ScatterCtx {
  const int *perm;
  int fits;
  const double *src0, *src1;  // [fits][w0], [fits][w1]
  double *dst0, *dst1;        // rows perm[j] of the caller's arrays; null: not wanted
  int w0, w1;                 // w0 + w1 < kScatterLanes
  const int *isrc;            // [fits]
  int *idst;
};
__global__ __launch_bounds__(kPT) void packed_scatter_kernel(ScatterCtx c) {
  const long long j = ((long long)blockIdx.x * kPT + threadIdx.x) / kScatterLanes;
  const int e = threadIdx.x % kScatterLanes;
  if (j >= c.fits) return;
  const size_t s = (size_t)c.perm[j];
  if (e < c.w0) {
    if (c.dst0) c.dst0[s * c.w0 + e] = c.src0[(size_t)j * c.w0 + e];
  } else if (e - c.w0 < c.w1) {
    if (c.dst1) c.dst1[s * c.w1 + (e - c.w0)] = c.src1[(size_t)j * c.w1 + (e - c.w0)];
  } else if (e == kScatterLanes - 1) {
    if (c.idst) c.idst[s] = c.isrc[j];
  }
}

// class 5: what the host needs of every large fit -- its index, where it starts, its count -- and its starting point
struct LargeFit {
  long long s, off, k;
  double p[kM];
};
__global__ __launch_bounds__(kPT) void packed_large_kernel(const long long *__restrict__ off, const int *__restrict__ perm, int fits,
                                                           const double *__restrict__ p, LargeFit *__restrict__ out) {
  const int j = blockIdx.x * kPT + threadIdx.x;
  if (j >= fits) return;
  const long long s = perm[j];
  LargeFit f;
  f.s = s;
  f.off = off[s];
  f.k = packed_count(off, s);
  for (int i = 0; i < kM; ++i) f.p[i] = p[(size_t)s * kM + i];
  out[j] = f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
#define PACKED_OK(call)                                                     \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) {                                                 \
      set_error("%s(): %s failed: %s", who, #call, hipGetErrorString(e_));  \
      return kLmError;                                                      \
    }                                                                       \
  } while (0)

// a stream-ordered allocation, given back in stream order when the scope ends (also on an error path)
struct AsyncBuf {
  void *ptr = nullptr;
  hipStream_t stream = nullptr;
  AsyncBuf() = default;
  AsyncBuf(const AsyncBuf &) = delete;
  AsyncBuf &operator=(const AsyncBuf &) = delete;
  ~AsyncBuf() { release(); }
  hipError_t get(size_t bytes, hipStream_t s) {
    release();
    stream = s;
    const hipError_t e = hipMallocAsync(&ptr, bytes ? bytes : 1, s);
    if (e != hipSuccess) ptr = nullptr;
    return e;
  }
  void release() {
    if (ptr) (void)hipFreeAsync(ptr, stream);
    ptr = nullptr;
  }
};

struct Plan {
  AsyncBuf perm;  // [S]: the fit indices, class after class
  long long fits[kPackedClasses], first[kPackedClasses];  // first: where the class starts in perm
  int largest[kPackedClasses];
  const int *perm_of(int cls) const { return static_cast<const int *>(perm.ptr) + first[cls]; }
};

int make_plan(const long long *d_offsets, int S, hipStream_t stream, Plan *pl, const char *who) {
  const int nb = (int)(((long long)S + kPT - 1) / kPT);
  AsyncBuf hist, head;  // block_hist[nb][6]; class_max[6] ints behind plan[12] long longs
  PACKED_OK(hist.get(sizeof(int) * (size_t)nb * kPackedClasses, stream));
  PACKED_OK(head.get(sizeof(long long) * 2 * kPackedClasses + sizeof(int) * kPackedClasses, stream));
  PACKED_OK(pl->perm.get(sizeof(int) * (size_t)S, stream));
  long long *d_plan = static_cast<long long *>(head.ptr);
  int *d_max = reinterpret_cast<int *>(d_plan + 2 * kPackedClasses);
  int *d_hist = static_cast<int *>(hist.ptr);
  PACKED_OK(hipMemsetAsync(d_max, 0, sizeof(int) * kPackedClasses, stream));
  hipLaunchKernelGGL(packed_count_kernel, dim3(nb), dim3(kPT), 0, stream, d_offsets, S, d_hist, d_max);
  hipLaunchKernelGGL(packed_scan_kernel, dim3(1), dim3(kPT), 0, stream, d_hist, nb, d_max, d_plan);
  hipLaunchKernelGGL(packed_place_kernel, dim3(nb), dim3(kPT), 0, stream, d_offsets, S, d_hist, static_cast<int *>(pl->perm.ptr));
  PACKED_OK(hipGetLastError());
  long long h_plan[2 * kPackedClasses];
  PACKED_OK(hipMemcpyAsync(h_plan, d_plan, sizeof h_plan, hipMemcpyDeviceToHost, stream));
  PACKED_OK(hipStreamSynchronize(stream));  // the one wait of a packed call
  long long at = 0;
  for (int c = 0; c < kPackedClasses; ++c) {
    pl->fits[c] = h_plan[c];
    pl->largest[c] = (int)h_plan[kPackedClasses + c];
    pl->first[c] = at;
    at += h_plan[c];
  }
  if (at != S) {
    set_error("%s(): the plan places %lld of %d fits", who, at, S);
    return kLmError;
  }
  return 0;
}

// a chunk's workspace, carved out of one allocation: the doubles first
struct Workspace {
  AsyncBuf buf;
  double *wa, *wx, *wp, *wd0, *wd1;  // wd0 / wd1: info[10] and nothing (the fit), covar[9] and stats[8] (the statistics)
  int *wc, *wi;                      // counts; ret or rank
};
int carve(Workspace *w, long long fits, int stride, hipStream_t stream, const char *who) {
  PACKED_OK(w->buf.get((size_t)fits * (size_t)packed_fit_bytes(stride), stream));
  const size_t f = (size_t)fits;
  w->wa = static_cast<double *>(w->buf.ptr);
  w->wx = w->wa + f * 3 * stride;
  w->wp = w->wx + f * stride;
  w->wd0 = w->wp + f * kM;
  w->wd1 = w->wd0 + f * kInfoSz;  // (info[10] or covar[9] in front of it)
  w->wc = reinterpret_cast<int *>(w->wd1 + f * (kM * kM + kStatsSz));
  w->wi = w->wc + f;
  return 0;
}
static_assert(packed_fit_bytes(16) == 8 * (4 * 16 + kM + kInfoSz + kM * kM + kStatsSz) + 12, "packed_plan.h: the workspace of one fit");

int gather_enqueue(int cls, const GatherCtx &g, hipStream_t stream, const char *who) {
  const int lanes = cls == 0 ? 16 : cls <= 2 ? kWave : kPT;
  const unsigned blocks = (unsigned)(((long long)g.fits * lanes + kPT - 1) / kPT);
  if (lanes == 16) hipLaunchKernelGGL(packed_gather_kernel<16>, dim3(blocks), dim3(kPT), 0, stream, g);
  else if (lanes == kWave) hipLaunchKernelGGL(packed_gather_kernel<kWave>, dim3(blocks), dim3(kPT), 0, stream, g);
  else hipLaunchKernelGGL(packed_gather_kernel<kPT>, dim3(blocks), dim3(kPT), 0, stream, g);
  PACKED_OK(hipGetLastError());
  return 0;
}

int scatter_enqueue(const ScatterCtx &s, hipStream_t stream, const char *who) {
  const unsigned blocks = (unsigned)(((long long)s.fits * kScatterLanes + kPT - 1) / kPT);
  hipLaunchKernelGGL(packed_scatter_kernel, dim3(blocks), dim3(kPT), 0, stream, s);
  PACKED_OK(hipGetLastError());
  return 0;
}

// the large fits of a plan on the host: one launch, one download
int download_large(const Plan &pl, const long long *d_offsets, const double *d_p, hipStream_t stream, std::vector<LargeFit> *out, const char *who) {
  const int n5 = (int)pl.fits[kPackedLargeClass];
  out->resize(n5);
  AsyncBuf d;
  PACKED_OK(d.get(sizeof(LargeFit) * (size_t)n5, stream));
  hipLaunchKernelGGL(packed_large_kernel, dim3((n5 + kPT - 1) / kPT), dim3(kPT), 0, stream, d_offsets, pl.perm_of(kPackedLargeClass), n5, d_p,
                     static_cast<LargeFit *>(d.ptr));
  PACKED_OK(hipGetLastError());
  PACKED_OK(hipMemcpyAsync(out->data(), d.ptr, sizeof(LargeFit) * (size_t)n5, hipMemcpyDeviceToHost, stream));
  PACKED_OK(hipStreamSynchronize(stream));
  return 0;
}

bool common_args_bad(const void *angles, const void *x, const void *offsets, const void *p, int S, long long workspace_bytes, const char *who) {
  if (!angles || !x || !offsets || !p) {
    set_error("%s(): null angles, x, offsets or p", who);
    return true;
  }
  if (S <= 0 || workspace_bytes < 0) {
    set_error("%s(): S = %d, workspace_bytes = %lld: need S > 0 and workspace_bytes >= 0", who, S, workspace_bytes);
    return true;
  }
  return false;
}

// what the fit and the statistics call share
struct PackedIn {
  const double *angles, *x, *p;
  const long long *off;
  long long workspace_bytes;
  hipStream_t stream;
};
// the results of a chunk: two double columns and one int column of its workspace, and the caller's arrays their rows go to
struct Columns {
  double *Workspace::*src0, *Workspace::*src1;
  double *dst0, *dst1;  // null: not wanted
  int w0, w1;
  int *idst;  // from Workspace::wi
};

// Classes 0..4 of the plan: per class the stride, the chunk size and one workspace; per chunk gather, enqueue(w, fits, stride) -- the
// caller's ragged launch on the padded rows --, scatter.
template <class Enqueue>
int run_small_classes(const Plan &pl, const PackedIn &in, const Columns &out, const char *who, Enqueue enqueue) {
  for (int cls = 0; cls < kPackedLargeClass; ++cls) {
    if (pl.fits[cls] == 0) continue;
    const int stride = packed_stride(pl.largest[cls]);
    long long chunk = packed_chunk_fits(in.workspace_bytes, stride);
    if (chunk > pl.fits[cls]) chunk = pl.fits[cls];
    g_last.fits[cls] = pl.fits[cls];
    g_last.stride[cls] = stride;
    Workspace w;
    if (carve(&w, chunk, stride, in.stream, who) != 0) return kLmError;
    for (long long at = 0; at < pl.fits[cls]; at += chunk) {
      const int fits = (int)(pl.fits[cls] - at < chunk ? pl.fits[cls] - at : chunk);
      const int *perm = pl.perm_of(cls) + at;
      const GatherCtx g = {in.angles, in.x, in.p, in.off, perm, fits, stride, w.wa, w.wx, w.wp, w.wc};
      if (gather_enqueue(cls, g, in.stream, who) != 0 || enqueue(w, fits, stride) != 0) return kLmError;
      const ScatterCtx s = {perm, fits, w.*out.src0, w.*out.src1, out.dst0, out.dst1, out.w0, out.w1, w.wi, out.idst};
      if (scatter_enqueue(s, in.stream, who) != 0) return kLmError;
      ++g_last.chunks[cls];
    }
  }
  return 0;
}

// class 5 on the host (one launch, one download), as the fits the single-fit path runs: a segment already is its layout.  row_is_fit:
// a fit's row is its index in the batch (the statistics write there), otherwise its place in the class
int big_fits_of(const Plan &pl, const PackedIn &in, bool row_is_fit, std::vector<LargeFit> *large, std::vector<BigFit> *big, const char *who) {
  if (download_large(pl, in.off, in.p, in.stream, large, who) != 0) return kLmError;
  for (size_t j = 0; j < large->size(); ++j) {
    const LargeFit &f = (*large)[j];
    big->push_back({in.angles + 3 * f.off, in.x + f.off, (int)f.k, (int)f.k, row_is_fit ? f.s : (long long)j});
  }
  g_last.fits[kPackedLargeClass] = g_last.chunks[kPackedLargeClass] = (int)large->size();
  g_last.stride[kPackedLargeClass] = pl.largest[kPackedLargeClass];
  return 0;
}

}  // namespace

PackedLastStats packed_last_stats() { return g_last; }

int packed_fit_check(const PackedFitArgs &a, const char *who) {
  MethodSpec ms;
  if (!known_model_method(a.model, a.method, &ms, who) || common_args_bad(a.d_angles, a.d_x, a.d_offsets, a.d_p, a.S, a.workspace_bytes, who) ||
      box_refused(ms, a.lb, a.ub, who))  // (the whole call, its fits above 4096 samples included: batch_fit_check lets those pass)
    return kLmError;
  return 0;
}

int packed_fit_run(const PackedFitArgs &a, const char *who) {
  if (packed_fit_check(a, who) != 0) return kLmError;
  (void)hipGetLastError();
  g_last = PackedLastStats{};
  Plan pl;
  if (make_plan(a.d_offsets, a.S, a.stream, &pl, who) != 0) return kLmError;
  const PackedIn in = {a.d_angles, a.d_x, a.d_p, a.d_offsets, a.workspace_bytes, a.stream};
  const Columns out = {&Workspace::wp, &Workspace::wd0, a.d_p, a.d_info, kM, kInfoSz, a.d_ret};
  if (run_small_classes(pl, in, out, who, [&](const Workspace &w, int fits, int stride) {
        const BatchFitArgs b = {a.method, a.model, w.wa, w.wx, fits, stride, w.wp, a.lb, a.ub, a.itmax, a.opts, w.wd0, w.wi, a.stream, w.wc};
        return batch_fit_enqueue(b, who);
      }) != 0)
    return kLmError;
  const int n5 = (int)pl.fits[kPackedLargeClass];
  if (n5 == 0) return 0;
  // class 5: the fits run where they lie, one after the other, each spread over the chip (synchronous, as in the uniform call)
  std::vector<LargeFit> large;
  std::vector<BigFit> big;
  if (big_fits_of(pl, in, false, &large, &big, who) != 0) return kLmError;
  // the results, laid out as the scatter reads them: p[n5][3], info[n5][10], then ret[n5]
  std::vector<double> res((size_t)n5 * (kM + kInfoSz) + ((size_t)n5 + 1) / 2);
  double *hp = res.data(), *hinfo = hp + (size_t)n5 * kM;
  int *hret = reinterpret_cast<int *>(hinfo + (size_t)n5 * kInfoSz);
  for (int j = 0; j < n5; ++j)
    for (int i = 0; i < kM; ++i) hp[(size_t)j * kM + i] = large[j].p[i];
  const BatchFitArgs b = {a.method, a.model, a.d_angles, a.d_x, n5, 0, nullptr, a.lb, a.ub, a.itmax, a.opts, nullptr, nullptr, a.stream};
  if (big_fits_run(b, big.data(), n5, hp, hinfo, hret) != 0) return kLmError;
  AsyncBuf d;
  PACKED_OK(d.get(sizeof(double) * res.size(), a.stream));
  PACKED_OK(hipMemcpyAsync(d.ptr, res.data(), sizeof(double) * res.size(), hipMemcpyHostToDevice, a.stream));
  const double *dp = static_cast<const double *>(d.ptr), *dinfo = dp + (size_t)n5 * kM;
  const ScatterCtx s = {pl.perm_of(kPackedLargeClass), n5, dp, dinfo, a.d_p, a.d_info, kM, kInfoSz,
                        reinterpret_cast<const int *>(dinfo + (size_t)n5 * kInfoSz), a.d_ret};
  if (scatter_enqueue(s, a.stream, who) != 0) return kLmError;
  PACKED_OK(hipStreamSynchronize(a.stream));  // (the host vector above is about to go away)
  return 0;
}

int packed_stats_check(const PackedStatsArgs &a, const char *who) {
  MethodSpec ms;
  if (!known_model_method(a.model, a.method, &ms, who) || common_args_bad(a.d_angles, a.d_x, a.d_offsets, a.d_p, a.S, a.workspace_bytes, who))
    return kLmError;
  if (!a.d_covar && !a.d_stats && !a.d_rank) {
    set_error("%s(): covar, stats and rank are all NULL: nothing to compute", who);
    return kLmError;
  }
  return 0;
}

int packed_stats_run(const PackedStatsArgs &a, const char *who) {
  if (packed_stats_check(a, who) != 0) return kLmError;
  (void)hipGetLastError();
  g_last = PackedLastStats{};
  Plan pl;
  if (make_plan(a.d_offsets, a.S, a.stream, &pl, who) != 0) return kLmError;
  const PackedIn in = {a.d_angles, a.d_x, a.d_p, a.d_offsets, a.workspace_bytes, a.stream};
  const Columns out = {&Workspace::wd0, &Workspace::wd1, a.d_covar, a.d_stats, kM * kM, kStatsSz, a.d_rank};
  if (run_small_classes(pl, in, out, who, [&](const Workspace &w, int fits, int stride) {
        const FitStatsArgs f = {a.method, a.model, w.wa, w.wx, fits, stride, w.wp, a.opts, w.wd0, w.wd1, w.wi, nullptr, 0, a.stream, w.wc};
        return fit_stats_enqueue(f, who);
      }) != 0)
    return kLmError;
  if (pl.fits[kPackedLargeClass] == 0) return 0;
  // class 5: the uniform pass with S = 1 on the segment, results straight into the caller's rows
  std::vector<LargeFit> large;
  std::vector<BigFit> big;
  if (big_fits_of(pl, in, true, &large, &big, who) != 0) return kLmError;
  const FitStatsArgs rows = {a.method, a.model, a.d_angles, a.d_x, a.S, 0, a.d_p, a.opts, a.d_covar, a.d_stats, a.d_rank, nullptr, 0, a.stream};
  for (const BigFit &b : big)
    if (big_fit_stats_enqueue(rows, b, b.d_angles, who) != 0) return kLmError;
  return 0;
}

}  // namespace brdf
