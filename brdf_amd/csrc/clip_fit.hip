// clip_fit.hip -- sigma-clipped packed batches (clip_fit.h holds the definition).
//
// The cumulative mask over the CALLER's sample positions is the state of the loop: a clip round walks the caller's batch, one lane per
// sample position, skips what the mask has dropped, and writes the survivors into ONE working batch, which the next statistics call
// reads, and those of the fits the round clipped into a refit batch as well.  So a dropped sample cannot return, the caller's batch is never written, and a position's fit is looked up in
// an array built once (fit_of: a binary search of the offsets per position, 4 bytes per sample and round afterwards, where a search
// per round would walk log2 S offsets again).
//
//   sigma     per fit: the threshold kappa * sigma from the statistics pass's sumsq, the settled flag, the uniforms of f(p)
//   mark      per sample: the exact-path residual against the fit's threshold -> one byte; per fit the survivors, counted by
//             integer atomics (one per run of a fit inside a wave: ballot + popcount)
//   guard     per fit: nothing dropped or fewer than 3 survivors -> settled, the clip is not applied; otherwise the fit's new count.
//             Counted BEFORE anything moves.  Three integer counters tell the host the refits, the dropped samples and the refit
//             batch's samples of the round.
//   scan      one workgroup, one column: the new offsets from the new counts, and the blocks' offsets from the blocks' counts
//   count / place  per sample: the final decision (the guard may have withdrawn a clip), ballot + popcount inside the workgroup,
//             the survivor to its place in the working batch: planes [3][k'] at 3 offsets'[s], measurement at offsets'[s]; the mask.
//             Two columns: every survivor, and the survivors of the fits clipped in this round (the refit batch)
//   take      per fit: the refit's p, info and ret for the fits that were clipped.  The refit is a packed call on the refit batch -- S fits,
//             the ones the round did not clip empty and refused at once -- into temporaries: packed results do not depend on what
//             else is in the batch
//
// No float atomics; the integer ones count, their order cannot show.  Two calls give the same bytes.
#include <climits>
#include <cmath>
#include <type_traits>

#include "../../include/brdf_levmar.h"
#include "capture_group.h"  // (device_common.h first: the device macros of what follows)
#include "brdf_models.h"
#include "clip_fit.h"
#include "fit_stats.h"

namespace brdf {

namespace {

constexpr int kSettled = 1, kClipped = 2;  // a fit's state: settled for good; clipped in this round (its refit is taken)

thread_local ClipLastStats g_clip_last = {};

// the uniforms of f(p) of one fit, as model_value reads them
struct FitUniforms {
  Lin l0;
  Nl n0;
};

struct ClipCtx {
  const double *angles, *x;  // the caller's batch
  const long long *off;      // the caller's offsets [S + 1]
  long long off0, N;         // offsets[0]; the sample positions the batch covers
  int S, round;
  double kappa, sigma_min;
  int *fit_of;               // [N]: the fit of a position, -1 where the offsets name none
  unsigned char *mask;       // [N]: 1 = still in its fit's sample set
  unsigned char *keep;       // [N]: this round's comparison
  const double *p;           // [S][3]
  const double *stats;       // [S][kStatsSz]
  const int *ret;            // [S]
  double *thr;               // [S]
  FitUniforms *uni;          // [S]
  int *state, *kept, *surv, *rounds_used;  // [S]
  int *rkept;                // [S]: the refit batch's counts -- the survivors of a fit clipped in this round, 0 for every other fit
  unsigned long long *head;  // of this round: {fits clipped, samples dropped, samples of the clipped fits that survive}; [3]: 1 + the first fit whose offsets descend
  int *block_count;          // [2][blocks]: the block's survivors; those of them whose fit was clipped in this round
  const long long *block_off;  // [2][blocks + 1]
  long long nb;              // blocks
  const long long *noff;     // [S + 1]: the working batch's offsets
  const long long *roff;     // [S + 1]: the refit batch's
  double *wa, *wx;           // the working batch: every fit's current samples
  double *ra, *rx;           // the refit batch: the current samples of the fits clipped in this round
};

// a fit's own count, as the packed plan reads it: 0 where the offsets decrease or differ by more than an int
__device__ __forceinline__ int count_of(const long long *__restrict__ off, long long s) {
  const long long k = off[s + 1] - off[s];
  return (k < 0 || k > 0x7fffffffLL) ? 0 : (int)k;
}

// ---- built once --------------------------------------------------------------------------------------------------------------
// (descending: or null; set where two neighbouring offsets decrease or differ by more than an int -- the clip rounds refuse such a batch)
__global__ __launch_bounds__(kCT) void clip_init_kernel(const long long *__restrict__ off, int S, int *__restrict__ kept, int *__restrict__ state,
                                                        int *__restrict__ rounds_used, unsigned long long *__restrict__ descending) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= S) return;
  if (kept) kept[s] = count_of(off, s);
  if (state) state[s] = 0;
  if (rounds_used) rounds_used[s] = 0;
  const long long k = off[s + 1] - off[s];
  if (descending && (k < 0 || k > 0x7fffffffLL)) atomicMax(descending, (unsigned long long)s + 1ull);
}

// a mask of ones (rounds = 0)
__global__ __launch_bounds__(kCT) void clip_ones_kernel(unsigned char *__restrict__ mask, long long N) {
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t < N) mask[t] = 1;
}

// position t belongs to the last fit whose offset is not above it (the empty fits in front of it share that offset)
__global__ __launch_bounds__(kCT) void clip_fit_of_kernel(ClipCtx c) {
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  if (t >= c.N) return;
  const long long pos = c.off0 + t;
  int lo = 0, hi = c.S - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (c.off[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  const long long o = c.off[lo];
  const bool inside = o <= pos && pos - o < count_of(c.off, lo) && o >= c.off0 && o + count_of(c.off, lo) <= c.off0 + c.N;
  c.fit_of[t] = inside ? lo : -1;  // (always inside: the offsets ascend, clip_fit_run has checked)
  c.mask[t] = inside ? 1 : 0;
}

// ---- a clip round ------------------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kCT) void clip_sigma_kernel(ClipCtx c) {
  using Mdl = BrdfModel<MODEL>;
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= c.S) return;
  bool settled = (c.state[s] & kSettled) != 0;
  if (!settled) {
    const int k = c.kept[s];
    const double sumsq = c.stats[(size_t)s * kStatsSz];
    if (c.ret[s] < 0 || k < 3 || !isfinite(sumsq)) {
      settled = true;
    } else {
      const double sigma = k > 3 ? fmax(sqrt(sumsq / (double)(k - 3)), c.sigma_min) : c.sigma_min;
      c.thr[s] = c.kappa * sigma;
      const double *p = c.p + (size_t)s * kM;
      c.uni[s] = FitUniforms{Mdl::lin(p), Mdl::nl(p)};
    }
  }
  c.state[s] = settled ? kSettled : 0;
  c.surv[s] = 0;
}

// One lane per sample position.  The lanes of a fit are next to each other, so a wave adds a fit's survivors once per run.
template <int MODEL>
__global__ __launch_bounds__(kCT) void clip_mark_kernel(ClipCtx c) {
  using Mdl = BrdfModel<MODEL>;
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  int s = t < c.N ? c.fit_of[t] : -1;
  if (s >= 0 && (c.state[s] & kSettled)) s = -1;  // a settled fit: nothing to decide
  bool keep = false;
  if (s >= 0 && c.mask[t]) {
    const long long o = c.off[s], i = c.off0 + t - o;
    const size_t k = (size_t)count_of(c.off, s);
    const double *__restrict__ a = c.angles + 3 * o;
    const double c0 = a[i];
    const double c1 = Mdl::uses_c1 ? a[k + i] : 1.0;
    const double c2 = Mdl::uses_c2 ? a[2 * k + i] : 1.0;
    const FitUniforms u = c.uni[s];
    const double e = c.x[o + i] - model_value<MODEL, false>(u, c0, Mdl::template prepare<false>(c0, c1, c2));
    keep = fabs(e) <= c.thr[s];  // (a NaN residual, or a NaN threshold, fails)
  }
  if (t < c.N) c.keep[t] = keep ? 1 : 0;
  const int prev = __shfl_up(s, 1);
  const bool head = lane == 0 || prev != s;
  const unsigned long long heads = __ballot(head), keeps = __ballot(keep);
  if (head && s >= 0) {
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);
    const unsigned long long upto = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1ull) : ~0ull;
    const int n = __popcll(keeps & upto & ~((1ull << lane) - 1ull));
    if (n) atomicAdd(&c.surv[s], n);
  }
}

__global__ __launch_bounds__(kCT) void clip_guard_kernel(ClipCtx c) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= c.S) return;
  c.rkept[s] = 0;
  if (c.state[s] & kSettled) return;
  const int k = c.kept[s], sv = c.surv[s];
  if (sv >= k || sv < 3) {  // nothing dropped; or a clip to fewer than 3 survivors, which is not applied
    c.state[s] = kSettled;
    return;
  }
  c.state[s] = kClipped;
  c.kept[s] = c.rkept[s] = sv;
  c.rounds_used[s] = c.round;
  atomicAdd(&c.head[0], 1ull);
  atomicAdd(&c.head[1], (unsigned long long)(k - sv));
  atomicAdd(&c.head[2], (unsigned long long)sv);
}

// out[i] = the sum of cnt[0, i), i <= n: one workgroup, one column
__global__ __launch_bounds__(kCT) void clip_scan_kernel(const int *__restrict__ cnt, long long n, long long *__restrict__ out) {
  __shared__ long long part[kCT];
  const int t = threadIdx.x;
  const long long per = (n + kCT - 1) / kCT;
  const long long b0 = t * per < n ? t * per : n, b1 = b0 + per < n ? b0 + per : n;
  long long sum = 0;
  for (long long b = b0; b < b1; ++b) sum += cnt[b];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < kCT; ++i) {
      const long long v = part[i];
      part[i] = run;
      run += v;
    }
    out[n] = run;
  }
  __syncthreads();
  sum = part[t];
  for (long long b = b0; b < b1; ++b) {
    out[b] = sum;
    sum += cnt[b];
  }
}

// A survivor's place among the block's: ballot + popcount, the waves of the block in order (capture_compact.h: ChannelPlaces, one column)
__device__ __forceinline__ long long place_of(unsigned long long m, const int *wave_cnt, long long block_off) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  long long at = block_off + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += wave_cnt[w];
  return at;
}

// sample i of the caller's fit s -> sample j of fit s in a batch with offsets off2 (planes [3][n] at 3 off2[s], measurement at off2[s])
__device__ __forceinline__ void move_sample(const ClipCtx &c, int s, long long t, const long long *__restrict__ off2, long long at, double *__restrict__ da,
                                            double *__restrict__ dx) {
  const long long no = off2[s], n = off2[s + 1] - no, j = at - no;
  if (j < 0 || j >= n || no + n > c.N) return;  // (cannot happen: the fits' counts are the blocks' counts, added up another way)
  const long long o = c.off[s], i = c.off0 + t - o;
  const size_t k = (size_t)count_of(c.off, s);
  const double *__restrict__ a = c.angles + 3 * o;
  double *__restrict__ dst = da + 3 * no + j;
  dst[0] = a[i];
  dst[n] = a[k + i];
  dst[2 * n] = a[2 * k + i];
  dx[at] = c.x[o + i];
}

// PASS 0: the block's survivors, and those of them whose fit was clipped in this round.  PASS 1: every survivor to its place in the
// working batch and, where its fit was clipped, in the refit batch; the mask.
template <int PASS>
__global__ __launch_bounds__(kCT) void clip_place_kernel(ClipCtx c) {
  __shared__ int wave_cnt[2][kWaves];
  const long long t = (long long)blockIdx.x * kCT + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int s = t < c.N ? c.fit_of[t] : -1;
  bool keep = s >= 0 && c.mask[t];
  const bool clipped = keep && (c.state[s] & kClipped);
  if (clipped) keep = c.keep[t] != 0;
  const unsigned long long m = __ballot(keep), mr = __ballot(keep && clipped);
  if (lane == 0) {
    wave_cnt[0][wave] = __popcll(m);
    wave_cnt[1][wave] = __popcll(mr);
  }
  __syncthreads();
  if (PASS == 0) {
    if (threadIdx.x < 2) {
      const int *w = wave_cnt[threadIdx.x];
      c.block_count[threadIdx.x * c.nb + blockIdx.x] = w[0] + w[1] + w[2] + w[3];
    }
    return;
  }
  if (t >= c.N) return;
  c.mask[t] = keep ? 1 : 0;
  if (!keep) return;
  move_sample(c, s, t, c.noff, place_of(m, wave_cnt[0], c.block_off[blockIdx.x]), c.wa, c.wx);
  if (clipped) move_sample(c, s, t, c.roff, place_of(mr, wave_cnt[1], c.block_off[c.nb + 1 + blockIdx.x]), c.ra, c.rx);
}
static_assert(kWaves == 4, "clip_place_kernel adds four waves' counts");

// the refit's results of the fits clipped in this round
__global__ __launch_bounds__(kCT) void clip_take_kernel(const int *__restrict__ state, int S, const double *__restrict__ tp, const double *__restrict__ tinfo,
                                                        const int *__restrict__ tret, double *__restrict__ p, double *__restrict__ info, int *__restrict__ ret) {
  const long long s = (long long)blockIdx.x * kCT + threadIdx.x;
  if (s >= S || !(state[s] & kClipped)) return;
  for (int k = 0; k < kM; ++k) p[s * kM + k] = tp[s * kM + k];
  if (info)
    for (int k = 0; k < kInfoSz; ++k) info[s * kInfoSz + k] = tinfo[s * kInfoSz + k];
  ret[s] = tret[s];
}

// (kept null: the fits' own counts, from the offsets; rounds null: 0 -- what a call without clip rounds returns)
__global__ __launch_bounds__(kCT) void clip_scatter_maps_kernel(const int *__restrict__ face_list, int F, const int *__restrict__ kept,
                                                                const int *__restrict__ rounds, const long long *__restrict__ offsets,
                                                                int *__restrict__ s_kept, int *__restrict__ s_rounds) {
  const long long q = (long long)blockIdx.x * kCT + threadIdx.x;
  if (q >= 3LL * F) return;
  const int r = (int)(q / 3), ch = (int)(q - 3LL * r);
  const size_t src = (size_t)ch * F + r, dst = (size_t)face_list[r] * 3 + ch;
  if (s_kept) s_kept[dst] = kept ? kept[src] : count_of(offsets, (long long)src);
  if (s_rounds) s_rounds[dst] = rounds ? rounds[src] : 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// one allocation, carved into aligned pieces
struct Arena {
  DevBuf buf;
  size_t used = 0;
  size_t reserve(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) / 256 * 256;
    return at;
  }
  template <class T>
  T *at(size_t off) const { return reinterpret_cast<T *>(buf.as<char>() + off); }
};

template <class Launch>
void launch_by_model(int model, Launch launch) {
  if (model == MODEL_PHONG) launch(std::integral_constant<int, MODEL_PHONG>());
  else if (model == MODEL_BLINN_PHONG) launch(std::integral_constant<int, MODEL_BLINN_PHONG>());
  else launch(std::integral_constant<int, MODEL_WARD>());
}

unsigned blocks_of(long long n) { return (unsigned)((n + kCT - 1) / kCT); }

}  // namespace

ClipLastStats clip_last_stats() { return g_clip_last; }
void clip_last_stats_set(const ClipLastStats &s) { g_clip_last = s; }

int clip_spec_check(const ClipSpec &c, const char *who) {
  if (!(c.kappa > 0.0) || !(c.sigma_min >= 0.0) || c.rounds < 0 || c.rounds > kClipMaxRounds) {
    set_error("%s(): kappa = %g, sigma_min = %g, rounds = %d: need kappa > 0 (+inf is allowed), sigma_min >= 0 and 0 <= rounds <= %d", who, c.kappa,
              c.sigma_min, c.rounds, kClipMaxRounds);
    return kLmError;
  }
  return 0;
}

int clip_fit_check(const ClipFitArgs &a, const char *who) {
  if (packed_fit_check(a.fit, who) != 0) return kLmError;
  return clip_spec_check(a.clip, who);
}

int clip_scatter_maps(const char *who, const int *d_face_list, int F, const int *d_kept, const int *d_rounds, const long long *d_offsets,
                      int *d_surface_kept, int *d_surface_rounds, hipStream_t stream) {
  if (!d_surface_kept && !d_surface_rounds) return 0;
  hipLaunchKernelGGL(clip_scatter_maps_kernel, dim3(blocks_of(3LL * F)), dim3(kCT), 0, stream, d_face_list, F, d_kept, d_rounds, d_offsets,
                     d_surface_kept, d_surface_rounds);
  CAPTURE_OK(who, hipGetLastError());
  return 0;
}

int clip_fit_run(const ClipFitArgs &a, const char *who) {
  if (clip_fit_check(a, who) != 0) return kLmError;
  (void)hipGetLastError();
  g_clip_last = ClipLastStats{};
  const PackedFitArgs &f = a.fit;
  hipStream_t stream = f.stream;
  const int S = f.S;
  const bool want_stats = a.d_covar || a.d_stats || a.d_rank;

  // ---- the per-fit state of the clip rounds: 8 doubles of statistics, 13 of the refit, 5 of the threshold and uniforms, 2 offsets, 7 ints
  // (rounds = 0 takes none: the packed calls' launches and one small kernel for kept and rounds_used, one more for a mask) ----
  const bool loop = a.clip.rounds > 0;
  Arena fa;
  const size_t o_stats = fa.reserve(sizeof(double) * kStatsSz * S), o_tp = fa.reserve(sizeof(double) * kM * S),
               o_tinfo = fa.reserve(sizeof(double) * kInfoSz * S), o_thr = fa.reserve(sizeof(double) * S), o_uni = fa.reserve(sizeof(FitUniforms) * S),
               o_noff = fa.reserve(sizeof(long long) * ((size_t)S + 1)), o_roff = fa.reserve(sizeof(long long) * ((size_t)S + 1)),
               o_rkept = fa.reserve(sizeof(int) * S), o_state = fa.reserve(sizeof(int) * S), o_kept = fa.reserve(sizeof(int) * S),
               o_surv = fa.reserve(sizeof(int) * S), o_rounds = fa.reserve(sizeof(int) * S), o_ret = fa.reserve(sizeof(int) * S),
               o_tret = fa.reserve(sizeof(int) * S), o_head = fa.reserve(sizeof(unsigned long long) * 4);
  if (loop && !take(fa.buf, fa.used, "the fits' clip state", who)) return kLmError;
  int *ret = f.d_ret || !loop ? f.d_ret : fa.at<int>(o_ret);
  int *kept = a.d_kept || !loop ? a.d_kept : fa.at<int>(o_kept);
  int *rounds_used = a.d_rounds_used || !loop ? a.d_rounds_used : fa.at<int>(o_rounds);
  double *stats = a.d_stats || !loop ? a.d_stats : fa.at<double>(o_stats);

  ClipCtx c = {};
  c.angles = f.d_angles;
  c.x = f.d_x;
  c.off = f.d_offsets;
  c.S = S;
  c.kappa = a.clip.kappa;
  c.sigma_min = a.clip.sigma_min;
  c.p = f.d_p;
  c.stats = stats;
  c.ret = ret;
  c.kept = kept;
  c.rounds_used = rounds_used;
  if (loop) {
    c.thr = fa.at<double>(o_thr);
    c.uni = fa.at<FitUniforms>(o_uni);
    c.state = fa.at<int>(o_state);
    c.surv = fa.at<int>(o_surv);
    c.rkept = fa.at<int>(o_rkept);
    c.head = fa.at<unsigned long long>(o_head);
    c.noff = fa.at<long long>(o_noff);
    c.roff = fa.at<long long>(o_roff);
  }

  // ---- kept, rounds_used; with clip rounds the state, and the check of the offsets ----
  if (kept || loop || rounds_used) {
    if (loop) CAPTURE_OK(who, hipMemsetAsync(c.head + 3, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(clip_init_kernel, dim3(blocks_of(S)), dim3(kCT), 0, stream, f.d_offsets, S, kept, c.state, rounds_used, loop ? c.head + 3 : nullptr);
    CAPTURE_OK(who, hipGetLastError());
  }

  // ---- the batch's extent (with clip rounds or a mask).  The clip rounds give every sample position ONE fit and size the working batch
  // by the extent: offsets that descend, which the packed calls read as a count of 0, are refused here, before anything is written ----
  const long long *cur_off = f.d_offsets;  // the current sample sets: the caller's batch until a round clips
  const double *cur_angles = f.d_angles, *cur_x = f.d_x;
  bool stats_fresh = false;
  Arena sa;
  DevBuf refit;  // the refit batch of a round: 32 bytes per sample of the fits the round clips
  if (loop || a.d_mask) {
    long long ext[2] = {0, 0};
    unsigned long long descending = 0;
    CAPTURE_OK(who, hipMemcpyAsync(&ext[0], f.d_offsets, sizeof(long long), hipMemcpyDeviceToHost, stream));
    CAPTURE_OK(who, hipMemcpyAsync(&ext[1], f.d_offsets + S, sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (loop) CAPTURE_OK(who, hipMemcpyAsync(&descending, c.head + 3, sizeof descending, hipMemcpyDeviceToHost, stream));
    CAPTURE_OK(who, hipStreamSynchronize(stream));
    if (descending) {
      set_error("%s(): offsets descend (or differ by more than INT_MAX) at fit %llu: the clip rounds need ascending offsets", who, descending - 1);
      return kLmError;
    }
    c.off0 = ext[0];
    c.N = ext[1] - ext[0];
    if (c.N < 0 || (c.N + kCT - 1) / kCT > INT_MAX) {
      set_error("%s(): offsets[0] = %lld, offsets[S] = %lld: the batch covers %lld samples, need 0 <= samples <= %lld", who, ext[0], ext[1], c.N,
                (long long)INT_MAX * kCT);
      return kLmError;
    }
  }
  const long long N = c.N;
  const unsigned nb = blocks_of(N);
  if (N > 0 && !loop) {  // rounds = 0 with a mask: ones
    hipLaunchKernelGGL(clip_ones_kernel, dim3(nb), dim3(kCT), 0, stream, a.d_mask, N);
    CAPTURE_OK(who, hipGetLastError());
  }
  if (N > 0 && loop) {  // what a clip round needs per sample position: 38 bytes
    const size_t o_fit_of = sa.reserve(sizeof(int) * (size_t)N), o_mask = sa.reserve(a.d_mask ? 0 : (size_t)N), o_keep = sa.reserve((size_t)N),
                 o_wa = sa.reserve(sizeof(double) * 3 * (size_t)N), o_wx = sa.reserve(sizeof(double) * (size_t)N),
                 o_bc = sa.reserve(sizeof(int) * 2 * (size_t)nb), o_bo = sa.reserve(sizeof(long long) * 2 * ((size_t)nb + 1));
    if (!take(sa.buf, sa.used, "the clip rounds' sample state", who)) return kLmError;
    c.fit_of = sa.at<int>(o_fit_of);
    c.mask = a.d_mask ? a.d_mask : sa.at<unsigned char>(o_mask);
    c.keep = sa.at<unsigned char>(o_keep);
    c.wa = sa.at<double>(o_wa);
    c.wx = sa.at<double>(o_wx);
    c.block_count = sa.at<int>(o_bc);
    c.block_off = sa.at<long long>(o_bo);
    c.nb = nb;
    hipLaunchKernelGGL(clip_fit_of_kernel, dim3(nb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
  }

  // ---- round 0 ----
  PackedFitArgs fit0 = f;
  fit0.d_ret = ret;
  if (packed_fit_run(fit0, who) != 0) return kLmError;

  // ---- the clip rounds ----
  for (int r = 1; r <= a.clip.rounds && N > 0; ++r) {
    // sumsq of every fit at its p over its current samples.  With the caller's maps where they are asked for: should this round
    // settle every fit, they already hold the returned statistics.
    const PackedStatsArgs ps = {f.method, f.model, cur_angles, cur_x, cur_off, S, f.d_p, f.opts, a.d_covar, stats, a.d_rank, f.workspace_bytes, stream};
    if (packed_stats_run(ps, who) != 0) return kLmError;
    stats_fresh = true;
    c.round = r;
    CAPTURE_OK(who, hipMemsetAsync(c.head, 0, sizeof(unsigned long long) * 3, stream));
    launch_by_model(f.model, [&](auto m) {
      hipLaunchKernelGGL(clip_sigma_kernel<decltype(m)::value>, dim3(blocks_of(S)), dim3(kCT), 0, stream, c);
      hipLaunchKernelGGL(clip_mark_kernel<decltype(m)::value>, dim3(nb), dim3(kCT), 0, stream, c);
    });
    hipLaunchKernelGGL(clip_guard_kernel, dim3(blocks_of(S)), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    unsigned long long head[3] = {0, 0, 0};
    CAPTURE_OK(who, hipMemcpyAsync(head, c.head, sizeof head, hipMemcpyDeviceToHost, stream));
    CAPTURE_OK(who, hipStreamSynchronize(stream));  // the round's one readback: is any fit still active?
    g_clip_last.rounds = r;
    g_clip_last.active[r - 1] = (long long)head[0];
    g_clip_last.clipped[r - 1] = (long long)head[1];
    if (head[0] == 0) break;

    if (head[2] > (unsigned long long)N) {
      set_error("%s(): clip round %d keeps %llu samples of %lld", who, r, head[2], N);
      return kLmError;
    }
    if (!take(refit, sizeof(double) * 4 * (size_t)head[2], "the refit batch", who)) return kLmError;
    c.ra = refit.as<double>();
    c.rx = c.ra + 3 * (size_t)head[2];

    // The survivors become the working batch (the statistics above have read the last one: it is overwritten in place), those of
    // the fits clipped in this round the refit batch as well: S fits again, every other one empty.
    long long *block_off = const_cast<long long *>(c.block_off);
    hipLaunchKernelGGL(clip_place_kernel<0>, dim3(nb), dim3(kCT), 0, stream, c);
    hipLaunchKernelGGL(clip_scan_kernel, dim3(1), dim3(kCT), 0, stream, c.block_count, (long long)nb, block_off);
    hipLaunchKernelGGL(clip_scan_kernel, dim3(1), dim3(kCT), 0, stream, c.block_count + nb, (long long)nb, block_off + nb + 1);
    hipLaunchKernelGGL(clip_scan_kernel, dim3(1), dim3(kCT), 0, stream, kept, (long long)S, const_cast<long long *>(c.noff));
    hipLaunchKernelGGL(clip_scan_kernel, dim3(1), dim3(kCT), 0, stream, c.rkept, (long long)S, const_cast<long long *>(c.roff));
    hipLaunchKernelGGL(clip_place_kernel<1>, dim3(nb), dim3(kCT), 0, stream, c);
    CAPTURE_OK(who, hipGetLastError());
    cur_off = c.noff;
    cur_angles = c.wa;
    cur_x = c.wx;

    // The refit: the refit batch from the fits' current p into temporaries -- the fits the round did not clip have no sample there and
    // are refused at once --, and the clipped ones are taken.
    double *tp = fa.at<double>(o_tp), *tinfo = fa.at<double>(o_tinfo);
    int *tret = fa.at<int>(o_tret);
    CAPTURE_OK(who, hipMemcpyAsync(tp, f.d_p, sizeof(double) * kM * S, hipMemcpyDeviceToDevice, stream));
    const PackedFitArgs rf = {f.method, f.model, c.ra, c.rx, c.roff, S, tp, f.lb, f.ub, f.itmax, f.opts, f.d_info ? tinfo : nullptr, tret,
                              f.workspace_bytes, stream};
    if (packed_fit_run(rf, who) != 0) return kLmError;
    hipLaunchKernelGGL(clip_take_kernel, dim3(blocks_of(S)), dim3(kCT), 0, stream, c.state, S, tp, tinfo, tret, f.d_p, f.d_info, ret);
    CAPTURE_OK(who, hipGetLastError());
    stats_fresh = false;
  }

  // ---- the statistics at the returned p over the returned sample sets ----
  if (want_stats && !stats_fresh) {
    const PackedStatsArgs ps = {f.method, f.model, cur_angles, cur_x, cur_off, S, f.d_p, f.opts, a.d_covar, a.d_stats, a.d_rank, f.workspace_bytes, stream};
    if (packed_stats_run(ps, who) != 0) return kLmError;
  }
  if (fa.buf.ptr || sa.buf.ptr) CAPTURE_OK(who, hipStreamSynchronize(stream));  // (the arenas are about to go away)
  return 0;
}

}  // namespace brdf
