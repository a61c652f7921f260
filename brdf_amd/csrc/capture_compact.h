// capture_compact.h -- the device text the capture units share (capture_fit.hip, capture_group.hip, capture_faces.hip,
// capture_means.hip, capture_single_faces.hip): the reference's x-major pixel index, the candidate (sorted pixel, light) of the
// per-face entries and its validity rule, a channel's stream compaction inside a workgroup, the scan of the blocks' counts between
// two candidate passes, and the fixed-order block sum of three columns.
//
// Shared text is the rule here: these kernels hold 14-48 VGPRs at occupancy 8.  Whoever changes this header compares the compiler's
// report of every capture unit with profiles/capture_layer_kernel_resources.txt: no scratch, no spill, no occupancy below the one there.
#pragma once

#include "device_common.h"

namespace brdf {

// ---- the candidates of the per-face entries ------------------------------------------------------------------------------------
// Candidate t = sorted pixel * L + light, of all three channels.  capture_candidates() fills this from the call and its CaptureGroup.
struct CandidateCtx {
  const unsigned char *images;
  int L, H, W;
  const long long *pixel_sorted;  // [S]: x-major pixel index, grouped by face
  const unsigned *face_sorted;    // [S]
  const int *rank_of_face;        // [nf]
  const long long *face_first;    // [F + 1]
  const double *angles_f;         // [F][3][L]
  long long T;                    // candidates of one channel: S * L
  int F;
  int v_min, v_max;
  double cos_min;
  int use1, use2;  // the planes the model reads besides the first (brdf_models.h: uses_c1, uses_c2)
};

struct Candidate {
  long long s = 0;  // sorted pixel
  int i = 0, r = 0;  // light, face rank
  int v[3] = {0, 0, 0};  // the pixel's B, G, R bytes: one read
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;  // the face's cosines at the light
  bool valid[3] = {false, false, false};  // the rule, per channel; t >= T: no channel
};

namespace {

constexpr int kCT = 256;
constexpr int kWaves = kCT / kWave;

// x-major index g = x * H + y  <->  pixel_map[y][x]                                   (brdfdata.cpp:1195-1197)
__device__ __forceinline__ int face_of(const int *pm, int H, int W, long long g) {
  const int x = (int)(g / H), y = (int)(g % H);
  return pm[(size_t)y * W + x];
}

__device__ __forceinline__ Candidate read_candidate(const CandidateCtx &c, long long t) {
  Candidate k;
  if (t >= c.T) return k;
  k.s = t / c.L;
  k.i = (int)(t - k.s * c.L);
  k.r = c.rank_of_face[c.face_sorted[k.s]];
  const long long g = c.pixel_sorted[k.s];
  const int px = (int)(g / c.H), py = (int)(g % c.H);
  const unsigned char *pxl = c.images + (((size_t)k.i * c.H + (size_t)(c.H - 1 - py)) * c.W + px) * 3;
  const double *a = c.angles_f + (size_t)k.r * 3 * c.L + k.i;
  k.c0 = a[0];
  k.c1 = a[c.L];
  k.c2 = a[2 * c.L];
  const bool cos_ok = k.c0 > c.cos_min && (!c.use1 || k.c1 > c.cos_min) && (!c.use2 || k.c2 > c.cos_min);  // (a NaN is not valid)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    k.v[ch] = pxl[ch];
    k.valid[ch] = cos_ok && k.v[ch] >= c.v_min && k.v[ch] <= c.v_max;
  }
  return k;
}

// A channel's stream compaction inside a workgroup of kCT, for all three channels: ballot + popcount.  Every thread calls place();
// then count(ch) is the workgroup's number of valid candidates and at(ch) the thread's place among them.
struct ChannelPlaces {
  int (*wave_cnt)[3];  // [kWaves][3], shared
  int before[3], wave;
  __device__ __forceinline__ void place(const bool valid[3]) {
    const int lane = threadIdx.x & (kWave - 1);
    wave = threadIdx.x / kWave;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const unsigned long long m = __ballot(valid[ch]);
      before[ch] = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wave_cnt[wave][ch] = __popcll(m);
    }
    __syncthreads();
  }
  __device__ __forceinline__ int count(int ch) const {
    int n = 0;
    for (int w = 0; w < kWaves; ++w) n += wave_cnt[w][ch];
    return n;
  }
  __device__ __forceinline__ long long at(int ch, long long block_off) const {
    long long a = block_off + before[ch];
    for (int w = 0; w < wave; ++w) a += wave_cnt[w][ch];
    return a;
  }
};

// The scan between two candidate passes, one workgroup: block_count[b][ch] -> block_off[b][ch], the place of the block's first valid
// candidate.  CHAIN: channel after channel, channel ch starts where the channels below it end; otherwise every channel from 0.
// totals[ch] and ends[ch * end_stride]: where channel ch ends.
template <bool CHAIN>
__global__ __launch_bounds__(kCT) void block_scan3_kernel(const int *__restrict__ block_count, long long nb, long long *__restrict__ block_off,
                                                          long long *__restrict__ ends, long long end_stride, long long *__restrict__ totals) {
  __shared__ long long part[kCT][3];
  const int t = threadIdx.x;
  const long long per = (nb + kCT - 1) / kCT;
  const long long b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
  long long sum[3] = {0, 0, 0};
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sum[ch] += block_count[b * 3 + ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) part[t][ch] = sum[ch];
  __syncthreads();
  if (t < (CHAIN ? 1 : 3)) {  // chained: one thread walks the three columns; otherwise one thread per column
    long long run = 0;
    for (int ch = t; ch < (CHAIN ? 3 : t + 1); ++ch) {
      for (int i = 0; i < kCT; ++i) {
        const long long v = part[i][ch];
        part[i][ch] = run;
        run += v;
      }
      ends[ch * end_stride] = run;
      totals[ch] = run;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) sum[ch] = part[t][ch];
  for (long long b = b0; b < b1; ++b) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      block_off[b * 3 + ch] = sum[ch];
      sum[ch] += block_count[b * 3 + ch];
    }
  }
}

// block_sums[block][k] = the workgroup's sum of v[k], k < 3, by a tree in a fixed order; every thread of the workgroup of kCT calls
__device__ __forceinline__ void block_sums3(const double v[3], double *block_sums) {
  __shared__ double red[3][kCT];
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = kCT / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) block_sums[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

}  // namespace

}  // namespace brdf
