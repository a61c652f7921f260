// capture_compact.h -- what the capture entries share of the walk over the pixel map (capture_fit.hip, capture_faces.hip): the
// reference's x-major pixel index and pass 1 of the deterministic two-pass compaction of the pixels that carry a face.
#pragma once

#include "device_common.h"

namespace brdf {

namespace {

constexpr int kCT = 256;

// x-major index g = x * H + y  <->  pixel_map[y][x]                                   (brdfdata.cpp:1195-1197)
__device__ __forceinline__ int face_of(const int *pm, int H, int W, long long g) {
  const int x = (int)(g / H), y = (int)(g % H);
  return pm[(size_t)y * W + x];
}

__global__ __launch_bounds__(kCT) void count_kernel(const int *pm, int H, int W, int nf, int *block_count) {
  __shared__ int wave_cnt[kCT / 64];
  const long long g = (long long)blockIdx.x * kCT + threadIdx.x;
  const int f = (g < (long long)H * W) ? face_of(pm, H, W, g) : -1;
  const bool valid = f > -1 && f < nf;
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

}  // namespace

}  // namespace brdf
