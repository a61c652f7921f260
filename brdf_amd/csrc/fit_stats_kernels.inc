// fit_stats_kernels.inc -- the text of the statistics pass's three per-fit kernels, included by fit_stats.hip twice:
//   FIT_STATS_KERNEL(kind)  the kernel's name: fit_stats_<kind>_kernel, or fit_stats_ragged_<kind>_kernel
//   FIT_STATS_RAGGED        false, or true: the fit's own sample count (StatsCtx::counts) instead of the stride c.n
// One text, two sets of kernels (and not one body called from two kernels, which moved a uniform kernel's register count): the
// uniform kernels are compiled from the tokens they were compiled from.

// ---- n <= 16: a 16-lane DPP row per fit (RAGGED: the count is per row) -------------------------------------------------------
template <int MODEL, int JAC, bool FAST>
__global__ __launch_bounds__(kRowsThreads) void FIT_STATS_KERNEL(rows)(StatsCtx c) {
  constexpr bool RAGGED = FIT_STATS_RAGGED;
  __shared__ double sh[kRowsFits][kRow];
  const int slot = threadIdx.x >> 4, i = threadIdx.x & 15, lane = threadIdx.x & (kWave - 1);
  const long long q = fit_of_row(c, (long long)blockIdx.x * kRowsFits + slot);
  const int nq = RAGGED ? (q >= 0 ? stats_count(c, q) : 0) : c.n;  // RAGGED: per 16-lane row
  const bool ok = q >= 0 && i < nq;
  double acc[kNS], xv = 0.0;
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = 0.0;
  if (ok) {
    JacUniforms u;
    build_uniforms<MODEL, JAC>(c.p + 3 * q, c.delta, u);
    xv = sample_acc<MODEL, JAC, FAST>(u, c.angles + (size_t)q * 3 * c.n, c.x + (size_t)q * c.n, c.n, i, acc);
  }
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = row_reduce_to_last<OpSum>(acc[k]);  // lanes beyond n add +0.0
  const double mean = __shfl(acc[kNS - 1], lane | 15) / (double)nq;         // misc_core.c:636
  const double dx = ok ? xv - mean : 0.0;
  const double st = row_reduce_to_last<OpSum>(dx * dx);
  if (i == 15) {
#pragma unroll
    for (int k = 0; k < kNS; ++k) sh[slot][k] = acc[k];
    sh[slot][kNS] = st;
  }
  __syncthreads();
  if (threadIdx.x < kRowsFits) {
    const long long r = (long long)blockIdx.x * kRowsFits + threadIdx.x;
    const long long qf = fit_of_row(c, r);
    if (qf >= 0) finish_fit<RAGGED>(c, r, qf, sh[threadIdx.x], RAGGED ? stats_count(c, qf) : c.n);
  }
}

// ---- n <= 256: a wavefront per fit (RAGGED: one scalar count per wavefront) --------------------------------------------------
template <int MODEL, int JAC, bool FAST>
__global__ __launch_bounds__(kWaveThreads) void FIT_STATS_KERNEL(wave)(StatsCtx c) {
  constexpr bool RAGGED = FIT_STATS_RAGGED;
  __shared__ double sh[kWaveFits][kRow];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const long long q = fit_of_row(c, (long long)blockIdx.x * kWaveFits + wave);  // wave-uniform
  const int nq = RAGGED ? (q >= 0 ? __builtin_amdgcn_readfirstlane(stats_count(c, q)) : 0) : c.n;  // ... and so is the fit's count
  double acc[kNS], xs[kWavePer];
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = 0.0;
  if (q >= 0) {
    JacUniforms u;
    build_uniforms<MODEL, JAC>(c.p + 3 * q, c.delta, u);
    u = scalar_copy(u);
    const double *a = c.angles + (size_t)q * 3 * c.n, *x = c.x + (size_t)q * c.n;
#pragma unroll
    for (int k = 0; k < kWavePer; ++k) {
      const int i = lane + k * kWave;
      xs[k] = 0.0;
      if (i < nq) xs[k] = sample_acc<MODEL, JAC, FAST>(u, a, x, c.n, i, acc);
    }
  }
#pragma unroll
  for (int k = 0; k < kNS; ++k) acc[k] = wave_reduce_to_last<OpSum>(acc[k]);
  const double mean = wave_last(acc[kNS - 1]) / (double)nq;
  double st = 0.0;
  if (q >= 0) {
#pragma unroll
    for (int k = 0; k < kWavePer; ++k)
      if (lane + k * kWave < nq) {
        const double dx = xs[k] - mean;
        st += dx * dx;
      }
  }
  st = wave_reduce_to_last<OpSum>(st);
  if (lane == kWave - 1) {
#pragma unroll
    for (int k = 0; k < kNS; ++k) sh[wave][k] = acc[k];
    sh[wave][kNS] = st;
  }
  __syncthreads();
  if (threadIdx.x < kWaveFits) {
    const long long r = (long long)blockIdx.x * kWaveFits + threadIdx.x;
    const long long qf = fit_of_row(c, r);
    if (qf >= 0) finish_fit<RAGGED>(c, r, qf, sh[threadIdx.x], RAGGED ? stats_count(c, qf) : c.n);
  }
}

// ---- n <= 4096: a workgroup per fit (RAGGED: one scalar count per workgroup) -------------------------------------------------
template <int MODEL, int JAC, bool FAST>
__global__ __launch_bounds__(kBlockThreads) void FIT_STATS_KERNEL(block)(StatsCtx c) {
  constexpr bool RAGGED = FIT_STATS_RAGGED;
  __shared__ double buf[reduce_buf_doubles<kBlockThreads>()];
  __shared__ double out[kSlots];
  const long long r = blockIdx.x, q = fit_of_row(c, r);  // workgroup-uniform
  if (q < 0) return;
  const int nq = RAGGED ? __builtin_amdgcn_readfirstlane(stats_count(c, q)) : c.n;
  block_sums<MODEL, JAC, FAST>(c, q, 0, nq, buf, out);
  double row[kRow];
#pragma unroll
  for (int k = 0; k < kNS; ++k) row[k] = out[k];
  block_spread(c, q, 0, nq, row[kNS - 1] / (double)nq, buf, out);  // (x is read again: the fit's 8 n bytes are in L2)
  row[kNS] = out[0];
  if (threadIdx.x == 0) finish_fit<RAGGED>(c, r, q, row, nq);
}
