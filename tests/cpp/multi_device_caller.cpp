// tests/cpp/multi_device_caller.cpp -- a C++ host program that reaches several GPUs through the C ABI alone.
//
// Written the way a relinked application would: host arrays, include/brdf_levmar.h, -lbrdf_hip,
// no HIP header.  It fits one batch with brdf_hip_fit_batch on the current device and the same batch with
// brdf_hip_fit_batch_multi on the device list {0, 0} (two shards, one worker thread), compares p, info, ret and the return
// values byte for byte, prints the per-shard statistics and returns from main(): a clean process exit after the call is
// part of what the test checks.
//
// usage: multi_device_caller [S n method model]   (defaults: 1001 fits of 16 samples, dlevmar_bc_dif, Blinn-Phong)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "brdf_levmar.h"

namespace {

// deterministic U[0,1) (splitmix64): the inputs only have to be the same for both calls
double uniform(uint64_t &state) {
  uint64_t z = (state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace

int main(int argc, char **argv) {
  const int S = argc > 1 ? atoi(argv[1]) : 1001;
  const int n = argc > 2 ? atoi(argv[2]) : 16;
  const int method = argc > 3 ? atoi(argv[3]) : BRDF_METHOD_BC_DIF;
  const int model = argc > 4 ? atoi(argv[4]) : BRDF_MODEL_BLINN_PHONG;
  if (S < 1 || n < 1) return 2;

  // surfel s: planes [3][n] of cosines in [0.05, 1), measurements of a Blinn-Phong lobe with per-surfel kd, ks, exponent
  std::vector<double> angles(3 * (size_t)S * n), x((size_t)S * n), p0(3 * (size_t)S);
  uint64_t state = 20240611;
  for (int s = 0; s < S; ++s) {
    const double kd = 0.1 + 0.8 * uniform(state), ks = 0.1 + 0.8 * uniform(state), e = 2.0 + 60.0 * uniform(state);
    double *a = angles.data() + 3 * (size_t)s * n;
    for (int i = 0; i < 3 * n; ++i) a[i] = 0.05 + 0.95 * uniform(state);
    for (int i = 0; i < n; ++i) x[(size_t)s * n + i] = kd * a[i] + ks * pow(a[n + i], e) + 0.01 * (uniform(state) - 0.5);
    p0[3 * s] = 0.5;
    p0[3 * s + 1] = 1.0;
    p0[3 * s + 2] = 1.0;
  }
  const double lb[3] = {0.0, 0.0, model == BRDF_MODEL_WARD ? 0.01 : 0.0}, ub[3] = {100.0, 100.0, 100.0};
  const double opts[5] = {LM_INIT_MU, 1e-15, 1e-15, 1e-20, LM_DIFF_DELTA};

  std::vector<double> p1(p0), info1(10 * (size_t)S), p2(p0), info2(10 * (size_t)S, -1.0);
  std::vector<int> ret1(S), ret2(S, 12345);
  const int rc1 = brdf_hip_fit_batch(method, model, angles.data(), x.data(), S, n, p1.data(), lb, ub, 100, opts, info1.data(),
                                     ret1.data());
  if (rc1 == LM_ERROR) {
    fprintf(stderr, "brdf_hip_fit_batch: %s\n", brdf_hip_last_error());
    return 3;
  }
  const int devices[2] = {0, 0};
  const int rc2 = brdf_hip_fit_batch_multi(method, model, angles.data(), x.data(), S, n, p2.data(), lb, ub, 100, opts,
                                           info2.data(), ret2.data(), devices, 2);
  if (rc2 == LM_ERROR) {
    fprintf(stderr, "brdf_hip_fit_batch_multi: %s\n", brdf_hip_last_error());
    return 4;
  }
  for (int k = 0;; ++k) {
    int dev = -1;
    long long first = 0, count = 0;
    double ms[3];
    if (brdf_hip_last_multi_stats(k, &dev, &first, &count, ms) != 0) break;
    printf("shard %d: device %d, fits [%lld, %lld), upload %.3f ms, fit %.3f ms, download %.3f ms\n", k, dev, first, first + count,
           ms[0], ms[1], ms[2]);
  }
  const bool same = rc1 == rc2 && memcmp(p1.data(), p2.data(), sizeof(double) * p1.size()) == 0 &&
                    memcmp(info1.data(), info2.data(), sizeof(double) * info1.size()) == 0 &&
                    memcmp(ret1.data(), ret2.data(), sizeof(int) * ret1.size()) == 0;
  printf("S=%d n=%d method=%d model=%d: brdf_hip_fit_batch returned %d, brdf_hip_fit_batch_multi {0,0} returned %d, results %s\n", S, n,
         method, model, rc1, rc2, same ? "bit-identical" : "DIFFER");
  return same ? 0 : 1;
}
