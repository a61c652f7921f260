// packed_plan_harness.cpp -- the plan arithmetic of a packed batch (brdf_amd/csrc/packed_plan.h) on a CPU: a stand-alone program,
// compiled by tests/test_packed_host.py with a host compiler and -fsanitize=address,undefined.  The expected classes are written out
// here independently of the header's bounds.  Exit status 0 and a last line "ok" when every check holds.
#include <climits>
#include <cstdio>

#include "../../brdf_amd/csrc/packed_plan.h"

using namespace brdf;

static int failures = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                               \
    }                                                           \
  } while (0)

static int want_class(long long k) {
  if (k <= 16) return 0;
  if (k <= 64) return 1;
  if (k <= 256) return 2;
  if (k <= 1024) return 3;
  if (k <= 4096) return 4;
  return 5;
}

int main() {
  for (long long k = 0; k <= 17; ++k) {
    std::printf("class(%lld) = %d\n", k, packed_class(k));
    CHECK(packed_class(k) == (k <= 16 ? 0 : 1));
  }
  const long long seams[] = {63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, INT_MAX};
  const int want[] = {1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5};
  for (unsigned i = 0; i < sizeof seams / sizeof seams[0]; ++i) {
    std::printf("class(%lld) = %d\n", seams[i], packed_class(seams[i]));
    CHECK(packed_class(seams[i]) == want[i]);
    CHECK(packed_class(seams[i]) == want_class(seams[i]));
  }
  CHECK(kPackedClasses == 6 && kPackedLargeClass == 5);
  for (int c = 0; c < kPackedLargeClass; ++c) CHECK(packed_class(packed_bound(c)) == c && packed_class(packed_bound(c) + 1LL) == c + 1);

  // a class's rows: its largest count, at least 3
  CHECK(packed_stride(0) == 3 && packed_stride(2) == 3 && packed_stride(3) == 3 && packed_stride(7) == 7 && packed_stride(4096) == 4096);

  // fits per chunk: max(1, workspace_bytes / bytes per padded fit), for every class's widest row and a narrow one
  const int strides[] = {3, 7, 16, 64, 256, 1024, 4096};
  for (int stride : strides) {
    const long long one = packed_fit_bytes(stride);
    std::printf("stride %d: %lld bytes per padded fit, %lld fits per default chunk\n", stride, one, packed_chunk_fits(0, stride));
    CHECK(one == 8LL * (4LL * stride + 30) + 12);  // angles[3][stride], x[stride]; p[3], info[10], covar[9], stats[8]; three ints
    CHECK(packed_chunk_fits(1, stride) == 1);            // less than one fit's bytes: still one fit
    CHECK(packed_chunk_fits(one - 1, stride) == 1);
    CHECK(packed_chunk_fits(one, stride) == 1);          // one fit's bytes exactly
    CHECK(packed_chunk_fits(2 * one - 1, stride) == 1);  // one byte less than two fits'
    CHECK(packed_chunk_fits(2 * one, stride) == 2);
    CHECK(packed_chunk_fits(0, stride) == (1LL << 30) / one);  // 0: the default, 1 GiB
    CHECK(packed_chunk_fits(LLONG_MAX, stride) == LLONG_MAX / one);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
