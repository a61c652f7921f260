// packed_plan.h -- the arithmetic of a packed batch's plan (packed_fit.hip): the size class of a sample count and the number of fits a
// workspace holds.  Plain C++ (no HIP), so that tests/cpp/packed_plan_harness.cpp checks it on a CPU, as fit_switches.h is checked.
//
// The class bounds are the batched kernels' own: batch_fit.hip asserts that packed_class() changes exactly where geometry_for() and
// kLaneMaxN / kRowLanes change the kernel, fit_stats.hip that the statistics kernels' bounds are among them.
#pragma once

namespace brdf {

constexpr int kPackedClasses = 6;  // 0..4: one batched launch per class; 5: above every batched kernel, single fits
constexpr int kPackedLargeClass = kPackedClasses - 1;

// the largest count of class cls < kPackedLargeClass
constexpr int packed_bound(int cls) { return cls == 0 ? 16 : cls == 1 ? 64 : cls == 2 ? 256 : cls == 3 ? 1024 : 4096; }

// 0 for k <= 16, 1 for <= 64, 2 for <= 256, 3 for <= 1024, 4 for <= 4096, 5 above
constexpr int packed_class(long long k) {
  return k <= packed_bound(0) ? 0 : k <= packed_bound(1) ? 1 : k <= packed_bound(2) ? 2 : k <= packed_bound(3) ? 3 : k <= packed_bound(4) ? 4 : kPackedLargeClass;
}

// A class's rows are as long as its largest count, and at least 3: the statistics pass refuses a shorter stride, and a class 0 that
// holds refused fits only (counts 0..2) still needs rows.
constexpr int packed_stride(int largest_count) { return largest_count < 3 ? 3 : largest_count; }

// What one fit of a chunk occupies in the workspace: its padded rows angles[3][stride] and x[stride]; p[3], info[10] (the fit) or p[3],
// covar[9], stats[8] (the statistics) -- one figure for both calls, the larger --; and three ints (count, ret or rank, spare).
constexpr long long packed_fit_bytes(int stride) { return 8LL * (4LL * stride + 3 + 10 + 9 + 8) + 3 * 4; }

constexpr long long kPackedDefaultWorkspace = 1LL << 30;  // workspace_bytes == 0

// fits per chunk: max(1, workspace_bytes / bytes per padded fit); workspace_bytes <= 0 is the default, 1 GiB
constexpr long long packed_chunk_fits(long long workspace_bytes, int stride) {
  return (workspace_bytes <= 0 ? kPackedDefaultWorkspace : workspace_bytes) / packed_fit_bytes(stride) < 1
             ? 1
             : (workspace_bytes <= 0 ? kPackedDefaultWorkspace : workspace_bytes) / packed_fit_bytes(stride);
}

}  // namespace brdf
