// resident_fit.hip -- the resident regime's host side: picks the (MODEL, METHOD) instance of resident_fit_impl.h's kernels and
// launches it.  The kernels themselves (and the file comment that explains the regime) live in resident_fit_impl.h; each
// (MODEL, METHOD) pair is its own translation unit (resident_inst.hip, compiled with -DRI_PAIR=<model><method>), because hipcc
// needs 40-60 s per pair and the nine of them used to be one 6.5-minute compile.  An instance exports its kernels' addresses.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>

#include "resident_fit_impl.h"  // (first: the diagnostic builds define LM_STAMP in front of lm_machine.h)
#include "fit_host.h"

namespace brdf {

#ifndef BRDF_DEV_WARD_ONLY
ResidentKernels resident_kernels_00(), resident_kernels_01(), resident_kernels_02();
ResidentKernels resident_kernels_10(), resident_kernels_11(), resident_kernels_12();
#endif
ResidentKernels resident_kernels_20(), resident_kernels_21(), resident_kernels_22();

namespace {

// [model][method]; null: not in this build (BRDF_DEV_WARD_ONLY, the diagnostic builds' Ward instances only)
ResidentKernels (*const kKernels[MODEL_COUNT][3])() = {
#ifndef BRDF_DEV_WARD_ONLY
    {resident_kernels_00, resident_kernels_01, resident_kernels_02},
    {resident_kernels_10, resident_kernels_11, resident_kernels_12},
#else
    {nullptr, nullptr, nullptr},
    {nullptr, nullptr, nullptr},
#endif
    {resident_kernels_20, resident_kernels_21, resident_kernels_22},
};
std::atomic<int> g_fits_a_cu[MODEL_COUNT][3][2];  // kernel_fits_a_cu()'s answers for the single-fit kernels

struct RWorkspace : ResidentWorkspace {
  // the device block: ctl | machine | rows + group rows | trace rows (diagnostic builds)
  static constexpr size_t kMachineBytes = 4096;
  static constexpr size_t off_rows = sizeof(ResidentCtl) + kMachineBytes;
  static constexpr size_t rows_bytes = sizeof(u64) * (kRowsGranules + kGroupsGranules);
  static constexpr size_t trace_bytes = sizeof(long long) * 8 * kRowStride;
  long long h_trace[8 * (kRowStride + 1)] = {0};  // + one row: the sections of the LM step (LM_STAMP)
  unsigned tag_base = 0;
  FitStats stats{};
  int ensure(int dev) {
    if (ready(dev)) return 0;
    tag_base = 0;
    return ResidentWorkspace::ensure(dev, off_rows + rows_bytes + trace_bytes, 1);
  }
};
thread_local RWorkspace g_rws;

int resident_attempt(const ResidentKernels &k, bool fast, const StreamFitArgs &a, RWorkspace &ws, bool *retry_exact, bool *unavailable) {
  *retry_exact = *unavailable = false;
  const int G = (int)std::min<long long>(ws.cus, std::max<long long>(1, ((long long)a.n + 1023) / 1024));
  MachineUnion scratch;  // started here for the entry point's argument checks and warnings only: the kernel starts its own
  if (start_fit_machine(scratch, a.method, a.p, a.n, a.lb, a.ub, a.dscl, a.itmax, a.opts, a.covar != nullptr, a.analytic != 0, fast) != 0)
    return kLmError;
  ws.clear_mailboxes();
  if (ws.tag_base > 0xF0000000u) {  // tag space nearly used up: start over from zeroed rows (and control words)
    if (ws.zero_tables(a.stream) != 0) return kLmError;
    ws.tag_base = 0;
  }

  ResidentCtx c;
  c.c0 = a.d_angles;
  c.c1 = a.d_angles + a.n;
  c.c2 = a.d_angles + 2 * (size_t)a.n;
  c.x = a.d_x;
  c.ctl = reinterpret_cast<ResidentCtl *>(ws.block.ptr);
  c.rows = reinterpret_cast<u64 *>(ws.block.ptr + RWorkspace::off_rows);
  c.groups = c.rows + kRowsGranules;
  c.launch_id = ws.tag_base + 1u;  // (tag_base grows by passes + 2 with every launch)
  for (int i = 0; i < kM; ++i) {
    c.p0[i] = a.p[i];
    c.lb[i] = a.lb ? a.lb[i] : 0.0;
    c.ub[i] = a.ub ? a.ub[i] : 0.0;
    c.dscl[i] = a.dscl ? a.dscl[i] : 1.0;
  }
  for (int i = 0; i < 5; ++i) c.opts[i] = a.opts ? a.opts[i] : 0.0;
  c.itmax = a.itmax;
  c.has_opts = a.opts != nullptr;
  c.has_lb = a.method == kBcMachine && a.lb != nullptr;
  c.has_ub = a.method == kBcMachine && a.ub != nullptr;
  c.has_dscl = a.method == kBcMachine && a.dscl != nullptr;
  c.want_covar = a.covar != nullptr;
  c.multi = (int)switch_number(kSwPgMulti);
  c.chain = (int)switch_number(kSwDifChain);
  c.spec_jac = switch_on(kSwSpecJac) ? 1 : 0;
  c.dif_fused = switch_on(kSwDifFused) ? 1 : 0;
  c.analytic = a.analytic ? 1 : 0;
  c.mbox = ws.d_mbox;
  c.n = a.n;
  c.tag_base = ws.tag_base;
  const ExchangeKnobs knobs = exchange_knobs(kReplicas, kSpinBudgetTicks);
  c.spin_ticks = knobs.spin_ticks;
  c.sabotage_epoch = knobs.sabotage_epoch;
  c.replicas = knobs.replicas;
  c.trace = nullptr;
  c.trace_epoch = -1;
#ifdef BRDF_STAMPS
  c.trace = reinterpret_cast<long long *>(ws.block.ptr + RWorkspace::off_rows + RWorkspace::rows_bytes);
  c.trace_epoch = (int)switch_number(kSwResidentTraceEpoch);
#endif

  const ResidentKernelFn kernel = k.single[fast ? kFastPath : kExactPath];
  if (!kernel_fits_a_cu((const void *)kernel, kRThreads, g_fits_a_cu[a.model][a.method][fast ? kFastPath : kExactPath])) {
    *unavailable = true;
    return 0;
  }
  ws.timer.before(a.stream);
  hipLaunchKernelGGL(kernel, dim3(G), dim3(kRThreads), 0, a.stream, c, BatchCtx{});
  HIP_OK(hipGetLastError());
  ws.timer.after(a.stream);
  bool done = false;
  if (ws.wait_for_mailboxes(1, a.stream, &done) != 0) return kLmError;
  if (!done) {  // aborted.  Tags of unknown epochs were stored: start over
    (void)ws.zero_tables(a.stream);
    ws.tag_base = 0;
    *unavailable = true;
    return 0;
  }
  const Mailbox &mb = *ws.h_mbox;
  ws.tag_base += (unsigned)mb.passes + 2u;
#ifdef BRDF_STAMPS
  (void)hipMemcpy(ws.h_trace, c.trace, RWorkspace::trace_bytes, hipMemcpyDeviceToHost);
  k.take_lm_stamps(ws.h_trace + 8 * kRowStride);
#endif
  if (fast && mb.domain_bad) {
    *retry_exact = true;
    return 0;
  }
  mailbox_to_caller(mb, a.p, a.info, a.covar, &ws.stats);
  ws.stats.launches = 1;
  ws.stats.kernel_us = ws.timer.elapsed_us();
  return mb.ret;
}

// the fast model path first; the exact one where that is switched off, or met a cosine <= 0 (Ward has no exact path)
int resident_run(const ResidentKernels &k, const StreamFitArgs &a, RWorkspace &ws, bool *unavailable) {
  return with_exact_retry(a.p, kM, brdf_fast_path_enabled(), k.single[kExactPath] != nullptr,
                          [&](bool fast, bool *retry) { return resident_attempt(k, fast, a, ws, retry, unavailable); });
}

}  // namespace

FitStats resident_fit_last_stats() { return g_rws.stats; }
int resident_fit_last_trace(long long *out, int max_rows) {
  const int rows = std::min(max_rows, kRowStride + 1);
  memcpy(out, g_rws.h_trace, sizeof(long long) * 8 * (size_t)rows);
  return rows;
}

int resident_batch_enqueue(int model, int method, bool fast, const BatchCtx &c, const int *counts, hipStream_t stream) {
  if (!kKernels[model][method]) {
    set_error("resident kernels of model %d / method %d are not in this build", model, method);
    return kLmError;
  }
  const ResidentKernels k = kKernels[model][method]();
  note_batch_launch(kLaunchEightWave, 0, c.S);
  return launch_fast_then_exact(fast, k.batched[kExactPath] != nullptr, c.flags, (size_t)c.S, nullptr, stream, [&](bool fast_kernel, int *) {
    if (counts)  // per-fit sample counts: the RAGGED instances
      hipLaunchKernelGGL(k.ragged[fast_kernel ? kFastPath : kExactPath], dim3(c.S), dim3(kRThreads), 0, stream, ResidentCtx{}, ragged_ctx(c, counts));
    else
      hipLaunchKernelGGL(k.batched[fast_kernel ? kFastPath : kExactPath], dim3(c.S), dim3(kRThreads), 0, stream, ResidentCtx{}, c);
  });
}

// returns true if the resident path handled the fit (*ret is then the solver's return value)
bool resident_fit_try(const StreamFitArgs &a, int *ret) {
  if (!switch_on(kSwResident)) return false;  // (the default for every single fit that fits the chip)
  int dev = 0;
  if (!kKernels[a.model][a.method] || hipGetDevice(&dev) != hipSuccess) return false;
  RWorkspace &ws = g_rws;
  if (ws.ensure(dev) != 0) return false;
  if ((long long)a.n > (long long)ws.cus * kRTile || ws.cus > kRowStride) return false;  // does not fit the chip: launch chain
  if (ws.step_aside()) return false;  // after an aborted launch
  bool unavailable = false;
  const int r = resident_run(kKernels[a.model][a.method](), a, ws, &unavailable);
  if (unavailable) {
    static std::atomic<bool> warned{false};  // once per process, also when host threads on several devices get here at once
    if (!warned.exchange(true))
      fprintf(stderr, "libbrdf_hip: resident single-launch path unavailable (grid not co-resident?); using the launch chain\n");
    ws.launch_unavailable();
    return false;
  }
  ws.launch_succeeded();
  *ret = r;
  return true;
}

}  // namespace brdf
