// fit_host.hip -- the host layer every regime shares (see fit_host.h).
#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "fit_host.h"

namespace brdf {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  fprintf(stderr, "libbrdf_hip: %s\n", g_err);
}
const char *get_error() { return g_err; }

void set_bad_input_error(const char *who, int bad_input, int n, int m) {
  switch (bad_input) {
  case 1: set_error("%s(): cannot solve a problem with fewer measurements [%d] than unknowns [%d]", who, n, m); break;
  case 2: set_error("%s(): at least one lower bound exceeds the upper one", who); break;
  default: set_error("%s(): scaling constants should be positive", who); break;
  }
}

void *HostCall::stage(hipError_t e, void *dev, const void *up, void *down, size_t bytes) {
  if (e != hipSuccess) {
    set_error("%s(): hipMalloc(%zu bytes) failed: %s", who_, bytes, hipGetErrorString(e));
  } else if (up && bytes && (e = hipMemcpy(dev, up, bytes, hipMemcpyHostToDevice)) != hipSuccess) {
    set_error("%s(): host->device copy failed: %s", who_, hipGetErrorString(e));
  }
  failed_ = e != hipSuccess;
  if (failed_) return nullptr;
  if (down) downloads_.push_back({down, dev, bytes});
  return dev;
}

int HostCall::finish() {
  hipError_t e = hipStreamSynchronize(nullptr);
  for (const Download &d : downloads_)
    if (e == hipSuccess) e = hipMemcpy(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) return 0;
  set_error("%s(): %s", who_, hipGetErrorString(e));
  return kLmError;
}

bool known_model_method(int model, int method, MethodSpec *ms, const char *who) {
  if (model >= 0 && model < MODEL_COUNT && method_spec(method, ms)) return true;
  set_error("%s(): unknown model %d / method %d", who, model, method);
  return false;
}

bool box_refused(MethodSpec ms, const double *lb, const double *ub, const char *who) {
  if (ms.machine != kBcMachine || !lb || !ub) return false;
  for (int i = 0; i < kM; ++i)
    if (lb[i] > ub[i]) {
      set_bad_input_error(who, 2, 0, kM);
      return true;
    }
  return false;
}

static thread_local BatchLaunchRecord g_batch_launch;
void note_batch_launch(int kernel, int waves_per_simd, long long grid, int quorum, int maxwait) {
  g_batch_launch.kernel = kernel;
  g_batch_launch.waves_per_simd = waves_per_simd;
  g_batch_launch.grid = grid;
  g_batch_launch.quorum = quorum;
  g_batch_launch.maxwait = maxwait;
}
BatchLaunchRecord last_batch_launch() { return g_batch_launch; }

int pack_plane_prefixes(const BigFit &f, DeviceBlock<double> &pack, hipStream_t stream) {
  HIP_OK(pack.ensure(3 * (size_t)f.stride));
  for (int pl = 0; pl < 3; ++pl)
    HIP_OK(hipMemcpyAsync(pack.ptr + (size_t)pl * f.k, f.d_angles + (size_t)pl * f.stride, sizeof(double) * f.k, hipMemcpyDeviceToDevice, stream));
  return 0;
}

void warn_start_projected(int i, double from, double to) {
  fprintf(stderr, "Warning: component %d of starting point not feasible in dlevmar_bc_dif()! [%g projected to %g]\n", i, from, to);
}

int start_fit_machine(MachineUnion &m, int method, const double *p, int n, const double *lb, const double *ub, const double *dscl, int itmax,
                      const double *opts, bool want_covar, bool analytic, bool fast) {
  if (method == kDifMachine) {
    m.dif.start(p, n, itmax, opts, want_covar, /*speculative=*/1, (int)switch_number(kSwDifChain));
    if (m.dif.h.req.kind != RQ_DONE) return 0;
    set_bad_input_error("dlevmar_dif", 1, n, kM);
    return kLmError;
  }
  if (method == kDerMachine) {
    m.der.start(p, n, itmax, opts, want_covar);
    if (m.der.h.req.kind != RQ_DONE) return 0;
    set_bad_input_error("dlevmar_der", 1, n, kM);
    return kLmError;
  }
  BcMachine<kM> &bc = m.bc;
  bc.start(p, n, lb, ub, dscl, itmax, opts, want_covar, (int)switch_number(kSwPgMulti), switch_on(kSwSpecJac) ? 1 : 0);
  bc.c.analytic_jac = analytic ? 1 : 0;
  if (bc.h.req.kind == RQ_DONE) {
    set_bad_input_error("dlevmar_bc_dif", bc.c.bad_input, n, kM);
    return kLmError;
  }
  if (fast || !brdf_fast_path_enabled())  // (an exact re-run must not print the warning twice)
    for (int i = 0; i < kM; ++i)
      if (bc.c.infeasible_mask & (1 << i)) warn_start_projected(i, bc.c.p_start[i], bc.h.p[i]);
  return 0;
}

void mailbox_to_caller(const Mailbox &mb, double *p, double *info, double *covar, FitStats *stats) {
  for (int i = 0; i < kM; ++i) p[i] = mb.p[i];
  if (info)
    for (int i = 0; i < kInfoSz; ++i) info[i] = mb.info[i];
  if (covar)
    for (int i = 0; i < kM * kM; ++i) covar[i] = mb.covar[i];
  stats->passes = mb.passes;
  stats->jac_passes = mb.n_jac;
  stats->eval_passes = mb.n_eval;
  stats->device_us = (double)(mb.t_last - mb.t_first) / 100.0;  // first pass start -> result (s_memrealtime, 100 MHz)
  for (int k = 0; k < 8; ++k) stats->stamps[k] = mb.stamps[k];
}

ExchangeKnobs exchange_knobs(int max_replicas, long long default_spin_ticks) {
  return {(int)switch_number(kSwResidentReplicas, max_replicas, 1, max_replicas), resident_spin_ticks(default_spin_ticks),
          (int)switch_number(kSwResidentSabotage)};
}

bool kernel_fits_a_cu(const void *kernel, int threads, std::atomic<int> &cached) {
  int v = cached.load(std::memory_order_relaxed);  // workgroups per CU + 1
  if (v == 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess) per_cu = 0;
    v = per_cu + 1;
    cached.store(v, std::memory_order_relaxed);
  }
  return v > 1;
}

// the blocks belong to `device`: they are given back THERE, whatever device is current now
void ResidentWorkspace::release() {
  block.release();
  if (h_mbox) {
    DeviceScope on(device);
    (void)hipHostFree(h_mbox);
  }
  h_mbox = d_mbox = nullptr;
  device = -1;
}

int ResidentWorkspace::allocate(size_t bytes, int mailboxes) {
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, device));
  cus = prop.multiProcessorCount;
  HIP_OK(block.ensure(bytes, device));
  HIP_OK(hipMemset(block.ptr, 0, bytes));
  HIP_OK(hipHostMalloc(&h_mbox, sizeof(Mailbox) * (size_t)mailboxes, hipHostMallocMapped | hipHostMallocCoherent));
  HIP_OK(hipHostGetDevicePointer((void **)&d_mbox, h_mbox, 0));
  n_mbox = mailboxes;
  return 0;
}

int ResidentWorkspace::ensure(int dev, size_t bytes, int mailboxes) {
  if (ready(dev)) return 0;
  release();
  device = dev;
  const int r = allocate(bytes, mailboxes);
  if (r != 0) release();  // not ready after any failure: what was allocated is given back, device = -1
  return r;
}

int ResidentWorkspace::zero_tables(hipStream_t stream) {
  HIP_OK(hipMemsetAsync(block.ptr, 0, block.cap, stream));
  return 0;
}

void ResidentWorkspace::launch_unavailable() {
  backoff = std::min(1024, std::max(8, backoff * 2));
  skip = backoff;
  if (const long long fits = switch_number(kSwResidentBackoff); fits >= 0) skip = (int)fits;
}

int ResidentWorkspace::wait_for_mailboxes(int K, hipStream_t stream, bool *done) {
  auto all_done = [&] {
    for (int k = 0; k < K; ++k)
      if (!*(volatile int *)&h_mbox[k].done) return false;
    return true;
  };
  for (unsigned spins = 0; !all_done(); ++spins)
    if ((spins & 0x3FFu) == 0x3FFu && hipStreamQuery(stream) != hipErrorNotReady) break;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (!all_done()) {
    HIP_OK(hipStreamSynchronize(stream));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
  }
  *done = all_done();
  return 0;
}

}  // namespace brdf
