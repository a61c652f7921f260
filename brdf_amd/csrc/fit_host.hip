// fit_host.hip -- the host half that the single-fit regimes share (see fit_host.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "fit_host.h"

namespace brdf {

void set_bad_input_error(const char *who, int bad_input, int n, int m) {
  switch (bad_input) {
  case 1: set_error("%s(): cannot solve a problem with fewer measurements [%d] than unknowns [%d]", who, n, m); break;
  case 2: set_error("%s(): at least one lower bound exceeds the upper one", who); break;
  default: set_error("%s(): scaling constants should be positive", who); break;
  }
}

void warn_start_projected(int i, double from, double to) {
  fprintf(stderr, "Warning: component %d of starting point not feasible in dlevmar_bc_dif()! [%g projected to %g]\n", i, from, to);
}

int start_fit_machine(MachineUnion &m, int method, const double *p, int n, const double *lb, const double *ub, const double *dscl, int itmax,
                      const double *opts, bool want_covar, bool analytic, bool fast) {
  if (method == 0) {
    m.dif.start(p, n, itmax, opts, want_covar, /*speculative=*/1, dif_chain_candidates());
    if (m.dif.h.req.kind != RQ_DONE) return 0;
    set_bad_input_error("dlevmar_dif", 1, n, kM);
    return kLmError;
  }
  if (method == 2) {
    m.der.start(p, n, itmax, opts, want_covar);
    if (m.der.h.req.kind != RQ_DONE) return 0;
    set_bad_input_error("dlevmar_der", 1, n, kM);
    return kLmError;
  }
  BcMachine<kM> &bc = m.bc;
  bc.start(p, n, lb, ub, dscl, itmax, opts, want_covar, pg_candidates(), bc_spec_jac_enabled() ? 1 : 0);
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
  ExchangeKnobs k{max_replicas, default_spin_ticks, -1};
  if (const char *e = getenv("BRDF_HIP_RESIDENT_REPLICAS")) k.replicas = std::min(max_replicas, std::max(1, atoi(e)));
  if (const char *e = getenv("BRDF_HIP_RESIDENT_SPIN_MS")) k.spin_ticks = std::max(1LL, atoll(e)) * 100000LL;
  if (const char *e = getenv("BRDF_HIP_RESIDENT_SABOTAGE")) k.sabotage_epoch = atoi(e);  // tests only: forces the fallback
  return k;
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

// the blocks belong to `device`: drain and free them THERE, whatever device is current now
void ResidentWorkspace::release() {
  if (d_block || h_mbox) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (device >= 0 && cur != device) (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (d_block) (void)hipFree(d_block);
    if (h_mbox) (void)hipHostFree(h_mbox);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  }
  d_block = nullptr;
  h_mbox = d_mbox = nullptr;
  device = -1;
}

int ResidentWorkspace::allocate(size_t bytes, int mailboxes) {
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, device));
  cus = prop.multiProcessorCount;
  HIP_OK(hipMalloc(&d_block, bytes));
  HIP_OK(hipMemset(d_block, 0, bytes));
  HIP_OK(hipHostMalloc(&h_mbox, sizeof(Mailbox) * (size_t)mailboxes, hipHostMallocMapped | hipHostMallocCoherent));
  HIP_OK(hipHostGetDevicePointer((void **)&d_mbox, h_mbox, 0));
  block_bytes = bytes;
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
  HIP_OK(hipMemsetAsync(d_block, 0, block_bytes, stream));
  return 0;
}

void ResidentWorkspace::launch_unavailable() {
  backoff = std::min(1024, std::max(8, backoff * 2));
  skip = backoff;
  if (const char *e = getenv("BRDF_HIP_RESIDENT_BACKOFF")) skip = std::max(0, atoi(e));
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
