// fit_host.h -- the host half that the single-fit regimes share: the launch chain (stream_fit.hip), the resident launch
// (resident_fit.hip) and channels sharing a launch (channels_fit.hip).  Host code only (fit_host.hip).
#pragma once

#include <atomic>
#include <cstring>

#include "stream_fit.h"

#define HIP_OK(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return kLmError;                                                                \
    }                                                                                 \
  } while (0)

namespace brdf {

// levmar's words for the arguments a machine refused (Cold::bad_input: 1 n < m, lm_core.c:502-505 / lmbc_core.c:440-443; 2 a lower
// bound above the upper one, lmbc_core.c:451-454; 3 a scaling constant <= 0, lmbc_core.c:456-461) and its warning about a
// starting point outside the box (lmbc_core.c:516-520).  `who`: the entry point's name as the text shows it
void set_bad_input_error(const char *who, int bad_input, int n, int m);
void warn_start_projected(int i, double from, double to);

// Starts the machine of `method` (0 dlevmar_dif, 1 dlevmar_bc_dif / bc_der, 2 dlevmar_der) in `m`.  The launch chain passes the
// machine it uploads; the resident regimes a scratch one (their kernels start their own) for what this function does with it:
// refused arguments become the error text and kLmError, a projected starting point is warned about -- unless this is the exact
// re-run of a fit the fast path has already warned about (`fast`: the attempt is on the fast model path).  Otherwise 0.
int start_fit_machine(MachineUnion &m, int method, const double *p, int n, const double *lb, const double *ub, const double *dscl, int itmax,
                      const double *opts, bool want_covar, bool analytic, bool fast);

// the finishing pass's mailbox -> the caller's vectors (info, covar: may be null) and the fit's statistics (`launches` and
// `kernel_us` are the regime's own to fill)
void mailbox_to_caller(const Mailbox &mb, double *p, double *info, double *covar, FitStats *stats);

// ---- the resident regimes -------------------------------------------------------------------------------------------------
// the exchange's knobs: BRDF_HIP_RESIDENT_REPLICAS (1..max_replicas copies of the group rows), _SPIN_MS (budget of one wait, in
// s_memrealtime ticks) and _SABOTAGE (tests only: the epoch at which the last workgroup withholds its row; -1 = never)
struct ExchangeKnobs {
  int replicas;
  long long spin_ticks;
  int sabotage_epoch;
};
ExchangeKnobs exchange_knobs(int max_replicas, long long default_spin_ticks);

// one workgroup of `threads` per CU must be able to live there at all (registers, LDS): asked once per kernel.  `cached`: that
// kernel's answer, 0 = not asked yet (atomic: host threads on several devices get here at once)
bool kernel_fits_a_cu(const void *kernel, int threads, std::atomic<int> &cached);

// What a host thread keeps per device for its resident launches: the device block (control words, exchange tables; zeroed),
// the pinned mailboxes the kernels report to, the launch's event pair and the stepping aside after a launch that did not run.
struct ResidentWorkspace {
  int device = -1, cus = 0;  // device < 0: not ready
  char *d_block = nullptr;
  size_t block_bytes = 0;
  Mailbox *h_mbox = nullptr, *d_mbox = nullptr;  // [n_mbox]
  int n_mbox = 0;
  LaunchTimer timer;
  // After a launch that could not run co-resident (GPU shared with other kernels / ranks: every workgroup burns its
  // spin budget before the launch drains) the resident path steps aside for the next `skip` fits, doubling up to
  // 1024 while it keeps failing, instead of paying that budget on every fit.
  int backoff = 0, skip = 0;

  ~ResidentWorkspace() { release(); }
  bool ready(int dev) const { return device == dev; }
  int ensure(int dev, size_t bytes, int mailboxes);  // not ready after any failure
  int allocate(size_t bytes, int mailboxes);         // (ensure()'s: the blocks, on `device`)
  void release();                                    // on the workspace's device, whatever device is current
  int zero_tables(hipStream_t stream);               // start over from zeroed control words and tables: the caller restarts its tags
  bool step_aside() {
    if (skip <= 0) return false;
    --skip;
    return true;
  }
  void launch_unavailable();  // (BRDF_HIP_RESIDENT_BACKOFF=<fits>: tests)
  void launch_succeeded() { backoff = 0; }
  void clear_mailboxes() { memset(h_mbox, 0, sizeof(Mailbox) * (size_t)n_mbox); }
  // Waits for the first K mailboxes after the launch on `stream` by polling them (a stream synchronise sleeps and wakes up tens
  // of microseconds late); the launch always terminates (bounded spins), which hipStreamQuery reports even if `done` never
  // comes: *done = false then (aborted: not co-resident / spin budget exhausted).
  int wait_for_mailboxes(int K, hipStream_t stream, bool *done);
};

}  // namespace brdf
