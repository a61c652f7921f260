// fit_host.h -- the host layer every regime shares (fit_host.hip): the C ABI's method codes, the environment switches
// (fit_switches.h), the library's error text, memory that belongs to a device, the fast-then-exact launch protocol, and the host
// half of the resident regimes (resident_fit.hip, channels_fit.hip).  Host code only.
#pragma once

#include "../../include/brdf_levmar.h"
#include "fit_switches.h"

namespace brdf {

// ---- method codes ---------------------------------------------------------------------------------------------------------
// Two numberings meet on the host.  The C ABI's BRDF_METHOD_{DIF, BC_DIF, BC_DER, DER} (0..3, include/brdf_levmar.h) names an
// entry point; the kernels are instantiated per state machine, and take where the Jacobian rows come from as a run-time flag.
enum Machine { kDifMachine = 0, kBcMachine = 1, kDerMachine = 2 };
struct MethodSpec {
  int machine;    // Machine: StreamFitArgs::method, the METHOD index of every kernel table
  bool analytic;  // dlevmar_bc_der / dlevmar_der: the model's analytic Jacobian instead of finite differences
};
// false for anything outside 0..3; *out is then {abi_method, false}, for the callers whose own check words the error
inline bool method_spec(int abi_method, MethodSpec *out) {
  switch (abi_method) {
  case BRDF_METHOD_DIF: *out = {kDifMachine, false}; return true;
  case BRDF_METHOD_BC_DIF: *out = {kBcMachine, false}; return true;
  case BRDF_METHOD_BC_DER: *out = {kBcMachine, true}; return true;
  case BRDF_METHOD_DER: *out = {kDerMachine, true}; return true;
  }
  *out = {abi_method, false};
  return false;
}

}  // namespace brdf

#ifdef __HIPCC__  // the rest needs the HIP runtime (tests/cpp/fit_switches_harness.cpp reads the part above with a host compiler)

#include <atomic>
#include <cstring>
#include <deque>
#include <tuple>
#include <vector>

#include "batch_fit.h"
#include "stream_fit.h"

namespace brdf {
// the calling thread's last error text (brdf_hip_last_error); set_error also prints it to stderr
void set_error(const char *fmt, ...);
const char *get_error();
}  // namespace brdf

#define HIP_OK(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return kLmError;                                                                \
    }                                                                                 \
  } while (0)

namespace brdf {

static_assert(kSwitchMaxCand == kMaxCand, "fit_switches.h clamps the candidate switches to lm_machine.h's kMaxCand");
inline bool brdf_fast_path_enabled() { return !switch_on(kSwExactPow); }

inline StreamFitArgs stream_fit_args(MethodSpec ms, int model, const double *d_angles, const double *d_x, int n, double *p, const double *lb,
                                     const double *ub, const double *dscl, int itmax, const double *opts, double *info, double *covar,
                                     hipStream_t stream) {
  StreamFitArgs a;
  a.method = ms.machine;
  a.model = model;
  a.analytic = ms.analytic ? 1 : 0;
  a.d_angles = d_angles;
  a.d_x = d_x;
  a.n = n;
  a.p = p;
  a.lb = lb;
  a.ub = ub;
  a.dscl = dscl;
  a.itmax = itmax;
  a.opts = opts;
  a.info = info;
  a.covar = covar;
  a.stream = stream;
  return a;
}

// ---- memory that belongs to a device --------------------------------------------------------------------------------------
// makes `dev` the current device for a scope (dev < 0: leaves it alone)
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  explicit DeviceScope(int dev) {
    if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope &) = delete;
  DeviceScope &operator=(const DeviceScope &) = delete;
};

// A grow-only block of `cap` T on device `device`.  It is given back on THAT device, whatever device is current then, after the
// work queued there has drained (a launch on any stream may still use it).
template <class T>
struct DeviceBlock {
  T *ptr = nullptr;
  size_t cap = 0;
  int device = -1;
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock &) = delete;
  DeviceBlock &operator=(const DeviceBlock &) = delete;
  ~DeviceBlock() { release(); }
  bool holds(size_t count, int dev) const { return ptr && device == dev && cap >= count; }
  // at least `count` elements on `dev`, which is the current device; what the block held before is lost when it has to move or grow
  hipError_t ensure(size_t count, int dev) {
    if (holds(count, dev)) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&ptr, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    cap = count;
    device = dev;
    return hipSuccess;
  }
  hipError_t ensure(size_t count) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    return e != hipSuccess ? e : ensure(count, dev);
  }
  void release() {
    if (!ptr) return;
    DeviceScope on(device);
    (void)hipDeviceSynchronize();
    (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    device = -1;
  }
  template <class U>
  U *as() const { return reinterpret_cast<U *>(ptr); }
};

// ---- a batched call through host pointers -----------------------------------------------------------------------------------
// Owns the call's device blocks.  in() uploads host[0, count), out() hands out device memory that finish() downloads into host,
// inout() both; a null host pointer gives null and no block.  The first HIP error is worded as the entry `who` where it happens and
// every later request gives null; finish() waits for the null stream once, then downloads in the order of the requests.
class HostCall {
 public:
  explicit HostCall(const char *who) : who_(who) {}
  template <class T>
  const T *in(const T *host, size_t count) { return add<T>(host, nullptr, count); }
  template <class T>
  T *out(T *host, size_t count) { return add<T>(nullptr, host, count); }
  template <class T>
  T *inout(T *host, size_t count) { return add<T>(host, host, count); }
  bool failed() const { return failed_; }
  int finish();  // 0, or kLmError and the error text

 private:
  template <class T>
  T *add(const T *up, T *down, size_t count) {
    if (failed_ || (!up && !down)) return nullptr;
    auto &blocks = std::get<std::deque<DeviceBlock<T>>>(blocks_);
    blocks.emplace_back();
    return static_cast<T *>(stage(blocks.back().ensure(count), blocks.back().ptr, up, down, count * sizeof(T)));
  }
  void *stage(hipError_t allocated, void *dev, const void *up, void *down, size_t bytes);
  struct Download {
    void *host;
    const void *dev;
    size_t bytes;
  };
  const char *who_;
  bool failed_ = false;
  std::vector<Download> downloads_;
  std::tuple<std::deque<DeviceBlock<double>>, std::deque<DeviceBlock<int>>, std::deque<DeviceBlock<long long>>, std::deque<DeviceBlock<unsigned char>>> blocks_;
};

// ---- what the batched entries refuse ------------------------------------------------------------------------------------------
// (no HIP call; `who`: the entry that was called, as the text shows it)
// an unknown model or method; otherwise *ms is the method's
bool known_model_method(int model, int method, MethodSpec *ms, const char *who);
// a lower bound above the upper one where the machine has a box: levmar's own refusal, lmbc_core.c:451-454
bool box_refused(MethodSpec ms, const double *lb, const double *ub, const char *who);

// a BigFit's (batch_fit.h) three plane prefixes [0, k) next to each other in `pack`, as a single fit reads them (k < stride: a ragged fit)
int pack_plane_prefixes(const BigFit &f, DeviceBlock<double> &pack, hipStream_t stream);

// ---- which kernel a batched call launched -------------------------------------------------------------------------------------
// The calling thread's last batched launch (brdf_hip_last_batch_launch): every enqueue below the batched entries notes the kernel it
// chose and the geometry and scheduler values it passed.  Host words only: what a test reads to know that a switch was obeyed.
enum BatchKernelCode {
  kLaunchLane = 0,       // lane_fit.hip: one lane per fit
  kLaunchRows = 1,       // four fits per wave
  kLaunchWave = 2,       // one wave per fit (n <= 256)
  kLaunchWorkgroup = 3,  // 256 threads per fit (n <= 1024)
  kLaunchEightWave = 4,  // resident_fit.hip's batched kernel (1024 < n <= 4096)
  kLaunchBig512 = 5,     // the symmetric 512 x 8 geometry
  kLaunchWeightedLane = 6,
};
struct BatchLaunchRecord {
  int kernel = -1;         // a BatchKernelCode; -1: this thread has launched none
  int waves_per_simd = 0;  // the chosen instance's launch bound (the lane kernels: BRDF_HIP_LANE_WAVES); 0: the kernel states none
  long long grid = 0;      // workgroups of the fast (or only) launch
  int quorum = 0, maxwait = 0;  // the lane kernels' scheduler values; 0 elsewhere
};
void note_batch_launch(int kernel, int waves_per_simd, long long grid, int quorum = 0, int maxwait = 0);
BatchLaunchRecord last_batch_launch();

// ---- fast, then exact -----------------------------------------------------------------------------------------------------
// Batched: launch(true, queue) enqueues the prepared-sample kernel, launch(false, queue + 1) its exact twin over the fits that
// marked themselves kNeedsExact (a cosine <= 0).  fast == false (BRDF_HIP_EXACT_POW=1): every fit is marked and only the exact
// kernel runs.  flags [S]; queue: the kernel's work-queue word, one per launch (null: the kernel has none); Ward has no twin.
template <class Launch>
int launch_fast_then_exact(bool fast, bool has_exact_twin, int *flags, size_t S, int *queue, hipStream_t stream, Launch launch) {
  if (!fast) HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flags), kNeedsExact, S, stream));
  launch(fast, queue);
  HIP_OK(hipGetLastError());
  if (fast && has_exact_twin) {
    launch(false, queue ? queue + 1 : nullptr);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// Single fit: attempt(fast, &retry_exact) runs one fit from p[0, count) and sets retry_exact when the fast path met a cosine <= 0
// and its result is to be discarded; the exact attempt then starts from the same p.  try_fast == false: the exact path only,
// where there is one.  (start_fit_machine keeps the starting point's warning from being printed by both attempts.)
constexpr int kRetryKeep = 9;  // three channels' parameters
template <class Attempt>
int with_exact_retry(double *p, int count, bool try_fast, bool has_exact, Attempt attempt) {
  bool retry = false;
  double keep[kRetryKeep];
  for (int i = 0; i < count; ++i) keep[i] = p[i];
  if (try_fast || !has_exact) {
    const int ret = attempt(true, &retry);
    if (!retry) return ret;
    for (int i = 0; i < count; ++i) p[i] = keep[i];
  }
  return has_exact ? attempt(false, &retry) : kLmError;
}

// ---- single fits ----------------------------------------------------------------------------------------------------------
// levmar's words for the arguments a machine refused (Cold::bad_input: 1 n < m, lm_core.c:502-505 / lmbc_core.c:440-443; 2 a lower
// bound above the upper one, lmbc_core.c:451-454; 3 a scaling constant <= 0, lmbc_core.c:456-461) and its warning about a
// starting point outside the box (lmbc_core.c:516-520).  `who`: the entry point's name as the text shows it
void set_bad_input_error(const char *who, int bad_input, int n, int m);
void warn_start_projected(int i, double from, double to);

// Starts the machine of `method` (a Machine) in `m`.  The launch chain passes the machine it uploads; the resident regimes a
// scratch one (their kernels start their own) for what this function does with it:
// refused arguments become the error text and kLmError, a projected starting point is warned about -- unless this is the exact
// re-run of a fit the fast path has already warned about (`fast`: the attempt is on the fast model path).  Otherwise 0.
int start_fit_machine(MachineUnion &m, int method, const double *p, int n, const double *lb, const double *ub, const double *dscl, int itmax,
                      const double *opts, bool want_covar, bool analytic, bool fast);

// the finishing pass's mailbox -> the caller's vectors (info, covar: may be null) and the fit's statistics (`launches` and
// `kernel_us` are the regime's own to fill)
void mailbox_to_caller(const Mailbox &mb, double *p, double *info, double *covar, FitStats *stats);

// ---- the resident regimes -------------------------------------------------------------------------------------------------
// the exchange's knobs: BRDF_HIP_RESIDENT_REPLICAS, _SPIN_MS (here in s_memrealtime ticks) and _SABOTAGE (fit_switches.h)
struct ExchangeKnobs {
  int replicas;
  long long spin_ticks;
  int sabotage_epoch;
};
ExchangeKnobs exchange_knobs(int max_replicas, long long default_spin_ticks);

// one workgroup of `threads` per CU must be able to live there at all (registers, LDS): asked once per kernel.  `cached`: that
// kernel's answer, 0 = not asked yet (atomic: host threads on several devices get here at once)
bool kernel_fits_a_cu(const void *kernel, int threads, std::atomic<int> &cached);

// brdf_hip_set_launch_timing(): an event pair per host thread, created on first use on the current device
struct LaunchTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int device = -1;  // the events belong to the device they were created on
  bool armed = false;
  void drop() {
    DeviceScope on(device);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
  }
  ~LaunchTimer() { drop(); }
  void before(hipStream_t s) {
    armed = false;
    if (!launch_timing_enabled()) return;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    if (dev != device) {
      drop();
      device = dev;
    }
    if (!e0 && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) {
      drop();
      return;
    }
    armed = hipEventRecord(e0, s) == hipSuccess;
  }
  void after(hipStream_t s) {
    if (armed) armed = hipEventRecord(e1, s) == hipSuccess;
  }
  double elapsed_us() {  // after the launch is known to have finished
    float ms = 0.0f;
    if (!armed || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.0;
    return 1e3 * (double)ms;
  }
};

// What a host thread keeps per device for its resident launches: the device block (control words, exchange tables; zeroed),
// the pinned mailboxes the kernels report to, the launch's event pair and the stepping aside after a launch that did not run.
struct ResidentWorkspace {
  int device = -1, cus = 0;  // device < 0: not ready
  DeviceBlock<char> block;
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
  void release();
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

// ---- host callbacks and small helpers (generic_fit.hip) -------------------------------------------------------------------
// method: a Machine; jacf null: finite differences
int generic_fit_run(int method, void (*func)(double *, double *, int, int, void *), void (*jacf)(double *, double *, int, int, void *),
                    double *p, double *x, int m, int n, double *lb, double *ub, double *dscl, int itmax, double *opts, double *info,
                    double *covar, void *adata);
int generic_fit_run_f(int method, void (*func)(float *, float *, int, int, void *), void (*jacf)(float *, float *, int, int, void *),
                      float *p, float *x, int m, int n, float *lb, float *ub, float *dscl, int itmax, float *opts, float *info,
                      float *covar, void *adata);
int chkjac_err_run(const double *fvec, const double *fjac, const double *fvecp, const double *p, int m, int n, double *err);
int chkjac_err_run_f(const float *fvec, const float *fjac, const float *fvecp, const float *p, int m, int n, float *err);
int r2_run(const double *x, const double *hx, int n, double *r2);
int r2_run_f(const float *x, const float *hx, int n, float *r2);

}  // namespace brdf

#endif  // __HIPCC__
