// channels_fit.hip -- K fits over one set of planes (brdf_hip_fit_channels_dev): dispatcher of channels_fit_impl.h's kernels,
// with the channels run one after the other through the single-fit regimes where the shared launch does not apply.
#include <algorithm>
#include <atomic>

#include "channels_fit_impl.h"
#include "fit_host.h"

namespace brdf {

ChannelsKernels channels_kernels_0(), channels_kernels_1(), channels_kernels_2();

namespace {

ChannelsKernels (*const kKernels[MODEL_COUNT])() = {channels_kernels_0, channels_kernels_1, channels_kernels_2};
std::atomic<int> g_fits_a_cu[MODEL_COUNT][2];  // kernel_fits_a_cu()'s answers

struct ChannelsArgs {
  int model;
  bool analytic;  // dlevmar_bc_der: the model's analytic Jacobian (the machine is always kBcMachine here)
  const double *d_angles;
  const double *d_x[kMaxChannels];
  int n, K;
  double *p;  // [K][3] in/out
  const double *lb, *ub, *dscl;
  int itmax;
  const double *opts;
  double *info, *covar;  // [K][10], [K][9] or null
  hipStream_t stream;
};

struct CWorkspace : ResidentWorkspace {
  // the device block: ctl | per channel: rows | group rows
  static constexpr size_t off_rows = sizeof(ResidentCtl);
  static constexpr size_t chan_bytes = sizeof(u64) * (kRowsGranules + kGroupsGranules);
  unsigned tag_base[kMaxChannels] = {0, 0, 0};
  unsigned launches = 0;
  FitStats stats[kMaxChannels] = {};
  void restart_tags() {
    for (int c = 0; c < kMaxChannels; ++c) tag_base[c] = 0;
    launches = 0;
  }
  int ensure(int dev) {
    if (ready(dev)) return 0;
    restart_tags();
    return ResidentWorkspace::ensure(dev, off_rows + kMaxChannels * chan_bytes, kMaxChannels);
  }
};
thread_local CWorkspace g_cws;

int channels_attempt(const ChannelsKernels &kn, bool fast, const ChannelsArgs &a, CWorkspace &ws, bool *retry_exact, bool *unavailable) {
  *retry_exact = *unavailable = false;
  const int G = (int)std::min<long long>(ws.cus, std::max<long long>(1, ((long long)a.n + 1023) / 1024));  // (the single fit's grid)
  for (int c = 0; c < a.K; ++c) {  // the entry point's argument checks and warnings, per channel (the kernel starts its own machines)
    MachineUnion scratch;
    if (start_fit_machine(scratch, kBcMachine, a.p + c * kM, a.n, a.lb, a.ub, a.dscl, a.itmax, a.opts, a.covar != nullptr, a.analytic, fast) != 0)
      return kLmError;
  }
  ws.clear_mailboxes();
  unsigned top = 0;
  for (int c = 0; c < kMaxChannels; ++c) top = std::max(top, ws.tag_base[c]);
  if (top > 0xF0000000u || ws.launches > 0xF0000000u) {  // tag / launch-id space nearly used up: start over from zeroed tables
    if (ws.zero_tables(a.stream) != 0) return kLmError;
    ws.restart_tags();
  }
  ChannelsCtx c;
  c.c0 = a.d_angles;
  c.c1 = a.d_angles + a.n;
  c.c2 = a.d_angles + 2 * (size_t)a.n;
  for (int k = 0; k < kMaxChannels; ++k) c.x[k] = a.d_x[k < a.K ? k : 0];
  c.ctl = reinterpret_cast<ResidentCtl *>(ws.block.ptr);
  c.rows = reinterpret_cast<u64 *>(ws.block.ptr + CWorkspace::off_rows);
  c.groups = c.rows + kMaxChannels * kRowsGranules;
  c.launch_id = ++ws.launches;  // nonzero, different for every launch on this workspace
  for (int k = 0; k < kMaxChannels; ++k)
    for (int i = 0; i < kM; ++i) c.p0[k][i] = a.p[(k < a.K ? k : 0) * kM + i];
  for (int i = 0; i < kM; ++i) {
    c.lb[i] = a.lb ? a.lb[i] : 0.0;
    c.ub[i] = a.ub ? a.ub[i] : 0.0;
    c.dscl[i] = a.dscl ? a.dscl[i] : 1.0;
  }
  for (int i = 0; i < 5; ++i) c.opts[i] = a.opts ? a.opts[i] : 0.0;
  c.itmax = a.itmax;
  c.has_opts = a.opts != nullptr;
  c.has_lb = a.lb != nullptr;
  c.has_ub = a.ub != nullptr;
  c.has_dscl = a.dscl != nullptr;
  c.want_covar = a.covar != nullptr;
  c.multi = (int)switch_number(kSwPgMulti);
  c.analytic = a.analytic ? 1 : 0;
  c.spec_jac = switch_on(kSwSpecJac) ? 1 : 0;
  c.mbox = ws.d_mbox;
  c.n = a.n;
  c.K = a.K;
  for (int k = 0; k < kMaxChannels; ++k) c.tag_base[k] = ws.tag_base[k];
  const ExchangeKnobs knobs = exchange_knobs(kReplicas, kSpinBudgetTicks);
  c.spin_ticks = knobs.spin_ticks;
  c.replicas = knobs.replicas;
  c.sabotage_epoch = knobs.sabotage_epoch;

  const ChannelsKernelFn kernel = kn.kernel[fast ? kFastPath : kExactPath];
  if (!kernel_fits_a_cu((const void *)kernel, kRThreads, g_fits_a_cu[a.model][fast ? kFastPath : kExactPath])) {
    *unavailable = true;
    return 0;
  }
  ws.timer.before(a.stream);
  hipLaunchKernelGGL(kernel, dim3(G), dim3(kRThreads), 0, a.stream, c);
  HIP_OK(hipGetLastError());
  ws.timer.after(a.stream);
  bool done = false;
  if (ws.wait_for_mailboxes(a.K, a.stream, &done) != 0) return kLmError;
  if (!done) {  // aborted.  Tags of unknown epochs were stored: start over
    (void)ws.zero_tables(a.stream);
    ws.restart_tags();
    *unavailable = true;
    return 0;
  }
#ifdef BRDF_STAMPS
  HIP_OK(hipStreamSynchronize(a.stream));  // (the sweeping waves write their stamps when they leave, after the last channel's result)
#endif
  int worst = 0;
  bool bad_domain = false;
  for (int k = 0; k < a.K; ++k) {
    const Mailbox &mb = ws.h_mbox[k];
    ws.tag_base[k] += (unsigned)mb.passes + 2u;
    bad_domain = bad_domain || (fast && mb.domain_bad);
  }
  if (bad_domain) {
    *retry_exact = true;
    return 0;
  }
  const double kernel_us = ws.timer.elapsed_us();  // (the shared launch's)
  for (int k = 0; k < a.K; ++k) {
    const Mailbox &mb = ws.h_mbox[k];
    mailbox_to_caller(mb, a.p + k * kM, a.info ? a.info + k * kInfoSz : nullptr, a.covar ? a.covar + k * kM * kM : nullptr, &ws.stats[k]);
    ws.stats[k].launches = 1;
    ws.stats[k].kernel_us = kernel_us;
    if (mb.ret < 0) worst = kLmError;
  }
  return worst;
}

// the fast model path first; the exact one where that is switched off, or met a cosine <= 0 (Ward has no exact path)
int channels_run(const ChannelsKernels &kn, const ChannelsArgs &a, CWorkspace &ws, bool *unavailable) {
  static_assert(kMaxChannels * kM <= kRetryKeep, "with_exact_retry keeps every channel's starting point");
  return with_exact_retry(a.p, a.K * kM, brdf_fast_path_enabled(), kn.kernel[kExactPath] != nullptr,
                          [&](bool fast, bool *retry) { return channels_attempt(kn, fast, a, ws, retry, unavailable); });
}

}  // namespace

thread_local int g_channels_shared = 0;  // 1: the last call ran as ONE shared launch

int channels_last_shared() { return g_channels_shared; }
FitStats channels_last_stats(int c) { return (c >= 0 && c < kMaxChannels) ? g_cws.stats[c] : FitStats{}; }

int channels_fit_run(int method, int model, const double *d_angles, const double *d_x, long long x_stride, int n, int K, double *p,
                     const double *lb, const double *ub, const double *dscl, int itmax, const double *opts, double *info, double *covar,
                     hipStream_t stream) {
  g_channels_shared = 0;
  MethodSpec ms;
  (void)method_spec(method, &ms);  // (the entry point has refused anything else)
  int dev = 0;
  // the shared launch: box-constrained entry points, up to three channels, a fit that fits the chip
  if (switch_on(kSwChannels) && switch_on(kSwResident) && ms.machine == kBcMachine && K >= 2 && K <= kMaxChannels && hipGetDevice(&dev) == hipSuccess &&
      g_cws.ensure(dev) == 0 && (long long)n <= (long long)g_cws.cus * kRTile && g_cws.cus <= kRowStride) {
    CWorkspace &ws = g_cws;
    if (!ws.step_aside()) {  // (stepping aside after an aborted launch)
      ChannelsArgs a;
      a.analytic = ms.analytic;
      a.model = model;
      a.d_angles = d_angles;
      for (int c = 0; c < kMaxChannels; ++c) a.d_x[c] = d_x + (size_t)(c < K ? c : 0) * x_stride;
      a.n = n;
      a.K = K;
      a.p = p;
      a.lb = lb;
      a.ub = ub;
      a.dscl = dscl;
      a.itmax = itmax;
      a.opts = opts;
      a.info = info;
      a.covar = covar;
      a.stream = stream;
      bool unavailable = false;
      const int r = channels_run(kKernels[model](), a, ws, &unavailable);
      if (!unavailable) {
        ws.launch_succeeded();
        g_channels_shared = 1;
        return r;
      }
      ws.launch_unavailable();
    }
  }
  int worst = 0;
  for (int c = 0; c < K; ++c) {  // one fit after the other: the single-fit regimes (resident launch or launch chain)
    const StreamFitArgs a = stream_fit_args(ms, model, d_angles, d_x + (size_t)c * x_stride, n, p + c * kM, lb, ub, dscl, itmax, opts,
                                            info ? info + c * kInfoSz : nullptr, covar ? covar + c * kM * kM : nullptr, stream);
    const int r = stream_fit_run(a);
    if (c < kMaxChannels) g_cws.stats[c] = stream_fit_last_stats();
    if (r < 0) worst = kLmError;
  }
  return worst;
}

}  // namespace brdf
