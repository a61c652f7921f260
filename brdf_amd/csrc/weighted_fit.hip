// weighted_fit.hip -- batched fits with per-sample weights, n <= 16 samples per fit, dlevmar_bc_dif / dlevmar_bc_der.
//
// Fit s is levmar on hx_i = sw_i f_i(p) against x'_i = sw_i x_i, sw_i = sqrt(w_i), over the first counts[s] samples of its rows:
// the problem a levmar caller poses today by scaling inside the callback.  ONE LANE PER FIT, as lane_fit.hip: the kernels here are
// a second set that carries the body of lane_fit.hip's kernel with per-fit counts (a copy: sharing the text through an include moved
// the spill counts of eight unweighted instances) -- one more LDS plane per sample (sw; the x plane holds sw x, both stored at
// refill), one multiplication by sw per model value and per Jacobian entry, and nothing else: the state machine, the gating of heavy
// rounds, the queue and the sweeps in the reference's summation order (lmbc_core.c:595-615, misc_core.c:721-807) are lane_fit.hip's.
// With all weights 1.0 every added multiplication is exact, so the call returns the bytes of the unweighted ragged call.  NP + 1
// planes: Ward at n = 16 takes 40 KB per wave, four waves per CU.
//
// A weight of 0 is a sample that contributes nothing and still counts in n.  A negative or non-finite weight among a fit's counted
// samples refuses the fit at refill, as n < m is refused: ret -1, zero info, p untouched.  Fits with a cosine <= 0 take the exact
// twin behind the fast kernel (launch_fast_then_exact), as everywhere.
#include <algorithm>
#include <cstring>

#include "weighted_fit.h"
#include "fit_host.h"

namespace brdf {

// The body of lane_fit.hip's kernel with per-fit counts (see there for the rounds, the gating and the queue), with the weights.
// W = waves per SIMD the register allocator plans for (BRDF_HIP_LANE_WAVES); every lane carries the sample count of its own fit
// (ctx.counts, or the stride ctx.n where there are none); the sweeps run to that count in the reference's order for it.
template <int MODEL, bool FAST, int W>
__global__ __launch_bounds__(kWave, W) void lane_fit_weighted_kernel(WeightedBatchCtx ctx, int *queue) {
  using Mdl = BrdfModel<MODEL>;
  constexpr int NP = 3 + (Mdl::prep_planes == 2 ? 1 : 0);  // c0, q1, [q2], sw x
  constexpr int NPL = NP + 1;                              // + sw
  extern __shared__ double smp[];                          // [n][NPL][64]
  const int lane = threadIdx.x;
  const int n = ctx.n;
  int ncnt = n;  // samples of this lane's fit (set at refill)
  const int S = ctx.S;
  // (locals, not pointers into the by-value ctx: taking its members' addresses parks the whole struct in scratch)
  const double ov[5] = {ctx.opts[0], ctx.opts[1], ctx.opts[2], ctx.opts[3], ctx.opts[4]};
  const double lbv[kM] = {ctx.lb[0], ctx.lb[1], ctx.lb[2]}, ubv[kM] = {ctx.ub[0], ctx.ub[1], ctx.ub[2]};
  const double *opts = ctx.has_opts ? ov : nullptr;
  const double *lb = ctx.has_lb ? lbv : nullptr;
  const double *ub = ctx.has_ub ? ubv : nullptr;

  BcMachine<kM> m;
  // the half of the machine every fit of the batch shares is configured once, here, in wave-uniform control flow: options,
  // box and limits then live in scalar registers instead of 64 identical per-lane copies
  m.configure(n, lb, ub, nullptr, ctx.itmax, opts, 0, 1);
  m.c.analytic_jac = ctx.analytic;
  m.h.req.kind = RQ_DONE;
  int fit = -1;
  bool more = true;  // wave-uniform: the queue may still hold fits
  int since_heavy = 0;

  // Rounds.  In a round every lane with an evaluation request sweeps its samples and steps its machine.  The EXPENSIVE
  // things -- a Jacobian sweep with the 3x3 solve behind it, the line-search prologue (pow, square roots), the epilogue of
  // a fit, fetching and preparing the next fit -- are needed by a lane about once per LM iteration, i.e. in ~10 % of its
  // rounds, but with 64 lanes somebody needs each of them in EVERY round, and a wave pays for a phase body whenever one
  // lane runs it.  So they are gated (BcMachine::run<GATED>): lanes that reach one wait, and the wave runs a "heavy" round
  // for all of them together once a quorum waits (or nobody has anything else to do, or a lane has waited long enough).
  // Light rounds then cost an evaluation sweep plus the cheap phases only.  Scheduling cannot change a result.
  for (;;) {
    // a fit's results are written by the step that ends it and stored right behind that step (below): nothing of them
    // is carried from one round to the next, and saying so keeps 2 x 20 registers per lane free between the two
    for (int i = 0; i < kInfoSz; ++i) m.c.info[i] = 0.0;
    for (int i = 0; i < kM * kM; ++i) m.c.covar[i] = 0.0;
    m.c.ret = kLmError;
    const int kind0 = (fit >= 0) ? m.h.req.kind : (int)RQ_DONE;
    const bool wants_heavy = (fit < 0 && more) || kind0 == RQ_JAC || kind0 == RQ_YIELD;
    const bool light_work = fit >= 0 && kind0 != RQ_JAC && kind0 != RQ_YIELD;
    const int nh = __popcll(__ballot(wants_heavy));
    const int nl = __popcll(__ballot(light_work));
    if (nh == 0 && nl == 0) break;
    const bool heavy = nl == 0 || nh >= ctx.lane_quorum || since_heavy >= ctx.lane_maxwait;
    since_heavy = heavy ? 0 : since_heavy + 1;

    // ---- refill (heavy rounds): every idle lane takes the next fit of the queue ------------------------------
    bool want = heavy && fit < 0;
    while (more && __any(want)) {
      const unsigned long long mask = __ballot(want);
      const int cnt = __popcll(mask);
      const int first = __ffsll((long long)mask) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(queue, cnt);
      base = __shfl(base, first);
      if (base + cnt >= S) more = false;
      if (want) {
        const int f = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (f < S && (FAST || ctx.flags[f] == kNeedsExact)) {
          const double *a = ctx.angles + (size_t)f * 3 * n;
          const double *xs = ctx.x + (size_t)f * n;
          bool bad = false;
          bool bad_w = false;  // a counted weight that is negative or not finite
          ncnt = ctx.counts ? ragged_count(ctx.counts, f, n) : n;
          for (int i = 0; i < ncnt; ++i) {
            const double c0 = a[i];
            const double r1 = Mdl::uses_c1 ? a[n + i] : 0.0;
            const double r2 = Mdl::uses_c2 ? a[2 * n + i] : 0.0;
            const Prep q = Mdl::template prepare<FAST>(c0, r1, r2);
            if (FAST && !Mdl::domain_ok(c0, r1, r2)) bad = true;
            double *d = smp + (size_t)i * NPL * kWave + lane;
            d[0] = c0;
            d[kWave] = q.q1;
            if (NP == 4) d[2 * kWave] = q.q2;
            const double w = ctx.w[(size_t)f * n + i];
            const double sw = sqrt(w);
            if (!(w >= 0.0) || !lm_finite(w)) bad_w = true;
            d[(NP - 1) * kWave] = sw * xs[i];
            d[NP * kWave] = sw;
          }
          if (FAST) ctx.flags[f] = bad ? kNeedsExact : 0;
          if (!(FAST && bad)) {
            const double p0[kM] = {ctx.p[(size_t)f * kM], ctx.p[(size_t)f * kM + 1], ctx.p[(size_t)f * kM + 2]};
            m.begin(p0);
            if (ncnt < kM) m.h.req.kind = RQ_DONE;  // lmbc_core.c:440-443 for this lane's own count
            if (bad_w) m.h.req.kind = RQ_DONE;      // a weight sqrt() has no value for: refused the same way
            if (m.h.req.kind == RQ_DONE) {  // refused by start() (n < m, inconsistent box): lmbc_core.c:440-454
              if (ctx.ret) ctx.ret[f] = kLmError;
              if (ctx.info)
                for (int i = 0; i < kInfoSz; ++i) ctx.info[(size_t)f * kInfoSz + i] = 0.0;
            } else {
              fit = f;
              want = false;
            }
          }
        }
        if (f >= S) want = false;  // nothing left for this lane
      }
    }

    if (fit >= 0) {
      // ---- one pass over this lane's samples, sums in the reference's order -----------------------------------
      const Request<kM> &r = m.h.req;
      const int kind = r.kind;
      double s[kSlots];
#pragma unroll
      for (int k = 0; k < kSlots; ++k) s[k] = 0.0;
      double mx = 0.0;
      const double *sp = smp + lane;
      bool do_step = false;
      if (kind == RQ_JAC) {
        if (heavy) {  // lmbc_core.c:595-615: for l = n-1..0 { jtj[i][j] += row[j]*row[i]; jte[i] += row[i]*e[l] }
          PassUniforms<MODEL> u;
          u.build(r, true, ctx.analytic != 0);
          auto row = [&](int l, double &e, double *j) {
            const double *d = sp + (size_t)l * NPL * kWave;
            const Prep q{d[kWave], NP == 4 ? d[2 * kWave] : 0.0};
            double f0 = 0.0;
            if (ctx.analytic)  // dlevmar_bc_der: the model's analytic Jacobian (wave-uniform branch)
              model_an_row<MODEL, FAST>(u, d[0], q, f0, j);
            else
              model_fd_row<MODEL, FAST>(u, d[0], q, true, f0, 0.0, false, j);
            const double sw = d[NP * kWave];  // hx = sw f; the row of sw f is sw times the row of f
            f0 = sw * f0;
#pragma unroll
            for (int k = 0; k < kM; ++k) j[k] = sw * j[k];
            e = d[(NP - 1) * kWave] - f0;
          };
          // two rows per trip (one wave per SIMD: nothing else hides a row's dependent exp chains), accumulated in the
          // reference's order all the same
          int l = ncnt;
          for (; W == 1 && l >= 2; l -= 2) {
            double ea, eb, ja[kM], jb[kM];
            row(l - 1, ea, ja);
            row(l - 2, eb, jb);
            acc_normal_eq(ja, ea, s, s + kNL);
            acc_normal_eq(jb, eb, s, s + kNL);
          }
          for (; l >= 1; --l) {  // (two waves per SIMD hide each other's chains: one row per trip, fewer registers)
            double ea, ja[kM];
            row(l - 1, ea, ja);
            acc_normal_eq(ja, ea, s, s + kNL);
          }
          do_step = true;
        }
      } else if (kind == RQ_YIELD) {
        do_step = heavy;
      } else {
        PassUniforms<MODEL> u;  // an evaluation reads l0, n0 (and scal) only
        u.l0 = Mdl::lin(r.p);
        u.n0 = Mdl::nl(r.p);
        u.scal = r.scal;
        if (kind == RQ_SCALED) {  // lmbc_core.c:163-166, descending
          for (int l = ncnt; l-- > 0;) {
            const double *d = sp + (size_t)l * NPL * kWave;
            const Prep q{d[kWave], NP == 4 ? d[2 * kWave] : 0.0};
            const double f = d[NP * kWave] * model_value<MODEL, FAST>(u, d[0], q);  // sw f
            const double t = (d[(NP - 1) * kWave] - f) / u.scal;
            s[0] += t * t;
          }
        } else {  // RQ_EVAL: misc_core.c:721-807 -- blocks of 8 from the top down, accumulator (top - j) & 3; then the tail upwards
          double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
          const int body = (ncnt >> 3) << 3;
          for (int jb = body - 4; jb >= 0; jb -= 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const double *d = sp + (size_t)(jb + 3 - k) * NPL * kWave;
              const Prep q{d[kWave], NP == 4 ? d[2 * kWave] : 0.0};
              const double f = d[NP * kWave] * model_value<MODEL, FAST>(u, d[0], q);  // sw f
              const double e = d[(NP - 1) * kWave] - f;
              const double e2 = e * e;
              if (k == 0) a0 += e2;
              if (k == 1) a1 += e2;
              if (k == 2) a2 += e2;
              if (k == 3) a3 += e2;
              mx = fmax(mx, fabs(e));
            }
          }
          for (int t = body; t < ncnt; ++t) {
            const double *d = sp + (size_t)t * NPL * kWave;
            const Prep q{d[kWave], NP == 4 ? d[2 * kWave] : 0.0};
            const double f = d[NP * kWave] * model_value<MODEL, FAST>(u, d[0], q);  // sw f
            const double e = d[(NP - 1) * kWave] - f;
            const double e2 = e * e;
            const int k = (7 - (ncnt - t)) & 3;
            a0 += (k == 0) ? e2 : 0.0;
            a1 += (k == 1) ? e2 : 0.0;
            a2 += (k == 2) ? e2 : 0.0;
            a3 += (k == 3) ? e2 : 0.0;
            mx = fmax(mx, fabs(e));
          }
          s[0] = a0 + a1 + a2 + a3;
        }
        do_step = true;
      }
      if (do_step) {
        m.template step<false, false, true>(s, mx, heavy);
        if (m.h.req.kind == RQ_DONE) {
          double *po = ctx.p + (size_t)fit * kM;
          for (int i = 0; i < kM; ++i) po[i] = m.h.p[i];
          if (ctx.info)
            for (int i = 0; i < kInfoSz; ++i) ctx.info[(size_t)fit * kInfoSz + i] = m.c.info[i];
          if (ctx.ret) ctx.ret[fit] = m.c.ret;
          fit = -1;
        }
      }
    }
  }
}

namespace {
using WeightedFn = void (*)(WeightedBatchCtx, int *);
template <int W>
WeightedFn weighted_kernel_w(int model, bool fast) {
  static const WeightedFn table[2][MODEL_COUNT] = {
      {lane_fit_weighted_kernel<0, false, W>, lane_fit_weighted_kernel<1, false, W>, nullptr},  // Ward's prepared path has no domain restriction
      {lane_fit_weighted_kernel<0, true, W>, lane_fit_weighted_kernel<1, true, W>, lane_fit_weighted_kernel<2, true, W>},
  };
  return table[fast ? 1 : 0][model];
}
WeightedFn weighted_kernel(int model, bool fast, int w) {
  return w == 1 ? weighted_kernel_w<1>(model, fast) : (w == 4 ? weighted_kernel_w<4>(model, fast) : weighted_kernel_w<2>(model, fast));
}

// Per-thread scratch of a call, batch_fit.hip's scheme: flags[S] (kNeedsExact marks, read by the second launch) and the two
// work-queue words.  The next call of this thread, on whatever stream, waits on the event recorded behind this call's last launch.
struct WeightedScratch {
  DeviceBlock<int> block;  // flags[fits()], then the two queue words
  hipEvent_t last_use = nullptr;
  bool in_use = false;
  size_t fits() const { return block.cap - 2; }
  void release() {
    if (!block.ptr) return;
    DeviceScope on(block.device);
    block.release();
    if (last_use) (void)hipEventDestroy(last_use);
    last_use = nullptr;
    in_use = false;
  }
  ~WeightedScratch() { release(); }
};
thread_local WeightedScratch g_wscratch;

int weighted_launches(const WeightedFitArgs &wa, MethodSpec ms, int *flags, int *queue) {
  const BatchFitArgs &a = wa.fit;
  WeightedBatchCtx c;
  memset(&c, 0, sizeof c);
  c.analytic = ms.analytic ? 1 : 0;
  c.angles = a.d_angles;
  c.x = a.d_x;
  c.w = wa.d_w;
  c.counts = a.d_counts;
  c.p = a.d_p;
  c.info = a.d_info;
  c.ret = a.d_ret;
  c.flags = flags;
  c.S = a.S;
  c.n = a.n;
  c.itmax = a.itmax;
  c.has_opts = a.opts != nullptr;
  c.has_lb = a.lb != nullptr;
  c.has_ub = a.ub != nullptr;
  c.multi = 1;
  c.chain = 1;
  c.lane_quorum = (int)switch_number(kSwLaneQuorum);
  c.lane_maxwait = (int)switch_number(kSwLaneMaxwait);
  for (int i = 0; i < 5; ++i) c.opts[i] = a.opts ? a.opts[i] : 0.0;
  for (int i = 0; i < kM; ++i) {
    c.lb[i] = a.lb ? a.lb[i] : 0.0;
    c.ub[i] = a.ub ? a.ub[i] : 0.0;
  }
  HIP_OK(hipMemsetAsync(queue, 0, 2 * sizeof(int), a.stream));
  int dev = 0, cus = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int np = ((a.model == MODEL_WARD) ? 4 : 3) + 1;  // lane_fit.hip's planes and sw
  const size_t lds = sizeof(double) * (size_t)a.n * np * kWave;
  const int w = lane_waves_per_simd();
  long long per_cu = (160 * 1024) / (long long)std::max<size_t>(lds, 1);
  if (per_cu > 4 * w) per_cu = 4 * w;
  if (per_cu < 1) per_cu = 1;
  long long waves = (long long)cus * per_cu;
  const long long need = ((long long)a.S + kWave - 1) / kWave;
  if (waves > need) waves = need;
  note_batch_launch(kLaunchWeightedLane, w, waves, c.lane_quorum, c.lane_maxwait);
  const bool fast = brdf_fast_path_enabled() || a.model == MODEL_WARD;
  return launch_fast_then_exact(fast, a.model != MODEL_WARD, flags, (size_t)a.S, queue, a.stream, [&](bool fast_kernel, int *q) {
    hipLaunchKernelGGL(weighted_kernel(a.model, fast_kernel, w), dim3((unsigned)waves), dim3(kWave), lds, a.stream, c, q);
  });
}
}  // namespace

int weighted_fit_check(const WeightedFitArgs &a, const char *who) {
  if (batch_fit_check(a.fit, who) != 0) return kLmError;
  if (a.fit.method != BRDF_METHOD_BC_DIF && a.fit.method != BRDF_METHOD_BC_DER) {
    set_error("%s(): weights are limited to BRDF_METHOD_BC_DIF and BRDF_METHOD_BC_DER (got method %d)", who, a.fit.method);
    return kLmError;
  }
  if (a.fit.n > kLaneMaxN) {
    set_error("%s(): weights are limited to n <= %d samples per fit (got n = %d)", who, kLaneMaxN, a.fit.n);
    return kLmError;
  }
  if (!a.d_w) {
    set_error("%s(): null weights", who);
    return kLmError;
  }
  return 0;
}

int weighted_fit_enqueue(const WeightedFitArgs &a, const char *who) {
  if (weighted_fit_check(a, who) != 0) return kLmError;
  MethodSpec ms;
  (void)method_spec(a.fit.method, &ms);
  (void)hipGetLastError();
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  WeightedScratch &sc = g_wscratch;
  if (!sc.block.holds((size_t)a.fit.S + 2, dev)) {
    sc.release();  // (a previous call, on any stream, may still use the old block)
    HIP_OK(sc.block.ensure((size_t)a.fit.S + 2, dev));
    HIP_OK(hipEventCreateWithFlags(&sc.last_use, hipEventDisableTiming));
  }
  if (sc.in_use) HIP_OK(hipStreamWaitEvent(a.fit.stream, sc.last_use, 0));
  const int rc = weighted_launches(a, ms, sc.block.ptr, sc.block.ptr + sc.fits());
  sc.in_use = true;  // (also after a failed enqueue: some launches may be in flight)
  HIP_OK(hipEventRecord(sc.last_use, a.fit.stream));
  return rc;
}

}  // namespace brdf
