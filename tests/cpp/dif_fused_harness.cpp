// tests/cpp/dif_fused_harness.cpp -- TEST HARNESS (not product code).
//
// DifMachine::fused_trial_step (brdf_amd/csrc/lm_machine.h) promises to leave, whenever it takes a step, the bits the
// generic run() would have left in EVERY field of the machine.  This harness drives TWO DifMachine<3> through whole
// fits side by side with the reference-order pass executor of host_machine.cpp: one stepped by run() alone, one that
// tries the fused step first.  The executor runs once per pass (the two requests are compared first) and both machines
// consume the same sums.  After every step CoreInts, CoreReals, Cool and Request must be memcmp-equal; at the end p,
// info, covar and ret.  Built by tests/test_dif_fused_step.py (g++ -O2 -ffp-contract=off, against oracle/liboracle.so).
#include <cstring>

#include "host_machine.cpp"  // HostPasses: the pass executor (its extern "C" entry points come along unused)

namespace {

using Dif = DifMachine<3>;

// 0 if the two machines' hot state is identical, else which part differs (1 ints, 2 reals, 3 cool, 4 request)
int hot_differs(const Dif &a, const Dif &b) {
  if (memcmp(static_cast<const Dif::CoreInts *>(&a.h), static_cast<const Dif::CoreInts *>(&b.h), sizeof(Dif::CoreInts))) return 1;
  if (memcmp(static_cast<const Dif::CoreReals *>(&a.h), static_cast<const Dif::CoreReals *>(&b.h), sizeof(Dif::CoreReals))) return 2;
  if (memcmp(&a.h.cool, &b.h.cool, sizeof(Dif::Cool))) return 3;
  if (memcmp(&a.h.req, &b.h.req, sizeof(Request<3>))) return 4;
  return 0;
}

template <int MODEL>
int fit_pair(double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi, int want_covar,
             long long *counts, double *p_out, double *info_out) {
  HostPasses<MODEL, false> hp(angles, x, n, 0);
  static Dif a, b;  // (zeroed, padding included, so that memcmp sees only what the machines wrote)
  memset(&a, 0, sizeof a);
  memset(&b, 0, sizeof b);
  a.start(p0, n, itmax, opts, want_covar, /*speculative=*/1, multi);
  b.start(p0, n, itmax, opts, want_covar, /*speculative=*/1, multi);
  double s[SumLayout<3>::MAX] = {0};
  double mx = 0.0;
  long long steps = 0, fused = 0, trial_steps = 0;
  int bad = hot_differs(a, b);
  while (!bad && a.h.req.kind != RQ_DONE) {
    const bool trial = a.h.req.kind == RQ_DIF_TRIAL;
    hp.run(a.h.req, s, mx);
    a.template step<false, true>(s, mx);
    if (Dif::template fused_trial_step<false, true>(b.c, b.h, b.h, b.h.cool, b.h.req, s))
      ++fused;
    else
      b.template step<false, true>(s, mx);
    ++steps;
    trial_steps += trial;
    bad = hot_differs(a, b);
    if (bad) bad += 10 * (int)(steps < 100000 ? steps : 99999);  // <step> * 10 + part
  }
  counts[0] = steps;
  counts[1] = fused;
  counts[2] = trial_steps;
  if (bad) return bad;
  if (memcmp(a.h.p, b.h.p, sizeof a.h.p)) return -1;
  if (memcmp(a.c.info, b.c.info, sizeof a.c.info)) return -2;
  if (memcmp(a.c.covar, b.c.covar, sizeof a.c.covar)) return -3;
  if (a.c.ret != b.c.ret) return -4;
  for (int i = 0; i < 3; ++i) p_out[i] = b.h.p[i];
  for (int i = 0; i < kInfoSz; ++i) info_out[i] = b.c.info[i];
  return 0;
}

}  // namespace

// counts[3]: steps, steps the fused path took, steps behind a trial pass.  Returns 0 when the two machines agreed after every step
// and at the end; <step> * 10 + part (1 ints, 2 reals, 3 cool, 4 request) at the first step they did not; -1 p, -2 info, -3 covar, -4 ret.
extern "C" int dfh_fit_pair(int model, double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi,
                            int want_covar, long long *counts, double *p_out, double *info_out) {
  switch (model) {
  case 0: return fit_pair<0>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  case 1: return fit_pair<1>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  case 2: return fit_pair<2>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  }
  return -100;
}
