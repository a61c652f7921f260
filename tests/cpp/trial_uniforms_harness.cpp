// tests/cpp/trial_uniforms_harness.cpp -- TEST HARNESS (not product code).
//
// PassUniforms::build_trial (brdf_amd/csrc/brdf_models.h) forms the uniforms of the trial request DifMachine::fused_trial_step
// issues from what the step hands out (DifMachine::NextTrial: q, Dp, ||Dp||^2 -- its locals) instead of reading the request back.
// It promises the bytes build(req, need_base = false) leaves, in EVERY field.  This harness drives a DifMachine<3> through whole
// fits with the reference-order pass executor of host_machine.cpp, fused step first as the resident kernel does, and keeps two
// PassUniforms side by side the way the kernel keeps its one: never cleared between passes.  After every step one is built by
// build() from the request, the other by build_trial() where the fused path took the step (by build() otherwise); the two must
// be memcmp-equal after every step, and what the step handed out must be the request's q, dp and dp_l2 bit for bit.
#include <cstring>

#include "host_machine.cpp"  // HostPasses: the pass executor (its extern "C" entry points come along unused)

namespace {

using Dif = DifMachine<3>;

template <int MODEL>
int fit_uniforms(double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi, long long *counts) {
  HostPasses<MODEL, false> hp(angles, x, n, 0);
  static Dif m;
  static PassUniforms<MODEL> ua, ub;  // (zeroed, padding included, so that memcmp sees only what the builders wrote)
  memset(&m, 0, sizeof m);
  memset(&ua, 0, sizeof ua);
  memset(&ub, 0, sizeof ub);
  m.start(p0, n, itmax, opts, /*want_covar=*/0, /*speculative=*/1, multi);
  ua.build(m.h.req, true, false);
  ub.build(m.h.req, true, false);
  double s[SumLayout<3>::MAX] = {0};
  double mx = 0.0;
  long long steps = 0, fused = 0;
  while (m.h.req.kind != RQ_DONE) {
    hp.run(m.h.req, s, mx);
    Dif::NextTrial nx;
    memset(&nx, 0, sizeof nx);
    const bool took = Dif::template fused_trial_step<false, true>(m.c, m.h, m.h, m.h.cool, m.h.req, s, &nx);
    if (!took) m.template step<false, true>(s, mx);
    ++steps;
    if (m.h.req.kind == RQ_DONE) break;
    ua.build(m.h.req, /*need_base=*/false, false);
    if (took) {
      ++fused;
      if (m.h.req.kind != RQ_DIF_TRIAL) return (int)(steps < 100000 ? steps : 99999) * 10 + 1;
      if (memcmp(nx.q, m.h.req.q, sizeof nx.q) || memcmp(nx.dp, m.h.req.dp, sizeof nx.dp) || memcmp(&nx.dp_l2, &m.h.req.dp_l2, sizeof nx.dp_l2))
        return (int)(steps < 100000 ? steps : 99999) * 10 + 2;
      ub.build_trial(nx.q, nx.dp, nx.dp_l2, false);
    } else {
      ub.build(m.h.req, /*need_base=*/false, false);
    }
    if (memcmp(&ua, &ub, sizeof ua)) return (int)(steps < 100000 ? steps : 99999) * 10 + 3;
  }
  counts[0] = steps;
  counts[1] = fused;
  return 0;
}

}  // namespace

// counts[2]: steps, steps the fused path took.  Returns 0 when the two sets of uniforms agreed after every step; else <step> * 10 +
// what differed: 1 the fused step left another kind of request, 2 what it handed out is not the request's, 3 the uniforms' bytes.
extern "C" int tuh_fit_uniforms(int model, double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi,
                                long long *counts) {
  switch (model) {
  case 0: return fit_uniforms<0>(angles, x, n, p0, itmax, opts, multi, counts);
  case 1: return fit_uniforms<1>(angles, x, n, p0, itmax, opts, multi, counts);
  case 2: return fit_uniforms<2>(angles, x, n, p0, itmax, opts, multi, counts);
  }
  return -100;
}
