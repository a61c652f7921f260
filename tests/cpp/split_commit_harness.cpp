// tests/cpp/split_commit_harness.cpp -- TEST HARNESS (not product code).
//
// DifMachine::fused_trial_step (brdf_amd/csrc/lm_machine.h) exists in two stages for the single-fit resident kernel:
// fused_trial_step_split's first stage stores what other waves read before the next exchange (the early fields: CoreInts,
// req.kind, req.sel_hx, req.sel_j), calls the caller's part with the rest in a TrialCommit -- the kernel's barrier is in there --
// and fused_trial_commit then stores the rest (the late fields).
// This harness drives TWO DifMachine<3> through whole fits with the reference-order pass executor of host_machine.cpp, as
// dif_fused_harness.cpp does: `a` is stepped by the one-shot fused step, `b` by the split form (both by run() where the fused
// step declines -- they must decline together).  After every step CoreInts, CoreReals, Cool and Request are memcmp-equal.
// BETWEEN the stages the early fields of `b` already hold the bytes `a` has, and every late field still holds the previous
// step's: the second stage is all that is missing.  Built by tests/test_split_commit_host.py.
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

// between the stages: 0, or 5 an early field is not final yet, 6 a late field has been touched
int between_stages(const Dif &done, const Dif &mid, const Dif &prev) {
  if (memcmp(static_cast<const Dif::CoreInts *>(&done.h), static_cast<const Dif::CoreInts *>(&mid.h), sizeof(Dif::CoreInts))) return 5;
  if (mid.h.req.kind != done.h.req.kind || mid.h.req.sel_hx != done.h.req.sel_hx || mid.h.req.sel_j != done.h.req.sel_j) return 5;
  if (memcmp(static_cast<const Dif::CoreReals *>(&prev.h), static_cast<const Dif::CoreReals *>(&mid.h), sizeof(Dif::CoreReals))) return 6;
  if (memcmp(&prev.h.cool, &mid.h.cool, sizeof(Dif::Cool))) return 6;
  Request<3> r;
  memcpy(&r, &mid.h.req, sizeof r);  // (bytes, padding included)
  r.kind = prev.h.req.kind;
  r.sel_hx = prev.h.req.sel_hx;
  r.sel_j = prev.h.req.sel_j;
  if (memcmp(&r, &prev.h.req, sizeof r)) return 6;
  return 0;
}

template <int MODEL>
int fit_pair(double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi, int want_covar,
             long long *counts, double *p_out, double *info_out) {
  HostPasses<MODEL, false> hp(angles, x, n, 0);
  static Dif a, b, prev;  // (zeroed, padding included, so that memcmp sees only what the machines wrote)
  memset(&a, 0, sizeof a);
  memset(&b, 0, sizeof b);
  a.start(p0, n, itmax, opts, want_covar, /*speculative=*/1, multi);
  b.start(p0, n, itmax, opts, want_covar, /*speculative=*/1, multi);
  double s[SumLayout<3>::MAX] = {0};
  double mx = 0.0;
  long long steps = 0, fused = 0, trial_steps = 0, late_moved = 0;
  int bad = hot_differs(a, b);
  while (!bad && a.h.req.kind != RQ_DONE) {
    const bool trial = a.h.req.kind == RQ_DIF_TRIAL;
    hp.run(a.h.req, s, mx);
    const bool took_a = Dif::template fused_trial_step<false, true>(a.c, a.h, a.h, a.h.cool, a.h.req, s);
    if (!took_a) a.template step<false, true>(s, mx);
    memcpy(&prev, &b, sizeof prev);
    int mid = 0;  // what the state between the stages looked like
    const bool took_b = Dif::template fused_trial_step_split<false, true>(b.c, b.h, b.h, b.h.cool, b.h.req, s, [&](const Dif::TrialCommit &tc) {
      mid = between_stages(a, b, prev);
      // ... and tc carries what the next trial's uniforms are formed from
      if (!mid && (memcmp(tc.pdp, a.h.req.q, sizeof tc.pdp) || memcmp(tc.dp, a.h.req.dp, sizeof tc.dp) || memcmp(&tc.dp_l2, &a.h.req.dp_l2, sizeof tc.dp_l2))) mid = 9;
    });
    if (took_b != took_a) {
      bad = 7;
    } else if (took_b) {
      ++fused;
      bad = mid;
      // the second stage moves something (else the check above proves nothing): the late fields differ from the previous step's
      late_moved += memcmp(static_cast<const Dif::CoreReals *>(&prev.h), static_cast<const Dif::CoreReals *>(&b.h), sizeof(Dif::CoreReals)) != 0;
    } else {
      if (memcmp(&prev, &b, sizeof prev)) bad = 8;  // declined: nothing was written
      b.template step<false, true>(s, mx);
    }
    ++steps;
    trial_steps += trial;
    if (!bad) bad = hot_differs(a, b);
    if (bad) bad += 10 * (int)(steps < 100000 ? steps : 99999);  // <step> * 10 + part
  }
  counts[0] = steps;
  counts[1] = fused;
  counts[2] = trial_steps;
  counts[3] = late_moved;
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

// counts[4]: steps, steps the fused path took, steps behind a trial pass, fused steps whose second stage changed the reals.
// Returns 0 when the machines agreed after every step and at the end, and the state between the stages was as documented;
// else <step> * 10 + part: 1 ints, 2 reals, 3 cool, 4 request differ behind the step; 5 an early field not final between the
// stages, 6 a late field touched by the first stage, 7 one form took the step and the other declined, 8 a declined first stage
// wrote something, 9 the TrialCommit does not carry the next trial; -1 p, -2 info, -3 covar, -4 ret.
extern "C" int sch_fit_pair(int model, double *angles, double *x, int n, const double *p0, int itmax, double *opts, int multi,
                            int want_covar, long long *counts, double *p_out, double *info_out) {
  switch (model) {
  case 0: return fit_pair<0>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  case 1: return fit_pair<1>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  case 2: return fit_pair<2>(angles, x, n, p0, itmax, opts, multi, want_covar, counts, p_out, info_out);
  }
  return -100;
}
