// tests/cpp/fit_switches_harness.cpp -- the library's environment switches (brdf_amd/csrc/fit_switches.h: the table and its
// readers) and method codes (fit_host.h: method_spec) behind a C interface, for tests/test_fit_switches.py.  Host compiler, no HIP.
#include "../../brdf_amd/csrc/fit_host.h"

using namespace brdf;

extern "C" {

int fsw_count() { return (int)(sizeof kSwitches / sizeof kSwitches[0]); }
const char *fsw_name(int i) { return kSwitches[i]->name; }
const char *fsw_meaning(int i) { return kSwitches[i]->meaning; }
int fsw_kind(int i) { return kSwitches[i]->kind; }

// what the library makes of switch i right now, read the way its call sites read it.  BRDF_HIP_ROWS: bit 0 the answer for
// dlevmar_dif, bit 1 for dlevmar_bc_dif; text switches: 1 when set; max_replicas, default_spin_ticks: the resident kernels' own
long long fsw_read(int i, int max_replicas, long long default_spin_ticks) {
  const Switch *s = kSwitches[i];
  if (s == &kSwRows) return (rows_path_enabled(true) ? 1 : 0) | (rows_path_enabled(false) ? 2 : 0);
  if (s == &kSwBatchDifChain) return batch_dif_chain();
  if (s == &kSwLaneWaves) return lane_waves_per_simd();
  if (s == &kSwResidentReplicas) return switch_number(*s, max_replicas, 1, max_replicas);
  if (s == &kSwResidentSpinMs) return resident_spin_ticks(default_spin_ticks);
  switch (s->kind) {
  case kOnUnless0:
  case kOffUnless1: return switch_on(*s) ? 1 : 0;
  case kNumber: return switch_number(*s);
  default: return switch_text(*s) ? 1 : 0;
  }
}

int fsw_method_spec(int abi_method, int *machine, int *analytic) {
  MethodSpec ms;
  const bool known = method_spec(abi_method, &ms);
  *machine = ms.machine;
  *analytic = ms.analytic ? 1 : 0;
  return known ? 1 : 0;
}

}  // extern "C"
