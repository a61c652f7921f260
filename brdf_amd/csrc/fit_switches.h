// fit_switches.h -- every BRDF_HIP_* environment switch the library reads: the table, and the only getenv calls of this
// directory.  Plain C++ (no HIP), so that tests/cpp/fit_switches_harness.cpp checks it on a CPU.  Every reader reads the
// environment again on every call: a process may change a switch between two fits (the tests do).
#pragma once

#include <cstdlib>

namespace brdf {

enum SwitchKind {
  kOnUnless0,   // on, off only when the value's first character is '0'
  kOffUnless1,  // off, on only when the value's first character is '1'
  kNumber,      // atoll of the value, clamped to lo..hi; `unset` when the variable is not set
  kText,        // the value itself (readers below, or switch_text)
};

struct Switch {
  const char *name;
  SwitchKind kind;
  long long unset, lo, hi;  // kNumber only
  const char *meaning;
};

constexpr int kSwitchMaxCand = 8;  // lm_machine.h: kMaxCand (fit_host.h asserts that they agree)
constexpr long long kSwitchNoLimit = 0x7fffffffLL;

// clang-format off
constexpr Switch kSwResident        {"BRDF_HIP_RESIDENT", kOnUnless0, 0, 0, 0, "0: the launch chain (and one channel after the other) instead of the resident single-launch regimes"};
  // (default for every single fit that fits the chip.  Measured on MI355X, 1M-sample Ward fit: 14.3 us per dlevmar_dif pass against
  // 19.7 us for the launch chain -- the secant Jacobian no longer travels through HBM -- and 10.7 us per dlevmar_bc_dif pass against 11.3 us)
constexpr Switch kSwChannels        {"BRDF_HIP_CHANNELS", kOnUnless0, 0, 0, 0, "0: brdf_hip_fit_channels_dev fits its channels one after the other, never in one shared launch"};
constexpr Switch kSwLane            {"BRDF_HIP_LANE", kOnUnless0, 0, 0, 0, "0: n <= 16 dlevmar_bc_dif batches take the wave-per-fit / rows kernels instead of one lane per fit"};
constexpr Switch kSwBatchBig        {"BRDF_HIP_BATCH_BIG", kOnUnless0, 0, 0, 0, "0: the symmetric 512 x 8 batched geometry instead of the control-wave kernel for 1024 < n <= 4096"};
constexpr Switch kSwDifFused        {"BRDF_HIP_DIF_FUSED", kOnUnless0, 0, 0, 0, "0: resident dlevmar_dif kernels step every pass with the generic run(), never DifMachine::fused_trial_step (same results)"};
constexpr Switch kSwSpecJac         {"BRDF_HIP_SPEC_JAC", kOnUnless0, 0, 0, 0, "0: single dlevmar_bc_dif / bc_der fits evaluate candidates by plain evaluation passes (BcMachine::Cold::spec_jac)"};
constexpr Switch kSwCosinesRows     {"BRDF_HIP_COSINES_ROWS", kOnUnless0, 0, 0, 0, "0: the one-lane-per-(surfel, light) cosines kernel also for 16 lights"};
constexpr Switch kSwExactPow        {"BRDF_HIP_EXACT_POW", kOffUnless1, 0, 0, 0, "1: the exact model path (reference expression, pow per evaluation) instead of the prepared-sample path"};
constexpr Switch kSwStatsFast       {"BRDF_HIP_STATS_FAST", kOffUnless1, 0, 0, 0, "1: the statistics pass with exp(n log c) for pow (A/B measurements only: no exact fallback)"};
constexpr Switch kSwRows            {"BRDF_HIP_ROWS", kText, 0, 0, 0, "0: never the four-fits-per-wave kernel for n <= 16; 1: always; otherwise dlevmar_dif only (rows_path_enabled)"};
constexpr Switch kSwPgMulti         {"BRDF_HIP_PG_MULTI", kNumber, kSwitchMaxCand, 1, kSwitchMaxCand, "candidates per sweep in dlevmar_bc_dif's projected-gradient search (1 = one at a time)"};
constexpr Switch kSwDifChain        {"BRDF_HIP_DIF_CHAIN", kNumber, kSwitchMaxCand, 1, kSwitchMaxCand, "dlevmar_dif trial points per sweep in a chain of rejections (DifMachine::Cold::multi; 1 = one at a time)"};
constexpr Switch kSwBatchDifChain   {"BRDF_HIP_BATCH_DIF_CHAIN", kNumber, -1, 1, kSwitchMaxCand, "the same for the eight-wave batched kernel; unset: BRDF_HIP_DIF_CHAIN's value (batch_dif_chain)"};
constexpr Switch kSwLaneWaves       {"BRDF_HIP_LANE_WAVES", kNumber, 1, -kSwitchNoLimit, kSwitchNoLimit, "waves per SIMD of the lane-per-fit kernel: 2 or 4, anything else is 1 (lane_waves_per_simd)"};
  // (measured, 2^20 Blinn-Phong fits: 1.43e7 / 1.12e7 / 5.5e6 fits/s at 1 / 2 / 4 -- spills beat occupancy)
constexpr Switch kSwLaneQuorum      {"BRDF_HIP_LANE_QUORUM", kNumber, 24, 1, kSwitchNoLimit, "lane-per-fit kernel: lanes that must wait for a heavy round before one runs"};
  // (measured, 2^20 fits, one wave per SIMD: quorum 1 (no gating) 1.18e7, 8 1.38e7, 16 1.44e7, 24 1.47e7, 32 1.45e7, 40 1.37e7 fits/s)
constexpr Switch kSwLaneMaxwait     {"BRDF_HIP_LANE_MAXWAIT", kNumber, 6, 0, kSwitchNoLimit, "lane-per-fit kernel: most light rounds between two heavy ones"};
constexpr Switch kSwResidentReplicas{"BRDF_HIP_RESIDENT_REPLICAS", kNumber, -1, 1, -1, "copies of the exchange's group rows in use, 1..the kernels' maximum (also the default): switch_number's arguments"};
constexpr Switch kSwResidentSpinMs  {"BRDF_HIP_RESIDENT_SPIN_MS", kNumber, 0, 1, kSwitchNoLimit, "budget of one wait of the exchange in ms, at least 1; unset (0): the kernels' own budget (resident_spin_ticks)"};
constexpr Switch kSwResidentSabotage{"BRDF_HIP_RESIDENT_SABOTAGE", kNumber, -1, -kSwitchNoLimit, kSwitchNoLimit, "tests only: the epoch at which the last workgroup withholds its row, forcing the fallback (-1: never)"};
constexpr Switch kSwResidentBackoff {"BRDF_HIP_RESIDENT_BACKOFF", kNumber, -1, 0, kSwitchNoLimit, "tests: fits for which the resident regime steps aside after an aborted launch; unset (-1): 8, doubling to 1024"};
constexpr Switch kSwResidentTraceEpoch{"BRDF_HIP_RESIDENT_TRACE_EPOCH", kNumber, 20, -kSwitchNoLimit, kSwitchNoLimit, "diagnostic builds (BRDF_STAMPS) only: the epoch whose timeline brdf_hip_last_fit_trace returns"};
constexpr Switch kSwStepDump        {"BRDF_HIP_STEP_DUMP", kText, 0, 0, 0, "diagnostic builds (BRDF_STAMPS) only: file the launch chain appends its per-pass LM step costs to"};
// clang-format on

constexpr const Switch *kSwitches[] = {
    &kSwResident,      &kSwChannels,  &kSwLane,       &kSwBatchBig,         &kSwDifFused,       &kSwSpecJac,          &kSwCosinesRows,
    &kSwExactPow,      &kSwStatsFast, &kSwRows,       &kSwPgMulti,          &kSwDifChain,       &kSwBatchDifChain,    &kSwLaneWaves,
    &kSwLaneQuorum,    &kSwLaneMaxwait, &kSwResidentReplicas, &kSwResidentSpinMs, &kSwResidentSabotage, &kSwResidentBackoff,
    &kSwResidentTraceEpoch, &kSwStepDump,
};

inline const char *switch_text(const Switch &s) { return getenv(s.name); }  // null: not set

inline bool switch_on(const Switch &s) {  // kOnUnless0, kOffUnless1
  const char *e = switch_text(s);
  return s.kind == kOnUnless0 ? !(e && e[0] == '0') : (e && e[0] == '1');
}

inline long long switch_number(const Switch &s, long long unset, long long lo, long long hi) {
  const char *e = switch_text(s);
  if (!e) return unset;
  const long long v = atoll(e);
  return v < lo ? lo : (v > hi ? hi : v);
}
inline long long switch_number(const Switch &s) { return switch_number(s, s.unset, s.lo, s.hi); }

// the switches whose rule is more than a clamp
inline bool rows_path_enabled(bool dif) {
  const char *e = switch_text(kSwRows);
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  return dif;
}
inline int batch_dif_chain() {
  const long long k = switch_number(kSwBatchDifChain);
  return (int)(k < 0 ? switch_number(kSwDifChain) : k);
}
inline long long resident_spin_ticks(long long default_ticks) {  // s_memrealtime ticks (100 MHz)
  const long long ms = switch_number(kSwResidentSpinMs);
  return ms ? ms * 100000LL : default_ticks;
}
inline int lane_waves_per_simd() {
  const long long w = switch_number(kSwLaneWaves);
  return (w == 2 || w == 4) ? (int)w : 1;
}

}  // namespace brdf
