#pragma once
// resident_fit_impl.h -- kernels of the resident regime (their host side: resident_fit.hip); compiled once per (MODEL, METHOD) by
// resident_inst.hip (nine translation units: one 6.5-minute compile became nine of under a minute, in parallel).
//
// "resident" regime: ONE launch per fit, the samples never leave the chip.
//
// For fits that fit the chip's register file + LDS (n <= #CUs * 4096 samples, i.e. 1,048,576 on MI355X) the whole
// fit runs inside one launch of #CUs workgroups (one 512-thread workgroup per CU, all co-resident).  Every workgroup
// reads its tile of the sample planes from HBM exactly once and keeps it for the rest of the fit:
//
//   waves 1..7                         per lane 8 samples in registers: c0, x, the two per-sample invariants
//                                      (brdf_models.h: Prep) and, for dlevmar_dif, f(p), f(p+Dp) (lm_core.c:551, :742)
//                                      and the Broyden scalar of the last trial (lm_core.c:763)
//   wave 0, "control wave"             the same 8 samples per lane, but parked in LDS (28 KiB): it sweeps them from
//                                      there with a rolled loop, so that the ~250 live registers of the serial LM step it
//                                      also runs never compete with resident samples -- and all four SIMDs carry the
//                                      same sweep load (2 waves x 8 samples; the first version had seven sample waves
//                                      x 10 samples and an idle control wave: 20 sample-iterations on three SIMDs, 10 on
//                                      the fourth)
//   LDS (dlevmar_dif only, 96 KiB)     the secant Jacobian rows, three SoA planes            (lm_core.c:759-769)
//
// A pass (= one LM evaluation: e=x-hx / ||e||^2, FD Jacobian, J^T J / J^T e, Broyden update, brdfdata.cpp:975-988 +
// misc_core.c:153-171 + lm_core.c:617-653) therefore moves no sample bytes at all.  Passes are separated by an
// in-launch exchange of the per-workgroup partial sums instead of a kernel boundary:
//
//   all waves    : sweep -> reduction over the eight waves (barrier X1); the wave that finishes a partial sum publishes it as a
//                  tagged 16-byte cell {lo32, tag, hi32, tag}, ONE write-through (sc1) store (worker_reduce).  (A fit of one
//                  workgroup, and the batched kernels: <= 14 partial sums in LDS behind barrier X2, no exchange.)
//   control wave : gathers everybody's cells in two levels (control_exchange below); folds in a fixed order;
//                  steps ITS OWN copy of the LM state machine (lm_machine.h) -- the same redundant execution as in
//                  the launch chain of stream_fit.hip, so there is no broadcast hop -- in LDS (a register copy of
//                  the machine's busy half was measured and lost, see the control wave's comment below); builds the
//                  next pass's uniforms                                                             (barrier B)
//
// The speculative dlevmar_dif protocol (lm_machine.h): a trial pass forms the Broyden-updated Jacobian row for the sums
// only and keeps the update's scalar t = (f(p+Dp) - f(p) - J Dp)/||Dp||^2 per sample; if the machine adopts the update,
// the NEXT trial pass applies J += t Dp^T on the fly while it reads the row anyway (the first version re-derived t in
// a separate commit sweep: ~1 us per pass).
//
// The cells are recipe R2 of the CDNA guide (cdna_hip_programming.md, Guideline 16: "the data IS the flag"): each
// 8-byte half {32 bits of the double, tag} is naturally aligned and carries its own tag, so a torn cell reads as "not
// ready yet"; no flag, no fence, no ordering between cells is needed.  Tags are (launch base + epoch + 1): the tables are never zeroed between fits.  They
// are double-buffered by epoch parity: a workgroup can be at most one epoch ahead of the slowest one (it needs
// everybody's row of epoch e+1 before it can publish epoch e+2), so two buffers suffice.  Results do not depend on
// dispatch order or XCD placement (fold order = workgroup index).  Every spin is bounded by a wall-clock budget: if
// the grid is not co-resident (or anything else goes wrong) all workgroups drain, the launch ends with ctl->abort set
// and the host falls back to the launch chain (tests/test_gpu_parity.py exercises that path by sabotage).
#include <type_traits>

#if defined(BRDF_STAMPS)
#include <hip/hip_runtime.h>
static __device__ long long g_rlm_stamps[8];  // diagnostic: cycles per section of the machines' run(), workgroup 0 only, summed over passes
static __device__ long long g_rlm_last;
#endif
#if defined(BRDF_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
#define LM_STAMP(i) do { if (blockIdx.x == 0) { const long long now_ = clock64(); if ((i) != 0) g_rlm_stamps[i] += now_ - g_rlm_last; g_rlm_last = now_; } } while (0)
#endif
#include "batch_fit.h"
#include "stream_fit.h"

namespace brdf {

constexpr int kRThreads = 512;               // eight waves, all of them sweep; wave 0 is also the control wave
constexpr int kRSpt = 8;                      // samples per lane
constexpr int kRTile = kRThreads * kRSpt;     // 4096 samples per workgroup (so that #CUs * kRTile >= 2^20 on MI355X)
constexpr int kRCap = kRTile;                 // sample slots per workgroup
constexpr int kRowWords = 2 * kSlots;         // 8-byte granules per partial row: 2 per slot
constexpr int kRowStride = 256;               // most workgroups of a launch (>= #CUs)
constexpr int kRedCols = kRThreads / 4;       // reduction buffer columns (after two in-row DPP steps)
constexpr long long kSpinBudgetTicks = 200000000LL;  // default budget per wait: 2 s of s_memrealtime (100 MHz)

typedef unsigned long long u64;

struct ResidentCtl {  // never zeroed between launches: a word is "set" when it equals the launch's id (ResidentCtx::launch_id)
  unsigned abort;
  unsigned domain_bad;
  unsigned pad[30];
};

struct ResidentCtx {
  const double *c0, *c1, *c2, *x;
  u64 *rows;            // [2][kMaxGroups][kRowWords][kGroup] tagged granules; every tag stored so far is <= tag_base
  u64 *groups;          // [2][kReplicas][kRowWords][kMaxGroups]: sums over groups of 16 workgroups, same granule format
  ResidentCtl *ctl;
  unsigned launch_id;    // nonzero, different for every launch on this workspace
  // what the machine is started from (single fits: every workgroup starts its own copy, as the batched kernels do; the
  // host starts one too, for the argument checks and warnings of the entry point, but nothing is uploaded)
  double p0[kM], opts[5], lb[kM], ub[kM], dscl[kM];
  int itmax, has_opts, has_lb, has_ub, has_dscl, want_covar, multi, analytic;
  int chain;     // dlevmar_dif: trial points per sweep in a chain of rejections (DifMachine::Cold::multi)
  int spec_jac;  // dlevmar_bc_dif / bc_der: candidates evaluated by Jacobian passes (BcMachine::Cold::spec_jac)
  int dif_fused; // dlevmar_dif: the step behind a trial pass tries DifMachine::fused_trial_step first (BRDF_HIP_DIF_FUSED, default on)
  Mailbox *mbox;
  int n;
  unsigned tag_base;  // tags of this launch are tag_base + epoch + 1: the rows need no zeroing between launches
  long long spin_ticks;  // budget of one wait (s_memrealtime ticks)
  int sabotage_epoch;    // test hook (BRDF_HIP_RESIDENT_SABOTAGE): the last workgroup withholds its row at this epoch; -1 = never
  int replicas;          // copies of the group rows in use (1..kReplicas): readers pick copy blockIdx % replicas
  long long *trace;      // diagnostic builds (-DBRDF_STAMPS): [workgroup][8] s_memrealtime stamps of epoch trace_epoch
  int trace_epoch;
};

// METHOD 0 dlevmar_dif, 1 dlevmar_bc_dif / bc_der, 2 dlevmar_der (analytic Jacobian, lm_core.c:64-432)
template <int METHOD>
using RMachine = typename std::conditional<METHOD == 0, DifMachine<kM>, typename std::conditional<METHOD == 1, BcMachine<kM>, DerMachine<kM>>::type>::type;

__device__ __forceinline__ double read_lane(double v, int lane) {  // lane is wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// The sweeps of this kernel are bound by fp64 issue, not by memory, so the accumulations are written as fused
// multiply-adds (one instruction and one rounding instead of two; the library is otherwise built with
// -ffp-contract=off so that lm_machine.h performs the reference's operations one by one).
__device__ __forceinline__ void acc_normal_eq_fma(const double *j, double e, double *jtj6, double *jte3) {
  jtj6[0] = fma(j[0], j[0], jtj6[0]);
  jtj6[1] = fma(j[0], j[1], jtj6[1]);
  jtj6[2] = fma(j[1], j[1], jtj6[2]);
  jtj6[3] = fma(j[0], j[2], jtj6[3]);
  jtj6[4] = fma(j[1], j[2], jtj6[4]);
  jtj6[5] = fma(j[2], j[2], jtj6[5]);
  jte3[0] = fma(j[0], e, jte3[0]);
  jte3[1] = fma(j[1], e, jte3[1]);
  jte3[2] = fma(j[2], e, jte3[2]);
}
// x / d given r = RN(1/d): RN(x*r) followed by one correction step is the correctly rounded quotient (Markstein's
// theorem; the operands here are normal numbers) -- 3 instructions instead of the ~15 of a full fp64 division, for a
// divisor that is the same for every sample of a pass (||Dp||^2, lm_core.c:763)
__device__ __forceinline__ double div_by(double x, double d, double r) {
  const double q = x * r;
  return fma(fma(-q, d, x), r, q);
}

#ifdef BRDF_STAMPS
#define RSTAMP(i) do { const long long now_ = clock64(); st_[i] += now_ - last_; last_ = now_; } while (0)
// one epoch's timeline of EVERY workgroup (arrival skew, hop latencies): slot <- s_memrealtime (100 MHz) or a counter
#define RTRACE(ctx_, epoch_, slot_, val_) do { if ((ctx_).trace && (int)(epoch_) == (ctx_).trace_epoch && (threadIdx.x & 63) == 0) (ctx_).trace[blockIdx.x * 8 + (slot_)] = (long long)(val_); } while (0)
#else
#define RSTAMP(i) do {} while (0)
#define RTRACE(ctx_, epoch_, slot_, val_) do {} while (0)
#endif

// ---- where a lane's samples live ---------------------------------------------------------------------------------
// Fields: 0 c0, 1 x, 2 q1, 3 q2 (Ward only), and for dlevmar_dif 4 hx = f(p), 5 wrk = f(p+Dp), 6 tb = Broyden scalar.
// RegSamples: registers (every index a compile-time constant: the loops over k are fully unrolled).
// LdsSamples: the control wave's copy, [field][k][lane] in LDS, swept by a rolled loop.
constexpr int kFc0 = 0, kFx = 1, kFq1 = 2, kFq2 = 3, kFhx = 4, kFwrk = 5, kFtb = 6;
template <int METHOD>
constexpr int sample_fields() { return METHOD == 0 ? 7 : 4; }

template <int METHOD>
struct RegSamples {
  static constexpr bool kUnrolled = true, kFlips = false;
  double v[sample_fields<METHOD>()][kRSpt];
  __device__ __forceinline__ double get(int f, int k) const { return v[f][k]; }
  __device__ __forceinline__ void set(int f, int k, double x) { v[f][k] = x; }
};
// FLIPS (the control wave of a single dlevmar_dif fit; the batched kernels keep the plain form and their code): "hx <- wrk" on an
// accepted step is a flip of which plane is which -- flip_hx(): a wave-uniform offset added to the two fields' addresses -- and
// not eight ds_read / ds_write pairs in front of the sweep.  After a flip wrk holds the OLD f(p) instead of a second copy of the
// new one: nothing reads wrk before the next trial sweep has written it, and every flip has a trial sweep behind it.
template <int METHOD, bool FLIPS = false>
struct LdsSamples {
  static constexpr bool kUnrolled = false, kFlips = FLIPS;
  double *base;  // + lane
  int hx_off;    // FLIPS: 0, or one field's stride while f(p) lives in the plane named kFwrk and f(p + Dp) in kFhx's
  __device__ __forceinline__ int at(int f, int k) const {
    const int i = (f * kRSpt + k) * kWave;
    if constexpr (FLIPS) return i + (f == kFhx ? hx_off : f == kFwrk ? -hx_off : 0);
    return i;
  }
  __device__ __forceinline__ double get(int f, int k) const { return base[at(f, k)]; }
  __device__ __forceinline__ void set(int f, int k, double x) { base[at(f, k)] = x; }
  __device__ __forceinline__ void flip_hx() { hx_off = (kFwrk - kFhx) * kRSpt * kWave - hx_off; }
};

template <bool UNROLLED, class F>
__device__ __forceinline__ void for_samples(int nk, F &&f) {
  if constexpr (UNROLLED) {
    // (one sample per guarded block.  Two per block -- so that the scheduler can interleave two samples' exp / Broyden chains
    // inside one basic block -- was measured: 28-36 more spilled VGPRs, 539 against 527 us per 10^6-sample dlevmar_dif fit)
#pragma unroll
    for (int k = 0; k < kRSpt; ++k)
      if (k < nk) f(k);
  } else {  // two samples per trip: one sample's dependent chain (exp, Broyden, 13 accumulations) alone leaves the pipe idle
    // (the eight slots unrolled for full tiles -- constant LDS offsets, the next sample's loads free to move up -- was measured: 33
    // spilled VGPRs, 469 against 428 us per 10^6-sample dlevmar_dif fit: this kernel has no register to spare)
#pragma unroll 2
    for (int k = 0; k < nk; ++k) f(k);
  }
}

// ---- the exchange tables' geometry and cells (the exchange itself: control_exchange below; the reducing waves publish into them) ----
constexpr int kGroup = 16;
constexpr int kMaxGroups = 16;  // >= ceil(#CUs / kGroup); also the width of a level-2 row
constexpr int kReplicas = 8;
constexpr size_t kBlockGranules = (size_t)kRowWords * kGroup;                    // one group's rows / one copy of the group rows
constexpr size_t kRowsGranules = 2 * (size_t)kMaxGroups * kBlockGranules;         // [parity][group]
constexpr size_t kGroupsGranules = 2 * (size_t)kReplicas * kBlockGranules;        // [parity][replica]

// A value travels as ONE 16-byte cell = two granules {lo32, tag | hi32, tag}, written by one write-through (sc1) store and
// read by one sc1 load: a scalar sc1 store is one fabric write whatever its size, so 8-byte stores cost 2.7x the time per
// byte of 16-byte ones (MI355X_MICROARCH.md, inter-workgroup visibility table) -- a leader publishes up to 14 x 8 cells
// per pass.  Each half carries its own tag, so a cell torn between its halves is simply "not ready yet".
// A block is [slot][16 columns] cells.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kCacheSc1 = 16;  // aux bits of the gfx940+ buffer instructions: sc1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t table_rsrc(const u64 *p, size_t granules) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<u64 *>(p), 0, (int)(granules * sizeof(u64)), 0x00027000);
}
__device__ __forceinline__ void put_cell(__amdgpu_buffer_rsrc_t t, unsigned cell, unsigned tag, double v) {
  const u32x4 d = {(unsigned)__double2loint(v), tag, (unsigned)__double2hiint(v), tag};
  __builtin_amdgcn_raw_buffer_store_b128(d, t, (int)(cell * 16u), 0, kCacheSc1);
}

// Reduction of NS sums and one max over the eight waves: two DPP steps inside each row of 16 lanes leave the sum of
// every 4 consecutive lanes in lanes 3,7,11,..; those park their values as buf[slot][thread/4]; wave w then owns slots
// {w, w+8}: each lane adds its two entries and one DPP tree per slot finishes it.  A pure function of NS: reproducible.
// MAX = false (dlevmar_dif: its machine never looks at max |e|): no max slot -- one value less per wave, one 16-byte cell less
// per row and, with nine sums, one of the four gather instructions of an exchange
//
// PUB (a single fit spread over several workgroups, pub.on): nobody in this workgroup reads its pre-exchange sums -- only the
// other workgroups do, through the row table.  So the lane that finishes a slot stores that slot's cell itself (the cell, tag
// and store control_exchange() would use: cells are self-validating, any wave may write one) and there is no out[] store, no
// barrier X2 and no read-back by the control wave between the last DPP step and the publish.  All eight waves skip X2 alike;
// red[] has no writer before the next pass's stage 1, behind barrier B.
struct RowPublish {
  const u64 *rows;  // ResidentCtx::rows
  unsigned cell0;   // this workgroup's column of its group's block of this epoch's parity: slot v is cell cell0 + v * kGroup
  unsigned tag;
  bool on;          // the grid has more than one workgroup
  bool withhold;    // test hook (ResidentCtx::sabotage_epoch): this workgroup publishes nothing this epoch
};

template <int NS, bool MAX = true, bool PUB = false>
__device__ __forceinline__ void worker_reduce(const double *acc, double mx, double *buf, double *out, const RowPublish &pub, long long *st_,
                                              long long &last_) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;  // 0..7
  double v[NS + 1];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double t = acc[k];
    t = t + dpp_move<0x111, 0xf, 0xf>(t, 0.0);  // row_shr:1
    t = t + dpp_move<0x112, 0xf, 0xf>(t, 0.0);  // row_shr:2
    v[k] = t;
  }
  if constexpr (MAX) {
    double t = mx;
    t = fmax(t, dpp_move<0x111, 0xf, 0xf>(t, 0.0));
    t = fmax(t, dpp_move<0x112, 0xf, 0xf>(t, 0.0));
    v[NS] = t;
  }
  constexpr int NV = NS + (MAX ? 1 : 0);  // values per lane
  if ((threadIdx.x & 3) == 3) {
#pragma unroll
    for (int k = 0; k < NV; ++k) buf[k * kRedCols + (threadIdx.x >> 2)] = v[k];
  }
  __syncthreads();  // X1
  RSTAMP(6);
  {  // wave w finishes slots w and w + 8 (wave-uniform conditions), the two dependent DPP trees interleaved
    constexpr int NW = kRThreads / kWave;
    const int k0 = wave, k1 = wave + NW;
    const bool has0 = k0 < NV, has1 = k1 < NV;
    double s0 = 0.0, s1 = 0.0;
    if (has0) {
      const double *src = buf + k0 * kRedCols;
      s0 = (k0 < NS || !MAX) ? src[lane] + src[lane + kWave] : fmax(src[lane], src[lane + kWave]);
    }
    if (has1) {
      const double *src = buf + k1 * kRedCols;
      s1 = (k1 < NS || !MAX) ? src[lane] + src[lane + kWave] : fmax(src[lane], src[lane + kWave]);
    }
    // (the max slot is slot NS: it is the LAST slot of whichever wave owns it, so at most one of the two is a max)
    const bool max0 = MAX && has0 && k0 == NS, max1 = MAX && has1 && k1 == NS;
    if (!max0 && !max1) {
      wave_reduce2_to_last<OpSum, OpSum>(s0, s1);
    } else if (max1) {
      wave_reduce2_to_last<OpSum, OpMax>(s0, s1);
    } else {
      wave_reduce2_to_last<OpMax, OpSum>(s0, s1);
    }
    if constexpr (PUB) {
      if (pub.on) {
        if (lane == kWave - 1 && !pub.withhold) {
          const __amdgpu_buffer_rsrc_t rows = table_rsrc(pub.rows, kRowsGranules);
          if (has0) put_cell(rows, pub.cell0 + (max0 ? kSums : k0) * kGroup, pub.tag, s0);
          if (has1) put_cell(rows, pub.cell0 + (max1 ? kSums : k1) * kGroup, pub.tag, s1);
        }
        return;
      }
    }
    if (lane == kWave - 1) {
      if (has0) out[max0 ? kSums : k0] = s0;
      if (has1) out[max1 ? kSums : k1] = s1;
    }
  }
  __syncthreads();  // X2
}

// the RowPublish of this workgroup at `epoch` (the cell and tag arithmetic of control_exchange())
__device__ __forceinline__ RowPublish row_publish(const ResidentCtx &ctx, unsigned epoch) {
  const unsigned grp = blockIdx.x / kGroup;
  return RowPublish{ctx.rows, ((epoch & 1u) * kMaxGroups + grp) * (kSlots * kGroup) + blockIdx.x % kGroup, ctx.tag_base + epoch + 1u, gridDim.x > 1,
                    (int)epoch == ctx.sabotage_epoch && blockIdx.x == gridDim.x - 1};
}

// The exchange, executed by the control wave: a two-level gather.  (A flat all-gather -- every workgroup reading all
// 256 rows -- was measured at 6.2 us: 256 readers per line make the few hundred lines of the row table a hot spot
// of the memory side; more loads in flight per reader made it slower, not faster.)
//
//   level 1  rows [parity][group][slot][member]: workgroups are grouped 16 by 16 and a group's 14 slots x 16 members
//            are 3.5 KB of CONSECUTIVE 16-byte cells.  Every workgroup publishes its NS sums + max, one cell each (slot kSums
//            is the max's): lane 63 of the wave that reduced the slot, or -- !PUBLISHED, the channel kernel -- lanes 0..NS-1
//            and lane 13 of the control wave, from sums[].  One workgroup of a group is its leader (a different
//            position in every group, so that the leaders -- blockIdx % 8 tells which workgroups share an XCD -- are spread
//            over the XCDs).  ALL 64 lanes of its control wave gather: lane l takes member l % 16 of slot 4j + l / 16,
//            j = 0..3 (a wave load instruction reads 1 KB = 8 whole lines; 4 instructions fetch a TRIAL row set), so the 16
//            members of a slot sit in one DPP row and four row reductions (fixed order) fold everything.  (The first
//            version kept ONE table [word][256 workgroups]: a leader's 16 active lanes issued 28 loads, 2 KB apart, per
//            attempt, and an attempt took ~1.5 us -- the in-kernel trace showed level 1 alone at 3.4 us.)
//   level 2  groups [parity][replica][slot][group]: the leader broadcasts each folded value inside its DPP row
//            (row_newbcast) and lanes 0..replicas-1 of the row store one copy each, so that a line is polled by #CUs /
//            replicas workgroups instead of all of them (one copy: +0.9 us).  Every workgroup (leaders too) gathers the
//            <= 16 group rows of copy blockIdx % replicas the same way and folds them: identical bits everywhere.
//
// A gather re-reads its block until every tag matches; false = wait abandoned (spin budget, or somebody else gave up).
template <int NS, bool MAX = true>
__device__ __forceinline__ constexpr bool slot_used(int v) { return v < NS || (MAX && v == kSums); }

// val[j] <- slot 4j + lane/16 of column lane%16 of the block starting at cell `first` (0 where the slot is not used or
// the column >= ncols)
// (Ctx: ResidentCtx, or the per-channel view of channels_fit_impl.h -- anything with ctl, launch_id, spin_ticks)
template <int NS, bool MAX = true, class Ctx>
__device__ __forceinline__ bool gather_block(const Ctx &ctx, __amdgpu_buffer_rsrc_t t, unsigned first, unsigned tag, int ncols,
                                             double (&val)[4], unsigned *polls) {
  const int lane = threadIdx.x & (kWave - 1);  // a control wave's lane (the single-fit kernel's control wave is wave 0)
  const int col = lane & 15, r = lane >> 4;
  const long long t0 = (long long)wall_clock64();
  for (unsigned spins = 0;; ++spins) {
    u32x4 d[4];
    bool ready = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = u32x4{0u, tag, 0u, tag};
      if ((4 * j < NS) || (MAX && 4 * j <= kSums && kSums < 4 * j + 4)) {  // (compile time) some row of this instruction is used
        const int v = 4 * j + r;
        if (slot_used<NS, MAX>(v) && col < ncols) d[j] = __builtin_amdgcn_raw_buffer_load_b128(t, (int)((first + v * kGroup + col) * 16u), 0, kCacheSc1);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ready = ready && d[j].y == tag && d[j].w == tag;
    if (__all(ready)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) val[j] = __hiloint2double((int)d[j].z, (int)d[j].x);
      *polls = spins;
      return true;
    }
    if ((spins & 63u) == 63u) {  // (wave-uniform)
      if (__hip_atomic_load(&ctx.ctl->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ctx.launch_id ||
          (long long)wall_clock64() - t0 > ctx.spin_ticks) {
        __hip_atomic_store(&ctx.ctl->abort, ctx.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// folds the 16 columns of every slot: the total of slot 4j + r ends in lane 16r + 15 of val[j] (the max slot by max)
template <int NS, bool MAX>
__device__ __forceinline__ void fold_block(double (&val)[4]) {
  const int r = (int)(threadIdx.x & (kWave - 1)) >> 4;
  double mx = 0.0;
  if constexpr (MAX) mx = row_reduce_to_last<OpMax>(val[kSums / 4]);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if ((4 * j < NS) || (MAX && j == kSums / 4)) val[j] = row_reduce_to_last<OpSum>(val[j]);  // (compile time: rows in use)
  if (MAX && r == (kSums & 3)) val[kSums / 4] = mx;
}

// PUBLISHED: this workgroup's row is already on its way (worker_reduce<.., PUB>): start at the gathers; sums[] is written only
template <int NS, bool MAX = true, bool PUBLISHED = false, class Ctx>
__device__ __forceinline__ bool control_exchange(const Ctx &ctx, unsigned epoch, double *sums, int *s_abort,
                                                 long long *st_, long long &last_) {
  const int lane = threadIdx.x & (kWave - 1);  // a control wave's lane
  const int col = lane & 15, r = lane >> 4;
  const int G = gridDim.x;
  const int grp = blockIdx.x / kGroup, ngrp = (G + kGroup - 1) / kGroup;
  const int members = min(kGroup, G - grp * kGroup);
  const int leader = grp * kGroup + (grp & 7) % members;
  const unsigned tag = ctx.tag_base + epoch + 1u;
  constexpr unsigned kBlockCells = kSlots * kGroup;
  const __amdgpu_buffer_rsrc_t rows = table_rsrc(ctx.rows, kRowsGranules), groups = table_rsrc(ctx.groups, kGroupsGranules);
  const unsigned my_rows = ((epoch & 1u) * kMaxGroups + grp) * kBlockCells;   // first cell of this group's block
  const unsigned my_groups = (epoch & 1u) * kReplicas * kBlockCells;           // first cell of copy 0 of the group rows
  if constexpr (!PUBLISHED) {
    const bool withhold = (int)epoch == ctx.sabotage_epoch && blockIdx.x == gridDim.x - 1;  // test hook, see ResidentCtx
    if (slot_used<NS, MAX>(lane) && lane <= kSums && !withhold) put_cell(rows, my_rows + lane * kGroup + blockIdx.x % kGroup, tag, sums[lane]);
  }

  double val[4];
  unsigned polls = 0;
  if ((int)blockIdx.x == leader) {  // group leader (workgroup-uniform branch)
    if (!gather_block<NS, MAX>(ctx, rows, my_rows, tag, members, val, &polls)) {
      *s_abort = 1;
      return false;
    }
#ifndef BRDF_TRACE_WORKERS
    RTRACE(ctx, epoch, 6, polls + 1);
#endif
    fold_block<NS, MAX>(val);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double t = dpp_move<0x15F, 0xf, 0xf>(val[j], 0.0);  // row_newbcast:15: the row's total in all 16 lanes of the row
      const int v = 4 * j + r;
      if (slot_used<NS, MAX>(v) && col < ctx.replicas) put_cell(groups, my_groups + col * kBlockCells + v * kGroup + grp, tag, t);
    }
  }
  RSTAMP(2);
  RTRACE(ctx, epoch, 3, wall_clock64());
  if (!gather_block<NS, MAX>(ctx, groups, my_groups + (blockIdx.x % ctx.replicas) * kBlockCells, tag, ngrp, val, &polls)) {
    *s_abort = 1;
    return false;
  }
  fold_block<NS, MAX>(val);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = 4 * j + r;
    if (slot_used<NS, MAX>(v) && col == kGroup - 1) sums[v] = val[j];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  RSTAMP(3);
  RTRACE(ctx, epoch, 4, wall_clock64());
#ifndef BRDF_TRACE_WORKERS
  RTRACE(ctx, epoch, 7, polls);
#endif
  return true;
}

// ---- the uniforms of a request, built by the control wave --------------------------------------------------------------------
// PassUniforms::build() forms them one after the other on one lane's worth of values (every lane the same); each lin() / nl()
// hides an fp64 division or two, and a finite-difference Jacobian request needs seven parameter sets (p, p + d_j e_j, p - d_j e_j),
// a multi-candidate request up to eight: 2,500 shader-clock ticks of the 12 us a dlevmar_bc_dif pass takes.  Here lane l of the
// wave forms parameter set l -- the same operations on the same operands as build(), hence the same bits -- and stores its
// results where build() would.  Everything else goes to build().
template <int MODEL>
__device__ __forceinline__ void build_uniforms_wave(PassUniforms<MODEL> &u, const Request<kM> &r, bool need_base, bool analytic_jac) {
  using Mdl = BrdfModel<MODEL>;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  if (r.kind == RQ_EVAL_MULTI) {
    u.ncand = r.nk;
    u.analytic = analytic_jac ? 1 : 0;
    if (lane < kMaxCand && lane < r.nk) {
      const double pk[kM] = {r.pk[lane][0], r.pk[lane][1], r.pk[lane][2]};
      u.lk[lane] = Mdl::lin(pk);
      u.nk[lane] = Mdl::nl(pk);
    }
    return;
  }
  if ((r.kind == RQ_JAC && !analytic_jac) || r.kind == RQ_DIF_JAC) {
    u.ncand = 0;
    u.analytic = 0;
    u.central = r.central;
    u.scal = r.scal;
    u.dp_l2 = r.dp_l2;
#pragma unroll
    for (int j = 0; j < kM; ++j) u.dp[j] = r.dp[j];
    if (lane < 1 + 2 * kM) {  // 0: p;  1..3: p + d_j e_j;  4..6: p - d_j e_j
      const int j = lane == 0 ? 0 : (lane - 1) % kM;
      const bool plus = lane >= 1 && lane <= kM, minus = lane > kM;
      double pp[kM];
#pragma unroll
      for (int i = 0; i < kM; ++i) {
        pp[i] = r.p[i];
        if (i == j && plus) pp[i] = r.p[i] + r.d[i];   // "p[j]+=d", misc_core.c:161 / "tmp+d", :202
        if (i == j && minus) pp[i] = r.p[i] - r.d[i];  // "p[j]-=d", misc_core.c:199
      }
      const Lin l = Mdl::lin(pp);
      const Nl nn = Mdl::nl(pp);
      if (lane == 0) {
        u.l0 = l;
        u.n0 = nn;
      } else if (plus) {
        u.lp[j] = l;
        if (j == kM - 1) u.np2 = nn;
        double dj = r.d[0];
#pragma unroll
        for (int i = 1; i < kM; ++i)
          if (i == j) dj = r.d[i];
        u.dinv[j] = (r.central ? 0.5 : 1.0) / dj;
      } else {
        u.lm[j] = l;
        if (j == kM - 1) u.nm2 = nn;
      }
    }
    return;
  }
  u.build(r, need_base, analytic_jac);
}

// ---- one pass over a lane's samples ------------------------------------------------------------------------------
// Executed by all eight waves: waves 1..7 on RegSamples (unrolled), the control wave on LdsSamples (rolled).  Leaves the
// lane's partial sums in acc[] / mx and returns the number of sum slots of the request kind (a wave-uniform value).
// `pend` (dlevmar_dif): the machine adopted the Broyden update of the previous trial; tb[] holds its scalar and
// dpp[] its Dp: J += tb Dp^T is applied to the row while it is being read (lm_core.c:760-766).
template <int MODEL, int METHOD, bool FAST, class Store>
__device__ __forceinline__ void sweep_pass(int kind, const PassUniforms<MODEL> &u, Store &st, double *jl, int tid, int nk, int nfull, unsigned okm,
                                           bool pend, const double *dpp, double *acc, double &mx) {
  constexpr bool U = Store::kUnrolled;
  constexpr bool W2 = BrdfModel<MODEL>::prep_planes == 2;
  auto prep = [&](int k) { return Prep{st.get(kFq1, k), W2 ? st.get(kFq2, k) : 0.0}; };
  // slots below nfull = (this workgroup's sample count) / 512 are full in every lane: the masking code sits behind a
  // workgroup-uniform branch and is skipped for them.  (nfull is the WORKGROUP's own count, not the tile's: the last
  // workgroup of a single fit holds up to #workgroups - 1 samples fewer than a tile, so its slot nk - 2 can be partly
  // empty and its slot nk - 1 entirely -- e.g. n = 262,145 on 256 CUs: tile 1025, last workgroup 770 samples.)
  auto dead = [&](int k) { return k >= nfull && !(okm >> k & 1u); };
  // (one sample per guarded block in the evaluation / Jacobian sweeps too.  Two were measured, 10^6-sample Ward dlevmar_bc_dif with every
  // candidate a Jacobian pass: 178 against 172 us per fit -- the register-resident Jacobian body already interleaves its two exp chains)
  switch (kind) {
  case RQ_EVAL:  // (the four kinds only dlevmar_bc_dif / bc_der / der issue are compiled into those kernels only)
    if constexpr (METHOD != 0) {
      const EvalUniforms eu{scalar_copy(u.l0), scalar_copy(u.n0), 1.0};  // (scalar registers: see RQ_DIF_TRIAL)
      for_samples<U>(nk, [&](int k) {
        const double f = model_value<MODEL, FAST>(eu, st.get(kFc0, k), prep(k));
        double e = st.get(kFx, k) - f;
        if (dead(k)) e = 0.0;
        acc[0] = fma(e, e, acc[0]);
        mx = fmax(mx, fabs(e));
      });
    }
    break;
  case RQ_SCALED:
    if constexpr (METHOD != 0) {
      const EvalUniforms eu{scalar_copy(u.l0), scalar_copy(u.n0), scalar_copy(u.scal)};
      for_samples<U>(nk, [&](int k) {
        const double f = model_value<MODEL, FAST>(eu, st.get(kFc0, k), prep(k));
        double t = (st.get(kFx, k) - f) / eu.scal;
        if (dead(k)) t = 0.0;
        acc[0] = fma(t, t, acc[0]);
      });
    }
    break;
  case RQ_EVAL_MULTI:  // bc: candidates of a projected-gradient search; dif: the trial points of a chain of rejections
    if constexpr (METHOD != 2) {
      if (u.ncand == kMaxCand) {
        // the usual case, a full set of candidates: no `j < ncand` guard between the candidates of a sample, so that four
        // independent exp chains share a basic block and interleave (guarded, every candidate is a block of its own and its
        // chain runs alone: scripts/micro/exp_ilp.hip measures 76 cycles per exp and SIMD that way, 51 with four side by side)
        if constexpr (METHOD == 0) {  // (the dlevmar_dif kernels have no register to spare: sample by sample, uniforms read from LDS;
                                      // the group-major form below cost them 24 us per 10^6-sample fit)
          for_samples<U>(nk, [&](int k) {
            const double c0 = st.get(kFc0, k), x = st.get(kFx, k);
            const Prep q = prep(k);
            const bool d = dead(k);
#pragma unroll
            for (int j0 = 0; j0 < kMaxCand; j0 += 4) {
              double e[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) e[j] = x - model_value_k<MODEL, FAST>(u, j0 + j, c0, q);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                if (d) e[j] = 0.0;
                acc[j0 + j] = fma(e[j], e[j], acc[j0 + j]);
              }
            }
          });
          break;
        }
        // ... four candidates at a time over ALL samples, their uniforms (sixteen doubles) in scalar registers for that sweep (see
        // RQ_DIF_TRIAL); every candidate's sum still takes its samples in slot order: configs[3] dlevmar_bc_dif 0.93 -> 0.84 s
#pragma unroll
        for (int j0 = 0; j0 < kMaxCand; j0 += 4) {
          Lin l4[4];
          Nl n4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            l4[j] = scalar_copy(u.lk[j0 + j]);
            n4[j] = scalar_copy(u.nk[j0 + j]);
          }
          for_samples<U>(nk, [&](int k) {
            const double c0 = st.get(kFc0, k), x = st.get(kFx, k);
            const Prep q = prep(k);
            const bool d = dead(k);
            double e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = x - BrdfModel<MODEL>::combine(l4[j], c0, BrdfModel<MODEL>::template shape<FAST>(n4[j], c0, q));  // model_value_k()
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (d) e[j] = 0.0;
              acc[j0 + j] = fma(e[j], e[j], acc[j0 + j]);
            }
          });
        }
        break;
      }
      for_samples<U>(nk, [&](int k) {
        const double c0 = st.get(kFc0, k), x = st.get(kFx, k);
        const Prep q = prep(k);
#pragma unroll
        for (int j = 0; j < kMaxCand; ++j)
          if (j < u.ncand) {
            double e = x - model_value_k<MODEL, FAST>(u, j, c0, q);
            if (dead(k)) e = 0.0;
            acc[j] = fma(e, e, acc[j]);
          }
      });
    }
    break;
  case RQ_JAC:
    if constexpr (METHOD != 0) {
      // The kind of row -- forward differences, central differences, the model's analytic Jacobian (dlevmar_bc_der / dlevmar_der)
      // -- is the same for every sample of a pass: chosen HERE, not inside the sample body.  A branch in the body, uniform or not,
      // splits its basic block between the row's two exp chains; in one block the scheduler interleaves them (measured with
      // scripts/micro/exp_ilp.hip: a lone dependent exp chain takes 237 cycles per exp on a wave, two interleaved 110 each).
      auto jac = [&](auto jk) {
        constexpr int JK = decltype(jk)::value;
        JacUniforms ju;  // the fields this kind of row reads, in scalar registers for the sweep (see RQ_DIF_TRIAL)
        ju.l0 = scalar_copy(u.l0);
        ju.n0 = scalar_copy(u.n0);
        ju.analytic = JK == 2;
        ju.central = JK == 1;
        if (JK == 2) {
          ju.an[0] = scalar_copy(u.an[0]);
          ju.an[1] = scalar_copy(u.an[1]);
        } else {
#pragma unroll
          for (int j = 0; j < kM; ++j) {
            ju.lp[j] = scalar_copy(u.lp[j]);
            ju.dinv[j] = scalar_copy(u.dinv[j]);
            if (JK == 1) ju.lm[j] = scalar_copy(u.lm[j]);
          }
          ju.np2 = scalar_copy(u.np2);
          if (JK == 1) ju.nm2 = scalar_copy(u.nm2);
        }
        for_samples<U>(nk, [&](int k) {
          double f0 = 0.0, j[kM];
          if (JK == 2)
            model_an_row<MODEL, FAST>(ju, st.get(kFc0, k), prep(k), f0, j);
          else if (JK == 1)
            model_fd_row_t<MODEL, FAST, true>(ju, st.get(kFc0, k), prep(k), true, f0, 0.0, false, j);
          else
            model_fd_row_t<MODEL, FAST, false>(ju, st.get(kFc0, k), prep(k), true, f0, 0.0, false, j);
          double e = st.get(kFx, k) - f0;
          if (dead(k)) e = j[0] = j[1] = j[2] = 0.0;
          acc_normal_eq_fma(j, e, acc, acc + kNL);
          acc[kNL + kM] = fma(e, e, acc[kNL + kM]);
        });
      };
      if (u.analytic)
        jac(std::integral_constant<int, 2>{});
      else if (u.central)
        jac(std::integral_constant<int, 1>{});
      else
        jac(std::integral_constant<int, 0>{});
    }
    break;
  case RQ_DIF_INIT:
    if constexpr (METHOD == 0) {
      for_samples<U>(nk, [&](int k) {
        const double h = model_value<MODEL, FAST>(u, st.get(kFc0, k), prep(k));
        st.set(kFhx, k, h);
        double e = st.get(kFx, k) - h;
        if (dead(k)) e = 0.0;
        acc[0] = fma(e, e, acc[0]);
      });
    }
    break;
  case RQ_DIF_JAC:
    if constexpr (METHOD == 0) {
      for_samples<U>(nk, [&](int k) {
        const int s = k * kRThreads + tid;
        const double h = st.get(kFhx, k);
        double f0 = 0.0, j[kM];
        model_fd_row<MODEL, FAST>(u, st.get(kFc0, k), prep(k), false, f0, h, true, j);
        double e = st.get(kFx, k) - h;
        if (dead(k)) e = j[0] = j[1] = j[2] = 0.0;
        jl[s] = j[0];
        jl[kRCap + s] = j[1];
        jl[2 * kRCap + s] = j[2];
        acc_normal_eq_fma(j, e, acc, acc + kNL);
      });
    }
    break;
  case RQ_DIF_TRIAL:  // speculative protocol: the Broyden-updated row is formed for the sums only (see the file comment)
    if constexpr (METHOD == 0) {
      // The pass's uniforms live in LDS (the control wave builds them there); read through `su`, the sweep keeps them in VECTOR
      // registers, and every use of one in an fp64 instruction then costs a register, a copy or an operand slot.  Copied into
      // SCALAR registers once per sweep (readfirstlane: they are wave-uniform) the same loop runs 2.4x faster in isolation
      // (scripts/micro/trial_sweep.hip: 2.0k against 4.9k ticks per sweep of eight samples at two waves per SIMD).
      struct TrialUniforms {
        Lin lq;
        Nl nq;
        double dp[kM], dp_l2;
      };
      TrialUniforms tu;
      tu.lq = scalar_copy(u.lq);
      tu.nq = scalar_copy(u.nq);
#pragma unroll
      for (int j = 0; j < kM; ++j) tu.dp[j] = scalar_copy(u.dp[j]);
      tu.dp_l2 = scalar_copy(u.dp_l2);
      const double dpp_s[kM] = {scalar_copy(dpp[0]), scalar_copy(dpp[1]), scalar_copy(dpp[2])};
      const TrialUniforms &u = tu;  // (shadows the LDS uniforms for the rest of this case)
      const double *dpp = dpp_s;
      const double rinv = 1.0 / u.dp_l2;
      auto value_q = [&](int k) { return model_value_q<MODEL, FAST>(u, st.get(kFc0, k), prep(k)); };
      auto body = [&](int k, const double w) {
        const int s = k * kRThreads + tid;
        const double h = st.get(kFhx, k), x = st.get(kFx, k);
        double jo[kM] = {jl[s], jl[kRCap + s], jl[2 * kRCap + s]};
        if (pend) {  // adopt the previous trial's update: the same operation that formed its jn[] below
          const double tp = st.get(kFtb, k);
#pragma unroll
          for (int j = 0; j < kM; ++j) jo[j] = fma(tp, dpp[j], jo[j]);
          jl[s] = jo[0];
          jl[kRCap + s] = jo[1];
          jl[2 * kRCap + s] = jo[2];
        }
        // broyden_row() (lm_core.c:760-766) with fused multiply-adds (the sweeps are bound by fp64 issue) and the division
        // by ||Dp||^2 done by div_by()
        double t = jo[0] * u.dp[0], jn[kM];
        t = fma(jo[1], u.dp[1], t);
        t = fma(jo[2], u.dp[2], t);
        t = div_by(w - h - t, u.dp_l2, rinv);
#pragma unroll
        for (int j = 0; j < kM; ++j) jn[j] = fma(t, u.dp[j], jo[j]);
        double en = x - w, eo = x - h;
        // (compiling this select into the last slot's copy of the body only -- it is predicated, not branched around, 5 of ~85
        // instructions -- was measured: 43 spilled VGPRs, 605 against 520 us per fit)
        if (dead(k)) en = eo = jn[0] = jn[1] = jn[2] = t = 0.0;
        st.set(kFwrk, k, w);
        st.set(kFtb, k, t);
        // NINE sums, not the machine's thirteen: with J' = J + t Dp^T the products of the updated Jacobian follow from those
        // of the current one, which the machine holds:  J'^T J' = J^T J + a Dp^T + Dp a^T + (t^T t) Dp Dp^T with a = J^T t, and
        // J'^T e = J^T e + Dp (t^T e); only J'^T e' (against the NEW residual) is accumulated directly.  The control wave
        // expands them after the exchange (expand_trial_sums).  Layout: [e'^2, a (3), t^T t, J'^T e' (3), t^T e].  Four
        // accumulators, four reduction slots and four exchange cells fewer per pass: 521 -> 501 us per 10^6-sample fit.
        acc[0] = fma(en, en, acc[0]);
#pragma unroll
        for (int j = 0; j < kM; ++j) acc[1 + j] = fma(jo[j], t, acc[1 + j]);
        acc[1 + kM] = fma(t, t, acc[1 + kM]);
#pragma unroll
        for (int j = 0; j < kM; ++j) acc[2 + kM + j] = fma(jn[j], en, acc[2 + kM + j]);
        acc[2 + 2 * kM] = fma(t, eo, acc[2 + 2 * kM]);
      };
      // (the exp chains of two samples side by side and the Broyden / accumulation halves one after the other was measured too:
      // 455 against 446 us per 10^6-sample fit; whole bodies in pairs spill 28-36 VGPRs)
      for_samples<U>(nk, [&](int k) { body(k, value_q(k)); });  // (the `pend` branch stays in the body)
    }
    break;
  default: break;  // unknown request: the control wave will not survive it either
  }
}

// the matching reduction (the number of sums depends on the request kind only: wave-uniform; a trial sweep leaves kTrialSums:
// device_common.h)
template <int METHOD, bool PUB = false>
__device__ __forceinline__ void reduce_pass(int kind, const double *acc, double mx, double *red, double *sums, const RowPublish &pub, long long *st_,
                                            long long &last_) {
  if constexpr (METHOD == 0) {
    switch (kind) {
    case RQ_DIF_JAC: worker_reduce<SumLayout<kM>::DIF_JAC, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    case RQ_DIF_TRIAL: worker_reduce<kTrialSums, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    case RQ_EVAL_MULTI: worker_reduce<kMaxCand, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    default: worker_reduce<1, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    }
  } else {
    switch (kind) {
    // (max |e| is read after plain evaluations only -- the overflow guards of lmbc_core.c:748, :915 -- so the Jacobian and
    // multi-candidate passes carry no max slot: one reduction value, one exchange cell and one gather instruction less)
    case RQ_JAC: worker_reduce<SumLayout<kM>::JAC, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    case RQ_EVAL_MULTI: worker_reduce<kMaxCand, false, PUB>(acc, mx, red, sums, pub, st_, last_); break;
    default: worker_reduce<1, METHOD == 1, PUB>(acc, mx, red, sums, pub, st_, last_); break;  // (dlevmar_der never reads max |e|)
    }
  }
}

// BATCHED = false: one fit spread over the grid (ctx).  BATCHED = true: one workgroup per fit of 1024 < n <= 4096 samples
// (bctx, batch_fit.h) -- the same eight waves / LDS Jacobian, no exchange between workgroups, the speculative
// dlevmar_dif protocol (one pass per LM iteration), the machine started on the device.
// RAGGED (resident_fit_ragged_kernel, BATCHED): the fit's own sample count (bctx.counts, one scalar load) is n; the row base and
// the plane offsets keep the stride bctx.n.  Both kernels are compiled from one text, resident_fit_kernel.inc.
#define RESIDENT_KERNEL_HEAD                                      \
  template <int MODEL, int METHOD, bool FAST, bool BATCHED>       \
  __global__ __launch_bounds__(kRThreads) void resident_fit_kernel(ResidentCtx ctx, BatchCtx bctx)
#define RESIDENT_KERNEL_FLAGS constexpr bool RAGGED = false;
#define RESIDENT_KERNEL_COUNT(fit_, stride_) (stride_)
#include "resident_fit_kernel.inc"
#undef RESIDENT_KERNEL_HEAD
#undef RESIDENT_KERNEL_FLAGS
#undef RESIDENT_KERNEL_COUNT

#define RESIDENT_KERNEL_HEAD                          \
  template <int MODEL, int METHOD, bool FAST>         \
  __global__ __launch_bounds__(kRThreads) void resident_fit_ragged_kernel(ResidentCtx ctx, RaggedBatchCtx bctx)
#define RESIDENT_KERNEL_FLAGS constexpr bool BATCHED = true, RAGGED = true;
#define RESIDENT_KERNEL_COUNT(fit_, stride_) ragged_count(bctx.counts, (fit_), (stride_))
#include "resident_fit_kernel.inc"
#undef RESIDENT_KERNEL_HEAD
#undef RESIDENT_KERNEL_FLAGS
#undef RESIDENT_KERNEL_COUNT

// ---------------------------------------------------------------------------------------------------
// what an instance exports: a host function that tells its kernels' addresses (the host side that launches them is resident_fit.hip)
// ---------------------------------------------------------------------------------------------------
using ResidentKernelFn = void (*)(ResidentCtx, BatchCtx);
using ResidentRaggedFn = void (*)(ResidentCtx, RaggedBatchCtx);
constexpr int kFastPath = 0, kExactPath = 1;
struct ResidentKernels {
  ResidentKernelFn single[2], batched[2];  // [kFastPath], [kExactPath] (null for Ward, which has no exact path)
  ResidentRaggedFn ragged[2];              // the batched kernels with per-fit sample counts
#ifdef BRDF_STAMPS
  void (*take_lm_stamps)(long long *out8);  // the instance's g_rlm_stamps -> out8, and zeroed
#endif
};

// a kernel's address; null for Ward's exact path (taking the address would instantiate a kernel that is not built)
template <int MODEL, int METHOD, bool FAST, bool BATCHED>
constexpr ResidentKernelFn resident_kernel() {
  if constexpr (FAST || MODEL != MODEL_WARD)
    return resident_fit_kernel<MODEL, METHOD, FAST, BATCHED>;
  else
    return nullptr;
}

template <int MODEL, int METHOD, bool FAST>
constexpr ResidentRaggedFn resident_ragged_kernel() {
  if constexpr (FAST || MODEL != MODEL_WARD)
    return resident_fit_ragged_kernel<MODEL, METHOD, FAST>;
  else
    return nullptr;
}

#ifdef BRDF_STAMPS
static void take_lm_stamps(long long *out8) {
  const long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_rlm_stamps), sizeof zero);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rlm_stamps), zero, sizeof zero);
}
#define BRDF_RESIDENT_STAMPS_ENTRY , take_lm_stamps
#else
#define BRDF_RESIDENT_STAMPS_ENTRY
#endif

// one translation unit per (MODEL, METHOD): resident_inst.hip defines this function for its pair
#define BRDF_RESIDENT_INSTANCE(MODEL_, METHOD_, NAME_)                                                                      \
  ResidentKernels resident_kernels_##NAME_() {                                                                              \
    return {{resident_kernel<MODEL_, METHOD_, true, false>(), resident_kernel<MODEL_, METHOD_, false, false>()},            \
            {resident_kernel<MODEL_, METHOD_, true, true>(), resident_kernel<MODEL_, METHOD_, false, true>()},              \
            {resident_ragged_kernel<MODEL_, METHOD_, true>(), resident_ragged_kernel<MODEL_, METHOD_, false>()} BRDF_RESIDENT_STAMPS_ENTRY}; \
  }

}  // namespace brdf
