// resident_fit_kernel.inc -- the text of the resident regime's kernel, included by resident_fit_impl.h once per kernel NAME:
//   RESIDENT_KERNEL_HEAD    the template head, the kernel's name and its two arguments (ResidentCtx ctx, <batch context> bctx)
//   RESIDENT_KERNEL_FLAGS   the compile-time properties the head does not carry (RAGGED; for the ragged kernel BATCHED too)
//   RESIDENT_KERNEL_COUNT   (fit, stride) -> the fit's sample count: the stride, or the fit's entry of bctx.counts
// One text, two kernels -- and not one body called from two: a register-tuned kernel whose code is to stay what it was is
// compiled from the tokens it was compiled from (a shared inlined body moved the uniform kernels' allocation by a few spills).
RESIDENT_KERNEL_HEAD {
  RESIDENT_KERNEL_FLAGS
  using Machine = RMachine<METHOD>;
  using Mdl = BrdfModel<MODEL>;
  constexpr int NF = sample_fields<METHOD>();
  // dlevmar_dif: the control wave's 7 x 8 doubles of sample state do not fit next to the LM step's registers: they are
  // parked in LDS.  The other entry points keep 4 x 8 doubles per lane: registers, like every other wave -- except
  // dlevmar_bc_dif spread over the grid, where the exchange code on top of the machine's step spilled 56 VGPRs.
  constexpr bool kControlFromLds = (METHOD == 0) || (METHOD == 1 && !BATCHED);
  static_assert(sizeof(Machine) % 4 == 0, "machine copied as dwords");
  __shared__ Machine sm;
  __shared__ PassUniforms<MODEL> su;
  __shared__ double red[kSlots * kRedCols];
  __shared__ double sums[kSlots];
  __shared__ double dp_prev[kM + 1];  // Dp and ||Dp||^2 of the last trial (dif)
  __shared__ int s_abort, s_bad;
  __shared__ double cst[kControlFromLds ? NF * kRSpt * kWave : 2];  // the control wave's samples
  constexpr int kJl = (METHOD == 0) ? 3 * kRCap : 2;
  __shared__ double jl[kJl];  // dif: the secant Jacobian, SoA planes

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int G = BATCHED ? 1 : (int)gridDim.x;
  const int fit = blockIdx.x;  // BATCHED only
  const int stride = BATCHED ? bctx.n : ctx.n;
  const int n = RESIDENT_KERNEL_COUNT(fit, stride);
  if constexpr (BATCHED && !FAST) {
    if (bctx.flags[fit] != kNeedsExact) return;  // exact kernel: only the fits the fast kernel declined
  }

  // The machine is started here, by all 64 lanes of the control wave (identical values): a fit costs ONE launch and no
  // upload.  (The first version uploaded a host-started machine + two zeroed control words through a pinned staging block
  // before every launch: ~25 us of a 550 us fit; passing the 1.4 KB machine as a kernel ARGUMENT was worse still -- the
  // argument segment is host memory and 256 workgroups read it over the host link.)
  if (wave == 0) {
    // (the arguments are copied into locals first: handing start() pointers INTO the by-value argument structs makes hipcc
    // spill the whole struct to scratch and serve every later ctx.field access from there -- measured +1.3 us per pass)
    double p0[kM], opts[5], lb[kM], ub[kM], dscl[kM];
    int itmax, has_opts, has_lb, has_ub, has_dscl = 0, want_covar = 0, multi, analytic, chain, spec_jac;
    if constexpr (BATCHED) {
#pragma unroll
      for (int i = 0; i < kM; ++i) {
        p0[i] = bctx.p[(size_t)fit * kM + i];
        lb[i] = bctx.lb[i];
        ub[i] = bctx.ub[i];
        dscl[i] = 1.0;
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) opts[i] = bctx.opts[i];
      itmax = bctx.itmax, has_opts = bctx.has_opts, has_lb = bctx.has_lb, has_ub = bctx.has_ub, multi = bctx.multi, analytic = bctx.analytic;
      chain = bctx.chain, spec_jac = bctx.spec_jac;
    } else {
#pragma unroll
      for (int i = 0; i < kM; ++i) {
        p0[i] = ctx.p0[i];
        lb[i] = ctx.lb[i];
        ub[i] = ctx.ub[i];
        dscl[i] = ctx.dscl[i];
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) opts[i] = ctx.opts[i];
      itmax = ctx.itmax, has_opts = ctx.has_opts, has_lb = ctx.has_lb, has_ub = ctx.has_ub, has_dscl = ctx.has_dscl;
      want_covar = ctx.want_covar, multi = ctx.multi, analytic = ctx.analytic, chain = ctx.chain, spec_jac = ctx.spec_jac;
    }
    const double *po = has_opts ? opts : nullptr;
    if constexpr (METHOD == 0) {
      sm.start(p0, n, itmax, po, want_covar, /*speculative=*/1, chain);
    } else if constexpr (METHOD == 1) {
      sm.start(p0, n, has_lb ? lb : nullptr, has_ub ? ub : nullptr, has_dscl ? dscl : nullptr, itmax, po, want_covar, multi, BATCHED ? 0 : spec_jac);
      sm.c.analytic_jac = analytic;
    } else {
      sm.start(p0, n, itmax, po, want_covar);
    }
    (void)analytic, (void)chain, (void)spec_jac;
  }
  if (tid == 0) s_abort = s_bad = 0;
  if (tid <= kM) dp_prev[tid] = 0.0;
  __syncthreads();
  if (wave == 0) {
    if constexpr (METHOD == 1)
      su.build(sm.h.req, true, sm.c.analytic_jac != 0);
    else
      su.build(sm.h.req, true, METHOD == 2);
  }

  // ---- the resident tile: one HBM read ---------------------------------------------------------------------------
  int vb = BATCHED ? 0 : (int)blockIdx.x;  // same XCD-contiguous dealing of tiles as the launch chain
  if (!BATCHED && (G & 7) == 0) vb = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  const int tile = (n + G - 1) / G;  // <= kRTile, checked on the host
  const int begin = vb * tile;
  const int end = min(n, begin + tile);
  const double *pc0 = BATCHED ? bctx.angles + (size_t)fit * 3 * stride : ctx.c0;
  const double *pc1 = BATCHED ? pc0 + stride : ctx.c1;
  const double *pc2 = BATCHED ? pc0 + 2 * (size_t)stride : ctx.c2;
  const double *px = BATCHED ? bctx.x + (size_t)fit * stride : ctx.x;
  const int nk = (tile + kRThreads - 1) / kRThreads;  // occupied sample slots of a lane (workgroup-uniform)
  const int nfull = max(end - begin, 0) / kRThreads;   // slots in which every lane of this workgroup holds a sample
  RegSamples<METHOD> rs;
  LdsSamples<METHOD, METHOD == 0 && !BATCHED> ls{cst + (tid & (kWave - 1)), 0};
  unsigned okm = 0;
  {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kRSpt; ++k) {
      const int i = begin + tid + k * kRThreads;
      const bool ok = i < end;
      okm |= ok ? (1u << k) : 0u;
      const int ii = ok ? i : begin;
      const double r0 = pc0[ii];
      const double r1 = Mdl::uses_c1 ? pc1[ii] : 0.0;
      const double r2 = Mdl::uses_c2 ? pc2[ii] : 0.0;
      const Prep q = Mdl::template prepare<FAST>(r0, r1, r2);
      rs.v[kFc0][k] = r0;
      rs.v[kFx][k] = px[ii];
      rs.v[kFq1][k] = q.q1;
      rs.v[kFq2][k] = q.q2;
      if constexpr (METHOD == 0) rs.v[kFhx][k] = rs.v[kFwrk][k] = rs.v[kFtb][k] = 0.0;
      if (FAST && ok && !Mdl::domain_ok(r0, r1, r2)) bad = true;
    }
    if constexpr (BATCHED) {
      if (FAST && bad) s_bad = 1;  // benign race: every writer stores 1
    } else {
      if (FAST && bad) __hip_atomic_store(&ctx.ctl->domain_bad, ctx.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (kControlFromLds && wave == 0) {  // park the control wave's samples in LDS
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < kRSpt; ++k) ls.set(f, k, rs.v[f][k]);
    }
  }
  __syncthreads();  // machine, uniforms, s_bad and the parked samples are visible

  // a single fit over several workgroups: the waves that finish a reduction slot publish its exchange cell (worker_reduce)
  constexpr bool kPub = !BATCHED;
  auto row_pub = [&](unsigned epoch) {
    if constexpr (kPub)
      return row_publish(ctx, epoch);
    else
      return RowPublish{nullptr, 0u, 0u, false, false};
  };
  int cur_sel_hx = 0, cur_sel_j = 0;
  // what every wave does at the top of a pass (dlevmar_dif): learn what the machine decided about the previous trial
  auto decisions = [&](auto &st, bool &pend) {
    pend = false;
    if constexpr (METHOD == 0) {
      pend = sm.h.req.sel_j != cur_sel_j;  // the Broyden update was adopted: J += tb Dp^T, applied by the next trial sweep
      if (pend && sm.h.req.kind != RQ_DIF_TRIAL) pend = false;  // (a fresh FD Jacobian overwrites J anyway)
      cur_sel_j = sm.h.req.sel_j;
      using Store = typename std::remove_reference<decltype(st)>::type;
      if constexpr (Store::kFlips) {  // step accepted: the two planes trade names (LdsSamples)
        const int sel = lm_uniform(sm.h.req.sel_hx);
        if (sel != cur_sel_hx) st.flip_hx();
        cur_sel_hx = sel;
      } else if (sm.h.req.sel_hx != cur_sel_hx) {  // step accepted: hx <- f(p + Dp)
        for_samples<Store::kUnrolled>(nk, [&](int k) { st.set(kFhx, k, st.get(kFwrk, k)); });
        cur_sel_hx = sm.h.req.sel_hx;
      }
    }
  };

  if (wave == 0) {
    // =========================== control wave: sweep from LDS, exchange, fold, LM step ============================
    // All 64 lanes execute the scalar step with identical values (stream_fit.hip explains why that beats one lane).
    long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long last_ = clock64();
    long long n_jac = 0;
    // The machine is stepped where it lives, in LDS.  Register variants were built and measured (production builds, 10^6-sample
    // Ward dlevmar_dif, us per pass): Machine::Core (the busy half, ~45 doubles + the counters) kept in this wave's registers
    // for the whole fit 11.29 against 10.53 in LDS -- although the step itself got shorter in the stamped build (6970 against
    // 7950 cycles: every `if (h.k < c.itmax ...)` in LDS is a dependent ds_read -> s_waitcnt -> compare -> branch); a register
    // copy made for every step (170 LDS operations to copy in and out) and all of the machine in registers (105 VGPRs
    // spilled) were slower still.
    // dlevmar_dif: what the step reads in every pass but never (constants: options, limits) or only itself (its counters and
    // flags) changes lives in SCALAR registers for the whole fit; the reals stay in LDS with the rest of the machine.  On an
    // LDS-resident machine every `if (h.k < c.itmax ...)` is a dependent ds_read -> s_waitcnt -> compare -> branch.  Same box,
    // 10^6-sample fits: Ward 403.2 -> 401.9 us (constants) -> 398.8 us (+ counters), Blinn-Phong 342.9 -> 338.2 us; all of
    // Machine::Core in (vector) registers was slower (see above), the integers alone cost no vector register.
    typename Machine::Cold cold0;
    typename std::conditional<METHOD == 0, typename DifMachine<kM>::CoreInts, int>::type ints_regs{};
    if constexpr (METHOD == 0) {
      cold0.itmax = lm_uniform(sm.c.itmax);
      cold0.n = lm_uniform(sm.c.n);
      cold0.want_covar = lm_uniform(sm.c.want_covar);
      cold0.refresh = lm_uniform(sm.c.refresh);
      cold0.speculative = lm_uniform(sm.c.speculative);
      cold0.multi = lm_uniform(sm.c.multi);
      cold0.o.forward = lm_uniform(sm.c.o.forward);
      cold0.o.tau = scalar_copy(sm.c.o.tau);
      cold0.o.eps1 = scalar_copy(sm.c.o.eps1);
      cold0.o.eps2 = scalar_copy(sm.c.o.eps2);
      cold0.o.eps2sq = scalar_copy(sm.c.o.eps2sq);
      cold0.o.eps3 = scalar_copy(sm.c.o.eps3);
      cold0.o.delta = scalar_copy(sm.c.o.delta);
      ints_regs = sm.h;
      Machine::uniform_ints(ints_regs);
    }
    const int fused = (METHOD == 0) ? (BATCHED ? bctx.dif_fused : ctx.dif_fused) : 0;
    int n_fused = 0;  // steps fused_trial_step took (reported in the mailbox's stamps[0])
    (void)cold0, (void)ints_regs, (void)fused;
    const long long t_first = (long long)wall_clock64();
    unsigned epoch = 0;
    for (;; ++epoch) {
      const int kind = sm.h.req.kind;
      if (kind == RQ_DONE) break;
      if (kind == RQ_JAC || kind == RQ_DIF_JAC) ++n_jac;
      RTRACE(ctx, epoch, 0, wall_clock64());
      {
        bool pend;
        double acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
        double mx = 0.0;
        const double dpp[kM] = {dp_prev[0], dp_prev[1], dp_prev[2]};
        if constexpr (kControlFromLds) {
          decisions(ls, pend);
          sweep_pass<MODEL, METHOD, FAST>(kind, su, ls, jl, tid, nk, nfull, okm, pend, dpp, acc, mx);
          // (measured and lost: the parked samples brought into registers for the sweep by one burst of ds_reads,
          // the other waves' unrolled register sweep, what the pass changed parked again.  The rolled LDS loop below pays the LDS latency
          // of a sample's seven fields -- 7.0k ticks per sweep against the register waves' ~5k -- but the burst variant spills 46 VGPRs
          // inside the sweep: 480 against 425 us per 10^6-sample fit.)
        } else {
          decisions(rs, pend);
          sweep_pass<MODEL, METHOD, FAST>(kind, su, rs, jl, tid, nk, nfull, okm, pend, dpp, acc, mx);
        }
        RSTAMP(5);  // the control wave's own sweep
        RTRACE(ctx, epoch, 1, wall_clock64());
        // X1, X2: sums[] hold this workgroup's partial sums -- or, in a fit over several workgroups, X1: its row is published
        reduce_pass<METHOD, kPub>(kind, acc, mx, red, sums, row_pub(epoch), st_, last_);
      }
      RSTAMP(1);  // reduction + waiting for the slowest wave
      RTRACE(ctx, epoch, 2, wall_clock64());
      bool alive = true;
      if constexpr (BATCHED && FAST) {  // every wave looked at its cosines while loading the tile
        if (epoch == 0) {
          if (s_bad) {  // log of a non-positive cosine: leave this fit to the exact kernel
            if (tid == 0) bctx.flags[fit] = kNeedsExact;
            s_abort = 1;
            alive = false;
          } else if (tid == 0) {
            bctx.flags[fit] = 0;
          }
        }
      }
      if constexpr (!BATCHED) {  // (a batched fit is one workgroup: sums[] already hold everything)
       if (gridDim.x > 1) {      // ... and so is a single fit of <= 4096 samples: no exchange, no visibility hops
        if constexpr (METHOD == 0) {
          switch (kind) {
          case RQ_DIF_JAC: alive = control_exchange<SumLayout<kM>::DIF_JAC, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          case RQ_DIF_TRIAL: alive = control_exchange<kTrialSums, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          case RQ_EVAL_MULTI: alive = control_exchange<kMaxCand, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          default: alive = control_exchange<1, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          }
        } else {
          switch (kind) {
          case RQ_JAC: alive = control_exchange<SumLayout<kM>::JAC, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          case RQ_EVAL_MULTI: alive = control_exchange<kMaxCand, false, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          default: alive = control_exchange<1, METHOD == 1, kPub>(ctx, epoch, sums, &s_abort, st_, last_); break;
          }
        }
       }
      }
      if (!alive) {  // give up: the host sees no `done`, reads ctl->abort and falls back
        __syncthreads();  // B (the other waves read s_abort behind it)
        return;
      }
      bool stepped = false;
      constexpr bool kTrialFromRegs = METHOD == 0 && !BATCHED;  // (the batched kernels keep su.build)
      if (kind == RQ_DIF_TRIAL) {
        if constexpr (METHOD == 0) {
          // trial judged -> next trial, most steps of a fit: one straight-line block on registers (lm_machine.h:
          // fused_trial_step; nothing of it is live outside this block).  Declined: the machine and sums[] are untouched.
          if (fused) {
            if constexpr (kTrialFromRegs) {
              // A single fit runs the step in its two stages.  The first stores what the other waves read at the top of the next
              // pass (lm_machine.h lists the fields).  Between the stages: the next trial's uniforms from the step's registers,
              // nothing read back, and barrier B.  Behind it, while the other seven waves sweep, the second stage stores the rest
              // of the machine's new state (~30 ds_writes nobody but this wave reads, one exchange away: expand_trial_sums_to).
              const bool took = fused_trial_step_split_device<Machine>(
                  cold0, ints_regs, static_cast<typename Machine::CoreReals &>(sm.h), sm.h.cool, sm.h.req, sums, su.dp, [&](const typename Machine::TrialCommit &late) {
#pragma unroll
                    for (int j = 0; j < kM; ++j) dp_prev[j] = su.dp[j];
                    dp_prev[kM] = su.dp_l2;
                    RSTAMP(7);  // the step alone
                    su.build_trial(late.pdp, late.dp, late.dp_l2, false);
                    RTRACE(ctx, epoch, 5, wall_clock64());
                    __syncthreads();  // B: the next request and its uniforms are in LDS
                    RSTAMP(4);
                  });
              if (took) {  // (the pass has ended in there)
                ++n_fused;
                Machine::uniform_ints(ints_regs);
                continue;
              }
            } else {
              stepped = fused_trial_step_device<Machine>(cold0, ints_regs, static_cast<typename Machine::CoreReals &>(sm.h), sm.h.cool, sm.h.req, sums, su.dp);
              if (stepped) {
                ++n_fused;
                Machine::uniform_ints(ints_regs);
              }
            }
          }
          if (!stepped) expand_trial_sums(static_cast<const typename Machine::Core &>(sm.h), sm.h.cool, su.dp, sums);
        }
#pragma unroll
        for (int j = 0; j < kM; ++j) dp_prev[j] = su.dp[j];
        dp_prev[kM] = su.dp_l2;
      }
      if (!stepped) {  // the LM step, on the machine in LDS
        if constexpr (METHOD == 0) {  // (+ chains of rejections, several trial points to a sweep)
          typename Machine::Cold cc;  // (results are written by the finishing step only and stored right behind it: nothing carried)
          cc.itmax = cold0.itmax, cc.n = cold0.n, cc.want_covar = cold0.want_covar, cc.refresh = cold0.refresh;
          cc.speculative = cold0.speculative, cc.multi = cold0.multi, cc.o = cold0.o;
          for (int i = 0; i < kInfoSz; ++i) cc.info[i] = 0.0;
          for (int i = 0; i < kM * kM; ++i) cc.covar[i] = 0.0;
          cc.ret = kLmError;
          Machine::template run<true, true>(cc, ints_regs, static_cast<typename Machine::CoreReals &>(sm.h), sm.h.cool, sm.h.req, sums, sums[kSums]);
          Machine::uniform_ints(ints_regs);  // (assignments under formally divergent branches lose their uniformity: re-assert it)
          if (sm.h.req.kind == RQ_DONE) {
            for (int i = 0; i < kInfoSz; ++i) sm.c.info[i] = cc.info[i];
            for (int i = 0; i < kM * kM; ++i) sm.c.covar[i] = cc.covar[i];
            sm.c.ret = cc.ret;
          }
        } else
        if constexpr (METHOD == 1)
          sm.template step<true, true, false, !BATCHED>(sums, sums[kSums]);  // (+ candidates evaluated by Jacobian passes: single fits only)
        else
          sm.template step<true>(sums, sums[kSums]);
      }
      RSTAMP(7);  // the step alone
      if (sm.h.req.kind != RQ_DONE) {
        // (lane-parallel for the single box-constrained fit only: the dif kernels have no register for it -- 5 -> 10 spilled VGPRs --
        // and hardly a request that gains; the batched bc kernel spills 8 with it)
        if constexpr (METHOD == 1 && !BATCHED)
          build_uniforms_wave(su, sm.h.req, /*need_base=*/false, sm.c.analytic_jac != 0);
        else if constexpr (METHOD == 1)
          su.build(sm.h.req, /*need_base=*/false, sm.c.analytic_jac != 0);
        else
          su.build(sm.h.req, /*need_base=*/false, METHOD == 2);
      }
      RTRACE(ctx, epoch, 5, wall_clock64());
      __syncthreads();  // B: the next request and its uniforms are in LDS
      RSTAMP(4);
    }
    if constexpr (BATCHED) {
      if constexpr (RAGGED && FAST) {
        if (epoch == 0 && tid == 0) bctx.flags[fit] = 0;  // a start refused for its count ran no pass: nothing for the exact twin
      }
      if (tid == 0) {
        double *po = bctx.p + (size_t)fit * kM;
        for (int i = 0; i < kM; ++i) po[i] = sm.h.p[i];
        if (bctx.info)
          for (int i = 0; i < kInfoSz; ++i) bctx.info[(size_t)fit * kInfoSz + i] = sm.c.info[i];
        if (bctx.ret) bctx.ret[fit] = sm.c.ret;
      }
      return;
    }
    if (blockIdx.x == 0 && tid == 0) {  // every workgroup holds the same finished machine; workgroup 0 reports
      Mailbox *mb = ctx.mbox;
      mb->ret = sm.c.ret;
      mb->passes = (int)epoch;
      if constexpr (METHOD == 1)
        mb->infeasible_mask = sm.c.infeasible_mask;
      else
        mb->infeasible_mask = 0;
      mb->domain_bad = __hip_atomic_load(&ctx.ctl->domain_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ctx.launch_id ? 1 : 0;
      mb->n_jac = n_jac;
      mb->n_eval = (long long)epoch - n_jac;
      mb->t_first = t_first;
      mb->t_last = (long long)wall_clock64();
      st_[0] = n_fused;  // (slot 0 carries no time stamp)
      for (int k = 0; k < 8; ++k) mb->stamps[k] = st_[k];
      for (int i = 0; i < kM; ++i) mb->p[i] = sm.h.p[i];
      for (int i = 0; i < kInfoSz; ++i) mb->info[i] = sm.c.info[i];
      for (int i = 0; i < kM * kM; ++i) mb->covar[i] = sm.c.covar[i];
      __threadfence_system();
      __hip_atomic_store(&mb->done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  // ============================= waves 1..7: register-resident samples ===========================================
  long long wst_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wlast_ = 0;  // (stamps are the control wave's; these are never read)
  for (unsigned epoch = 0;; ++epoch) {  // (the waves loop in lockstep with the control wave: its epoch)
    const int kind = sm.h.req.kind;
    if (kind == RQ_DONE) break;
    bool pend;
    decisions(rs, pend);
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    double mx = 0.0;
    const double dpp[kM] = {dp_prev[0], dp_prev[1], dp_prev[2]};
    sweep_pass<MODEL, METHOD, FAST>(kind, su, rs, jl, tid, nk, nfull, okm, pend, dpp, acc, mx);
#ifdef BRDF_TRACE_WORKERS  // (diagnostic: when do the register-resident waves finish their sweeps? slots 6, 7 = waves 4, 7)
    if constexpr (!BATCHED) {
      if (wave == 4) RTRACE(ctx, epoch, 6, wall_clock64());
      if (wave == 7) RTRACE(ctx, epoch, 7, wall_clock64());
    }
#endif
    reduce_pass<METHOD, kPub>(kind, acc, mx, red, sums, row_pub(epoch), wst_, wlast_);
    __syncthreads();  // B: the control wave has stepped the machine
    if (s_abort) return;
  }
}
