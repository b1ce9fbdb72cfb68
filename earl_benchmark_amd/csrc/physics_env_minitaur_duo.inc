// the body of minitaur_duo_kernel and of minitaur_policy_duo_kernel (physics_env_minitaur.h): `a` is the kernel's argument, a MinitaurArgs or a MinitaurPolicyArgs
#pragma clang fp contract(off)
  // BRANCH (minitaur_branch_kernel / minitaur_branch_duo_kernel, `a` a MinitaurBranchArgs): the K n virtual envs of earl_minitaur_branch_rollout -- `n` is their number, `env`
  // a virtual env, the rows of `a.st` the workspace's.  It takes the POLICY arms as the population launch runs them (a.out.obs == NULL: one carried row, summaries), but for
  // the action, which is given per branch, the pair, which it has none of, and the id of the goal-switch draw, which is the env's
  constexpr bool BRANCH = std::is_same<decltype(a), const MinitaurBranchArgs>::value;
  constexpr bool POLICY = std::is_same<decltype(a), const MinitaurPolicyArgs>::value || BRANCH;
  constexpr int NV = 22, LPE = 32, EPW = 64 / LPE, NP = MT_DUO_PAIRS;
  __shared__ alignas(16) typename ModelOf<NV>::T m;
  __shared__ alignas(16) BlkTable<Lim<NV>::MB, Lim<NV>::KBT> bt;
  __shared__ alignas(16) SharedMT sh[NP * 2 * EPW];
  __shared__ alignas(16) PairTabMT ptab;
  __shared__ int slots_done[NP][2];                     // per pair and role: slots finished (the pair's own barrier; see the slot loop)
  if (threadIdx.x < 2 * NP) (&slots_done[0][0])[threadIdx.x] = 0;
  stage_blocks(bt, a.col);
  stage_kb<NV>(bt, a.m, a.col);
  stage_pairs_mt(ptab, a.col);
  stage_model(m, a.m);                                  // (ends with a workgroup barrier)
  const earl_minitaur_cfg& cfg = a.cfg;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPE, grp = lane / LPE, n = cfg.n;
  const int pair = wave & (NP - 1);
  const bool role_b = wave >= NP;                       // (waves w and w + 4 of a workgroup land on the same SIMD: every SIMD hosts one wave of each role)
  // (measured and left out: issue priority for the solver half -- the longer one -- 138.7 -> 147.5 ms per bench launch, for the dynamics half 139.9; s_sleep 1 / 32 in the pair barrier 139.3 / 140.2)
  // (this lane's motor constants are re-read where they are used, from a lane index the compiler cannot follow: hoisted out of the slot loop they sat in registers across both
  // halves of the timestep and were spilled around them)
  const int NS = cfg.num_substeps, TT = a.T * NS;       // timesteps per env of this launch
  const int gcf = a.st.steps_since_goal_change ? cfg.goal_change_frequency : 0;
  auto env_of = [&](const int q, const int grp_) { return (int)((blockIdx.x * NP + pair) * 2 + q) * EPW + grp_; };
  // ---- both slots of this pair: state rows -> LDS (wave A; wave B waits at the first barrier)
  if (!role_b) {
    for (int q = 0; q < 2; ++q) {
      const int env_raw = env_of(q, grp), env = env_raw < n ? env_raw : n - 1;
      SharedMT& s = sh[(pair * 2 + q) * EPW + grp];
      const double* mp = a.st.motor_param + (size_t)env * 6;
      load_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
#ifdef EARL_MT_DEBUG
      if (sub == 0) { s.dbg_env = env < 4096 ? env : 4095; s.dbg_ts = 0; }
#endif
      if (sub < NV) s.xt.ext[sub] = 0.0;
      if (sub < 8) {
        s.ev.oh[sub] = a.st.overheat[(size_t)env * 8 + sub]; s.ev.en[sub] = a.st.motor_enabled[(size_t)env * 8 + sub] != 0 ? 1 : 0;
        s.ev.obs_t[sub] = a.st.observed_torque[(size_t)env * 8 + sub]; s.ev.cmd[sub] = 0.0;
      }
      if (sub == 0) {
        s.xt.mscale[0] = mp[2]; s.xt.mscale[1] = mp[3]; s.xt.mscale[2] = mp[4]; s.xt.foot_mu = mp[5]; s.xt.motor_volt = mp[0]; s.xt.motor_visc = mp[1];
        s.ev.goal[0] = a.st.goal[(size_t)env * 2]; s.ev.goal[1] = a.st.goal[(size_t)env * 2 + 1];
        s.ev.steps = a.st.steps_since_reset ? a.st.steps_since_reset[env] : 0;
        s.ev.sgc = gcf > 0 ? a.st.steps_since_goal_change[env] : 0;
      }
    }
    fence();
  }
  // (wave A) what stands between the last timestep of env step t and the first of env step t + 1 of slot q: the tail of minitaur_kernel's step loop
  auto finish_step = [&](SharedMT& s, const int env, const bool live, const int t, const int sub, const int grp) {      // (sub, grp: the caller's laundered lane indices, see the slot loop)
    const size_t row = (size_t)t * n + env;
    const bool bad_lane = (sub < NV && !(fabs(s.qp[sub]) < EARL_BAD_VALUE && fabs(s.qv[sub]) < EARL_BAD_VALUE)) || (sub < 4 && !(fabs(s.bq[sub]) < EARL_BAD_VALUE));
    const bool failed = group_any<LPE>(bad_lane, grp);
    const int steps = s.ev.steps + 1;
    double goal0 = s.ev.goal[0], goal1 = s.ev.goal[1];
    double v;
    [[maybe_unused]] double rew = 0.0;                // POLICY: what out.reward / out.success hold or would hold for this step, for the episode summary
    [[maybe_unused]] uint8_t suc = 0;
    if (failed) {
      load_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
      if (sub < 8) {
        s.ev.oh[sub] = a.st.overheat[(size_t)env * 8 + sub]; s.ev.en[sub] = a.st.motor_enabled[(size_t)env * 8 + sub] != 0 ? 1 : 0; s.ev.obs_t[sub] = a.st.observed_torque[(size_t)env * 8 + sub];
      }
      if constexpr (POLICY) {
        // (POLICY only, as in the one-wave kernel: without out.obs the env's row of st.last_obs stays; reward 0 and success 0 go out with the summary below)
        if (a.out.obs) {
          v = t > 0 ? a.out.obs[(row - n) * 32 + sub] : (a.st.last_obs ? a.st.last_obs[(size_t)env * 32 + sub] : NAN);
          if (live) a.out.obs[row * 32 + sub] = v;
        }
        if (live && sub == 0 && a.st.fail_count) a.st.fail_count[env] += 1;
      } else {
      v = t > 0 ? a.out.obs[(row - n) * 32 + sub] : (a.st.last_obs ? a.st.last_obs[(size_t)env * 32 + sub] : NAN);
      if (live) {
        a.out.obs[row * 32 + sub] = v;
        if (sub == 0) {
          a.out.reward[row] = 0.0; a.out.success[row] = 0;
          if (a.st.fail_count) a.st.fail_count[env] += 1;
        }
      }
      }
      fence();
    } else {
      // GetObservation + goal (minitaur.py:300-324, minitaur_gym_env.py:541-546): lane k holds entry k of the 32
      if (sub < 8) s.kit.obs[16 + sub] = s.ev.obs_t[sub];
      fence();
      if (sub < 8) v = s.qp[cfg.motor_dof[sub]] * cfg.motor_dir[sub];
      else if (sub < 16) v = s.qv[cfg.motor_dof[sub - 8]] * cfg.motor_dir[sub - 8];
      else if (sub < 24) v = s.kit.obs[sub];
      else if (sub < 28) v = s.bq[sub == 27 ? 0 : sub - 23];       // Bullet's (x, y, z, w)
      else if (sub < 30) v = s.qp[sub - 28];
      else v = sub == 30 ? goal0 : goal1;
      fence();
      s.kit.obs[sub] = v;
      fence();
      {
        const double qn = renormalised_quat_entry<NV>(s, sub);
        fence();
        if (live) store_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
        if (sub < 4) s.bq[sub] = qn;
        fence();
      }
      if (live) {
        if (sub < 8) {
          a.st.overheat[(size_t)env * 8 + sub] = s.ev.oh[sub]; a.st.motor_enabled[(size_t)env * 8 + sub] = s.ev.en[sub] ? 1 : 0; a.st.observed_torque[(size_t)env * 8 + sub] = s.ev.obs_t[sub];
        }
        if constexpr (POLICY) {
          // row t of out.obs, or -- out.obs == NULL -- the env's row of st.last_obs, the one observation row such a launch keeps (see the one-wave kernel)
          (a.out.obs ? a.out.obs + row * 32 : a.st.last_obs + (size_t)env * 32)[sub] = v;
          if (sub == 0) {                               // the same expressions as below, kept for the stores after the branch
            const double* o = s.kit.obs;
            const double xd = o[28] - goal0, yd = o[29] - goal1;
            double dotp = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) dotp = fma(o[16 + k], o[8 + k], dotp);
            rew = cfg.distance_weight * (-fabs(xd) - fabs(yd)) - cfg.energy_weight * (fabs(dotp) * m.dt);
            suc = sqrt(xd * xd + yd * yd) < cfg.success_radius;
          }
        } else {
        a.out.obs[row * 32 + sub] = v;
        if (sub == 0) {                                 // _reward (minitaur_gym_env.py:505-521) = compute_reward (:529-535) on this observation; is_successful :495-503
          const double* o = s.kit.obs;
          const double xd = o[28] - goal0, yd = o[29] - goal1;
          double dotp = 0.0;
#pragma unroll
          for (int k = 0; k < 8; ++k) dotp = fma(o[16 + k], o[8 + k], dotp);
          a.out.reward[row] = cfg.distance_weight * (-fabs(xd) - fabs(yd)) - cfg.energy_weight * (fabs(dotp) * m.dt);
          a.out.success[row] = sqrt(xd * xd + yd * yd) < cfg.success_radius;
        }
        }
      }
    }
    if constexpr (POLICY) {
      // reward and success of the step (a rolled-back step: 0 and 0) to their rows, each NULL or given, and into the env's episode summary, whose pointers are read
      // through the kernel-argument segment here, where they are used (as in the one-wave kernel)
      if (sub == 0 && live) {
        const double r_t = failed ? 0.0 : rew;
        const uint8_t s_t = failed ? (uint8_t)0 : suc;
        if (a.out.reward) a.out.reward[row] = r_t;
        if (a.out.success) a.out.success[row] = s_t;
        if constexpr (BRANCH) mt_branch_summary(t, env, r_t, s_t);      // (the same three words, rows [K n] of the caller's summary)
        else cl_episode_summary(cl_kernarg<MinitaurPolicyArgs>(), t, env, r_t, s_t);
        if (a.out.status) a.out.status[row] = failed ? EARL_STEP_DIVERGED : 0;
        if (a.out.done) a.out.done[row] = (cfg.horizon > 0 && steps >= cfg.horizon) ? 1 : 0;
      }
    } else {
    if (sub == 0 && live) {
      if (a.out.status) a.out.status[row] = failed ? EARL_STEP_DIVERGED : 0;
      a.out.done[row] = (cfg.horizon > 0 && steps >= cfg.horizon) ? 1 : 0;
    }
    }
    if constexpr (POLICY && !BRANCH) mt_pair_handover(a, t, env, row, sub, live, failed, suc, goal0, goal1);      // earl_minitaur_agents_rollout: the new goal goes to s.ev.goal below and to st.goal
    int sgc = s.ev.sgc;
    fence();
    if (gcf > 0 && ++sgc >= gcf) {                      // LifelongWrapper.step (lifelong_wrapper.py:36-42): new goal, the observation re-read with it
      sgc = 0;
      const int draw_env = mt_draw_env<BRANCH>(env);      // (BRANCH: the ENV's id, never the virtual index: every branch of an env sees the goal the env's next rollout will see)
      int gi = (int)(mt_draw(cfg, 0xFFFEu, draw_env, cfg.step_counter + (a.clock ? a.clock[1] : 0) + (uint64_t)t) * (double)cfg.n_goals);
      gi = gi >= cfg.n_goals ? cfg.n_goals - 1 : gi;
      goal0 = cfg.goal_table[2 * gi]; goal1 = cfg.goal_table[2 * gi + 1];
      if constexpr (POLICY) {
        if (live && sub >= 30) (a.out.obs ? a.out.obs + row * 32 : a.st.last_obs + (size_t)env * 32)[sub] = sub == 30 ? goal0 : goal1;
      } else
      if (live && sub >= 30) a.out.obs[row * 32 + sub] = sub == 30 ? goal0 : goal1;
      if (live && sub == 0) { a.st.goal[(size_t)env * 2] = goal0; a.st.goal[(size_t)env * 2 + 1] = goal1; }
    }
    if (sub == 0) { s.ev.steps = steps; s.ev.sgc = sgc; s.ev.goal[0] = goal0; s.ev.goal[1] = goal1; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");   // a later step of this launch may read this row / the state rows back (failure guard)
    fence();
  };
  // Slot j: wave A works on (slot q = j & 1, timestep j >> 1), wave B on the slot-timestep A finished in slot j - 1.  One barrier per slot.
#ifdef EARL_PHYS_PROF
  const unsigned long long duo_t0 = __builtin_readcyclecounter();
  unsigned long long duo_wait = 0;
#endif
  for (int j = 0; j <= 2 * TT + 1; ++j) {
#ifdef EARL_PHYS_PROF
    const unsigned long long slot_t0 = __builtin_readcyclecounter();
#endif
    if (!role_b) {
      // (the lane's indices pass through an empty asm once per slot: everything derived from them in the code around the timesteps -- rows of the kernel's tables, addresses of
      // the env's rows in HBM -- is then worked out where it is used instead of being hoisted out of the slot loop, held across both halves of the timestep, spilled, and reloaded
      // from scratch memory with a wait each: 33 reloads per slot)
      int lane_ = lane;
      asm volatile("" : "+v"(lane_));
      const int sub = lane_ % LPE, grp = lane_ / LPE;
      const int q = j & 1, ts = j >> 1, t = ts / NS, k = ts - t * NS;
      const int env_raw = env_of(q, grp), env = env_raw < n ? env_raw : n - 1;  // idle groups shadow the last env and store nothing
      const bool live = env_raw < n;
      SharedMT& s = sh[(pair * 2 + q) * EPW + grp];
      if (ts > 0) {                                     // K10 of this slot's timestep before: wave B left the solution in s.aprev (1.7 k cycles off the longer half)
        const bool isroot = sub < 6, ishinge = sub >= 8 && sub < 24, isl = isroot || ishinge;
        const int l = isroot ? sub : (ishinge ? sub - 2 : NV - 1);
        const double al = s.aprev[l], qd = s.qv[l], ql = s.qp[l];
        const Q4 Qb = ldq(s.bq);
        integrate_mt(s, m, sub, isl, l, m.dt, al, qd, ql, Qb);
      }
      if (k == 0) {
        if (t > 0) finish_step(s, env, live, t - 1, sub, grp);
        if (t < a.T) {                                  // ConvertFromLegModel of env step t's action -> this motor's command, kept for the step's timesteps
          double a64[8];
          mt_step_action<POLICY>(a, t, n, env, sub, live, a64);
          if (sub < 8) s.ev.cmd[sub] = earl::mt_leg_to_motor(a64, sub);
        }
      }
      if (ts < TT) {
        // Minitaur.ApplyAction (minitaur.py:326-390) of motor `mi`: as minitaur_kernel's apply_action, counters in LDS
        if (sub < 8) {
          int ml = sub;
          asm volatile("" : "+v"(ml));
          const int mdof = cfg.motor_dof[ml & 7];
          const double mdir = cfg.motor_dir[ml & 7], lim = m.dt * cfg.motor_velocity_limit;
          const double qm = s.qp[mdof] * mdir, qdm = s.qv[mdof] * mdir;
          const double c = earl::mt_clipd(s.ev.cmd[sub], qm - lim, qm + lim);
          double act, obs;
          earl::mt_motor_torque(cfg.motor_kp, cfg.motor_kd, s.xt.motor_volt, s.xt.motor_visc, false, c, qm, qdm, act, obs);
          const int oh = fabs(act) > cfg.overheat_torque ? s.ev.oh[sub] + 1 : 0;
          int en = s.ev.en[sub];
          if (oh > cfg.overheat_steps) en = 0;
          s.ev.oh[sub] = oh; s.ev.en[sub] = en; s.ev.obs_t[sub] = obs;
          s.xt.ext[mdof] = en ? act * mdir : 0.0;
        }
        fence();
        int sub_ = sub;
        asm volatile("" : "+v"(sub_));
        __builtin_assume(sub_ >= 0 && sub_ < LPE);
        substep_mt<true, 1>(s, m, bt, ptab, sub_, grp, k > 0, nullptr);
      }
    } else if (j >= 1) {
      const int jj = j - 1, q = jj & 1, ts = jj >> 1;
      if (ts < TT) {
        SharedMT& s = sh[(pair * 2 + q) * EPW + grp];
        int sub_ = sub;
        asm volatile("" : "+v"(sub_));
        __builtin_assume(sub_ >= 0 && sub_ < LPE);
        substep_mt<true, 2>(s, m, bt, ptab, sub_, grp, (ts % NS) > 0, nullptr);
      }
    }
#ifdef EARL_PHYS_PROF
    const unsigned long long slot_t1 = __builtin_readcyclecounter();
#endif
    // The PAIR's barrier (not the workgroup's: the four pairs have nothing to wait for in each other, and a slot lasts as long as its active-set passes): each wave
    // publishes the number of slots it has finished and waits for its partner's to reach the same.  (release / acquire at workgroup scope around the flag: the halves
    // hand their results over through LDS.)
    {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      volatile int* mine = &slots_done[pair][role_b ? 1 : 0];
      volatile int* other = &slots_done[pair][role_b ? 0 : 1];
      if (lane == 0) *mine = j + 1;
      while (*other < j + 1) __builtin_amdgcn_s_sleep(4);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
#ifdef EARL_PHYS_PROF
    PCOUNT(26, slot_t1 - slot_t0); PCOUNT(27, __builtin_readcyclecounter() - slot_t1); PCOUNT(28, 1);      // this wave's work and wait per slot
    duo_wait += __builtin_readcyclecounter() - slot_t1;
#endif
  }
#ifdef EARL_PHYS_PROF
  if (lane == 0 && blockIdx.x * 2 * NP + wave < 2048) {      // every wave's duration and the part of it spent at the pair's barrier (load balance: tools/prof_minitaur.py)
    g_wave_cycles[blockIdx.x * 2 * NP + wave] = __builtin_readcyclecounter() - duo_t0;
    g_wave_cycles[2048 + blockIdx.x * 2 * NP + wave] = duo_wait;
  }
#endif
  if (!role_b) {
    for (int q = 0; q < 2; ++q) {
      const int env_raw = env_of(q, grp), env = env_raw < n ? env_raw : n - 1;
      SharedMT& s = sh[(pair * 2 + q) * EPW + grp];
      if (env_raw < n) {
        if (sub == 0) {
          if (a.st.steps_since_reset) a.st.steps_since_reset[env] = s.ev.steps;
          if (gcf > 0) a.st.steps_since_goal_change[env] = s.ev.sgc;
        }
        if constexpr (POLICY) {                         // (without out.obs the env's row of last_obs was kept current step by step)
          if (a.out.obs && a.st.last_obs && a.T > 0) a.st.last_obs[(size_t)env * 32 + sub] = a.out.obs[((size_t)(a.T - 1) * n + env) * 32 + sub];
        } else
        if (a.st.last_obs && a.T > 0) a.st.last_obs[(size_t)env * 32 + sub] = a.out.obs[((size_t)(a.T - 1) * n + env) * 32 + sub];
      }
    }
  }
