// physics_env_sawyer_rollout.inc -- the body of the Sawyer door / peg rollout kernels (physics_env_sawyer.h): sawyer_rollout_kernel includes it with POLICY = false
// (every action given), sawyer_policy_rollout_kernel with POLICY = true (the action of env step t computed by the env's own 16 lanes from the observation the env
// last emitted), sawyer_branch_rollout_kernel with BRANCH = true (the K n virtual envs of earl_sawyer_branch_rollout: `a.cfg.n` is their number, `env` a virtual env, the rows
// of `a.st` the workspace's; actions given per branch, no [T] row written, per-branch summaries), sawyer_prior_rollout_kernel with BRANCH = true in the units built with
// EARL_BRANCH_PRIOR (the action of a prior branch computed by the policy on the row the virtual env carries).  Template parameters NV, LPE, SLICED and the kernel argument
// `a` are the including kernel's.
  static_assert(LPE >= 14, "the observation is written by 14 lanes");
  constexpr int EPW = 64 / LPE, WPB = Lim<NV>::WPB;
  __shared__ alignas(16) typename ModelOf<NV>::T m;
  __shared__ alignas(16) BlkTable<Lim<NV>::MB, Lim<NV>::KBT> bt;
  __shared__ alignas(16) Shared<NV> sh[EPW * WPB];
  stage_blocks(bt, a.col);
  stage_kb<NV>(bt, a.m, a.col);
  stage_model(m, a.m);
  const earl_sawyer_cfg& cfg = a.cfg;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPE, grp = lane / LPE, n = cfg.n;
#ifdef EARL_PHYS_PROF
  const unsigned long long wave_t0 = __builtin_readcyclecounter();
#endif
  Shared<NV>& s = sh[wave * EPW + grp];
  if constexpr (Lim<NV>::TS < Lim<NV>::NT) {            // the mass-matrix entries between the two trees are never written (K5): zero, once
    for (int k = sub; k < (int)(sizeof(s.M.v) / sizeof(double)); k += LPE) s.M.v[k] = 0.0;
  }
  const Q4 mq = ldq(cfg.mocap_quat);                     // as given, NOT normalised (include/earl_physics.h)
  const int gcf = a.st.steps_since_goal_change ? cfg.goal_change_frequency : 0;
  const float scale = (float)cfg.action_scale;
  const int G = (n + EPW - 1) / EPW;                     // env groups (one per wave at a time)
  for (;;) {
  int group = blockIdx.x * WPB + wave, t_begin = 0, t_end = a.T;
  if constexpr (SLICED) {
    group = sched_claim(a.st.sched, G, a.T, lane, (int)(((blockIdx.x * WPB + wave) * 2) % G), t_begin);
    if (group < 0) break;
    t_end = t_begin + a.slice < a.T ? t_begin + a.slice : a.T;
  }
  const int env_raw = group * EPW + grp;
  const bool live = env_raw < n;
  const int env = live ? env_raw : n - 1;
  load_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
  if (sub < 3) s.mocap[sub] = a.st.mocap_pos[(size_t)env * 3 + sub];
  fence();
  int steps = a.st.steps_since_reset ? a.st.steps_since_reset[env] : 0;
  int sgc = gcf > 0 ? a.st.steps_since_goal_change[env] : 0;
  RSTART();
  for (int t = t_begin; t < t_end; ++t) {
    float4 act;
#if EARL_BRANCH_PRIOR
    // (sawyer_prior_rollout_kernel: a prior branch's action is the policy's on the row the branch carries, plus the planner's noise; it is stored where a plain branch loads it)
    if constexpr (BRANCH) act = sawyer_prior_step_action(t, env, sub, live);
#else
    if constexpr (BRANCH) act = sawyer_branch_action(t, env);      // (`env` is the virtual env v, `n` their number K n_env: see SawyerBranchArgs)
#endif
    else act = sawyer_step_action<POLICY>(a, t, n, env, sub, live);
    // set_xyz_action [UPSTREAM]: clip, float32 product with the scale, float64 add, box clip
    const float cx = fminf(fmaxf(act.x, -1.f), 1.f) * scale, cy = fminf(fmaxf(act.y, -1.f), 1.f) * scale, cz = fminf(fmaxf(act.z, -1.f), 1.f) * scale;
    if (sub < 3) {                                      // lane k moves coordinate k
      const float ck = sub == 0 ? cx : (sub == 1 ? cy : cz);
      s.mocap[sub] = fmin(fmax(s.mocap[sub] + (double)ck, cfg.mocap_low[sub]), cfg.mocap_high[sub]);
    }
    fence();
    const double ctrl[EARL_MAXACT] = {(double)act.w, -(double)act.w, 0, 0};
    RSTAMP(12);
    for (int ts = 0; ts < cfg.frame_skip; ++ts) {
      // The lane's index is passed through an empty asm at the head of every timestep: the per-lane LDS addresses derived from it are then recomputed
      // inside the timestep (a few integer adds) instead of being hoisted out of the rollout loop, where dozens of them lived across the whole kernel
      // and went to scratch memory under the register cap -- every reload is a global-memory round trip on the timestep's critical path (scratch per
      // lane: eight-wave door build 296 -> 212 B, peg 36 -> 0 B).  (Doing the same to the block pointer hides that it is an LDS address: 640 B.)
      // (Small model only: the peg build, with 512 registers, loses 2 % to the recomputation although its last 36 B of scratch go too.)
      int sub_ = sub, grp_ = grp;
      if constexpr (POLICY || (BRANCH && kBranchPrior)) {
        // (the policy phase is a call: what lives across it sits in the callee-saved registers or is spilled around it, and the allocator chose `sub` -- reloaded
        // here, at the head of every timestep.  The lane's index costs two instructions to read again and nothing to keep.)
        const int lane_ = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        sub_ = lane_ % LPE; grp_ = lane_ / LPE;
      }
      if constexpr (NV <= 10) asm volatile("" : "+v"(sub_));
      else asm volatile("" : "+v"(grp_));               // (peg: the block's base address was what got spilled, and reloaded six times per timestep)
      __builtin_assume(sub_ >= 0 && sub_ < LPE);
      __builtin_assume(grp_ >= 0 && grp_ < EPW);
      substep<NV, LPE, true>(sh[wave * EPW + grp_], m, bt, a.col, sub_, grp_, mq, ctrl, ts > 0, nullptr, nullptr);   // (every env step starts cold: step() x T == rollout(T))
    }
    RSTAMP(13);
    const size_t row = (size_t)t * n + env;
    // where this step's observation row goes: row t of out.obs, or -- POLICY, out.obs == NULL (earl_sawyer_population_rollout) -- the env's row of st.last_obs, the one
    // observation row such a launch keeps: emitted, re-emitted by the rollback (it then simply stays), patched by the goal switch and read by the policy of step t + 1,
    // lane `sub` reading what lane `sub` wrote; across a time slice it travels under sched_release / sched_claim like qpos
    // (POLICY only: the plain kernels keep their statements, and with them their machine code)
    [[maybe_unused]] double* obs_row = nullptr;
    [[maybe_unused]] bool carried = false;
    [[maybe_unused]] float rew = 0.f;               // what out.reward / out.success hold or would hold for this step, for the episode summary
    [[maybe_unused]] uint8_t suc = 0;
    if constexpr (POLICY) {
      carried = a.out.obs == nullptr;
      obs_row = carried ? a.st.last_obs + (size_t)env * 14 : a.out.obs + row * 14;
    }
    // BRANCH: the virtual env's row of SawyerBranchArgs.obs_row is the one row it keeps, carried as the population launch carries st.last_obs; obj_init is the env's own
    // row, i = v % n_env (worked out here, where it is used: nothing of it lives across the timesteps above)
    [[maybe_unused]] const double* br_obj_init = nullptr;
    if constexpr (BRANCH) {
      carried = true;
      obs_row = cl_kernarg<SawyerBranchArgs>()->obs_row + (size_t)env * 14;
      if (a.st.obj_init) br_obj_init = a.st.obj_init + (size_t)sawyer_branch_env(env) * 6;
    }
    // failure guard (MuJoCo's mj_checkPos / mj_checkVel; metaworld's `except MujocoException` in SawyerXYZEnv.step [UPSTREAM]): an env whose
    // state went NaN or beyond EARL_BAD_VALUE is rolled back to its last stable state (the rows in HBM) and re-emits its last stable
    // observation with reward 0; its neighbours in the wavefront never see it (a group only reads its own LDS block)
    const bool bad_lane = (sub < NV && !(fabs(s.qp[sub]) < EARL_BAD_VALUE && fabs(s.qv[sub]) < EARL_BAD_VALUE)) || (sub < 4 && !(fabs(s.bq[sub]) < 2.0));
    const bool failed = group_any<LPE>(bad_lane, grp);
    if constexpr (BRANCH)
      sawyer_emit<NV>(s, m, cfg, sub, live && !failed, a.st.goal + (size_t)env * 7, obs_row, &rew, &suc, br_obj_init, (double)act.w, nullptr, nullptr);
    else if constexpr (POLICY)
      sawyer_emit<NV>(s, m, cfg, sub, live && !failed, a.st.goal + (size_t)env * 7, obs_row, &rew, &suc, a.st.obj_init ? a.st.obj_init + (size_t)env * 6 : nullptr,
                      (double)act.w, nullptr, (NV >= 15 && a.out.info) ? a.out.info + row * EARL_SAWYER_INFO : nullptr);
    else
    sawyer_emit<NV>(s, m, cfg, sub, live && !failed, a.st.goal + (size_t)env * 7, a.out.obs + row * 14, a.out.reward ? a.out.reward + row : nullptr,
                    a.out.success ? a.out.success + row : nullptr, a.st.obj_init ? a.st.obj_init + (size_t)env * 6 : nullptr, (double)act.w, nullptr,
                    (NV >= 15 && a.out.info) ? a.out.info + row * EARL_SAWYER_INFO : nullptr);
    RSTAMP(14);
    if (!BRANCH && sub == 0 && live && a.out.status) a.out.status[row] = failed ? EARL_STEP_DIVERGED : 0;      // (BRANCH: no [T] row of any kind; `!BRANCH && ...` folds away like `POLICY && ...` below)
    if (!failed) {
      // this state is the env's last stable one from here on
      if (live) {
        store_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
        if (sub < 3) a.st.mocap_pos[(size_t)env * 3 + sub] = s.mocap[sub];
      }
      if constexpr (NV >= 15) {
        // the free body's orientation as load_state would read it back from the row just stored (re-normalised, the same expression): a rollout, its
        // time slices taken by different waves, and T single-step launches then walk through the same bits (like the minitaur kernel)
        if (m.ball_dof >= 0) {
          const double qn = renormalised_quat_entry<NV>(s, sub);
          fence();
          if (sub < 4) s.bq[sub] = qn;
          fence();
        }
      }
    } else {
      load_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
      if (sub < 3) s.mocap[sub] = a.st.mocap_pos[(size_t)env * 3 + sub];
      if (live) {
        if constexpr (BRANCH) {
          // (the carried row IS the last stable observation -- before the first stable step the env's row of st->last_obs, which the replicate kernel put there;
          // reward 0, success 0 and the count of such steps are written with the summary below; the env's fail_count is not a branch's to touch)
        } else if constexpr (POLICY) {
          if (!carried) {        // (a carried row IS the last stable observation already; reward 0 and success 0 are written with the summary below)
            const double* prev = t > 0 ? a.out.obs + ((size_t)(t - 1) * n + env) * 14 : (a.st.last_obs ? a.st.last_obs + (size_t)env * 14 : nullptr);
            if (sub < 14) a.out.obs[row * 14 + sub] = prev ? prev[sub] : __builtin_nan("");
          }
          if (sub == 0 && a.st.fail_count) a.st.fail_count[env] += 1;
        } else {
        const double* prev = t > 0 ? a.out.obs + ((size_t)(t - 1) * n + env) * 14 : (a.st.last_obs ? a.st.last_obs + (size_t)env * 14 : nullptr);
        if (sub < 14) a.out.obs[row * 14 + sub] = prev ? prev[sub] : __builtin_nan("");
        if (sub == 0) {
          if (a.out.reward) a.out.reward[row] = 0.f;
          if (a.out.success) a.out.success[row] = 0;
          if (a.st.fail_count) a.st.fail_count[env] += 1;
        }
        }
        if (!BRANCH && NV >= 15 && a.out.info && sub < EARL_SAWYER_INFO) a.out.info[row * EARL_SAWYER_INFO + sub] = 0.0;
      }
    }
    if constexpr (BRANCH) {
      // reward and success of the step as a rollout would have stored them (a rolled-back step: 0 and 0) into the virtual env's summary, in device memory after every
      // env step like the population launch's: a time slice another wave takes finds the words under sched_release / sched_claim
      // (kBranchDiscount -- the units built with EARL_BRANCH_DISCOUNT --: the sum is the discounted one, d_t beside it in the workspace)
      if (sub == 0 && live) sawyer_branch_summary<kBranchDiscount>(t, env, (double)(failed ? 0.f : rew), failed ? (uint8_t)0 : suc, failed);
    }
    if constexpr (POLICY) {
      // reward and success of the step (a rolled-back step: 0 and 0) to their rows, and into the env's episode summary: each word is its definition applied to exactly
      // these values.  The summary pointers are read through the kernel-argument segment here, where they are used (see sawyer_policy_action on why).
      if (sub == 0 && live) {
        const float r_t = failed ? 0.f : rew;
        const uint8_t s_t = failed ? (uint8_t)0 : suc;
        if (a.out.reward) a.out.reward[row] = r_t;
        if (a.out.success) a.out.success[row] = s_t;
        cl_episode_summary(cl_kernarg<SawyerPolicyArgs>(), t, env, (double)r_t, s_t);
      }
    }
    fence();
    ++steps;
    RSTAMP(15);
    if (!BRANCH && sub == 0 && live && a.out.done) a.out.done[row] =(cfg.horizon > 0 && steps >= cfg.horizon) ? 1 : 0;
    // door with goal switching: slot 7 of EVERY row's info block is this kernel's to write -- 0, or 1 on a goal-switch row (below) -- so that earl_sawyer_door_info never reads
    // a marker the caller left behind (ADVICE r05: the Python side used to zero the column with a launch of its own before every call)
    if (!BRANCH && NV < 15 && gcf > 0 && a.out.info && sub == 11 && live) a.out.info[row * EARL_SAWYER_INFO + 7] = 0.0;
    // does this step end with a new goal row?  The lifelong switch's clock, or -- POLICY, earl_sawyer_agents_rollout -- a handover of the agent pair that changes the goal:
    // `fixed` is then the table of `fixed_rows` backward goals to draw from (entering the reset phase; earl_sawyer_pair_rollout's ONE row is the table of one row) or NULL
    // (entering the forward phase: the lifelong switch's own draw from cfg.goal_table)
    // (the plain kernels: `POLICY && ...` folds away in the front end, and their statements -- and machine code -- are what they were)
    [[maybe_unused]] bool pair_sw = false;
    [[maybe_unused]] const double* fixed = nullptr;
    [[maybe_unused]] int fixed_rows = 0;
    [[maybe_unused]] int32_t* row_of = nullptr;          // earl_backward_goals.row / row_out: where lane 7 of the env leaves the drawn row
    [[maybe_unused]] int32_t* row_at = nullptr;
    [[maybe_unused]] bool pair_on = false;
    if constexpr (POLICY) {
      // The pair's state machine (include/earl_physics.h, item 5), worked out by all 16 lanes of the env from the same words: the step's success flag from lane 0, phase
      // and steps_in_phase from HBM, where lane 0 stores them again -- nothing of it lives across substep.  The pointers are read through the kernel-argument segment
      // here, where they are used (see sawyer_policy_action on why).
      const EARL_KARG SawyerPolicyArgs* ka = cl_kernarg<SawyerPolicyArgs>();
      int8_t* const pair_phase = ka->pair_phase;
      if (pair_phase) {                                  // (wave-uniform)
        pair_on = true;
        int ph, sip;
        if (cl_pair_decide(ka, t, env, sub == 0 && live, __shfl((int)((!failed && suc) ? 1 : 0), 0, 16) != 0, ph, sip)) {
          // (the draw itself is the lifelong switch's ONE Philox call below, by direction: the shared handover's would be a second one in this body)
          if (ph) { fixed = ka->pair_goal; fixed_rows = ka->pair_goal_rows; row_of = ka->pair_row; pair_sw = fixed != nullptr; }      // entering the reset phase: a row of the backward table, if there is one
          else pair_sw = cfg.n_goal_rows > 0;                                   // entering the forward phase: the lifelong switch's draw for this step
        }
        if (sub == 0 && live) { pair_phase[env] = (int8_t)ph; ka->pair_sip[env] = sip; }
        // row_out: -1 at every step of a live env, overwritten below by the same lane on a step that draws (like slot 7 of the door's info block above)
        row_at = ka->pair_row_out;
        if (row_at && sub == 7 && live) row_at[row] = -1;
      }
    }
    if ((gcf > 0 && ++sgc >= gcf) || (POLICY && pair_sw)) {
      // LifelongWrapper.step (lifelong_wrapper.py:36-42): reset_goal() -> get_next_goal(), then the observation is re-read with the new
      // goal (same simulator state: only the goal block changes); the reward above used the old goal
      sgc = 0;
      if (((POLICY && fixed) || (cfg.n_goal_rows > 0 && cfg.goal_table)) && sub >= 7 && sub < 14 && live) {      // the lanes that wrote the goal block of this row
        // the host's step counter plus the clock word of a graph-captured launch (earl_sawyer_rollout_clocked), read here -- a goal-switch step -- and not at kernel
        // entry: a value held across the rollout loop costs the time-sliced peg build 32 B of scratch per lane and the 64-lane door build two AGPRs
        const uint64_t ev = cfg.step_counter + (a.clock ? a.clock[1] : 0) + (uint64_t)t;
        // ONE draw, by direction: the lifelong switch's (index 0xFFFE, cfg.goal_table) or -- POLICY, entering the reset phase -- the backward table's (index 0xFFFD, free:
        // the reset draws with 0 .. 31, 0xFFF0 .. 0xFFF2 and 0xFFFF, the head with 0x504F4C00); the same counter words, u01 and clamp
        const uint32_t draw = (POLICY && fixed) ? 0xFFFDu : 0xFFFEu;
        const int rows = (POLICY && fixed) ? fixed_rows : cfg.n_goal_rows;
        const double* const table = (POLICY && fixed) ? fixed : cfg.goal_table;
        // (BRANCH: the id is the ENV's, cfg.env_offset + v % n_env, never the virtual index: every branch of an env sees the draw the env's next rollout will see)
        int gid_env = env;
        if constexpr (BRANCH) gid_env = sawyer_branch_env(env);
        const earl::U4 b = earl::philox4x32_10(earl::U4{draw, (uint32_t)(cfg.env_offset + gid_env), (uint32_t)ev, (uint32_t)(ev >> 32)},
                                               (uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
        int grow = (int)(earl::u01(b.x, b.y) * (double)rows);
        grow = grow < rows ? grow : rows - 1;
        const double gv = table[(size_t)grow * 7 + (sub - 7)];
        if constexpr (POLICY) {
          if (fixed && sub == 7) {
            if (row_of) row_of[env] = grow;
            if (row_at) row_at[row] = grow;
          }
        }
        if (!BRANCH && NV < 15 && a.out.info && sub >= 11) {
          // the door's info dict is worked out after the launch from the emitted rows (earl_sawyer_door_info), whose goal block is about to change: this
          // row's info slots 0-2 carry the target the row's reward was computed with, slot 7 marks it (evaluate_state runs before reset_goal:
          // lifelong_wrapper.py:30-44; include/earl_physics.h)
          a.out.info[row * EARL_SAWYER_INFO + (sub - 11)] = a.st.goal[(size_t)env * 7 + (sub - 7)];
          if (sub == 11) a.out.info[row * EARL_SAWYER_INFO + 7] = 1.0;
        }
        a.st.goal[(size_t)env * 7 + (sub - 7)] = gv;
        if constexpr (POLICY || BRANCH) obs_row[sub] = gv;
        else a.out.obs[row * 14 + sub] = gv;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");      // the next step's observation reads the goal row back through global memory
    } else if constexpr (POLICY) {
      if (pair_on) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");      // (the same fence for the phase words: all 16 lanes read what lane 0 stored)
    }
  }
  if (live) {
    // (qpos / qvel / mocap_pos were written back after the last stable step)
    if constexpr (BRANCH) {      // (the carried row is in place; st.last_obs and st.steps_since_reset are NULL here, the goal-switch counter below is the workspace's)
    } else if constexpr (POLICY) {      // (a carried row is in place)
      if (t_end == a.T && a.st.last_obs && a.out.obs && a.T > 0 && sub < 14) a.st.last_obs[(size_t)env * 14 + sub] = a.out.obs[((size_t)(a.T - 1) * n + env) * 14 + sub];
    } else
    if (t_end == a.T && a.st.last_obs && a.T > 0 && sub < 14) a.st.last_obs[(size_t)env * 14 + sub] = a.out.obs[((size_t)(a.T - 1) * n + env) * 14 + sub];
    if (sub == 0 && a.st.steps_since_reset) a.st.steps_since_reset[env] = steps;
    if (sub == 0 && gcf > 0) a.st.steps_since_goal_change[env] = sgc;
  }
  if constexpr (SLICED) sched_release(a.st.sched, G, group, t_end, lane);
  else break;
  }
#ifdef EARL_PHYS_PROF
  if (lane == 0 && blockIdx.x * WPB + wave < 4096) g_wave_cycles[blockIdx.x * WPB + wave] = __builtin_readcyclecounter() - wave_t0;
#endif
