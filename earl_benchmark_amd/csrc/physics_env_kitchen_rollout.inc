// the body of kitchen_rollout_kernel<DUO> and of kitchen_policy_rollout_kernel<DUO> (physics_env_kitchen.h): `a` is the kernel's argument, a KitchenRolloutArgs or a KitchenPolicyArgs
#pragma clang fp contract(off)
  constexpr bool POLICY = std::is_same<decltype(a), const KitchenPolicyArgs>::value;
  constexpr int NV = 23, LPE = 32, EPW = 64 / LPE, WPB = Lim<NV>::WPB;
  __shared__ alignas(16) typename ModelOf<NV>::T m;
  __shared__ alignas(16) BlkTable<Lim<NV>::MB, Lim<NV>::KBT> bt;
  __shared__ alignas(16) Shared<NV> sh[EPW * WPB];
  __shared__ earl_kitchen_params kp;
  stage_blocks(bt, a.col);
  stage_kb<NV>(bt, a.m, a.col);
  if (threadIdx.x == 0) kp = a.p;
  stage_model(m, a.m);                                  // (ends with the workgroup barrier)
  const earl_kitchen_cfg& cfg = a.cfg;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPE, grp = lane / LPE, n = cfg.n;
  if (a.solo >= 2 && DUO == 0 && wave > 0) return;          // (after stage_model's barrier; the DUO form keeps all four waves: its later barriers count them)
  const bool role_a = DUO == 1 ? wave >= 1 : (DUO == 2 && (wave & 1));      // the helper waves: compute, store nothing outside LDS
  const int env_raw = a.solo >= 2 ? (DUO == 2 ? (int)(blockIdx.x * 2 + (wave >> 1)) : (int)blockIdx.x) : (a.solo == 1 ? (int)(blockIdx.x * WPB + wave) : (int)((blockIdx.x * WPB + wave) * EPW + grp));
  const bool live = env_raw < n && (a.solo == 0 || grp == 0) && !role_a;
  const int env = env_raw < n ? env_raw : n - 1;
  Shared<NV>& s = sh[wave * EPW + grp];
  Shared<NV>* const peer = DUO == 1 ? &sh[grp] : (DUO == 2 ? &sh[(wave ^ 1) * EPW + grp] : nullptr);      // helpers: the owner's block of the same 32-lane group; owners: their helper's (wave 1 of the four-wave form)
  load_state<NV>(s, m, a.st.qpos + (size_t)env * NV, a.st.qvel + (size_t)env * NV, sub);
  for (int k = sub; k < (int)(sizeof(s.M.v) / sizeof(double)); k += LPE) s.M.v[k] = 0.0;      // (entries between different trees are never written, K5)
  for (int k = sub; k < (int)(sizeof(s.hwst.Hw.v) / sizeof(double)); k += LPE) s.hwst.Hw.v[k] = 0.0;   // (nor the structural zeros of the equality Hessian, K9)
  if (sub < 3) s.mocap[sub] = a.st.mocap_pos[(size_t)env * 3 + sub];
  fence();
  const Q4 mq = ldq(cfg.mocap_quat_dev);
  if constexpr (DUO != 0) {
    __syncthreads();                                    // wave 0's mass matrix is zeroed before wave 1 writes into it
    if (role_a) {
      for (int t = 0; t < a.T; ++t) {
        __syncthreads();                                // barrier 0: wave 0 is through the env step's bookkeeping (a diverged env went back to its stored state); the step's targets are published
        const double ctrl_a[EARL_MAXACT] = {peer->duo_ctrl[0], peer->duo_ctrl[1], 0, 0};
        for (int ts = 0; ts < cfg.frame_skip; ++ts) {
          if (sub < NV) { s.qp[sub] = peer->qp[sub]; s.qv[sub] = peer->qv[sub]; }
          fence();
          if constexpr (DUO == 2) substep<NV, LPE, true, 5>(s, m, bt, a.col, sub, grp, mq, ctrl_a, false, nullptr, nullptr, peer);      // (barriers X, Y, Z inside)
          else if (wave == 1) substep<NV, LPE, true, 1>(s, m, bt, a.col, sub, grp, mq, ctrl_a, false, nullptr, nullptr, peer);
          else if (wave == 2) substep<NV, LPE, true, 3>(s, m, bt, a.col, sub, grp, mq, ctrl_a, false, nullptr, nullptr, peer);
          else substep<NV, LPE, true, 4>(s, m, bt, a.col, sub, grp, mq, ctrl_a, false, nullptr, nullptr, peer);
          __syncthreads();                              // barrier 2: wave 0 has integrated
        }
      }
      return;
    }
  }
  int steps = a.st.steps_since_reset[env];
  const int kk = sub < 9 ? sub : 8;                     // this lane's action component
#ifdef EARL_PHYS_PROF
  const unsigned long long wave_t0 = __builtin_readcyclecounter();
#endif
  for (int t = 0; t < a.T; ++t) {
    const size_t row = (size_t)t * n + env;
    // ---- KitchenV0.step up to do_simulation (kitchen_action_kernel): mocap target, the nine position targets
    const double mocap_prev = s.mocap[sub < 3 ? sub : 0];      // the target before this step's action: a diverged step goes back to it
    {
      double x;
      if constexpr (POLICY) x = kit_policy_step(a, t, n, env, sub, grp, kk, live);      // computed here by the env's lanes; the owner wave of the several-wave forms: before barrier 0
      else x = (double)a.action[row * 9 + kk];
      const double c = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
      const double ak = kp.act_mid[kk] + c * kp.act_amp[kk];
      if (sub < 3) {
        const double y = s.mocap[sub] + ak * kp.mocap_range[sub];
        s.mocap[sub] = y < kp.mocap_clip_lower[sub] ? kp.mocap_clip_lower[sub] : (y > kp.mocap_clip_upper[sub] ? kp.mocap_clip_upper[sub] : y);
      }
      if (sub < 9) {
        const double v = ak < kp.vel_bound[sub][0] ? kp.vel_bound[sub][0] : (ak > kp.vel_bound[sub][1] ? kp.vel_bound[sub][1] : ak);
        const double y = a.st.last_qp_robot[(size_t)env * 9 + sub] + v * kp.step_duration;
        s.kit.targets[sub] = y < kp.pos_bound[sub][0] ? kp.pos_bound[sub][0] : (y > kp.pos_bound[sub][1] ? kp.pos_bound[sub][1] : y);
      }
    }
    fence();
    const double ctrl[EARL_MAXACT] = {s.kit.targets[0], s.kit.targets[1], 0, 0};      // do_simulation: ctrl[i] = targets[i] for i < nu = 2
    if (sub < 3 && live) a.st.mocap_pos[(size_t)env * 3 + sub] = s.mocap[sub];
    fence();
    if constexpr (DUO != 0) {
      if (sub < 2) s.duo_ctrl[sub] = ctrl[sub];
      __syncthreads();                                  // barrier 0
      for (int ts = 0; ts < cfg.frame_skip; ++ts) {
        if constexpr (DUO == 2) substep<NV, LPE, true, 6>(s, m, bt, a.col, sub, grp, mq, ctrl, ts > 0, nullptr, nullptr, peer);     // (barriers X, Y, Z inside; `peer`: its helper's block, where that leaves K10's factor)
        else substep<NV, LPE, true, 2>(s, m, bt, a.col, sub, grp, mq, ctrl, ts > 0, nullptr, nullptr, &sh[EPW + grp]);
        __syncthreads();                                // barrier 2
      }
    } else
    for (int ts = 0; ts < cfg.frame_skip; ++ts) substep<NV, LPE, true>(s, m, bt, a.col, sub, grp, mq, ctrl, ts > 0, nullptr, nullptr);
    const bool bad_lane = sub < NV && !(fabs(s.qp[sub]) < EARL_BAD_VALUE && fabs(s.qv[sub]) < EARL_BAD_VALUE);
    const bool failed = group_any<LPE>(bad_lane, grp);
    [[maybe_unused]] double rew = 0.0;                // POLICY: what out.reward / out.success hold or would hold for this step, for the episode summary
    [[maybe_unused]] uint8_t suc = 0;
    if (failed) {
      // rolled back to the last stable state (the rows in HBM); returns its last stable observation, reward 0 (kitchen_guard / finish kernels)
      load_state<NV>(s, m, a.st.qpos + (size_t)env * NV, a.st.qvel + (size_t)env * NV, sub);
      if (sub < 3) {                                      // ... incl. the mocap target that pulled it there (att_xpos keeps the last stable positions)
        s.mocap[sub] = mocap_prev;
        if (live) a.st.mocap_pos[(size_t)env * 3 + sub] = mocap_prev;
      }
      if constexpr (POLICY) {
        // (POLICY only: the plain kernels keep their statements, and with them their machine code.  Without out.obs nothing is re-emitted: the env's row of st.last_obs
        // stands; reward 0 and success 0 go out with the summary below)
        if (live) {
          if (a.out.obs) for (int k = sub; k < 46; k += LPE) a.out.obs[row * 46 + k] = a.st.last_obs[(size_t)env * 46 + k];
          if (sub == 0 && a.st.fail_count) a.st.fail_count[env] += 1;
        }
      } else
      if (live) {
        for (int k = sub; k < 46; k += LPE) a.out.obs[row * 46 + k] = a.st.last_obs[(size_t)env * 46 + k];
        if (sub == 0) {
          a.out.reward[row] = 0.0; a.out.success[row] = 0;
          if (a.st.fail_count) a.st.fail_count[env] += 1;
        }
      }
    } else {
      if (live) store_state<NV>(s, m, a.st.qpos + (size_t)env * NV, a.st.qvel + (size_t)env * NV, sub);
      // attachments at the kinematics of the last timestep's start (written only for a step that ended finite); the eight task sites for the reward
      if (sub < m.n_att && live) {
        const V3 p = attachment<NV>(s, m, sub);
        double* o = a.st.att_xpos + ((size_t)env * m.n_att + sub) * 3;
        o[0] = p.x; o[1] = p.y; o[2] = p.z;
      }
      if (sub < 8) {
        const V3 p = attachment<NV>(s, m, cfg.site_att[sub]);
        s.kit.sites[sub][0] = p.x; s.kit.sites[sub][1] = p.y; s.kit.sites[sub][2] = p.z;
      }
      // Robot.get_obs + KitchenV0._get_obs: 46 draws of U(-1, 1) per env (uniform_kernel: one Philox block = two draws), then kitchen_obs_kernel
      if (cfg.sensor_noise && sub < 23) {
        const uint64_t ctr = cfg.counter + (a.clock ? a.clock[0] : 0) + (uint64_t)t;      // + the clock word of a graph-captured launch (earl_kitchen_rollout_clocked)
        const earl::U4 b = earl::philox4x32_10(earl::U4{0x4B00u + (uint32_t)sub, (uint32_t)(cfg.env_offset + env), (uint32_t)ctr, (uint32_t)(ctr >> 32)},
                                               (uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
        const double lo = -1.0, hi = 1.0;
        s.kit.noise[2 * sub] = lo + (hi - lo) * earl::u01(b.x, b.y);
        s.kit.noise[2 * sub + 1] = lo + (hi - lo) * earl::u01(b.z, b.w);
      }
      fence();
      for (int k = sub; k < 46; k += LPE) {
        double v;
        if (k < 23) {
          v = s.qp[k];
          if (cfg.sensor_noise) v = v + (kp.robot_noise_ratio * kp.pos_noise_amp[k]) * s.kit.noise[k < 9 ? k : k + 9];
        } else {
          v = a.st.goal[(size_t)env * 23 + (k - 23)];
        }
        s.kit.obs[k] = v;
        if (live) {
          if constexpr (POLICY) { if (a.out.obs) a.out.obs[row * 46 + k] = v; }
          else a.out.obs[row * 46 + k] = v;
          a.st.last_obs[(size_t)env * 46 + k] = v;
          if (k < 9) a.st.last_qp_robot[(size_t)env * 9 + k] = v;
        }
      }
      fence();
      if (sub == 0 && live) {                           // kitchen.py:141-183 (kitchen_reward_kernel)
        const double* o = s.kit.obs;
        const double dist = kit_norm_diff(o + 9, o + 32, 14);
        double r = -10 * dist;
        const int start[8] = {9, 11, 13, 15, 17, 19, 20, 22}, len[8] = {2, 2, 2, 2, 2, 1, 2, 1};
        bool reaching = false;
        for (int c = 0; c < 8; ++c) {
          if (kit_norm_diff(o + start[c], o + start[c] + 23, len[c]) < len[c] * 0.01) r += 1;
          else if (!reaching) {
            reaching = true;
            r += -0.5 * kit_norm_diff(s.mocap, s.kit.sites[c], 3);
          }
        }
        if constexpr (POLICY) { rew = r; suc = dist <= 0.3; }      // (stored after the branch, with the summary)
        else {
        a.out.reward[row] = r;
        a.out.success[row] = dist <= 0.3;
        }
      }
    }
    ++steps;
    if constexpr (POLICY) {
      // reward and success of the step (a rolled-back step: 0 and 0) to their rows, each NULL or given, and into the env's episode summary: each word is its definition
      // applied to exactly these values.  Lane 0 of the env's OWNER wave (`live` excludes the helper waves, which left for their own loop above).  The summary pointers are
      // read through the kernel-argument segment here, where they are used (see kitchen_policy_action on why)
      if (sub == 0 && live) {
        const double r_t = failed ? 0.0 : rew;
        const uint8_t s_t = failed ? (uint8_t)0 : suc;
        if (a.out.reward) a.out.reward[row] = r_t;
        if (a.out.success) a.out.success[row] = s_t;
        cl_episode_summary(cl_kernarg<KitchenPolicyArgs>(), t, env, r_t, s_t);
        if (a.out.status) a.out.status[row] = failed ? EARL_STEP_DIVERGED : 0;
        if (a.out.done) a.out.done[row] = (cfg.horizon > 0 && steps >= cfg.horizon) ? 1 : 0;
      }
    } else
    if (sub == 0 && live) {
      if (a.out.status) a.out.status[row] = failed ? EARL_STEP_DIVERGED : 0;
      a.out.done[row] = (cfg.horizon > 0 && steps >= cfg.horizon) ? 1 : 0;
    }
    if constexpr (POLICY) kit_pair_handover(a, t, env, row, sub, grp, live, failed, suc);      // earl_kitchen_agents_rollout: the pair's state machine and its goal rows (the owner wave)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");    // the next step reads last_qp_robot (and, after a failure, the state rows) back through global memory
    fence();
  }
#ifdef EARL_PHYS_PROF
  if (lane == 0 && blockIdx.x * WPB + wave < 4096) g_wave_cycles[blockIdx.x * WPB + wave] = __builtin_readcyclecounter() - wave_t0;
#endif
  if (sub == 0 && live) a.st.steps_since_reset[env] = steps;
