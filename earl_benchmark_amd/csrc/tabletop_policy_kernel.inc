// tabletop_policy_kernel.inc -- the BODY of the closed-loop policy kernel, included by tabletop_policy.h into its two __global__ templates (policy_rollout_kernel:
// POP = false; policy_population_kernel: POP = true) and by tabletop3_policy.hip into its one (POP = true, NOBJ = 3).  In scope: the template parameters NT2, GENERAL, GAUSS, a constexpr bool POP, a constexpr
// int NOBJ (1, or 3: the three-object env -- Lane<3>, 20 observations, five k-steps of layer 0, the LDS images after the observation's moved up), and the kernel argument `a`.
// It is text, not a function: routed through a __forceinline__ function the single-policy kernels compile to different register allocations
// (profiles/policy_kernel_resources.txt), and their twenty instantiations are to stay exactly what they were.
// TWIN: tabletop_pair_kernel.h restates this step body (layer 0, hidden layer, output chain, head, fence) per agent, once for both envs; the pair's actions are held bit
// for bit to this chain, so a change to the arithmetic or its order here is mirrored there by hand (tests/test_policy_pair.py and tests/test_tabletop3_pair.py, test 1, compare the two).
  constexpr int NOBS = Dims<NOBJ>::NOBS, KS0 = NOBS / 4;               // layer 0's K and its k-steps (12: 3, 20: 5; no padding)
  constexpr int XS = kPolicyEnvsPerWg * (NOBS - 12);                   // floats by which the wider observation image moves everything behind it
  constexpr int NOUT = GAUSS ? 6 : 3, ACTW = GAUSS ? 8 : 4, WO_OFF = (GAUSS ? kPolWoG : kPolWo) + XS;
  // three objects beside a 256-wide second hidden layer (NT2 = 4): Lane<3>, g[10] and o[20] do not fit next to w1's 256 registers and layer 0's 24, so layer 0's
  // B operand and bias live in LDS as well, in the order a lane reads them: [n][q][s] = W0[n][4 s + q], then b0[n] (21 KB of the workgroup's 160)
  constexpr bool W0_LDS = NOBJ == 3 && NT2 == 4;
  constexpr int W0_OFF = (GAUSS ? kPolLdsG : kPolLds) + XS;
  __shared__ __attribute__((aligned(16))) float lds[W0_OFF + (W0_LDS ? kPolicyMaxWidth * (NOBS + 1) : 0)];
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int H1 = a.p.dims[1], HL = a.p.dims[a.p.n_layers - 1], H2 = NT2 > 0 ? a.p.dims[2] : 0;
  // POP: the first local env index of this workgroup (may be negative in workgroup 0), and its member's parameters
  int base = (int)blockIdx.x * kPolicyEnvsPerWg;
  const float* params = a.p.params;
  if constexpr (POP) {
    base -= a.k.cfg.env_offset & (kPolicyEnvsPerWg - 1);
    params += population_param_offset(a.pop, a.k.cfg.env_offset + base);
  }
  const float* __restrict__ W0 = params;
  const float* __restrict__ B0 = W0 + H1 * NOBS;
  const float* __restrict__ W1 = B0 + H1;
  const float* __restrict__ B1 = W1 + H2 * H1;
  const float* __restrict__ WO = NT2 > 0 ? B1 + H2 : W1;
  const float* __restrict__ BO = WO + NOUT * HL;

  // ---- prologue: weights into registers, once
  const int nt0 = (H1 / 16 - wave + 3) >> 2;                          // this wave's N-tiles of layer 0: tl = wave + 4 j, j < nt0
  float w0[W0_LDS ? 1 : 4][KS0], b0[W0_LDS ? 1 : 4];
  if constexpr (W0_LDS) {
    for (int k = (int)threadIdx.x; k < H1 * NOBS; k += 256) {
      const int n = k / NOBS, kk = k - n * NOBS;
      lds[W0_OFF + (n * 4 + (kk & 3)) * KS0 + (kk >> 2)] = W0[k];
    }
    for (int n = (int)threadIdx.x; n < H1; n += 256) lds[W0_OFF + H1 * NOBS + n] = B0[n];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = (wave + 4 * j) * 16 + c;
      const bool ok = j < nt0;
#pragma unroll
      for (int s = 0; s < KS0; ++s) w0[j][s] = ok ? W0[n * NOBS + 4 * s + q] : 0.0f;
      b0[j] = ok ? B0[n] : 0.0f;
    }
  }
  constexpr int NT2A = NT2 > 0 ? NT2 : 1;
  const int nt1 = NT2 > 0 ? (H2 / 16 - wave + 3) >> 2 : 0;
  float w1[NT2A][64], b1[NT2A];
  if constexpr (NT2 > 0) {
#pragma unroll
    for (int j = 0; j < NT2; ++j) {
      const int n = (wave + 4 * j) * 16 + c;
      const bool ok = j < nt1;
#pragma unroll
      for (int s = 0; s < 64; ++s) w1[j][s] = (ok && 4 * s < H1) ? W1[n * H1 + 4 * s + q] : 0.0f;
      b1[j] = ok ? B1[n] : 0.0f;
    }
  }
  // the output layer's B operand: registers too, except beside a 256-wide second hidden layer (NT2 = 4), whose 256 weight registers per lane leave no
  // room for 64 more -- there it stays in LDS in the order a lane reads it (3 KB, one 16-byte read per four k-steps, independent of the MFMA chain)
  // three objects, one hidden layer (NT2 = 0): there too, so that the kernel keeps its single-object twin's two waves per SIMD (256 registers) with Lane<3> and o[20]
  constexpr bool WO_LDS = (GAUSS ? NT2 >= 3 : NT2 == 4) || (NOBJ == 3 && NT2 == 0);      // (the Gaussian head's own registers: from NT2 = 3 on)
  float wo[WO_LDS ? 1 : 64], bo;
  if constexpr (WO_LDS) {
    for (int k = (int)threadIdx.x; k < NOUT * HL; k += 256) {
      const int j = k / HL, kk = k - j * HL;
      lds[WO_OFF + (j * 4 + (kk & 3)) * (HL >> 2) + (kk >> 2)] = WO[k];
    }
    wo[0] = 0.0f;
  } else {
#pragma unroll
    for (int s = 0; s < 64; ++s) wo[s] = (wave == 0 && c < NOUT && 4 * s < HL) ? WO[c * HL + 4 * s + q] : 0.0f;
  }
  bo = c < NOUT ? BO[c] : 0.0f;

  // ---- env lanes
  const int i = POP ? base + (int)threadIdx.x : blockIdx.x * kPolicyEnvsPerWg + (int)threadIdx.x;
  const bool env_lane = threadIdx.x < kPolicyEnvsPerWg && i < a.k.cfg.n && (!POP || i >= 0);
  Lane<NOBJ> L;
  float g[Dims<NOBJ>::NG], o[NOBS];
#pragma unroll
  for (int k = 0; k < NOBS; ++k) o[k] = 0.0f;
  if (env_lane) {
    load_lane<NOBJ>(a.k, i, L);
    load_goal<NOBJ>(a.k.st.goal_table, L.goal_idx, g);
  }
  float* const X = lds + kPolX;
  float* const A1 = lds + kPolH1 + XS;
  float* const A2 = lds + kPolH2 + XS;
  float* const AL = NT2 > 0 ? A2 : A1;
  float* const ACT = lds + kPolAct + XS;
  [[maybe_unused]] float* const EPS = lds + kPolEpsG + XS;

#ifdef EARL_POLICY_STAMPS
  unsigned long long prof[6] = {0, 0, 0, 0, 0, 0}, last_ = 0;
#endif
  for (int e = 0; e < a.episodes; ++e) {
    if (env_lane) policy_episode_begin<GENERAL>(a, i, e, L, g, o);
    [[maybe_unused]] EpisodeSum es;
    if constexpr (POP) episode_sum_begin(es);
#ifdef EARL_POLICY_STAMPS
    last_ = pol_clock();
#endif
    for (int t = 0; t < a.k.T; ++t) {
      if (threadIdx.x < kPolicyEnvsPerWg) {                           // (rows of a ragged last workgroup: zeros, results never read)
#pragma unroll
        for (int k = 0; k < NOBS; ++k) X[pol_idx((int)threadIdx.x, k, NOBS)] = o[k];
      }
      __syncthreads();
      POL_STAMP(0);
      // ---- layer 0: NOBS -> H1
      {
        float xa[KS0];
#pragma unroll
        for (int s = 0; s < KS0; ++s) xa[s] = X[c * NOBS + q * KS0 + s];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nt0) {
            const int n = (wave + 4 * j) * 16 + c;
            f32x4 acc;
            if constexpr (W0_LDS) {
              const float bj = lds[W0_OFF + H1 * NOBS + n];
              acc = f32x4{bj, bj, bj, bj};
#pragma unroll
              for (int s = 0; s < KS0; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], lds[W0_OFF + (n * 4 + q) * KS0 + s], acc, 0, 0, 0);
            } else {
              acc = f32x4{b0[j], b0[j], b0[j], b0[j]};
#pragma unroll
              for (int s = 0; s < KS0; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], w0[j][s], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) A1[pol_idx(q * 4 + r, n, H1)] = policy_act(acc[r], a.p.hidden_act);
          }
        }
      }
      __syncthreads();
      POL_STAMP(1);
      // ---- hidden layer: H1 -> H2
      if constexpr (NT2 > 0) {
        f32x4 acc[NT2];
#pragma unroll
        for (int j = 0; j < NT2; ++j) acc[j] = f32x4{b1[j], b1[j], b1[j], b1[j]};
        if (nt1 > 0) {
          const float* arow = A1 + c * H1 + q * (H1 >> 2);
#pragma unroll
          for (int s4 = 0; s4 < 16; ++s4) {
            if (s4 * 16 < H1) {
              const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
#pragma unroll
              for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int j = 0; j < NT2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], w1[j][4 * s4 + s], acc[j], 0, 0, 0);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < NT2; ++j) {
            if (j < nt1) {
              const int n = (wave + 4 * j) * 16 + c;
#pragma unroll
              for (int r = 0; r < 4; ++r) A2[pol_idx(q * 4 + r, n, H2)] = policy_act(acc[j][r], a.p.hidden_act);
            }
          }
        }
        __syncthreads();
      }
      POL_STAMP(2);
      if constexpr (GAUSS) {
        // ---- the step's draws on wave 1, beside the output layer: lane = (env, dimension)
        if (wave == 1 && lane < 3 * kPolicyEnvsPerWg) {
          const int is = POP ? base + c : blockIdx.x * kPolicyEnvsPerWg + c;      // (q = the dimension)
          const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), is, kGaussDraw);
          const float eps = normal_quantile_f32((q == 0 ? b.x : (q == 1 ? b.y : b.z)) >> 8);
          EPS[c * 4 + q] = eps;
          if (a.head.eps_out && is < a.k.cfg.n && (!POP || is >= 0)) a.head.eps_out[(((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)is) * 3 + q] = eps;
        }
      }
      // ---- output layer on wave 0: one accumulator, HL / 4 dependent MFMAs
      if (wave == 0) {
        f32x4 acc = {bo, bo, bo, bo};
        const float* arow = AL + c * HL + q * (HL >> 2);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) {
          if (s4 * 16 < HL) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
            if constexpr (WO_LDS) {
              f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
              if (c < NOUT) bv = *reinterpret_cast<const f32x4*>(lds + WO_OFF + (c * 4 + q) * (HL >> 2) + 4 * s4);
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
            } else {
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wo[4 * s4 + s], acc, 0, 0, 0);
            }
          }
        }
        if (c < NOUT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ACT[(q * 4 + r) * ACTW + c] = acc[r];
        }
      }
      __syncthreads();
      POL_STAMP(3);
      if constexpr (GAUSS) {
        // ---- the head, one lane per (env, dimension): lanes 0..47 of wave 0
        if (threadIdx.x < 3 * kPolicyEnvsPerWg) {
          const float act = gaussian_head_action(a.head, a.p.out_act, ACT[c * ACTW + q], ACT[c * ACTW + 3 + q], EPS[c * 4 + q]);
          ACT[c * ACTW + q] = act;
        }
        if (wave == 0) {                                                // the env lanes are lanes of this wave: a wavefront fence, no workgroup barrier
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        POL_STAMP(5);
      }
      // ---- env step, one lane per env
      if (env_lane) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ACT + (int)threadIdx.x * ACTW);
        float a0 = av[0], a1 = av[1], a2 = av[2];
        if constexpr (!GAUSS) {
          a0 = policy_act(a0, a.p.out_act); a1 = policy_act(a1, a.p.out_act); a2 = policy_act(a2, a.p.out_act);
        }
        if constexpr (POP) {
          float reward;
          bool succ;
          policy_env_step<GENERAL>(a, i, e, t, L, g, a0, a1, a2, o, reward, succ);
          episode_sum_step(es, t, reward, succ);
        } else {
          policy_env_step<GENERAL>(a, i, e, t, L, g, a0, a1, a2, o);
        }
      }
      POL_STAMP(4);
    }
    if constexpr (POP) {
      if (env_lane) episode_sum_store(a.sum, (size_t)e * (size_t)a.k.cfg.n + (size_t)i, es);
    }
  }
#ifdef EARL_POLICY_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) g_policy_prof[k] = prof[k];
  }
#endif
  if (env_lane) store_lane<NOBJ>(a.k, i, L);
