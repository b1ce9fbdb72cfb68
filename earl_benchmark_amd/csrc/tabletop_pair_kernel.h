// tabletop_pair_kernel.h -- the kernel of earl_tabletop_pair_rollout and earl_tabletop3_pair_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout with
// the forward / reset agent pair of autonomous RL alternating inside ONE launch, for the one- and the three-object env.  ONE text, pair_kernel<NOBJ, NT2, GAUSS>, and
// one host front, launch_pair_rollout<NOBJ>; tabletop_policy_pair.hip (NOBJ = 1) and tabletop3_pair.hip (NOBJ = 3) instantiate them, as two units that compile side by
// side.  The env's side (phase state, handover rule, goal overlay) is tabletop_policy.h's pair_env_step<NOBJ>, shared with the host twin.  The forty single-policy /
// population kernels and the three-object env's twenty are not routed through this body.
// TWIN: the step body below restates tabletop_policy_kernel.inc's (layer 0, hidden layer, output chain, head, fence) once per agent -- the one restatement left.  Each
// env's action is held bit for bit to that chain at the same NOBJ, so a change to the arithmetic or its order in either file is mirrored in the other by hand.  Held by:
// tests/test_policy_pair.py (test 1) and tests/test_tabletop3_pair.py (test 1), the host twins against the single-policy entry points; tests/test_policy_pair_gpu.py and
// tests/test_tabletop3_pair_gpu.py, the device against both.
//
// The workgroup is the single-policy kernel's: 16 envs (the M of v_mfma_f32_16x16x4_f32) x four waves, env state on lanes 0..15 of wave 0 for the whole launch,
// the same lane maps and LDS image layout (tabletop_policy.h); the observation image is [16][NOBS] in pol_idx order, and each N-tile of layer 0 is NOBS / 4 (3 / 5)
// chained MFMAs with C = the bias.  What differs from the single-policy kernel:
//   weights   BOTH agents' weights are loaded once in the prologue, into register arrays [2][..] indexed by unrolled constants only (or into LDS images, below)
//   ballot    each step wave 0 forms the ballot of `phase` over the live env lanes and publishes, with the observation rows and before the step's first barrier,
//             one LDS word: bit k set = some live env of this workgroup is in phase k.  Every wave reads it after that barrier as a wave-uniform value
//   uniform   workgroup (one bit set -- the common case: fixed clocks from a common reset keep every workgroup uniform): only that agent's layers run, between
//             the single-policy kernel's barriers
//   mixed     workgroup (both bits): both networks are evaluated on all 16 rows, each into its OWN activation and action images in LDS, between the same
//             barriers -- no barrier is added on either path.  MFMA rows are independent, so the action row an env lane reads from the images of its own phase is
//             bit for bit its agent's single-policy chain
//   output    layer of agent k: wave 2 k (one accumulator, Hlast / 4 dependent MFMAs: the serial part) -- in a mixed workgroup the two chains run side by
//             side on waves 0 and 2 instead of back to back; the Gaussian head's draws stay on wave 1 (they do not depend on the phase), the head itself on
//             lanes 0..47 of wave 0, which take the phase of env c from the ballot
// GENERAL is always on (the forward handover draws from Philox inside the loop); instantiations are NOBJ x NT2 x GAUSS.
//
// Two weight sets do not fit one wave's 512 registers (VGPR + AGPR, one wave per SIMD) at every width -- a second network adds 64 NT2 + 64 + 13 to the single-policy
// kernel's ~214 / ~300 / ~386 at NT2 = 0 / 1 / 2, and NOBJ = 3 brings Lane<3> (four more doubles), g[10], o[20] and two more k-steps of layer 0 per tile and agent --
// so per env and width class some operands live in LDS instead, each in the order a lane reads it (PairPolicy below says which):
//   WO_LDS  both agents' output-layer B operands, [agent][6][4][HL / 4]: one 16-byte read per four k-steps, independent of the MFMA chain, as the single-policy
//           NT2 = 4 kernel's
//   W0_LDS  both agents' layer-0 B operand and bias, [agent][n][NOBS + 1]: slot (NOBS / 4) q + s = W0[n][4 s + q], slot NOBS = b0[n].  A lane's operands are
//           contiguous.  The row stride of 21 dwords is odd: the 32 lanes of a ds_read_b32 group (c = 0..15, two values of q: dword 21 c + 5 q + s, bank = dword
//           mod 32) fall on 31 banks -- only (c = 0, q) and (c = 15, q + 1) share one -- where a stride of 20 would put c and c + 8 on one bank throughout.  The bias
//           read is one address per c (the four q broadcast), 16 distinct banks
//   PARK    the env lanes' L.e.q[NQ] (doubles) and g[NG]: written to an LDS row per env with the observation rows at the top of the step (from there on the
//           registers are dead), read back just before the env step.  Only the env's own lane touches its row: no barrier
//
// The twelve kernels (the compiler's lines: profiles/policy_kernel_resources.txt; tests/test_policy_pair.py and tests/test_tabletop3_pair.py recompile and compare, and
// the latter holds every kernel's assembly to the build before the two texts became this one).  No instantiation has scratch:
//   NOBJ  NT2                                     VGPR + AGPR, deterministic (Gaussian head)   in LDS                  static LDS per workgroup
//   1     0 (one hidden layer, every width)       256 +  47 ( 57)                              --                       57,360 B
//   1     1 (H2 <= 64)                            256 + 192 (201)                              --                       57,360 B
//   1     2 (H2 <= 128)                           256 + 222 (232)                              WO_LDS                   57,360 B
//   3     0                                       256 + 130 (136)                              --                       51,728 B
//   3     1                                       256 + 147 (152)                              WO_LDS                   57,872 B
//   3     2                                       256 + 242 (246)                              WO_LDS, W0_LDS, PARK    102,672 B
//   NT2 >= 3   does not fit: EARL_PAIR_MAX_H2 = 128, refused by check_pair of both libraries
#pragma once
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

namespace earl {

// LDS float offsets of the pair kernel's images
template <int NOBJ>
struct PairLds {
  static constexpr int NOBS = Dims<NOBJ>::NOBS;
  static constexpr int X = 0;                                              // observation rows [16][NOBS]
  static constexpr int Flags = 16 * NOBS;                                  // the step's ballot word (+ 3 floats of padding: the images stay 16-byte aligned)
  static constexpr int H1 = Flags + 4;                                     // [2 agents][16][H1]
  static constexpr int H2 = H1 + 2 * 16 * kPolicyMaxWidth;                 // [2][16][H2], H2 <= kPairMaxH2
  static constexpr int Act = H2 + 2 * 16 * kPairMaxH2;                     // [2][16][8] action rows (0..2 mean -> action, 3..5 raw log_std)
  static constexpr int Eps = Act + 2 * 16 * 8;                             // the step's draws [16][4]
  static constexpr int Wo = Eps + 16 * 4;                                  // WO_LDS: [2][6][4][HL / 4], HL = H2 <= kPairMaxH2
  static constexpr int W0 = Wo + 2 * 6 * kPairMaxH2;                       // W0_LDS: [2][kPolicyMaxWidth][W0Row]
  static constexpr int W0Row = NOBS + 1;
  static constexpr int Park = W0 + 2 * kPolicyMaxWidth * W0Row;            // PARK: [16][ParkRow] = q[NQ] as doubles, g[NG], 2 floats of padding
  static constexpr int ParkRow = 2 * Dims<NOBJ>::NQ + Dims<NOBJ>::NG + 2;
  static constexpr int Lds = Park + 16 * ParkRow;
  static_assert(Park % 2 == 0 && ParkRow % 2 == 0, "the parked doubles are 8-byte aligned");
  static_assert(ParkRow >= 2 * Dims<NOBJ>::NQ + Dims<NOBJ>::NG, "the parked row is q[NQ] and g[NG]");
};

// What is policy and not arithmetic, per env and width class: which operands leave the registers for LDS (the table above), and two figures that follow from it
template <int NOBJ, int NT2>
struct PairPolicy {
  static constexpr bool WO_LDS = NT2 >= (NOBJ == 3 ? 1 : 2);               // NOBJ = 1: 2 x 128 hidden-layer weight registers per lane leave no room for 2 x 64 more
  static constexpr bool W0_LDS = NOBJ == 3 && NT2 >= 2;
  static constexpr bool PARK = W0_LDS;
  // The two below keep the code of the two texts this one replaced bit for bit (one object declared every image up to W0 whatever the class, and its output loop
  // always ran to 16) -- they are not a choice made here, and narrowing either changes the kernels' recorded figures or assembly: not without re-measuring
  static constexpr int kLdsFloats = PARK ? PairLds<NOBJ>::Lds : ((WO_LDS || NOBJ == 1) ? PairLds<NOBJ>::W0 : PairLds<NOBJ>::Wo);
  static constexpr int kOutS4 = (WO_LDS && NOBJ == 3) ? kPairMaxH2 / 16 : 16;      // the output layer's s4 bound (guarded by s4 * 16 < HL either way)
};

template <int NOBJ, int NT2, bool GAUSS>
__global__ __launch_bounds__(256) void pair_kernel(const PairArgs a) {
  using O = PairLds<NOBJ>;
  using Pol = PairPolicy<NOBJ, NT2>;
  constexpr int NOBS = Dims<NOBJ>::NOBS, KS0 = NOBS / 4, NQ = Dims<NOBJ>::NQ, NG = Dims<NOBJ>::NG, NOUT = GAUSS ? 6 : 3, ACTW = 8;
  constexpr bool WO_LDS = Pol::WO_LDS, W0_LDS = Pol::W0_LDS, PARK = Pol::PARK;
  __shared__ __attribute__((aligned(16))) float lds[Pol::kLdsFloats];
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int H1 = a.p.dims[1], HL = a.p.dims[a.p.n_layers - 1], H2 = NT2 > 0 ? a.p.dims[2] : 0;

  // ---- prologue: both agents' weights into registers (or their LDS images), once
  const int nt0 = (H1 / 16 - wave + 3) >> 2;                          // this wave's N-tiles of layer 0: tl = wave + 4 j, j < nt0
  constexpr int NT2A = NT2 > 0 ? NT2 : 1;
  const int nt1 = NT2 > 0 ? (H2 / 16 - wave + 3) >> 2 : 0;
  float w0[2][W0_LDS ? 1 : 4][KS0], b0[2][W0_LDS ? 1 : 4], w1[2][NT2A][64], b1[2][NT2A], wo[2][WO_LDS ? 1 : 64], bo[2];
#pragma unroll
  for (int ag = 0; ag < 2; ++ag) {
    const float* __restrict__ W0 = a.p.params + (size_t)ag * (size_t)a.pair.param_stride;
    const float* __restrict__ B0 = W0 + H1 * NOBS;
    const float* __restrict__ W1 = B0 + H1;
    const float* __restrict__ B1 = W1 + H2 * H1;
    const float* __restrict__ WO = NT2 > 0 ? B1 + H2 : W1;
    const float* __restrict__ BO = WO + NOUT * HL;
    if constexpr (W0_LDS) {
      float* const W0L = lds + O::W0 + ag * kPolicyMaxWidth * O::W0Row;
      for (int k = (int)threadIdx.x; k < H1 * NOBS; k += 256) {
        const int n = k / NOBS, kk = k - n * NOBS;
        W0L[n * O::W0Row + (kk & 3) * KS0 + (kk >> 2)] = W0[k];
      }
      for (int n = (int)threadIdx.x; n < H1; n += 256) W0L[n * O::W0Row + NOBS] = B0[n];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = (wave + 4 * j) * 16 + c;
        const bool ok = j < nt0;
#pragma unroll
        for (int s = 0; s < KS0; ++s) w0[ag][j][s] = ok ? W0[n * NOBS + 4 * s + q] : 0.0f;
        b0[ag][j] = ok ? B0[n] : 0.0f;
      }
    }
    if constexpr (NT2 > 0) {
#pragma unroll
      for (int j = 0; j < NT2; ++j) {
        const int n = (wave + 4 * j) * 16 + c;
        const bool ok = j < nt1;
#pragma unroll
        for (int s = 0; s < 64; ++s) w1[ag][j][s] = (ok && 4 * s < H1) ? W1[n * H1 + 4 * s + q] : 0.0f;
        b1[ag][j] = ok ? B1[n] : 0.0f;
      }
    } else {
      b1[ag][0] = 0.0f;
    }
    if constexpr (WO_LDS) {
      for (int k = (int)threadIdx.x; k < NOUT * HL; k += 256) {
        const int j = k / HL, kk = k - j * HL;
        lds[O::Wo + ag * 6 * kPairMaxH2 + (j * 4 + (kk & 3)) * (HL >> 2) + (kk >> 2)] = WO[k];
      }
      wo[ag][0] = 0.0f;
    } else {
#pragma unroll
      for (int s = 0; s < 64; ++s) wo[ag][s] = (wave == 2 * ag && c < NOUT && 4 * s < HL) ? WO[c * HL + 4 * s + q] : 0.0f;    // agent k's output layer: wave 2 k
    }
    bo[ag] = c < NOUT ? BO[c] : 0.0f;
  }
  // (the LDS images written above are first read after the step's first barrier)

  // ---- env lanes
  const int i = blockIdx.x * kPolicyEnvsPerWg + (int)threadIdx.x;
  const bool env_lane = threadIdx.x < kPolicyEnvsPerWg && i < a.k.cfg.n;
  Lane<NOBJ> L;
  PairLane P;
  P.phase = 0; P.sip = 0; P.fs = 0; P.bs = 0;
  float g[NG], o[NOBS];
#pragma unroll
  for (int k = 0; k < NOBS; ++k) o[k] = 0.0f;
  if (env_lane) {
    load_lane<NOBJ>(a.k, i, L);
    pair_load<NOBJ>(a, i, L, P, g);
  }
  float* const X = lds + O::X;
  int* const FLAGS = reinterpret_cast<int*>(lds + O::Flags);
  // PARK: this env's row (lanes 0..15 of wave 0 only)
  [[maybe_unused]] float* const PK = lds + (PARK ? O::Park + (int)(threadIdx.x & 15) * O::ParkRow : 0);

#ifdef EARL_POLICY_STAMPS
  unsigned long long prof[6] = {0, 0, 0, 0, 0, 0}, last_ = 0;      // (the single-policy kernel's phases, tabletop_policy.h; [0] includes the ballot)
#endif
  for (int e = 0; e < a.episodes; ++e) {
    if (env_lane) pair_episode_begin<NOBJ>(a, i, e, L, P, g, o);
#ifdef EARL_POLICY_STAMPS
    last_ = pol_clock();
#endif
    for (int t = 0; t < a.k.T; ++t) {
      unsigned long long in_reset = 0;                                  // (wave 0 only: the ballot, kept for the head's lanes)
      if (wave == 0) {
        if (threadIdx.x < kPolicyEnvsPerWg) {                           // (rows of a ragged last workgroup: zeros, results never read)
#pragma unroll
          for (int k = 0; k < NOBS; ++k) X[pol_idx((int)threadIdx.x, k, NOBS)] = o[k];
        }
        if constexpr (PARK) {
          if (env_lane) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) __builtin_memcpy(PK + 2 * k, &L.e.q[k], sizeof(double));      // (the row is declared float: a copy of the bytes, no double lvalue on it)
#pragma unroll
            for (int k = 0; k < NG; ++k) PK[2 * NQ + k] = g[k];
          }
        }
        in_reset = __builtin_amdgcn_ballot_w64(env_lane && P.phase != 0);
        const unsigned long long in_forward = __builtin_amdgcn_ballot_w64(env_lane && P.phase == 0);
        if (threadIdx.x == 0) FLAGS[0] = (in_forward != 0 ? 1 : 0) | (in_reset != 0 ? 2 : 0);
      }
      __syncthreads();
      const int flags = __builtin_amdgcn_readfirstlane(FLAGS[0]);      // wave-uniform: which networks this workgroup runs this step
      POL_STAMP(0);
      // ---- layer 0: NOBS -> H1
      {
        float xa[KS0];
#pragma unroll
        for (int s = 0; s < KS0; ++s) xa[s] = X[c * NOBS + q * KS0 + s];
#pragma unroll
        for (int ag = 0; ag < 2; ++ag) {
          if (flags & (1 << ag)) {
            float* const A1 = lds + O::H1 + ag * 16 * kPolicyMaxWidth;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (j < nt0) {
                const int n = (wave + 4 * j) * 16 + c;
                f32x4 acc;
                if constexpr (W0_LDS) {
                  const float* const wr = lds + O::W0 + (ag * kPolicyMaxWidth + n) * O::W0Row;
                  const float bj = wr[NOBS];
                  acc = f32x4{bj, bj, bj, bj};
#pragma unroll
                  for (int s = 0; s < KS0; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wr[q * KS0 + s], acc, 0, 0, 0);
                } else {
                  acc = f32x4{b0[ag][j], b0[ag][j], b0[ag][j], b0[ag][j]};
#pragma unroll
                  for (int s = 0; s < KS0; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], w0[ag][j][s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) A1[pol_idx(q * 4 + r, n, H1)] = policy_act(acc[r], a.p.hidden_act);
              }
            }
          }
        }
      }
      __syncthreads();
      POL_STAMP(1);
      // ---- hidden layer: H1 -> H2
      if constexpr (NT2 > 0) {
#pragma unroll
        for (int ag = 0; ag < 2; ++ag) {
          if ((flags & (1 << ag)) && nt1 > 0) {
            const float* const A1 = lds + O::H1 + ag * 16 * kPolicyMaxWidth;
            float* const A2 = lds + O::H2 + ag * 16 * kPairMaxH2;
            f32x4 acc[NT2];
#pragma unroll
            for (int j = 0; j < NT2; ++j) acc[j] = f32x4{b1[ag][j], b1[ag][j], b1[ag][j], b1[ag][j]};
            const float* arow = A1 + c * H1 + q * (H1 >> 2);
#pragma unroll
            for (int s4 = 0; s4 < 16; ++s4) {
              if (s4 * 16 < H1) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                  for (int j = 0; j < NT2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], w1[ag][j][4 * s4 + s], acc[j], 0, 0, 0);
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
        }
        __syncthreads();
      }
      POL_STAMP(2);
      if constexpr (GAUSS) {
        // ---- the step's draws on wave 1, beside the output layers: lane = (env, dimension); the draw does not depend on the phase
        if (wave == 1 && lane < 3 * kPolicyEnvsPerWg) {
          const int is = blockIdx.x * kPolicyEnvsPerWg + c;              // (q = the dimension)
          const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), is, kGaussDraw);
          const float eps = normal_quantile_f32((q == 0 ? b.x : (q == 1 ? b.y : b.z)) >> 8);
          lds[O::Eps + c * 4 + q] = eps;
          if (a.head.eps_out && is < a.k.cfg.n) a.head.eps_out[(((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)is) * 3 + q] = eps;
        }
      }
      // ---- output layer of agent k on wave 2 k: one accumulator, HL / 4 dependent MFMAs
#pragma unroll
      for (int ag = 0; ag < 2; ++ag) {
        if (wave == 2 * ag && (flags & (1 << ag))) {
          const float* const AL = NT2 > 0 ? lds + O::H2 + ag * 16 * kPairMaxH2 : lds + O::H1 + ag * 16 * kPolicyMaxWidth;
          float* const ACT = lds + O::Act + ag * 16 * ACTW;
          f32x4 acc = {bo[ag], bo[ag], bo[ag], bo[ag]};
          const float* arow = AL + c * HL + q * (HL >> 2);
#pragma unroll
          for (int s4 = 0; s4 < Pol::kOutS4; ++s4) {
            if (s4 * 16 < HL) {
              const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
              if constexpr (WO_LDS) {
                f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
                if (c < NOUT) bv = *reinterpret_cast<const f32x4*>(lds + O::Wo + ag * 6 * kPairMaxH2 + (c * 4 + q) * (HL >> 2) + 4 * s4);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
              } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wo[ag][4 * s4 + s], acc, 0, 0, 0);
              }
            }
          }
          if (c < NOUT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) ACT[(q * 4 + r) * ACTW + c] = acc[r];
          }
        }
      }
      __syncthreads();
      POL_STAMP(3);
      if constexpr (GAUSS) {
        // ---- the head, one lane per (env, dimension): lanes 0..47 of wave 0, on the action row of env c's own agent
        if (threadIdx.x < 3 * kPolicyEnvsPerWg) {
          float* const ACT = lds + O::Act + (int)((in_reset >> c) & 1ull) * 16 * ACTW;
          const float act = gaussian_head_action(a.head, a.p.out_act, ACT[c * ACTW + q], ACT[c * ACTW + 3 + q], lds[O::Eps + c * 4 + q]);
          ACT[c * ACTW + q] = act;
        }
        if (wave == 0) {                                                // the env lanes are lanes of this wave: a wavefront fence, no workgroup barrier
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        POL_STAMP(5);
      }
      // ---- env step, one lane per env: the action row of the env's own agent
      if (env_lane) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(lds + O::Act + P.phase * 16 * ACTW + (int)threadIdx.x * ACTW);
        float a0 = av[0], a1 = av[1], a2 = av[2];
        if constexpr (!GAUSS) {
          a0 = policy_act(a0, a.p.out_act); a1 = policy_act(a1, a.p.out_act); a2 = policy_act(a2, a.p.out_act);
        }
        if constexpr (PARK) {
#pragma unroll
          for (int k = 0; k < NQ; ++k) __builtin_memcpy(&L.e.q[k], PK + 2 * k, sizeof(double));
#pragma unroll
          for (int k = 0; k < NG; ++k) g[k] = PK[2 * NQ + k];
        }
        pair_env_step<NOBJ>(a, i, e, t, L, P, g, a0, a1, a2, o);
      }
      POL_STAMP(4);
    }
    if (env_lane) pair_episode_end(a, i, e, P);
  }
#ifdef EARL_POLICY_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) g_policy_prof[k] = prof[k];
  }
#endif
  if (env_lane) pair_store<NOBJ>(a, i, L, P);
}

namespace hostside {

// (both host templates are static: local to the unit that instantiates them, as the launchers of the other units, and no symbol of the library)
template <int NOBJ, bool GAUSS>
static void launch_pair(const PairArgs& a, dim3 grid, hipStream_t s) {
  static_assert(kPairMaxH2 == 128, "one instantiation per N-tile count a wave owns in the hidden -> hidden layer: 0, 1 (H2 <= 64), 2 (H2 <= 128)");
  switch (a.p.n_layers == 3 ? (a.p.dims[2] + 63) / 64 : 0) {
    case 0: pair_kernel<NOBJ, 0, GAUSS><<<grid, 256, 0, s>>>(a); break;
    case 1: pair_kernel<NOBJ, 1, GAUSS><<<grid, 256, 0, s>>>(a); break;
    default: pair_kernel<NOBJ, 2, GAUSS><<<grid, 256, 0, s>>>(a); break;
  }
}

// the body of both entry points; `what` names the launch in the error text
template <int NOBJ>
static int launch_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                        const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out,
                        earl_stream_t stream, const char* what) {
  if (int rc = check_pair(cfg, st, policy, pair, head, episodes, T, reset_first, out, NOBJ)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  const PairArgs a = pair_args(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, thresholds(), NOBJ);
  const dim3 grid((unsigned)((cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  if (head) launch_pair<NOBJ, true>(a, grid, s);
  else launch_pair<NOBJ, false>(a, grid, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EARL_OK;
}

}  // namespace hostside
}  // namespace earl
