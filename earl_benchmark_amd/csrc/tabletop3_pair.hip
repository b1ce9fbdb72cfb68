// tabletop3_pair.hip -- earl_tabletop3_pair_rollout (include/earl_tabletop.h): the closed-loop rollout of the THREE-object tabletop with the forward / reset agent
// pair alternating inside ONE launch.  The env's side (phase state, handover rule, the 10-wide goal overlay) is tabletop_policy.h's pair_env_step<3>, shared with the
// host twin and with the single-object pair; this unit holds the kernel.
// TWIN: the step body below restates tabletop_policy_pair.hip's (ballot, layer 0, hidden layer, output chains, draws, head, fence) at NOBJ = 3: the two are not one
// text, so that the single-object pair's six kernels keep their register figures whatever this one needs.  Each env's action is held bit for bit to
// tabletop_policy_kernel.inc's chain at NOBJ = 3, so a change to the arithmetic or its order in any of the three files is mirrored in the others by hand
// (tests/test_tabletop3_pair.py compares this entry point's host twin with earl_tabletop3_policy_rollout_cpu, tests/test_tabletop3_pair_gpu.py the device's with both).
//
// The workgroup, the ballot word, uniform / mixed workgroups, output layer k on wave 2 k, the draws on wave 1 and the head on lanes 0..47 of wave 0 are the
// single-object pair's (its header has the description).  What differs:
//   observation   image [16][20] in pol_idx order; each N-tile of layer 0 is five chained v_mfma_f32_16x16x4_f32 with C = the bias
//   registers     Lane<3> (four more doubles), g[10], o[20] and two more k-steps of layer 0 per tile and agent do not fit beside two weight sets from NT2 = 1
//                 on, so per width class some operands live in LDS instead, each in the order a lane reads it:
//     WO_LDS  (NT2 >= 1)  both agents' output-layer B operands, [agent][6][4][HL / 4]: one 16-byte read per four k-steps, independent of the MFMA chain
//     W0_LDS  (NT2 == 2)  both agents' layer-0 B operand and bias, [agent][n][21]: slot 5 q + s = W0[n][4 s + q], slot 20 = b0[n].  A lane's five operands are
//                         contiguous.  The row stride of 21 dwords is odd: the 32 lanes of a ds_read_b32 group (c = 0..15, two values of q: dword 21 c + 5 q + s,
//                         bank = dword mod 32) fall on 31 banks -- only (c = 0, q) and (c = 15, q + 1) share one -- where a stride of 20 would put c and c + 8
//                         on one bank throughout.  The bias read is one address per c (the four q broadcast), 16 distinct banks
//     PARK    (NT2 == 2)  the env lanes' L.e.q[8] (doubles) and g[10]: written to a 28-float LDS row per env with the observation rows at the top of the step
//                         (from there on the registers are dead), read back just before the env step.  Only the env's own lane touches its row: no barrier
//
// Registers (VGPR + AGPR, one wave per SIMD: 512) and static LDS per workgroup:
//   NT2 = 0 (one hidden layer, every width) 256 + 130 (Gaussian head: + 136)   all weights in registers              51,728 B
//   NT2 = 1 (H2 <= 64)                      256 + 147 (+ 152)                  WO_LDS                                57,872 B
//   NT2 = 2 (H2 <= 128)                     256 + 242 (+ 246)                  WO_LDS, W0_LDS, PARK                 102,672 B
//   NT2 >= 3                                does not fit: EARL_PAIR_MAX_H2 = 128, refused by check_pair of both libraries
// No instantiation has scratch; the compiler's lines are appended to profiles/policy_kernel_resources.txt, and tests/test_tabletop3_pair.py recompiles and compares.
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

using namespace earl;
using namespace earl::hostside;

namespace earl {

constexpr int kP3Obs = Dims<3>::NOBS, kP3Ks0 = kP3Obs / 4;             // 20 observations, five k-steps of layer 0
constexpr int kP3X = 0;                                                // LDS floats: observation rows [16][20]
constexpr int kP3Flags = 16 * kP3Obs;                                  // the step's ballot word (+ 3 floats of padding: the images stay 16-byte aligned)
constexpr int kP3H1 = kP3Flags + 4;                                    // [2 agents][16][H1]
constexpr int kP3H2 = kP3H1 + 2 * 16 * kPolicyMaxWidth;                // [2][16][H2], H2 <= kPairMaxH2
constexpr int kP3Act = kP3H2 + 2 * 16 * kPairMaxH2;                    // [2][16][8] action rows (0..2 mean -> action, 3..5 raw log_std)
constexpr int kP3Eps = kP3Act + 2 * 16 * 8;                            // the step's draws [16][4]
constexpr int kP3Wo = kP3Eps + 16 * 4;                                 // WO_LDS: [2][6][4][HL / 4], HL = H2 <= kPairMaxH2
constexpr int kP3W0 = kP3Wo + 2 * 6 * kPairMaxH2;                      // W0_LDS: [2][kPolicyMaxWidth][21]
constexpr int kP3W0Row = kP3Obs + 1;
constexpr int kP3Park = kP3W0 + 2 * kPolicyMaxWidth * kP3W0Row;        // PARK: [16][28] = q[8] as doubles, g[10], 2 floats of padding
constexpr int kP3ParkRow = 28;
constexpr int kP3Lds = kP3Park + 16 * kP3ParkRow;
static_assert(kP3Park % 2 == 0 && kP3ParkRow % 2 == 0, "the parked doubles are 8-byte aligned");
static_assert(Dims<3>::NQ == 8 && Dims<3>::NG == 10, "the parked row is q[8] and g[10]");

template <int NT2, bool GAUSS>
__global__ __launch_bounds__(256) void tabletop3_pair_kernel(const PairArgs a) {
  constexpr int NOBS = kP3Obs, KS0 = kP3Ks0, NOUT = GAUSS ? 6 : 3, ACTW = 8;
  constexpr bool WO_LDS = NT2 >= 1, W0_LDS = NT2 >= 2, PARK = NT2 >= 2;
  __shared__ __attribute__((aligned(16))) float lds[PARK ? kP3Lds : (WO_LDS ? kP3W0 : kP3Wo)];
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
      float* const W0L = lds + kP3W0 + ag * kPolicyMaxWidth * kP3W0Row;
      for (int k = (int)threadIdx.x; k < H1 * NOBS; k += 256) {
        const int n = k / NOBS, kk = k - n * NOBS;
        W0L[n * kP3W0Row + (kk & 3) * KS0 + (kk >> 2)] = W0[k];
      }
      for (int n = (int)threadIdx.x; n < H1; n += 256) W0L[n * kP3W0Row + NOBS] = B0[n];
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
        lds[kP3Wo + ag * 6 * kPairMaxH2 + (j * 4 + (kk & 3)) * (HL >> 2) + (kk >> 2)] = WO[k];
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
  Lane<3> L;
  PairLane P;
  P.phase = 0; P.sip = 0; P.fs = 0; P.bs = 0;
  float g[Dims<3>::NG], o[NOBS];
#pragma unroll
  for (int k = 0; k < NOBS; ++k) o[k] = 0.0f;
  if (env_lane) {
    load_lane<3>(a.k, i, L);
    pair_load<3>(a, i, L, P, g);
  }
  float* const X = lds + kP3X;
  int* const FLAGS = reinterpret_cast<int*>(lds + kP3Flags);
  // PARK: this env's row (lanes 0..15 of wave 0 only)
  [[maybe_unused]] float* const PK = lds + (PARK ? kP3Park + (int)(threadIdx.x & 15) * kP3ParkRow : 0);

  for (int e = 0; e < a.episodes; ++e) {
    if (env_lane) pair_episode_begin<3>(a, i, e, L, P, g, o);
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
            for (int k = 0; k < 8; ++k) __builtin_memcpy(PK + 2 * k, &L.e.q[k], sizeof(double));      // (the row is declared float: a copy of the bytes, no double lvalue on it)
#pragma unroll
            for (int k = 0; k < 10; ++k) PK[16 + k] = g[k];
          }
        }
        in_reset = __builtin_amdgcn_ballot_w64(env_lane && P.phase != 0);
        const unsigned long long in_forward = __builtin_amdgcn_ballot_w64(env_lane && P.phase == 0);
        if (threadIdx.x == 0) FLAGS[0] = (in_forward != 0 ? 1 : 0) | (in_reset != 0 ? 2 : 0);
      }
      __syncthreads();
      const int flags = __builtin_amdgcn_readfirstlane(FLAGS[0]);      // wave-uniform: which networks this workgroup runs this step
      // ---- layer 0: 20 -> H1
      {
        float xa[KS0];
#pragma unroll
        for (int s = 0; s < KS0; ++s) xa[s] = X[c * NOBS + q * KS0 + s];
#pragma unroll
        for (int ag = 0; ag < 2; ++ag) {
          if (flags & (1 << ag)) {
            float* const A1 = lds + kP3H1 + ag * 16 * kPolicyMaxWidth;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (j < nt0) {
                const int n = (wave + 4 * j) * 16 + c;
                f32x4 acc;
                if constexpr (W0_LDS) {
                  const float* const wr = lds + kP3W0 + (ag * kPolicyMaxWidth + n) * kP3W0Row;
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
      // ---- hidden layer: H1 -> H2
      if constexpr (NT2 > 0) {
#pragma unroll
        for (int ag = 0; ag < 2; ++ag) {
          if ((flags & (1 << ag)) && nt1 > 0) {
            const float* const A1 = lds + kP3H1 + ag * 16 * kPolicyMaxWidth;
            float* const A2 = lds + kP3H2 + ag * 16 * kPairMaxH2;
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
      if constexpr (GAUSS) {
        // ---- the step's draws on wave 1, beside the output layers: lane = (env, dimension); the draw does not depend on the phase
        if (wave == 1 && lane < 3 * kPolicyEnvsPerWg) {
          const int is = blockIdx.x * kPolicyEnvsPerWg + c;              // (q = the dimension)
          const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), is, kGaussDraw);
          const float eps = normal_quantile_f32((q == 0 ? b.x : (q == 1 ? b.y : b.z)) >> 8);
          lds[kP3Eps + c * 4 + q] = eps;
          if (a.head.eps_out && is < a.k.cfg.n) a.head.eps_out[(((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)is) * 3 + q] = eps;
        }
      }
      // ---- output layer of agent k on wave 2 k: one accumulator, HL / 4 dependent MFMAs
#pragma unroll
      for (int ag = 0; ag < 2; ++ag) {
        if (wave == 2 * ag && (flags & (1 << ag))) {
          const float* const AL = NT2 > 0 ? lds + kP3H2 + ag * 16 * kPairMaxH2 : lds + kP3H1 + ag * 16 * kPolicyMaxWidth;
          float* const ACT = lds + kP3Act + ag * 16 * ACTW;
          f32x4 acc = {bo[ag], bo[ag], bo[ag], bo[ag]};
          const float* arow = AL + c * HL + q * (HL >> 2);
#pragma unroll
          for (int s4 = 0; s4 < (WO_LDS ? kPairMaxH2 / 16 : 16); ++s4) {
            if (s4 * 16 < HL) {
              const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
              if constexpr (WO_LDS) {
                f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
                if (c < NOUT) bv = *reinterpret_cast<const f32x4*>(lds + kP3Wo + ag * 6 * kPairMaxH2 + (c * 4 + q) * (HL >> 2) + 4 * s4);
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
      if constexpr (GAUSS) {
        // ---- the head, one lane per (env, dimension): lanes 0..47 of wave 0, on the action row of env c's own agent
        if (threadIdx.x < 3 * kPolicyEnvsPerWg) {
          float* const ACT = lds + kP3Act + (int)((in_reset >> c) & 1ull) * 16 * ACTW;
          const float act = gaussian_head_action(a.head, a.p.out_act, ACT[c * ACTW + q], ACT[c * ACTW + 3 + q], lds[kP3Eps + c * 4 + q]);
          ACT[c * ACTW + q] = act;
        }
        if (wave == 0) {                                                // the env lanes are lanes of this wave: a wavefront fence, no workgroup barrier
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
      // ---- env step, one lane per env: the action row of the env's own agent
      if (env_lane) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(lds + kP3Act + P.phase * 16 * ACTW + (int)threadIdx.x * ACTW);
        float a0 = av[0], a1 = av[1], a2 = av[2];
        if constexpr (!GAUSS) {
          a0 = policy_act(a0, a.p.out_act); a1 = policy_act(a1, a.p.out_act); a2 = policy_act(a2, a.p.out_act);
        }
        if constexpr (PARK) {
#pragma unroll
          for (int k = 0; k < 8; ++k) __builtin_memcpy(&L.e.q[k], PK + 2 * k, sizeof(double));
#pragma unroll
          for (int k = 0; k < 10; ++k) g[k] = PK[16 + k];
        }
        pair_env_step<3>(a, i, e, t, L, P, g, a0, a1, a2, o);
      }
    }
    if (env_lane) pair_episode_end(a, i, e, P);
  }
  if (env_lane) pair_store<3>(a, i, L, P);
}

}  // namespace earl

namespace {

template <bool GAUSS>
void launch_pair3(const PairArgs& a, dim3 grid, hipStream_t s) {
  static_assert(kPairMaxH2 == 128, "one instantiation per N-tile count a wave owns in the hidden -> hidden layer: 0, 1 (H2 <= 64), 2 (H2 <= 128)");
  switch (a.p.n_layers == 3 ? (a.p.dims[2] + 63) / 64 : 0) {
    case 0: tabletop3_pair_kernel<0, GAUSS><<<grid, 256, 0, s>>>(a); break;
    case 1: tabletop3_pair_kernel<1, GAUSS><<<grid, 256, 0, s>>>(a); break;
    default: tabletop3_pair_kernel<2, GAUSS><<<grid, 256, 0, s>>>(a); break;
  }
}

}  // namespace

extern "C" int earl_tabletop3_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                           const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out,
                                           float* act_out, earl_stream_t stream) {
  if (int rc = check_pair(cfg, st, policy, pair, head, episodes, T, reset_first, out, 3)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  const PairArgs a = pair_args(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, thresholds(), 3);
  const dim3 grid((unsigned)((cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  if (head) launch_pair3<true>(a, grid, s);
  else launch_pair3<false>(a, grid, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "tabletop3_pair_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}
