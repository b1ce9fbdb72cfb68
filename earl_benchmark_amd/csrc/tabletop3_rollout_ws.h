// tabletop3_rollout_ws.h -- role-split evaluation kernel of the THREE-object tabletop (earl_tabletop3_eval_episodes, csrc/tabletop3_eval.hip).
//
// Why: the plain one-lane-per-env rollout (rollout_kernel<3>, tabletop_step.h: rollout_body) puts the action loads, an 80-byte observation row and three scalar
// stores per step on the wave that also walks the fp64 recurrence, and an evaluation of E episodes is 2 E launches of it.  Here a 64-env workgroup splits the step
// by ROLE, in the shape of rollout_ws_kernel (tabletop_rollout_ws.h), and one launch walks all episodes:
//
//   wave 0        COMPUTE  the recurrence only, one lane per env, Env<3> in registers: reset_env<3> at the head of each episode, then per step move<3>
//                          (tabletop_device.h: the three sqrt of the grasp test and the per-object selects, as every other NOBJ = 3 kernel) on actions read
//                          from LDS; writes the 8 float32 coordinates and the flag pair into the step's LDS row image.  No global access inside the step loop.
//   waves 1..2    LOADERS  stream the raw actions HBM -> registers ONE CHUNK AHEAD with coalesced dword loads (192 consecutive floats per step), transpose
//                          them through a private LDS row and rescale_action them to fp64 into the LDS action ring
//   waves 3..6    STORERS  copy finished row images LDS -> HBM: a step's 64 rows are 5,120 contiguous bytes of [T, n, 20], stored as non-temporal float4;
//                          evaluate reward_success<3> on the env's own row (sparse and dense), store reward and the done / success bytes from ballots
//
// One workgroup barrier per chunk of K = 8 steps.  In barrier interval `it` the loaders publish chunk it, the compute wave runs chunk it - 1 and the storers
// store chunk it - 2, so both rings are 2 deep: A[it & 1] is written while A[(it - 1) & 1] is read, R[(it - 1) & 1] is written while R[it & 1] is read.
// LDS: R 2 x 8 x 5,120 = 81,920 B, A 2 x 8 x 3 x 64 doubles = 24,576 B, loader staging 2 x 768 B: 108,032 B, one workgroup per CU.
//
// Row image = the HBM bytes: 20 floats per env (coords 0..7, flags 8..9, goal 10..19).  The compute wave writes floats 0..9 of its env's row (two 16-byte and one
// 8-byte LDS store: the row stride of 20 dwords puts 8 consecutive lanes of a 16-byte store on 32 distinct banks, 20 l mod 32 = 4 (5 l mod 8)); the goal slots
// are constant per episode and are written by the STORER that owns the step, env column = lane, in the first two chunks of each episode (one per ring slot;
// episodes are at least two chunks, host-checked) just before it reads the image back -- same wave, so no barrier, and nobody else touches floats 10..19.
// A storer's own-row read (two 16-byte reads at a stride of 80 bytes) is conflict-free as well: 20 l mod 64 = 4 (5 l mod 16).
//
// Episodes in flight (the single-object launch's rule): the grid is ep_groups x wgs workgroups, group g walks episodes [g ep_per_group, (g + 1) ep_per_group) of
// the launch with their own output rows, action rows and Philox counters; the group that holds the LAST episode writes the env state back, with
// num_interventions advanced by all episodes of the launch.
// Ragged tail: lanes beyond n compute on clamped (finite or not, never stored) actions in registers and LDS only; every global access is bounded by `valid`.
#pragma once
#include "tabletop_device.h"

namespace earl {

constexpr int kWs3K = 8;                    // steps per chunk (= EARL_TABLETOP3_EVAL_CHUNK)
constexpr int kWs3NL = 2, kWs3NS = 4;       // loader / storer waves
constexpr int kWs3Threads = 64 * (1 + kWs3NL + kWs3NS);

struct Ws3Args {
  int32_t n, Tep, episodes, horizon;        // Tep % kWs3K == 0, Tep >= 2 kWs3K, episodes * Tep < 2^24 (host-checked)
  const float* __restrict__ act;            // episode e: act + e * act_ep_stride, [Tep, n, 3]
  long long act_ep_stride;
  double* __restrict__ qpos;                // [n, 8]
  int8_t* __restrict__ attached;
  int32_t* __restrict__ goal_idx;
  const double* __restrict__ goal_table;    // [n_goals, 10]
  int32_t* __restrict__ steps_since_reset;
  int32_t* __restrict__ num_interventions;
  float* __restrict__ obs;                  // [episodes, Tep, n, 20]
  float* __restrict__ reward;               // [episodes, Tep, n]
  uint8_t* __restrict__ done;
  uint8_t* __restrict__ success;
  Thresholds th;
  earl_tabletop_cfg cfg;                    // seed / env_offset / reset mode / n_sample_goals / counter of the launch's first reset
  int32_t wgs, ep_groups, ep_per_group;
};

// Lanes of ONE wave exchange data through LDS: the wave's LDS queue is in order, the fence only pins the compiler's order (tabletop_rollout_ws.h: wave_lds_fence)
__device__ __forceinline__ void ws3_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int RT>
__global__ __launch_bounds__(kWs3Threads) void rollout3_ws_kernel(const Ws3Args a) {
  constexpr int E = 64, K = kWs3K, NL = kWs3NL, NS = kWs3NS, KL = K / NL, KS = K / NS;
  constexpr int ROW4 = Dims<3>::NOBS / 4, STEP4 = E * ROW4;      // float4 per env row (5) and per step image (320)
  static_assert(K % NL == 0 && K % NS == 0, "the steps of a chunk are dealt evenly");
  typedef float nt4 __attribute__((ext_vector_type(4)));
  __shared__ float4 R[2][K][STEP4];       // row images
  __shared__ double A[2][K][3][E];        // rescaled actions, one component row per 64 envs (8-byte reads at consecutive addresses)
  __shared__ float S[NL][E * 3];          // loader-private staging: one step's raw actions, coalesced order -> per env

  // XCD-aware block -> env-block map (workgroups are dealt round-robin over the 8 XCDs: those of one XCD cover consecutive env blocks, so the two 64-byte halves
  // of a done / success line meet in one L2; tabletop_rollout_ws.h)
  const int bid = (gridDim.x % 8 == 0) ? (int)((blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8) : (int)blockIdx.x;
  int wg = bid, ep0 = 0, neps = a.episodes;      // this workgroup's env block, its group's first episode and episode count
  if (a.ep_groups > 1) {
    const int grp = bid / a.wgs;
    wg = bid - grp * a.wgs;
    ep0 = grp * a.ep_per_group;
    neps = min(a.ep_per_group, a.episodes - ep0);
  }
  const bool leaves_state = ep0 + neps == a.episodes;

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = a.n, Tep = a.Tep;
  const int i0 = wg * E, i = i0 + lane;
  const int valid = min(E, n - i0);              // live envs of this workgroup (>= 1: wgs = ceil(n / 64))
  const bool live = lane < valid;
  const int cpe = Tep / K;                       // chunks per episode (>= 2)
  const int nch = neps * cpe;
  const int nit = nch + 2;                       // barrier intervals; every wave passes exactly nit barriers
  auto ep_counter = [&](int ep) -> uint64_t { return a.cfg.counter + (uint64_t)(ep0 + ep) * (uint64_t)(Tep + 1); };

  if (wave == 0) {
    // ================================================================= COMPUTE
    __builtin_amdgcn_s_setprio(3);               // the recurrence is the critical path: it wins issue arbitration on its SIMD
    Env<3> ev;
#pragma unroll
    for (int k = 0; k < 8; ++k) ev.q[k] = 0.0;
    ev.attached = -1;
    int gi = 0, ep = 0, cj = 0;
    for (int it = 0; it < nit; ++it) {
      const int c = it - 1;
      if (c >= 0 && c < nch) {
        if (cj == 0 && live) gi = reset_env<3>(ev, a.cfg, ep_counter(ep), i, a.goal_table, nullptr, a.th);   // the episode's reset (every env)
        const int rb = c & 1;
        double av[K][3];
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int m = 0; m < 3; ++m) av[k][m] = A[rb][k][m][lane];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          move<3>(ev, av[k][0], av[k][1], av[k][2], a.th);
          float4* row = &R[rb][k][lane * ROW4];
          row[0] = float4{(float)ev.q[0], (float)ev.q[1], (float)ev.q[2], (float)ev.q[3]};
          row[1] = float4{(float)ev.q[4], (float)ev.q[5], (float)ev.q[6], (float)ev.q[7]};
          const float flag = ev.attached < 0 ? -1.0f : 0.5f * (float)ev.attached;      // make_obs<3>
          *reinterpret_cast<float2*>(&row[2]) = float2{flag, flag};
        }
        if (++cj == cpe) { cj = 0; ++ep; }
      }
      __syncthreads();
    }
    if (live && leaves_state) {                  // what the sequence's last reset + rollout leave behind
      double2* q2 = reinterpret_cast<double2*>(a.qpos + (size_t)i * 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) q2[k] = double2{ev.q[2 * k], ev.q[2 * k + 1]};
      a.attached[i] = (int8_t)ev.attached;
      a.goal_idx[i] = gi;
      a.steps_since_reset[i] = Tep;
      a.num_interventions[i] += a.episodes;
    }
  } else if (wave <= NL) {
    // ================================================================= LOADERS
    // Lane l loads floats l, l + 64, l + 128 of a step's 192 (three coalesced 256-byte wave loads), indices clamped to the live part of a ragged workgroup.  The
    // loads are UNCONDITIONAL with a clamped chunk index (a load under a branch makes the compiler wait for it at once); clamped duplicates are never published.
    const int w = wave - 1;
    const int last = valid * 3 - 1;
    const int e0 = min(lane, last), e1 = min(lane + 64, last), e2 = min(lane + 128, last);
    const float* const base = a.act + (size_t)i0 * 3;
    const size_t step_stride = (size_t)n * 3;
    float rawA[KL][3], rawB[KL][3];
    auto issue = [&](float (&raw)[KL][3], int j) {       // raw <- this loader's steps (k = q NL + w) of chunk j
      j = min(j, nch - 1);
      const int ep = j / cpe, cj = j - ep * cpe;         // (wave-uniform, once per chunk)
      const float* p0 = base + (size_t)(ep0 + ep) * (size_t)a.act_ep_stride + (size_t)(cj * K + w) * step_stride;
#pragma unroll
      for (int q = 0; q < KL; ++q) {
        const float* p = p0 + (size_t)(q * NL) * step_stride;
        raw[q][0] = p[e0]; raw[q][1] = p[e1]; raw[q][2] = p[e2];
      }
    };
    auto process = [&](const float (&raw)[KL][3], int j) {   // transpose through LDS, rescale, publish chunk j
      const int ab = j & 1;
      float* sk = &S[w][0];
#pragma unroll
      for (int q = 0; q < KL; ++q) {
        sk[lane] = raw[q][0]; sk[lane + 64] = raw[q][1]; sk[lane + 128] = raw[q][2];
        ws3_wave_lds_fence();
        const float r0 = sk[lane * 3], r1 = sk[lane * 3 + 1], r2 = sk[lane * 3 + 2];      // (stride of 3 dwords: conflict-free)
        A[ab][q * NL + w][0][lane] = rescale_action(r0);
        A[ab][q * NL + w][1][lane] = rescale_action(r1);
        A[ab][q * NL + w][2][lane] = rescale_action(r2);
        ws3_wave_lds_fence();                    // the next staging writes stay behind these reads
      }
    };
    issue(rawA, 0);
    for (int it = 0; it < nit; it += 2) {        // two intervals per trip: the register buffers swap roles without a copy
      issue(rawB, it + 1);
      if (it < nch) process(rawA, it);
      __syncthreads();
      if (it + 1 < nit) {
        issue(rawA, it + 2);
        if (it + 1 < nch) process(rawB, it + 1);
        __syncthreads();
      }
    }
  } else {
    // ================================================================= STORERS
    const int s = wave - 1 - NL;                 // owns steps k = q NS + s of every chunk, both ring slots
    const bool full = (valid == E) && ((n & 3) == 0);    // whole workgroup live and the flag rows dword-aligned
    float g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int ep = 0, cj = 0;
    for (int it = 0; it < nit; ++it) {
      const int c = it - 2;
      if (c >= 0 && c < nch) {
        if (cj == 0 && live)                     // the goal of this episode: the draw its reset makes (every wave that needs it recomputes the same Philox block)
          load_goal<3>(a.goal_table, sample_goal(a.cfg, ep_counter(ep), i, nullptr), g);
        const int rb = c & 1;
        const size_t ep_row0 = (size_t)(ep0 + ep) * (size_t)Tep * (size_t)n;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          const int k = q * NS + s;
          float4* img = &R[rb][k][0];
          if (cj < 2) {                          // (wave-uniform) first use of this ring slot in the episode: its goal slots, env column = lane
            float4* row = img + lane * ROW4;
            *reinterpret_cast<float2*>(reinterpret_cast<float*>(&row[2]) + 2) = float2{g[0], g[1]};
            row[3] = float4{g[2], g[3], g[4], g[5]};
            row[4] = float4{g[6], g[7], g[8], g[9]};
            ws3_wave_lds_fence();
          }
          const float4 p0 = img[lane * ROW4], p1 = img[lane * ROW4 + 1];      // the env's own coordinates
          float4 v[ROW4];
#pragma unroll
          for (int m = 0; m < ROW4; ++m) v[m] = img[lane + 64 * m];           // the step's 5,120 bytes in HBM order
          const int tl = cj * K + k;                                          // step within the episode
          const size_t row0 = ep_row0 + (size_t)tl * (size_t)n + (size_t)i0;
          nt4* d4 = reinterpret_cast<nt4*>(a.obs + row0 * 20);
          const float o[20] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, 0.f, 0.f, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9]};
          double r;
          bool succ;
          reward_success<3>(o, RT, 0, a.th, r, succ);
          const float rew = (float)r;
          const bool dn = tl + 1 >= a.horizon;                                // steps_since_reset is 0 after the reset, + 1 per step (wrapped_step)
          if (full) {
#pragma unroll
            for (int m = 0; m < ROW4; ++m) __builtin_nontemporal_store(nt4{v[m].x, v[m].y, v[m].z, v[m].w}, d4 + lane + 64 * m);
            __builtin_nontemporal_store(rew, a.reward + row0 + lane);
            const unsigned long long ms = __ballot(succ);
            if (lane < 16) {                     // 64 flag bytes of a step = 16 dwords: ballot nibbles expanded to bytes
              const uint32_t ns = (uint32_t)(ms >> (4 * lane)) & 0xFu;
              __builtin_nontemporal_store((ns * 0x00204081u) & 0x01010101u, reinterpret_cast<uint32_t*>(a.success + row0) + lane);
              __builtin_nontemporal_store(dn ? 0x01010101u : 0u, reinterpret_cast<uint32_t*>(a.done + row0) + lane);
            }
          } else {
#pragma unroll
            for (int m = 0; m < ROW4; ++m) {
              const int idx = lane + 64 * m;
              if (idx < valid * ROW4) __builtin_nontemporal_store(nt4{v[m].x, v[m].y, v[m].z, v[m].w}, d4 + idx);
            }
            if (live) {
              a.reward[row0 + lane] = rew;
              a.success[row0 + lane] = succ;
              a.done[row0 + lane] = dn;
            }
          }
        }
        if (++cj == cpe) { cj = 0; ++ep; }
      }
      __syncthreads();
    }
  }
}

}  // namespace earl
