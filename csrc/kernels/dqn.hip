// DQN on the device: an epsilon-greedy fused actor that writes transitions into a replay ring,
// and a kernel that samples the ring, gathers the batch and builds the TD targets from a second
// (target) network.  The Q-learning gradient head lives in mlp_grad.hip (HEAD_Q_TD).
//
// The actor is the rollout kernels' step (rollout.hip): one 16-env tile per wave, the env replica
// in registers, the Q-network on fp32 MFMA out of LDS, the same Philox coordinates for the env
// noise (rnd.y of tag 0) and the resets (tag 1).  What differs:
//   * the action: with rnd = philox((env, gstep, 0), key) the env explores iff u01(rnd.z) < epsilon
//     and then takes min(A - 1, floor(u01(rnd.w) * A)); otherwise the lowest index among the maximal
//     Q-values (evaluate.hip's greedy convention).  rnd.x, the on-policy kernels' action draw, is unused.
//   * the output: T slots of a ring of C, obs / nobs / act / rew / done, where nobs is the post-step,
//     pre-reset observation of EVERY step (the bootstrap input of the TD target).  A launch never
//     wraps: C % T == 0, slot0 % T == 0 and slot0 + T <= C, the host advances the cursor.
//
// One form only, the tile-stride one (4 tiles per workgroup, one per wave): see docs/KERNELS.md.
#include "api.h"
#include "common.h"
#include "heads.h"
#include "envs.h"

namespace rrl {

// Lowest index among the maximal values (evaluate.hip, reference.greedy_from_logits).
RRL_DEV int dqn_argmax_first(int A, const float (&q)[kMaxAct]) {
  int pick = 0;
  float best = q[0];
#pragma unroll
  for (int a = 1; a < kMaxAct; ++a)
    if (a < A && q[a] > best) {
      best = q[a];
      pick = a;
    }
  return pick;
}

struct DqnRolloutArgs {
  const float* params;
  int N, T;
  float* state;     // [N][NS]
  int* ep_len;      // [N]
  float* ep_ret;    // [N]
  float* obs;       // ring [C][N][D], already offset to slot0
  float* nobs;      // ring [C][N][D]
  int* act;         // ring [C][N]
  float* rew;       // ring [C][N]
  float* done;      // ring [C][N]: 0 running, 1 terminal, 2 time-limit truncation
  float* ep_stats;  // [grid][8]: n_done, sum_ret, sumsq_ret, max_ret, min_ret, sum_len
  uint32_t seed_lo, seed_hi;
  uint32_t step_lo, step_hi;  // global step of t = 0 (RNG counter)
  float epsilon;
  int reset_all;
  int max_steps;
};

template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void dqn_rollout_kernel(DqnRolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = 1;
  using L = LdsNet<DT, HT>;
  constexpr int H = L::H;
  constexpr int D = Env::D, A = Env::A, NS = Env::NS;
  static_assert(D <= 16, "device envs use one input tile");
  stage_net<DT, HT>(lds, p.params, D, A, false);
  __syncthreads();

  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const int wave = wave_in_block + blockIdx.x * waves_per_block;
  const int total_waves = gridDim.x * waves_per_block;
  const int ntiles = (p.N + kTileB - 1) / kTileB;
  const uint2 key = make_uint2(p.seed_lo, p.seed_hi);
  const uint64_t step0 = ((uint64_t)p.step_hi << 32) | p.step_lo;

  float st_n = 0.f, st_sum = 0.f, st_sq = 0.f, st_max = -INFINITY, st_min = INFINITY, st_len = 0.f;

  for (int tile = wave; tile < ntiles; tile += total_waves) {
    const int env = tile * kTileB + j;
    const bool valid = env < p.N;
    const int envc = valid ? env : p.N - 1;
    float s[NS];
    int len;
    float ret;
    if (p.reset_all) {
      const uint4 r = philox4x32(make_uint4((uint32_t)envc, (uint32_t)step0, (uint32_t)(step0 >> 32), 1u), key);
      Env::reset(s, r);
      len = 0;
      ret = 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] = p.state[(size_t)envc * NS + k];
      len = p.ep_len[envc];
      ret = p.ep_ret[envc];
    }

    for (int t = 0; t < p.T; ++t) {
      const uint64_t gstep = step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + env;
      floatx4 x[1];
      x[0] = zero4();
#pragma unroll
      for (int f = 0; f < D; ++f) {
        const float o = Env::obs(s, f);
        if ((f & 3) == g) x[0][f >> 2] = o;
      }
      if (valid) {
#pragma unroll
        for (int f = 0; f < D; ++f)
          if ((f & 3) == g) p.obs[base * D + f] = x[0][f >> 2];
      }
      floatx4 h1[HT], h2[HT];
      dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, (D + 3) >> 2);
      dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
      float q[kMaxAct];
      policy_logits<HT>(lds + L::W3, lds + L::B3, A, H, h2, q);
      const uint4 rnd = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 0u), key);
      const bool explore = u01(rnd.z) < p.epsilon;
      const int a_rand = min(A - 1, (int)floorf(u01(rnd.w) * (float)A));
      const int a = explore ? a_rand : dqn_argmax_first(A, q);

      bool term;
      const float r = Env::step(s, a, term, u01(rnd.y));
      len += 1;
      ret += r;
      const bool trunc = len >= p.max_steps;
      const bool done = term || trunc;
      if (valid) {
#pragma unroll
        for (int f = 0; f < D; ++f)
          if ((f & 3) == g) p.nobs[base * D + f] = Env::obs(s, f);
        if (g == 0) {
          p.act[base] = a;
          p.rew[base] = r;
          p.done[base] = term ? 1.f : (trunc ? 2.f : 0.f);
        }
      }
      if (done) {
        if (valid && g == 0) {
          st_n += 1.f;
          st_sum += ret;
          st_sq += ret * ret;
          st_max = fmaxf(st_max, ret);
          st_min = fminf(st_min, ret);
          st_len += (float)len;
        }
        const uint4 rr = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 1u), key);
        Env::reset(s, rr);
        len = 0;
        ret = 0.f;
      }
    }
    // persistent env state
    if (valid && g == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) p.state[(size_t)env * NS + k] = s[k];
      p.ep_len[env] = len;
      p.ep_ret[env] = ret;
    }
  }

  // workgroup reduction of episode statistics
  __syncthreads();
  float* red = lds;  // weights no longer needed
  float v0 = wave_sum(st_n), v1 = wave_sum(st_sum), v2 = wave_sum(st_sq), v5 = wave_sum(st_len);
  float v3 = st_max, v4 = st_min;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    v3 = fmaxf(v3, __shfl_xor(v3, o, 64));
    v4 = fminf(v4, __shfl_xor(v4, o, 64));
  }
  if (l == 0) {
    red[wave_in_block * 8 + 0] = v0;
    red[wave_in_block * 8 + 1] = v1;
    red[wave_in_block * 8 + 2] = v2;
    red[wave_in_block * 8 + 3] = v3;
    red[wave_in_block * 8 + 4] = v4;
    red[wave_in_block * 8 + 5] = v5;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    float v = red[k];
    for (int w = 1; w < waves_per_block; ++w) {
      const float u = red[w * 8 + k];
      v = (k == 3) ? fmaxf(v, u) : (k == 4) ? fminf(v, u) : v + u;
    }
    p.ep_stats[blockIdx.x * 8 + k] = v;
  }
}

// ------------------------------------------------------------------ sample + gather + TD target
// Batch row b of update u reads ring row r = (philox((b, u, 0), sample_key).x * filled) >> 32 and
//   y[b] = rew[r] + gamma * (done[r] == 1 ? 0 : 1) * Q_tgt(nobs[r], a*),
// a* = the lowest-index argmax of Q_tgt(nobs[r], .) (double_q = 0) or of Q_online(nobs[r], .)
// (double_q = 1).  One route for every H: the workgroup stages ONE net at a time.  With double_q it
// stages the online net, walks its rows and parks a* in y[b] (as bits; the same thread reads it
// back), then re-stages the target net over the same LDS image and walks the same rows again.
// Two H = 128 images (2 x 80 KB) would leave the 160 KB of LDS no margin; see docs/KERNELS.md.
struct DqnTargetArgs {
  const float* online;
  const float* target;
  const float* obs;   // ring rows [filled][D]
  const float* nobs;
  const int* act;
  const float* rew;
  const float* done;
  int B, D, A;
  uint32_t filled;
  float gamma;
  int double_q;
  uint32_t key_lo, key_hi;
  uint32_t upd_lo, upd_hi;
  float* Xb;    // [B][D]
  int* act_b;   // [B]
  float* y;     // [B]
  int* idx;     // [B] or null
};

RRL_DEV uint32_t dqn_sample_row(int b, const DqnTargetArgs& p) {
  const uint4 r = philox4x32(make_uint4((uint32_t)b, p.upd_lo, p.upd_hi, 0u), make_uint2(p.key_lo, p.key_hi));
  return (uint32_t)(((uint64_t)r.x * (uint64_t)p.filled) >> 32);
}

template <int HT>
RRL_DEV void dqn_q_values(const float* __restrict__ lds, const float* __restrict__ nobs, size_t r, bool ok, int D,
                          int A, float (&q)[kMaxAct]) {
  using L = LdsNet<1, HT>;
  const int g = lane_id() >> 4;
  floatx4 x[1];
  const float* row = nobs + r * (size_t)D;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = 4 * k + g;
    x[0][k] = (ok && f < D) ? row[f] : 0.f;
  }
  floatx4 h1[HT], h2[HT];
  dense_fwd<1, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, (D + 3) >> 2);
  dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
  policy_logits<HT>(lds + L::W3, lds + L::B3, A, L::H, h2, q);
}

template <int HT>
__global__ __launch_bounds__(256, 1) void dqn_targets_kernel(DqnTargetArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;

  if (p.double_q) {
    stage_net<1, HT>(lds, p.online, p.D, p.A, false);
    __syncthreads();
    for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
      const int b = base + 16 * wave + j;
      const bool ok = b < p.B;
      const size_t r = ok ? dqn_sample_row(b, p) : 0;
      float q[kMaxAct];
      dqn_q_values<HT>(lds, p.nobs, r, ok, p.D, p.A, q);
      if (ok && g == 0) p.y[b] = __int_as_float(dqn_argmax_first(p.A, q));
    }
    __syncthreads();  // every wave is done with the online image
  }
  stage_net<1, HT>(lds, p.target, p.D, p.A, false);
  __syncthreads();
  for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
    const int b = base + 16 * wave + j;
    const bool ok = b < p.B;
    const size_t r = ok ? dqn_sample_row(b, p) : 0;
    float q[kMaxAct];
    dqn_q_values<HT>(lds, p.nobs, r, ok, p.D, p.A, q);
    if (ok) {
      for (int f = g; f < p.D; f += 4) p.Xb[(size_t)b * p.D + f] = p.obs[r * p.D + f];
      if (g == 0) {
        const int astar = p.double_q ? __float_as_int(p.y[b]) : dqn_argmax_first(p.A, q);
        const float boot = (p.done[r] == 1.f) ? 0.f : 1.f;
        p.y[b] = p.rew[r] + p.gamma * boot * pick_logit(p.A, q, astar);
        p.act_b[b] = p.act[r];
        if (p.idx != nullptr) p.idx[b] = (int)r;
      }
    }
  }
}

}  // namespace rrl

using namespace rrl;

// 4 tiles per workgroup, one per wave; at most two workgroups per CU, beyond that the waves stride.
extern "C" int rrl_dqn_rollout_grid(int N, int num_cu) {
  const int tiles = (N + kTileB - 1) / kTileB;
  int grid = (tiles + 3) / 4;
  const int cap = 2 * (num_cu > 0 ? num_cu : 256);
  if (grid > cap) grid = cap;
  return grid < 1 ? 1 : grid;
}

template <class Env, int HT>
static int launch_dqn_rollout(DqnRolloutArgs a, int slot0, int grid, hipStream_t s) {
  using L = LdsNet<1, HT>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dqn_rollout_kernel<Env, HT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              163840);
    attr = true;
  }
  const size_t off = (size_t)slot0 * a.N;
  a.obs += off * Env::D;
  a.nobs += off * Env::D;
  a.act += off;
  a.rew += off;
  a.done += off;
  const size_t bytes = (size_t)L::floats(Env::A) * sizeof(float);
  hipLaunchKernelGGL((dqn_rollout_kernel<Env, HT>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

extern "C" int rrl_dqn_rollout(int env, const float* params, int N, int T, int H, int C, int slot0, float* state,
                               int* ep_len, float* ep_ret, float* obs, float* nobs, int* act, float* rew,
                               float* done, float* ep_stats, uint64_t seed, uint64_t step0, float epsilon,
                               int reset_all, int max_steps, int num_cu, void* stream) {
  if (!params || !state || !ep_len || !ep_ret || !obs || !nobs || !act || !rew || !done || !ep_stats) return -1;
  if (N <= 0 || T <= 0 || C <= 0 || max_steps < 1) return -2;
  if (slot0 < 0 || C % T != 0 || slot0 % T != 0 || (long long)slot0 + T > C) return -4;
  DqnRolloutArgs a{params, N, T, state, ep_len, ep_ret, obs, nobs, act, rew, done, ep_stats,
                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), epsilon,
                   reset_all, max_steps};
  const int grid = rrl_dqn_rollout_grid(N, num_cu);
  hipStream_t s = (hipStream_t)stream;
  if (H == 128) {
    switch (env) {
      case ENV_CARTPOLE: return launch_dqn_rollout<CartPoleEnv, 8>(a, slot0, grid, s);
      case ENV_MOUNTAINCAR: return launch_dqn_rollout<MountainCarEnv, 8>(a, slot0, grid, s);
      case ENV_ACROBOT: return launch_dqn_rollout<AcrobotEnv, 8>(a, slot0, grid, s);
      case ENV_LUNARLANDER: return launch_dqn_rollout<LunarLanderSynthEnv, 8>(a, slot0, grid, s);
    }
  } else if (H == 64) {
    switch (env) {
      case ENV_CARTPOLE: return launch_dqn_rollout<CartPoleEnv, 4>(a, slot0, grid, s);
      case ENV_MOUNTAINCAR: return launch_dqn_rollout<MountainCarEnv, 4>(a, slot0, grid, s);
      case ENV_ACROBOT: return launch_dqn_rollout<AcrobotEnv, 4>(a, slot0, grid, s);
      case ENV_LUNARLANDER: return launch_dqn_rollout<LunarLanderSynthEnv, 4>(a, slot0, grid, s);
    }
  }
  return -3;
}

template <int HT>
static int launch_dqn_targets(const DqnTargetArgs& a, int grid, hipStream_t s) {
  using L = LdsNet<1, HT>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dqn_targets_kernel<HT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              163840);
    attr = true;
  }
  const size_t bytes = (size_t)L::floats(a.A) * sizeof(float);
  hipLaunchKernelGGL((dqn_targets_kernel<HT>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

extern "C" int rrl_dqn_targets(const float* online, const float* target, const float* obs, const float* nobs,
                               const int* act, const float* rew, const float* done, long long filled, int B, int D,
                               int A, int H, float gamma, int double_q, uint64_t sample_key, uint64_t update,
                               float* Xb, int* act_b, float* y, int* idx, int num_cu, void* stream) {
  if (!target || (double_q && !online) || !obs || !nobs || !act || !rew || !done || !Xb || !act_b || !y) return -1;
  if (filled < 1 || filled > 0x7FFFFFFFll || B < 1) return -2;
  if ((H != 64 && H != 128) || D < 1 || D > 16 || A < 1 || A > kMaxAct) return -3;
  DqnTargetArgs a{online, target, obs, nobs, act, rew, done, B, D, A, (uint32_t)filled, gamma, double_q ? 1 : 0,
                  (uint32_t)sample_key, (uint32_t)(sample_key >> 32), (uint32_t)update, (uint32_t)(update >> 32),
                  Xb, act_b, y, idx};
  int grid = (B + 63) / 64;
  const int cap = num_cu > 0 ? num_cu : 256;
  if (grid > cap) grid = cap;
  hipStream_t s = (hipStream_t)stream;
  return H == 128 ? launch_dqn_targets<8>(a, grid, s) : launch_dqn_targets<4>(a, grid, s);
}
