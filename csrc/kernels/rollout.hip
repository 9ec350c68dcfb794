// Fused on-device actor: T steps of {policy MLP forward -> masked softmax -> Philox
// categorical sample -> log-prob -> env physics -> auto-reset} for N vectorised envs
// in ONE launch, writing a time-major SoA rollout into HBM.
//
// This replaces the reference's per-step agent path (request_for_action ->
// TorchScript step() at batch 1 -> safetensors encode -> ZMQ push; SURVEY §3.3,
// agent_zmq.rs:458-571) for the on-GPU actor.  Each wave owns 16 envs; every lane
// of an env column keeps a replica of that env's state in registers, so the whole
// step needs no cross-lane traffic except the two head reductions.
//
// The step itself (env slot, observation tile, forward, draws, episode statistics) is
// actor_step.h; the kernels here add the action heads and their output stores.
#include "actor_step.h"

namespace rrl {

struct RolloutArgs {
  const float* params;
  const float* env_consts;  // continuous kernel only
  int N, T;
  float* state;     // [N][NS]
  int* ep_len;      // [N]
  float* ep_ret;    // [N]
  float* obs_buf;   // [T+1][N][D]
  void* act_buf;    // [T][N] int32 (discrete) / [T][N][A] float (continuous)
  float* logp_buf;  // [T][N]
  float* rew_buf;   // [T][N]
  float* done_buf;  // [T][N]: 0 running, 1 terminal, 2 time-limit truncation (needs tobs_buf)
  float* tobs_buf;  // [T][N][D] pre-reset observation where done == 2, or null (truncation -> 1)
  float* ep_stats;  // [grid][8]: n_done, sum_ret, sumsq_ret, max_ret, min_ret, sum_len
  uint32_t seed_lo, seed_hi;
  uint32_t step_lo, step_hi;  // global step of t = 0 (RNG counter)
  int reset_all;
  int max_steps;
};

template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void rollout_kernel(RolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = 1;
  constexpr int D = Env::D, A = Env::A;
  static_assert(D <= 16, "device envs use one input tile");
  const TileCtx c = tile_ctx(p);
  stage_net<DT, HT>(lds, p.params, D, A, false);
  __syncthreads();

  int* act_buf = static_cast<int*>(p.act_buf);
  EpStats st;

  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.load_or_reset(c, p.reset_all, p.state, p.ep_len, p.ep_ret);

    for (int t = 0; t < p.T; ++t) {
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, c.g, x);
      if (e.valid) store_obs_row<D, DT>(p.obs_buf + base * D, c.g, x);
      float logits[kMaxAct];
      policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), A, logits);
      const CatStats cs = cat_stats(A, logits);
      const uint4 rnd = step_draw(e.envc, gstep, c.key);
      const int a = cat_sample(A, logits, cs.lse, u01(rnd.x));
      const float logp = pick_logit(A, logits, a) - cs.lse;

      bool term;
      const float r = Env::step(e.s, a, term, u01(rnd.y));
      e.advance(r);
      const bool trunc = e.len >= p.max_steps;
      const bool done = term || trunc;
      const bool boot = trunc && !term && p.tobs_buf != nullptr;  // cut path: bootstrap V(s_t+1)
      if (e.valid && c.g == 0) {
        act_buf[base] = a;
        p.logp_buf[base] = logp;
        p.rew_buf[base] = r;
        p.done_buf[base] = boot ? 2.f : (done ? 1.f : 0.f);
      }
      if (boot && e.valid) store_obs<Env>(p.tobs_buf + base * D, c.g, e.s);
      if (done) {
        if (e.valid && c.g == 0) st.add(e.ret, e.len);
        e.end_episode(c, gstep);
      }
    }
    // final observation (bootstrap row T) and persistent env state
    if (e.valid) {
      store_obs<Env>(p.obs_buf + ((size_t)p.T * p.N + e.env) * D, c.g, e.s);
      if (c.g == 0) e.write_back(p.state, p.ep_len, p.ep_ret);
    }
  }
  st.reduce_block(c, lds, p.ep_stats);  // the weights are no longer needed
}

// ------------------------------------------------------------------ small-N variant
// rollout_kernel gives each wave 16 envs and a whole 128x128 layer per step, so a short
// rollout over few envs (the time-to-threshold config: 1,024 envs = 64 tiles) runs 64 long
// serial chains on 16 CUs.  Here a workgroup's WPT = 4 waves share ONE 16-env tile: every
// wave keeps the env replica and the full layer 1 (HT MFMAs), computes HT/WPT output tiles of layer 2 and their partial logits, and the partials meet in LDS
// (double-buffered by step parity: one barrier per step).  All waves then sum the WPT
// partials in the same order, so they draw the same action and step identical env
// replicas; wave 0 writes.  Measured at 1,024 envs x 64 steps: 340 us (rollout_kernel),
// 166 us (4 waves per tile), 187 us (8 waves per tile: the per-step barrier and the
// redundant layer 1 outweigh the shorter layer-2 slice).
template <class Env, int HT, int WPT>
__global__ __launch_bounds__(64 * WPT, 1) void rollout_wide_kernel(RolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = 1;
  using L = LdsNet<DT, HT>;
  constexpr int H = L::H;
  constexpr int D = Env::D, A = Env::A;
  constexpr int QT = HT / WPT;  // layer-2 output tiles per wave
  static_assert(D <= 16 && HT % WPT == 0, "one input tile, layer 2 split over the tile's waves");
  const TileCtx c = tile_ctx(p, true);
  stage_net<DT, HT>(lds, p.params, D, A, false);
  float* part = lds + ((L::floats(A) + 3) & ~3);  // [2 parity][WPT waves][kMaxAct][16 envs]
  __syncthreads();

  const int w = c.wib, j = c.j, g = c.g;
  const int to0 = w * QT;
  const bool writer = (w == 0) && (g == 0);
  int* act_buf = static_cast<int*>(p.act_buf);
  int parity = 0;
  EpStats st;

  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.load_or_reset(c, p.reset_all, p.state, p.ep_len, p.ep_ret);

    for (int t = 0; t < p.T; ++t) {
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, g, x);
      if (e.valid && w == 0) store_obs_row<D, DT>(p.obs_buf + base * D, g, x);
      // the whole of layer 1, this wave's slice of layer 2 and its partial logits
      floatx4 h1[HT], h2[QT];
      layer1_fwd<DT, HT>(lds, x, input_kr_last(D, DT), h1);
      dense_fwd<HT, QT, true>(lds + L::W2 + 16 * to0 * L::S2, L::S2, lds + L::B2 + 16 * to0, h1, h2);
      float* pp = part + parity * (WPT * kMaxAct * 16);
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const float v = head_dot<QT>(lds + L::W3 + a * H + 16 * to0, 0.f, h2);
        if (g == 0) pp[(w * kMaxAct + a) * 16 + j] = v;
      }
      __syncthreads();
      float logits[kMaxAct];
#pragma unroll
      for (int a = 0; a < kMaxAct; ++a) {
        if (a < A) {
          const float* q = pp + a * 16 + j;
          float z = q[0];
#pragma unroll
          for (int v = 1; v < WPT; ++v) z += q[v * kMaxAct * 16];  // same order in every wave
          logits[a] = z + lds[L::B3 + a];
        } else {
          logits[a] = -INFINITY;
        }
      }
      parity ^= 1;
      const CatStats cs = cat_stats(A, logits);
      const uint4 rnd = step_draw(e.envc, gstep, c.key);
      const int a = cat_sample(A, logits, cs.lse, u01(rnd.x));
      const float logp = pick_logit(A, logits, a) - cs.lse;

      bool term;
      const float r = Env::step(e.s, a, term, u01(rnd.y));
      e.advance(r);
      const bool trunc = e.len >= p.max_steps;
      const bool done = term || trunc;
      const bool boot = trunc && !term && p.tobs_buf != nullptr;
      if (e.valid && writer) {
        act_buf[base] = a;
        p.logp_buf[base] = logp;
        p.rew_buf[base] = r;
        p.done_buf[base] = boot ? 2.f : (done ? 1.f : 0.f);
      }
      if (boot && e.valid && w == 0) store_obs<Env>(p.tobs_buf + base * D, g, e.s);
      if (done) {
        if (e.valid && writer) st.add(e.ret, e.len);
        e.end_episode(c, gstep);
      }
    }
    if (e.valid && w == 0) {
      store_obs<Env>(p.obs_buf + ((size_t)p.T * p.N + e.env) * D, g, e.s);
      if (g == 0) e.write_back(p.state, p.ep_len, p.ep_ret);
    }
  }
  if (w == 0) st.reduce_wave(c, p.ep_stats);  // only wave 0 accumulated
}

// ------------------------------------------------------------------ continuous envs
// Same structure for a diagonal-Gaussian policy (PPO / REINFORCE on HalfCheetahSynth):
// mu = MLP(obs), a = mu + exp(log_std) * n with n from Box-Muller over Philox draws
// (tags 0 and 2), logp = sum(-n^2/2 - log_std - log(2 pi)/2) -- the learner's GAUSS_EVAL
// formula.  Env constant tables (system matrices) are staged in LDS after the net.
template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void rollout_cont_kernel(RolloutArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  constexpr int D = Env::D, A = Env::A;
  float* cst = lds + ((L::floats(A) + 3) & ~3);
  const TileCtx c = tile_ctx(p);
  stage_net<DT, HT>(lds, p.params, D, A, true);
  for (int i = threadIdx.x; i < Env::kConsts; i += blockDim.x) cst[i] = p.env_consts[i];
  __syncthreads();

  float* act_buf = static_cast<float*>(p.act_buf);
  EpStats st;

  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.load_or_reset(c, p.reset_all, p.state, p.ep_len, p.ep_ret);

    for (int t = 0; t < p.T; ++t) {
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, c.g, x);
      if (e.valid) store_obs_row<D, DT>(p.obs_buf + base * D, c.g, x);
      float mu[kMaxAct];
      policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), A, mu);
      float nrm[8], act[kMaxAct];
      gauss_noise(e.envc, gstep, c.key, nrm);
      const float logp = gauss_act(A, mu, lds + L::LOGSTD, nrm, act);

      const float r = Env::step(e.s, act, cst, c.key, (uint32_t)e.envc, gstep);
      e.advance(r);
      const bool done = e.len >= p.max_steps;  // this env only truncates (time limit)
      const bool boot = done && p.tobs_buf != nullptr;
      if (e.valid && c.g == 0) {
#pragma unroll
        for (int a = 0; a < A; ++a) act_buf[base * A + a] = act[a];
        p.logp_buf[base] = logp;
        p.rew_buf[base] = r;
        p.done_buf[base] = boot ? 2.f : (done ? 1.f : 0.f);
      }
      if (boot && e.valid) store_obs<Env>(p.tobs_buf + base * D, c.g, e.s);
      if (done) {
        if (e.valid && c.g == 0) st.add(e.ret, e.len);
        e.end_episode(c, gstep);
      }
    }
    if (e.valid) {
      store_obs<Env>(p.obs_buf + ((size_t)p.T * p.N + e.env) * D, c.g, e.s);
      if (c.g == 0) e.write_back(p.state, p.ep_len, p.ep_ret);
    }
  }
  st.reduce_block(c, lds, p.ep_stats);
}

}  // namespace rrl

using namespace rrl;

extern "C" int rrl_env_dims(int env, int* D, int* A, int* NS, int* max_steps) {
  switch (env) {
    case ENV_CARTPOLE: *D = CartPoleEnv::D; *A = CartPoleEnv::A; *NS = CartPoleEnv::NS; *max_steps = CartPoleEnv::kMaxSteps; return 0;
    case ENV_MOUNTAINCAR: *D = MountainCarEnv::D; *A = MountainCarEnv::A; *NS = MountainCarEnv::NS; *max_steps = MountainCarEnv::kMaxSteps; return 0;
    case ENV_ACROBOT: *D = AcrobotEnv::D; *A = AcrobotEnv::A; *NS = AcrobotEnv::NS; *max_steps = AcrobotEnv::kMaxSteps; return 0;
    case ENV_LUNARLANDER:
      *D = LunarLanderSynthEnv::D;
      *A = LunarLanderSynthEnv::A;
      *NS = LunarLanderSynthEnv::NS;
      *max_steps = LunarLanderSynthEnv::kMaxSteps;
      return 0;
    case ENV_HALFCHEETAH:
      *D = HalfCheetahSynthEnv::D;
      *A = HalfCheetahSynthEnv::A;
      *NS = HalfCheetahSynthEnv::NS;
      *max_steps = HalfCheetahSynthEnv::kMaxSteps;
      return 0;
  }
  return -1;
}

// Few envs (at most two 16-env tiles per CU): one workgroup per tile, layer 2 split over
// its waves (rollout_wide_kernel); otherwise 4 tiles per workgroup, one per wave.
static bool rollout_wide(int N, int num_cu) {
  const int tiles = (N + kTileB - 1) / kTileB;
  return tiles <= grid_cap(num_cu);
}

extern "C" int rrl_rollout_grid(int N, int num_cu) {
  const int tiles = (N + kTileB - 1) / kTileB;
  if (rollout_wide(N, num_cu)) return tiles < 1 ? 1 : tiles;
  return tile_stride_grid(N, num_cu);
}

template <class Env, int HT>
static int launch_rollout(const RolloutArgs& a, int grid, bool wide, hipStream_t s) {
  using L = LdsNet<1, HT>;
  if (wide) {
    constexpr int WPT = 4;  // 8 waves per tile (one layer-2 output tile each) measured slower: 187 vs 166 us
    raise_lds_limit<rollout_wide_kernel<Env, HT, WPT>>();
    const size_t bytes = ((size_t)((L::floats(Env::A) + 3) & ~3) + 2 * WPT * kMaxAct * 16) * sizeof(float);
    hipLaunchKernelGGL((rollout_wide_kernel<Env, HT, WPT>), dim3(grid), dim3(64 * WPT), bytes, s, a);
  } else {
    raise_lds_limit<rollout_kernel<Env, HT>>();
    const size_t bytes = (size_t)L::floats(Env::A) * sizeof(float);
    hipLaunchKernelGGL((rollout_kernel<Env, HT>), dim3(grid), dim3(256), bytes, s, a);
  }
  return (int)hipGetLastError();
}

extern "C" int rrl_rollout(int env, const float* params, int N, int T, int H, float* state, int* ep_len,
                           float* ep_ret, float* obs_buf, int* act_buf, float* logp_buf, float* rew_buf,
                           float* done_buf, float* tobs_buf, float* ep_stats, uint64_t seed, uint64_t step0,
                           int reset_all, int max_steps, int num_cu, void* stream) {
  if (N <= 0 || T <= 0) return -2;
  const RolloutArgs a{params, nullptr, N, T, state, ep_len, ep_ret, obs_buf, act_buf, logp_buf, rew_buf, done_buf,
                      tobs_buf, ep_stats, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0,
                      (uint32_t)(step0 >> 32), reset_all, max_steps};
  const int grid = rrl_rollout_grid(N, num_cu);
  const bool wide = rollout_wide(N, num_cu);
  return dispatch_env_h(env, H, [&](auto k) {
    using K = decltype(k);
    return launch_rollout<typename K::Env, K::HT>(a, grid, wide, (hipStream_t)stream);
  });
}

template <class Env, int HT>
static int launch_rollout_cont(const RolloutArgs& a, int grid, hipStream_t s) {
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  const size_t bytes = ((size_t)((L::floats(Env::A) + 3) & ~3) + Env::kConsts) * sizeof(float);
  raise_lds_limit<rollout_cont_kernel<Env, HT>>();
  hipLaunchKernelGGL((rollout_cont_kernel<Env, HT>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

// Continuous-action device envs (env id ENV_HALFCHEETAH); env_consts = env_constants(name).
extern "C" int rrl_rollout_cont(int env, const float* params, const float* env_consts, int N, int T, int H,
                                float* state, int* ep_len, float* ep_ret, float* obs_buf, float* act_buf,
                                float* logp_buf, float* rew_buf, float* done_buf, float* tobs_buf, float* ep_stats,
                                uint64_t seed, uint64_t step0, int reset_all, int max_steps, int num_cu, void* stream) {
  if (N <= 0 || T <= 0 || env != ENV_HALFCHEETAH || env_consts == nullptr) return -2;
  const RolloutArgs a{params, env_consts, N, T, state, ep_len, ep_ret, obs_buf, act_buf, logp_buf, rew_buf, done_buf,
                      tobs_buf, ep_stats, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0,
                      (uint32_t)(step0 >> 32), reset_all, max_steps};
  const int grid = rrl_rollout_grid(N, num_cu);
  hipStream_t s = (hipStream_t)stream;
  if (H == 128) return launch_rollout_cont<HalfCheetahSynthEnv, 8>(a, grid, s);
  if (H == 64) return launch_rollout_cont<HalfCheetahSynthEnv, 4>(a, grid, s);
  return -3;
}
