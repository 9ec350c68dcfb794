// Fused policy evaluation: every one of N vectorised envs runs E complete episodes under fixed
// weights in ONE launch, and only the O(E * N) episode results reach HBM.
//
// The step is the shared one of actor_step.h, the code the rollout kernels run: one 16-env tile
// per wave, the env replica in registers (EnvSlot), the policy MLP on fp32 MFMA out of LDS
// (policy_forward), and, because EnvSlot, step_draw and gauss_noise own the Philox coordinates,
// the rollout's first reset, its action draw and env noise of step t (counter step0 + t) and its
// reset after a finished episode.  tests/test_actor_step_gpu.py holds a sampled trace to the
// rollout bit for bit.  What this file adds:
//   * greedy = 1 takes the lowest index among the maximal logits (a = mu for the Gaussian
//     policy); greedy = 0 draws exactly what the rollout kernels draw.  Env noise is drawn as in
//     training in both modes: greedy removes policy noise, not env noise.
//   * a lane is active while env < N and it has finished fewer than E episodes.  Inactive lanes
//     stay in the wave (the MFMAs need all 64 lanes): only their stores and their env stepping
//     are masked.  A tile's step loop ends when a wave vote finds no active lane; it is bounded
//     by E * max_steps.
//   * outputs are ep_ret / ep_len / ep_code [E][N] (the fp32 running sum ret += r, the length,
//     1 terminal / 2 time limit) and, optionally, a trace of the first Tc steps in the rollout
//     buffers' layout.  No reductions: statistics are torch reductions over the [E][N] tensors.
#include <type_traits>

#include "actor_step.h"

namespace rrl {

struct EvalArgs {
  const float* params;
  const float* env_consts;  // continuous kernel only
  int N, E, Tc;
  float* ep_ret;   // [E][N]
  int* ep_len;     // [E][N]
  int* ep_code;    // [E][N]: 1 terminal, 2 time limit
  float* tr_obs;   // [Tc][N][D] observation the action of step t was computed from, or null
  void* tr_act;    // [Tc][N] int32 (discrete) / [Tc][N][A] float (continuous), or null
  float* tr_rew;   // [Tc][N], or null
  float* tr_done;  // [Tc][N]: 0 running, 1 episode end of either kind, or null
  uint32_t seed_lo, seed_hi;
  uint32_t step_lo, step_hi;  // RNG counter of t = 0
  int greedy;
  int max_steps;
};

// The quantile instance of evaluate_kernel (QR = true) takes NQ behind the block; the others keep theirs.
struct EvalQrArgs : EvalArgs {
  int NQ = 1;  // quantiles per action, Env::A * NQ <= kMaxAct
};

// One lane of an env that finished episode `ep` records it.
template <class Env>
RRL_DEV void store_episode(const EvalArgs& p, const EnvSlot<Env>& e, int ep, int code) {
  const size_t o = (size_t)ep * p.N + e.env;
  p.ep_ret[o] = e.ret;
  p.ep_len[o] = e.len;
  p.ep_code[o] = code;
}

// DUEL = true: a dueling Q-network (heads.h) of Env::A + 1 outputs, scored greedily: the action is the
// argmax of the A advantage outputs.  The host refuses greedy = 0 for it.
// QR = true: a quantile Q-network (heads.h) of Env::A * p.NQ outputs, scored greedily on the quantile sums.
template <class Env, int HT, bool DUEL = false, bool QR = false>
__global__ __launch_bounds__(256, 2) void evaluate_kernel(std::conditional_t<QR, EvalQrArgs, EvalArgs> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = 1;
  constexpr int D = Env::D, A = Env::A;
  static_assert(!(DUEL && QR), "quantiles with the dueling head are not built");
  int AO = A + (DUEL ? 1 : 0);  // outputs of the net
  if constexpr (QR) AO = A * p.NQ;
  static_assert(D <= 16, "device envs use one input tile");
  static_assert(Env::A + 1 <= kMaxAct, "the dueling net has one output more than actions");
  const TileCtx c = tile_ctx(p);
  stage_net<DT, HT>(lds, p.params, D, AO, false);
  __syncthreads();

  const int tmax = p.E * p.max_steps;  // < 2^31: checked by the host entry point
  const bool trace = p.tr_obs != nullptr;
  int* tr_act = static_cast<int*>(p.tr_act);

  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.reset(c, c.step0, false);
    int ep = 0;

    for (int t = 0; t < tmax; ++t) {
      const bool active = e.valid && ep < p.E;
      if (__ballot(active) == 0) break;  // wave-uniform: every lane of the tile has its E episodes
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      const bool tr = trace && active && t < p.Tc;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, c.g, x);
      if (tr) store_obs_row<D, DT>(p.tr_obs + base * D, c.g, x);
      float logits[kMaxAct];
      policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), AO, logits);
      const uint4 rnd = step_draw(e.envc, gstep, c.key);
      int a;
      if constexpr (QR) {
        a = quantile_argmax(A, p.NQ, logits);
      } else if (DUEL || p.greedy) {
        a = argmax_first(A, logits);
      } else {
        const CatStats cs = cat_stats(A, logits);
        a = cat_sample(A, logits, cs.lse, u01(rnd.x));
      }

      if (active) {
        bool term;
        const float r = Env::step(e.s, a, term, u01(rnd.y));
        e.advance(r);
        const bool done = term || e.len >= p.max_steps;
        if (tr && c.g == 0) {
          tr_act[base] = a;
          p.tr_rew[base] = r;
          p.tr_done[base] = done ? 1.f : 0.f;
        }
        if (done) {
          if (c.g == 0) store_episode(p, e, ep, term ? 1 : 2);
          e.end_episode(c, gstep);
          ep += 1;
        }
      }
    }
  }
}

// Diagonal-Gaussian policy on the continuous device env: a = mu + exp(log_std) * n with the
// rollout kernel's Box-Muller draws (gauss_noise), or a = mu when greedy.
template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void evaluate_cont_kernel(EvalArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  constexpr int D = Env::D, A = Env::A;
  float* cst = lds + ((L::floats(A) + 3) & ~3);
  const TileCtx c = tile_ctx(p);
  stage_net<DT, HT>(lds, p.params, D, A, true);
  for (int i = threadIdx.x; i < Env::kConsts; i += blockDim.x) cst[i] = p.env_consts[i];
  __syncthreads();

  const int tmax = p.E * p.max_steps;
  const bool trace = p.tr_obs != nullptr;
  float* tr_act = static_cast<float*>(p.tr_act);

  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.reset(c, c.step0, false);
    int ep = 0;

    for (int t = 0; t < tmax; ++t) {
      const bool active = e.valid && ep < p.E;
      if (__ballot(active) == 0) break;
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      const bool tr = trace && active && t < p.Tc;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, c.g, x);
      if (tr) store_obs_row<D, DT>(p.tr_obs + base * D, c.g, x);
      float mu[kMaxAct];
      policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), A, mu);
      float act[kMaxAct];
      if (p.greedy) {
#pragma unroll
        for (int a = 0; a < kMaxAct; ++a) act[a] = a < A ? mu[a] : 0.f;
      } else {
        float nrm[8];
        gauss_noise(e.envc, gstep, c.key, nrm);
        gauss_act(A, mu, lds + L::LOGSTD, nrm, act);
      }

      if (active) {
        const float r = Env::step(e.s, act, cst, c.key, (uint32_t)e.envc, gstep);
        e.advance(r);
        const bool done = e.len >= p.max_steps;  // this env only truncates (time limit)
        if (tr && c.g == 0) {
#pragma unroll
          for (int a = 0; a < A; ++a) tr_act[base * A + a] = act[a];
          p.tr_rew[base] = r;
          p.tr_done[base] = done ? 1.f : 0.f;
        }
        if (done) {
          if (c.g == 0) store_episode(p, e, ep, 2);
          e.end_episode(c, gstep);
          ep += 1;
        }
      }
    }
  }
}

}  // namespace rrl

using namespace rrl;

namespace {

// One tile per wave.  Few tiles: one-wave workgroups, so the tiles spread over the CUs (a step
// reads the whole of W2 from LDS, and the waves of a workgroup share one CU's LDS bandwidth);
// then 2 and 4 waves per workgroup, and from 8 tiles per CU on the grid is capped at 2 x CUs and
// the waves stride over the tiles like rollout_kernel's.
void eval_geometry(int N, int num_cu, int* grid, int* block) {
  const int tiles = (N + kTileB - 1) / kTileB;
  int wpb = 1;
  while (wpb < 4 && (tiles + wpb - 1) / wpb > grid_cap(num_cu)) wpb *= 2;
  *grid = tile_stride_grid(N, num_cu, wpb);
  *block = 64 * wpb;
}

// -2: a size below 1, trace pointers that are not given together, or a step count past int32
int eval_args_bad(int N, int E, int Tc, int max_steps, const void* tr_obs, const void* tr_act, const void* tr_rew,
                  const void* tr_done) {
  if (N < 1 || E < 1 || max_steps < 1 || Tc < 0) return -2;
  if ((long long)E * (long long)max_steps >= (1ll << 31)) return -2;
  const int given = (tr_obs != nullptr) + (tr_act != nullptr) + (tr_rew != nullptr) + (tr_done != nullptr);
  if (given != 0 && given != 4) return -2;
  if (given == 4 && Tc < 1) return -2;
  return 0;
}

// QR = true: the block with NQ behind it, and the LDS image of Env::A * NQ outputs (-3 past kMaxAct of them).
template <class Env, int HT, bool DUEL = false, bool QR = false>
int launch_evaluate(const std::conditional_t<QR, EvalQrArgs, EvalArgs>& a, int num_cu, hipStream_t s) {
  using L = LdsNet<1, HT>;
  int outputs = Env::A + (DUEL ? 1 : 0);
  if constexpr (QR) {
    if (a.NQ < 1 || Env::A * a.NQ > kMaxAct) return -3;
    outputs = Env::A * a.NQ;
  }
  raise_lds_limit<evaluate_kernel<Env, HT, DUEL, QR>>();
  int grid, block;
  eval_geometry(a.N, num_cu, &grid, &block);
  const size_t bytes = (size_t)L::floats(outputs) * sizeof(float);
  hipLaunchKernelGGL((evaluate_kernel<Env, HT, DUEL, QR>), dim3(grid), dim3(block), bytes, s, a);
  return (int)hipGetLastError();
}

template <class Env, int HT>
int launch_evaluate_cont(const EvalArgs& a, int num_cu, hipStream_t s) {
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  raise_lds_limit<evaluate_cont_kernel<Env, HT>>();
  int grid, block;
  eval_geometry(a.N, num_cu, &grid, &block);
  const size_t bytes = ((size_t)((L::floats(Env::A) + 3) & ~3) + Env::kConsts) * sizeof(float);
  hipLaunchKernelGGL((evaluate_cont_kernel<Env, HT>), dim3(grid), dim3(block), bytes, s, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int rrl_evaluate(int env, const float* params, int N, int E, int Tc, int H, float* ep_ret, int* ep_len,
                            int* ep_code, float* tr_obs, int* tr_act, float* tr_rew, float* tr_done, uint64_t seed,
                            uint64_t step0, int greedy, int max_steps, int dueling, int quantiles, int num_cu,
                            void* stream) {
  if (const int bad = eval_args_bad(N, E, Tc, max_steps, tr_obs, tr_act, tr_rew, tr_done)) return bad;
  if ((dueling || quantiles) && !greedy) return -3;  // softmax-of-Q is not a DQN policy
  if (quantiles < 0 || (quantiles > 0 && dueling)) return -3;
  EvalArgs a{params, nullptr, N, E, Tc, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done,
             (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), greedy ? 1 : 0,
             max_steps};
  return dispatch_env_h(env, H, [&](auto k) {
    using K = decltype(k);
    if (quantiles > 0) {
      EvalQrArgs aq;
      static_cast<EvalArgs&>(aq) = a;
      aq.NQ = quantiles;
      return launch_evaluate<typename K::Env, K::HT, false, true>(aq, num_cu, (hipStream_t)stream);
    }
    if (dueling) return launch_evaluate<typename K::Env, K::HT, true>(a, num_cu, (hipStream_t)stream);
    return launch_evaluate<typename K::Env, K::HT>(a, num_cu, (hipStream_t)stream);
  });
}

extern "C" int rrl_evaluate_cont(int env, const float* params, const float* env_consts, int N, int E, int Tc, int H,
                                 float* ep_ret, int* ep_len, int* ep_code, float* tr_obs, float* tr_act,
                                 float* tr_rew, float* tr_done, uint64_t seed, uint64_t step0, int greedy,
                                 int max_steps, int num_cu, void* stream) {
  if (const int bad = eval_args_bad(N, E, Tc, max_steps, tr_obs, tr_act, tr_rew, tr_done)) return bad;
  if (env != ENV_HALFCHEETAH || env_consts == nullptr) return -3;
  EvalArgs a{params, env_consts, N, E, Tc, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done,
             (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), greedy ? 1 : 0,
             max_steps};
  hipStream_t s = (hipStream_t)stream;
  if (H == 128) return launch_evaluate_cont<HalfCheetahSynthEnv, 8>(a, num_cu, s);
  if (H == 64) return launch_evaluate_cont<HalfCheetahSynthEnv, 4>(a, num_cu, s);
  return -3;
}
