// Fused policy evaluation: every one of N vectorised envs runs E complete episodes under fixed
// weights in ONE launch, and only the O(E * N) episode results reach HBM.
//
// The step is the rollout kernels' (rollout.hip): one 16-env tile per wave, the env replica in
// registers, the policy MLP on fp32 MFMA out of LDS, the same Philox coordinates for the first
// reset (env, step0, tag 1), the action draw and env noise of step t (counter step0 + t) and the
// reset that follows a finished episode.  What differs:
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
#include "api.h"
#include "common.h"
#include "heads.h"
#include "envs.h"

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

// Lowest index among the maximal logits.
RRL_DEV int argmax_first(int A, const float (&logits)[kMaxAct]) {
  int pick = 0;
  float best = logits[0];
#pragma unroll
  for (int a = 1; a < kMaxAct; ++a)
    if (a < A && logits[a] > best) {
      best = logits[a];
      pick = a;
    }
  return pick;
}

template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void evaluate_kernel(EvalArgs p) {
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
  const int waves_per_block = blockDim.x >> 6;
  const int wave = (threadIdx.x >> 6) + blockIdx.x * waves_per_block;
  const int total_waves = gridDim.x * waves_per_block;
  const int ntiles = (p.N + kTileB - 1) / kTileB;
  const uint2 key = make_uint2(p.seed_lo, p.seed_hi);
  const uint64_t step0 = ((uint64_t)p.step_hi << 32) | p.step_lo;
  const int tmax = p.E * p.max_steps;  // < 2^31: checked by the host entry point
  const bool trace = p.tr_obs != nullptr;
  int* tr_act = static_cast<int*>(p.tr_act);

  for (int tile = wave; tile < ntiles; tile += total_waves) {
    const int env = tile * kTileB + j;
    const bool valid = env < p.N;
    const int envc = valid ? env : p.N - 1;
    float s[NS];
    {
      const uint4 r = philox4x32(make_uint4((uint32_t)envc, (uint32_t)step0, (uint32_t)(step0 >> 32), 1u), key);
      Env::reset(s, r);
    }
    int len = 0, ep = 0;
    float ret = 0.f;

    for (int t = 0; t < tmax; ++t) {
      const bool active = valid && ep < p.E;
      if (__ballot(active) == 0) break;  // wave-uniform: every lane of the tile has its E episodes
      const uint64_t gstep = step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + env;
      const bool tr = trace && active && t < p.Tc;
      floatx4 x[1];
      x[0] = zero4();
#pragma unroll
      for (int f = 0; f < D; ++f) {
        const float o = Env::obs(s, f);
        if ((f & 3) == g) x[0][f >> 2] = o;
      }
      if (tr) {
#pragma unroll
        for (int f = 0; f < D; ++f)
          if ((f & 3) == g) p.tr_obs[base * D + f] = x[0][f >> 2];
      }
      floatx4 h1[HT], h2[HT];
      dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, (D + 3) >> 2);
      dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
      float logits[kMaxAct];
      policy_logits<HT>(lds + L::W3, lds + L::B3, A, H, h2, logits);
      const uint4 rnd = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 0u), key);
      int a;
      if (p.greedy) {
        a = argmax_first(A, logits);
      } else {
        const CatStats cs = cat_stats(A, logits);
        a = cat_sample(A, logits, cs.lse, u01(rnd.x));
      }

      if (active) {
        bool term;
        const float r = Env::step(s, a, term, u01(rnd.y));
        len += 1;
        ret += r;
        const bool done = term || len >= p.max_steps;
        if (tr && g == 0) {
          tr_act[base] = a;
          p.tr_rew[base] = r;
          p.tr_done[base] = done ? 1.f : 0.f;
        }
        if (done) {
          if (g == 0) {
            const size_t o = (size_t)ep * p.N + env;
            p.ep_ret[o] = ret;
            p.ep_len[o] = len;
            p.ep_code[o] = term ? 1 : 2;
          }
          const uint4 rr = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 1u), key);
          Env::reset(s, rr);
          ep += 1;
          len = 0;
          ret = 0.f;
        }
      }
    }
  }
}

// Diagonal-Gaussian policy on the continuous device env: a = mu + exp(log_std) * n with the
// rollout kernel's Box-Muller draws (tags 0 and 2), or a = mu when greedy.
template <class Env, int HT>
__global__ __launch_bounds__(256, 2) void evaluate_cont_kernel(EvalArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  constexpr int H = L::H;
  constexpr int D = Env::D, A = Env::A, NS = Env::NS;
  static_assert(NS == D, "continuous device envs observe their full state");
  const int net_floats = (L::floats(A) + 3) & ~3;
  float* cst = lds + net_floats;
  stage_net<DT, HT>(lds, p.params, D, A, true);
  for (int i = threadIdx.x; i < Env::kConsts; i += blockDim.x) cst[i] = p.env_consts[i];
  __syncthreads();

  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int waves_per_block = blockDim.x >> 6;
  const int wave = (threadIdx.x >> 6) + blockIdx.x * waves_per_block;
  const int total_waves = gridDim.x * waves_per_block;
  const int ntiles = (p.N + kTileB - 1) / kTileB;
  const uint2 key = make_uint2(p.seed_lo, p.seed_hi);
  const uint64_t step0 = ((uint64_t)p.step_hi << 32) | p.step_lo;
  const int kr1 = input_kr_last(D, DT);
  const int tmax = p.E * p.max_steps;
  const bool trace = p.tr_obs != nullptr;
  float* tr_act = static_cast<float*>(p.tr_act);

  for (int tile = wave; tile < ntiles; tile += total_waves) {
    const int env = tile * kTileB + j;
    const bool valid = env < p.N;
    const int envc = valid ? env : p.N - 1;
    float s[NS];
    Env::reset(s, key, (uint32_t)envc, step0);
    int len = 0, ep = 0;
    float ret = 0.f;

    for (int t = 0; t < tmax; ++t) {
      const bool active = valid && ep < p.E;
      if (__ballot(active) == 0) break;
      const uint64_t gstep = step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + env;
      const bool tr = trace && active && t < p.Tc;
      floatx4 x[DT];
#pragma unroll
      for (int q = 0; q < DT; ++q) x[q] = zero4();
#pragma unroll
      for (int f = 0; f < D; ++f)
        if ((f & 3) == g) x[f >> 4][(f >> 2) & 3] = s[f];
      if (tr) {
#pragma unroll
        for (int f = 0; f < D; ++f)
          if ((f & 3) == g) p.tr_obs[base * D + f] = s[f];
      }
      floatx4 h1[HT], h2[HT];
      dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, kr1);
      dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
      float mu[kMaxAct];
      policy_logits<HT>(lds + L::W3, lds + L::B3, A, H, h2, mu);
      float act[kMaxAct];
      if (p.greedy) {
#pragma unroll
        for (int a = 0; a < kMaxAct; ++a) act[a] = a < A ? mu[a] : 0.f;
      } else {
        const uint4 r0 = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 0u), key);
        const uint4 r1 = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 2u), key);
        const float uu[8] = {u01(r0.x), u01(r0.y), u01(r0.z), u01(r0.w), u01(r1.x), u01(r1.y), u01(r1.z), u01(r1.w)};
        float nrm[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float rad = sqrtf(-2.f * __logf(1.f - uu[2 * q]));
          float sn, cs;
          __sincosf(6.283185307179586f * uu[2 * q + 1], &sn, &cs);
          nrm[2 * q] = rad * cs;
          nrm[2 * q + 1] = rad * sn;
        }
#pragma unroll
        for (int a = 0; a < kMaxAct; ++a) {
          act[a] = 0.f;
          if (a < A) act[a] = mu[a] + __expf(lds[L::LOGSTD + a]) * nrm[a < 8 ? a : 0];
        }
      }

      if (active) {
        const float r = Env::step(s, act, cst, key, (uint32_t)envc, gstep);
        len += 1;
        ret += r;
        const bool done = len >= p.max_steps;  // this env only truncates (time limit)
        if (tr && g == 0) {
#pragma unroll
          for (int a = 0; a < A; ++a) tr_act[base * A + a] = act[a];
          p.tr_rew[base] = r;
          p.tr_done[base] = done ? 1.f : 0.f;
        }
        if (done) {
          if (g == 0) {
            const size_t o = (size_t)ep * p.N + env;
            p.ep_ret[o] = ret;
            p.ep_len[o] = len;
            p.ep_code[o] = 2;
          }
          Env::reset(s, key, (uint32_t)envc, gstep + 0x100000000ull);
          ep += 1;
          len = 0;
          ret = 0.f;
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
  const int cap = 2 * (num_cu > 0 ? num_cu : 256);
  int wpb = 1;
  while (wpb < 4 && (tiles + wpb - 1) / wpb > cap) wpb *= 2;
  int g = (tiles + wpb - 1) / wpb;
  if (g > cap) g = cap;
  *grid = g < 1 ? 1 : g;
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

template <class Env, int HT>
int launch_evaluate(const EvalArgs& a, int num_cu, hipStream_t s) {
  using L = LdsNet<1, HT>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)evaluate_kernel<Env, HT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              163840);
    attr = true;
  }
  int grid, block;
  eval_geometry(a.N, num_cu, &grid, &block);
  const size_t bytes = (size_t)L::floats(Env::A) * sizeof(float);
  hipLaunchKernelGGL((evaluate_kernel<Env, HT>), dim3(grid), dim3(block), bytes, s, a);
  return (int)hipGetLastError();
}

template <class Env, int HT>
int launch_evaluate_cont(const EvalArgs& a, int num_cu, hipStream_t s) {
  constexpr int DT = (Env::D + 15) / 16;
  using L = LdsNet<DT, HT>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)evaluate_cont_kernel<Env, HT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    attr = true;
  }
  int grid, block;
  eval_geometry(a.N, num_cu, &grid, &block);
  const size_t bytes = ((size_t)((L::floats(Env::A) + 3) & ~3) + Env::kConsts) * sizeof(float);
  hipLaunchKernelGGL((evaluate_cont_kernel<Env, HT>), dim3(grid), dim3(block), bytes, s, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int rrl_evaluate(int env, const float* params, int N, int E, int Tc, int H, float* ep_ret, int* ep_len,
                            int* ep_code, float* tr_obs, int* tr_act, float* tr_rew, float* tr_done, uint64_t seed,
                            uint64_t step0, int greedy, int max_steps, int num_cu, void* stream) {
  if (const int bad = eval_args_bad(N, E, Tc, max_steps, tr_obs, tr_act, tr_rew, tr_done)) return bad;
  EvalArgs a{params, nullptr, N, E, Tc, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done,
             (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), greedy ? 1 : 0,
             max_steps};
  hipStream_t s = (hipStream_t)stream;
  if (H == 128) {
    switch (env) {
      case ENV_CARTPOLE: return launch_evaluate<CartPoleEnv, 8>(a, num_cu, s);
      case ENV_MOUNTAINCAR: return launch_evaluate<MountainCarEnv, 8>(a, num_cu, s);
      case ENV_ACROBOT: return launch_evaluate<AcrobotEnv, 8>(a, num_cu, s);
      case ENV_LUNARLANDER: return launch_evaluate<LunarLanderSynthEnv, 8>(a, num_cu, s);
    }
  } else if (H == 64) {
    switch (env) {
      case ENV_CARTPOLE: return launch_evaluate<CartPoleEnv, 4>(a, num_cu, s);
      case ENV_MOUNTAINCAR: return launch_evaluate<MountainCarEnv, 4>(a, num_cu, s);
      case ENV_ACROBOT: return launch_evaluate<AcrobotEnv, 4>(a, num_cu, s);
      case ENV_LUNARLANDER: return launch_evaluate<LunarLanderSynthEnv, 4>(a, num_cu, s);
    }
  }
  return -3;
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
