// DQN on the device: an epsilon-greedy fused actor that writes transitions into a replay ring,
// and a kernel that samples the ring, gathers the batch and builds the TD targets from a second
// (target) network, uniformly or through the priority sum tree of prioritised replay (per.hip).  The
// Q-learning gradient head lives in mlp_grad.hip (HEAD_Q_TD).
//
// The actor is the shared step of actor_step.h, the one the rollout and evaluation kernels are built
// from: one 16-env tile per wave, the env replica in registers (EnvSlot), the Q-network on fp32 MFMA
// out of LDS (policy_forward), the step's Philox word (step_draw; .y is the env noise), the resets and
// the episode statistics.  What this kernel adds:
//   * the action: with rnd = step_draw(env, gstep) the env explores iff u01(rnd.z) < epsilon and then
//     takes min(A - 1, floor(u01(rnd.w) * A)); otherwise the lowest index among the maximal Q-values
//     (argmax_first, the evaluation kernels' greedy rule).  rnd.x, the on-policy action draw, is unused.
//   * the output: T slots of a ring of C, obs / nobs / act / rew / done, where nobs is the post-step,
//     pre-reset observation of EVERY step (the bootstrap input of the TD target).  A launch never
//     wraps: C % T == 0, slot0 % T == 0 and slot0 + T <= C, the host advances the cursor.
//
// One form only, the tile-stride one (4 tiles per workgroup, one per wave): see docs/KERNELS.md.
//
// Both kernels have a DUEL instance for the dueling Q-network (heads.h: A + 1 outputs, Q = V + adv - mean adv):
// it stages and evaluates A + 1 outputs, acts on the argmax of the A advantages and bootstraps from the
// dueling Q.  The DUEL = false instances are the kernels as they were.
//
// Both also have a QR instance for the quantile-regression Q-network (heads.h: A * NQ outputs, action-major):
// it stages and evaluates A * NQ outputs, acts on the argmax of the per-action quantile sums and writes NQ
// targets per batch row.  NQ travels in an argument block of its own, so the QR = false instances keep theirs.
#include <type_traits>

#include "actor_step.h"

namespace rrl {

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

struct DqnRolloutQrArgs : DqnRolloutArgs {
  int NQ = 1;  // quantiles per action, Env::A * NQ <= kMaxAct
};

// DUEL = true: the dueling Q-network (heads.h), Env::A + 1 outputs staged and evaluated; the greedy action
// is the argmax of the A advantage outputs.  The draws, the ring writes and the episode slots do not change.
// QR = true: the quantile Q-network, Env::A * p.NQ outputs; the greedy action is the argmax of the quantile sums.
template <class Env, int HT, bool DUEL = false, bool QR = false>
__global__ __launch_bounds__(256, 2) void dqn_rollout_kernel(
    std::conditional_t<QR, DqnRolloutQrArgs, DqnRolloutArgs> p) {
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

  EpStats st;
  for (int tile = c.first; tile < c.ntiles; tile += c.stride) {
    EnvSlot<Env> e(c, tile, p.N);
    e.load_or_reset(c, p.reset_all, p.state, p.ep_len, p.ep_ret);

    for (int t = 0; t < p.T; ++t) {
      const uint64_t gstep = c.step0 + (uint64_t)t;
      const size_t base = (size_t)t * p.N + e.env;
      floatx4 x[DT];
      pack_obs<Env, DT>(e.s, c.g, x);
      if (e.valid) store_obs_row<D, DT>(p.obs + base * D, c.g, x);
      float q[kMaxAct];
      policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), AO, q);
      const uint4 rnd = step_draw(e.envc, gstep, c.key);
      const bool explore = u01(rnd.z) < p.epsilon;
      const int a_rand = min(A - 1, (int)floorf(u01(rnd.w) * (float)A));
      int a;
      if constexpr (QR) a = explore ? a_rand : quantile_argmax(A, p.NQ, q);
      else a = explore ? a_rand : argmax_first(A, q);

      bool term;
      const float r = Env::step(e.s, a, term, u01(rnd.y));
      e.advance(r);
      const bool trunc = e.len >= p.max_steps;
      const bool done = term || trunc;
      if (e.valid) {
        store_obs<Env>(p.nobs + base * D, c.g, e.s);
        if (c.g == 0) {
          p.act[base] = a;
          p.rew[base] = r;
          p.done[base] = term ? 1.f : (trunc ? 2.f : 0.f);
        }
      }
      if (done) {
        if (e.valid && c.g == 0) st.add(e.ret, e.len);
        e.end_episode(c, gstep);
      }
    }
    if (e.valid && c.g == 0) e.write_back(p.state, p.ep_len, p.ep_ret);  // persistent env state
  }
  st.reduce_block(c, lds, p.ep_stats);  // the weights are no longer needed
}

// ------------------------------------------------------------------ sample + gather + TD target
// Batch row b of update u reads ring row r = (philox((b, u, 0), sample_key).x * filled) >> 32 and
//   y[b] = rew[r] + gamma * (done[r] == 1 ? 0 : 1) * Q_tgt(nobs[r], a*),
// a* = the lowest-index argmax of Q_tgt(nobs[r], .) (double_q = 0) or of Q_online(nobs[r], .)
// (double_q = 1).  One route for every H: the workgroup stages ONE net at a time.  With double_q it
// stages the online net, walks its rows and parks a* in y[b] (as bits; the same thread reads it
// back), then re-stages the target net over the same LDS image and walks the same rows again.
// Two H = 128 images (2 x 80 KB) would leave the 160 KB of LDS no margin; see docs/KERNELS.md.
//
// The n-step instance (NSTEP = true) first walks the sampled row r0 forward through the time-major ring,
// same env, next slot (dqn_nstep_walk), and bootstraps from the row `last` the walk ended on:
//   y[b] = G + disc * (done[last] == 1 ? 0 : 1) * Q_tgt(nobs[last], a*),   a* chosen at nobs[last];
// Xb, act_b, idx and the priorities still refer to r0.  The walk happens once per batch row: with
// double_q the online pass parks its length (m - 1) in act_b[b] and G in Xb[b][0], next to a* in y[b]
// (all three are outputs the same thread overwrites in the target pass), and the target pass rebuilds
// last = r0 + (m - 1) * N and disc = gamma^m (the walk's own products, no loads) from them.
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
  // the prioritised instance (PER = true) only
  const float* tree = nullptr;  // [2 * P2] priority sum tree (per.hip)
  uint32_t P2 = 0;              // leaves of the tree, a power of two
  int levels = 0;               // log2(P2)
  float beta = 0.f;
  float* w = nullptr;           // [B] importance weights (filled * leaf / total)^-beta
  int* wmax = nullptr;          // [1] max_b w[b] as float bits, zeroed by the launcher
};

// The n-step instances take their own argument block, so that the one-step kernels keep theirs (and
// with it their code, down to the offsets of the launch's implicit arguments).
struct DqnNStepArgs : DqnTargetArgs {
  int n_step = 1;
  uint32_t N = 1;           // envs per slot: the successor of row r is row r + N (mod filled)
  uint32_t slots = 1;       // filled / N
  uint32_t newest_row = 0;  // newest * N: the rows [newest_row, newest_row + N) end a walk
  int* last = nullptr;      // [B] or null: the row the target bootstrapped from
};

// The quantile instances (QR = true) add NQ to either block: y is [B][NQ].
template <class Base>
struct DqnQrArgs : Base {
  int NQ = 1;
};

template <bool NSTEP, bool QR>
using DqnTargetArgsOf = std::conditional_t<
    QR, DqnQrArgs<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>,
    std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>;

RRL_DEV uint32_t dqn_sample_row(int b, const DqnTargetArgs& p) {
  const uint4 r = philox4x32(make_uint4((uint32_t)b, p.upd_lo, p.upd_hi, 0u), make_uint2(p.key_lo, p.key_hi));
  return (uint32_t)(((uint64_t)r.x * (uint64_t)p.filled) >> 32);
}

template <int HT>
RRL_DEV void dqn_q_values(const float* __restrict__ lds, const float* __restrict__ nobs, size_t r, bool ok, int D,
                          int A, float (&q)[kMaxAct]) {
  const int g = lane_id() >> 4;
  floatx4 x[1];
  const float* row = nobs + r * (size_t)D;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = 4 * k + g;
    x[0][k] = (ok && f < D) ? row[f] : 0.f;
  }
  policy_forward<1, HT>(lds, x, (D + 3) >> 2, A, q);
}

// The prioritised draw: batch row b takes the point m = (b + u) * (total / B) of its own stratum of the
// tree's mass and descends from the root, exactly `levels` steps whatever the tree holds.  Every step is
// one fp32 operation (the numpy oracle per_sample_rows_ref repeats them bit for bit).  The `r > 0` guard
// ends the walk on a leaf of positive priority, hence on a written row, whatever rounding did to m; the
// clamp to [0, filled - 1] keeps a corrupt tree from reading out of bounds.  Counter word 3 = 1: not
// the uniform sampler's draws.
RRL_DEV uint32_t per_sample_row(int b, const DqnTargetArgs& p) {
  const uint4 rnd = philox4x32(make_uint4((uint32_t)b, p.upd_lo, p.upd_hi, 1u), make_uint2(p.key_lo, p.key_hi));
  const float total = p.tree[1];
  const float seg = total / (float)p.B;
  float m = ((float)b + u01(rnd.x)) * seg;
  uint32_t i = 1;
  for (int k = 0; k < p.levels; ++k) {
    const float l = p.tree[2 * (size_t)i], r = p.tree[2 * (size_t)i + 1];
    if (m >= l && r > 0.f) {
      m -= l;
      i = 2 * i + 1;
    } else {
      i = 2 * i;
    }
  }
  const uint32_t row = (i & (p.P2 - 1));  // i - P2 for a walk that started at the root
  return min(row, p.filled - 1u);
}

// The n-step walk from the sampled row r0 < filled: while fewer than n_step steps are summed, the row is
// running (done == 0) and it is not in the newest slot, go to the same env in the next slot (the ring
// wraps at filled) and add its discounted reward.  G (one fused multiply-add) and disc (one product)
// are updated in this order, step by step (ops/dqn.py dqn_nstep_walk_ref repeats the order).  N <= filled
// and last < filled, so last + N < 2^32 and one subtraction wraps it: last stays in [0, filled) whatever
// the ring holds.
struct NStepWalk {
  uint32_t last;
  float G, disc;
  int m;  // steps summed, 1 .. n_step
};

RRL_DEV NStepWalk dqn_nstep_walk(uint32_t r0, const DqnNStepArgs& p) {
  NStepWalk w{r0, p.rew[r0], p.gamma, 1};
  while (w.m < p.n_step && p.done[w.last] == 0.f && w.last - p.newest_row >= p.N) {
    w.last += p.N;
    if (w.last >= p.filled) w.last -= p.filled;
    w.G = fmaf(w.disc, p.rew[w.last], w.G);
    w.disc = w.disc * p.gamma;
    ++w.m;
  }
  return w;
}

// The row a walk of m1 + 1 steps from r0 ended on.  m1 comes back from memory (parked by the online pass):
// the clamp to slots - 1 keeps m1 * N < filled, so the sum stays below 2^32 and the row inside the ring.
RRL_DEV uint32_t dqn_nstep_last(uint32_t r0, uint32_t m1, const DqnNStepArgs& p) {
  uint32_t last = r0 + min(m1, p.slots - 1u) * p.N;
  if (last >= p.filled) last -= p.filled;
  return last;
}

// PER = false: the uniform sampler.  PER = true: the rows come from the priority tree, and the kernel
// also writes the importance weight w[b] and raises *wmax to it (a maximum on the bits of non-negative
// floats).  With double_q the online pass parks the row in idx[b], so the tree is descended once.
// NSTEP = true: the n-step instance (above); NSTEP = false is the one-step kernel, untouched.
// DUEL = true: both nets are dueling (heads.h) with p.A + 1 outputs; a* is the argmax of the selecting
// net's ADVANTAGES and the bootstrap is the dueling Q of the target net at a*.  What is parked between
// the two passes does not change.
// QR = true: both nets are quantile nets (heads.h) with p.A * p.NQ outputs and y is [B][NQ]; a* is the argmax of
// the selecting net's quantile sums, parked in y[b * NQ], and row b receives the NQ quantiles of the target
// net at a*, each through the expression of the scalar kernel.  Everything but y is that of QR = false.
template <int HT, bool PER, bool NSTEP = false, bool DUEL = false, bool QR = false>
__global__ __launch_bounds__(256, 1) void dqn_targets_kernel(DqnTargetArgsOf<NSTEP, QR> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(!(DUEL && QR), "quantiles with the dueling head are not built");
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;
  int AO = p.A + (DUEL ? 1 : 0);  // outputs of the nets
  int NQ = 1;                     // targets per batch row
  if constexpr (QR) {
    NQ = p.NQ;
    AO = p.A * NQ;
  }

  if (p.double_q) {
    stage_net<1, HT>(lds, p.online, p.D, AO, false);
    __syncthreads();
    for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
      const int b = base + 16 * wave + j;
      const bool ok = b < p.B;
      const size_t r = ok ? (PER ? per_sample_row(b, p) : dqn_sample_row(b, p)) : 0;
      float q[kMaxAct];
      if constexpr (NSTEP) {
        NStepWalk w{0u, 0.f, 0.f, 1};
        if (ok) w = dqn_nstep_walk((uint32_t)r, p);
        dqn_q_values<HT>(lds, p.nobs, w.last, ok, p.D, AO, q);
        if (ok && g == 0) {
          p.act_b[b] = w.m - 1;
          p.Xb[(size_t)b * p.D] = w.G;
        }
      } else {
        dqn_q_values<HT>(lds, p.nobs, r, ok, p.D, AO, q);
      }
      if (ok && g == 0) {
        if constexpr (QR) p.y[(size_t)b * NQ] = __int_as_float(quantile_argmax(p.A, NQ, q));
        else p.y[b] = __int_as_float(argmax_first(p.A, q));
        if (PER) p.idx[b] = (int)r;
      }
    }
    __syncthreads();  // every wave is done with the online image
  }
  stage_net<1, HT>(lds, p.target, p.D, AO, false);
  __syncthreads();
  for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
    const int b = base + 16 * wave + j;
    const bool ok = b < p.B;
    size_t r = 0;
    if (ok) {
      if (!PER) r = dqn_sample_row(b, p);
      else if (p.double_q) r = min((uint32_t)p.idx[b], p.filled - 1u);  // parked by this wave's lane g = 0
      else r = per_sample_row(b, p);
    }
    float q[kMaxAct];
    size_t last = r;     // the row the target bootstraps from
    float G = 0.f, disc = p.gamma;
    if constexpr (NSTEP) {
      if (ok) {
        if (p.double_q) {  // parked by this wave's lane g = 0: the walk is not repeated
          const uint32_t m1 = (uint32_t)p.act_b[b];
          last = dqn_nstep_last((uint32_t)r, m1, p);
          for (uint32_t k = 0; k < min(m1, p.slots - 1u); ++k) disc = disc * p.gamma;
          if (g == 0) G = p.Xb[(size_t)b * p.D];  // before this thread overwrites it below
        } else {
          const NStepWalk w = dqn_nstep_walk((uint32_t)r, p);
          last = w.last, G = w.G, disc = w.disc;
        }
      }
    }
    dqn_q_values<HT>(lds, p.nobs, last, ok, p.D, AO, q);
    if (ok) {
      for (int f = g; f < p.D; f += 4) p.Xb[(size_t)b * p.D + f] = p.obs[r * p.D + f];
      if (g == 0) {
        if constexpr (QR) {
          const float boot = (p.done[last] == 1.f) ? 0.f : 1.f;
          // the parked a* comes back from memory: the clamp keeps the quantile index inside the 16 outputs
          const int astar = p.double_q ? min(max(__float_as_int(p.y[(size_t)b * NQ]), 0), p.A - 1)
                                       : quantile_argmax(p.A, NQ, q);
          float rew0 = 0.f;
          if constexpr (!NSTEP) rew0 = p.rew[r];
          for (int i = 0; i < NQ; ++i) {
            const float theta = pick_logit(AO, q, astar * NQ + i);
            if constexpr (NSTEP) p.y[(size_t)b * NQ + i] = G + disc * boot * theta;
            else p.y[(size_t)b * NQ + i] = rew0 + p.gamma * boot * theta;
          }
          if constexpr (NSTEP) {
            if (p.last != nullptr) p.last[b] = (int)last;
          }
        } else {
          const int astar = p.double_q ? __float_as_int(p.y[b]) : argmax_first(p.A, q);
          const float boot = (p.done[last] == 1.f) ? 0.f : 1.f;
          float qstar;
          if constexpr (DUEL) qstar = dueling_q(p.A, q, astar);
          else qstar = pick_logit(p.A, q, astar);
          if constexpr (NSTEP) {
            p.y[b] = G + disc * boot * qstar;
            if (p.last != nullptr) p.last[b] = (int)last;
          } else {
            p.y[b] = p.rew[r] + p.gamma * boot * qstar;
          }
        }
        p.act_b[b] = p.act[r];
        if (p.idx != nullptr) p.idx[b] = (int)r;
        if (PER) {
          const float leaf = p.tree[p.P2 + r], total = p.tree[1];
          // a walk on a sound tree ends on a positive leaf; anything else weighs like the uniform sampler
          const float wb = (leaf > 0.f && total > 0.f) ? powf((float)p.filled * leaf / total, -p.beta) : 1.f;
          p.w[b] = wb;
          atomicMax(p.wmax, __float_as_int(wb));
        }
      }
    }
  }
}

}  // namespace rrl

using namespace rrl;

// 4 tiles per workgroup, one per wave; at most two workgroups per CU, beyond that the waves stride.
extern "C" int rrl_dqn_rollout_grid(int N, int num_cu) { return tile_stride_grid(N, num_cu); }

// QR = true: the block with NQ behind it, and the LDS image of Env::A * NQ outputs (-3 past kMaxAct of them).
template <class Env, int HT, bool DUEL = false, bool QR = false>
static int launch_dqn_rollout(std::conditional_t<QR, DqnRolloutQrArgs, DqnRolloutArgs> a, int slot0, int grid,
                              hipStream_t s) {
  using L = LdsNet<1, HT>;
  int outputs = Env::A + (DUEL ? 1 : 0);
  if constexpr (QR) {
    if (a.NQ < 1 || Env::A * a.NQ > kMaxAct) return -3;
    outputs = Env::A * a.NQ;
  }
  raise_lds_limit<dqn_rollout_kernel<Env, HT, DUEL, QR>>();
  const size_t off = (size_t)slot0 * a.N;
  a.obs += off * Env::D;
  a.nobs += off * Env::D;
  a.act += off;
  a.rew += off;
  a.done += off;
  const size_t bytes = (size_t)L::floats(outputs) * sizeof(float);
  hipLaunchKernelGGL((dqn_rollout_kernel<Env, HT, DUEL, QR>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

extern "C" int rrl_dqn_rollout(int env, const float* params, int N, int T, int H, int C, int slot0, float* state,
                               int* ep_len, float* ep_ret, float* obs, float* nobs, int* act, float* rew,
                               float* done, float* ep_stats, uint64_t seed, uint64_t step0, float epsilon,
                               int reset_all, int max_steps, int dueling, int quantiles, int num_cu,
                               void* stream) {
  if (!params || !state || !ep_len || !ep_ret || !obs || !nobs || !act || !rew || !done || !ep_stats) return -1;
  if (N <= 0 || T <= 0 || C <= 0 || max_steps < 1) return -2;
  if (quantiles < 0 || (quantiles > 0 && dueling)) return -3;
  if (slot0 < 0 || C % T != 0 || slot0 % T != 0 || (long long)slot0 + T > C) return -4;
  DqnRolloutArgs a{params, N, T, state, ep_len, ep_ret, obs, nobs, act, rew, done, ep_stats,
                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), epsilon,
                   reset_all, max_steps};
  const int grid = rrl_dqn_rollout_grid(N, num_cu);
  return dispatch_env_h(env, H, [&](auto k) {
    using K = decltype(k);
    if (quantiles > 0) {
      DqnRolloutQrArgs aq;
      static_cast<DqnRolloutArgs&>(aq) = a;
      aq.NQ = quantiles;
      return launch_dqn_rollout<typename K::Env, K::HT, false, true>(aq, slot0, grid, (hipStream_t)stream);
    }
    if (dueling) return launch_dqn_rollout<typename K::Env, K::HT, true>(a, slot0, grid, (hipStream_t)stream);
    return launch_dqn_rollout<typename K::Env, K::HT>(a, slot0, grid, (hipStream_t)stream);
  });
}

template <int HT, bool PER = false, bool NSTEP = false, bool DUEL = false>
static int launch_dqn_targets(const std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>& a, int grid,
                              hipStream_t s) {
  using L = LdsNet<1, HT>;
  raise_lds_limit<dqn_targets_kernel<HT, PER, NSTEP, DUEL>>();
  const size_t bytes = (size_t)L::floats(a.A + (DUEL ? 1 : 0)) * sizeof(float);
  hipLaunchKernelGGL((dqn_targets_kernel<HT, PER, NSTEP, DUEL>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

// The instance of (H, PER, NSTEP, DUEL); the one-step instances take the base of the block.  The order of the
// cases has no functional meaning: it only keeps the kernels in the order they always had in the code object.
static int dispatch_dqn_targets(const DqnNStepArgs& a, int H, bool per, bool nstep, bool duel, int grid,
                                hipStream_t s) {
  const DqnTargetArgs& one = a;
  switch ((per ? 8 : 0) | (nstep ? 4 : 0) | (duel ? 2 : 0) | (H == 128 ? 1 : 0)) {
    case 3: return launch_dqn_targets<8, false, false, true>(one, grid, s);
    case 2: return launch_dqn_targets<4, false, false, true>(one, grid, s);
    case 1: return launch_dqn_targets<8, false, false, false>(one, grid, s);
    case 0: return launch_dqn_targets<4, false, false, false>(one, grid, s);
    case 7: return launch_dqn_targets<8, false, true, true>(a, grid, s);
    case 6: return launch_dqn_targets<4, false, true, true>(a, grid, s);
    case 5: return launch_dqn_targets<8, false, true, false>(a, grid, s);
    case 4: return launch_dqn_targets<4, false, true, false>(a, grid, s);
    case 11: return launch_dqn_targets<8, true, false, true>(one, grid, s);
    case 10: return launch_dqn_targets<4, true, false, true>(one, grid, s);
    case 9: return launch_dqn_targets<8, true, false, false>(one, grid, s);
    case 8: return launch_dqn_targets<4, true, false, false>(one, grid, s);
    case 15: return launch_dqn_targets<8, true, true, true>(a, grid, s);
    case 14: return launch_dqn_targets<4, true, true, true>(a, grid, s);
    case 13: return launch_dqn_targets<8, true, true, false>(a, grid, s);
    default: return launch_dqn_targets<4, true, true, false>(a, grid, s);
  }
}

// The quantile instances of (H, PER, NSTEP): the same blocks with NQ behind them.
template <int HT, bool PER, bool NSTEP>
static int launch_dqn_targets_qr(const DqnNStepArgs& a, int NQ, int grid, hipStream_t s) {
  using L = LdsNet<1, HT>;
  DqnTargetArgsOf<NSTEP, true> q;
  static_cast<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>&>(q) = a;
  q.NQ = NQ;
  raise_lds_limit<dqn_targets_kernel<HT, PER, NSTEP, false, true>>();
  const size_t bytes = (size_t)L::floats(a.A * NQ) * sizeof(float);
  hipLaunchKernelGGL((dqn_targets_kernel<HT, PER, NSTEP, false, true>), dim3(grid), dim3(256), bytes, s, q);
  return (int)hipGetLastError();
}

static int dispatch_dqn_targets_qr(const DqnNStepArgs& a, int NQ, int H, bool per, bool nstep, int grid,
                                   hipStream_t s) {
  switch ((per ? 4 : 0) | (nstep ? 2 : 0) | (H == 128 ? 1 : 0)) {
    case 0: return launch_dqn_targets_qr<4, false, false>(a, NQ, grid, s);
    case 1: return launch_dqn_targets_qr<8, false, false>(a, NQ, grid, s);
    case 2: return launch_dqn_targets_qr<4, false, true>(a, NQ, grid, s);
    case 3: return launch_dqn_targets_qr<8, false, true>(a, NQ, grid, s);
    case 4: return launch_dqn_targets_qr<4, true, false>(a, NQ, grid, s);
    case 5: return launch_dqn_targets_qr<8, true, false>(a, NQ, grid, s);
    case 6: return launch_dqn_targets_qr<4, true, true>(a, NQ, grid, s);
    default: return launch_dqn_targets_qr<8, true, true>(a, NQ, grid, s);
  }
}

static int dqn_targets_grid(int B, int num_cu) {
  int grid = (B + 63) / 64;
  const int cap = num_cu > 0 ? num_cu : 256;
  return grid > cap ? cap : grid;
}

extern "C" int rrl_dqn_targets(const DqnTargetsCall* c, int num_cu, void* stream) {
  if (!c || !c->target || (c->double_q && !c->online) || !c->obs || !c->nobs || !c->act || !c->rew || !c->done ||
      !c->Xb || !c->act_b || !c->y)
    return -1;
  const bool per = c->tree != nullptr, nstep = c->n_step != 1, duel = c->dueling != 0;
  if (per ? (!c->idx || !c->w || !c->wmax) : (!nstep && c->last && !c->idx)) return -1;
  const long long P2 = per ? rrl_per_tree_leaves(c->L) : 1, most = per ? c->L : 0x7FFFFFFFll;
  if (P2 < 1 || c->filled < 1 || c->filled > most || c->B < 1) return -2;
  if ((c->H != 64 && c->H != 128) || c->D < 1 || c->D > 16 || c->A < 1 || c->A + (duel ? 1 : 0) > kMaxAct) return -3;
  const int NQ = c->quantiles;
  if (NQ < 0 || (NQ > 0 && duel) || (long long)c->A * NQ > kMaxAct) return -3;
  if (c->n_step < 1 || c->N < 1 || c->filled % c->N != 0) return -2;
  if (c->newest < 0 || c->newest >= c->filled / c->N) return -4;
  DqnNStepArgs a;
  static_cast<DqnTargetArgs&>(a) = {c->online, c->target, c->obs, c->nobs, c->act, c->rew, c->done, c->B, c->D, c->A,
                                    (uint32_t)c->filled, c->gamma, c->double_q ? 1 : 0, (uint32_t)c->sample_key,
                                    (uint32_t)(c->sample_key >> 32), (uint32_t)c->update, (uint32_t)(c->update >> 32),
                                    c->Xb, c->act_b, c->y, c->idx};
  a.n_step = c->n_step;
  a.N = (uint32_t)c->N;
  a.slots = (uint32_t)(c->filled / c->N);
  a.newest_row = (uint32_t)c->newest * (uint32_t)c->N;
  a.last = c->last;
  hipStream_t s = (hipStream_t)stream;
  if (per) {
    a.tree = c->tree;
    a.P2 = (uint32_t)P2;
    for (a.levels = 0; (1ll << a.levels) < P2; ++a.levels) {
    }
    a.beta = c->beta;
    a.w = c->w;
    a.wmax = reinterpret_cast<int*>(c->wmax);
    const hipError_t e = hipMemsetAsync(c->wmax, 0, sizeof(float), s);  // +0.0f: below every weight
    if (e != hipSuccess) return (int)e;
  }
  const int grid = dqn_targets_grid(c->B, num_cu);
  const int rc = NQ > 0 ? dispatch_dqn_targets_qr(a, NQ, c->H, per, nstep, grid, s)
                        : dispatch_dqn_targets(a, c->H, per, nstep, duel, grid, s);
  if (rc || nstep || !c->last) return rc;
  // the one-step kernel has no walk: its target bootstraps from the sampled row itself
  return (int)hipMemcpyAsync(c->last, c->idx, (size_t)c->B * sizeof(int), hipMemcpyDeviceToDevice, s);
}
