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
//
// Two more targets kernels change the target alone and share the sampling, the walk and the store tail: the Munchausen
// (soft) targets, dqn_soft_targets_kernel, and the lambda-returns, dqn_lambda_targets_kernel, which runs every row of the
// n-step walk through the staged net(s).
#include <type_traits>

#include "actor_step.h"
#include "wide.h"

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

// The categorical instances (TPA > 0) take the support behind the block: Env::A * sup.NA outputs, TPA tiles each.
struct DqnRolloutC51Args : DqnRolloutArgs {
  C51Support sup;
};

template <bool QR, int TPA>
using DqnRolloutArgsOf =
    std::conditional_t<(TPA > 0), DqnRolloutC51Args, std::conditional_t<QR, DqnRolloutQrArgs, DqnRolloutArgs>>;

// DUEL = true: the dueling Q-network (heads.h), Env::A + 1 outputs staged and evaluated; the greedy action
// is the argmax of the A advantage outputs.  The draws, the ring writes and the episode slots do not change.
// QR = true: the quantile Q-network, Env::A * p.NQ outputs; the greedy action is the argmax of the quantile sums.
// TPA > 0: the categorical Q-network on the wide output layer (wide.h), Env::A * p.sup.NA outputs; the greedy action
// is the argmax of the per-action expectations.
template <class Env, int HT, bool DUEL = false, bool QR = false, int TPA = 0>
__global__ __launch_bounds__(256, 2) void dqn_rollout_kernel(DqnRolloutArgsOf<QR, TPA> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DT = 1;
  constexpr int D = Env::D, A = Env::A;
  static_assert(!(DUEL && QR), "quantiles with the dueling head are not built");
  static_assert(TPA == 0 || !(DUEL || QR), "atoms with the dueling or the quantile head are not built");
  int AO = A + (DUEL ? 1 : 0);  // outputs of the net
  if constexpr (QR) AO = A * p.NQ;
  static_assert(D <= 16, "device envs use one input tile");
  static_assert(Env::A + 1 <= kMaxAct, "the dueling net has one output more than actions");
  const TileCtx c = tile_ctx(p);
  if constexpr (TPA > 0) stage_wide<HT>(lds, p.params, D, A, p.sup.NA, TPA);
  else stage_net<DT, HT>(lds, p.params, D, AO, false);
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
      int a_wide = 0;
      if constexpr (TPA > 0) {
        floatx4 h2[HT];
        wide_trunk<HT>(lds, x, input_kr_last(D, DT), h2);
        a_wide = c51_greedy<HT, TPA>(lds, A, p.sup, h2, &q[0]);
      } else {
        policy_forward<DT, HT>(lds, x, input_kr_last(D, DT), AO, q);
      }
      const uint4 rnd = step_draw(e.envc, gstep, c.key);
      const bool explore = u01(rnd.z) < p.epsilon;
      const int a_rand = min(A - 1, (int)floorf(u01(rnd.w) * (float)A));
      int a;
      if constexpr (TPA > 0) a = explore ? a_rand : a_wide;
      else if constexpr (QR) a = explore ? a_rand : quantile_argmax(A, p.NQ, q);
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

// The categorical instances (TPA > 0) add the support: y is [B][sup.NA].
template <class Base>
struct DqnC51Args : Base {
  C51Support sup;
};

template <bool NSTEP, bool QR, int TPA = 0>
using DqnTargetArgsOf = std::conditional_t<
    (TPA > 0), DqnC51Args<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>,
    std::conditional_t<QR, DqnQrArgs<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>,
                       std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>>;

RRL_DEV uint32_t dqn_sample_row(int b, const DqnTargetArgs& p) {
  const uint4 r = philox4x32(make_uint4((uint32_t)b, p.upd_lo, p.upd_hi, 0u), make_uint2(p.key_lo, p.key_hi));
  return (uint32_t)(((uint64_t)r.x * (uint64_t)p.filled) >> 32);
}

// The categorical net's greedy action (or `pick`) at ring row r, its expectation in q[0] and, where keep is given,
// the probabilities of that action (c51_greedy).
template <int HT, int TPA>
RRL_DEV int dqn_c51_greedy(const float* __restrict__ lds, const float* __restrict__ nobs, size_t r, bool ok, int D,
                           int A, const C51Support& sup, float (&q)[kMaxAct], floatx4 (*keep)[TPA] = nullptr,
                           int pick = -1) {
  const int g = lane_id() >> 4;
  floatx4 x[1], h2[HT];
  const float* row = nobs + r * (size_t)D;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = 4 * k + g;
    x[0][k] = (ok && f < D) ? row[f] : 0.f;
  }
  wide_trunk<HT>(lds, x, (D + 3) >> 2, h2);
  return c51_greedy<HT, TPA>(lds, A, sup, h2, &q[0], keep, pick);
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
// TPA > 0: both nets are categorical nets on the wide output layer (wide.h) with p.A * NA outputs, NA = p.sup.NA, and
// y is m [B][NA]: a* is the argmax of the selecting net's expectations, parked in y[b * NA] and clamped as for QR, and
// row b receives the projection (c51_project) of the target net's distribution of a* at nobs[last] through
// Tz_j = G + disc * boot * z_j.  All four lane groups of a row take part (each owns a quarter of the atoms), so what
// lane group 0 parked or read (a*, G) reaches the others by a lane broadcast.  Everything but y is that of TPA = 0.
template <int HT, bool PER, bool NSTEP = false, bool DUEL = false, bool QR = false, int TPA = 0>
__global__ __launch_bounds__(256, 1) void dqn_targets_kernel(DqnTargetArgsOf<NSTEP, QR, TPA> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(!(DUEL && QR), "quantiles with the dueling head are not built");
  static_assert(TPA == 0 || !(DUEL || QR), "atoms with the dueling or the quantile head are not built");
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;
  int AO = p.A + (DUEL ? 1 : 0);  // outputs of the nets
  int NQ = 1;                     // targets per batch row
  if constexpr (QR) {
    NQ = p.NQ;
    AO = p.A * NQ;
  }
  if constexpr (TPA > 0) NQ = p.sup.NA;

  if (p.double_q) {
    if constexpr (TPA > 0) stage_wide<HT>(lds, p.online, p.D, p.A, p.sup.NA, TPA);
    else stage_net<1, HT>(lds, p.online, p.D, AO, false);
    __syncthreads();
    for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
      const int b = base + 16 * wave + j;
      const bool ok = b < p.B;
      const size_t r = ok ? (PER ? per_sample_row(b, p) : dqn_sample_row(b, p)) : 0;
      float q[kMaxAct];
      int a_wide = 0;
      if constexpr (NSTEP) {
        NStepWalk w{0u, 0.f, 0.f, 1};
        if (ok) w = dqn_nstep_walk((uint32_t)r, p);
        if constexpr (TPA > 0) a_wide = dqn_c51_greedy<HT, TPA>(lds, p.nobs, w.last, ok, p.D, p.A, p.sup, q);
        else dqn_q_values<HT>(lds, p.nobs, w.last, ok, p.D, AO, q);
        if (ok && g == 0) {
          p.act_b[b] = w.m - 1;
          p.Xb[(size_t)b * p.D] = w.G;
        }
      } else {
        if constexpr (TPA > 0) a_wide = dqn_c51_greedy<HT, TPA>(lds, p.nobs, r, ok, p.D, p.A, p.sup, q);
        else dqn_q_values<HT>(lds, p.nobs, r, ok, p.D, AO, q);
      }
      if (ok && g == 0) {
        if constexpr (TPA > 0) p.y[(size_t)b * NQ] = __int_as_float(a_wide);
        else if constexpr (QR) p.y[(size_t)b * NQ] = __int_as_float(quantile_argmax(p.A, NQ, q));
        else p.y[b] = __int_as_float(argmax_first(p.A, q));
        if (PER) p.idx[b] = (int)r;
      }
    }
    __syncthreads();  // every wave is done with the online image
  }
  if constexpr (TPA > 0) stage_wide<HT>(lds, p.target, p.D, p.A, p.sup.NA, TPA);
  else stage_net<1, HT>(lds, p.target, p.D, AO, false);
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
    if constexpr (TPA > 0) {
      // every lane of the wave runs this (MFMAs and lane broadcasts); rows past B compute on ring row 0 and store nothing
      if constexpr (!NSTEP) G = p.rew[r];
      else G = __shfl(G, j, 64);  // with double_q lane group 0 read it back
      int pick = -1;
      if (p.double_q) {
        int parked = 0;
        if (ok && g == 0) parked = min(max(__float_as_int(p.y[(size_t)b * NQ]), 0), p.A - 1);
        pick = __shfl(parked, j, 64);
      }
      floatx4 pr[TPA], m[TPA];
      dqn_c51_greedy<HT, TPA>(lds, p.nobs, last, ok, p.D, p.A, p.sup, q, &pr, pick);
      const float boot = (p.done[last] == 1.f) ? 0.f : 1.f;
      c51_project<TPA>(p.sup, G, disc * boot, pr, m);
      if (ok) {
#pragma unroll
        for (int t = 0; t < TPA; ++t) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int i = 16 * t + 4 * g + rr;
            if (i < NQ) p.y[(size_t)b * NQ + i] = m[t][rr];
          }
        }
      }
    } else {
      dqn_q_values<HT>(lds, p.nobs, last, ok, p.D, AO, q);
    }
    if (ok) {
      for (int f = g; f < p.D; f += 4) p.Xb[(size_t)b * p.D + f] = p.obs[r * p.D + f];
      if (g == 0) {
        if constexpr (TPA > 0) {
          if constexpr (NSTEP) {
            if (p.last != nullptr) p.last[b] = (int)last;
          }
        } else if constexpr (QR) {
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

// ------------------------------------------------------------------ Munchausen (soft) targets
// Munchausen RL (Vieillard, Pietquin, Geist 2020) changes only the target.  With q[0..A) the target net's Q-values
// (on a quantile net the MEAN of each action's quantiles: the ascending sum of quantile_sum, then one division by NQ),
// all in fp32, a ascending, with the precise expf / logf:
//   mx = max_a q[a];  d[a] = q[a] - mx;  S = sum_a expf(d[a] / tau);  lse = logf(S)        (S >= 1: the max adds 1)
//   tlp[a] = d[a] - tau * lse   (tau * log pi(a));   pi[a] = expf(d[a] / tau) / S
//   bonus = alpha * clamp(tlp at obs[r0] of act[r0], clip, 0)                               act clamped into [0, A)
//   V     = sum_a pi[a] * (q[a] - tlp[a])                          at nobs[last]            scalar net
//   V_j   = sum_a pi[a] * (theta[a * NQ + j] - tlp[a])             at nobs[last]            quantile net, j < NQ
//   y     = (G + bonus) + disc * boot * V                          G, disc, boot, last: those of dqn_targets_kernel
// The bonus is added once, for the sampled transition, whatever n_step is.  There is no argmax, hence no online pass
// and nothing parked between passes: the target net is staged once and every batch row takes TWO trunk passes
// through that one LDS image, obs[r0] and nobs[last].  They run as one pass over the weights (dense_fwd2): each weight
// fragment is read from LDS once and feeds the MFMA of either row tile, and the two accumulate chains are
// independent, so one covers the other's latency.  The registers that hold the obs[r0] tile for the forward pass
// (feature 4k + g in lane group g) are the ones stored to Xb[b]: the row is read from the ring once.
// Sampling, the walk and every output but y are those of dqn_targets_kernel, bit for bit (the store tail is repeated
// here so that its instances keep their code).
template <class Base>
struct DqnSoftArgs : Base {
  float alpha = 0.f;  // scale of the bonus, in (0, 1]
  float tau = 1.f;    // entropy temperature, > 0
  float clip = -1.f;  // lower clip of tau * log pi, < 0
};

template <bool NSTEP, bool QR>
using DqnSoftArgsOf = std::conditional_t<QR, DqnQrArgs<DqnSoftArgs<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>>,
                                         DqnSoftArgs<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>>>;

// dense_fwd (with the ReLU) for two row tiles at once: the same loads of W, one MFMA per tile and weight fragment.
// Each tile's accumulate order is dense_fwd's, so its result is dense_fwd's bit for bit.
template <int NI, int NO>
RRL_DEV void dense_fwd2(const float* __restrict__ W, int S, const float* __restrict__ b, const floatx4 (&in0)[NI],
                        const floatx4 (&in1)[NI], floatx4 (&out0)[NO], floatx4 (&out1)[NO], int kr_last = 4) {
  const int l = lane_id();
  const int i = l & 15, g = l >> 4;
#pragma unroll
  for (int to = 0; to < NO; ++to) out0[to] = out1[to] = *reinterpret_cast<const floatx4*>(b + 16 * to + 4 * g);
  floatx4 wc[NO], wn[NO];
#pragma unroll
  for (int to = 0; to < NO; ++to) wc[to] = *reinterpret_cast<const floatx4*>(W + (16 * to + i) * S + 4 * g);
#pragma unroll
  for (int ti = 0; ti < NI; ++ti) {
    if (ti + 1 < NI) {
#pragma unroll
      for (int to = 0; to < NO; ++to)
        wn[to] = *reinterpret_cast<const floatx4*>(W + (16 * to + i) * S + 16 * (ti + 1) + 4 * g);
    }
    const int kr = (ti == NI - 1) ? kr_last : 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r < kr) {
#pragma unroll
        for (int to = 0; to < NO; ++to) {
          out0[to] = mfma4(wc[to][r], in0[ti][r], out0[to]);
          out1[to] = mfma4(wc[to][r], in1[ti][r], out1[to]);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (ti + 1 < NI) {
#pragma unroll
      for (int to = 0; to < NO; ++to) wc[to] = wn[to];
    }
  }
#pragma unroll
  for (int to = 0; to < NO; ++to) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      out0[to][r] = fmaxf(out0[to][r], 0.f);
      out1[to][r] = fmaxf(out1[to][r], 0.f);
    }
  }
}

// policy_forward for the two row tiles x0, x1 of one column of rows.
template <int HT>
RRL_DEV void soft_forward2(const float* __restrict__ lds, const floatx4 (&x0)[1], const floatx4 (&x1)[1], int kr_last,
                           int AO, float (&out0)[kMaxAct], float (&out1)[kMaxAct]) {
  using L = LdsNet<1, HT>;
  floatx4 a1[HT], b1[HT], a2[HT], b2[HT];
  dense_fwd2<1, HT>(lds + L::W1, L::S1, lds + L::B1, x0, x1, a1, b1, kr_last);
  dense_fwd2<HT, HT>(lds + L::W2, L::S2, lds + L::B2, a1, b1, a2, b2);
  policy_logits<HT>(lds + L::W3, lds + L::B3, AO, L::H, a2, out0);
  policy_logits<HT>(lds + L::W3, lds + L::B3, AO, L::H, b2, out1);
}

// tlp and pi of one row's AO = A * NQ outputs (NQ = 1: a scalar net), held at every register of the action, so that
// the callers' unrolled walks never index a register array by a variable.  The walk over the 16 registers carries a
// quantile counter, as quantile_sum does: the last register of an action closes its ascending sum, `ends` has a bit
// for each such register, and the max, S and the terms run over those registers in ascending order.
RRL_DEV void soft_terms(int AO, int NQ, float tau, const float (&out)[kMaxAct], float (&tlp)[kMaxAct],
                        float (&pi)[kMaxAct]) {
  float q[kMaxAct], e[kMaxAct];
  uint32_t ends = 0;
  int i = 0;
  float s = 0.f, mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < kMaxAct; ++k) {
    q[k] = 0.f;
    if (k < AO) {
      s = (i == 0) ? out[k] : s + out[k];
      if (++i == NQ) {
        q[k] = s / (float)NQ;
        mx = fmaxf(mx, q[k]);
        ends |= 1u << k;
        i = 0;
      }
    }
  }
  float S = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxAct; ++k) {
    e[k] = 0.f;
    if ((ends >> k) & 1u) {
      e[k] = expf((q[k] - mx) / tau);
      S += e[k];
    }
  }
  const float lse = logf(S);
  float t = 0.f, pr = 0.f;
#pragma unroll
  for (int k = kMaxAct - 1; k >= 0; --k) {  // downwards: an action's registers take the values of its last one
    if ((ends >> k) & 1u) {
      t = (q[k] - mx) - tau * lse;
      pr = e[k] / S;
    }
    tlp[k] = t;
    pi[k] = pr;
  }
}

template <int HT, bool PER, bool NSTEP, bool QR>
__global__ __launch_bounds__(256, 1) void dqn_soft_targets_kernel(DqnSoftArgsOf<NSTEP, QR> p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;
  int NQ = 1;
  if constexpr (QR) NQ = p.NQ;
  const int AO = p.A * NQ;

  stage_net<1, HT>(lds, p.target, p.D, AO, false);
  __syncthreads();
  for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
    const int b = base + 16 * wave + j;
    const bool ok = b < p.B;
    size_t r = 0;
    if (ok) r = PER ? per_sample_row(b, p) : dqn_sample_row(b, p);
    size_t last = r;
    float G = 0.f, disc = p.gamma;
    if (ok) {
      if constexpr (NSTEP) {
        const NStepWalk w = dqn_nstep_walk((uint32_t)r, p);
        last = w.last, G = w.G, disc = w.disc;
      } else {
        G = p.rew[r];
      }
    }
    floatx4 x0[1], x1[1];
    const float* row0 = p.obs + r * (size_t)p.D;
    const float* row1 = p.nobs + last * (size_t)p.D;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int f = 4 * k + g;
      x0[0][k] = (ok && f < p.D) ? row0[f] : 0.f;
      x1[0][k] = (ok && f < p.D) ? row1[f] : 0.f;
    }
    float out0[kMaxAct], out1[kMaxAct];
    soft_forward2<HT>(lds, x0, x1, (p.D + 3) >> 2, AO, out0, out1);

    // the head, replicated in the four lane groups: the bonus from obs[r0], then the soft values from nobs[last]
    float tlp[kMaxAct], pi[kMaxAct];
    soft_terms(AO, NQ, p.tau, out0, tlp, pi);
    const int a0 = ok ? min(max(p.act[r], 0), p.A - 1) : 0;
    float tlp0 = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxAct; ++k)
      if (k == a0 * NQ) tlp0 = tlp[k];
    const float head = G + p.alpha * fminf(fmaxf(tlp0, p.clip), 0.f);
    soft_terms(AO, NQ, p.tau, out1, tlp, pi);
    const float boot = (ok && p.done[last] == 1.f) ? 0.f : 1.f;
    for (int jq = 0; jq < NQ; ++jq) {  // one target live at a time
      float V = 0.f;
      int i = 0;
#pragma unroll
      for (int k = 0; k < kMaxAct; ++k)
        if (k < AO) {
          if (i == jq) V += pi[k] * (out1[k] - tlp[k]);
          if (++i == NQ) i = 0;
        }
      if (ok && g == 0) p.y[(size_t)b * NQ + jq] = head + disc * boot * V;
    }
    if (ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int f = 4 * k + g;
        if (f < p.D) p.Xb[(size_t)b * p.D + f] = x0[0][k];
      }
      if (g == 0) {
        if constexpr (NSTEP) {
          if (p.last != nullptr) p.last[b] = (int)last;
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

// ------------------------------------------------------------------ lambda-return targets
// Peng's Q(lambda) on the replay ring (Kozuno et al. 2021; DQN(lambda), Daley & Amato 2019): the exponentially weighted
// mix of the 1 .. m-step targets along ONE walk.  The walk is dqn_nstep_walk: it visits r_0 = r0, r_1, .., r_{m-1} =
// last (r_{k+1} = r_k + N, wrapped at filled), 1 <= m <= n_step.  At every visited row a*_k is the lowest-index argmax
// of the selecting net at nobs[r_k] (the online net with double_q, else the target net; the advantages of a dueling
// net) and V_k = Q_target(nobs[r_k], a*_k) (the dueling Q of a dueling net).  With lam = q_lambda in [0, 1), all fp32:
//   gl = gamma * lam;  one = 1 - lam;  g1 = gamma * one;  gb = gamma * (done[last] == 1 ? 0 : 1)
//   c = 1;  y = 0
//   for k = 0 .. m - 1:  t = fma(k < m - 1 ? g1 : gb, V_k, rew[r_k]);  y = fma(c, t, y);  c = c * gl
// the forward-order sum  y = sum_k c_k (rew[r_k] + gamma beta_k V_k),  c_k = (gamma lam)^k,  beta_k = 1 - lam before
// the last row and the bootstrap flag on it: nothing per step is stored.  lam -> 1 is the n-step target, lam = 0 the
// one-step one (an intermediate row of a walk is running, so its own bootstrap flag is 1).
//
// How the work is split.  A wave owns 16 batch rows, as in the kernels above, and its lanes walk first: all that is
// kept of a walk is m (the rows follow from r0 and k).  The forward passes then run in lock-step over k: the wave takes
// the steps two at a time, k and k + 1, as the two row tiles of ONE pass over the staged weights (soft_forward2: each
// weight fragment is read from LDS once and feeds the MFMA of either tile, the two accumulate chains cover each
// other's latency), so a walk of m rows costs ceil(m / 2) passes over the LDS image, not m.  The loop ends, for the
// whole wave at once, when no lane has a step left, and runs the one-tile body when no lane has a step k + 1.  A lane
// whose walk is shorter stays in the MFMAs on a zero tile and its visit is skipped; either tile's result is
// policy_forward's bit for bit, so a row's target does not depend on the walks of its neighbours.
//
// double_q: one LDS image at a time, as above.  The online pass runs the same loop and packs a*_k into 4 bits each
// (n_step <= 8 and A <= 16: one word), parks the word in y[b] as bits, m - 1 in act_b[b] and, prioritised, the row in
// idx[b]; the target pass reads them back in lane group 0 (the thread that wrote them), clamps them (m - 1 to the walk
// lengths the ring and n_step allow, each a* into [0, A)), and hands them to the other lane groups by a lane broadcast.
// The walk and the tree descent happen once per batch row.
// Xb, act_b, idx, last, w and wmax are those of dqn_targets_kernel<.., NSTEP = true, ..>, bit for bit.
struct DqnLambdaArgs : DqnNStepArgs {
  float lam = 0.f;  // q_lambda, in [0, 1)
};

// The Q-values of the m rows of one walk, two steps per pass over the LDS image: visit(k, r_k, q) for k < m, ascending.
template <int HT, class Visit>
RRL_DEV void lambda_rows(const float* __restrict__ lds, const DqnLambdaArgs& p, uint32_t r0, int m, int AO,
                         Visit&& visit) {
  const int g = lane_id() >> 4;
  const int kr_last = (p.D + 3) >> 2;
  uint32_t ra = r0;  // r_k; N <= filled and r_k < filled, so one subtraction wraps the sum
  for (int k = 0; k < p.n_step; k += 2) {
    const bool on_a = k < m, on_b = k + 1 < m;
    if (__ballot(on_a) == 0) break;  // wave-uniform: every walk of the tile is through
    uint32_t rb = ra + p.N;
    if (rb >= p.filled) rb -= p.filled;
    floatx4 xa[1], xb[1];
    const float* row_a = p.nobs + (size_t)ra * p.D;
    const float* row_b = p.nobs + (size_t)rb * p.D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 4 * i + g;
      xa[0][i] = (on_a && f < p.D) ? row_a[f] : 0.f;
      xb[0][i] = (on_b && f < p.D) ? row_b[f] : 0.f;
    }
    float qa[kMaxAct], qb[kMaxAct];
    if (__ballot(on_b) != 0) {  // wave-uniform again: all 64 lanes are in the MFMAs of either body
      soft_forward2<HT>(lds, xa, xb, kr_last, AO, qa, qb);
    } else {
      policy_forward<1, HT>(lds, xa, kr_last, AO, qa);
#pragma unroll
      for (int a = 0; a < kMaxAct; ++a) qb[a] = 0.f;
    }
    if (on_a) visit(k, ra, qa);
    if (on_b) visit(k + 1, rb, qb);
    ra = rb + p.N;
    if (ra >= p.filled) ra -= p.filled;
  }
}

template <int HT, bool PER, bool DUEL>
__global__ __launch_bounds__(256, 1) void dqn_lambda_targets_kernel(DqnLambdaArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;
  const int AO = p.A + (DUEL ? 1 : 0);
  const float gl = p.gamma * p.lam;
  const float g1 = p.gamma * (1.f - p.lam);

  if (p.double_q) {
    stage_net<1, HT>(lds, p.online, p.D, AO, false);
    __syncthreads();
    for (int base = blockIdx.x * 64; base < p.B; base += gridDim.x * 64) {
      const int b = base + 16 * wave + j;
      const bool ok = b < p.B;
      uint32_t r = 0;
      int m = 0;  // a row past B visits nothing
      if (ok) {
        r = PER ? per_sample_row(b, p) : dqn_sample_row(b, p);
        m = dqn_nstep_walk(r, p).m;
      }
      uint32_t picks = 0;
      lambda_rows<HT>(lds, p, r, m, AO, [&](int k, uint32_t, const float (&q)[kMaxAct]) {
        picks |= (uint32_t)argmax_first(p.A, q) << (4 * k);
      });
      if (ok && g == 0) {
        p.y[b] = __uint_as_float(picks);
        p.act_b[b] = m - 1;
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
    uint32_t r = 0, picks = 0;
    int m = 0;
    if (p.double_q) {
      // parked by this wave's lane group 0, which reads it back: the walk is not repeated.  m - 1 is clamped to what
      // n_step and the ring allow (so r_k stays inside the ring and 4 k inside the word)
      uint32_t m1 = 0;
      if (ok && g == 0) {
        r = PER ? min((uint32_t)p.idx[b], p.filled - 1u) : dqn_sample_row(b, p);
        m1 = min((uint32_t)p.act_b[b], min((uint32_t)p.n_step, p.slots) - 1u);
        picks = __float_as_uint(p.y[b]);
      }
      r = __shfl(r, j, 64);
      picks = __shfl(picks, j, 64);
      m = ok ? 1 + (int)__shfl(m1, j, 64) : 0;
    } else if (ok) {
      r = PER ? per_sample_row(b, p) : dqn_sample_row(b, p);
      m = dqn_nstep_walk(r, p).m;
    }
    const uint32_t last = ok ? dqn_nstep_last(r, (uint32_t)(m - 1), p) : 0u;
    const float gb = p.gamma * ((ok && p.done[last] == 1.f) ? 0.f : 1.f);
    float c = 1.f, y = 0.f;
    lambda_rows<HT>(lds, p, r, m, AO, [&](int k, uint32_t rk, const float (&q)[kMaxAct]) {
      // a parked a* comes back from memory: the clamp keeps it among the A outputs
      const int astar = p.double_q ? min((int)((picks >> (4 * k)) & 15u), p.A - 1) : argmax_first(p.A, q);
      float V;
      if constexpr (DUEL) V = dueling_q(p.A, q, astar);
      else V = pick_logit(p.A, q, astar);
      const float t = fmaf(k < m - 1 ? g1 : gb, V, p.rew[rk]);
      y = fmaf(c, t, y);
      c = c * gl;
    });
    if (ok) {
      for (int f = g; f < p.D; f += 4) p.Xb[(size_t)b * p.D + f] = p.obs[(size_t)r * p.D + f];
      if (g == 0) {
        p.y[b] = y;
        if (p.last != nullptr) p.last[b] = (int)last;
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

// The categorical instance of (Env, HT, TPA): the block with the support behind it and the wide LDS image.
template <class Env, int HT, int TPA>
static int launch_c51_rollout(DqnRolloutC51Args a, int slot0, int grid, hipStream_t s) {
  raise_lds_limit<dqn_rollout_kernel<Env, HT, false, false, TPA>>();
  const size_t off = (size_t)slot0 * a.N;
  a.obs += off * Env::D;
  a.nobs += off * Env::D;
  a.act += off;
  a.rew += off;
  a.done += off;
  const size_t bytes = (size_t)LdsWide<HT>::floats(Env::A * TPA) * sizeof(float);
  hipLaunchKernelGGL((dqn_rollout_kernel<Env, HT, false, false, TPA>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

extern "C" int rrl_dqn_rollout(int env, const float* params, int N, int T, int H, int C, int slot0, float* state,
                               int* ep_len, float* ep_ret, float* obs, float* nobs, int* act, float* rew,
                               float* done, float* ep_stats, uint64_t seed, uint64_t step0, float epsilon,
                               int reset_all, int max_steps, int dueling, int quantiles, int atoms, float v_min,
                               float v_max, int num_cu, void* stream) {
  if (!params || !state || !ep_len || !ep_ret || !obs || !nobs || !act || !rew || !done || !ep_stats) return -1;
  if (N <= 0 || T <= 0 || C <= 0 || max_steps < 1) return -2;
  if (quantiles < 0 || (quantiles > 0 && dueling)) return -3;
  if (atoms < 0 || (atoms > 0 && (dueling || quantiles > 0))) return -3;
  if (slot0 < 0 || C % T != 0 || slot0 % T != 0 || (long long)slot0 + T > C) return -4;
  DqnRolloutArgs a{params, N, T, state, ep_len, ep_ret, obs, nobs, act, rew, done, ep_stats,
                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step0, (uint32_t)(step0 >> 32), epsilon,
                   reset_all, max_steps};
  const int grid = rrl_dqn_rollout_grid(N, num_cu);
  return dispatch_env_h(env, H, [&](auto k) {
    using K = decltype(k);
    if (atoms > 0) {
      using Env = typename K::Env;
      DqnRolloutC51Args ac;
      static_cast<DqnRolloutArgs&>(ac) = a;
      const int tpa = c51_support(Env::A, atoms, v_min, v_max, &ac.sup);
      return dispatch_tpa<(Env::A <= 2 ? 4 : kMaxWideTiles / Env::A)>(tpa, [&](auto w) {
        return launch_c51_rollout<Env, K::HT, decltype(w)::TPA>(ac, slot0, grid, (hipStream_t)stream);
      });
    }
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
static int launch_quantile_targets(const DqnNStepArgs& a, int NQ, int grid, hipStream_t s) {
  using L = LdsNet<1, HT>;
  DqnTargetArgsOf<NSTEP, true> q;
  static_cast<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>&>(q) = a;
  q.NQ = NQ;
  raise_lds_limit<dqn_targets_kernel<HT, PER, NSTEP, false, true>>();
  const size_t bytes = (size_t)L::floats(a.A * NQ) * sizeof(float);
  hipLaunchKernelGGL((dqn_targets_kernel<HT, PER, NSTEP, false, true>), dim3(grid), dim3(256), bytes, s, q);
  return (int)hipGetLastError();
}

static int dispatch_quantile_targets(const DqnNStepArgs& a, int NQ, int H, bool per, bool nstep, int grid,
                                   hipStream_t s) {
  switch ((per ? 4 : 0) | (nstep ? 2 : 0) | (H == 128 ? 1 : 0)) {
    case 0: return launch_quantile_targets<4, false, false>(a, NQ, grid, s);
    case 1: return launch_quantile_targets<8, false, false>(a, NQ, grid, s);
    case 2: return launch_quantile_targets<4, false, true>(a, NQ, grid, s);
    case 3: return launch_quantile_targets<8, false, true>(a, NQ, grid, s);
    case 4: return launch_quantile_targets<4, true, false>(a, NQ, grid, s);
    case 5: return launch_quantile_targets<8, true, false>(a, NQ, grid, s);
    case 6: return launch_quantile_targets<4, true, true>(a, NQ, grid, s);
    default: return launch_quantile_targets<8, true, true>(a, NQ, grid, s);
  }
}

// The categorical instances of (H, PER, NSTEP, TPA): the same blocks with the support behind them.
template <int HT, bool PER, bool NSTEP, int TPA>
static int launch_c51_targets(const DqnNStepArgs& a, const C51Support& sup, int grid, hipStream_t s) {
  DqnTargetArgsOf<NSTEP, false, TPA> q;
  static_cast<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>&>(q) = a;
  q.sup = sup;
  raise_lds_limit<dqn_targets_kernel<HT, PER, NSTEP, false, false, TPA>>();
  const size_t bytes = (size_t)LdsWide<HT>::floats(a.A * TPA) * sizeof(float);
  hipLaunchKernelGGL((dqn_targets_kernel<HT, PER, NSTEP, false, false, TPA>), dim3(grid), dim3(256), bytes, s, q);
  return (int)hipGetLastError();
}

template <int TPA>
static int dispatch_c51_targets(const DqnNStepArgs& a, const C51Support& sup, int H, bool per, bool nstep, int grid,
                                hipStream_t s) {
  switch ((per ? 4 : 0) | (nstep ? 2 : 0) | (H == 128 ? 1 : 0)) {
    case 0: return launch_c51_targets<4, false, false, TPA>(a, sup, grid, s);
    case 1: return launch_c51_targets<8, false, false, TPA>(a, sup, grid, s);
    case 2: return launch_c51_targets<4, false, true, TPA>(a, sup, grid, s);
    case 3: return launch_c51_targets<8, false, true, TPA>(a, sup, grid, s);
    case 4: return launch_c51_targets<4, true, false, TPA>(a, sup, grid, s);
    case 5: return launch_c51_targets<8, true, false, TPA>(a, sup, grid, s);
    case 6: return launch_c51_targets<4, true, true, TPA>(a, sup, grid, s);
    default: return launch_c51_targets<8, true, true, TPA>(a, sup, grid, s);
  }
}

// The Munchausen instances of (H, PER, NSTEP, QR): the same blocks with alpha, tau and the clip behind them (and NQ
// behind those); NQ = 0 is the scalar net.
template <int HT, bool PER, bool NSTEP, bool QR>
static int launch_soft_targets(const DqnNStepArgs& a, const DqnTargetsCall& c, int grid, hipStream_t s) {
  DqnSoftArgsOf<NSTEP, QR> q;
  static_cast<std::conditional_t<NSTEP, DqnNStepArgs, DqnTargetArgs>&>(q) = a;
  q.alpha = c.munchausen;
  q.tau = c.m_tau;
  q.clip = c.m_clip;
  int outputs = a.A;
  if constexpr (QR) {
    q.NQ = c.quantiles;
    outputs = a.A * c.quantiles;
  }
  raise_lds_limit<dqn_soft_targets_kernel<HT, PER, NSTEP, QR>>();
  const size_t bytes = (size_t)LdsNet<1, HT>::floats(outputs) * sizeof(float);
  hipLaunchKernelGGL((dqn_soft_targets_kernel<HT, PER, NSTEP, QR>), dim3(grid), dim3(256), bytes, s, q);
  return (int)hipGetLastError();
}

template <bool QR>
static int dispatch_soft_targets(const DqnNStepArgs& a, const DqnTargetsCall& c, bool per, bool nstep, int grid,
                                 hipStream_t s) {
  switch ((per ? 4 : 0) | (nstep ? 2 : 0) | (c.H == 128 ? 1 : 0)) {
    case 0: return launch_soft_targets<4, false, false, QR>(a, c, grid, s);
    case 1: return launch_soft_targets<8, false, false, QR>(a, c, grid, s);
    case 2: return launch_soft_targets<4, false, true, QR>(a, c, grid, s);
    case 3: return launch_soft_targets<8, false, true, QR>(a, c, grid, s);
    case 4: return launch_soft_targets<4, true, false, QR>(a, c, grid, s);
    case 5: return launch_soft_targets<8, true, false, QR>(a, c, grid, s);
    case 6: return launch_soft_targets<4, true, true, QR>(a, c, grid, s);
    default: return launch_soft_targets<8, true, true, QR>(a, c, grid, s);
  }
}

// The lambda-return instances of (H, PER, DUEL): the n-step block with q_lambda behind it.
template <int HT, bool PER, bool DUEL>
static int launch_lambda_targets(const DqnNStepArgs& a, float lam, int grid, hipStream_t s) {
  DqnLambdaArgs q;
  static_cast<DqnNStepArgs&>(q) = a;
  q.lam = lam;
  raise_lds_limit<dqn_lambda_targets_kernel<HT, PER, DUEL>>();
  const size_t bytes = (size_t)LdsNet<1, HT>::floats(a.A + (DUEL ? 1 : 0)) * sizeof(float);
  hipLaunchKernelGGL((dqn_lambda_targets_kernel<HT, PER, DUEL>), dim3(grid), dim3(256), bytes, s, q);
  return (int)hipGetLastError();
}

static int dispatch_lambda_targets(const DqnNStepArgs& a, float lam, int H, bool per, bool duel, int grid,
                                   hipStream_t s) {
  switch ((per ? 4 : 0) | (duel ? 2 : 0) | (H == 128 ? 1 : 0)) {
    case 0: return launch_lambda_targets<4, false, false>(a, lam, grid, s);
    case 1: return launch_lambda_targets<8, false, false>(a, lam, grid, s);
    case 2: return launch_lambda_targets<4, false, true>(a, lam, grid, s);
    case 3: return launch_lambda_targets<8, false, true>(a, lam, grid, s);
    case 4: return launch_lambda_targets<4, true, false>(a, lam, grid, s);
    case 5: return launch_lambda_targets<8, true, false>(a, lam, grid, s);
    case 6: return launch_lambda_targets<4, true, true>(a, lam, grid, s);
    default: return launch_lambda_targets<8, true, true>(a, lam, grid, s);
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
  C51Support sup{};
  int tpa = 0;
  if (c->atoms != 0) {
    if (c->atoms < 0 || duel || NQ > 0) return -3;
    tpa = c51_support(c->A, c->atoms, c->v_min, c->v_max, &sup);
    if (tpa == 0) return -3;
  }
  // Munchausen targets: alpha in [0, 1]; alpha > 0 needs tau > 0 and a clip < 0, has no argmax for double_q to select
  // and is built for the plain and the quantile net
  const bool soft = c->munchausen > 0.f;
  if (!(c->munchausen >= 0.f && c->munchausen <= 1.f)) return -3;
  if (soft && (!(c->m_tau > 0.f) || !(c->m_clip < 0.f) || c->double_q || duel || c->atoms != 0)) return -3;
  // lambda-returns: q_lambda in [0, 1]; below 1 the walk has 2 to 8 steps (the parked a* are 4 bits each in one word)
  // and the target is the scalar hard-max one: a mixture of return distributions is not the mean of their quantiles
  // or atoms, and the soft target has no a* to mix
  const bool lam_on = c->q_lambda < 1.f;
  if (!(c->q_lambda >= 0.f && c->q_lambda <= 1.f)) return -3;
  if (lam_on && (c->n_step < 2 || c->n_step > 8 || NQ != 0 || c->atoms != 0 || soft)) return -3;
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
  int rc;
  if (lam_on) {
    rc = dispatch_lambda_targets(a, c->q_lambda, c->H, per, duel, grid, s);
  } else if (soft) {
    rc = NQ > 0 ? dispatch_soft_targets<true>(a, *c, per, nstep, grid, s)
                : dispatch_soft_targets<false>(a, *c, per, nstep, grid, s);
  } else if (tpa > 0) {
    rc = dispatch_tpa<kMaxTpa>(tpa, [&](auto w) {
      return dispatch_c51_targets<decltype(w)::TPA>(a, sup, c->H, per, nstep, grid, s);
    });
  } else {
    rc = NQ > 0 ? dispatch_quantile_targets(a, NQ, c->H, per, nstep, grid, s)
                : dispatch_dqn_targets(a, c->H, per, nstep, duel, grid, s);
  }
  if (rc || nstep || !c->last) return rc;
  // the one-step kernel has no walk: its target bootstraps from the sampled row itself
  return (int)hipMemcpyAsync(c->last, c->idx, (size_t)c->B * sizeof(int), hipMemcpyDeviceToDevice, s);
}
