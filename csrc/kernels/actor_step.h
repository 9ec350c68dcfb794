// The fused device actor's step, once.  rollout.hip, evaluate.hip and dqn.hip assemble their
// kernels from these pieces, so the same Philox coordinates, the same draws, the same resets and
// the same episode bookkeeping hold in all of them by construction:
//
//   TileCtx        lane / wave / tile indices, the Philox key and the step counter of t = 0
//   EnvSlot<Env>   one env replica in registers: load-or-reset, episode end, persistent write-back
//   pack_obs / store_obs_row   the interleaved observation tile and its one row store
//   policy_forward the MLP out of LDS (layer1_fwd alone for the kernel that splits layer 2)
//   step_draw / gauss_noise / gauss_act   the policy's random words
//   EpStats        the six episode statistics and their reduction into a [grid][8] row
//
// and, for the host side, dispatch_env_h, raise_lds_limit and tile_stride_grid.
#pragma once
#include "api.h"
#include "common.h"
#include "heads.h"
#include "envs.h"

namespace rrl {

// ---------------------------------------------------------------- tile context
struct TileCtx {
  int l, j, g;        // lane, env column (lane & 15), lane group (lane >> 4)
  int wib, wpb;       // wave in the workgroup, waves per workgroup
  int first, stride;  // this wave's first tile and its stride over the tiles
  int ntiles;
  uint2 key;
  uint64_t step0;     // global step of t = 0 (RNG counter)
};

// P: any argument struct with N, seed_lo/hi and step_lo/hi.  wide = false: one 16-env tile per
// wave, the waves of the grid stride over the tiles; wide = true: one tile per workgroup.
template <class P>
RRL_DEV TileCtx tile_ctx(const P& p, bool wide = false) {
  TileCtx c;
  c.l = lane_id();
  c.j = c.l & 15;
  c.g = c.l >> 4;
  c.wib = threadIdx.x >> 6;
  // the launched block size, read straight from the kernel's implicit arguments: blockDim.x
  // here compiled to a select between two addresses and a vector load on the kernel's critical path
  c.wpb = __builtin_amdgcn_workgroup_size_x() >> 6;
  c.first = wide ? blockIdx.x : c.wib + blockIdx.x * c.wpb;
  c.stride = wide ? gridDim.x : gridDim.x * c.wpb;
  c.ntiles = (p.N + kTileB - 1) / kTileB;
  c.key = make_uint2(p.seed_lo, p.seed_hi);
  c.step0 = ((uint64_t)p.step_hi << 32) | p.step_lo;
  return c;
}

// ---------------------------------------------------------------- env slot
// Lanes past N replicate env N - 1 (the MFMAs need all 64 lanes); `valid` masks their stores.
template <class Env>
struct EnvSlot {
  int env;
  bool valid;
  int envc;
  float s[Env::NS];
  int len;
  float ret;

  RRL_DEV EnvSlot(const TileCtx& c, int tile, int N)
      : env(tile * kTileB + c.j), valid(env < N), envc(valid ? env : N - 1) {}

  RRL_DEV void reset(const TileCtx& c, uint64_t step, bool after_episode) {
    env_reset<Env>(s, c.key, (uint32_t)envc, step, after_episode);
    len = 0;
    ret = 0.f;
  }
  RRL_DEV void load_or_reset(const TileCtx& c, int reset_all, const float* state, const int* ep_len,
                             const float* ep_ret) {
    if (reset_all) {
      reset(c, c.step0, false);
    } else {
#pragma unroll
      for (int k = 0; k < Env::NS; ++k) s[k] = state[(size_t)envc * Env::NS + k];
      len = ep_len[envc];
      ret = ep_ret[envc];
    }
  }
  RRL_DEV void advance(float r) {
    len += 1;
    ret += r;
  }
  RRL_DEV void end_episode(const TileCtx& c, uint64_t gstep) { reset(c, gstep, true); }
  // one lane of a valid env calls this
  RRL_DEV void write_back(float* state, int* ep_len, float* ep_ret) const {
#pragma unroll
    for (int k = 0; k < Env::NS; ++k) state[(size_t)env * Env::NS + k] = s[k];
    ep_len[env] = len;
    ep_ret[env] = ret;
  }
};

// ---------------------------------------------------------------- observations
// Interleaved layout: feature f of env j lives in lane group f & 3, register (f >> 2) & 3 of
// tile f >> 4 (so the 4 CartPole features are ONE MFMA k-step).
template <class Env, int DT>
RRL_DEV void pack_obs(const float (&s)[Env::NS], int g, floatx4 (&x)[DT]) {
#pragma unroll
  for (int q = 0; q < DT; ++q) x[q] = zero4();
#pragma unroll
  for (int f = 0; f < Env::D; ++f) {
    const float o = Env::obs(s, f);
    if ((f & 3) == g) x[f >> 4][(f >> 2) & 3] = o;
  }
}
// The lane groups of one env write its D-float row from a packed tile.
template <int D, int DT>
RRL_DEV void store_obs_row(float* __restrict__ row, int g, const floatx4 (&x)[DT]) {
#pragma unroll
  for (int f = 0; f < D; ++f)
    if ((f & 3) == g) row[f] = x[f >> 4][(f >> 2) & 3];
}
// The same row straight from the state (no tile is needed afterwards).
template <class Env>
RRL_DEV void store_obs(float* __restrict__ row, int g, const float (&s)[Env::NS]) {
#pragma unroll
  for (int f = 0; f < Env::D; ++f)
    if ((f & 3) == g) row[f] = Env::obs(s, f);
}

// ---------------------------------------------------------------- policy forward
template <int DT, int HT>
RRL_DEV void layer1_fwd(const float* __restrict__ lds, const floatx4 (&x)[DT], int kr_last, floatx4 (&h1)[HT]) {
  using L = LdsNet<DT, HT>;
  dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, kr_last);
}
// out[a] = logit / mean / Q-value a of this lane's env (every lane of the column has all A).
template <int DT, int HT>
RRL_DEV void policy_forward(const float* __restrict__ lds, const floatx4 (&x)[DT], int kr_last, int A,
                            float (&out)[kMaxAct]) {
  using L = LdsNet<DT, HT>;
  floatx4 h1[HT], h2[HT];
  layer1_fwd<DT, HT>(lds, x, kr_last, h1);
  dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
  policy_logits<HT>(lds + L::W3, lds + L::B3, A, L::H, h2, out);
}

// ---------------------------------------------------------------- random words of a step
// The policy's word of step gstep: .x the categorical draw, .y the env's noise, .z / .w the
// epsilon-greedy flag and random action.
RRL_DEV uint4 step_draw(int envc, uint64_t gstep, uint2 key) {
  return philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 0u), key);
}
// Eight standard normals: Box-Muller over the step's word and the word at tag 2.
RRL_DEV void gauss_noise(int envc, uint64_t gstep, uint2 key, float (&nrm)[8]) {
  const uint4 r0 = step_draw(envc, gstep, key);
  const uint4 r1 = philox4x32(make_uint4((uint32_t)envc, (uint32_t)gstep, (uint32_t)(gstep >> 32), 2u), key);
  const float uu[8] = {u01(r0.x), u01(r0.y), u01(r0.z), u01(r0.w), u01(r1.x), u01(r1.y), u01(r1.z), u01(r1.w)};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float rad = sqrtf(-2.f * __logf(1.f - uu[2 * q]));
    float sn, cs;
    __sincosf(6.283185307179586f * uu[2 * q + 1], &sn, &cs);
    nrm[2 * q] = rad * cs;
    nrm[2 * q + 1] = rad * sn;
  }
}
// act = mu + exp(log_std) * n; returns log N(act; mu, sigma) summed over the A dims (the
// learner's GAUSS_EVAL formula).
RRL_DEV float gauss_act(int A, const float (&mu)[kMaxAct], const float* __restrict__ log_std, const float (&nrm)[8],
                        float (&act)[kMaxAct]) {
  float logp = 0.f;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a) {
    act[a] = 0.f;
    if (a < A) {
      const float ls = log_std[a];
      const float n = nrm[a < 8 ? a : 0];
      act[a] = mu[a] + __expf(ls) * n;
      logp += -0.5f * n * n - ls - kHalfLog2Pi;
    }
  }
  return logp;
}

// ---------------------------------------------------------------- episode statistics
// Columns of an ep_stats row: n_done, sum_ret, sumsq_ret, max_ret, min_ret, sum_len.
struct EpStats {
  float n = 0.f, sum = 0.f, sq = 0.f, mx = -INFINITY, mn = INFINITY, len = 0.f;

  RRL_DEV void add(float ret, int ep_len) {
    n += 1.f;
    sum += ret;
    sq += ret * ret;
    mx = fmaxf(mx, ret);
    mn = fminf(mn, ret);
    len += (float)ep_len;
  }
  RRL_DEV void wave_reduce() {
    n = wave_sum(n);
    sum = wave_sum(sum);
    sq = wave_sum(sq);
    len = wave_sum(len);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
  }
  RRL_DEV void store(float* __restrict__ row) const {
    row[0] = n;
    row[1] = sum;
    row[2] = sq;
    row[3] = mx;
    row[4] = mn;
    row[5] = len;
  }
  // Every wave of the workgroup accumulated: reduce over the waves through `red` (LDS that no
  // wave needs any more, 8 floats per wave) into this workgroup's row.
  RRL_DEV void reduce_block(const TileCtx& c, float* red, float* __restrict__ ep_stats) {
    __syncthreads();
    wave_reduce();
    if (c.l == 0) store(red + c.wib * 8);
    __syncthreads();
    if (threadIdx.x < 6) {
      const int q = threadIdx.x;
      float v = red[q];
      for (int w = 1; w < c.wpb; ++w) {
        const float u = red[w * 8 + q];
        v = (q == 3) ? fmaxf(v, u) : (q == 4) ? fminf(v, u) : v + u;
      }
      ep_stats[blockIdx.x * 8 + q] = v;
    }
  }
  // Only this wave accumulated: its wave reduction is the workgroup's row.
  RRL_DEV void reduce_wave(const TileCtx& c, float* __restrict__ ep_stats) {
    wave_reduce();
    if (c.l == 0) store(ep_stats + blockIdx.x * 8);
  }
};

// ---------------------------------------------------------------- host side
template <class E, int HT_>
struct EnvH {
  using Env = E;
  static constexpr int HT = HT_;
};

// f(EnvH<Env, HT>{}) for a discrete device env and H = 16 * HT in {64, 128}; -3 otherwise.
template <class F>
int dispatch_env_h(int env, int H, F&& f) {
  if (H != 128 && H != 64) return -3;
  const bool big = H == 128;
  switch (env) {
    case ENV_CARTPOLE: return big ? f(EnvH<CartPoleEnv, 8>{}) : f(EnvH<CartPoleEnv, 4>{});
    case ENV_MOUNTAINCAR: return big ? f(EnvH<MountainCarEnv, 8>{}) : f(EnvH<MountainCarEnv, 4>{});
    case ENV_ACROBOT: return big ? f(EnvH<AcrobotEnv, 8>{}) : f(EnvH<AcrobotEnv, 4>{});
    case ENV_LUNARLANDER: return big ? f(EnvH<LunarLanderSynthEnv, 8>{}) : f(EnvH<LunarLanderSynthEnv, 4>{});
  }
  return -3;
}

// Lets kernel K use the whole 160 KB of LDS as dynamic shared memory; set once per kernel.
template <auto K>
void raise_lds_limit() {
  static const hipError_t once =
      hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
  (void)once;
}

inline int grid_cap(int num_cu) { return 2 * (num_cu > 0 ? num_cu : 256); }

// One tile per wave, `waves` per workgroup; at most two workgroups per CU, beyond that the
// waves stride over the tiles.
inline int tile_stride_grid(int N, int num_cu, int waves = 4) {
  const int tiles = (N + kTileB - 1) / kTileB;
  int grid = (tiles + waves - 1) / waves;
  if (grid > grid_cap(num_cu)) grid = grid_cap(num_cu);
  return grid < 1 ? 1 : grid;
}

}  // namespace rrl
