// Categorical policies of 17 .. 64 actions: the forward modes MODE_CAT_SAMPLE, MODE_CAT_EVAL, MODE_LOGITS and the
// gradient heads HEAD_PG_CAT, HEAD_PPO_CAT on the wide output layer of wide.h, D <= 32, H = 64 or 128.
//
// The heads of heads.h hold kMaxAct = 16 logits per row, every one replicated in the four lane groups.  Here the last
// layer runs on the matrix cores and the A logits of a row are ONE block of the wide layout (its "A" = 1, its "NA" =
// the actions): TPA = ceil(A / 16) tiles, and tile t, lane group g, register r of the lane with lane & 15 == j holds
// the logit of action i = 16 t + 4 g + r of batch column j.  A lane owns 4 TPA logits; logits past A are -inf.  W3 and
// b3 are staged padded to 16 TPA rows (stage_wide_w3), row stride H + 4.
//
// Head, per lane and then across the four lanes of a column (group_max / group_sum: xor 16, xor 32, i.e.
// (g0 + g1) + (g2 + g3), the same bits in all four):
//   mask     logit_i + (mask[row][i] - 1) * 1e8 on the lane's own i < A (apply_mask's formula; null mask: none)
//   softmax  m = max_i logit_i; e_i = exp(logit_i - m); s = sum e_i, sx = sum e_i (logit_i - m), each per lane with t
//            ascending then r ascending, then across the groups; lse = m + log s, entropy = log s - sx / s
//   logp(a)  the lane that holds a contributes logit_a, the others 0, one group sum; minus lse
//   sample   u = u01(philox((row_offset + row, step_lo, step_hi, 0), seed).x), p_i = exp(logit_i - lse), and the pick
//            is the lowest i with u < cdf_i and p_i > 0, else the highest i with p_i > 0, else 0.  The cdf, tile by tile
//            (carry_0 = 0):
//              c_0 = p_0;  c_r = c_(r-1) + p_r  (r = 1 .. 3)      in-lane prefix over the tile's four registers
//              T_g = c_3 of lane group g (shuffles);  E_0 = 0, E_1 = T_0, E_2 = T_0 + T_1, E_3 = (T_0 + T_1) + T_2
//              cdf_i = (carry_t + E_g) + c_r
//              carry_(t+1) = carry_t + (((T_0 + T_1) + T_2) + T_3)
//            Every lane proposes its lowest qualifying i (t, then r ascending) and a minimum over the groups takes the
//            pick.  cdf_i is fp32 and ascends up to one rounding between the lane groups.
//
// Forward: trunk (stage_net) and the padded W3 resident in LDS, a wave per 16-row tile as mlp_forward_kernel.
// Gradient: mlp_grad_c51_kernel's scheme with a single block.  The padded W3 LIVES IN THE STAGING AREA while the head
// and dh2 run, phase A overwrites it and every slab after the first stages it again; dout is 4 TPA registers per lane,
// dh2 = W3^T dout by MFMA (dense_bwd_acc), dW3 / db3 go through the staging images into wgrad and the epilogue drops
// the padding rows.  The head's arithmetic is mlp_grad_kernel's HEAD_PG_CAT / HEAD_PPO_CAT, per lane-held logit.
#include <limits.h>

#include "api.h"
#include "common.h"
#include "fwd_args.h"
#include "grad_args.h"
#include "actor_step.h"  // raise_lds_limit
#include "wgrad.h"
#include "wide.h"

namespace rrl {

// logit + (mask - 1) * 1e8 on the lane's own logits; mrow is the row's [A] mask.
template <int TPA>
RRL_DEV void wide_apply_mask(const float* __restrict__ mrow, int A, floatx4 (&lg)[TPA]) {
  const int g = lane_id() >> 4;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * t + 4 * g + r;
      if (i < A) lg[t][r] = lg[t][r] + (mrow[i] - 1.f) * 1e8f;
    }
  }
}

struct WideCatStats {
  float lse;      // log-sum-exp of the row's logits
  float entropy;  // -sum p log p
};

// cat_stats of heads.h over logits distributed across the lane groups, in the order of the header.
template <int TPA>
RRL_DEV WideCatStats wide_cat_stats(int A, const floatx4 (&lg)[TPA]) {
  const int g = lane_id() >> 4;
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, lg[t][r]);
  }
  m = group_max(m);
  float s = 0.f, sx = 0.f;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (16 * t + 4 * g + r < A) {  // a padded logit is -inf: 0 * -inf
        const float e = __expf(lg[t][r] - m);
        s += e;
        sx += e * (lg[t][r] - m);
      }
    }
  }
  s = group_sum(s);
  sx = group_sum(sx);
  WideCatStats c;
  c.lse = m + __logf(s);
  c.entropy = __logf(s) - sx / s;
  return c;
}

// The logit of action a, in every lane of the column: 0 where no lane holds a (pick_logit of heads.h).
template <int TPA>
RRL_DEV float wide_pick_logit(const floatx4 (&lg)[TPA], int a) {
  const int g = lane_id() >> 4;
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * t + 4 * g + r == a) v = lg[t][r];
  }
  return group_sum(v);
}

// Inverse-cdf draw with uniform u in [0, 1), the contract of cat_sample (heads.h); the cdf in the header's order.
template <int TPA>
RRL_DEV int wide_cat_sample(int A, const floatx4 (&lg)[TPA], float lse, float u) {
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  float carry = 0.f;
  int first = INT_MAX, last = -1;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
    float pr[4], c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pr[r] = (16 * t + 4 * g + r < A) ? __expf(lg[t][r] - lse) : 0.f;
    c[0] = pr[0];
#pragma unroll
    for (int r = 1; r < 4; ++r) c[r] = c[r - 1] + pr[r];
    const float t0 = __shfl(c[3], j, 64), t1 = __shfl(c[3], 16 + j, 64);
    const float t2 = __shfl(c[3], 32 + j, 64), t3 = __shfl(c[3], 48 + j, 64);
    const float e2 = t0 + t1, e3 = e2 + t2;
    const float base = carry + (g == 0 ? 0.f : g == 1 ? t0 : g == 2 ? e2 : e3);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * t + 4 * g + r;
      if (pr[r] > 0.f) {
        last = i;
        if (first == INT_MAX && u < base + c[r]) first = i;
      }
    }
    carry = carry + (e3 + t3);
  }
  first = min(first, __shfl_xor(first, 16, 64));
  first = min(first, __shfl_xor(first, 32, 64));
  last = max(last, __shfl_xor(last, 16, 64));
  last = max(last, __shfl_xor(last, 32, 64));
  return first != INT_MAX ? first : max(last, 0);  // u beyond the rounded cdf: the last action with p > 0
}

// LDS image of the forward kernel: LdsNet<DT, HT> without a head, then the padded b3 and W3.
template <int DT, int HT>
struct LdsCatWide {
  using T = LdsNet<DT, HT>;
  static constexpr int B3 = T::fixed_floats();  // [16 * TPA]
  static constexpr int W3_of(int TPA) { return B3 + 16 * TPA; }
  static constexpr int floats(int TPA) { return W3_of(TPA) + 16 * TPA * LdsWide<HT>::S3; }
};

// ------------------------------------------------------------------ forward
template <int DT, int HT, int TPA>
__global__ __launch_bounds__(256, 2) void mlp_cat_wide_fwd_kernel(FwdArgs p, int mode) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using L = LdsNet<DT, HT>;
  using LC = LdsCatWide<DT, HT>;
  const int A = p.A;
  const float* b3 = lds + LC::B3;
  const float* w3 = lds + LC::W3_of(TPA);
  stage_net<DT, HT>(lds, p.params, p.D, 0, false);
  stage_wide_w3<HT>(lds + LC::W3_of(TPA), lds + LC::B3, p.params, p.D, 1, A, TPA);
  __syncthreads();

  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int waves_per_block = blockDim.x >> 6;
  const int wave = (threadIdx.x >> 6) + blockIdx.x * waves_per_block;
  const int total_waves = gridDim.x * waves_per_block;
  const int ntiles = (p.B + kTileB - 1) / kTileB;
  const int kr1 = input_kr_last(p.D, DT);

  for (int tile = wave; tile < ntiles; tile += total_waves) {
    const int row0 = tile * kTileB;
    const int nrows = min(kTileB, p.B - row0);
    const int row = row0 + j;
    const bool valid = j < nrows;

    floatx4 x[DT], h1[HT], h2[HT], lg[TPA];
    load_x_tile<DT>(p.X, p.D, p.D, row0, nrows, x);
    if (p.x_copy != nullptr && valid) {  // every (row, feature) is held by exactly one lane
      float* xr = p.x_copy + (size_t)row * p.D;
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * t + 4 * r + g;
          if (f < p.D) xr[f] = x[t][r];
        }
    }
    dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, kr1);
    dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);
    wide_logits_at<HT, TPA>(w3, b3, A, h2, lg);
    if (valid && p.mask != nullptr) wide_apply_mask<TPA>(p.mask + (size_t)row * A, A, lg);

    if (mode == MODE_LOGITS) {
      if (valid) {
#pragma unroll
        for (int t = 0; t < TPA; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * t + 4 * g + r;
            if (i < A) p.logits_out[(size_t)row * A + i] = lg[t][r];
          }
        }
      }
      continue;
    }
    const WideCatStats cs = wide_cat_stats<TPA>(A, lg);
    int a;
    if (mode == MODE_CAT_SAMPLE) {
      const uint4 rnd = philox4x32(make_uint4(p.row_offset + (uint32_t)row, p.step_lo, p.step_hi, 0u),
                                   make_uint2(p.seed_lo, p.seed_hi));
      a = wide_cat_sample<TPA>(A, lg, cs.lse, u01(rnd.x));
    } else {
      a = valid ? p.act_in[row] : 0;
    }
    const float logp = wide_pick_logit<TPA>(lg, a) - cs.lse;
    if (valid && g == 0) {
      if (mode == MODE_CAT_SAMPLE) {
        p.act_out[row] = a;
        if (p.act_host != nullptr) p.act_host[row] = a;
      }
      p.out0[row] = logp;
      if (p.out1) p.out1[row] = cs.entropy;
    }
  }
}

// ------------------------------------------------------------------ gradient
// LDS: the trunk of LdsNet<DT, HT>, b3 padded [16 * TPA], then the two [H][68] staging images (16 TPA <= 64 <= H rows
// of dout fit one); the padded W3 [16 * TPA][H + 4] lies over both while the head runs.
template <int DT, int HT, int TPA, int HEAD>
__global__ __launch_bounds__(256, 1) void mlp_cat_wide_grad_kernel(GradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using L = LdsNet<DT, HT>;
  using LW = LdsWide<HT>;
  constexpr int H = L::H;
  constexpr int TO = HT / 4;   // dW2 / dW1 output tiles per wave
  constexpr int TI3 = HT / 4;  // dW3 input tiles per wave
  static_assert(HEAD == HEAD_PG_CAT || HEAD == HEAD_PPO_CAT, "the categorical policy heads only");
  static_assert(16 * TPA * LW::S3 <= 2 * H * kStageLd, "the padded W3 must fit the two staging images");
  const int A = p.A;
  float* b3 = lds + L::fixed_floats();  // [16 * TPA]
  float* st0 = b3 + 16 * TPA;           // [H][68]
  float* st1 = st0 + H * kStageLd;      // [H][68]
  float* w3 = st0;                      // [16 * TPA][H + 4] while the head runs

  stage_net<DT, HT>(lds, p.params, p.D, 0, false);
  stage_wide_w3<HT>(w3, b3, p.params, p.D, 1, A, TPA);

  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
  const int wave = threadIdx.x >> 6;

  float adv_mean = 0.f, adv_rstd = 1.f;
  if (p.adv_stats != nullptr) {
    const float n = fmaxf(p.adv_stats[2], 1.f);
    adv_mean = p.adv_stats[0] / n;
    const float var = fmaxf(p.adv_stats[1] / n - adv_mean * adv_mean, 0.f);
    adv_rstd = 1.f / (sqrtf(var) + 1e-8f);
  }

  floatx4 acc2[TO][HT], acc1[TO][DT], acc3[TPA][1][TI3];
  float bacc2[TO], bacc1[TO], bacc3[TPA][1];
#pragma unroll
  for (int a = 0; a < TO; ++a) {
    bacc2[a] = 0.f;
    bacc1[a] = 0.f;
#pragma unroll
    for (int b = 0; b < HT; ++b) acc2[a][b] = zero4();
#pragma unroll
    for (int b = 0; b < DT; ++b) acc1[a][b] = zero4();
  }
#pragma unroll
  for (int a = 0; a < TPA; ++a) {
    bacc3[a][0] = 0.f;
#pragma unroll
    for (int b = 0; b < TI3; ++b) acc3[a][0][b] = zero4();
  }
  float s_loss = 0.f, s_ent = 0.f, s_kl = 0.f, s_clip = 0.f, s_cnt = 0.f;
  const int kr1 = input_kr_last(p.D, DT);
  // device-side batch shape (grad_args.h): rows >= Bv inert, inv_B from memory
  const int Bv = p.nvalid ? min(*p.nvalid, p.B) : p.B;
  const float invB = p.inv_B_dev ? *p.inv_B_dev : p.inv_B;
  bool staged = true;  // the first slab's W3 came with the net

  for (int base = blockIdx.x * 64; base < Bv; base += gridDim.x * 64) {
    __syncthreads();  // the net is staged / the previous slab's phase-C readers are done with st0, st1
    if (!staged) {
      stage_wide_w3<HT>(w3, nullptr, p.params, p.D, 1, A, TPA);
      __syncthreads();
    }
    staged = false;
    const int row0 = base + 16 * wave;
    const int nrows = max(0, min(16, Bv - row0));
    const bool valid = j < nrows;
    const int row = row0 + j;

    floatx4 x[DT], h1[HT], h2[HT];
    load_x_tile<DT>(p.X, p.D, p.D, row0, nrows, x);
    dense_fwd<DT, HT, true>(lds + L::W1, L::S1, lds + L::B1, x, h1, kr1);
    dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);

    // ------------------------------------------------------------ head + dLoss/dout (as mlp_grad_kernel)
    floatx4 lg[TPA], d[TPA];
    wide_logits_at<HT, TPA>(w3, b3, A, h2, lg);
    if (valid && p.mask != nullptr) wide_apply_mask<TPA>(p.mask + (size_t)row * A, A, lg);
    const WideCatStats cs = wide_cat_stats<TPA>(A, lg);
    const int act = valid ? p.act[row] : 0;
    const float logp = wide_pick_logit<TPA>(lg, act) - cs.lse;
    float adv = valid ? p.adv[row] : 0.f;
    adv = (adv - adv_mean) * adv_rstd;
    const bool count = valid && g == 0;
    float dlogp, loss_i;  // dLoss_i / dlogp_i (before the 1/B mean)
    if constexpr (HEAD == HEAD_PG_CAT) {
      dlogp = -adv;
      loss_i = -logp * adv;
    } else {
      const float lpo = valid ? p.logp_old[row] : logp;
      const float ratio = __expf(logp - lpo);
      const float s1 = ratio * adv;
      const float s2 = fminf(fmaxf(ratio, 1.f - p.clip_eps), 1.f + p.clip_eps) * adv;
      dlogp = (s1 <= s2) ? -adv * ratio : 0.f;
      loss_i = -fminf(s1, s2);
      if (count) s_clip += (fabsf(ratio - 1.f) > p.clip_eps) ? 1.f : 0.f;
    }
    const float scale = valid ? invB : 0.f;
#pragma unroll
    for (int t = 0; t < TPA; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * t + 4 * g + r;
        d[t][r] = 0.f;
        if (i < A) {
          const float lpa = lg[t][r] - cs.lse;
          const float pa = __expf(lpa);
          // d(logp_act)/dlogit_i = onehot - p ;  dH/dlogit_i = -p (log p_i + H)
          const float dpg = dlogp * ((i == act ? 1.f : 0.f) - pa);
          const float dent = pa > 0.f ? p.ent_coef * pa * (lpa + cs.entropy) : 0.f;
          d[t][r] = scale * (dpg + dent);
        }
      }
    }
    if (count) {
      s_loss += loss_i;
      s_ent += cs.entropy;
      if (p.logp_old) s_kl += p.logp_old[row] - logp;
      s_cnt += 1.f;
    }

    // ------------------------------------------------------------ dh2 = W3^T dout * relu'
    floatx4 dh2[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) dh2[t] = zero4();
    dense_bwd_acc<HT, TPA>(w3, LW::S3, d, dh2);
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dh2[t][r] = h2[t][r] > 0.f ? dh2[t][r] : 0.f;
    }

    // ------------------------------------------------------------ phase A: dW3, db3 (W3 is overwritten)
    __syncthreads();  // every wave has read its last W3 fragment
    stage_tiles<HT>(st0, wave, h2);
    stage_tiles<TPA>(st1, wave, d);
    __syncthreads();
#pragma unroll
    for (int to = 0; to < TPA; ++to) wgrad<1, TI3>(st1, st0, to, wave * TI3, acc3[to], bacc3[to]);

    // ------------------------------------------------------------ phase B: dW2, db2
    __syncthreads();
    stage_tiles<HT>(st0, wave, h1);
    stage_tiles<HT>(st1, wave, dh2);
    floatx4 dh1[HT];
    // dh1 needs only registers + W2: its MFMAs before the barrier hide the staging-write latency
    dense_bwd_data<HT, HT, true>(lds + L::W2, L::S2, dh2, h1, dh1);
    __syncthreads();
    wgrad<TO, HT>(st1, st0, wave * TO, 0, acc2, bacc2);

    // ------------------------------------------------------------ phase C: dW1, db1
    __syncthreads();
    stage_x_tiles<DT>(st0, wave, x);
    stage_tiles<HT>(st1, wave, dh1);
    __syncthreads();
    wgrad<TO, DT>(st1, st0, wave * TO, 0, acc1, bacc1);
  }

  // ------------------------------------------------------------------ epilogue
  const FlatOffsets o = flat_offsets(p.D, H, A);
  float* slab = p.grad_slab + (size_t)blockIdx.x * p.P;
#pragma unroll
  for (int to = 0; to < TO; ++to) {
    const int ot = wave * TO + to;
#pragma unroll
    for (int ti = 0; ti < HT; ++ti) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[o.w2 + (16 * ot + 4 * g + r) * H + 16 * ti + j] = acc2[to][ti][r];
    }
    const float b2 = group_sum(bacc2[to]);
    if (g == 0) slab[o.b2 + 16 * ot + j] = b2;
#pragma unroll
    for (int ti = 0; ti < DT; ++ti) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * ti + j;
        if (col < p.D) slab[o.w1 + (16 * ot + 4 * g + r) * p.D + col] = acc1[to][ti][r];
      }
    }
    const float b1 = group_sum(bacc1[to]);
    if (g == 0) slab[o.b1 + 16 * ot + j] = b1;
  }
  // dW3 / db3: padded tile `to` is actions 16 to .. 16 to + 15; the padding rows are dropped
#pragma unroll
  for (int to = 0; to < TPA; ++to) {
#pragma unroll
    for (int ti = 0; ti < TI3; ++ti) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * to + 4 * g + r;
        if (i < A) slab[o.w3 + i * H + 16 * (wave * TI3 + ti) + j] = acc3[to][0][ti][r];
      }
    }
    const float b3g = group_sum(bacc3[to][0]);
    if (wave == 0 && g == 0 && 16 * to + j < A) slab[o.b3 + 16 * to + j] = b3g;
  }

  // loss statistics: reduce over the workgroup via LDS
  __syncthreads();
  float* red = st0;  // reuse staging: [4 waves][8]
  float stats[6] = {s_loss, s_ent, s_kl, s_clip, 0.f, s_cnt};
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const float v = wave_sum(stats[s]);
    if (l == 0) red[wave * 8 + s] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int s = threadIdx.x;
    p.loss_slab[blockIdx.x * 8 + s] = red[s] + red[8 + s] + red[16 + s] + red[24 + s];
  }
}

// ------------------------------------------------------------------ host side
template <int DT, int HT>
static int launch_fwd_dt(const FwdArgs& a, int mode, int num_cu, hipStream_t s) {
  const int tpa = wide_tpa(1, a.A);
  const size_t bytes = sizeof(float) * (size_t)LdsCatWide<DT, HT>::floats(tpa);
  if (bytes > 163840) return -4;
  // one wave per tile; two workgroups per CU where two images fit the LDS, else one
  int grid = ((a.B + kTileB - 1) / kTileB + 3) / 4;
  const int cap = (2 * bytes <= 163840 ? 2 : 1) * (num_cu > 0 ? num_cu : 256);
  if (grid > cap) grid = cap;
  return dispatch_tpa<kMaxTpa>(tpa, [&](auto tag) {
    constexpr int TPA = decltype(tag)::TPA;
    if constexpr (TPA == 1) {
      return -2;  // up to 16 actions: mlp_forward_kernel
    } else {
      raise_lds_limit<mlp_cat_wide_fwd_kernel<DT, HT, TPA>>();
      hipLaunchKernelGGL((mlp_cat_wide_fwd_kernel<DT, HT, TPA>), dim3(grid), dim3(256), bytes, s, a, mode);
      return (int)hipGetLastError();
    }
  });
}

int launch_fwd_cat_wide(const FwdArgs& a, int mode, int num_cu, hipStream_t s) {
  if (mode != MODE_CAT_SAMPLE && mode != MODE_CAT_EVAL && mode != MODE_LOGITS) return -2;
  if (a.A <= kMaxAct || a.A > kMaxCatAct || a.D < 1 || a.D > 32) return -2;
  if (a.H == 128) return a.D <= 16 ? launch_fwd_dt<1, 8>(a, mode, num_cu, s) : launch_fwd_dt<2, 8>(a, mode, num_cu, s);
  if (a.H == 64) return a.D <= 16 ? launch_fwd_dt<1, 4>(a, mode, num_cu, s) : launch_fwd_dt<2, 4>(a, mode, num_cu, s);
  return -3;
}

template <int DT, int HT>
static int launch_grad_dt(const GradArgs& a, int head, int grid, hipStream_t s) {
  const int tpa = wide_tpa(1, a.A);
  const size_t bytes =
      sizeof(float) * ((size_t)LdsNet<DT, HT>::fixed_floats() + 16 * tpa + 2 * (size_t)(16 * HT) * kStageLd);
  if (bytes > 163840) return -4;
  return dispatch_tpa<kMaxTpa>(tpa, [&](auto tag) {
    constexpr int TPA = decltype(tag)::TPA;
    if constexpr (TPA == 1) {
      return -2;  // up to 16 actions: mlp_grad_kernel
    } else {
      if (head == HEAD_PG_CAT) {
        raise_lds_limit<mlp_cat_wide_grad_kernel<DT, HT, TPA, HEAD_PG_CAT>>();
        hipLaunchKernelGGL((mlp_cat_wide_grad_kernel<DT, HT, TPA, HEAD_PG_CAT>), dim3(grid), dim3(256), bytes, s, a);
      } else {
        raise_lds_limit<mlp_cat_wide_grad_kernel<DT, HT, TPA, HEAD_PPO_CAT>>();
        hipLaunchKernelGGL((mlp_cat_wide_grad_kernel<DT, HT, TPA, HEAD_PPO_CAT>), dim3(grid), dim3(256), bytes, s, a);
      }
      return (int)hipGetLastError();
    }
  });
}

int launch_grad_cat_wide(const GradArgs& a, int head, int H, int grid, hipStream_t s) {
  if (head != HEAD_PG_CAT && head != HEAD_PPO_CAT) return -2;
  if (a.A <= kMaxAct || a.A > kMaxCatAct || a.D < 1 || a.D > 32 || (H != 64 && H != 128)) return -2;
  if (H == 128) return a.D <= 16 ? launch_grad_dt<1, 8>(a, head, grid, s) : launch_grad_dt<2, 8>(a, head, grid, s);
  return a.D <= 16 ? launch_grad_dt<1, 4>(a, head, grid, s) : launch_grad_dt<2, 4>(a, head, grid, s);
}

}  // namespace rrl
