// The wide output layer and the categorical (C51, Bellemare et al. 2017) head built on it.
//
// The fused heads of heads.h hold kMaxAct = 16 outputs per row, each a VALU dot product replicated in the four
// lane groups.  A categorical Q-network has A * NA outputs (NA atoms per action, 50 to 130 in all), so its last
// layer runs on the matrix cores instead and its outputs stay DISTRIBUTED over the lane groups:
//
//   * LDS image (LdsWide): the trunk of LdsNet<1, HT> (W1, W2, b1, b2 at the same offsets, so dense_fwd and
//     stage_net serve it), then b3 and W3 PADDED: every action's NA rows are rounded up to TPA = ceil(NA / 16)
//     whole 16-row tiles, padding rows zero, row stride H + 4 like W2.  A tile then belongs to one action,
//     wave-uniformly.  OT = A * TPA <= 8 tiles (H = 128: 147,072 B of the 160 KB).
//   * forward: one action at a time, dense_fwd<HT, TPA, false> over that action's TPA tiles.  Tile t, lane group
//     g, register r holds the logit of atom 16 t + 4 g + r of the action for the batch column lane & 15; only
//     4 * TPA logits are live whatever A is.  Padded atoms take the logit -inf.
//   * softmax and expectation of one action: per-lane partial max / sum / sum z_i e_i over the lane's registers
//     (t ascending, r ascending), then the two cross-lane steps xor 16, xor 32 over the lane groups, i.e.
//     (g0 + g1) + (g2 + g3) in every lane.  reference.c51_q repeats the order in fp32.
//   * the greedy action is the lowest-index argmax of the A expectations, found while the actions stream by; the
//     targets kernel keeps the probabilities of the best action so far in 4 * TPA registers.
#pragma once
#include "common.h"

namespace rrl {

constexpr int kMaxWideTiles = 8;  // OT = A * TPA output tiles at most
constexpr int kMaxTpa = 4;        // 64 atoms per action at most
// A categorical POLICY of 17 .. 64 actions is one block of this layout (A = 1, NA = the actions): mlp_cat_wide.hip
constexpr int kMaxCatAct = 16 * kMaxTpa;

// The support z_i = v_min + i * dz, dz = (v_max - v_min) / (NA - 1), as one fused multiply-add.
struct C51Support {
  int NA;
  float v_min, dz;
};
RRL_DEV float c51_atom(const C51Support& s, int i) { return fmaf((float)i, s.dz, s.v_min); }

template <int HT>
struct LdsWide {
  using T = LdsNet<1, HT>;  // the trunk: W1, W2, B1, B2 and the 32 floats of its B3 / LOGSTD slots
  static constexpr int H = T::H;
  static constexpr int S3 = H + 4;               // W3 row stride (floats)
  static constexpr int B3 = T::fixed_floats();   // [16 * OT]
  static constexpr int W3_of(int OT) { return B3 + 16 * OT; }
  static constexpr int floats(int OT) { return W3_of(OT) + 16 * OT * S3; }
};

// The tiles per action of NA atoms, or 0 for a head that is not built: NA < 2, more than 64 atoms per action or
// more than 8 tiles in all.
__host__ __device__ inline int wide_tpa(int A, int NA) {
  if (A < 1 || NA < 2 || NA > 16 * kMaxTpa) return 0;
  const int tpa = (NA + 15) >> 4;
  return A * tpa <= kMaxWideTiles ? tpa : 0;
}

// Global -> LDS staging of the padded last layer of MLPSpec(D, H, A * NA): W3 [16 * A * TPA][H + 4] and b3.
template <int HT>
RRL_DEV void stage_wide_w3(float* __restrict__ w3, float* __restrict__ b3, const float* __restrict__ flat, int D,
                           int A, int NA, int TPA) {
  using L = LdsWide<HT>;
  constexpr int H = L::H;
  const FlatOffsets o = flat_offsets(D, H, A * NA);
  const int rows = 16 * A * TPA;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int idx = tid; idx < rows * (H / 4); idx += nt) {
    const int row = idx / (H / 4), c4 = idx - row * (H / 4);
    const int a = row / (16 * TPA), i = row - a * 16 * TPA;
    floatx4 v = zero4();
    if (i < NA) v = *reinterpret_cast<const floatx4*>(flat + o.w3 + (size_t)(a * NA + i) * H + 4 * c4);
    *reinterpret_cast<floatx4*>(w3 + row * L::S3 + 4 * c4) = v;
  }
  if (b3 != nullptr) {
    for (int row = tid; row < rows; row += nt) {
      const int a = row / (16 * TPA), i = row - a * 16 * TPA;
      b3[row] = (i < NA) ? flat[o.b3 + a * NA + i] : 0.f;
    }
  }
}

// Global -> LDS staging of MLPSpec(D, H, A * NA): the trunk through stage_net (which stages no head for A = 0),
// then the padded b3 and W3.
template <int HT>
RRL_DEV void stage_wide(float* __restrict__ lds, const float* __restrict__ flat, int D, int A, int NA, int TPA) {
  using L = LdsWide<HT>;
  stage_net<1, HT>(lds, flat, D, 0, false);
  stage_wide_w3<HT>(lds + L::W3_of(A * TPA), lds + L::B3, flat, D, A, NA, TPA);
}

// h2 of this wave's 16 batch columns from an interleaved observation tile.
template <int HT>
RRL_DEV void wide_trunk(const float* __restrict__ lds, const floatx4 (&x)[1], int kr_last, floatx4 (&h2)[HT]) {
  using T = LdsNet<1, HT>;
  floatx4 h1[HT];
  dense_fwd<1, HT, true>(lds + T::W1, T::S1, lds + T::B1, x, h1, kr_last);
  dense_fwd<HT, HT, true>(lds + T::W2, T::S2, lds + T::B2, h1, h2);
}

// The logits of one action from its block of the padded W3 / b3: lg[t][r] is atom 16 t + 4 g + r, -inf past NA.
template <int HT, int TPA>
RRL_DEV void wide_logits_at(const float* __restrict__ w3a, const float* __restrict__ b3a, int NA,
                            const floatx4 (&h2)[HT], floatx4 (&lg)[TPA]) {
  const int g = lane_id() >> 4;
  dense_fwd<HT, TPA, false>(w3a, LdsWide<HT>::S3, b3a, h2, lg);
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * t + 4 * g + r >= NA) lg[t][r] = -INFINITY;
  }
}

// The logits of action a of the image LdsWide.
template <int HT, int TPA>
RRL_DEV void wide_logits(const float* __restrict__ lds, int OT, int a, int NA, const floatx4 (&h2)[HT],
                         floatx4 (&lg)[TPA]) {
  using L = LdsWide<HT>;
  wide_logits_at<HT, TPA>(lds + L::W3_of(OT) + 16 * TPA * a * L::S3, lds + L::B3 + 16 * TPA * a, NA, h2, lg);
}

// din += W^T dout over the NO tiles of one action's block of the padded W3 (dense_bwd_data without the clear and
// the mask, so that the actions accumulate into one dh2).
template <int NI, int NO>
RRL_DEV void dense_bwd_acc(const float* __restrict__ W, int S, const floatx4 (&dout)[NO], floatx4 (&din)[NI]) {
  const int l = lane_id();
  const int i = l & 15, g = l >> 4;
#pragma unroll
  for (int to = 0; to < NO; ++to) {
    float wc[4][NI];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int ti = 0; ti < NI; ++ti) wc[r][ti] = W[(16 * to + 4 * g + r) * S + i + 16 * ti];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int ti = 0; ti < NI; ++ti) din[ti] = mfma4(wc[r][ti], dout[to][r], din[ti]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Softmax of one action's logits in place (lg becomes p) and its expectation sum_i z_i p_i, in the order of the
// header.  Every lane of a batch column returns the same bits.  *lse (where given) is log sum_i exp(logit_i).
template <int TPA>
RRL_DEV float c51_softmax_q(const C51Support& sup, floatx4 (&lg)[TPA], float* lse = nullptr) {
  const int g = lane_id() >> 4;
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, lg[t][r]);
  }
  m = group_max(m);
  float s = 0.f, sz = 0.f;
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = expf(lg[t][r] - m);  // 0 for a padded atom
      lg[t][r] = e;
      s += e;
      sz = fmaf(c51_atom(sup, 16 * t + 4 * g + r), e, sz);
    }
  }
  s = group_sum(s);
  sz = group_sum(sz);
  if (lse != nullptr) *lse = m + logf(s);
#pragma unroll
  for (int t = 0; t < TPA; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) lg[t][r] = lg[t][r] / s;
  }
  return sz / s;
}

// The greedy action of a categorical net at h2: the lowest-index argmax of the A expectations; *q_best is its
// value and, where keep is given, keep[t][r] the probability of its atom 16 t + 4 g + r.  pick >= 0 (double Q:
// the action another net chose) replaces the argmax.
template <int HT, int TPA>
RRL_DEV int c51_greedy(const float* __restrict__ lds, int A, const C51Support& sup, const floatx4 (&h2)[HT],
                       float* q_best, floatx4 (*keep)[TPA] = nullptr, int pick = -1) {
  int best = 0;
  float qb = 0.f;
  for (int a = 0; a < A; ++a) {
    floatx4 lg[TPA];
    wide_logits<HT, TPA>(lds, A * TPA, a, sup.NA, h2, lg);
    const float q = c51_softmax_q<TPA>(sup, lg);
    const bool take = pick >= 0 ? a == pick : (a == 0 || q > qb);
    if (take) {
      best = a;
      qb = q;
      if (keep != nullptr) {
#pragma unroll
        for (int t = 0; t < TPA; ++t) (*keep)[t] = lg[t];
      }
    }
  }
  *q_best = qb;
  return best;
}

// The categorical projection of the target distribution onto the support, in the gather form
//   b_j = (clamp(G + c * z_j, v_min, v_max) - v_min) / dz,   m_i = sum_j p_j * max(0, 1 - |b_j - i|),
// c = disc * boot.  It is scatter-free and deterministic, and right where b_j is an integer.  Each lane forms the
// m_i of its own registers, so it needs every p_j of its row: step k = 0 .. 3 reads lane group k's registers by
// ds_bpermute (no LDS patch: at H = 128 with 8 tiles 16,768 B are left, which four waves' [16][64] patches would
// fill to the last byte, and the rotation needs no barrier).  The j order, k outer, then t, then r, is the same in
// every lane (reference.c51_project repeats it in fp32).
template <int TPA>
RRL_DEV void c51_project(const C51Support& sup, float G, float c, const floatx4 (&p)[TPA], floatx4 (&m)[TPA]) {
  const int l = lane_id();
  const int g = l >> 4;
  const float v_max = c51_atom(sup, sup.NA - 1);
#pragma unroll
  for (int t = 0; t < TPA; ++t) m[t] = zero4();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int tj = 0; tj < TPA; ++tj) {
#pragma unroll
      for (int rj = 0; rj < 4; ++rj) {
        const float pj = __shfl(p[tj][rj], 16 * k + (l & 15), 64);
        const float tz = fminf(fmaxf(fmaf(c, c51_atom(sup, 16 * tj + 4 * k + rj), G), sup.v_min), v_max);
        const float bj = (tz - sup.v_min) / sup.dz;
#pragma unroll
        for (int t = 0; t < TPA; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            m[t][r] = fmaf(pj, fmaxf(0.f, 1.f - fabsf(bj - (float)(16 * t + 4 * g + r))), m[t][r]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- host side
// atoms / v_min / v_max as the entry points take them -> the tiles per action and the support, or 0 for what
// they refuse with -3: NA < 2, v_max <= v_min (or not finite), or a head past the tile limit.
inline int c51_support(int A, int atoms, float v_min, float v_max, C51Support* sup) {
  const int tpa = wide_tpa(A, atoms);
  if (tpa == 0 || !(v_max > v_min) || !(v_max - v_min < INFINITY)) return 0;
  *sup = C51Support{atoms, v_min, (v_max - v_min) / (float)(atoms - 1)};
  return tpa;
}

template <int N>
struct TpaTag {
  static constexpr int TPA = N;
};
// f(TpaTag<tpa>{}) for tpa in 1 .. MAX_TPA; -3 otherwise.
template <int MAX_TPA, class F>
int dispatch_tpa(int tpa, F&& f) {
  if (tpa == 1) return f(TpaTag<1>{});
  if constexpr (MAX_TPA >= 2) {
    if (tpa == 2) return f(TpaTag<2>{});
  }
  if constexpr (MAX_TPA >= 4) {
    if (tpa == 3) return f(TpaTag<3>{});
    if (tpa == 4) return f(TpaTag<4>{});
  }
  return -3;
}

}  // namespace rrl
