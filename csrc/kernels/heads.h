// Policy / value heads fused into the MLP epilogue (K2-K6 of SURVEY §2.6).
//
// Reference semantics (kernel.py:23-37): logits += (mask - 1) * 1e8, softmax,
// torch.multinomial sample.  Unlike the reference (which gathers the raw logit and
// calls it a log-prob) we return the true log_softmax[a]; the
// entropy is the true -sum p log p.
#pragma once
#include "common.h"

namespace rrl {

// Full logits (every lane of column j ends up with all A values).
template <int HT>
RRL_DEV void policy_logits(const float* __restrict__ W3, const float* __restrict__ b3, int A, int H,
                           const floatx4 (&h)[HT], float (&logits)[kMaxAct]) {
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a) {
    if (a < A) logits[a] = head_dot<HT>(W3 + a * H, b3[a], h);
    else logits[a] = -INFINITY;
  }
}

RRL_DEV void apply_mask(const float* __restrict__ mrow, int A, float (&logits)[kMaxAct]) {
  if (mrow == nullptr) return;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a)
    if (a < A) logits[a] = logits[a] + (mrow[a] - 1.f) * 1e8f;
}

struct CatStats {
  float lse;      // log-sum-exp of logits
  float entropy;  // -sum p log p
};

RRL_DEV CatStats cat_stats(int A, const float (&logits)[kMaxAct]) {
  float m = -INFINITY;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a)
    if (a < A) m = fmaxf(m, logits[a]);
  float s = 0.f, sx = 0.f;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a)
    if (a < A) {
      const float e = __expf(logits[a] - m);
      s += e;
      sx += e * (logits[a] - m);
    }
  CatStats c;
  c.lse = m + __logf(s);
  // H = lse - sum p*logit = log s - sx/s   (shifted by m)
  c.entropy = __logf(s) - sx / s;
  return c;
}

// Inverse-CDF categorical draw with uniform u in [0,1).
RRL_DEV int cat_sample(int A, const float (&logits)[kMaxAct], float lse, float u) {
  float c = 0.f;
  int pick = -1;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a)
    if (a < A) {
      const float p = __expf(logits[a] - lse);
      c += p;
      if (pick < 0 && u < c && p > 0.f) pick = a;
    }
  if (pick < 0) {  // u beyond the rounded cdf: take the last action with p > 0
#pragma unroll
    for (int a = 0; a < kMaxAct; ++a)
      if (a < A && __expf(logits[a] - lse) > 0.f) pick = a;
  }
  return pick < 0 ? 0 : pick;
}

// Lowest index among the maximal values: the greedy action (reference.greedy_from_logits).
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

RRL_DEV float pick_logit(int A, const float (&logits)[kMaxAct], int act) {
  float v = 0.f;
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a)
    if (a == act) v = logits[a];
  return v;
}

// Dueling head (Wang et al. 2016) over A + 1 outputs: out[0 .. A-1] are the advantages, out[A] the state
// value, and Q(a) = V + adv[a] - mean adv.  dueling_base is the per-row constant V - mean: the advantages
// are summed ascending, one add each, then one division (reference.dueling_q repeats the order).  The greedy
// action is argmax_first over the ADVANTAGES: adding the constant in fp32 could create ties they do not have.
RRL_DEV float dueling_base(int A, const float (&out)[kMaxAct]) {
  float s = out[0];
#pragma unroll
  for (int k = 1; k < kMaxAct; ++k)
    if (k < A) s += out[k];
  const float m = s / (float)A;
  return pick_logit(A + 1, out, A) - m;
}
// Q of action act: (V - mean) + adv[act]; the unrolled select of pick_logit keeps `out` in registers.
RRL_DEV float dueling_q(int A, const float (&out)[kMaxAct], int act) {
  return dueling_base(A, out) + pick_logit(A, out, act);
}

// Quantile-regression head (Dabney et al. 2018) over A * NQ outputs: out[a * NQ + i] is quantile i of action a
// (action-major).  The greedy value of an action is the SUM of its quantiles, s = out[a * NQ]; s += out[a * NQ + i]
// for i = 1 .. NQ-1 ascending, one add each, never divided (reference.quantile_q repeats the order); the
// greedy action is argmax_first over the A sums.  NQ is a run-time value: the walk over the 16 registers is
// unrolled and carries (action, quantile) counters, so `out` is never indexed by a variable.
RRL_DEV int quantile_argmax(int A, int NQ, const float (&out)[kMaxAct]) {
  int pick = 0, a = 0, i = 0;
  float best = 0.f, s = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxAct; ++k)
    if (k < A * NQ) {
      s = (i == 0) ? out[k] : s + out[k];
      if (++i == NQ) {
        if (a == 0 || s > best) {
          best = s;
          pick = a;
        }
        ++a;
        i = 0;
      }
    }
  return pick;
}
// The quantile sum of action act, in the same order.
RRL_DEV float quantile_sum(int NQ, const float (&out)[kMaxAct], int act) {
  const int lo = act * NQ;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxAct; ++k)
    if (k >= lo && k < lo + NQ) s = (k == lo) ? out[k] : s + out[k];
  return s;
}

// Gaussian head: log N(x; mu, sigma) summed over dims.
constexpr float kHalfLog2Pi = 0.91893853320467274f;

}  // namespace rrl
