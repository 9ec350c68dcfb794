// Fused learner kernel for wide observations, 33 <= D <= 128 (DT = 4 or 8 input tiles): the forward recompute, loss
// head, backward and weight gradients of mlp_grad.hip for the five on-policy heads, one launch per optimisation step.
//
// What is different from mlp_grad_kernel is where W1 lives.  At H = 128, D = 128 a resident W1 [128][132] (67.6 KB)
// beside W2 (67.6 KB) and the two [H][68] staging images (69.6 KB) would need about 205 KB of the 160 KB.  No dX is
// formed, so W1 is read by the layer-1 forward of a slab and by nothing else: its padded image LIVES IN THE STAGING
// AREA from the top of a 64-row slab until h1 is formed (as the padded W3 of mlp_grad_c51_kernel does).  Phase A then
// overwrites it and the next slab stages it again, behind the barrier that says the previous slab's phase-C readers
// are done.  W1 comes from L2 in natural feature order (coalesced rows) and is written in the interleaved column order
// of load_x_tile.  H = 64 takes the same scheme, so there is one code path.
//
// The staging images have SR = max(H, 16 DT) rows: phase C stages the 16 DT feature rows of x in one image, so dW1 is
// one wgrad<TO, DT> whatever H is.  dW3 always takes the MFMA tile (no VALU form), which keeps it to one instance per
// (DT, HT, head).  Everything else (heads, nvalid / inv_B_dev, mask, adv_stats, the ragged last slab, the slab
// layout) is mlp_grad_kernel's.
#include "api.h"
#include "common.h"
#include "heads.h"
#include "grad_args.h"
#include "actor_step.h"  // raise_lds_limit
#include "wgrad.h"

namespace rrl {

// LDS image: the trunk without W1, 16 rows of W3, then the two staging images that also hold W1.
template <int DT, int HT>
struct LdsWideIn {
  static constexpr int H = 16 * HT;
  static constexpr int S1 = 16 * DT + 4;  // W1 row stride (floats)
  static constexpr int S2 = H + 4;        // W2 row stride (floats)
  static constexpr int SR = H > 16 * DT ? H : 16 * DT;  // rows of a staging image
  static constexpr int W2 = 0;
  static constexpr int B1 = W2 + H * S2;
  static constexpr int B2 = B1 + H;
  static constexpr int B3 = B2 + H;  // kMaxAct floats
  static constexpr int LOGSTD = B3 + kMaxAct;
  static constexpr int W3 = LOGSTD + kMaxAct;  // [kMaxAct][H]
  static constexpr int ST0 = W3 + kMaxAct * H;
  static constexpr int ST1 = ST0 + SR * kStageLd;
  static constexpr int W1 = ST0;  // while layer 1 runs
  static constexpr int floats = ST1 + SR * kStageLd;
  static_assert(H * S1 <= 2 * SR * kStageLd, "W1 must fit the two staging images");
  static_assert(floats * sizeof(float) <= 163840, "the image must fit the LDS");
};

// Everything but W1, once per workgroup.
template <int DT, int HT>
RRL_DEV void stage_trunk_wide(float* __restrict__ lds, const float* __restrict__ flat, int D, int A, bool has_log_std) {
  using L = LdsWideIn<DT, HT>;
  constexpr int H = L::H;
  const FlatOffsets o = flat_offsets(D, H, A);
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int idx = tid; idx < H * (H / 4); idx += nt) {
    const int r = idx / (H / 4), c4 = idx - r * (H / 4);
    // o.w2 = H * D + H is a multiple of 4 floats, as H is a multiple of 16
    const floatx4 v = *reinterpret_cast<const floatx4*>(flat + o.w2 + r * H + 4 * c4);
    *reinterpret_cast<floatx4*>(lds + L::W2 + r * L::S2 + 4 * c4) = v;
  }
  for (int idx = tid; idx < H; idx += nt) {
    lds[L::B1 + idx] = flat[o.b1 + idx];
    lds[L::B2 + idx] = flat[o.b2 + idx];
  }
  for (int idx = tid; idx < kMaxAct; idx += nt) {
    lds[L::B3 + idx] = (idx < A) ? flat[o.b3 + idx] : 0.f;
    lds[L::LOGSTD + idx] = (has_log_std && idx < A) ? flat[o.log_std + idx] : 0.f;
  }
  for (int idx = tid; idx < A * H; idx += nt) lds[L::W3 + idx] = flat[o.w3 + idx];
}

// W1 [H][D] -> the padded image [H][16 DT + 4]: feature f = 16t + 4r + g goes to column 16t + 4g + r (the k-step
// order of load_x_tile), features >= D are zero.  Consecutive threads read consecutive features of a row (coalesced)
// and write 64 different columns of it (no bank conflict); the 4 pad columns of a row are never read.  The restage
// is bound by the latency of L2.  At H = 64 a thread loads all its H * 16 DT / 256 elements (16 or 32) before it
// stores the first; at H = 128, beside the 136 accumulator registers, that spills, and the loads go 8 at a time.
template <int DT, int HT>
RRL_DEV void stage_w1_wide(float* __restrict__ w1, const float* __restrict__ flat, int D) {
  constexpr int H = 16 * HT, S1 = 16 * DT + 4, C = 16 * DT, N = H * C / 256;
  if constexpr (HT == 8) {
#pragma unroll 8
    for (int idx = threadIdx.x; idx < H * C; idx += 256) {
      const int row = idx / C, f = idx - row * C;
      w1[row * S1 + (f & ~15) + 4 * (f & 3) + ((f >> 2) & 3)] = (f < D) ? flat[row * D + f] : 0.f;
    }
  } else {
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int row = idx / C, f = idx - row * C;
      v[k] = (f < D) ? flat[row * D + f] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int idx = threadIdx.x + 256 * k;
      const int row = idx / C, f = idx - row * C;
      w1[row * S1 + (f & ~15) + 4 * (f & 3) + ((f >> 2) & 3)] = v[k];
    }
  }
}

template <int DT, int HT, int HEAD>
__global__ __launch_bounds__(256, 1) void mlp_grad_wide_kernel(GradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using L = LdsWideIn<DT, HT>;
  constexpr int H = L::H;
  constexpr bool kGauss = (HEAD == HEAD_PPO_GAUSS || HEAD == HEAD_PG_GAUSS);
  constexpr bool kCat = (HEAD == HEAD_PG_CAT || HEAD == HEAD_PPO_CAT);
  constexpr bool kPpo = (HEAD == HEAD_PPO_CAT || HEAD == HEAD_PPO_GAUSS);
  static_assert(kGauss || kCat || HEAD == HEAD_VALUE_MSE, "the on-policy heads only");
  constexpr int TO = HT / 4;   // dW2 / dW1 output tiles per wave
  constexpr int TI3 = HT / 4;  // dW3 input tiles per wave
  const int A = (HEAD == HEAD_VALUE_MSE) ? 1 : p.A;
  float* st0 = lds + L::ST0;  // [SR][68]
  float* st1 = lds + L::ST1;  // [SR][68]
  float* w1 = lds + L::W1;    // [H][16 DT + 4] over both, from the top of a slab until h1 is formed

  stage_trunk_wide<DT, HT>(lds, p.params, p.D, A, kGauss);

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

  floatx4 acc2[TO][HT], acc1[TO][DT], acc3[1][TI3];
  float bacc2[TO], bacc1[TO], bacc3[1];
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
  for (int b = 0; b < TI3; ++b) acc3[0][b] = zero4();
  bacc3[0] = 0.f;
  float dls_acc[kMaxAct];  // Gaussian d(log_std) accumulators (per lane)
#pragma unroll
  for (int a = 0; a < kMaxAct; ++a) dls_acc[a] = 0.f;
  float s_loss = 0.f, s_ent = 0.f, s_kl = 0.f, s_clip = 0.f, s_val = 0.f, s_cnt = 0.f;
  // k-steps of the last input tile; 0 where D leaves that whole tile empty (D = 33 in DT = 4)
  const int kr1 = max(input_kr_last(p.D, DT), 0);
  // device-side batch shape (grad_args.h): rows >= Bv inert, inv_B from memory
  const int Bv = p.nvalid ? min(*p.nvalid, p.B) : p.B;
  const float invB = p.inv_B_dev ? *p.inv_B_dev : p.inv_B;

  for (int base = blockIdx.x * 64; base < Bv; base += gridDim.x * 64) {
    const int row0 = base + 16 * wave;
    const int nrows = max(0, min(16, Bv - row0));
    const bool valid = j < nrows;
    const int row = row0 + j;

    floatx4 x[DT], h1[HT], h2[HT];
    load_x_tile<DT>(p.X, p.D, p.D, row0, nrows, x);
    __syncthreads();  // the trunk is staged / the previous slab's phase-C readers are done with st0, st1
    stage_w1_wide<DT, HT>(w1, p.params, p.D);
    __syncthreads();
    dense_fwd<DT, HT, true>(w1, L::S1, lds + L::B1, x, h1, kr1);
    dense_fwd<HT, HT, true>(lds + L::W2, L::S2, lds + L::B2, h1, h2);

    // ------------------------------------------------------------ head + dLoss/dout (as mlp_grad_kernel)
    float dout[kMaxAct];
#pragma unroll
    for (int a = 0; a < kMaxAct; ++a) dout[a] = 0.f;
    const bool count = valid && g == 0;
    if constexpr (HEAD == HEAD_VALUE_MSE) {
      const float v = head_dot<HT>(lds + L::W3, lds[L::B3], h2);
      const float target = valid ? p.ret[row] : 0.f;
      const float diff = v - target;
      dout[0] = valid ? 2.f * diff * invB : 0.f;
      if (count) {
        s_loss += diff * diff;
        s_val += v;
        s_cnt += 1.f;
      }
    } else {
      float adv = valid ? p.adv[row] : 0.f;
      adv = (adv - adv_mean) * adv_rstd;
      float logits[kMaxAct];  // the means of the Gaussian heads
      float logp = 0.f, lse = 0.f, ent = 0.f;
      int act = 0;
      if constexpr (kCat) {
        policy_logits<HT>(lds + L::W3, lds + L::B3, A, H, h2, logits);
        if (valid) apply_mask(p.mask ? p.mask + (size_t)row * A : nullptr, A, logits);
        const CatStats cs = cat_stats(A, logits);
        act = valid ? p.act[row] : 0;
        lse = cs.lse;
        ent = cs.entropy;
        logp = pick_logit(A, logits, act) - lse;
      } else {
#pragma unroll
        for (int a = 0; a < kMaxAct; ++a) {
          logits[a] = 0.f;
          if (a < A) {
            logits[a] = head_dot<HT>(lds + L::W3 + a * H, lds[L::B3 + a], h2);
            const float ls = lds[L::LOGSTD + a];
            const float xa = valid ? p.actc[(size_t)row * A + a] : logits[a];
            const float z = (xa - logits[a]) * __expf(-ls);
            logp += -0.5f * z * z - ls - kHalfLog2Pi;
          }
        }
      }
      float dlogp, loss_i;  // dLoss_i / dlogp_i (before the 1/B mean)
      if constexpr (!kPpo) {
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
      for (int a = 0; a < kMaxAct; ++a) {
        if (a < A) {
          if constexpr (kCat) {
            const float pa = __expf(logits[a] - lse);
            const float lpa = logits[a] - lse;
            // d(logp_act)/dlogit_a = onehot - p ;  dH/dlogit_a = -p (log p_a + H)
            const float dpg = dlogp * ((a == act ? 1.f : 0.f) - pa);
            const float dent = pa > 0.f ? p.ent_coef * pa * (lpa + ent) : 0.f;
            dout[a] = scale * (dpg + dent);
          } else {
            const float ls = lds[L::LOGSTD + a];
            const float inv_var = __expf(-2.f * ls);
            const float xa = valid ? p.actc[(size_t)row * A + a] : logits[a];
            const float d = xa - logits[a];
            // dlogp/dmu = d / var ; dlogp/dls = d^2/var - 1 ; dH/dls = 1
            dout[a] = scale * dlogp * d * inv_var;
            if (g == 0) dls_acc[a] += scale * (dlogp * (d * d * inv_var - 1.f) - p.ent_coef);
            ent += 0.5f + kHalfLog2Pi + ls;
          }
        }
      }
      if (count) {
        s_loss += loss_i;
        s_ent += ent;
        if (p.logp_old) s_kl += p.logp_old[row] - logp;
        s_cnt += 1.f;
      }
    }

    // ------------------------------------------------------------ dh2 = W3^T dout * relu'
    floatx4 dh2[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) dh2[t] = zero4();
#pragma unroll
    for (int a = 0; a < kMaxAct; ++a) {
      if (a < A) {
#pragma unroll
        for (int t = 0; t < HT; ++t) {
          const floatx4 w = *reinterpret_cast<const floatx4*>(lds + L::W3 + a * H + 16 * t + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) dh2[t][r] = fmaf(w[r], dout[a], dh2[t][r]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dh2[t][r] = h2[t][r] > 0.f ? dh2[t][r] : 0.f;
    }

    // ------------------------------------------------------------ phase A: dW3, db3 (W1 is overwritten)
    __syncthreads();  // every wave has read its last W1 fragment
    stage_tiles<HT>(st0, wave, h2);
#pragma unroll
    for (int a = 0; a < kMaxAct; ++a)
      if ((a >> 2) == g) st1[a * kStageLd + 16 * wave + j] = (a < A) ? dout[a] : 0.f;
    __syncthreads();
    wgrad<1, TI3>(st1, st0, 0, wave * TI3, acc3, bacc3);

    // ------------------------------------------------------------ phase B: dW2, db2
    __syncthreads();
    stage_tiles<HT>(st0, wave, h1);
    stage_tiles<HT>(st1, wave, dh2);
    floatx4 dh1[HT];
    // dh1 needs only registers + W2: its MFMAs before the barrier hide the staging-write latency
    dense_bwd_data<HT, HT, true>(lds + L::W2, L::S2, dh2, h1, dh1);
    __syncthreads();
    wgrad<TO, HT>(st1, st0, wave * TO, 0, acc2, bacc2);

    // ------------------------------------------------------------ phase C: dW1, db1 (16 DT feature rows of x)
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
#pragma unroll
  for (int ti = 0; ti < TI3; ++ti) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 4 * g + r;
      if (a < A) slab[o.w3 + a * H + 16 * (wave * TI3 + ti) + j] = acc3[0][ti][r];
    }
  }
  const float b3 = group_sum(bacc3[0]);
  if (wave == 0 && g == 0 && j < A) slab[o.b3 + j] = b3;

  // Gaussian log_std grads and loss statistics: reduce over the workgroup via LDS
  __syncthreads();
  float* red = st0;  // reuse staging: [4 waves][32]
  float stats[6] = {s_loss, s_ent, s_kl, s_clip, s_val, s_cnt};
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const float v = wave_sum(stats[s]);
    if (l == 0) red[wave * 32 + s] = v;
  }
  if (kGauss) {
#pragma unroll
    for (int a = 0; a < kMaxAct; ++a) {
      const float v = wave_sum(dls_acc[a]);
      if (l == 0) red[wave * 32 + 8 + a] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int s = threadIdx.x;
    const float v = red[s] + red[32 + s] + red[64 + s] + red[96 + s];
    if (s < 6) p.loss_slab[blockIdx.x * 8 + s] = v;
    if (kGauss && s >= 8 && s - 8 < A) slab[o.log_std + (s - 8)] = v;
  }
}

template <int DT, int HT, int HEAD>
static int launch_wide(const GradArgs& a, int grid, hipStream_t s) {
  raise_lds_limit<mlp_grad_wide_kernel<DT, HT, HEAD>>();
  using L = LdsWideIn<DT, HT>;
  const size_t bytes = L::floats * sizeof(float);
  hipLaunchKernelGGL((mlp_grad_wide_kernel<DT, HT, HEAD>), dim3(grid), dim3(256), bytes, s, a);
  return (int)hipGetLastError();
}

template <int DT, int HT>
static int dispatch_wide_head(int head, const GradArgs& a, int grid, hipStream_t s) {
  switch (head) {
    case HEAD_PG_CAT: return launch_wide<DT, HT, HEAD_PG_CAT>(a, grid, s);
    case HEAD_VALUE_MSE: return launch_wide<DT, HT, HEAD_VALUE_MSE>(a, grid, s);
    case HEAD_PPO_CAT: return launch_wide<DT, HT, HEAD_PPO_CAT>(a, grid, s);
    case HEAD_PPO_GAUSS: return launch_wide<DT, HT, HEAD_PPO_GAUSS>(a, grid, s);
    case HEAD_PG_GAUSS: return launch_wide<DT, HT, HEAD_PG_GAUSS>(a, grid, s);
  }
  return -2;  // the Q heads take D <= 32
}

bool grad_wide_supported(int D, int H, int head) {
  return D > 32 && D <= 128 && (H == 64 || H == 128) && head >= HEAD_PG_CAT && head <= HEAD_PG_GAUSS;
}

int launch_grad_wide(const GradArgs& a, int head, int H, int grid, hipStream_t s) {
  if (!grad_wide_supported(a.D, H, head)) return -2;
  if (a.D <= 64) return H == 128 ? dispatch_wide_head<4, 8>(head, a, grid, s) : dispatch_wide_head<4, 4>(head, a, grid, s);
  return H == 128 ? dispatch_wide_head<8, 8>(head, a, grid, s) : dispatch_wide_head<8, 4>(head, a, grid, s);
}

}  // namespace rrl
