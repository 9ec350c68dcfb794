// Weight-gradient staging of the fused learner kernels (mlp_grad.hip, mlp_grad_wide.hip): the [feature][64 batch]
// LDS images that transpose an operand pair once per 64-row slab, and the MFMA product that sums over the batch.
#pragma once
#include "common.h"

namespace rrl {

constexpr int kStageLd = 68;  // [feature][64 batch + 4 pad]

// acc[to][ti] += sum_b At[16*(to0+to)+i][b] * Bt[16*(ti0+ti)+i][b], b over the 64-row slab.
// Operands of batch block bb+1 are loaded while block bb's MFMAs issue.
template <int NTO, int NTI>
RRL_DEV void wgrad(const float* __restrict__ At, const float* __restrict__ Bt, int to0, int ti0,
                   floatx4 (&acc)[NTO][NTI], float (&bacc)[NTO]) {
  const int l = lane_id();
  const int i = l & 15, g = l >> 4;
  floatx4 a[NTO], b[NTI], an[NTO], bn[NTI];
#pragma unroll
  for (int to = 0; to < NTO; ++to)
    a[to] = *reinterpret_cast<const floatx4*>(At + (16 * (to0 + to) + i) * kStageLd + 4 * g);
#pragma unroll
  for (int ti = 0; ti < NTI; ++ti)
    b[ti] = *reinterpret_cast<const floatx4*>(Bt + (16 * (ti0 + ti) + i) * kStageLd + 4 * g);
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    if (bb < 3) {
#pragma unroll
      for (int to = 0; to < NTO; ++to)
        an[to] = *reinterpret_cast<const floatx4*>(At + (16 * (to0 + to) + i) * kStageLd + 16 * (bb + 1) + 4 * g);
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti)
        bn[ti] = *reinterpret_cast<const floatx4*>(Bt + (16 * (ti0 + ti) + i) * kStageLd + 16 * (bb + 1) + 4 * g);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int to = 0; to < NTO; ++to) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) acc[to][ti] = mfma4(a[to][r], b[ti][r], acc[to][ti]);
      }
    }
#pragma unroll
    for (int to = 0; to < NTO; ++to) bacc[to] += (a[to][0] + a[to][1]) + (a[to][2] + a[to][3]);
    __builtin_amdgcn_sched_barrier(0);
    if (bb < 3) {
#pragma unroll
      for (int to = 0; to < NTO; ++to) a[to] = an[to];
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti) b[ti] = bn[ti];
    }
  }
}

// Write NT transposed tiles of this wave (16 batch columns) into a staging image.
template <int NT>
RRL_DEV void stage_tiles(float* __restrict__ St, int wave, const floatx4 (&v)[NT]) {
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) St[(16 * t + 4 * g + r) * kStageLd + 16 * wave + j] = v[t][r];
  }
}

// Interleaved input tile (load_x_tile layout: reg r of group g = feature 16t + 4r + g)
// written into the staging image in natural feature order.
template <int NT>
RRL_DEV void stage_x_tiles(float* __restrict__ St, int wave, const floatx4 (&v)[NT]) {
  const int l = lane_id();
  const int j = l & 15, g = l >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) St[(16 * t + 4 * r + g) * kStageLd + 16 * wave + j] = v[t][r];
  }
}

}  // namespace rrl
