// Arguments of the batched forward kernels (mlp_forward.hip, mlp_cat_wide.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rrl {

struct FwdArgs {
  const float* params;
  const float* X;        // [B][D]
  int B, D, A, H;
  const float* mask;     // [B][A] or null
  const int* act_in;     // [B] (CAT_EVAL)
  const float* actc_in;  // [B][A] (GAUSS_EVAL)
  int* act_out;          // [B]
  float* actc_out;       // [B][A]
  float* out0;           // v / logp
  float* out1;           // entropy (may be null)
  float* logits_out;     // [B][A] (MODE_LOGITS) or mean for Gaussian (may be null)
  uint32_t seed_lo, seed_hi;
  uint32_t step_lo, step_hi;
  uint32_t row_offset;   // stream id of row 0 (global env index)
  const float* gate;     // MODE_VALUE: [B] done codes; only 16-row tiles holding a code 2
                         // (time-limit truncation) are evaluated, or null = every row
  // host-env rollout (runtime/host_rollout.cpp): X may be PINNED HOST memory read over PCIe
  // (zero-copy); x_copy gets the rows in HBM for the learner and act_host / actc_host the
  // sampled actions in pinned host memory for the env threads -- one launch per half-step,
  // no H2D / D2H copies.  All null on the ordinary path.
  float* x_copy;         // [B][D] or null
  int* act_host;         // [B] or null (CAT_SAMPLE)
  float* actc_host;      // [B][A] or null (GAUSS_SAMPLE)
};

// Categorical policies of 17 .. 64 actions (mlp_cat_wide.hip): MODE_CAT_SAMPLE, MODE_CAT_EVAL and MODE_LOGITS at
// D <= 32, H = 64 or 128.  -2 for any other mode or shape, -3 for another H.
int launch_fwd_cat_wide(const FwdArgs& a, int mode, int num_cu, hipStream_t s);

}  // namespace rrl
