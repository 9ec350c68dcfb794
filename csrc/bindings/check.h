// Helpers shared by the kernel bindings (hip_ops.cpp, cnn_ops.cpp): every tensor is validated
// here before a launch, so that a bad call raises a Python exception instead of faulting the GPU.
#pragma once
#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <optional>

namespace rrl_bind {

using at::Tensor;
using OptT = std::optional<Tensor>;

// Launches go to the current HIP stream (capturable into a hipGraph via torch.cuda.graph).
inline void* cur_stream() { return (void*)at::hip::getCurrentHIPStream().stream(); }

// CUs the grids of this process are sized for (hip_ops.cpp: the device's, or set_cu_limit's).
int grid_cus();

// On its own where the minimum is known only after other arguments have been checked.
inline void check_numel(const Tensor& t, const char* name, int64_t min_numel) {
  TORCH_CHECK(t.numel() >= min_numel, name, " has ", t.numel(), " elements, need >= ", min_numel);
}

inline void check(const Tensor& t, const char* name, at::ScalarType dt, int64_t min_numel = 0) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  check_numel(t, name, min_numel);
}

// Null for an absent tensor, else its checked data pointer.
template <class T>
T* opt_ptr(const OptT& t, const char* name, at::ScalarType dt, int64_t min_numel) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check(*t, name, dt, min_numel);
  return reinterpret_cast<T*>(t->data_ptr());
}

// rc: 0, a hipError_t (> 0) or a kernel launcher's negative code (``negative`` words it).
inline void check_rc(int rc, const char* what, const char* negative = "bad argument") {
  TORCH_CHECK(rc == 0, what, " failed with code ", rc, " (", (rc > 0 ? hipGetErrorString((hipError_t)rc) : negative),
              ")");
}

// Outputs of a Q-network over A actions, and whether the combination is one the kernels have: A for the plain net,
// A + 1 (the state value) for the dueling one, A * quantiles for the quantile one (quantiles = 0: a scalar net),
// never both, and kMaxAct = 16 outputs are what the kernels hold.
inline int64_t q_outputs(int64_t A, bool dueling, int64_t quantiles) {
  TORCH_CHECK(quantiles >= 0, "quantiles must be >= 0, got ", quantiles);
  TORCH_CHECK(quantiles == 0 || !dueling, "quantiles with dueling is not built: set one of the two");
  TORCH_CHECK(A * quantiles <= 16, "a quantile net has A * quantiles <= 16 outputs, got ", A, " * ", quantiles);
  TORCH_CHECK(!dueling || A <= 15, "a dueling net has A + 1 outputs: act dim must be in [1, 15], got ", A);
  return quantiles > 0 ? A * quantiles : A + (dueling ? 1 : 0);
}

// Outputs of a categorical (C51) Q-network over A actions, A * atoms, and whether the kernels have it: it goes with
// neither the dueling nor the quantile head, has 2 <= atoms, v_min < v_max, and fits the wide output layer's 8 tiles
// of 16 outputs with every action's atoms rounded up to whole tiles.
inline int64_t c51_outputs(int64_t A, int64_t atoms, double v_min, double v_max, bool dueling, int64_t quantiles) {
  TORCH_CHECK(quantiles == 0, "atoms with quantiles is not built: set one of the two");
  TORCH_CHECK(!dueling, "atoms with dueling is not built: set one of the two");
  TORCH_CHECK(atoms >= 2, "atoms must be 0 or >= 2, got ", atoms);
  TORCH_CHECK(v_max > v_min, "atoms needs v_min < v_max, got v_min = ", v_min, " and v_max = ", v_max);
  TORCH_CHECK(A >= 1 && atoms <= 64 && A * ((atoms + 15) / 16) <= 8, "a categorical net has A * ceil(atoms / 16) <= 8 ",
              "output tiles, got A = ", A, " and atoms = ", atoms);
  return A * atoms;
}

// Munchausen targets (alpha = munchausen): alpha in [0, 1]; alpha > 0 needs a temperature > 0 and a clip < 0, has no
// argmax for double_q to select and is built for the plain and the quantile net.  Returns whether they are on.
inline bool munchausen_on(double munchausen, double m_tau, double m_clip, bool double_q, bool dueling, int64_t atoms) {
  TORCH_CHECK(munchausen >= 0.0 && munchausen <= 1.0, "munchausen must be in [0, 1], got ", munchausen);
  if (munchausen == 0.0) return false;
  TORCH_CHECK(m_tau > 0.0, "munchausen needs m_tau > 0, got ", m_tau);
  TORCH_CHECK(m_clip < 0.0, "munchausen needs m_clip < 0, got ", m_clip);
  TORCH_CHECK(!double_q, "munchausen with double_q is not built: the soft target has no argmax to select");
  TORCH_CHECK(!dueling, "munchausen with dueling is not built: set one of the two");
  TORCH_CHECK(atoms == 0, "munchausen with atoms is not built: set one of the two");
  return true;
}

// Lambda-return targets (lam = q_lambda): lam in [0, 1]; lam < 1 mixes the 1 .. n-step targets of a walk of 2 to 8
// steps on the scalar hard-max target, so it goes with neither distributional head nor the soft target.  Returns
// whether they are on.  A NaN fails the first comparison and is refused.
inline bool lambda_on(double q_lambda, int64_t n_step, int64_t quantiles, int64_t atoms, double munchausen) {
  TORCH_CHECK(q_lambda >= 0.0 && q_lambda <= 1.0, "q_lambda must be in [0, 1], got ", q_lambda);
  if (q_lambda == 1.0) return false;
  TORCH_CHECK(n_step >= 2 && n_step <= 8, "q_lambda = ", q_lambda, " needs n_step in [2, 8], got ", n_step);
  TORCH_CHECK(quantiles == 0, "q_lambda = ", q_lambda, " with quantiles = ", quantiles,
              " is not built: a mixture of return distributions is not the mean of their quantiles");
  TORCH_CHECK(atoms == 0, "q_lambda = ", q_lambda, " with atoms = ", atoms,
              " is not built: a mixture of return distributions is not the mean of their atoms");
  TORCH_CHECK(munchausen == 0.0, "q_lambda = ", q_lambda, " with munchausen = ", munchausen,
              " is not built: set one of the two");
  return true;
}

// Floats of MLPSpec(D, H, A) (+ log_std).
inline int64_t flat_size(int64_t D, int64_t H, int64_t A, bool log_std = false) {
  return H * D + H + H * H + H + A * H + A + (log_std ? A : 0);
}

}  // namespace rrl_bind
