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

}  // namespace rrl_bind
