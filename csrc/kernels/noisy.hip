// NoisyNet exploration (Fortunato et al. 2018, factorised Gaussian noise) for the DQN path.
//
// A noisy Q-network keeps theta = [mu (P); sigma (P)] in the flat MLPSpec layout and every kernel that reads
// weights (dqn_rollout, dqn_targets, mlp_grad) gets the effective parameters mu + sigma * eps of one
// (role, draw) instead.  So the feature is two small kernels around launches that stay as they are:
//
//   rrl_noisy_compose  out[k] = mu_k + sigma_k * eps(role_k, draw_k) for up to three jobs in one launch
//   rrl_noisy_grad     [sum of the gradient slabs; that sum * eps(role, draw)], the gradient of [mu; sigma]
//
// The noise (docs/KERNELS.md has the contract): unit i of (role r, layer l = 1..3, side s = 0 in / 1 out) at
// the 64-bit draw d takes the Philox word at counter (i, lo32(d), hi32(d), 16 + 8 r + 2 (l - 1) + s);
//   n = sqrtf(-2 logf(1 - u01(w.x))) * cosf(6.283185307179586f * u01(w.y)),  f = copysignf(sqrtf(fabsf(n)), n)
// with the precise library functions, eps_W[j][i] = f_out[j] * f_in[i], eps_b[j] = f_out[j], and the effective
// weight is ONE fp32 multiply and ONE fp32 add, never contracted into an fma, so a torch fp32 expression on
// the CPU reproduces everything after the unit factors bit for bit.
//
// Only U = D + 4 H + A_out <= 544 units exist per (role, draw).  Every workgroup fills all of them into LDS
// (two or three Philox words per thread), and after one barrier streams its slice of the P elements; an
// element is a pure function of its index, so nothing depends on the grid.  P may be odd: scalar accesses.
#include "api.h"
#include "common.h"

// Everything below is exact fp32: no fma contraction in this file.
#pragma clang fp contract(off)

namespace rrl {

constexpr int kNoisyThreads = 256;
constexpr int kNoisyMaxUnits = 16 + 4 * 128 + 16;
constexpr int kNoisyMaxJobs = 3;

struct NoisyGeom {
  int D, H, A, P, U;
};

// Unit factor u (index into [in1 (D), out1 (H), in2 (H), out2 (H), in3 (H), out3 (A)]) of (role, draw).
RRL_DEV float noisy_unit(int u, int role, uint64_t draw, uint2 key, const NoisyGeom& g) {
  int blk, i;  // blk = 2 (l - 1) + s
  if (u < g.D) {
    blk = 0;
    i = u;
  } else {
    const int v = u - g.D;
    blk = 1 + v / g.H;  // 1 .. 5; the last block holds A <= H units
    i = v - (blk - 1) * g.H;
  }
  const uint4 w = philox4x32(make_uint4((uint32_t)i, (uint32_t)draw, (uint32_t)(draw >> 32), (uint32_t)(16 + 8 * role + blk)), key);
  const float u0 = u01(w.x), u1 = u01(w.y);
  const float n = sqrtf(-2.0f * logf(1.0f - u0)) * cosf(6.283185307179586f * u1);
  return copysignf(sqrtf(fabsf(n)), n);
}

RRL_DEV void noisy_fill_units(float* f, int role, uint64_t draw, uint2 key, const NoisyGeom& g) {
  for (int u = threadIdx.x; u < g.U; u += kNoisyThreads) f[u] = noisy_unit(u, role, draw, key, g);
  __syncthreads();
}

// eps of flat parameter p from the unit factors in LDS
RRL_DEV float noisy_eps(const float* f, int p, const NoisyGeom& g) {
  const int D = g.D, H = g.H, A = g.A;
  const float* in1 = f;
  const float* out1 = in1 + D;
  const float* in2 = out1 + H;
  const float* out2 = in2 + H;
  const float* in3 = out2 + H;
  const float* out3 = in3 + H;
  if (p < H * D) return out1[p / D] * in1[p % D];
  p -= H * D;
  if (p < H) return out1[p];
  p -= H;
  if (p < H * H) return out2[p / H] * in2[p % H];
  p -= H * H;
  if (p < H) return out2[p];
  p -= H;
  if (p < A * H) return out3[p / H] * in3[p % H];
  p -= A * H;
  return out3[p];
}

struct NoisyComposeArgs {
  const float* theta[kNoisyMaxJobs];
  uint64_t draw[kNoisyMaxJobs];
  int role[kNoisyMaxJobs];
  NoisyGeom g;
  uint2 key;
  float* out;
  float* units_out;
};

// blockIdx.y = the job, blockIdx.x strides over P
__global__ __launch_bounds__(kNoisyThreads) void noisy_compose_kernel(NoisyComposeArgs a) {
  __shared__ float f[kNoisyMaxUnits];
  const int k = blockIdx.y;
  const NoisyGeom g = a.g;
  noisy_fill_units(f, a.role[k], a.draw[k], a.key, g);
  if (a.units_out && blockIdx.x == 0) {
    for (int u = threadIdx.x; u < g.U; u += kNoisyThreads) a.units_out[(size_t)k * g.U + u] = f[u];
  }
  const float* mu = a.theta[k];
  const float* sigma = mu + g.P;
  float* out = a.out + (size_t)k * g.P;
  for (int p = blockIdx.x * kNoisyThreads + threadIdx.x; p < g.P; p += gridDim.x * kNoisyThreads) {
    const float se = sigma[p] * noisy_eps(f, p, g);
    out[p] = mu[p] + se;
  }
}

__global__ __launch_bounds__(kNoisyThreads) void noisy_grad_kernel(const float* slab, int nslab, int role, uint64_t draw,
                                                                   NoisyGeom g, uint2 key, float* grad_out) {
  __shared__ float f[kNoisyMaxUnits];
  noisy_fill_units(f, role, draw, key, g);
  for (int p = blockIdx.x * kNoisyThreads + threadIdx.x; p < g.P; p += gridDim.x * kNoisyThreads) {
    const float* s = slab + p;
    float acc = s[0];
    int k = 1;
    for (; k + 8 <= nslab; k += 8) {  // eight loads in flight, the adds in ascending slab order
      float q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = s[(size_t)(k + i) * g.P];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = acc + q[i];
    }
    for (; k < nslab; ++k) acc = acc + s[(size_t)k * g.P];
    grad_out[p] = acc;
    grad_out[g.P + p] = acc * noisy_eps(f, p, g);
  }
}

// 0, or the refusal code of both entry points for the net's shape
static int noisy_geom(int D, int H, int A, NoisyGeom* g) {
  if (D < 1 || D > 16 || A < 1 || A > kMaxAct) return -2;
  if (H != 64 && H != 128) return -3;
  *g = NoisyGeom{D, H, A, H * D + H + H * H + H + A * H + A, D + 4 * H + A};
  return 0;
}

static int noisy_grid(int P, int num_cu) {
  const int blocks = (P + kNoisyThreads - 1) / kNoisyThreads;
  const int cap = num_cu > 0 ? num_cu : 256;
  return blocks < cap ? blocks : cap;
}

}  // namespace rrl

using namespace rrl;

extern "C" int rrl_noisy_compose(const float* const* theta, int njobs, const int* roles, const uint64_t* draws, int D,
                                 int H, int A_out, uint64_t key, float* out, float* units_out, int num_cu,
                                 void* stream) {
  if (!theta || !roles || !draws || !out) return -1;
  if (njobs < 1 || njobs > kNoisyMaxJobs) return -2;
  NoisyComposeArgs a{};
  for (int k = 0; k < njobs; ++k) {
    if (!theta[k]) return -1;
    if (roles[k] < 0 || roles[k] > 3) return -2;
    a.theta[k] = theta[k];
    a.role[k] = roles[k];
    a.draw[k] = draws[k];
  }
  if (const int rc = noisy_geom(D, H, A_out, &a.g)) return rc;
  a.key = make_uint2((uint32_t)key, (uint32_t)(key >> 32));
  a.out = out;
  a.units_out = units_out;
  hipLaunchKernelGGL(noisy_compose_kernel, dim3(noisy_grid(a.g.P, num_cu), njobs), dim3(kNoisyThreads), 0,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int rrl_noisy_grad(const float* slab, int nslab, int P, int role, uint64_t draw, int D, int H, int A_out,
                              uint64_t key, float* grad_out, int num_cu, void* stream) {
  if (!slab || !grad_out) return -1;
  if (nslab < 1 || role < 0 || role > 3) return -2;
  NoisyGeom g;
  if (const int rc = noisy_geom(D, H, A_out, &g)) return rc;
  if (P != g.P) return -2;
  hipLaunchKernelGGL(noisy_grad_kernel, dim3(noisy_grid(P, num_cu)), dim3(kNoisyThreads), 0, (hipStream_t)stream, slab,
                     nslab, role, draw, g, make_uint2((uint32_t)key, (uint32_t)(key >> 32)), grad_out);
  return (int)hipGetLastError();
}
