// Prioritised experience replay (Schaul et al., proportional variant): the priority sum tree.
//
// The ring of the DQN path has L = C * N rows (row = slot * N + env); P2 is the smallest power of two
// >= L.  tree is fp32 [2 * P2]: node 1 the root, the leaf of row r at tree[P2 + r], padding leaves and
// rows never written 0.  pmax (one float, 1.0 at the start) is the running maximum of every leaf value
// ever assigned.  The contract of every launch here: afterwards every internal node is ONE fp32 add of
// its two children, tree[i] == tree[2i] + tree[2i + 1].  That makes the tree a pure function of its
// leaves (a checkpoint saves the leaves and rebuilds it) and lets a numpy oracle predict the sampled rows
// bit for bit.  So no float atomic adds and no delta propagation: every touched node is recomputed from
// its children, level by level.
//
// Both kernels are ONE workgroup of 1024 threads that walks the levels bottom-up with a workgroup
// barrier between levels: no cross-CU hand-off, nothing depends on a grid.  Nodes a level above were
// written by other waves of this workgroup, and the leaves of rrl_per_update by atomics that execute in
// L2, so every child is read with a relaxed agent-scope load (served by L2, never a stale L1 line) and
// every node written with the matching store.  Threads loop where a level has more touched nodes than
// the workgroup has threads; duplicates recompute the same value.
#include "api.h"
#include "common.h"

namespace rrl {

constexpr int kPerThreads = 1024;

RRL_DEV float tree_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RRL_DEV void tree_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Every store of this wave has reached L2 before any wave of the workgroup passes the barrier.
RRL_DEV void level_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// node <- left child + right child: the one fp32 add of the invariant
RRL_DEV void tree_refresh(float* tree, uint32_t node) {
  const float l = tree_load(tree + 2 * (size_t)node);
  const float r = tree_load(tree + 2 * (size_t)node + 1);
  tree_store(tree + node, l + r);
}

// Leaves [row0, row0 + n) <- *pmax.  The touched nodes of a level are one contiguous range.
__global__ __launch_bounds__(kPerThreads) void per_insert_kernel(float* tree, const float* pmax, uint32_t P2,
                                                                 int levels, uint32_t row0, uint32_t n) {
  const float v = *pmax;
  for (uint32_t i = threadIdx.x; i < n; i += kPerThreads) tree_store(tree + P2 + row0 + i, v);
  const uint32_t first = P2 + row0, last = P2 + row0 + n - 1;
  for (int k = 1; k <= levels; ++k) {
    level_barrier();
    const uint32_t lo = first >> k, hi = last >> k;
    for (uint32_t node = lo + threadIdx.x; node <= hi; node += kPerThreads) tree_refresh(tree, node);
  }
}

// New leaf of row r = the maximum over the batch rows that sampled r of (td_abs + eps)^alpha.  The
// leaves are first zeroed, then raised by a maximum on the int bits of the non-negative floats: the
// result does not depend on the order of the batch rows.
__global__ __launch_bounds__(kPerThreads) void per_update_kernel(float* tree, float* pmax, const int* idx,
                                                                 const float* td_abs, int B, uint32_t L, uint32_t P2,
                                                                 int levels, float alpha, float prio_eps) {
  __shared__ float red[kPerThreads / 64];
  const float pm = *pmax;
  for (int b = threadIdx.x; b < B; b += kPerThreads) {
    const uint32_t r = (uint32_t)idx[b];
    if (r < L) tree_store(tree + P2 + r, 0.f);
  }
  level_barrier();
  float mine = pm;
  for (int b = threadIdx.x; b < B; b += kPerThreads) {
    const uint32_t r = (uint32_t)idx[b];
    if (r >= L) continue;
    const float td = fabsf(td_abs[b]);
    float v = powf(td + prio_eps, alpha);
    if (!(td <= 3.0e38f) || !(v <= 3.0e38f)) v = pm;  // NaN or infinity: the tree never holds either
    atomicMax(reinterpret_cast<int*>(tree + P2 + r), __float_as_int(v));
    mine = fmaxf(mine, v);
  }
  // pmax <- max(pmax, every new leaf): wave maximum, then the 16 waves through LDS
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine = fmaxf(mine, __shfl_xor(mine, off));
  if (lane_id() == 0) red[threadIdx.x >> 6] = mine;
  for (int k = 1; k <= levels; ++k) {
    level_barrier();
    for (int b = threadIdx.x; b < B; b += kPerThreads) {
      const uint32_t r = (uint32_t)idx[b];
      if (r < L) tree_refresh(tree, (P2 + r) >> k);
    }
  }
  if (levels == 0) __syncthreads();
  if (threadIdx.x == 0) {
    float m = red[0];
#pragma unroll
    for (int w = 1; w < kPerThreads / 64; ++w) m = fmaxf(m, red[w]);
    *pmax = m;
  }
}

struct PerShape {
  uint32_t P2;
  int levels;
};

static bool per_shape(long long L, PerShape* s) {
  if (L < 1 || L > (1ll << 30)) return false;
  s->P2 = 1;
  s->levels = 0;
  while ((long long)s->P2 < L) {
    s->P2 <<= 1;
    ++s->levels;
  }
  return true;
}

}  // namespace rrl

using namespace rrl;

extern "C" long long rrl_per_tree_leaves(long long L) {
  PerShape s;
  return per_shape(L, &s) ? (long long)s.P2 : 0;
}

extern "C" int rrl_per_insert(float* tree, const float* pmax, int C, int N, int T, int slot0, void* stream) {
  if (!tree || !pmax) return -1;
  PerShape s;
  if (N <= 0 || T <= 0 || C <= 0 || !per_shape((long long)C * N, &s)) return -2;
  if (slot0 < 0 || C % T != 0 || slot0 % T != 0 || (long long)slot0 + T > C) return -4;
  hipLaunchKernelGGL(per_insert_kernel, dim3(1), dim3(kPerThreads), 0, (hipStream_t)stream, tree, pmax, s.P2, s.levels,
                     (uint32_t)((long long)slot0 * N), (uint32_t)((long long)T * N));
  return (int)hipGetLastError();
}

extern "C" int rrl_per_update(float* tree, float* pmax, const int* idx, const float* td_abs, int B, long long L,
                              float alpha, float prio_eps, void* stream) {
  if (!tree || !pmax || !idx || !td_abs) return -1;
  PerShape s;
  if (B < 1 || !per_shape(L, &s) || !(alpha >= 0.f) || !(prio_eps > 0.f)) return -2;
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kPerThreads), 0, (hipStream_t)stream, tree, pmax, idx, td_abs, B,
                     (uint32_t)L, s.P2, s.levels, alpha, prio_eps);
  return (int)hipGetLastError();
}
