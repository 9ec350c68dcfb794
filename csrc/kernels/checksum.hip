// Rollout payload checksum + header verification (docs/KERNELS.md "Rollout integrity").
//
// The actor -> learner payload (observations, actions, log-probs, rewards, dones, header) is
// treated as ONE sequence of 32-bit words w_0 .. w_{n-1}: the concatenation, in a fixed order,
// of up to 8 contiguous segments.  Two sums modulo 2^64 over the BIT PATTERNS of the words
//
//     s1 = sum_i w_i            s2 = sum_i (i + 1) * w_i
//
// are computed in integer arithmetic only, so the result is exact and independent of the launch
// geometry and of the summation order: two ranks (or two CU limits) always agree, -0.0 and every
// NaN payload count as their bits.  A change to one word changes s1; a swap of two unequal words
// or a shifted / replayed block changes s2.
//
// Read-only streaming kernel: 16-byte loads over the 16-byte-aligned body of every segment
// (4 in flight per lane), scalar loads for the <= 3 head and <= 3 tail words of a segment that
// starts or ends off a 16-byte boundary.  Per-lane uint64 accumulators -> wave shuffle
// reduction -> LDS block reduction -> one (s1, s2) partial per workgroup, stored plainly; a
// one-workgroup finishing launch on the same stream sums the partials into the two result words
// (integer adds commute: bit-deterministic for every grid).  No atomics: 2 x 2048 adds to the
// same two words serialise at ~10 ns each and took 38 us for a 21 MB payload, ten times the read.
#include "api.h"
#include "common.h"

namespace rrl {

constexpr int kCkMaxSeg = 8;
constexpr int kCkBlock = 256;

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

struct CkSeg {
  const uint32_t* p;        // 4-byte aligned
  unsigned long long n;     // words
  unsigned long long base;  // index of the segment's first word in the concatenation
};

struct CkArgs {
  CkSeg seg[kCkMaxSeg];
  int nseg;
  unsigned long long* part;  // [gridDim.x][2] per-workgroup (s1, s2)
};

RRL_DEV unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// words 4j .. 4j+3 of the body; i1 = (global index of word 4j) + 1
RRL_DEV void ck_acc4(const uintx4 v, unsigned long long i1, unsigned long long& s1, unsigned long long& s2) {
  const unsigned long long a = (unsigned long long)v[0] + v[1] + v[2] + v[3];
  const unsigned long long b = (unsigned long long)v[1] + 2ull * v[2] + 3ull * v[3];
  s1 += a;
  s2 += i1 * a + b;
}

__global__ __launch_bounds__(kCkBlock) void payload_checksum_kernel(CkArgs a) {
  __shared__ unsigned long long red[2][kCkBlock / kWave];
  const unsigned long long gid = (unsigned long long)blockIdx.x * kCkBlock + threadIdx.x;
  const unsigned long long stride = (unsigned long long)gridDim.x * kCkBlock;
  unsigned long long s1 = 0, s2 = 0;
  for (int s = 0; s < a.nseg; ++s) {
    const uint32_t* __restrict__ p = a.seg[s].p;
    const unsigned long long n = a.seg[s].n, base = a.seg[s].base;
    // head: words before the first 16-byte boundary (0..3, never more than n)
    unsigned long long head = ((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const unsigned long long nvec = (n - head) >> 2;
    const unsigned long long tail0 = head + 4 * nvec;  // first tail word; n - tail0 in 0..3
    if (gid < head) {
      const unsigned long long w = p[gid];
      s1 += w;
      s2 += (base + gid + 1) * w;
    }
    if (gid < n - tail0) {
      const unsigned long long w = p[tail0 + gid];
      s1 += w;
      s2 += (base + tail0 + gid + 1) * w;
    }
    const uintx4* __restrict__ pv = reinterpret_cast<const uintx4*>(p + head);
    const unsigned long long i0 = base + head + 1;
    unsigned long long j = gid;
    for (; j + 3 * stride < nvec; j += 4 * stride) {
      const uintx4 v0 = pv[j], v1 = pv[j + stride], v2 = pv[j + 2 * stride], v3 = pv[j + 3 * stride];
      ck_acc4(v0, i0 + 4 * j, s1, s2);
      ck_acc4(v1, i0 + 4 * (j + stride), s1, s2);
      ck_acc4(v2, i0 + 4 * (j + 2 * stride), s1, s2);
      ck_acc4(v3, i0 + 4 * (j + 3 * stride), s1, s2);
    }
    for (; j < nvec; j += stride) ck_acc4(pv[j], i0 + 4 * j, s1, s2);
  }
  s1 = wave_sum_u64(s1);
  s2 = wave_sum_u64(s2);
  const int wave = threadIdx.x / kWave;
  if (lane_id() == 0) {
    red[0][wave] = s1;
    red[1][wave] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t1 = 0, t2 = 0;
#pragma unroll
    for (int w = 0; w < kCkBlock / kWave; ++w) {
      t1 += red[0][w];
      t2 += red[1][w];
    }
    a.part[2 * blockIdx.x] = t1;
    a.part[2 * blockIdx.x + 1] = t2;
  }
}

// out[0..1] = column sums of part[nblocks][2]; one workgroup, launched behind the kernel above.
__global__ __launch_bounds__(kCkBlock) void payload_checksum_finish_kernel(const unsigned long long* __restrict__ part,
                                                                           int nblocks,
                                                                           unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[2][kCkBlock / kWave];
  unsigned long long s1 = 0, s2 = 0;
  for (int b = threadIdx.x; b < nblocks; b += kCkBlock) {
    s1 += part[2 * b];
    s2 += part[2 * b + 1];
  }
  s1 = wave_sum_u64(s1);
  s2 = wave_sum_u64(s2);
  const int wave = threadIdx.x / kWave;
  if (lane_id() == 0) {
    red[0][wave] = s1;
    red[1][wave] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t1 = 0, t2 = 0;
#pragma unroll
    for (int w = 0; w < kCkBlock / kWave; ++w) {
      t1 += red[0][w];
      t2 += red[1][w];
    }
    out[0] = t1;
    out[1] = t2;
  }
}

// status[k]: bit 0 = recomputed sums differ from header columns ck_col, ck_col + 1 (raw 64-bit
// integers), bit 1 = header seq (column 0) != expected, bit 2 = header version (column 7)
// outside [lo, hi].  One thread per slot.
__global__ void payload_verify_kernel(const unsigned long long* __restrict__ sums, const double* __restrict__ hdr,
                                      int ld, int ck_col, int K, double expected_seq, double lo, double hi,
                                      int* __restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double* h = hdr + (size_t)k * ld;
  const unsigned long long* hw = reinterpret_cast<const unsigned long long*>(h);
  int st = 0;
  if (hw[ck_col] != sums[2 * k] || hw[ck_col + 1] != sums[2 * k + 1]) st |= 1;
  if (!(h[0] == expected_seq)) st |= 2;
  if (!(h[7] >= lo && h[7] <= hi)) st |= 4;
  status[k] = st;
}

}  // namespace rrl

using namespace rrl;

// Workgroups of the checksum launch for these segment lengths: 4 x 16 B in flight per lane, at most
// 8 workgroups per CU, the rest grid-strides.  The caller's workspace holds 2 words per workgroup.
extern "C" int rrl_payload_checksum_blocks(const unsigned long long* words, int nseg, int num_cu) {
  unsigned long long nvec = 0;
  for (int s = 0; s < nseg && s < kCkMaxSeg; ++s) nvec += words[s] / 4 + 1;
  const unsigned long long per_block = (unsigned long long)kCkBlock * 4;
  unsigned long long grid = (nvec + per_block - 1) / per_block;
  const unsigned long long cap = (unsigned long long)(num_cu > 0 ? num_cu : 1) * 8;
  if (grid > cap) grid = cap;
  return grid < 1 ? 1 : (int)grid;
}

// nseg (pointer, word count) pairs in payload order; part: rrl_payload_checksum_blocks() x 2 words of
// workspace on the device; out: two 64-bit words on the device.
extern "C" int rrl_payload_checksum(const void* const* ptrs, const unsigned long long* words, int nseg,
                                    unsigned long long* part, unsigned long long* out, int num_cu, void* stream) {
  if (nseg < 0 || nseg > kCkMaxSeg || out == nullptr || part == nullptr) return -1;
  CkArgs a;
  unsigned long long total = 0;
  for (int s = 0; s < kCkMaxSeg; ++s) {
    if (s < nseg) {
      if (((uintptr_t)ptrs[s] & 3u) != 0 || (words[s] != 0 && ptrs[s] == nullptr)) return -1;
      a.seg[s] = CkSeg{static_cast<const uint32_t*>(ptrs[s]), words[s], total};
      total += words[s];
    } else {
      a.seg[s] = CkSeg{nullptr, 0, 0};
    }
  }
  a.nseg = nseg;
  a.part = part;
  const int grid = rrl_payload_checksum_blocks(words, nseg, num_cu);
  hipLaunchKernelGGL(payload_checksum_kernel, dim3((unsigned)grid), dim3(kCkBlock), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(payload_checksum_finish_kernel, dim3(1), dim3(kCkBlock), 0, (hipStream_t)stream, part, grid, out);
  return (int)hipGetLastError();
}

extern "C" int rrl_payload_verify(const unsigned long long* sums, const double* hdr, int ld, int ck_col, int K,
                                  double expected_seq, double lo, double hi, int* status, void* stream) {
  if (K < 1 || ld < 8 || ck_col < 0 || ld < ck_col + 2) return -1;
  hipLaunchKernelGGL(payload_verify_kernel, dim3((K + 63) / 64), dim3(64), 0, (hipStream_t)stream, sums, hdr, ld,
                     ck_col, K, expected_seq, lo, hi, status);
  return (int)hipGetLastError();
}
