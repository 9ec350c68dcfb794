// PyTorch bindings for the gfx950 HIP kernels (csrc/kernels/*.hip).
//
// The kernels are compiled by hipcc into plain objects with a C ABI; this file is
// compiled by the host C++ compiler against the PyTorch-ROCm headers, validates every
// tensor (device, dtype, contiguity, shape) BEFORE a launch so that a bad call raises a
// Python exception instead of faulting the GPU, and launches on the current HIP stream
// (so everything here is capturable into a hipGraph via torch.cuda.graph).
#include <algorithm>
#include <vector>

#include "api.h"
#include "check.h"

namespace {

using namespace rrl;
using namespace rrl_bind;

int g_cu_limit = 0;  // > 0: size every grid for this many CUs (set_cu_limit)

int device_cus() {
  static int n = -1;
  if (n < 0) n = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  return n;
}

// CUs the grids of this process are sized for: all of them, or the learner's share when the
// host-env trainer partitions the chip between its actor and learner streams.
int num_cus() { return g_cu_limit > 0 ? std::min(g_cu_limit, device_cus()) : device_cus(); }

int64_t set_cu_limit(int64_t n) {
  const int64_t prev = g_cu_limit;
  g_cu_limit = (int)std::max<int64_t>(n, 0);
  return prev;
}

// A stream whose kernels run only on the listed CUs (hipExtStreamCreateWithCUMask): the
// actor / learner partition of the overlapped host-env trainer, so the rollout's sampling
// launches never queue behind the learner's persistent one-workgroup-per-CU kernels.
int64_t cu_masked_stream(const std::vector<int64_t>& cus) {
  const int n = device_cus();
  std::vector<uint32_t> mask((n + 31) / 32, 0u);
  for (int64_t c : cus) {
    TORCH_CHECK(c >= 0 && c < n, "CU index ", c, " out of range [0, ", n, ")");
    mask[c / 32] |= 1u << (c % 32);
  }
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
  TORCH_CHECK(e == hipSuccess, "hipExtStreamCreateWithCUMask: ", hipGetErrorString(e));
  return (int64_t)(uintptr_t)st;
}

void destroy_stream(int64_t st) {
  if (st) (void)hipStreamDestroy((hipStream_t)(uintptr_t)st);
}

int64_t flat_size(int64_t D, int64_t H, int64_t A, bool log_std) {
  return H * D + H + H * H + H + A * H + A + (log_std ? A : 0);
}

void mlp_forward(int64_t mode, const Tensor& params, const Tensor& X, int64_t A, int64_t H, const OptT& mask,
                 const OptT& act_in, const OptT& actc_in, const OptT& act_out, const OptT& actc_out,
                 const Tensor& out0, const OptT& out1, const OptT& logits_out, int64_t seed, int64_t step,
                 int64_t row_offset, const OptT& gate) {
  check(params, "params", at::kFloat);
  check(X, "X", at::kFloat);
  TORCH_CHECK(X.dim() == 2, "X must be [B, D]");
  const int64_t B = X.size(0), D = X.size(1);
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(D >= 1 && D <= 32, "obs dim must be in [1, 32]");
  TORCH_CHECK(A >= 1 && A <= 16, "act dim must be in [1, 16]");
  TORCH_CHECK(mode >= MODE_VALUE && mode <= MODE_GAUSS_EVAL, "bad mode");
  const bool gauss = mode == MODE_GAUSS_SAMPLE || mode == MODE_GAUSS_EVAL;
  const int64_t Aeff = mode == MODE_VALUE ? 1 : A;
  check_numel(params, "params", flat_size(D, H, Aeff, gauss));
  check(out0, "out0", at::kFloat, B);
  const float* m = opt_ptr<const float>(mask, "mask", at::kFloat, B * A);
  const int* ai = opt_ptr<const int>(act_in, "act_in", at::kInt, mode == MODE_CAT_EVAL ? B : 0);
  const float* ci = opt_ptr<const float>(actc_in, "actc_in", at::kFloat, mode == MODE_GAUSS_EVAL ? B * A : 0);
  if (mode == MODE_CAT_EVAL) TORCH_CHECK(ai != nullptr, "act_in required for CAT_EVAL");
  if (mode == MODE_GAUSS_EVAL) TORCH_CHECK(ci != nullptr, "actc_in required for GAUSS_EVAL");
  int* ao = opt_ptr<int>(act_out, "act_out", at::kInt, mode == MODE_CAT_SAMPLE ? B : 0);
  if (mode == MODE_CAT_SAMPLE) TORCH_CHECK(ao != nullptr, "act_out required for CAT_SAMPLE");
  float* co = opt_ptr<float>(actc_out, "actc_out", at::kFloat, mode == MODE_GAUSS_SAMPLE ? B * A : 0);
  if (mode == MODE_GAUSS_SAMPLE) TORCH_CHECK(co != nullptr, "actc_out required for GAUSS_SAMPLE");
  float* o1 = opt_ptr<float>(out1, "out1", at::kFloat, B);
  float* lo = opt_ptr<float>(logits_out, "logits_out", at::kFloat, B * A);
  if (mode == MODE_LOGITS) TORCH_CHECK(lo != nullptr, "logits_out required for LOGITS");
  const float* gt = opt_ptr<const float>(gate, "gate", at::kFloat, B);
  TORCH_CHECK(gt == nullptr || mode == MODE_VALUE, "gate applies to the VALUE mode only");
  const int rc = rrl_mlp_forward((int)mode, params.data_ptr<float>(), X.data_ptr<float>(), (int)B, (int)D, (int)A,
                                 (int)H, m, ai, ci, ao, co, out0.data_ptr<float>(), o1, lo, (uint64_t)seed,
                                 (uint64_t)step, (uint32_t)row_offset, gt, nullptr, nullptr, nullptr, num_cus(),
                                 cur_stream());
  check_rc(rc, "mlp_forward");
}

int64_t mlp_grad_slabs(int64_t B) { return rrl_mlp_grad_slabs((int)B, num_cus()); }

void mlp_grad(int64_t head, const Tensor& params, const Tensor& X, int64_t A, int64_t H, const OptT& mask,
              const OptT& act, const OptT& actc, const OptT& adv, const OptT& ret, const OptT& logp_old,
              const OptT& adv_stats, double inv_B, double clip_eps, double ent_coef, const Tensor& grad_slab,
              const Tensor& loss_slab, const OptT& nvalid, const OptT& inv_B_dev, const OptT& row_w,
              const OptT& w_norm, const OptT& td_abs) {
  check(params, "params", at::kFloat);
  check(X, "X", at::kFloat);
  TORCH_CHECK(X.dim() == 2, "X must be [B, D]");
  const int64_t B = X.size(0), D = X.size(1);
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(D >= 1 && D <= 32, "obs dim must be in [1, 32]");
  TORCH_CHECK(A >= 1 && A <= 16, "act dim must be in [1, 16]");
  TORCH_CHECK(head >= HEAD_PG_CAT && head <= HEAD_Q_DUEL, "bad head");
  TORCH_CHECK(B * std::max<int64_t>(D, A) < (int64_t)INT32_MAX, "batch too large for 32-bit row indexing");
  const bool gauss = head == HEAD_PPO_GAUSS || head == HEAD_PG_GAUSS;
  const bool cat = head == HEAD_PG_CAT || head == HEAD_PPO_CAT;
  const bool value = head == HEAD_VALUE_MSE;
  const bool duel = head == HEAD_Q_DUEL;       // the net has A + 1 outputs: A advantages and the state value
  const bool qtd = head == HEAD_Q_TD || duel;  // reads act + ret; no advantages
  TORCH_CHECK(!duel || A <= 15, "a dueling net has A + 1 outputs: act dim must be in [1, 15], got ", A);
  const int64_t P = flat_size(D, H, value ? 1 : (duel ? A + 1 : A), gauss);
  check_numel(params, "params", P);
  const int64_t nslab = mlp_grad_slabs(B);
  check(grad_slab, "grad_slab", at::kFloat, nslab * P);
  check(loss_slab, "loss_slab", at::kFloat, nslab * 8);
  const float* m = opt_ptr<const float>(mask, "mask", at::kFloat, B * A);
  const int* a = opt_ptr<const int>(act, "act", at::kInt, cat || qtd ? B : 0);
  if (cat || qtd) TORCH_CHECK(a != nullptr, "act required for categorical and Q heads");
  const float* ac = opt_ptr<const float>(actc, "actc", at::kFloat, gauss ? B * A : 0);
  if (gauss) TORCH_CHECK(ac != nullptr, "actc required for Gaussian heads");
  const float* ad = opt_ptr<const float>(adv, "adv", at::kFloat, B);
  if (!value && !qtd) TORCH_CHECK(ad != nullptr, "adv required for policy heads");
  const float* rt = opt_ptr<const float>(ret, "ret", at::kFloat, B);
  if (value || qtd) TORCH_CHECK(rt != nullptr, "ret required for the value and Q heads");
  const float* lpo = opt_ptr<const float>(logp_old, "logp_old", at::kFloat, B);
  if (head == HEAD_PPO_CAT || head == HEAD_PPO_GAUSS) TORCH_CHECK(lpo != nullptr, "logp_old required for PPO heads");
  const float* st = opt_ptr<const float>(adv_stats, "adv_stats", at::kFloat, 3);
  // device-side batch shape (graph replays with a changing batch): valid rows / 1 / global rows
  const int* nv = opt_ptr<const int>(nvalid, "nvalid", at::kInt, 1);
  const float* ibd = opt_ptr<const float>(inv_B_dev, "inv_B_dev", at::kFloat, 1);
  // prioritised replay (the Q head only): importance weights, their normaliser, |TD error| out
  const float* rw = opt_ptr<const float>(row_w, "row_w", at::kFloat, B);
  const float* wn = opt_ptr<const float>(w_norm, "w_norm", at::kFloat, 1);
  float* ta = opt_ptr<float>(td_abs, "td_abs", at::kFloat, B);
  TORCH_CHECK((rw == nullptr) == (wn == nullptr), "row_w and w_norm come together");
  TORCH_CHECK(qtd || (rw == nullptr && ta == nullptr), "row_w / w_norm / td_abs apply to the Q heads only");
  const int rc = rrl_mlp_grad_weighted((int)head, params.data_ptr<float>(), X.data_ptr<float>(), (int)B, (int)D,
                                       (int)A, (int)H, m, a, ac, ad, rt, lpo, st, (float)inv_B, (float)clip_eps,
                                       (float)ent_coef, grad_slab.data_ptr<float>(), loss_slab.data_ptr<float>(),
                                       (int)P, nv, ibd, rw, wn, ta, num_cus(), cur_stream());
  check_rc(rc, "mlp_grad");
}

// HEAD_Q_QR, the quantile-regression head (rrl_mlp_grad_qr): the net has A * quantiles outputs and ret is
// [B][quantiles].  A binding of its own, so that mlp_grad above stays what it was.
void mlp_grad_qr(const Tensor& params, const Tensor& X, int64_t A, int64_t quantiles, int64_t H, const Tensor& act,
                 const Tensor& ret, double inv_B, double kappa, const Tensor& grad_slab, const Tensor& loss_slab,
                 const OptT& nvalid, const OptT& inv_B_dev, const OptT& row_w, const OptT& w_norm, const OptT& td_abs) {
  check(params, "params", at::kFloat);
  check(X, "X", at::kFloat);
  TORCH_CHECK(X.dim() == 2, "X must be [B, D]");
  const int64_t B = X.size(0), D = X.size(1), NQ = quantiles;
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(D >= 1 && D <= 32, "obs dim must be in [1, 32]");
  TORCH_CHECK(A >= 1 && NQ >= 1 && A * NQ <= 16, "a quantile net has 1 <= A * quantiles <= 16 outputs, got ", A, " * ",
              NQ);
  TORCH_CHECK(kappa > 0.0, "the quantile head needs a Huber threshold > 0, got ", kappa);
  TORCH_CHECK(B >= 1 && B * std::max<int64_t>(D, A * NQ) < (int64_t)INT32_MAX,
              "batch out of range for 32-bit row indexing");
  const int64_t P = flat_size(D, H, A * NQ, false);
  TORCH_CHECK(params.numel() == P, "params has ", params.numel(), " floats; MLPSpec(D, H, A * quantiles) has ", P);
  const int64_t nslab = mlp_grad_slabs(B);
  check(grad_slab, "grad_slab", at::kFloat, nslab * P);
  check(loss_slab, "loss_slab", at::kFloat, nslab * 8);
  check(act, "act", at::kInt, B);
  check(ret, "ret", at::kFloat, B * NQ);
  const int* nv = opt_ptr<const int>(nvalid, "nvalid", at::kInt, 1);
  const float* ibd = opt_ptr<const float>(inv_B_dev, "inv_B_dev", at::kFloat, 1);
  const float* rw = opt_ptr<const float>(row_w, "row_w", at::kFloat, B);
  const float* wn = opt_ptr<const float>(w_norm, "w_norm", at::kFloat, 1);
  float* ta = opt_ptr<float>(td_abs, "td_abs", at::kFloat, B);
  TORCH_CHECK((rw == nullptr) == (wn == nullptr), "row_w and w_norm come together");
  check_rc(rrl_mlp_grad_qr(params.data_ptr<float>(), X.data_ptr<float>(), (int)B, (int)D, (int)A, (int)NQ, (int)H,
                           act.data_ptr<int>(), ret.data_ptr<float>(), (float)inv_B, (float)kappa,
                           grad_slab.data_ptr<float>(), loss_slab.data_ptr<float>(), (int)P, nv, ibd, rw, wn, ta,
                           num_cus(), cur_stream()),
           "mlp_grad_qr");
}

int64_t scan_tm_parts(int64_t N) { return rrl_scan_tm_parts((int)N); }

void gae_scan_tm(const Tensor& rew, const Tensor& done, const OptT& val, const OptT& tval, const Tensor& adv,
                 const Tensor& ret, const Tensor& stats_part, const OptT& stats_out, double gamma, double lam,
                 const std::vector<std::tuple<Tensor, int64_t>>& counters) {
  // rew [T, N] or [K, T, N] (K actor blocks of one learner shard); val [K*T*N + K*N]
  check(rew, "rew", at::kFloat);
  TORCH_CHECK(rew.dim() == 2 || rew.dim() == 3, "rew must be [T, N] or [K, T, N]");
  const int64_t K = rew.dim() == 3 ? rew.size(0) : 1;
  const int64_t T = rew.size(rew.dim() - 2), N = rew.size(rew.dim() - 1);
  check(done, "done", at::kFloat, K * T * N);
  const float* v = opt_ptr<const float>(val, "val", at::kFloat, K * (T + 1) * N);
  const float* tv = opt_ptr<const float>(tval, "tval", at::kFloat, K * T * N);
  check(adv, "adv", at::kFloat, K * T * N);
  check(ret, "ret", at::kFloat, K * T * N);
  check(stats_part, "stats_part", at::kFloat, scan_tm_parts(K * N) * 3);
  float* so = opt_ptr<float>(stats_out, "stats_out", at::kFloat, 3);
  // device step counters advanced by the same launch (int64 scalars on this device)
  TORCH_CHECK(counters.size() <= 3, "gae_scan_tm: at most 3 counters");
  long long* cnt[3] = {nullptr, nullptr, nullptr};
  long long inc[3] = {0, 0, 0};
  for (size_t q = 0; q < counters.size(); ++q) {
    const Tensor& c = std::get<0>(counters[q]);
    TORCH_CHECK(c.is_cuda() && c.scalar_type() == at::kLong && c.numel() == 1, "gae_scan_tm: counter must be an int64 scalar on the device");
    cnt[q] = reinterpret_cast<long long*>(c.data_ptr<int64_t>());
    inc[q] = (long long)std::get<1>(counters[q]);
  }
  const int rc = rrl_gae_scan_tm(rew.data_ptr<float>(), done.data_ptr<float>(), v, tv, adv.data_ptr<float>(),
                                 ret.data_ptr<float>(), stats_part.data_ptr<float>(), so, (int)K, (int)T, (int)N,
                                 (float)gamma, (float)lam, cnt, inc, (int)counters.size(), cur_stream());
  check_rc(rc, "gae_scan_tm");
}

// V-trace on the layout of gae_scan_tm; part holds scan_tm_parts(K * N) x 5 floats (scan.hip).
void vtrace_scan_tm(const Tensor& rew, const Tensor& done, const Tensor& val, const OptT& tval,
                    const Tensor& logp_mu, const Tensor& logp_pi, const Tensor& adv, const Tensor& ret,
                    const Tensor& part, const OptT& stats_out, const OptT& is_out, double gamma, double lam,
                    double rho_bar, double c_bar, double pg_rho_bar) {
  check(rew, "rew", at::kFloat);
  TORCH_CHECK(rew.dim() == 2 || rew.dim() == 3, "rew must be [T, N] or [K, T, N]");
  const int64_t K = rew.dim() == 3 ? rew.size(0) : 1;
  const int64_t T = rew.size(rew.dim() - 2), N = rew.size(rew.dim() - 1);
  TORCH_CHECK(K >= 1 && T >= 1 && N >= 1 && K * N <= (int64_t)INT32_MAX, "vtrace_scan_tm: empty or oversized batch [",
              K, ", ", T, ", ", N, "]");
  check(done, "done", at::kFloat, K * T * N);
  check(val, "val", at::kFloat, K * (T + 1) * N);
  const float* tv = opt_ptr<const float>(tval, "tval", at::kFloat, K * T * N);
  check(logp_mu, "logp_mu", at::kFloat);
  check(logp_pi, "logp_pi", at::kFloat);
  TORCH_CHECK(logp_mu.sizes() == rew.sizes() && logp_pi.sizes() == rew.sizes(),
              "logp_mu / logp_pi must have the shape of rew");
  check(adv, "adv", at::kFloat, K * T * N);
  check(ret, "ret", at::kFloat, K * T * N);
  check(part, "stats_part", at::kFloat, scan_tm_parts(K * N) * 5);
  float* so = opt_ptr<float>(stats_out, "stats_out", at::kFloat, 3);
  float* io = opt_ptr<float>(is_out, "is_out", at::kFloat, 2);
  TORCH_CHECK(rho_bar > 0 && c_bar > 0 && pg_rho_bar > 0, "vtrace_scan_tm: the clip thresholds must be positive");
  const int rc = rrl_vtrace_scan_tm(rew.data_ptr<float>(), done.data_ptr<float>(), val.data_ptr<float>(), tv,
                                    logp_mu.data_ptr<float>(), logp_pi.data_ptr<float>(), adv.data_ptr<float>(),
                                    ret.data_ptr<float>(), part.data_ptr<float>(), so, io, (int)K, (int)T, (int)N,
                                    (float)gamma, (float)lam, (float)rho_bar, (float)c_bar, (float)pg_rho_bar,
                                    cur_stream());
  check_rc(rc, "vtrace_scan_tm");
}

int64_t scan_flat_blocks(int64_t L) { return rrl_scan_flat_blocks((int)L); }

void scan_flat(const Tensor& rew, const Tensor& done, const OptT& val, const OptT& boot, const Tensor& adv,
               const Tensor& ret, const Tensor& work, const OptT& stats_out, double gamma, double lam) {
  check(rew, "rew", at::kFloat);
  const int64_t L = rew.numel();
  check(done, "done", at::kFloat, L);
  const float* v = opt_ptr<const float>(val, "val", at::kFloat, L);
  const float* b = opt_ptr<const float>(boot, "boot", at::kFloat, L);
  check(adv, "adv", at::kFloat, L);
  check(ret, "ret", at::kFloat, L);
  check(work, "work", at::kFloat, scan_flat_blocks(L) * 9);
  float* so = opt_ptr<float>(stats_out, "stats_out", at::kFloat, 3);
  const int rc = rrl_scan_flat(rew.data_ptr<float>(), done.data_ptr<float>(), v, b, adv.data_ptr<float>(),
                               ret.data_ptr<float>(), work.data_ptr<float>(), so, (int)L, (float)gamma, (float)lam,
                               cur_stream());
  check_rc(rc, "scan_flat");
}

void stats_reduce(const Tensor& part, const Tensor& out) {
  check(part, "part", at::kFloat);
  TORCH_CHECK(part.numel() % 3 == 0, "part must be [n, 3]");
  check(out, "out", at::kFloat, 3);
  check_rc(rrl_stats_reduce(part.data_ptr<float>(), (int)(part.numel() / 3), out.data_ptr<float>(), cur_stream()),
           "stats_reduce");
}

void column_sums(const Tensor& part, int64_t cols, const Tensor& out) {
  check(part, "part", at::kFloat);
  TORCH_CHECK(part.dim() == 2 && part.is_contiguous(), "column_sums: part must be a contiguous [rows, ld] tensor");
  TORCH_CHECK(cols >= 1 && cols <= 8 && cols <= part.size(1), "column_sums: 1 <= cols <= min(8, ld)");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kDouble && out.numel() >= cols && out.is_contiguous(),
              "column_sums: out must be a contiguous float64 device tensor of >= cols elements");
  check_rc(rrl_column_sums(part.data_ptr<float>(), (int)part.size(0), (int)part.size(1), (int)cols,
                           out.data_ptr<double>(), cur_stream()),
           "column_sums");
}

void adam(const Tensor& param, const Tensor& m, const Tensor& v, const OptT& grad, const OptT& slab,
          const OptT& grad_out, const Tensor& step, const Tensor& ticket, double lr, double beta1, double beta2,
          double eps, double grad_scale, double weight_decay, int64_t step_add, int64_t step_inc) {
  check(param, "param", at::kFloat);
  const int64_t P = param.numel();
  check(m, "m", at::kFloat, P);
  check(v, "v", at::kFloat, P);
  const float* g = opt_ptr<const float>(grad, "grad", at::kFloat, P);
  const float* s = nullptr;
  int64_t nslab = 0;
  if (slab.has_value() && slab->defined()) {
    check(*slab, "slab", at::kFloat);
    TORCH_CHECK(slab->dim() == 2 && slab->size(1) == P, "slab must be [nslab, P]");
    nslab = slab->size(0);
    s = slab->data_ptr<float>();
  }
  TORCH_CHECK((g != nullptr) != (s != nullptr), "exactly one of grad / slab must be given");
  float* go = opt_ptr<float>(grad_out, "grad_out", at::kFloat, P);
  check(step, "step", at::kInt);
  check(ticket, "ticket", at::kInt);
  const int rc = rrl_adam(param.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), g, s, (int)nslab, go,
                          step.data_ptr<int>(), reinterpret_cast<unsigned*>(ticket.data_ptr<int>()), (int)P, (float)lr,
                          (float)beta1, (float)beta2, (float)eps, (float)grad_scale, (float)weight_decay,
                          (int)step_add, (int)step_inc, cur_stream());
  check_rc(rc, "adam");
}

void reduce_slabs(const Tensor& slab, double scale, const Tensor& out) {
  check(slab, "slab", at::kFloat);
  TORCH_CHECK(slab.dim() == 2, "slab must be [nslab, P]");
  check(out, "out", at::kFloat, slab.size(1));
  check_rc(rrl_reduce_slabs(slab.data_ptr<float>(), (int)slab.size(0), (int)slab.size(1), (float)scale,
                            out.data_ptr<float>(), cur_stream()),
           "reduce_slabs");
}

// (s1, s2) over the bit patterns of up to 8 contiguous segments, in order (checksum.hip).
void payload_checksum(const std::vector<Tensor>& segments, const Tensor& out) {
  TORCH_CHECK(segments.size() <= 8, "payload_checksum: at most 8 segments, got ", segments.size());
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.numel() == 2 && out.is_contiguous(),
              "payload_checksum: out must be a contiguous int64[2] device tensor");
  const void* ptrs[8];
  unsigned long long words[8];
  for (size_t s = 0; s < segments.size(); ++s) {
    const Tensor& t = segments[s];
    TORCH_CHECK(t.is_cuda() && t.get_device() == out.get_device(), "payload_checksum: segment ", s,
                " must be on the device of out");
    TORCH_CHECK(t.is_contiguous(), "payload_checksum: segment ", s, " must be contiguous");
    const int64_t isz = (int64_t)t.element_size();
    TORCH_CHECK(isz % 4 == 0, "payload_checksum: segment ", s, " has dtype ", t.scalar_type(),
                "; the element size must be a multiple of 4 bytes");
    ptrs[s] = t.numel() ? t.data_ptr() : nullptr;
    words[s] = (unsigned long long)(t.numel() * (isz / 4));
    TORCH_CHECK(((uintptr_t)ptrs[s] & 3u) == 0, "payload_checksum: segment ", s, " is not 4-byte aligned");
  }
  // per-workgroup partials: from the caching allocator (stream-ordered reuse, no hipMalloc per call)
  const int nseg = (int)segments.size(), cus = num_cus();
  const Tensor part = at::empty({2 * (int64_t)rrl_payload_checksum_blocks(words, nseg, cus)}, out.options());
  check_rc(rrl_payload_checksum(ptrs, words, nseg, reinterpret_cast<unsigned long long*>(part.data_ptr<int64_t>()),
                                reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()), cus, cur_stream()),
           "payload_checksum");
}

// status[k] bits: 1 checksum mismatch, 2 seq != expected, 4 version outside [lo, hi] (checksum.hip).
void payload_verify(const Tensor& sums, const Tensor& hdr, int64_t ck_col, int64_t expected_seq, int64_t lo,
                    int64_t hi, const Tensor& status) {
  TORCH_CHECK(hdr.is_cuda() && hdr.scalar_type() == at::kDouble && hdr.dim() == 2 && hdr.is_contiguous(),
              "payload_verify: hdr must be a contiguous float64 [K, HDR] device tensor");
  const int64_t K = hdr.size(0), ld = hdr.size(1);
  TORCH_CHECK(K >= 1 && ld >= 8 && ck_col >= 0 && ck_col + 2 <= ld, "payload_verify: bad header shape [", K, ", ",
              ld, "] for checksum column ", ck_col);
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kLong && sums.is_contiguous() && sums.numel() == 2 * K,
              "payload_verify: sums must be a contiguous int64 [K, 2] device tensor");
  check(status, "status", at::kInt);
  TORCH_CHECK(status.numel() == K, "payload_verify: status must have K elements");
  check_rc(rrl_payload_verify(reinterpret_cast<const unsigned long long*>(sums.data_ptr<int64_t>()),
                              hdr.data_ptr<double>(), (int)ld, (int)ck_col, (int)K, (double)expected_seq,
                              (double)lo, (double)hi, status.data_ptr<int>(), cur_stream()),
           "payload_verify");
}

std::tuple<int64_t, int64_t, int64_t, int64_t> env_dims(int64_t env) {
  int D = 0, A = 0, NS = 0, ms = 0;
  TORCH_CHECK(rrl_env_dims((int)env, &D, &A, &NS, &ms) == 0, "unknown device env id ", env);
  return {D, A, NS, ms};
}

int64_t rollout_grid(int64_t N) { return rrl_rollout_grid((int)N, num_cus()); }

// The buffers rollout() and rollout_cont() have in common, for T steps of N envs with D observation
// and NS state floats each; returns tobs_buf's pointer (null when absent).
float* check_rollout_bufs(int64_t T, int64_t N, int64_t D, int64_t NS, const Tensor& state, const Tensor& ep_len,
                          const Tensor& ep_ret, const Tensor& obs_buf, const Tensor& logp_buf, const Tensor& rew_buf,
                          const Tensor& done_buf, const Tensor& ep_stats, const OptT& tobs_buf) {
  check(state, "state", at::kFloat, N * NS);
  check(ep_len, "ep_len", at::kInt, N);
  check(ep_ret, "ep_ret", at::kFloat, N);
  check(obs_buf, "obs_buf", at::kFloat, (T + 1) * N * D);
  check(logp_buf, "logp_buf", at::kFloat, T * N);
  check(rew_buf, "rew_buf", at::kFloat, T * N);
  check(done_buf, "done_buf", at::kFloat, T * N);
  check(ep_stats, "ep_stats", at::kFloat, rollout_grid(N) * 8);
  return opt_ptr<float>(tobs_buf, "tobs_buf", at::kFloat, T * N * D);
}

void rollout(int64_t env, const Tensor& params, int64_t H, const Tensor& state, const Tensor& ep_len,
             const Tensor& ep_ret, const Tensor& obs_buf, const Tensor& act_buf, const Tensor& logp_buf,
             const Tensor& rew_buf, const Tensor& done_buf, const OptT& tobs_buf, const Tensor& ep_stats,
             int64_t seed, int64_t step0, bool reset_all, int64_t max_steps) {
  auto [D, A, NS, ms] = env_dims(env);
  (void)ms;
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  check(params, "params", at::kFloat, flat_size(D, H, A, false));
  check(act_buf, "act_buf", at::kInt);
  TORCH_CHECK(act_buf.dim() == 2, "act_buf must be [T, N]");
  const int64_t T = act_buf.size(0), N = act_buf.size(1);
  float* tob = check_rollout_bufs(T, N, D, NS, state, ep_len, ep_ret, obs_buf, logp_buf, rew_buf, done_buf, ep_stats,
                                  tobs_buf);
  const int rc = rrl_rollout((int)env, params.data_ptr<float>(), (int)N, (int)T, (int)H, state.data_ptr<float>(),
                             ep_len.data_ptr<int>(), ep_ret.data_ptr<float>(), obs_buf.data_ptr<float>(),
                             act_buf.data_ptr<int>(), logp_buf.data_ptr<float>(), rew_buf.data_ptr<float>(),
                             done_buf.data_ptr<float>(), tob, ep_stats.data_ptr<float>(), (uint64_t)seed, (uint64_t)step0,
                             reset_all ? 1 : 0, (int)max_steps, num_cus(), cur_stream());
  check_rc(rc, "rollout");
}

// Continuous-action fused rollout (diagonal Gaussian policy; env id 4 = HalfCheetahSynth).
void rollout_cont(int64_t env, const Tensor& params, const Tensor& env_consts, int64_t H, const Tensor& state,
                  const Tensor& ep_len, const Tensor& ep_ret, const Tensor& obs_buf, const Tensor& act_buf,
                  const Tensor& logp_buf, const Tensor& rew_buf, const Tensor& done_buf, const OptT& tobs_buf,
                  const Tensor& ep_stats, int64_t seed, int64_t step0, bool reset_all, int64_t max_steps) {
  auto [D, A, NS, ms] = env_dims(env);
  (void)ms;
  TORCH_CHECK(env == ENV_HALFCHEETAH, "rollout_cont supports the continuous device env 4 (HalfCheetahSynth)");
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  check(params, "params", at::kFloat, flat_size(D, H, A, true));
  check(env_consts, "env_consts", at::kFloat, 17 * 17 + 17 * 6);
  check(act_buf, "act_buf", at::kFloat);
  TORCH_CHECK(act_buf.dim() == 3 && act_buf.size(2) == A, "act_buf must be [T, N, A]");
  const int64_t T = act_buf.size(0), N = act_buf.size(1);
  float* tob = check_rollout_bufs(T, N, D, NS, state, ep_len, ep_ret, obs_buf, logp_buf, rew_buf, done_buf, ep_stats,
                                  tobs_buf);
  check_rc(rrl_rollout_cont((int)env, params.data_ptr<float>(), env_consts.data_ptr<float>(), (int)N, (int)T, (int)H,
                            state.data_ptr<float>(), ep_len.data_ptr<int>(), ep_ret.data_ptr<float>(),
                            obs_buf.data_ptr<float>(), act_buf.data_ptr<float>(), logp_buf.data_ptr<float>(),
                            rew_buf.data_ptr<float>(), done_buf.data_ptr<float>(), tob, ep_stats.data_ptr<float>(),
                            (uint64_t)seed, (uint64_t)step0, reset_all ? 1 : 0, (int)max_steps, num_cus(),
                            cur_stream()),
           "rollout_cont");
}

// A tensor of evaluate(): checked like check(), with exactly n elements.
void check_exact(const Tensor& t, const char* name, at::ScalarType dt, int64_t n) {
  check(t, name, dt);
  TORCH_CHECK(t.numel() == n, name, " has ", t.numel(), " elements, expected ", n);
}

struct EvalShape {
  int64_t E, N, Tc;
};

// The outputs evaluate() and evaluate_cont() have in common: ep_* are [E, N]; the trace tensors come
// together or not at all, [Tc, N, ...] with act_dt / A_cols for tr_act (A_cols 0: [Tc, N]).
EvalShape check_eval_bufs(int64_t D, const Tensor& ep_ret, const Tensor& ep_len, const Tensor& ep_code,
                          const OptT& tr_obs, const OptT& tr_act, const OptT& tr_rew, const OptT& tr_done,
                          at::ScalarType act_dt, int64_t A_cols, int64_t max_steps) {
  check(ep_ret, "ep_ret", at::kFloat);
  TORCH_CHECK(ep_ret.dim() == 2 && ep_ret.size(0) >= 1 && ep_ret.size(1) >= 1, "ep_ret must be [E, N], E, N >= 1");
  EvalShape sh{ep_ret.size(0), ep_ret.size(1), 0};
  TORCH_CHECK(sh.N < (int64_t(1) << 31) - 16, "too many envs");
  check_exact(ep_len, "ep_len", at::kInt, sh.E * sh.N);
  check_exact(ep_code, "ep_code", at::kInt, sh.E * sh.N);
  TORCH_CHECK(max_steps >= 1, "max_steps must be >= 1");
  TORCH_CHECK(sh.E * max_steps < (int64_t(1) << 31), "E * max_steps must stay below 2^31");
  auto has = [](const OptT& t) { return t.has_value() && t->defined(); };
  const int given = has(tr_obs) + has(tr_act) + has(tr_rew) + has(tr_done);
  TORCH_CHECK(given == 0 || given == 4, "the trace tensors tr_obs, tr_act, tr_rew, tr_done are given together");
  if (given == 4) {
    check(*tr_rew, "tr_rew", at::kFloat);
    TORCH_CHECK(tr_rew->dim() == 2 && tr_rew->size(0) >= 1 && tr_rew->size(1) == sh.N, "tr_rew must be [Tc, N]");
    sh.Tc = tr_rew->size(0);
    check_exact(*tr_done, "tr_done", at::kFloat, sh.Tc * sh.N);
    check_exact(*tr_obs, "tr_obs", at::kFloat, sh.Tc * sh.N * D);
    check_exact(*tr_act, "tr_act", act_dt, sh.Tc * sh.N * (A_cols > 0 ? A_cols : 1));
  }
  return sh;
}

// Fused policy evaluation (evaluate.hip): every env runs E complete episodes under fixed weights.
void evaluate_qr(int64_t env, const Tensor& params, int64_t H, const Tensor& ep_ret, const Tensor& ep_len,
              const Tensor& ep_code, const OptT& tr_obs, const OptT& tr_act, const OptT& tr_rew, const OptT& tr_done,
              int64_t seed, int64_t step0, bool greedy, int64_t max_steps, bool dueling, int64_t quantiles) {
  auto [D, A, NS, ms] = env_dims(env);
  (void)NS;
  (void)ms;
  TORCH_CHECK(env != ENV_HALFCHEETAH, "evaluate takes the discrete device envs; use evaluate_cont for env 4");
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(!dueling || greedy, "a dueling Q-network is evaluated greedily: softmax-of-Q is not its policy");
  TORCH_CHECK(!dueling || A <= 15, "a dueling net has A + 1 outputs: act dim must be in [1, 15], got ", A);
  TORCH_CHECK(quantiles >= 0, "quantiles must be >= 0, got ", quantiles);
  TORCH_CHECK(quantiles == 0 || greedy, "a quantile Q-network is evaluated greedily: softmax-of-Q is not its policy");
  TORCH_CHECK(quantiles == 0 || !dueling, "quantiles with dueling is not built: set one of the two");
  TORCH_CHECK(A * quantiles <= 16, "a quantile net has A * quantiles <= 16 outputs, got ", A, " * ", quantiles);
  check_exact(params, "params", at::kFloat,
              flat_size(D, H, quantiles > 0 ? A * quantiles : A + (dueling ? 1 : 0), false));
  const EvalShape sh = check_eval_bufs(D, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done, at::kInt, 0,
                                       max_steps);
  const bool tr = sh.Tc > 0;
  check_rc(rrl_evaluate((int)env, params.data_ptr<float>(), (int)sh.N, (int)sh.E, (int)sh.Tc, (int)H,
                        ep_ret.data_ptr<float>(), ep_len.data_ptr<int>(), ep_code.data_ptr<int>(),
                        tr ? tr_obs->data_ptr<float>() : nullptr, tr ? tr_act->data_ptr<int>() : nullptr,
                        tr ? tr_rew->data_ptr<float>() : nullptr, tr ? tr_done->data_ptr<float>() : nullptr,
                        (uint64_t)seed, (uint64_t)step0, greedy ? 1 : 0, (int)max_steps, dueling ? 1 : 0,
                        (int)quantiles, num_cus(), cur_stream()),
           "evaluate");
}

// The scalar nets (plain or dueling): the binding as it always parsed.
void evaluate(int64_t env, const Tensor& params, int64_t H, const Tensor& ep_ret, const Tensor& ep_len,
              const Tensor& ep_code, const OptT& tr_obs, const OptT& tr_act, const OptT& tr_rew, const OptT& tr_done,
              int64_t seed, int64_t step0, bool greedy, int64_t max_steps, bool dueling) {
  evaluate_qr(env, params, H, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done, seed, step0, greedy, max_steps,
              dueling, 0);
}

void evaluate_cont(int64_t env, const Tensor& params, const Tensor& env_consts, int64_t H, const Tensor& ep_ret,
                   const Tensor& ep_len, const Tensor& ep_code, const OptT& tr_obs, const OptT& tr_act,
                   const OptT& tr_rew, const OptT& tr_done, int64_t seed, int64_t step0, bool greedy,
                   int64_t max_steps) {
  auto [D, A, NS, ms] = env_dims(env);
  (void)NS;
  (void)ms;
  TORCH_CHECK(env == ENV_HALFCHEETAH, "evaluate_cont supports the continuous device env 4 (HalfCheetahSynth)");
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  check_exact(params, "params", at::kFloat, flat_size(D, H, A, true));
  check_exact(env_consts, "env_consts", at::kFloat, 17 * 17 + 17 * 6);
  const EvalShape sh = check_eval_bufs(D, ep_ret, ep_len, ep_code, tr_obs, tr_act, tr_rew, tr_done, at::kFloat, A,
                                       max_steps);
  const bool tr = sh.Tc > 0;
  check_rc(rrl_evaluate_cont((int)env, params.data_ptr<float>(), env_consts.data_ptr<float>(), (int)sh.N, (int)sh.E,
                             (int)sh.Tc, (int)H, ep_ret.data_ptr<float>(), ep_len.data_ptr<int>(),
                             ep_code.data_ptr<int>(), tr ? tr_obs->data_ptr<float>() : nullptr,
                             tr ? tr_act->data_ptr<float>() : nullptr, tr ? tr_rew->data_ptr<float>() : nullptr,
                             tr ? tr_done->data_ptr<float>() : nullptr, (uint64_t)seed, (uint64_t)step0,
                             greedy ? 1 : 0, (int)max_steps, num_cus(), cur_stream()),
           "evaluate_cont");
}

}  // namespace

void register_cnn_ops(pybind11::module_& m);      // cnn_ops.cpp
void register_rollout_ops(pybind11::module_& m);  // rollout_ops.cpp (host-env rollout driver)
void register_dqn_ops(pybind11::module_& m);      // dqn_ops.cpp

namespace rrl_bind {
int grid_cus() { return num_cus(); }
}  // namespace rrl_bind

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "relayrl_prototype_amd gfx950 HIP kernels";
  m.def("num_cus", &num_cus);
  m.def("device_cus", &device_cus);
  m.def("relax_thread_capture_mode", []() {
    // hipThreadExchangeStreamCaptureMode(relaxed) for the calling thread, for good: a helper
    // thread's event waits then leave other threads' graph captures alone
    hipStreamCaptureMode m = hipStreamCaptureModeRelaxed;
    return (int)hipThreadExchangeStreamCaptureMode(&m);
  });
  m.def("set_cu_limit", &set_cu_limit, "size grids for n CUs (0 = all); returns the previous limit");
  m.def("cu_masked_stream", &cu_masked_stream);
  m.def("destroy_stream", &destroy_stream);
  m.def("mlp_forward", &mlp_forward);
  m.def("mlp_grad_slabs", &mlp_grad_slabs);
  m.def("mlp_grad", &mlp_grad);
  m.def("mlp_grad_qr", &mlp_grad_qr, pybind11::arg("params"), pybind11::arg("X"), pybind11::arg("A"),
        pybind11::arg("quantiles"), pybind11::arg("H"), pybind11::arg("act"), pybind11::arg("ret"),
        pybind11::arg("inv_B"), pybind11::arg("kappa"), pybind11::arg("grad_slab"), pybind11::arg("loss_slab"),
        pybind11::arg("nvalid") = pybind11::none(), pybind11::arg("inv_B_dev") = pybind11::none(),
        pybind11::arg("row_w") = pybind11::none(), pybind11::arg("w_norm") = pybind11::none(),
        pybind11::arg("td_abs") = pybind11::none());
  m.def("set_value_grad_stamps", [](const Tensor& t) { rrl_set_value_grad_stamps(t.numel() ? t.data_ptr() : nullptr); });
  m.def("set_value_grad_tune", [](int64_t t) { return (int64_t)rrl_set_value_grad_tune((int)t); });
  m.def("set_value_grad_mode", [](int64_t mode) { return (int64_t)rrl_set_value_grad_mode((int)mode); },
        "value-MSE gradient kernel: 1 = bf16x6 weight-stationary (H 128, D <= 8), 0 = fp32 MFMA; returns the "
        "previous mode (-1 queries without changing)");
  m.def("set_value_fwd_mode", [](int64_t mode) { return (int64_t)rrl_set_value_fwd_mode((int)mode); },
        "value forward: 1 = bf16x6 weight-stationary split kernel (H 128, D <= 24), 0 = fp32 MFMA; returns "
        "the previous mode (-1 queries)");
  m.def("scan_tm_parts", &scan_tm_parts);
  m.def("gae_scan_tm", &gae_scan_tm, pybind11::arg("rew"), pybind11::arg("done"), pybind11::arg("val"),
        pybind11::arg("tval"), pybind11::arg("adv"), pybind11::arg("ret"), pybind11::arg("stats_part"),
        pybind11::arg("stats_out"), pybind11::arg("gamma"), pybind11::arg("lam"),
        pybind11::arg("counters") = std::vector<std::tuple<Tensor, int64_t>>{});
  m.def("vtrace_scan_tm", &vtrace_scan_tm, pybind11::arg("rew"), pybind11::arg("done"), pybind11::arg("val"),
        pybind11::arg("tval"), pybind11::arg("logp_mu"), pybind11::arg("logp_pi"), pybind11::arg("adv"),
        pybind11::arg("ret"), pybind11::arg("stats_part"), pybind11::arg("stats_out"), pybind11::arg("is_out"),
        pybind11::arg("gamma"), pybind11::arg("lam"), pybind11::arg("rho_bar"), pybind11::arg("c_bar"),
        pybind11::arg("pg_rho_bar"));
  m.def("scan_flat_blocks", &scan_flat_blocks);
  m.def("scan_flat", &scan_flat);
  m.def("stats_reduce", &stats_reduce);
  m.def("column_sums", &column_sums, "double column sums of the first cols columns of a [rows, ld] fp32 tensor");
  // step_add / step_inc: t = step + step_add + 1, the counter advances by step_inc (adam.hip)
  m.def("adam", &adam, pybind11::arg("param"), pybind11::arg("m"), pybind11::arg("v"), pybind11::arg("grad"),
        pybind11::arg("slab"), pybind11::arg("grad_out"), pybind11::arg("step"), pybind11::arg("ticket"),
        pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("grad_scale"), pybind11::arg("weight_decay"), pybind11::arg("step_add") = 0,
        pybind11::arg("step_inc") = 1);
  m.def("reduce_slabs", &reduce_slabs);
  m.def("payload_checksum", &payload_checksum, "int64[2] (s1, s2) over the words of up to 8 contiguous segments");
  m.def("payload_verify", &payload_verify);
  m.def("env_dims", &env_dims);
  m.def("rollout_grid", &rollout_grid);
  m.def("rollout", &rollout);
  m.def("rollout_cont", &rollout_cont);
  m.def("evaluate", &evaluate, pybind11::arg("env"), pybind11::arg("params"), pybind11::arg("H"),
        pybind11::arg("ep_ret"), pybind11::arg("ep_len"), pybind11::arg("ep_code"), pybind11::arg("tr_obs"),
        pybind11::arg("tr_act"), pybind11::arg("tr_rew"), pybind11::arg("tr_done"), pybind11::arg("seed"),
        pybind11::arg("step0"), pybind11::arg("greedy"), pybind11::arg("max_steps"),
        pybind11::arg("dueling") = false);
  m.def("evaluate_qr", &evaluate_qr, pybind11::arg("env"), pybind11::arg("params"), pybind11::arg("H"),
        pybind11::arg("ep_ret"), pybind11::arg("ep_len"), pybind11::arg("ep_code"), pybind11::arg("tr_obs"),
        pybind11::arg("tr_act"), pybind11::arg("tr_rew"), pybind11::arg("tr_done"), pybind11::arg("seed"),
        pybind11::arg("step0"), pybind11::arg("greedy"), pybind11::arg("max_steps"),
        pybind11::arg("dueling") = false, pybind11::arg("quantiles") = 0);
  m.def("evaluate_cont", &evaluate_cont, pybind11::arg("env"), pybind11::arg("params"), pybind11::arg("env_consts"),
        pybind11::arg("H"), pybind11::arg("ep_ret"), pybind11::arg("ep_len"), pybind11::arg("ep_code"),
        pybind11::arg("tr_obs"), pybind11::arg("tr_act"), pybind11::arg("tr_rew"), pybind11::arg("tr_done"),
        pybind11::arg("seed"), pybind11::arg("step0"), pybind11::arg("greedy"), pybind11::arg("max_steps"));
  // the enumerators of api.h by name: the Python tables (ops/mlp.py, DEVICE_ENVS) are tested against these
#define RRL_ENUM(e) pybind11::arg(#e) = (int)rrl::e
  m.attr("FWD_MODES") = pybind11::dict(RRL_ENUM(MODE_VALUE), RRL_ENUM(MODE_CAT_SAMPLE), RRL_ENUM(MODE_CAT_EVAL),
                                       RRL_ENUM(MODE_LOGITS), RRL_ENUM(MODE_GAUSS_SAMPLE), RRL_ENUM(MODE_GAUSS_EVAL));
  m.attr("GRAD_HEADS") = pybind11::dict(RRL_ENUM(HEAD_PG_CAT), RRL_ENUM(HEAD_VALUE_MSE), RRL_ENUM(HEAD_PPO_CAT),
                                        RRL_ENUM(HEAD_PPO_GAUSS), RRL_ENUM(HEAD_PG_GAUSS), RRL_ENUM(HEAD_Q_TD),
                                        RRL_ENUM(HEAD_Q_DUEL), RRL_ENUM(HEAD_Q_QR));
  m.attr("ENV_IDS") = pybind11::dict(RRL_ENUM(ENV_CARTPOLE), RRL_ENUM(ENV_MOUNTAINCAR), RRL_ENUM(ENV_ACROBOT),
                                     RRL_ENUM(ENV_LUNARLANDER), RRL_ENUM(ENV_HALFCHEETAH));
#undef RRL_ENUM
  register_cnn_ops(m);
  register_rollout_ops(m);
  register_dqn_ops(m);
}
