// The C ABI of the gfx950 kernels: every extern "C" entry point of csrc/kernels/*.hip and the
// integer vocabularies that cross it.  This is the only place a rrl_* prototype is written: the
// .hip file that defines an entry point includes it (a definition that disagrees is a compile
// error) and so does every caller (csrc/bindings, csrc/runtime).  Plain C++: no HIP or torch
// include; a stream is a hipStream_t passed as void*.  Unless a comment says otherwise an entry
// point returns 0, a hipError_t (> 0) or a negative code for arguments it does not support.
#pragma once
#include <cstdint>

namespace rrl {

enum FwdMode : int {
  MODE_VALUE = 0,
  MODE_CAT_SAMPLE = 1,
  MODE_CAT_EVAL = 2,
  MODE_LOGITS = 3,
  MODE_GAUSS_SAMPLE = 4,
  MODE_GAUSS_EVAL = 5,
};

enum GradHead : int {
  HEAD_PG_CAT = 0,     // REINFORCE: loss = -mean(logp(a) * adv)
  HEAD_VALUE_MSE = 1,  // baseline: loss = mean((v - ret)^2)
  HEAD_PPO_CAT = 2,    // PPO clipped surrogate, categorical
  HEAD_PPO_GAUSS = 3,  // PPO clipped surrogate, diagonal Gaussian
  HEAD_PG_GAUSS = 4,   // REINFORCE / A2C with a Gaussian policy
  HEAD_Q_TD = 5,       // DQN: loss = mean(huber(Q(x)[act] - ret, delta)); delta travels in clip_eps
  HEAD_Q_DUEL = 6,     // HEAD_Q_TD on a dueling net of A + 1 outputs: Q = out[A] + out[act] - mean(out[0 .. A-1])
  HEAD_Q_QR = 7,       // QR-DQN: quantile-Huber loss on a net of A * NQ outputs (rrl_mlp_grad_qr has the contract)
};

enum EnvId : int { ENV_CARTPOLE = 0, ENV_MOUNTAINCAR = 1, ENV_ACROBOT = 2, ENV_LUNARLANDER = 3, ENV_HALFCHEETAH = 4 };

// The arguments of rrl_dqn_targets, which has the contract.
struct DqnTargetsCall {
  const float *online, *target;  // nets: MLPSpec(D, H, A + dueling); online is read with double_q only
  const float *obs, *nobs;       // ring: rows [slot][env] of D floats, the first `filled` of them are sampled
  const int* act;
  const float *rew, *done;       // done: 0 running, 1 terminal, 2 time-limit truncation
  long long filled;
  int B, D, A, H;                // shape: batch rows, obs dim, actions, hidden size
  float gamma;                   // target
  int double_q, dueling;
  uint64_t sample_key, update;   // sampling
  float *Xb, *y;                 // outputs: Xb [B][D], y [B]
  int *act_b, *idx;              // [B] each; idx may be null without a tree
  const float* tree;             // prioritised part, used iff tree != nullptr: [2 * P2] over the ring's L rows
  long long L;
  float beta;
  float *w, *wmax;               // [B], [1]
  int n_step, N, newest;         // walk: N envs per slot, newest the slot written last
  int* last;                     // [B], may be null; n_step, N, newest, last = 1, 1, 0, nullptr is "no walk"
  int quantiles;                 // 0: the scalar forms above; NQ >= 1: nets MLPSpec(D, H, A * NQ) and y [B][NQ]
};

}  // namespace rrl

extern "C" {

// ---- mlp_forward.hip
// mode: a FwdMode
int rrl_mlp_forward(int mode, const float* params, const float* X, int B, int D, int A, int H, const float* mask,
                    const int* act_in, const float* actc_in, int* act_out, float* actc_out, float* out0,
                    float* out1, float* logits_out, uint64_t seed, uint64_t step, uint32_t row_offset,
                    const float* gate, float* x_copy, int* act_host, float* actc_host, int num_cu, void* stream);
// 1 = bf16x6 weight-stationary split kernel, 0 = fp32 MFMA; returns the previous mode (-1 queries)
int rrl_set_value_fwd_mode(int mode);

// ---- mlp_grad.hip
// head: a GradHead.  HEAD_Q_TD reads act and ret (the TD target) and takes its Huber threshold delta
// from clip_eps, which it has no other use for; mask, adv, logp_old and ent_coef are ignored.
// HEAD_Q_DUEL is HEAD_Q_TD on the dueling net: A stays the number of actions, params / P / the slabs are
// those of A + 1 outputs (rows 0 .. A-1 the advantages, row A the state value), and in fp32
//   s = out[0]; s += out[k] (k = 1 .. A-1, ascending);  m = s / A;  Q(a) = (out[A] - m) + out[a].
// -2: A outside [1, 16] or D outside [1, 32]; -3: H not 64 / 128, or HEAD_Q_DUEL with A > 15; -4: the net
// and the staging do not fit the LDS; -1: HEAD_Q_QR, which has its own entry point below
int rrl_mlp_grad(int head, const float* params, const float* X, int B, int D, int A, int H, const float* mask,
                 const int* act, const float* actc, const float* adv, const float* ret, const float* logp_old,
                 const float* adv_stats, float inv_B, float clip_eps, float ent_coef, float* grad_slab,
                 float* loss_slab, int P, const int* nvalid, const float* inv_B_dev, int num_cu, void* stream);
// rrl_mlp_grad plus the per-row weights of prioritised replay, read by HEAD_Q_TD and HEAD_Q_DUEL alone: with w_i =
// row_w[i] / *w_norm the row's loss is w_i * huber and its gradient is scaled by w_i; td_abs[i] (may be
// null) receives |Q(x_i)[act_i] - ret_i| of every valid row.  row_w and w_norm come together or not at
// all (-1); all three null is rrl_mlp_grad
int rrl_mlp_grad_weighted(int head, const float* params, const float* X, int B, int D, int A, int H,
                          const float* mask, const int* act, const float* actc, const float* adv, const float* ret,
                          const float* logp_old, const float* adv_stats, float inv_B, float clip_eps, float ent_coef,
                          float* grad_slab, float* loss_slab, int P, const int* nvalid, const float* inv_B_dev,
                          const float* row_w, const float* w_norm, float* td_abs, int num_cu, void* stream);
// HEAD_Q_QR, the quantile-regression head of QR-DQN (Dabney et al. 2018).  params / P / the slabs are those of
// MLPSpec(D, H, A * NQ); output a * NQ + i is quantile i of action a at level tau_i = (2 i + 1) / (2 NQ).  For a
// row with action act: theta_i = out[act * NQ + i], T_j = qtarget[row][j] ([B][NQ]), u_ij = T_j - theta_i and
//   rho = (1 / NQ) sum_i sum_j |tau_i - [u_ij < 0]| * huber_kappa(u_ij) / kappa,
//   dout[act * NQ + i] = inv_B * w * -(1 / NQ) sum_j |tau_i - [u_ij < 0]| * clamp(u_ij, -kappa, kappa) / kappa,
// every other output 0, w = row_w[row] / *w_norm or 1.  Loss slab: [0] += w * rho, [4] += s_act / NQ (s_act the
// ascending fp32 sum of the action's quantiles), [5] += 1.  td_abs[row] (may be null) = rho, the unweighted row
// loss.  act[row] is clamped into [0, A) (it indexes the output registers): an out-of-range action of a valid row
// trains action 0 or A - 1, where HEAD_Q_TD would give the row no gradient.  nvalid / inv_B_dev as rrl_mlp_grad.
// Nothing is written on a refusal: -1 a null pointer, or row_w without w_norm; -2 B < 1, A < 1, NQ < 1,
// A * NQ > 16, D outside [1, 32], kappa <= 0, or P not the net's; -3 H not 64 / 128; -4 the net and the staging do
// not fit the LDS
int rrl_mlp_grad_qr(const float* params, const float* X, int B, int D, int A, int NQ, int H, const int* act,
                    const float* qtarget, float inv_B, float kappa, float* grad_slab, float* loss_slab, int P,
                    const int* nvalid, const float* inv_B_dev, const float* row_w, const float* w_norm,
                    float* td_abs, int num_cu, void* stream);
// number of partial-gradient slabs (== grid size) rrl_mlp_grad uses
int rrl_mlp_grad_slabs(int B, int num_cu);
// 1 = bf16x6 weight-stationary kernels, 0 = fp32 MFMA; returns the previous mode (-1 queries)
int rrl_set_value_grad_mode(int mode);

// ---- value_grad.hip
void rrl_set_value_grad_stamps(void* buf);
int rrl_set_value_grad_tune(int t);  // returns the previous variant

// ---- scan.hip
int rrl_scan_tm_parts(int N);
// stats_part: rrl_scan_tm_parts(K * N) x 3 floats; cnt / inc: ncnt <= 3 device counters advanced by the launch
int rrl_gae_scan_tm(const float* rew, const float* done, const float* val, const float* tval, float* adv,
                    float* ret, float* stats_part, float* stats_out, int K, int T, int N, float gamma, float lam,
                    long long* const* cnt, const long long* inc, int ncnt, void* stream);
// V-trace on the same layout.  part: rrl_scan_tm_parts(K * N) x 5 floats ([n][3] advantage statistics, then
// [n][2] importance-weight sums); stats_out[3] / is_out[2] (sum min(rho_bar, ratio), sum |logp_pi - logp_mu|)
// may be null.  -1: null val / logp_*, a threshold <= 0 or an empty batch
int rrl_vtrace_scan_tm(const float* rew, const float* done, const float* val, const float* tval,
                       const float* logp_mu, const float* logp_pi, float* adv, float* ret, float* part,
                       float* stats_out, float* is_out, int K, int T, int N, float gamma, float lam, float rho_bar,
                       float c_bar, float pg_rho_bar, void* stream);
int rrl_scan_flat_blocks(int L);
// work: rrl_scan_flat_blocks(L) x 9 floats
int rrl_scan_flat(const float* rew, const float* done, const float* val, const float* boot, float* adv, float* ret,
                  float* work, float* stats_out, int L, float gamma, float lam, void* stream);
int rrl_stats_reduce(const float* part, int nparts, float* out, void* stream);
int rrl_column_sums(const float* part, int rows, int ld, int cols, double* out, void* stream);

// ---- adam.hip
// t = *step + step_add + 1; the counter advances by step_inc
int rrl_adam(float* param, float* m, float* v, const float* grad, const float* slab, int nslab, float* grad_out,
             int* step, unsigned* ticket, int P, float lr, float beta1, float beta2, float eps, float grad_scale,
             float weight_decay, int step_add, int step_inc, void* stream);
int rrl_reduce_slabs(const float* slab, int nslab, int P, float scale, float* out, void* stream);

// ---- checksum.hip
int rrl_payload_checksum_blocks(const unsigned long long* words, int nseg, int num_cu);
// part: rrl_payload_checksum_blocks() x 2 words of device workspace; out: two 64-bit words on the device
int rrl_payload_checksum(const void* const* ptrs, const unsigned long long* words, int nseg,
                         unsigned long long* part, unsigned long long* out, int num_cu, void* stream);
// status[k] bits: 1 checksum mismatch, 2 seq != expected, 4 version outside [lo, hi]
int rrl_payload_verify(const unsigned long long* sums, const double* hdr, int ld, int ck_col, int K,
                       double expected_seq, double lo, double hi, int* status, void* stream);

// ---- rollout.hip
// env: an EnvId; nonzero for an unknown one
int rrl_env_dims(int env, int* D, int* A, int* NS, int* max_steps);
int rrl_rollout_grid(int N, int num_cu);
int rrl_rollout(int env, const float* params, int N, int T, int H, float* state, int* ep_len, float* ep_ret,
                float* obs_buf, int* act_buf, float* logp_buf, float* rew_buf, float* done_buf, float* tobs_buf,
                float* ep_stats, uint64_t seed, uint64_t step0, int reset_all, int max_steps, int num_cu,
                void* stream);
// continuous-action envs (ENV_HALFCHEETAH)
int rrl_rollout_cont(int env, const float* params, const float* env_consts, int N, int T, int H, float* state,
                     int* ep_len, float* ep_ret, float* obs_buf, float* act_buf, float* logp_buf, float* rew_buf,
                     float* done_buf, float* tobs_buf, float* ep_stats, uint64_t seed, uint64_t step0,
                     int reset_all, int max_steps, int num_cu, void* stream);

// ---- evaluate.hip
// Every env runs E complete episodes (greedy: argmax / mu instead of the rollout kernels' draws) into
// ep_ret / ep_len / ep_code [E][N] (code 1 terminal, 2 time limit).  tr_*: optional trace of the first Tc
// steps, all four pointers or none (then Tc may be 0).  -2: N, E, Tc or max_steps below 1, or
// E * max_steps >= 2^31; -3: unsupported H or env.  dueling != 0 (rrl_evaluate only): params is a dueling
// Q-network of A + 1 outputs (HEAD_Q_DUEL) and the greedy action is the lowest-index argmax of its A
// advantage outputs; -3 with greedy == 0, which is not a policy of that net.  quantiles = NQ >= 1 (rrl_evaluate
// only): params is a quantile Q-network of A * NQ outputs (HEAD_Q_QR) and the greedy action is the lowest-index
// argmax of the per-action sums s_a = out[a * NQ]; s_a += out[a * NQ + i] (i ascending); -3 with greedy == 0,
// with quantiles < 0, with dueling != 0 as well, or with A * NQ > 16
int rrl_evaluate(int env, const float* params, int N, int E, int Tc, int H, float* ep_ret, int* ep_len,
                 int* ep_code, float* tr_obs, int* tr_act, float* tr_rew, float* tr_done, uint64_t seed,
                 uint64_t step0, int greedy, int max_steps, int dueling, int quantiles, int num_cu, void* stream);
// continuous-action envs (ENV_HALFCHEETAH); tr_act is [Tc][N][A]
int rrl_evaluate_cont(int env, const float* params, const float* env_consts, int N, int E, int Tc, int H,
                      float* ep_ret, int* ep_len, int* ep_code, float* tr_obs, float* tr_act, float* tr_rew,
                      float* tr_done, uint64_t seed, uint64_t step0, int greedy, int max_steps, int num_cu,
                      void* stream);

// ---- dqn.hip
// Epsilon-greedy actor: T steps of N envs into slots slot0 .. slot0 + T - 1 of a replay ring of C slots
// (obs / nobs [C][N][D], act / rew / done [C][N]; nobs = the post-step, pre-reset observation; done 0
// running, 1 terminal, 2 time limit).  state / ep_len / ep_ret / reset_all / max_steps / ep_stats as
// rrl_rollout, with ep_stats [rrl_dqn_rollout_grid()][8].  -1: a null pointer; -2: N, T, C or max_steps
// below 1; -3: unsupported H or env; -4 (nothing written): a launch that would wrap, i.e. unless
// C % T == 0, slot0 % T == 0 and slot0 + T <= C.  dueling != 0: params is a dueling Q-network of A + 1
// outputs (HEAD_Q_DUEL) and the greedy action is the lowest-index argmax of its A advantage outputs.
// quantiles = NQ >= 1: params is a quantile Q-network of A * NQ outputs (HEAD_Q_QR) and the greedy action is the
// lowest-index argmax of the per-action quantile sums; the draws, the ring and the statistics do not depend on
// it.  -3 (nothing written) with quantiles < 0, with dueling != 0 as well, or with A * NQ > 16
int rrl_dqn_rollout_grid(int N, int num_cu);
int rrl_dqn_rollout(int env, const float* params, int N, int T, int H, int C, int slot0, float* state, int* ep_len,
                    float* ep_ret, float* obs, float* nobs, int* act, float* rew, float* done, float* ep_stats,
                    uint64_t seed, uint64_t step0, float epsilon, int reset_all, int max_steps, int dueling,
                    int quantiles, int num_cu, void* stream);
// The TD targets of one update.  Batch row b samples ring row r0, gathers obs[r0] -> Xb[b], act[r0] -> act_b[b],
// r0 -> idx[b], walks to the row `last` (last[b] <- last) and writes, a* being the lowest-index argmax of
// Q_target(nobs[last], .) (double_q = 0) or of Q_online (double_q = 1),
//   y[b] = G + disc * (done[last] == 1 ? 0 : 1) * Q_target(nobs[last], a*).
// Sampling: r0 = (philox((b, update, 0), sample_key).x * filled) >> 32; with a tree (per.hip, leaf of row r at
// tree[P2 + r]) b descends it with m = (b + u01(philox((b, update, 1), sample_key).x)) * (tree[1] / B), exactly
// log2(P2) steps `if (m >= left && right > 0) { m -= left; go right } else go left`, r0 is clamped to [0, filled - 1],
// w[b] = (filled * leaf / tree[1])^-beta and *wmax = max_b w[b] (reset on the stream before the launch, a
// bit-pattern maximum: the same bits every launch).  The walk, in fp32 and in this order:
//   last = r0; G = rew[r0]; disc = gamma; m = 1
//   while (m < n_step && done[last] == 0 && last / N != newest) {
//     last += N; if (last >= filled) last -= filled;  G = fma(disc, rew[last], G);  disc *= gamma;  ++m; }
// n_step == 1 launches the one-step kernel, which has no walk, and then copies idx to last.  dueling != 0: the
// nets have A + 1 outputs (HEAD_Q_DUEL has the combine), a* is the argmax of the selecting net's A advantages and
// Q_target the target net's dueling Q; only y depends on it.  quantiles = NQ >= 1: the nets have A * NQ outputs
// (HEAD_Q_QR), a* is the argmax of the selecting net's per-action quantile sums, y is [B][NQ] and
//   y[b][j] = G + disc * (done[last] == 1 ? 0 : 1) * theta_target(nobs[last])[a* * NQ + j]
// (at n_step == 1: rew[r0] + gamma * ...); again only y depends on it.  -3 also for quantiles < 0, quantiles with
// dueling, or A * NQ > 16.  Refusals write nothing and are checked in this order.
// -1: a null pointer (online with double_q; idx, w, wmax with a tree; idx with last at n_step == 1); -2: B < 1,
// filled outside [1, 2^31) or, with a tree, outside [1, L], L outside [1, 2^30]; -3: H not 64 / 128, D outside
// [1, 16], A < 1 or A + dueling > 16; -2: n_step < 1, N < 1 or filled % N != 0; -4: newest outside [0, filled / N)
int rrl_dqn_targets(const rrl::DqnTargetsCall* c, int num_cu, void* stream);

// ---- per.hip
// The priority sum tree of prioritised replay over a ring of L = C * N rows: fp32 tree[2 * P2], P2 =
// rrl_per_tree_leaves(L) the smallest power of two >= L, root tree[1], leaf of row r tree[P2 + r], and
// after every launch tree[i] == tree[2i] + tree[2i + 1] (one fp32 add) for every internal node.  Each
// launch is ONE workgroup that walks the levels bottom-up.  0 for L outside [1, 2^30]
long long rrl_per_tree_leaves(long long L);
// leaves of rows [slot0 * N, (slot0 + T) * N) <- *pmax, ancestors refreshed.  The codes of
// rrl_dqn_rollout: -1 a null pointer; -2 N, T or C below 1 or C * N > 2^30; -4 (nothing written) unless
// C % T == 0, slot0 % T == 0 and slot0 + T <= C
int rrl_per_insert(float* tree, const float* pmax, int C, int N, int T, int slot0, void* stream);
// leaf of every row r in idx[0 .. B) <- max over {b : idx[b] == r} of (td_abs[b] + prio_eps)^alpha (a
// non-finite td_abs[b], or a power that is not finite, counts as the *pmax of before the launch), *pmax <-
// max(*pmax, every new leaf), ancestors refreshed.  An idx outside [0, L) is skipped.  -1: a null
// pointer; -2: B < 1, L outside [1, 2^30], alpha < 0 or prio_eps <= 0
int rrl_per_update(float* tree, float* pmax, const int* idx, const float* td_abs, int B, long long L, float alpha,
                   float prio_eps, void* stream);

// ---- noisy.hip
// NoisyNet layers (factorised Gaussian noise) for a Q-network MLPSpec(D, H, A_out) of P parameters.  Unit i
// of (role r in [0, 3], layer l = 1..3, side s = 0 in / 1 out) at the 64-bit draw d:
//   w = philox((i, lo32(d), hi32(d), 16 + 8 r + 2 (l - 1) + s), key)
//   n = sqrtf(-2 logf(1 - u01(w.x))) * cosf(6.283185307179586f * u01(w.y));  f = copysignf(sqrtf(fabsf(n)), n)
// (the precise functions), eps_W[j][i] = f_out[j] * f_in[i], eps_b[j] = f_out[j], every product and sum one
// rounded fp32 operation, never an fma.  The U = D + 4 H + A_out unit factors of one (role, draw) are laid out
// [in1 (D), out1 (H), in2 (H), out2 (H), in3 (H), out3 (A_out)].
//
// Job k < njobs (theta / roles / draws: HOST arrays of njobs entries) reads theta[k] = [mu (P); sigma (P)] and
// writes out[k][p] = mu[p] + sigma[p] * eps(roles[k], draws[k])[p]; all jobs are one launch.  units_out (may be
// null) [njobs][U] receives the unit factors f.  Both entry points, nothing written on a refusal: -1 a null
// pointer; -2 D or A_out outside [1, 16], njobs outside [1, 3], nslab < 1, a role outside [0, 3] or P not the
// net's; -3 H not 64 / 128.  No output depends on the grid
int rrl_noisy_compose(const float* const* theta, int njobs, const int* roles, const uint64_t* draws, int D, int H,
                      int A_out, uint64_t key, float* out, float* units_out, int num_cu, void* stream);
// slab [nslab][P]: g = slab[0][p], then g = g + slab[s][p] for s = 1 .. nslab - 1 in this order;
// grad_out[p] = g, grad_out[P + p] = g * eps(role, draw)[p]: the gradient of [mu; sigma] from the gradient
// slabs of the effective parameters
int rrl_noisy_grad(const float* slab, int nslab, int P, int role, uint64_t draw, int D, int H, int A_out,
                   uint64_t key, float* grad_out, int num_cu, void* stream);

// ---- cnn.hip (bf16 tensors as uint16_t)
int rrl_conv_fwd(const void* x, int x_u8, const uint16_t* w, const float* b, uint16_t* y, int N, int H, int W,
                 int C, int KH, int KW, int S, int Cout, int relu, float* work, long long work_elems, void* stream);
int rrl_gemm_dgrad(const uint16_t* dy, const uint16_t* w, const uint16_t* mask, uint16_t* out, int M, int Cout,
                   int K, void* stream);
// -1 (nothing launched) for a geometry without an implicit-dgrad kernel
int rrl_conv_dgrad(const uint16_t* dy, const uint16_t* w, const uint16_t* xact, uint16_t* dx, int N, int H, int W,
                   int C, int KH, int KW, int S, int Cout, void* stream);
int rrl_col2im_mask(const uint16_t* dcol, const uint16_t* xact, uint16_t* dx, int N, int H, int W, int C, int KH,
                    int KW, int S, void* stream);
int rrl_conv_wgrad(const uint16_t* dy, const void* x, int x_u8, float* part, float* bias_part, int splits, int N,
                   int H, int W, int C, int KH, int KW, int S, int Cout, void* stream);
// number of splits actually used for a reduction of length R
int rrl_gemm_splits(int R, int splits);
int rrl_sum_splits_multi(const float* const* parts, const int* splits, const long long* ns, float* const* outs,
                         int count, void* stream);
int rrl_sum_splits(const float* part, int splits, long long n, float* out, void* stream);
int rrl_colsum(const uint16_t* y, int M, int C, float* part, int splits, void* stream);
int rrl_sumsq(const float* x, long long n, float* work, int work_n, float* out, void* stream);
// returns the number of partials written (> 0), or minus a hipError_t
int rrl_sumsq_partial(const float* x, long long n, float* work, int work_n, void* stream);
int rrl_adam_clip(float* p, float* m, float* v, const float* g, uint16_t* shadow, long long n, const float* norm_sq,
                  float max_norm, float lr, float b1, float b2, float eps, int step, const long long* step_dev,
                  int norm_parts, void* stream);
int rrl_counter_add_n(long long* const* c, const long long* inc, int n, void* stream);
int rrl_counter_add(long long* c, long long inc, void* stream);
int rrl_to_bf16(const float* x, uint16_t* y, long long n, void* stream);
// mode 0: rollout (sample act / logp / value), 1: training (dh, dhead, stats)
int rrl_a2c_head(int mode, const uint16_t* h, const float* head_params, int B, int A, int32_t* act, float* logp,
                 float* value, float* logits_out, unsigned long long seed, unsigned long long step,
                 const unsigned long long* step_base, int row_offset, const int32_t* act_in, const float* adv,
                 const float* ret, float inv_B, float vf_coef, float ent_coef, uint16_t* dh, float* dhead,
                 float* stats, int grid, const float* part, int splits, const float* fc_b, uint16_t* h_out,
                 void* stream);
int rrl_head_wgrad(const uint16_t* h, const float* dhead, int B, int A, float* part, int nblk, void* stream);

// ---- fc.hip
// both *_part: return the number of splits used (> 0), negative on failure
int rrl_fc_nt_part(const uint16_t* a, const uint16_t* b, float* part, int M, int N, int K, int splits, void* stream);
int rrl_fc_nt_mask(const uint16_t* a, const uint16_t* b, const uint16_t* mask, uint16_t* out, int M, int N, int K,
                   void* stream);
int rrl_fc_tn_part(const uint16_t* x, const uint16_t* y, float* part, int R, int I, int J, int splits,
                   const uint16_t* ones, float* bias_part, void* stream);
int rrl_transpose_bf16(const uint16_t* in, uint16_t* out, int R, int C, void* stream);

// ---- cnn_fused.hip
int rrl_conv_stack_fwd(const uint8_t* x, const float* hist, const uint8_t* frames, const int32_t* fidx,
                       const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const uint16_t* w3,
                       const float* b3, uint16_t* y1, uint16_t* y2, uint16_t* y3, int N, int max_grid, void* stream);
int rrl_conv3_bwd(const uint16_t* dy, const uint16_t* w, const uint16_t* xact, uint16_t* dx, float* part,
                  float* bias_part, int N, int grid, int variant, void* stream);
int rrl_conv2_bwd(const uint16_t* dy, const uint16_t* w, const uint16_t* xact, uint16_t* dx, float* part,
                  float* bias_part, int N, int grid, int staged, void* stream);
int rrl_conv1_wgrad8(const uint8_t* x, const float* hist, const uint8_t* frames, const int32_t* fidx,
                     const uint16_t* dy, float* part, float* bias_part, int N, int grid, int T, void* stream);

// ---- pong.hip
int rrl_pong_state_size();  // floats of state per env
int rrl_pong_step(float* state, const int32_t* act, float* rew, float* done, float* fin_ret, float* fin_len,
                  float* ep_acc, int N, unsigned long long seed, unsigned long long step,
                  const unsigned long long* step_base, int max_steps, int reset_all, float* hist_out, void* stream);
// frames != nullptr: the frame-ring form (frames [R][N][7056], fidx [N][4]; obs unused)
int rrl_pong_step_render(float* state, const int32_t* act, float* rew, float* done, float* fin_ret, float* fin_len,
                         float* ep_acc, uint8_t* obs, int N, unsigned long long seed, unsigned long long step,
                         const unsigned long long* step_base, int max_steps, int reset_all, uint8_t* frames,
                         int32_t* fidx, int R, void* stream);
int rrl_pong_ring_fill(float* state, uint8_t* frames, int32_t* fidx, int N, int R, unsigned long long step,
                       const unsigned long long* step_base, void* stream);
int rrl_pong_render_hist(const float* hist, uint8_t* obs, int N, void* stream);
int rrl_pong_render(const float* state, uint8_t* obs, int N, void* stream);
int rrl_pong_head_step_render(const float* part, int splits, const float* fc_b, const float* head_params, int A,
                              uint16_t* h_out, int32_t* act, float* logp, float* value,
                              unsigned long long sample_seed, unsigned long long sample_step,
                              const unsigned long long* sample_base, float* state, float* rew, float* done,
                              float* fin_ret, float* fin_len, float* ep_acc, uint8_t* obs, int N,
                              unsigned long long seed, unsigned long long step, const unsigned long long* step_base,
                              int max_steps, uint8_t* frames, int32_t* fidx, int R, void* stream);
// One policy-evaluation step: the head (greedy != 0: lowest index among the maximal logits, else the
// rollout's draw) + env step at the host counter `step` + render (frames + fidx, or obs) of every env
// with ep_cnt[e] < E; the others are frozen and nothing of theirs is written.  A finished episode
// fills slot ep_cnt[e] of ep_ret / ep_len / ep_code [E][N] (code 1: a score reached 21, 2: the time
// limit) and the env's E-th one decrements *remaining.  tr_act / tr_rew / tr_done [N], tr_logits
// [N][A]: all four or none.  -1: a null or inconsistent argument; -2: E or max_steps below 1, or
// E * max_steps >= 2^31; -3: A > 8
int rrl_pong_eval_step(const float* part, int splits, const float* fc_b, const float* head_params, int A, int greedy,
                       unsigned long long sample_seed, unsigned long long sample_step, float* state, float* rew,
                       float* done, float* fin_ret, float* fin_len, uint8_t* obs, int N, unsigned long long seed,
                       unsigned long long step, int max_steps, uint8_t* frames, int32_t* fidx, int R, int E,
                       int32_t* ep_cnt, float* ep_ret, int32_t* ep_len, int32_t* ep_code, int32_t* remaining,
                       int32_t* tr_act, float* tr_logits, float* tr_rew, float* tr_done, void* stream);

}  // extern "C"
