// Bindings of the DQN kernels (csrc/kernels/dqn.hip): the epsilon-greedy actor that fills the replay
// ring and the sample + gather + TD-target launch (one dqn_targets for every form), of the priority sum
// tree (csrc/kernels/per.hip) and of the noisy layers (csrc/kernels/noisy.hip).  Every tensor is
// validated before a launch.
#include <algorithm>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "api.h"
#include "check.h"

namespace {

using namespace rrl;
using namespace rrl_bind;

int64_t dqn_rollout_grid(int64_t N) { return rrl_dqn_rollout_grid((int)N, grid_cus()); }

// The ring is obs / nobs [C, N, D], act / rew / done [C, N]; returns (C, N).
std::tuple<int64_t, int64_t> check_ring(int64_t D, const Tensor& obs, const Tensor& nobs, const Tensor& act,
                                        const Tensor& rew, const Tensor& done) {
  check(act, "ring act", at::kInt);
  TORCH_CHECK(act.dim() == 2 && act.size(0) >= 1 && act.size(1) >= 1, "ring act must be [C, N]");
  const int64_t C = act.size(0), N = act.size(1);
  TORCH_CHECK(C * N * std::max<int64_t>(D, 1) < (int64_t)INT32_MAX, "replay ring too large for 32-bit rows");
  check(obs, "ring obs", at::kFloat, C * N * D);
  check(nobs, "ring nobs", at::kFloat, C * N * D);
  check(rew, "ring rew", at::kFloat, C * N);
  check(done, "ring done", at::kFloat, C * N);
  TORCH_CHECK(obs.numel() == C * N * D && nobs.numel() == C * N * D && rew.numel() == C * N && done.numel() == C * N,
              "ring tensors disagree on [C, N, D]");
  return {C, N};
}

// Outputs of a Q-network over A actions: the dueling net has one more, the state value, and kMaxAct = 16
// outputs are what the kernels hold.
int64_t dueling_outputs(int64_t A, bool dueling) {
  TORCH_CHECK(!dueling || A <= 15, "a dueling net has A + 1 outputs: act dim must be in [1, 15], got ", A);
  return A + (dueling ? 1 : 0);
}

// Outputs of a quantile Q-network over A actions, NQ per action (0: the scalar net, dueling or not).
int64_t q_outputs(int64_t A, bool dueling, int64_t quantiles) {
  TORCH_CHECK(quantiles >= 0, "quantiles must be >= 0, got ", quantiles);
  TORCH_CHECK(quantiles == 0 || !dueling, "quantiles with dueling is not built: set one of the two");
  TORCH_CHECK(A * quantiles <= 16, "a quantile net has A * quantiles <= 16 outputs, got ", A, " * ", quantiles);
  return quantiles > 0 ? A * quantiles : dueling_outputs(A, dueling);
}

// Returns the kernel's code for a launch that would wrap (-4, nothing written); raises for anything else.
int64_t dqn_rollout_qr(int64_t env, const Tensor& params, int64_t H, int64_t T, int64_t slot0, const Tensor& state,
                    const Tensor& ep_len, const Tensor& ep_ret, const Tensor& obs, const Tensor& nobs,
                    const Tensor& act, const Tensor& rew, const Tensor& done, const Tensor& ep_stats, int64_t seed,
                    int64_t step0, double epsilon, bool reset_all, int64_t max_steps, bool dueling,
                    int64_t quantiles) {
  int D = 0, A = 0, NS = 0, ms = 0;
  TORCH_CHECK(rrl_env_dims((int)env, &D, &A, &NS, &ms) == 0, "unknown device env id ", env);
  TORCH_CHECK(env != ENV_HALFCHEETAH, "dqn_rollout takes the discrete device envs");
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(T >= 1 && max_steps >= 1, "T and max_steps must be >= 1");
  const int64_t AO = q_outputs(A, dueling, quantiles);
  check(params, "params", at::kFloat, (int64_t)H * D + H + H * H + H + AO * H + AO);
  TORCH_CHECK(quantiles == 0 || params.numel() == (int64_t)H * D + H + H * H + H + AO * H + AO,
              "params is not the quantile net MLPSpec(D, H, A * quantiles)");
  auto [C, N] = check_ring(D, obs, nobs, act, rew, done);
  check(state, "state", at::kFloat, N * NS);
  check(ep_len, "ep_len", at::kInt, N);
  check(ep_ret, "ep_ret", at::kFloat, N);
  check(ep_stats, "ep_stats", at::kFloat, dqn_rollout_grid(N) * 8);
  TORCH_CHECK(slot0 >= 0 && slot0 < (int64_t)INT32_MAX && T < (int64_t)INT32_MAX, "slot0 / T out of range");
  const int rc = rrl_dqn_rollout((int)env, params.data_ptr<float>(), (int)N, (int)T, (int)H, (int)C, (int)slot0,
                                 state.data_ptr<float>(), ep_len.data_ptr<int>(), ep_ret.data_ptr<float>(),
                                 obs.data_ptr<float>(), nobs.data_ptr<float>(), act.data_ptr<int>(),
                                 rew.data_ptr<float>(), done.data_ptr<float>(), ep_stats.data_ptr<float>(),
                                 (uint64_t)seed, (uint64_t)step0, (float)epsilon, reset_all ? 1 : 0, (int)max_steps,
                                 dueling ? 1 : 0, (int)quantiles, grid_cus(), cur_stream());
  if (rc == -4) return rc;
  check_rc(rc, "dqn_rollout");
  return 0;
}

// The scalar nets (plain or dueling): the binding as it always parsed.
int64_t dqn_rollout(int64_t env, const Tensor& params, int64_t H, int64_t T, int64_t slot0, const Tensor& state,
                    const Tensor& ep_len, const Tensor& ep_ret, const Tensor& obs, const Tensor& nobs,
                    const Tensor& act, const Tensor& rew, const Tensor& done, const Tensor& ep_stats, int64_t seed,
                    int64_t step0, double epsilon, bool reset_all, int64_t max_steps, bool dueling) {
  return dqn_rollout_qr(env, params, H, T, slot0, state, ep_len, ep_ret, obs, nobs, act, rew, done, ep_stats, seed,
                        step0, epsilon, reset_all, max_steps, dueling, 0);
}

// ------------------------------------------------------------------ prioritised replay (per.hip)
int64_t per_tree_leaves(int64_t L) { return rrl_per_tree_leaves((long long)L); }

// tree [2 * P2] for a ring of L rows and a one-float companion (pmax, wmax); returns P2
int64_t check_tree(const Tensor& tree, const Tensor& one, const char* one_name, int64_t L) {
  const int64_t P2 = per_tree_leaves(L);
  TORCH_CHECK(P2 >= 1, "a priority tree needs 1 <= C * N <= 2^30 rows, got ", L);
  check(tree, "tree", at::kFloat, 2 * P2);
  TORCH_CHECK(tree.numel() == 2 * P2, "tree must hold 2 * ", P2, " floats for ", L, " rows, has ", tree.numel());
  check(one, one_name, at::kFloat, 1);
  return P2;
}

// Returns the kernel's code for a range that would wrap (-4, nothing written); raises for anything else.
int64_t per_insert(const Tensor& tree, const Tensor& pmax, int64_t C, int64_t N, int64_t T, int64_t slot0) {
  TORCH_CHECK(C >= 1 && N >= 1 && T >= 1 && C < (int64_t)INT32_MAX && N < (int64_t)INT32_MAX &&
                  T < (int64_t)INT32_MAX && slot0 >= 0 && slot0 < (int64_t)INT32_MAX,
              "C, N, T must be >= 1 and slot0 >= 0, all below 2^31");
  check_tree(tree, pmax, "pmax", C * N);
  const int rc = rrl_per_insert(tree.data_ptr<float>(), pmax.data_ptr<float>(), (int)C, (int)N, (int)T, (int)slot0,
                                cur_stream());
  if (rc == -4) return rc;
  check_rc(rc, "per_insert");
  return 0;
}

void per_update(const Tensor& tree, const Tensor& pmax, int64_t L, const Tensor& idx, const Tensor& td_abs,
                double alpha, double prio_eps) {
  check_tree(tree, pmax, "pmax", L);
  check(idx, "idx", at::kInt, 1);
  const int64_t B = idx.numel();
  TORCH_CHECK(B < (int64_t)INT32_MAX, "batch size out of range");
  check(td_abs, "td_abs", at::kFloat, B);
  TORCH_CHECK(alpha >= 0.0 && prio_eps > 0.0, "per_update needs alpha >= 0 and prio_eps > 0");
  check_rc(rrl_per_update(tree.data_ptr<float>(), pmax.data_ptr<float>(), idx.data_ptr<int>(),
                          td_abs.data_ptr<float>(), (int)B, (long long)L, (float)alpha, (float)prio_eps, cur_stream()),
           "per_update");
}

// ------------------------------------------------------------------ TD targets (dqn.hip)
// One launch for every form: a tree selects the prioritised one (it needs beta, idx, w and wmax, which are not
// looked at without one), n_step > 1 the walk.  Without `newest` there is no walk to check and the slots are one
// row each (N = 1, newest = 0); with it N is the ring's, and n_step, filled % N and newest are the entry point's
// to refuse.
void dqn_targets_qr(const OptT& online, const Tensor& target, int64_t H, int64_t A, const Tensor& obs,
                    const Tensor& nobs, const Tensor& act, const Tensor& rew, const Tensor& done, int64_t filled,
                    double gamma, bool double_q, int64_t sample_key, int64_t update, const Tensor& Xb,
                    const Tensor& act_b, const Tensor& y, const OptT& idx, const OptT& tree,
                    std::optional<double> beta, const OptT& w, const OptT& wmax, int64_t n_step,
                    std::optional<int64_t> newest, const OptT& last, bool dueling, int64_t quantiles) {
  TORCH_CHECK(obs.dim() == 3, "ring obs must be [C, N, D]");
  const int64_t D = obs.size(2);
  TORCH_CHECK(H == 64 || H == 128, "hidden size must be 64 or 128");
  TORCH_CHECK(D >= 1 && D <= 16, "obs dim must be in [1, 16]");
  TORCH_CHECK(A >= 1 && A <= 16, "act dim must be in [1, 16]");
  const int64_t AO = q_outputs(A, dueling, quantiles);
  const int64_t NQ = std::max<int64_t>(quantiles, 1);  // targets per batch row
  auto [C, N] = check_ring(D, obs, nobs, act, rew, done);
  TORCH_CHECK(filled >= 1 && filled <= C * N, "filled must be in [1, C * N], got ", filled);
  const int64_t P = H * D + H + H * H + H + AO * H + AO;
  check(target, "target", at::kFloat, P);
  const float* on = opt_ptr<const float>(online, "online", at::kFloat, P);
  TORCH_CHECK(!double_q || on != nullptr, "double_q needs the online parameters");
  check(y, "y", at::kFloat);
  TORCH_CHECK(y.numel() % NQ == 0, "y must hold quantiles = ", NQ, " targets per batch row, has ", y.numel());
  const int64_t B = y.numel() / NQ;
  TORCH_CHECK(B >= 1 && B * D < (int64_t)INT32_MAX, "batch size out of range");
  check(Xb, "Xb", at::kFloat, B * D);
  check(act_b, "act_b", at::kInt, B);
  const int64_t nw = newest.value_or(0);
  TORCH_CHECK(std::abs(n_step) < (int64_t)INT32_MAX && std::abs(nw) < (int64_t)INT32_MAX,
              "n_step / newest out of range");
  DqnTargetsCall c{};
  if (tree.has_value()) {
    TORCH_CHECK(beta.has_value() && idx.has_value() && w.has_value() && wmax.has_value(),
                "the prioritised form needs beta, idx, w and wmax");
    TORCH_CHECK(*beta > 0.0 && *beta <= 1.0, "beta must be in (0, 1], got ", *beta);
    check_tree(*tree, *wmax, "wmax", C * N);
    check(*w, "w", at::kFloat, B);
    c.tree = tree->data_ptr<float>();
    c.L = C * N;
    c.beta = (float)*beta;
    c.w = w->data_ptr<float>();
    c.wmax = wmax->data_ptr<float>();
  }
  c.online = on;
  c.target = target.data_ptr<float>();
  c.obs = obs.data_ptr<float>();
  c.nobs = nobs.data_ptr<float>();
  c.act = act.data_ptr<int>();
  c.rew = rew.data_ptr<float>();
  c.done = done.data_ptr<float>();
  c.filled = filled;
  c.B = (int)B, c.D = (int)D, c.A = (int)A, c.H = (int)H;
  c.gamma = (float)gamma;
  c.double_q = double_q ? 1 : 0;
  c.dueling = dueling ? 1 : 0;
  c.quantiles = (int)quantiles;
  c.sample_key = (uint64_t)sample_key;
  c.update = (uint64_t)update;
  c.Xb = Xb.data_ptr<float>();
  c.act_b = act_b.data_ptr<int>();
  c.y = y.data_ptr<float>();
  c.idx = opt_ptr<int>(idx, "idx", at::kInt, B);
  c.n_step = (int)n_step;
  c.N = newest.has_value() ? (int)N : 1;
  c.newest = (int)nw;
  c.last = opt_ptr<int>(last, "last", at::kInt, B);
  check_rc(rrl_dqn_targets(&c, grid_cus(), cur_stream()), "dqn_targets");
}

// The scalar nets (plain or dueling): the binding as it always parsed.
void dqn_targets(const OptT& online, const Tensor& target, int64_t H, int64_t A, const Tensor& obs, const Tensor& nobs,
                 const Tensor& act, const Tensor& rew, const Tensor& done, int64_t filled, double gamma, bool double_q,
                 int64_t sample_key, int64_t update, const Tensor& Xb, const Tensor& act_b, const Tensor& y,
                 const OptT& idx, const OptT& tree, std::optional<double> beta, const OptT& w, const OptT& wmax,
                 int64_t n_step, std::optional<int64_t> newest, const OptT& last, bool dueling) {
  dqn_targets_qr(online, target, H, A, obs, nobs, act, rew, done, filled, gamma, double_q, sample_key, update, Xb,
                 act_b, y, idx, tree, beta, w, wmax, n_step, newest, last, dueling, 0);
}

// ------------------------------------------------------------------ noisy layers (noisy.hip)
// A shape the entry points refuse is theirs to refuse (the code comes back, nothing is launched); for a shape
// they take, every tensor is sized here first.  Returns 0 or the negative code; a HIP error raises.
bool noisy_shape_ok(int64_t D, int64_t H, int64_t A_out) {
  return D >= 1 && D <= 16 && A_out >= 1 && A_out <= 16 && (H == 64 || H == 128);
}

int narrow(int64_t v) { return v < -1 || v > (int64_t)INT32_MAX ? -1 : (int)v; }

int64_t noisy_compose(const std::vector<OptT>& thetas, const std::vector<int64_t>& roles,
                      const std::vector<int64_t>& draws, int64_t D, int64_t H, int64_t A_out, int64_t key,
                      const OptT& out, const OptT& units_out) {
  const int64_t njobs = (int64_t)roles.size();
  TORCH_CHECK((int64_t)thetas.size() == njobs && (int64_t)draws.size() == njobs,
              "noisy_compose takes one theta, role and draw per job");
  const bool ok = noisy_shape_ok(D, H, A_out) && njobs >= 1 && njobs <= 3;
  const int64_t P = H * D + H + H * H + H + A_out * H + A_out, U = D + 4 * H + A_out;
  std::vector<const float*> tp;
  std::vector<int> rl;
  std::vector<uint64_t> dr;
  for (int64_t k = 0; k < njobs; ++k) {
    tp.push_back(ok ? opt_ptr<const float>(thetas[k], "theta", at::kFloat, 2 * P) : nullptr);
    rl.push_back(narrow(roles[k]));
    dr.push_back((uint64_t)draws[k]);
  }
  float* o = ok ? opt_ptr<float>(out, "out", at::kFloat, njobs * P) : nullptr;
  float* uo = ok ? opt_ptr<float>(units_out, "units_out", at::kFloat, njobs * U) : nullptr;
  static const float dummy = 0.f;  // a refused shape never dereferences its pointers: they only must not be null
  if (!ok) {
    tp.assign((size_t)std::max<int64_t>(njobs, 1), &dummy);
    o = const_cast<float*>(&dummy);
    if (njobs == 0) {
      rl.push_back(0);
      dr.push_back(0);
    }
  }
  const int rc = rrl_noisy_compose(tp.data(), narrow(njobs), rl.data(), dr.data(), narrow(D),
                                   narrow(H), narrow(A_out), (uint64_t)key, o, uo, grid_cus(), cur_stream());
  if (rc < 0) return rc;
  check_rc(rc, "noisy_compose");
  return 0;
}

int64_t noisy_grad(const OptT& slab, int64_t role, int64_t draw, int64_t D, int64_t H, int64_t A_out, int64_t key,
                   const OptT& grad_out, int64_t nslab) {
  const bool ok = noisy_shape_ok(D, H, A_out) && nslab >= 1;
  const int64_t P = H * D + H + H * H + H + A_out * H + A_out;
  TORCH_CHECK(nslab < (int64_t)INT32_MAX / std::max<int64_t>(P, 1), "too many slabs");
  static const float dummy = 0.f;
  const float* s = ok ? opt_ptr<const float>(slab, "slab", at::kFloat, nslab * P) : &dummy;
  float* g = ok ? opt_ptr<float>(grad_out, "grad_out", at::kFloat, 2 * P) : const_cast<float*>(&dummy);
  const int rc = rrl_noisy_grad(s, narrow(nslab), narrow(P), narrow(role), (uint64_t)draw, narrow(D), narrow(H),
                                narrow(A_out), (uint64_t)key, g, grid_cus(), cur_stream());
  if (rc < 0) return rc;
  check_rc(rc, "noisy_grad");
  return 0;
}

}  // namespace

void register_dqn_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.def("noisy_compose", &noisy_compose, py::arg("thetas"), py::arg("roles"), py::arg("draws"), py::arg("D"),
        py::arg("H"), py::arg("A_out"), py::arg("key"), py::arg("out"), py::arg("units_out"));
  m.def("noisy_grad", &noisy_grad, py::arg("slab"), py::arg("role"), py::arg("draw"), py::arg("D"), py::arg("H"),
        py::arg("A_out"), py::arg("key"), py::arg("grad_out"), py::arg("nslab"));
  m.def("per_tree_leaves", &per_tree_leaves);
  m.def("per_insert", &per_insert, py::arg("tree"), py::arg("pmax"), py::arg("C"), py::arg("N"), py::arg("T"),
        py::arg("slot0"));
  m.def("per_update", &per_update, py::arg("tree"), py::arg("pmax"), py::arg("L"), py::arg("idx"), py::arg("td_abs"),
        py::arg("alpha"), py::arg("prio_eps"));
  m.def("dqn_rollout_grid", &dqn_rollout_grid);
  m.def("dqn_rollout", &dqn_rollout, py::arg("env"), py::arg("params"), py::arg("H"), py::arg("T"), py::arg("slot0"),
        py::arg("state"), py::arg("ep_len"), py::arg("ep_ret"), py::arg("obs"), py::arg("nobs"), py::arg("act"),
        py::arg("rew"), py::arg("done"), py::arg("ep_stats"), py::arg("seed"), py::arg("step0"), py::arg("epsilon"),
        py::arg("reset_all"), py::arg("max_steps"), py::arg("dueling") = false);
  m.def("dqn_rollout_qr", &dqn_rollout_qr, py::arg("env"), py::arg("params"), py::arg("H"), py::arg("T"),
        py::arg("slot0"), py::arg("state"), py::arg("ep_len"), py::arg("ep_ret"), py::arg("obs"), py::arg("nobs"),
        py::arg("act"), py::arg("rew"), py::arg("done"), py::arg("ep_stats"), py::arg("seed"), py::arg("step0"),
        py::arg("epsilon"), py::arg("reset_all"), py::arg("max_steps"), py::arg("dueling") = false,
        py::arg("quantiles") = 0);
  m.def("dqn_targets", &dqn_targets, py::arg("online"), py::arg("target"), py::arg("H"), py::arg("A"), py::arg("obs"),
        py::arg("nobs"), py::arg("act"), py::arg("rew"), py::arg("done"), py::arg("filled"), py::arg("gamma"),
        py::arg("double_q"), py::arg("sample_key"), py::arg("update"), py::arg("Xb"), py::arg("act_b"), py::arg("y"),
        py::arg("idx"), py::arg("tree") = py::none(), py::arg("beta") = py::none(), py::arg("w") = py::none(),
        py::arg("wmax") = py::none(), py::arg("n_step") = 1, py::arg("newest") = py::none(),
        py::arg("last") = py::none(), py::arg("dueling") = false);
  m.def("dqn_targets_qr", &dqn_targets_qr, py::arg("online"), py::arg("target"), py::arg("H"), py::arg("A"),
        py::arg("obs"), py::arg("nobs"), py::arg("act"), py::arg("rew"), py::arg("done"), py::arg("filled"),
        py::arg("gamma"), py::arg("double_q"), py::arg("sample_key"), py::arg("update"), py::arg("Xb"),
        py::arg("act_b"), py::arg("y"), py::arg("idx"), py::arg("tree") = py::none(), py::arg("beta") = py::none(),
        py::arg("w") = py::none(), py::arg("wmax") = py::none(), py::arg("n_step") = 1, py::arg("newest") = py::none(),
        py::arg("last") = py::none(), py::arg("dueling") = false, py::arg("quantiles") = 0);
}
