// Driver of tests/test_lm_policy_host.py: csrc/lm_policy.hpp - the product's trust-region rules - compiled with plain g++, no device and no library.
//
//   powell | helloworld   a dense normal-equation Levenberg-Marquardt on Ceres' two tutorial problems in which EVERY decision (the tests before a step,
//                         the verdict on a step, radius, reuse of the diagonal, rows) is LmPolicy's; only the arithmetic of a dense step (evaluation,
//                         Jacobi scale, LM diagonal, Cholesky) is the oracle's.  Prints "policy <7 columns>" rows, the rows of the oracle's own
//                         DenseLevenbergMarquardt as "oracle <7 columns>", the final x and the termination.
//   script                reads commands from stdin and prints the policy's answer and state after each:
//                           opt <name> <value> (before start) | start <cost> <gmax> | before <pending> | resolve <cost> <gmax> |
//                           judge <model_change> <cost> <step_norm2> <x_norm2> <flag> <retry>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../oracle/trust_region.h"
#include "../privacy_preserving_sfm_amd/csrc/lm_policy.hpp"

using ppsfm::LmNext;
using ppsfm::LmPolicy;
using ppsfm::LmTrialStep;
using ppsfm::LmVerdict;
using Eval = std::function<void(const double*, double*, double*)>;

static pp_ba_options CeresDefaults(int max_num_iterations) {
  const oracle::lm::Options d;
  pp_ba_options o;
  std::memset(&o, 0, sizeof(o));
  o.max_num_iterations = max_num_iterations; o.max_num_consecutive_invalid_steps = 5;
  o.function_tolerance = d.function_tolerance; o.gradient_tolerance = d.gradient_tolerance; o.parameter_tolerance = d.parameter_tolerance;
  o.initial_trust_region_radius = d.initial_trust_region_radius; o.max_trust_region_radius = d.max_trust_region_radius;
  o.min_trust_region_radius = d.min_trust_region_radius; o.min_relative_decrease = d.min_relative_decrease;
  o.min_lm_diagonal = d.min_lm_diagonal; o.max_lm_diagonal = d.max_lm_diagonal; o.jacobi_scaling = 1;
  return o;
}

static void PrintRows(const char* tag, const std::vector<double>& trace) {
  for (size_t i = 0; i + 7 <= trace.size(); i += 7) {
    std::printf("%s", tag);
    for (int k = 0; k < 7; ++k) std::printf(" %.17g", trace[i + k]);
    std::printf("\n");
  }
}

// eval(x, r, J): residuals r (m) and the row-major m x n Jacobian J at x
static void DenseSolve(int m, int n, const Eval& eval, double* x, const pp_ba_options& o) {
  namespace lm = oracle::lm;
  std::vector<double> trace, r(m), J((size_t)m * n), rc(m), Jc((size_t)m * n), xc(n), scale(n), g(n), diag(n), A((size_t)n * n), step(n);
  auto cost_of = [&](const std::vector<double>& res) { double c = 0; for (double v : res) c += v * v; return 0.5 * c; };
  auto gradient = [&]() { double gm = 0; for (int j = 0; j < n; ++j) { double s = 0; for (int i = 0; i < m; ++i) s += J[(size_t)i * n + j] * r[i]; g[j] = s; gm = std::fmax(gm, std::fabs(s)); } return gm; };
  eval(x, r.data(), J.data());
  for (int j = 0; j < n; ++j) { double cn = 0; for (int i = 0; i < m; ++i) cn += J[(size_t)i * n + j] * J[(size_t)i * n + j]; scale[j] = lm::JacobiScale(cn); }
  LmPolicy policy(o, trace);
  bool go_on = policy.Start(cost_of(r), gradient());
  while (go_on && policy.BeforeStep(false) == LmNext::kStep && trace.size() < 7 * 400) {
    if (!policy.reuse_diagonal)
      for (int j = 0; j < n; ++j) { double cn = 0; for (int i = 0; i < m; ++i) { const double v = J[(size_t)i * n + j] * scale[j]; cn += v * v; } diag[j] = lm::ClampDiagonal(cn, o.min_lm_diagonal, o.max_lm_diagonal); }
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b) { double s = 0; for (int i = 0; i < m; ++i) s += J[(size_t)i * n + a] * scale[a] * J[(size_t)i * n + b] * scale[b]; A[(size_t)a * n + b] = s; }
    for (int j = 0; j < n; ++j) { const double d = lm::LmD(diag[j], policy.radius); A[(size_t)j * n + j] += d * d; step[j] = -scale[j] * g[j]; }
    LmTrialStep t = {0.0, 0.0, 0.0, 0.0, 0, false};
    if (oracle::CholeskyFactor(n, A.data())) {
      oracle::CholeskySolve(n, A.data(), step.data());
      for (int i = 0; i < m; ++i) { double jd = 0; for (int j = 0; j < n; ++j) jd += J[(size_t)i * n + j] * scale[j] * step[j]; t.model_change -= jd * (r[i] + jd / 2.0); }
      for (int j = 0; j < n; ++j) { const double d = step[j] * scale[j]; t.step_norm2 += d * d; t.x_norm2 += x[j] * x[j]; xc[j] = x[j] + d; }
      eval(xc.data(), rc.data(), Jc.data());
      t.cost = cost_of(rc);
    } else {
      t.flag = 1;      // the failed-pivot bit
    }
    const LmVerdict v = policy.Judge(t);
    if (v == LmVerdict::kAccepted) {      // move, and bring the evaluation at the new point
      for (int j = 0; j < n; ++j) x[j] = xc[j];
      r.swap(rc); J.swap(Jc);
      policy.Resolve(cost_of(r), gradient());
    }
    go_on = !ppsfm::LmTerminates(v);
  }
  PrintRows("policy", trace);
  std::printf("x");
  for (int j = 0; j < n; ++j) std::printf(" %.17g", x[j]);
  std::printf("\ntermination %d\n", policy.termination);
}

static const char* Name(LmVerdict v) {
  switch (v) {
    case LmVerdict::kRetryAfterTimeout: return "retry";
    case LmVerdict::kInvalid: return "invalid";
    case LmVerdict::kInvalidFailed: return "invalid_failed";
    case LmVerdict::kParameterTolerance: return "parameter_tolerance";
    case LmVerdict::kFunctionTolerance: return "function_tolerance";
    case LmVerdict::kAccepted: return "accepted";
    case LmVerdict::kRejected: return "rejected";
  }
  return "?";
}

static int Script() {
  pp_ba_options o = CeresDefaults(50);
  std::vector<double> trace;
  std::vector<LmPolicy> policy;      // (built at "start", from the options set until then)
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, answer = "ok";
    in >> cmd;
    if (cmd.empty()) continue;
    if (cmd == "opt") {
      std::string name; double v = 0;
      in >> name >> v;
      if (name == "max_num_iterations") o.max_num_iterations = (int)v;
      else if (name == "max_num_consecutive_invalid_steps") o.max_num_consecutive_invalid_steps = (int)v;
      else if (name == "function_tolerance") o.function_tolerance = v;
      else if (name == "gradient_tolerance") o.gradient_tolerance = v;
      else if (name == "parameter_tolerance") o.parameter_tolerance = v;
      else if (name == "initial_trust_region_radius") o.initial_trust_region_radius = v;
      else if (name == "max_trust_region_radius") o.max_trust_region_radius = v;
      else if (name == "min_trust_region_radius") o.min_trust_region_radius = v;
      else if (name == "min_relative_decrease") o.min_relative_decrease = v;
      else { std::fprintf(stderr, "unknown option %s\n", name.c_str()); return 2; }
      continue;
    }
    if (cmd == "start") {
      double c = 0, g = 0;
      in >> c >> g;
      policy.emplace_back(o, trace);
      answer = policy[0].Start(c, g) ? "started" : "failure";
    } else if (policy.empty()) {
      std::fprintf(stderr, "%s before start\n", cmd.c_str());
      return 2;
    } else if (cmd == "before") {
      int pending = 0;
      in >> pending;
      const LmNext n = policy[0].BeforeStep(pending != 0);
      answer = n == LmNext::kStep ? "step" : (n == LmNext::kStop ? "stop" : "resolve_first");
    } else if (cmd == "resolve") {
      double c = 0, g = 0;
      in >> c >> g;
      policy[0].Resolve(c, g);
    } else if (cmd == "judge") {
      LmTrialStep t; int flag = 0, retry = 0;
      in >> t.model_change >> t.cost >> t.step_norm2 >> t.x_norm2 >> flag >> retry;
      t.flag = flag; t.retry_after_timeout = retry != 0;
      answer = Name(policy[0].Judge(t));
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
    const LmPolicy& p = policy[0];
    std::printf("%s rows=%d radius=%.17g factor=%.17g reuse=%d last_ok=%d invalid=%d ok=%d bad=%d term=%d cost=%.17g gmax=%.17g\n", answer.c_str(), p.iteration(), p.radius,
                p.decrease_factor, p.reuse_diagonal ? 1 : 0, p.last_successful ? 1 : 0, p.invalid, p.num_successful_steps, p.num_unsuccessful_steps, p.termination, p.cost, p.gmax);
  }
  PrintRows("row", trace);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "script") return Script();
  const double s5 = std::sqrt(5.0), s10 = std::sqrt(10.0);
  // Powell's function and hello-world as Ceres' examples/powell.cc and examples/helloworld.cc state them (the oracle's own drivers restate them too)
  const Eval powell = [=](const double* p, double* r, double* J) {
    r[0] = p[0] + 10.0 * p[1]; r[1] = s5 * (p[2] - p[3]); r[2] = (p[1] - 2.0 * p[2]) * (p[1] - 2.0 * p[2]); r[3] = s10 * (p[0] - p[3]) * (p[0] - p[3]);
    for (int i = 0; i < 16; ++i) J[i] = 0.0;
    J[0] = 1.0; J[1] = 10.0;
    J[4 + 2] = s5; J[4 + 3] = -s5;
    J[8 + 1] = 2.0 * (p[1] - 2.0 * p[2]); J[8 + 2] = -4.0 * (p[1] - 2.0 * p[2]);
    J[12 + 0] = 2.0 * s10 * (p[0] - p[3]); J[12 + 3] = -2.0 * s10 * (p[0] - p[3]);
  };
  const Eval hello = [](const double* p, double* r, double* J) { r[0] = 10.0 - p[0]; J[0] = -1.0; };
  oracle::lm::Options oo;
  std::vector<oracle::lm::Iteration> want;
  if (mode == "powell") {
    double x[4] = {3.0, -1.0, 0.0, 1.0}, xo[4] = {3.0, -1.0, 0.0, 1.0};
    DenseSolve(4, 4, powell, x, CeresDefaults(100));
    oo.max_num_iterations = 100;
    want = oracle::lm::PowellTrace(xo, oo);
  } else if (mode == "helloworld") {
    double x[1] = {0.5}, xo[1] = {0.5};
    DenseSolve(1, 1, hello, x, CeresDefaults(50));
    want = oracle::lm::HelloWorldTrace(xo, oo);
  } else {
    std::fprintf(stderr, "usage: %s powell|helloworld|script\n", argv[0]);
    return 2;
  }
  for (const oracle::lm::Iteration& it : want)
    std::printf("oracle %.17g %.17g %.17g %.17g %.17g %.17g %d\n", it.cost, it.cost_change, it.gradient_max_norm, it.step_norm, it.relative_decrease, it.radius, it.successful);
  return 0;
}
