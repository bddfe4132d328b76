// The trust-region rules of pp_ba_solve: Ceres' TrustRegionMinimizer with the Levenberg-Marquardt strategy as published ("LM loop"), and
// nothing else - no device, no handle, no HIP: host-only and std-only (include/ppsfm_hip.h is plain C), so that tests/test_lm_policy_host.py pins THIS
// code, with g++ and without a GPU, to the iteration tables Ceres publishes.  csrc/ba_solver.hip supplies the numbers (the read-back scalars of a trial
// step, the evaluation at an accepted point) and acts on the verdicts; every decision of the loop is taken here.
//
// The arithmetic is kept letter for letter (std::pow in the radius update, the order of the tests): traces are compared bit for bit between versions.
// init_lsq.hpp's device-side Accept is a different function on purpose (it avoids pow); the test oracle has its own copy (oracle/trust_region.h).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ppsfm_hip.h"

namespace ppsfm {

// what the host reads back of one trial step
struct LmTrialStep {
  double model_change, cost, step_norm2, x_norm2;      // -(J d)'(r + J d / 2), the cost at the candidate, |step|^2, |x|^2
  int32_t flag;                                        // failure bits of the linear solve / the point blocks (0 = none)
  bool retry_after_timeout;                            // the one-launch factorisation ran out of its bounded wait and the caller can repeat it another way
};

enum class LmVerdict { kRetryAfterTimeout, kInvalid, kInvalidFailed, kParameterTolerance, kFunctionTolerance, kAccepted, kRejected };
// the solve ends with this verdict (LmPolicy::termination says how)
inline bool LmTerminates(LmVerdict v) { return v == LmVerdict::kInvalidFailed || v == LmVerdict::kParameterTolerance || v == LmVerdict::kFunctionTolerance; }
// the solve goes on FROM THE OLD POINT: whoever evaluated the candidate in its place ahead of the verdict has to evaluate the old point again
inline bool LmStaysAtOldPoint(LmVerdict v) { return v == LmVerdict::kRetryAfterTimeout || v == LmVerdict::kInvalid || v == LmVerdict::kRejected; }

enum class LmNext { kStep, kStop, kResolveFirst };

// Invariant: `cost`, `gmax` and the last trace row describe the current (last accepted) point - provisionally after an accepted step (the candidate's
// cost, the previous gradient norm) until Resolve brings the evaluation made there; `radius` is the radius of the NEXT trial step.
struct LmPolicy {
  const pp_ba_options o;
  std::vector<double>& trace;      // rows of 7: cost, cost_change, |gradient|_max, |step|, relative decrease, radius, successful
  double cost = 0.0, gmax = 0.0, radius = 0.0, decrease_factor = 2.0;
  bool reuse_diagonal = false, last_successful = true;
  int invalid = 0, num_successful_steps = 0, num_unsuccessful_steps = 0;
  int termination = PP_TERM_NO_CONVERGENCE;

  LmPolicy(const pp_ba_options& options, std::vector<double>& rows) : o(options), trace(rows) {}

  // row 0: the initial evaluation.  false = the cost is not finite (termination = FAILURE)
  bool Start(double initial_cost, double initial_gmax) {
    cost = initial_cost; gmax = initial_gmax; radius = o.initial_trust_region_radius;
    Push(cost, 0, gmax, 0, 0, radius, 1);
    if (!std::isfinite(cost)) termination = PP_TERM_FAILURE;
    return termination != PP_TERM_FAILURE;
  }
  // every iteration adds exactly one row, a repeated step after a timeout none: the number of the iteration about to be made
  int iteration() const { return (int)(trace.size() / 7); }
  const double* last_row() const { return trace.data() + trace.size() - 7; }

  // The tests before a trial step, in Ceres' order.  `pending`: the evaluation at the current point has not arrived yet, so the gradient test has to
  // wait for it - unless the solve would end here anyway: then the caller resolves it first (kResolveFirst) and asks again with pending = false.
  LmNext BeforeStep(bool pending) {
    if (pending && (iteration() > o.max_num_iterations || radius < o.min_trust_region_radius)) return LmNext::kResolveFirst;
    if (!pending && GradientToleranceReached()) return LmNext::kStop;
    if (iteration() > o.max_num_iterations) { termination = PP_TERM_NO_CONVERGENCE; return LmNext::kStop; }
    if (radius < o.min_trust_region_radius) { termination = PP_TERM_CONVERGENCE; return LmNext::kStop; }
    return LmNext::kStep;
  }
  // only ever true at a point a successful step led to (or the start); sets the termination
  bool GradientToleranceReached() {
    if (!(last_successful && gmax <= o.gradient_tolerance)) return false;
    termination = PP_TERM_CONVERGENCE;
    return true;
  }
  // the evaluation at the accepted point has arrived: replaces the provisional cost / the previous gradient norm, also in the last row
  void Resolve(double evaluated_cost, double evaluated_gmax) {
    cost = evaluated_cost; gmax = evaluated_gmax;
    double* row = trace.data() + trace.size() - 7;
    row[0] = cost; row[2] = gmax;
  }

  // Exactly one verdict per trial step, applied to the state here (radius, factor, counters, row, termination).
  LmVerdict Judge(const LmTrialStep& t) {
    reuse_diagonal = true;      // the LM diagonal now belongs to the current point: it stays until an accepted step leaves the point
    if (t.retry_after_timeout) return LmVerdict::kRetryAfterTimeout;      // nothing wrong with the system: not an iteration
    const double model_change = t.model_change, ccost = t.cost;
    const double step_norm = std::sqrt(t.step_norm2), x_norm = std::sqrt(t.x_norm2);
    const bool valid = t.flag == 0 && std::isfinite(model_change) && model_change > 0.0 && std::isfinite(step_norm);
    if (!valid) {
      ++invalid;
      if (invalid >= o.max_num_consecutive_invalid_steps) { termination = PP_TERM_FAILURE; return LmVerdict::kInvalidFailed; }
      Shrink();
      Push(cost, 0, gmax, 0, 0, radius, 0);
      return LmVerdict::kInvalid;
    }
    invalid = 0;
    if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { termination = PP_TERM_CONVERGENCE; return LmVerdict::kParameterTolerance; }
    const double cost_change = cost - ccost;
    // (Ceres records this iteration and moves to the candidate before it stops; this loop, like oracle/bundle_adjustment.h, does neither)
    if (std::fabs(cost_change) <= o.function_tolerance * cost) { termination = PP_TERM_CONVERGENCE; return LmVerdict::kFunctionTolerance; }
    const double rel = cost_change / model_change;
    if (rel > o.min_relative_decrease) {
      cost = ccost;     // provisional (the candidate evaluation); replaced by the re-evaluated cost when it arrives
      radius = radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rel - 1.0, 3));
      radius = std::fmin(o.max_trust_region_radius, radius);
      decrease_factor = 2.0; reuse_diagonal = false;
      ++num_successful_steps; last_successful = true;
      Push(cost, cost_change, gmax, step_norm, rel, radius, 1);
      return LmVerdict::kAccepted;
    }
    Shrink();
    Push(cost, cost_change, gmax, step_norm, rel, radius, 0);
    return LmVerdict::kRejected;
  }

 private:
  void Push(double c, double dc, double g, double sn, double rel, double rad, int ok) {
    const double row[7] = {c, dc, g, sn, rel, rad, (double)ok};
    trace.insert(trace.end(), row, row + 7);
  }
  // an unsuccessful (invalid or rejected) step
  void Shrink() {
    radius /= decrease_factor; decrease_factor *= 2.0;
    ++num_unsuccessful_steps; last_successful = false;
  }
};

}  // namespace ppsfm
