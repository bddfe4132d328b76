// The Levenberg-Marquardt driver: the device-side replacement of ceres::Solve as the
// reference configures it (src/optim/bundle_adjustment.cc:273-306, options from
// src/optim/bundle_adjustment.h:80-93 and src/controllers/incremental_mapper.cc:196-243).
//
// Per LM iteration, all on the handle's stream (the host only reads back a few scalars): K1 residuals + Jacobians (ba_eval.hip), K2 the normal-equation
// blocks (ba_step.hip), K3a the damped reduced camera system (ba_schur.hip), K3b its Cholesky (cholesky.hip) or conjugate gradients (ba_pcg.hip), K3c the
// step kernels and the norms (ba_step.hip).  K3c is k_step_points - point steps, model cost change, the trial point and the COST there in one pass, variable
// intrinsics included; the two-kernel form (k_backsub_points, k_model_cost_apply, K1 in cost-only mode where the trial cost is not fused) is its A/B partner
// (PPSFM_BA_FUSED_STEP=0) and the path of a host-callback group.
// Here: the solver buffers, the group exchange, the order of those calls (StepPlan: which form, decided once per solve), the speculation around the verdict,
// the ticket wait and the C entry points.
// The trust-region logic restates Ceres' published Levenberg-Marquardt strategy (radius update,
// Jacobi scaling fixed at the first point, clamped LM diagonal, invalid/unsuccessful step handling),
// see DESIGN.md §LM and lm_policy.hpp; Ceres itself is third-party and not part of the reference.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ba_impl.hpp"
#include "host_ticket.hpp"
#include "lm_policy.hpp"
#include "resource_pool.hpp"
#include "rccl_comm.hpp"

namespace ppsfm {

// (re)binds the factorisation to the handle's current state: the tile map (or none) and the solved-tile array of the one-launch path
// (allocated only when that path can run: N x N doubles, 7 GB at 5000 images)
static int ApplyLinearSolverStructure(pp_ba_impl* h) {
  if (!h->S || h->iterative) return PP_OK;      // EnsureSolverBuffers calls this once the buffers exist; an iterative handle has no factorisation
  // the setters that end up here (pp_ba_set_communicator / pp_ba_set_allreduce) may be called, after a solve, from a host thread whose
  // current device is another one: the allocations below belong on the handle's device
  PP_HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::recursive_mutex> setup_lock(DeviceSetupMutex());
  if (!h->Lfac && CholeskyNeedsFactorArray(h->chol, h->N)) PP_TRY(h->blocks.Alloc(&h->Lfac, (size_t)h->N * h->N));
  // (the solution comes out in the reduced system's column order: the vectors' order unless the intrinsics sit beside their images' pose columns)
  const CholeskySystem sys{h->S, h->N, h->n_red, h->Linv, h->Lfac, h->spos_identity ? h->step_c : h->step_s, h->d_flag, h->stream};
  bool new_map = false;
  { const int rc = CholeskyBind(h->chol, sys, BaSparseActive(h) ? h->tile_nz.data() : nullptr, &new_map); if (rc) return rc; }
  // whatever an earlier factorisation left outside the tiles the new structure rewrites
  if (new_map) PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, h->stream));
  return PP_OK;
}

static int EnsureSolverBuffers(pp_ba_impl* h) {
  if (h->S || h->pcg_state) return PP_OK;
  std::lock_guard<std::recursive_mutex> setup_lock(DeviceSetupMutex());      // (allocations: not beside another host thread's graph capture)
  const int C = h->C, P = h->P;
  h->N = ((h->n_red + 1 + 63) / 64) * 64;
  DeviceBlocks& B = h->blocks;
  const size_t n = (size_t)h->n_red, N = (size_t)h->N;
  PP_TRY(B.Alloc(&h->U, 36 * (size_t)C)); PP_TRY(B.Alloc(&h->gc, n)); PP_TRY(B.Alloc(&h->V, 6 * (size_t)P)); PP_TRY(B.Alloc(&h->gp, 3 * (size_t)P));
  PP_TRY(B.Alloc(&h->Vinv, 6 * (size_t)P)); PP_TRY(B.Alloc(&h->vb, 3 * (size_t)P));
  PP_TRY(B.Alloc(&h->scale_c, n)); PP_TRY(B.Alloc(&h->scale_p, 3 * (size_t)P)); PP_TRY(B.Alloc(&h->diag_c, n)); PP_TRY(B.Alloc(&h->diag_p, 3 * (size_t)P));
  if (!h->iterative) { PP_TRY(B.Alloc(&h->S, N * N)); PP_TRY(B.Alloc(&h->Linv, CholeskyWorkspaceDoubles(h->N))); }
  PP_TRY(B.Alloc(&h->JpS, kRecStride * (size_t)h->M)); PP_TRY(B.Alloc(&h->norm_part, 3 * 256)); PP_TRY(B.Alloc(&h->step_c, N)); PP_TRY(B.Alloc(&h->step_p, 3 * (size_t)P));
  if (!h->spos_identity) PP_TRY(B.Alloc(&h->step_s, N));
  for (int i = 0; i < 8; ++i) PP_TRY(PoolEventAcquire(&h->tev[i], true));
  for (int i = 0; i < 2; ++i) PP_TRY(PoolEventAcquire(&h->tev_eval[i], true));
  PP_TRY(PoolEventAcquire(&h->ev_readback, false));
  if (h->iterative) return PcgEnsureBuffers(h);
  PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, h->stream));
  if (h->sparse_tiles) {      // the factorisation and the assembly skip the tiles that stay zero
    const int T = h->N / 64;
    std::vector<int32_t> list;
    for (int i = 0; i < T; ++i) for (int j = 0; j <= i; ++j) if (h->tile_nz[(size_t)i * T + j]) { list.push_back(i); list.push_back(j); }
    PP_TRY(B.Put(&h->nz_tile_list, list.data(), list.size(), h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return ApplyLinearSolverStructure(h);
}

// the group exchange (declared in ba_impl.hpp: the assembly and the PCG loop use it too)
bool BaInGroup(const pp_ba_impl* h) { return h->comm != nullptr || h->allreduce != nullptr; }
int BaGroupReduce(pp_ba_impl* h, double* ptr, int64_t count, int op) {
  if (h->comm) return CommAllReduce(h->comm, ptr, count, op, h->stream);      // stream-ordered: no host synchronisation
  if (!h->allreduce) return PP_OK;
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  const int rc = h->allreduce(h->allreduce_ctx, ptr, count, op);
  if (rc) { SetLastError("allreduce callback returned %d", rc); return PP_ERR_INVALID; }
  return PP_OK;
}
static int GroupEnd(pp_ba_impl* h) { return h->comm ? CommGroupEnd() : PP_OK; }
int GroupScope::Begin() { const int rc = h->comm ? CommGroupStart() : PP_OK; open = rc == PP_OK; return rc; }
int GroupScope::End() { open = false; return GroupEnd(h); }
GroupScope::~GroupScope() { if (open) (void)GroupEnd(h); }
// The failure bits (d_flag[0]: 1 = pivot, 2 = point block, 4 = a bounded wait of the one-launch factorisation ran out) are rank-local,
// the decisions they drive (invalid step, retry with per-column launches) issue collectives: every rank of a group must take the same
// one.  The bits travel as a double through the unused device slot kTicketSlot, MAX-reduced with the scalars of the trial step.
__global__ void k_flag_to_scalar(const int32_t* __restrict__ flag, double* __restrict__ slot) { *slot = (double)(*flag & 7); }
__global__ void k_scalar_to_flag(const double* __restrict__ slot, int32_t* __restrict__ flag) { const int v = (int)*slot; if (v) atomicOr(flag, v); }

// K1 (Jacobian) + K2 at the current parameters; leaves cost in scal[kCost]
// fold_cost: the cost partials are summed by the LaunchNorms call that follows (fold = 1) instead of a kernel of their own
static int EvaluateAndReduce(pp_ba_impl* h, bool fold_cost = false) {
  int rc = LaunchEval(h, 0, h->NI > 0 ? 1 : 0, true, h->poses, h->points, fold_cost ? nullptr : h->scal + kCost, /*compact_cam=*/true);
  if (rc) return rc;
  if ((rc = BaReduceNormalEquations(h))) return rc;
  if ((rc = IntrSumsAfterEval(h))) return rc;
  if (BaInGroup(h)) {      // the per-pose blocks (and the intrinsics sums) of all shards: one exchange
    GroupScope g(h);
    if ((rc = g.Begin())) return rc;
    if ((rc = BaGroupReduce(h, h->U, 36 * (int64_t)h->C, PP_REDUCE_SUM))) return rc;
    if ((rc = BaGroupReduce(h, h->gc, (int64_t)h->n_red, PP_REDUCE_SUM))) return rc;
    if (h->NI > 0 && (rc = BaGroupReduce(h, h->cnI, (int64_t)h->NI, PP_REDUCE_SUM))) return rc;
    if (!fold_cost && (rc = BaGroupReduce(h, h->scal + kCost, 1, PP_REDUCE_SUM))) return rc;
    if ((rc = g.End())) return rc;
  }
  return PP_OK;
}

// the norms kernels (fold, host_slot, ticket: BaLaunchNorms) and, in a group, the exchange of what they left in the device scalars
static int LaunchNorms(pp_ba_impl* h, bool with_step, int fold = 0, double* host_slot = nullptr, unsigned long long ticket = 0) {
  if (const int rc = BaLaunchNorms(h, with_step, fold, host_slot, ticket)) return rc;
  if (BaInGroup(h)) {
    // one exchange for the scalars of this evaluation: the gradient max norm as a max; |step|^2 and |x|^2 as sums (the point
    // parts are sharded, the replicated pose / intrinsics parts were counted on rank 0 only: parameter_tolerance sees the
    // same global norms on every rank); the sums this call folded (cost, or candidate cost + model cost change) as sums
    int rc;
    if (with_step) hipLaunchKernelGGL(k_flag_to_scalar, dim3(1), dim3(1), 0, h->stream, h->d_flag, h->scal + kTicketSlot);
    {
      GroupScope g(h);
      if ((rc = g.Begin())) return rc;
      if ((rc = BaGroupReduce(h, h->scal + kGradMax, 1, PP_REDUCE_MAX))) return rc;
      if ((rc = BaGroupReduce(h, h->scal + kStepNorm2, 2, PP_REDUCE_SUM))) return rc;          // kStepNorm2, kXNorm2 are adjacent
      if (fold == 1 && (rc = BaGroupReduce(h, h->scal + kCost, 1, PP_REDUCE_SUM))) return rc;
      if (fold == 2 && (rc = BaGroupReduce(h, h->scal + kCostCand, 2, PP_REDUCE_SUM))) return rc;   // kCostCand, kModelChange are adjacent
      if (with_step && (rc = BaGroupReduce(h, h->scal + kTicketSlot, 1, PP_REDUCE_MAX))) return rc;    // the failure bits: every rank sees the worst
      if ((rc = g.End())) return rc;
    }
    if (with_step) hipLaunchKernelGGL(k_scalar_to_flag, dim3(1), dim3(1), 0, h->stream, h->scal + kTicketSlot, h->d_flag);
    PP_HIP_TRY(hipGetLastError());
  }
  return PP_OK;
}

static int ReadScalars(pp_ba_impl* h) {
  PP_HIP_TRY(hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, h->stream));   // the flag rides in the last slot
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
}
// The norms kernel of a trial step writes the scalars and then a ticket into the pinned slot; the host polls the ticket.
// The poll is a busy spin only for as long as a cfg-3 sized iteration lasts (PPSFM_TICKET_SPIN_US, default 1500 us, 0 = never
// spin): with larger reduced systems (C ~ 5000: ~1 s per factorisation) a spinning caller thread per handle would burn a host
// core per GPU, so after that the thread sleeps between polls (50 us naps: < 0.1 % of such an iteration).  Bounded: after ~2 s
// without the ticket the stream is synchronised once and the ticket re-checked (a failed launch would otherwise wait forever).
static int WaitTicket(pp_ba_impl* h, unsigned long long ticket) {
  const volatile unsigned long long* t = reinterpret_cast<const volatile unsigned long long*>(h->h_scal) + kTicketSlot;
  hipError_t e = hipSuccess;
  switch (WaitHostTicket(t, ticket, h->sw.ticket_spin_us, [&] { return (e = hipStreamSynchronize(h->stream)) == hipSuccess; })) {
    case TicketWait::kArrived: return PP_OK;
    case TicketWait::kSyncFailed: SetLastError("pp_ba_solve: hipStreamSynchronize failed while waiting for the trial step's scalars: %s", hipGetErrorString(e)); break;
    case TicketWait::kNeverArrived: SetLastError("pp_ba_solve: the trial step's scalars never arrived"); break;
  }
  return PP_ERR_HIP;
}
static int32_t HostFlag(const pp_ba_impl* h) { int32_t f; std::memcpy(&f, h->h_scal + kNumScalars - 1, sizeof(f)); return f; }

// pp_ba_options::phase_timings: HIP events between the phases of an iteration.  Off by default: every record is a barrier
// packet on the stream (~5 us each, ~7 per iteration measured on MI355X).
struct PhaseTimer {
  pp_ba_impl* h; bool on; int n = 0; int phase[8];
  PhaseTimer(pp_ba_impl* hh, bool enabled) : h(hh), on(enabled) { if (on) (void)hipEventRecord(h->tev[0], h->stream); }
  void Mark(int ph) { if (on && n < 7) { phase[n] = ph; ++n; (void)hipEventRecord(h->tev[n], h->stream); } }
  void Collect() {
    if (!on) return;
    if (n > 0) (void)hipEventSynchronize(h->tev[n]);     // the host may be ahead of the last mark (it polls a ticket, not the stream)
    for (int i = 0; i < n; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, h->tev[i], h->tev[i + 1]) == hipSuccess) { h->timings_ms[phase[i]] += ms; h->timing_calls[phase[i]] += 1; }
    }
    n = 0;
  }
};

// The start of a solve at the handle's parameters: the failure bits cleared, K1 + K2 there, and the Jacobi scale, which stays what it is here for the
// whole solve (pp_ba_solve goes on with the gradient norm, pp_ba_reduced_system with one LM diagonal and one assembly).
static int EvaluateAndScale(pp_ba_impl* h, const pp_ba_options* o, bool fold, PhaseTimer& timer) {
  PP_HIP_TRY(hipMemsetAsync(h->d_flag, 0, 4 * sizeof(int32_t), h->stream));     // failure bits, the Cholesky token, the norms kernel's block counter
  if (const int rc = EvaluateAndReduce(h, fold)) return rc;
  timer.Mark(PP_BA_T_EVAL);
  if (const int rc = BaJacobiScale(h, o->jacobi_scaling)) return rc;
  return IntrScale(h, o->jacobi_scaling);
}

// How a solve enqueues its trial steps and gets their scalars: decided once, from the handle and the options, and the same for every iteration.
struct StepPlan {
  bool fold;                // the norms kernel sums the cost partials (a host-callback all-reduce needs the sums before it; RCCL reduces what the norms kernel folded)
  bool speculate;           // the accept path is enqueued before the verdict is known (see Speculation); not with a host-callback all-reduce
  bool direct;              // the norms kernel hands the scalars to the pinned host slot itself (no copy-engine hop) when nothing else touches them after it:
                            // no group all-reduce, no intrinsics norms kernel (LaunchNorms sees to the latter)
  bool fused_trial_cost;    // the cost at the trial point inside the step kernel (one launch less) whenever its partials are summed by the norms kernel anyway
  bool fused_step;          // point steps, model cost change, trial point and its cost in one pass (variable intrinsics: k_step_points<true>, the trial intrinsics applied before it)
  bool phase_timings;
};
static StepPlan MakeStepPlan(const pp_ba_impl* h, const pp_ba_options* o) {
  StepPlan p;
  p.fold = h->allreduce == nullptr;
  p.speculate = h->allreduce == nullptr;
  p.direct = p.speculate && !BaInGroup(h) && h->h_scal_dev != nullptr;
  p.fused_trial_cost = p.fold && (h->NI == 0 || h->sw.ba_fused_step) && h->sw.ba_fused_trial_cost;
  p.fused_step = p.fused_trial_cost && h->sw.ba_fused_step;
  p.phase_timings = o->phase_timings != 0;
  return p;
}

// One trial step for `radius` from the current point, straight down the stream: LM diagonal (when the point is new), reduced system, linear solve, point
// steps + model cost change + trial point in the candidate buffers, its cost, and the norms kernel that gathers the step's scalars (and hands them to
// the host under *ticket when plan.direct).  Waits for nothing and touches nothing of the current point.
static int EnqueueTrialStep(pp_ba_impl* h, const pp_ba_options* o, const StepPlan& plan, double radius, bool refresh_diagonal, PhaseTimer& timer, unsigned long long* ticket) {
  int rc;
  if (refresh_diagonal && (rc = IntrDiagonal(h, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  if ((rc = BaAssembleReducedSystem(h, radius, refresh_diagonal, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  timer.Mark(PP_BA_T_SCHUR);
  if (h->iterative) {
    int cg = 0;
    if ((rc = PcgSolve(h, radius, o->max_linear_solver_iterations, o->eta, &cg))) return rc;
    h->linear_solver_iterations += cg;
  } else {
    if ((rc = CholeskySolve(h->chol))) return rc;
    if ((rc = BaGatherStep(h))) return rc;
  }
  timer.Mark(PP_BA_T_CHOLESKY);
  if ((rc = BaLaunchStepKernels(h, plan.fused_step, plan.fused_trial_cost, /*sum_model_cost=*/!plan.fold))) return rc;
  timer.Mark(PP_BA_T_BACKSUB);
  if (!plan.fused_trial_cost && (rc = LaunchCostOnly(h, h->poses_c, h->points_c, h->NI > 0 ? h->intr_c : nullptr, plan.fold ? nullptr : h->scal + kCostCand))) return rc;
  if (h->allreduce) {      // (host callback: the two sums exist before the norms kernel here; with RCCL the norms call reduces what it folded)
    if ((rc = BaGroupReduce(h, h->scal + kCostCand, 2, PP_REDUCE_SUM))) return rc;   // kCostCand, kModelChange are adjacent
  }
  *ticket = plan.direct ? ++h->ticket_seq : 0;
  if ((rc = LaunchNorms(h, true, plan.fold ? 2 : 0, plan.direct ? h->h_scal_dev : nullptr, *ticket))) return rc;
  timer.Mark(PP_BA_T_UPDATE_COST);
  return PP_OK;
}

// Latency hiding around the verdict on a trial step.
//
// Speculative acceptance: almost every trial step is accepted, and the accept decision needs a host round trip (~30 us of idle GPU, after which the
// host has to catch up launching ~15 kernels).  So the accept path - make the candidate the current point (a swap of buffer pointers, no copies),
// evaluate + reduce there, norms - is enqueued BEFORE the host waits for the trial step's scalars, and the wait is on their ticket or on an event
// recorded right after their copy, never on the stream.  Invariant: while `speculated`, h->poses / h->points hold the CANDIDATE and the Jacobians and
// sums on the device are the candidate's; Keep or Undo ends that state, and every verdict goes through one of the two.
//
// Pending evaluation: the evaluation at an accepted point (cost, gradient max-norm) is only enqueued; its two scalars are first needed after the next
// trial step's own read-back, so an accepted iteration synchronises with the host once, not twice.  Invariant: while `pending`, `pending_slot` is the
// host slot that evaluation was enqueued into - fixed by Keep, so a later speculation, which flips `eval_slot` for ITS evaluation, cannot redirect it.
// The sequence of accepted points, costs, radii and the termination are those of the eager loop.
struct Speculation {
  pp_ba_impl* const h;
  const StepPlan plan;
  bool speculated = false, pending = false;
  int eval_slot = 0;                       // one of two host slots: the next evaluation is enqueued before the pending one is consumed
  const double* pending_slot = nullptr;

  void SwapPoints() {
    std::swap(h->poses, h->poses_c); std::swap(h->points, h->points_c);
    if (h->NI > 0) std::swap(h->intr, h->intr_c);
  }
  int EnqueueEvaluation() {      // at h->poses / h->points: K1 + K2, norms, scalars -> the free host slot
    hipStream_t s = h->stream;
    int r;
    if (plan.phase_timings) PP_HIP_TRY(hipEventRecord(h->tev_eval[0], s));
    if ((r = EvaluateAndReduce(h, plan.fold))) return r;
    if (plan.phase_timings) PP_HIP_TRY(hipEventRecord(h->tev_eval[1], s));
    eval_slot ^= 1;
    if ((r = LaunchNorms(h, false, plan.fold ? 1 : 0, plan.direct ? h->h_scal_dev + kNumScalars * (1 + eval_slot) : nullptr))) return r;
    if (!plan.direct) PP_HIP_TRY(hipMemcpyAsync(h->h_scal + kNumScalars * (1 + eval_slot), h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, s));
    return PP_OK;
  }
  // the trial step's scalars (and a pending evaluation's, enqueued before them) are in host memory when this returns; with plan.speculate the accept
  // path is on the stream by then, and the host has not waited on the stream
  int AwaitTrialStep(unsigned long long ticket) {
    if (!plan.speculate) return ReadScalars(h);
    if (!plan.direct) {
      PP_HIP_TRY(hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, h->stream));
      PP_HIP_TRY(hipEventRecord(h->ev_readback, h->stream));
    }
    SwapPoints();
    if (const int rc = EnqueueEvaluation()) return rc;
    speculated = true;
    if (plan.direct) return WaitTicket(h, ticket);
    PP_HIP_TRY(hipEventSynchronize(h->ev_readback));
    return PP_OK;
  }
  // the step was accepted: the candidate is the current point and its evaluation is pending
  int Keep() {
    if (!speculated) {
      SwapPoints();
      if (const int rc = EnqueueEvaluation()) return rc;
    }
    speculated = false;
    pending_slot = h->h_scal + kNumScalars * (1 + eval_slot);
    pending = true;
    return PP_OK;
  }
  // the step was not accepted: the old point is current again; `reevaluate` restores its Jacobians and sums, which a solve that goes on needs (the
  // result is what the policy already holds and is never consumed)
  int Undo(bool reevaluate) {
    if (!speculated) return PP_OK;
    speculated = false;
    SwapPoints();
    return reevaluate ? EnqueueEvaluation() : PP_OK;
  }
  // requires the pending evaluation to have reached its slot (a later read-back on the same stream has arrived, or the stream was synchronised)
  void Resolve(LmPolicy* policy) {
    policy->Resolve(pending_slot[kCost], pending_slot[kGradMax]);
    float ms = 0;
    if (plan.phase_timings && hipEventElapsedTime(&ms, h->tev_eval[0], h->tev_eval[1]) == hipSuccess) { h->timings_ms[PP_BA_T_EVAL] += ms; h->timing_calls[PP_BA_T_EVAL] += 1; }
    pending = false;
  }
};

// After a trial step that raised failure bits: the bits are cleared and so is what the failed run left in buffers that the assembly relies on but never
// rewrites (the zero padding of S).  Bit 4, a bounded wait of the one-launch factorisation (k_cholesky_tasks) that ran out: nothing wrong with the
// system - *retry = the handle switched to one launch per block column (it stays with them) and the same step is to be made again.  Bit 1, a
// non-positive pivot: the factorisation leaves NaN where it stopped, on which the next, more strongly damped system would fail too; also in the factor
// array.  An iterative handle has no S (its conjugate-gradient loop raises the same bit).
static int RecoverAfterFlag(pp_ba_impl* h, int32_t flag, bool* retry) {
  *retry = false;
  if (flag == 0) return PP_OK;
  hipStream_t s = h->stream;
  PP_HIP_TRY(hipMemsetAsync(h->d_flag, 0, sizeof(int32_t), s));
  *retry = (flag & 4) && CholeskyFallBackToColumns(h->chol);
  const bool failed_pivot = !*retry && (flag & 1) && !h->iterative && h->S;
  if (*retry || failed_pivot) PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, s));
  if (failed_pivot && h->Lfac) PP_HIP_TRY(hipMemsetAsync(h->Lfac, 0, sizeof(double) * (size_t)h->N * h->N, s));
  return PP_OK;
}

// ceres::IterationCallback with the policy's last row; true = the callback ended the solve (termination set).  Every row is followed by exactly one
// call, so the iteration number is the row's index.
static bool UserStops(const pp_ba_options* o, LmPolicy* policy) {
  if (!o->iteration_callback) return false;
  const double* row = policy->last_row();
  pp_ba_iteration_summary it;
  it.iteration = policy->iteration() - 1; it.step_is_successful = row[6] != 0.0;
  it.cost = row[0]; it.cost_change = row[1]; it.gradient_max_norm = row[2]; it.step_norm = row[3]; it.relative_decrease = row[4];
  it.trust_region_radius = row[5];
  const int32_t r = o->iteration_callback(o->iteration_callback_ctx, &it);
  if (r == PP_SOLVER_ABORT) policy->termination = PP_TERM_USER_FAILURE;
  if (r == PP_SOLVER_TERMINATE_SUCCESSFULLY) policy->termination = PP_TERM_USER_SUCCESS;
  return r == PP_SOLVER_ABORT || r == PP_SOLVER_TERMINATE_SUCCESSFULLY;
}

int BaEnsureSolverBuffers(pp_ba_impl* h) { return EnsureSolverBuffers(h); }
int BaAssembleUndamped(pp_ba_impl* h, const pp_ba_options* o, bool evaluate) {
  if (evaluate) {
    PhaseTimer untimed(h, false);
    if (const int rc = EvaluateAndScale(h, o, /*fold=*/true, untimed)) return rc;      // (no cost sum: nothing of the solver's scalars is touched)
  }
  PP_HIP_TRY(hipMemsetAsync(h->diag_c, 0, sizeof(double) * (size_t)h->n_red, h->stream));
  PP_HIP_TRY(hipMemsetAsync(h->diag_p, 0, sizeof(double) * 3 * (size_t)h->P, h->stream));
  return BaAssembleReducedSystem(h, HUGE_VAL);      // 1 / radius == 0.0
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

// What every rank of a point-sharded group must agree on before it exchanges anything: the layout of the reduced system (order, width, tile map) decides
// the COUNT of every all-reduce of a solve (num_nz_tiles x 4096 doubles or the packed triangle) - ranks that disagree hang in RCCL or sum mismatched tiles.
// 52 bits of an FNV-1a hash, i.e. exactly representable as the double that travels.
static double GroupStructureHash(const pp_ba_impl* h) {
  uint64_t x = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(p); for (size_t i = 0; i < n; ++i) { x ^= b[i]; x *= 1099511628211ull; } };
  const int32_t head[8] = {h->C, h->n_red, h->N, h->NI, h->structure_from_covisibility ? 1 : 0, (h->sparse_tiles && h->structure_from_covisibility) ? 1 : 0,
                           (h->sparse_tiles && h->structure_from_covisibility) ? h->num_nz_tiles : 0, h->iterative ? 1 : 0};
  mix(head, sizeof(head));
  if (h->sparse_tiles && h->structure_from_covisibility) mix(h->tile_nz.data(), h->tile_nz.size());      // (outside that case a group factorises the dense system: the map is not used)
  mix(h->pose_new_of_old.data(), h->pose_new_of_old.size() * sizeof(int32_t));
  return (double)(x >> 12);
}

// The attach calls are COLLECTIVE over the group: one MAX all-reduce of three doubles through the exchange that is about to be attached - [refusal of any
// rank, structure hash, -structure hash] - so that the ranks refuse TOGETHER (one returning an error while the others enter a collective is a hang) and a
// group whose handles lay out the reduced system differently is refused before its first exchange.  A group of one rank exchanges nothing.
static int GroupAgreeOnRefusal(pp_ba_impl* h, int* bad, int* mismatch, pp_allreduce_fn fn, void* ctx, pp_comm_handle comm, int group_size) {
  *mismatch = 0;
  if (group_size <= 1) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  const double hash = GroupStructureHash(h);
  double v[3] = {*bad ? 1.0 : 0.0, hash, -hash};
  if (!h->attach_slot) PP_TRY(h->blocks.Alloc(&h->attach_slot, 4));      // (a slot of its own: nothing of a solve lives here)
  double* slot = h->attach_slot;
  PP_HIP_TRY(hipMemcpyAsync(slot, v, sizeof(v), hipMemcpyHostToDevice, h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  int rc = PP_OK;
  if (comm) rc = pp_comm_allreduce(comm, slot, 3, PP_REDUCE_MAX);
  else if (fn) { rc = fn(ctx, slot, 3, PP_REDUCE_MAX); if (rc) { SetLastError("pp_ba_set_allreduce: the reduction callback returned %d", rc); rc = PP_ERR_HIP; } }
  if (rc) return rc;
  PP_HIP_TRY(hipMemcpy(v, slot, sizeof(v), hipMemcpyDeviceToHost));
  *bad = v[0] != 0.0 ? 1 : 0;
  *mismatch = (v[1] != -v[2]) ? 1 : 0;      // max(hash) != min(hash)
  return PP_OK;
}
#define PP_GROUP_MISMATCH_TEXT "the handles of this group do not lay out the reduced camera system alike (image count, variable intrinsics, internal image order or " \
                               "the block-sparse tile map differ between ranks - e.g. one rank was created without pp_ba_problem_desc::covisibility or with a stale one): " \
                               "every rank of a point-sharded group passes the same order and, with PP_ORDERING_AUTO, the group's union co-visibility"

int pp_ba_set_allreduce(pp_ba_handle h, pp_allreduce_fn fn, void* ctx, int32_t group_rank, int32_t group_size) try {
  PP_REQUIRE(h, "pp_ba_set_allreduce: null handle");
  PP_REQUIRE(group_size >= 1 && group_rank >= 0 && group_rank < group_size, "pp_ba_set_allreduce: bad group");
  if (fn) {
    // every rank must lay out the exchanged system alike: the caller's order, or an order taken from the co-visibility every rank was given.  The verdict is
    // exchanged before anybody refuses, so that the ranks of a group fail TOGETHER instead of one returning an error while the others enter a collective
    int bad = (!h->pose_new_of_old.empty() && !h->structure_from_covisibility) ? 1 : 0, mismatch = 0;
    const int rc = GroupAgreeOnRefusal(h, &bad, &mismatch, fn, ctx, nullptr, group_size);
    if (rc) return rc;
    PP_REQUIRE(bad || !mismatch, "pp_ba_set_allreduce: " PP_GROUP_MISMATCH_TEXT);
    PP_REQUIRE(!bad, "pp_ba_set_allreduce: a handle of this group renumbered its images from its own shard's co-visibility (pp_ba_problem_desc::ordering = AUTO "
               "without ::covisibility); the handles of a point-sharded group keep the caller's order (PP_ORDERING_NATURAL) or are all created with the group's union "
               "co-visibility, so that every rank lays out the exchanged system alike");
  }
  h->allreduce = fn; h->allreduce_ctx = ctx; h->comm = nullptr;
  h->group_rank = fn ? group_rank : 0; h->group_size = fn ? group_size : 1;
  // a host callback is where other host threads do device-wide things (allocate, synchronize) while this handle would be capturing
  // its factorisation graph, and the callback's own synchronisation per LM iteration dwarfs what the graph saves: enqueue eagerly
  if (fn) CholeskyDisableGraph(h->chol);
  return ApplyLinearSolverStructure(h);      // (a block-sparse tile map made from the shard's own observations is rank-local: not used inside a group)
} PP_API_CATCH("pp_ba_set_allreduce")

int pp_ba_set_communicator(pp_ba_handle h, pp_comm_handle comm) try {
  PP_REQUIRE(h, "pp_ba_set_communicator: null handle");
  PP_REQUIRE(!comm || comm->device == h->device, "pp_ba_set_communicator: the communicator lives on device %d, the handle on device %d", comm ? comm->device : -1, h->device);
  if (comm) {
    int bad = (!h->pose_new_of_old.empty() && !h->structure_from_covisibility) ? 1 : 0, mismatch = 0;      // (see pp_ba_set_allreduce: the ranks of a group refuse together)
    const int rc = GroupAgreeOnRefusal(h, &bad, &mismatch, nullptr, nullptr, comm, comm->size);
    if (rc) return rc;
    PP_REQUIRE(bad || !mismatch, "pp_ba_set_communicator: " PP_GROUP_MISMATCH_TEXT);
    PP_REQUIRE(!bad, "pp_ba_set_communicator: a handle of this group renumbered its images from its own shard's co-visibility (pp_ba_problem_desc::ordering = AUTO "
               "without ::covisibility); the handles of a point-sharded group keep the caller's order (PP_ORDERING_NATURAL) or are all created with the group's union "
               "co-visibility, so that every rank lays out the exchanged system alike");
  }
  h->comm = comm; h->allreduce = nullptr; h->allreduce_ctx = nullptr;
  h->group_rank = comm ? comm->rank : 0; h->group_size = comm ? comm->size : 1;
  return ApplyLinearSolverStructure(h);
} PP_API_CATCH("pp_ba_set_communicator")

int pp_ba_get_structure(pp_ba_handle h, int32_t* info) try {
  PP_REQUIRE(h && info, "pp_ba_get_structure: null argument");
  const int T = ((h->n_red + 1 + 63) / 64);
  info[0] = T * (T + 1) / 2;
  info[1] = h->nnz_tiles_natural >= 0 ? h->nnz_tiles_natural : h->num_nz_tiles;
  info[2] = h->num_nz_tiles;
  info[3] = h->pose_new_of_old.empty() ? 0 : 1;
  info[4] = BaSparseActive(h) ? 1 : 0;
  info[5] = h->iterative ? 1 : 0;
  // the chains of the one-launch factorisation (several: a nested-dissection order whose sub-trees are factorised side by side) and its chain steps
  info[6] = 1; info[7] = T;
  if (BaSparseActive(h) && UseTasks(T) && !h->tile_nz.empty()) {
    if (h->structure_steps < 0) h->structure_steps = CholeskyChainSteps(T, h->tile_nz.data(), h->sw, &h->structure_chains);      // (planned once per handle; the plan itself is cached per tile map)
    info[6] = h->structure_chains; info[7] = h->structure_steps;
  }
  return PP_OK;
} PP_API_CATCH("pp_ba_get_structure")

int pp_ba_get_intrinsics_layout(pp_ba_handle h, int32_t* info) try {
  PP_REQUIRE(h && info, "pp_ba_get_intrinsics_layout: null argument");
  info[0] = h->NI; info[1] = h->intr_private_nv; info[2] = h->intr_wide_nv; info[3] = h->jcam_stride;
  return PP_OK;
} PP_API_CATCH("pp_ba_get_intrinsics_layout")

int pp_ba_get_trace(pp_ba_handle h, double* trace, int32_t capacity_rows, int32_t* num_rows) try {
  PP_REQUIRE(h && num_rows, "pp_ba_get_trace: null argument");
  const int rows = (int)(h->trace.size() / 7);
  *num_rows = rows;
  if (trace) std::memcpy(trace, h->trace.data(), sizeof(double) * 7 * (size_t)std::min(rows, capacity_rows));
  return PP_OK;
} PP_API_CATCH("pp_ba_get_trace")

int pp_ba_get_timings(pp_ba_handle h, double* ms, int32_t* calls) try {
  PP_REQUIRE(h && ms && calls, "pp_ba_get_timings: null argument");
  for (int i = 0; i < PP_BA_T_COUNT; ++i) { ms[i] = h->timings_ms[i]; calls[i] = h->timing_calls[i]; }
  return PP_OK;
} PP_API_CATCH("pp_ba_get_timings")

int pp_ba_reduced_system(pp_ba_handle h, const pp_ba_options* o, double radius, int32_t* n_out, double* S, double* rhs, int64_t capacity) try {
  PP_REQUIRE(h && o && n_out && radius > 0, "pp_ba_reduced_system: bad argument");
  PP_REQUIRE(!h->iterative, "pp_ba_reduced_system: an iterative (ITERATIVE_SCHUR) handle never forms the reduced system - create the handle with "
             "pp_ba_problem_desc::linear_solver = PP_LINEAR_SOLVER_DIRECT (or PPSFM_BA_LINEAR_SOLVER=direct) for the direct solve");
  PP_HIP_TRY(hipSetDevice(h->device));
  int rc;
  if ((rc = BaEnsureJacobianBuffers(h, 0, h->NI > 0 ? 1 : 0))) return rc;
  if ((rc = EnsureSolverBuffers(h))) return rc;
  PhaseTimer untimed(h, false);
  if ((rc = EvaluateAndScale(h, o, false, untimed))) return rc;
  if ((rc = BaLmDiagonal(h, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  if ((rc = IntrDiagonal(h, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  if ((rc = BaAssembleReducedSystem(h, radius))) return rc;
  const int n = h->n_red;
  *n_out = n;
  if (S) {
    PP_REQUIRE(capacity >= (int64_t)n * n, "pp_ba_reduced_system: capacity %lld < %lld", (long long)capacity, (long long)n * n);
    std::vector<double> full((size_t)h->N * h->N);
    PP_HIP_TRY(hipMemcpyAsync(full.data(), h->S, sizeof(double) * full.size(), hipMemcpyDeviceToHost, h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
    // (the caller's image order: column c of the output sits at internal position at(c) when pp_ba_create renumbered the images)
    // and the position of a vector column in S: pp_ba_impl::spos)
    const bool perm = !h->pose_new_of_old.empty();
    auto at = [&](int c) { const int v = (perm && c < 6 * h->C) ? 6 * h->pose_new_of_old[c / 6] + c % 6 : c; return h->spos_host.empty() ? v : h->spos_host[v]; };
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const int a = at(i), b = at(j);
        S[(size_t)i * n + j] = (b <= a) ? full[(size_t)a * h->N + b] : full[(size_t)b * h->N + a];
      }
    if (rhs) for (int j = 0; j < n; ++j) rhs[j] = full[(size_t)n * h->N + at(j)];
  }
  return PP_OK;
} PP_API_CATCH("pp_ba_reduced_system")

int pp_ba_solve(pp_ba_handle h, const pp_ba_options* o, pp_ba_summary* sum) try {
  PP_REQUIRE(h && o && sum, "pp_ba_solve: null argument");
  PP_REQUIRE(o->max_num_iterations >= 0 && o->initial_trust_region_radius > 0, "pp_ba_solve: bad options");
  PP_HIP_TRY(hipSetDevice(h->device));
  const auto t_start = std::chrono::steady_clock::now();
  std::memset(sum, 0, sizeof(*sum));
  int rc;
  if ((rc = BaEnsureJacobianBuffers(h, 0, h->NI > 0 ? 1 : 0))) return rc;
  if ((rc = EnsureSolverBuffers(h))) return rc;
  hipStream_t s = h->stream;
  h->trace.clear();
  h->linear_solver_iterations = 0;
  for (int i = 0; i < PP_BA_T_COUNT; ++i) { h->timings_ms[i] = 0; h->timing_calls[i] = 0; }
  PP_HIP_TRY(hipMemsetAsync(h->step_c, 0, sizeof(double) * h->N, s));
  PP_HIP_TRY(hipEventRecord(h->ev0, s));
  const StepPlan plan = MakeStepPlan(h, o);

  // iteration 0: evaluate, Jacobi scale, gradient norm
  {
    PhaseTimer timer(h, plan.phase_timings);
    if ((rc = EvaluateAndScale(h, o, plan.fold, timer))) return rc;
    if (!BaInGroup(h) && h->h_scal_dev != nullptr) {      // the scalars reach the host without the copy engine when nothing else touches them after the norms kernel
      const unsigned long long ticket = ++h->ticket_seq;
      if ((rc = LaunchNorms(h, false, plan.fold ? 1 : 0, h->h_scal_dev, ticket))) return rc;
      if ((rc = WaitTicket(h, ticket))) return rc;
    } else {
      if ((rc = LaunchNorms(h, false, plan.fold ? 1 : 0))) return rc;
      if ((rc = ReadScalars(h))) return rc;
    }
    timer.Collect();
  }
  LmPolicy policy(*o, h->trace);
  Speculation spec{h, plan};
  bool go_on = policy.Start(h->h_scal[kCost], h->h_scal[kGradMax]);
  sum->initial_cost = policy.cost;
  sum->num_residuals = (int32_t)(2 * h->M);
  if (!go_on) SetLastError("pp_ba_solve: initial cost is not finite");
  else go_on = !UserStops(o, &policy);

  while (go_on) {
    LmNext next = policy.BeforeStep(spec.pending);
    if (next == LmNext::kResolveFirst) {
      PP_HIP_TRY(hipStreamSynchronize(s));
      spec.Resolve(&policy);
      next = policy.BeforeStep(false);
    }
    if (next == LmNext::kStop) break;

    PhaseTimer timer(h, plan.phase_timings);
    unsigned long long ticket = 0;
    if ((rc = EnqueueTrialStep(h, o, plan, policy.radius, !policy.reuse_diagonal, timer, &ticket))) return rc;
    if ((rc = spec.AwaitTrialStep(ticket))) return rc;
    timer.Collect();
    if (spec.pending) {      // the previous accepted step's evaluation came with this read-back
      spec.Resolve(&policy);
      if (policy.GradientToleranceReached()) {      // drops the trial step that was computed ahead of this test
        if ((rc = spec.Undo(false))) return rc;
        break;
      }
    }
    LmTrialStep step = {h->h_scal[kModelChange], h->h_scal[kCostCand], h->h_scal[kStepNorm2], h->h_scal[kXNorm2], HostFlag(h), false};
    if ((rc = RecoverAfterFlag(h, step.flag, &step.retry_after_timeout))) return rc;
    const LmVerdict verdict = policy.Judge(step);
    // the one place that leaves the speculated state: the candidate stays the current point, or the old point is current again - evaluated again
    // (its Jacobians and sums) exactly when the solve goes on from it
    if ((rc = verdict == LmVerdict::kAccepted ? spec.Keep() : spec.Undo(LmStaysAtOldPoint(verdict)))) return rc;
    switch (verdict) {
      case LmVerdict::kInvalidFailed:
        SetLastError("pp_ba_solve: %d consecutive invalid steps (linear system not positive definite or step without model decrease)", policy.invalid);
        [[fallthrough]];
      case LmVerdict::kParameterTolerance:
      case LmVerdict::kFunctionTolerance:
        go_on = false;
        break;
      case LmVerdict::kRetryAfterTimeout:      // the same step again: no iteration, no row, no callback
        break;
      case LmVerdict::kAccepted:
        if (o->iteration_callback) {     // the callback sees the cost / gradient norm AT the accepted point: wait for its evaluation
          PP_HIP_TRY(hipStreamSynchronize(s));
          spec.Resolve(&policy);
        }
        [[fallthrough]];
      case LmVerdict::kInvalid:
      case LmVerdict::kRejected:
        go_on = !UserStops(o, &policy);
        break;
    }
  }
  PP_HIP_TRY(hipEventRecord(h->ev1, s));
  PP_HIP_TRY(hipEventSynchronize(h->ev1));
  if (spec.pending) spec.Resolve(&policy);
  float ms = 0;
  PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  sum->termination = policy.termination;
  sum->final_cost = policy.cost;
  sum->num_successful_steps = policy.num_successful_steps;
  sum->num_unsuccessful_steps = policy.num_unsuccessful_steps;
  sum->num_iterations = sum->num_successful_steps + sum->num_unsuccessful_steps;
  sum->device_time_s = ms * 1e-3;
  sum->total_time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  sum->num_effective_parameters = h->num_effective_pose_point + h->NI;
  sum->linear_solver_iterations = h->linear_solver_iterations;
  sum->linear_solver = h->iterative ? PP_LINSOLVE_PCG : CholeskyLinsolve(h->chol);
  sum->cholesky_fallbacks = CholeskyFallbacks(h->chol);
  return sum->termination == PP_TERM_FAILURE ? PP_ERR_NUMERIC : PP_OK;
} PP_API_CATCH("pp_ba_solve")

}  // extern "C"
