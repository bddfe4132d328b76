// The PPSFM_* environment switches: one snapshot, read where a handle (or a stand-alone entry point) starts, and handed down from there.
// ReadSwitches (switches.hip) is the only place in the library that reads the environment; nothing reads it again at solve time, so changing a
// variable affects the handles created after the change and no existing one.
//
// Every switch, with its values, its default, the code that reads it and its kind - fallback: an escape hatch off a default path;
// A/B: a test comparison of two paths the code also picks between by itself; debug: stderr output only.  "atoi": any value, parsed by atoi
// (so "off" is 0); "letter": only the first character of the value counts; unset or any other value is the default.
//
//   name                        values                       default          read by                                      kind
//   PPSFM_CHOL_MODE             letter c|0 columns           by size          CholeskyCreate (per-column launches only)    fallback
//   PPSFM_CHOL_GRAPH            atoi, 0 = off                on               CholeskyCreate (graph capture)               fallback
//   PPSFM_CHOL_SMALL            atoi, 0 = off                on               ChoosePath (one-workgroup <= 128 cols)       fallback
//   PPSFM_CHOL_SPARSE           atoi, 0 = off                on               pp_dense_cholesky_solve (skip zero tiles)     A/B
//   PPSFM_CHOL_CHAINS           atoi, clamped to [1, 16]     by structure     PlanChains (chol_plan.hpp: max chains)       A/B
//   PPSFM_CHOL_WHOLE_FROM       atoi                         WholeFrom(T)     TaskListBuilder (chol_plan.hpp)              A/B
//   PPSFM_CHOL_TWO_PANELS       atoi, 0 = off                on               TaskListBuilder (two panels per dense task)  A/B
//   PPSFM_CHOL_SLOPE            atof                         kUpdateSlope     TaskListBuilder (deferral of far updates)    A/B
//   PPSFM_CHOL_TEST_DROP_TASKS  atoi, non-0 = on             off              EnqueueCholesky (half the list: a timeout)    A/B
//   PPSFM_BACKSUB_PAIRS         atoi, 0 = off                on               LaunchBacksub (paired dense back subst.)     A/B
//   PPSFM_CHOL_DEBUG            set = on                     off              EnsureTaskList (the chains of a list)         debug
//   PPSFM_CHOL_DEBUG_SLOW       set = on                     off              pp_dense_cholesky_solve (solves > 5 ms)       debug
//   PPSFM_CHOL_PLAN_PRINT       set = on                     off              PrintPlan (chains, closed tile map)           debug
//   PPSFM_BA_LINEAR_SOLVER      letter i|I iterative,        descriptor's     WillIterate (pp_ba_create, SetupOf)           A/B
//                               d|D direct
//   PPSFM_BA_SPARSE             atoi, 0 = off                on               BuildTileMap, SetupOf (block-sparse system)   A/B
//   PPSFM_BA_ORDERING           letter n natural, r rcm,     by chain steps   SetupOf, ChooseImageOrdering                 A/B
//                               b band (any case)
//   PPSFM_BA_GRAPH_ND           atoi, 0 never / else always  by band cuts     DissectionCandidates (image_ordering.hpp)    A/B
//   PPSFM_BA_INTR_LAYOUT        letter t|T tail              beside the pose  PrivateIntrinsicsColumns                     A/B
//   PPSFM_BA_INTR_WIDE          atoi, 0 = off                on               ApplyImageOrder (k_schur_wide_* blocks)       A/B
//   PPSFM_BA_PAIR_LISTS         letter h|H host, d|D device  by size          PairListsOnDeviceEligible                    A/B
//   PPSFM_BA_CHUNKED_PAIRS      atoi, 0 = off                on               ChunkPairLists (ba_structure.hpp)             A/B
//   PPSFM_BA_CHUNK_XCD          atoi, 0 = off                on               ChunkPairLists (XCD run order of chunks)      A/B
//   PPSFM_BA_FUSED_STEP         atoi, 0 = off                on               the LM loop (k_step_points)                  A/B
//   PPSFM_BA_FUSED_TRIAL_COST   atoi, 0 = off                on               the LM loop (cost inside k_model_cost_apply)  A/B
//   PPSFM_PCG_FUSED             atoi, 0 = off                on               PcgSolve (three-launch iteration)            A/B
//   PPSFM_TICKET_SPIN_US        atol, microseconds           1500             WaitTicket, WaitPcgTicket (host_ticket.hpp)  fallback
//   PPSFM_PCG_LOG               set = on                     off              PcgFinishCount (CG iterations per solve)     debug
//   PPSFM_ORDER_DEBUG           set = on                     off              ChooseImageOrdering (laps, candidates)       debug
//   PPSFM_CREATE_DEBUG          set = on                     off              pp_ba_create (host time per phase)           debug
//   PPSFM_POOL_MAX_MB           atol, <= 0 = no pool         1024             the resource pool (read once per process)    fallback
//   PPSFM_POOL_POISON           atoi, non-0 = on             off              the resource pool (0xFF-filled blocks)        debug
#pragma once
#include <optional>

namespace ppsfm {

enum class LinearSolverSwitch { Descriptor, Direct, Iterative };
enum class OrderingSwitch { ByChainSteps, Natural, Rcm, Band };
enum class PairListsSwitch { BySize, Host, Device };
enum class IntrLayout { Beside, Tail };

// What the Cholesky planner (PlanChains, BuildTaskList) reads: the plan cache's key beside the tile map, so a planner switch cannot be read
// without being part of the key.
struct PlanSwitches {
  std::optional<int> chains, whole_from;
  bool two_panels = true;
  std::optional<double> slope;
  bool operator==(const PlanSwitches& o) const { return chains == o.chains && whole_from == o.whole_from && two_panels == o.two_panels && slope == o.slope; }
};

struct Switches {
  bool chol_columns = false;      // per-column launches only (otherwise by size: the one-launch factorisation up to 128 block columns)
  bool chol_graph = true, chol_small = true, chol_sparse = true, chol_test_drop_tasks = false, backsub_pairs = true;
  PlanSwitches plan;
  bool chol_debug = false, chol_debug_slow = false, chol_plan_print = false;
  LinearSolverSwitch ba_linear_solver = LinearSolverSwitch::Descriptor;
  bool ba_sparse = true;
  OrderingSwitch ba_ordering = OrderingSwitch::ByChainSteps;
  int ba_graph_nd = -1;      // -1: by the band's cuts, 0: never, 1: always
  IntrLayout ba_intr_layout = IntrLayout::Beside;
  bool ba_intr_wide = true;
  PairListsSwitch ba_pair_lists = PairListsSwitch::BySize;
  bool ba_chunked_pairs = true, ba_chunk_xcd = true, ba_fused_step = true, ba_fused_trial_cost = true, pcg_fused = true;
  long ticket_spin_us = 1500;
  bool pcg_log = false, order_debug = false, create_debug = false;
  long pool_max_mb = 1024;
  bool pool_poison = false;
};

Switches ReadSwitches();

}  // namespace ppsfm
