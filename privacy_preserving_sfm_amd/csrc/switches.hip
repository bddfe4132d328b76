// ReadSwitches: the one reader of the PPSFM_* environment switches (the table: switches.hpp).
#include <cstdlib>

#include "switches.hpp"

namespace ppsfm {

namespace {
// a numeric switch: `unset` when the variable is not set, atoi / atol of its value otherwise
int Int(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}
long Long(const char* name, long unset) {
  const char* e = std::getenv(name);
  return e ? std::atol(e) : unset;
}
bool Set(const char* name) { return std::getenv(name) != nullptr; }
// a word switch, matched on its first letter: the value starts with `a` or `b`
bool Starts(const char* name, char a, char b) {
  const char* e = std::getenv(name);
  return e && (e[0] == a || e[0] == b);
}
}  // namespace

Switches ReadSwitches() {
  Switches s;
  s.chol_columns = Starts("PPSFM_CHOL_MODE", 'c', '0');
  s.chol_graph = Int("PPSFM_CHOL_GRAPH", 1) != 0;
  s.chol_small = Int("PPSFM_CHOL_SMALL", 1) != 0;
  s.chol_sparse = Int("PPSFM_CHOL_SPARSE", 1) != 0;
  s.chol_test_drop_tasks = Int("PPSFM_CHOL_TEST_DROP_TASKS", 0) != 0;
  s.backsub_pairs = Int("PPSFM_BACKSUB_PAIRS", 1) != 0;
  if (Set("PPSFM_CHOL_CHAINS")) s.plan.chains = Int("PPSFM_CHOL_CHAINS", 0);
  if (Set("PPSFM_CHOL_WHOLE_FROM")) s.plan.whole_from = Int("PPSFM_CHOL_WHOLE_FROM", 0);
  s.plan.two_panels = Int("PPSFM_CHOL_TWO_PANELS", 1) != 0;
  if (const char* e = std::getenv("PPSFM_CHOL_SLOPE")) s.plan.slope = std::atof(e);
  s.chol_debug = Set("PPSFM_CHOL_DEBUG");
  s.chol_debug_slow = Set("PPSFM_CHOL_DEBUG_SLOW");
  s.chol_plan_print = Set("PPSFM_CHOL_PLAN_PRINT");
  s.ba_linear_solver = Starts("PPSFM_BA_LINEAR_SOLVER", 'i', 'I') ? LinearSolverSwitch::Iterative
                     : (Starts("PPSFM_BA_LINEAR_SOLVER", 'd', 'D') ? LinearSolverSwitch::Direct : LinearSolverSwitch::Descriptor);
  s.ba_sparse = Int("PPSFM_BA_SPARSE", 1) != 0;
  s.ba_ordering = Starts("PPSFM_BA_ORDERING", 'n', 'N') ? OrderingSwitch::Natural
                : Starts("PPSFM_BA_ORDERING", 'r', 'R') ? OrderingSwitch::Rcm
                : Starts("PPSFM_BA_ORDERING", 'b', 'B') ? OrderingSwitch::Band : OrderingSwitch::ByChainSteps;
  if (Set("PPSFM_BA_GRAPH_ND")) s.ba_graph_nd = Int("PPSFM_BA_GRAPH_ND", 0) != 0 ? 1 : 0;
  s.ba_intr_layout = Starts("PPSFM_BA_INTR_LAYOUT", 't', 'T') ? IntrLayout::Tail : IntrLayout::Beside;
  s.ba_intr_wide = Int("PPSFM_BA_INTR_WIDE", 1) != 0;
  s.ba_pair_lists = Starts("PPSFM_BA_PAIR_LISTS", 'h', 'H') ? PairListsSwitch::Host
                  : (Starts("PPSFM_BA_PAIR_LISTS", 'd', 'D') ? PairListsSwitch::Device : PairListsSwitch::BySize);
  s.ba_chunked_pairs = Int("PPSFM_BA_CHUNKED_PAIRS", 1) != 0;
  s.ba_chunk_xcd = Int("PPSFM_BA_CHUNK_XCD", 1) != 0;
  s.ba_fused_step = Int("PPSFM_BA_FUSED_STEP", 1) != 0;
  s.ba_fused_trial_cost = Int("PPSFM_BA_FUSED_TRIAL_COST", 1) != 0;
  s.pcg_fused = Int("PPSFM_PCG_FUSED", 1) != 0;
  s.ticket_spin_us = Long("PPSFM_TICKET_SPIN_US", 1500);
  s.pcg_log = Set("PPSFM_PCG_LOG");
  s.order_debug = Set("PPSFM_ORDER_DEBUG");
  s.create_debug = Set("PPSFM_CREATE_DEBUG");
  s.pool_max_mb = Long("PPSFM_POOL_MAX_MB", 1024);
  s.pool_poison = Int("PPSFM_POOL_POISON", 0) != 0;
  return s;
}

}  // namespace ppsfm
