// The task planner of the one-launch Cholesky factorisation (chol_tasks.hpp: k_cholesky_tasks), host only and free of any device API: the vocabulary the
// kernel shares with it (chain ranges, the counter layout, ChainTask and the accessors of its packed fields), the layout of the workspace every launch
// path takes its pointers from (CholWorkspace), the chains of a tile map (PlanChains), the
// priority-sorted task list of a plan (BuildTaskList), the host replay that decides whether a list may be launched at all (TaskListWaitsAreMet) and the
// per-column row / super-tile lists of the block-sparse per-column launches (BuildSparseColumnLists).
// Includes the standard library and switches.hpp only: g++ -std=c++17 compiles it on its own, and tests/chol_plan_host_driver.cpp runs it under
// ASan/UBSan with no device and no library.  What stays in cholesky.hip: the process-wide plan cache, the uploads, every launch, the entry points.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "switches.hpp"

#ifdef __HIPCC__
#define PP_PLAN_HD __host__ __device__ __forceinline__
#else
#define PP_PLAN_HD inline
#endif

namespace ppsfm {

// SEVERAL CHAINS (a block-sparse system whose elimination tree has independent sub-trees - a nested-dissection order of the cameras: the leaves are
// factorised side by side, the separators last).  A chain is a run of consecutive block columns [begin, end) whose tiles (k+1,k) / (k+2,k) exist; it
// STARTS at a block column whose rows k, k+1, k+2 have nothing left of column k (no panel ever touches the three tiles of its first step: k_potrf64
// factorises every chain's first diagonal block) and a chain that is followed by another one STOPS after the step that produces M_(end-1): its last
// block column is solved by solve tasks alone (rows >= end + 3: the separators), and `post` is what it stores into sol[end - 1] when the solved tile
// (end-1,end-2) is in L.  Workgroup c of k_cholesky_tasks runs chain c; the task list follows.
constexpr int kMaxChains = 16;
struct ChainRanges { int32_t n; int32_t begin[kMaxChains]; int32_t end[kMaxChains]; int32_t post[kMaxChains]; };
inline ChainRanges OneChain(int T) { ChainRanges cr; std::memset(&cr, 0, sizeof(cr)); cr.n = 1; cr.end[0] = T; return cr; }

// lower-triangular tile index t -> (row, col), row >= col
PP_PLAN_HD void TriIndex(int t, int* row, int* col) {
  int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  *row = r; *col = t - r * (r + 1) / 2;
}

constexpr int BacksubNumPairs(int T) { return T >= 7 ? (T - 3) / 2 : 0; }      // blocks 0 .. 2 npairs - 1 in pairs, the 3 or 4 above singly

constexpr int kMaxSteps = 128;       // block columns the counter arrays hold (N <= 8192)
constexpr int kMaxSuper = kMaxSteps / 2 + 1;
// The sizes of the one-launch path, dense or block-sparse: up to kMaxSteps block columns, the whole range of its counter arrays (round 2 stopped at 88 - equal
// at n = 6000, slower at 8000; with the two-panel updates of round 3: n = 3000 0.68 against 0.83 ms, 4000 1.08 / 1.36, 6000 2.57 / 3.00, 8000 5.53 / 5.96 -
// tools/chol_time.py)
constexpr bool UseTasks(int T) { return T >= 4 && T <= kMaxSteps; }
constexpr int kScratchCounters = 2048;      // counters of the per-chain accumulation sequences (several chains, see ChainRanges), handed out by the host
enum { cSol0 = 8, cVer0 = cSol0 + kMaxChains * kMaxSteps, cSub0 = cVer0 + kMaxSuper * kMaxSuper, cScratch0 = cSub0 + kMaxSuper * kMaxSuper,
       kNumCounters = cScratch0 + kScratchCounters };      // sol: one set of row counters per chain (cSol0 + chain x kMaxSteps + row)

// The workspace `Linv_ws` of one factorisation of T block columns: where each part starts, in doubles, and the total - the one place that knows.
//   Minv[T]     the 64 x 64 row-major inverses L_kk^-1 = the M_k mailboxes of task mode (solves, back substitution, CholeskyFactor)
//   xs[T+1]     the chain's X tile per step (per-column mode uses slots k & 1 in turn; task mode: one mailbox per step)
//   ds[T+1], xsol[T+1]   the D and solved-X mailboxes of task mode
//   counters    kNumCounters int32 (the progress counters of task mode) in kCounterDoubles doubles
//   Pw[npairs], Zw[4 npairs]   pair inverses and pair couplings of the paired back substitution, npairs = BacksubNumPairs(T) <= T / 2 + 1 (what is reserved)
// The MailDoubles() in front of the counters are the mailbox slots: what k_potrf64 presets to the "not ready" pattern.
struct CholWorkspace {
  static constexpr size_t kTile = 64 * 64, kCounterDoubles = 8192;
  size_t Minv, xs, ds, xsol, counters, Pw, Zw, total;
  constexpr explicit CholWorkspace(int T)
      : Minv(0), xs(Minv + (size_t)T * kTile), ds(xs + (size_t)(T + 1) * kTile), xsol(ds + (size_t)(T + 1) * kTile), counters(xsol + (size_t)(T + 1) * kTile),
        Pw(counters + kCounterDoubles), Zw(Pw + (size_t)BacksubNumPairs(T) * kTile), total(Pw + (size_t)(T / 2 + 1) * 5 * kTile) {}
  constexpr size_t MailDoubles() const { return counters; }
};
static_assert(kNumCounters * sizeof(int32_t) <= CholWorkspace::kCounterDoubles * sizeof(double), "the counters exceed their part of the workspace");
static_assert(CholWorkspace(kMaxSteps).Zw + 4 * (size_t)BacksubNumPairs(kMaxSteps) * CholWorkspace::kTile <= CholWorkspace(kMaxSteps).total, "the pairs exceed theirs");
enum { kTaskPrepX = 1, kTaskPrepD = 2, kTaskSolve = 3, kTaskUpdate = 4, kTaskPairPrep = 5, kTaskMerge = 6 };      // pair prep: a = pair, b = part (paired back substitution)
// solve: a = block row; update: a = I, b = J | part << 8 | parts << 12 | target << 16: a PART of super-tile (I,J) - parts = 2: block row
// 2I + part (both block columns); parts = 4: the one 64x64 tile (2I + part / 2, 2J + part % 2).  The part that brings the
// super-tile's sub-counter to `target` (the parts listed for it so far) moves its ver counter.
// w0, w1: the values the task's ver counters must have reached (the panels an EXISTING earlier task applies; in a dense system k - 1).  In a
// block-sparse system a panel only touches the super-tiles whose tiles it couples, so "every panel below k" becomes "the last panel below k that has
// an update task for this super-tile" - which only the host, who lists the tasks, knows.
// w2: the value the row counter sol[] of the row the task SOLVES a tile of must have reached - the row's previous structurally non-zero column, solved:
// the solves of a row stay in column order (a counter value then says "every non-zero column below it is solved"), whichever columns exist.
// Values a task STORES into a counter come from the host as well (they were k / k + 1 while the block columns were eliminated in index order):
//   PrepX / PrepD  a = the value "column k-1 of a row is solved" (0 for the first step of a chain), b = "column k is solved"
//   solve          w1 = "column k is solved" (stored into sol[i])
//   update         w1 = the value the super-tile's ver counter takes once every part of this panel is applied, w2 = "column k-1 is solved"
// flags: bit 0 = k is the FIRST block column of a chain (nothing pending from a column k-1; M_k is k_potrf64's); bits 4..7 = the chain whose row counters the
// task waits for / moves (the chain of block column k; of column k-1 for an update)
// update / merge tasks: cidx / sidx = the ver / sub counter of the sequence the task belongs to (absolute index), zsel = -1: the tiles of S themselves, >= 0:
// the chain whose scratch tiles the task accumulates into (update) or adds to S (merge: cidx = the super-tile's own ver counter, sidx = the scratch sequence's, w2 = the
// value that one must have reached), mask = bits 0..3: tiles of the super-tile nothing has been accumulated into yet (update: taken as zero instead of read;
// merge: the tiles to add)
// slot[q]: where tile q (2 x row + column) of the super-tile lives in the scratch pool (64 x 64 doubles per slot, row stride 64) when zsel >= 0
struct ChainTask { int32_t type, k, a, b, w0, w1, w2, flags, cidx, sidx, zsel, mask, slot[4]; };
// the packed fields b (update / merge tasks) and flags: nothing outside this header shifts or masks them by hand
constexpr int TaskSuperColumn(int32_t b) { return b & 255; }      // J
constexpr int TaskPart(int32_t b) { return (b >> 8) & 15; }
constexpr int TaskParts(int32_t b) { return (b >> 12) & 15; }
constexpr int TaskTarget(int32_t b) { return b >> 16; }
constexpr bool TaskFirstOfChain(int32_t flags) { return (flags & 1) != 0; }
constexpr int TaskChain(int32_t flags) { return (flags >> 4) & 15; }
constexpr int32_t PackUpdate(int J, int part, int parts, int target) { return J | (part << 8) | (parts << 12) | (target << 16); }
constexpr int32_t PackFlags(bool first, int chain) { return (first ? 1 : 0) | (chain << 4); }
constexpr int kPartsTwoPanels = 8;      // `parts` of an update task that applies panels k-1 and k to its whole super-tile (far from the front)
// Super-tile columns this far right of the front are updated whole, nearer ones in two halves.  Halves keep the per-super-tile
// sequence of updates shorter than a step of the chain (they cannot fall behind), whole super-tiles move the least operand bytes
// per flop: the smaller the matrix, the more the chain bounds the time and the further out halves pay.  Measured optimum
// (tools/chol_time.py with PPSFM_CHOL_WHOLE_FROM), round 2, priority slope 0.5: 12 at 47 block columns (0.73 against 0.77 ms with 6), 9 at 63,
// 6 at 79, 3 at 94.  Round 3 (tools/sched_sweep.sh, the knobs swept on one box): what the chain still waited for in steps 8-18 of a
// 47-column factorisation (~45 us in all) was the BULK - every CU busy with updates, the front updates of the step dispatched late - and
// not the position of PrepX / PrepD in the list (moving them one or two steps ahead changed nothing); and the bulk of the early steps is
// bound by its TRAFFIC (~800 tiles per step x ~100 KB per tile and panel = 6 TB/s).  So: (a) a flatter priority (far updates deferred
// by 0.3 instead of 0.5 steps per super-column: less of the far work piles up behind the front later on; steeper ones are much worse -
// 0.75: 804 us, 1.0: 887 us at 47 columns) with whole super-tiles five columns nearer: 743 -> 728 us (factorisation + back
// substitution in the tool); (b) far super-tiles take TWO panels per task (UpdateSuperTile<true>: C read and written once per two
// steps, the second panel's operands in flight under the first panel's products), and with that "far" starts three super-columns from
// the front: 47 columns 728 -> 706 us, 63: 1262 -> 1120, 79: 2135 -> 1765 (whole_from 2), 16 - 32 columns unchanged.
constexpr double kUpdateSlope = 0.3;
inline int WholeFrom(int T) { return T >= 56 ? 2 : 3; }

// the three tiles the chain / the prep tasks of step k update themselves
constexpr bool StepOwnsTile(int k, int r, int c) { return (r == k + 1 && c == k + 1) || (r == k + 2 && (c == k + 1 || c == k + 2)); }

// Symbolic Cholesky on the tile graph: eliminating block column k couples every pair of rows that have a non-zero tile in it.
inline int CloseTileMap(int T, uint8_t* nz) {
  for (int i = 0; i < T; ++i) nz[(size_t)i * T + i] = 1;
  std::vector<int> rows;
  for (int k = 0; k < T; ++k) {
    rows.clear();
    for (int i = k + 1; i < T; ++i) if (nz[(size_t)i * T + k]) rows.push_back(i);
    for (size_t a = 0; a < rows.size(); ++a)
      for (size_t b = 0; b <= a; ++b) nz[(size_t)rows[a] * T + rows[b]] = 1;
  }
  int count = 0;
  for (int i = 0; i < T; ++i) for (int j = 0; j <= i; ++j) count += nz[(size_t)i * T + j] ? 1 : 0;
  return count;
}

// Block-sparse structure: tile_nz (T x T, lower triangle, row-major; the caller has already closed it under the fill-in of
// the factorisation) -> per launch k the rows of the solve workgroups and the super-tiles of the update workgroups.
// Layout of `lists`: [T+1 offsets of the row lists | T+1 offsets of the super-tile lists | the lists]; base_rows / base_sups: where the rows / the
// super-tiles start.
struct SparseColumnLists { std::vector<int32_t> lists; int base_rows = 0, base_sups = 0; };
inline SparseColumnLists BuildSparseColumnLists(int T, const uint8_t* nz) {
  auto has = [&](int i, int j) { return i < T && j < T && nz[(size_t)i * T + j] != 0; };
  std::vector<int32_t> rows, sups, row_off(T + 1, 0), sup_off(T + 1, 0);
  for (int k = 0; k + 1 < T; ++k) {
    row_off[k] = (int32_t)rows.size(); sup_off[k] = (int32_t)sups.size();
    for (int i = k + 3; i < T; ++i) if (has(i, k)) rows.push_back(i);
    if (k >= 1) {
      const int kp = k - 1, k1 = kp + 2, nb = T - k1, ns = (nb + 1) / 2, nsup = ns * (ns + 1) / 2 - 1;
      for (int u = 0; u < nsup; ++u) {
        int I, J;
        TriIndex(u + 1, &I, &J);
        bool any = false;
        for (int q = 0; q < 4; ++q) {
          const int bi = k1 + 2 * I + (q >> 1), bj = k1 + 2 * J + (q & 1);
          any = any || (bi < T && bj < T && bi >= bj && has(bi, kp) && has(bj, kp));
        }
        if (any) sups.push_back(u);
      }
    }
  }
  for (int k = T - 1; k <= T; ++k) { row_off[k] = (int32_t)rows.size(); sup_off[k] = (int32_t)sups.size(); }
  SparseColumnLists out;
  out.lists.insert(out.lists.end(), row_off.begin(), row_off.end());
  out.lists.insert(out.lists.end(), sup_off.begin(), sup_off.end());
  out.base_rows = (int)out.lists.size();
  out.lists.insert(out.lists.end(), rows.begin(), rows.end());
  out.base_sups = (int)out.lists.size();
  out.lists.insert(out.lists.end(), sups.begin(), sups.end());
  return out;
}

// The chains of a tile map (see ChainRanges), the map the one-launch mode works with, and the ORDER in which its block columns are eliminated:
//   map      the caller's (already closed under fill-in) plus, inside every chain, the two sub-diagonals - the tiles the chain and the prep tasks own at
//            every step whether anything couples them or not - closed under fill-in again (a no-op for a band of at least two tiles)
//   time[k]  length of the longest dependency path below block column k (k for one chain): columns of different chains with the same time are
//            eliminated side by side
//   rho1[k]  1 + the rank of k in the order (time, k): the value that says "column k is done" in a counter.  Every counter is moved by tasks that wait
//            for each other in this order, so "counter >= rho1[k]" means k's contribution and every earlier one are in (k + 1 for one chain).
struct ChainPlan {
  ChainRanges cr;
  std::vector<uint8_t> map;      // empty: dense
  std::vector<int> time, rho1, chain_of;
  const uint8_t* Map() const { return map.empty() ? nullptr : map.data(); }
  int Steps() const {      // the block columns on the longest dependency path
    int steps = 0;
    for (int t : time) steps = std::max(steps, t + 1);
    return steps;
  }
};
inline ChainPlan PlanChains(int T, const uint8_t* nz, const PlanSwitches& ps, int max_chains = kMaxChains) {
  ChainPlan p;
  std::memset(&p.cr, 0, sizeof(p.cr));
  std::vector<int> starts{0};
  if (ps.chains) max_chains = std::max(1, std::min(kMaxChains, *ps.chains));
  if (nz) {
    for (int k = 3; k + 4 <= T && (int)starts.size() < max_chains; ++k) {
      if (k - starts.back() < 3) continue;
      bool empty = true;
      for (int r = k; r <= k + 2 && empty; ++r)
        for (int c = 0; c < k && empty; ++c) empty = nz[(size_t)r * T + c] == 0;
      if (empty) starts.push_back(k);
    }
  }
  p.cr.n = (int)starts.size();
  p.chain_of.assign(T, 0);
  for (int c = 0; c < p.cr.n; ++c) {
    p.cr.begin[c] = starts[c]; p.cr.end[c] = c + 1 < p.cr.n ? starts[c + 1] : T;
    for (int k = p.cr.begin[c]; k < p.cr.end[c]; ++k) p.chain_of[k] = c;
  }
  if (nz) {
    p.map.assign(nz, nz + (size_t)T * T);
    for (int c = 0; c < p.cr.n; ++c)
      for (int k = p.cr.begin[c]; k < p.cr.end[c]; ++k)
        for (int i = k; i < p.cr.end[c] && i <= k + 2; ++i) p.map[(size_t)i * T + k] = 1;
    (void)CloseTileMap(T, p.map.data());
  }
  p.time.assign(T, 0);
  for (int k = 0; k < T; ++k) {
    // (the panels of ANOTHER chain reach the tiles of this column's tasks - rows k .. k+2: PrepX / PrepD(k) finish tiles of row k+2 - when that chain is
    // through: its merge tasks are listed a step behind the solves of its last block column, and they must be listed before this column's tasks)
    int t = 0;
    const int ck = p.chain_of[k];
    for (int j = 0; j < k; ++j) {
      if (!nz) { t = std::max(t, p.time[j] + 1); continue; }
      if (p.chain_of[j] == ck) { if (p.map[(size_t)k * T + j]) t = std::max(t, p.time[j] + 1); continue; }
      for (int r = k; r <= k + 2 && r < p.cr.end[ck]; ++r) if (p.map[(size_t)r * T + j]) t = std::max(t, p.time[p.cr.end[p.chain_of[j]] - 1] + 2);
    }
    p.time[k] = t;
  }
  std::vector<int> order(T);
  for (int k = 0; k < T; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.time[a] < p.time[b]; });
  p.rho1.assign(T, 0);
  for (int r = 0; r < T; ++r) p.rho1[order[r]] = r + 1;
  for (int c = 0; c < p.cr.n; ++c) p.cr.post[c] = p.cr.end[c] < T ? p.rho1[p.cr.end[c] - 2] : 0;
  return p;
}

// The task list of a plan.  A solve task exists per non-zero tile below the two sub-diagonals, an update task per super-tile and panel that couples one of
// its tiles; the values that depend on which tasks exist and on the elimination order (ChainTask::w0, w1, w2, a, b) are computed here.  The block columns
// are visited in the plan's order; the update tasks of panel k-1 are listed with block column k ("step k"), those of a stopping chain's last panel
// (end-1) in a pseudo step of their own (k = end) behind it.
// Priorities: a task's key is the one of the single-chain list with the step's TIME in place of its index - and never below the key of anything the task
// waits for (the task that stored the counter value it waits for, the prep tasks of the chain step whose mailbox it reads): tasks are generated in an
// order in which every task only waits for earlier ones, so one pass suffices and the sorted list is a topological order by construction (for one chain
// no key is ever raised: the list is what it was).
struct TaskListInfo { bool fits = true; int scratch_tiles = 0; };      // fits: the scratch sequences found counters; scratch_tiles: slots of the scratch tile pool
class TaskListBuilder {
 public:
  TaskListBuilder(int T, const ChainPlan& plan, const PlanSwitches& ps)
      : T(T), plan(plan), nz(plan.Map()), nch(plan.cr.n), whole_from(ps.whole_from ? *ps.whole_from : WholeFrom(T)), two_panels(!nz && ps.two_panels),
        slope(ps.slope ? *ps.slope : kUpdateSlope), time(plan.time), rho1(plan.rho1), own(kMaxSuper * kMaxSuper), scratch(nch),
        solpost((size_t)nch * (T + 4), 0), rowkey((size_t)nch * (T + 4), kNone), tilekey((size_t)(T + 4) * (T + 4), kNone), stepkey(T + 4, kNone) {
    for (int I = 0; I < kMaxSuper; ++I) for (int J = 0; J < kMaxSuper; ++J) { own[I * kMaxSuper + J].cidx = cVer0 + I * kMaxSuper + J; own[I * kMaxSuper + J].sidx = cSub0 + I * kMaxSuper + J; }
  }

  // the schedule: the block columns in the plan's order; behind a stopping chain's last step the updates of its last panel and its merges
  std::vector<ChainTask> Build(TaskListInfo* info) {
    struct Event { int t, kind, k; };
    std::vector<Event> events;
    for (int k = 0; k + 1 < T; ++k) events.push_back({time[k], 0, k});
    for (int c = 0; c + 1 < nch; ++c) events.push_back({time[plan.cr.end[c] - 1] + 1, 1, plan.cr.end[c]});
    std::stable_sort(events.begin(), events.end(), [](const Event& a, const Event& b) { return a.t != b.t ? a.t < b.t : (a.kind != b.kind ? a.kind < b.kind : a.k < b.k); });
    for (const Event& ev : events) {
      if (ev.kind == 1) { ListUpdates(ev.k, ev.t, true); ListMerges(plan.chain_of[ev.k - 1], ev.t); continue; }
      ListChainStep(ev.k);
      if (ev.k != plan.cr.begin[plan.chain_of[ev.k]]) ListUpdates(ev.k, time[ev.k], false);
    }
    // the pair inverses / couplings of the paired back substitution (dense systems): off every critical path, behind the tasks of step 2g + 2
    if (!nz)
      for (int gp = 0; gp < BacksubNumPairs(T); ++gp)
        for (int part = 0; part < (gp + 1 < BacksubNumPairs(T) ? 3 : 1); ++part) items.push_back({2 * gp + 2.2, {kTaskPairPrep, 2 * gp + 2, gp, part, 0, 0, 0, 0, 0, 0, -1, 0, {0, 0, 0, 0}}});
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key < b.key; });
    std::vector<ChainTask> list(items.size());
    for (size_t i = 0; i < items.size(); ++i) list[i] = items[i].t;
    if (info) { info->fits = ok; info->scratch_tiles = slots_used; }
    return list;
  }

 private:
  static constexpr double kNone = -1e30;
  struct Item { double key; ChainTask t; };
  // one SEQUENCE of updates per super-tile and accumulation target: the tiles themselves (panels of the chain that owns the super-tile's columns) or the
  // scratch array of another chain c (its panels; added to the tiles by one merge task when chain c is through).  Per sequence: ver / sub counter,
  // parts listed, the value of ver once the tasks listed so far are done, the key of the last task, the tiles touched so far (scratch: what is not zero yet)
  struct Seq { int cidx = 0, sidx = 0, listed = 0, post = 0, touched = 0; double key = -1e30; int slot[4] = {-1, -1, -1, -1}; };      // slot: the scratch tiles of a scratch sequence's four tiles

  const int T;
  const ChainPlan& plan;
  const uint8_t* const nz;
  const int nch, whole_from;
  const bool two_panels;      // (two panels per task: dense systems)
  const double slope;
  const std::vector<int>& time;
  const std::vector<int>& rho1;
  // per super-tile key: its own sequence; per chain: the scratch sequences (I * kMaxSuper + J, sequence) and what they took from the counter / tile pools
  std::vector<Seq> own;
  std::vector<std::vector<std::pair<int, Seq>>> scratch;
  int scratch_used = 0, slots_used = 0;
  bool ok = true;
  // per chain and row; per tile; per chain step
  std::vector<int> solpost;        // per chain: value of the row's sol counter once the solves listed so far are done
  std::vector<double> rowkey;      // key of the last task that moves it
  std::vector<double> tilekey;     // key of the task that solves tile (row, column)
  std::vector<double> stepkey;     // key of the last prep task chain step s takes its inputs from (a chain's first step: none)
  std::vector<Item> items;

  bool Has(int i, int j) const { return i < T && j < T && (!nz || nz[(size_t)i * T + j] != 0); }
  double& TileKey(int r, int c) { return tilekey[(size_t)r * (T + 4) + c]; }
  int& SolPost(int c, int row) { return solpost[(size_t)c * (T + 4) + row]; }
  double& RowKey(int c, int row) { return rowkey[(size_t)c * (T + 4) + row]; }
  int VerPost(int I, int J) const { return own[I * kMaxSuper + J].post; }
  double VerKey(int I, int J) const { return own[I * kMaxSuper + J].key; }
  static double Raised(double desired, std::initializer_list<double> deps) { double k = desired; for (double d : deps) k = std::max(k, d); return k; }
  int Owner(int J) const { return plan.chain_of[std::min(2 * J, T - 1)]; }      // (a super-tile column that straddles two chains: its second block column starts a chain and never takes a panel)
  Seq& SeqOf(int c, int I, int J) {
    if (c == Owner(J)) return own[I * kMaxSuper + J];
    for (auto& e : scratch[c]) if (e.first == I * kMaxSuper + J) return e.second;
    Seq q;
    if (scratch_used + 2 > kScratchCounters) ok = false; else { q.cidx = cScratch0 + scratch_used; q.sidx = cScratch0 + scratch_used + 1; scratch_used += 2; }
    scratch[c].push_back({I * kMaxSuper + J, q});
    return scratch[c].back().second;
  }
  // the latest key among the tiles (row, col) of the block rows of super-tile (I,J) that an update at step k reads (`if_nz`: only the non-zero ones)
  double OperandKey(double dep, int k, int I, int J, int col, bool if_nz) {
    for (int row : {2 * I, 2 * I + 1, 2 * J, 2 * J + 1})
      if (row < T && row >= k + 1 && (!if_nz || Has(row, col))) dep = std::max(dep, TileKey(row, col));
    return dep;
  }

  // the tasks of chain step k: PrepX / PrepD (the next step's inputs), the solves of column k
  void ListChainStep(int k) {
    const int c = plan.chain_of[k], e = plan.cr.end[c];
    const bool first = k == plan.cr.begin[c];
    const int fl = PackFlags(first, c), tk = time[k];
    const int prev_done = first ? 0 : rho1[k - 1];
    const double step_prev = first ? kNone : stepkey[k - 1];      // M_k and the solved tile (k,k-1): chain step k-1
    if (k + 2 < e) {
      // (their ver waits only exist behind a chain's first step: PrepTask's `prev`)
      const int I2 = (k + 2) >> 1;
      const int wx0 = !first ? VerPost(I2, k >> 1) : 0, wx1 = !first ? VerPost(I2, (k + 1) >> 1) : 0, wd1 = !first ? VerPost(I2, (k + 2) >> 1) : 0;
      const double far_key = !first && Has(k + 2, k - 1) ? TileKey(k + 2, k - 1) : kNone;
      const double kx = first ? tk - 0.4 : Raised(tk - 0.4, {VerKey(I2, k >> 1), VerKey(I2, (k + 1) >> 1), RowKey(c, k + 2), RowKey(c, k + 1), step_prev, stepkey[k]});
      const double kd = first ? tk - 0.4 : Raised(tk - 0.4, {VerKey(I2, k >> 1), VerKey(I2, (k + 2) >> 1), far_key, step_prev});
      // PrepX: a = what sol[k+1] must have reached (column k-1 solved - by PrepX(k-1)), w2 = the same for sol[k+2];  PrepD: a = "column k-1 of row k+2 is solved"
      items.push_back({kx, {kTaskPrepX, k, first ? 0 : SolPost(c, k + 1), rho1[k], wx0, wx1, SolPost(c, k + 2), fl, 0, 0, -1, 0, {0, 0, 0, 0}}});
      items.push_back({kd, {kTaskPrepD, k, prev_done, rho1[k], wx0, wd1, 0, fl, 0, 0, -1, 0, {0, 0, 0, 0}}});
      TileKey(k + 2, k) = kx; TileKey(k + 1, k) = kx; RowKey(c, k + 2) = kx; RowKey(c, k + 1) = kx;
      stepkey[k + 1] = std::max(std::max(kx, kd), stepkey[k]);
      SolPost(c, k + 2) = rho1[k]; SolPost(c, k + 1) = rho1[k];
    } else if (k + 1 < e) {      // the last step of a chain that stops: the chain itself stores the tile and moves the counter
      TileKey(k + 1, k) = stepkey[k]; RowKey(c, k + 1) = std::max(RowKey(c, k + 1), stepkey[k]);
      SolPost(c, k + 1) = rho1[k];
    }
    for (int i = k + 3; i < T; ++i)
      if (Has(i, k)) {
        const double key = Raised(tk - 0.3, {VerKey(i >> 1, k >> 1), RowKey(c, i), step_prev});
        items.push_back({key, {kTaskSolve, k, i, 0, VerPost(i >> 1, k >> 1), rho1[k], SolPost(c, i), fl, 0, 0, -1, 0, {0, 0, 0, 0}}});
        SolPost(c, i) = rho1[k]; TileKey(i, k) = key; RowKey(c, i) = key;
      }
  }

  // the tiles of super-tile (I,J) in the region below / right of (k+1,k+1) that are not one of the chain's / prep's three and that panel k-1 couples (the device's `valid`)
  int CoupledTiles(int k, int I, int J) const {
    int tiles = 0;
    for (int q = 0; q < 4; ++q) {
      const int bi = 2 * I + (q >> 1), bj = 2 * J + (q & 1);
      if (bi < T && bj < T && bi >= bj && bj >= k + 1 && !StepOwnsTile(k, bi, bj) && Has(bi, k - 1) && Has(bj, k - 1)) tiles |= 1 << q;
    }
    return tiles;
  }

  // the update tasks of panel k - 1 at (pseudo) step k, which happens at time ts
  void ListUpdates(int k, int ts, bool pseudo) {
    const int pc = plan.chain_of[k - 1], fl = PackFlags(false, pc);
    for (int J = (k + 1) / 2; 2 * J < T; ++J)
      for (int I = J; 2 * I < T; ++I) {
        const int tiles = CoupledTiles(k, I, J);
        if (!tiles) continue;
        Seq& sq = SeqOf(pc, I, J);
        const bool into_scratch = pc != Owner(J);
        const int zsel = into_scratch ? pc : -1;
        // what the task waits for: the sequence's previous update, column k-1 of the block rows it reads
        double dep = OperandKey(sq.key, k, I, J, k - 1, true);
        // the time at which the super-tile's columns become the front, in steps from now (2J - (k+1) for one chain)
        const int tJ = std::min(time[2 * J], 2 * J + 1 < T ? time[2 * J + 1] : time[2 * J]);
        const int Jt = std::max(tJ / 2, (ts + 1) / 2);
        // in parts (UpdateTilesTask): four single tiles for the super-tiles PrepX(k+1) / PrepD(k+1) wait for, two block rows otherwise
        const bool front = !pseudo && I == (k + 3) / 2 && (J == I - 1 || J == I);
        const bool far = Jt - (ts + 1) / 2 >= whole_from;
        // far at the next step too: steps k (odd) and k + 1 in one task, listed where step k + 1's update would be
        const bool far_next = two_panels && k + 2 < T && J - (k + 2) / 2 >= whole_from;
        if (far && (k & 1) == 0 && two_panels) continue;      // (the odd step before it took this one along: far at k => far at k - 1)
        if (far && far_next && (k & 1) == 1) {
          sq.listed += 1;
          dep = OperandKey(dep, k, I, J, k, false);      // (column k as well)
          const double key = Raised((k + 1) + slope * (J - 0.5 * (k + 2)), {dep});
          items.push_back({key, {kTaskUpdate, k, I, PackUpdate(J, 0, kPartsTwoPanels, sq.listed), sq.post, k + 1, k, 0, sq.cidx, sq.sidx, -1, 0, {0, 0, 0, 0}}});
          sq.post = k + 1; sq.key = key;
          continue;
        }      // (whole: the least operand traffic per flop; a far super-tile has steps of slack.  A lower
               // threshold for the first steps, where the bulk is the bound: +-1 %, not kept)
        const int parts = front ? 4 : (far ? 1 : 2);      // (four tiles also for the next ring of super-tiles, other slopes of the priority: measured, no gain)
        sq.listed += parts;
        const double dist = std::max(0.5 * tJ - 0.5 * (ts + 1), -0.5);
        const double key = Raised(front ? ts - 0.2 : ts + slope * dist, {dep});
        const int post = std::max(rho1[k - 1], sq.post + 1);      // (k for one chain; several sequences and merges move a separator's counters)
        const int fresh = into_scratch ? (tiles & ~sq.touched) : 0;
        if (into_scratch) for (int q = 0; q < 4; ++q) if (((fresh >> q) & 1) && sq.slot[q] < 0) sq.slot[q] = slots_used++;
        for (int q = 0; q < parts; ++q)
          items.push_back({key, {kTaskUpdate, k, I, PackUpdate(J, q, parts, sq.listed), sq.post, post, rho1[k - 1], fl, sq.cidx, sq.sidx, zsel, fresh,
                                 {sq.slot[0], sq.slot[1], sq.slot[2], sq.slot[3]}}});
        sq.post = post; sq.key = key; sq.touched |= tiles;
      }
  }

  // chain c is through (its last panel's updates are listed): what it accumulated for other chains' super-tiles joins their own sequences
  void ListMerges(int c, int ts) {
    for (auto& e : scratch[c]) {
      const int I = e.first / kMaxSuper, J = e.first % kMaxSuper;
      Seq& z = e.second;
      Seq& o = own[e.first];
      const double key = Raised(ts + 0.05, {z.key, o.key});
      const int post = o.post + 1;
      items.push_back({key, {kTaskMerge, plan.cr.end[c], I, PackUpdate(J, 0, 0, 0), o.post, post, z.post, 0, o.cidx, z.cidx, c, z.touched, {z.slot[0], z.slot[1], z.slot[2], z.slot[3]}}});
      o.post = post; o.key = key;
    }
  }
};
inline std::vector<ChainTask> BuildTaskList(int T, const ChainPlan& plan, const PlanSwitches& ps, TaskListInfo* info = nullptr) {
  return TaskListBuilder(T, plan, ps).Build(info);
}

// Replay of a list on the host (what tests/test_cholesky_task_order.py does for a set of shapes, here for the structure at hand):
//   * every counter value a task waits for has been stored by a task EARLIER in the list (or by a chain whose inputs were), and every counter only
//     grows - what makes the one launch free of deadlocks however few workgroups are resident;
//   * every tile has received exactly the panels that couple it when a task consumes it, every operand is solved, every non-zero tile gets solved.
class TaskListReplay {
 public:
  TaskListReplay(int T, const ChainPlan& plan)
      : T(T), plan(plan), nz(plan.Map()), nch(plan.cr.n), ctr(kNumCounters, 0), px(T + 2, 0), pd(T + 2, 0), solved((size_t)T * T, 0), applied((size_t)T * T),
        zapplied(nch, std::vector<Bits>((size_t)T * T)), zslot(nch, std::vector<int>((size_t)T * T, -1)) {}

  bool Run(const std::vector<ChainTask>& list) {
    for (const ChainTask& t : list) {
      const bool met = t.type == kTaskPrepX || t.type == kTaskPrepD ? Prep(t) : t.type == kTaskSolve ? Solve(t) : t.type == kTaskMerge ? Merge(t)
                       : t.type == kTaskUpdate ? Update(t) : true;
      if (!met) return false;
    }
    return Complete();
  }

 private:
  struct Bits { uint64_t w[2] = {0, 0}; bool operator==(const Bits& o) const { return w[0] == o.w[0] && w[1] == o.w[1]; } bool none() const { return !w[0] && !w[1]; } };
  const int T;
  const ChainPlan& plan;
  const uint8_t* const nz;
  const int nch;
  std::vector<int> ctr;      // the device's counters
  std::vector<char> px, pd, solved;
  std::vector<Bits> applied;
  std::vector<std::vector<Bits>> zapplied;      // per chain: what sits in its scratch tiles
  std::vector<std::vector<int>> zslot;          // ... and where: a slot of the pool per (chain, tile), nobody else's
  std::vector<char> slot_taken;

  bool Has(int i, int j) const { return i < T && j < T && (!nz || nz[(size_t)i * T + j] != 0); }
  int& Ver(int I, int J) { return ctr[cVer0 + I * kMaxSuper + J]; }
  int& Sol(int c, int row) { return ctr[cSol0 + c * kMaxSteps + row]; }
  char& Solved(int r, int c) { return solved[(size_t)r * T + c]; }
  Bits& Applied(int r, int c) { return applied[(size_t)r * T + c]; }
  static void SetBit(Bits* b, int p) { b->w[p >> 6] |= 1ull << (p & 63); }
  Bits Coupling(int r, int c, int below) const {      // the panels p < below that couple tile (r,c)
    Bits b;
    for (int p = 0; p < below && p < c; ++p) if (Has(r, p) && Has(c, p)) SetBit(&b, p);
    return b;
  }
  // chain step s (the solve of tile (s+1,s), M_(s+1)) can run: its inputs come from k_potrf64 (a chain's first step) or from PrepX / PrepD(s-1), and step s-1 ran
  bool CanRun(int s) const {
    const int c = plan.chain_of[s], b = plan.cr.begin[c];
    if (s + 1 >= plan.cr.end[c]) return false;
    for (int q = b + 1; q <= s; ++q) if (!px[q - 1] || !pd[q - 1]) return false;
    return true;
  }
  bool ChainStores(int row, int col) const {      // tile (row,col) is the last solved tile of a chain that stops, and that step can run
    const int c = plan.chain_of[col];
    return plan.cr.end[c] < T && row == plan.cr.end[c] - 1 && col == row - 1 && CanRun(col);
  }

  bool Prep(const ChainTask& t) {
    const int k = t.k, fc = TaskChain(t.flags);
    const bool first = TaskFirstOfChain(t.flags), X = t.type == kTaskPrepX;
    const int oc = X ? k + 1 : k + 2;
    if (fc != plan.chain_of[k] || k + 2 >= plan.cr.end[fc] || first != (k == plan.cr.begin[fc])) return false;
    if (!first) {
      if (Ver((k + 2) >> 1, k >> 1) < t.w0) return false;
      if (Ver((k + 2) >> 1, oc >> 1) < t.w1) return false;
      const bool far = Has(k + 2, k - 1);
      if (Sol(fc, k + 2) < (X ? t.w2 : (far ? t.a : 0))) return false;
      if (X && Sol(fc, k + 1) < t.a) return false;
      if (!CanRun(k - 1)) return false;      // M_k, the solved tile (k,k-1)
      if (far && !Solved(k + 2, k - 1)) return false;
      if (X && !Solved(k + 1, k - 1)) return false;
    }
    // the update tasks have applied every panel below k-1 (k-1 and k the task applies itself; a chain's first step: there are none at all)
    if (!(Applied(k + 2, k) == Coupling(k + 2, k, first ? k : k - 1))) return false;
    if (!(Applied(k + 2, oc) == Coupling(k + 2, oc, first ? k : k - 1))) return false;
    if (X) {
      if (!CanRun(k)) return false;          // the solved tile (k+1,k)
      if (Sol(fc, k + 2) >= t.b || Sol(fc, k + 1) >= t.b) return false;
      Sol(fc, k + 2) = t.b; Sol(fc, k + 1) = t.b;
      Solved(k + 2, k) = 1; Solved(k + 1, k) = 1;
      px[k] = 1;
    } else pd[k] = 1;
    return true;
  }

  bool Solve(const ChainTask& t) {
    const int k = t.k, fc = TaskChain(t.flags), i = t.a;
    const bool first = TaskFirstOfChain(t.flags);
    if (fc != plan.chain_of[k] || i < k + 3 || i >= T || !Has(i, k) || first != (k == plan.cr.begin[fc])) return false;
    if (Sol(fc, i) < t.w2 || Ver(i >> 1, k >> 1) < t.w0) return false;
    if (!first && (!CanRun(k - 1) || (Has(i, k - 1) && !Solved(i, k - 1)))) return false;
    if (!(Applied(i, k) == Coupling(i, k, first ? k : k - 1))) return false;
    if (Sol(fc, i) >= t.w1) return false;
    Sol(fc, i) = t.w1;
    Solved(i, k) = 1;
    return true;
  }

  bool Merge(const ChainTask& t) {
    const int I = t.a, J = TaskSuperColumn(t.b), c = t.zsel;
    if (c < 0 || c >= nch || t.cidx != cVer0 + I * kMaxSuper + J) return false;
    if (ctr[t.cidx] < t.w0 || ctr[t.sidx] < t.w2) return false;
    for (int q = 0; q < 4; ++q) {
      const int r = 2 * I + (q >> 1), cc = 2 * J + (q & 1);
      if (r >= T || cc >= T) { if ((t.mask >> q) & 1) return false; continue; }
      Bits& z = zapplied[c][(size_t)r * T + cc];
      if (((t.mask >> q) & 1) != (z.none() ? 0 : 1)) return false;
      if (!z.none() && t.slot[q] != zslot[c][(size_t)r * T + cc]) return false;      // ... from the scratch tile they were accumulated in
      Bits& a = Applied(r, cc);
      if ((a.w[0] & z.w[0]) || (a.w[1] & z.w[1])) return false;
      a.w[0] |= z.w[0]; a.w[1] |= z.w[1];
      z = Bits();
    }
    if (ctr[t.cidx] >= t.w1) return false;
    ctr[t.cidx] = t.w1;
    return true;
  }

  // tile q of an update into chain zsel's scratch tiles sits in one slot of the pool, this (chain, tile)'s alone
  bool ScratchSlotIsOwn(const ChainTask& t, int q, int r, int c) {
    int& zs = zslot[t.zsel][(size_t)r * T + c];
    if (t.slot[q] < 0) return false;
    if (zs < 0) {
      if ((int)slot_taken.size() <= t.slot[q]) slot_taken.resize(t.slot[q] + 1, 0);
      if (slot_taken[t.slot[q]]) return false;
      slot_taken[t.slot[q]] = 1; zs = t.slot[q];
    } else if (zs != t.slot[q]) return false;
    return true;
  }

  bool Update(const ChainTask& t) {
    const int k = t.k, fc = TaskChain(t.flags);
    const int I = t.a, J = TaskSuperColumn(t.b), part = TaskPart(t.b), parts = TaskParts(t.b), target = TaskTarget(t.b);
    const bool two = parts == kPartsTwoPanels;
    if (fc != plan.chain_of[k - 1] || t.zsel >= nch || (t.zsel >= 0 && t.zsel != fc)) return false;
    if (t.zsel < 0 && (t.cidx != cVer0 + I * kMaxSuper + J || t.sidx != cSub0 + I * kMaxSuper + J)) return false;
    if (ctr[t.cidx] < t.w0) return false;
    auto row_ok = [&](int row, bool distinct) {
      if (!(distinct && row < T && row >= k + 1 && Has(row, k - 1))) return true;
      int have = Sol(fc, row);
      if (ChainStores(row, k - 1)) have = std::max(have, plan.cr.post[fc]);
      return have >= (two ? t.w2 + 1 : t.w2);
    };
    const int bi = 2 * I + (parts == 2 ? part : part >> 1), bj0 = 2 * J + (parts == 2 ? 0 : part & 1), nb = parts == 2 ? 2 : 1;
    bool rows_ok;
    if (parts == 1 || two) rows_ok = row_ok(2 * I, true) && row_ok(2 * I + 1, true) && row_ok(2 * J, J != I) && row_ok(2 * J + 1, J != I);
    else rows_ok = row_ok(bi, true) && row_ok(bj0, bj0 != bi) && row_ok(bj0 + 1, nb == 2 && bj0 + 1 != bi);
    if (!rows_ok) return false;
    // the tiles it updates (the device's `valid`), panel k-1 (and k: two)
    for (int q = 0; q < 4; ++q) {
      const int r = 2 * I + (q >> 1), c = 2 * J + (q & 1);
      const bool mine = (parts == 1 || two) || (parts == 2 ? (q >> 1) == part : q == part);
      for (int kk = k; kk <= (two ? k + 1 : k); ++kk) {
        const bool valid = r < T && c < T && r >= c && c >= kk + 1 && !StepOwnsTile(kk, r, c) && Has(r, kk - 1) && Has(c, kk - 1);
        if (!mine || !valid) continue;
        for (int row : {r, c}) if (!Solved(row, kk - 1) && !ChainStores(row, kk - 1) && !(two && kk == k + 1)) return false;
        // a panel goes to the tile itself exactly when its chain owns the tile's block column
        if ((t.zsel < 0) != (plan.chain_of[kk - 1] == plan.chain_of[c])) return false;
        Bits& a = t.zsel < 0 ? Applied(r, c) : zapplied[t.zsel][(size_t)r * T + c];
        if (t.zsel >= 0 && (((t.mask >> q) & 1) != (a.none() ? 1 : 0))) return false;      // taken as zero exactly when nothing has been accumulated yet
        if (t.zsel >= 0 && !ScratchSlotIsOwn(t, q, r, c)) return false;
        if (a.w[(kk - 1) >> 6] >> ((kk - 1) & 63) & 1) return false;
        SetBit(&a, kk - 1);
      }
    }
    if (++ctr[t.sidx] == target) {
      if (ctr[t.cidx] >= t.w1) return false;
      ctr[t.cidx] = t.w1;
    }
    return true;
  }

  // every non-zero tile below the diagonal is solved, every tile got the panels that couple it (those its own tasks apply aside), nothing is left in a scratch array
  bool Complete() {
    for (int c = 0; c + 1 < T; ++c)
      for (int r = c + 1; r < T; ++r) {
        if (!Has(r, c)) continue;
        const int e = plan.cr.end[plan.chain_of[c]];
        if (r == c + 1 && r < e) { if (!Solved(r, c) && !(c + 2 >= e && CanRun(c))) return false; }
        else if (!Solved(r, c)) return false;
      }
    for (int c = 1; c < T; ++c)
      for (int r = c; r < T; ++r) {
        for (int ch = 0; ch < nch; ++ch) if (!zapplied[ch][(size_t)r * T + c].none()) return false;
        if (!Has(r, c)) continue;
        Bits want = Coupling(r, c, c);
        auto clear = [&](int p) { if (p >= 0) want.w[p >> 6] &= ~(1ull << (p & 63)); };
        clear(c - 1); if (r <= c + 1) clear(c - 2); if (r == c) clear(c - 3);
        if (!(Applied(r, c) == want)) return false;
      }
    return true;
  }
};
inline bool TaskListWaitsAreMet(int T, const ChainPlan& plan, const std::vector<ChainTask>& list) { return TaskListReplay(T, plan).Run(list); }

// (debugging aid: the chains and the closed tile map of the structure at hand)
inline void PrintPlan(int T, const ChainPlan& plan) {
  fprintf(stderr, "ppsfm plan: T %d, %d chains:", T, plan.cr.n);
  for (int c = 0; c < plan.cr.n; ++c) fprintf(stderr, " [%d,%d)", plan.cr.begin[c], plan.cr.end[c]);
  fprintf(stderr, "\n");
  for (int r = 0; r < T && !plan.map.empty(); ++r) { for (int c = 0; c <= r; ++c) fputc(plan.map[(size_t)r * T + c] ? '#' : '.', stderr); fputc('\n', stderr); }
}

// plan + list for a tile map (null: dense); a plan of several chains whose list does not pass the replay falls back to ONE chain (the former behaviour)
inline ChainPlan PlanAndList(int T, const uint8_t* nz, const PlanSwitches& ps, bool print, std::vector<ChainTask>* list, bool* verified = nullptr,
                             int* scratch_tiles = nullptr) {
  ChainPlan plan = PlanChains(T, nz, ps);
  TaskListInfo info;
  *list = BuildTaskList(T, plan, ps, &info);
  bool ok = info.fits && TaskListWaitsAreMet(T, plan, *list);
  if (!ok && plan.cr.n > 1) {
    fprintf(stderr, "ppsfm: the task list of %d chains over %d block columns did not pass its replay - one chain\n", plan.cr.n, T);
    plan = PlanChains(T, nz, ps, 1);
    *list = BuildTaskList(T, plan, ps, &info);
    ok = TaskListWaitsAreMet(T, plan, *list);
  }
  if (print) PrintPlan(T, plan);
  if (verified) *verified = ok;
  if (scratch_tiles) *scratch_tiles = info.scratch_tiles;
  return plan;
}

}  // namespace ppsfm
