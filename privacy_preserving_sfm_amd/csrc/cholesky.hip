// K3b — dense fp64 Cholesky solve of the reduced camera system on the matrix cores.
//
// Replaces the linear solve Ceres performs inside ceres::Solve for the Schur-reduced camera
// system (DENSE_SCHUR / SPARSE_SCHUR chosen at reference src/optim/bundle_adjustment.cc:275-286).
//
// Layout: S is N x N row-major, N a multiple of 64, only the lower triangle is referenced.  Row
// `rhs_row` (= 6C) holds the right-hand side b (augmented system [S b; b' BIG]): its Cholesky
// factor's row rhs_row is y = L^-1 b, i.e. the forward substitution is performed by the
// factorisation itself.  Rows beyond rhs_row are identity padding.
//
// Four launch paths, chosen in ONE place (ChoosePath) when a system is bound (CholeskyBind) and when a bounded wait of task mode runs out
// (CholeskyFallBackToColumns); a solve (CholeskySolve) only enqueues or replays what was chosen:
//   small         (k_small_cholesky, 1 or 2 block columns) one launch of one workgroup, the tiles in LDS;
//   task mode     (k_cholesky_tasks, 4 to 128 block columns, dense or block-sparse) the whole factorisation in ONE launch: a persistent chain
//                 workgroup + one workgroup per item of a priority-sorted task list, per-tile dependency counters, mailbox
//                 hand-offs - see "task mode" in chol_tasks.hpp; a block-sparse system whose elimination tree has independent sub-trees (a nested-dissection
//                 order of the cameras, image_ordering.hpp BandDissector) gets a chain workgroup per sub-tree - see "ChainRanges" in chol_plan.hpp;
//   column mode   (k_column_step: 3 or more than 128 block columns, PPSFM_CHOL_MODE=columns, a task list that failed its host replay, and
//                 after a fallback) one launch per block column, over every tile or, for a block-sparse system, over its non-zero tiles only
//                 (the per-launch lists of EnsureSparseLists); captured into a graph once per bind and replayed.
// Task and column mode run the same work items (same arithmetic per 16x16 piece, bitwise equal results up to 48 block columns).
// This file is the launch driver (CholeskyState, ChoosePath, CholeskyBind, CholeskySolve, the plan cache, the uploads, EnqueueCholesky, the entry points)
// and the ONE translation unit of the device code, which it includes (k_cholesky_tasks sits at its 128-VGPR cap; the tools under tools/ include this
// file whole and launch the kernels by name):
//   chol_columns.hpp   column mode: k_potrf64 (the first diagonal blocks; launched in front of task mode too), k_column_step and its four workgroup bodies
//   chol_tasks.hpp     task mode: the mailboxes, the bounded waits, the chain loop and the task bodies of k_cholesky_tasks
//   chol_backsub.hpp   the back substitutions: k_backsub_all, k_backsub_prepare + k_backsub_pairs
//   chol_block.hpp     the building blocks all of them share (tiles in LDS, PotrfPanels, the super-tile products, the "not ready" pattern)
// k_small_cholesky, which only this driver launches, is here (in front of EnqueueCholesky).  The PLANNER of task mode - the chains of a tile map, the
// task list, its host replay, the lists of the block-sparse per-column launches, the vocabulary the kernels share with it (ChainRanges, the counter
// layout, ChainTask) and the layout of the workspace (CholWorkspace) - is host-only and lives in chol_plan.hpp.
// Column mode: right-looking blocked algorithm, 64 x 64 blocks, ONE launch per block column (k_column_step, see there):
// a chain workgroup (solve of the tile X left of the next diagonal block, that block's update by X X', its
// factorisation and the 64x64 INVERSE of the new diagonal factor) runs in the same grid as a prep workgroup (applies
// the panel-k update to the NEXT launch's chain inputs, X into a staging tile) and the bulk work that only depends
// on earlier launches (triangular solves of column k as plain products with L_kk^-1, trailing updates of
// panel k-1).  A cross-queue event edge was measured at ~9 us and a kernel boundary at ~1.7 us on MI355X, so the
// overlap is expressed INSIDE a grid and a step of the critical path pays one boundary.
// One CU sustains 307 GFLOP/s of v_mfma_f64_16x16x4 (26.6 ns per MFMA per SIMD, = the fp64 vector rate), so the
// chain workgroup is sized at 16 wavefronts and every product is spread one 16x16 tile per wavefront.
//   PotrfPanel16    16-column panel in the REGISTERS of one wavefront (lane = row, pivots/multipliers by
//                   v_readlane, no barriers); the last panel and the 16x16 tile inverses use DPP row broadcasts
//                   (PotrfLastPanelWithInverse, InverseDiag16)
//   PotrfPanels     panels on wavefront 0; in-block trailing updates one tile per wavefront; the other wavefronts
//                   build L^-1 (16x16 tile inverses by substitution, off-diagonal tiles by MFMA products) while
//                   wavefront 0 is in the next panel
//   k_backsub_all   the whole back substitution in one launch, block j waiting on the x_k (k > j) it needs
// Roofline: the trailing update is fp64-MFMA bound (n^3/3 flop); the chain workgroup is latency bound.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ba_impl.hpp"
#include "chol_backsub.hpp"
#include "chol_block.hpp"
#include "chol_columns.hpp"
#include "chol_plan.hpp"
#include "chol_tasks.hpp"
#include "resource_pool.hpp"

namespace ppsfm {

enum class CholPath { Small, Tasks, Columns, SparseColumns };      // the launch path of a bound system (ChoosePath)

struct CholeskyState {
  explicit CholeskyState(const Switches& s) : sw(s), columns(s.chol_columns), use_graph(s.chol_graph) {}
  Switches sw;                      // the owner's snapshot: the planner's switches, the back substitution, the small-system kernel
  bool columns = false;             // per-column launches only: PPSFM_CHOL_MODE=columns, or after a fallback (CholeskyFallBackToColumns)
  bool use_graph = true;            // capture the launch structure once per bind, replay per solve (off: PPSFM_CHOL_GRAPH=0, CholeskyDisableGraph, a failed capture)
  CholeskySystem sys{};             // the bound system
  const uint8_t* tile_nz = nullptr; // the bound tile map (owned by the caller, null = dense)
  CholPath path = CholPath::Columns;
  bool capture = false;             // the bound path is replayed from a graph
  hipGraphExec_t graph_exec = nullptr;
  // the owners of every device pointer below: plain device memory for the lists and maps (giving one back early waits for the device, as hipFree
  // does), the pool for the scratch tiles (resource_pool.hpp)
  DeviceBlocks lists{false}, pooled;
  ChainTask* tasks = nullptr;            // the one-launch path: the sorted task list for tasks_T block columns (device memory)
  int num_tasks = 0, tasks_T = 0;
  bool tasks_rejected = false;            // the list for (tasks_T, tasks_src_nz) did not pass its host replay: per-column launches for this structure
  const uint8_t* tasks_src_nz = nullptr;  // the tile map the list was built for (null: dense)
  uint8_t* tasks_nz = nullptr;            // device: that map + the two sub-diagonals, closed under fill-in (what the one-launch kernel and its back substitution skip by)
  ChainRanges chains{};                   // the chains of the task list
  double* scratch = nullptr;              // several chains: pool of 64 x 64 tiles in which a chain accumulates for another chain's tiles
  int scratch_tiles = 0;
  double plan_ms = 0;                     // host time of the last EnsureTaskList (plan, list, replay, upload; a cache hit: the upload)
  // block-sparse per-column launches: the per-launch row / super-tile lists of tile_nz (host + device copies) and the byte map on the device
  int sparse_T = 0, sparse_base_rows = 0, sparse_base_sups = 0;
  std::vector<int32_t> sparse_host;
  int32_t* sparse_lists = nullptr;
  uint8_t* sparse_nz = nullptr;
  int fallbacks = 0;                // one-launch factorisations that ran into a bounded wait and were repeated per column (pp_ba_summary::cholesky_fallbacks)
};

// Block-sparse structure: the per-launch lists of the bound tile map (BuildSparseColumnLists, chol_plan.hpp) in st->sparse_host; the same
// array on the device, plus the T x T byte map for the back substitution.
static int EnsureSparseLists(CholeskyState* st, int T, hipStream_t strm) {
  if (st->sparse_lists && st->sparse_T == T) return PP_OK;
  st->lists.Free(&st->sparse_lists); st->lists.Free(&st->sparse_nz);
  const uint8_t* nz = st->tile_nz;
  SparseColumnLists lists = BuildSparseColumnLists(T, nz);
  st->sparse_host.swap(lists.lists);
  st->sparse_base_rows = lists.base_rows; st->sparse_base_sups = lists.base_sups;
  PP_TRY(st->lists.Put(&st->sparse_lists, (const int32_t*)st->sparse_host.data(), st->sparse_host.size(), strm, 1));
  PP_TRY(st->lists.Put(&st->sparse_nz, nz, (size_t)T * T, strm));
  PP_HIP_TRY(hipStreamSynchronize(strm));     // (the caller's stream, not the legacy one: another host thread may be capturing its own factorisation)
  st->sparse_T = T;
  return PP_OK;
}

static std::recursive_mutex g_setup_mutex;
// Plans are kept process-wide, keyed on the tile map: the mapper builds a new BundleAdjuster per global bundle adjustment (src/sfm/incremental_mapper.cc:893-936)
// and an unchanged structure (the dense list of a size; the same sequence a second time) must not pay the plan, the list and its replay again.
// The planner's switches are part of the key: PlanChains / BuildTaskList read them from `ps` alone, and a plan made under other switches is another
// plan (without this the switches stopped doing anything once a matrix's plan was cached, and the tests that compare them compared a plan with itself).
struct CachedPlan { int T; std::vector<uint8_t> key; PlanSwitches ps; ChainPlan plan; std::vector<ChainTask> list; bool verified; int scratch_tiles; };
static std::vector<CachedPlan> g_plan_cache;      // (guarded by g_setup_mutex, most recently used last)
static constexpr size_t kPlanCacheEntries = 16, kPlanCacheBytes = (size_t)32 << 20;
static const CachedPlan& PlanCached(int T, const uint8_t* nz, const Switches& sw) {
  const size_t bytes = nz ? (size_t)T * T : 0;
  for (size_t i = g_plan_cache.size(); i-- > 0;) {
    CachedPlan& c = g_plan_cache[i];
    if (c.T == T && c.key.size() == bytes && c.ps == sw.plan && (bytes == 0 || std::memcmp(c.key.data(), nz, bytes) == 0)) {
      if (i + 1 != g_plan_cache.size()) std::rotate(g_plan_cache.begin() + i, g_plan_cache.begin() + i + 1, g_plan_cache.end());
      return g_plan_cache.back();
    }
  }
  // (least recently used first; an entry is its list - 64 bytes per task, ~5 000 tasks at 47 dense block columns, ~100 000 at 128 - plus its maps: bounded by
  // entries AND bytes)
  auto bytes_of = [](const CachedPlan& e) { return e.list.size() * sizeof(ChainTask) + e.key.size() + e.plan.map.size(); };
  size_t held = 0;
  for (const CachedPlan& e : g_plan_cache) held += bytes_of(e);
  while (!g_plan_cache.empty() && (g_plan_cache.size() >= kPlanCacheEntries || held > kPlanCacheBytes)) { held -= bytes_of(g_plan_cache.front()); g_plan_cache.erase(g_plan_cache.begin()); }
  g_plan_cache.emplace_back();
  CachedPlan& c = g_plan_cache.back();
  c.T = T; c.ps = sw.plan;
  if (nz) c.key.assign(nz, nz + bytes);
  c.plan = PlanAndList(T, nz, sw.plan, sw.chol_plan_print, &c.list, &c.verified, &c.scratch_tiles);
  return c;
}

int CholeskyChainSteps(int T, const uint8_t* nz, const Switches& sw, int* chains) {
  if (chains) *chains = 1;
  if (!nz || !UseTasks(T)) return T;
  std::lock_guard<std::recursive_mutex> lock(g_setup_mutex);
  const CachedPlan& cp = PlanCached(T, nz, sw);      // (plan + list + replay, once per tile map: pp_ba_create's winner is what EnsureTaskList asks for next)
  if (chains) *chains = cp.plan.cr.n;
  return cp.plan.Steps();
}

// The task list of the one-launch path for T block columns and the bound tile map: PrepX / PrepD / solve / update tasks sorted by priority (see above);
// built once per structure (CholeskyBind), outside any stream capture.
static int EnsureTaskList(CholeskyState* st, int T, hipStream_t strm) {
  const uint8_t* src = st->tile_nz;
  if (st->tasks_T == T && st->tasks_src_nz == src && (st->tasks || st->tasks_rejected)) return PP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  st->lists.Free(&st->tasks); st->lists.Free(&st->tasks_nz);
  std::lock_guard<std::recursive_mutex> lock(g_setup_mutex);
  const CachedPlan& cp = PlanCached(T, src, st->sw);
  const ChainPlan& plan = cp.plan;
  st->tasks_T = T;
  st->tasks_src_nz = src;
  st->tasks_rejected = !cp.verified;
  if (!cp.verified) {
    // a list whose host replay finds a wait that no earlier task meets is not launched at all (it would run into the device's bounded waits):
    // this structure is factorised by per-column launches over its tile lists
    fprintf(stderr, "ppsfm: the one-launch task list of %d block columns (%s) did not pass its replay - per-column launches for this structure\n", T, src ? "block-sparse" : "dense");
    st->num_tasks = 0;
    st->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PP_OK;
  }
  if (src) PP_TRY(st->lists.Put(&st->tasks_nz, plan.map.data(), plan.map.size(), strm));
  // (measured and dropped in round 6, PPSFM_CHOL_QUIET_XCD: an empty task at every list position whose workgroup lands on the chain's XCD - a quieter L2 /
  // fabric port for the chain, a seventh less of the chip for the bulk: 705-720 -> 721-731 us per factorisation + back substitution, 809 -> 824 us per LM iteration)
  // (on the caller's stream, not the legacy one: another host thread may be capturing its own factorisation just now)
  PP_TRY(st->lists.Put(&st->tasks, cp.list.data(), cp.list.size(), strm));
  PP_HIP_TRY(hipStreamSynchronize(strm));
  st->num_tasks = (int)cp.list.size();
  // several chains: the pool of 64 x 64 scratch tiles in which a chain accumulates for another chain's tiles
  if (cp.scratch_tiles > st->scratch_tiles) {
    st->pooled.Free(&st->scratch); st->scratch_tiles = 0;      // (recycled blocks: resource_pool.hpp)
    PP_TRY(st->pooled.Alloc(&st->scratch, (size_t)cp.scratch_tiles * kNB * kNB));
    st->scratch_tiles = cp.scratch_tiles;
  }
  st->chains = plan.cr;
  if (st->sw.chol_debug && plan.cr.n > 1) {
    fprintf(stderr, "ppsfm: %d chains over %d block columns, %d tasks, %d scratch tiles:", plan.cr.n, T, (int)cp.list.size(), cp.scratch_tiles);
    for (int c = 0; c < plan.cr.n; ++c) fprintf(stderr, " [%d,%d) t=%d..%d", plan.cr.begin[c], plan.cr.end[c], plan.time[plan.cr.begin[c]], plan.time[plan.cr.end[c] - 1]);
    fprintf(stderr, "\n");
  }
  st->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PP_OK;
}

// the back substitution: pairs for a dense factor (k_backsub_prepare + k_backsub_pairs), block by block for a block-sparse one or a
// small system.  Lw: where the factor's solved tiles live (S in per-column mode, the solved-tile array in task mode).
// pairs = false (PPSFM_BACKSUB_PAIRS=0): block by block also for dense systems (what a block-sparse system always takes; tests compare the two)
static void LaunchBacksub(const double* Lw, int N, int T, int rhs_row, double* Linv_ws, double* x_out, int32_t* d_flag, hipStream_t s, const uint8_t* nz,
                          bool pairs, bool prepared = false) {
  const int npairs = BacksubNumPairs(T);
  const CholWorkspace w(T);
  const double* Minv = Linv_ws + w.Minv;
  if (nz || npairs == 0 || !pairs) {
    hipLaunchKernelGGL(k_backsub_all, dim3(T), dim3(256), 0, s, Lw, N, T, rhs_row, Minv, x_out, d_flag, nz);
    return;
  }
  double *Pw = Linv_ws + w.Pw, *Zw = Linv_ws + w.Zw;
  if (!prepared) hipLaunchKernelGGL(k_backsub_prepare, dim3(3 * npairs), dim3(kPanelThreads), 0, s, Lw, N, T, Minv, Pw, Zw);
  hipLaunchKernelGGL(k_backsub_pairs, dim3(T - 2 * npairs + npairs), dim3(kPairThreads), 0, s, Lw, N, T, rhs_row, Minv, (const double*)Pw,
                     (const double*)Zw, x_out, d_flag);
}

// A system of one or two block columns (at most 21 images: the mapper's local bundle adjustment) in ONE launch of one workgroup: the tiles
// come into LDS, SmallFactorSolveTiles does the rest.  (k_potrf64 + k_column_step + k_backsub_all: three launches, ~40 us of a ~105 us LM
// iteration at 20 images.)  Neither the factor nor the block inverses leave the CU: nothing after the solve reads them.
__global__ __launch_bounds__(kPanelThreads) void k_small_cholesky(const double* __restrict__ S, int N, int rhs_row, double* __restrict__ x_out, int32_t* __restrict__ flag) {
  __shared__ __attribute__((aligned(16))) double tiles[4 * kNB * kLS];
  __shared__ double inv_diag[kNB], xs[2 * kNB], ys[2 * kNB];
  const int tid = threadIdx.x, T = N / kNB;
  LoadTile(tiles, S, N, tid);
  if (T == 2) LoadTiles2(tiles + kNB * kLS, S + (size_t)kNB * N, tiles + 2 * kNB * kLS, S + (size_t)kNB * N + kNB, N, tid);
  __syncthreads();
  SmallFactorSolveTiles(tiles, inv_diag, xs, ys, flag, T, rhs_row, x_out);
}

// enqueue the whole factorisation + solve of the bound system, its path as CholeskyBind chose it
// Linv_ws: the workspace, laid out by CholWorkspace (chol_plan.hpp).  Lfac: the solved-tile array of task mode, N x N like S.
static int EnqueueCholesky(const CholeskyState& st) {
  double *S = st.sys.S, *Linv_ws = st.sys.Linv_ws, *Lfac = st.sys.Lfac, *x_out = st.sys.x;
  int32_t* d_flag = st.sys.flag;
  const hipStream_t s = st.sys.stream;
  const int N = st.sys.N, rhs_row = st.sys.rhs_row, T = N / kNB;
  if (st.path == CholPath::Small) {
    hipLaunchKernelGGL(k_small_cholesky, dim3(1), dim3(kPanelThreads), 0, s, (const double*)S, N, rhs_row, x_out, d_flag);
    PP_HIP_TRY(hipGetLastError());
    return PP_OK;
  }
  const CholWorkspace w(T);
  const Mailboxes mb = MailboxesOf(Linv_ws, w);
  double *Minv = mb.Minv, *xs = mb.xs;
  int32_t* ctr = reinterpret_cast<int32_t*>(Linv_ws + w.counters);
  const bool tasks = st.path == CholPath::Tasks, sparse = st.path == CholPath::SparseColumns;
  const ChainRanges cr = tasks ? st.chains : OneChain(T);
  hipLaunchKernelGGL(k_potrf64, dim3(tasks ? 64 + cr.n : 1), dim3(kPanelThreads), 0, s, S, N, Minv, xs, d_flag, x_out, tasks ? Lfac : S, ctr, (int)kNumCounters, Minv,
                     (long long)w.MailDoubles(), cr);      // (the mailbox slots start with M_0)
  if (tasks) {
    // ONE launch: workgroup 0 = the chain, then the task list (see k_cholesky_tasks)
    // (test hook: with half of the task list missing the chain's wait for a prep task runs into its bound - the host must then repeat
    // the solve with per-column launches, tests/test_gpu_bundle_adjustment.py::test_task_mode_timeout_falls_back_to_column_launches)
    const int grid_tasks = st.sw.chol_test_drop_tasks ? st.num_tasks / 2 : st.num_tasks;
    const uint8_t* nz = st.tile_nz ? (const uint8_t*)st.tasks_nz : (const uint8_t*)nullptr;
    hipLaunchKernelGGL(k_cholesky_tasks, dim3(cr.n + grid_tasks), dim3(kPanelThreads), 0, s, S, Lfac, N, T, mb, d_flag, ctr, st.tasks, nz, cr, st.scratch);
    LaunchBacksub(Lfac, N, T, rhs_row, Linv_ws, x_out, d_flag, s, nz, st.sw.backsub_pairs, /*prepared=*/true);      // (dense: the kTaskPairPrep tasks of the launch above; block-sparse: block by block over the non-zero tiles)
    PP_HIP_TRY(hipGetLastError());
    return PP_OK;
  }
  // per-column mode: P(0); then ONE launch per block column: chain || prep (next chain's inputs) || trsm tiles of column k || syrk tiles of panel k-1.
  const int kNever = 1 << 30;
  int pending_double = kNever;      // set by the first launch of a deferred pair for the second one
  for (int k = 0; k + 1 < T; ++k) {
    const int n_prep = (k + 2 < T) ? 2 : 0, nT = std::max(T - k - 3, 0), nb = T - k - 1;
    // trailing update by panel k-1: 128x128 super-tiles of the region below (k+1,k+1) without the first one; as many
    // workgroups as fill the chip next to the chain, prep and trsm workgroups (one 16-wavefront workgroup per CU)
    const int ns = (nb + 1) / 2, nsup = (k >= 1) ? ns * (ns + 1) / 2 - 1 : 0;
    const int nW = std::min(nsup, 4 * kNumCUs);      // one super-tile per workgroup (those beyond the CU count start as trsm workgroups retire)
    // deferred pairs (see SyrkSuperTiles): while a launch has more super-tiles than the chip has CUs, every other launch
    // leaves the far block columns to the next one, which applies two panels to them at once
    int skip_from = kNever, double_from = pending_double;
    pending_double = kNever;
    if (sparse) {      // block-sparse: only the structurally non-zero tiles get a workgroup (no deferred pairs)
      const int32_t* h = st.sparse_host.data();
      const int nTs = h[k + 1] - h[k], nWs = h[T + 1 + k + 1] - h[T + 1 + k];
      hipLaunchKernelGGL(k_column_step, dim3(1 + n_prep + nTs + nWs), dim3(kPanelThreads), 0, s, S, N, k, T, Minv, xs, d_flag, kNever, kNever,
                         (const int32_t*)st.sparse_lists, st.sparse_base_rows + h[k], nTs, st.sparse_base_sups + h[T + 1 + k]);
      continue;
    }
    if (double_from == kNever && k >= 1 && nsup > kDeferAbove && k + 6 < T && k + 2 < T - 1) { skip_from = k + 6; pending_double = k + 6; }
    hipLaunchKernelGGL(k_column_step, dim3(1 + n_prep + nT + nW), dim3(kPanelThreads), 0, s, S, N, k, T, Minv, xs, d_flag, skip_from, double_from,
                       (const int32_t*)nullptr, 0, 0, 0);
  }
  LaunchBacksub(S, N, T, rhs_row, Linv_ws, x_out, d_flag, s, sparse ? (const uint8_t*)st.sparse_nz : (const uint8_t*)nullptr, st.sw.backsub_pairs);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

// Allocations, uploads and the graph capture of one handle must not run beside the capture of another host thread's handle
// (a hipMalloc from thread B invalidates thread A's capture in progress): one process-wide lock around both.
std::recursive_mutex& DeviceSetupMutex() { return g_setup_mutex; }

CholeskyState* CholeskyCreate(const Switches& sw) { return new CholeskyState(sw); }
static void DropGraph(CholeskyState* st) { if (st->graph_exec) (void)hipGraphExecDestroy(st->graph_exec); st->graph_exec = nullptr; }
void CholeskyDestroy(CholeskyState* st) {
  if (!st) return;
  DropGraph(st);
  delete st;      // (its device blocks go back with their owners)
}
bool CholeskyNeedsFactorArray(const CholeskyState* st, int N) { return !st->columns && UseTasks(N / kNB); }

// The one place the launch path is chosen (a bind, a fallback; the paths: top of this file).  The per-column launches (~190 dependent ones) are
// captured ONCE per bind into a hipGraph and replayed per LM iteration: host launch cost would otherwise bound the ~35 us steps of the critical path.
// Not captured: the small path (one launch) and any system the one-launch path is eligible for, even when its list failed the replay (three launches:
// nothing to gain, and a capture is one thing less that can collide with whatever other host threads do on the device meanwhile - a device-wide
// synchronize in another thread fails while any stream captures).
static void ChoosePath(CholeskyState* st) {
  const bool one_launch = st->sys.Lfac && CholeskyNeedsFactorArray(st, st->sys.N);      // (the bind built the task list then; null: it failed the replay)
  if (st->sw.chol_small && st->sys.N <= 2 * kNB) st->path = CholPath::Small;
  else if (one_launch && st->tasks) st->path = CholPath::Tasks;
  else st->path = st->tile_nz ? CholPath::SparseColumns : CholPath::Columns;
  st->capture = st->use_graph && st->path != CholPath::Small && !one_launch;
}

int CholeskyBind(CholeskyState* st, const CholeskySystem& sys, const uint8_t* tile_nz, bool* map_changed) {
  std::lock_guard<std::recursive_mutex> lock(g_setup_mutex);
  const int T = sys.N / kNB;
  if (map_changed) *map_changed = st->tile_nz != tile_nz;
  if (st->tile_nz != tile_nz) {
    PP_HIP_TRY(hipStreamSynchronize(sys.stream));      // (the lists of the old map may still be read)
    st->lists.Free(&st->sparse_lists); st->lists.Free(&st->sparse_nz);
    st->sparse_T = 0;
    st->tile_nz = tile_nz;
  }
  st->sys = sys;
  DropGraph(st);
  if (tile_nz) { const int rc = EnsureSparseLists(st, T, sys.stream); if (rc) return rc; }
  if (sys.Lfac && CholeskyNeedsFactorArray(st, sys.N)) { const int rc = EnsureTaskList(st, T, sys.stream); if (rc) return rc; }
  ChoosePath(st);
  return PP_OK;
}

int CholeskySolve(CholeskyState* st) {
  if (st->capture && !st->graph_exec) {
    std::lock_guard<std::recursive_mutex> lock(g_setup_mutex);
    hipGraph_t graph = nullptr;
    bool ok = hipStreamBeginCapture(st->sys.stream, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
      const int rc = EnqueueCholesky(*st);
      ok = hipStreamEndCapture(st->sys.stream, &graph) == hipSuccess && rc == PP_OK && graph &&
           hipGraphInstantiate(&st->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess;
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) { st->graph_exec = nullptr; st->use_graph = st->capture = false; (void)hipGetLastError(); }      // (eager from here on: no retry)
  }
  if (st->graph_exec) {
    PP_HIP_TRY(hipGraphLaunch(st->graph_exec, st->sys.stream));
    return PP_OK;
  }
  return EnqueueCholesky(*st);
}

bool CholeskyFallBackToColumns(CholeskyState* st) {
  if (st->columns) return false;
  st->columns = true; ++st->fallbacks;
  DropGraph(st);
  ChoosePath(st);      // (the lists of the per-column paths were built by the bind)
  return true;
}
void CholeskyDisableGraph(CholeskyState* st) { st->use_graph = st->capture = false; DropGraph(st); }
int CholeskyLinsolve(const CholeskyState* st) {      // (a block-sparse system reports SPARSE on either of its paths)
  return st->path == CholPath::Small || st->path == CholPath::Columns ? PP_LINSOLVE_CHOLESKY_COLUMNS : st->tile_nz ? PP_LINSOLVE_CHOLESKY_SPARSE : PP_LINSOLVE_CHOLESKY_TASKS;
}
int CholeskyFallbacks(const CholeskyState* st) { return st->fallbacks; }
double CholeskyPlanMs(const CholeskyState* st) { return st->plan_ms; }
bool CholeskyColumnsOnly(const CholeskyState* st) { return st->columns; }
const double* CholeskyFactor(const CholeskyState* st, const double** diag_inverses, const uint8_t** tile_map) {
  if (st->path == CholPath::Small) return nullptr;      // (neither the factor nor the block inverses leave the CU)
  *diag_inverses = st->sys.Linv_ws + CholWorkspace(st->sys.N / kNB).Minv;
  *tile_map = st->path == CholPath::Tasks ? (st->tile_nz ? st->tasks_nz : nullptr) : st->path == CholPath::SparseColumns ? st->sparse_nz : nullptr;
  return st->path == CholPath::Tasks ? st->sys.Lfac : st->sys.S;
}

}  // namespace ppsfm

using namespace ppsfm;

// The three probes of the planner (tests, tools): the task list of a tile map (null: dense, through PlanAndList as a solve builds it; else closed under
// fill-in first) of at most max_chains chains, the first `words` words of every task; the plan and the replay's verdict where asked for.
static void ProbeTaskList(int T, const uint8_t* tile_nz, int max_chains, int words, uint8_t* map_out, int32_t* tasks, int64_t capacity, int64_t* count,
                          int32_t* chains_out = nullptr, int32_t* time_out = nullptr, int32_t* rho1_out = nullptr, int32_t* verified = nullptr) {
  const Switches sw = ReadSwitches();
  std::vector<ChainTask> list;
  ChainPlan plan;
  if (tile_nz) {
    std::vector<uint8_t> closed(tile_nz, tile_nz + (size_t)T * T);
    (void)CloseTileMap(T, closed.data());
    plan = PlanChains(T, closed.data(), sw.plan, max_chains);
    TaskListInfo info;
    list = BuildTaskList(T, plan, sw.plan, &info);
    if (verified) *verified = (info.fits && TaskListWaitsAreMet(T, plan, list)) ? 1 : 0;
  } else plan = PlanAndList(T, nullptr, sw.plan, sw.chol_plan_print, &list);
  if (map_out) std::memcpy(map_out, plan.map.data(), plan.map.size());
  if (chains_out) {
    chains_out[0] = plan.cr.n;
    for (int c = 0; c < kMaxChains; ++c) { chains_out[1 + 3 * c] = plan.cr.begin[c]; chains_out[2 + 3 * c] = plan.cr.end[c]; chains_out[3 + 3 * c] = plan.cr.post[c]; }
  }
  for (int k = 0; k < T; ++k) { if (time_out) time_out[k] = plan.time[k]; if (rho1_out) rho1_out[k] = plan.rho1[k]; }
  *count = (int64_t)list.size();
  for (int64_t i = 0; i < (int64_t)list.size() && i < capacity; ++i) std::memcpy(tasks + words * i, &list[i], words * sizeof(int32_t));      // (type, k, a, b, w0, w1, w2, ...: ChainTask's order)
}

extern "C" int pp_cholesky_task_list(int32_t block_columns, int32_t* tasks, int64_t capacity, int64_t* count) try {
  PP_REQUIRE(block_columns >= 4 && block_columns <= kMaxSteps && count && (tasks || capacity == 0), "pp_cholesky_task_list: bad argument");
  ProbeTaskList(block_columns, nullptr, kMaxChains, 4, nullptr, tasks, capacity, count);
  return PP_OK;
} PP_API_CATCH("pp_cholesky_task_list")

extern "C" int pp_cholesky_task_list_sparse(int32_t block_columns, const uint8_t* tile_nz, uint8_t* map_out, int32_t* tasks, int64_t capacity, int64_t* count) try {
  PP_REQUIRE(block_columns >= 4 && block_columns <= kMaxSteps && count && tile_nz && (tasks || capacity == 0), "pp_cholesky_task_list_sparse: bad argument");
  ProbeTaskList(block_columns, tile_nz, 1, 7, map_out, tasks, capacity, count);      // ONE chain (pp_cholesky_task_plan: as many as the structure has)
  return PP_OK;
} PP_API_CATCH("pp_cholesky_task_list_sparse")

extern "C" int pp_cholesky_task_plan(int32_t block_columns, const uint8_t* tile_nz, int32_t max_chains, uint8_t* map_out, int32_t* tasks, int64_t capacity,
                                     int64_t* count, int32_t* chains_out, int32_t* time_out, int32_t* rho1_out, int32_t* verified) try {
  PP_REQUIRE(block_columns >= 4 && block_columns <= kMaxSteps && count && tile_nz && (tasks || capacity == 0), "pp_cholesky_task_plan: bad argument");
  ProbeTaskList(block_columns, tile_nz, max_chains > 0 ? max_chains : kMaxChains, 16, map_out, tasks, capacity, count, chains_out, time_out, rho1_out, verified);
  return PP_OK;
} PP_API_CATCH("pp_cholesky_task_plan")

extern "C" int pp_dense_cholesky_solve(int32_t n, const double* A, const double* b, double* x, int device, int32_t repeat,
                                       float* ms_per_solve) try {
  PP_REQUIRE(n > 0 && A && b && x && repeat >= 1, "pp_dense_cholesky_solve: bad argument");
  PP_HIP_TRY(hipSetDevice(device));
  const int N = ((n + 1 + 63) / 64) * 64;
  std::vector<double> h((size_t)N * N, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) h[(size_t)i * N + j] = A[(size_t)i * n + j];
  for (int j = 0; j < n; ++j) h[(size_t)n * N + j] = b[j];
  h[(size_t)n * N + n] = 1e100;
  for (int i = n + 1; i < N; ++i) h[(size_t)i * N + i] = 1.0;
  double *dS = nullptr, *dS0 = nullptr, *dLinv = nullptr, *dx = nullptr, *dL = nullptr;
  int32_t* dflag = nullptr;
  DeviceBlocks scratch(false);      // (released last: after the factorisation's state and the stream it ran on)
  struct Session {
    CholeskyState* st = nullptr;
    hipStream_t strm = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Session() { CholeskyDestroy(st); if (strm) (void)hipStreamDestroy(strm); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ses;
  PP_TRY(scratch.Alloc(&dS, (size_t)N * N)); PP_TRY(scratch.Alloc(&dS0, (size_t)N * N)); PP_TRY(scratch.Alloc(&dLinv, CholeskyWorkspaceDoubles(N)));
  PP_TRY(scratch.Alloc(&dx, (size_t)N)); PP_TRY(scratch.Alloc(&dflag, 4)); PP_TRY(scratch.Alloc(&dL, (size_t)N * N));
  PP_HIP_TRY(hipEventCreate(&ses.e0)); PP_HIP_TRY(hipEventCreate(&ses.e1));
  PP_HIP_TRY(hipStreamCreateWithFlags(&ses.strm, hipStreamNonBlocking));
  const hipEvent_t e0 = ses.e0, e1 = ses.e1;
  const hipStream_t strm = ses.strm;
  const Switches sw = ReadSwitches();
  CholeskyState* const st = ses.st = CholeskyCreate(sw);
  // block-sparse input (PPSFM_CHOL_SPARSE=0 disables): tiles of the lower triangle that are entirely zero and stay zero in the
  // factor get no workgroup (the reference switches to SPARSE_SCHUR above 50 images, src/optim/bundle_adjustment.cc:275-286)
  std::vector<uint8_t> tile_nz;
  {
    const int T = N / kNB;
    if (sw.chol_sparse && T >= 4) {
      tile_nz.assign((size_t)T * T, 0);
      for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j)
          if (h[(size_t)i * N + j] != 0.0) tile_nz[(size_t)(i / kNB) * T + j / kNB] = 1;
      if (CloseTileMap(T, tile_nz.data()) == T * (T + 1) / 2) tile_nz.clear();      // (nothing to skip: dense)
    }
  }
  PP_TRY(CholeskyBind(st, CholeskySystem{dS, N, n, dLinv, dL, dx, dflag, strm}, tile_nz.empty() ? nullptr : tile_nz.data()));
  PP_HIP_TRY(hipMemcpy(dS0, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  PP_HIP_TRY(hipMemset(dflag, 0, sizeof(int32_t) * 4));
  // per-solve times; the MEDIAN is reported.  This entry point creates its stream (a new hardware queue), its buffers and the kernels'
  // scratch per call, and the first dispatches on a fresh queue now and then take tens of milliseconds (observed: the untimed warm-up at
  // 70 ms instead of ~2, flag clear, three times a timed solve at 62-69 ms in ~60 calls of five to ten solves; never in 4000 LM
  // iterations on a handle, whose stream and buffers persist): one such solve must not pass for the factorisation's time.
  std::vector<float> times;
  for (int it = -1; it < repeat; ++it) {   // it = -1: untimed warm-up (graph capture + instantiate)
    if (it == -1 && repeat == 1) continue;
    PP_HIP_TRY(hipMemcpy(dS, dS0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice));
    PP_HIP_TRY(hipDeviceSynchronize());
    PP_HIP_TRY(hipEventRecord(e0, strm));
    PP_TRY(CholeskySolve(st));
    PP_HIP_TRY(hipEventRecord(e1, strm));
    PP_HIP_TRY(hipEventSynchronize(e1));
    float ms = 0; PP_HIP_TRY(hipEventElapsedTime(&ms, e0, e1)); if (it >= 0) times.push_back(ms);
    if (sw.chol_debug_slow && ms > 5.0f) {      // (how the outliers described at `times` were caught)
      int32_t f4[4] = {0, 0, 0, 0};
      (void)hipMemcpy(f4, dflag, sizeof(f4), hipMemcpyDeviceToHost);
      fprintf(stderr, "SLOW dense solve: n=%d it=%d ms=%.3f linear_solver=%d flag=%d %d %d %d\n", n, it, ms, CholeskyLinsolve(st), f4[0], f4[1], f4[2], f4[3]);
    }
    int32_t f = 0;
    PP_HIP_TRY(hipMemcpy(&f, dflag, sizeof(f), hipMemcpyDeviceToHost));
    if ((f & 4) && CholeskyFallBackToColumns(st)) {      // a bounded wait of the one-launch factorisation ran out: once more, with per-column launches from here on
      PP_HIP_TRY(hipMemset(dflag, 0, sizeof(int32_t) * 4));
      if (it >= 0) times.pop_back();
      --it;
    }
  }
  int32_t flag = 0;
  PP_HIP_TRY(hipMemcpy(&flag, dflag, sizeof(flag), hipMemcpyDeviceToHost));
  PP_HIP_TRY(hipMemcpy(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (ms_per_solve) {
    std::sort(times.begin(), times.end());
    const size_t m = times.size();
    *ms_per_solve = m == 0 ? 0.0f : (m & 1 ? times[m / 2] : 0.5f * (times[m / 2 - 1] + times[m / 2]));
  }
  if (flag) { SetLastError("pp_dense_cholesky_solve: matrix is not positive definite"); return PP_ERR_NUMERIC; }
  return PP_OK;
} PP_API_CATCH("pp_dense_cholesky_solve")
