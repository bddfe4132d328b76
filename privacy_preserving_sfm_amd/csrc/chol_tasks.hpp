// K3b, the one-launch structure of the dense fp64 Cholesky (cholesky.hip, "task mode"): device code only, included by cholesky.hip alone.  The task list,
// its chains and the counter layout the kernel walks are the planner's (chol_plan.hpp); k_potrf64, launched in front, is in chol_columns.hpp.
#pragma once
#include "chol_backsub.hpp"      // PairPrepBody: the kTaskPairPrep tasks
#include "chol_block.hpp"
#include "chol_plan.hpp"

namespace ppsfm {

// ---- task mode: the whole factorisation in ONE launch ------------------------------------------------------------------
// The per-column launches pay, on the critical path of every block column, a kernel boundary (~2.6 us of a ~15 us step) and a
// cold reload of M_k / X / D by a freshly dispatched chain workgroup, and every launch waits for its slowest workgroup.
// Here the same work items are ONE grid:
//   workgroup 0      the CHAIN, persistent: loops over the block columns; M_k never leaves LDS, the next step's X and D
//                    tiles are fetched by wavefronts that idle through the panels, nothing waits for the step's own stores
//   workgroups 1..   one TASK each, read from a list the host builds once per matrix size: PrepX(k), PrepD(k), the
//                    triangular solve of tile (i,k), the update of one 128x128 super-tile by panel k-1.
// Dependencies are tracked per TILE, not per step, so the tiles near the diagonal (which the chain needs next) run ahead of
// the far ones instead of waiting for the whole trailing update of the previous column (launches 1-10 of the per-column mode
// are bound by that update: 18-30 us against a ~12 us chain):
//   sol[i]      number of solved columns of block row i (tile (i,c) solved for every c < sol[i]); set by the solve task of
//               (i,c) and by PrepX(c) for rows c+1 (the chain's tile, which it copies to L) and c+2
//   ver[I][J]   number of panels applied to super-tile (I,J) = block rows 2I,2I+1 x block columns 2J,2J+1 (a FIXED grid:
//               one counter follows a super-tile through all its updates)
// (No counter follows the chain: whatever it produces is taken from a mailbox, see below.)
// The task list is sorted by a priority that is also a topological order: key = k + 0.3 x (distance of the super-column from the
// front) for an update, slightly less than k for PrepX / PrepD / a solve of step k.  A task only waits on the chain
// (resident from the first cycle) and on tasks EARLIER in the list; every XCD dispatches its share of the grid in increasing
// block index, so the lowest unfinished task is always resident with its inputs complete: the grid cannot deadlock however
// few workgroups fit the chip.  Every wait is bounded all the same: a timeout fails the factorisation (error bit 4), the other
// waits see the bit and leave, the host repeats the solve with per-column launches and stays with them.
// Hand-offs FROM and TO the chain (chain -> PrepX / PrepD / solve tasks, PrepX / PrepD -> chain) do not go through a counter at all: a memory round trip is
// 0.7 us idle and 1.5-2.5 us under load, and "store, wait for the acknowledgement, set a counter, poll it, load the data" is
// four of them per direction.  Instead every such tile has a MAILBOX slot of its own per step (M_k, the chain's X and D
// inputs, the solved X tile), preset to an all-ones NaN pattern by k_potrf64's side workgroups; the producer just stores, the
// consumer loads the data with agent-scope loads until no element is the pattern: one round trip per direction.
// Coherence without fences (the XCD L2s are not coherent inside a kernel, MI355X_MICROARCH.md "Correctness boundaries"):
//   * everything a workgroup hands to another one is stored write-through (agent-scope stores);
//   * tiles of S that are REWRITTEN during the launch (the running Schur complement) and the mailboxes (read before and
//     after they are written) are read with agent-scope loads;
//   * data written exactly ONCE per launch and only read after a counter says so can not be stale in any L2 and is read with
//     plain, L2-cached loads: the solved tiles live in their own array L (the factor ends up there; the back substitution reads
//     it from there), and so does M_k for the solve tasks.
constexpr int kSpinBound = 1 << 21;

// mailboxes of one factorisation: 64x64 row-major slots (stride 64), one per step; where they lie in the workspace: CholWorkspace (chol_plan.hpp)
struct Mailboxes {
  double* Minv;   // [T]    M_k       chain(k-1) -> PrepX(k), PrepD(k), the solve tasks of column k
  double* xs;     // [T+1]  X of chain(k) = tile (k+1,k), panels <= k-1 applied          PrepX(k-1) -> chain(k)
  double* ds;     // [T+1]  D of chain(k) = tile (k+1,k+1), panels <= k-1 applied        PrepD(k-1) -> chain(k)
  double* xsol;   // [T+1]  the solved tile (k+1,k)                                      chain(k) -> PrepX(k)
  double* Pw;     // pair inverses and pair couplings of the paired back substitution (kTaskPairPrep -> k_backsub_pairs)
  double* Zw;
};
inline Mailboxes MailboxesOf(double* ws, const CholWorkspace& w) { return Mailboxes{ws + w.Minv, ws + w.xs, ws + w.ds, ws + w.xsol, ws + w.Pw, ws + w.Zw}; }

__device__ __forceinline__ void WaitOwnStores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// every store of a task is a write-through store: once this workgroup's have been acknowledged a counter may move
__device__ __forceinline__ void TaskStoresDone() {
  WaitOwnStores();
  __syncthreads();
}
__device__ __forceinline__ bool IsPoison(double v) { return (unsigned long long)__double_as_longlong(v) == kNotReady; }
// a result that happens to be the mailbox pattern (only a NaN can be) is stored as another NaN
__device__ __forceinline__ void StoreMail(double* p, double v) { StoreThrough(p, IsPoison(v) ? __longlong_as_double((long long)kNotReadyNaN) : v); }

// All threads call; true once every one of the n <= 6 counters has reached its value.  Lane i of wavefront 0 polls counter i,
// so the wait costs ONE memory round trip, not one per counter; the other wavefronts wait at the barrier.  *s_failed is sticky
// (zeroed by thread 0 at kernel start, before the first barrier), so one barrier suffices.
// (scalars, not arrays: a lane-indexed array of pointers ends up in scratch memory)
struct WaitList {
  const int32_t *p0 = nullptr, *p1 = nullptr, *p2 = nullptr, *p3 = nullptr, *p4 = nullptr;
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0;      // <= 0: nothing to wait for in this slot
};
__device__ __forceinline__ bool TaskWait(const WaitList& wl, int32_t* flag, int* s_failed, unsigned long long* last_missing = nullptr) {
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    const int32_t* p = l == 0 ? wl.p0 : (l == 1 ? wl.p1 : (l == 2 ? wl.p2 : (l == 3 ? wl.p3 : wl.p4)));
    const int need = l == 0 ? wl.n0 : (l == 1 ? wl.n1 : (l == 2 ? wl.n2 : (l == 3 ? wl.n3 : wl.n4)));
    bool mine = l >= 5 || need <= 0;
    for (int spins = 0;; ++spins) {
      if (last_missing && l == 0) *last_missing = __ballot(!mine) | ((unsigned long long)spins << 8);      // (trace builds: what the last round still waited for)
      if (!mine) mine = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
      if (__all(mine)) break;
      bool give_up = spins >= kSpinBound;
      if ((spins & 1023) == 1023) give_up = give_up || (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4);   // somebody else gave up
      if (give_up) { if (l == 0) { atomicOr(flag, 4); *s_failed = 1; } break; }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  return *s_failed == 0;
}

// A whole mailbox tile -> LDS (row stride kLS), all 1024 threads.  One attempt with everybody (agent-scope loads; the common case:
// the tile has been there for a while - ONE memory round trip); if any element still is the pattern, ONE wavefront samples 64
// elements of the slot (one per row) until none is, the others sleep at the barrier (a workgroup that polls with all its threads
// reads 32 KB per round from below the L2s), then everybody tries again.  Bounded; false (after a barrier) if the wait gave up.
// `deposit` runs once, right after the first attempt's loads have been issued: the place for the LDS stores of tiles whose loads
// the caller issued just before the call - all of them share one memory round trip instead of queueing up behind each other.
// kEager (the two prep workgroups, whose answer the chain is waiting for): every thread polls its own elements instead - the tile
// is in LDS one round trip after it became visible, not two.
struct NoDeposit { __device__ void operator()() const {} };
template <bool kEager = false, typename Deposit = NoDeposit>
__device__ __forceinline__ bool FetchMailTile(double* dst, const double* __restrict__ src, int tid, int32_t* flag, int* s_failed, Deposit deposit = Deposit()) {
  const int r0 = tid >> 5, c2 = tid & 31;       // rows r0 and r0 + 32, columns 2 c2, 2 c2 + 1
  const double* p0 = src + (size_t)r0 * kNB + 2 * c2;
  const double* p1 = p0 + (size_t)32 * kNB;
  const double* probe = src + (size_t)(tid & 63) * kNB + (((tid & 63) * 5) & 63);
  bool mine = false;
  for (int spins = 0;; ++spins) {
    if (!mine) {
      const double a = LoadCoherent(p0), b = LoadCoherent(p0 + 1), c = LoadCoherent(p1), d = LoadCoherent(p1 + 1);
      if (spins == 0) deposit();
      if (!IsPoison(a) && !IsPoison(b) && !IsPoison(c) && !IsPoison(d)) {
        *reinterpret_cast<double2*>(dst + r0 * kLS + 2 * c2) = make_double2(a, b);
        *reinterpret_cast<double2*>(dst + (r0 + 32) * kLS + 2 * c2) = make_double2(c, d);
        mine = true;
      }
    }
    if (kEager) {
      if (mine) break;
      bool give_up = spins >= kSpinBound;
      if ((spins & 1023) == 1023) give_up = give_up || (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4);
      if (give_up) { atomicOr(flag, 4); *s_failed = 1; break; }
      continue;
    }
    if (__syncthreads_and(mine)) break;        // (also the barrier that publishes the LDS tile)
    if (tid < 64) {
      for (int inner = 0;; ++inner) {
        if (__all(!IsPoison(LoadCoherent(probe)))) break;
        bool give_up = inner >= kSpinBound || spins >= 4096;
        if ((inner & 1023) == 1023) give_up = give_up || (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4);
        if (give_up) { if (tid == 0) { atomicOr(flag, 4); *s_failed = 1; } break; }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __syncthreads();
    if (*s_failed) break;
  }
  if (kEager) __syncthreads();
  return *s_failed == 0;
}

// The chain workgroup.  Per step k: X M_k^T, D -= X X^T, the panels (M_{k+1} built beside them), stores.  What keeps a step at
// the length of its arithmetic:
//   * M_k never leaves LDS: bufM holds it (built by the previous step), bufX takes X and is rebuilt into M_{k+1}; the two swap;
//   * the NEXT step's X and D tiles come out of their mailboxes through the nine wavefronts that idle through panels 2 and 3:
//     loads issued beside panel 2, looked at beside panel 3 (re-issued if the tile was not there yet) and after the last panel
//     - nothing blocks while wavefront 0 is in a panel - and written to LDS (X into the then free M_k buffer, D into the
//     buffer of the solved X, dead after panel 1); only after the last panel do they wait, bounded, for PrepX / PrepD;
//   * nothing waits for the step's own stores: the solved X goes out beside panel 0, M_{k+1} after the last panel, both to
//     mailboxes their consumers poll (no acknowledgement, no counter).
// Every pointer and thread index is laundered through an empty asm per step: inlined into the k-loop, the loop-invariant
// arithmetic the compiler hoists pushed the 128-VGPR body into spills; a real call cost a 48-register save / restore per step.
template <typename P>
__device__ __forceinline__ P* Launder(P* p) { long long z = 0; asm volatile("" : "+s"(z)); return p + z; }      // (an opaque zero OFFSET: the pointer keeps its address space - laundering the pointer itself makes every access through it a FLAT one)

// kb, ke: the chain's block columns [kb, ke) (0, T for the only chain of a system); post: see ChainRanges
__device__ __forceinline__ void ChainLoop(double* S_, double* L_, int ld_, int T, Mailboxes mb_, int32_t* flag_, int32_t* ctr_, double* smem_, double* inv_diag_,
                                          int* s_failed, int kb, int ke, int post, int solbase) {
  int swap = 0;
  // X of the first step (k_potrf64's staging copy), M_kb and the raw D of the first step
  LoadTile(smem_, mb_.xs + (size_t)kb * kNB * kNB, kNB, threadIdx.x);
  LoadTile(smem_ + kNB * kLS, mb_.Minv + (size_t)kb * kNB * kNB, kNB, threadIdx.x);
  LoadTile(smem_ + 3 * kNB * kLS, S_ + (size_t)(kb + 1) * kNB * ld_ + (size_t)(kb + 1) * kNB, ld_, threadIdx.x);
  const int wave_index = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  for (int k = kb; k + 1 < ke; ++k) {
    double* S = Launder(S_); double* L = Launder(L_); int32_t* flag = Launder(flag_);
    double* smem = smem_; double* inv_diag = inv_diag_;      // LDS: compile-time addresses - laundering them would turn every LDS access into a FLAT one
    double* mbM = Launder(mb_.Minv); const double* mbX = Launder(mb_.xs); const double* mbD = Launder(mb_.ds); double* mbS = Launder(mb_.xsol);
    int ld = ld_; asm volatile("" : "+s"(ld));
    // the thread index, re-derived per step from the lane count of the wavefront and its index in the workgroup (an SGPR): taken
    // from threadIdx.x it was one more VGPR live around the whole loop - the one the compiler spilled, and reloaded from scratch in
    // four places of the step (every index below is re-derived per step: none stays live around the loop)
    int tid;
    {
      int wv = wave_index; asm volatile("" : "+s"(wv));
      int ln; asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      tid = wv * 64 + ln;
    }
    (void)S;
    const int lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
    const bool dlate = w >= 5 && w < 12 && (w & 3) != 0;
    const bool dwave = w < 4 || dlate;
    int dti = w & 3, dtj = 0;
    if (dlate) { if (w < 8) { dti = w - 4; dtj = 1; } else { dti = w == 9 ? 2 : 3; dtj = w == 11 ? 3 : 2; } }     // as in ChainBody
    // the wavefronts that idle through panels 2 and 3 (PotrfPanels: 4, 7..14) and do NOT share wavefront 0's SIMD (w & 3 == 0): 7, 9, 10, 11, 13, 14
    // -> 0..5.  Wavefronts 4, 8, 12 fetched too at first: behind wavefront 0's raised priority they got through their 16 load instructions
    // 0.85 us AFTER the panel had ended (barrier arrivals of step 20: 6.72 / 7.08 / 7.20 us against 6.36 for wavefront 0 and 5.85 for the
    // six others) and slowed the panel itself (1.88 against 1.52 us): the panel-2 phase lasted 2.4 us.
#ifdef PP_FETCH_9WAVES      // (A/B switch for tools/chol_task_trace.hip: the former assignment)
    const int spare_rank = w == 4 ? 0 : w - 6;
    constexpr int kFetchWaves = 9, kFetchRounds = 4;
#else
    const int spare_rank = (w & 3) == 0 ? -1 : (w == 7 ? 0 : (w < 12 ? w - 8 : w - 9));
    constexpr int kFetchWaves = 6, kFetchRounds = 6;       // 32 row pairs over six wavefronts
#endif
    double* bufX = smem + (swap ? kNB * kLS : 0);
    double* bufM = smem + (swap ? 0 : kNB * kLS);
    double* BD = smem + 2 * kNB * kLS;
    double* BS = smem + 3 * kNB * kLS;
    PP_TASK_MAX(1, k);
#ifdef PP_CHOL_TRACE
    if (tid == 0) g_chol_step = k;
#endif
    const size_t xbase = (size_t)(k + 1) * kNB * ld + (size_t)k * kNB;
    PP_CHAIN_PHASE(0, k);
    PP_WAVE_ARRIVE(8);
    __syncthreads();          // X is in bufX, D in BS (fetched during the previous step, or above)
    PP_CHAIN_PHASE(1, k);
    if (*s_failed) return;
    v4f64 d = (v4f64){0.0, 0.0, 0.0, 0.0};
    if (dwave) {
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = PP_TILE(BS, dti, dtj)[(g + 4 * i) * kLS + lr];
    }
    const int s = w & 3, ct = w >> 2;
    const v4f64 x = SolveTile(bufX, bufM, s, ct, lr, g);
    PP_WAVE_ARRIVE(9);
    __syncthreads();          // every wavefront has its D tile out of BS
    TileStoreD(PP_TILE(BS, s, ct), x, lr, g);
    // the solved X straight from the registers to its mailbox (PrepX(k), PrepX(k+1), the solve tasks of column k+1 poll it): PrepX(k)'s
    // answer - the next step's X - is due before this step's last panel ends, and every microsecond the tile leaves later comes back
    // as a wait of the spare wavefronts after that panel
    if (!PP_EXP(1)) {
      double* mail = mbS + (size_t)k * kNB * kNB;
#pragma unroll
      for (int r = 0; r < 4; ++r) StoreMail(mail + (size_t)(16 * s + g + 4 * r) * kNB + 16 * ct + lr, x[r]);
    }
    PP_CHAIN_PHASE(2, k);
    PP_WAVE_ARRIVE(10);
    __syncthreads();
    PP_CHAIN_PHASE(3, k);
    ZeroTileFresh(bufX, tid);
    if (w < 4) {
      d = UpdateTileRegs(d, BS, BS, dti, dtj, lr, g);
      TileStoreD(PP_TILE(BD, dti, dtj), d, lr, g);
    }
    PP_WAVE_ARRIVE(11);
    __syncthreads();
    PP_CHAIN_PHASE(4, k);
    const bool has_next = k + 2 < ke;
    auto side = [&](int wv) {
      if (dlate) {
        if (dtj == 1) d = UpdateTileRegs(d, BS, BS, dti, dtj, lr, g);
        TileStoreD(PP_TILE(BD, dti, dtj), d, lr, g);
      } else if ((wv & 3) != 0) {
        // wavefronts 1,2,3,13,14,15 (idle beside panel 0).  The LAST step
        // has no PrepX task that copies its solved X from the mailbox to L (the back substitution reads it there): stored here.
        if (!has_next && !PP_EXP(2)) {
          const int p = (wv < 4 ? wv - 1 : wv - 10) * 64 + lane;
          for (int idx = p; idx < 2048; idx += 384) {
            const int r = idx >> 5, c2 = idx & 31;
            const double2 v = *reinterpret_cast<const double2*>(BS + r * kLS + 2 * c2);
            StoreThrough(L + xbase + (size_t)r * ld + 2 * c2, v.x);
            StoreThrough(L + xbase + (size_t)r * ld + 2 * c2 + 1, v.y);
          }
        }
      }
    };
    auto side1 = [&](int) {
      if (dlate && dtj != 1) UpdateTileInPlace(BD, BS, BS, dti, dtj, lr, g);
    };
    // the next step's X and D tiles: mailbox -> LDS by the nine spare wavefronts, BOTH tiles in flight together and WITHOUT passing
    // through registers: `global_load_lds_dwordx4` (gfx950) writes 16 bytes per lane straight into LDS at M0 + 16 x lane, agent scope
    // (sc1).  Through registers one tile at a time was all the spare branch could hold (the values that live across PotrfPanels
    // leave it ~20 VGPRs: two tiles' worth spilled, and a spill after a load is a blocking wait) - and then the D request only left
    // when X had arrived, a memory round trip after the last panel whenever X missed the first look.
    // A row of the padded LDS tile is 32 lanes x 16 bytes, so a wavefront loads two rows with two half-wave instructions (the second
    // one's M0 points 512 bytes before its row: lanes 32..63 write at M0 + 512 ..).  Arrival is checked by reading the tile back from
    // LDS (after s_waitcnt vmcnt(0)): if an element still is the mailbox pattern, the wavefront's share is requested again.
    //   per tile: 0 = not requested, 1 = in flight, 2 = in LDS;  stage 4 = both in LDS
    const double* srcX = mbX + (size_t)(k + 1) * kNB * kNB;
    const double* srcD = mbD + (size_t)(k + 1) * kNB * kNB;
    int sx = 0, sd = 0;
    int stage = (has_next && spare_rank >= 0) ? 0 : 4;
    auto issue = [&](const double* src, double* dst) {
#pragma unroll
      for (int j = 0; j < kFetchRounds; ++j) {
        const int pair = spare_rank + kFetchWaves * j;       // rows 2 pair, 2 pair + 1 (wave-uniform)
        if (pair < 32) {
          const int r = 2 * pair + (lane >> 5), c = lane & 31;
          const double* g = src + (size_t)r * kNB + 2 * c;
          // both half-wave loads in ONE asm block with its own EXEC halves: written as `if (lane < 32) load(row) else load(row + 1)` with
          // the builtin, the compiler merged the two into one instruction whose LDS base came from lane 0 (rows 2 pair + 1 landed 16
          // bytes off)
          const int lo = __builtin_amdgcn_readfirstlane((int)(size_t)(__attribute__((address_space(3))) void*)(dst + (2 * pair) * kLS));
          const int hi = __builtin_amdgcn_readfirstlane((int)(size_t)(__attribute__((address_space(3))) void*)(dst + (2 * pair + 1) * kLS - 64));
          unsigned long long saved;
          int saved_m0;      // (M0 is a reserved register: saved and restored rather than declared clobbered)
          asm volatile("s_mov_b64 %[sv], exec\n\t"
                       "s_mov_b32 %[m0s], m0\n\t"
                       "s_mov_b32 m0, %[lo]\n\t"
                       "s_mov_b32 exec_lo, -1\n\t"
                       "s_mov_b32 exec_hi, 0\n\t"
                       "global_load_lds_dwordx4 %[g], off sc1\n\t"
                       "s_mov_b32 m0, %[hi]\n\t"
                       "s_mov_b32 exec_lo, 0\n\t"
                       "s_mov_b32 exec_hi, -1\n\t"
                       "global_load_lds_dwordx4 %[g], off sc1\n\t"
                       "s_mov_b32 m0, %[m0s]\n\t"
                       "s_mov_b64 exec, %[sv]"
                       : [sv] "=&s"(saved), [m0s] "=&s"(saved_m0) : [g] "v"(g), [lo] "s"(lo), [hi] "s"(hi) : "memory");
        }
      }
    };
    auto arrived = [&](const double* dst) -> bool {      // wave-uniform: every element of this wavefront's share is there
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      bool ok = true;
#pragma unroll
      for (int j = 0; j < kFetchRounds; ++j) {
        const int pair = spare_rank + kFetchWaves * j;
        if (pair < 32) {
          const int r = 2 * pair + (lane >> 5), c = lane & 31;
          const double2 v = *reinterpret_cast<const double2*>(dst + r * kLS + 2 * c);      // (re-read each time: the asm above clobbers memory)
          ok = ok && !IsPoison(v.x) && !IsPoison(v.y);
        }
      }
      return __all(ok);
    };
    auto advance = [&]() {      // one move; X -> the M_k buffer (free since the solve), D -> BS (free since panel 1)
      if (stage == 4) return;
      const bool look_x = sx == 1, look_d = sd == 1;
      bool have_x = sx == 2, have_d = sd == 2;
      if (look_x) have_x = arrived(bufM);
      if (look_d) have_d = arrived(BS);
      if (!have_x) { issue(srcX, bufM); sx = 1; } else sx = 2;
      if (!have_d) { issue(srcD, BS); sd = 1; } else sd = 2;
      if (sx == 2 && sd == 2) stage = 4;
    };
    // beside panel 2: both requested; beside panel 3: what has arrived goes to LDS, the rest is requested again; after the last
    // panel: whatever has not arrived yet is waited for (bounded)
    auto spare_job = [&](int phase) {
      if (phase < 2) { if (!PP_EXP(8)) advance(); return; }
#ifdef PP_CHOL_TRACE
      const long long wait_t0 = wall_clock64();      // (wavefront 4 only writes it: how long the step waited for its next inputs after the last panel)
      const int wait_stage0 = sx * 4 + sd;
#endif
      for (int spins = 0; stage != 4; ++spins) {
        advance();
        if (stage == 4) break;
        bool give_up = spins >= kSpinBound;
        if ((spins & 255) == 255) give_up = give_up || (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4);
        if (give_up) { if (lane == 0) { atomicOr(flag, 4); *s_failed = 1; } break; }
      }
#ifdef PP_CHOL_TRACE
      if (w == 7 && lane == 0 && k < 128) { g_spare_wait[0][k] = wall_clock64() - wait_t0; g_spare_wait[1][k] = wait_stage0; g_spare_wait[2][k] = wait_t0; }
      if (has_next && spare_rank >= 0 && PP_EXP(16)) {      // check (switch 16 of tools/chol_task_trace.hip): what sits in LDS against what the mailbox holds now
        for (int which = 0; which < 2; ++which) {
          const double* src = which ? srcD : srcX; const double* dst = which ? BS : bufM;
          for (int j = 0; j < kFetchRounds; ++j) {
            const int pair = spare_rank + kFetchWaves * j;
            if (pair < 32) {
              const int r = 2 * pair + (lane >> 5), c = lane & 31;
              const double a = dst[r * kLS + 2 * c], b = dst[r * kLS + 2 * c + 1];
              const double ga = LoadCoherent(src + (size_t)r * kNB + 2 * c), gb = LoadCoherent(src + (size_t)r * kNB + 2 * c + 1);
              if (__double_as_longlong(a) != __double_as_longlong(ga) || __double_as_longlong(b) != __double_as_longlong(gb)) atomicAdd(&g_dbg_mismatch[which * 8 + (lane >> 5) * 4 + (j & 3)], 1);
            }
          }
        }
      }
#endif
    };
    PotrfPanels(BD, bufX, inv_diag, flag, lane, w, side, side1, spare_job);
    PP_CHAIN_PHASE(5, k);
    {      // M_{k+1} -> its mailbox (PrepX(k+1) / PrepD(k+1) and the solve tasks of column k+1 are polling it): two 16-byte pieces per thread
      double* mail = mbM + (size_t)(k + 1) * kNB * kNB;
#pragma unroll
      for (int it = 0; it < 2 && !PP_EXP(4); ++it) {
        const int idx = tid + kPanelThreads * it, r = idx >> 5, c2 = idx & 31;
        const double2 v = *reinterpret_cast<const double2*>(bufX + r * kLS + 2 * c2);
        StoreMail(mail + (size_t)r * kNB + 2 * c2, v.x);
        StoreMail(mail + (size_t)r * kNB + 2 * c2 + 1, v.y);
      }
    }
    if (k + 2 == T) StoreTile(L + xbase + kNB, BD, ld, tid);      // the last diagonal block holds part of the right-hand side's row: the back substitution reads it
    PP_CHAIN_PHASE(6, k);
    PP_TASK_MAX(2, k);
    swap ^= 1;
  }
  // the last step's stores (nothing waits for them inside the kernel - unless another chain follows: the update tasks of panel ke - 2 read the solved tile
  // (ke-1,ke-2) from L once the row's counter says so)
  TaskStoresDone();
  if (ke < T && threadIdx.x == 0) __hip_atomic_store(ctr_ + solbase + (ke - 1), post, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t* VerCounter(int32_t* ctr, int I, int J) { return ctr + cVer0 + I * kMaxSuper + J; }

// PrepX(k) / PrepD(k): everything that does not need M_k (the panel k-1 updates of the three tiles) is done before the
// workgroup looks for M_k's mailbox; after it has arrived one solve and one rank-64 update remain.  PrepX takes the solved tile
// (k+1,k) from the chain's mailbox instead of solving it a second time.  Results for the chain go to the xs / ds mailboxes;
// solved tiles go to L, so PrepX never overwrites what PrepD still reads.
template <bool kIsX>
__device__ __forceinline__ void PrepTask(double* S, double* L, int ld, int k, Mailboxes mb, int32_t* __restrict__ flag, int32_t* __restrict__ ctr, int* s_failed,
                                         double* Ba, double* Bb, double* Bc, double* Bm, int w0, int w1, int w2, bool far_nz, bool first, int done_km1, int done_k, int solbase) {
  // far_nz: tile (k+2,k-1) is structurally non-zero; first: k starts a chain; done_km1 / done_k: the counter values "column k-1 / k of a row is solved"
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int ti = w >> 2, tj = w & 3, s = w & 3, ct = w >> 2;
  const bool prev = !first;
  const size_t row_k1 = (size_t)(k + 1) * kNB * ld, row_k2 = (size_t)(k + 2) * kNB * ld;
  const size_t col_km1 = (size_t)(k - 1) * kNB, col_k = (size_t)k * kNB, col_k1 = (size_t)(k + 1) * kNB, col_k2 = (size_t)(k + 2) * kNB;
  int di = 0, dj = 0;
  if (!kIsX) { int rem = w; while (rem > di) { rem -= di + 1; ++di; } dj = rem; }
  const bool has_out = kIsX || w < 10;
  const size_t obase = kIsX ? row_k2 + col_k1 + (size_t)(16 * ti) * ld + 16 * tj : row_k2 + col_k2 + (size_t)(16 * di) * ld + 16 * dj;
  // ---- phase A: the tiles with the panels <= k-2 applied, column k-1 of rows k+1, k+2 solved
  PP_TASK_MAX(kIsX ? 19 : 20, k);
  if (prev) {
    WaitList wl;
    wl.p0 = VerCounter(ctr, (k + 2) >> 1, k >> 1); wl.n0 = w0;                                             // tile (k+2,k)
    wl.p1 = VerCounter(ctr, (k + 2) >> 1, kIsX ? (k + 1) >> 1 : (k + 2) >> 1); wl.n1 = w1;                // the output tile
    wl.p3 = ctr + solbase + (k + 2); wl.n3 = kIsX ? w2 : (far_nz ? done_km1 : 0);      // (PrepX moves this counter: behind the row's previous non-zero column, w2 >= k if far_nz)
    // PrepX: A_{k+1,k-1} = PrepX(k-1)'s solved tile, in the SAME wait (round 5).  The wait above ends with the solve task of tile (k+2,k-1), ~6 us after
    // M_{k-1} exists; PrepX(k-1) moves this counter ~1.5 us earlier, so asking for it here costs nothing and saves the second wait's round trip and the
    // tile's own load round trip below: phase A was 8.7 us (tools/chol_task_trace, round 5), the PrepX(k-1) -> PrepX(k) -> chain cycle 14 us per step
    if (kIsX) { wl.p2 = ctr + solbase + (k + 1); wl.n2 = done_km1; }
    if (!TaskWait(wl, flag, s_failed)) return;
  }
  PP_TASK_MAX(kIsX ? 3 : 11, k);
  v4f64 out = (v4f64){0.0, 0.0, 0.0, 0.0};
  if (has_out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = LoadCoherent(S + obase + (size_t)(g + 4 * i) * ld + lr);
  }
  // (k+2,k) with the panels <= k-2 applied, A_{k+2,k-1}, and A_{k,k-1} = the solved X tile of chain(k-1) from its mailbox (in there
  // since early in that step): every load of phase A in flight together
  const double2 c0 = TileLoad2Coherent(S + row_k2 + col_k, ld, tid, 0), c1 = TileLoad2Coherent(S + row_k2 + col_k, ld, tid, 1);
  if (prev) {
    // (a structurally zero tile (k+2,k-1) was never solved: its place in L holds nothing - an exact zero tile instead)
    const double2 zz = make_double2(0.0, 0.0);
    const double2 b0 = far_nz ? TileLoad2(L + row_k2 + col_km1, ld, tid, 0) : zz, b1 = far_nz ? TileLoad2(L + row_k2 + col_km1, ld, tid, 1) : zz;
    // (PrepX: A_{k+1,k-1} rides in the same round trip, into the buffer M_k takes later)
    const double2 m0 = kIsX ? TileLoad2(L + row_k1 + col_km1, ld, tid, 0) : zz, m1 = kIsX ? TileLoad2(L + row_k1 + col_km1, ld, tid, 1) : zz;
    auto deposit = [&]() {
      TileStore2(Bc, tid, 0, c0); TileStore2(Bc, tid, 1, c1); TileStore2(Bb, tid, 0, b0); TileStore2(Bb, tid, 1, b1);
      if (kIsX) { TileStore2(Bm, tid, 0, m0); TileStore2(Bm, tid, 1, m1); }
    };
    if (!FetchMailTile<false>(Ba, mb.xsol + (size_t)(k - 1) * kNB * kNB, tid, flag, s_failed, deposit)) return;
    UpdateTileInPlace(Bc, Bb, Ba, ti, tj, lr, g);
    if (kIsX) out = UpdateTileRegs(out, Bb, Bm, ti, tj, lr, g);
    else if (has_out) out = UpdateTileRegs(out, Bb, Bb, di, dj, lr, g);
    __syncthreads();                                                                 // Bm's readers are done before M_k lands in it
  }
  // ---- phase B: M_k (its mailbox; step 0's is k_potrf64's)
  PP_TASK_MAX(kIsX ? 12 : 13, k);
  if (prev) { if (!FetchMailTile<true>(Bm, mb.Minv + (size_t)k * kNB * kNB, tid, flag, s_failed)) return; }
  else { TileStore2(Bc, tid, 0, c0); TileStore2(Bc, tid, 1, c1); LoadTile(Bm, mb.Minv + (size_t)k * kNB * kNB, kNB, tid); __syncthreads(); }
  PP_TASK_MAX(kIsX ? 4 : 14, k);
  const v4f64 x = SolveTile(Bc, Bm, s, ct, lr, g);                                   // A_{k+2,k}
  __syncthreads();
  TileStoreD(PP_TILE(Bc, s, ct), x, lr, g);
  if (kIsX) {
#pragma unroll
    for (int r = 0; r < 4; ++r) StoreThrough(L + row_k2 + col_k + (size_t)(16 * s + g + 4 * r) * ld + 16 * ct + lr, x[r]);
    if (!FetchMailTile<true>(Ba, mb.xsol + (size_t)k * kNB * kNB, tid, flag, s_failed)) return;      // the solved tile (k+1,k), stored by chain(k) beside its first panel
    TaskStoresDone();      // (the fetch above was a memory round trip: the stores of A_{k+2,k} have been acknowledged)
    // row k+2: column k solved (in L) - PrepX(k+1)'s phase A waits for it: this counter, not the X below, is on the longest cycle of the factorisation
    // (round 5: with the product and the X stores ahead of it the chain waited ~2 us per step for its next X - 787 against 721 us)
    if (tid == 0) __hip_atomic_store(ctr + solbase + (k + 2), done_k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out = UpdateTileRegs(out, Bc, Ba, ti, tj, lr, g);
    double* mail = mb.xs + (size_t)(k + 1) * kNB * kNB;
#pragma unroll
    for (int i = 0; i < 4; ++i) StoreMail(mail + (16 * ti + g + 4 * i) * kNB + 16 * tj + lr, out[i]);
    PP_TASK_MAX(5, k);
    StoreTile(L + row_k1 + col_k, Ba, ld, tid);      // the chain's solved tile (k+1,k) -> L (the chain itself only fills the mailbox: one store set less beside its first panel)
    TaskStoresDone();
    if (tid == 0) __hip_atomic_store(ctr + solbase + (k + 1), done_k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // row k+1: column k solved (in L)
  } else {
    __syncthreads();
    double* mail = mb.ds + (size_t)(k + 1) * kNB * kNB;
    if (has_out) {
      out = UpdateTileRegs(out, Bc, Bc, di, dj, lr, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) StoreMail(mail + (16 * di + g + 4 * i) * kNB + 16 * dj + lr, out[i]);
    } else {      // the strictly upper 16x16 tiles of D are never read by the factorisation, but the chain waits for the WHOLE slot
      int ui = 0, uj = 1, rem = w - 10;      // wavefronts 10..15 -> (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
      while (rem >= 3 - ui) { rem -= 3 - ui; ++ui; }
      uj = ui + 1 + rem;
#pragma unroll
      for (int i = 0; i < 4; ++i) StoreThrough(mail + (16 * ui + g + 4 * i) * kNB + 16 * uj + lr, 0.0);
    }
    PP_TASK_MAX(6, k);
  }
}

// update of ONE super-tile (block rows 2I, 2I+1 x block columns 2J, 2J+1 of the FIXED grid) by panel kp at step k = kp + 1:
// the tiles of the region below / right of (k+1,k+1) except the three the chain and the prep tasks own at this step; per tile
// the same arithmetic, in the same order, as SyrkSuperTiles (each wavefront a 32x32 piece = 2x2 MFMA tiles, 16 k-slices)
// kTwo: panels kp AND kp + 1 in one pass over the super-tile (a super-tile far from the front: every tile of it takes both): the
// operands of the second panel are requested before the first panel's products and wait in registers, C is read and written once -
// (c - p_kp) - p_kp+1, the bits of two single passes.  The early steps of a factorisation are bound by the traffic of the updates
// (~100 KB moved per 64x64 tile and panel, ~800 tiles per step); a far super-tile has steps of slack for the second panel's solves.
template <bool kTwo>
__device__ __forceinline__ void UpdateSuperTile(double* S, const double* L, int ld, int kp, int T, int I, int J, double* As, double* Bs, const uint8_t* __restrict__ nz, int fresh_mask = 0, double* zpool = nullptr, const int32_t* slot = nullptr) {
  // zpool / slot: the tiles are accumulated in scratch tiles (slot[2 x row + column] of the pool, row stride 64) instead of S; fresh_mask: tiles that count as zero
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wi = w >> 2, wj = w & 3;
  const int k = kp + 1, bi0 = 2 * I, bj0 = 2 * J;
  const int bi = bi0 + (wi >> 1), bj = bj0 + (wj >> 1);
  const bool front = (bi == k + 1 && bj == k + 1) || (bi == k + 2 && (bj == k + 1 || bj == k + 2));
  bool valid = bi < T && bj < T && bi >= bj && bj >= k + 1 && !front;
  if (valid && nz) valid = nz[(size_t)bi * T + kp] && nz[(size_t)bj * T + kp];      // (block-sparse: the panel only touches the tiles it couples; the others' operands were never solved)
  const size_t cbase = (size_t)bi * kNB * ld + (size_t)bj * kNB + (size_t)(32 * (wi & 1) + lk) * ld + 32 * (wj & 1) + lr;
  const v4f64 z = (v4f64){0.0, 0.0, 0.0, 0.0};
  v4f64 c[2][2], p[2][2] = {{z, z}, {z, z}};
  const size_t col = (size_t)kp * kNB;
  const int ra1 = bi0 + 1 < T ? bi0 + 1 : bi0, rb1 = bj0 + 1 < T ? bj0 + 1 : bj0;      // a missing block: any valid address, its results are not stored
  const double* s0 = L + (size_t)bi0 * kNB * ld + col; const double* s1 = L + (size_t)ra1 * kNB * ld + col;
  const double* s2 = L + (size_t)bj0 * kNB * ld + col; const double* s3 = L + (size_t)rb1 * kNB * ld + col;
  LoadTiles4(As, s0, As + kNB * kLS, s1, Bs, s2, Bs + kNB * kLS, s3, ld, tid);
  const int tq = 2 * (wi >> 1) + (wj >> 1);
  const bool fresh = (fresh_mask >> tq) & 1;
  double* Cw = S + cbase;
  size_t ldc = (size_t)ld;
  if (zpool && valid) { Cw = zpool + (size_t)slot[tq] * kNB * kNB + (size_t)(32 * (wi & 1) + lk) * kNB + 32 * (wj & 1) + lr; ldc = kNB; }
  if (valid) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) c[a][b][i] = fresh ? 0.0 : LoadCoherent(Cw + (size_t)(16 * a + 4 * i) * ldc + 16 * b);
  }
  double2 nx[kTwo ? 8 : 1];
  if (kTwo) {      // the second panel's four operand tiles: in flight under the first panel's products
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      nx[it] = TileLoad2(s0 + kNB, ld, tid, it); nx[2 + it] = TileLoad2(s1 + kNB, ld, tid, it);
      nx[4 + it] = TileLoad2(s2 + kNB, ld, tid, it); nx[6 + it] = TileLoad2(s3 + kNB, ld, tid, it);
    }
  }
  __syncthreads();
  const double* ar = As + (32 * wi + lr) * kLS + lk;
  const double* br = Bs + (32 * wj + lr) * kLS + lk;
  if (valid) SuperTileProducts(p, ar, br);
  if (kTwo) {
    if (valid) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { c[a][b] = c[a][b] - p[a][b]; p[a][b] = z; }
    }
    __syncthreads();      // every wavefront is done with the first panel's operands
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      TileStore2(As, tid, it, nx[it]); TileStore2(As + kNB * kLS, tid, it, nx[2 + it]);
      TileStore2(Bs, tid, it, nx[4 + it]); TileStore2(Bs + kNB * kLS, tid, it, nx[6 + it]);
    }
    __syncthreads();
    if (valid) SuperTileProducts(p, ar, br);
  }
  if (valid) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          __hip_atomic_store(Cw + (size_t)(16 * a + 4 * i) * ldc + 16 * b, c[a][b][i] - p[a][b][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The update of block row bi of a super-tile - block columns bj0 .. bj0 + nb - 1, nb <= 2 - by panel kp on all 16 wavefronts (one 16x16
// piece per wavefront and tile).  A whole super-tile on one workgroup is 11-12 us (its fp64 MFMA rate) plus the hand-over to the next
// panel's update of the same super-tile - as long as a step of the chain: the updates fell further behind with every step.  Halves
// (nb = 2) take 6 us; the super-tiles the next step's PrepX / PrepD wait for are done as four single tiles (nb = 1) on four CUs, 4 us.
// Per 16x16 piece the same arithmetic in the same order as SyrkSuperTiles (one accumulator over the 16 k-slices, then c - p).
__device__ __forceinline__ void UpdateTilesTask(double* S, const double* L, int ld, int kp, int bi, int bj0, bool valid0, bool valid1, double* At, double* Bt, bool fresh0 = false, bool fresh1 = false, double* z0 = nullptr, double* z1 = nullptr) {      // z0 / z1: scratch tiles (row stride 64) that take the place of the two tiles of S
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int ti = w >> 2, tj = w & 3;
  const size_t col = (size_t)kp * kNB;
  const size_t cbase = (size_t)bi * kNB * ld + (size_t)bj0 * kNB + (size_t)(16 * ti + lk) * ld + 16 * tj + lr;
  const v4f64 z = (v4f64){0.0, 0.0, 0.0, 0.0};
  {
    const double2 a0 = TileLoad2(L + (size_t)bi * kNB * ld + col, ld, tid, 0), a1 = TileLoad2(L + (size_t)bi * kNB * ld + col, ld, tid, 1);
    double2 b0 = make_double2(0.0, 0.0), b1 = b0, e0 = b0, e1 = b0;
    if (valid0) { b0 = TileLoad2(L + (size_t)bj0 * kNB * ld + col, ld, tid, 0); b1 = TileLoad2(L + (size_t)bj0 * kNB * ld + col, ld, tid, 1); }
    if (valid1) { e0 = TileLoad2(L + (size_t)(bj0 + 1) * kNB * ld + col, ld, tid, 0); e1 = TileLoad2(L + (size_t)(bj0 + 1) * kNB * ld + col, ld, tid, 1); }
    TileStore2(At, tid, 0, a0); TileStore2(At, tid, 1, a1);
    if (valid0) { TileStore2(Bt, tid, 0, b0); TileStore2(Bt, tid, 1, b1); }
    if (valid1) { TileStore2(Bt + kNB * kLS, tid, 0, e0); TileStore2(Bt + kNB * kLS, tid, 1, e1); }
  }
  const size_t zoff = (size_t)(16 * ti + lk) * kNB + 16 * tj + lr;
  double* C0 = z0 ? z0 + zoff : S + cbase; double* C1 = z1 ? z1 + zoff : S + cbase + kNB;
  const size_t ld0 = z0 ? (size_t)kNB : (size_t)ld, ld1 = z1 ? (size_t)kNB : (size_t)ld;
  v4f64 c0 = z, c1 = z, p0 = z, p1 = z;
  if (valid0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c0[i] = fresh0 ? 0.0 : LoadCoherent(C0 + (size_t)(4 * i) * ld0);
  }
  if (valid1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c1[i] = fresh1 ? 0.0 : LoadCoherent(C1 + (size_t)(4 * i) * ld1);
  }
  __syncthreads();
  const double* ar = At + (16 * ti + lr) * kLS + lk;
  const double* br = Bt + (16 * tj + lr) * kLS + lk;
  if (valid0 && valid1) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double av = ar[4 * kk];
      p0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[4 * kk], p0, 0, 0, 0);
      p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[kNB * kLS + 4 * kk], p1, 0, 0, 0);
    }
  } else {      // one tile: its operand is in the slot of the tile that is updated (see the loads above)
    const double* b1 = br + (valid1 ? kNB * kLS : 0);
    v4f64 p = z;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) p = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[4 * kk], b1[4 * kk], p, 0, 0, 0);
    if (valid1) p1 = p; else p0 = p;
  }
  if (valid0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) __hip_atomic_store(C0 + (size_t)(4 * i) * ld0, c0[i] - p0[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (valid1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) __hip_atomic_store(C1 + (size_t)(4 * i) * ld1, c1[i] - p1[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Solve task of tile (i,k), i >= k+3.  Nothing of it waits for a counter the chain moves: the solved tile (k,k-1) comes out of
// chain(k-1)'s mailbox (in there ~5 us into that step) and M_k out of its mailbox (stored at the end of that step), so the pending
// panel k-1 update runs during chain(k-1) and the solve starts one memory round trip after M_k exists.
__device__ __forceinline__ bool SolveTask(double* S, double* L, int ld, int k, int i, Mailboxes mb, int32_t* __restrict__ flag, int* s_failed,
                                          double* BX, double* Mk, double* B1, double* B2, bool prev_nz, bool first) {      // prev_nz: tile (i,k-1) is structurally non-zero; first: k starts a chain
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const size_t pbase = (size_t)i * kNB * ld + (size_t)k * kNB;
  const double2 x0 = TileLoad2Coherent(S + pbase, ld, tid, 0), x1 = TileLoad2Coherent(S + pbase, ld, tid, 1);
  if (!first) {
    const double2 zz = make_double2(0.0, 0.0);      // (a structurally zero tile (i,k-1) was never solved: an exact zero tile, the pending update adds nothing)
    const double2 a0 = prev_nz ? TileLoad2(L + pbase - kNB, ld, tid, 0) : zz, a1 = prev_nz ? TileLoad2(L + pbase - kNB, ld, tid, 1) : zz;
    auto deposit = [&]() { TileStore2(BX, tid, 0, x0); TileStore2(BX, tid, 1, x1); TileStore2(B1, tid, 0, a0); TileStore2(B1, tid, 1, a1); };
    if (!FetchMailTile<false>(B2, mb.xsol + (size_t)(k - 1) * kNB * kNB, tid, flag, s_failed, deposit)) return false;
    UpdateTileInPlace(BX, B1, B2, w >> 2, w & 3, lr, g);
    __syncthreads();
    // (the tiles of rows k+3, k+4 are what PrepX(k+1) / PrepX(k+2) and the front updates wait for: their workgroups poll M_k with every thread - the tile is in
    // LDS one round trip after it becomes visible, not two)
    if (i <= k + 4) { if (!FetchMailTile<true>(Mk, mb.Minv + (size_t)k * kNB * kNB, tid, flag, s_failed)) return false; }
    else if (!FetchMailTile(Mk, mb.Minv + (size_t)k * kNB * kNB, tid, flag, s_failed)) return false;
  } else {
    TileStore2(BX, tid, 0, x0); TileStore2(BX, tid, 1, x1);
    LoadTile(Mk, mb.Minv + (size_t)k * kNB * kNB, kNB, tid);      // k_potrf64's, from the previous launch
    __syncthreads();
  }
  const int s = w & 3, ct = w >> 2;
  const v4f64 x = SolveTile(BX, Mk, s, ct, lr, g);
#pragma unroll
  for (int r = 0; r < 4; ++r) StoreThrough(L + pbase + (size_t)(16 * s + g + 4 * r) * ld + 16 * ct + lr, x[r]);
  return true;
}

// nz (may be null = dense): T x T bytes, the structurally non-zero tiles of the factor (closed under fill-in, the two sub-diagonals the chain and the
// prep tasks own included): tasks only exist for those, and a task skips operands that are not (they were never solved)
__global__ __launch_bounds__(kPanelThreads) void k_cholesky_tasks(double* S, double* L, int ld, int T, Mailboxes mb, int32_t* __restrict__ flag,
                                                                  int32_t* __restrict__ ctr, const ChainTask* __restrict__ tasks, const uint8_t* __restrict__ nz, ChainRanges cr, double* Z) {      // Z: the scratch tile pool of several chains
  __shared__ __attribute__((aligned(16))) double smem[4 * kNB * kLS];
  __shared__ double inv_diag[kNB];
  __shared__ int s_failed;      // sticky: a wait of this workgroup ran into its bound
  const int b = blockIdx.x;
  if (threadIdx.x == 0) s_failed = 0;
  if (b < cr.n) {
#ifdef PP_CHOL_TRACE
    if (threadIdx.x == 0) {
      unsigned id; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
      unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      g_burn_hwid[0] = (id & 0xffff) | (xcc << 16);
    }
#endif
    int kb = 0, ke = T, post = 0;      // (selects, not cr.begin[b]: a dynamically indexed kernel argument is copied to scratch memory)
#pragma unroll
    for (int c = 0; c < kMaxChains; ++c) if (c == b) { kb = cr.begin[c]; ke = cr.end[c]; post = cr.post[c]; }
    ChainLoop(S, L, ld, T, mb, flag, ctr, smem, inv_diag, &s_failed, kb, ke, post, cSol0 + b * kMaxSteps);
#ifdef PP_CHOL_TRACE
    if (threadIdx.x == 0) __hip_atomic_store(&g_burn_stop, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    return;
  }
#ifdef PP_CHOL_TRACE
  if (tasks == nullptr) {
    // contention experiment (tools/chol_task_trace.hip ... iso N): workgroups that keep their CUs busy with ~30 KB of LDS-only code
    // (the block factorisation, on garbage) while the chain runs alone - no memory traffic, no dependence on the chain
    if (threadIdx.x == 0) {
      unsigned id; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
      unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      if (b < 512) g_burn_hwid[b] = (id & 0xffff) | (xcc << 16);
    }
    __shared__ int burn_flag[4];
    for (int i = threadIdx.x; i < 4 * kNB * kLS; i += kPanelThreads) smem[i] = (i % 67 == 0) ? 64.0 : 0.001 * (i % 13);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    while (__hip_atomic_load(&g_burn_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      PotrfPanels(smem + 2 * kNB * kLS, smem, inv_diag, (int32_t*)burn_flag, lane, w, NoSideJob(), NoSideJob());
      __syncthreads();
    }
    return;
  }
#endif
  const ChainTask t = tasks[b - cr.n];
  const int k = t.k;
  const bool first = TaskFirstOfChain(t.flags);
  const int solbase = cSol0 + TaskChain(t.flags) * kMaxSteps;
  double* B0 = smem; double* B1 = smem + kNB * kLS; double* B2 = smem + 2 * kNB * kLS; double* B3 = smem + 3 * kNB * kLS;
  auto tile_nz = [&](int r, int c) { return !nz || nz[(size_t)r * T + c] != 0; };
  if (t.type == kTaskPrepX || t.type == kTaskPrepD) {
    const bool far_nz = !first && tile_nz(k + 2, k - 1);
    if (t.type == kTaskPrepX) PrepTask<true>(S, L, ld, k, mb, flag, ctr, &s_failed, B0, B1, B2, B3, t.w0, t.w1, t.w2, far_nz, first, t.a, t.b, solbase);
    else PrepTask<false>(S, L, ld, k, mb, flag, ctr, &s_failed, B0, B1, B2, B3, t.w0, t.w1, t.w2, far_nz, first, t.a, t.b, solbase);
    return;
  }
  if (t.type == kTaskPairPrep) {
    // P and Z of pair t.a for the paired back substitution: the solved tiles (b,a), (a+2,{a,b}), (a+3,{a,b}) and the inverses M_a, M_b
    const int gp = t.a, a = 2 * gp, b = a + 1;
    const bool has_z = gp + 1 < BacksubNumPairs(T);
    WaitList wl;
    wl.p0 = ctr + cSol0 + b; wl.n0 = a + 1;
    if (has_z) { wl.p1 = ctr + cSol0 + (a + 2); wl.n1 = a + 2; wl.p2 = ctr + cSol0 + (a + 3); wl.n2 = a + 2; }
    if (!TaskWait(wl, flag, &s_failed)) return;
    int* sf = &s_failed;
    auto fetch_m = [&](double* dst, int kk) { return FetchMailTile<false>(dst, mb.Minv + (size_t)kk * kNB * kNB, (int)threadIdx.x, flag, sf); };
    (void)PairPrepBody(gp, t.b, T, L, ld, mb.Pw, mb.Zw, B0, B1, B2, B3, fetch_m);
    return;
  }
  if (t.type == kTaskSolve) {
    // tile (i,k), i >= k+3: M_k (chain(k-1)), the solved tiles (k,k-1) and (i,k-1), the panels <= k-2 applied to (i,k)
    const int i = t.a;
    const bool prev_nz = !first && tile_nz(i, k - 1);
    WaitList wl;
    wl.p1 = ctr + solbase + i; wl.n1 = t.w2;      // (the row's previous non-zero column of this chain: k if tile (i,k-1) is one)
    wl.p3 = VerCounter(ctr, i >> 1, k >> 1); wl.n3 = t.w0;
    if (!TaskWait(wl, flag, &s_failed)) return;
    PP_TASK_MIN(7, k);
    if (!SolveTask(S, L, ld, k, i, mb, flag, &s_failed, B0, B1, B2, B3, prev_nz, first)) return;
    TaskStoresDone();
    if (threadIdx.x == 0) __hip_atomic_store(ctr + solbase + i, t.w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    PP_TASK_MAX(9, k);
    return;
  }
  if (t.type == kTaskMerge) {
    // what another chain has accumulated for super-tile (I,J) in its scratch array is added to the tiles themselves: one step of the super-tile's own sequence
    const int I = t.a, J = t.b & 255;      // (TaskSuperColumn, spelled out: through the accessor the four tile offsets below come out with other shifts)
    WaitList wl;
    wl.p0 = ctr + t.cidx; wl.n0 = t.w0;
    wl.p1 = ctr + t.sidx; wl.n1 = t.w2;
    if (!TaskWait(wl, flag, &s_failed)) return;
#pragma unroll      // (constant indices into t.slot: a dynamically indexed member would put the whole task record into scratch memory)
    for (int q = 0; q < 4; ++q) {
      if (!((t.mask >> q) & 1)) continue;
      const size_t base = (size_t)(2 * I + (q >> 1)) * kNB * ld + (size_t)(2 * J + (q & 1)) * kNB;
      const double* Zt = Z + (size_t)t.slot[q] * kNB * kNB;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = (int)threadIdx.x + kPanelThreads * it, r = idx >> 6, c = idx & 63;
        const size_t o = base + (size_t)r * ld + c;
        __hip_atomic_store(S + o, LoadCoherent(S + o) + LoadCoherent(Zt + r * kNB + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    TaskStoresDone();
    if (threadIdx.x == 0) __hip_atomic_store(ctr + t.cidx, t.w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  {
    // super-tile (I,J) by panel k-1: column k-1 of its block rows solved, the panels <= k-2 applied to it
    const int I = t.a, J = TaskSuperColumn(t.b), part = TaskPart(t.b), parts = TaskParts(t.b), target = TaskTarget(t.b);
    const bool two = parts == kPartsTwoPanels;      // the whole super-tile by panels k-1 AND k: column k solved as well, ver moves by two
    WaitList wl;
    wl.p0 = ctr + t.cidx; wl.n0 = t.w0;
    auto row_slot = [&](int row, bool distinct, const int32_t** p, int* n) {      // column k-1 (and k) of a block row this task reads
      const bool used = distinct && row < T && row >= k + 1 && tile_nz(row, k - 1);
      *p = ctr + solbase + (used ? row : 0); *n = used ? (two ? t.w2 + 1 : t.w2) : 0;
    };
    const int bi = 2 * I + (parts == 2 ? part : part >> 1), bj0 = 2 * J + (parts == 2 ? 0 : part & 1), nb = parts == 2 ? 2 : 1;
    if (parts == 1 || two) {
      row_slot(2 * I, true, &wl.p1, &wl.n1); row_slot(2 * I + 1, true, &wl.p2, &wl.n2);
      row_slot(2 * J, J != I, &wl.p3, &wl.n3); row_slot(2 * J + 1, J != I, &wl.p4, &wl.n4);
    } else {
      row_slot(bi, true, &wl.p1, &wl.n1);
      row_slot(bj0, bj0 != bi, &wl.p3, &wl.n3); row_slot(bj0 + 1, nb == 2 && bj0 + 1 != bi, &wl.p4, &wl.n4);
    }
#ifdef PP_CHOL_TRACE
    const bool front = (I == (k + 3) >> 1) && (J == (k + 1) >> 1 || J == (k + 3) >> 1);      // the super-tiles PrepX(k+1) / PrepD(k+1) wait for
    const int fs = J == (k + 1) >> 1 ? 16 : 21;
    if (front) PP_TASK_MAX(fs, k);
    unsigned long long* wait_trace = (front && fs == 16 && part == 0 && k < 128) ? &g_wait_missing[k] : nullptr;
    if (!TaskWait(wl, flag, &s_failed, wait_trace)) return;
    if (false)
#endif
    if (!TaskWait(wl, flag, &s_failed)) return;
    PP_TASK_MIN(10, k);
#ifdef PP_CHOL_TRACE
    if (front) PP_TASK_MAX(fs + 1, k);
#endif
    auto valid = [&](int r, int c) {
      const bool own = (r == k + 1 && c == k + 1) || (r == k + 2 && (c == k + 1 || c == k + 2));      // the chain's / prep's three tiles
      return r < T && c < T && r >= c && c >= k + 1 && !own && tile_nz(r, k - 1) && tile_nz(c, k - 1);
    };
    const bool v0 = valid(bi, bj0), v1 = nb == 2 && valid(bi, bj0 + 1);
    const int q0 = 2 * (bi - 2 * I) + (bj0 - 2 * J);
    const int ts0 = t.slot[0], ts1 = t.slot[1], ts2 = t.slot[2], ts3 = t.slot[3];
    auto slot_of = [=](int q) { return q == 0 ? ts0 : (q == 1 ? ts1 : (q == 2 ? ts2 : ts3)); };      // (no dynamic index into the task record: it would live in scratch memory)
    const bool zs = t.zsel >= 0;      // (another chain's super-tile: into this chain's scratch tiles)
    if (parts == 1) UpdateSuperTile<false>(S, L, ld, k - 1, T, I, J, B0, B2, nz, t.mask, zs ? Z : nullptr, tasks[b - cr.n].slot);
    else if (two) UpdateSuperTile<true>(S, L, ld, k - 1, T, I, J, B0, B2, nullptr);      // (two panels per task: dense systems only)
    else if (v0 || v1) UpdateTilesTask(S, L, ld, k - 1, bi, bj0, v0, v1, B0, B2, (t.mask >> q0) & 1, (t.mask >> (q0 + 1)) & 1,
                                       zs && v0 ? Z + (size_t)slot_of(q0) * kNB * kNB : nullptr, zs && v1 ? Z + (size_t)slot_of(q0 + 1) * kNB * kNB : nullptr);
    TaskStoresDone();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(ctr + t.sidx, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == target)
      __hip_atomic_store(ctr + t.cidx, t.w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    PP_TASK_MAX(8, k);
#ifdef PP_CHOL_TRACE
    if (front) PP_TASK_MAX(fs + 2, k);
#endif
  }
}

}  // namespace ppsfm
