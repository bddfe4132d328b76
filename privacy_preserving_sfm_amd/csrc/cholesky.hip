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
//                 hand-offs - see "task mode" below; a block-sparse system whose elimination tree has independent sub-trees (a nested-dissection
//                 order of the cameras, image_ordering.hip DissectBand) gets a chain workgroup per sub-tree - see "ChainRanges";
//   column mode   (k_column_step: 3 or more than 128 block columns, PPSFM_CHOL_MODE=columns, a task list that failed its host replay, and
//                 after a fallback) one launch per block column, over every tile or, for a block-sparse system, over its non-zero tiles only
//                 (the per-launch lists of EnsureSparseLists); captured into a graph once per bind and replayed.
// Task and column mode run the same work items (same arithmetic per 16x16 piece, bitwise equal results up to 48 block columns).
// This file is the device code and its launch driver (CholeskyState, ChoosePath, CholeskyBind, CholeskySolve, the plan cache, the uploads).  The
// PLANNER of task mode - the chains of a tile map, the task list, its host replay, the lists of the block-sparse per-column launches, and the
// vocabulary the kernels share with it (ChainRanges, the counter layout, ChainTask) - is host-only and lives in chol_plan.hpp.
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
#include "chol_block.hpp"
#include "chol_plan.hpp"
#include "resource_pool.hpp"

namespace ppsfm {

// the FIRST diagonal block of every chain (workgroup c: block column cr.begin[c]; one chain: block column 0): factor in place, emit its inverse
// (row-major 64x64) to that block column's slot of Minv, copy the tile below it to its X slot
// Lout: where the factored block goes (S itself in the per-column mode, the solved-tile array in task mode);
// ctr / nctr: the progress counters of task mode, reset by workgroup 0;  workgroups cr.n .. (task mode only): preset the mailbox slots
// [mail, mail + mail_doubles) to the "not written yet" pattern, except the M and X slots of the chains' first block columns
__global__ __launch_bounds__(kPanelThreads) void k_potrf64(double* __restrict__ S, int ld, double* __restrict__ Minv, double* __restrict__ xs, int32_t* __restrict__ flag,
                                                           double* __restrict__ x_out, double* Lout, int32_t* __restrict__ ctr, int nctr, double* mail,
                                                           long long mail_doubles, ChainRanges cr) {
  __shared__ __attribute__((aligned(16))) double smem[2 * kNB * kLS];
  __shared__ double inv_diag[kNB];
  double* A = smem;
  double* M = smem + kNB * kLS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // workgroups 0 .. cr.n - 1: the first diagonal block of chain c (block column kb: M_kb and the X slot of step kb are written here, not preset)
  if ((int)blockIdx.x >= cr.n) {
    // slot by slot (64 x 64 doubles each; the X slots follow the T slots of M): whether a slot is one of a chain's first step is decided once per slot
    const int nslots = (int)(mail_doubles / (kNB * kNB)), xslot0 = (int)((xs - mail) / (kNB * kNB));
    const double pattern = __longlong_as_double(-1ll);
    for (int sl = (int)blockIdx.x - cr.n; sl < nslots; sl += (int)gridDim.x - cr.n) {
      bool keep = false;
#pragma unroll
      for (int c = 0; c < kMaxChains; ++c) keep = keep || (c < cr.n && (sl == cr.begin[c] || sl == xslot0 + cr.begin[c]));
      if (keep) continue;
      double* dst = mail + (size_t)sl * kNB * kNB;
#pragma unroll
      for (int it = 0; it < 4; ++it) StoreThrough(dst + tid + kPanelThreads * it, pattern);
    }
    return;
  }
  int kb = 0;
#pragma unroll
  for (int c = 0; c < kMaxChains; ++c) if (c == (int)blockIdx.x) kb = cr.begin[c];
  if (blockIdx.x == 0) {
    if (tid == 0) __hip_atomic_store(flag + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // the PrepD -> PrepX token of k_column_step
    for (int i = tid; i < nctr; i += kPanelThreads) __hip_atomic_store(ctr + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // progress counters (task mode)
    // the back substitution's hand-off buffer starts as 'not ready' (k_backsub_all); x_out may be null (factorisation only)
    if (x_out) for (int i = tid; i < ld; i += kPanelThreads) __hip_atomic_store(reinterpret_cast<unsigned long long*>(x_out + i), 0xFFFFFFFFFFFFFFFFull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const size_t diag = (size_t)kb * kNB * ld + (size_t)kb * kNB;
  LoadTile(A, S + diag, ld, tid);
  ZeroTile(M, tid);
  __syncthreads();
  PotrfPanels(A, M, inv_diag, flag, lane, w, NoSideJob(), NoSideJob());
  StoreTile(Lout + diag, A, ld, tid);    // the strictly upper part of a diagonal block is never read
  StoreTile(Minv + (size_t)kb * kNB * kNB, M, kNB, tid);
  if (ld > kNB * (kb + 1)) {      // staging copy of tile (kb+1,kb) for the chain's first step (see k_column_step)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + kPanelThreads * it, r = idx >> 5, c2 = idx & 31;
      *reinterpret_cast<double2*>(xs + (size_t)kb * kNB * kNB + r * kNB + 2 * c2) = *reinterpret_cast<const double2*>(S + diag + (size_t)(kNB + r) * ld + 2 * c2);
    }
  }
}

// Trailing update by block column kp of the region below / right of block (kp+2, kp+2):  C -= A_i A_j^T, in 128x128
// SUPER-TILES (2x2 blocks): the workgroup stages the two 128x64 operand panels in LDS (135 KB) and each of its 16
// wavefronts owns a 32x32 piece of C = 2x2 MFMA tiles, so every operand fetched from LDS feeds two MFMAs and every operand
// byte fetched from L2 serves two block rows / columns.  Why: with one 64x64 tile per workgroup the update moved 128 KB
// per 0.5 MFLOP and the early launches (k <~ 15, ~1000 tiles) were bound by memory and by the dispatcher (1000 sixteen-
// wavefront workgroups took 19 us to START at k = 2), 20-27 us against a 15 us chain.  The accumulators start at zero and
// the C piece, whose loads are issued before the products, is combined at the end (no exposed global round trip).
// Super-tile u -> TriIndex(u + 1) = (I, J): super-tile (0, 0) is exactly the three tiles the chain / prep workgroups own.
// Workgroup q of nW takes u = q, q + nW, ...
// Deferred pairs (early launches, where this update is bound by the read-modify-write of C in HBM/MALL): in the first
// launch of a pair the tiles of block columns >= skip_from are left out, in the second one the tiles of block columns
// >= double_from (the same set, aligned to a super-column there) take the panels kp-1 AND kp in one visit — C moves once
// for 128 columns of update.  Nothing reads those tiles in between (they are >= 5 block columns ahead of the front).
template <bool kTask>      // kTask: operand panels come from the solved-tile array L (write-once), C is read coherently from S
__device__ __forceinline__ void SyrkSuperTiles(double* S, const double* L, int ld, int kp, int T, int q, int nW, int skip_from,
                                               int double_from, double* As, double* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wi = w >> 2, wj = w & 3;
  const int k1 = kp + 2, nb = T - k1, ns = (nb + 1) / 2, nsup = ns * (ns + 1) / 2 - 1;
  for (int u = q; u < nsup; u += nW) {
    int I, J;
    TriIndex(u + 1, &I, &J);
    const int bi0 = k1 + 2 * I, bj0 = k1 + 2 * J;
    if (bj0 >= skip_from) continue;                                  // the whole super-tile is deferred
    const bool has_i1 = bi0 + 1 < T, has_j1 = bj0 + 1 < T;
    const bool two = bj0 >= double_from;                             // workgroup-uniform: double_from starts a super-column
    // this wavefront's block and 32x32 piece
    const int bi = bi0 + (wi >> 1), bj = bj0 + (wj >> 1);
    const bool valid = bi < T && bj < T && bi >= bj && bj < skip_from;
    const size_t cbase = (size_t)bi * kNB * ld + (size_t)bj * kNB + (size_t)(32 * (wi & 1) + lk) * ld + 32 * (wj & 1) + lr;
    const v4f64 z = (v4f64){0.0, 0.0, 0.0, 0.0};
    v4f64 c[2][2], p[2][2] = {{z, z}, {z, z}};
    for (int pass = two ? 0 : 1; pass < 2; ++pass) {
      const size_t col = (size_t)(kp - 1 + pass) * kNB;
      __syncthreads();                    // the previous pass's / super-tile's (or the previous role's) LDS reads are done
      {
        const double* a0 = L + (size_t)bi0 * kNB * ld + col;
        const double* b0 = L + (size_t)bj0 * kNB * ld + col;
        const double* a1 = has_i1 ? a0 + (size_t)kNB * ld : a0;      // a missing block: any valid address, its results are not stored
        const double* b1 = has_j1 ? b0 + (size_t)kNB * ld : b0;
        LoadTiles4(As, a0, As + kNB * kLS, a1, Bs, b0, Bs + kNB * kLS, b1, ld, tid);
      }
      if (valid && pass == (two ? 0 : 1)) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) c[a][b][i] = LoadS<kTask>(S + cbase + (size_t)(16 * a + 4 * i) * ld + 16 * b);
      }
      __syncthreads();
      if (valid) {
        const double* ar = As + (32 * wi + lr) * kLS + lk;
        const double* br = Bs + (32 * wj + lr) * kLS + lk;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          const double a0v = ar[4 * kk], a1v = ar[16 * kLS + 4 * kk], b0v = br[4 * kk], b1v = br[16 * kLS + 4 * kk];
          p[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b0v, p[0][0], 0, 0, 0);
          p[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b1v, p[0][1], 0, 0, 0);
          p[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b0v, p[1][0], 0, 0, 0);
          p[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b1v, p[1][1], 0, 0, 0);
        }
      }
    }
    if (valid) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i)      // write-through: 30 MB of dirty lines per launch would otherwise be flushed at the kernel boundary, on the critical path
            __hip_atomic_store(S + cbase + (size_t)(16 * a + 4 * i) * ld + 16 * b, c[a][b][i] - p[a][b][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- one launch per block column ------------------------------------------------------------------------
// Launch k (k = 0 .. T-2).  Before it: L_kk and M_k = L_kk^-1 are final, block column k-1 is solved, every tile (i,j),
// j >= k, carries the trailing updates of panels 0 .. k-2, and the two tiles the chain needs — X = (k+1,k) and
// D = (k+1,k+1) — already carry panel k-1 as well (prepared by the previous launch); X is read from a staging copy
// xs[k & 1] so that nobody reads a tile another workgroup of the same launch overwrites.
// The launch holds four kinds of workgroup, all depending on EARLIER launches only:
//   chain (blockIdx 0):  X <- X M_k^T (stored to S);  D -= X X^T, factor D, store L_{k+1,k+1} and M_{k+1}
//   prep  (blockIdx 1 = PrepX, 2 = PrepD, when block row k+2 exists): everything the NEXT chain needs, redundantly where
//          necessary (PrepBody):
//          A_{k+1,k} = X M_k^T and A_{k+2,k} = ((k+2,k) - A_{k+2,k-1} A_{k,k-1}^T) M_k^T (stored: it is also column k's tile),
//          X' = (k+2,k+1) - A_{k+2,k-1} A_{k+1,k-1}^T - A_{k+2,k} A_{k+1,k}^T  (stored to S and to xs[(k+1) & 1]),
//          D' = (k+2,k+2) - A_{k+2,k-1} A_{k+2,k-1}^T - A_{k+2,k} A_{k+2,k}^T
//   trsm tiles  (i >= k+3):  tile (i,k) -= A_{i,k-1} A_{k,k-1}^T, times M_k^T, store
//   trailing update (SyrkSuperTiles): tiles (i,j), i >= j >= k+1, except the three the chain and the prep workgroups own:
//          -= A_{i,k-1} A_{j,k-1}^T, one 128x128 super-tile per workgroup
// so the critical path of a step is: load X, M_k, D -> one product -> one rank-64 update of D's first block column ->
// the panels -> ONE kernel boundary.  Everything else (the prep pair, the solves, the trailing update) runs beside it.
// The triangular solve is a plain product with the explicit inverse of the 64x64 diagonal factor: 10 independent
// 16x16x16 products per 16-row strip instead of a 7-stage dependent substitution chain, and the back substitution gets
// its L_kk^-1 for free.

template <bool kTask>      // kTask: the unsolved tile is read coherently from S, solved tiles live in L (legacy: L == S)
__device__ __forceinline__ void TrsmTileBody(double* S, double* L, int ld, int k, int i, const double* __restrict__ Minv, double* BX,
                                             double* Mk, double* B1, double* B2) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const size_t dbase = (size_t)k * kNB * ld + (size_t)k * kNB, pbase = (size_t)i * kNB * ld + (size_t)k * kNB;
  const double* mk = Minv + (size_t)k * kNB * kNB;
  if (k > 0) {
    // X, A_{i,k-1}, A_{k,k-1} (row stride ld) and M_k (row stride 64)
    if (kTask) { LoadTileT<true>(BX, S + pbase, ld, tid); LoadTile(B1, L + pbase - kNB, ld, tid); }
    else LoadTiles2(BX, S + pbase, B1, S + pbase - kNB, ld, tid);
    LoadTile(B2, L + dbase - kNB, ld, tid);
    LoadTileT<kTask>(Mk, mk, kNB, tid);      // (task mode: M_k's slot is a mailbox other workgroups have polled - its lines may sit stale in an L2)
    __syncthreads();
    UpdateTileInPlace(BX, B1, B2, w >> 2, w & 3, lr, g);
  } else {
    LoadTileT<kTask>(BX, S + pbase, ld, tid);
    LoadTile(Mk, mk, kNB, tid);
  }
  __syncthreads();
  const int s = w & 3, ct = w >> 2;    // SIMD (w & 3) gets one tile of every column tile: balanced MFMA load
  const v4f64 x = SolveTile(BX, Mk, s, ct, lr, g);
#pragma unroll
  for (int r = 0; r < 4; ++r) StoreThrough(L + pbase + (size_t)(16 * s + g + 4 * r) * ld + 16 * ct + lr, x[r]);
}

__device__ __forceinline__ void ChainBody(double* __restrict__ S, int ld, int k, int T, double* __restrict__ Minv, const double* __restrict__ xs_k,
                                          int32_t* __restrict__ flag, double* BX, double* Mk, double* BD, double* BS, double* inv_diag) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const size_t xbase = (size_t)(k + 1) * kNB * ld + (size_t)k * kNB;       // X
  const size_t nbase = xbase + kNB;                                        // D
  // D tiles: the first block column (needed by panel 0) on wavefronts 0..3; the six others on wavefronts
  // 5,6,7,9,10,11, which finish them while wavefront 0 is already in panel 0 — none of them shares wavefront 0's
  // SIMD (w & 3 == 0), whose issue slots the panel needs
  const bool dlate = w >= 5 && w < 12 && (w & 3) != 0;
  const bool dwave = w < 4 || dlate;
  int dti = w & 3, dtj = 0;
  if (dlate) {   // wavefronts 5,6,7: (1,1) (2,1) (3,1);  9,10,11: (2,2) (3,2) (3,3)
    if (w < 8) { dti = w - 4; dtj = 1; } else { dti = w == 9 ? 2 : 3; dtj = w == 11 ? 3 : 2; }
  }
  PP_CHOL_PHASE(0);
  v4f64 d = (v4f64){0.0, 0.0, 0.0, 0.0};
  if (dwave) {
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = S[nbase + (size_t)(16 * dti + g + 4 * i) * ld + 16 * dtj + lr];
  }
  LoadTiles2(BX, xs_k, Mk, Minv + (size_t)k * kNB * kNB, kNB, tid);          // both row-major 64x64, row stride 64
  __syncthreads();
  PP_CHOL_PHASE(1);
  PP_CHOL_PHASE(2);
  const int s = w & 3, ct = w >> 2;      // SIMD (w & 3) gets one tile of every column tile: balanced MFMA load
  const v4f64 x = SolveTile(BX, Mk, s, ct, lr, g);
  TileStoreD(PP_TILE(BS, s, ct), x, lr, g);   // solved X
  __syncthreads();
  ZeroTile(BX, tid);                          // BX becomes M_{k+1} (every read of it is done)
  PP_CHOL_PHASE(12);
  if (w < 4) {   // first block column of D -= X X^T
    d = UpdateTileRegs(d, BS, BS, dti, dtj, lr, g);
    TileStoreD(PP_TILE(BD, dti, dtj), d, lr, g);
  }
  __syncthreads();
  PP_CHOL_PHASE(13);
  // Beside panel 0: the D tiles of block column 1 (the next panel's) on wavefronts 5,6,7 - one per SIMD other than wavefront 0's -
  // while wavefronts 9,10,11 only park their raw D tiles (2,2) (3,2) (3,3) in LDS; beside panel 1 those three tiles get their
  // X X^T (nothing reads them before the trailing update that follows panel 1).  With all six tiles beside panel 0 that phase
  // lasted 1.8 us for a 1.45 us panel (two 16-MFMA tiles per SIMD).  The solved X goes back to S from wavefronts that idle
  // beside panel 0 (issued later, its write-through stores were still in flight at the end of the workgroup).
  auto side = [&](int wv) {
    if (dlate) {
      if (dtj == 1) d = UpdateTileRegs(d, BS, BS, dti, dtj, lr, g);
      TileStoreD(PP_TILE(BD, dti, dtj), d, lr, g);
    } else if ((wv & 3) != 0) {
      const int p = (wv < 4 ? wv - 1 : wv - 10) * 64 + lane;     // wavefronts 1,2,3,13,14,15
      for (int idx = p; idx < 2048; idx += 384) {
        const int r = idx >> 5, c2 = idx & 31;
        const double2 v = *reinterpret_cast<const double2*>(BS + r * kLS + 2 * c2);
        StoreThrough(S + xbase + (size_t)r * ld + 2 * c2, v.x);
        StoreThrough(S + xbase + (size_t)r * ld + 2 * c2 + 1, v.y);
      }
    }
  };
  auto side1 = [&](int wv) {
    if (dlate && dtj != 1) UpdateTileInPlace(BD, BS, BS, dti, dtj, lr, g);
  };
  PotrfPanels(BD, BX, inv_diag, flag, lane, w, side, side1);
  PP_CHOL_PHASE(10);
  StoreTile(S + nbase, BD, ld, tid);
  StoreTile(Minv + (size_t)(k + 1) * kNB * kNB, BX, kNB, tid);
  PP_CHOL_PHASE(11);
}

// The two workgroups that prepare the NEXT launch's chain inputs (see above); require k + 2 < T.  Both need the solved
// tile A_{k+2,k} and compute it themselves (an update + a solve: ~3.6 us of MFMA) rather than hand it over inside the
// launch; one workgroup doing everything was ~11 us of MFMA work on one CU and had become longer than the chain.
//   PrepX: A_{k+2,k} (stored), A_{k+1,k}, X' = (k+2,k+1) - A_{k+2,k-1} A_{k+1,k-1}^T - A_{k+2,k} A_{k+1,k}^T
//   PrepD: A_{k+2,k},           D' = (k+2,k+2) - A_{k+2,k-1} A_{k+2,k-1}^T - A_{k+2,k} A_{k+2,k}^T
// Every global load is issued before the first product (tiles that have no free LDS buffer yet wait in registers).
template <bool kIsX>
__device__ __forceinline__ void PrepBody(double* __restrict__ S, int ld, int k, const double* __restrict__ Minv, const double* __restrict__ xs_k,
                                         double* __restrict__ xs_next, int32_t* __restrict__ flag, double* Ba, double* Bb, double* Bc, double* Bm) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int ti = w >> 2, tj = w & 3, s = w & 3, ct = w >> 2;
  const bool prev = k > 0;
  const size_t row_k = (size_t)k * kNB * ld, row_k1 = (size_t)(k + 1) * kNB * ld, row_k2 = (size_t)(k + 2) * kNB * ld;
  const size_t col_km1 = (size_t)(k - 1) * kNB, col_k = (size_t)k * kNB, col_k1 = (size_t)(k + 1) * kNB, col_k2 = (size_t)(k + 2) * kNB;
  // D' tile of this wavefront (PrepD, wavefronts 0..9: the lower triangle of 16x16 tiles)
  int di = 0, dj = 0;
  if (!kIsX) { int rem = w; while (rem > di) { rem -= di + 1; ++di; } dj = rem; }
  const bool has_out = kIsX || w < 10;
  const size_t obase = kIsX ? row_k2 + col_k1 + (size_t)(16 * ti) * ld + 16 * tj : row_k2 + col_k2 + (size_t)(16 * di) * ld + 16 * dj;
  // ---- all global loads
  if (prev) LoadTiles2(Ba, S + row_k + col_km1, Bb, S + row_k2 + col_km1, ld, tid);     // A_{k,k-1}, A_{k+2,k-1}
  LoadTile(Bc, S + row_k2 + col_k, ld, tid);
  LoadTile(Bm, Minv + (size_t)k * kNB * kNB, kNB, tid);
  double2 x0, x1, q0, q1;     // PrepX: the staging copy of X = (k+1,k) and A_{k+1,k-1}
  if (kIsX) {
    x0 = TileLoad2(xs_k, kNB, tid, 0); x1 = TileLoad2(xs_k, kNB, tid, 1);
    if (prev) { q0 = TileLoad2(S + row_k1 + col_km1, ld, tid, 0); q1 = TileLoad2(S + row_k1 + col_km1, ld, tid, 1); }
  }
  v4f64 out = (v4f64){0.0, 0.0, 0.0, 0.0};
  if (has_out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = S[obase + (size_t)(g + 4 * i) * ld + lr];
  }
  __syncthreads();
  // PrepX overwrites tile (k+2,k) with its solved form while PrepD reads the unsolved one: PrepD's loads have all
  // returned here (they went through registers into LDS), which it announces in flag[1]; PrepX waits for that token
  // before its store (~4 us later; both workgroups are resident from the start of the launch: blockIdx 1 and 2)
  if (!kIsX && tid == 0) __hip_atomic_store(flag + 1, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // ---- A_{k+2,k}: panel k-1 update, then the solve
  if (prev) { UpdateTileInPlace(Bc, Bb, Ba, ti, tj, lr, g); __syncthreads(); }
  v4f64 x = SolveTile(Bc, Bm, s, ct, lr, g);
  if (!kIsX && prev && has_out) out = UpdateTileRegs(out, Bb, Bb, di, dj, lr, g);   // independent of the solve: fills its latency
  __syncthreads();
  TileStoreD(PP_TILE(Bc, s, ct), x, lr, g);
  if (kIsX) {
    // A_{k+1,k} from the staging copy of X (the chain workgroup stores it to S)
    TileStore2(Ba, tid, 0, x0); TileStore2(Ba, tid, 1, x1);
    if (tid == 0) {
      int spins = 0;
      while (__hip_atomic_load(flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k + 1 && spins < (1 << 20)) { __builtin_amdgcn_s_sleep(1); ++spins; }
      if (spins >= (1 << 20)) atomicOr(flag, 2);      // never observed; reported as a failed factorisation instead of a silent race
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) StoreThrough(S + row_k2 + col_k + (size_t)(16 * s + g + 4 * r) * ld + 16 * ct + lr, x[r]);
    x = SolveTile(Ba, Bm, s, ct, lr, g);
    __syncthreads();
    TileStoreD(PP_TILE(Ba, s, ct), x, lr, g);
    if (prev) { TileStore2(Bm, tid, 0, q0); TileStore2(Bm, tid, 1, q1); }      // A_{k+1,k-1} (M_k is no longer needed)
    __syncthreads();
    if (prev) out = UpdateTileRegs(out, Bb, Bm, ti, tj, lr, g);
    out = UpdateTileRegs(out, Bc, Ba, ti, tj, lr, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      StoreThrough(S + obase + (size_t)(g + 4 * i) * ld + lr, out[i]);
      StoreThrough(xs_next + (16 * ti + g + 4 * i) * kNB + 16 * tj + lr, out[i]);
    }
  } else {
    __syncthreads();
    if (has_out) {
      out = UpdateTileRegs(out, Bc, Bc, di, dj, lr, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) StoreThrough(S + obase + (size_t)(g + 4 * i) * ld + lr, out[i]);
    }
  }
}

// Block-sparse systems (lists != nullptr; see BuildSparseLists): the launch holds a solve workgroup only for the rows whose tile
// (i,k) is structurally non-zero in the factor, and an update workgroup only for the super-tiles that panel k-1 actually
// touches - lists[trsm_off ..) = the nT_list rows, lists[syrk_off ..) = one super-tile index u per remaining workgroup.
__global__ __launch_bounds__(kPanelThreads) void k_column_step(double* __restrict__ S, int ld, int k, int T, double* __restrict__ Minv, double* __restrict__ xs,
                                                               int32_t* __restrict__ flag, int skip_from, int double_from, const int32_t* __restrict__ lists,
                                                               int trsm_off, int nT_list, int syrk_off) {
  __shared__ __attribute__((aligned(16))) double smem[4 * kNB * kLS];   // registers already limit a CU to one such workgroup
  __shared__ double inv_diag[kNB];
  const int b = blockIdx.x;
  const int n_prep = (k + 2 < T) ? 2 : 0;
  const int nT = lists ? nT_list : (T - k - 3 > 0 ? T - k - 3 : 0);   // rows k+3 .. T-1 (row k+2 belongs to the prep workgroups)
  double* xs_k = xs + (size_t)(k & 1) * kNB * kNB;
  double* xs_next = xs + (size_t)((k + 1) & 1) * kNB * kNB;
  if (b == 0) {
    if (PP_CHOL_SKIPPED(0)) return;
    PP_CHOL_STAMP(20);
    PP_CHOL_LAUNCH(0, k);
    ChainBody(S, ld, k, T, Minv, xs_k, flag, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS, inv_diag);
    PP_CHOL_STAMP(21);
    PP_CHOL_LAUNCH(1, k);
  } else if (b <= n_prep) {
    if (PP_CHOL_SKIPPED(1)) return;
    if (b == 1) {
      PP_CHOL_STAMP(16);
      PrepBody<true>(S, ld, k, Minv, xs_k, xs_next, flag, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS);
      PP_CHOL_STAMP(17);
    } else {
      PP_CHOL_STAMP(24);
      PrepBody<false>(S, ld, k, Minv, xs_k, xs_next, flag, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS);
      PP_CHOL_STAMP(25);
    }
  } else if (b - n_prep <= nT) {
    if (PP_CHOL_SKIPPED(2)) return;
    if (b == 1 + n_prep) PP_CHOL_STAMP(22);
    const int row = lists ? lists[trsm_off + (b - n_prep - 1)] : k + 2 + (b - n_prep);
    TrsmTileBody<false>(S, S, ld, k, row, Minv, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS);
    if (b == 1 + n_prep) PP_CHOL_STAMP(23);
  }
  else if (k >= 1) {
    // trailing update by panel k-1 of the region below (k+1,k+1), except the three tiles the chain / prep workgroups own
    const int nW = (int)gridDim.x - 1 - n_prep - nT, q = b - 1 - n_prep - nT;
    if (PP_CHOL_SKIPPED(3)) return;
    if (q == nW - 1) PP_CHOL_STAMP(18);
    if (lists) SyrkSuperTiles<false>(S, S, ld, k - 1, T, lists[syrk_off + q], 1 << 30, skip_from, double_from, smem, smem + 2 * kNB * kLS);
    else SyrkSuperTiles<false>(S, S, ld, k - 1, T, q, nW, skip_from, double_from, smem, smem + 2 * kNB * kLS);
    if (q == nW - 1) PP_CHOL_STAMP(19);
  }
  PP_CHOL_LAUNCH(2, k);
}

// C (16 x 16 piece (ti, tj), D layout) = A B over K = 64, A and B 64 x 64 tiles in LDS (row stride kLS), four partial accumulators
__device__ __forceinline__ v4f64 TileProduct64(const double* A, const double* B, int ti, int tj, int lr, int g) {
  double av[16], bv[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) { av[kk] = A[(16 * ti + lr) * kLS + 4 * kk + g]; bv[kk] = B[(4 * kk + g) * kLS + 16 * tj + lr]; }
  return MfmaK16(av, bv, (v4f64){0.0, 0.0, 0.0, 0.0});
}
__device__ __forceinline__ void StoreTileRegs(double* __restrict__ dst, int ld, const v4f64& c, int ti, int tj, int lr, int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[(size_t)(16 * ti + g + 4 * i) * ld + 16 * tj + lr] = c[i];
}

// Pair gp, part 0: P_g (stored) and Z rows of block 2g+2, columns a; part 1: P_g again (not stored: two products are cheaper than a
// hand-over) and Z rows of block 2g+3, columns a; part 2: Z columns b of both rows.  The top pair has no Z.  `fetch_m(dst, k)` brings
// M_k into an LDS tile: a plain load after the factorisation (k_backsub_prepare), a mailbox fetch inside it (the task mode's
// kTaskPairPrep: the same arithmetic, hidden behind the factorisation).  Returns false if a bounded wait gave up.
template <typename FetchM>
__device__ __forceinline__ bool PairPrepBody(int gp, int part, int T, const double* __restrict__ L, int ld, double* __restrict__ Pw, double* __restrict__ Zw,
                                             double* B0, double* B1, double* B2, double* B3, FetchM fetch_m) {
  const int npairs = BacksubNumPairs(T);
  const int a = 2 * gp, b = a + 1, r0 = a + 2, r1 = a + 3;
  const bool has_z = gp + 1 < npairs;
  if (part > 0 && !has_z) return true;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4, ti = w >> 2, tj = w & 3;
  const size_t tile = (size_t)kNB * kNB;
  auto Ltile = [&](int i, int j) { return L + (size_t)i * kNB * ld + (size_t)j * kNB; };
  double* Z = Zw + (size_t)gp * 4 * tile;      // 128 x 128, row-major, row stride 128
  if (part == 2) {
    LoadTiles2(B2, Ltile(r0, b), B3, Ltile(r1, b), ld, tid);
    if (!fetch_m(B1, b)) return false;
    __syncthreads();
    StoreTileRegs(Z + kNB, 2 * kNB, TileProduct64(B2, B1, ti, tj, lr, g), ti, tj, lr, g);
    StoreTileRegs(Z + (size_t)kNB * 2 * kNB + kNB, 2 * kNB, TileProduct64(B3, B1, ti, tj, lr, g), ti, tj, lr, g);
    return true;
  }
  LoadTile(B0, Ltile(b, a), ld, tid);
  // the tiles of the second half travel with the first half's (registers until their LDS buffers are free)
  const int r = part == 0 ? r0 : r1;
  double2 la0 = make_double2(0.0, 0.0), la1 = la0, lb0 = la0, lb1 = la0;
  if (has_z) { la0 = TileLoad2(Ltile(r, a), ld, tid, 0); la1 = TileLoad2(Ltile(r, a), ld, tid, 1); lb0 = TileLoad2(Ltile(r, b), ld, tid, 0); lb1 = TileLoad2(Ltile(r, b), ld, tid, 1); }
  if (!fetch_m(B1, a) || !fetch_m(B2, b)) return false;
  __syncthreads();
  const v4f64 t1 = TileProduct64(B0, B1, ti, tj, lr, g);      // L_ba M_a
  __syncthreads();
  TileStoreD(PP_TILE(B0, ti, tj), t1, lr, g);
  if (has_z) { TileStore2(B3, tid, 0, lb0); TileStore2(B3, tid, 1, lb1); }
  __syncthreads();
  const v4f64 pv = -TileProduct64(B2, B0, ti, tj, lr, g);     // P = -M_b (L_ba M_a)
  if (part == 0) StoreTileRegs(Pw + (size_t)gp * tile, kNB, pv, ti, tj, lr, g);
  if (!has_z) return true;
  __syncthreads();
  TileStoreD(PP_TILE(B0, ti, tj), pv, lr, g);
  TileStore2(B2, tid, 0, la0); TileStore2(B2, tid, 1, la1);
  __syncthreads();
  // L_ra M_a + L_rb P, one product after the other: with both in one expression the scheduler fetched the operands of both (128 VGPRs)
  // before the first MFMA - the three spilled registers that were the only scratch use of the 128-VGPR kernels
  const v4f64 z1 = TileProduct64(B2, B1, ti, tj, lr, g);
  __builtin_amdgcn_sched_barrier(0);
  const v4f64 z = z1 + TileProduct64(B3, B0, ti, tj, lr, g);
  StoreTileRegs(Z + (size_t)(part == 0 ? 0 : kNB) * 2 * kNB, 2 * kNB, z, ti, tj, lr, g);
  return true;
}

// the per-column launch structure: one launch between the factorisation and the solve, grid = 3 npairs
__global__ __launch_bounds__(kPanelThreads) void k_backsub_prepare(const double* __restrict__ L, int ld, int T, const double* __restrict__ Linv,
                                                                   double* __restrict__ Pw, double* __restrict__ Zw) {
  __shared__ __attribute__((aligned(16))) double smem[4 * kNB * kLS];
  auto fetch_m = [&](double* dst, int k) { LoadTile(dst, Linv + (size_t)k * kNB * kNB, kNB, threadIdx.x); return true; };
  (void)PairPrepBody(blockIdx.x / 3, blockIdx.x % 3, T, L, ld, Pw, Zw, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS, fetch_m);
}

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
constexpr unsigned long long kPoison = 0xFFFFFFFFFFFFFFFFull;

// mailboxes of one factorisation: 64x64 row-major slots (stride 64), one per step
struct Mailboxes {
  double* Minv;   // [T]    M_k       chain(k-1) -> PrepX(k), PrepD(k), the solve tasks of column k
  double* xs;     // [T+1]  X of chain(k) = tile (k+1,k), panels <= k-1 applied          PrepX(k-1) -> chain(k)
  double* ds;     // [T+1]  D of chain(k) = tile (k+1,k+1), panels <= k-1 applied        PrepD(k-1) -> chain(k)
  double* xsol;   // [T+1]  the solved tile (k+1,k)                                      chain(k) -> PrepX(k)
  double* Pw;     // pair inverses and pair couplings of the paired back substitution (kTaskPairPrep -> k_backsub_pairs)
  double* Zw;
};

__device__ __forceinline__ void WaitOwnStores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// every store of a task is a write-through store: once this workgroup's have been acknowledged a counter may move
__device__ __forceinline__ void TaskStoresDone() {
  WaitOwnStores();
  __syncthreads();
}
__device__ __forceinline__ bool IsPoison(double v) { return (unsigned long long)__double_as_longlong(v) == kPoison; }
// a result that happens to be the mailbox pattern (only a NaN can be) is stored as another NaN
__device__ __forceinline__ void StoreMail(double* p, double v) { StoreThrough(p, IsPoison(v) ? __longlong_as_double(0x7FF8000000000000ll) : v); }

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
  const double2 c0 = TileLoad2T<true>(S + row_k2 + col_k, ld, tid, 0), c1 = TileLoad2T<true>(S + row_k2 + col_k, ld, tid, 1);
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
  auto products = [&]() {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double a0v = ar[4 * kk], a1v = ar[16 * kLS + 4 * kk], b0v = br[4 * kk], b1v = br[16 * kLS + 4 * kk];
      p[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b0v, p[0][0], 0, 0, 0);
      p[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0v, b1v, p[0][1], 0, 0, 0);
      p[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b0v, p[1][0], 0, 0, 0);
      p[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1v, b1v, p[1][1], 0, 0, 0);
    }
  };
  if (valid) products();
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
    if (valid) products();
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
  const double2 x0 = TileLoad2T<true>(S + pbase, ld, tid, 0), x1 = TileLoad2T<true>(S + pbase, ld, tid, 1);
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

// Back substitution L^T x = y (y = row rhs_row of the factor) in ONE launch: workgroup j owns the 64 unknowns of
// block j, applies  y_j -= L[k-block, j-block]^T x_k  for k = T-1 .. j+1 as the x_k arrive, then solves its block
// with the precomputed L_jj^-1 and publishes x_j.  The 47 dependent launches of a per-block kernel cost ~5.7 us
// each (launch boundary + two dependent global round trips); here a step of the chain is one 8-byte-granule
// hand-off (x values are their own ready flags: the buffer is preset to an all-ones NaN pattern and written with
// write-through agent-scope stores, read with agent-scope loads — MI355X_MICROARCH.md, inter-workgroup visibility).
// A workgroup only ever waits on HIGHER block indices, which are given the lower blockIdx (dispatched first),
// so the wait cannot deadlock even if not all workgroups are resident; every spin is bounded.
constexpr unsigned long long kNotReady = 0xFFFFFFFFFFFFFFFFull;
// nz (may be null): T x T bytes, nz[k T + j] = tile (k,j) of the factor is structurally non-zero - the others are skipped (a
// block-sparse factor: block j only waits for the x_k it is coupled to)
__global__ __launch_bounds__(256) void k_backsub_all(const double* __restrict__ S, int ld, int T, int rhs_row, const double* __restrict__ Linv,
                                                     double* x_out, int32_t* __restrict__ flag, const uint8_t* __restrict__ nz) {
  __shared__ double part[4][kNB];
  __shared__ double ys[kNB];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int j = T - 1 - (int)blockIdx.x;
  // this thread's slice of L_jj^-1: rows 16q .. 16q+15, column c
  double linv[16];
  {
    const double* Lb = Linv + (size_t)j * kNB * kNB;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) linv[rr] = Lb[(16 * q + rr) * kNB + c];
  }
  double acc = 0.0;
  bool dead = false;    // a lane whose wait timed out stops waiting: the solve is reported invalid instead of hanging
  for (int k = T - 1; k > j; --k) {
    if (nz && !nz[(size_t)k * T + j]) continue;
    double lt[16];
    const double* Lt = S + ((size_t)k * kNB + 16 * q) * ld + (size_t)j * kNB + c;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) lt[rr] = Lt[(size_t)rr * ld];
    // lanes 0..15 of every wavefront poll the 16 values of x_k this wavefront needs
    double xv = 0.0;
    if (c < 16) {
      unsigned long long* src = reinterpret_cast<unsigned long long*>(x_out + (size_t)k * kNB + 16 * q + c);
      unsigned long long bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int spins = 0;
      while (bits == kNotReady && !dead && spins < (1 << 18)) {
        __builtin_amdgcn_s_sleep(1);
        bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++spins;
      }
      if (bits == kNotReady) { if (!dead) atomicOr(flag, 4); dead = true; bits = 0ull; }
      xv = __longlong_as_double((long long)bits);
    }
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;      // four short chains instead of one 16-deep one (this is the hop's critical path)
#pragma unroll
    for (int rr = 0; rr < 16; rr += 4) {
      p0 = fma(lt[rr], ReadLane(xv, rr), p0); p1 = fma(lt[rr + 1], ReadLane(xv, rr + 1), p1);
      p2 = fma(lt[rr + 2], ReadLane(xv, rr + 2), p2); p3 = fma(lt[rr + 3], ReadLane(xv, rr + 3), p3);
    }
    acc += (p0 + p1) + (p2 + p3);
  }
  part[q][c] = acc;
  __syncthreads();
  if (tid < kNB) {
    const int col = j * kNB + tid;
    const double y = (col < rhs_row) ? S[(size_t)rhs_row * ld + col] : 0.0;   // padding / the rhs row's own diagonal carry no unknown
    ys[tid] = y - ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]));
  }
  __syncthreads();
  {  // x[c] = sum_r Linv[r][c] * y[r]  (L^-T y), 4 partial sums over r
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int rr = 0; rr < 16; rr += 4) {
      s0 = fma(linv[rr], ys[16 * q + rr], s0); s1 = fma(linv[rr + 1], ys[16 * q + rr + 1], s1);
      s2 = fma(linv[rr + 2], ys[16 * q + rr + 2], s2); s3 = fma(linv[rr + 3], ys[16 * q + rr + 3], s3);
    }
    part[q][c] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  if (tid < kNB) {
    const double v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if (bits == kNotReady) bits = 0x7FF8000000000000ull;    // a NaN result stays a NaN, never the not-ready pattern
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(x_out + (size_t)j * kNB + tid), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- paired back substitution (dense systems) --------------------------------------------------------------------------------
// k_backsub_all pays one memory hand-off (~1.0 us: the store's visibility + a poll round trip) and two dependent mat-vec stages per
// 64-block: 47 x 1.3 us = 62 us.  Here two consecutive blocks a = 2g, b = 2g + 1 form a PAIR solved by one workgroup in ONE stage
// after its newest inputs arrive:
//     x_ab = G^T u  -  Z^T x_new,        G = [M_a 0; P M_b] = the inverse of the pair's 128 x 128 diagonal factor, P = -M_b L_ba M_a,
//                                        u = y_ab - sum over the blocks BEYOND the next pair of L_k,ab^T x_k      (known a hop earlier),
//                                        Z = L_new,ab G   (128 x 128; new = the pair above, blocks 2g+2, 2g+3)
// so the critical path of a hop is the hand-off + one 128 x 128 mat-vec, and there are half as many hops: 22 pairs + the three or four
// top blocks (solved singly, as in k_backsub_all: their inverses are the last thing the factorisation produces) = ~33 us.
// P and Z are 8 products of 64 x 64 tiles per pair, computed by k_backsub_prepare in one launch between the factorisation and the
// solve (three workgroups per pair, ~4 us): the same kernels in both launch structures, so their solutions stay bitwise equal.
// Block-sparse systems keep k_backsub_all (it skips the structurally zero tiles).
constexpr int kPairThreads = 1024;
__device__ __forceinline__ double PollReady(const double* p, int32_t* flag, bool* dead) {
  unsigned long long* src = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(p));
  unsigned long long bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int spins = 0;
  while (bits == kNotReady && !*dead && spins < (1 << 18)) {
    __builtin_amdgcn_s_sleep(1);
    bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++spins;
  }
  if (bits == kNotReady) { if (!*dead) atomicOr(flag, 4); *dead = true; bits = 0ull; }
  return __longlong_as_double((long long)bits);
}
// two values per lane with BOTH requests in flight before either is looked at (two PollReady calls in a row are two round trips)
__device__ __forceinline__ void PollReady2(const double* pa, const double* pb, int32_t* flag, bool* dead, double* va, double* vb) {
  unsigned long long* sa = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(pa));
  unsigned long long* sb = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(pb));
  unsigned long long a = __hip_atomic_load(sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b = __hip_atomic_load(sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int spins = 0;
  while ((a == kNotReady || b == kNotReady) && !*dead && spins < (1 << 18)) {
    __builtin_amdgcn_s_sleep(1);
    a = __hip_atomic_load(sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); b = __hip_atomic_load(sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++spins;
  }
  if (a == kNotReady || b == kNotReady) { if (!*dead) atomicOr(flag, 4); *dead = true; a = 0ull; b = 0ull; }
  *va = __longlong_as_double((long long)a); *vb = __longlong_as_double((long long)b);
}
__device__ __forceinline__ void PublishX(double* p, double v) {
  unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  if (bits == kNotReady) bits = 0x7FF8000000000000ull;    // a NaN result stays a NaN, never the not-ready pattern
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid = nsingles + npairs: the top blocks first (T-1 downwards), then the pairs from the top one down - a workgroup only waits for
// workgroups with a lower blockIdx.  Thread (c, q): c = tid & 127 the unknown inside the pair (block a: 0..63, block b: 64..127),
// q = tid >> 7 = 0..7 the slice of rows it sums over.
__global__ __launch_bounds__(kPairThreads) void k_backsub_pairs(const double* __restrict__ S, int ld, int T, int rhs_row, const double* __restrict__ Linv,
                                                                const double* __restrict__ Pw, const double* __restrict__ Zw, double* x_out,
                                                                int32_t* __restrict__ flag) {
  __shared__ double part[8][2 * kNB];
  __shared__ double us[2 * kNB];
  const int tid = threadIdx.x, lane = tid & 63, c = tid & 127, q = tid >> 7;
  const int npairs = BacksubNumPairs(T), nsingles = T - 2 * npairs;
  const size_t tile = (size_t)kNB * kNB;
  bool dead = false;
  if ((int)blockIdx.x < nsingles) {
    // ---- one of the top blocks, as k_backsub_all (threads (c < 64, q): 8 rows each)
    const int j = T - 1 - (int)blockIdx.x;
    const bool act = c < kNB;
    PP_BS_STAMP(0, j);
    double linv[8];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) linv[rr] = act ? Linv[(size_t)j * tile + (size_t)(8 * q + rr) * kNB + c] : 0.0;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) asm volatile("" : "+v"(linv[rr]));      // (in registers before the waiting starts, see the pairs below)
    double acc = 0.0;
    for (int k = T - 1; k > j; --k) {
      double lt[8];
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) lt[rr] = act ? S[((size_t)k * kNB + 8 * q + rr) * ld + (size_t)j * kNB + c] : 0.0;
      const double xv = (lane < 8 && act) ? PollReady(x_out + (size_t)k * kNB + 8 * q + lane, flag, &dead) : 0.0;      // (`act` is wave-uniform: the idle half does not poll)
      double p0 = 0.0, p1 = 0.0;
#pragma unroll
      for (int rr = 0; rr < 8; rr += 2) { p0 = fma(lt[rr], ReadLane(xv, rr), p0); p1 = fma(lt[rr + 1], ReadLane(xv, rr + 1), p1); }
      acc += p0 + p1;
    }
    part[q][c] = acc;
    __syncthreads();
    if (tid < kNB) {
      const int col = j * kNB + tid;
      const double y = (col < rhs_row) ? S[(size_t)rhs_row * ld + col] : 0.0;
      double sum = 0.0;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) sum += part[qq][tid];
      us[tid] = y - sum;
    }
    __syncthreads();
    {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int rr = 0; rr < 8; rr += 2) { s0 = fma(linv[rr], us[8 * q + rr], s0); s1 = fma(linv[rr + 1], us[8 * q + rr + 1], s1); }
      part[q][c] = s0 + s1;
    }
    __syncthreads();
    if (tid < kNB) {
      double v = 0.0;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) v += part[qq][tid];
      PublishX(x_out + (size_t)j * kNB + tid, v);
    }
    PP_BS_STAMP(3, j);
    return;
  }
  // ---- a pair
  const int gp = npairs - 1 - ((int)blockIdx.x - nsingles);
  const int a = 2 * gp;
  const bool has_z = gp + 1 < npairs;
  const int first_far = has_z ? a + 4 : a + 2;      // blocks >= first_far enter through their tiles of L; the pair above through Z
  PP_BS_STAMP(0, a);
  // G = [M_a 0; P M_b] goes to LDS (96 KB; the workgroup has the CU to itself anyway), this thread's slice of Z (rows 16q .. 16q+15 of
  // 128, column c) to registers: Z is what the hop's critical path multiplies with, and it must be THERE before the waiting starts -
  // left to itself the compiler sinks the loads to their first use, behind the poll of the newest input (2.7 us per hop).  With G's
  // slices in registers as well the kernel spilled (128 VGPRs at 1024 threads): every use of a spilled slice was a scratch load.
  __shared__ double Gs[3 * kNB * kNB];      // M_a | P | M_b, row-major 64 x 64 each
  double z[16];
  double y_rhs = 0.0;      // this thread's entry of the right-hand side (threads 0..127), fetched now: it is needed on the two-hop cycle below
  if (tid < 2 * kNB) { const int col = a * kNB + tid; y_rhs = (col < rhs_row) ? S[(size_t)rhs_row * ld + col] : 0.0; }
  {
    const double* Ma = Linv + (size_t)a * tile;
    const double* P = Pw + (size_t)gp * tile;
    for (int i = tid; i < (int)tile; i += kPairThreads) { Gs[i] = Ma[i]; Gs[tile + i] = P[i]; Gs[2 * tile + i] = Ma[tile + i]; }
    if (has_z) {
      const double* Z = Zw + (size_t)gp * 4 * tile;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) z[rr] = Z[(size_t)(16 * q + rr) * 2 * kNB + c];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) asm volatile("" : "+v"(z[rr]));
    }
    asm volatile("" : "+v"(y_rhs));
  }
  // Far terms, one ARRIVAL at a time: the blocks above arrive singly while they are the top singles and two at a time below (a pair
  // publishes both its blocks at once).  Both blocks of an arrival are polled together (lanes 0..7 / 8..15: ONE memory round trip) and
  // the tile slices of the next arrival are requested before this one's are used.  This loop and the G^T u stage after it are on a
  // two-hop cycle (x of pair g+2 -> far terms and G^T u of pair g -> ready for x of pair g+1): block by block with a poll round trip and a
  // tile fetch per block, and the right-hand side fetched only when needed, the cycle was 5.8 us and a hop 2.9 us (tools/chol_task_trace.hip, PP_BS_TRACE).
  double acc = 0.0;
  auto load_slice = [&](int k, double (&lt)[8]) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) lt[rr] = S[((size_t)k * kNB + 8 * q + rr) * ld + (size_t)a * kNB + c];
  };
  auto use_slice = [&](const double (&lt)[8], const double* xb) {
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int rr = 0; rr < 8; rr += 2) { p0 = fma(lt[rr], xb[8 * q + rr], p0); p1 = fma(lt[rr + 1], xb[8 * q + rr + 1], p1); }
    acc += p0 + p1;
  };
  // Only wavefront 0 polls (lane = unknown; two values per lane for a two-block arrival) and hands the values over through LDS: with
  // every wavefront of every waiting workgroup polling its own slice (22 x 16 wavefronts on the same few lines, each poll a transaction
  // below the L2s) the slowest of a workgroup's sixteen polls came back 1-2 us after the fastest, and the barrier waits for the slowest.
  __shared__ double xs[2][2 * kNB];      // double-buffered: the next arrival may be written while slow wavefronts still read this one
  {
    const int top_pairs_block = 2 * npairs - 1;      // highest block that belongs to a pair
    int k = T - 1, buf = 0;
    while (k >= first_far) {
      const int n = k > top_pairs_block ? 1 : 2;
      double cur0[8], cur1[8];      // the tile slices travel with the poll (both a memory round trip)
      load_slice(k, cur0);
      if (n == 2) load_slice(k - 1, cur1);
      if (tid < kNB) {
        if (n == 2) PollReady2(x_out + (size_t)k * kNB + tid, x_out + (size_t)(k - 1) * kNB + tid, flag, &dead, &xs[buf][tid], &xs[buf][kNB + tid]);
        else xs[buf][tid] = PollReady(x_out + (size_t)k * kNB + tid, flag, &dead);
      }
      __syncthreads();
      use_slice(cur0, xs[buf]);
      if (n == 2) use_slice(cur1, xs[buf] + kNB);
      k -= n; buf ^= 1;
    }
  }
  PP_BS_STAMP(1, a);
  part[q][c] = acc;
  __syncthreads();
  if (tid < 2 * kNB) {
    double sum = 0.0;
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) sum += part[qq][tid];
    us[tid] = y_rhs - sum;
  }
  __syncthreads();
  {      // G^T u:  x_a = M_a^T u_a + P^T u_b,  x_b = M_b^T u_b  (this thread: rows 8q .. 8q+7)
    double s0 = 0.0, s1 = 0.0;
    if (c < kNB) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) { const int r = 8 * q + rr; s0 = fma(Gs[r * kNB + c], us[r], s0); s1 = fma(Gs[tile + r * kNB + c], us[kNB + r], s1); }
    } else {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) { const int r = 8 * q + rr; s1 = fma(Gs[2 * tile + r * kNB + (c - kNB)], us[kNB + r], s1); }
    }
    part[q][c] = s0 + s1;
  }
  __syncthreads();
  double v = 0.0;
  if (tid < 2 * kNB) {
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) v += part[qq][tid];
  }
  if (has_z) {
    PP_BS_STAMP(4, a);
    if (tid < kNB) {      // the pair above: wavefront 0 polls its 128 values
      PollReady2(x_out + (size_t)(a + 2) * kNB + tid, x_out + (size_t)(a + 3) * kNB + tid, flag, &dead, &xs[0][tid], &xs[0][kNB + tid]);
    }
    __syncthreads();      // (also: part is reused below)
    PP_BS_STAMP(2, a);
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
    for (int rr = 0; rr < 16; rr += 4) {
      p0 = fma(z[rr], xs[0][16 * q + rr], p0); p1 = fma(z[rr + 1], xs[0][16 * q + rr + 1], p1);
      p2 = fma(z[rr + 2], xs[0][16 * q + rr + 2], p2); p3 = fma(z[rr + 3], xs[0][16 * q + rr + 3], p3);
    }
    part[q][c] = (p0 + p1) + (p2 + p3);
    __syncthreads();
    if (tid < 2 * kNB) {
      double sum = 0.0;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) sum += part[qq][tid];
      v -= sum;
    }
  }
  if (tid < 2 * kNB) PublishX(x_out + (size_t)a * kNB + tid, v);
  PP_BS_STAMP(3, a);
}

// (Four consecutive blocks per workgroup - 12 hand-offs between workgroups instead of 47, the hops inside a group through LDS - was
// measured at 98 us against 62 us: the x_k of the group above arrive as a burst, and the 4 x 4 tiles they multiply (512 KB) have no
// place on the CU to wait in, so their loads queue up behind each other on the critical path; see DESIGN.md.)

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
  ChainTask* tasks = nullptr;             // the one-launch path: the sorted task list for tasks_T block columns (device memory)
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
  if (st->sparse_lists) { (void)hipFree(st->sparse_lists); st->sparse_lists = nullptr; }
  if (st->sparse_nz) { (void)hipFree(st->sparse_nz); st->sparse_nz = nullptr; }
  const uint8_t* nz = st->tile_nz;
  SparseColumnLists lists = BuildSparseColumnLists(T, nz);
  st->sparse_host.swap(lists.lists);
  st->sparse_base_rows = lists.base_rows; st->sparse_base_sups = lists.base_sups;
  PP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st->sparse_lists), sizeof(int32_t) * std::max<size_t>(st->sparse_host.size(), 1)));
  PP_HIP_TRY(hipMemcpyAsync(st->sparse_lists, st->sparse_host.data(), sizeof(int32_t) * st->sparse_host.size(), hipMemcpyHostToDevice, strm));
  PP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st->sparse_nz), (size_t)T * T));
  PP_HIP_TRY(hipMemcpyAsync(st->sparse_nz, nz, (size_t)T * T, hipMemcpyHostToDevice, strm));
  PP_HIP_TRY(hipStreamSynchronize(strm));      // (the caller's stream, not the legacy one: another host thread may be capturing its own factorisation)
  st->sparse_T = T;
  return PP_OK;
}

// The sizes of the one-launch path, dense or block-sparse: up to kMaxSteps block columns, the whole range of its counter arrays (round 2 stopped at 88 - equal
// at n = 6000, slower at 8000; with the two-panel updates of round 3: n = 3000 0.68 against 0.83 ms, 4000 1.08 / 1.36, 6000 2.57 / 3.00, 8000 5.53 / 5.96 -
// tools/chol_time.py)
static bool UseTasks(int T) { return T >= 4 && T <= kMaxSteps; }

int CholeskyPlanSteps(int T, const uint8_t* nz, const Switches& sw, int* chains) {
  if (chains) *chains = 1;
  if (!nz || !UseTasks(T)) return T;
  const ChainPlan plan = PlanChains(T, nz, sw.plan);
  if (chains) *chains = plan.cr.n;
  return plan.Steps();
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
  if (st->tasks) { (void)hipFree(st->tasks); st->tasks = nullptr; }
  if (st->tasks_nz) { (void)hipFree(st->tasks_nz); st->tasks_nz = nullptr; }
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
  if (src) {
    PP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st->tasks_nz), plan.map.size()));
    PP_HIP_TRY(hipMemcpyAsync(st->tasks_nz, plan.map.data(), plan.map.size(), hipMemcpyHostToDevice, strm));
  }
  // (measured and dropped in round 6, PPSFM_CHOL_QUIET_XCD: an empty task at every list position whose workgroup lands on the chain's XCD - a quieter L2 /
  // fabric port for the chain, a seventh less of the chip for the bulk: 705-720 -> 721-731 us per factorisation + back substitution, 809 -> 824 us per LM iteration)
  const std::vector<ChainTask>* to_upload = &cp.list;
  PP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st->tasks), sizeof(ChainTask) * to_upload->size()));
  // (on the caller's stream, not the legacy one: another host thread may be capturing its own factorisation just now)
  PP_HIP_TRY(hipMemcpyAsync(st->tasks, to_upload->data(), sizeof(ChainTask) * to_upload->size(), hipMemcpyHostToDevice, strm));
  PP_HIP_TRY(hipStreamSynchronize(strm));
  st->num_tasks = (int)to_upload->size();
  // several chains: the pool of 64 x 64 scratch tiles in which a chain accumulates for another chain's tiles
  if (cp.scratch_tiles > st->scratch_tiles) {
    if (st->scratch) { PoolDeviceFree(st->scratch); st->scratch = nullptr; st->scratch_tiles = 0; }      // (recycled blocks: resource_pool.hpp)
    { const int rc = PoolDeviceAlloc(reinterpret_cast<void**>(&st->scratch), sizeof(double) * (size_t)cp.scratch_tiles * kNB * kNB); if (rc) return rc; }
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
  if (nz || npairs == 0 || !pairs) {
    hipLaunchKernelGGL(k_backsub_all, dim3(T), dim3(256), 0, s, Lw, N, T, rhs_row, (const double*)Linv_ws, x_out, d_flag, nz);
    return;
  }
  const size_t tile = (size_t)kNB * kNB;
  double* Pw = Linv_ws + (size_t)(4 * T + 3) * tile + 8192;      // behind the mailboxes and the counters (CholeskyWorkspaceDoubles)
  double* Zw = Pw + (size_t)npairs * tile;
  if (!prepared) hipLaunchKernelGGL(k_backsub_prepare, dim3(3 * npairs), dim3(kPanelThreads), 0, s, Lw, N, T, (const double*)Linv_ws, Pw, Zw);
  hipLaunchKernelGGL(k_backsub_pairs, dim3(T - 2 * npairs + npairs), dim3(kPairThreads), 0, s, Lw, N, T, rhs_row, (const double*)Linv_ws, (const double*)Pw,
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
// Linv_ws: [0, N*64) L_kk^-1 (row-major 64x64) of every diagonal block = the M_k mailboxes (solves + back substitution), then T+1
// staging slots for the chain's X tile (per-column mode uses two of them in turn; task mode: one mailbox per step), then the D and
// solved-X mailboxes of task mode (T+1 slots each), then the progress counters of task mode.
// Lfac: the solved-tile array of task mode, N x N like S.
static int EnqueueCholesky(const CholeskyState& st) {
  double *S = st.sys.S, *Linv_ws = st.sys.Linv_ws, *Lfac = st.sys.Lfac, *x_out = st.sys.x;
  int32_t* d_flag = st.sys.flag;
  const hipStream_t s = st.sys.stream;
  const int N = st.sys.N, rhs_row = st.sys.rhs_row, T = N / kNB;
  const size_t tile = (size_t)kNB * kNB;
  if (st.path == CholPath::Small) {
    hipLaunchKernelGGL(k_small_cholesky, dim3(1), dim3(kPanelThreads), 0, s, (const double*)S, N, rhs_row, x_out, d_flag);
    PP_HIP_TRY(hipGetLastError());
    return PP_OK;
  }
  Mailboxes mb;
  mb.Minv = Linv_ws; mb.xs = Linv_ws + (size_t)T * tile; mb.ds = mb.xs + (size_t)(T + 1) * tile; mb.xsol = mb.ds + (size_t)(T + 1) * tile;
  double* xs = mb.xs;
  int32_t* ctr = reinterpret_cast<int32_t*>(mb.xsol + (size_t)(T + 1) * tile);
  mb.Pw = Linv_ws + (size_t)(4 * T + 3) * tile + 8192;      // behind the mailboxes and the counters (CholeskyWorkspaceDoubles)
  mb.Zw = mb.Pw + (size_t)BacksubNumPairs(T) * tile;
  const bool tasks = st.path == CholPath::Tasks, sparse = st.path == CholPath::SparseColumns;
  const ChainRanges cr = tasks ? st.chains : OneChain(T);
  hipLaunchKernelGGL(k_potrf64, dim3(tasks ? 64 + cr.n : 1), dim3(kPanelThreads), 0, s, S, N, Linv_ws, xs, d_flag, x_out, tasks ? Lfac : S, ctr, (int)kNumCounters, Linv_ws,
                     (long long)((size_t)(4 * T + 3) * tile), cr);
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
      hipLaunchKernelGGL(k_column_step, dim3(1 + n_prep + nTs + nWs), dim3(kPanelThreads), 0, s, S, N, k, T, Linv_ws, xs, d_flag, kNever, kNever,
                         (const int32_t*)st.sparse_lists, st.sparse_base_rows + h[k], nTs, st.sparse_base_sups + h[T + 1 + k]);
      continue;
    }
    if (double_from == kNever && k >= 1 && nsup > kDeferAbove && k + 6 < T && k + 2 < T - 1) { skip_from = k + 6; pending_double = k + 6; }
    hipLaunchKernelGGL(k_column_step, dim3(1 + n_prep + nT + nW), dim3(kPanelThreads), 0, s, S, N, k, T, Linv_ws, xs, d_flag, skip_from, double_from,
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
  if (st->tasks) (void)hipFree(st->tasks);
  if (st->tasks_nz) (void)hipFree(st->tasks_nz);
  if (st->scratch) PoolDeviceFree(st->scratch);
  if (st->sparse_lists) (void)hipFree(st->sparse_lists);
  if (st->sparse_nz) (void)hipFree(st->sparse_nz);
  delete st;
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
    if (st->sparse_lists) { (void)hipFree(st->sparse_lists); st->sparse_lists = nullptr; }
    if (st->sparse_nz) { (void)hipFree(st->sparse_nz); st->sparse_nz = nullptr; }
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
  *diag_inverses = st->sys.Linv_ws;
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
