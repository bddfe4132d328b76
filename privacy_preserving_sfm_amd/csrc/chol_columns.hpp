// K3b, the per-column launch structure of the dense fp64 Cholesky (cholesky.hip, "column mode"): device code only, included by cholesky.hip alone (one
// translation unit: the kernels are launched by name from there and from the tools that include cholesky.hip whole).
//   k_potrf64       the launch in front of BOTH launch structures: the first diagonal block of every chain, and for task mode (chol_tasks.hpp) the reset
//                   of its counters and mailboxes - it lives here because it is launch "-1" of the per-column sequence and shares nothing with the tasks
//   k_column_step   one launch per block column: the chain workgroup (ChainBody), the two prep workgroups (PrepBody), the solves of column k
//                   (TrsmTileBody) and the trailing update by panel k-1 (SyrkSuperTiles)
// The building blocks (tiles in LDS, PotrfPanels, the super-tile products) are chol_block.hpp's; the lists of the block-sparse launches are chol_plan.hpp's.
#pragma once
#include "chol_block.hpp"
#include "chol_plan.hpp"

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
    const double pattern = __longlong_as_double((long long)kNotReady);
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
    if (x_out) for (int i = tid; i < ld; i += kPanelThreads) __hip_atomic_store(reinterpret_cast<unsigned long long*>(x_out + i), kNotReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
__device__ __forceinline__ void SyrkSuperTiles(double* S, int ld, int kp, int T, int q, int nW, int skip_from, int double_from, double* As, double* Bs) {
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
        const double* a0 = S + (size_t)bi0 * kNB * ld + col;
        const double* b0 = S + (size_t)bj0 * kNB * ld + col;
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
            for (int i = 0; i < 4; ++i) c[a][b][i] = S[cbase + (size_t)(16 * a + 4 * i) * ld + 16 * b];
      }
      __syncthreads();
      if (valid) SuperTileProducts(p, As + (32 * wi + lr) * kLS + lk, Bs + (32 * wj + lr) * kLS + lk);
    }
    if (valid) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int i = 0; i < 4; ++i)      // write-through: 30 MB of dirty lines per launch would otherwise be flushed at the kernel boundary, on the critical path
            StoreThrough(S + cbase + (size_t)(16 * a + 4 * i) * ld + 16 * b, c[a][b][i] - p[a][b][i]);
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

__device__ __forceinline__ void TrsmTileBody(double* S, int ld, int k, int i, const double* __restrict__ Minv, double* BX, double* Mk, double* B1, double* B2) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, g = lane >> 4;
  const size_t dbase = (size_t)k * kNB * ld + (size_t)k * kNB, pbase = (size_t)i * kNB * ld + (size_t)k * kNB;
  const double* mk = Minv + (size_t)k * kNB * kNB;
  if (k > 0) {
    // X, A_{i,k-1}, A_{k,k-1} (row stride ld) and M_k (row stride 64)
    LoadTiles2(BX, S + pbase, B1, S + pbase - kNB, ld, tid);
    LoadTile(B2, S + dbase - kNB, ld, tid);
    LoadTile(Mk, mk, kNB, tid);
    __syncthreads();
    UpdateTileInPlace(BX, B1, B2, w >> 2, w & 3, lr, g);
  } else {
    LoadTile(BX, S + pbase, ld, tid);
    LoadTile(Mk, mk, kNB, tid);
  }
  __syncthreads();
  const int s = w & 3, ct = w >> 2;    // SIMD (w & 3) gets one tile of every column tile: balanced MFMA load
  const v4f64 x = SolveTile(BX, Mk, s, ct, lr, g);
#pragma unroll
  for (int r = 0; r < 4; ++r) StoreThrough(S + pbase + (size_t)(16 * s + g + 4 * r) * ld + 16 * ct + lr, x[r]);
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
    TrsmTileBody(S, ld, k, row, Minv, smem, smem + kNB * kLS, smem + 2 * kNB * kLS, smem + 3 * kNB * kLS);
    if (b == 1 + n_prep) PP_CHOL_STAMP(23);
  }
  else if (k >= 1) {
    // trailing update by panel k-1 of the region below (k+1,k+1), except the three tiles the chain / prep workgroups own
    const int nW = (int)gridDim.x - 1 - n_prep - nT, q = b - 1 - n_prep - nT;
    if (PP_CHOL_SKIPPED(3)) return;
    if (q == nW - 1) PP_CHOL_STAMP(18);
    if (lists) SyrkSuperTiles(S, ld, k - 1, T, lists[syrk_off + q], 1 << 30, skip_from, double_from, smem, smem + 2 * kNB * kLS);
    else SyrkSuperTiles(S, ld, k - 1, T, q, nW, skip_from, double_from, smem, smem + 2 * kNB * kLS);
    if (q == nW - 1) PP_CHOL_STAMP(19);
  }
  PP_CHOL_LAUNCH(2, k);
}

}  // namespace ppsfm
