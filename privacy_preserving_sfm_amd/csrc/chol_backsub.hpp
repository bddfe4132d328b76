// K3b, the back substitution L^T x = y of the dense fp64 Cholesky (cholesky.hip: LaunchBacksub): device code only, included by cholesky.hip alone.
//   k_backsub_all                          block by block in one launch (block-sparse factors, small systems, PPSFM_BACKSUB_PAIRS=0)
//   k_backsub_prepare + k_backsub_pairs    two blocks per hop (dense factors); the preparation's body (PairPrepBody) also runs as the kTaskPairPrep tasks
//                                          of the one-launch factorisation (chol_tasks.hpp), hidden behind it
#pragma once
#include "chol_block.hpp"
#include "chol_plan.hpp"

namespace ppsfm {

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

// Back substitution L^T x = y (y = row rhs_row of the factor) in ONE launch: workgroup j owns the 64 unknowns of
// block j, applies  y_j -= L[k-block, j-block]^T x_k  for k = T-1 .. j+1 as the x_k arrive, then solves its block
// with the precomputed L_jj^-1 and publishes x_j.  The 47 dependent launches of a per-block kernel cost ~5.7 us
// each (launch boundary + two dependent global round trips); here a step of the chain is one 8-byte-granule
// hand-off (x values are their own ready flags: the buffer is preset to an all-ones NaN pattern and written with
// write-through agent-scope stores, read with agent-scope loads — MI355X_MICROARCH.md, inter-workgroup visibility).
// A workgroup only ever waits on HIGHER block indices, which are given the lower blockIdx (dispatched first),
// so the wait cannot deadlock even if not all workgroups are resident; every spin is bounded.
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
    if (bits == kNotReady) bits = kNotReadyNaN;    // a NaN result stays a NaN, never the not-ready pattern
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
  if (bits == kNotReady) bits = kNotReadyNaN;    // a NaN result stays a NaN, never the not-ready pattern
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

}  // namespace ppsfm
