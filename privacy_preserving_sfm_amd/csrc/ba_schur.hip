// K3a: the Schur assembly of an LM attempt - from K2's blocks (U, g_c, V, g_p: ba_step.hip) and the trust-region radius to the damped reduced camera
// system S (lower triangle + rhs row) that K3b factorises, or an iterative handle's diagonal blocks and right-hand side (ba_pcg.hip).
//
//   k_prepare            one launch, two roles: per point (V_p + D_p^2)^-1 and V^-1 b_p for the current trust-region radius; per
//                        observation the 192-byte record (J_pt V^-1 | scaled J_pose | J_pt) of the gather, its point's inverse
//                        block recomputed on the spot (the same 72 bytes gathered: no dependence between the roles)
//   SchurSelfBody        per image (one workgroup): diagonal block of S = U + D_c^2 - sum_p W V^-1 W^T and the
//                        reduced right-hand side b_c - sum W V^-1 b_p            (k_schur_self_rhs, k_schur_wide_self, the first C workgroups of
//                        k_schur_blocks / k_schur_self_chunks)
//   SchurPairWalk        off-diagonal blocks by GATHER: six lanes per 6x6 block pair (i,j), ten pairs per
//                        wavefront, each walking the precomputed list of observation pairs that share a point
//                        (pairs ordered by list length) — deterministic, no fp64 atomics      (k_schur_pairs, k_schur_blocks, k_schur_wide_pairs; by
//                        chunks of long lists k_schur_self_chunks + k_schur_chunk_reduce)
//   BaAssembleReducedSystem   which of them an assembly launches, and the group exchange of S
// Columns of constant blocks (constant pose, SubsetParameterization of tvec, constant points) keep
// their slot but get Jacobi scale 0, so their step is exactly 0 and their diagonal is 1.
#include <algorithm>

#include "ba_impl.hpp"

namespace ppsfm {

constexpr double kBig = 1e100;  // diagonal of the augmented rhs row: large enough that BIG - y^T y > 0

// kWithDiagonal: also refreshes the LM diagonal (k_lm_diagonal's work: the pose part by the first 6C threads, a point's
// three entries by its own thread) — one launch less on every accepted step; grid covers max(P, 6C) threads then
// (s (V + D^2 / radius) s)^-1 of one point, D^2 = its LM diagonal: vi = the six entries of the symmetric inverse; returns the determinant
__device__ __forceinline__ double PointBlockInverse(const double* __restrict__ v, double s0, double s1, double s2, double d0, double d1, double d2,
                                                    double inv_radius, double (&vi)[6]) {
  const double a = s0 * s0 * v[0] + d0 * inv_radius, b = s0 * s1 * v[1], c = s0 * s2 * v[2];
  const double d = s1 * s1 * v[3] + d1 * inv_radius, e = s1 * s2 * v[4];
  const double f = s2 * s2 * v[5] + d2 * inv_radius;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  const double id = 1.0 / det;
  vi[0] = c00 * id; vi[1] = c01 * id; vi[2] = c02 * id;
  vi[3] = (a * f - c * c) * id; vi[4] = (b * c - a * e) * id; vi[5] = (a * d - b * b) * id;
  return det;
}
__device__ __forceinline__ double LmDiagonalEntry(double scale, double jtj, double dmin, double dmax) { return fmin(fmax(scale * scale * jtj, dmin), dmax); }

template <bool kWithDiagonal>
__device__ __forceinline__ void PointPrepareBody(int block, int P, const double* __restrict__ V, const double* __restrict__ gp,
                                                 const double* __restrict__ scale_p, double* __restrict__ diag_p,
                                                 const uint8_t* __restrict__ point_const, double inv_radius,
                                                 double* __restrict__ Vinv, double* __restrict__ vb, int32_t* __restrict__ flag,
                                                 int C, const double* __restrict__ U, const double* __restrict__ scale_c, double dmin, double dmax,
                                                 double* __restrict__ diag_c) {
  const int p = block * 256 + threadIdx.x;
  if (kWithDiagonal) {
    if (p < 6 * C) {
      const int c = p / 6, j = p % 6;
      diag_c[p] = LmDiagonalEntry(scale_c[p], U[36 * (size_t)c + 7 * j], dmin, dmax);
    }
    if (p < P) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int di = j == 0 ? 0 : (j == 1 ? 3 : 5);
        diag_p[3 * p + j] = LmDiagonalEntry(scale_p[3 * p + j], V[6 * (size_t)p + di], dmin, dmax);
      }
    }
  }
  if (p >= P) return;
  double* vi = Vinv + 6 * (size_t)p;
  double* vbp = vb + 3 * (size_t)p;
  if (point_const[p]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) vi[i] = 0.0;
    vbp[0] = vbp[1] = vbp[2] = 0.0;
    return;
  }
  const double s0 = scale_p[3 * p], s1 = scale_p[3 * p + 1], s2 = scale_p[3 * p + 2];
  double w[6];
  const double det = PointBlockInverse(V + 6 * (size_t)p, s0, s1, s2, diag_p[3 * p], diag_p[3 * p + 1], diag_p[3 * p + 2], inv_radius, w);
  if (!(det > 0.0) || !isfinite(det)) { atomicOr(flag, 2); }
#pragma unroll
  for (int i = 0; i < 6; ++i) vi[i] = w[i];
  const double b0 = -s0 * gp[3 * p], b1 = -s1 * gp[3 * p + 1], b2 = -s2 * gp[3 * p + 2];
  vbp[0] = w[0] * b0 + w[1] * b1 + w[2] * b2;
  vbp[1] = w[1] * b0 + w[3] * b1 + w[4] * b2;
  vbp[2] = w[2] * b0 + w[4] * b1 + w[5] * b2;
}

struct SchurArgs {
  int C, N, rhs_row;
  const int32_t *pose_start, *pose_obs, *obs_point;
  const double *Jpose, *Jpoint, *U, *gc, *Vinv, *vb, *scale_c, *scale_p, *diag_c;
  double inv_radius;
  double* S;
  int add_diagonal;  // group rank 0 adds U + D^2 (point-sharded multi-GPU: the sum over ranks must contain it once)
  // iterative handles (ba_pcg.hip) have no N x N system: the diagonal blocks go to Sd [C][36] and the reduced rhs to rhs_out [6C]
  double* Sd = nullptr;
  double* rhs_out = nullptr;
  // position in S of every column of the parameter vectors (pose c: columns 6c .. 6c+5 of the vectors; pp_ba_impl::spos): 6c unless every image carries its
  // own variable intrinsics beside its pose columns
  const int32_t* spos = nullptr;
};

// per observation and per attempt: the scaled Jacobian rows the Schur gather needs, ONE 192-byte record (ba_impl.hpp, kRecStride):
//   [ T_o = J_pt,o s_p (V+D^2)^-1 s_p (2 x 3) | J_pose,o diag(s_c) (2 x 6) | J_pt,o (2 x 3) ]      so that  G_oo' = T_o J_pt,o'^T
// The records of a workgroup's 256 observations are staged through LDS and written as one contiguous 48 KB slab with fully
// coalesced 16-byte stores (as K1 does; one lane writing 16-byte pieces at a record stride touched 48 cache lines per store).
// The point's inverse block is computed HERE, per observation, from V / the scales / the LM diagonal (PointBlockInverse: the arithmetic of
// the point role) instead of being read back from Vinv: the same 72 bytes gathered per observation, and no dependence on the point role -
// the two run in ONE launch (k_prepare).  kWithDiagonal: the LM diagonal is being refreshed in this launch: taken from V as well.
template <bool kWithDiagonal>
__device__ __forceinline__ void ObsPrepareBody(int block, int64_t M, const int32_t* __restrict__ obs_pose, const int32_t* __restrict__ obs_point,
                                               const double* __restrict__ Jpose, const double* __restrict__ Jpoint,
                                               const double* __restrict__ V, const double* __restrict__ diag_p, const uint8_t* __restrict__ point_const,
                                               double inv_radius, double dmin, double dmax, const double* __restrict__ scale_c,
                                               const double* __restrict__ scale_p, double* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) double sR[256 * kRecStride];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)block * 256, o = o0 + tid;
  if (o < M) {
    const int c = obs_pose[o], p = obs_point[o];
    double jp[12], jx[6];
    LoadJp(Jpose, (int)o, jp);
    LoadJx(Jpoint, (int)o, jx);
    double2* jo = reinterpret_cast<double2*>(sR + kRecStride * tid + 6);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int j0 = (2 * i) % 6, j1 = (2 * i + 1) % 6;
      jo[i] = make_double2(jp[2 * i] * scale_c[6 * c + j0], jp[2 * i + 1] * scale_c[6 * c + j1]);
    }
    const double s0 = scale_p[3 * p], s1 = scale_p[3 * p + 1], s2 = scale_p[3 * p + 2];
    double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!point_const[p]) {
      const double* v = V + 6 * (size_t)p;
      double d0, d1, d2;
      if (kWithDiagonal) { d0 = LmDiagonalEntry(s0, v[0], dmin, dmax); d1 = LmDiagonalEntry(s1, v[3], dmin, dmax); d2 = LmDiagonalEntry(s2, v[5], dmin, dmax); }
      else { d0 = diag_p[3 * p]; d1 = diag_p[3 * p + 1]; d2 = diag_p[3 * p + 2]; }
      (void)PointBlockInverse(v, s0, s1, s2, d0, d1, d2, inv_radius, vi);
    }
    const double v00 = vi[0] * s0 * s0, v01 = vi[1] * s0 * s1, v02 = vi[2] * s0 * s2, v11 = vi[3] * s1 * s1, v12 = vi[4] * s1 * s2,
                 v22 = vi[5] * s2 * s2;
    double t[6];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      t[3 * r + 0] = jx[3 * r] * v00 + jx[3 * r + 1] * v01 + jx[3 * r + 2] * v02;
      t[3 * r + 1] = jx[3 * r] * v01 + jx[3 * r + 1] * v11 + jx[3 * r + 2] * v12;
      t[3 * r + 2] = jx[3 * r] * v02 + jx[3 * r + 1] * v12 + jx[3 * r + 2] * v22;
    }
    double2* to = reinterpret_cast<double2*>(sR + kRecStride * tid);
    double2* xo = reinterpret_cast<double2*>(sR + kRecStride * tid + 18);
    to[0] = make_double2(t[0], t[1]); to[1] = make_double2(t[2], t[3]); to[2] = make_double2(t[4], t[5]);
    xo[0] = make_double2(jx[0], jx[1]); xo[1] = make_double2(jx[2], jx[3]); xo[2] = make_double2(jx[4], jx[5]);
  }
  __syncthreads();
  const int64_t left = M - o0;
  const int n2 = (left < 256 ? (int)left : 256) * (kRecStride / 2);     // double2 chunks of the slab
  double2* dr = reinterpret_cast<double2*>(rec + (size_t)kRecStride * o0);
  const double2* sr = reinterpret_cast<const double2*>(sR);
#pragma unroll
  for (int it = 0; it < kRecStride / 2; ++it) {
    const int idx = it * 256 + tid;
    if (idx < n2) dr[idx] = sr[idx];
  }
}

// point role (the first point_blocks workgroups) and observation role in ONE launch: neither reads what the other writes
template <bool kWithDiagonal>
__global__ __launch_bounds__(256) void k_prepare(int point_blocks, int P, const double* __restrict__ V, const double* __restrict__ gp, const double* __restrict__ scale_p,
                                                 double* __restrict__ diag_p, const uint8_t* __restrict__ point_const, double inv_radius, double* __restrict__ Vinv,
                                                 double* __restrict__ vb, int32_t* __restrict__ flag, int C, const double* __restrict__ U,
                                                 const double* __restrict__ scale_c, double dmin, double dmax, double* __restrict__ diag_c, int64_t M,
                                                 const int32_t* __restrict__ obs_pose, const int32_t* __restrict__ obs_point, const double* __restrict__ Jpose,
                                                 const double* __restrict__ Jpoint, double* __restrict__ rec, int obs_blocks, double* __restrict__ zS, int zN,
                                                 const int32_t* __restrict__ ztiles) {
  if ((int)blockIdx.x < point_blocks)
    PointPrepareBody<kWithDiagonal>(blockIdx.x, P, V, gp, scale_p, diag_p, point_const, inv_radius, Vinv, vb, flag, C, U, scale_c, dmin, dmax, diag_c);
  else if ((int)blockIdx.x < point_blocks + obs_blocks)
    ObsPrepareBody<kWithDiagonal>((int)blockIdx.x - point_blocks, M, obs_pose, obs_point, Jpose, Jpoint, V, diag_p, point_const, inv_radius, dmin, dmax, scale_c, scale_p, rec);
  else {
    // third role (block-sparse systems): clears the listed 64x64 tiles of S - the factorisation fills exactly these, all others stay zero for good (a launch
    // of its own, 6 us, before this one until the sequence scenes made the rest of the iteration count)
    const int zt = (int)blockIdx.x - point_blocks - obs_blocks;
    const int ti = ztiles[2 * zt], tj = ztiles[2 * zt + 1];
    double2* base = reinterpret_cast<double2*>(zS + (size_t)ti * 64 * zN + (size_t)tj * 64);
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) base[(size_t)(idx >> 5) * (zN / 2) + (idx & 31)] = make_double2(0.0, 0.0);
  }
}

// Per image, ONE workgroup (4 wavefronts, observations strided over 256 lanes, wavefront sums + fixed-order LDS sum: WorkgroupSum4):
//   diagonal block       U_s + D^2 - sum_{o of this image} J_o^T G_oo J_o            (identity on constant columns)
//   reduced rhs          b_c - sum_{o in c} J_c,o^T (J_p,o (V^-1 b_p))               -> row rhs_row of S
// (both walk the same observation list and the same records; they used to be two wavefront-per-image kernels of ~25 us each), and by image 0 the
// augmented corner and the identity padding.  (What was tried here after k_reduce: the remark at PoseReduceBody, ba_step.hip.)
// NV = 0: the 6 x 6 pose block; an iterative handle (a.Sd) gets the blocks in Sd [C][36] and the rhs in rhs_out [6C] instead.
// NV > 0: every image with NV variable intrinsics of its own beside its pose columns (pp_ba_impl::intr_wide_nv; image_ordering.hpp PrivateIntrinsicsColumns).
// The image's W = 6 + NV columns are ONE block of the reduced system, J_w,o = [J_pose,o diag(s_c) | J_intr,o diag(s_k)] (2 x W: the record's pose rows and
// the compact scaled rows of JkS), and the blocks are those of the pose gather with wider rows:
//   diagonal   S_cc = U_c + D^2 (pose part) + sum_{o of c} J_w^T J_w (every entry with an intrinsics column) - sum_o J_w^T G_oo J_w
//   off it     S_ij -= sum over the pair list of (i, j) of J_w,oi^T (T_oi X_oj^T) J_w,oj          (the lists of pp_ba_create, every image listed whatever its pose)
//   rhs        -s g - sum_o J_w^T (J_pt,o (V^-1 b_p))
// instead of the block-pair lists of ba_intr.hip (k_intr_L / k_schur_gen / k_intr_kk / k_intr_sums<1>: built for cameras SHARED between images; a camera per
// image gave 250 000 twelve-lane pairs of one chunk - 0.46 ms per assembly at 500 images / 200k observations against 0.11 for the pose blocks).
template <int NV>
__device__ __forceinline__ void SchurSelfBody(const SchurArgs& a, const double* __restrict__ rec, const double* __restrict__ JkS,
                                              const int32_t* __restrict__ pose_camera, const int32_t* __restrict__ intr_off, int c) {
  constexpr int W = 6 + NV, NU = W * (W + 1) / 2;
  __shared__ double red[4][NU + W];
  const bool blocks_only = NV == 0 && a.Sd != nullptr;
  if (c == 0 && threadIdx.x < 64 && !blocks_only) {     // the corner of the augmented system: BIG at (rhs_row, rhs_row), identity padding below
    const int j = a.rhs_row + threadIdx.x;
    if (j < a.N) {
      if (threadIdx.x > 0) a.S[(size_t)j * a.N + j] = 1.0;
      else if (a.add_diagonal) a.S[(size_t)j * a.N + j] = kBig;
    }
  }
  double run[NU + W];      // the upper triangle, then the rhs row
  double* u = run;
  double* acc = run + NU;
#pragma unroll
  for (int i = 0; i < NU + W; ++i) run[i] = 0.0;
  for (int e = a.pose_start[c] + (int)threadIdx.x; e < a.pose_start[c + 1]; e += 256) {
    const int o = a.pose_obs[e];
    const int p = a.obs_point[o];
    double j0[W], j1[W], q[12];
    {      // the whole record: [T_o | J_pose,o diag(s_c) | J_pt,o]
      const double2* r2 = reinterpret_cast<const double2*>(RecT(rec, (size_t)o));
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double2 v = r2[i]; q[2 * i] = v.x; q[2 * i + 1] = v.y; }
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double2 v = r2[3 + i]; j0[2 * i] = v.x; j0[2 * i + 1] = v.y; }
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double2 v = r2[6 + i]; j1[2 * i] = v.x; j1[2 * i + 1] = v.y; }
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double2 v = r2[9 + i]; q[6 + 2 * i] = v.x; q[6 + 2 * i + 1] = v.y; }
      if constexpr (NV > 0) {
        const double2* k2 = reinterpret_cast<const double2*>(JkS + (size_t)2 * kCamStride * o);
#pragma unroll
        for (int i = 0; i < NV / 2; ++i) { const double2 v0 = k2[i], v1 = k2[kCamStride / 2 + i]; j0[6 + 2 * i] = v0.x; j0[7 + 2 * i] = v0.y; j1[6 + 2 * i] = v1.x; j1[7 + 2 * i] = v1.y; }
      }
    }
    const double g00 = q[0] * q[6] + q[1] * q[7] + q[2] * q[8], g01 = q[0] * q[9] + q[1] * q[10] + q[2] * q[11];
    const double g10 = q[3] * q[6] + q[4] * q[7] + q[5] * q[8], g11 = q[3] * q[9] + q[4] * q[10] + q[5] * q[11];
    int idx = 0;
#pragma unroll
    for (int x = 0; x < W; ++x) {
      const double h0 = j0[x] * g00 + j1[x] * g10, h1 = j0[x] * g01 + j1[x] * g11;
      if constexpr (NV == 0) {
#pragma unroll
        for (int y = x; y < W; ++y) u[idx++] += h0 * j0[y] + h1 * j1[y];
      } else {
        const double d0 = h0 - j0[x], d1 = h1 - j1[x];      // (G - I): the direct term J^T J of every entry with an intrinsics column (the pose part's is U)
#pragma unroll
        for (int y = x; y < W; ++y) u[idx++] += (y < 6) ? h0 * j0[y] + h1 * j1[y] : d0 * j0[y] + d1 * j1[y];
      }
    }
    const double w0 = a.scale_p[3 * p] * a.vb[3 * (size_t)p], w1 = a.scale_p[3 * p + 1] * a.vb[3 * (size_t)p + 1],
                 w2 = a.scale_p[3 * p + 2] * a.vb[3 * (size_t)p + 2];
    const double t0 = q[6] * w0 + q[7] * w1 + q[8] * w2, t1 = q[9] * w0 + q[10] * w1 + q[11] * w2;
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] += j0[j] * t0 + j1[j] * t1;    // already scaled by s_c (the record) / s_k (JkS)
  }
  double sum;
  if (!WorkgroupSum4(run, red, &sum)) return;
  const int i = threadIdx.x;
  const int sp = blocks_only ? 0 : a.spos[6 * c];
  int ioff = 0;      // the image's intrinsics columns in the parameter vectors
  if constexpr (NV > 0) ioff = 6 * a.C + intr_off[pose_camera[c]];
  if (i >= NU) {
    const int j = i - NU;
    const int v = (NV == 0 || j < 6) ? 6 * c + j : ioff + j - 6;
    const double own = a.add_diagonal ? -a.scale_c[v] * a.gc[v] : 0.0;
    if (blocks_only) a.rhs_out[6 * (size_t)c + j] = own - sum;
    else a.S[(size_t)a.rhs_row * a.N + sp + j] = own - sum;
  } else {
    int x, y;
    UpperTriangleIndex<W>(i, &x, &y);
    double v = 0.0;
    if (a.add_diagonal) {
      if (NV == 0 || y < 6) {
        const double sa = a.scale_c[6 * c + x], sb = a.scale_c[6 * c + y];
        v = sa * sb * a.U[36 * (size_t)c + 6 * x + y];
        if (x == y) v = (sa == 0.0) ? 1.0 : v + a.diag_c[6 * c + x] * a.inv_radius;
      } else if (x == y) v = a.diag_c[ioff + x - 6] * a.inv_radius;
    }
    v -= sum;
    if (blocks_only) { a.Sd[36 * (size_t)c + 6 * x + y] = v; a.Sd[36 * (size_t)c + 6 * y + x] = v; }
    else { a.S[(size_t)(sp + x) * a.N + sp + y] = v; a.S[(size_t)(sp + y) * a.N + sp + x] = v; }
  }
}

// Off-diagonal blocks: S_ij -= sum over observation pairs sharing a point of J_i^T (T_oi J_pt,oj^T) J_j.
// W = 6 + NV LANES PER BLOCK PAIR (lane = one row `ar` of the W x W block), 64 / W pairs per wavefront (ten of the 6 x 6 pose blocks): the lists are
// short (5.6 entries per pair on the 500-camera scene, 124k pairs), so a wavefront per pair was all fixed cost and latency
// (122 us); here a wavefront walks ten lists at once and the six lanes of a pair read the same 96-byte records
// (one transaction).  Entries are summed in list order: deterministic, no atomics.
// The walk of the entries [e0, e1) of a list: acc = this lane's row of sum_e J_w,oi^T (T_oi X_oj^T) J_w,oj.  JkS: the compact scaled intrinsics rows
// (NV > 0 only).
template <int NV>
__device__ __forceinline__ void SchurPairWalk(const double* __restrict__ rec, const double* __restrict__ JkS, const int32_t* __restrict__ pair_entries,
                                              int e0, int e1, int ar, double (&acc)[6 + NV]) {
#pragma unroll
  for (int i = 0; i < 6 + NV; ++i) acc[i] = 0.0;
  int2 next = e0 < e1 ? *reinterpret_cast<const int2*>(pair_entries + 2 * (size_t)e0) : make_int2(0, 0);
  for (int e = e0; e < e1; ++e) {
    const int2 oo = next;
    if (e + 1 < e1) next = *reinterpret_cast<const int2*>(pair_entries + 2 * (size_t)(e + 1));   // the next entry's indices travel with this entry's records
    const double2* qi = reinterpret_cast<const double2*>(RecT(rec, (size_t)oo.x));       // T_oi (2x3)
    const double2* qj = reinterpret_cast<const double2*>(RecX(rec, (size_t)oo.y));       // J_pt,oj (2x3)
    const double2* pj = reinterpret_cast<const double2*>(RecJ(rec, (size_t)oo.y));
    const double2 t0 = qi[0], t1 = qi[1], t2 = qi[2];
    const double2 x0 = qj[0], x1 = qj[1], x2 = qj[2];
    double pi0, pi1;      // this lane's row of J_w,oi^T
    if constexpr (NV == 0) {
      pi0 = RecJ(rec, (size_t)oo.x)[ar]; pi1 = RecJ(rec, (size_t)oo.x)[6 + ar];
    } else {
      const double* ri = ar < 6 ? RecJ(rec, (size_t)oo.x) + ar : JkS + (size_t)2 * kCamStride * oo.x + (ar - 6);      // (ri[0], ri[stride])
      pi0 = ri[0]; pi1 = ri[ar < 6 ? 6 : kCamStride];
    }
    // G = T X^T : T rows (t0.x t0.y t1.x | t1.y t2.x t2.y), X rows (x0.x x0.y x1.x | x1.y x2.x x2.y)
    const double g00 = t0.x * x0.x + t0.y * x0.y + t1.x * x1.x, g01 = t0.x * x1.y + t0.y * x2.x + t1.x * x2.y;
    const double g10 = t1.y * x0.x + t2.x * x0.y + t2.y * x1.x, g11 = t1.y * x1.y + t2.x * x2.x + t2.y * x2.y;
    const double h0 = pi0 * g00 + pi1 * g10, h1 = pi0 * g01 + pi1 * g11;
    const double2 j0 = pj[0], j1 = pj[1], j2 = pj[2], j3 = pj[3], j4 = pj[4], j5 = pj[5];   // rows: (j0 j1 j2), (j3 j4 j5)
    acc[0] += h0 * j0.x + h1 * j3.x; acc[1] += h0 * j0.y + h1 * j3.y;
    acc[2] += h0 * j1.x + h1 * j4.x; acc[3] += h0 * j1.y + h1 * j4.y;
    acc[4] += h0 * j2.x + h1 * j5.x; acc[5] += h0 * j2.y + h1 * j5.y;
    if constexpr (NV > 0) {
      const double2* kj = reinterpret_cast<const double2*>(JkS + (size_t)2 * kCamStride * oo.y);
#pragma unroll
      for (int b = 0; b < NV / 2; ++b) {
        const double2 k0 = kj[b], k1 = kj[kCamStride / 2 + b];
        acc[6 + 2 * b] += h0 * k0.x + h1 * k1.x; acc[7 + 2 * b] += h0 * k0.y + h1 * k1.y;
      }
    }
  }
}

// the lists of 4 x (64 / W) pairs per workgroup `block`, each block of S accumulated into - or, kStore, written (every pair of images has a list,
// pp_ba_impl::pairs_complete: S needs no clearing)
template <int NV, bool kStore>
__device__ __forceinline__ void SchurPairsBody(const SchurArgs& a, const double* __restrict__ rec, const double* __restrict__ JkS,
                                               int64_t num_pairs, const int32_t* __restrict__ pair_start,
                                               const int32_t* __restrict__ pair_ij, const int32_t* __restrict__ pair_entries, int64_t block) {
  constexpr int W = 6 + NV, kSlots = 64 / W;
  const int lane = threadIdx.x & 63;
  const int slot = lane / W, ar = lane % W;
  const int64_t wave = block * 4 + (threadIdx.x >> 6);
  const int64_t pr = wave * kSlots + slot;
  if (slot >= kSlots || pr >= num_pairs) return;
  const int bi = pair_ij[2 * pr], bj = pair_ij[2 * pr + 1];
  const int e0 = pair_start[2 * pr], e1 = pair_start[2 * pr + 1];    // (first, last + 1), pairs ordered by list length
  double acc[W];
  SchurPairWalk<NV>(rec, JkS, pair_entries, e0, e1, ar, acc);
  double2* dst = reinterpret_cast<double2*>(a.S + (size_t)(a.spos[6 * bi] + ar) * a.N + a.spos[6 * bj]);
#pragma unroll
  for (int b = 0; b < W / 2; ++b) { double2 d = kStore ? make_double2(0.0, 0.0) : dst[b]; d.x -= acc[2 * b]; d.y -= acc[2 * b + 1]; dst[b] = d; }
}

__global__ __launch_bounds__(256) void k_schur_self_rhs(SchurArgs a, const double* __restrict__ rec) {
  SchurSelfBody<0>(a, rec, nullptr, nullptr, nullptr, blockIdx.x);
}
template <bool kStore>      // kStore: the block is written, not accumulated into (pp_ba_impl::pairs_complete)
__global__ __launch_bounds__(256) void k_schur_pairs(SchurArgs a, const double* __restrict__ rec, int64_t num_pairs,
                                                     const int32_t* __restrict__ pair_start, const int32_t* __restrict__ pair_ij,
                                                     const int32_t* __restrict__ pair_entries) {
  SchurPairsBody<0, kStore>(a, rec, nullptr, num_pairs, pair_start, pair_ij, pair_entries, blockIdx.x);
}
// store mode: the diagonal blocks + rhs (first C workgroups) and the off-diagonal blocks write disjoint parts of S and read the
// same records — one launch, the ~500 per-image workgroups run under the pair gather instead of before it
__global__ __launch_bounds__(256) void k_schur_blocks(SchurArgs a, const double* __restrict__ rec, int64_t num_pairs,
                                                      const int32_t* __restrict__ pair_start, const int32_t* __restrict__ pair_ij,
                                                      const int32_t* __restrict__ pair_entries) {
  if ((int)blockIdx.x < a.C) SchurSelfBody<0>(a, rec, nullptr, nullptr, nullptr, blockIdx.x);
  else SchurPairsBody<0, true>(a, rec, nullptr, num_pairs, pair_start, pair_ij, pair_entries, (int64_t)blockIdx.x - a.C);
}
template <int NV>
__global__ __launch_bounds__(256) void k_schur_wide_self(SchurArgs a, const double* __restrict__ rec, const double* __restrict__ JkS,
                                                         const int32_t* __restrict__ pose_camera, const int32_t* __restrict__ intr_off) {
  SchurSelfBody<NV>(a, rec, JkS, pose_camera, intr_off, blockIdx.x);
}
template <int NV, bool kStore>
__global__ __launch_bounds__(256) void k_schur_wide_pairs(SchurArgs a, const double* __restrict__ rec, const double* __restrict__ JkS, int64_t num_pairs,
                                                          const int32_t* __restrict__ pair_start, const int32_t* __restrict__ pair_ij,
                                                          const int32_t* __restrict__ pair_entries) {
  SchurPairsBody<NV, kStore>(a, rec, JkS, num_pairs, pair_start, pair_ij, pair_entries, blockIdx.x);
}

// Few images, many shared points (the mapper's local bundle adjustment: 6 images, src/sfm/incremental_mapper.cc:813-858): fifteen block pairs with
// lists of hundreds of entries, each walked by six lanes - 134 us of a 190 us LM iteration at 6 images / 2004 observations.  When a list is longer
// than 64 entries (pp_ba_create) the lists are cut into chunks of 32: the same six lanes per CHUNK (the walk of a sub-range),
// partial blocks to memory, then every block = the sum of its chunks in chunk order (k_schur_chunk_reduce) - deterministic, no atomics.
__device__ __forceinline__ void SchurChunksBody(const double* __restrict__ rec, int num_chunks, const int32_t* __restrict__ chunk, const int32_t* __restrict__ pair_entries,
                                                double* __restrict__ partials, int64_t block) {
  const int lane = threadIdx.x & 63;
  const int slot = lane / 6, ar = lane % 6;
  const int64_t ch = (block * 4 + (threadIdx.x >> 6)) * 10 + slot;
  if (slot >= 10 || ch >= num_chunks) return;
  double acc[6];
  SchurPairWalk<0>(rec, nullptr, pair_entries, chunk[3 * ch + 1], chunk[3 * ch + 2], ar, acc);
  double2* dst = reinterpret_cast<double2*>(partials + 36 * (size_t)chunk[3 * ch] + 6 * ar);      // (the chunk's id: the processing order is pp_ba_create's, see "L2 locality of the chunk kernel")
  dst[0] = make_double2(acc[0], acc[1]); dst[1] = make_double2(acc[2], acc[3]); dst[2] = make_double2(acc[4], acc[5]);
}
// the per-image part (first C workgroups) and the chunks in one launch
__global__ __launch_bounds__(256) void k_schur_self_chunks(SchurArgs a, const double* __restrict__ rec, int num_chunks, const int32_t* __restrict__ chunk,
                                                           const int32_t* __restrict__ pair_entries, double* __restrict__ partials) {
  if ((int)blockIdx.x < a.C) SchurSelfBody<0>(a, rec, nullptr, nullptr, nullptr, blockIdx.x);
  else SchurChunksBody(rec, num_chunks, chunk, pair_entries, partials, (int64_t)blockIdx.x - a.C);
}
template <bool kStore>      // kStore: the block is written, not accumulated into (pp_ba_impl::pairs_complete)
__global__ __launch_bounds__(256) void k_schur_chunk_reduce(SchurArgs a, int64_t num_pairs, const int32_t* __restrict__ pair_ij, const int32_t* __restrict__ pair_chunk,
                                                            const double* __restrict__ partials) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= 36 * num_pairs) return;
  const int64_t pr = it / 36;
  const int el = (int)(it % 36);
  const int c0 = pair_chunk[pr], c1 = pair_chunk[pr + 1];
  if (c0 == c1 && !kStore) return;
  double sum = 0.0;
  int ch = c0;
  for (; ch + 8 <= c1; ch += 8) {      // eight partials in flight, added in chunk order (a load per addition was 0.3 us per chunk: 14 us for the 42 chunks of a 334-entry list)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[36 * (size_t)(ch + u) + el];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; ch < c1; ++ch) sum += partials[36 * (size_t)ch + el];
  double* dst = a.S + (size_t)(a.spos[6 * pair_ij[2 * pr]] + el / 6) * a.N + a.spos[6 * pair_ij[2 * pr + 1]] + el % 6;
  *dst = (kStore ? 0.0 : *dst) - sum;
}

// lower triangle + rhs row of S (rows 0 .. n_red, row r = r + 1 entries) <-> a contiguous buffer: the group exchange moves
// (n+1)(n+2)/2 doubles (36 MB at 500 images) instead of the (n+1) x N rectangle (72 MB)
__global__ __launch_bounds__(256) void k_pack_lower(const double* __restrict__ S, int N, int rows, double* __restrict__ packed, int unpack, double* __restrict__ Sout) {
  const int r = blockIdx.y;
  const size_t base = (size_t)r * (r + 1) / 2;
  for (int c = blockIdx.x * 256 + threadIdx.x; c <= r && r < rows; c += gridDim.x * 256) {
    if (unpack) Sout[(size_t)r * N + c] = packed[base + c];
    else packed[base + c] = S[(size_t)r * N + c];
  }
}

// the same for a block-sparse system (a group whose ranks were created with the union co-visibility: the same tile map everywhere): only the non-zero
// 64 x 64 tiles travel - 12 MB instead of 36 at banded cfg 3 ("exploit block sparsity of S when cameras don't co-observe")
__global__ __launch_bounds__(256) void k_pack_tiles(const double* __restrict__ S, int N, const int32_t* __restrict__ tiles, double* __restrict__ packed, int unpack, double* __restrict__ Sout) {
  const int ti = tiles[2 * blockIdx.x], tj = tiles[2 * blockIdx.x + 1];
  double2* pk = reinterpret_cast<double2*>(packed + (size_t)blockIdx.x * 64 * 64);
  for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
    const size_t at = ((size_t)ti * 64 + (idx >> 5)) * N + (size_t)tj * 64 + 2 * (idx & 31);
    if (unpack) *reinterpret_cast<double2*>(Sout + at) = pk[idx];
    else pk[idx] = *reinterpret_cast<const double2*>(S + at);
  }
}

// ---- host ---------------------------------------------------------------------------------------
static SchurArgs MakeSchurArgs(pp_ba_impl* h, double radius) {
  SchurArgs a;
  a.C = h->C; a.N = h->N; a.rhs_row = h->n_red;
  a.pose_start = h->pose_start; a.pose_obs = h->pose_obs; a.obs_point = h->obs_point;
  a.Jpose = h->Jpose; a.Jpoint = h->Jpoint; a.U = h->U; a.gc = h->gc; a.Vinv = h->Vinv; a.vb = h->vb;
  a.scale_c = h->scale_c; a.scale_p = h->scale_p; a.diag_c = h->diag_c;
  a.inv_radius = 1.0 / radius; a.S = h->S; a.add_diagonal = h->group_rank == 0 ? 1 : 0;
  a.spos = h->spos;
  return a;
}

// the group exchange's packed copy of S holds at least `count` doubles (grown, never shrunk; the old content is not kept)
static int EnsureSpack(pp_ba_impl* h, int64_t count) {
  if (h->Spack_cap >= count) return PP_OK;
  h->blocks.Free(&h->Spack);
  h->Spack_cap = 0;
  PP_TRY(h->blocks.Alloc(&h->Spack, (size_t)count));
  h->Spack_cap = count;
  return PP_OK;
}

// every image's 6 + NV columns as one block: the per-image blocks, then the pose gather with wider rows
template <int NV>
static void LaunchWide(pp_ba_impl* h, const SchurArgs& a, bool store_blocks) {
  hipLaunchKernelGGL(k_schur_wide_self<NV>, dim3(h->C), dim3(256), 0, h->stream, a, h->JpS, h->JkS_intr, h->pose_camera, h->intr_off);
  if (h->num_pairs == 0) return;
  const dim3 grid((unsigned)CeilDiv(h->num_pairs, (int64_t)(4 * (64 / (6 + NV)))));
  hipLaunchKernelGGL((store_blocks ? k_schur_wide_pairs<NV, true> : k_schur_wide_pairs<NV, false>), grid, dim3(256), 0, h->stream, a, h->JpS, h->JkS_intr, h->num_pairs,
                     h->pair_start, h->pair_ij, h->pair_entries);
}

// assemble the damped reduced system for `radius` into S (lower triangle + rhs row)
int BaAssembleReducedSystem(pp_ba_impl* h, double radius, bool refresh_diagonal, double dmin, double dmax) {
  hipStream_t s = h->stream;
  // The factorisation overwrites S with L (fill-in included), so blocks without a pair list must be cleared again;
  // when every block has one (dense scenes), the assembly kernels rewrite the whole lower triangle and the padding
  // rows keep their zeros (cleared once at allocation): no 72 MB clear, no read-modify-write in k_schur_pairs.
  // (variable intrinsics: beside their images' pose columns they are part of the images' blocks, all of which are rewritten (k_schur_wide_*); behind the pose
  // columns - the vectors' order - their rows are cleared, a few rows, and the pose part is stored as without them; other layouts clear S)
  const bool store_blocks = h->pairs_complete && !h->iterative && !BaInGroup(h) && (h->NI == 0 || h->intr_wide_nv > 0 || h->spos_identity);
  const int zero_tiles = (!store_blocks && !h->iterative && BaSparseActive(h)) ? h->num_nz_tiles : 0;      // (only the tiles anything is written to: k_prepare's third role)
  if (!store_blocks && !h->iterative && !zero_tiles) PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, s));
  if (store_blocks && h->NI > 0 && h->spos_identity) PP_HIP_TRY(hipMemsetAsync(h->S + (size_t)6 * h->C * h->N, 0, sizeof(double) * (size_t)h->NI * h->N, s));
  {      // (V + D^2 / radius)^-1, V^-1 b_p per point and the per-observation records: one launch
    const int point_blocks = CeilDiv(refresh_diagonal ? std::max(h->P, 6 * h->C) : h->P, 256);
    const dim3 grid(point_blocks + h->num_partials + zero_tiles);
    hipLaunchKernelGGL(refresh_diagonal ? k_prepare<true> : k_prepare<false>, grid, dim3(256), 0, s, point_blocks, h->P, h->V, h->gp, h->scale_p, h->diag_p, h->point_const,
                       1.0 / radius, h->Vinv, h->vb, h->d_flag, h->C, h->U, h->scale_c, dmin, dmax, h->diag_c, h->M, h->obs_pose, h->obs_point, h->Jpose, h->Jpoint, h->JpS,
                       h->num_partials, h->S, h->N, (const int32_t*)h->nz_tile_list);
  }
  SchurArgs a = MakeSchurArgs(h, radius);
  if (h->iterative) {      // the diagonal blocks (preconditioner) and the reduced right-hand side; S itself is applied from the records
    a.Sd = h->pcg_Sd; a.rhs_out = h->pcg_b;
    hipLaunchKernelGGL(k_schur_self_rhs, dim3(h->C), dim3(256), 0, s, a, h->JpS);
    PP_HIP_TRY(hipGetLastError());
    if (BaInGroup(h)) {      // every shard's part of the diagonal blocks and of the right-hand side (rank 0 carries U + D^2 and -g)
      GroupScope g(h);
      PP_TRY(g.Begin());
      PP_TRY(BaGroupReduce(h, h->pcg_Sd, 36 * (int64_t)h->C, PP_REDUCE_SUM));
      PP_TRY(BaGroupReduce(h, h->pcg_b, 6 * (int64_t)h->C, PP_REDUCE_SUM));
      PP_TRY(g.End());
    }
    PP_TRY(IntrAssemble(h, 1.0 / radius, a.add_diagonal));      // (variable intrinsics: their diagonal blocks and their part of the right-hand side)
    if (BaInGroup(h) && h->NI > 0) {      // the per-camera sums of every shard: the compact diagonal blocks (the preconditioner's) and the intrinsics rows of the right-hand side
      GroupScope g(h);
      PP_TRY(g.Begin());
      PP_TRY(BaGroupReduce(h, h->pcg_Scomp, 12 * (int64_t)h->NI, PP_REDUCE_SUM));
      PP_TRY(BaGroupReduce(h, h->pcg_b + 6 * (size_t)h->C, (int64_t)h->NI, PP_REDUCE_SUM));
      PP_TRY(g.End());
    }
    return PP_OK;
  }
  if (h->pairs_chunked && h->num_pairs > 0) {      // long lists (few images, many shared points): chunks of the lists, then the blocks from their chunks
    hipLaunchKernelGGL(k_schur_self_chunks, dim3(h->C + CeilDiv(h->small_num_chunks, 40)), dim3(256), 0, s, a, h->JpS, h->small_num_chunks, h->small_chunk, h->pair_entries,
                       h->small_partials);
    hipLaunchKernelGGL(store_blocks ? k_schur_chunk_reduce<true> : k_schur_chunk_reduce<false>, dim3(CeilDiv(36 * h->num_pairs, 256)), dim3(256), 0, s, a, h->num_pairs,
                       h->pair_ij, h->small_pair_chunk, h->small_partials);
  } else if (h->intr_wide_nv > 0) {
    PP_TRY(IntrScaledJacobians(h));
    switch (h->intr_wide_nv) {
      case 2: LaunchWide<2>(h, a, store_blocks); break;
      case 4: LaunchWide<4>(h, a, store_blocks); break;
      case 6: LaunchWide<6>(h, a, store_blocks); break;
      default: LaunchWide<8>(h, a, store_blocks); break;
    }
  } else if (store_blocks && h->num_pairs > 0) {
    hipLaunchKernelGGL(k_schur_blocks, dim3(h->C + CeilDiv(h->num_pairs, 40)), dim3(256), 0, s, a, h->JpS, h->num_pairs, h->pair_start, h->pair_ij,
                       h->pair_entries);
  } else {
    hipLaunchKernelGGL(k_schur_self_rhs, dim3(h->C), dim3(256), 0, s, a, h->JpS);
    if (h->num_pairs > 0)
      hipLaunchKernelGGL(k_schur_pairs<false>, dim3(CeilDiv(h->num_pairs, 40)), dim3(256), 0, s, a, h->JpS, h->num_pairs, h->pair_start, h->pair_ij,
                         h->pair_entries);
  }
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(IntrAssemble(h, 1.0 / radius, a.add_diagonal));
  if (!BaInGroup(h)) return PP_OK;
  // the group exchange of S, packed: the non-zero tiles (every rank has the group's tile map), or the lower triangle + rhs row - half the bytes of the
  // rectangle on the wire (RCCL or the host callback)
  const bool tiles = BaSparseActive(h) && h->nz_tile_list && h->num_nz_tiles > 0;
  const int rows = h->n_red + 1;
  const int64_t count = tiles ? (int64_t)h->num_nz_tiles * 64 * 64 : (int64_t)rows * (rows + 1) / 2;
  PP_TRY(EnsureSpack(h, count));
  const dim3 grid(std::max(1, std::min(64, CeilDiv(rows, 256))), rows);
  auto pack = [&](const double* from, int unpack, double* to) {
    if (tiles) hipLaunchKernelGGL(k_pack_tiles, dim3(h->num_nz_tiles), dim3(256), 0, s, from, h->N, (const int32_t*)h->nz_tile_list, h->Spack, unpack, to);
    else hipLaunchKernelGGL(k_pack_lower, grid, dim3(256), 0, s, from, h->N, rows, h->Spack, unpack, to);
  };
  pack(h->S, 0, nullptr);
  PP_TRY(BaGroupReduce(h, h->Spack, count, PP_REDUCE_SUM));
  pack(nullptr, 1, h->S);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

}  // namespace ppsfm
