// pp_ba_covariance: covariance blocks of poses and points from the factorised reduced camera system (ceres::Covariance with
// apply_loss_function = true is the model; the reference has no counterpart).
//
// At the handle's parameters H = J^T J, J the loss-corrected Jacobian in the tangent coordinates of pp_ba_eval, no LM damping.  With the points eliminated,
// S = U - W V^-1 W^T = L L^T and Z = L^-1:
//   Cov(pose i, pose j)  = (S^-1)_ij = sum_k Z[k, cols_i]^T Z[k, cols_j]
//   Cov(point p)         = V_p^-1 + Y^T Y,   Y = Z (W_p V_p^-1)        (W_p V_p^-1 is non-zero only in the columns of p's observing images)
// The solver works in Jacobi-scaled coordinates (S_s = D S D): Z is the inverse factor of S_s, the pose blocks are scaled back by s_i s_j, and the scaled
// records (J_pose s)^T J_pt V_p^-1 of the solver's own gather (ba_impl.hpp, kRecStride) make Y^T Y come out unscaled.  Columns of constant blocks carry
// scale 0: their rows and columns of the result are exactly zero.
//
// Device path: the solver's own evaluate / reduce / prepare / Schur kernels with a zero LM diagonal (BaAssembleUndamped) and its own factorisation
// (a CholeskyState of this call, the launch path the handle's has), all on buffers of this call - the handle's S, factor arrays, Jacobi scale and LM
// diagonal are not touched; then
//   k_tri_inverse        Z = L^-1 on 64 x 64 tiles (v_mfma_f64_16x16x4_f64), stored TRANSPOSED (row c of Zt = column c of Z: the gathers below read along k)
//   k_cov_pose_blocks    one workgroup per requested pair
//   k_cov_points         one workgroup per requested point
// No kernel here waits for another workgroup.
//
// pp_ba_covariance_blocks: the block of any pair of parameter blocks (pose, intrinsics, point) from the same Zt.  With Y_p = Z (W_p V_p^-1), the panel
// k_cov_points forms row by row, and X_p = -Y_p, a point is three more columns of Z:
//   Cov(c_a, c_b) = Z[:, a]^T Z[:, b]    Cov(c_a, point p) = Z[:, a]^T X_p    Cov(p, q) = X_p^T X_q  (+ V_p^-1 when p == q)
//   k_cov_blocks         one workgroup per requested block, 6 x 6 accumulators per pass (a 12-wide side takes two passes)
// Both entry points share their front half (CovInverseFactor: buffers, undamped assembly, factorisation, k_tri_inverse).
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): k_cov_blocks (its one instantiation: the kinds are
// workgroup-uniform branches) 186 VGPRs, 0 bytes of scratch, 32 680 bytes of LDS; k_cov_pose_blocks 146 / 0 / 1 152; k_cov_points 92 / 0 / 31 432.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_impl.hpp"
#include "resource_pool.hpp"

namespace ppsfm {

typedef double cov_v4 __attribute__((ext_vector_type(4)));
constexpr int kTile = 64;

// acc + A B over an inner dimension of 64: lane (lr = l & 15, g = l >> 4) holds A[lr][16 g + kk] and B[16 g + kk][lr], kk = 0 .. 15 - the inner index of
// slice kk is 16 g + kk for both operands (any pairing of the inner index is a valid product; this one makes every lane's 16 values contiguous in memory).
// Four independent accumulators (a dependent v_mfma_f64_16x16x4 waits for its predecessor), summed in a fixed order.
__device__ __forceinline__ cov_v4 CovMfma64(const double (&a)[16], const double (&b)[16], cov_v4 acc) {
  cov_v4 p1 = (cov_v4){0.0, 0.0, 0.0, 0.0}, p2 = p1, p3 = p1;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 + kk], b[4 + kk], p1, 0, 0, 0);
    p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[8 + kk], b[8 + kk], p2, 0, 0, 0);
    p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[12 + kk], b[12 + kk], p3, 0, 0, 0);
  }
  return (acc + p1) + (p2 + p3);
}
__device__ __forceinline__ void CovLoad16(const double* __restrict__ p, double (&v)[16]) {      // 16 contiguous doubles, 16-byte aligned
  const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) { const double2 t = q[i]; v[2 * i] = t.x; v[2 * i + 1] = t.y; }
}

// Z = L^-1 by block columns: Z_jj = M_j (= L_jj^-1, left in memory by the factorisation), Z_kj = -M_k sum_{j <= m < k} L_km Z_mj.  A column of Z depends on L
// and on itself only: workgroup (j, strip) computes the 16 columns `strip` of block column j top down and never looks at another workgroup's part.  Wavefront
// w owns rows 16 w .. 16 w + 15 of every 64 x 16 piece; the piece goes through LDS between the two products, and what the workgroup wrote to Zt is read back
// by the same workgroup after a barrier.  nz (may be null): the tile map of a block-sparse factor - only its non-zero tiles L_km are read; Z is dense.
// L: tile (k, m) at L[(64 k + r) ld + 64 m + c]; Minv: T row-major 64 x 64 tiles; Zt[c ld + k] = Z[k][c] (zero above the diagonal: the diagonal tiles
// are masked here, the tiles above them are never written and were cleared by the caller).
__global__ __launch_bounds__(256) void k_tri_inverse(const double* __restrict__ L, int ld, int T, const double* __restrict__ Minv, const uint8_t* __restrict__ nz, double* Zt) {
  __shared__ double P[kTile * 17];
  const int j = (int)blockIdx.x >> 2, strip = (int)blockIdx.x & 3;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  double* zcol = Zt + ((size_t)j * kTile + 16 * strip) * ld;
  for (int idx = tid; idx < kTile * 16; idx += 256) {
    const int cc = idx >> 6, rr = idx & 63, gcol = 16 * strip + cc;
    zcol[(size_t)cc * ld + (size_t)j * kTile + rr] = rr >= gcol ? Minv[(size_t)j * kTile * kTile + rr * kTile + gcol] : 0.0;
  }
  __syncthreads();
  for (int k = j + 1; k < T; ++k) {
    cov_v4 acc = (cov_v4){0.0, 0.0, 0.0, 0.0};
    for (int m = j; m < k; ++m) {
      if (nz && !nz[(size_t)k * T + m]) continue;
      double av[16], bv[16];
      CovLoad16(L + ((size_t)k * kTile + 16 * w + lr) * ld + (size_t)m * kTile + 16 * g, av);
      CovLoad16(zcol + (size_t)lr * ld + (size_t)m * kTile + 16 * g, bv);
      acc = CovMfma64(av, bv, acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) P[(16 * w + g + 4 * i) * 17 + lr] = acc[i];      // D layout: register i <-> row g + 4 i, column lr
    __syncthreads();
    double av[16], bv[16];
    CovLoad16(Minv + (size_t)k * kTile * kTile + (size_t)(16 * w + lr) * kTile + 16 * g, av);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      if (16 * g + kk > 16 * w + lr) av[kk] = 0.0;      // (the strictly upper part of an inverse tile is not relied on)
      bv[kk] = P[(16 * g + kk) * 17 + lr];
    }
    const cov_v4 d = CovMfma64(av, bv, (cov_v4){0.0, 0.0, 0.0, 0.0});
#pragma unroll
    for (int i = 0; i < 4; ++i) zcol[(size_t)lr * ld + (size_t)k * kTile + 16 * w + g + 4 * i] = -d[i];
    __syncthreads();
  }
}

// Cov(pose i, pose j) = s_i s_j sum_{k >= max(col_i, col_j)} Z[k, col_i + a] Z[k, col_j + b]: one workgroup per pair, thread t the rows k0 + t, k0 + t + 256, ..
// in order, then the wavefront butterfly and the four wavefronts in order - the same bits on every call.  pairs: the handle's image numbering.
__global__ __launch_bounds__(256) void k_cov_pose_blocks(const int32_t* __restrict__ pairs, const int32_t* __restrict__ spos, const double* __restrict__ scale_c,
                                                         const double* __restrict__ Zt, int N, int n, double* __restrict__ out) {
  __shared__ double red[4][36];
  const int pr = blockIdx.x, tid = threadIdx.x;
  const int pi = pairs[2 * pr], pj = pairs[2 * pr + 1];
  const int ci = spos[6 * pi], cj = spos[6 * pj];
  const double* zi = Zt + (size_t)ci * N;
  const double* zj = Zt + (size_t)cj * N;
  double acc[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) acc[i] = 0.0;
  for (int k = max(ci, cj) + tid; k < n; k += 256) {
    double a[6], b[6];
#pragma unroll
    for (int x = 0; x < 6; ++x) { a[x] = zi[(size_t)x * N + k]; b[x] = zj[(size_t)x * N + k]; }
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
      for (int y = 0; y < 6; ++y) acc[6 * x + y] += a[x] * b[y];
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) acc[i] = WaveSum(acc[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 36; ++i) red[tid >> 6][i] = acc[i];
  }
  __syncthreads();
  if (tid < 36) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    out[36 * (size_t)pr + tid] = scale_c[6 * pi + tid / 6] * scale_c[6 * pj + tid % 6] * v;
  }
}

struct CovPointArgs {
  int C, n, N;
  const int32_t *pt_start, *pt_obs, *obs_pose, *obs_cam, *spos, *intr_off, *intr_nv;
  const uint8_t* point_const;
  const double *rec, *JkS /* null: no variable intrinsics */, *Vinv, *scale_p, *Zt;
};
constexpr int kCovChunk = 64;      // observations of a point staged at a time

// Cov(point p) = V_p^-1 + Y^T Y, Y = Z B, B = the point's 6 x 3 records (J_pose s)^T J_pt V_p^-1 in the columns of its observing images (and, with variable
// intrinsics, (J_intr s)^T J_pt V_p^-1 in theirs): one workgroup per requested point, thread t row k of Y (rows in blocks of 256 from the first column the
// point touches), the observations in list order; y y^T is summed per thread in row order, then as in k_cov_pose_blocks.  The records are those the
// prepare kernel left at zero damping; V_p^-1 = s (s V s)^-1 s from the point role's inverse.
__global__ __launch_bounds__(256) void k_cov_points(CovPointArgs a, const int32_t* __restrict__ ids, double* __restrict__ out) {
  __shared__ int s_kmin, s_col[kCovChunk], s_nv[kCovChunk], s_colI[kCovChunk][kCamStride];      // 31 KB of LDS in all
  __shared__ double s_B[kCovChunk][18], s_BI[kCovChunk][3 * kCamStride], red[4][6];
  const int tid = threadIdx.x;
  const int p = ids[blockIdx.x];
  if (a.point_const[p]) {      // (workgroup-uniform) Ceres' convention: a constant block has a zero covariance
    if (tid < 9) out[9 * (size_t)blockIdx.x + tid] = 0.0;
    return;
  }
  const int begin = a.pt_start[p], end = a.pt_start[p + 1];
  if (tid == 0) s_kmin = a.n;
  __syncthreads();
  for (int e = begin + tid; e < end; e += 256) {
    const int o = a.pt_obs[e];
    int kmin = a.spos[6 * a.obs_pose[o]];
    if (a.JkS) {
      const int cam = a.obs_cam[o] >> 4, off = a.intr_off[cam];
      if (off >= 0) for (int c = 0; c < a.intr_nv[cam]; ++c) kmin = min(kmin, a.spos[6 * a.C + off + c]);
    }
    atomicMin(&s_kmin, kmin);
  }
  __syncthreads();
  const int kmin = s_kmin;
  const int nchunks = (end - begin + kCovChunk - 1) / kCovChunk;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k0 = kmin; k0 < a.n; k0 += 256) {
    const int k = k0 + tid;
    const bool live = k < a.n;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int cnt = min(kCovChunk, end - begin - kCovChunk * ch);
      if (nchunks > 1 || k0 == kmin) {      // (workgroup-uniform) one chunk: staged once
        __syncthreads();
        if (tid < cnt) {
          const int o = a.pt_obs[begin + kCovChunk * ch + tid];
          const double* t = RecT(a.rec, (size_t)o);
          const double* jp = RecJ(a.rec, (size_t)o);
          s_col[tid] = a.spos[6 * a.obs_pose[o]];
#pragma unroll
          for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int c = 0; c < 3; ++c) s_B[tid][3 * x + c] = jp[x] * t[c] + jp[6 + x] * t[3 + c];
          int nv = 0;
          if (a.JkS) {
            const int cam = a.obs_cam[o] >> 4, off = a.intr_off[cam];
            if (off >= 0) {
              nv = a.intr_nv[cam];      // (at most kCamStride: every variable parameter of the model)
              const double* jk = a.JkS + (size_t)2 * kCamStride * o;
              for (int x = 0; x < nv; ++x) {
                s_colI[tid][x] = a.spos[6 * a.C + off + x];
#pragma unroll
                for (int c = 0; c < 3; ++c) s_BI[tid][3 * x + c] = jk[x] * t[c] + jk[kCamStride + x] * t[3 + c];
              }
            }
          }
          s_nv[tid] = nv;
        }
        __syncthreads();
      }
      if (live) {
        for (int q = 0; q < cnt; ++q) {
          const double* z = a.Zt + (size_t)s_col[q] * a.N + k;
#pragma unroll
          for (int x = 0; x < 6; ++x) {
            const double zz = z[(size_t)x * a.N];
            y0 += zz * s_B[q][3 * x]; y1 += zz * s_B[q][3 * x + 1]; y2 += zz * s_B[q][3 * x + 2];
          }
          const int nv = s_nv[q];
          for (int x = 0; x < nv; ++x) {
            const double zz = a.Zt[(size_t)s_colI[q][x] * a.N + k];
            y0 += zz * s_BI[q][3 * x]; y1 += zz * s_BI[q][3 * x + 1]; y2 += zz * s_BI[q][3 * x + 2];
          }
        }
      }
    }
    acc[0] += y0 * y0; acc[1] += y0 * y1; acc[2] += y0 * y2; acc[3] += y1 * y1; acc[4] += y1 * y2; acc[5] += y2 * y2;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = WaveSum(acc[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) red[tid >> 6][i] = acc[i];
  }
  __syncthreads();
  if (tid < 9) {
    const int r = tid / 3, c = tid % 3;
    const int lo = min(r, c), hi = max(r, c);
    const int sym = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);      // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    const double yy = ((red[0][sym] + red[1][sym]) + red[2][sym]) + red[3][sym];
    out[9 * (size_t)blockIdx.x + tid] = a.scale_p[3 * p + r] * a.scale_p[3 * p + c] * a.Vinv[6 * (size_t)p + sym] + yy;
  }
}

// ---- any pair of parameter blocks ---------------------------------------------------------------
struct CovBlockArgs {
  CovPointArgs p;                  // structure, records and Zt as k_cov_points takes them
  const int32_t* intr_col;
  const double* scale_c;
  const pp_cov_block* blocks;      // image indices in the handle's numbering
  const int64_t* offset;           // first double of every block in out
};
// A point side stages its records as k_cov_points does, 32 observations at a time: two point sides together take the 31 KB of LDS k_cov_points takes for
// one, so five workgroups fit a CU's 160 KB here as there.
constexpr int kCovBlockChunk = 32;
struct CovPointStage {
  int col[kCovBlockChunk], nv[kCovBlockChunk], colI[kCovBlockChunk][kCamStride];
  double B[kCovBlockChunk][18], BI[kCovBlockChunk][3 * kCamStride];
};
__host__ __device__ constexpr int CovWidth(int kind) { return kind == PP_COV_POSE ? 6 : kind == PP_COV_INTRINSICS ? kCamStride : 3; }

// One side of a block as up to 12 columns: col[j] = the column of Zt behind row j, scl[j] = its factor (scale_c of a camera-side column, -1 for the rows
// of a point: X_p = -Y_p; 0 = a zero row: constant, or no such row - it reads column 0 and is not counted), *first = the first row that is not zero in
// every counted column (Z is lower triangular: the smallest column; a point's kmin of k_cov_points; n when nothing counts).  Every thread calls it.
__device__ __forceinline__ void CovSideSetup(const CovBlockArgs& a, int kind, int idx, int* col, double* scl, int* first) {
  const CovPointArgs& p = a.p;
  const int tid = threadIdx.x;
  if (tid == 0) *first = p.n;
  __syncthreads();
  if (kind == PP_COV_POINT) {
    const bool live = !p.point_const[idx];
    if (tid < kCamStride) { col[tid] = 0; scl[tid] = live && tid < 3 ? -1.0 : 0.0; }
    if (live)
      for (int e = p.pt_start[idx] + tid; e < p.pt_start[idx + 1]; e += 256) {
        const int o = p.pt_obs[e];
        int kmin = p.spos[6 * p.obs_pose[o]];
        if (p.JkS) {
          const int cam = p.obs_cam[o] >> 4, off = p.intr_off[cam];
          if (off >= 0) for (int c = 0; c < p.intr_nv[cam]; ++c) kmin = min(kmin, p.spos[6 * p.C + off + c]);
        }
        atomicMin(first, kmin);
      }
  } else if (tid < kCamStride) {
    int g = -1;      // the row's place in the parameter vectors (scale_c, spos)
    if (kind == PP_COV_POSE) {
      if (tid < 6) g = 6 * idx + tid;
    } else {
      const int off = a.p.intr_off[idx], c = off >= 0 ? a.intr_col[kCamStride * idx + tid] : -1;
      if (c >= 0) g = 6 * p.C + off + c;
    }
    const double s = g >= 0 ? a.scale_c[g] : 0.0;
    col[tid] = s != 0.0 ? p.spos[g] : 0;
    scl[tid] = s;
    if (s != 0.0) atomicMin(first, col[tid]);
  }
  __syncthreads();
}

// Row k of Y_p = Z B_p into y[0 .. 2], the sum k_cov_points takes (observations in list order, pose columns then the camera's variable intrinsics).  Every
// thread calls it (the staging has barriers); *staged: a point of one chunk is staged once per workgroup.
__device__ __forceinline__ void CovPointRow(const CovPointArgs& a, CovPointStage& st, int p, bool* staged, int k, bool live, double (&y)[6]) {
  const int tid = threadIdx.x;
  const int begin = a.pt_start[p], end = a.pt_start[p + 1];
  const int nchunks = (end - begin + kCovBlockChunk - 1) / kCovBlockChunk;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int cnt = min(kCovBlockChunk, end - begin - kCovBlockChunk * ch);
    if (nchunks > 1 || !*staged) {      // (workgroup-uniform)
      __syncthreads();
      if (tid < cnt) {
        const int o = a.pt_obs[begin + kCovBlockChunk * ch + tid];
        const double* t = RecT(a.rec, (size_t)o);
        const double* jp = RecJ(a.rec, (size_t)o);
        st.col[tid] = a.spos[6 * a.obs_pose[o]];
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int c = 0; c < 3; ++c) st.B[tid][3 * x + c] = jp[x] * t[c] + jp[6 + x] * t[3 + c];
        int nv = 0;
        if (a.JkS) {
          const int cam = a.obs_cam[o] >> 4, off = a.intr_off[cam];
          if (off >= 0) {
            nv = a.intr_nv[cam];      // (at most kCamStride)
            const double* jk = a.JkS + (size_t)2 * kCamStride * o;
            for (int x = 0; x < nv; ++x) {
              st.colI[tid][x] = a.spos[6 * a.C + off + x];
#pragma unroll
              for (int c = 0; c < 3; ++c) st.BI[tid][3 * x + c] = jk[x] * t[c] + jk[kCamStride + x] * t[3 + c];
            }
          }
        }
        st.nv[tid] = nv;
      }
      __syncthreads();
      *staged = true;
    }
    if (live) {
      for (int q = 0; q < cnt; ++q) {
        const double* z = a.Zt + (size_t)st.col[q] * a.N + k;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
          const double zz = z[(size_t)x * a.N];
          y0 += zz * st.B[q][3 * x]; y1 += zz * st.B[q][3 * x + 1]; y2 += zz * st.B[q][3 * x + 2];
        }
        const int nv = st.nv[q];
        for (int x = 0; x < nv; ++x) {
          const double zz = a.Zt[(size_t)st.colI[q][x] * a.N + k];
          y0 += zz * st.BI[q][3 * x]; y1 += zz * st.BI[q][3 * x + 1]; y2 += zz * st.BI[q][3 * x + 2];
        }
      }
    }
  }
  y[0] = y0; y[1] = y1; y[2] = y2; y[3] = 0.0; y[4] = 0.0; y[5] = 0.0;
}

// Block q = sa sb sum_{k >= k0} A[k, :]^T B[k, :], A and B the two sides' columns of Z (a point's: the row of CovPointRow), k0 the larger of the sides' first
// rows: one workgroup per block, six rows of A against six of B at a time (36 accumulators: a 12-wide side takes two passes), thread t the rows k0 + t,
// k0 + t + 256, .. in order, then the sum of k_cov_pose_blocks - the same bits on every call.  The same point on both sides adds s s V_p^-1 as k_cov_points does.
__global__ __launch_bounds__(256) void k_cov_blocks(CovBlockArgs a, double* __restrict__ out) {
  __shared__ CovPointStage s_stage[2];
  __shared__ int s_col[2][kCamStride], s_first[2];
  __shared__ double s_scl[2][kCamStride], red[4][36];
  const int tid = threadIdx.x;
  const pp_cov_block blk = a.blocks[blockIdx.x];
  const int ka = blk.kind_a, ia = blk.index_a, kb = blk.kind_b, ib = blk.index_b;
  CovSideSetup(a, ka, ia, s_col[0], s_scl[0], &s_first[0]);
  CovSideSetup(a, kb, ib, s_col[1], s_scl[1], &s_first[1]);
  const int wa = CovWidth(ka), wb = CovWidth(kb), n = a.p.n, N = a.p.N;
  const bool same = ka == PP_COV_POINT && kb == PP_COV_POINT && ia == ib;
  const int k0 = max(s_first[0], s_first[1]);
  double* o = out + a.offset[blockIdx.x];
  bool staged_a = false, staged_b = false;
  for (int ha = 0; ha < wa; ha += 6)
    for (int hb = 0; hb < wb; hb += 6) {
      double acc[36];
#pragma unroll
      for (int i = 0; i < 36; ++i) acc[i] = 0.0;
      for (int kk = k0; kk < n; kk += 256) {
        const int k = kk + tid;
        const bool live = k < n;
        double va[6], vb[6];
        if (ka == PP_COV_POINT) CovPointRow(a.p, s_stage[0], ia, &staged_a, k, live, va);
        else {
#pragma unroll
          for (int x = 0; x < 6; ++x) va[x] = live ? a.p.Zt[(size_t)s_col[0][ha + x] * N + k] : 0.0;
        }
        if (same) {
#pragma unroll
          for (int x = 0; x < 6; ++x) vb[x] = va[x];
        } else if (kb == PP_COV_POINT) CovPointRow(a.p, s_stage[1], ib, &staged_b, k, live, vb);
        else {
#pragma unroll
          for (int x = 0; x < 6; ++x) vb[x] = live ? a.p.Zt[(size_t)s_col[1][hb + x] * N + k] : 0.0;
        }
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int y = 0; y < 6; ++y) acc[6 * x + y] += va[x] * vb[y];
      }
#pragma unroll
      for (int i = 0; i < 36; ++i) acc[i] = WaveSum(acc[i]);
      if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 36; ++i) red[tid >> 6][i] = acc[i];
      }
      __syncthreads();
      const int r = ha + tid / 6, c = hb + tid % 6;
      if (tid < 36 && r < wa && c < wb) {
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const double sa = s_scl[0][r], sb = s_scl[1][c];
        double res = sa == 0.0 || sb == 0.0 ? 0.0 : sa * sb * v;
        if (same && sa != 0.0) {      // (sa sb = 1)
          const int lo = min(r, c), hi = max(r, c);
          const int sym = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
          res = a.p.scale_p[3 * ia + r] * a.p.scale_p[3 * ia + c] * a.p.Vinv[6 * (size_t)ia + sym] + v;
        }
        o[(size_t)r * wb + c] = res;
      }
      __syncthreads();      // (red is written again by the next pass)
    }
}

namespace {
// the buffers of one pp_ba_covariance call: pool blocks, returned on every way out - after the stream has drained (`blocks` is destroyed after the body)
struct CovBuffers {
  hipStream_t stream = nullptr;
  CholeskyState* chol = nullptr;
  DeviceBlocks blocks;
  ~CovBuffers() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (chol) CholeskyDestroy(chol);
  }
};
// the handle's solver buffers while the assembly kernels run on this call's: put back on every way out.  This relies on every evaluate / assembly launch
// taking its pointers from the handle when it is enqueued (MakeStepArgs and its like; nothing of the assembly is cached or captured in a graph - only the
// factorisation is, and that runs on a CholeskyState of this call); tests/test_gpu_covariance.py pins it on fresh and on used handles.
struct BufferSwap {
  pp_ba_impl* h;
  double *S, *scale_c, *scale_p, *diag_c, *diag_p, *Vinv, *vb;
  int32_t* d_flag;
  explicit BufferSwap(pp_ba_impl* hh) : h(hh), S(hh->S), scale_c(hh->scale_c), scale_p(hh->scale_p), diag_c(hh->diag_c), diag_p(hh->diag_p), Vinv(hh->Vinv), vb(hh->vb), d_flag(hh->d_flag) {}
  ~BufferSwap() { h->S = S; h->scale_c = scale_c; h->scale_p = scale_p; h->diag_c = diag_c; h->diag_p = diag_p; h->Vinv = Vinv; h->vb = vb; h->d_flag = d_flag; }
};
// what the front half of an entry point leaves for its gather kernels: the call's buffers, and in them the inverse factor Zt (k_tri_inverse enqueued), the
// Jacobi scales and V^-1 of the undamped system; the gather records are the handle's (JpS, JkS_intr)
struct CovSystem {
  CovBuffers buf;
  double *scale_c = nullptr, *scale_p = nullptr, *Vinv = nullptr, *Zt = nullptr;
  int N = 0, n = 0;
};

// The front half of both entry points (`who`), from the handle checks to the k_tri_inverse launch: the buffers of the call, the solver's own undamped
// assembly on them (BufferSwap), the factorisation in two attempts and its flag.  stage_request(blocks, stream): allocates and uploads the entry point's
// request and output arrays with the call's other buffers, ahead of the timed device path (h->ev0).
template <class StageRequest>
int CovInverseFactor(const char* who, pp_ba_impl* h, const pp_ba_options* o, pp_ba_covariance_info* info, CovSystem* cs, StageRequest&& stage_request) {
  PP_REQUIRE(!h->iterative, "%s: an iterative (ITERATIVE_SCHUR) handle never forms the reduced camera system the covariance is taken from - create "
             "the handle with pp_ba_problem_desc::linear_solver = PP_LINEAR_SOLVER_DIRECT (or PPSFM_BA_LINEAR_SOLVER=direct)", who);
  PP_REQUIRE(!BaInGroup(h), "%s: the handle is attached to a group (pp_ba_set_allreduce / pp_ba_set_communicator) and holds one shard of the points - "
             "detach it, or take the covariance from a handle that holds the whole problem", who);
  if (info) std::memset(info, 0, sizeof(*info));
  PP_HIP_TRY(hipSetDevice(h->device));
  PP_TRY(BaEnsureJacobianBuffers(h, 0, h->NI > 0 ? 1 : 0));
  PP_TRY(BaEnsureSolverBuffers(h));
  hipStream_t s = h->stream;
  const int N = h->N, n = h->n_red, T = N / kTile;
  const size_t NN = (size_t)N * N;

  CovBuffers& buf = cs->buf;
  buf.stream = s;
  double *S2 = nullptr, *Linv2 = nullptr, *Lfac2 = nullptr, *x2 = nullptr, *scale_c2 = nullptr, *scale_p2 = nullptr, *diag_c2 = nullptr, *diag_p2 = nullptr, *Vinv2 = nullptr,
         *vb2 = nullptr, *Zt = nullptr;
  int32_t* flag2 = nullptr;
  Switches sw = h->sw;
  sw.chol_small = false;      // (the one-workgroup kernel of one or two block columns keeps its factor in LDS: per-column launches leave it in memory, the same arithmetic)
  {
    std::lock_guard<std::recursive_mutex> setup_lock(DeviceSetupMutex());      // (allocations: not beside another host thread's graph capture)
    DeviceBlocks& B = buf.blocks;
    PP_TRY(B.Alloc(&S2, NN)); PP_TRY(B.Alloc(&Linv2, CholeskyWorkspaceDoubles(N))); PP_TRY(B.Alloc(&x2, (size_t)N)); PP_TRY(B.Alloc(&flag2, 4));
    PP_TRY(B.Alloc(&scale_c2, (size_t)n)); PP_TRY(B.Alloc(&scale_p2, 3 * (size_t)h->P)); PP_TRY(B.Alloc(&diag_c2, (size_t)n)); PP_TRY(B.Alloc(&diag_p2, 3 * (size_t)h->P));
    PP_TRY(B.Alloc(&Vinv2, 6 * (size_t)h->P)); PP_TRY(B.Alloc(&vb2, 3 * (size_t)h->P)); PP_TRY(B.Alloc(&Zt, NN));
    PP_TRY(stage_request(B, s));
    buf.chol = CholeskyCreate(sw);
    CholeskyDisableGraph(buf.chol);      // one factorisation: nothing to replay
    if (CholeskyNeedsFactorArray(buf.chol, N) && !CholeskyColumnsOnly(h->chol)) PP_TRY(B.Alloc(&Lfac2, NN));
    PP_HIP_TRY(hipMemsetAsync(S2, 0, sizeof(double) * NN, s));
    if (Lfac2) PP_HIP_TRY(hipMemsetAsync(Lfac2, 0, sizeof(double) * NN, s));
    PP_HIP_TRY(hipMemsetAsync(Zt, 0, sizeof(double) * NN, s));
    PP_HIP_TRY(hipMemsetAsync(flag2, 0, 4 * sizeof(int32_t), s));
    const CholeskySystem sys{S2, N, n, Linv2, Lfac2, x2, flag2, s};
    const bool sparse = h->sparse_tiles && !h->tile_nz.empty();
    PP_TRY(CholeskyBind(buf.chol, sys, sparse ? h->tile_nz.data() : nullptr));
    if (CholeskyColumnsOnly(h->chol)) (void)CholeskyFallBackToColumns(buf.chol);      // the launch path the handle's own factorisation has
  }
  PP_HIP_TRY(hipEventRecord(h->ev0, s));

  int32_t flag = 0;
  {
    BufferSwap swap(h);
    h->S = S2; h->scale_c = scale_c2; h->scale_p = scale_p2; h->diag_c = diag_c2; h->diag_p = diag_p2; h->Vinv = Vinv2; h->vb = vb2; h->d_flag = flag2;
    for (int attempt = 0; attempt < 2; ++attempt) {
      PP_TRY(BaAssembleUndamped(h, o, attempt == 0));
      PP_TRY(CholeskySolve(buf.chol));
      PP_HIP_TRY(hipMemcpyAsync(&flag, flag2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      PP_HIP_TRY(hipStreamSynchronize(s));
      // a bounded wait of the one-launch factorisation ran out: nothing wrong with the system - once more with per-column launches (what RecoverAfterFlag does)
      if (!(flag & 4) || (flag & 3) || attempt == 1 || !CholeskyFallBackToColumns(buf.chol)) break;
      PP_HIP_TRY(hipMemsetAsync(flag2, 0, sizeof(int32_t), s));
      PP_HIP_TRY(hipMemsetAsync(S2, 0, sizeof(double) * NN, s));
    }
  }
  if (flag & 7) {      // (this call's buffers carry whatever the failed factorisation left: they are returned, the handle's own were never written)
    SetLastError("%s: the undamped reduced camera system is not positive definite (%s) - a free gauge, or a point seen along one direction only, has no covariance", who,
                 (flag & 2) ? "a point block is singular" : (flag & 1) ? "non-positive pivot" : "the factorisation did not finish");
    return PP_ERR_NUMERIC;
  }
  const double* Minv = nullptr;
  const uint8_t* nz = nullptr;
  const double* L = CholeskyFactor(buf.chol, &Minv, &nz);
  if (!L) { SetLastError("%s: the factorisation left no factor in memory", who); return PP_ERR_INTERNAL; }
  hipLaunchKernelGGL(k_tri_inverse, dim3(4 * T), dim3(256), 0, s, L, N, T, Minv, nz, Zt);
  cs->scale_c = scale_c2; cs->scale_p = scale_p2; cs->Vinv = Vinv2; cs->Zt = Zt; cs->N = N; cs->n = n;
  return PP_OK;
}

// what a point's rows are formed from (k_cov_points, k_cov_blocks)
CovPointArgs MakeCovPointArgs(const pp_ba_impl* h, const CovSystem& cs) {
  CovPointArgs a;
  a.C = h->C; a.n = cs.n; a.N = cs.N;
  a.pt_start = h->pt_start; a.pt_obs = h->pt_obs; a.obs_pose = h->obs_pose; a.obs_cam = h->obs_cam; a.spos = h->spos; a.intr_off = h->intr_off; a.intr_nv = h->intr_nv;
  a.point_const = h->point_const; a.rec = h->JpS; a.JkS = h->NI > 0 ? h->JkS_intr : nullptr; a.Vinv = cs.Vinv; a.scale_p = cs.scale_p; a.Zt = cs.Zt;
  return a;
}

// the back half of both entry points, after the result copies are enqueued behind h->ev1
int CovFinish(pp_ba_impl* h, const CovSystem& cs, pp_ba_covariance_info* info) {
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  if (info) {
    float ms = 0;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    info->n = cs.n; info->path = CholeskyLinsolve(cs.buf.chol); info->device_ms = ms;
  }
  return PP_OK;
}
}  // namespace

}  // namespace ppsfm

using namespace ppsfm;

extern "C" int pp_ba_covariance(pp_ba_handle h, const pp_ba_options* o, int32_t num_pose_pairs, const int32_t* pose_i, const int32_t* pose_j, double* pose_cov,
                                int32_t num_points, const int32_t* point_ids, double* point_cov, pp_ba_covariance_info* info) try {
  PP_REQUIRE(h && o, "pp_ba_covariance: null handle or options");
  PP_REQUIRE(num_pose_pairs >= 0 && num_points >= 0, "pp_ba_covariance: negative count");
  PP_REQUIRE(num_pose_pairs == 0 || (pose_i && pose_j && pose_cov), "pp_ba_covariance: %d pose pairs without their arrays", (int)num_pose_pairs);
  PP_REQUIRE(num_points == 0 || (point_ids && point_cov), "pp_ba_covariance: %d points without their arrays", (int)num_points);
  for (int32_t q = 0; q < num_pose_pairs; ++q)
    PP_REQUIRE(pose_i[q] >= 0 && pose_i[q] < h->C && pose_j[q] >= 0 && pose_j[q] < h->C, "pp_ba_covariance: pose pair %d = (%d, %d) is out of range (%d images)", (int)q,
               (int)pose_i[q], (int)pose_j[q], (int)h->C);
  for (int32_t q = 0; q < num_points; ++q)
    PP_REQUIRE(point_ids[q] >= 0 && point_ids[q] < h->P, "pp_ba_covariance: point %d = %d is out of range (%d points)", (int)q, (int)point_ids[q], (int)h->P);
  double *d_pose = nullptr, *d_point = nullptr;
  int32_t *d_pairs = nullptr, *d_ids = nullptr;
  CovSystem cs;
  PP_TRY(CovInverseFactor("pp_ba_covariance", h, o, info, &cs, [&](DeviceBlocks& B, hipStream_t s) -> int {
    PP_TRY(B.Alloc(&d_pose, 36 * (size_t)num_pose_pairs)); PP_TRY(B.Alloc(&d_point, 9 * (size_t)num_points)); PP_TRY(B.Alloc(&d_pairs, 2 * (size_t)num_pose_pairs));
    PP_TRY(B.Alloc(&d_ids, (size_t)num_points));
    // the requests in the handle's image numbering (pp_ba_create may have renumbered the images; the points keep their order)
    if (num_pose_pairs > 0) {
      std::vector<int32_t> pairs(2 * (size_t)num_pose_pairs);
      const bool perm = !h->pose_new_of_old.empty();
      for (int32_t q = 0; q < num_pose_pairs; ++q) {
        pairs[2 * (size_t)q] = perm ? h->pose_new_of_old[pose_i[q]] : pose_i[q];
        pairs[2 * (size_t)q + 1] = perm ? h->pose_new_of_old[pose_j[q]] : pose_j[q];
      }
      PP_HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(int32_t) * pairs.size(), hipMemcpyHostToDevice, s));
      PP_HIP_TRY(hipStreamSynchronize(s));
    }
    if (num_points > 0) PP_HIP_TRY(hipMemcpyAsync(d_ids, point_ids, sizeof(int32_t) * (size_t)num_points, hipMemcpyHostToDevice, s));
    return PP_OK;
  }));
  hipStream_t s = h->stream;
  if (num_pose_pairs > 0)
    hipLaunchKernelGGL(k_cov_pose_blocks, dim3(num_pose_pairs), dim3(256), 0, s, (const int32_t*)d_pairs, (const int32_t*)h->spos, (const double*)cs.scale_c, (const double*)cs.Zt, cs.N, cs.n, d_pose);
  if (num_points > 0) hipLaunchKernelGGL(k_cov_points, dim3(num_points), dim3(256), 0, s, MakeCovPointArgs(h, cs), (const int32_t*)d_ids, d_point);
  PP_HIP_TRY(hipGetLastError());
  PP_HIP_TRY(hipEventRecord(h->ev1, s));
  if (num_pose_pairs > 0) PP_HIP_TRY(hipMemcpyAsync(pose_cov, d_pose, sizeof(double) * 36 * (size_t)num_pose_pairs, hipMemcpyDeviceToHost, s));
  if (num_points > 0) PP_HIP_TRY(hipMemcpyAsync(point_cov, d_point, sizeof(double) * 9 * (size_t)num_points, hipMemcpyDeviceToHost, s));
  return CovFinish(h, cs, info);
} PP_API_CATCH("pp_ba_covariance")

extern "C" int pp_ba_covariance_blocks(pp_ba_handle h, const pp_ba_options* o, int64_t num_blocks, const pp_cov_block* blocks, double* out, int64_t capacity,
                                       pp_ba_covariance_info* info) try {
  PP_REQUIRE(h && o, "pp_ba_covariance_blocks: null handle or options");
  PP_REQUIRE(num_blocks >= 0 && num_blocks <= INT32_MAX, "pp_ba_covariance_blocks: %lld blocks (0 .. 2^31 - 1 in one call)", (long long)num_blocks);
  PP_REQUIRE(num_blocks == 0 || (blocks && out), "pp_ba_covariance_blocks: %lld blocks without their arrays", (long long)num_blocks);
  // the request in the handle's image numbering (the cameras and the points keep their order), and where every block starts in out
  std::vector<pp_cov_block> req(blocks, blocks + num_blocks);
  std::vector<int64_t> offset((size_t)num_blocks + 1, 0);
  const bool perm = !h->pose_new_of_old.empty();
  for (int64_t q = 0; q < num_blocks; ++q) {
    int32_t* side[2][2] = {{&req[(size_t)q].kind_a, &req[(size_t)q].index_a}, {&req[(size_t)q].kind_b, &req[(size_t)q].index_b}};
    for (auto& sd : side) {
      const int32_t kind = *sd[0], idx = *sd[1];
      PP_REQUIRE(kind == PP_COV_POSE || kind == PP_COV_INTRINSICS || kind == PP_COV_POINT, "pp_ba_covariance_blocks: block %lld has the unknown kind %d", (long long)q, (int)kind);
      const int32_t count = kind == PP_COV_POSE ? h->C : kind == PP_COV_INTRINSICS ? h->K : h->P;
      PP_REQUIRE(idx >= 0 && idx < count, "pp_ba_covariance_blocks: block %lld: %s %d is out of range (%d %s)", (long long)q,
                 kind == PP_COV_POSE ? "image" : kind == PP_COV_INTRINSICS ? "camera" : "point", (int)idx, (int)count,
                 kind == PP_COV_POSE ? "images" : kind == PP_COV_INTRINSICS ? "cameras" : "points");
      if (kind == PP_COV_POSE && perm) *sd[1] = h->pose_new_of_old[idx];
    }
    offset[(size_t)q + 1] = offset[(size_t)q] + CovWidth(req[(size_t)q].kind_a) * CovWidth(req[(size_t)q].kind_b);
  }
  const int64_t total = offset[(size_t)num_blocks];
  PP_REQUIRE(capacity >= total, "pp_ba_covariance_blocks: the %lld blocks take %lld doubles, capacity is %lld", (long long)num_blocks, (long long)total, (long long)capacity);
  if (num_blocks == 0) {      // nothing asked for, nothing computed
    if (info) std::memset(info, 0, sizeof(*info));
    return PP_OK;
  }
  double* d_out = nullptr;
  pp_cov_block* d_req = nullptr;
  int64_t* d_offset = nullptr;
  CovSystem cs;
  PP_TRY(CovInverseFactor("pp_ba_covariance_blocks", h, o, info, &cs, [&](DeviceBlocks& B, hipStream_t s) -> int {
    PP_TRY(B.Alloc(&d_out, (size_t)total)); PP_TRY(B.Alloc(&d_req, (size_t)num_blocks)); PP_TRY(B.Alloc(&d_offset, (size_t)num_blocks));
    PP_HIP_TRY(hipMemcpyAsync(d_req, req.data(), sizeof(pp_cov_block) * (size_t)num_blocks, hipMemcpyHostToDevice, s));      // (req and offset outlive the call's last wait)
    PP_HIP_TRY(hipMemcpyAsync(d_offset, offset.data(), sizeof(int64_t) * (size_t)num_blocks, hipMemcpyHostToDevice, s));
    return PP_OK;
  }));
  hipStream_t s = h->stream;
  CovBlockArgs a;
  a.p = MakeCovPointArgs(h, cs);
  a.intr_col = h->intr_col; a.scale_c = cs.scale_c; a.blocks = d_req; a.offset = d_offset;
  hipLaunchKernelGGL(k_cov_blocks, dim3((unsigned)num_blocks), dim3(256), 0, s, a, d_out);
  PP_HIP_TRY(hipGetLastError());
  PP_HIP_TRY(hipEventRecord(h->ev1, s));
  PP_HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, s));
  return CovFinish(h, cs, info);
} PP_API_CATCH("pp_ba_covariance_blocks")
