// K2 / K3 + the Levenberg-Marquardt driver: the device-side replacement of ceres::Solve as the
// reference configures it (src/optim/bundle_adjustment.cc:273-306, options from
// src/optim/bundle_adjustment.h:80-93 and src/controllers/incremental_mapper.cc:196-243).
//
// Per LM iteration (all on the handle's stream; the host only reads back a few scalars):
//   K1   k_line_eval          residuals + Jacobians, loss-corrected            (ba_eval.hip)
//   K2   k_reduce             U_c = sum J_c^T J_c (6x6), g_c = J_c^T r   one WORKGROUP per image,
//                             27 running sums per lane, butterfly + fixed-order LDS reduction (no atomics)
//                             V_p (3x3), g_p                              one lane per point (same launch)
//   K3a  BaAssembleReducedSystem   the damped reduced camera system S for the current trust-region radius: k_prepare, k_schur_*  (ba_schur.hip)
//   K3b  CholeskySolve        dense fp64 MFMA Cholesky of S (cholesky.hip)
//   K3c  k_step_points        point steps, -(J d)^T (r + J d / 2), the trial point x (+) d (quaternion Plus) and the COST at the trial point in one
//                             pass over the observations (four lanes per point; every observation applies the step to its own pose).
//                             With variable intrinsics or a host-callback group: k_backsub_points, k_model_cost_apply and K1 in
//                             cost-only mode at the stored trial point instead
// The trust-region logic restates Ceres' published Levenberg-Marquardt strategy (radius update,
// Jacobi scaling fixed at the first point, clamped LM diagonal, invalid/unsuccessful step handling),
// see DESIGN.md §LM; Ceres itself is third-party and not part of /root/reference.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ba_impl.hpp"
#include "host_ticket.hpp"
#include "lm_policy.hpp"
#include "resource_pool.hpp"
#include "line_residual.hpp"
#include "rccl_comm.hpp"

namespace ppsfm {

// ---- K2 ---------------------------------------------------------------------------------------
__device__ __forceinline__ void PoseReduceBody(int c, const int32_t* __restrict__ pose_start, const int32_t* __restrict__ pose_obs,
                                               const double* __restrict__ Jpose, const double* __restrict__ r,
                                               double* __restrict__ U, double* __restrict__ gc) {
  // one WORKGROUP per image: its observations are strided over 256 lanes, wave sums by DPP row exchanges + v_readlane (WaveSumDpp:
  // the 27 ds_bpermute butterflies of four wavefronts queued up on the LDS crossbar), the four wave totals are added in wave order
  // through LDS (fixed order: deterministic; WorkgroupSum4).  k_reduce 22.0 -> 16.0 us at 500 images x 400 observations (rocprofv3) with the two
  // changes; the same two changes in SchurSelfBody (ba_schur.hip) / k_pcg_images bought nothing (they share their launch with, or are as long
  // as, a gather that is the bound) and cost k_schur_blocks 2 us of occupancy: not applied there.
  __shared__ double red[4][27];
  double run[27];      // the upper triangle of U_c, then g_c
  double* u = run;
  double* g = run + 21;
#pragma unroll
  for (int i = 0; i < 27; ++i) run[i] = 0.0;
  // two observations per lane and round, both index loads and then both rows in flight together (an image has ~400 observations: one
  // round; one observation per round was two dependent round trips per round, twice)
  auto add = [&](const double (&jp)[12], double r0, double r1) {
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      g[a] += jp[a] * r0 + jp[6 + a] * r1;
#pragma unroll
      for (int b = a; b < 6; ++b) u[idx++] += jp[a] * jp[b] + jp[6 + a] * jp[6 + b];
    }
  };
  const int begin = pose_start[c], end = pose_start[c + 1];
  if (end - begin <= 256) {      // (workgroup-uniform) one round at most: nothing to overlap
    const int e = begin + (int)threadIdx.x;
    if (e < end) {
      const int o = pose_obs[e];
      double jp[12];
      LoadJp(Jpose, o, jp);
      add(jp, r[2 * (size_t)o], r[2 * (size_t)o + 1]);
    }
  } else {
    for (int e = begin + (int)threadIdx.x; e < end; e += 512) {
      const bool two = e + 256 < end;
      const int o = pose_obs[e], o2 = pose_obs[two ? e + 256 : e];
      double jp[12], jq[12];
      LoadJp(Jpose, o, jp);
      LoadJp(Jpose, o2, jq);
      const double r0 = r[2 * (size_t)o], r1 = r[2 * (size_t)o + 1];
      const double w = two ? 1.0 : 0.0;
      const double q0 = w * r[2 * (size_t)o2], q1 = w * r[2 * (size_t)o2 + 1];
#pragma unroll
      for (int i = 0; i < 12; ++i) jq[i] *= w;
      add(jp, r0, r1);
      add(jq, q0, q1);
    }
  }
  double v;
  if (!WorkgroupSum4(run, red, &v)) return;
  const int i = threadIdx.x;
  if (i >= 21) {
    gc[6 * (size_t)c + (i - 21)] = v;
  } else {
    int a, b;
    UpperTriangleIndex<6>(i, &a, &b);
    U[36 * (size_t)c + 6 * a + b] = v; U[36 * (size_t)c + 6 * b + a] = v;
  }
}

// four lanes per point (lane q: observations q, q+4, ... of the point, then a fixed two-step butterfly); gid = 4 p + q
__device__ __forceinline__ void PointReduceBody(int gid, int P, const int32_t* __restrict__ pt_start, const int32_t* __restrict__ pt_obs,
                                                const double* __restrict__ Jpoint, const double* __restrict__ r,
                                                double* __restrict__ V, double* __restrict__ gp) {
  const int p = gid >> 2, q = gid & 3;
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  if (p < P) {
    for (int e = pt_start[p] + q; e < pt_start[p + 1]; e += 4) {
      const int o = pt_obs[e];
      double jx[6];
      LoadJx(Jpoint, o, jx);
      const double r0 = r[2 * (size_t)o], r1 = r[2 * (size_t)o + 1];
      v[0] += jx[0] * jx[0] + jx[3] * jx[3]; v[1] += jx[0] * jx[1] + jx[3] * jx[4]; v[2] += jx[0] * jx[2] + jx[3] * jx[5];
      v[3] += jx[1] * jx[1] + jx[4] * jx[4]; v[4] += jx[1] * jx[2] + jx[4] * jx[5]; v[5] += jx[2] * jx[2] + jx[5] * jx[5];
      g[0] += jx[0] * r0 + jx[3] * r1; g[1] += jx[1] * r0 + jx[4] * r1; g[2] += jx[2] * r0 + jx[5] * r1;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) { v[i] += __shfl_xor(v[i], 1, 64); v[i] += __shfl_xor(v[i], 2, 64); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { g[i] += __shfl_xor(g[i], 1, 64); g[i] += __shfl_xor(g[i], 2, 64); }
  if (p >= P || q != 0) return;
#pragma unroll
  for (int i = 0; i < 6; ++i) V[6 * (size_t)p + i] = v[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) gp[3 * (size_t)p + i] = g[i];
}

// K2 in one launch: the first C workgroups reduce one image each (U_c, g_c), the others 64 points each (V_p, g_p); the two
// parts are independent and both latency-bound, so they overlap instead of running back to back (16 + 12 us -> ~17 us)
__global__ __launch_bounds__(256) void k_reduce(int C, int P, const int32_t* __restrict__ pose_start, const int32_t* __restrict__ pose_obs,
                                                const int32_t* __restrict__ pt_start, const int32_t* __restrict__ pt_obs, const double* __restrict__ Jpose,
                                                const double* __restrict__ Jpoint, const double* __restrict__ r, double* __restrict__ U,
                                                double* __restrict__ gc, double* __restrict__ V, double* __restrict__ gp) {
  if ((int)blockIdx.x < C) PoseReduceBody(blockIdx.x, pose_start, pose_obs, Jpose, r, U, gc);
  else PointReduceBody(((int)blockIdx.x - C) * 256 + threadIdx.x, P, pt_start, pt_obs, Jpoint, r, V, gp);     // 64 points per workgroup
}

// Jacobi scaling 1/(1+||col||) (Ceres jacobi_scaling, fixed at the first evaluation); 0 for constant columns
__global__ __launch_bounds__(256) void k_jacobi_scale(int C, int P, const double* __restrict__ U, const double* __restrict__ V,
                                                      const uint8_t* __restrict__ pose_const, const uint8_t* __restrict__ tvec_mask,
                                                      const uint8_t* __restrict__ point_const, int jacobi, double* __restrict__ scale_c,
                                                      double* __restrict__ scale_p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 6 * C) {
    const int c = i / 6, j = i % 6;
    const bool fixed = pose_const[c] || (j >= 3 && ((tvec_mask[c] >> (j - 3)) & 1));
    const double n2 = U[36 * (size_t)c + 7 * j];
    scale_c[i] = fixed ? 0.0 : (jacobi ? 1.0 / (1.0 + sqrt(n2)) : 1.0);
  }
  if (i < 3 * P) {
    const int p = i / 3, j = i % 3;
    const int di = j == 0 ? 0 : (j == 1 ? 3 : 5);
    const double n2 = V[6 * (size_t)p + di];
    scale_p[i] = point_const[p] ? 0.0 : (jacobi ? 1.0 / (1.0 + sqrt(n2)) : 1.0);
  }
}

// LM diagonal: clamp(diag(J_s^T J_s), min, max)   (LevenbergMarquardtStrategy::ComputeStep)
__global__ __launch_bounds__(256) void k_lm_diagonal(int C, int P, const double* __restrict__ U, const double* __restrict__ V,
                                                     const double* __restrict__ scale_c, const double* __restrict__ scale_p, double dmin,
                                                     double dmax, double* __restrict__ diag_c, double* __restrict__ diag_p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 6 * C) {
    const int c = i / 6, j = i % 6;
    const double s = scale_c[i];
    diag_c[i] = fmin(fmax(s * s * U[36 * (size_t)c + 7 * j], dmin), dmax);
  }
  if (i < 3 * P) {
    const int p = i / 3, j = i % 3;
    const int di = j == 0 ? 0 : (j == 1 ? 3 : 5);
    const double s = scale_p[i];
    diag_p[i] = fmin(fmax(s * s * V[6 * (size_t)p + di], dmin), dmax);
  }
}

// ---- K3c --------------------------------------------------------------------------------------
struct StepArgs {
  int C, P;
  int64_t M;
  const int32_t *pt_start, *pt_obs, *obs_pose, *obs_point;
  const double *Jpose, *Jpoint, *r, *Vinv, *vb, *scale_c, *scale_p, *step_c;
  double* step_p;
  double* partials;
  // variable intrinsics (JkS == nullptr: none): compact scaled Jacobian records, block offsets/widths
  const double* JkS;
  const int32_t *obs_cam, *intr_off, *intr_nv;
  // cand_partials != nullptr (no variable intrinsics): k_model_cost_apply also evaluates the cost AT THE TRIAL POINT - each observation
  // applies the step to its own pose and point (the arithmetic of ApplyStepBody) and evaluates its residual there (k_line_eval<0>'s
  // arithmetic and block sums: the same bits), one launch instead of two
  double* cand_partials = nullptr;
  const double *la = nullptr, *lb = nullptr, *lc = nullptr, *poses = nullptr, *points = nullptr, *intr = nullptr;
  int loss_type = 0;
  double loss_scale = 1.0;
};

// (J_k diag(s)) . step of the intrinsics block of observation o  (two rows)
__device__ __forceinline__ void IntrStepProduct(const StepArgs& a, int64_t o, double* m0, double* m1) {
  if (!a.JkS) return;
  const int k = a.obs_cam[o] >> 4;
  const int off = a.intr_off[k];
  if (off < 0) return;
  const int nv = a.intr_nv[k];
  const double* j = a.JkS + (size_t)2 * kCamStride * o;
  const double* d = a.step_c + 6 * a.C + off;
  for (int c = 0; c < nv; ++c) { *m0 += j[c] * d[c]; *m1 += j[kCamStride + c] * d[c]; }
}

// FOUR lanes per point (lane q takes the point's observations q, q+4, ... in list order, then a fixed two-step butterfly):
// one lane per point walked its ~8 observations as eight dependent gather rounds on 391 wavefronts (19 us)
__global__ __launch_bounds__(256) void k_backsub_points(StepArgs a) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int p = gid >> 2, q = gid & 3;
  double acc[3] = {0, 0, 0};
  if (p < a.P) {
    for (int e = a.pt_start[p] + q; e < a.pt_start[p + 1]; e += 4) {
      const int o = a.pt_obs[e];
      const int c = a.obs_pose[o];
      double jp[12], jx[6];
      LoadJp(a.Jpose, o, jp);
      LoadJx(a.Jpoint, o, jx);
      double m0 = 0.0, m1 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) { const double d = a.scale_c[6 * c + j] * a.step_c[6 * c + j]; m0 += jp[j] * d; m1 += jp[6 + j] * d; }
      IntrStepProduct(a, o, &m0, &m1);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += jx[j] * m0 + jx[3 + j] * m1;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { acc[j] += __shfl_xor(acc[j], 1, 64); acc[j] += __shfl_xor(acc[j], 2, 64); }
  if (p >= a.P || q != 0) return;
  const double s0 = a.scale_p[3 * p], s1 = a.scale_p[3 * p + 1], s2 = a.scale_p[3 * p + 2];
  const double w0 = s0 * acc[0], w1 = s1 * acc[1], w2 = s2 * acc[2];
  const double* vi = a.Vinv + 6 * (size_t)p;
  a.step_p[3 * (size_t)p + 0] = a.vb[3 * (size_t)p + 0] - (vi[0] * w0 + vi[1] * w1 + vi[2] * w2);
  a.step_p[3 * (size_t)p + 1] = a.vb[3 * (size_t)p + 1] - (vi[1] * w0 + vi[3] * w1 + vi[4] * w2);
  a.step_p[3 * (size_t)p + 2] = a.vb[3 * (size_t)p + 2] - (vi[2] * w0 + vi[4] * w1 + vi[5] * w2);
}

// model_cost_change = -sum_o (J d)_o . (r_o + (J d)_o / 2)     (TrustRegionMinimizer)
// "last block done": every block calls this after its global results are written; exactly one block (the one whose
// increment completes the count) gets true, with the other blocks' results visible to it.  The counter resets itself.
__device__ __forceinline__ bool LastBlockDone(int32_t* counter, int num_blocks) {
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();                                   // release this block's results
    const int t = atomicAdd(counter, 1);
    s_last = (t == num_blocks - 1) ? 1 : 0;
    if (s_last) { *counter = 0; __threadfence(); }     // acquire the others'
  }
  __syncthreads();
  return s_last != 0;
}
// sum of n values by the 256 threads of a block in a fixed order -> *out
// (the values were written by EARLIER kernels: plain loads)
__device__ __forceinline__ void BlockSumTo(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sh[0];
}

__device__ __forceinline__ void QuatPlus(const double* q, double d0, double d1, double d2, double* out);
// delta = scale * step, never contracted into the addition that applies it: ApplyStepBody (the stored trial point) and ModelCostBody (every
// observation's own copy of it) must produce the same bits
__device__ __forceinline__ double ScaledStep(double scale, double step) {
#pragma clang fp contract(off)
  return scale * step;
}
__device__ __forceinline__ void ModelCostBody(const StepArgs& a, int block) {
  const int64_t o = (int64_t)block * 256 + threadIdx.x;
  double val = 0.0, half_rho = 0.0;
  if (o < a.M) {
    const int c = a.obs_pose[o], p = a.obs_point[o];
    double jp[12], jx[6];
    LoadJp(a.Jpose, (int)o, jp);
    LoadJx(a.Jpoint, (int)o, jx);
    double dc[6], dp[3];
#pragma unroll
    for (int j = 0; j < 6; ++j) dc[j] = ScaledStep(a.scale_c[6 * c + j], a.step_c[6 * c + j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) dp[j] = ScaledStep(a.scale_p[3 * p + j], a.step_p[3 * (size_t)p + j]);
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) { m0 += jp[j] * dc[j]; m1 += jp[6 + j] * dc[j]; }
    IntrStepProduct(a, o, &m0, &m1);
#pragma unroll
    for (int j = 0; j < 3; ++j) { m0 += jx[j] * dp[j]; m1 += jx[3 + j] * dp[j]; }
    val = -(m0 * (a.r[2 * o] + m0 / 2.0) + m1 * (a.r[2 * o + 1] + m1 / 2.0));
    if (a.cand_partials) {      // the residual at this observation's trial pose / point
      const double* pose = a.poses + 7 * (size_t)c;
      double qn[4];
      QuatPlus(pose, dc[0], dc[1], dc[2], qn);
      const double tn[3] = {pose[4] + dc[3], pose[5] + dc[4], pose[6] + dc[5]};
      const double Xn[3] = {a.points[3 * (size_t)p] + dp[0], a.points[3 * (size_t)p + 1] + dp[1], a.points[3 * (size_t)p + 2] + dp[2]};
      const int ck = a.obs_cam[o];
      double res[2];
      LineResidualOnly(ck & 15, a.intr + (size_t)kCamStride * (ck >> 4), qn, tn, Xn, a.la[o], a.lb[o], a.lc[o], res);
      double rho0, rho1;
      LossRho(a.loss_type, a.loss_scale, res[0] * res[0] + res[1] * res[1], &rho0, &rho1);
      half_rho = 0.5 * rho0;
    }
  }
  __shared__ double wsum[4], csum[4];
  val = WaveSum(val);
  if (a.cand_partials) half_rho = WaveSum(half_rho);
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = val; csum[threadIdx.x >> 6] = half_rho; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.partials[block] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (a.cand_partials) a.cand_partials[block] = (csum[0] + csum[1]) + (csum[2] + csum[3]);
  }
}
// second stage (a last-block-done fold was measured SLOWER here: ~800 blocks each paying an agent-scope release fence)
__global__ __launch_bounds__(256) void k_sum(const double* __restrict__ partials, int n, double* __restrict__ out) { BlockSumTo(partials, n, out); }

__device__ __forceinline__ void QuatPlus(const double* q, double d0, double d1, double d2, double* out) {
  const double n = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  if (n > 0.0) {
    const double s = sin(n) / n, w1 = cos(n);
    const double x1 = s * d0, y1 = s * d1, z1 = s * d2;
    const double w2 = q[0], x2 = q[1], y2 = q[2], z2 = q[3];
    out[0] = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
    out[1] = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
    out[2] = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2;
    out[3] = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2;
  } else {
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
  }
}

// trial point x (+) delta, delta = scale * step
__device__ __forceinline__ void ApplyStepBody(int i, int C, int P, const double* __restrict__ poses, const double* __restrict__ points,
                                              const double* __restrict__ scale_c, const double* __restrict__ scale_p,
                                              const double* __restrict__ step_c, const double* __restrict__ step_p,
                                              double* __restrict__ poses_c, double* __restrict__ points_c) {
  if (i < C) {
    const double* q = poses + 7 * (size_t)i;
    double d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) d[j] = ScaledStep(scale_c[6 * i + j], step_c[6 * i + j]);
    double qn[4];
    QuatPlus(q, d[0], d[1], d[2], qn);
    double* o = poses_c + 7 * (size_t)i;
    o[0] = qn[0]; o[1] = qn[1]; o[2] = qn[2]; o[3] = qn[3];
    o[4] = q[4] + d[3]; o[5] = q[5] + d[4]; o[6] = q[6] + d[5];
  }
  if (i < P) {
#pragma unroll
    for (int j = 0; j < 3; ++j) points_c[3 * (size_t)i + j] = points[3 * (size_t)i + j] + ScaledStep(scale_p[3 * i + j], step_p[3 * (size_t)i + j]);
  }
}

// the model cost change of the step (first obs_blocks workgroups, one per 256 observations) and the trial point x (+) d (the
// others): independent of each other, one launch
__global__ __launch_bounds__(256) void k_model_cost_apply(StepArgs a, int obs_blocks, const double* __restrict__ poses, const double* __restrict__ points,
                                                          double* __restrict__ poses_c, double* __restrict__ points_c) {
  if ((int)blockIdx.x < obs_blocks) ModelCostBody(a, blockIdx.x);
  else ApplyStepBody(((int)blockIdx.x - obs_blocks) * 256 + threadIdx.x, a.C, a.P, poses, points, a.scale_c, a.scale_p, a.step_c, a.step_p, poses_c, points_c);
}

// The point step, the model cost change, the trial point and the cost there in ONE pass over the observations (no variable
// intrinsics): four lanes per point as in k_backsub_points; a lane keeps its first two observations' rows in registers between the
// sum that gives the point's step and the terms that need it (further observations of a point are loaded again), so the Jacobian is
// read once where k_backsub_points + k_model_cost_apply read it twice.  Sums: per workgroup in lane / wavefront order, then the norms
// kernel's fixed-order sums - deterministic, a different association than the per-observation kernels' (the costs agree to rounding).
// The last pose_blocks workgroups write the trial poses.
// kIntr (variable intrinsics): every observation's camera-side product also carries (J_k diag(s)) . step of its intrinsics block, and the trial residual is taken with
// the trial intrinsics a.intr (k_apply_intr runs before this kernel then).
template <bool kIntr>
__global__ __launch_bounds__(256) void k_step_points(StepArgs a, int point_blocks, const double* __restrict__ poses, const double* __restrict__ points,
                                                     double* __restrict__ poses_c, double* __restrict__ points_c) {
  if ((int)blockIdx.x >= point_blocks) {
    const int i = ((int)blockIdx.x - point_blocks) * 256 + threadIdx.x;
    if (i < a.C) {
      const double* q = poses + 7 * (size_t)i;
      double d[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) d[j] = ScaledStep(a.scale_c[6 * i + j], a.step_c[6 * i + j]);
      double qn[4];
      QuatPlus(q, d[0], d[1], d[2], qn);
      double* o = poses_c + 7 * (size_t)i;
      o[0] = qn[0]; o[1] = qn[1]; o[2] = qn[2]; o[3] = qn[3];
      o[4] = q[4] + d[3]; o[5] = q[5] + d[4]; o[6] = q[6] + d[5];
    }
    return;
  }
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int p = gid >> 2, q = gid & 3;
  const bool live = p < a.P;
  struct Row { double jp[12], jx[6], dc[6], u0, u1; int o, c; };
  Row R[2];
  auto load = [&](int o, Row& w) {
    w.o = o; w.c = a.obs_pose[o];
    LoadJp(a.Jpose, o, w.jp);
    LoadJx(a.Jpoint, o, w.jx);
    w.u0 = 0.0; w.u1 = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) { w.dc[j] = ScaledStep(a.scale_c[6 * w.c + j], a.step_c[6 * w.c + j]); w.u0 += w.jp[j] * w.dc[j]; w.u1 += w.jp[6 + j] * w.dc[j]; }
    if (kIntr) IntrStepProduct(a, o, &w.u0, &w.u1);
  };
  double acc[3] = {0.0, 0.0, 0.0};
  const int begin = live ? a.pt_start[p] + q : 0, end = live ? a.pt_start[p + 1] : 0;
  bool have[2] = {false, false};
  if (begin < end) {      // the first two observations of this lane: both index loads and then both rows in flight together
    have[0] = true; have[1] = begin + 4 < end;
    const int o0 = a.pt_obs[begin], o1 = a.pt_obs[have[1] ? begin + 4 : begin];
    load(o0, R[0]);
    load(o1, R[1]);
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] += R[0].jx[j] * R[0].u0 + R[0].jx[3 + j] * R[0].u1;
    if (have[1]) {
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += R[1].jx[j] * R[1].u0 + R[1].jx[3 + j] * R[1].u1;
    }
  }
  for (int e = begin + 8; e < end; e += 4) {
    Row w;
    load(a.pt_obs[e], w);
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] += w.jx[j] * w.u0 + w.jx[3 + j] * w.u1;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { acc[j] += __shfl_xor(acc[j], 1, 64); acc[j] += __shfl_xor(acc[j], 2, 64); }
  double dp[3] = {0.0, 0.0, 0.0}, Xn[3] = {0.0, 0.0, 0.0};
  if (live) {
    const double s0 = a.scale_p[3 * p], s1 = a.scale_p[3 * p + 1], s2 = a.scale_p[3 * p + 2];
    const double w0 = s0 * acc[0], w1 = s1 * acc[1], w2 = s2 * acc[2];
    const double* vi = a.Vinv + 6 * (size_t)p;
    const double e0 = a.vb[3 * (size_t)p + 0] - (vi[0] * w0 + vi[1] * w1 + vi[2] * w2);
    const double e1 = a.vb[3 * (size_t)p + 1] - (vi[1] * w0 + vi[3] * w1 + vi[4] * w2);
    const double e2 = a.vb[3 * (size_t)p + 2] - (vi[2] * w0 + vi[4] * w1 + vi[5] * w2);
    dp[0] = ScaledStep(s0, e0); dp[1] = ScaledStep(s1, e1); dp[2] = ScaledStep(s2, e2);
#pragma unroll
    for (int j = 0; j < 3; ++j) Xn[j] = points[3 * (size_t)p + j] + dp[j];
    if (q == 0) {
      a.step_p[3 * (size_t)p + 0] = e0; a.step_p[3 * (size_t)p + 1] = e1; a.step_p[3 * (size_t)p + 2] = e2;
#pragma unroll
      for (int j = 0; j < 3; ++j) points_c[3 * (size_t)p + j] = Xn[j];
    }
  }
  double val = 0.0, half_rho = 0.0;
  auto terms = [&](const Row& w) {
    double m0 = w.u0, m1 = w.u1;
#pragma unroll
    for (int j = 0; j < 3; ++j) { m0 += w.jx[j] * dp[j]; m1 += w.jx[3 + j] * dp[j]; }
    val -= m0 * (a.r[2 * (size_t)w.o] + m0 / 2.0) + m1 * (a.r[2 * (size_t)w.o + 1] + m1 / 2.0);
    const double* pose = poses + 7 * (size_t)w.c;
    double qn[4];
    QuatPlus(pose, w.dc[0], w.dc[1], w.dc[2], qn);
    const double tn[3] = {pose[4] + w.dc[3], pose[5] + w.dc[4], pose[6] + w.dc[5]};
    const int ck = a.obs_cam[w.o];
    double res[2];
    LineResidualOnly(ck & 15, a.intr + (size_t)kCamStride * (ck >> 4), qn, tn, Xn, a.la[w.o], a.lb[w.o], a.lc[w.o], res);
    double rho0, rho1;
    LossRho(a.loss_type, a.loss_scale, res[0] * res[0] + res[1] * res[1], &rho0, &rho1);
    half_rho += 0.5 * rho0;
  };
  if (have[0]) terms(R[0]);
  if (have[1]) terms(R[1]);
  for (int e = begin + 8; e < end; e += 4) {
    Row w;
    load(a.pt_obs[e], w);
    terms(w);
  }
  __shared__ double wsum[4], csum[4];
  val = WaveSum(val);
  half_rho = WaveSum(half_rho);
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = val; csum[threadIdx.x >> 6] = half_rho; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    a.cand_partials[blockIdx.x] = (csum[0] + csum[1]) + (csum[2] + csum[3]);
  }
}

// trial intrinsics: variable parameters move by scale * step, the others are copied
__global__ __launch_bounds__(256) void k_apply_intr(int K, int C, const int32_t* __restrict__ intr_off, const int32_t* __restrict__ intr_col,
                                                    const double* __restrict__ intr, const double* __restrict__ scale_c, const double* __restrict__ step_c,
                                                    double* __restrict__ intr_c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K * kCamStride) return;
  const int k = i / kCamStride;
  const int col = intr_col[i], off = intr_off[k];
  double v = intr[i];
  if (off >= 0 && col >= 0) v += scale_c[6 * C + off + col] * step_c[6 * C + off + col];
  intr_c[i] = v;
}

// intrinsics part of the three norms, folded into the scalars by one lane (NI is small): gradient max-norm over the
// variable columns (Euclidean parameters: |g|), |delta|^2, and |x|^2 over every parameter of a variable block
constexpr int kNormsIntrThreads = 1024;
__global__ __launch_bounds__(kNormsIntrThreads) void k_norms_intr(int K, int C, const int32_t* __restrict__ intr_off, const int32_t* __restrict__ intr_nv,
                                                   const int32_t* __restrict__ camera_model_np, const double* __restrict__ intr, const double* __restrict__ gc,
                                                   const double* __restrict__ scale_c, const double* __restrict__ step_c, double* __restrict__ scal, int count_norms,
                                                   double* __restrict__ host_out, unsigned long long ticket) {
  // one workgroup of sixteen wavefronts, thread t the cameras t, t + 1024, ..: fixed order (a single thread walking 1100 cameras with their dependent loads
  // took 350 us, one wavefront 14.5 us at 500 cameras: a camera per image puts this kernel twice into every LM iteration)
  __shared__ double wmax[kNormsIntrThreads / 64], wst[kNormsIntrThreads / 64], wxn[kNormsIntrThreads / 64];
  double gmax = 0.0, st = 0.0, xn = 0.0;
  for (int k = threadIdx.x; k < K; k += kNormsIntrThreads) {
    const int off = intr_off[k];
    if (off < 0) continue;
    for (int j = 0; j < intr_nv[k]; ++j) {
      gmax = fmax(gmax, fabs(gc[6 * C + off + j]));
      if (step_c && count_norms) { const double d = scale_c[6 * C + off + j] * step_c[6 * C + off + j]; st += d * d; }
    }
    if (count_norms) for (int j = 0; j < camera_model_np[k]; ++j) xn += intr[k * kCamStride + j] * intr[k * kCamStride + j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, off, 64));
  st = WaveSum(st); xn = WaveSum(xn);
  if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = gmax; wst[threadIdx.x >> 6] = st; wxn[threadIdx.x >> 6] = xn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    gmax = 0.0; st = 0.0; xn = 0.0;
    for (int w = 0; w < kNormsIntrThreads / 64; ++w) { gmax = fmax(gmax, wmax[w]); st += wst[w]; xn += wxn[w]; }      // (wavefront order: fixed)
    scal[kGradMax] = fmax(scal[kGradMax], gmax); scal[kStepNorm2] += st; scal[kXNorm2] += xn; __threadfence();
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // with variable intrinsics THIS kernel is the last one to touch the scalars: it hands them to the host's pinned slot (and the ticket the host
  // polls) the way k_norms_partial does without them
  if (host_out) {
    const int b = threadIdx.x;
    if (b < kNumScalars && b != kTicketSlot) {
      const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(scal) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (ticket != 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");        // system scope
      if (b == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + kTicketSlot, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// gradient max norm (Ceres 2.x: ||x - Plus(x, -g)||_inf), |delta|^2, |x|^2: per-block partials + a final block
__global__ __launch_bounds__(256) void k_norms_partial(int C, int P, const double* __restrict__ poses, const double* __restrict__ points,
                                                       const double* __restrict__ gc, const double* __restrict__ gp, const double* __restrict__ scale_c,
                                                       const double* __restrict__ scale_p, const double* __restrict__ step_c,
                                                       const double* __restrict__ step_p, double* __restrict__ part, int32_t* __restrict__ done_counter,
                                                       double* __restrict__ scal, int norm_blocks, const double* __restrict__ sum0, int n0,
                                                       double* __restrict__ out0, const double* __restrict__ sum1, int n1, double* __restrict__ out1,
                                                       double* __restrict__ host_out, unsigned long long ticket, int count_pose_norms, int pose_blocks) {
  __shared__ double smax[256], sstep[256], sx[256];
  // second stages folded in (one launch each saved): the cost partials of the evaluation before this kernel and the model-cost
  // partials of the trial step are summed by two workgroups of their own, beside the norms (inside the last norm block they
  // were ~2 us each on the critical path of the launch)
  if ((int)blockIdx.x >= norm_blocks) {
    if ((int)blockIdx.x == norm_blocks) BlockSumTo(sum0, n0, out0);
    else BlockSumTo(sum1, n1, out1);
  } else {
    // the LAST pose_blocks of the norm blocks take the poses (a quaternion Plus each: an fp64 sin / cos, 1.8 us on the two workgroups that
    // also had their share of the points), the others the points (every load unconditional: one round trip per pass instead of two)
    double gmax = 0.0, st = 0.0, xn = 0.0;
    const int point_blocks = norm_blocks - pose_blocks;
    const bool pose_role = (int)blockIdx.x >= point_blocks;
    const int stride = (pose_role ? pose_blocks : point_blocks) * 256, t0 = ((int)blockIdx.x - (pose_role ? point_blocks : 0)) * 256 + threadIdx.x;
    for (int c = t0; c < C && pose_role; c += stride) {
      const double* q = poses + 7 * (size_t)c;
      if (scale_c[6 * c] != 0.0) {
        double qn[4];
        QuatPlus(q, -gc[6 * (size_t)c], -gc[6 * (size_t)c + 1], -gc[6 * (size_t)c + 2], qn);
#pragma unroll
        for (int j = 0; j < 4; ++j) gmax = fmax(gmax, fabs(q[j] - qn[j]));
        if (count_pose_norms) {      // (a point-sharded group: the poses are replicated, their part of |x|^2 and |step|^2 is counted on rank 0 only)
#pragma unroll
          for (int j = 0; j < 7; ++j) xn += q[j] * q[j];
        }
      }
#pragma unroll
      for (int j = 3; j < 6; ++j) if (scale_c[6 * c + j] != 0.0) gmax = fmax(gmax, fabs(gc[6 * (size_t)c + j]));
      if (step_c && count_pose_norms) {
#pragma unroll
        for (int j = 0; j < 6; ++j) { const double d = scale_c[6 * c + j] * step_c[6 * c + j]; st += d * d; }
      }
    }
    for (int i = t0; i < 3 * P && !pose_role; i += stride) {
      const double sp = scale_p[i], gv = gp[i], xv = points[i], sv = step_p ? step_p[i] : 0.0;
      if (sp != 0.0) { gmax = fmax(gmax, fabs(gv)); xn += xv * xv; }
      const double d = sp * sv;
      st += d * d;
    }
    smax[threadIdx.x] = gmax; sstep[threadIdx.x] = st; sx[threadIdx.x] = xn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        sstep[threadIdx.x] += sstep[threadIdx.x + s];
        sx[threadIdx.x] += sx[threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = smax[0]; part[3 * blockIdx.x + 1] = sstep[0]; part[3 * blockIdx.x + 2] = sx[0]; }
  }
  // the block that finishes last (of ALL blocks) combines the per-block norm partials (fixed order: block b -> slot b, then the
  // same tree) and, when asked to, hands the scalars to the host: it writes them into the pinned host slot itself.  The
  // hipMemcpyAsync this replaces cost ~4 us of copy engine plus ~5 us before the next kernel could start.
  if (LastBlockDone(done_counter, (int)gridDim.x)) {
    const int b = threadIdx.x;
    const bool in = b < norm_blocks;
    smax[b] = in ? __hip_atomic_load(part + 3 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    sstep[b] = in ? __hip_atomic_load(part + 3 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    sx[b] = in ? __hip_atomic_load(part + 3 * b + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (b < s) { smax[b] = fmax(smax[b], smax[b + s]); sstep[b] += sstep[b + s]; sx[b] += sx[b + s]; }
      __syncthreads();
    }
    if (b == 0) {
      __hip_atomic_store(scal + kGradMax, smax[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(scal + kStepNorm2, sstep[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(scal + kXNorm2, sx[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (host_out) {
      __syncthreads();
      if (b < kNumScalars) {      // the three norms from LDS, the other slots (sums of other blocks / earlier kernels, the flag) from memory
        unsigned long long v;
        if (b == kGradMax) v = __double_as_longlong(smax[0]);
        else if (b == kStepNorm2) v = __double_as_longlong(sstep[0]);
        else if (b == kXNorm2) v = __double_as_longlong(sx[0]);
        else v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(scal) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b != kTicketSlot) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      // the ticket goes last (the host polls it instead of waiting on an event: an event record between this kernel and the
      // next one was a ~5 us hole in the stream)
      if (ticket != 0 && b < 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");        // system scope
        if (b == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + kTicketSlot, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// ---- host driver ----------------------------------------------------------------------------------
// (re)binds the factorisation to the handle's current state: the tile map (or none) and the solved-tile array of the one-launch path
// (allocated only when that path can run: N x N doubles, 7 GB at 5000 images)
static int ApplyLinearSolverStructure(pp_ba_impl* h) {
  if (!h->S || h->iterative) return PP_OK;      // EnsureSolverBuffers calls this once the buffers exist; an iterative handle has no factorisation
  // the setters that end up here (pp_ba_set_communicator / pp_ba_set_allreduce) may be called, after a solve, from a host thread whose
  // current device is another one: the allocations below belong on the handle's device
  PP_HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::recursive_mutex> setup_lock(DeviceSetupMutex());
  if (!h->Lfac && CholeskyNeedsFactorArray(h->chol, h->N)) PP_TRY(h->blocks.Alloc(&h->Lfac, (size_t)h->N * h->N));
  // (the solution comes out in the reduced system's column order: the vectors' order unless the intrinsics sit beside their images' pose columns)
  const CholeskySystem sys{h->S, h->N, h->n_red, h->Linv, h->Lfac, h->spos_identity ? h->step_c : h->step_s, h->d_flag, h->stream};
  bool new_map = false;
  { const int rc = CholeskyBind(h->chol, sys, BaSparseActive(h) ? h->tile_nz.data() : nullptr, &new_map); if (rc) return rc; }
  // whatever an earlier factorisation left outside the tiles the new structure rewrites
  if (new_map) PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, h->stream));
  return PP_OK;
}

static int EnsureSolverBuffers(pp_ba_impl* h) {
  if (h->S || h->pcg_state) return PP_OK;
  std::lock_guard<std::recursive_mutex> setup_lock(DeviceSetupMutex());      // (allocations: not beside another host thread's graph capture)
  const int C = h->C, P = h->P;
  h->N = ((h->n_red + 1 + 63) / 64) * 64;
  DeviceBlocks& B = h->blocks;
  const size_t n = (size_t)h->n_red, N = (size_t)h->N;
  PP_TRY(B.Alloc(&h->U, 36 * (size_t)C)); PP_TRY(B.Alloc(&h->gc, n)); PP_TRY(B.Alloc(&h->V, 6 * (size_t)P)); PP_TRY(B.Alloc(&h->gp, 3 * (size_t)P));
  PP_TRY(B.Alloc(&h->Vinv, 6 * (size_t)P)); PP_TRY(B.Alloc(&h->vb, 3 * (size_t)P));
  PP_TRY(B.Alloc(&h->scale_c, n)); PP_TRY(B.Alloc(&h->scale_p, 3 * (size_t)P)); PP_TRY(B.Alloc(&h->diag_c, n)); PP_TRY(B.Alloc(&h->diag_p, 3 * (size_t)P));
  if (!h->iterative) { PP_TRY(B.Alloc(&h->S, N * N)); PP_TRY(B.Alloc(&h->Linv, CholeskyWorkspaceDoubles(h->N))); }
  PP_TRY(B.Alloc(&h->JpS, kRecStride * (size_t)h->M)); PP_TRY(B.Alloc(&h->norm_part, 3 * 256)); PP_TRY(B.Alloc(&h->step_c, N)); PP_TRY(B.Alloc(&h->step_p, 3 * (size_t)P));
  if (!h->spos_identity) PP_TRY(B.Alloc(&h->step_s, N));
  for (int i = 0; i < 8; ++i) PP_TRY(PoolEventAcquire(&h->tev[i], true));
  for (int i = 0; i < 2; ++i) PP_TRY(PoolEventAcquire(&h->tev_eval[i], true));
  PP_TRY(PoolEventAcquire(&h->ev_readback, false));
  if (h->iterative) return PcgEnsureBuffers(h);
  PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, h->stream));
  if (h->sparse_tiles) {      // the factorisation and the assembly skip the tiles that stay zero
    const int T = h->N / 64;
    std::vector<int32_t> list;
    for (int i = 0; i < T; ++i) for (int j = 0; j <= i; ++j) if (h->tile_nz[(size_t)i * T + j]) { list.push_back(i); list.push_back(j); }
    PP_TRY(B.Put(&h->nz_tile_list, list.data(), list.size(), h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return ApplyLinearSolverStructure(h);
}

__global__ __launch_bounds__(256) void k_gather_step(int n, const int32_t* __restrict__ spos, const double* __restrict__ x, double* __restrict__ step) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) step[v] = x[spos[v]];
}

static StepArgs MakeStepArgs(pp_ba_impl* h) {
  StepArgs a;
  a.C = h->C; a.P = h->P; a.M = h->M;
  a.pt_start = h->pt_start; a.pt_obs = h->pt_obs; a.obs_pose = h->obs_pose; a.obs_point = h->obs_point;
  a.Jpose = h->Jpose; a.Jpoint = h->Jpoint; a.r = h->r; a.Vinv = h->Vinv; a.vb = h->vb;
  a.scale_c = h->scale_c; a.scale_p = h->scale_p; a.step_c = h->step_c; a.step_p = h->step_p; a.partials = h->partials + h->partials_stride;   // second region: K1's partials stay valid
  a.JkS = h->NI > 0 ? h->JkS_intr : nullptr; a.obs_cam = h->obs_cam; a.intr_off = h->intr_off; a.intr_nv = h->intr_nv;
  return a;
}

// the group exchange (declared in ba_impl.hpp: the assembly and the PCG loop use it too)
bool BaInGroup(const pp_ba_impl* h) { return h->comm != nullptr || h->allreduce != nullptr; }
int BaGroupReduce(pp_ba_impl* h, double* ptr, int64_t count, int op) {
  if (h->comm) return CommAllReduce(h->comm, ptr, count, op, h->stream);      // stream-ordered: no host synchronisation
  if (!h->allreduce) return PP_OK;
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  const int rc = h->allreduce(h->allreduce_ctx, ptr, count, op);
  if (rc) { SetLastError("allreduce callback returned %d", rc); return PP_ERR_INVALID; }
  return PP_OK;
}
static int GroupEnd(pp_ba_impl* h) { return h->comm ? CommGroupEnd() : PP_OK; }
int GroupScope::Begin() { const int rc = h->comm ? CommGroupStart() : PP_OK; open = rc == PP_OK; return rc; }
int GroupScope::End() { open = false; return GroupEnd(h); }
GroupScope::~GroupScope() { if (open) (void)GroupEnd(h); }
// The failure bits (d_flag[0]: 1 = pivot, 2 = point block, 4 = a bounded wait of the one-launch factorisation ran out) are rank-local,
// the decisions they drive (invalid step, retry with per-column launches) issue collectives: every rank of a group must take the same
// one.  The bits travel as a double through the unused device slot kTicketSlot, MAX-reduced with the scalars of the trial step.
__global__ void k_flag_to_scalar(const int32_t* __restrict__ flag, double* __restrict__ slot) { *slot = (double)(*flag & 7); }
__global__ void k_scalar_to_flag(const double* __restrict__ slot, int32_t* __restrict__ flag) { const int v = (int)*slot; if (v) atomicOr(flag, v); }

// K1 (Jacobian) + K2 at the current parameters; leaves cost in scal[kCost]
// fold_cost: the cost partials are summed by the LaunchNorms call that follows (fold = 1) instead of a kernel of their own
static int EvaluateAndReduce(pp_ba_impl* h, bool fold_cost = false) {
  hipStream_t s = h->stream;
  int rc = LaunchEval(h, 0, h->NI > 0 ? 1 : 0, true, h->poses, h->points, fold_cost ? nullptr : h->scal + kCost, /*compact_cam=*/true);
  if (rc) return rc;
  hipLaunchKernelGGL(k_reduce, dim3(h->C + CeilDiv(4 * (int64_t)h->P, 256)), dim3(256), 0, s, h->C, h->P, h->pose_start, h->pose_obs, h->pt_start, h->pt_obs, h->Jpose,
                     h->Jpoint, h->r, h->U, h->gc, h->V, h->gp);
  PP_HIP_TRY(hipGetLastError());
  if ((rc = IntrSumsAfterEval(h))) return rc;
  if (BaInGroup(h)) {      // the per-pose blocks (and the intrinsics sums) of all shards: one exchange
    GroupScope g(h);
    if ((rc = g.Begin())) return rc;
    if ((rc = BaGroupReduce(h, h->U, 36 * (int64_t)h->C, PP_REDUCE_SUM))) return rc;
    if ((rc = BaGroupReduce(h, h->gc, (int64_t)h->n_red, PP_REDUCE_SUM))) return rc;
    if (h->NI > 0 && (rc = BaGroupReduce(h, h->cnI, (int64_t)h->NI, PP_REDUCE_SUM))) return rc;
    if (!fold_cost && (rc = BaGroupReduce(h, h->scal + kCost, 1, PP_REDUCE_SUM))) return rc;
    if ((rc = g.End())) return rc;
  }
  return PP_OK;
}

// fold: 0 nothing; 1 K1's cost partials -> scal[kCost]; 2 K1's cost partials -> scal[kCostCand] and the model-cost partials
// -> scal[kModelChange] (the trial step)
static int LaunchNorms(pp_ba_impl* h, bool with_step, int fold = 0, double* host_slot = nullptr, unsigned long long ticket = 0) {
  const int pose_blocks = std::min(8, CeilDiv(h->C, 256));
  const int nblk = 64 + pose_blocks;      // (<= 256: the last block combines one partial per thread; norm_part holds 3 x 256)
  const double* model_partials = h->partials + h->partials_stride;
  const int n_trial = fold == 2 && h->trial_partials > 0 ? h->trial_partials : h->num_partials;      // (k_step_points sums per point workgroup)
  hipLaunchKernelGGL(k_norms_partial, dim3(nblk + fold), dim3(256), 0, h->stream, h->C, h->P, h->poses, h->points, h->gc, h->gp, h->scale_c,
                     h->scale_p, with_step ? h->step_c : nullptr, with_step ? h->step_p : nullptr, h->norm_part, h->d_flag + 2, h->scal, nblk,
                     fold ? h->partials : nullptr, fold == 2 ? n_trial : h->num_partials, fold == 2 ? h->scal + kCostCand : h->scal + kCost,
                     fold == 2 ? model_partials : nullptr, n_trial, h->scal + kModelChange, h->NI > 0 ? nullptr : host_slot, h->NI > 0 ? 0ull : ticket,
                     h->group_rank == 0 ? 1 : 0, pose_blocks);
  if (h->NI > 0)
    hipLaunchKernelGGL(k_norms_intr, dim3(1), dim3(kNormsIntrThreads), 0, h->stream, h->K, h->C, h->intr_off, h->intr_nv, h->cam_np, h->intr, h->gc, h->scale_c,
                       with_step ? h->step_c : nullptr, h->scal, h->group_rank == 0 ? 1 : 0, host_slot, ticket);
  PP_HIP_TRY(hipGetLastError());
  if (BaInGroup(h)) {
    // one exchange for the scalars of this evaluation: the gradient max norm as a max; |step|^2 and |x|^2 as sums (the point
    // parts are sharded, the replicated pose / intrinsics parts were counted on rank 0 only: parameter_tolerance sees the
    // same global norms on every rank); the sums this call folded (cost, or candidate cost + model cost change) as sums
    int rc;
    if (with_step) hipLaunchKernelGGL(k_flag_to_scalar, dim3(1), dim3(1), 0, h->stream, h->d_flag, h->scal + kTicketSlot);
    {
      GroupScope g(h);
      if ((rc = g.Begin())) return rc;
      if ((rc = BaGroupReduce(h, h->scal + kGradMax, 1, PP_REDUCE_MAX))) return rc;
      if ((rc = BaGroupReduce(h, h->scal + kStepNorm2, 2, PP_REDUCE_SUM))) return rc;          // kStepNorm2, kXNorm2 are adjacent
      if (fold == 1 && (rc = BaGroupReduce(h, h->scal + kCost, 1, PP_REDUCE_SUM))) return rc;
      if (fold == 2 && (rc = BaGroupReduce(h, h->scal + kCostCand, 2, PP_REDUCE_SUM))) return rc;   // kCostCand, kModelChange are adjacent
      if (with_step && (rc = BaGroupReduce(h, h->scal + kTicketSlot, 1, PP_REDUCE_MAX))) return rc;    // the failure bits: every rank sees the worst
      if ((rc = g.End())) return rc;
    }
    if (with_step) hipLaunchKernelGGL(k_scalar_to_flag, dim3(1), dim3(1), 0, h->stream, h->scal + kTicketSlot, h->d_flag);
    PP_HIP_TRY(hipGetLastError());
  }
  return PP_OK;
}

static int ReadScalars(pp_ba_impl* h) {
  PP_HIP_TRY(hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, h->stream));   // the flag rides in the last slot
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
}
// The norms kernel of a trial step writes the scalars and then a ticket into the pinned slot; the host polls the ticket.
// The poll is a busy spin only for as long as a cfg-3 sized iteration lasts (PPSFM_TICKET_SPIN_US, default 1500 us, 0 = never
// spin): with larger reduced systems (C ~ 5000: ~1 s per factorisation) a spinning caller thread per handle would burn a host
// core per GPU, so after that the thread sleeps between polls (50 us naps: < 0.1 % of such an iteration).  Bounded: after ~2 s
// without the ticket the stream is synchronised once and the ticket re-checked (a failed launch would otherwise wait forever).
static int WaitTicket(pp_ba_impl* h, unsigned long long ticket) {
  const volatile unsigned long long* t = reinterpret_cast<const volatile unsigned long long*>(h->h_scal) + kTicketSlot;
  hipError_t e = hipSuccess;
  switch (WaitHostTicket(t, ticket, h->sw.ticket_spin_us, [&] { return (e = hipStreamSynchronize(h->stream)) == hipSuccess; })) {
    case TicketWait::kArrived: return PP_OK;
    case TicketWait::kSyncFailed: SetLastError("pp_ba_solve: hipStreamSynchronize failed while waiting for the trial step's scalars: %s", hipGetErrorString(e)); break;
    case TicketWait::kNeverArrived: SetLastError("pp_ba_solve: the trial step's scalars never arrived"); break;
  }
  return PP_ERR_HIP;
}
static int32_t HostFlag(const pp_ba_impl* h) { int32_t f; std::memcpy(&f, h->h_scal + kNumScalars - 1, sizeof(f)); return f; }

// pp_ba_options::phase_timings: HIP events between the phases of an iteration.  Off by default: every record is a barrier
// packet on the stream (~5 us each, ~7 per iteration measured on MI355X).
struct PhaseTimer {
  pp_ba_impl* h; bool on; int n = 0; int phase[8];
  PhaseTimer(pp_ba_impl* hh, bool enabled) : h(hh), on(enabled) { if (on) (void)hipEventRecord(h->tev[0], h->stream); }
  void Mark(int ph) { if (on && n < 7) { phase[n] = ph; ++n; (void)hipEventRecord(h->tev[n], h->stream); } }
  void Collect() {
    if (!on) return;
    if (n > 0) (void)hipEventSynchronize(h->tev[n]);     // the host may be ahead of the last mark (it polls a ticket, not the stream)
    for (int i = 0; i < n; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, h->tev[i], h->tev[i + 1]) == hipSuccess) { h->timings_ms[phase[i]] += ms; h->timing_calls[phase[i]] += 1; }
    }
    n = 0;
  }
};


// The start of a solve at the handle's parameters: the failure bits cleared, K1 + K2 there, and the Jacobi scale, which stays what it is here for the
// whole solve (pp_ba_solve goes on with the gradient norm, pp_ba_reduced_system with one LM diagonal and one assembly).
static int EvaluateAndScale(pp_ba_impl* h, const pp_ba_options* o, bool fold, PhaseTimer& timer) {
  PP_HIP_TRY(hipMemsetAsync(h->d_flag, 0, 4 * sizeof(int32_t), h->stream));     // failure bits, the Cholesky token, the norms kernel's block counter
  if (const int rc = EvaluateAndReduce(h, fold)) return rc;
  timer.Mark(PP_BA_T_EVAL);
  const int grid = CeilDiv(std::max<int64_t>(6 * (int64_t)h->C, 3 * (int64_t)h->P), 256);
  hipLaunchKernelGGL(k_jacobi_scale, dim3(grid), dim3(256), 0, h->stream, h->C, h->P, h->U, h->V, h->pose_const, h->tvec_mask, h->point_const,
                     o->jacobi_scaling, h->scale_c, h->scale_p);
  return IntrScale(h, o->jacobi_scaling);
}

// How a solve enqueues its trial steps and gets their scalars: decided once, from the handle and the options, and the same for every iteration.
struct StepPlan {
  bool fold;                // the norms kernel sums the cost partials (a host-callback all-reduce needs the sums before it; RCCL reduces what the norms kernel folded)
  bool speculate;           // the accept path is enqueued before the verdict is known (see Speculation); not with a host-callback all-reduce
  bool direct;              // the norms kernel hands the scalars to the pinned host slot itself (no copy-engine hop) when nothing else touches them after it:
                            // no group all-reduce, no intrinsics norms kernel (LaunchNorms sees to the latter)
  bool fused_trial_cost;    // the cost at the trial point inside the step kernel (one launch less) whenever its partials are summed by the norms kernel anyway
  bool fused_step;          // point steps, model cost change, trial point and its cost in one pass (variable intrinsics: k_step_points<true>, the trial intrinsics applied before it)
  bool phase_timings;
};
static StepPlan MakeStepPlan(const pp_ba_impl* h, const pp_ba_options* o) {
  StepPlan p;
  p.fold = h->allreduce == nullptr;
  p.speculate = h->allreduce == nullptr;
  p.direct = p.speculate && !BaInGroup(h) && h->h_scal_dev != nullptr;
  p.fused_trial_cost = p.fold && (h->NI == 0 || h->sw.ba_fused_step) && h->sw.ba_fused_trial_cost;
  p.fused_step = p.fused_trial_cost && h->sw.ba_fused_step;
  p.phase_timings = o->phase_timings != 0;
  return p;
}

// One trial step for `radius` from the current point, straight down the stream: LM diagonal (when the point is new), reduced system, linear solve, point
// steps + model cost change + trial point in the candidate buffers, its cost, and the norms kernel that gathers the step's scalars (and hands them to
// the host under *ticket when plan.direct).  Waits for nothing and touches nothing of the current point.
static int EnqueueTrialStep(pp_ba_impl* h, const pp_ba_options* o, const StepPlan& plan, double radius, bool refresh_diagonal, PhaseTimer& timer, unsigned long long* ticket) {
  hipStream_t s = h->stream;
  const int grid_obs = h->num_partials;
  int rc;
  if (refresh_diagonal && (rc = IntrDiagonal(h, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  if ((rc = BaAssembleReducedSystem(h, radius, refresh_diagonal, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  timer.Mark(PP_BA_T_SCHUR);
  if (h->iterative) {
    int cg = 0;
    if ((rc = PcgSolve(h, radius, o->max_linear_solver_iterations, o->eta, &cg))) return rc;
    h->linear_solver_iterations += cg;
  } else {
    if ((rc = CholeskySolve(h->chol))) return rc;
    if (!h->spos_identity) hipLaunchKernelGGL(k_gather_step, dim3(CeilDiv(h->n_red, 256)), dim3(256), 0, s, h->n_red, h->spos, h->step_s, h->step_c);
  }
  timer.Mark(PP_BA_T_CHOLESKY);
  StepArgs sa = MakeStepArgs(h);
  if (plan.fused_trial_cost) {
    sa.cand_partials = h->partials; sa.la = h->la; sa.lb = h->lb; sa.lc = h->lc; sa.poses = h->poses; sa.points = h->points; sa.intr = h->intr;
    sa.loss_type = h->loss_type; sa.loss_scale = h->loss_scale;
  }
  h->trial_partials = 0;
  if (plan.fused_step) {
    const int point_blocks = CeilDiv(4 * (int64_t)h->P, 256);
    h->trial_partials = point_blocks;
    if (h->NI > 0) {
      hipLaunchKernelGGL(k_apply_intr, dim3(CeilDiv(h->K * kCamStride, 256)), dim3(256), 0, s, h->K, h->C, h->intr_off, h->intr_col, h->intr, h->scale_c, h->step_c, h->intr_c);
      sa.intr = h->intr_c;      // (the trial residuals are taken with the trial intrinsics)
    }
    hipLaunchKernelGGL(h->NI > 0 ? k_step_points<true> : k_step_points<false>, dim3(point_blocks + CeilDiv(h->C, 256)), dim3(256), 0, s, sa, point_blocks, h->poses, h->points,
                       h->poses_c, h->points_c);
  } else {
    hipLaunchKernelGGL(k_backsub_points, dim3(CeilDiv(4 * (int64_t)h->P, 256)), dim3(256), 0, s, sa);
    hipLaunchKernelGGL(k_model_cost_apply, dim3(grid_obs + CeilDiv(std::max(h->C, h->P), 256)), dim3(256), 0, s, sa, grid_obs, h->poses, h->points,
                       h->poses_c, h->points_c);
  }
  if (!plan.fold) hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, s, sa.partials, grid_obs, h->scal + kModelChange);
  timer.Mark(PP_BA_T_BACKSUB);
  if (h->NI > 0 && !plan.fused_step)
    hipLaunchKernelGGL(k_apply_intr, dim3(CeilDiv(h->K * kCamStride, 256)), dim3(256), 0, s, h->K, h->C, h->intr_off, h->intr_col, h->intr, h->scale_c,
                       h->step_c, h->intr_c);
  if (!plan.fused_trial_cost && (rc = LaunchCostOnly(h, h->poses_c, h->points_c, h->NI > 0 ? h->intr_c : nullptr, plan.fold ? nullptr : h->scal + kCostCand))) return rc;
  PP_HIP_TRY(hipGetLastError());
  if (h->allreduce) {      // (host callback: the two sums exist before the norms kernel here; with RCCL the norms call reduces what it folded)
    if ((rc = BaGroupReduce(h, h->scal + kCostCand, 2, PP_REDUCE_SUM))) return rc;   // kCostCand, kModelChange are adjacent
  }
  *ticket = plan.direct ? ++h->ticket_seq : 0;
  if ((rc = LaunchNorms(h, true, plan.fold ? 2 : 0, plan.direct ? h->h_scal_dev : nullptr, *ticket))) return rc;
  timer.Mark(PP_BA_T_UPDATE_COST);
  return PP_OK;
}

// Latency hiding around the verdict on a trial step.
//
// Speculative acceptance: almost every trial step is accepted, and the accept decision needs a host round trip (~30 us of idle GPU, after which the
// host has to catch up launching ~15 kernels).  So the accept path - make the candidate the current point (a swap of buffer pointers, no copies),
// evaluate + reduce there, norms - is enqueued BEFORE the host waits for the trial step's scalars, and the wait is on their ticket or on an event
// recorded right after their copy, never on the stream.  Invariant: while `speculated`, h->poses / h->points hold the CANDIDATE and the Jacobians and
// sums on the device are the candidate's; Keep or Undo ends that state, and every verdict goes through one of the two.
//
// Pending evaluation: the evaluation at an accepted point (cost, gradient max-norm) is only enqueued; its two scalars are first needed after the next
// trial step's own read-back, so an accepted iteration synchronises with the host once, not twice.  Invariant: while `pending`, `pending_slot` is the
// host slot that evaluation was enqueued into - fixed by Keep, so a later speculation, which flips `eval_slot` for ITS evaluation, cannot redirect it.
// The sequence of accepted points, costs, radii and the termination are those of the eager loop.
struct Speculation {
  pp_ba_impl* const h;
  const StepPlan plan;
  bool speculated = false, pending = false;
  int eval_slot = 0;                       // one of two host slots: the next evaluation is enqueued before the pending one is consumed
  const double* pending_slot = nullptr;

  void SwapPoints() {
    std::swap(h->poses, h->poses_c); std::swap(h->points, h->points_c);
    if (h->NI > 0) std::swap(h->intr, h->intr_c);
  }
  int EnqueueEvaluation() {      // at h->poses / h->points: K1 + K2, norms, scalars -> the free host slot
    hipStream_t s = h->stream;
    int r;
    if (plan.phase_timings) PP_HIP_TRY(hipEventRecord(h->tev_eval[0], s));
    if ((r = EvaluateAndReduce(h, plan.fold))) return r;
    if (plan.phase_timings) PP_HIP_TRY(hipEventRecord(h->tev_eval[1], s));
    eval_slot ^= 1;
    if ((r = LaunchNorms(h, false, plan.fold ? 1 : 0, plan.direct ? h->h_scal_dev + kNumScalars * (1 + eval_slot) : nullptr))) return r;
    if (!plan.direct) PP_HIP_TRY(hipMemcpyAsync(h->h_scal + kNumScalars * (1 + eval_slot), h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, s));
    return PP_OK;
  }
  // the trial step's scalars (and a pending evaluation's, enqueued before them) are in host memory when this returns; with plan.speculate the accept
  // path is on the stream by then, and the host has not waited on the stream
  int AwaitTrialStep(unsigned long long ticket) {
    if (!plan.speculate) return ReadScalars(h);
    if (!plan.direct) {
      PP_HIP_TRY(hipMemcpyAsync(h->h_scal, h->scal, sizeof(double) * kNumScalars, hipMemcpyDeviceToHost, h->stream));
      PP_HIP_TRY(hipEventRecord(h->ev_readback, h->stream));
    }
    SwapPoints();
    if (const int rc = EnqueueEvaluation()) return rc;
    speculated = true;
    if (plan.direct) return WaitTicket(h, ticket);
    PP_HIP_TRY(hipEventSynchronize(h->ev_readback));
    return PP_OK;
  }
  // the step was accepted: the candidate is the current point and its evaluation is pending
  int Keep() {
    if (!speculated) {
      SwapPoints();
      if (const int rc = EnqueueEvaluation()) return rc;
    }
    speculated = false;
    pending_slot = h->h_scal + kNumScalars * (1 + eval_slot);
    pending = true;
    return PP_OK;
  }
  // the step was not accepted: the old point is current again; `reevaluate` restores its Jacobians and sums, which a solve that goes on needs (the
  // result is what the policy already holds and is never consumed)
  int Undo(bool reevaluate) {
    if (!speculated) return PP_OK;
    speculated = false;
    SwapPoints();
    return reevaluate ? EnqueueEvaluation() : PP_OK;
  }
  // requires the pending evaluation to have reached its slot (a later read-back on the same stream has arrived, or the stream was synchronised)
  void Resolve(LmPolicy* policy) {
    policy->Resolve(pending_slot[kCost], pending_slot[kGradMax]);
    float ms = 0;
    if (plan.phase_timings && hipEventElapsedTime(&ms, h->tev_eval[0], h->tev_eval[1]) == hipSuccess) { h->timings_ms[PP_BA_T_EVAL] += ms; h->timing_calls[PP_BA_T_EVAL] += 1; }
    pending = false;
  }
};

// After a trial step that raised failure bits: the bits are cleared and so is what the failed run left in buffers that the assembly relies on but never
// rewrites (the zero padding of S).  Bit 4, a bounded wait of the one-launch factorisation (k_cholesky_tasks) that ran out: nothing wrong with the
// system - *retry = the handle switched to one launch per block column (it stays with them) and the same step is to be made again.  Bit 1, a
// non-positive pivot: the factorisation leaves NaN where it stopped, on which the next, more strongly damped system would fail too; also in the factor
// array.  An iterative handle has no S (its conjugate-gradient loop raises the same bit).
static int RecoverAfterFlag(pp_ba_impl* h, int32_t flag, bool* retry) {
  *retry = false;
  if (flag == 0) return PP_OK;
  hipStream_t s = h->stream;
  PP_HIP_TRY(hipMemsetAsync(h->d_flag, 0, sizeof(int32_t), s));
  *retry = (flag & 4) && CholeskyFallBackToColumns(h->chol);
  const bool failed_pivot = !*retry && (flag & 1) && !h->iterative && h->S;
  if (*retry || failed_pivot) PP_HIP_TRY(hipMemsetAsync(h->S, 0, sizeof(double) * (size_t)h->N * h->N, s));
  if (failed_pivot && h->Lfac) PP_HIP_TRY(hipMemsetAsync(h->Lfac, 0, sizeof(double) * (size_t)h->N * h->N, s));
  return PP_OK;
}

// ceres::IterationCallback with the policy's last row; true = the callback ended the solve (termination set).  Every row is followed by exactly one
// call, so the iteration number is the row's index.
static bool UserStops(const pp_ba_options* o, LmPolicy* policy) {
  if (!o->iteration_callback) return false;
  const double* row = policy->last_row();
  pp_ba_iteration_summary it;
  it.iteration = policy->iteration() - 1; it.step_is_successful = row[6] != 0.0;
  it.cost = row[0]; it.cost_change = row[1]; it.gradient_max_norm = row[2]; it.step_norm = row[3]; it.relative_decrease = row[4];
  it.trust_region_radius = row[5];
  const int32_t r = o->iteration_callback(o->iteration_callback_ctx, &it);
  if (r == PP_SOLVER_ABORT) policy->termination = PP_TERM_USER_FAILURE;
  if (r == PP_SOLVER_TERMINATE_SUCCESSFULLY) policy->termination = PP_TERM_USER_SUCCESS;
  return r == PP_SOLVER_ABORT || r == PP_SOLVER_TERMINATE_SUCCESSFULLY;
}

int BaEnsureSolverBuffers(pp_ba_impl* h) { return EnsureSolverBuffers(h); }
int BaAssembleUndamped(pp_ba_impl* h, const pp_ba_options* o, bool evaluate) {
  if (evaluate) {
    PhaseTimer untimed(h, false);
    if (const int rc = EvaluateAndScale(h, o, /*fold=*/true, untimed)) return rc;      // (no cost sum: nothing of the solver's scalars is touched)
  }
  PP_HIP_TRY(hipMemsetAsync(h->diag_c, 0, sizeof(double) * (size_t)h->n_red, h->stream));
  PP_HIP_TRY(hipMemsetAsync(h->diag_p, 0, sizeof(double) * 3 * (size_t)h->P, h->stream));
  return BaAssembleReducedSystem(h, HUGE_VAL);      // 1 / radius == 0.0
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

// What every rank of a point-sharded group must agree on before it exchanges anything: the layout of the reduced system (order, width, tile map) decides
// the COUNT of every all-reduce of a solve (num_nz_tiles x 4096 doubles or the packed triangle) - ranks that disagree hang in RCCL or sum mismatched tiles.
// 52 bits of an FNV-1a hash, i.e. exactly representable as the double that travels.
static double GroupStructureHash(const pp_ba_impl* h) {
  uint64_t x = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(p); for (size_t i = 0; i < n; ++i) { x ^= b[i]; x *= 1099511628211ull; } };
  const int32_t head[8] = {h->C, h->n_red, h->N, h->NI, h->structure_from_covisibility ? 1 : 0, (h->sparse_tiles && h->structure_from_covisibility) ? 1 : 0,
                           (h->sparse_tiles && h->structure_from_covisibility) ? h->num_nz_tiles : 0, h->iterative ? 1 : 0};
  mix(head, sizeof(head));
  if (h->sparse_tiles && h->structure_from_covisibility) mix(h->tile_nz.data(), h->tile_nz.size());      // (outside that case a group factorises the dense system: the map is not used)
  mix(h->pose_new_of_old.data(), h->pose_new_of_old.size() * sizeof(int32_t));
  return (double)(x >> 12);
}

// The attach calls are COLLECTIVE over the group: one MAX all-reduce of three doubles through the exchange that is about to be attached - [refusal of any
// rank, structure hash, -structure hash] - so that the ranks refuse TOGETHER (one returning an error while the others enter a collective is a hang) and a
// group whose handles lay out the reduced system differently is refused before its first exchange.  A group of one rank exchanges nothing.
static int GroupAgreeOnRefusal(pp_ba_impl* h, int* bad, int* mismatch, pp_allreduce_fn fn, void* ctx, pp_comm_handle comm, int group_size) {
  *mismatch = 0;
  if (group_size <= 1) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  const double hash = GroupStructureHash(h);
  double v[3] = {*bad ? 1.0 : 0.0, hash, -hash};
  if (!h->attach_slot) PP_TRY(h->blocks.Alloc(&h->attach_slot, 4));      // (a slot of its own: nothing of a solve lives here)
  double* slot = h->attach_slot;
  PP_HIP_TRY(hipMemcpyAsync(slot, v, sizeof(v), hipMemcpyHostToDevice, h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  int rc = PP_OK;
  if (comm) rc = pp_comm_allreduce(comm, slot, 3, PP_REDUCE_MAX);
  else if (fn) { rc = fn(ctx, slot, 3, PP_REDUCE_MAX); if (rc) { SetLastError("pp_ba_set_allreduce: the reduction callback returned %d", rc); rc = PP_ERR_HIP; } }
  if (rc) return rc;
  PP_HIP_TRY(hipMemcpy(v, slot, sizeof(v), hipMemcpyDeviceToHost));
  *bad = v[0] != 0.0 ? 1 : 0;
  *mismatch = (v[1] != -v[2]) ? 1 : 0;      // max(hash) != min(hash)
  return PP_OK;
}
#define PP_GROUP_MISMATCH_TEXT "the handles of this group do not lay out the reduced camera system alike (image count, variable intrinsics, internal image order or " \
                               "the block-sparse tile map differ between ranks - e.g. one rank was created without pp_ba_problem_desc::covisibility or with a stale one): " \
                               "every rank of a point-sharded group passes the same order and, with PP_ORDERING_AUTO, the group's union co-visibility"

int pp_ba_set_allreduce(pp_ba_handle h, pp_allreduce_fn fn, void* ctx, int32_t group_rank, int32_t group_size) try {
  PP_REQUIRE(h, "pp_ba_set_allreduce: null handle");
  PP_REQUIRE(group_size >= 1 && group_rank >= 0 && group_rank < group_size, "pp_ba_set_allreduce: bad group");
  if (fn) {
    // every rank must lay out the exchanged system alike: the caller's order, or an order taken from the co-visibility every rank was given.  The verdict is
    // exchanged before anybody refuses, so that the ranks of a group fail TOGETHER instead of one returning an error while the others enter a collective
    int bad = (!h->pose_new_of_old.empty() && !h->structure_from_covisibility) ? 1 : 0, mismatch = 0;
    const int rc = GroupAgreeOnRefusal(h, &bad, &mismatch, fn, ctx, nullptr, group_size);
    if (rc) return rc;
    PP_REQUIRE(bad || !mismatch, "pp_ba_set_allreduce: " PP_GROUP_MISMATCH_TEXT);
    PP_REQUIRE(!bad, "pp_ba_set_allreduce: a handle of this group renumbered its images from its own shard's co-visibility (pp_ba_problem_desc::ordering = AUTO "
               "without ::covisibility); the handles of a point-sharded group keep the caller's order (PP_ORDERING_NATURAL) or are all created with the group's union "
               "co-visibility, so that every rank lays out the exchanged system alike");
  }
  h->allreduce = fn; h->allreduce_ctx = ctx; h->comm = nullptr;
  h->group_rank = fn ? group_rank : 0; h->group_size = fn ? group_size : 1;
  // a host callback is where other host threads do device-wide things (allocate, synchronize) while this handle would be capturing
  // its factorisation graph, and the callback's own synchronisation per LM iteration dwarfs what the graph saves: enqueue eagerly
  if (fn) CholeskyDisableGraph(h->chol);
  return ApplyLinearSolverStructure(h);      // (a block-sparse tile map made from the shard's own observations is rank-local: not used inside a group)
} PP_API_CATCH("pp_ba_set_allreduce")

int pp_ba_set_communicator(pp_ba_handle h, pp_comm_handle comm) try {
  PP_REQUIRE(h, "pp_ba_set_communicator: null handle");
  PP_REQUIRE(!comm || comm->device == h->device, "pp_ba_set_communicator: the communicator lives on device %d, the handle on device %d", comm ? comm->device : -1, h->device);
  if (comm) {
    int bad = (!h->pose_new_of_old.empty() && !h->structure_from_covisibility) ? 1 : 0, mismatch = 0;      // (see pp_ba_set_allreduce: the ranks of a group refuse together)
    const int rc = GroupAgreeOnRefusal(h, &bad, &mismatch, nullptr, nullptr, comm, comm->size);
    if (rc) return rc;
    PP_REQUIRE(bad || !mismatch, "pp_ba_set_communicator: " PP_GROUP_MISMATCH_TEXT);
    PP_REQUIRE(!bad, "pp_ba_set_communicator: a handle of this group renumbered its images from its own shard's co-visibility (pp_ba_problem_desc::ordering = AUTO "
               "without ::covisibility); the handles of a point-sharded group keep the caller's order (PP_ORDERING_NATURAL) or are all created with the group's union "
               "co-visibility, so that every rank lays out the exchanged system alike");
  }
  h->comm = comm; h->allreduce = nullptr; h->allreduce_ctx = nullptr;
  h->group_rank = comm ? comm->rank : 0; h->group_size = comm ? comm->size : 1;
  return ApplyLinearSolverStructure(h);
} PP_API_CATCH("pp_ba_set_communicator")

int pp_ba_get_structure(pp_ba_handle h, int32_t* info) try {
  PP_REQUIRE(h && info, "pp_ba_get_structure: null argument");
  const int T = ((h->n_red + 1 + 63) / 64);
  info[0] = T * (T + 1) / 2;
  info[1] = h->nnz_tiles_natural >= 0 ? h->nnz_tiles_natural : h->num_nz_tiles;
  info[2] = h->num_nz_tiles;
  info[3] = h->pose_new_of_old.empty() ? 0 : 1;
  info[4] = BaSparseActive(h) ? 1 : 0;
  info[5] = h->iterative ? 1 : 0;
  // the chains of the one-launch factorisation (several: a nested-dissection order whose sub-trees are factorised side by side) and its chain steps
  info[6] = 1; info[7] = T;
  if (BaSparseActive(h) && T >= 4 && T <= 128 && !h->tile_nz.empty()) {
    if (h->structure_steps < 0) h->structure_steps = CholeskyChainSteps(T, h->tile_nz.data(), h->sw, &h->structure_chains);      // (planned once per handle; the plan itself is cached per tile map)
    info[6] = h->structure_chains; info[7] = h->structure_steps;
  }
  return PP_OK;
} PP_API_CATCH("pp_ba_get_structure")

int pp_ba_get_intrinsics_layout(pp_ba_handle h, int32_t* info) try {
  PP_REQUIRE(h && info, "pp_ba_get_intrinsics_layout: null argument");
  info[0] = h->NI; info[1] = h->intr_private_nv; info[2] = h->intr_wide_nv; info[3] = h->jcam_stride;
  return PP_OK;
} PP_API_CATCH("pp_ba_get_intrinsics_layout")

int pp_ba_get_trace(pp_ba_handle h, double* trace, int32_t capacity_rows, int32_t* num_rows) try {
  PP_REQUIRE(h && num_rows, "pp_ba_get_trace: null argument");
  const int rows = (int)(h->trace.size() / 7);
  *num_rows = rows;
  if (trace) std::memcpy(trace, h->trace.data(), sizeof(double) * 7 * (size_t)std::min(rows, capacity_rows));
  return PP_OK;
} PP_API_CATCH("pp_ba_get_trace")

int pp_ba_get_timings(pp_ba_handle h, double* ms, int32_t* calls) try {
  PP_REQUIRE(h && ms && calls, "pp_ba_get_timings: null argument");
  for (int i = 0; i < PP_BA_T_COUNT; ++i) { ms[i] = h->timings_ms[i]; calls[i] = h->timing_calls[i]; }
  return PP_OK;
} PP_API_CATCH("pp_ba_get_timings")

int pp_ba_reduced_system(pp_ba_handle h, const pp_ba_options* o, double radius, int32_t* n_out, double* S, double* rhs, int64_t capacity) try {
  PP_REQUIRE(h && o && n_out && radius > 0, "pp_ba_reduced_system: bad argument");
  PP_REQUIRE(!h->iterative, "pp_ba_reduced_system: an iterative (ITERATIVE_SCHUR) handle never forms the reduced system - create the handle with "
             "pp_ba_problem_desc::linear_solver = PP_LINEAR_SOLVER_DIRECT (or PPSFM_BA_LINEAR_SOLVER=direct) for the direct solve");
  PP_HIP_TRY(hipSetDevice(h->device));
  int rc;
  if ((rc = BaEnsureJacobianBuffers(h, 0, h->NI > 0 ? 1 : 0))) return rc;
  if ((rc = EnsureSolverBuffers(h))) return rc;
  PhaseTimer untimed(h, false);
  if ((rc = EvaluateAndScale(h, o, false, untimed))) return rc;
  const int grid = CeilDiv(std::max<int64_t>(6 * (int64_t)h->C, 3 * (int64_t)h->P), 256);
  hipLaunchKernelGGL(k_lm_diagonal, dim3(grid), dim3(256), 0, h->stream, h->C, h->P, h->U, h->V, h->scale_c, h->scale_p, o->min_lm_diagonal,
                     o->max_lm_diagonal, h->diag_c, h->diag_p);
  if ((rc = IntrDiagonal(h, o->min_lm_diagonal, o->max_lm_diagonal))) return rc;
  if ((rc = BaAssembleReducedSystem(h, radius))) return rc;
  const int n = h->n_red;
  *n_out = n;
  if (S) {
    PP_REQUIRE(capacity >= (int64_t)n * n, "pp_ba_reduced_system: capacity %lld < %lld", (long long)capacity, (long long)n * n);
    std::vector<double> full((size_t)h->N * h->N);
    PP_HIP_TRY(hipMemcpyAsync(full.data(), h->S, sizeof(double) * full.size(), hipMemcpyDeviceToHost, h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
    // (the caller's image order: column c of the output sits at internal position at(c) when pp_ba_create renumbered the images)
    // and the position of a vector column in S: pp_ba_impl::spos)
    const bool perm = !h->pose_new_of_old.empty();
    auto at = [&](int c) { const int v = (perm && c < 6 * h->C) ? 6 * h->pose_new_of_old[c / 6] + c % 6 : c; return h->spos_host.empty() ? v : h->spos_host[v]; };
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const int a = at(i), b = at(j);
        S[(size_t)i * n + j] = (b <= a) ? full[(size_t)a * h->N + b] : full[(size_t)b * h->N + a];
      }
    if (rhs) for (int j = 0; j < n; ++j) rhs[j] = full[(size_t)n * h->N + at(j)];
  }
  return PP_OK;
} PP_API_CATCH("pp_ba_reduced_system")

int pp_ba_solve(pp_ba_handle h, const pp_ba_options* o, pp_ba_summary* sum) try {
  PP_REQUIRE(h && o && sum, "pp_ba_solve: null argument");
  PP_REQUIRE(o->max_num_iterations >= 0 && o->initial_trust_region_radius > 0, "pp_ba_solve: bad options");
  PP_HIP_TRY(hipSetDevice(h->device));
  const auto t_start = std::chrono::steady_clock::now();
  std::memset(sum, 0, sizeof(*sum));
  int rc;
  if ((rc = BaEnsureJacobianBuffers(h, 0, h->NI > 0 ? 1 : 0))) return rc;
  if ((rc = EnsureSolverBuffers(h))) return rc;
  hipStream_t s = h->stream;
  h->trace.clear();
  h->linear_solver_iterations = 0;
  for (int i = 0; i < PP_BA_T_COUNT; ++i) { h->timings_ms[i] = 0; h->timing_calls[i] = 0; }
  PP_HIP_TRY(hipMemsetAsync(h->step_c, 0, sizeof(double) * h->N, s));
  PP_HIP_TRY(hipEventRecord(h->ev0, s));
  const StepPlan plan = MakeStepPlan(h, o);

  // iteration 0: evaluate, Jacobi scale, gradient norm
  {
    PhaseTimer timer(h, plan.phase_timings);
    if ((rc = EvaluateAndScale(h, o, plan.fold, timer))) return rc;
    if (!BaInGroup(h) && h->h_scal_dev != nullptr) {      // the scalars reach the host without the copy engine when nothing else touches them after the norms kernel
      const unsigned long long ticket = ++h->ticket_seq;
      if ((rc = LaunchNorms(h, false, plan.fold ? 1 : 0, h->h_scal_dev, ticket))) return rc;
      if ((rc = WaitTicket(h, ticket))) return rc;
    } else {
      if ((rc = LaunchNorms(h, false, plan.fold ? 1 : 0))) return rc;
      if ((rc = ReadScalars(h))) return rc;
    }
    timer.Collect();
  }
  LmPolicy policy(*o, h->trace);
  Speculation spec{h, plan};
  bool go_on = policy.Start(h->h_scal[kCost], h->h_scal[kGradMax]);
  sum->initial_cost = policy.cost;
  sum->num_residuals = (int32_t)(2 * h->M);
  if (!go_on) SetLastError("pp_ba_solve: initial cost is not finite");
  else go_on = !UserStops(o, &policy);

  while (go_on) {
    LmNext next = policy.BeforeStep(spec.pending);
    if (next == LmNext::kResolveFirst) {
      PP_HIP_TRY(hipStreamSynchronize(s));
      spec.Resolve(&policy);
      next = policy.BeforeStep(false);
    }
    if (next == LmNext::kStop) break;

    PhaseTimer timer(h, plan.phase_timings);
    unsigned long long ticket = 0;
    if ((rc = EnqueueTrialStep(h, o, plan, policy.radius, !policy.reuse_diagonal, timer, &ticket))) return rc;
    if ((rc = spec.AwaitTrialStep(ticket))) return rc;
    timer.Collect();
    if (spec.pending) {      // the previous accepted step's evaluation came with this read-back
      spec.Resolve(&policy);
      if (policy.GradientToleranceReached()) {      // drops the trial step that was computed ahead of this test
        if ((rc = spec.Undo(false))) return rc;
        break;
      }
    }
    LmTrialStep step = {h->h_scal[kModelChange], h->h_scal[kCostCand], h->h_scal[kStepNorm2], h->h_scal[kXNorm2], HostFlag(h), false};
    if ((rc = RecoverAfterFlag(h, step.flag, &step.retry_after_timeout))) return rc;
    const LmVerdict verdict = policy.Judge(step);
    // the one place that leaves the speculated state: the candidate stays the current point, or the old point is current again - evaluated again
    // (its Jacobians and sums) exactly when the solve goes on from it
    if ((rc = verdict == LmVerdict::kAccepted ? spec.Keep() : spec.Undo(LmStaysAtOldPoint(verdict)))) return rc;
    switch (verdict) {
      case LmVerdict::kInvalidFailed:
        SetLastError("pp_ba_solve: %d consecutive invalid steps (linear system not positive definite or step without model decrease)", policy.invalid);
        [[fallthrough]];
      case LmVerdict::kParameterTolerance:
      case LmVerdict::kFunctionTolerance:
        go_on = false;
        break;
      case LmVerdict::kRetryAfterTimeout:      // the same step again: no iteration, no row, no callback
        break;
      case LmVerdict::kAccepted:
        if (o->iteration_callback) {     // the callback sees the cost / gradient norm AT the accepted point: wait for its evaluation
          PP_HIP_TRY(hipStreamSynchronize(s));
          spec.Resolve(&policy);
        }
        [[fallthrough]];
      case LmVerdict::kInvalid:
      case LmVerdict::kRejected:
        go_on = !UserStops(o, &policy);
        break;
    }
  }
  PP_HIP_TRY(hipEventRecord(h->ev1, s));
  PP_HIP_TRY(hipEventSynchronize(h->ev1));
  if (spec.pending) spec.Resolve(&policy);
  float ms = 0;
  PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  sum->termination = policy.termination;
  sum->final_cost = policy.cost;
  sum->num_successful_steps = policy.num_successful_steps;
  sum->num_unsuccessful_steps = policy.num_unsuccessful_steps;
  sum->num_iterations = sum->num_successful_steps + sum->num_unsuccessful_steps;
  sum->device_time_s = ms * 1e-3;
  sum->total_time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  sum->num_effective_parameters = h->num_effective_pose_point + h->NI;
  sum->linear_solver_iterations = h->linear_solver_iterations;
  sum->linear_solver = h->iterative ? PP_LINSOLVE_PCG : CholeskyLinsolve(h->chol);
  sum->cholesky_fallbacks = CholeskyFallbacks(h->chol);
  return sum->termination == PP_TERM_FAILURE ? PP_ERR_NUMERIC : PP_OK;
} PP_API_CATCH("pp_ba_solve")

}  // extern "C"
