// K2, K3c and the norms of the LM iteration: what runs on K1's rows before the Schur assembly (ba_schur.hip) and on the linear solve's camera step after it.
//
// K2: k_reduce, and the Jacobi scale / LM diagonal from its blocks.  K3c: k_step_points<kIntr> or, in two passes, k_backsub_points + k_model_cost_apply, its
// A/B partner and the path of a host-callback group.  Norms: k_norms_partial, k_norms_intr, which also hand the scalars to the host.
// Every piece of arithmetic the forms share is ONE function here (TrialPose, PointStep, CameraSideProduct, ObservationTerms, QuadSum, BlockPartialSum of
// ba_impl.hpp, BlockTree256, HandScalarsToHost): the bitwise tests of the forms against each other rest on that.
// The launchers at the end take plain booleans: which form runs is the driver's decision (StepPlan, ba_solver.hip).
#include <algorithm>

#include "ba_impl.hpp"
#include "line_residual.hpp"

namespace ppsfm {

// the sum over the FOUR lanes of a point (lane q holds the point's observations q, q+4, ... in list order): a fixed two-step butterfly, every lane ends with it
template <int N>
__device__ __forceinline__ void QuadSum(double (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) { v[i] += __shfl_xor(v[i], 1, 64); v[i] += __shfl_xor(v[i], 2, 64); }
}

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

// four lanes per point; gid = 4 p + q
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
  QuadSum(v);
  QuadSum(g);
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

// entry (j, j) of a point's V: the upper triangle of the symmetric 3x3, rows one after the other (00 01 02 11 12 22)
__device__ __forceinline__ int PointDiagonalIndex(int j) { return j == 0 ? 0 : (j == 1 ? 3 : 5); }

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
    const double n2 = V[6 * (size_t)p + PointDiagonalIndex(j)];
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
    const double s = scale_p[i];
    diag_p[i] = fmin(fmax(s * s * V[6 * (size_t)p + PointDiagonalIndex(j)], dmin), dmax);
  }
}

// the solution of the reduced system from its column order into the vectors' order (variable intrinsics beside their images' pose columns)
__global__ __launch_bounds__(256) void k_gather_step(int n, const int32_t* __restrict__ spos, const double* __restrict__ x, double* __restrict__ step) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) step[v] = x[spos[v]];
}

// ---- K3c --------------------------------------------------------------------------------------
struct StepArgs {
  int C, P;
  int64_t M;
  const int32_t *pt_start, *pt_obs, *obs_pose, *obs_point;
  const double *Jpose, *Jpoint, *r, *Vinv, *vb, *scale_c, *scale_p, *step_c;
  double *step_p, *partials;
  const double *poses, *points;      // the current point
  double *poses_c, *points_c;        // the trial point
  // variable intrinsics (JkS == nullptr: none): compact scaled Jacobian records, block offsets/widths
  const double* JkS;
  const int32_t *obs_cam, *intr_off, *intr_nv;
  // cand_partials != nullptr: the step kernel also evaluates the cost AT THE TRIAL POINT - each observation applies the step to its own pose and point (the
  // arithmetic of ApplyStepBody) and takes its residual there with `intr` (k_line_eval<0>'s arithmetic and block sums: the same bits), one launch instead of two
  double* cand_partials;
  const double *la, *lb, *lc, *intr;
  int loss_type; double loss_scale;
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
// delta = scale * step, never contracted into the addition that applies it: the stored trial point (TrialPose, ApplyStepBody) and every observation's own
// copy of it (ObservationTerms) must produce the same bits
__device__ __forceinline__ double ScaledStep(double scale, double step) {
#pragma clang fp contract(off)
  return scale * step;
}
// The camera side of one observation's J d: dc = s_c . step_c of its image c, (u0, u1) = J_pose dc from its loaded row jp and, with kIntr, + (J_k diag(s)) . step
// of its intrinsics block (a handle without variable intrinsics has a.JkS == nullptr and adds nothing).
template <bool kIntr>
__device__ __forceinline__ void CameraSideProduct(const StepArgs& a, int64_t o, int c, const double (&jp)[12], double (&dc)[6], double* u0, double* u1) {
  *u0 = 0.0; *u1 = 0.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) { dc[j] = ScaledStep(a.scale_c[6 * c + j], a.step_c[6 * c + j]); *u0 += jp[j] * dc[j]; *u1 += jp[6 + j] * dc[j]; }
  if (kIntr) IntrStepProduct(a, o, u0, u1);
}
// The step of point p from the sum of J_pt^T (camera-side product) over its observations (QuadSum's result): e = vb - Vinv (s . acc); s: the point's scale
__device__ __forceinline__ void PointStep(const StepArgs& a, int p, const double (&acc)[3], double (&s)[3], double (&e)[3]) {
  s[0] = a.scale_p[3 * p]; s[1] = a.scale_p[3 * p + 1]; s[2] = a.scale_p[3 * p + 2];
  const double w0 = s[0] * acc[0], w1 = s[1] * acc[1], w2 = s[2] * acc[2];
  const double* vi = a.Vinv + 6 * (size_t)p;
  e[0] = a.vb[3 * (size_t)p + 0] - (vi[0] * w0 + vi[1] * w1 + vi[2] * w2);
  e[1] = a.vb[3 * (size_t)p + 1] - (vi[1] * w0 + vi[3] * w1 + vi[4] * w2);
  e[2] = a.vb[3 * (size_t)p + 2] - (vi[2] * w0 + vi[4] * w1 + vi[5] * w2);
}
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
// One observation's terms of a trial step in k_step_points: *val loses m . (r + m / 2), m = (m0, m1) + J_pt dp, the camera-side product on entry, and
// *half_rho gains rho(|r|^2) / 2 of the residual at the observation's own trial pose (+) dc and the trial point Xn.
__device__ __forceinline__ void ObservationTerms(const StepArgs& a, int64_t o, int c, const double (&jx)[6], double m0, double m1, const double (&dc)[6],
                                                 const double (&dp)[3], const double (&Xn)[3], double* val, double* half_rho) {
#pragma unroll
  for (int j = 0; j < 3; ++j) { m0 += jx[j] * dp[j]; m1 += jx[3 + j] * dp[j]; }
  *val -= m0 * (a.r[2 * o] + m0 / 2.0) + m1 * (a.r[2 * o + 1] + m1 / 2.0);
  {
    const double* pose = a.poses + 7 * (size_t)c;
    double qn[4];
    QuatPlus(pose, dc[0], dc[1], dc[2], qn);
    const double tn[3] = {pose[4] + dc[3], pose[5] + dc[4], pose[6] + dc[5]};
    const int ck = a.obs_cam[o];
    double res[2];
    LineResidualOnly(ck & 15, a.intr + (size_t)kCamStride * (ck >> 4), qn, tn, Xn, a.la[o], a.lb[o], a.lc[o], res);
    double rho0, rho1;
    LossRho(a.loss_type, a.loss_scale, res[0] * res[0] + res[1] * res[1], &rho0, &rho1);
    *half_rho += 0.5 * rho0;
  }
}

// FOUR lanes per point: one lane per point walked its ~8 observations as eight dependent gather rounds on 391 wavefronts (19 us)
__global__ __launch_bounds__(256) void k_backsub_points(StepArgs a) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int p = gid >> 2, q = gid & 3;
  double acc[3] = {0, 0, 0};
  if (p < a.P) {
    for (int e = a.pt_start[p] + q; e < a.pt_start[p + 1]; e += 4) {
      const int o = a.pt_obs[e];
      const int c = a.obs_pose[o];
      double jp[12], jx[6], dc[6], m0, m1;
      LoadJp(a.Jpose, o, jp);
      LoadJx(a.Jpoint, o, jx);
      CameraSideProduct<true>(a, o, c, jp, dc, &m0, &m1);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += jx[j] * m0 + jx[3 + j] * m1;
    }
  }
  QuadSum(acc);
  if (p >= a.P || q != 0) return;
  double s[3], e[3];
  PointStep(a, p, acc, s, e);
#pragma unroll
  for (int j = 0; j < 3; ++j) a.step_p[3 * (size_t)p + j] = e[j];
}

// model_cost_change = -sum_o (J d)_o . (r_o + (J d)_o / 2)     (TrustRegionMinimizer)
// One observation per lane.  Its camera-side product and its terms are written out here and NOT taken from CameraSideProduct / ObservationTerms: routed
// through them the compiler orders the operands of a * b + c * d sums differently (which product ends up inside the fma), and the last bit of the model
// cost and of the cost at the trial point moves - the latter away from k_line_eval<0>'s, which the fused trial cost has to equal bit for bit.
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
  BlockPartialSum(val, a.partials, half_rho, a.cand_partials);
}

// the trial pose of image i: x (+) delta, delta = scale * step
__device__ __forceinline__ void TrialPose(const StepArgs& a, int i) {
  const double* q = a.poses + 7 * (size_t)i;
  double d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = ScaledStep(a.scale_c[6 * i + j], a.step_c[6 * i + j]);
  double* o = a.poses_c + 7 * (size_t)i;
  QuatPlus(q, d[0], d[1], d[2], o);
  o[4] = q[4] + d[3]; o[5] = q[5] + d[4]; o[6] = q[6] + d[5];
}
// trial point x (+) delta
__device__ __forceinline__ void ApplyStepBody(const StepArgs& a, int i) {
  if (i < a.C) TrialPose(a, i);
  if (i < a.P) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.points_c[3 * (size_t)i + j] = a.points[3 * (size_t)i + j] + ScaledStep(a.scale_p[3 * i + j], a.step_p[3 * (size_t)i + j]);
  }
}

// the model cost change of the step (first obs_blocks workgroups, one per 256 observations) and the trial point x (+) d (the
// others): independent of each other, one launch
__global__ __launch_bounds__(256) void k_model_cost_apply(StepArgs a, int obs_blocks) {
  if ((int)blockIdx.x < obs_blocks) ModelCostBody(a, blockIdx.x);
  else ApplyStepBody(a, ((int)blockIdx.x - obs_blocks) * 256 + threadIdx.x);
}

// The point step, the model cost change, the trial point and the cost there in ONE pass over the observations: four lanes per point as in
// k_backsub_points; a lane keeps its first two observations' rows in registers between the sum that gives the point's step and the terms that need it
// (further observations of a point are loaded again), so the Jacobian is read once where k_backsub_points + k_model_cost_apply read it twice.  Sums: per
// workgroup in lane / wavefront order, then the norms kernel's fixed-order sums - deterministic, a different association than the per-observation kernels'
// (the costs agree to rounding).  The last pose_blocks workgroups write the trial poses.
// kIntr (variable intrinsics): every observation's camera-side product also carries (J_k diag(s)) . step of its intrinsics block, and the trial residual is
// taken with the trial intrinsics a.intr (k_apply_intr runs before this kernel).
template <bool kIntr>
__global__ __launch_bounds__(256) void k_step_points(StepArgs a, int point_blocks) {
  if ((int)blockIdx.x >= point_blocks) {
    const int i = ((int)blockIdx.x - point_blocks) * 256 + threadIdx.x;
    if (i < a.C) TrialPose(a, i);
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
    CameraSideProduct<kIntr>(a, o, w.c, w.jp, w.dc, &w.u0, &w.u1);
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
  QuadSum(acc);
  double dp[3] = {0.0, 0.0, 0.0}, Xn[3] = {0.0, 0.0, 0.0};
  if (live) {
    double s[3], e[3];
    PointStep(a, p, acc, s, e);
#pragma unroll
    for (int j = 0; j < 3; ++j) { dp[j] = ScaledStep(s[j], e[j]); Xn[j] = a.points[3 * (size_t)p + j] + dp[j]; }
    if (q == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { a.step_p[3 * (size_t)p + j] = e[j]; a.points_c[3 * (size_t)p + j] = Xn[j]; }
    }
  }
  double val = 0.0, half_rho = 0.0;
  auto terms = [&](const Row& w) { ObservationTerms(a, w.o, w.c, w.jx, w.u0, w.u1, w.dc, dp, Xn, &val, &half_rho); };
  if (have[0]) terms(R[0]);
  if (have[1]) terms(R[1]);
  for (int e = begin + 8; e < end; e += 4) {
    Row w;
    load(a.pt_obs[e], w);
    terms(w);
  }
  BlockPartialSum(val, a.partials, half_rho, a.cand_partials);
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

// ---- norms and second-stage sums ----------------------------------------------------------------
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

// The fixed-order tree over the 256 threads of a block, strides 128, 64, .., 1: combine(i, j) folds slot j into slot i of EVERY LDS array that rides these
// barriers (a maximum and two sums take one set of them).  The slots are written and a barrier passed before the call; the result is in slot 0 after it.
template <class Combine>
__device__ __forceinline__ void BlockTree256(Combine combine) {
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) combine((int)threadIdx.x, (int)threadIdx.x + s);
    __syncthreads();
  }
}
// sum of n values by the 256 threads of a block in a fixed order -> *out  (the values were written by EARLIER kernels: plain loads)
__device__ __forceinline__ void BlockSumTo(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  BlockTree256([&](int i, int j) { sh[i] += sh[j]; });
  if (threadIdx.x == 0) *out = sh[0];
}
// second stage (a last-block-done fold was measured SLOWER here: ~800 blocks each paying an agent-scope release fence)
__global__ __launch_bounds__(256) void k_sum(const double* __restrict__ partials, int n, double* __restrict__ out) { BlockSumTo(partials, n, out); }

// The last kernel to touch the device scalars hands them to the host: slot b of `scal` by thread b into the pinned host slot (relaxed system-scope stores),
// then - ticket != 0 - a system-scope release fence on the first wavefront and the ticket by thread 0, LAST: the host polls it (WaitTicket, ba_solver.hip).
// A copy and an event record in its place cost ~4 us of copy engine and a ~5 us hole in the stream.  Called by (at least) the first wavefront of ONE
// workgroup, behind a barrier that orders the workgroup's own stores to `scal`.  kTicketSlot of `scal` carries a group's failure bits, not a scalar.
// norms (or null: every slot from memory): kGradMax, kStepNorm2, kXNorm2 when the caller's thread 0 stored them to `scal` only just now - those stores are
// not ordered before the other threads' loads, so the three values come from the caller (its LDS) and not from memory.
__device__ __forceinline__ void HandScalarsToHost(const double* __restrict__ scal, double* __restrict__ host_out, unsigned long long ticket, const double* norms) {
  static_assert(kStepNorm2 == kGradMax + 1 && kXNorm2 == kGradMax + 2, "the three norms are adjacent slots");
  const int b = threadIdx.x;
  if (b < kNumScalars && b != kTicketSlot) {
    unsigned long long v;
    if (norms && b >= kGradMax && b <= kXNorm2) v = __double_as_longlong(norms[b - kGradMax]);
    else v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(scal) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (ticket != 0 && b < 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");        // system scope
    if (b == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out) + kTicketSlot, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
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
  // with variable intrinsics THIS kernel is the last one to touch the scalars (k_norms_partial hands them over without them)
  if (host_out) HandScalarsToHost(scal, host_out, ticket, nullptr);
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
  auto tree = [&] { BlockTree256([&](int i, int j) { smax[i] = fmax(smax[i], smax[j]); sstep[i] += sstep[j]; sx[i] += sx[j]; }); };
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
    tree();
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = smax[0]; part[3 * blockIdx.x + 1] = sstep[0]; part[3 * blockIdx.x + 2] = sx[0]; }
  }
  // the block that finishes last (of ALL blocks) combines the per-block norm partials (fixed order: block b -> slot b, then the
  // same tree) and, when asked to, hands the scalars to the host
  if (LastBlockDone(done_counter, (int)gridDim.x)) {
    const int b = threadIdx.x;
    const bool in = b < norm_blocks;
    smax[b] = in ? __hip_atomic_load(part + 3 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    sstep[b] = in ? __hip_atomic_load(part + 3 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    sx[b] = in ? __hip_atomic_load(part + 3 * b + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    tree();
    if (b == 0) {
      __hip_atomic_store(scal + kGradMax, smax[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(scal + kStepNorm2, sstep[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(scal + kXNorm2, sx[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (host_out) {
      __syncthreads();
      const double norms[3] = {smax[0], sstep[0], sx[0]};      // (the other slots - sums of other blocks / earlier kernels - come from memory)
      HandScalarsToHost(scal, host_out, ticket, norms);
    }
  }
}

// ---- launchers (declared in ba_impl.hpp) ----------------------------------------------------------
static int Launched() { PP_HIP_TRY(hipGetLastError()); return PP_OK; }
int BaReduceNormalEquations(pp_ba_impl* h) {
  hipLaunchKernelGGL(k_reduce, dim3(h->C + CeilDiv(4 * (int64_t)h->P, 256)), dim3(256), 0, h->stream, h->C, h->P, h->pose_start, h->pose_obs, h->pt_start, h->pt_obs,
                     h->Jpose, h->Jpoint, h->r, h->U, h->gc, h->V, h->gp);
  return Launched();
}
static int ColumnGrid(const pp_ba_impl* h) { return CeilDiv(std::max<int64_t>(6 * (int64_t)h->C, 3 * (int64_t)h->P), 256); }      // a thread per pose column and per point column
int BaJacobiScale(pp_ba_impl* h, int jacobi) {
  hipLaunchKernelGGL(k_jacobi_scale, dim3(ColumnGrid(h)), dim3(256), 0, h->stream, h->C, h->P, h->U, h->V, h->pose_const, h->tvec_mask, h->point_const, jacobi,
                     h->scale_c, h->scale_p);
  return Launched();
}
int BaLmDiagonal(pp_ba_impl* h, double dmin, double dmax) {
  hipLaunchKernelGGL(k_lm_diagonal, dim3(ColumnGrid(h)), dim3(256), 0, h->stream, h->C, h->P, h->U, h->V, h->scale_c, h->scale_p, dmin, dmax, h->diag_c, h->diag_p);
  return Launched();
}
int BaGatherStep(pp_ba_impl* h) {
  if (h->spos_identity) return PP_OK;
  hipLaunchKernelGGL(k_gather_step, dim3(CeilDiv(h->n_red, 256)), dim3(256), 0, h->stream, h->n_red, h->spos, h->step_s, h->step_c);
  return Launched();
}
int BaLaunchStepKernels(pp_ba_impl* h, bool fused_step, bool fused_trial_cost, bool sum_model_cost) {
  StepArgs a;
  a.C = h->C; a.P = h->P; a.M = h->M;
  a.pt_start = h->pt_start; a.pt_obs = h->pt_obs; a.obs_pose = h->obs_pose; a.obs_point = h->obs_point;
  a.Jpose = h->Jpose; a.Jpoint = h->Jpoint; a.r = h->r; a.Vinv = h->Vinv; a.vb = h->vb;
  a.scale_c = h->scale_c; a.scale_p = h->scale_p; a.step_c = h->step_c; a.step_p = h->step_p; a.partials = h->partials + h->partials_stride;   // second region: K1's partials stay valid
  a.poses = h->poses; a.points = h->points; a.poses_c = h->poses_c; a.points_c = h->points_c;
  a.JkS = h->NI > 0 ? h->JkS_intr : nullptr; a.obs_cam = h->obs_cam; a.intr_off = h->intr_off; a.intr_nv = h->intr_nv;
  a.cand_partials = fused_trial_cost ? h->partials : nullptr; a.la = h->la; a.lb = h->lb; a.lc = h->lc; a.loss_type = h->loss_type; a.loss_scale = h->loss_scale;
  a.intr = fused_step && h->NI > 0 ? h->intr_c : h->intr;      // (k_step_points takes the trial residuals with the trial intrinsics)
  hipStream_t s = h->stream;
  const int grid_obs = h->num_partials, point_blocks = CeilDiv(4 * (int64_t)h->P, 256);
  h->trial_partials = fused_step ? point_blocks : 0;
  // the trial intrinsics, ahead of either form: k_step_points<true> takes its trial residuals with them, the two-kernel form's cost-only evaluation after it
  if (h->NI > 0)
    hipLaunchKernelGGL(k_apply_intr, dim3(CeilDiv(h->K * kCamStride, 256)), dim3(256), 0, s, h->K, h->C, h->intr_off, h->intr_col, h->intr, h->scale_c, h->step_c, h->intr_c);
  if (fused_step) {
    hipLaunchKernelGGL(h->NI > 0 ? k_step_points<true> : k_step_points<false>, dim3(point_blocks + CeilDiv(h->C, 256)), dim3(256), 0, s, a, point_blocks);
  } else {
    hipLaunchKernelGGL(k_backsub_points, dim3(point_blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_model_cost_apply, dim3(grid_obs + CeilDiv(std::max(h->C, h->P), 256)), dim3(256), 0, s, a, grid_obs);
  }
  if (sum_model_cost) hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, s, a.partials, grid_obs, h->scal + kModelChange);
  return Launched();
}
int BaLaunchNorms(pp_ba_impl* h, bool with_step, int fold, double* host_slot, unsigned long long ticket) {
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
  return Launched();
}

}  // namespace ppsfm
