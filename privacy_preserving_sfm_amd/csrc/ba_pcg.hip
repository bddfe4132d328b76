// K3-it — matrix-free preconditioned conjugate gradients on the point-Schur complement of the camera system.
//
// Replaces the linear solve Ceres performs for bundle adjustments of more than 1000 images, where the reference switches to
// ITERATIVE_SCHUR with the SCHUR_JACOBI preconditioner (src/optim/bundle_adjustment.cc:283-286; iteration cap
// max_linear_solver_iterations = 200, bundle_adjustment.h:87).  Ceres is third-party and absent: the loop restates its published
// ConjugateGradientsSolver (*** parity unpinned ***, like the LM driver): x0 = 0, explicit residual every 10th iteration,
// termination on the quadratic-model criterion  i (Q_i - Q_{i-1}) / Q_i < eta  (the residual criterion is switched off by the
// trust-region strategy), preconditioner = inverses of the diagonal blocks of S per PARAMETER BLOCK (rotation tangent 3x3, translation
// 3x3).  oracle/bundle_adjustment.h SchurJacobiConjugateGradients is the CPU restatement the tests compare with.
//
// The reduced system S = U + D_c^2 - W (V + D_p^2)^-1 W^T is never formed (at 5000 images it would be 7 GB and a second of
// factorisation): S v is applied from the per-observation records k_prepare builds anyway ([T_o | J_c,o s_c | J_p,o], 192 bytes):
//   k_pcg_points   per point (four lanes):   a_p = sum_{o in p} J_p,o^T (J^_c,o v_c(o))
//   k_pcg_images   per image (one workgroup): (S v)_c = sum_{o in c} J^_c,o^T (J^_c,o v_c - T_o a_p(o)) + d_c v_c, and v_c . (S v)_c
// both HBM/L2-bound gathers of 144 of a record's 192 bytes per observation (algorithmic: 2 x 144 B per observation and product).
// The vector updates and dot products (fixed order: deterministic) of an iteration: k_pcg_step (many workgroups); the termination test and
// the new direction: k_pcg_wide_b (a second launch).  The host enqueues a few iterations at a time and reads the state back; once the loop
// has ended the kernels already in the stream return at their first instruction.  That four-launch form (k_pcg_points, k_pcg_images,
// k_pcg_step, k_pcg_wide_b) is what point-sharded groups and variable intrinsics run.
// DEFAULT otherwise: three launches per iteration (k_pcg_points_q, k_pcg_images_q, k_pcg_step - see below): the product kernels take the
// decision and form the direction themselves, k_pcg_wide_b is not launched.  PPSFM_PCG_FUSED=0 selects the four-launch form (tests compare
// the two).  Both forms share the rules of the loop (PcgAdvance) and the vector step (k_pcg_step); each sums in its own fixed order.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "ba_impl.hpp"
#include "host_ticket.hpp"
#include "resource_pool.hpp"

namespace ppsfm {

constexpr int kResidualResetPeriod = 10;      // ConjugateGradientsSolver::Options::residual_reset_period
enum { kPcgRunning = 0, kPcgConverged = 1, kPcgNoConvergence = 2, kPcgFailure = 3 };

// inverse of a symmetric 3x3 block that sits in a 6x6 row-major diagonal block of S (D: its first entry; rotation tangent: rows 0.., translation:
// rows 3..).  false: the block is not positive, or not finite
__device__ __forceinline__ bool InverseSym3(const double* __restrict__ D, double* o) {
  const double a = D[0], b = D[1], cc = D[2], d = D[7], e = D[8], f = D[14];
  const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d;
  const double det = a * c00 + b * c01 + cc * c02;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
  o[3] = c01 * id; o[4] = (a * f - cc * cc) * id; o[5] = (b * cc - a * e) * id;
  o[6] = c02 * id; o[7] = (b * cc - a * e) * id; o[8] = (a * d - b * b) * id;
  return det > 0.0 && isfinite(det);
}

__global__ __launch_bounds__(256) void k_pcg_points(int P, const int32_t* __restrict__ pt_start, const int32_t* __restrict__ pt_obs,
                                                    const int32_t* __restrict__ obs_pose, const double* __restrict__ rec, const double* __restrict__ v,
                                                    double* __restrict__ a, const PcgState* __restrict__ st, const double2* __restrict__ tk) {
  if (st->done) return;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int p = gid >> 2, q = gid & 3;
  double acc[3] = {0.0, 0.0, 0.0};
  if (p < P) {
    for (int e = pt_start[p] + q; e < pt_start[p + 1]; e += 4) {
      const int o = pt_obs[e];
      const int c = obs_pose[o];
      const double2* rj = reinterpret_cast<const double2*>(RecJ(rec, (size_t)o));      // J_pose,o s_c (2 x 6) then J_pt,o (2 x 3): 144 contiguous bytes
      double jp[12], jx[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) { const double2 t = rj[i]; jp[2 * i] = t.x; jp[2 * i + 1] = t.y; }
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double2 t = rj[6 + i]; jx[2 * i] = t.x; jx[2 * i + 1] = t.y; }
      double m0 = 0.0, m1 = 0.0;
      if (tk) { const double2 t = tk[o]; m0 = t.x; m1 = t.y; }      // (variable intrinsics: J^_k,o v_k)
#pragma unroll
      for (int j = 0; j < 6; ++j) { const double d = v[6 * (size_t)c + j]; m0 += jp[j] * d; m1 += jp[6 + j] * d; }
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += jx[k] * m0 + jx[3 + k] * m1;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {      // the four lanes of a point: fixed two-step butterfly
    acc[k] += __shfl_xor(acc[k], 1);
    acc[k] += __shfl_xor(acc[k], 2);
  }
  if (p < P && q == 0) { a[3 * (size_t)p] = acc[0]; a[3 * (size_t)p + 1] = acc[1]; a[3 * (size_t)p + 2] = acc[2]; }
}

__global__ __launch_bounds__(256) void k_pcg_images(int C, const int32_t* __restrict__ pose_start, const int32_t* __restrict__ pose_obs,
                                                    const int32_t* __restrict__ obs_point, const double* __restrict__ rec, const double* __restrict__ v,
                                                    const double* __restrict__ a, const double* __restrict__ scale_c, const double* __restrict__ diag_c,
                                                    double inv_radius, double* __restrict__ out, double* __restrict__ dotp, const PcgState* __restrict__ st,
                                                    int add_diagonal, const double2* __restrict__ tk, double2* __restrict__ w_out) {
  if (st->done) return;
  __shared__ double red[4][6];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double vc[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) vc[j] = v[6 * (size_t)c + j];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int e = pose_start[c] + (int)threadIdx.x; e < pose_start[c + 1]; e += 256) {
    const int o = pose_obs[e];
    const int p = obs_point[o];
    const double2* rt = reinterpret_cast<const double2*>(RecT(rec, (size_t)o));      // T_o (2 x 3) then J_pose,o s_c (2 x 6): 144 contiguous bytes
    double t[6], jp[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const double2 x = rt[i]; t[2 * i] = x.x; t[2 * i + 1] = x.y; }
#pragma unroll
    for (int i = 0; i < 6; ++i) { const double2 x = rt[3 + i]; jp[2 * i] = x.x; jp[2 * i + 1] = x.y; }
    const double a0 = a[3 * (size_t)p], a1 = a[3 * (size_t)p + 1], a2 = a[3 * (size_t)p + 2];
    double m0 = -(t[0] * a0 + t[1] * a1 + t[2] * a2), m1 = -(t[3] * a0 + t[4] * a1 + t[5] * a2);
    if (tk) { const double2 tt = tk[o]; m0 += tt.x; m1 += tt.y; }      // (variable intrinsics: J^_k,o v_k)
#pragma unroll
    for (int j = 0; j < 6; ++j) { m0 += jp[j] * vc[j]; m1 += jp[6 + j] * vc[j]; }
    if (w_out) w_out[o] = make_double2(m0, m1);      // (what the per-camera sums J^_k^T m take)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] += jp[j] * m0 + jp[6 + j] * m1;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) acc[j] = WaveSum(acc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) red[wv][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double s = scale_c[6 * (size_t)c + j];
      // constant column: identity row (as the assembled system has it); in a point-sharded group the diagonal term is added once, by rank 0
      const double d = add_diagonal ? ((s == 0.0) ? 1.0 : diag_c[6 * (size_t)c + j] * inv_radius) : 0.0;
      const double qv = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j] + d * vc[j];
      out[6 * (size_t)c + j] = qv;
      dot += vc[j] * qv;
    }
    if (dotp) dotp[c] = dot;      // (a group sums the products of all ranks first: v . S v is taken from the reduced vector then)
  }
}

// ---- the vector step over MANY workgroups (a single workgroup was 12.5 us at 1100 images and 30 us at 4000 - the longest kernel of an
// iteration there).  A thread per 3 x 3 parameter block:
//   k_pcg_step     alpha = rho / (p . S p) from the per-image parts (every workgroup sums them itself, in the same order: the same
//                  bits everywhere, no exchange), x += alpha p, r -= alpha q (or the explicit residual), z = M^-1 r, and this
//                  workgroup's parts of Q = -x . (b + r) / ... and of r . z; at the start of a solve also M^-1 itself
//   k_pcg_wide_b   (four-launch form) every workgroup sums the parts, takes the termination decision (PcgAdvance) and updates its
//                  slice of the direction p = z + beta p
// The state is read by every workgroup of a launch and written by workgroup 0 of k_pcg_wide_b (of k_pcg_images_q in the three-launch
// form): it ping-pongs between two copies (a workgroup dispatched late must not find the NEXT iteration's state), the host tracks which
// one is current.
constexpr int kWideThreads = 256;
// Variable intrinsics on the iterative path (bundle_adjustment.cc:283-286 with :490-528): the NI intrinsics columns follow the 6 C pose columns in
// every vector of the loop.  Their part of the operator, matrix-free like the rest:
//   k_pcg_cam_t    t_o = J^_k,o v_k per observation (the scaled compact intrinsics Jacobians k_intr_prepare builds)
//   k_pcg_points / k_pcg_images add t_o to J^_c,o v_c; the image kernel also stores m_o = J^_c,o v_c + t_o - T_o a_p
//   k_pcg_cam_q    (S v)_k = sum_{o of camera k} J^_k,o^T m_o + d_k v_k: per-camera chunks of the observations (the lists of k_intr_sums), then one
//                  wavefront per camera adds the chunks in order and forms the camera's part of v . S v
// The preconditioner's intrinsics blocks (SCHUR_JACOBI: one block per parameter block) are the diagonal blocks S_kk, assembled per trial radius
// from the (k, k) pair lists alone (IntrAssemble into pcg_Scomp) and inverted by k_pcg_intr_inverse; the vector step treats a camera's block in
// one thread (workgroups behind the pose workgroups of k_pcg_step<true> / k_pcg_wide_b).  The four-launch form of the loop runs these (7 launches per iteration).
struct PcgIntr {
  int K = 0, pose_blocks = 1 << 30;      // cameras; the workgroups before the intrinsics' ones
  const int32_t* intr_off = nullptr; const int32_t* intr_nv = nullptr;
  const double* binvI = nullptr;         // [NI][12]: row i of the intrinsics columns holds its block's row of the inverse
};
__global__ __launch_bounds__(256) void k_pcg_cam_t(int64_t M, int C, const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ intr_off,
                                                   const int32_t* __restrict__ intr_nv, const double* __restrict__ JkS, const double* __restrict__ v,
                                                   double2* __restrict__ tk, const PcgState* __restrict__ st) {
  if (st->done) return;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= M) return;
  const int k = obs_cam[o] >> 4;
  const int off = intr_off[k];
  double t0 = 0.0, t1 = 0.0;
  if (off >= 0) {
    const int nv = intr_nv[k];
    const double* j = JkS + (size_t)2 * kCamStride * o;
    const double* vk = v + 6 * (size_t)C + off;
    for (int c = 0; c < nv; ++c) { const double d = vk[c]; t0 += j[c] * d; t1 += j[kCamStride + c] * d; }
  }
  tk[o] = make_double2(t0, t1);
}
__global__ __launch_bounds__(256) void k_pcg_cam_q(const int32_t* __restrict__ chunk, const int32_t* __restrict__ cam_obs, const double* __restrict__ JkS,
                                                   const double2* __restrict__ w, double* __restrict__ partial, const PcgState* __restrict__ st) {
  if (st->done) return;
  __shared__ double red[4][12];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e0 = chunk[3 * blockIdx.x + 1], e1 = chunk[3 * blockIdx.x + 2];
  double acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.0;
  for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
    const int o = cam_obs[e];
    const double* j = JkS + (size_t)2 * kCamStride * o;
    const double2 m = w[o];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] += j[c] * m.x + j[kCamStride + c] * m.y;
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = WaveSum(acc[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) red[wv][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < 12) partial[(size_t)blockIdx.x * 24 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
// one wavefront per camera: the chunk sums in chunk order, the damping term, the camera's part of v . S v
__global__ __launch_bounds__(64) void k_pcg_cam_q_reduce(int C, const int32_t* __restrict__ cam_chunk, const int32_t* __restrict__ intr_off, const int32_t* __restrict__ intr_nv,
                                                         const double* __restrict__ partial, const double* __restrict__ v, const double* __restrict__ diag_c, double inv_radius,
                                                         double* __restrict__ out, double* __restrict__ dotp, const PcgState* __restrict__ st, int add_diag) {      // add_diag: this rank carries the damping term (rank 0 of a group)
  if (st->done) return;
  const int k = blockIdx.x, t = threadIdx.x;
  const int off = intr_off[k];
  double term = 0.0;
  if (off >= 0 && t < intr_nv[k]) {
    double s = 0.0;
    int c = cam_chunk[k];
    const int ce = cam_chunk[k + 1];
    for (; c + 8 <= ce; c += 8) {      // eight partials in flight, added in chunk order (one shared camera at 1100 images: 86 chunks, 15.8 us one load at a time)
      double v8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v8[u] = partial[(size_t)(c + u) * 24 + t];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v8[u];
    }
    for (; c < ce; ++c) s += partial[(size_t)c * 24 + t];
    const size_t idx = 6 * (size_t)C + off + t;
    const double qv = add_diag ? s + diag_c[idx] * inv_radius * v[idx] : s;
    out[idx] = qv;
    term = v[idx] * qv;
  }
  double dot = 0.0;
#pragma unroll
  for (int j = 0; j < 12; ++j) dot += __shfl(term, j);
  if (t == 0) dotp[C + k] = dot;
}
// inverses of the intrinsics' diagonal blocks (Gauss-Jordan on the symmetric positive definite block, as the oracle does): a thread per camera
__global__ __launch_bounds__(64) void k_pcg_intr_inverse(int K, const int32_t* __restrict__ intr_off, const int32_t* __restrict__ intr_nv, const double* __restrict__ Scomp,
                                                         double* __restrict__ binvI, int32_t* __restrict__ flag) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const int off = intr_off[k];
  if (off < 0) return;
  const int m = intr_nv[k];
  double A[12][12], I[12][12];
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) { A[i][j] = Scomp[12 * (size_t)(off + i) + j]; I[i][j] = i == j ? 1.0 : 0.0; }
  bool bad = false;
  for (int c = 0; c < m; ++c) {
    const double piv = A[c][c];
    if (!(piv > 0.0) || !isfinite(piv)) { bad = true; break; }
    for (int j = 0; j < m; ++j) { A[c][j] /= piv; I[c][j] /= piv; }
    for (int r = 0; r < m; ++r) {
      if (r == c) continue;
      const double f = A[r][c];
      for (int j = 0; j < m; ++j) { A[r][j] -= f * A[c][j]; I[r][j] -= f * I[c][j]; }
    }
  }
  if (bad) atomicOr(flag, 1);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < 12; ++j) binvI[12 * (size_t)(off + i) + j] = (j < m && !bad) ? I[i][j] : 0.0;
}
// per-image parts of p . q for a point-sharded group, where q is the all-reduced product (k_pcg_images' own parts would be this rank's only)
__global__ __launch_bounds__(256) void k_pcg_dot(int C, const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ dotp,
                                                 const PcgState* __restrict__ st, int K, const int32_t* __restrict__ intr_off, const int32_t* __restrict__ intr_nv) {      // K > 0: the cameras' parts behind the images'
  if (st->done) return;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C + K) return;
  double d = 0.0;
  if (c < C) {
#pragma unroll
    for (int j = 0; j < 6; ++j) d += p[6 * (size_t)c + j] * q[6 * (size_t)c + j];
  } else {
    const int k = c - C, off = intr_off[k];
    if (off >= 0) for (int j = 0; j < intr_nv[k]; ++j) d += p[6 * (size_t)C + off + j] * q[6 * (size_t)C + off + j];
  }
  dotp[c] = d;
}
__device__ __forceinline__ double WideBlockSum(double v, double* red) {      // fixed order, result in every thread
  v = WaveSum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
// ---- the rules of the loop (ConjugateGradientsSolver's tests, in its order): written once, for both forms.  The callers differ in who sums the parts
// k_pcg_step left - part: 4 doubles per workgroup [Q part (start: |b|^2 part) | r . z part | status | alpha] - and in what order.
struct PcgDecision { PcgState s; double beta; int run; int failed; };

// (status, alpha) of the vector step that has just run: a step that ended the loop (indefinite direction, overflow) ends it here.  Alone, this is what
// follows the x-only step of a residual-reset iteration.
__device__ __forceinline__ PcgDecision PcgCarryOver(const PcgState& s, int status, double alpha) {
  PcgDecision d;
  d.s = s; d.beta = 0.0; d.run = 0; d.failed = 0;
  d.s.alpha = alpha;
  if (status != kPcgRunning) { d.s.done = 1; d.s.status = status; d.failed = status == kPcgFailure; return d; }
  d.run = 1;
  return d;
}
// The decision after iteration it_prev (0: the start of a solve) from the totals a0 (Q; at the start |b|^2) and a1 (r . z): the state as it is from
// here on, beta of the next direction, run = the loop goes on.
__device__ __forceinline__ PcgDecision PcgAdvance(const PcgState& s, int it_prev, double a0, double a1, int status, double alpha, double eta, int max_iterations) {
  PcgDecision d = PcgCarryOver(s, status, alpha);
  if (!d.run) return d;
  d.run = 0;
  auto finish = [&](int st_code) { d.s.done = 1; d.s.status = st_code; d.failed = st_code == kPcgFailure; };
  if (it_prev == 0) {
    d.s.iter = 1; d.s.done = 0; d.s.status = kPcgRunning; d.s.rho = 1.0; d.s.Q0 = 0.0; d.s.norm_b = sqrt(a0); d.s.alpha = 0.0;
    if (!(a0 > 0.0)) { d.s.iter = 0; finish(a0 == 0.0 ? kPcgConverged : kPcgFailure); return d; }
  } else {
    const double zeta = it_prev * (a0 - d.s.Q0) / a0;
    if (zeta < eta) { finish(kPcgConverged); return d; }
    if (it_prev >= max_iterations) { finish(kPcgNoConvergence); return d; }
    d.s.Q0 = a0; d.s.iter = it_prev + 1;
  }
  const double rho = a1;
  if (rho == 0.0 || isinf(rho) || isnan(rho)) { finish(kPcgFailure); return d; }
  if (it_prev != 0) {
    d.beta = rho / d.s.rho;
    if (d.beta == 0.0 || isinf(d.beta) || isnan(d.beta)) { finish(kPcgFailure); return d; }
  }
  d.s.rho = rho;
  d.run = 1;
  return d;
}

// mode 0: start (it = 0); 1: an iteration's end; 3: after the x-only step of a residual-reset iteration (only carries a failure of that step over)
__global__ __launch_bounds__(kWideThreads) void k_pcg_wide_b(int mode, int it, int C, int G, const double* __restrict__ z, double* __restrict__ p,
                                                             const double* __restrict__ part, const PcgState* __restrict__ st, PcgState* __restrict__ st_out,
                                                             double eta, int max_iterations, int32_t* __restrict__ flag, PcgIntr in) {
  __shared__ double red[4];
  const PcgState s = *st;
  const int tid = threadIdx.x;
  const bool writer = blockIdx.x == 0 && tid == 0;
  if (mode != 0 && (s.done || s.iter != it)) { if (writer) *st_out = s; return; }      // (both copies say "done" from here on)
  double a0 = 0.0, a1 = 0.0;
  for (int w = tid; w < G; w += kWideThreads) { a0 += part[4 * (size_t)w]; a1 += part[4 * (size_t)w + 1]; }
  a0 = WideBlockSum(a0, red);
  a1 = WideBlockSum(a1, red);
  const int status = (int)part[2];
  const double alpha = part[3];
  const PcgDecision d = mode == 3 ? PcgCarryOver(s, status, alpha) : PcgAdvance(s, it, a0, a1, status, alpha, eta, max_iterations);
  if (writer) { *st_out = d.s; if (d.failed) atomicOr(flag, 1); }
  if (!d.run || mode == 3) return;
  const int g = blockIdx.x * kWideThreads + tid;
  if ((int)blockIdx.x >= in.pose_blocks) {      // the intrinsics blocks
    const int k = ((int)blockIdx.x - in.pose_blocks) * kWideThreads + tid;
    const int off = k < in.K ? in.intr_off[k] : -1;
    if (off >= 0) {
      const size_t i0 = 6 * (size_t)C + off;
      for (int j = 0; j < in.intr_nv[k]; ++j) p[i0 + j] = (mode == 0) ? z[i0 + j] : z[i0 + j] + d.beta * p[i0 + j];
    }
  } else if (g < 2 * C) {
    const size_t i = 3 * (size_t)g;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[i + k] = (mode == 0) ? z[i + k] : z[i + k] + d.beta * p[i + k];
  }
}

// ---- THREE launches per iteration (the default outside point-sharded groups).  k_pcg_wide_b is not launched: the decision it takes and the
// direction it writes are taken by the product kernels themselves.
//   k_pcg_points_q     every wavefront sums the parts of Q and r . z k_pcg_step left (the same order everywhere: the same bits, no
//                      exchange), takes the termination decision and beta, and forms the direction of the images it touches on the
//                      fly: p_c = z_c + beta p_old,c (both vectors are L2 resident: 53 KB at 1100 images)
//   k_pcg_images_q     the same decision, p_c once more for ITS image - stored: the direction buffer ping-pongs, like the state that workgroup 0
//                      writes - then (S p)_c and the image's part of p . S p
//   k_pcg_step         alpha, x, r, z = M^-1 r, parts (the vector step of both forms, see there)
// and the index walks are one level shorter: (observation, image) pairs per point-list entry and (observation, point) pairs per image-list
// entry (k_pcg_entries, built once per handle), two, four or eight records of a point in flight by the mean track.  The kernels of an iteration are
// bound by the LATENCY of their dependent loads (344 + 1100 + 9 workgroups at 1100 images, a few microseconds each), not by bytes.
// The decision after iteration it_prev (0: the start of a solve), by one wavefront for itself (k_pcg_wide_b's, with the parts summed by lanes).
__device__ __forceinline__ PcgDecision PcgDecide(int it_prev, int G, const double* __restrict__ part, const PcgState* __restrict__ st, double eta,
                                                 int max_iterations) {
  const PcgState s = *st;
  const int lane = threadIdx.x & 63;
  double a0 = 0.0, a1 = 0.0;
  for (int w = lane; w < G; w += 64) { a0 += part[4 * (size_t)w]; a1 += part[4 * (size_t)w + 1]; }
  const int status = (int)part[2];
  const double alpha = part[3];
  if (it_prev != 0 && (s.done || s.iter != it_prev)) return PcgDecision{s, 0.0, 0, 0};      // (ended before: both copies of the state keep saying so)
  a0 = WaveSum(a0); a1 = WaveSum(a1);
  return PcgAdvance(s, it_prev, a0, a1, status, alpha, eta, max_iterations);
}
// the x-only step of a residual-reset iteration left (status, alpha) in the parts: carries a failure of that step over (k_pcg_wide_b's mode 3)
__device__ __forceinline__ PcgDecision PcgCarry(int it, const double* __restrict__ part, const PcgState* __restrict__ st) {
  const PcgState s = *st;
  const int status = (int)part[2];
  const double alpha = part[3];
  if (s.done || s.iter != it) return PcgDecision{s, 0.0, 0, 0};
  return PcgCarryOver(s, status, alpha);
}
// has the loop ended before this launch (the test PcgDecide / PcgCarry begin with)?  One load, asked for together with the list entry: a launch enqueued
// beyond the loop's end leaves after ONE round trip instead of after the record fetch it would never use
__device__ __forceinline__ bool PcgEnded(const PcgState* __restrict__ st, int it, bool dir) {
  const int2 w = *reinterpret_cast<const int2*>(&st->iter);      // (iter, done)
  return (!dir || it != 0) && (w.y != 0 || w.x != it);
}
__device__ __forceinline__ double PcgDirection(bool first, double beta, double z, double p_old) { return first ? z : fma(beta, p_old, z); }

__global__ __launch_bounds__(256) void k_pcg_entries(int64_t M, const int32_t* __restrict__ pt_obs, const int32_t* __restrict__ obs_pose,
                                                     const int32_t* __restrict__ pose_obs, const int32_t* __restrict__ obs_point,
                                                     int2* __restrict__ pt_entry, int2* __restrict__ pose_entry) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= M) return;
  const int o = pt_obs[e], o2 = pose_obs[e];
  pt_entry[e] = make_int2(o, obs_pose[o]);
  pose_entry[e] = make_int2(o2, obs_point[o2]);
}

// the decision alone, for the host's look at the loop: writes the state as it will be after the decision on iteration `it`
// (`out` is pinned host memory: the state, then - released at system scope - the ticket the host spins on: a stream synchronisation wakes the
// caller ~10 us after the kernel has ended, and every microsecond of it is an idle device in the middle of an LM iteration)
__global__ __launch_bounds__(64) void k_pcg_decide(int it, int G, const double* __restrict__ part, const PcgState* __restrict__ st, PcgState* __restrict__ out,
                                                   double eta, int max_iterations, int32_t* __restrict__ flag, int32_t ticket) {
  const PcgDecision d = PcgDecide(it, G, part, st, eta, max_iterations);
  if (threadIdx.x == 0) {
    PcgState o = d.s;
    o.pad_ = 0;
    *out = o;
    if (d.failed) atomicOr(flag, 1);
    __hip_atomic_store(&out->pad_, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- the product kernels with COALESCED record reads.  A lane that reads its own record takes nine 16-byte pieces at a 192-byte stride: 64
// distinct lines per wave-level load, ~15 line requests per record and product - the texture-address path bounded that first form of the
// product kernels, not bytes and not latency.  Here FOUR lanes share a record: in load i lane q takes piece 4 i + q, so a quad reads 64 contiguous
// bytes per load and the record in three.  What a lane holds (pieces of 2 doubles: T = pieces 0-2, J_pose row 0 = 3-5, row 1 = 6-8, J_point = 9-11):
//   lane 0: T[0:2]   Jc0[2:4]  Jc1[4:6]          lane 2: T[4:6]    Jc1[0:2]  Jx[2:4]
//   lane 1: T[2:4]   Jc0[4:6]  Jx[0:2]           lane 3: Jc0[0:2]  Jc1[2:4]  Jx[4:6]
// every lane forms the terms of the two-vector m = J_c v (- T a) it has the factors for, the quad adds them up (two DPP moves), and every lane adds
// the products of m with ITS pieces of J_point (points) / J_pose (images) to private sums that are sorted into components once, at the end.
__device__ __forceinline__ double QuadSum(double v) {
  v += DppMove<0xB1>(v);       // quad_perm [1,0,3,2]
  v += DppMove<0x4E>(v);       // quad_perm [2,3,0,1]
  return v;
}
struct QuadRecord { double2 r0, r1, r2; };
__device__ __forceinline__ QuadRecord LoadQuadRecord(const double* __restrict__ rec, int o, int q) {
  const double2* base = reinterpret_cast<const double2*>(rec + kRecStride * (size_t)o);
  QuadRecord r;
  r.r0 = base[q]; r.r1 = base[4 + q]; r.r2 = base[8 + q];
  return r;
}

// (workgroups of 1024: at 256 threads the 2750 workgroups of 1100 images / 22 000 points took ~5 us to DISPATCH - a launch whose workgroups return at once was 6.2 us)
constexpr int kPointsQThreads = 1024;
// kDir: v = the direction z + beta p_old after the decision on iteration `it` (= the one before); otherwise v = the vector given (x of a residual-reset iteration `it`)
template <bool kDir, int kQuads>      // kQuads quads (records in flight) per point: 2, 4 or 8
__global__ __launch_bounds__(kPointsQThreads) void k_pcg_points_q(int P, const int32_t* __restrict__ pt_start, const int2* __restrict__ pt_entry, const double* __restrict__ rec,
                                                                  const double* __restrict__ v, const double* __restrict__ p_old, double* __restrict__ a,
                                                                  const PcgState* __restrict__ st, const double* __restrict__ part, int G, int it, double eta, int max_iterations) {
  const int gid = blockIdx.x * kPointsQThreads + threadIdx.x;
  const int q = gid & 3, quad = gid >> 2;
  const int p = quad / kQuads, slot = quad % kQuads;
  int e0 = 0, e1 = 0;
  if (p < P) { e0 = pt_start[p] + slot; e1 = pt_start[p + 1]; }
  const bool first = kDir && it == 0;
  // the pairs of the direction this lane multiplies with: lane 0: (2,3) and (4,5); lane 1: (4,5); lane 2: (0,1); lane 3: (0,1) and (2,3)
  const int ta = q == 0 ? 1 : (q == 1 ? 2 : 0), tb = q == 0 ? 2 : (q == 3 ? 1 : ta);
  QuadRecord r;
  double2 va, vb, pa = make_double2(0.0, 0.0), pb = make_double2(0.0, 0.0);
  auto fetch_at = [&](const int2 en) {
    r = LoadQuadRecord(rec, en.x, q);
    const double2* vv = reinterpret_cast<const double2*>(v + 6 * (size_t)en.y);
    va = vv[ta]; vb = vv[tb];
    if (kDir && !first) { const double2* pp = reinterpret_cast<const double2*>(p_old + 6 * (size_t)en.y); pa = pp[ta]; pb = pp[tb]; }
  };
  auto fetch = [&](int e) { fetch_at(pt_entry[e]); };
  {      // the first entry and "has the loop ended" travel together; the record fetch goes out before the decision, whose loads and wavefront sums run beside it
    const int2 en0 = pt_entry[e0 < e1 ? e0 : 0];
    if (PcgEnded(st, it, kDir)) return;
    fetch_at(en0);
  }
  const PcgDecision d = kDir ? PcgDecide(it, G, part, st, eta, max_iterations) : PcgCarry(it, part, st);
  if (!d.run) return;
  double acc0 = 0.0, acc1 = 0.0;      // lane 1: components 0, 1 (m0); lane 2: 2 (m0), 0 (m1); lane 3: 1, 2 (m1)
  for (int e = e0; e < e1; e += kQuads) {
    if (e != e0) fetch(e);
    if (kDir) {
      va.x = PcgDirection(first, d.beta, va.x, pa.x); va.y = PcgDirection(first, d.beta, va.y, pa.y);
      vb.x = PcgDirection(first, d.beta, vb.x, pb.x); vb.y = PcgDirection(first, d.beta, vb.y, pb.y);
    }
    const double2 fa = q == 3 ? r.r0 : r.r1, fb = q == 0 ? r.r2 : r.r1;      // the J_pose pieces that go with va / vb
    const double da = fa.x * va.x + fa.y * va.y, db = fb.x * vb.x + fb.y * vb.y;
    const double m0 = QuadSum(q == 2 ? 0.0 : da);                              // lanes 0, 1, 3 hold row 0's pieces in `fa`
    const double m1 = QuadSum((q == 2 ? da : 0.0) + ((q == 0 || q == 3) ? db : 0.0));
    // J_point^T m: lane 1 has (x00, x01), lane 2 (x02, x10), lane 3 (x11, x12)
    acc0 += r.r2.x * (q == 1 || q == 2 ? m0 : m1);
    acc1 += r.r2.y * (q == 1 ? m0 : m1);
  }
  // sort the private sums into components: c0 = lane1.acc0 + lane2.acc1, c1 = lane1.acc1 + lane3.acc0, c2 = lane2.acc0 + lane3.acc1
  double c[3];
  c[0] = (q == 1 ? acc0 : 0.0) + (q == 2 ? acc1 : 0.0);
  c[1] = (q == 1 ? acc1 : 0.0) + (q == 3 ? acc0 : 0.0);
  c[2] = (q == 2 ? acc0 : 0.0) + (q == 3 ? acc1 : 0.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {      // the 4 kQuads lanes of a point: fixed order - quad, half row, row, (two rows)
    c[k] = QuadSum(c[k]);
    if (kQuads >= 2) c[k] += DppMove<0x141>(c[k]);      // row_half_mirror
    if (kQuads >= 4) c[k] += DppMove<0x140>(c[k]);      // row_mirror: every lane holds the sum of its 16-lane row
    if (kQuads == 8) c[k] += __shfl_xor(c[k], 16);
  }
  if (p < P && slot == 0 && q == 0) { a[3 * (size_t)p] = c[0]; a[3 * (size_t)p + 1] = c[1]; a[3 * (size_t)p + 2] = c[2]; }
}

// (256 threads = 64 quads per image.  1024 threads - a few hundred observations in ONE round of dependent loads - was 25 us against 11: at 74 VGPRs one
// such workgroup fills a CU, and 1100 of them run in four rounds)
constexpr int kImagesQThreads = 256;
template <bool kDir>
__global__ __launch_bounds__(kImagesQThreads) void k_pcg_images_q(int C, const int32_t* __restrict__ pose_start, const int2* __restrict__ pose_entry, const double* __restrict__ rec,
                                                      const double* __restrict__ v, const double* __restrict__ p_old, double* __restrict__ p_new,
                                                      const double* __restrict__ a, const double* __restrict__ scale_c, const double* __restrict__ diag_c, double inv_radius,
                                                      double* __restrict__ out, double* __restrict__ dotp, const PcgState* __restrict__ st, PcgState* __restrict__ st_out,
                                                      const double* __restrict__ part, int G, int it, double eta, int max_iterations, int32_t* __restrict__ flag) {
  __shared__ double red[kImagesQThreads / 64][6];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = threadIdx.x & 3;
  const int e0 = pose_start[c] + (int)(threadIdx.x >> 2), e1 = pose_start[c + 1];
  double vc[6], po[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) { vc[j] = v[6 * (size_t)c + j]; po[j] = (kDir && it != 0) ? p_old[6 * (size_t)c + j] : 0.0; }
  double sc = 1.0, dg = 0.0;
  if (threadIdx.x < 6) { sc = scale_c[6 * (size_t)c + threadIdx.x]; dg = diag_c[6 * (size_t)c + threadIdx.x]; }
  QuadRecord r;
  double a0, a1, a2;
  auto fetch_at = [&](const int2 en) {
    r = LoadQuadRecord(rec, en.x, q);      // (lanes 1-3 do not use their third piece: J_point)
    a0 = a[3 * (size_t)en.y]; a1 = a[3 * (size_t)en.y + 1]; a2 = a[3 * (size_t)en.y + 2];
  };
  auto fetch = [&](int e) { fetch_at(pose_entry[e]); };
  {
    const int2 en0 = pose_entry[e0 < e1 ? e0 : pose_start[0]];
    if (PcgEnded(st, it, kDir)) {      // (both copies of the state keep saying so)
      if (c == 0 && threadIdx.x == 0) *st_out = *st;
      return;
    }
    fetch_at(en0);
  }
  const PcgDecision d = kDir ? PcgDecide(it, G, part, st, eta, max_iterations) : PcgCarry(it, part, st);
  if (c == 0 && threadIdx.x == 0) { *st_out = d.s; if (d.failed) atomicOr(flag, 1); }
  if (!d.run) return;
  const bool first = kDir && it == 0;
  if (kDir) {
#pragma unroll
    for (int j = 0; j < 6; ++j) vc[j] = PcgDirection(first, d.beta, vc[j], po[j]);
    if (threadIdx.x < 6) {
      double mine = vc[0];
#pragma unroll
      for (int j = 1; j < 6; ++j) mine = ((int)threadIdx.x == j) ? vc[j] : mine;
      p_new[6 * (size_t)c + threadIdx.x] = mine;
    }
  }
  // this lane's pairs of v_c: the one that goes with its first J_pose piece and the one that goes with its second
  //   lane 0: Jc0[2:4] (v 2,3), Jc1[4:6] (v 4,5)   lane 1: Jc0[4:6] (v 4,5), -   lane 2: Jc1[0:2] (v 0,1), -   lane 3: Jc0[0:2] (v 0,1), Jc1[2:4] (v 2,3)
  const double vax = q == 0 ? vc[2] : (q == 1 ? vc[4] : vc[0]), vay = q == 0 ? vc[3] : (q == 1 ? vc[5] : vc[1]);
  const double vbx = q == 0 ? vc[4] : vc[2], vby = q == 0 ? vc[5] : vc[3];
  double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
  for (int e = e0; e < e1; e += kImagesQThreads / 4) {
    if (e != e0) fetch(e);
    const double2 fa = q == 3 ? r.r0 : r.r1, fb = q == 0 ? r.r2 : r.r1;
    const double da = fa.x * vax + fa.y * vay, db = fb.x * vbx + fb.y * vby;
    // T a: lane 0 (T00, T01) -> m0; lane 1 (T02 -> m0, T10 -> m1); lane 2 (T11, T12) -> m1
    const double t0 = q == 0 ? r.r0.x * a0 + r.r0.y * a1 : (q == 1 ? r.r0.x * a2 : 0.0);
    const double t1 = q == 1 ? r.r0.y * a0 : (q == 2 ? r.r0.x * a1 + r.r0.y * a2 : 0.0);
    const double m0 = QuadSum((q == 2 ? 0.0 : da) - t0);
    const double m1 = QuadSum((q == 2 ? da : 0.0) + ((q == 0 || q == 3) ? db : 0.0) - t1);
    const double ma = q == 2 ? m1 : m0;      // the row `fa` belongs to
    u0 += fa.x * ma; u1 += fa.y * ma;
    u2 += fb.x * m1; u3 += fb.y * m1;        // (lanes 1, 2: not used below)
  }
  double acc[6];
  acc[0] = (q == 2 || q == 3) ? u0 : 0.0; acc[1] = (q == 2 || q == 3) ? u1 : 0.0;
  acc[2] = (q == 0 ? u0 : 0.0) + (q == 3 ? u2 : 0.0); acc[3] = (q == 0 ? u1 : 0.0) + (q == 3 ? u3 : 0.0);
  acc[4] = (q == 1 ? u0 : 0.0) + (q == 0 ? u2 : 0.0); acc[5] = (q == 1 ? u1 : 0.0) + (q == 0 ? u3 : 0.0);
#pragma unroll
  for (int j = 0; j < 6; ++j) acc[j] = WaveSumDpp(acc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) red[wv][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int j = threadIdx.x < 6 ? (int)threadIdx.x : 0;
    double mine = vc[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) mine = (j == k) ? vc[k] : mine;
    const double dd = (sc == 0.0) ? 1.0 : dg * inv_radius;
    double rs = 0.0;
#pragma unroll
    for (int w = 0; w < kImagesQThreads / 64; ++w) rs += red[w][j];      // wave order
    const double qv = rs + dd * mine;
    if (threadIdx.x < 6) out[6 * (size_t)c + j] = qv;
    const double term = mine * qv;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) dot += __shfl(term, k);
    if (threadIdx.x == 0) dotp[c] = dot;
  }
}

// the vector step of camera k's intrinsics block (variable intrinsics): the rows of the block one after the other
__device__ __forceinline__ void PcgStepIntrBlock(int mode, bool reset, double alpha, int C, int k, const PcgIntr& in, const double* __restrict__ b, double* __restrict__ x,
                                                 double* __restrict__ r, double* __restrict__ z, const double* __restrict__ p, const double* __restrict__ q, double& s0, double& s1) {
  const int off = k < in.K ? in.intr_off[k] : -1;
  if (off < 0) return;
  const int nv = in.intr_nv[k];
  const size_t i0 = 6 * (size_t)C + off;
  double rn[12], xn[12];
  for (int j = 0; j < nv; ++j) {
    const double bj = b[i0 + j];
    if (mode == 0) { xn[j] = 0.0; rn[j] = bj; x[i0 + j] = 0.0; s0 += bj * bj; }
    else if (mode == 1) { xn[j] = x[i0 + j] + alpha * p[i0 + j]; x[i0 + j] = xn[j]; rn[j] = reset ? 0.0 : r[i0 + j] - alpha * q[i0 + j]; }
    else { xn[j] = x[i0 + j]; rn[j] = bj - q[i0 + j]; }
    if (!reset && mode != 0) s0 -= xn[j] * (bj + rn[j]);
  }
  if (!reset) {
    for (int a = 0; a < nv; ++a) {
      const double* B = in.binvI + 12 * (size_t)(off + a);
      double zv = 0.0;
      for (int j = 0; j < nv; ++j) zv += B[j] * rn[j];
      z[i0 + a] = zv; r[i0 + a] = rn[a];
      s1 += rn[a] * zv;
    }
  }
}

// The vector step of both forms.  mode 0: start (x = 0, r = b, and the inverses of the diagonal blocks Sd -> binv); 1: after q = S p of iteration `it`;
// 2: after q = S x (explicit residual).  Every load is issued before the first workgroup sum.  kIntr: the intrinsics blocks as well - a thread per camera,
// in workgroups behind the pose workgroups - and the cameras' parts of p . S p behind the images'.
template <bool kIntr>
__global__ __launch_bounds__(kWideThreads) void k_pcg_step(int mode, int it, int C, const double* __restrict__ Sd, const double* __restrict__ b, double* __restrict__ x,
                                                           double* __restrict__ r, double* __restrict__ z, const double* __restrict__ p, const double* __restrict__ q,
                                                           double* __restrict__ binv, const double* __restrict__ dotp, const PcgState* __restrict__ st,
                                                           double* __restrict__ part, int32_t* __restrict__ flag, PcgIntr in) {
  __shared__ double red[4];
  __shared__ double red2[4][2];
  const int tid = threadIdx.x;
  const int g = blockIdx.x * kWideThreads + tid;      // parameter block: rows 3 g .. 3 g + 2
  const bool active = g < 2 * C;
  const size_t i = 3 * (size_t)(active ? g : 0);
  // ---- every load of the step (none depends on alpha) ----
  PcgState s;
  if (mode != 0) s = *st;
  double pq = 0.0;
  if (mode == 1) { for (int c = tid; c < C + (kIntr ? in.K : 0); c += kWideThreads) pq += dotp[c]; }
  double bv[3], xv[3] = {0, 0, 0}, rv[3] = {0, 0, 0}, pv[3] = {0, 0, 0}, qv[3] = {0, 0, 0}, B[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) bv[k] = b[i + k];
  if (mode != 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { xv[k] = x[i + k]; qv[k] = q[i + k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) B[k] = binv[9 * (size_t)(active ? g : 0) + k];
  }
  if (mode == 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { pv[k] = p[i + k]; rv[k] = r[i + k]; }
  }
  if (mode == 0) {      // the inverse of this parameter block's 3 x 3 diagonal block of S (rotation tangent / translation)
    const int c = (active ? g : 0) >> 1, hh = g & 1;
    const bool good = InverseSym3(Sd + 36 * (size_t)c + 21 * hh, B);
    if (active && !good) atomicOr(flag, 1);
    if (active) {
#pragma unroll
      for (int k = 0; k < 9; ++k) binv[9 * (size_t)g + k] = B[k];
    }
  }
  if (mode != 0 && (s.done || s.iter != it)) return;
  double alpha = 0.0;
  int status = kPcgRunning;
  if (mode == 1) {
    pq = WideBlockSum(pq, red);
    if (!(pq > 0.0) || isinf(pq)) status = isnan(pq) ? kPcgFailure : kPcgNoConvergence;      // indefinite direction: the iterate so far is the answer
    else { alpha = s.rho / pq; if (isinf(alpha)) status = kPcgFailure; }
  }
  const bool reset = mode == 1 && (it % kResidualResetPeriod) == 0;
  double s0 = 0.0, s1 = 0.0;
  if (kIntr && (int)blockIdx.x >= in.pose_blocks) {
    if (status == kPcgRunning) PcgStepIntrBlock(mode, reset, alpha, C, ((int)blockIdx.x - in.pose_blocks) * kWideThreads + tid, in, b, x, r, z, p, q, s0, s1);
  } else if (active && status == kPcgRunning) {
    if (mode == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { xv[k] = 0.0; rv[k] = bv[k]; x[i + k] = 0.0; s0 += bv[k] * bv[k]; }
    } else if (mode == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { xv[k] = xv[k] + alpha * pv[k]; x[i + k] = xv[k]; }
      if (!reset) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rv[k] = rv[k] - alpha * qv[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) rv[k] = bv[k] - qv[k];
    }
    if (!reset) {
      if (mode != 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s0 -= xv[k] * (bv[k] + rv[k]);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double zv = B[3 * k] * rv[0] + B[3 * k + 1] * rv[1] + B[3 * k + 2] * rv[2];
        z[i + k] = zv; r[i + k] = rv[k];
        s1 += rv[k] * zv;
      }
    }
  }
  s0 = WaveSum(s0); s1 = WaveSum(s1);      // (both sums behind ONE pair of barriers; the order of WideBlockSum)
  __syncthreads();
  if ((tid & 63) == 0) { red2[tid >> 6][0] = s0; red2[tid >> 6][1] = s1; }
  __syncthreads();
  if (tid == 0) {
    double* o = part + 4 * (size_t)blockIdx.x;
    o[0] = ((red2[0][0] + red2[1][0]) + red2[2][0]) + red2[3][0]; o[1] = ((red2[0][1] + red2[1][1]) + red2[2][1]) + red2[3][1]; o[2] = (double)status; o[3] = alpha;
  }
}

int PcgEnsureBuffers(pp_ba_impl* h) {
  if (h->pcg_state) return PP_OK;
  const size_t n = (size_t)h->n_red;      // 6 C pose columns, then the NI variable intrinsics
  DeviceBlocks& B = h->blocks;
  PP_TRY(B.Alloc(&h->pcg_Sd, 36 * (size_t)h->C)); PP_TRY(B.Alloc(&h->pcg_binv, 18 * (size_t)h->C)); PP_TRY(B.Alloc(&h->pcg_b, n)); PP_TRY(B.Alloc(&h->pcg_r, n)); PP_TRY(B.Alloc(&h->pcg_z, n));
  PP_TRY(B.Alloc(&h->pcg_p, 2 * n)); PP_TRY(B.Alloc(&h->pcg_q, n));      // (pcg_p: two copies, the fused direction update ping-pongs)
  PP_TRY(B.Alloc(&h->pcg_a, 3 * (size_t)h->P)); PP_TRY(B.Alloc(&h->pcg_dot, (size_t)h->C + (h->NI > 0 ? h->K : 0)));
  PP_TRY(B.Alloc(&h->pcg_part, 4 * (size_t)(CeilDiv(2 * (int64_t)h->C, kWideThreads) + (h->NI > 0 ? CeilDiv(h->K, kWideThreads) : 0))));
  if (h->NI > 0) { PP_TRY(B.Alloc(&h->pcg_tk, 2 * (size_t)h->M)); PP_TRY(B.Alloc(&h->pcg_w, 2 * (size_t)h->M)); PP_TRY(B.Alloc(&h->pcg_Scomp, 12 * (size_t)h->NI)); PP_TRY(B.Alloc(&h->pcg_binvI, 12 * (size_t)h->NI)); }
  PP_TRY(B.Alloc(&h->pcg_state, 2));      // (two copies: the many-workgroup vector step ping-pongs)
  PP_TRY(B.AllocPinned(reinterpret_cast<void**>(&h->pcg_state_host), sizeof(PcgState)));
  // the list entries with what they point at beside them (one dependent load less per product kernel)
  PP_TRY(B.Alloc(reinterpret_cast<int2**>(&h->pcg_pt_entry), std::max<size_t>(1, (size_t)h->M)));
  PP_TRY(B.Alloc(reinterpret_cast<int2**>(&h->pcg_pose_entry), std::max<size_t>(1, (size_t)h->M)));
  if (h->M > 0) {
    hipLaunchKernelGGL(k_pcg_entries, dim3(CeilDiv(h->M, (int64_t)256)), dim3(256), 0, h->stream, h->M, h->pt_obs, h->obs_pose, h->pose_obs, h->obs_point,
                       reinterpret_cast<int2*>(h->pcg_pt_entry), reinterpret_cast<int2*>(h->pcg_pose_entry));
    PP_HIP_TRY(hipGetLastError());
  }
  return PP_OK;
}

// the host's wait for k_pcg_decide (host_ticket.hpp; PPSFM_TICKET_SPIN_US, default 1500 us; 0 = never spin: the stream is synchronised instead)
static int WaitPcgTicket(pp_ba_impl* h, int32_t ticket) {
  const long spin_us = h->sw.ticket_spin_us;
  hipError_t e = hipSuccess;
  switch (WaitHostTicket(&h->pcg_state_host->pad_, ticket, spin_us, [&] { return (e = hipStreamSynchronize(h->stream)) == hipSuccess; }, spin_us == 0)) {
    case TicketWait::kArrived: return PP_OK;
    case TicketWait::kSyncFailed: SetLastError("pp_ba_solve: hipStreamSynchronize failed while waiting for the conjugate-gradient state: %s", hipGetErrorString(e)); break;
    case TicketWait::kNeverArrived: SetLastError("pp_ba_solve: the conjugate-gradient state never arrived"); break;
  }
  return PP_ERR_HIP;
}

// When the host looks at the loop's state.  Iterations enqueued before the first look: what the previous solve of this handle needed, + 1 (consecutive
// LM iterations take about the same number of CG iterations - ~6 at 1100 images with eta = 0.1 - and every iteration enqueued beyond the end is launches
// of kernels that return at once plus the wait for them: a fixed first batch of 8 was ~10 % of such an LM iteration).  Longer than last time: look
// again soon, then less and less often.  every_iteration (a point-sharded group): every iteration enqueued beyond the end is a real collective of 6 C
// doubles on every rank - look after each one.
struct PcgLooks {
  int batch, next;
  bool every_iteration;
  PcgLooks(int last_iterations, bool every) : batch(last_iterations > 0 ? std::min(32, last_iterations + 1) : 8), next(batch), every_iteration(every) {}
  bool Now(int it, int cap) const { return it == next || it == cap; }
  void After(int it) {
    batch = every_iteration ? 1 : (it == next && next > batch ? std::min(32, batch * 2) : 2);
    next = it + batch;
  }
};

static int PcgFinishCount(pp_ba_impl* h, int* iterations) {
  const PcgState* hs = h->pcg_state_host;
  if (iterations) *iterations = hs->iter;
  if (h->sw.pcg_log) fprintf(stderr, "pcg: %d iterations (previous solve %d)\n", hs->iter, h->pcg_last_iterations);
  h->pcg_last_iterations = hs->iter;
  return PP_OK;
}

// the vector step of both forms (p: the direction of this iteration; st: the current copy of the state)
static void LaunchStep(pp_ba_impl* h, int G, const PcgIntr& in, int mode, int it, const double* p, const PcgState* st) {
  auto* k = in.K > 0 ? k_pcg_step<true> : k_pcg_step<false>;
  hipLaunchKernelGGL(k, dim3(G), dim3(kWideThreads), 0, h->stream, mode, it, h->C, h->pcg_Sd, h->pcg_b, h->step_c, h->pcg_r, h->pcg_z, p, h->pcg_q, h->pcg_binv, h->pcg_dot, st,
                     h->pcg_part, h->d_flag, in);
}

// what a product of the three-launch form needs beside the vector: the loop's constants and the current copies of the state (cur) and of the direction (pc)
struct PcgFusedLoop {
  pp_ba_impl* h;
  double inv_radius, eta;
  int max_iterations, G;
  // quads per point (a record each per round): 2 up to a mean track of 2.5, 4 up to 4.5, 8 beyond (two records in flight per quad with half the
  // quads: 11.3 us against 9.1 - the early exit waits for both)
  int qp;
  int cur = 0, pc = 0;
};
template <bool kDir, int kQuads>
static void LaunchPointsQ(const PcgFusedLoop& L, const double* v, const double* p_old, int it) {
  pp_ba_impl* h = L.h;
  hipLaunchKernelGGL((k_pcg_points_q<kDir, kQuads>), dim3(CeilDiv(4 * kQuads * (int64_t)h->P, kPointsQThreads)), dim3(kPointsQThreads), 0, h->stream, h->P, h->pt_start,
                     reinterpret_cast<const int2*>(h->pcg_pt_entry), h->JpS, v, p_old, h->pcg_a, h->pcg_state + L.cur, h->pcg_part, L.G, it, L.eta, L.max_iterations);
}
// kDir: pcg_q = S (z + beta p) after the decision on iteration `it`, v = z; else pcg_q = S v
template <bool kDir>
static void LaunchProductQ(PcgFusedLoop& L, const double* v, int it) {
  pp_ba_impl* h = L.h;
  const size_t n = 6 * (size_t)h->C;
  const double* p_old = h->pcg_p + (size_t)L.pc * n;
  double* p_new = h->pcg_p + (size_t)(L.pc ^ 1) * n;
  if (L.qp == 8) LaunchPointsQ<kDir, 8>(L, v, p_old, it); else if (L.qp == 4) LaunchPointsQ<kDir, 4>(L, v, p_old, it); else LaunchPointsQ<kDir, 2>(L, v, p_old, it);
  hipLaunchKernelGGL((k_pcg_images_q<kDir>), dim3(h->C), dim3(kImagesQThreads), 0, h->stream, h->C, h->pose_start, reinterpret_cast<const int2*>(h->pcg_pose_entry), h->JpS, v, p_old,
                     p_new, h->pcg_a, h->scale_c, h->diag_c, L.inv_radius, h->pcg_q, h->pcg_dot, h->pcg_state + L.cur, h->pcg_state + (L.cur ^ 1), h->pcg_part, L.G, it, L.eta,
                     L.max_iterations, h->d_flag);
  if (kDir) L.pc ^= 1;
  L.cur ^= 1;
}

// The three-launch loop (the default outside point-sharded groups): the product kernels take the decision and form the direction themselves.
static int PcgFusedRun(pp_ba_impl* h, double inv_radius, int max_iterations, double eta, int* iterations) {
  const size_t n = 6 * (size_t)h->C;
  const int G = CeilDiv(2 * (int64_t)h->C, kWideThreads);
  const int cap = std::max(1, max_iterations);
  PcgState* hs = h->pcg_state_host;
  PcgLooks looks(h->pcg_last_iterations, false);
  PcgFusedLoop L{h, inv_radius, eta, max_iterations, G, h->M > (int64_t)h->P * 9 / 2 ? 8 : (h->M > (int64_t)h->P * 5 / 2 ? 4 : 2)};
  const PcgIntr none;
  auto step = [&](int mode, int it) { LaunchStep(h, G, none, mode, it, h->pcg_p + (size_t)L.pc * n, h->pcg_state + L.cur); };
  step(0, 0);
  for (int it = 1; it <= cap; ++it) {
    LaunchProductQ<true>(L, h->pcg_z, it - 1);
    step(1, it);
    if (it % kResidualResetPeriod == 0) { LaunchProductQ<false>(L, h->step_c, it); step(2, it); }
    if (looks.Now(it, cap)) {
      // (the state goes straight into the pinned block the host reads: no copy in between)
      const int32_t ticket = ++h->pcg_ticket == 0 ? ++h->pcg_ticket : h->pcg_ticket;
      hs->pad_ = 0;
      hipLaunchKernelGGL(k_pcg_decide, dim3(1), dim3(64), 0, h->stream, it, G, h->pcg_part, h->pcg_state + L.cur, hs, eta, max_iterations, h->d_flag, ticket);
      PP_HIP_TRY(hipGetLastError());
      PP_TRY(WaitPcgTicket(h, ticket));
      if (hs->done) break;
      looks.After(it);
    }
  }
  return PcgFinishCount(h, iterations);
}

// S x = b for the system k_schur_self_rhs (compact) + k_prepare have set up for `radius`; x -> h->step_c (scaled space).
// Synchronises the stream (the loop's length is data dependent).  *iterations: conjugate-gradient iterations run.
int PcgSolve(pp_ba_impl* h, double radius, int max_iterations, double eta, int* iterations) {
  hipStream_t s = h->stream;
  const int n = h->n_red, C = h->C;
  const double inv_radius = 1.0 / radius;
  const bool group = BaInGroup(h);
  const bool intr = h->NI > 0;      // variable intrinsics: the four-launch form with the per-camera kernels (see PcgIntr)
  const int Gp = CeilDiv(2 * (int64_t)C, kWideThreads);
  const int G = Gp + (intr ? CeilDiv(h->K, kWideThreads) : 0);
  PcgIntr in;
  if (intr) { in.K = h->K; in.pose_blocks = Gp; in.intr_off = h->intr_off; in.intr_nv = h->intr_nv; in.binvI = h->pcg_binvI; }
  const int cap = std::max(1, max_iterations);
  PcgState* hs = h->pcg_state_host;
  hs->done = 0; hs->iter = 0; hs->status = kPcgRunning;
  if (!group && !intr && h->sw.pcg_fused) return PcgFusedRun(h, inv_radius, max_iterations, eta, iterations);
  PcgLooks looks(h->pcg_last_iterations, group);
  if (intr) hipLaunchKernelGGL(k_pcg_intr_inverse, dim3(CeilDiv(h->K, 64)), dim3(64), 0, s, h->K, h->intr_off, h->intr_nv, h->pcg_Scomp, h->pcg_binvI, h->d_flag);
  // the vector step: many workgroups (k_pcg_step / k_pcg_wide_b, two launches) - 1100 images: 2460 -> 2860 LM it/s against the one-workgroup
  // kernel (12.5 us per step; 29.6 us at 4000 images, where it was the longest kernel of an iteration, against 6.1 + 4.4 us); 600 images
  // +6 %.  In a point-sharded group p . S p belongs to the all-reduced product: k_pcg_dot forms its per-image parts after the exchange.
  int cur = 0;      // which copy of the state is current (ping-pong)
  auto wide_a = [&](int mode, int it) { LaunchStep(h, G, in, mode, it, h->pcg_p, h->pcg_state + cur); };
  auto wide_b = [&](int mode, int it) {
    hipLaunchKernelGGL(k_pcg_wide_b, dim3(G), dim3(kWideThreads), 0, s, mode, it, C, G, h->pcg_z, h->pcg_p, h->pcg_part, h->pcg_state + cur, h->pcg_state + (cur ^ 1), eta,
                       max_iterations, h->d_flag, in);
    cur ^= 1;
  };
  wide_a(0, 0); wide_b(0, 0);
  // A point-sharded group (pp_ba_set_communicator / pp_ba_set_allreduce): every rank applies S to the same vector with ITS points'
  // observations (a point's observations all live on its owner, so the partial products simply add up), the products are summed over the
  // group - 6 C doubles per product, 24 KB at 500 images, against the 36 MB lower triangle the direct solver exchanges per LM iteration -
  // and every rank runs the same vector updates on the same data: identical decisions, identical iterates, no further exchange.
  double* dotp = group ? nullptr : h->pcg_dot;
  int rc_group = PP_OK;
  auto apply = [&](const double* v) {      // pcg_q = S v (and pcg_dot = the per-image parts of v . S v)
    const double2* tk = intr ? reinterpret_cast<const double2*>(h->pcg_tk) : nullptr;
    double2* w = intr ? reinterpret_cast<double2*>(h->pcg_w) : nullptr;
    if (intr) hipLaunchKernelGGL(k_pcg_cam_t, dim3(CeilDiv(h->M, (int64_t)256)), dim3(256), 0, s, h->M, C, h->obs_cam, h->intr_off, h->intr_nv, h->JkS_intr, v,
                                 reinterpret_cast<double2*>(h->pcg_tk), h->pcg_state + cur);
    hipLaunchKernelGGL(k_pcg_points, dim3(CeilDiv(4 * (int64_t)h->P, 256)), dim3(256), 0, s, h->P, h->pt_start, h->pt_obs, h->obs_pose, h->JpS, v, h->pcg_a, h->pcg_state + cur, tk);
    hipLaunchKernelGGL(k_pcg_images, dim3(C), dim3(256), 0, s, C, h->pose_start, h->pose_obs, h->obs_point, h->JpS, v, h->pcg_a, h->scale_c, h->diag_c, inv_radius,
                       h->pcg_q, dotp, h->pcg_state + cur, h->group_rank == 0 ? 1 : 0, tk, w);
    if (intr) {      // the intrinsics rows of the product and the cameras' parts of v . S v
      if (h->isum_num_chunks > 0)
        hipLaunchKernelGGL(k_pcg_cam_q, dim3((unsigned)h->isum_num_chunks), dim3(256), 0, s, h->isum_chunk, h->cam_obs, h->JkS_intr, (const double2*)w, h->isum_partial,
                           h->pcg_state + cur);
      hipLaunchKernelGGL(k_pcg_cam_q_reduce, dim3(h->K), dim3(64), 0, s, C, h->isum_cam_chunk, h->intr_off, h->intr_nv, h->isum_partial, v, h->diag_c, inv_radius, h->pcg_q,
                         h->pcg_dot, h->pcg_state + cur, h->group_rank == 0 ? 1 : 0);
    }
    if (group && rc_group == PP_OK) rc_group = BaGroupReduce(h, h->pcg_q, n, PP_REDUCE_SUM);
    // (the all-reduced product carries the intrinsics rows as well: n = 6 C + NI doubles; the cameras' parts of v . S v follow the images')
    if (group) hipLaunchKernelGGL(k_pcg_dot, dim3(CeilDiv(C + (intr ? h->K : 0), 256)), dim3(256), 0, s, C, v, h->pcg_q, h->pcg_dot, h->pcg_state + cur, intr ? h->K : 0,
                                          (const int32_t*)h->intr_off, (const int32_t*)h->intr_nv);
  };
  for (int it = 1; it <= cap; ++it) {
    apply(h->pcg_p);
    if (rc_group) { (void)hipStreamSynchronize(s); return rc_group; }      // (what is already enqueued reads the buffers the caller may free next)
    const bool reset = it % kResidualResetPeriod == 0;
    wide_a(1, it); wide_b(reset ? 3 : 1, it);
    if (reset) {
      apply(h->step_c);
      if (rc_group) { (void)hipStreamSynchronize(s); return rc_group; }
      wide_a(2, it); wide_b(1, it);
    }
    if (looks.Now(it, cap)) {
      PP_HIP_TRY(hipGetLastError());
      PP_HIP_TRY(hipMemcpyAsync(hs, h->pcg_state + cur, sizeof(PcgState), hipMemcpyDeviceToHost, s));
      PP_HIP_TRY(hipStreamSynchronize(s));
      if (hs->done) break;
      looks.After(it);
    }
  }
  return PcgFinishCount(h, iterations);      // (the look at it == cap has seen the end: the cap ends the loop)
}

}  // namespace ppsfm
