// K1 — batched residual + Jacobian evaluation of the line-to-point reprojection cost, and its entry points
// (the pp_ba_handle lifecycle: ba_create.hip).
//
// Replaces, for all M residual blocks at once, what Ceres does by calling
// AutoDiffCostFunction<BundleAdjustment[ConstantPose]LineCostFunction<CameraModel>,...>::Evaluate
// once per block from its thread pool (reference src/base/cost_functions.h:55-60, :130-137, call
// sites src/optim/bundle_adjustment.cc:381-415, :470-486).
//
// Roofline: HBM.  Algorithmic bytes per observation: 60 B in (line 24, two int32
// indices 8 (+4 amortised), point gather 24, pose/intrinsics amortised over the image's
// observations) + 160 B out (r 16, J_pose 2x6 96, J_point 2x3 48) = 220 B.
// Mapping: one lane per observation, 256-lane workgroups (4 wavefronts), >= 3 workgroups per CU at
// the 200k-observation size.  Line coefficients are SoA streams (coalesced 512 B / wavefront /
// stream).  Poses (56 B) and points (24 B) are gathered; with observations grouped by image the pose
// gather is wave-uniform and served by L1/L2.
#include "ba_impl.hpp"
#include "resource_pool.hpp"
#include "line_residual.hpp"

namespace ppsfm {

struct EvalArgs {
  int64_t M;
  const double *la, *lb, *lc;
  const int32_t *obs_pose, *obs_point, *obs_cam;   // obs_cam = (intrinsics index << 4) | camera model id
  const double *poses, *points, *intr;
  double *r, *Jpose, *Jpoint, *Jcam;
  // Jcam rows: ambient (2 x kCamStride per observation: the C ABI's layout) when cam_col is null; otherwise COMPACT - only the variable parameters, column
  // cam_col[camera][parameter] (< cam_stride) of rows cam_stride wide: what the solver's own evaluations write (32 bytes per observation for two
  // variable parameters instead of 192, and contiguous across the lanes of a wavefront)
  const int32_t* cam_col;
  int cam_stride;
  double* partials;
  int loss_type;
  double loss_scale;
};

// MODE 0: residual/cost only; 1: tangent pose Jacobian (2x6); 2: ambient pose Jacobian (2x7)
// The Jacobian rows (96/112 + 48 bytes per observation) are staged through LDS so that the workgroup
// writes its contiguous 36 KB slab with fully coalesced 16-byte stores instead of 9 strided stores per lane.
template <int MODE, bool WANT_CAM, bool LOSS_CORRECT>
__global__ __launch_bounds__(256) void k_line_eval(EvalArgs a) {
  constexpr int JW = MODE == 2 ? 14 : 12;
  __shared__ __attribute__((aligned(16))) double sJp[MODE == 0 ? 2 : 256 * JW];
  __shared__ __attribute__((aligned(16))) double sJx[MODE == 0 ? 2 : 256 * 6];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * 256;
  const int64_t o = o0 + tid;
  double half_rho = 0.0;
  if (o < a.M) {
    // independent loads first: indices, line, then the gathers they feed
    const int c = a.obs_pose[o], p = a.obs_point[o], ck = a.obs_cam[o];
    const double la = a.la[o], lb = a.lb[o], lc = a.lc[o];
    const int model = ck & 15;
    const double* cam = a.intr + (size_t)kCamStride * (ck >> 4);
    const double* pose = a.poses + (size_t)7 * c;
    const double q[4] = {pose[0], pose[1], pose[2], pose[3]};
    const double t[3] = {pose[4], pose[5], pose[6]};
    const double X[3] = {a.points[3 * (size_t)p], a.points[3 * (size_t)p + 1], a.points[3 * (size_t)p + 2]};
    if (MODE == 0) {
      double r[2];
      LineResidualOnly(model, cam, q, t, X, la, lb, lc, r);
      double rho0, rho1;
      LossRho(a.loss_type, a.loss_scale, r[0] * r[0] + r[1] * r[1], &rho0, &rho1);
      half_rho = 0.5 * rho0;
      if (a.r) { a.r[2 * o] = r[0]; a.r[2 * o + 1] = r[1]; }
    } else {
      LineObsJac J;
      LineResidualJacobian<MODE == 2>(model, cam, q, t, X, la, lb, lc, &J);
      double rho0, rho1;
      LossRho(a.loss_type, a.loss_scale, J.r[0] * J.r[0] + J.r[1] * J.r[1], &rho0, &rho1);
      half_rho = 0.5 * rho0;
      const double sr = LOSS_CORRECT ? sqrt(rho1) : 1.0;  // Ceres Corrector with alpha = 0 (rho'' <= 0)
      double2* r2 = reinterpret_cast<double2*>(a.r);
      r2[o] = make_double2(sr * J.r[0], sr * J.r[1]);
      double2* jp = reinterpret_cast<double2*>(sJp + JW * tid);
      if (MODE == 1) {
        jp[0] = make_double2(sr * J.Jrot[0], sr * J.Jrot[1]);
        jp[1] = make_double2(sr * J.Jrot[2], sr * J.Jt[0]);
        jp[2] = make_double2(sr * J.Jt[1], sr * J.Jt[2]);
        jp[3] = make_double2(sr * J.Jrot[3], sr * J.Jrot[4]);
        jp[4] = make_double2(sr * J.Jrot[5], sr * J.Jt[3]);
        jp[5] = make_double2(sr * J.Jt[4], sr * J.Jt[5]);
      } else {
        jp[0] = make_double2(sr * J.Jq[0], sr * J.Jq[1]);
        jp[1] = make_double2(sr * J.Jq[2], sr * J.Jq[3]);
        jp[2] = make_double2(sr * J.Jt[0], sr * J.Jt[1]);
        jp[3] = make_double2(sr * J.Jt[2], sr * J.Jq[4]);
        jp[4] = make_double2(sr * J.Jq[5], sr * J.Jq[6]);
        jp[5] = make_double2(sr * J.Jq[7], sr * J.Jt[3]);
        jp[6] = make_double2(sr * J.Jt[4], sr * J.Jt[5]);
      }
      double2* jx = reinterpret_cast<double2*>(sJx + 6 * tid);
      jx[0] = make_double2(sr * J.JX[0], sr * J.JX[1]);
      jx[1] = make_double2(sr * J.JX[2], sr * J.JX[3]);
      jx[2] = make_double2(sr * J.JX[4], sr * J.JX[5]);
      if (WANT_CAM) {
        double jl[2 * kCamStride];
#pragma unroll
        for (int i = 0; i < 2 * kCamStride; ++i) jl[i] = 0.0;
        LineResidualCameraJacobian(model, cam, q, t, X, la, lb, lc, jl, kCamStride);
        if (LOSS_CORRECT) {
#pragma unroll
          for (int i = 0; i < 2 * kCamStride; ++i) jl[i] *= sr;
        }
        if (a.cam_col) {
          const int W = a.cam_stride;
          double* jc = a.Jcam + (size_t)2 * W * o;
          double2* z = reinterpret_cast<double2*>(jc);
          for (int i = 0; i < W; ++i) z[i] = make_double2(0.0, 0.0);      // (a camera with fewer variable parameters than the widest one)
          const int32_t* col = a.cam_col + (size_t)kCamStride * (ck >> 4);
#pragma unroll
          for (int i = 0; i < kCamStride; ++i) { const int cc = col[i]; if (cc >= 0) { jc[cc] = jl[i]; jc[W + cc] = jl[kCamStride + i]; } }
        } else {
          double2* jc = reinterpret_cast<double2*>(a.Jcam + (size_t)2 * kCamStride * o);
#pragma unroll
          for (int i = 0; i < kCamStride; ++i) jc[i] = make_double2(jl[2 * i], jl[2 * i + 1]);
        }
      }
    }
  }
  if (MODE != 0) {
    __syncthreads();
    const int64_t left = a.M - o0;
    const int nobs = left < 256 ? (int)left : 256;
    {  // J_pose slab: nobs * JW doubles, contiguous in global memory
      const int n2 = nobs * JW / 2;   // double2 chunks
      double2* dst = reinterpret_cast<double2*>(a.Jpose + (size_t)JW * o0);
      const double2* src = reinterpret_cast<const double2*>(sJp);
#pragma unroll
      for (int it = 0; it < (256 * JW / 2 + 255) / 256; ++it) {
        const int idx = it * 256 + tid;
        if (idx < n2) { const double2 v = src[idx]; __builtin_nontemporal_store(v.x, &dst[idx].x); __builtin_nontemporal_store(v.y, &dst[idx].y); }
      }
    }
    {
      const int n2 = nobs * 3;
      double2* dst = reinterpret_cast<double2*>(a.Jpoint + (size_t)6 * o0);
      const double2* src = reinterpret_cast<const double2*>(sJx);
#pragma unroll
      for (int it = 0; it < 3; ++it) {
        const int idx = it * 256 + tid;
        if (idx < n2) { const double2 v = src[idx]; __builtin_nontemporal_store(v.x, &dst[idx].x); __builtin_nontemporal_store(v.y, &dst[idx].y); }
      }
    }
  }
  BlockPartialSum(half_rho, a.partials);
}

// fixed-order final reduction of the per-block partial sums (deterministic cost)
__global__ __launch_bounds__(256) void k_sum_partials(const double* partials, int n, double* out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sh[0];
}

static EvalArgs MakeArgs(pp_ba_impl* h, const double* poses, const double* points, const double* intr = nullptr) {
  EvalArgs a;
  a.M = h->M; a.la = h->la; a.lb = h->lb; a.lc = h->lc;
  a.obs_pose = h->obs_pose; a.obs_point = h->obs_point; a.obs_cam = h->obs_cam;
  a.poses = poses; a.points = points; a.intr = intr ? intr : h->intr;
  a.r = h->r; a.Jpose = h->Jpose; a.Jpoint = h->Jpoint; a.Jcam = h->Jcam; a.cam_col = nullptr; a.cam_stride = kCamStride;
  a.partials = h->partials; a.loss_type = h->loss_type; a.loss_scale = h->loss_scale;
  return a;
}

int BaEnsureJacobianBuffers(pp_ba_impl* h, int jac_mode, int want_cam) {
  const int width = jac_mode == 1 ? 14 : 12;
  if (!h->Jpose || h->jpose_width < width) {
    h->blocks.Free(&h->Jpose);
    PP_TRY(h->blocks.Alloc(&h->Jpose, (size_t)h->M * width));
    h->jpose_width = width;
  }
  if (want_cam && !h->Jcam) PP_TRY(h->blocks.Alloc(&h->Jcam, (size_t)h->M * 2 * kCamStride));
  return PP_OK;
}

int LaunchEval(pp_ba_impl* h, int jac_mode, int want_cam, bool loss_correct, const double* poses, const double* points,
               double* cost_slot, bool compact_cam) {
  EvalArgs a = MakeArgs(h, poses, points);
  if (want_cam) {      // (the readers of Jcam - IntrSumsAfterEval, IntrScaledJacobians - are told which layout the last evaluation left)
    h->jcam_compact = compact_cam && h->NI > 0;
    if (h->jcam_compact) { a.cam_col = h->intr_col; a.cam_stride = h->jcam_stride; }
  }
  const int grid = h->num_partials;
  hipStream_t s = h->stream;
  if (jac_mode == 0) {
    if (want_cam) { if (loss_correct) hipLaunchKernelGGL((k_line_eval<1, true, true>), dim3(grid), dim3(256), 0, s, a); else hipLaunchKernelGGL((k_line_eval<1, true, false>), dim3(grid), dim3(256), 0, s, a); }
    else { if (loss_correct) hipLaunchKernelGGL((k_line_eval<1, false, true>), dim3(grid), dim3(256), 0, s, a); else hipLaunchKernelGGL((k_line_eval<1, false, false>), dim3(grid), dim3(256), 0, s, a); }
  } else {
    if (want_cam) hipLaunchKernelGGL((k_line_eval<2, true, false>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_line_eval<2, false, false>), dim3(grid), dim3(256), 0, s, a);
  }
  if (cost_slot) hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, h->partials, grid, cost_slot);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

int LaunchCostOnly(pp_ba_impl* h, const double* poses, const double* points, const double* intr, double* cost_slot) {
  EvalArgs a = MakeArgs(h, poses, points, intr);
  a.r = nullptr;
  const int grid = h->num_partials;
  hipLaunchKernelGGL((k_line_eval<0, false, false>), dim3(grid), dim3(256), 0, h->stream, a);
  if (cost_slot) hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, h->stream, h->partials, grid, cost_slot);   // else: summed by the caller's next kernel
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

// residuals (not loss-corrected) + cost, no Jacobians: what Ceres asks for at a trial point
static int LaunchResidualsOnly(pp_ba_impl* h, const double* poses, const double* points, double* cost_slot) {
  EvalArgs a = MakeArgs(h, poses, points);
  const int grid = h->num_partials;
  hipLaunchKernelGGL((k_line_eval<0, false, false>), dim3(grid), dim3(256), 0, h->stream, a);
  if (cost_slot) hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, h->stream, h->partials, grid, cost_slot);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

int pp_ba_eval(pp_ba_handle h, int jac_mode, int want_cam, double* residuals_out, double* jpose_out, double* jpoint_out,
               double* jcam_out, double* cost_out) try {
  PP_REQUIRE(h, "pp_ba_eval: null handle");
  PP_REQUIRE(jac_mode == 0 || jac_mode == 1, "pp_ba_eval: jac_mode must be 0 (tangent) or 1 (ambient)");
  PP_HIP_TRY(hipSetDevice(h->device));
  int rc = BaEnsureJacobianBuffers(h, jac_mode, want_cam || jcam_out != nullptr);
  if (rc) return rc;
  const int cam = (want_cam || jcam_out) ? 1 : 0;
  rc = LaunchEval(h, jac_mode, cam, false, h->poses, h->points, h->scal + kCost);
  if (rc) return rc;
  const int width = jac_mode == 1 ? 14 : 12;
  if (residuals_out) { rc = Download(residuals_out, h->r, (size_t)2 * h->M, h->stream); if (rc) return rc; }
  if (jpose_out) { rc = Download(jpose_out, h->Jpose, (size_t)width * h->M, h->stream); if (rc) return rc; }
  if (jpoint_out) { rc = Download(jpoint_out, h->Jpoint, (size_t)6 * h->M, h->stream); if (rc) return rc; }
  if (jcam_out) { rc = Download(jcam_out, h->Jcam, (size_t)2 * kCamStride * h->M, h->stream); if (rc) return rc; }
  if (cost_out) { rc = Download(cost_out, h->scal + kCost, 1, h->stream); if (rc) return rc; }
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
} PP_API_CATCH("pp_ba_eval")

int pp_ba_eval_host_view(pp_ba_handle h, int jac_mode, int want_cam, int want_jacobians, const double** residuals, const double** jpose,
                         const double** jpoint, const double** jcam, double* cost_out) try {
  PP_REQUIRE(h && residuals, "pp_ba_eval_host_view: null argument");
  PP_REQUIRE(jac_mode == 0 || jac_mode == 1, "pp_ba_eval_host_view: jac_mode must be 0 (tangent) or 1 (ambient)");
  PP_HIP_TRY(hipSetDevice(h->device));
  const int cam = want_cam ? 1 : 0, width = jac_mode == 1 ? 14 : 12;
  int rc = BaEnsureJacobianBuffers(h, jac_mode, cam);
  if (rc) return rc;
  const size_t M = (size_t)h->M;
  auto pin = [&](double** p, size_t doubles) { return *p ? PP_OK : h->mirrors.AllocPinned(reinterpret_cast<void**>(p), sizeof(double) * doubles); };
  PP_TRY(pin(&h->pin_r, 2 * M));
  if (want_jacobians) {
    if (h->pin_jpose && h->pin_width < width) h->mirrors.Free(&h->pin_jpose);
    if (!h->pin_jpose) { PP_TRY(pin(&h->pin_jpose, width * M)); h->pin_width = width; }
    PP_TRY(pin(&h->pin_jpoint, 6 * M));
    if (cam) PP_TRY(pin(&h->pin_jcam, 2 * kCamStride * M));
  }
  // a cost-only evaluation (Ceres asks for residuals without Jacobians at every trial point) runs K1's cost-only variant and
  // moves 16 B per observation instead of 220 B+
  if (want_jacobians) rc = LaunchEval(h, jac_mode, cam, false, h->poses, h->points, h->scal + kCost);
  else rc = LaunchResidualsOnly(h, h->poses, h->points, h->scal + kCost);
  if (rc) return rc;
  rc = Download(h->pin_r, h->r, 2 * M, h->stream); if (rc) return rc;
  if (want_jacobians) {
    rc = Download(h->pin_jpose, h->Jpose, (size_t)width * M, h->stream); if (rc) return rc;
    rc = Download(h->pin_jpoint, h->Jpoint, 6 * M, h->stream); if (rc) return rc;
    if (cam) { rc = Download(h->pin_jcam, h->Jcam, (size_t)2 * kCamStride * M, h->stream); if (rc) return rc; }
  }
  if (cost_out) { rc = Download(cost_out, h->scal + kCost, 1, h->stream); if (rc) return rc; }
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  *residuals = h->pin_r;
  if (jpose) *jpose = want_jacobians ? h->pin_jpose : nullptr;
  if (jpoint) *jpoint = want_jacobians ? h->pin_jpoint : nullptr;
  if (jcam) *jcam = (want_jacobians && cam) ? h->pin_jcam : nullptr;
  return PP_OK;
} PP_API_CATCH("pp_ba_eval_host_view")

int pp_ba_eval_device(pp_ba_handle h, int jac_mode, int want_cam, int repeat, float* ms_per_launch) try {
  PP_REQUIRE(h && repeat > 0, "pp_ba_eval_device: bad argument");
  PP_REQUIRE(jac_mode == 0 || jac_mode == 1, "pp_ba_eval_device: jac_mode must be 0 or 1");
  PP_HIP_TRY(hipSetDevice(h->device));
  int rc = BaEnsureJacobianBuffers(h, jac_mode, want_cam);
  if (rc) return rc;
  PP_HIP_TRY(hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < repeat; ++i) {
    rc = LaunchEval(h, jac_mode, want_cam, false, h->poses, h->points, nullptr);
    if (rc) return rc;
  }
  PP_HIP_TRY(hipEventRecord(h->ev1, h->stream));
  PP_HIP_TRY(hipEventSynchronize(h->ev1));
  float ms = 0;
  PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (ms_per_launch) *ms_per_launch = ms / repeat;
  return PP_OK;
} PP_API_CATCH("pp_ba_eval_device")

}  // extern "C"
