// K8 — batched robust track triangulation: thousands of tiny, independent LORANSAC problems
// (one per track) — the mapper's IncrementalTriangulator calls EstimateTriangulation per track
// (reference src/sfm/incremental_triangulator.cc:214, 536).
//   EstimateTriangulation, TriangulationEstimator::{Estimate, Residuals}      src/estimators/triangulation.cc:55-149
//   TriangulateMultiViewPoint (null vector of the K x 4 system [l_i^T P_i])    src/base/triangulation.cc:41-57
//   LORANSAC<..., InlierSupportMeasurer, CombinationSampler>::Estimate          src/optim/loransac.h:88-235
//   CombinationSampler: the 3-combinations in lexicographic order               src/optim/combination_sampler.cc:41-70
//   residuals: squared pixel line error / squared angular line error            src/base/projection.cc:161-203, 238-262
// One LANE per track; the device functions live in tri_device.hpp (K11b, tracks_image.hip, runs them over the create sets of an image).  The current
// inlier flags of a track live in its slice of the output mask.
#include <algorithm>

#include "ransac_host.hpp"
#include "device_handle.hpp"
#include "tri_device.hpp"

namespace ppsfm {

struct TriArgs {
  int T;
  const int32_t *track_start, *obs_view;
  const double* lines;
  TriModel m;
  unsigned long long min_num_trials;
  uint8_t *success, *mask;
  double* xyz;
  int32_t* num_trials;
};

struct TrackObs {      // observation i of a track: a row of the caller's arrays
  const int32_t* views;
  const double* lines;
  __device__ __forceinline__ int view(int i) const { return views[i]; }
  __device__ __forceinline__ const double* line(int i) const { return lines + 3 * (size_t)i; }
};

__global__ __launch_bounds__(64) void k_triangulate_tracks(TriArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.T) return;
  const int e0 = a.track_start[t], n = a.track_start[t + 1] - e0;
  a.success[t] = 0; a.num_trials[t] = 0;
  a.xyz[3 * t] = a.xyz[3 * t + 1] = a.xyz[3 * t + 2] = 0.0;
  for (int i = 0; i < n; ++i) a.mask[e0 + i] = 0;
  if (n < 3) return;                                                   // triangulation.cc:124-125
  const TrackObs obs{a.obs_view + e0, a.lines + 3 * (size_t)e0};
  double best[3];
  unsigned long long trials;
  const bool ok = TriRansac(a.m, obs, n, a.min_num_trials, a.mask + e0, best, &trials);
  a.num_trials[t] = (int32_t)(trials > 0x7FFFFFFFull ? 0x7FFFFFFFull : trials);
  a.xyz[3 * t] = best[0]; a.xyz[3 * t + 1] = best[1]; a.xyz[3 * t + 2] = best[2];
  a.success[t] = ok ? 1 : 0;
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" int pp_triangulate_tracks(int device, int32_t num_tracks, const int32_t* track_start, const double* lines, const int32_t* obs_view, int32_t num_views,
                                     const double* proj_matrices, const double* proj_centers, const int32_t* view_camera, int32_t num_cameras,
                                     const int32_t* camera_model, const double* intr, const int32_t* cam_size, const pp_triangulation_options* o, uint8_t* success,
                                     double* xyz, uint8_t* inlier_mask, int32_t* num_trials, float* device_ms) try {
  PP_REQUIRE(num_tracks >= 0 && num_views > 0 && num_cameras > 0 && o && (num_tracks == 0 || (track_start && lines && obs_view && success && xyz && inlier_mask && num_trials)) &&
                 proj_matrices && proj_centers && view_camera && camera_model && intr && cam_size,
             "pp_triangulate_tracks: bad argument");
  PP_REQUIRE(o->min_tri_angle >= 0 && o->ransac.max_error > 0 && (o->residual_type == 0 || o->residual_type == 1), "pp_triangulate_tracks: bad options");
  if (num_tracks == 0) return PP_OK;
  const int64_t N = track_start[num_tracks];
  for (int64_t i = 0; i < N; ++i) PP_REQUIRE(obs_view[i] >= 0 && obs_view[i] < num_views, "pp_triangulate_tracks: view index out of range");
  for (int v = 0; v < num_views; ++v) PP_REQUIRE(view_camera[v] >= 0 && view_camera[v] < num_cameras, "pp_triangulate_tracks: camera index out of range");
  for (int k = 0; k < num_cameras; ++k) PP_REQUIRE(pp_camera_num_params(camera_model[k]) > 0, "pp_triangulate_tracks: unknown camera model");
  PP_TRY(UseDevice("pp_triangulate_tracks", device));
  TriArgs a{};
  int32_t *d_ts = nullptr, *d_ov = nullptr, *d_vc = nullptr, *d_cm = nullptr, *d_cs = nullptr, *d_nt = nullptr;
  double *d_l = nullptr, *d_P = nullptr, *d_c = nullptr, *d_in = nullptr, *d_xyz = nullptr;
  uint8_t *d_s = nullptr, *d_m = nullptr;
  DeviceHandle call(false);      // the call's stream, events and blocks (plain hipMalloc)
  PP_TRY(call.Open(device));
  const hipStream_t s = call.stream;
  DeviceBlocks& scratch = call.blocks;
  PP_TRY(scratch.Put(&d_ts, track_start, (size_t)num_tracks + 1, s)); PP_TRY(scratch.Put(&d_ov, obs_view, (size_t)N, s)); PP_TRY(scratch.Put(&d_vc, view_camera, (size_t)num_views, s));
  PP_TRY(scratch.Put(&d_cm, camera_model, (size_t)num_cameras, s)); PP_TRY(scratch.Put(&d_cs, cam_size, (size_t)2 * num_cameras, s)); PP_TRY(scratch.Alloc(&d_nt, (size_t)num_tracks));
  PP_TRY(scratch.Put(&d_l, lines, (size_t)3 * N, s)); PP_TRY(scratch.Put(&d_P, proj_matrices, (size_t)12 * num_views, s)); PP_TRY(scratch.Put(&d_c, proj_centers, (size_t)3 * num_views, s));
  PP_TRY(scratch.Put(&d_in, intr, (size_t)kCamStride * num_cameras, s)); PP_TRY(scratch.Alloc(&d_xyz, (size_t)3 * num_tracks));
  PP_TRY(scratch.Alloc(&d_s, (size_t)num_tracks)); PP_TRY(scratch.Alloc(&d_m, (size_t)std::max<int64_t>(N, 1)));
  a.T = num_tracks; a.track_start = d_ts; a.obs_view = d_ov; a.lines = d_l;
  a.m.view_camera = d_vc; a.m.camera_model = d_cm; a.m.cam_size = d_cs; a.m.P = d_P; a.m.centers = d_c; a.m.intr = d_in;
  a.m.min_tri_angle = o->min_tri_angle; a.m.max_residual = o->ransac.max_error * o->ransac.max_error; a.m.confidence = o->ransac.confidence;
  a.m.multiplier = o->ransac.dyn_num_trials_multiplier; a.m.residual_type = o->residual_type; a.min_num_trials = o->ransac.min_num_trials;
  {  // RANSAC ctor: cap max_num_trials from the a-priori inlier ratio (optim/ransac.h:149-155)
    const uint64_t cap = ComputeNumTrials((uint64_t)(o->ransac.min_inlier_ratio * 100000), 100000, o->ransac.confidence, o->ransac.dyn_num_trials_multiplier, 3);
    a.m.max_num_trials = std::min<uint64_t>(o->ransac.max_num_trials, cap);
  }
  a.success = d_s; a.mask = d_m; a.xyz = d_xyz; a.num_trials = d_nt;
  StreamTimer timer(call);
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_triangulate_tracks, dim3(CeilDiv(num_tracks, 64)), dim3(64), 0, s, a);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  PP_TRY(Download(success, d_s, (size_t)num_tracks, s)); PP_TRY(Download(xyz, d_xyz, (size_t)3 * num_tracks, s)); PP_TRY(Download(inlier_mask, d_m, (size_t)N, s));
  PP_TRY(Download(num_trials, d_nt, (size_t)num_tracks, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  if (device_ms) *device_ms = timer.ms;
  return PP_OK;
} PP_API_CATCH("pp_triangulate_tracks")
