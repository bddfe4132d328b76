// K16 - BundleAdjuster::SetUp on a pp_tracks_handle: which observations, poses, points and cameras a BundleAdjustmentConfig puts into the problem.
//   SetUp                                    reference src/optim/bundle_adjustment.cc:326-542
//   AddImageToProblem :348-435 (pass A)      AddPointToProblem :437-488 (pass B)      ParameterizeCameras :490-528      ParameterizePoints :530-542
// As K10-K15: the device does the line- and track-element-sized part on what the handle holds, the host validates first and does the image- and
// camera-sized rest afterwards (bundle_setup_replay.hpp).  The stream of observations is pass A (the config's lines with a point, ascending) followed by
// pass B (the out-of-config track elements of the listed points, point by point in the order given, each track in track order).
// K16 k_bundle_lines        one lane per line: flag[l] = the line is an observation of pass A; an integer atomicAdd into count_a[point]; the norm test of
//                           :373 with an integer atomicMin of the line number for bad_line.
//     LaunchExclusiveScan   (scan.hpp) the exclusive int scans: the flags of pass A over L, the counts of pass B over the listed points, and the two
//                           first-appearance flag arrays over M as two jobs of one call, side by side in the same launches.
//     k_bundle_tracks       <fill = false> counts, <fill = true> writes.  ONE WAVEFRONT PER LISTED POINT: a point whose count_a equals its track length is
//                           skipped; of the others the track is walked in 64-element chunks in track order, a ballot ranks the elements whose image is
//                           not in the config.
//     k_bundle_lines_fill   one lane per line: the flagged lines to their stream positions.
//     k_bundle_first        one lane per observation: integer atomicMin of the stream position into first_point[point] and first_image[image].
//     k_bundle_first_flags  one lane per observation: 1 where the observation is its point's / its image's first.  Their scans are the ranks.
//     k_bundle_gather       one lane per observation: obs_point / obs_pose through the ranks, the line coefficients from the handle's resident L x 3; the
//                           first observation of a point also writes point_index, the position and point_const, that of an image pose_image.
// Integer atomics only, each with an order-free result (a sum, a minimum): the output is the same whatever the schedule.  No kernel waits for another
// workgroup.
#include <climits>
#include <cstring>

#include "bundle_setup_replay.hpp"
#include "scan.hpp"
#include "tracks_device.hpp"

namespace ppsfm {

struct BundleArgs {
  int64_t L;
  int P, C, Q;                      // points of the state, images, listed points
  const uint8_t* image_flags;       // C
  const uint8_t* mark;              // P (BundlePointList::mark)
  const int32_t* listed;            // Q
  int32_t* flag_a;                  // L
  int32_t* pos_a;                   // L + 1: exclusive scan of flag_a, the total last
  int32_t* count_a;                 // P: observations of pass A per point
  int32_t* count_b;                 // P: observations of pass B per point (0 for a point that is not listed or is skipped)
  int32_t* listed_count;            // Q: count_b of the listed points, in list order
  int32_t* pos_b;                   // Q + 1
  int32_t* bad_line;                // 1, INT_MAX = none
  // the stream (valid once M is known)
  int M_a, M;
  int32_t *obs_line, *obs_key;      // M: handle line and handle point of each observation
  unsigned *first_point, *first_image;      // P, C: stream position of the first observation, 0xFFFFFFFF = none
  int32_t *flag_point, *flag_image;         // M
  int32_t *rank_point, *rank_image;         // M + 1
  // outputs
  double* lines;                    // M x 3
  int32_t *obs_pose, *obs_point;    // M
  int32_t *point_index, *pose_image;
  uint8_t* point_const;
  double* points;
  int point_cap, pose_cap;
};

__global__ __launch_bounds__(256) void k_bundle_lines(TrackDev d, BundleArgs a) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= a.L) return;
  const int img = d.line_image[l], p = d.line_point[l];
  const bool obs = img >= 0 && img < a.C && (a.image_flags[img] & kBundleImage) && p >= 0 && p < a.P;
  a.flag_a[l] = obs ? 1 : 0;
  if (!obs) return;
  atomicAdd(&a.count_a[p], 1);
  const double la = d.lines[3 * l], lb = d.lines[3 * l + 1];
  if (fabs(hypot(la, lb) - 1.0) > 1e-6) atomicMin(a.bad_line, (int)l);
}

template <bool kFill>
__global__ __launch_bounds__(64) void k_bundle_tracks(TrackDev d, BundleArgs a) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= a.Q) return;
  const int p = a.listed[q];
  if (p < 0 || p >= a.P) return;      // (the host validated the lists)
  const int e0 = d.track_start[p], e1 = d.track_start[p + 1];
  int n = 0;
  if (a.count_a[p] != e1 - e0) {      // else: every observation of the point is in the problem already (:444-447)
    const int64_t base_pos = kFill ? (int64_t)a.M_a + a.pos_b[q] : 0;
    for (int base = e0; base < e1; base += 64) {
      const int e = base + lane;
      bool outside = false;
      int l = -1;
      if (e < e1) {
        l = d.track_line[e];
        const int img = d.line_image[l];
        outside = !(img >= 0 && img < a.C && (a.image_flags[img] & kBundleImage));
      }
      const unsigned long long m = __ballot(outside);
      if (kFill && outside) {
        const int64_t pos = base_pos + n + __popcll(m & ((1ull << lane) - 1));
        if (pos < a.M) { a.obs_line[pos] = l; a.obs_key[pos] = p; }
      }
      n += __popcll(m);
    }
  }
  if (!kFill && lane == 0) { a.listed_count[q] = n; a.count_b[p] = n; }      // (a point is listed once: no other wavefront writes count_b[p])
}

__global__ __launch_bounds__(256) void k_bundle_lines_fill(TrackDev d, BundleArgs a) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= a.L || !a.flag_a[l]) return;
  const int pos = a.pos_a[l];
  if (pos < 0 || pos >= a.M_a) return;
  a.obs_line[pos] = (int32_t)l;
  a.obs_key[pos] = d.line_point[l];
}

__global__ __launch_bounds__(256) void k_bundle_first(TrackDev d, BundleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.M) return;
  atomicMin(&a.first_point[a.obs_key[i]], (unsigned)i);
  atomicMin(&a.first_image[d.line_image[a.obs_line[i]]], (unsigned)i);
}

__global__ __launch_bounds__(256) void k_bundle_first_flags(TrackDev d, BundleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.M) return;
  a.flag_point[i] = a.first_point[a.obs_key[i]] == (unsigned)i;
  a.flag_image[i] = a.first_image[d.line_image[a.obs_line[i]]] == (unsigned)i;
}

__global__ __launch_bounds__(256) void k_bundle_gather(TrackDev d, BundleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.M) return;
  const int l = a.obs_line[i], p = a.obs_key[i], img = d.line_image[l];
  a.obs_point[i] = a.rank_point[a.first_point[p]];
  a.obs_pose[i] = a.rank_image[a.first_image[img]];
  a.lines[3 * i] = d.lines[3 * (size_t)l]; a.lines[3 * i + 1] = d.lines[3 * (size_t)l + 1]; a.lines[3 * i + 2] = d.lines[3 * (size_t)l + 2];
  if (a.flag_point[i]) {
    const int k = a.rank_point[i];
    if (k >= 0 && k < a.point_cap) {
      a.point_index[k] = p;
      a.points[3 * (size_t)k] = d.points[3 * (size_t)p]; a.points[3 * (size_t)k + 1] = d.points[3 * (size_t)p + 1]; a.points[3 * (size_t)k + 2] = d.points[3 * (size_t)p + 2];
      const int len = d.track_start[p + 1] - d.track_start[p];
      a.point_const[k] = (len > a.count_a[p] + a.count_b[p] || (a.mark[p] & kBundleListedConst)) ? 1 : 0;      // :530-542
    }
  }
  if (a.flag_image[i]) {
    const int k = a.rank_image[i];
    if (k >= 0 && k < a.pose_cap) a.pose_image[k] = img;
  }
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

int pp_tracks_bundle_setup(pp_tracks_handle h, const pp_bundle_config* cfg, pp_bundle_setup_report* report, double* lines, int32_t* obs_pose,
                           int32_t* obs_point, int32_t* obs_line, int64_t obs_capacity, int32_t* pose_image, uint8_t* pose_const, uint8_t* pose_tvec_mask,
                           int32_t* pose_camera, int32_t* point_index, uint8_t* point_const, double* points, int32_t point_capacity, int32_t* camera_index,
                           uint16_t* camera_const_mask) try {
  const char* where = "pp_tracks_bundle_setup";
  PP_REQUIRE(h && cfg && report, "%s: bad argument", where);
  PP_REQUIRE(lines && obs_pose && obs_point && obs_line && pose_image && pose_const && pose_tvec_mask && pose_camera && point_index && point_const && points &&
                 camera_index && camera_const_mask && obs_capacity >= 0 && point_capacity >= 0, "%s: bad argument", where);
  const TrackState& st = h->st;
  const int C = h->C, K = h->K, P = st.NumPoints();
  const BundleConfigView view{cfg->image_flags, cfg->tvec_const_mask, cfg->camera_const, cfg->camera_subset_mask, cfg->variable_points, cfg->constant_points,
                              cfg->num_variable_points, cfg->num_constant_points};
  {
    const std::string wrong = ValidateBundleConfig(st, C, view);
    PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  }
  const auto t_begin = Clock::now();
  const BundlePointList list = DedupBundlePoints(P, view);
  const int Q = (int)list.points.size();
  int64_t T = 0;      // what always suffices: every track element, every existing point
  int32_t existing = 0;
  for (int p = 0; p < P; ++p) { T += (int64_t)st.tracks[(size_t)p].size(); existing += st.Exists(p); }
  PP_REQUIRE(T < 0x7FFFFFFFll && h->L < 0x7FFFFFFFll, "%s: too many track elements or lines", where);
  if (obs_capacity < T || point_capacity < existing) {
    int64_t need_obs = 0;
    int32_t need_points = 0;
    CountBundleSetup(st, cfg->image_flags, list.points, &need_obs, &need_points);
    PP_REQUIRE(need_obs <= obs_capacity, "%s: %lld observations, obs_capacity is %lld", where, (long long)need_obs, (long long)obs_capacity);
    PP_REQUIRE(need_points <= point_capacity, "%s: %d points, point_capacity is %d", where, need_points, point_capacity);
  }
  const double host_ms = MsSince(t_begin);
  std::memset(report, 0, sizeof(*report));
  report->bad_line = -1;
  auto finish = [&](double replay_ms) {
    report->replay_ms = host_ms + replay_ms;
    report->total_ms = MsSince(t_begin);
    return PP_OK;
  };
  const int64_t L = h->L;
  if (L == 0 || P == 0) return finish(0.0);      // no line has a point
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  StreamTimer timer(*h);
  CallScratch cb(s);
  std::vector<int32_t> start, elems;
  TrackDev d;
  PP_TRY(UploadState(h, cb, nullptr, start, elems, &d));
  BundleArgs a{};
  a.L = L; a.P = P; a.C = C; a.Q = Q;
  uint8_t *d_flags = nullptr, *d_mark = nullptr;
  int32_t* d_listed = nullptr;
  PP_TRY(cb.Put(&d_flags, cfg->image_flags, (size_t)C)); PP_TRY(cb.Put(&d_mark, list.mark.data(), (size_t)P)); PP_TRY(cb.Put(&d_listed, list.points.data(), (size_t)Q));
  a.image_flags = d_flags; a.mark = d_mark; a.listed = d_listed;
  PP_TRY(cb.Alloc(&a.flag_a, (size_t)L)); PP_TRY(cb.Alloc(&a.pos_a, (size_t)L + 1)); PP_TRY(cb.Alloc(&a.count_a, (size_t)P)); PP_TRY(cb.Alloc(&a.count_b, (size_t)P));
  PP_TRY(cb.Alloc(&a.listed_count, (size_t)Q)); PP_TRY(cb.Alloc(&a.pos_b, (size_t)Q + 1)); PP_TRY(cb.Alloc(&a.bad_line, 1));
  PP_TRY(cb.Alloc(&a.first_point, (size_t)P)); PP_TRY(cb.Alloc(&a.first_image, (size_t)C));
  const int32_t none = INT_MAX;
  PP_HIP_TRY(hipMemsetAsync(a.count_a, 0, (size_t)P * sizeof(int32_t), s)); PP_HIP_TRY(hipMemsetAsync(a.count_b, 0, (size_t)P * sizeof(int32_t), s));
  PP_HIP_TRY(hipMemsetAsync(a.pos_b, 0, ((size_t)Q + 1) * sizeof(int32_t), s));
  PP_HIP_TRY(hipMemsetAsync(a.first_point, 0xFF, (size_t)P * sizeof(unsigned), s)); PP_HIP_TRY(hipMemsetAsync(a.first_image, 0xFF, (size_t)C * sizeof(unsigned), s));
  PP_TRY(Upload(a.bad_line, &none, 1, s));
  int32_t* d_scan = nullptr;      // the scratch of both scans: they follow each other on the stream
  PP_TRY(cb.Alloc(&d_scan, std::max(ScanScratchCount(L), ScanScratchCount(Q))));
  const ScanJob<int32_t> scan_a{a.flag_a, a.pos_a, a.pos_a + L}, scan_b{a.listed_count, a.pos_b, a.pos_b + Q};
  // the counts: pass A over the lines, pass B over the listed points
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_bundle_lines, dim3(CeilDiv(L, 256)), dim3(256), 0, s, d, a);
  LaunchExclusiveScan(s, L, &scan_a, 1, d_scan);
  if (Q > 0) {
    hipLaunchKernelGGL(k_bundle_tracks<false>, dim3((unsigned)Q), dim3(64), 0, s, d, a);
    LaunchExclusiveScan(s, Q, &scan_b, 1, d_scan);
  }
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  int32_t M_a = 0, M_b = 0, bad = none;
  PP_TRY(Download(&M_a, a.pos_a + L, 1, s)); PP_TRY(Download(&M_b, a.pos_b + Q, 1, s)); PP_TRY(Download(&bad, a.bad_line, 1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  report->device_ms = timer.ms;
  const int64_t M = (int64_t)M_a + M_b;
  if (M_a < 0 || M_b < 0 || M > T || M > obs_capacity) { SetLastError("%s: the count of observations is out of range", where); return PP_ERR_INTERNAL; }
  report->num_obs = M; report->num_config_obs = M_a;
  report->bad_line = bad == none ? -1 : bad;
  if (M == 0) return finish(0.0);
  // the stream, the ranks of first appearance, the gather
  a.M_a = M_a; a.M = (int)M;
  a.point_cap = (int)std::min<int64_t>(M, std::min<int64_t>(P, point_capacity)); a.pose_cap = (int)std::min<int64_t>(M, C);
  PP_TRY(cb.Alloc(&a.obs_line, (size_t)M)); PP_TRY(cb.Alloc(&a.obs_key, (size_t)M)); PP_TRY(cb.Alloc(&a.flag_point, (size_t)M)); PP_TRY(cb.Alloc(&a.flag_image, (size_t)M));
  PP_TRY(cb.Alloc(&a.rank_point, (size_t)M + 1)); PP_TRY(cb.Alloc(&a.rank_image, (size_t)M + 1));
  PP_TRY(cb.Alloc(&a.lines, 3 * (size_t)M)); PP_TRY(cb.Alloc(&a.obs_pose, (size_t)M)); PP_TRY(cb.Alloc(&a.obs_point, (size_t)M));
  PP_TRY(cb.Alloc(&a.point_index, (size_t)a.point_cap)); PP_TRY(cb.Alloc(&a.point_const, (size_t)a.point_cap)); PP_TRY(cb.Alloc(&a.points, 3 * (size_t)a.point_cap));
  PP_TRY(cb.Alloc(&a.pose_image, (size_t)a.pose_cap));
  int32_t* d_ranks = nullptr;
  PP_TRY(cb.Alloc(&d_ranks, 2 * ScanScratchCount(M)));
  PP_HIP_TRY(hipMemsetAsync(a.obs_line, 0, (size_t)M * sizeof(int32_t), s));      // (an entry a fill left out would still name a line and a point that exist)
  PP_HIP_TRY(hipMemsetAsync(a.obs_key, 0, (size_t)M * sizeof(int32_t), s));
  const unsigned grid_m = (unsigned)CeilDiv(M, 256);
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_bundle_lines_fill, dim3(CeilDiv(L, 256)), dim3(256), 0, s, d, a);
  if (M_b > 0) hipLaunchKernelGGL(k_bundle_tracks<true>, dim3((unsigned)Q), dim3(64), 0, s, d, a);
  hipLaunchKernelGGL(k_bundle_first, dim3(grid_m), dim3(256), 0, s, d, a);
  hipLaunchKernelGGL(k_bundle_first_flags, dim3(grid_m), dim3(256), 0, s, d, a);
  const ScanJob<int32_t> ranks[2] = {{a.flag_point, a.rank_point, a.rank_point + M}, {a.flag_image, a.rank_image, a.rank_image + M}};
  LaunchExclusiveScan(s, M, ranks, 2, d_ranks);
  hipLaunchKernelGGL(k_bundle_gather, dim3(grid_m), dim3(256), 0, s, d, a);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  int32_t num_points = 0, num_poses = 0;
  PP_TRY(Download(&num_points, a.rank_point + M, 1, s)); PP_TRY(Download(&num_poses, a.rank_image + M, 1, s));
  PP_TRY(Download(lines, a.lines, 3 * (size_t)M, s)); PP_TRY(Download(obs_pose, a.obs_pose, (size_t)M, s)); PP_TRY(Download(obs_point, a.obs_point, (size_t)M, s));
  PP_TRY(Download(obs_line, a.obs_line, (size_t)M, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  report->device_ms = timer.ms;
  if (num_points <= 0 || num_points > a.point_cap || num_poses <= 0 || num_poses > a.pose_cap) {
    SetLastError("%s: the count of points (%d) or poses (%d) is out of range", where, num_points, num_poses);
    return PP_ERR_INTERNAL;
  }
  PP_TRY(Download(point_index, a.point_index, (size_t)num_points, s)); PP_TRY(Download(point_const, a.point_const, (size_t)num_points, s));
  PP_TRY(Download(points, a.points, 3 * (size_t)num_points, s)); PP_TRY(Download(pose_image, a.pose_image, (size_t)num_poses, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  const auto t_replay = Clock::now();
  const BundlePoseResult r = ReplayBundlePoses(pose_image, num_poses, h->pose_camera.data(), K, view);
  std::copy(r.pose_const.begin(), r.pose_const.end(), pose_const); std::copy(r.pose_tvec_mask.begin(), r.pose_tvec_mask.end(), pose_tvec_mask);
  std::copy(r.pose_camera.begin(), r.pose_camera.end(), pose_camera);
  std::copy(r.camera_index.begin(), r.camera_index.end(), camera_index); std::copy(r.camera_const_mask.begin(), r.camera_const_mask.end(), camera_const_mask);
  report->num_poses = num_poses; report->num_points = num_points; report->num_cameras = (int32_t)r.camera_index.size();
  int32_t config_poses = 0;
  for (int32_t k = 0; k < num_poses; ++k) config_poses += (cfg->image_flags[pose_image[k]] & kBundleImage) != 0;
  report->num_config_poses = config_poses;
  return finish(MsSince(t_replay));
} PP_API_CATCH("pp_tracks_bundle_setup")

}  // extern "C"
