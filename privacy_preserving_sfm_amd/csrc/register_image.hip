// K13 - IncrementalMapper::FindNextImages and RegisterNextImage on a pp_tracks_handle: choosing the next image and registering it.
//   FindNextImages                 reference src/sfm/incremental_mapper.cc:139-190 (ranks :66-73, SortAndAppendNextImages :50-64)
//   RegisterNextImage              :570-760 (gate :585, 2D-3D search :601-647, RANSAC options :668-681, gate :725, commit :743-757)
//   FindTransitiveCorrespondences  src/base/correspondence_graph.cc:166-224 (transitivity 1: the direct list as it is, :169-171)
//   NumObservations / NumVisiblePoints3D   correspondence_graph.cc:58-65, src/base/image.cc:91-98
//   EstimateAbsolutePoseFromLines  src/estimators/pose.cc:52-94 (the RANSAC is pp_pose_ransac, abs_pose.hip, unchanged)
// As K10-K12: the device does the data-parallel part on the state at the start of the call, the host replays the sequential rest
// (register_replay.hpp: ranking and buckets, the gates, the commit rule).
// K13a k_visible_points   ONE LANE PER LINE, over all lines.  A line's work is a scan of its neighbour list that stops at the first neighbour with a
//                         point; lists are a handful of entries long, so a wavefront per line would leave 60 of 64 lanes idle and cost 64 times the
//                         wavefronts, while a lane simply loops (a list longer than 64 is just a longer loop).  Lines are numbered image by image,
//                         so the lanes of a wavefront mostly share an image: the wavefront adds the population count of each image's lanes with one
//                         integer atomic per (image, counter) - order-free and exact - instead of one per line.
// K13b k_register_corrs   <fill = false> counts, <fill = true> writes.  One wavefront per line of the query image, the lanes over its neighbour list
//                         in corr_line order, 64 at a time.  A neighbour is kept when its image is registered, it has a point, its camera is not
//                         flagged, and no earlier kept neighbour OF THIS LINE has the same point: inside a chunk DropLaterDuplicates, across chunks
//                         the list of accepted points - in LDS up to kRegList entries, for a longer neighbour list in a segment of global memory
//                         the host sized by that list (it cannot overflow).  The count form also says whether the line is visible.
//                         The counts are scanned in ascending line index (LaunchExclusiveScan, scan.hpp).
//                         The fill form writes, at offset[line] + rank, the pair (line, point), the six SoA streams and the aligned flag straight into
//                         the buffers of a pose handle (pose_device.hpp): only the pair list travels to the host.
// No kernel here waits for another workgroup.
#include <cfloat>

#include "pose_device.hpp"
#include "register_replay.hpp"
#include "scan.hpp"
#include "tracks_device.hpp"

namespace ppsfm {

constexpr int kRegList = 256;      // accepted points of a line kept on chip (1 KiB of LDS per wavefront)

__global__ __launch_bounds__(256) void k_visible_points(int64_t L, int C, const int32_t* __restrict__ line_image, const int32_t* __restrict__ corr_start,
                                                        const int32_t* __restrict__ corr_line, const int32_t* __restrict__ line_point,
                                                        int32_t* __restrict__ visible, int32_t* __restrict__ observed) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int img = -1;
  bool obs = false, vis = false;
  if (l < L) {
    img = line_image[l];
    const int c0 = corr_start[l], c1 = corr_start[l + 1];
    obs = c1 > c0;
    for (int e = c0; e < c1 && !vis; ++e) vis = line_point[corr_line[e]] >= 0;
  }
  if (img < 0 || img >= C) { img = -1; obs = false; }
  // per image of this wavefront: one atomic per counter
  unsigned long long todo = __ballot(obs);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int li = __shfl(img, leader, 64);
    const unsigned long long same = __ballot(obs && img == li);
    const int nv = __popcll(__ballot(vis && img == li));
    if (lane == leader) {
      atomicAdd(&observed[li], __popcll(same));
      if (nv) atomicAdd(&visible[li], nv);
    }
    todo &= ~same;
  }
}

struct RegArgs {
  int N;                              // lines of the query image
  const int32_t* work_line;           // N, ascending
  const int64_t* glist_off;           // N: -1 = the accepted points stay in LDS, else the line's segment of glist
  int32_t* glist;
  int32_t* count;                     // N (count form: written; fill form: unused)
  int32_t* visible;                   // count form: [0] += lines with a neighbour that has a point
  const int32_t* offset;              // fill form: N, exclusive scan of count
  int32_t total;                      // fill form: entries in all
  int32_t* pair;                      // fill form: total x 2 (line, point)
  PoseStreams out;
  const uint8_t* line_aligned;        // L or nullptr
};

template <bool kFill>
__global__ __launch_bounds__(64) void k_register_corrs(TrackDev d, RegArgs a) {
  __shared__ int32_t s_list[kRegList];
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= a.N) return;
  const int ref = a.work_line[w];
  const int c0 = d.corr_start[ref], c1 = d.corr_start[ref + 1];
  const int64_t goff = a.glist_off[w];
  int32_t* list = goff < 0 ? s_list : a.glist + goff;      // (the host chose: c1 - c0 <= kRegList or a segment of c1 - c0 entries)
  const bool keep_list = c1 - c0 > 64;                      // a single chunk needs no list
  const int base_out = kFill ? a.offset[w] : 0;
  int n = 0;
  bool vis = false;
  for (int base = c0; base < c1; base += 64) {
    const int i = base + lane;
    bool cand = false;
    int q = -1;
    if (i < c1) {
      const int l = d.corr_line[i];
      q = d.line_point[l];
      vis = vis || q >= 0;
      const int img = d.line_image[l];
      if (q >= 0 && q < d.P && d.image_registered[img] && !d.camera_skip[d.pose_camera[img]]) {
        bool seen = false;
        if (keep_list) for (int j = 0; j < n; ++j) seen = seen || list[j] == q;      // (every lane reads the same entry: a broadcast)
        cand = !seen;
      }
    }
    const unsigned long long m = DropLaterDuplicates(__ballot(cand), q, lane);
    const int cnt = __popcll(m);
    if (cnt == 0) continue;
    if ((m >> lane) & 1) {
      const int pos = n + __popcll(m & ((1ull << lane) - 1));
      if (keep_list) list[pos] = q;
      if (kFill && base_out + pos < a.total) {
        const size_t o = (size_t)(base_out + pos);
        a.pair[2 * o] = ref; a.pair[2 * o + 1] = q;
        const double* ln = d.lines + 3 * (size_t)ref;
        const double* X = d.points + 3 * (size_t)q;
        a.out.l0[o] = ln[0]; a.out.l1[o] = ln[1]; a.out.l2[o] = ln[2];
        a.out.x0[o] = X[0]; a.out.x1[o] = X[1]; a.out.x2[o] = X[2];
        if (a.out.aligned) a.out.aligned[o] = a.line_aligned ? a.line_aligned[ref] : 0;
      }
    }
    n += cnt;
    if (keep_list) __syncthreads();      // (one wavefront per workgroup, wave-uniform control flow: the appended entries become visible to every lane)
  }
  if (!kFill) {
    const bool any = __ballot(vis) != 0;      // (every lane takes part)
    if (lane == 0) {
      a.count[w] = n;
      if (any) atomicAdd(a.visible, 1);
    }
  }
}

}  // namespace ppsfm

using namespace ppsfm;

namespace {

int CheckNextImageOptions(const pp_next_image_options* o, const char* where) {
  PP_REQUIRE(o && o->abs_pose_min_num_inliers > 0 && o->max_reg_trials >= 0 && (o->image_selection_method == 0 || o->image_selection_method == 1),
             "%s: bad options", where);
  return PP_OK;
}

struct PoseHandleGuard {
  pp_pose_handle p = nullptr;
  ~PoseHandleGuard() { if (p) (void)pp_pose_destroy(p); }
};

}  // namespace

extern "C" {

void pp_next_image_options_default(pp_next_image_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->abs_pose_min_num_inliers = 30; o->max_reg_trials = 3; o->image_selection_method = 1;
}

int pp_tracks_find_next_images(pp_tracks_handle h, const pp_next_image_options* o, const int32_t* num_reg_trials, const uint8_t* filtered,
                               pp_next_image_report* report, int32_t* ranked, int32_t capacity, int32_t* num_visible, int32_t* num_observations) try {
  const char* where = "pp_tracks_find_next_images";
  PP_REQUIRE(h && report && capacity >= 0 && (capacity == 0 || ranked), "%s: bad argument", where);
  PP_TRY(CheckNextImageOptions(o, where));
  const int C = h->C;
  if (num_reg_trials) for (int c = 0; c < C; ++c) PP_REQUIRE(num_reg_trials[c] >= 0, "%s: num_reg_trials[%d] is negative", where, c);
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  const TrackState& st = h->st;
  std::vector<int32_t> counts(2 * (size_t)C, 0);      // visible, then observed
  if (h->L > 0) {
    PP_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CallScratch cb(s);
    int32_t* d_counts = nullptr;
    PP_TRY(cb.Alloc(&d_counts, 2 * (size_t)C));
    PP_TRY(Upload(h->d_line_point, st.line_point.data(), (size_t)h->L, s));
    PP_HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * (size_t)C * sizeof(int32_t), s));
    StreamTimer t(*h);
    PP_TRY(t.Begin());
    hipLaunchKernelGGL(k_visible_points, dim3(CeilDiv(h->L, 256)), dim3(256), 0, s, h->L, C, h->dev.line_image, h->dev.corr_start, h->dev.corr_line,
                       (const int32_t*)h->d_line_point, d_counts, d_counts + C);
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(t.End());
    PP_TRY(Download(counts.data(), d_counts, counts.size(), s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    PP_TRY(t.Add());
    report->device_ms = t.ms;
  }
  const auto t_replay = Clock::now();
  const NextImagesResult r = ReplayFindNextImages(C, counts.data(), counts.data() + C, st.image_registered.data(), num_reg_trials, filtered,
                                                  o->abs_pose_min_num_inliers, o->max_reg_trials, o->image_selection_method);
  report->num_ranked = (int32_t)r.ranked.size(); report->num_first_bucket = r.num_first_bucket; report->num_unregistered = r.num_unregistered;
  for (size_t i = 0; i < r.ranked.size() && i < (size_t)capacity; ++i) ranked[i] = r.ranked[i];
  if (num_visible) std::copy(counts.begin(), counts.begin() + C, num_visible);
  if (num_observations) std::copy(counts.begin() + C, counts.end(), num_observations);
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_find_next_images")

int pp_tracks_estimate_image_pose(pp_tracks_handle h, const pp_next_image_options* o, const pp_ransac_options* ransac, int32_t image,
                                  const uint8_t* line_aligned, pp_image_pose_report* report, double* pose7, int32_t* corr_line, int32_t* corr_point,
                                  uint8_t* inlier_mask, int64_t capacity) try {
  const char* where = "pp_tracks_estimate_image_pose";
  PP_REQUIRE(h && report && ransac && pose7 && capacity >= 0 && (capacity == 0 || (corr_line && corr_point && inlier_mask)), "%s: bad argument", where);
  PP_TRY(CheckNextImageOptions(o, where));
  PP_REQUIRE(image >= 0 && image < h->C, "%s: image %d of %d", where, image, h->C);
  const TrackState& st = h->st;
  PP_REQUIRE(!st.image_registered[(size_t)image], "%s: image %d is registered already", where, image);      // CHECK(!image.IsRegistered()) (:580)
  PP_REQUIRE(ransac->max_error > 0 && ransac->min_inlier_ratio >= 0 && ransac->min_inlier_ratio <= 1 && ransac->confidence >= 0 && ransac->confidence <= 1 &&
                 ransac->min_num_trials <= ransac->max_num_trials, "%s: RANSACOptions::Check failed", where);
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  for (int i = 0; i < 7; ++i) pose7[i] = 0.0;
  if (capacity > 0) std::memset(inlier_mask, 0, (size_t)capacity);
  // the lines of the image, ascending; a neighbour list longer than the on-chip list gets a segment of global memory
  std::vector<int32_t> work;
  std::vector<int64_t> goff;
  int64_t gtotal = 0, max_corrs = 0;
  for (int64_t l = 0; l < st.L; ++l) {
    if (st.line_image[(size_t)l] != image) continue;
    const int64_t len = st.corr_start[(size_t)l + 1] - st.corr_start[(size_t)l];
    work.push_back((int32_t)l);
    goff.push_back(len > kRegList ? gtotal : -1);
    if (len > kRegList) gtotal += len;
    max_corrs += len;
  }
  const int N = (int)work.size();
  auto finish = [&](int failure) {
    report->failure = failure;
    report->total_ms = MsSince(t_begin);
    return PP_OK;
  };
  if (N == 0 || max_corrs == 0) return finish(kRegFewVisible);      // no neighbour at all: NumVisiblePoints3D() = 0 < abs_pose_min_num_inliers
  PP_REQUIRE(max_corrs < 0x7FFFFFFF, "%s: too many correspondences", where);
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  StreamTimer timer(*h);
  PoseHandleGuard pose;      // (destroyed after the call's blocks have drained the stream: declared first)
  CallScratch cb(s);
  TrackDev d = h->dev;
  d.P = st.NumPoints();
  PP_TRY(Upload(h->d_line_point, st.line_point.data(), (size_t)h->L, s));
  d.line_point = h->d_line_point;
  double* d_points = nullptr;
  PP_TRY(cb.Put(&d_points, st.points.data(), st.points.size()));
  d.points = d_points;
  RegArgs a{};
  a.N = N;
  int32_t *d_work = nullptr, *d_offset = nullptr, *d_tot = nullptr, *d_scan = nullptr;
  int64_t* d_goff = nullptr;
  uint8_t* d_aligned = nullptr;
  PP_TRY(cb.Put(&d_work, work.data(), (size_t)N)); PP_TRY(cb.Put(&d_goff, goff.data(), (size_t)N));
  PP_TRY(cb.Alloc(&a.glist, (size_t)gtotal)); PP_TRY(cb.Alloc(&a.count, (size_t)N)); PP_TRY(cb.Alloc(&d_offset, (size_t)N)); PP_TRY(cb.Alloc(&d_tot, 2));
  PP_TRY(cb.Alloc(&d_scan, ScanScratchCount(N)));
  if (line_aligned) PP_TRY(cb.Put(&d_aligned, line_aligned, (size_t)h->L));
  a.work_line = d_work; a.glist_off = d_goff; a.visible = d_tot + 1; a.offset = d_offset; a.line_aligned = d_aligned;
  PP_HIP_TRY(hipMemsetAsync(d_tot, 0, 2 * sizeof(int32_t), s));
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_register_corrs<false>, dim3((unsigned)N), dim3(64), 0, s, d, a);
  const ScanJob<int32_t> offsets{a.count, d_offset, d_tot};
  LaunchExclusiveScan(s, N, &offsets, 1, d_scan);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  int32_t tot[2] = {0, 0};      // entries, visible lines
  PP_TRY(Download(tot, d_tot, 2, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  report->device_ms = timer.ms;
  report->num_visible = tot[1];
  if (!RegisterVisibleGate(tot[1], o->abs_pose_min_num_inliers)) return finish(kRegFewVisible);      // :585 (the reference does not search)
  const int32_t M = tot[0];
  if (M < 0 || (int64_t)M > max_corrs) { SetLastError("%s: the count of correspondences is out of range", where); return PP_ERR_INTERNAL; }
  report->num_corrs = M;
  std::vector<int32_t> pairs(2 * (size_t)M);
  if (M > 0) {
    PP_TRY(PoseCreateUnfilled(M, line_aligned != nullptr, h->device, &pose.p, &a.out));
    a.total = M;
    PP_TRY(cb.Alloc(&a.pair, 2 * (size_t)M));
    PP_TRY(timer.Begin());
    hipLaunchKernelGGL(k_register_corrs<true>, dim3((unsigned)N), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(timer.End());
    PP_TRY(Download(pairs.data(), a.pair, pairs.size(), s));
    PP_HIP_TRY(hipStreamSynchronize(s));      // (the pose handle's own stream starts after this)
    PP_TRY(timer.Add());
    report->device_ms = timer.ms;
    for (int64_t i = 0; i < M && i < capacity; ++i) { corr_line[i] = pairs[2 * (size_t)i]; corr_point[i] = pairs[2 * (size_t)i + 1]; }
  }
  if (!RegisterCorrsGate(M, o->abs_pose_min_num_inliers)) return finish(kRegFewCorrs);      // :653-657
  // EstimateAbsolutePoseFromLines: the RANSAC of pp_pose_ransac on the handle K13b filled
  pp_ransac_report rr;
  std::vector<uint8_t> mask((size_t)M, 0), aligned((size_t)M, 0);
  PP_TRY(pp_pose_ransac(pose.p, ransac, &rr, mask.data()));
  report->device_ms = timer.ms + rr.device_time_s * 1e3;
  const auto t_replay = Clock::now();
  report->num_trials = rr.num_trials; report->num_inliers = (int64_t)rr.num_inliers;
  if (!rr.success) std::fill(mask.begin(), mask.end(), 0);      // (report.inlier_mask stays empty in the reference)
  if (line_aligned) for (int32_t i = 0; i < M; ++i) aligned[(size_t)i] = line_aligned[(size_t)pairs[2 * (size_t)i]];
  const PoseGateResult g = ReplayPoseGates(rr.num_inliers, rr.model, M, mask.data(), line_aligned ? aligned.data() : nullptr, o->abs_pose_min_num_inliers, pose7);
  report->num_aligned_inliers = g.num_aligned_inliers;
  for (int64_t i = 0; i < M && i < capacity; ++i) inlier_mask[i] = mask[(size_t)i];
  report->replay_ms = MsSince(t_replay) + (rr.total_time_s - rr.device_time_s) * 1e3;
  return finish(g.failure);
} PP_API_CATCH("pp_tracks_estimate_image_pose")

int pp_tracks_register_image(pp_tracks_handle h, int32_t image, const double* pose7, int64_t n, const int32_t* corr_line, const int32_t* corr_point,
                             const uint8_t* inlier_mask, int64_t* num_added, int32_t* event_point, int32_t* event_line, int64_t capacity) try {
  const char* where = "pp_tracks_register_image";
  PP_REQUIRE(h && pose7 && n >= 0 && (n == 0 || (corr_line && corr_point)) && capacity >= 0 && (capacity == 0 || (event_point && event_line)), "%s: bad argument", where);
  TrackState& st = h->st;
  static const char* const kWhat[] = {"", "the image does not exist or is registered already", "a line does not belong to the image",
                                      "a point does not exist or is deleted", "the pose is not finite"};
  const int bad = CheckRegisterCommit(st, h->C, image, pose7, n, corr_line, corr_point);
  PP_REQUIRE(bad == 0, "%s: image %d: %s", where, image, kWhat[bad]);
  PP_HIP_TRY(hipSetDevice(h->device));
  int64_t written = 0;
  const int64_t added = ReplayRegisterCommit(st, image, n, corr_line, corr_point, inlier_mask, [&](int p, int32_t l) {
    if (written < capacity) { event_point[written] = p; event_line[written] = l; }
    ++written;
  });
  if (num_added) *num_added = added;
  std::copy(pose7, pose7 + 7, h->poses.begin() + 7 * (size_t)image);
  // (an error from here on leaves the host state ahead of the device copies: as pp_tracks_complete's errors, destroy the handle)
  PP_TRY(Upload(h->d_registered, st.image_registered.data(), (size_t)h->C, h->stream));
  PP_TRY(UploadPoses(h));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
} PP_API_CATCH("pp_tracks_register_image")

}  // extern "C"
