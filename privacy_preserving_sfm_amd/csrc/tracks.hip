// K10 - track completion and merging: IncrementalTriangulator::CompleteTracks / MergeTracks and their All forms
//   Complete   reference src/sfm/incremental_triangulator.cc:697-765      Merge   :606-695      drivers :237-293
//   CalculateSquaredLineReprojectionError   src/base/projection.cc:162-203 (line_error.hpp, shared with K7a)
//   Reconstruction::AddObservation / MergePoints3D   src/base/reconstruction.cc:190-232
// The arithmetic is data-parallel (one line error per candidate), the control flow sequential (a line one point claims is gone for the
// next, a merge creates a point and recurses).  As pp_pose_ransac: the device SPECULATES on the state at the start of the call, the host
// replays the sequential decisions in ascending point order (tracks_replay.hpp).
// K10a k_complete_tracks   one wavefront per point: its whole transitive closure over the free lines that pass, breadth first; the lanes run
//                         over the correspondences of the current frontier line; the accepted lines live in LDS (kLdsList entries), appended
//                         by ballot + lane prefix in (frontier, correspondence) order.  A closure that outgrows the list flags its point,
//                         which the <true> instantiation finishes with a list in global memory sized by the host.
// K10b k_merge_candidates  one wavefront per point: the de-duplicated partner points in (track element, correspondence) order, then per
//                         candidate the merged position and both tracks against it, the lanes over the track elements, 64 at a time, stopping
//                         at the first chunk with a failure.
// K10c k_merge_pair        one wavefront: the same test for ONE pair whose tracks the host hands over (a merged point, a changed candidate).
// (K10a, the handle and the speculative completion live in tracks_device.hpp: pp_tracks_complete_image, tracks_image.hip, runs them too.)
// No kernel here waits for another workgroup; the only atomics reserve a point's output segment (one per point) and sum the counters.
#include "tracks_device.hpp"

namespace ppsfm {

__global__ __launch_bounds__(256) void k_tracks_proj(int C, const double* __restrict__ poses, double* __restrict__ proj) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double R[9];
  QuatToRotNormalized(poses + 7 * (size_t)c, R);      // ComposeProjectionMatrix(qvec, tvec)
  double* o = proj + 12 * (size_t)c;
#pragma unroll
  for (int r = 0; r < 3; ++r) { o[4 * r] = R[3 * r]; o[4 * r + 1] = R[3 * r + 1]; o[4 * r + 2] = R[3 * r + 2]; o[4 * r + 3] = poses[7 * (size_t)c + 4 + r]; }
}

struct MergeArgs {
  double max2;
  int32_t* pool_cand;
  uint8_t* pool_ok;
  unsigned long long pool_cap;
  unsigned long long* counters;      // [0] pool cursor, [1] line errors computed
  int64_t* out_start;
  int32_t* out_count;
  uint8_t* overflow;
};

// every element of track a, then of track b, against the merged position: false at the first chunk of 64 with a failure
template <typename LineAt>
__device__ __forceinline__ bool MergedTracksPass(const TrackDev& d, const double* Xa, const double* Xb, int la, int lb, double max2, int lane, int* evals, LineAt&& line_at) {
  const double wa = (double)la, wb = (double)lb;
  const double M0 = (wa * Xa[0] + wb * Xb[0]) / (wa + wb), M1 = (wa * Xa[1] + wb * Xb[1]) / (wa + wb), M2 = (wa * Xa[2] + wb * Xb[2]) / (wa + wb);
  const int total = la + lb;
  for (int base = 0; base < total; base += 64) {
    const int i = base + lane;
    bool fail = false;
    if (i < total) { ++*evals; fail = TrackLineError(d, M0, M1, M2, line_at(i)) > max2; }
    if (__ballot(fail)) return false;
  }
  return true;
}

__global__ __launch_bounds__(64) void k_merge_candidates(TrackDev d, MergeArgs a) {
  __shared__ int32_t s_cand[kCandList];
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= d.P) return;
  if (lane == 0) { a.out_count[p] = 0; a.out_start[p] = 0; a.overflow[p] = 0; }
  const int e0 = d.track_start[p], e1 = d.track_start[p + 1];
  if (e1 == e0 || (d.subset && !d.subset[p])) return;
  int n = 0;
  bool overflow = false;
  for (int f = e0; f < e1 && !overflow; ++f) {
    const int fl = d.track_line[f];
    const int c0 = d.corr_start[fl], c1 = d.corr_start[fl + 1];
    for (int base = c0; base < c1; base += 64) {
      const int i = base + lane;
      bool cand = false;
      int q = -1;
      if (i < c1) {
        const int l = d.corr_line[i];
        if (d.image_registered[d.line_image[l]]) {
          q = d.line_point[l];
          if (q >= 0 && q != p) {
            bool seen = false;
            for (int j = 0; j < n; ++j) seen = seen || s_cand[j] == q;
            cand = !seen;
          }
        }
      }
      const unsigned long long m = DropLaterDuplicates(__ballot(cand), q, lane);
      const int cnt = __popcll(m);
      if (cnt == 0) continue;
      if (n + cnt > kCandList) { overflow = true; break; }
      if ((m >> lane) & 1) s_cand[n + __popcll(m & ((1ull << lane) - 1))] = q;
      n += cnt;
      __syncthreads();
    }
  }
  unsigned long long off = 0;
  if (lane == 0) {
    if (!overflow && n > 0) {
      off = atomicAdd(&a.counters[0], (unsigned long long)n);
      if (off + (unsigned long long)n > a.pool_cap) overflow = true;
    }
    a.overflow[p] = overflow ? 1 : 0;
    a.out_count[p] = overflow ? 0 : n;
    a.out_start[p] = (int64_t)off;
  }
  overflow = __shfl((int)overflow, 0, 64) != 0;
  off = ((unsigned long long)(unsigned)__shfl((int)(off >> 32), 0, 64) << 32) | (unsigned)__shfl((int)(off & 0xFFFFFFFFull), 0, 64);
  if (overflow) return;
  int evals = 0;
  const double* Xa = d.points + 3 * (size_t)p;
  for (int ci = 0; ci < n; ++ci) {
    const int q = s_cand[ci];
    const int b0 = d.track_start[q], lb = d.track_start[q + 1] - b0, la = e1 - e0;
    const bool ok = MergedTracksPass(d, Xa, d.points + 3 * (size_t)q, la, lb, a.max2, lane, &evals,
                                     [&](int i) { return i < la ? d.track_line[e0 + i] : d.track_line[b0 + i - la]; });
    if (lane == 0) { a.pool_cand[off + ci] = q; a.pool_ok[off + ci] = ok ? 1 : 0; }
  }
  evals = WaveSumInt(evals);
  if (lane == 0) atomicAdd(&a.counters[1], (unsigned long long)evals);
}

// one pair: slot[0] <- 1 / 0, slot[1] <- line errors computed; slot + 2 = the la + lb lines of the two tracks (pinned host memory)
__global__ __launch_bounds__(64) void k_merge_pair(TrackDev d, int32_t* slot, int la, int lb, double xa0, double xa1, double xa2, double xb0, double xb1, double xb2, double max2) {
  const int lane = threadIdx.x;
  const double Xa[3] = {xa0, xa1, xa2}, Xb[3] = {xb0, xb1, xb2};
  const int32_t* lines = slot + 2;
  int evals = 0;
  const bool ok = MergedTracksPass(d, Xa, Xb, la, lb, max2, lane, &evals, [&](int i) { return lines[i]; });
  evals = WaveSumInt(evals);
  if (lane == 0) { slot[1] = evals; slot[0] = ok ? 1 : 0; }
}

}  // namespace ppsfm

int ppsfm::UploadPoses(pp_tracks_impl* h) {
  PP_TRY(Upload(h->d_poses, h->poses.data(), h->poses.size(), h->stream));
  hipLaunchKernelGGL(k_tracks_proj, dim3(CeilDiv(h->C, 256)), dim3(256), 0, h->stream, h->C, h->d_poses, h->d_proj);
  PP_HIP_TRY(hipGetLastError());
  if (h->d_centers) PP_TRY(ComputeCenters(h));
  return PP_OK;
}

using namespace ppsfm;

namespace {

int CheckOptions(const pp_tracks_options* o, const char* where) {
  PP_REQUIRE(o && o->merge_max_reproj_error >= 0 && o->complete_max_reproj_error >= 0 && o->complete_max_transitivity >= 0, "%s: bad options", where);
  return PP_OK;
}

}  // namespace

extern "C" {

void pp_tracks_options_default(pp_tracks_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->merge_max_reproj_error = 4.0; o->complete_max_reproj_error = 4.0; o->complete_max_transitivity = 5;
}

int pp_tracks_destroy(pp_tracks_handle h) try {
  delete h;      // (~DeviceHandle)
  return PP_OK;
} PP_API_CATCH("pp_tracks_destroy")

int pp_tracks_create(const pp_tracks_desc* d, int device, pp_tracks_handle* out) try {
  PP_REQUIRE(d && out, "pp_tracks_create: null argument");
  *out = nullptr;
  const int C = d->num_images, K = d->num_cameras, P = d->num_points;
  const int64_t L = d->num_lines, E = d->num_corrs;
  PP_REQUIRE(C > 0 && K > 0 && P >= 0 && L >= 0 && E >= 0 && L < 0x7FFFFFFF && E < 0x7FFFFFFF, "pp_tracks_create: bad sizes");
  PP_REQUIRE(d->poses && d->pose_camera && d->camera_model && d->intr && d->cam_size && d->corr_start && d->track_start && (P == 0 || d->points) &&
                 (L == 0 || (d->lines && d->line_image && d->line_point)) && (E == 0 || d->corr_line),
             "pp_tracks_create: null array");
  for (int k = 0; k < K; ++k) PP_REQUIRE(pp_camera_num_params(d->camera_model[k]) > 0, "pp_tracks_create: unknown camera model");
  for (int c = 0; c < C; ++c) PP_REQUIRE(d->pose_camera[c] >= 0 && d->pose_camera[c] < K, "pp_tracks_create: camera index out of range");
  PP_REQUIRE(d->corr_start[0] == 0 && d->corr_start[L] == E, "pp_tracks_create: corr_start does not span num_corrs");
  for (int64_t l = 0; l < L; ++l) {
    PP_REQUIRE(d->line_image[l] >= 0 && d->line_image[l] < C, "pp_tracks_create: image index out of range");
    PP_REQUIRE(d->line_point[l] >= -1 && d->line_point[l] < P, "pp_tracks_create: point index out of range");
    PP_REQUIRE(d->corr_start[l] <= d->corr_start[l + 1], "pp_tracks_create: corr_start decreases");
    const double a = d->lines[3 * l], b = d->lines[3 * l + 1];
    PP_REQUIRE(std::fabs(std::sqrt(a * a + b * b) - 1.0) <= 1e-6, "pp_tracks_create: line %lld is not normalised (a^2 + b^2 = 1)", (long long)l);
  }
  for (int64_t e = 0; e < E; ++e) PP_REQUIRE(d->corr_line[e] >= 0 && d->corr_line[e] < L, "pp_tracks_create: correspondence out of range");
  PP_REQUIRE(d->track_start[0] == 0, "pp_tracks_create: track_start[0] != 0");
  for (int p = 0; p < P; ++p) PP_REQUIRE(d->track_start[p] <= d->track_start[p + 1], "pp_tracks_create: track_start decreases");
  const int64_t T = d->track_start[P];
  PP_REQUIRE(T == 0 || d->track_line, "pp_tracks_create: null array");
  {
    std::vector<uint8_t> seen((size_t)L, 0);
    for (int p = 0; p < P; ++p)
      for (int64_t e = d->track_start[p]; e < d->track_start[p + 1]; ++e) {
        const int32_t l = d->track_line[e];
        PP_REQUIRE(l >= 0 && l < L && d->line_point[l] == p && !seen[(size_t)l], "pp_tracks_create: track of point %d and line_point disagree", p);
        seen[(size_t)l] = 1;
      }
    for (int64_t l = 0; l < L; ++l) PP_REQUIRE((d->line_point[l] >= 0) == (seen[(size_t)l] != 0), "pp_tracks_create: line %lld has a point but is in no track", (long long)l);
  }
  PP_TRY(UseDevice("pp_tracks_create", device));
  UnderConstruction<pp_tracks_impl, pp_tracks_destroy> h{new pp_tracks_impl()};
  h->C = C; h->K = K; h->L = L; h->E = E;
  TrackState& st = h->st;
  st.L = L;
  st.line_image.assign(d->line_image, d->line_image + L);
  st.corr_start.assign(d->corr_start, d->corr_start + L + 1);
  st.corr_line.assign(d->corr_line, d->corr_line + E);
  st.image_registered.assign((size_t)C, 1);
  if (d->image_registered) st.image_registered.assign(d->image_registered, d->image_registered + C);
  st.line_point.assign(d->line_point, d->line_point + L);
  st.points.assign(d->points, d->points + 3 * (size_t)P);
  st.tracks.resize((size_t)P);
  st.deleted.assign((size_t)P, 0);
  for (int p = 0; p < P; ++p) { st.tracks[(size_t)p].assign(d->track_line + d->track_start[p], d->track_line + d->track_start[p + 1]); st.deleted[(size_t)p] = st.tracks[(size_t)p].empty(); }
  std::vector<uint8_t> skip((size_t)K, 0);
  if (d->camera_skip) skip.assign(d->camera_skip, d->camera_skip + K);
  h->image_skip.resize((size_t)C);
  for (int c = 0; c < C; ++c) h->image_skip[(size_t)c] = skip[(size_t)d->pose_camera[c]];
  h->pose_camera.assign(d->pose_camera, d->pose_camera + C);
  h->poses.assign(d->poses, d->poses + (size_t)7 * C);
  h->intr.assign(d->intr, d->intr + (size_t)kCamStride * K);
  h->camera_skip = skip;
  PP_TRY(h->Open(device));
  hipStream_t s = h->stream;
  auto put = [&](auto** p, const auto* src, size_t count) { return h->blocks.Put(p, src, count, s, 1); };
  double *d_poses = nullptr, *d_proj = nullptr, *d_intr = nullptr, *d_lines = nullptr;
  int32_t *d_pc = nullptr, *d_cm = nullptr, *d_cs = nullptr, *d_li = nullptr, *d_c0 = nullptr, *d_cl = nullptr;
  uint8_t *d_skip = nullptr, *d_reg = nullptr;
  PP_TRY(put(&d_poses, d->poses, (size_t)7 * C)); PP_TRY(put(&d_proj, (const double*)nullptr, (size_t)12 * C)); PP_TRY(put(&d_intr, d->intr, (size_t)kCamStride * K));
  PP_TRY(put(&d_lines, d->lines, (size_t)3 * L)); PP_TRY(put(&d_pc, d->pose_camera, (size_t)C)); PP_TRY(put(&d_cm, d->camera_model, (size_t)K));
  PP_TRY(put(&d_cs, d->cam_size, (size_t)2 * K)); PP_TRY(put(&d_li, d->line_image, (size_t)L)); PP_TRY(put(&d_c0, d->corr_start, (size_t)L + 1));
  PP_TRY(put(&d_cl, d->corr_line, (size_t)E)); PP_TRY(put(&d_skip, skip.data(), (size_t)K)); PP_TRY(put(&d_reg, st.image_registered.data(), (size_t)C));
  PP_TRY(put(&h->d_line_point, (const int32_t*)nullptr, (size_t)L));
  hipLaunchKernelGGL(k_tracks_proj, dim3(CeilDiv(C, 256)), dim3(256), 0, s, C, d_poses, d_proj);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { SetLastError("pp_tracks_create: upload failed"); return PP_ERR_HIP; }
  h->d_poses = d_poses; h->d_proj = d_proj; h->d_intr = d_intr; h->d_skip = d_skip; h->d_registered = d_reg;
  h->dev.proj = d_proj; h->dev.intr = d_intr; h->dev.lines = d_lines; h->dev.pose_camera = d_pc; h->dev.camera_model = d_cm; h->dev.cam_size = d_cs;
  h->dev.line_image = d_li; h->dev.corr_start = d_c0; h->dev.corr_line = d_cl; h->dev.camera_skip = d_skip; h->dev.image_registered = d_reg;
  *out = h.release();
  return PP_OK;
} PP_API_CATCH("pp_tracks_create")

int pp_tracks_complete(pp_tracks_handle h, const pp_tracks_options* o, const uint8_t* point_subset, pp_tracks_report* report, int32_t* added_point,
                       int32_t* added_line, int64_t capacity) try {
  PP_REQUIRE(h && report && capacity >= 0 && (capacity == 0 || (added_point && added_line)), "pp_tracks_complete: bad argument");
  PP_TRY(CheckOptions(o, "pp_tracks_complete"));
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  PP_HIP_TRY(hipSetDevice(h->device));
  TrackState& st = h->st;
  const int P = st.NumPoints();
  if (P == 0) return PP_OK;
  CompleteSpec spec;
  PP_TRY(SpeculateComplete(h, point_subset, o->complete_max_transitivity, o->complete_max_reproj_error * o->complete_max_reproj_error, "pp_tracks_complete", &spec));
  report->overflow_points = spec.overflow_points; report->second_launches = spec.second_launches;
  report->device_ms = spec.device_ms;
  report->candidates_evaluated = (int64_t)spec.counters[1];
  const auto t_replay = Clock::now();
  int64_t written = 0;
  const CompleteCounters cnt = ReplayComplete(
      st, point_subset, o->complete_max_transitivity, [&](int p) { return spec.List(p); },
      [&](int p, int32_t l) { if (written < capacity) { added_point[written] = p; added_line[written] = l; } ++written; });
  report->num_changed = cnt.num_completed;
  report->num_entries = written;
  report->conflict_replays = cnt.conflict_replays;
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_complete")

int pp_tracks_merge(pp_tracks_handle h, const pp_tracks_options* o, const uint8_t* point_subset, pp_tracks_report* report, int32_t* merged_a,
                    int32_t* merged_b, int32_t* merged_new, int64_t capacity) try {
  PP_REQUIRE(h && report && capacity >= 0 && (capacity == 0 || (merged_a && merged_b && merged_new)), "pp_tracks_merge: bad argument");
  PP_TRY(CheckOptions(o, "pp_tracks_merge"));
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  TrackState& st = h->st;
  const int P0 = st.NumPoints();
  if (P0 == 0) return PP_OK;
  const double max2 = o->merge_max_reproj_error * o->merge_max_reproj_error;
  std::vector<int32_t> start, elems, count((size_t)P0), pool_cand;
  std::vector<int64_t> seg((size_t)P0);
  std::vector<uint8_t> over((size_t)P0), pool_ok;
  unsigned long long counters[2] = {0, 0};
  TrackDev d;
  CallScratch cb(s);      // (the state arrays stay up for the fresh-pair launches)
  PP_TRY(UploadState(h, cb, point_subset, start, elems, &d));
  {
    MergeArgs a{};
    a.max2 = max2;
    a.pool_cap = (unsigned long long)(h->E + 1);      // a line has one point: the candidate lists together hold at most one entry per correspondence
    PP_TRY(cb.Alloc(&a.pool_cand, (size_t)a.pool_cap)); PP_TRY(cb.Alloc(&a.pool_ok, (size_t)a.pool_cap)); PP_TRY(cb.Alloc(&a.counters, 2));
    PP_TRY(cb.Alloc(&a.out_start, (size_t)P0)); PP_TRY(cb.Alloc(&a.out_count, (size_t)P0)); PP_TRY(cb.Alloc(&a.overflow, (size_t)P0));
    PP_HIP_TRY(hipMemsetAsync(a.counters, 0, 2 * sizeof(unsigned long long), s));
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_merge_candidates, dim3(P0), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    PP_TRY(Download(count.data(), a.out_count, (size_t)P0, s)); PP_TRY(Download(seg.data(), a.out_start, (size_t)P0, s)); PP_TRY(Download(over.data(), a.overflow, (size_t)P0, s));
    PP_TRY(Download(counters, a.counters, 2, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    report->device_ms = ms;
    const size_t used = (size_t)std::min<unsigned long long>(counters[0], a.pool_cap);
    pool_cand.resize(used); pool_ok.resize(used);
    PP_TRY(Download(pool_cand.data(), a.pool_cand, used, s)); PP_TRY(Download(pool_ok.data(), a.pool_ok, used, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
  }
  for (int p = 0; p < P0; ++p) report->overflow_points += over[(size_t)p];
  int64_t evaluated = (int64_t)counters[1];
  const auto t_replay = Clock::now();
  auto fresh = [&](int a, int q) -> int {      // one small synchronous launch; the result comes back through the pinned slot
    const std::vector<int32_t>&ta = st.tracks[(size_t)a], &tb = st.tracks[(size_t)q];
    const size_t need = 2 + ta.size() + tb.size();
    if (need > h->pin_ints) {
      h->blocks.Free(&h->pin); h->pin_ints = 0;
      if (h->blocks.AllocPinned(reinterpret_cast<void**>(&h->pin), std::max<size_t>(need * 2, 1024) * sizeof(int32_t))) return PP_ERR_HIP;
      h->pin_ints = std::max<size_t>(need * 2, 1024);
    }
    h->pin[0] = -1; h->pin[1] = 0;
    std::copy(ta.begin(), ta.end(), h->pin + 2);
    std::copy(tb.begin(), tb.end(), h->pin + 2 + ta.size());
    const double *xa = &st.points[3 * (size_t)a], *xb = &st.points[3 * (size_t)q];
    hipLaunchKernelGGL(k_merge_pair, dim3(1), dim3(64), 0, s, d, h->pin, (int)ta.size(), (int)tb.size(), xa[0], xa[1], xa[2], xb[0], xb[1], xb[2], max2);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || h->pin[0] < 0) { SetLastError("pp_tracks_merge: the launch for pair (%d, %d) failed", a, q); return PP_ERR_HIP; }
    ++report->fresh_pair_launches;
    evaluated += h->pin[1];
    return h->pin[0];
  };
  auto eval = [&](int a, int q) -> int {
    if (a < P0 && q < P0 && !over[(size_t)a]) {      // both as the speculation saw them (a merge only deletes points and creates new ones)
      const int32_t* c = pool_cand.data() + seg[(size_t)a];
      for (int32_t i = 0; i < count[(size_t)a]; ++i) if (c[i] == q) return pool_ok[(size_t)seg[(size_t)a] + i];
    }
    return fresh(a, q);
  };
  int64_t written = 0;
  auto emit = [&](int a, int q, int m) { if (written < capacity) { merged_a[written] = a; merged_b[written] = q; merged_new[written] = m; } ++written; };
  MergeReplay<decltype(eval), decltype(emit)> replay{st, eval, emit, {}, {}, 0};
  replay.Run(point_subset);
  if (replay.error) return replay.error;      // (the merges made so far stay applied: the header tells the caller to destroy the handle)
  report->num_changed = replay.cnt.num_merged;
  report->num_entries = written;
  report->candidates_evaluated = evaluated;
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_merge")

int pp_tracks_update(pp_tracks_handle h, int32_t num_images, const int32_t* image_idx, const double* poses, int32_t num_points, const int32_t* point_idx,
                     const double* xyz, const double* intr, const uint8_t* camera_skip) try {
  const char* where = "pp_tracks_update";
  PP_REQUIRE(h && num_images >= 0 && num_points >= 0 && (num_images == 0 || (image_idx && poses)) && (num_points == 0 || (point_idx && xyz)) &&
                 (intr || !camera_skip), "%s: bad argument", where);
  TrackState& st = h->st;
  const int C = h->C, K = h->K;
  for (int32_t i = 0; i < num_images; ++i) {
    PP_REQUIRE(image_idx[i] >= 0 && image_idx[i] < C, "%s: image %d of %d", where, image_idx[i], C);
    for (int j = 0; j < 7; ++j) PP_REQUIRE(std::isfinite(poses[7 * (size_t)i + j]), "%s: the pose of image %d is not finite", where, image_idx[i]);
  }
  for (int32_t i = 0; i < num_points; ++i) {
    PP_REQUIRE(point_idx[i] >= 0 && point_idx[i] < st.NumPoints(), "%s: point %d of %d", where, point_idx[i], st.NumPoints());
    PP_REQUIRE(st.Exists(point_idx[i]), "%s: point %d is deleted", where, point_idx[i]);
    for (int j = 0; j < 3; ++j) PP_REQUIRE(std::isfinite(xyz[3 * (size_t)i + j]), "%s: the position of point %d is not finite", where, point_idx[i]);
  }
  if (intr) for (size_t i = 0; i < (size_t)kCamStride * K; ++i) PP_REQUIRE(std::isfinite(intr[i]), "%s: an intrinsic parameter is not finite", where);
  if (num_images == 0 && num_points == 0 && !intr) return PP_OK;
  for (int32_t i = 0; i < num_points; ++i) std::copy(xyz + 3 * (size_t)i, xyz + 3 * (size_t)i + 3, st.points.begin() + 3 * (size_t)point_idx[i]);      // (the points go up with each call's state)
  if (num_images == 0 && !intr) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (intr) {
    h->intr.assign(intr, intr + (size_t)kCamStride * K);
    h->camera_skip.assign((size_t)K, 0);
    if (camera_skip) h->camera_skip.assign(camera_skip, camera_skip + K);
    for (int c = 0; c < C; ++c) h->image_skip[(size_t)c] = h->camera_skip[(size_t)h->pose_camera[(size_t)c]];
    PP_TRY(Upload(h->d_intr, h->intr.data(), h->intr.size(), s)); PP_TRY(Upload(h->d_skip, h->camera_skip.data(), (size_t)K, s));
  }
  if (num_images > 0) {
    for (int32_t i = 0; i < num_images; ++i) std::copy(poses + 7 * (size_t)i, poses + 7 * (size_t)i + 7, h->poses.begin() + 7 * (size_t)image_idx[i]);
    PP_TRY(UploadPoses(h));
  }
  PP_HIP_TRY(hipStreamSynchronize(s));      // (the host copies are the handle's own: nothing of the caller's is read after the return)
  return PP_OK;
} PP_API_CATCH("pp_tracks_update")

int pp_tracks_get_state(pp_tracks_handle h, int32_t* num_points, int64_t* num_track_elements, int32_t* line_point, double* points, uint8_t* deleted,
                        int32_t* track_start, int32_t* track_line, int32_t point_capacity, int64_t element_capacity) try {
  PP_REQUIRE(h && num_points && num_track_elements, "pp_tracks_get_state: null argument");
  const TrackState& st = h->st;
  const int P = st.NumPoints();
  int64_t T = 0;
  for (int p = 0; p < P; ++p) T += (int64_t)st.tracks[(size_t)p].size();
  *num_points = P; *num_track_elements = T;
  PP_REQUIRE(!(points || deleted || track_start) || point_capacity >= P, "pp_tracks_get_state: point_capacity %d < %d points", point_capacity, P);
  PP_REQUIRE(!track_line || element_capacity >= T, "pp_tracks_get_state: element_capacity too small");
  if (line_point) std::copy(st.line_point.begin(), st.line_point.end(), line_point);
  if (points) std::copy(st.points.begin(), st.points.end(), points);
  if (deleted) for (int p = 0; p < P; ++p) deleted[p] = st.tracks[(size_t)p].empty() ? 1 : 0;
  int64_t e = 0;
  for (int p = 0; p < P; ++p) {
    if (track_start) track_start[p] = (int32_t)e;
    if (track_line) std::copy(st.tracks[(size_t)p].begin(), st.tracks[(size_t)p].end(), track_line + e);
    e += (int64_t)st.tracks[(size_t)p].size();
  }
  if (track_start) track_start[P] = (int32_t)e;
  return PP_OK;
} PP_API_CATCH("pp_tracks_get_state")

}  // extern "C"
