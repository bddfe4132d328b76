// K14 - deletion on a live pp_tracks_handle: the mapper's three filters and the de-registration of an image
//   Reconstruction::FilterPoints3D / FilterPoints3DInImages / FilterAllPoints3D       reference src/base/reconstruction.cc:412-439, 594-719
//   Reconstruction::FilterObservationsWithNegativeDepth :442-460     FilterImages :462-484     DeRegisterImage :285-300     DeleteObservation :255-275
//   CalculateSquaredLineReprojectionError src/base/projection.cc:162-203 (line_error.hpp)     CalculateTriangulationAngle src/base/triangulation.cc:59-82
// The rules are those of K7b k_filter_points (ba_filter.hip), which runs them on a pp_ba_handle; here they run on the tracks the handle already holds, so
// that nothing is flattened and no second problem is built.  The device gives verdicts on the state at the start of the call, the host applies them
// (tracks_filter_replay.hpp) - points are independent under the point filter, and the negative-depth test of a line does not depend on the other lines.
// K14a k_track_filter  one wavefront per point.  The lanes stride over the track (line error per element, a ballot for "has a line that is not aligned",
//                      the count of elements above the threshold, the sum of sqrt(err2) over the others), then over the PAIRS of surviving elements for
//                      the triangulation angle, 64 pairs at a time, leaving at the first chunk with a sufficient angle.  A track of any length takes as
//                      many lane passes as it needs; the per-element flags live in global memory (the output), nothing is kept on chip.
// K14b k_track_depth   one lane per line: HasPointPositiveDepth on the handle's projection matrix, as K7a k_filter_obs.
// No kernel here waits for another workgroup and none uses an atomic: every wavefront (lane) writes its own point's (line's) outputs.
#include "tracks_device.hpp"
#include "tracks_filter_replay.hpp"

namespace ppsfm {

struct TrackFilterArgs {
  const uint8_t* aligned;        // L or nullptr (none aligned)
  const uint8_t* image_subset;   // C or nullptr; the point subset is TrackDev::subset
  const double* centers;         // C x 3
  double max2, min_rad;
  uint8_t* verdict;              // P: kFilter*
  int32_t* ndel;                 // P: elements above the threshold (kept points and points deleted by the angle)
  double* error;                 // P: mean of sqrt(err2) over the survivors, -1 where not set
  uint8_t* elem_flag;            // one per track element, aligned with track_start / track_line
};

__global__ __launch_bounds__(64) void k_track_filter(TrackDev d, TrackFilterArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= d.P) return;
  const int e0 = d.track_start[p], len = d.track_start[p + 1] - e0;
  if (lane == 0) { a.verdict[p] = kFilterNotTested; a.ndel[p] = 0; a.error[p] = -1.0; }
  if (len == 0 || (d.subset && !d.subset[p])) return;      // (a deleted point in a subset is skipped, as an id that no longer exists)
  if (a.image_subset) {      // FilterPoints3DInImages: the points the lines of these images have
    bool in_images = false;
    for (int base = 0; base < len && !in_images; base += 64) {
      const int i = base + lane;
      in_images = __ballot(i < len && a.image_subset[d.line_image[d.track_line[e0 + i]]]) != 0;
    }
    if (!in_images) return;
  }
  const double X0 = d.points[3 * (size_t)p], X1 = d.points[3 * (size_t)p + 1], X2 = d.points[3 * (size_t)p + 2];
  bool non_aligned = false;
  int ndel = 0;
  double sum = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    bool free_line = false;
    if (i < len) {
      const int l = d.track_line[e0 + i];
      free_line = !(a.aligned && a.aligned[l]);
      const double err2 = TrackLineError(d, X0, X1, X2, l);
      const bool bad = err2 > a.max2;
      a.elem_flag[e0 + i] = bad ? 1 : 0;
      if (bad) ++ndel; else sum += sqrt(err2);
    }
    non_aligned = non_aligned || __ballot(free_line) != 0;
  }
  ndel = WaveSumInt(ndel);
  sum = WaveSum(sum);
  if (!non_aligned || len < 3 || ndel >= len - 3) {      // reconstruction.cc:673-689, :705-707 (a track of exactly 3 never survives)
    if (lane == 0) a.verdict[p] = kFilterDeletedByTrack;
    return;
  }
  __syncthreads();      // (one wavefront per workgroup, wave-uniform control flow: the flags written above become visible to every lane)
  // FilterPoints3DWithSmallTriangulationAngle (:594-654) over the pairs (i1, i2 < i1) of the elements that stay
  const long long num_pairs = (long long)len * (len - 1) / 2;
  bool keep = false;
  for (long long base = 0; base < num_pairs && !keep; base += 64) {
    const long long k = base + lane;
    bool ok = false;
    if (k < num_pairs) {
      long long i1 = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
      while (i1 * (i1 - 1) / 2 > k) --i1;
      while ((i1 + 1) * i1 / 2 <= k) ++i1;
      const long long i2 = k - i1 * (i1 - 1) / 2;      // 0 <= i2 < i1 < len
      if (!a.elem_flag[e0 + i1] && !a.elem_flag[e0 + i2]) {
        const int c1 = d.line_image[d.track_line[e0 + i1]], c2 = d.line_image[d.track_line[e0 + i2]];
        ok = TriangulationAngle(a.centers + 3 * (size_t)c1, a.centers + 3 * (size_t)c2, X0, X1, X2) >= a.min_rad;
      }
    }
    keep = __ballot(ok) != 0;
  }
  if (lane == 0) {
    a.ndel[p] = ndel;
    if (keep) { a.verdict[p] = kFilterKept; a.error[p] = sum / (double)(len - ndel); }
    else a.verdict[p] = kFilterDeletedByAngle;      // :649-652
  }
}

__global__ __launch_bounds__(256) void k_track_depth(int64_t L, const int32_t* __restrict__ line_image, const int32_t* __restrict__ line_point,
                                                     const uint8_t* __restrict__ image_registered, const double* __restrict__ proj,
                                                     const double* __restrict__ points, uint8_t* __restrict__ flag) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= L) return;
  const int p = line_point[l], c = line_image[l];
  bool negative = false;
  if (p >= 0 && image_registered[c]) {
    const double* Pm = proj + 12 * (size_t)c;
    const double* X = points + 3 * (size_t)p;
    negative = !(Pm[8] * X[0] + Pm[9] * X[1] + Pm[10] * X[2] + Pm[11] >= DBL_EPSILON);      // HasPointPositiveDepth
  }
  flag[l] = negative ? 1 : 0;
}

}  // namespace ppsfm

using namespace ppsfm;

namespace {

// VALIDATION ORDER, pinned (tests/test_tracks_filter_capi_host.py passes a handle that is not one): every entry point checks its plain arguments - this
// function, then the options, the subsets, filtered_images - BEFORE the first read of *h; only image_order, which needs the handle's state, comes after.
int CheckFilterCall(pp_tracks_handle h, pp_tracks_filter_report* report, const int32_t* event_point, const int32_t* event_line, int64_t capacity, const char* where) {
  PP_REQUIRE(h && report && capacity >= 0 && (capacity == 0 || (event_point && event_line)), "%s: bad argument", where);
  return PP_OK;
}

struct EventSink {
  int32_t *point, *line;
  int64_t capacity, written = 0;
  void operator()(int p, int32_t l) {
    if (written < capacity) { point[written] = p; line[written] = l; }
    ++written;
  }
};

void FillReport(pp_tracks_filter_report* r, const FilterCounts& c, const EventSink& ev) {
  r->num_filtered = c.num_filtered; r->num_points_deleted = c.num_points_deleted; r->num_observations_deleted = c.num_observations_deleted;
  r->num_entries = ev.written; r->points_tested = c.points_tested; r->images_filtered = c.images_filtered;
}

}  // namespace

extern "C" {

int pp_tracks_filter_points(pp_tracks_handle h, const pp_filter_options* o, const uint8_t* line_aligned, const uint8_t* point_subset, const uint8_t* image_subset,
                            pp_tracks_filter_report* report, int32_t* event_point, int32_t* event_line, int64_t capacity, double* point_error) try {
  const char* where = "pp_tracks_filter_points";
  PP_TRY(CheckFilterCall(h, report, event_point, event_line, capacity, where));
  PP_REQUIRE(o && o->max_reproj_error >= 0 && o->min_tri_angle_deg >= 0, "%s: bad options", where);
  PP_REQUIRE(!(point_subset && image_subset), "%s: point_subset and image_subset are both given", where);
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  TrackState& st = h->st;
  const int P = st.NumPoints();
  if (P == 0) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  std::vector<int32_t> start, elems, ndel((size_t)P);
  std::vector<uint8_t> verdict((size_t)P), flags;
  std::vector<double> error((size_t)P);
  {
    PP_TRY(EnsureCenters(h));
    CallScratch cb(s);
    TrackDev d;
    PP_TRY(UploadState(h, cb, point_subset, start, elems, &d));
    const size_t T = elems.size();
    flags.resize(T);
    TrackFilterArgs a{};
    uint8_t *d_aligned = nullptr, *d_images = nullptr;
    if (line_aligned) PP_TRY(cb.Put(&d_aligned, line_aligned, (size_t)h->L));
    if (image_subset) PP_TRY(cb.Put(&d_images, image_subset, (size_t)h->C));
    a.aligned = d_aligned; a.image_subset = d_images; a.centers = h->d_centers;
    a.max2 = o->max_reproj_error * o->max_reproj_error;
    a.min_rad = o->min_tri_angle_deg * 3.14159265358979323846 / 180.0;
    PP_TRY(cb.Alloc(&a.verdict, (size_t)P)); PP_TRY(cb.Alloc(&a.ndel, (size_t)P)); PP_TRY(cb.Alloc(&a.error, (size_t)P)); PP_TRY(cb.Alloc(&a.elem_flag, T));
    PP_HIP_TRY(hipMemsetAsync(a.elem_flag, 0, std::max<size_t>(T, 1), s));
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_track_filter, dim3((unsigned)P), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    PP_TRY(Download(verdict.data(), a.verdict, (size_t)P, s)); PP_TRY(Download(ndel.data(), a.ndel, (size_t)P, s)); PP_TRY(Download(error.data(), a.error, (size_t)P, s));
    PP_TRY(Download(flags.data(), a.elem_flag, T, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    report->device_ms = ms;
  }
  for (int p = 0; p < P; ++p)
    if (verdict[(size_t)p] > kFilterDeletedByAngle || ndel[(size_t)p] < 0 || ndel[(size_t)p] > start[(size_t)p + 1] - start[(size_t)p]) {
      SetLastError("%s: the verdict of point %d is out of range", where, p);
      return PP_ERR_INTERNAL;
    }
  const auto t_replay = Clock::now();
  EventSink ev{event_point, event_line, capacity};
  const FilterCounts cnt = ApplyPointFilter(st, start.data(), verdict.data(), ndel.data(), error.data(), flags.data(), point_error, ev);
  FillReport(report, cnt, ev);
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_filter_points")

int pp_tracks_filter_negative_depth(pp_tracks_handle h, const int32_t* image_order, int32_t num_registered, pp_tracks_filter_report* report, int32_t* event_point,
                                    int32_t* event_line, int64_t capacity) try {
  const char* where = "pp_tracks_filter_negative_depth";
  PP_TRY(CheckFilterCall(h, report, event_point, event_line, capacity, where));
  TrackState& st = h->st;
  PP_REQUIRE(IsRegistrationOrder(st, image_order, num_registered), "%s: image_order is not the registered images, each once", where);
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  if (h->L == 0 || st.NumPoints() == 0) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  std::vector<uint8_t> flag((size_t)h->L);
  {
    CallScratch cb(s);
    double* d_points = nullptr;
    uint8_t* d_flag = nullptr;
    PP_TRY(Upload(h->d_line_point, st.line_point.data(), (size_t)h->L, s));
    PP_TRY(cb.Put(&d_points, st.points.data(), st.points.size()));
    PP_TRY(cb.Alloc(&d_flag, (size_t)h->L));
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_track_depth, dim3(CeilDiv(h->L, 256)), dim3(256), 0, s, h->L, h->dev.line_image, (const int32_t*)h->d_line_point, h->dev.image_registered,
                       h->dev.proj, (const double*)d_points, d_flag);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    PP_TRY(Download(flag.data(), d_flag, (size_t)h->L, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    report->device_ms = ms;
  }
  const auto t_replay = Clock::now();
  EventSink ev{event_point, event_line, capacity};
  const FilterCounts cnt = ReplayNegativeDepth(st, image_order, num_registered, flag.data(), ev);
  FillReport(report, cnt, ev);
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_filter_negative_depth")

int pp_tracks_filter_images(pp_tracks_handle h, const int32_t* image_order, int32_t num_registered, int32_t* filtered_images, pp_tracks_filter_report* report,
                            int32_t* event_point, int32_t* event_line, int64_t capacity) try {
  const char* where = "pp_tracks_filter_images";
  PP_TRY(CheckFilterCall(h, report, event_point, event_line, capacity, where));
  PP_REQUIRE(filtered_images, "%s: bad argument", where);
  TrackState& st = h->st;
  PP_REQUIRE(IsRegistrationOrder(st, image_order, num_registered), "%s: image_order is not the registered images, each once", where);
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  PP_HIP_TRY(hipSetDevice(h->device));
  EventSink ev{event_point, event_line, capacity};
  const FilterCounts cnt = ReplayFilterImages(st, h->image_skip.data(), image_order, num_registered, filtered_images, ev);
  FillReport(report, cnt, ev);
  report->replay_ms = MsSince(t_begin);
  if (cnt.images_filtered > 0) {
    // (an error from here on leaves the host state ahead of the device copy: as pp_tracks_complete's errors, destroy the handle)
    PP_TRY(Upload(h->d_registered, st.image_registered.data(), (size_t)h->C, h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_filter_images")

}  // extern "C"
