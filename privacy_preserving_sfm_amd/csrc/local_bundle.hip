// K12 - IncrementalMapper::FindLocalBundle on a pp_tracks_handle: the step that runs after every registered image.
//   FindLocalBundle                          reference src/sfm/incremental_mapper.cc:993-1160
//   CalculateTriangulationAngles             src/base/triangulation.cc:84-118 (TriAngle of tri_device.hpp, shared with K8 / K11b)
//   Percentile                               src/util/math.h:232-246          Image::ProjectionCenter   src/base/image.cc (-R^T t)
// As K10 / K11: the device does the data-parallel part, the host replays the sequential rest (local_bundle_replay.hpp: the sort, the eight
// relaxing thresholds, the lazy angle, the fill-up).
// K12a k_local_bundle_count    one wavefront per line of the query image that has a point, the lanes over the point's track: one integer atomic
//                             per element whose image is not the query image into count[C] (order-free), and the point's position into the
//                             compacted list (one entry per line: a point with two lines in the image is walked twice and appears twice, as in
//                             the reference's loops :1008-1017, :1106-1110).  The counts are NOT privatised in LDS: a workgroup is one wavefront
//                             with one track, so a private copy would be flushed after a handful of additions.
// K12b k_local_bundle_angles   one workgroup per candidate image: its threads share the N points (TriAngle against the two projection centres),
//                             the angles go to the workgroup's row of a scratch block as bit patterns; then a radix select over the 64-bit
//                             patterns, eight passes of eight bits with a 256-bin LDS histogram (integer atomics: exact whatever the schedule),
//                             finds the k-th smallest.  Angles are non-negative doubles, so their patterns order as unsigned integers; a NaN is
//                             stored as 0x7FF8000000000000, above every number (the pin of local_bundle_replay.hpp).  No cap on N.
//                             Candidates: the images whose count reaches the weakest overlap threshold (0.1 * NumPoints3D, the same double
//                             expression) - the sequential loop never asks for another.  The launch is skipped on the early return and for N = 0.
// No kernel here waits for another workgroup.
#include "local_bundle_replay.hpp"
#include "tracks_device.hpp"
#include "tri_device.hpp"

namespace ppsfm {

__global__ __launch_bounds__(64) void k_local_bundle_count(TrackDev d, int N, const int32_t* __restrict__ work_line, int query, int C,
                                                          int32_t* __restrict__ count, double* __restrict__ xyz) {
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= N) return;
  const int p = d.line_point[work_line[w]];
  if (p < 0 || p >= d.P) return;      // (the host lists lines that have a point)
  const int e0 = d.track_start[p], e1 = d.track_start[p + 1];
  for (int e = e0 + lane; e < e1; e += 64) {
    const int img = d.line_image[d.track_line[e]];
    if (img != query && img >= 0 && img < C) atomicAdd(&count[img], 1);
  }
  if (lane < 3) xyz[3 * (size_t)w + lane] = d.points[3 * (size_t)p + lane];
}

struct AngleArgs {
  int num_cand;
  const int32_t* cand;             // candidate images of this launch
  int query;
  const double* centers;           // C x 3
  const double* xyz;               // N x 3
  int N;
  unsigned k;                      // index of the percentile, < N
  unsigned long long* keys;        // num_cand x N scratch
  double* out;                     // num_cand
};

__global__ __launch_bounds__(256) void k_local_bundle_angles(AngleArgs a) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_k;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.num_cand) return;
  unsigned long long* keys = a.keys + (size_t)b * (size_t)a.N;
  const double* cq = a.centers + 3 * (size_t)a.query;
  const double* cc = a.centers + 3 * (size_t)a.cand[b];
  for (int i = tid; i < a.N; i += 256) {      // (a thread reads back only the entries it wrote)
    const double ang = TriAngle(cq, cc, a.xyz + 3 * (size_t)i);
    keys[i] = ang != ang ? 0x7FF8000000000000ull : (unsigned long long)__double_as_longlong(ang);
  }
  unsigned long long prefix = 0;
  unsigned k = a.k;
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = 8 * pass;
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < a.N; i += 256) {
      const unsigned long long key = keys[i];
      if (pass == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {      // 256 bins: the bin that holds rank k among the keys that share the prefix
      unsigned cum = 0;
      int bin = 0;
      for (; bin < 255; ++bin) {
        const unsigned c = s_hist[bin];
        if (k < cum + c) break;
        cum += c;
      }
      s_prefix = prefix | ((unsigned long long)bin << shift);
      s_k = k - cum;
    }
    __syncthreads();
    prefix = s_prefix;
    k = s_k;
  }
  if (tid == 0) a.out[b] = __longlong_as_double((long long)prefix);
}

}  // namespace ppsfm

using namespace ppsfm;

extern "C" {

void pp_local_bundle_options_default(pp_local_bundle_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->local_ba_num_images = 6; o->local_ba_min_tri_angle = 6.0;
}

int pp_tracks_find_local_bundle(pp_tracks_handle h, const pp_local_bundle_options* o, int32_t image, pp_local_bundle_report* report, int32_t* bundle,
                                int32_t bundle_capacity, int32_t* overlap_image, int32_t* overlap_count, double* overlap_tri_angle) try {
  const char* where = "pp_tracks_find_local_bundle";
  PP_REQUIRE(h && report && bundle_capacity >= 0 && (bundle_capacity == 0 || bundle), "%s: bad argument", where);
  PP_REQUIRE(image >= 0 && image < h->C, "%s: image %d of %d", where, image, h->C);
  PP_REQUIRE(o && o->local_ba_num_images >= 2 && o->local_ba_min_tri_angle >= 0, "%s: bad options", where);
  const TrackState& st = h->st;
  PP_REQUIRE(st.image_registered[(size_t)image], "%s: image %d is not registered", where, image);      // CHECK(image.IsRegistered()) (:998)
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  report->threshold_level = -1;
  std::vector<int32_t> work;      // the lines of the image that have a point, ascending
  for (int64_t l = 0; l < st.L; ++l) if (st.line_image[(size_t)l] == image && st.line_point[(size_t)l] >= 0) work.push_back((int32_t)l);
  const int N = (int)work.size();
  report->num_points3D = N;
  if (N == 0) { report->total_ms = MsSince(t_begin); return PP_OK; }      // nothing overlaps: the early return with an empty list
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int C = h->C;
  PP_TRY(EnsureCenters(h));
  float device_ms = 0.f;
  auto timed = [&]() -> int {
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    device_ms += ms;
    return PP_OK;
  };
  CallScratch cb(s);
  std::vector<int32_t> start, elems, count((size_t)C, 0);
  TrackDev d;
  PP_TRY(UploadState(h, cb, nullptr, start, elems, &d));
  int32_t *d_work = nullptr, *d_count = nullptr;
  double* d_xyz = nullptr;
  PP_TRY(cb.Put(&d_work, work.data(), (size_t)N)); PP_TRY(cb.Alloc(&d_count, (size_t)C)); PP_TRY(cb.Alloc(&d_xyz, 3 * (size_t)N));
  PP_HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)C * sizeof(int32_t), s));
  PP_HIP_TRY(hipEventRecord(h->ev0, s));
  hipLaunchKernelGGL(k_local_bundle_count, dim3((unsigned)N), dim3(64), 0, s, d, N, d_work, (int)image, C, d_count, d_xyz);
  PP_HIP_TRY(hipGetLastError());
  PP_HIP_TRY(hipEventRecord(h->ev1, s));
  PP_TRY(Download(count.data(), d_count, (size_t)C, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timed());
  // K12b for the images the sequential loop can ask for
  std::vector<int32_t> cand;
  std::vector<double> angle_of((size_t)C, -1.0);
  int64_t num_overlapping = 0;
  for (int c = 0; c < C; ++c) num_overlapping += count[(size_t)c] > 0;
  if (num_overlapping > (int64_t)o->local_ba_num_images - 1)
    for (int c = 0; c < C; ++c) if (count[(size_t)c] > 0 && LocalBundleCanBeAsked(count[(size_t)c], N)) cand.push_back(c);
  if (!cand.empty()) {
    const size_t batch = std::max<size_t>(1, std::min<size_t>(cand.size(), ((size_t)16 << 20) / (size_t)N));      // at most 128 MiB of patterns per launch
    AngleArgs a{};
    int32_t* d_cand = nullptr;
    PP_TRY(cb.Put(&d_cand, cand.data(), cand.size())); PP_TRY(cb.Alloc(&a.keys, batch * (size_t)N)); PP_TRY(cb.Alloc(&a.out, batch));
    a.query = image; a.centers = h->d_centers; a.xyz = d_xyz; a.N = N; a.k = (unsigned)LocalBundlePercentileIndex(N);
    std::vector<double> out(batch);
    for (size_t b0 = 0; b0 < cand.size(); b0 += batch) {
      const size_t nb = std::min(batch, cand.size() - b0);
      a.num_cand = (int)nb; a.cand = d_cand + b0;
      PP_HIP_TRY(hipEventRecord(h->ev0, s));
      hipLaunchKernelGGL(k_local_bundle_angles, dim3((unsigned)nb), dim3(256), 0, s, a);
      PP_HIP_TRY(hipGetLastError());
      PP_HIP_TRY(hipEventRecord(h->ev1, s));
      PP_TRY(Download(out.data(), a.out, nb, s));
      PP_HIP_TRY(hipStreamSynchronize(s));
      PP_TRY(timed());
      for (size_t i = 0; i < nb; ++i) angle_of[(size_t)cand[b0 + i]] = out[i];
    }
  }
  report->device_ms = device_ms;
  const auto t_replay = Clock::now();
  bool missing = false;
  const LocalBundleResult r = ReplayFindLocalBundle(count.data(), C, N, o->local_ba_num_images, o->local_ba_min_tri_angle, [&](int32_t c) {
    const double ang = angle_of[(size_t)c];
    if (ang < 0.0) missing = true;
    return ang;
  });
  if (missing) { SetLastError("%s: the replay asked for an angle the device did not compute", where); return PP_ERR_INTERNAL; }
  report->num_overlapping = (int32_t)r.overlap_image.size();
  report->num_selected = (int32_t)r.bundle.size();
  report->angles_computed = (int32_t)cand.size();
  report->angles_used = r.angles_used; report->threshold_level = r.threshold_level; report->filled = r.filled;
  for (size_t i = 0; i < r.bundle.size() && i < (size_t)bundle_capacity; ++i) bundle[i] = r.bundle[i];
  if (overlap_image) std::copy(r.overlap_image.begin(), r.overlap_image.end(), overlap_image);
  if (overlap_count) std::copy(r.overlap_count.begin(), r.overlap_count.end(), overlap_count);
  if (overlap_tri_angle) std::copy(r.overlap_tri_angle.begin(), r.overlap_tri_angle.end(), overlap_tri_angle);
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_find_local_bundle")

}  // extern "C"
