// Shared by tracks.hip (K10, pp_tracks_complete / pp_tracks_merge) and tracks_image.hip (K11, pp_tracks_triangulate_image / pp_tracks_complete_image):
// the device view of a pp_tracks_handle, K10a k_complete_tracks, the handle itself and the speculative completion of a set of points.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "line_error.hpp"
#include "device_handle.hpp"
#include "tracks_replay.hpp"

namespace ppsfm {

constexpr int kLdsList = 512;       // accepted lines of a point kept on chip (4 KiB of LDS per wavefront with their levels)
constexpr int kCandList = 256;      // candidate partner points of a point kept on chip

struct TrackDev {
  // static (uploaded at create)
  const double *proj, *intr, *lines;
  const int32_t *pose_camera, *camera_model, *cam_size, *line_image, *corr_start, *corr_line;
  const uint8_t *camera_skip, *image_registered;
  // state at the start of the call
  int P;
  const int32_t *line_point, *track_start, *track_line;
  const double* points;
  const uint8_t* subset;
};

__device__ __forceinline__ double TrackLineError(const TrackDev& d, double X0, double X1, double X2, int l) {
  const int c = d.line_image[l], k = d.pose_camera[c];
  const double* Pm = d.proj + 12 * (size_t)c;
  const double* ln = d.lines + 3 * (size_t)l;
  const double px = Pm[0] * X0 + Pm[1] * X1 + Pm[2] * X2 + Pm[3], py = Pm[4] * X0 + Pm[5] * X1 + Pm[6] * X2 + Pm[7];
  const double pz = Pm[8] * X0 + Pm[9] * X1 + Pm[10] * X2 + Pm[11];
  return SquaredPixelLineError(px, py, pz, ln[0], ln[1], ln[2], d.camera_model[k], d.intr + (size_t)kCamStride * k, d.cam_size + 2 * k);
}

// lanes whose key an earlier lane of `mask` also holds leave the mask: the first holder in lane order stays
__device__ __forceinline__ unsigned long long DropLaterDuplicates(unsigned long long mask, int key, int lane) {
  if (__popcll(mask) < 2) return mask;
  bool dup = false;
  for (unsigned long long m = mask; m; m &= m - 1) {
    const int k = __ffsll((long long)m) - 1;
    const int other = __shfl(key, k, 64);
    dup = dup || (k < lane && other == key);
  }
  return mask & ~__ballot(dup);
}

struct CompleteArgs {
  int num_work;                  // wavefronts: points (first launch) or entries of `work` (second launch)
  const int32_t* work;           // second launch: the flagged points
  int max_transitivity;
  double max2;
  int32_t *glist_line, *glist_level;      // second launch: num_work x gcap
  int64_t gcap;
  int32_t *pool_line, *pool_level;        // first launch: the points' segments
  unsigned long long pool_cap;
  unsigned long long* counters;           // [0] pool cursor, [1] line errors computed
  int64_t* out_start;                     // P: segment of the point (first launch) / unused
  int32_t* out_count;                     // P (first launch) or num_work (second launch)
  uint8_t* overflow;                      // P: 1 = finish this point in the second launch
};

template <bool kGlobal>
__global__ __launch_bounds__(64) void k_complete_tracks(TrackDev d, CompleteArgs a) {
  __shared__ int32_t s_line[kGlobal ? 1 : kLdsList], s_level[kGlobal ? 1 : kLdsList];
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= a.num_work) return;
  const int p = kGlobal ? a.work[w] : w;
  int32_t* list_line = kGlobal ? a.glist_line + (size_t)w * a.gcap : s_line;
  int32_t* list_level = kGlobal ? a.glist_level + (size_t)w * a.gcap : s_level;
  const int64_t cap = kGlobal ? a.gcap : kLdsList;
  const int e0 = d.track_start[p], e1 = d.track_start[p + 1];
  if (!kGlobal) {
    if (lane == 0) { a.out_count[p] = 0; a.out_start[p] = 0; a.overflow[p] = 0; }
    if (e1 == e0 || (d.subset && !d.subset[p])) return;
  }
  const double X0 = d.points[3 * (size_t)p], X1 = d.points[3 * (size_t)p + 1], X2 = d.points[3 * (size_t)p + 2];
  int n = 0, evals = 0;
  int lvl_begin = 0, lvl_end = 0;
  bool overflow = false;
  for (int t = 0; t < a.max_transitivity && !overflow; ++t) {
    const int nf = t == 0 ? e1 - e0 : lvl_end - lvl_begin;
    if (nf == 0) break;
    const int n_before = n;
    for (int f = 0; f < nf && !overflow; ++f) {
      const int fl = t == 0 ? d.track_line[e0 + f] : list_line[lvl_begin + f];
      const int c0 = d.corr_start[fl], c1 = d.corr_start[fl + 1];
      for (int base = c0; base < c1; base += 64) {
        const int i = base + lane;
        bool pass = false;
        int l = -1;
        if (i < c1) {
          l = d.corr_line[i];
          const int img = d.line_image[l];
          if (d.image_registered[img] && d.line_point[l] < 0 && !d.camera_skip[d.pose_camera[img]]) {
            bool seen = false;
            for (int j = 0; j < n; ++j) seen = seen || list_line[j] == l;      // (every lane reads the same entry: a broadcast)
            if (!seen) { ++evals; pass = !(TrackLineError(d, X0, X1, X2, l) > a.max2); }
          }
        }
        const unsigned long long m = DropLaterDuplicates(__ballot(pass), l, lane);
        const int cnt = __popcll(m);
        if (cnt == 0) continue;
        if ((int64_t)n + cnt > cap) { overflow = true; break; }
        if ((m >> lane) & 1) {
          const int pos = n + __popcll(m & ((1ull << lane) - 1));
          list_line[pos] = l; list_level[pos] = t;
        }
        n += cnt;
        __syncthreads();      // (one wavefront per workgroup, wave-uniform control flow: the appended entries become visible to every lane)
      }
    }
    lvl_begin = n_before; lvl_end = n;
    if (t >= a.max_transitivity - 1) break;      // what the last level adds is not queued again (:755)
  }
  evals = WaveSumInt(evals);
  if (kGlobal) {
    if (lane == 0) { a.out_count[w] = overflow ? -1 : n; atomicAdd(&a.counters[1], (unsigned long long)evals); }
    return;
  }
  unsigned long long off = 0;
  if (lane == 0) {
    atomicAdd(&a.counters[1], (unsigned long long)evals);
    if (!overflow && n > 0) {
      off = atomicAdd(&a.counters[0], (unsigned long long)n);      // the point's segment: one reservation per point, none per entry
      if (off + (unsigned long long)n > a.pool_cap) overflow = true;
    }
    a.overflow[p] = overflow ? 1 : 0;
    a.out_count[p] = overflow ? 0 : n;
    a.out_start[p] = (int64_t)off;
  }
  overflow = __shfl((int)overflow, 0, 64) != 0;
  off = ((unsigned long long)(unsigned)__shfl((int)(off >> 32), 0, 64) << 32) | (unsigned)__shfl((int)(off & 0xFFFFFFFFull), 0, 64);
  if (overflow) return;
  for (int j = lane; j < n; j += 64) { a.pool_line[off + j] = list_line[j]; a.pool_level[off + j] = list_level[j]; }
}

}  // namespace ppsfm

struct pp_tracks_impl : ppsfm::DeviceHandle {      // blocks: the static device arrays and the pinned slots (pool blocks)
  int C = 0, K = 0;
  int64_t L = 0, E = 0;
  ppsfm::TrackState st;
  std::vector<uint8_t> image_skip;      // per image: its camera is flagged in camera_skip
  std::vector<int32_t> pose_camera;     // C
  std::vector<double> poses, intr;      // C x 7, K x kCamStride: the host copies pp_tracks_update edits and uploads whole
  std::vector<uint8_t> camera_skip;     // K
  double *d_poses = nullptr, *d_proj = nullptr, *d_intr = nullptr;      // the writable views of dev.proj / dev.intr / dev.camera_skip
  uint8_t *d_skip = nullptr, *d_registered = nullptr;      // (d_registered: dev.image_registered, rewritten by pp_tracks_register_image)
  ppsfm::TrackDev dev{};
  int32_t* d_line_point = nullptr;
  double* d_centers = nullptr;    // C x 3 projection centres (K11b's triangulation-angle test, K12b)
  int32_t* pin = nullptr;         // pinned slots of the fresh-pair launches
  size_t pin_ints = 0;
};

namespace ppsfm {

// the C x 3 projection centres of the handle's projection matrices (tracks_image.hip): computed on first use, again after pp_tracks_update
int ComputeCenters(pp_tracks_impl* h);
inline int EnsureCenters(pp_tracks_impl* h) { return h->d_centers ? PP_OK : ComputeCenters(h); }

// h->poses to the device, the projection matrices and (once computed) the projection centres again (tracks.hip); the caller drains the stream
int UploadPoses(pp_tracks_impl* h);

// uploads the state at the start of a call; flat track CSR in start / elems (kept alive by the caller until the stream drains)
inline int UploadState(pp_tracks_impl* h, CallScratch& cb, const uint8_t* subset, std::vector<int32_t>& start, std::vector<int32_t>& elems, TrackDev* d) {
  const TrackState& st = h->st;
  const int P = st.NumPoints();
  start.assign((size_t)P + 1, 0);
  size_t T = 0;
  for (int p = 0; p < P; ++p) { T += st.tracks[(size_t)p].size(); PP_REQUIRE(T < 0x7FFFFFFFull, "pp_tracks: too many track elements"); start[(size_t)p + 1] = (int32_t)T; }
  elems.resize(T);
  for (int p = 0; p < P; ++p) std::copy(st.tracks[(size_t)p].begin(), st.tracks[(size_t)p].end(), elems.begin() + start[(size_t)p]);
  *d = h->dev;
  d->P = P;
  PP_TRY(Upload(h->d_line_point, st.line_point.data(), (size_t)h->L, h->stream));
  d->line_point = h->d_line_point;
  int32_t *d_start = nullptr, *d_elems = nullptr;
  double* d_points = nullptr;
  uint8_t* d_subset = nullptr;
  PP_TRY(cb.Put(&d_start, start.data(), start.size()));
  PP_TRY(cb.Put(&d_elems, elems.data(), elems.size()));
  PP_TRY(cb.Put(&d_points, st.points.data(), st.points.size()));
  if (subset) PP_TRY(cb.Put(&d_subset, subset, (size_t)P));
  d->track_start = d_start; d->track_line = d_elems; d->points = d_points; d->subset = d_subset;
  return PP_OK;
}

// K10a over the points of `subset` (nullptr = all) on the handle's current state: the first launch with the lists on chip, the second for the points it flagged
struct CompleteSpec {
  std::vector<int32_t> start, elems, pool_line, count, second_of;
  std::vector<int64_t> seg;
  std::vector<uint8_t> over;
  std::vector<std::vector<int32_t>> second;      // lists of the points the second launch finished
  unsigned long long counters[2] = {0, 0};
  float device_ms = 0.f;
  int32_t overflow_points = 0, second_launches = 0;
  SpecList List(int p) const {
    const int32_t k = second_of[(size_t)p];
    if (k >= 0) return SpecList{second[(size_t)k].data(), (int64_t)second[(size_t)k].size()};
    return SpecList{pool_line.data() + seg[(size_t)p], (int64_t)count[(size_t)p]};
  }
};

inline int SpeculateComplete(pp_tracks_impl* h, const uint8_t* point_subset, int max_transitivity, double max2, const char* where, CompleteSpec* out) {
  hipStream_t s = h->stream;
  TrackState& st = h->st;
  const int P = st.NumPoints();
  std::vector<int32_t>&start = out->start, &elems = out->elems, &pool_line = out->pool_line, &count = out->count, &second_of = out->second_of;
  std::vector<int64_t>& seg = out->seg;
  std::vector<uint8_t>& over = out->over;
  std::vector<std::vector<int32_t>>& second = out->second;
  unsigned long long* counters = out->counters;
  count.assign((size_t)P, 0); seg.assign((size_t)P, 0); over.assign((size_t)P, 0); second_of.assign((size_t)P, -1);
  float ms_total = 0.f;
  {
    CallScratch cb(s);
    TrackDev d;
    PP_TRY(UploadState(h, cb, point_subset, start, elems, &d));
    CompleteArgs a{};
    a.num_work = P; a.max_transitivity = max_transitivity; a.max2 = max2;
    a.pool_cap = (unsigned long long)(2 * h->E + 1024);
    PP_TRY(cb.Alloc(&a.pool_line, (size_t)a.pool_cap)); PP_TRY(cb.Alloc(&a.pool_level, (size_t)a.pool_cap)); PP_TRY(cb.Alloc(&a.counters, 2));
    PP_TRY(cb.Alloc(&a.out_start, (size_t)P)); PP_TRY(cb.Alloc(&a.out_count, (size_t)P)); PP_TRY(cb.Alloc(&a.overflow, (size_t)P));
    PP_HIP_TRY(hipMemsetAsync(a.counters, 0, 2 * sizeof(unsigned long long), s));
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_complete_tracks<false>, dim3(P), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    PP_TRY(Download(count.data(), a.out_count, (size_t)P, s)); PP_TRY(Download(seg.data(), a.out_start, (size_t)P, s)); PP_TRY(Download(over.data(), a.overflow, (size_t)P, s));
    PP_TRY(Download(counters, a.counters, 2, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ms_total += ms;
    const size_t used = (size_t)std::min<unsigned long long>(counters[0], a.pool_cap);
    pool_line.resize(used);
    PP_TRY(Download(pool_line.data(), a.pool_line, used, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    // the flagged points: a list in global memory that cannot overflow (a closure holds free lines only, each once)
    std::vector<int32_t> work;
    for (int p = 0; p < P; ++p) if (over[(size_t)p]) work.push_back(p);
    if (!work.empty()) {
      int64_t gcap = 0;
      for (int64_t l = 0; l < h->L; ++l) gcap += st.line_point[(size_t)l] < 0;
      gcap = std::max<int64_t>(gcap, 1);
      const size_t batch = (size_t)std::max<int64_t>(1, std::min<int64_t>((int64_t)work.size(), (int64_t)(32 << 20) / gcap));
      int32_t *d_work = nullptr, *d_cnt = nullptr;
      PP_TRY(cb.Alloc(&a.glist_line, batch * (size_t)gcap)); PP_TRY(cb.Alloc(&a.glist_level, batch * (size_t)gcap));
      PP_TRY(cb.Alloc(&d_work, batch)); PP_TRY(cb.Alloc(&d_cnt, batch));
      a.gcap = gcap;
      std::vector<int32_t> cnt2(batch), rows;
      for (size_t b0 = 0; b0 < work.size(); b0 += batch) {
        const size_t nb = std::min(batch, work.size() - b0);
        PP_TRY(Upload(d_work, work.data() + b0, nb, s));
        a.num_work = (int)nb; a.work = d_work; a.out_count = d_cnt;
        PP_HIP_TRY(hipEventRecord(h->ev0, s));
        hipLaunchKernelGGL(k_complete_tracks<true>, dim3((unsigned)nb), dim3(64), 0, s, d, a);
        PP_HIP_TRY(hipGetLastError());
        PP_HIP_TRY(hipEventRecord(h->ev1, s));
        PP_TRY(Download(cnt2.data(), d_cnt, nb, s));
        PP_HIP_TRY(hipStreamSynchronize(s));
        PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        ms_total += ms;
        ++out->second_launches;
        for (size_t i = 0; i < nb; ++i) {
          if (cnt2[i] < 0 || cnt2[i] > gcap) { SetLastError("%s: the closure of point %d outgrew every free line", where, work[b0 + i]); return PP_ERR_INTERNAL; }
          rows.resize((size_t)cnt2[i]);
          PP_TRY(Download(rows.data(), a.glist_line + i * (size_t)gcap, (size_t)cnt2[i], s));
          PP_HIP_TRY(hipStreamSynchronize(s));
          second_of[(size_t)work[b0 + i]] = (int32_t)second.size();
          second.push_back(rows);
        }
      }
      PP_TRY(Download(counters, a.counters, 2, s));
      PP_HIP_TRY(hipStreamSynchronize(s));
      out->overflow_points = (int32_t)work.size();
    }
  }
  out->device_ms = ms_total;
  return PP_OK;
}

}  // namespace ppsfm
