// K11 - IncrementalTriangulator::TriangulateImage / CompleteImage on a pp_tracks_handle: the two places where the reference creates 3D points.
//   TriangulateImage   reference src/sfm/incremental_triangulator.cc:63-121     CompleteImage :123-235
//   Find :426-466      Continue :563-604      Create :468-561
//   CorrespondenceGraph::FindTransitiveCorrespondences / IsTwoViewObservation   src/base/correspondence_graph.cc:166-224, 252-263
//   CalculateNormalizedLineAngularError                                         src/base/projection.cc:241-260
// As K10: the device SPECULATES over all lines of the image on the state at the start of the call, the host replays the sequential decisions in
// ascending line order (tracks_image_replay.hpp) and has a line whose inputs changed evaluated again on the current state.
// K11a k_image_find       one wavefront per reference line: the transitive closure in the reference's order (level-synchronous, a line collected on
//                        first sight, the query overwritten by the last element), filtered to registered images with sound cameras; the Continue
//                        candidate (the lanes over the triangulated neighbours, then a lexicographic (angle, index) minimum over the wavefront); the
//                        create set (the free neighbours, then the reference line if it stays free).  The list lives in LDS (kFindList entries); a
//                        closure that outgrows it flags its line, which the <true> instantiation finishes in global memory sized by the host.
// K11b k_image_triangulate one lane per create set: the LORANSAC of tri_device.hpp, and Create's recursion in place - after a success the inliers
//                        leave the set and the RANSAC runs again while at least three observations remain.
// CompleteImage's lines that already have a point go through K10a (tracks_device.hpp) on exactly those points.
// No kernel here waits for another workgroup; the only atomic reserves a line's output segment (one per line).
#include <climits>

#include "ransac_host.hpp"
#include "tracks_device.hpp"
#include "tracks_image_replay.hpp"
#include "tri_device.hpp"

namespace ppsfm {

constexpr int kFindList = 1024;      // closure of a line kept on chip (4 KiB of LDS per wavefront)

__global__ __launch_bounds__(256) void k_image_centers(int C, const double* __restrict__ proj, double* __restrict__ centers) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double* P = proj + 12 * (size_t)c;      // Image::ProjectionCenter: -R^T t
#pragma unroll
  for (int i = 0; i < 3; ++i) centers[3 * (size_t)c + i] = -(P[i] * P[3] + P[4 + i] * P[7] + P[8 + i] * P[11]);
}

int ComputeCenters(pp_tracks_impl* h) {
  if (!h->d_centers) PP_TRY(h->blocks.Alloc(&h->d_centers, std::max<size_t>((size_t)3 * h->C, 1)));
  hipLaunchKernelGGL(k_image_centers, dim3(CeilDiv(h->C, 256)), dim3(256), 0, h->stream, h->C, h->dev.proj, h->d_centers);
  PP_HIP_TRY(hipGetLastError());
  return PP_OK;
}

struct FindArgs {
  int num_work;
  const int32_t* work_line;      // the reference lines
  int transitivity;
  double continue_max;           // radians, un-squared
  int32_t *glist, *gset;         // <true>: num_work x gcap each
  int64_t gcap;
  int32_t *pool_list, *pool_set; // <false>: a line's segment holds its list and, at the same offset, its create set (at most one entry longer)
  unsigned long long pool_cap;
  unsigned long long* cursor;
  int64_t* out_start;            // all num_work long
  int32_t *out_count, *out_set_count, *out_num_tri, *out_cont_point;
  uint8_t* overflow;
};

template <bool kGlobal>
__global__ __launch_bounds__(64) void k_image_find(TrackDev d, FindArgs a) {
  __shared__ int32_t s_list[kGlobal ? 1 : kFindList];
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= a.num_work) return;
  const int ref = a.work_line[w];
  int32_t* list = kGlobal ? a.glist + (size_t)w * a.gcap : s_list;
  const int64_t cap = kGlobal ? a.gcap : kFindList;
  const unsigned long long below = (1ull << lane) - 1;
  int n = 0;
  bool overflow = false;
  const int r0 = d.corr_start[ref], r1 = d.corr_start[ref + 1];
  if (a.transitivity == 1) {      // the direct list as it is (:169-171)
    if (r1 - r0 > cap) overflow = true;
    else {
      n = r1 - r0;
      for (int i = lane; i < n; i += 64) list[i] = d.corr_line[r0 + i];
      __syncthreads();
    }
  } else if (r1 > r0) {
    if (lane == 0) list[0] = ref;
    n = 1;
    __syncthreads();
    int qb = 0, qe = 1;
    for (int t = 0; t < a.transitivity && !overflow; ++t) {
      for (int f = qb; f < qe && !overflow; ++f) {
        const int fl = list[f];
        const int c0 = d.corr_start[fl], c1 = d.corr_start[fl + 1];
        for (int base = c0; base < c1; base += 64) {
          const int i = base + lane;
          bool fresh = false;
          int l = -1;
          if (i < c1) {
            l = d.corr_line[i];
            bool seen = false;
            for (int j = 0; j < n; ++j) seen = seen || list[j] == l;      // (every lane reads the same entry: a broadcast)
            fresh = !seen;
          }
          const unsigned long long m = DropLaterDuplicates(__ballot(fresh), l, lane);
          const int cnt = __popcll(m);
          if (cnt == 0) continue;
          if ((int64_t)n + cnt > cap) { overflow = true; break; }
          if ((m >> lane) & 1) list[n + __popcll(m & below)] = l;
          n += cnt;
          __syncthreads();      // (one wavefront per workgroup, wave-uniform control flow: the appended entries become visible to every lane)
        }
      }
      qb = qe; qe = n;
      if (qb == qe) break;
    }
    if (!overflow) {            // the query leaves: the LAST element takes its place (:216-221)
      const int last = list[n - 1];
      __syncthreads();
      if (n > 1 && lane == 0) list[0] = last;
      --n;
      __syncthreads();
    }
  }
  // Find's filter (:440-449), in place; the triangulated neighbours counted
  int kept = 0, ntri = 0;
  if (!overflow) {
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      int l = -1;
      bool keep = false;
      if (i < n) {
        l = list[i];
        const int img = d.line_image[l];
        keep = d.image_registered[img] && !d.camera_skip[d.pose_camera[img]];
      }
      __syncthreads();
      const unsigned long long m = __ballot(keep);
      if (keep) {
        list[kept + __popcll(m & below)] = l;      // (at or before position i: no entry of a later chunk is overwritten)
        if (d.line_point[l] >= 0) ++ntri;
      }
      kept += __popcll(m);
      __syncthreads();
    }
    ntri = WaveSumInt(ntri);
    n = kept;
  }
  // Continue (:563-604): the first strictly smallest angular error of the reference line against the points of the triangulated neighbours
  const bool ref_free = d.line_point[ref] < 0;
  int cont_point = -1;
  if (!overflow && ref_free && ntri > 0) {
    const int c = d.line_image[ref], k = d.pose_camera[c];
    const double* Pm = d.proj + 12 * (size_t)c;
    const double* ln = d.lines + 3 * (size_t)ref;
    const double* cam = d.intr + (size_t)kCamStride * k;
    const int model = d.camera_model[k];
    const double cw = (double)d.cam_size[2 * k], ch = (double)d.cam_size[2 * k + 1];
    double best = DBL_MAX;
    int best_i = INT_MAX;
    for (int i = lane; i < n; i += 64) {
      const int q = d.line_point[list[i]];
      if (q < 0) continue;
      const double* X = d.points + 3 * (size_t)q;
      const double p0 = Pm[0] * X[0] + Pm[1] * X[1] + Pm[2] * X[2] + Pm[3], p1 = Pm[4] * X[0] + Pm[5] * X[1] + Pm[6] * X[2] + Pm[7];
      const double p2 = Pm[8] * X[0] + Pm[9] * X[1] + Pm[10] * X[2] + Pm[11];
      double ang;
      if (LineAngularError(model, cam, cw, ch, ln, p0, p1, p2, &ang) && ang < best) { best = ang; best_i = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(best_i, off, 64);
      if (ob < best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
    }
    if (best_i != INT_MAX && best <= a.continue_max) cont_point = d.line_point[list[best_i]];
  }
  unsigned long long off = 0;
  if (!kGlobal) {
    if (lane == 0 && !overflow) {
      off = atomicAdd(a.cursor, (unsigned long long)n + 1);      // the line's segment: one reservation per line
      if (off + (unsigned long long)n + 1 > a.pool_cap) overflow = true;
    }
    overflow = __shfl((int)overflow, 0, 64) != 0;
    off = ((unsigned long long)(unsigned)__shfl((int)(off >> 32), 0, 64) << 32) | (unsigned)__shfl((int)(off & 0xFFFFFFFFull), 0, 64);
  }
  if (overflow) {
    if (lane == 0) { a.overflow[w] = 1; a.out_start[w] = 0; a.out_count[w] = kGlobal ? -1 : 0; a.out_set_count[w] = 0; a.out_num_tri[w] = 0; a.out_cont_point[w] = -1; }
    return;
  }
  int32_t* out_set = kGlobal ? a.gset + (size_t)w * a.gcap : a.pool_set + off;
  if (!kGlobal) for (int j = lane; j < n; j += 64) a.pool_list[off + j] = list[j];
  // the create set: what Create keeps of corrs_data (:473-477) - the free neighbours, then the reference line unless it has or has just got a point
  int ns = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int l = -1;
    bool is_free = false;
    if (i < n) { l = list[i]; is_free = d.line_point[l] < 0; }
    const unsigned long long m = __ballot(is_free);
    if (is_free) out_set[ns + __popcll(m & below)] = l;
    ns += __popcll(m);
  }
  if (lane == 0) {
    if (n > 0 && ref_free && cont_point < 0) { out_set[ns] = ref; ++ns; }
    a.overflow[w] = 0; a.out_start[w] = (int64_t)off; a.out_count[w] = n; a.out_set_count[w] = ns; a.out_num_tri[w] = ntri; a.out_cont_point[w] = cont_point;
  }
}

struct LineObs {      // observation i of a create set: a line of the handle
  const int32_t* set;
  const int32_t* line_image;
  const double* lines;
  __device__ __forceinline__ int view(int i) const { return line_image[set[i]]; }
  __device__ __forceinline__ const double* line(int i) const { return lines + 3 * (size_t)set[i]; }
};

struct ImageTriArgs {
  int S;
  const int32_t* set_start;                // S + 1
  int32_t *work_line, *work_pos;           // N: the sets (compacted in place as inliers leave) and each entry's position in its original set
  const unsigned long long* min_trials;    // S: min_num_trials of the first RANSAC
  const uint8_t* aligned;                  // L or nullptr
  int recurse;                             // 1 Create (aligned rule, recursion), 0 CompleteImage
  TriModel m;
  uint8_t* flags;                          // N scratch
  int32_t* round_of;                       // N: 0, or k for an inlier of the k-th point of its set
  double* xyz;                             // 3 N: point k of set s at 3 (set_start[s] + k - 1)
  int32_t* num_rounds;                     // S
  unsigned long long* trials;              // S, summed over the rounds
};

__global__ __launch_bounds__(64) void k_image_triangulate(TrackDev d, ImageTriArgs a) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.S) return;
  const int e0 = a.set_start[s], n = a.set_start[s + 1] - e0;
  for (int i = 0; i < n; ++i) { a.work_pos[e0 + i] = i; a.round_of[e0 + i] = 0; }
  const LineObs obs{a.work_line + e0, d.line_image, d.lines};
  int cur = n, round = 0;
  unsigned long long total = 0, min_trials = a.min_trials[s];
  while (cur >= 3) {                                                   // :480
    if (a.recurse) {                                                   // no point from aligned lines alone (:511-514)
      bool random_line = a.aligned == nullptr;
      for (int i = 0; i < cur && !random_line; ++i) random_line = !a.aligned[a.work_line[e0 + i]];
      if (!random_line) break;
    }
    double best[3];
    unsigned long long trials;
    const bool ok = TriRansac(a.m, obs, cur, min_trials, a.flags + e0, best, &trials);
    total += trials;
    if (!ok) break;
    ++round;                                                           // (at most n / 3 rounds: every point takes at least three observations)
    double* X = a.xyz + 3 * (size_t)(e0 + round - 1);
    X[0] = best[0]; X[1] = best[1]; X[2] = best[2];
    int k = 0;
    for (int i = 0; i < cur; ++i) {
      if (a.flags[e0 + i]) a.round_of[e0 + a.work_pos[e0 + i]] = round;
      else { a.work_line[e0 + k] = a.work_line[e0 + i]; a.work_pos[e0 + k] = a.work_pos[e0 + i]; ++k; }
    }
    cur = k;
    if (!a.recurse) break;
    min_trials = cur <= 15 ? (unsigned long long)cur * (cur - 1) * (cur - 2) / 6 : 0;      // Create's fresh options (:527-531)
  }
  a.num_rounds[s] = round;
  a.trials[s] = total;
}

}  // namespace ppsfm

using namespace ppsfm;

namespace {

#define PP_REQUIRE_INTERNAL(cond, ...) do { if (!(cond)) { ::ppsfm::SetLastError(__VA_ARGS__); return PP_ERR_INTERNAL; } } while (0)

constexpr double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;

struct ImageCall {
  pp_tracks_impl* h;
  const pp_tracks_image_options* o;
  const uint8_t* aligned;
  bool create;                 // TriangulateImage (Create) / CompleteImage
  hipStream_t s;
  CallScratch cb;               // blocks that live for the whole call
  TrackDev d{};
  double* d_points = nullptr;
  uint8_t* d_aligned = nullptr;
  size_t points_cap = 0, points_up = 0;      // in points
  float device_ms = 0.f;
  int32_t launches = 0;

  ImageCall(pp_tracks_impl* handle, const pp_tracks_image_options* opt, const uint8_t* line_aligned, bool is_create)
      : h(handle), o(opt), aligned(line_aligned), create(is_create), s(handle->stream), cb(handle->stream) {}

  int Begin() {
    const TrackState& st = h->st;
    PP_TRY(EnsureCenters(h));
    points_cap = (size_t)st.NumPoints() + (size_t)h->L / 3 + 1;      // every new point takes at least three free lines
    PP_TRY(cb.Alloc(&d_points, 3 * points_cap));
    if (aligned) PP_TRY(cb.Put(&d_aligned, aligned, (size_t)h->L));
    d = h->dev;
    d.P = st.NumPoints();
    d.line_point = h->d_line_point;
    d.points = d_points;
    return Sync();
  }
  // the current line_point and the points created since the last upload
  int Sync() {
    const TrackState& st = h->st;
    const size_t P = (size_t)st.NumPoints();
    PP_REQUIRE(P <= points_cap, "pp_tracks: more new points than free lines allow");
    PP_TRY(Upload(h->d_line_point, st.line_point.data(), (size_t)h->L, s));
    if (P > points_up) PP_TRY(Upload(d_points + 3 * points_up, st.points.data() + 3 * points_up, 3 * (P - points_up), s));
    points_up = P;
    d.P = (int)P;
    return PP_OK;
  }
  int Timed(float* acc) {
    if (!acc) return PP_OK;
    float ms = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *acc += ms;
    return PP_OK;
  }

  // K11a for the lines of `work` on the uploaded state
  int Find(const std::vector<int32_t>& work, int transitivity, std::vector<ImageLineResult>& out, float* ms_acc) {
    const TrackState& st = h->st;
    const size_t W = work.size();
    out.assign(W, ImageLineResult());
    if (W == 0) return PP_OK;
    CallScratch lb(s);
    int64_t direct = 0, maxc = 0;
    for (const int32_t l : work) { const int64_t c = st.corr_start[(size_t)l + 1] - st.corr_start[(size_t)l]; direct += c + 1; maxc = std::max(maxc, c); }
    FindArgs a{};
    a.num_work = (int)W; a.transitivity = transitivity; a.continue_max = kDegToRad * o->continue_max_angle_error;
    a.pool_cap = (unsigned long long)(transitivity == 1 ? direct : direct + 2 * h->E + 1024);      // exact for the direct lists; a closure that finds the pool full goes to the second launch
    int32_t* d_work = nullptr;
    PP_TRY(lb.Put(&d_work, work.data(), W));
    a.work_line = d_work;
    PP_TRY(lb.Alloc(&a.pool_list, (size_t)a.pool_cap)); PP_TRY(lb.Alloc(&a.pool_set, (size_t)a.pool_cap)); PP_TRY(lb.Alloc(&a.cursor, 1));
    PP_TRY(lb.Alloc(&a.out_start, W)); PP_TRY(lb.Alloc(&a.out_count, W)); PP_TRY(lb.Alloc(&a.out_set_count, W)); PP_TRY(lb.Alloc(&a.out_num_tri, W));
    PP_TRY(lb.Alloc(&a.out_cont_point, W)); PP_TRY(lb.Alloc(&a.overflow, W));
    PP_HIP_TRY(hipMemsetAsync(a.cursor, 0, sizeof(unsigned long long), s));
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_image_find<false>, dim3((unsigned)W), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    ++launches;
    std::vector<int64_t> seg(W);
    std::vector<int32_t> count(W), set_count(W), num_tri(W), cont(W), pool_list, pool_set;
    std::vector<uint8_t> over(W);
    unsigned long long cursor = 0;
    auto fetch = [&](size_t nw) {
      PP_TRY(Download(seg.data(), a.out_start, nw, s)); PP_TRY(Download(count.data(), a.out_count, nw, s)); PP_TRY(Download(set_count.data(), a.out_set_count, nw, s));
      PP_TRY(Download(num_tri.data(), a.out_num_tri, nw, s)); PP_TRY(Download(cont.data(), a.out_cont_point, nw, s)); PP_TRY(Download(over.data(), a.overflow, nw, s));
      return PP_OK;
    };
    PP_TRY(fetch(W));
    PP_TRY(Download(&cursor, a.cursor, 1, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    PP_TRY(Timed(ms_acc));
    const size_t used = (size_t)std::min<unsigned long long>(cursor, a.pool_cap);
    pool_list.resize(used); pool_set.resize(used);
    PP_TRY(Download(pool_list.data(), a.pool_list, used, s)); PP_TRY(Download(pool_set.data(), a.pool_set, used, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> again;
    for (size_t w = 0; w < W; ++w) {
      if (over[w]) { again.push_back((int32_t)w); continue; }
      PP_REQUIRE_INTERNAL(seg[w] >= 0 && (size_t)seg[w] + (size_t)count[w] + 1 <= used && set_count[w] <= count[w] + 1, "pp_tracks: a find segment is out of range");
      ImageLineResult& r = out[w];
      r.list.assign(pool_list.begin() + seg[w], pool_list.begin() + seg[w] + count[w]);
      r.set.assign(pool_set.begin() + seg[w], pool_set.begin() + seg[w] + set_count[w]);
      r.num_triangulated = num_tri[w]; r.continue_point = cont[w];
    }
    if (again.empty()) return PP_OK;
    // the flagged lines: lists in global memory that cannot overflow (a closure holds every line at most once, a direct list is as long as its row)
    const int64_t gcap = std::max<int64_t>(h->L, maxc) + 1;
    const size_t batch = (size_t)std::max<int64_t>(1, std::min<int64_t>((int64_t)again.size(), (int64_t)(32 << 20) / gcap));
    PP_TRY(lb.Alloc(&a.glist, batch * (size_t)gcap)); PP_TRY(lb.Alloc(&a.gset, batch * (size_t)gcap));
    int32_t* d_work2 = nullptr;
    PP_TRY(lb.Alloc(&d_work2, batch));
    a.gcap = gcap; a.work_line = d_work2;
    std::vector<int32_t> lines2(batch);
    for (size_t b0 = 0; b0 < again.size(); b0 += batch) {
      const size_t nb = std::min(batch, again.size() - b0);
      for (size_t i = 0; i < nb; ++i) lines2[i] = work[(size_t)again[b0 + i]];
      PP_TRY(Upload(d_work2, lines2.data(), nb, s));
      a.num_work = (int)nb;
      PP_HIP_TRY(hipEventRecord(h->ev0, s));
      hipLaunchKernelGGL(k_image_find<true>, dim3((unsigned)nb), dim3(64), 0, s, d, a);
      PP_HIP_TRY(hipGetLastError());
      PP_HIP_TRY(hipEventRecord(h->ev1, s));
      ++launches;
      PP_TRY(fetch(nb));
      PP_HIP_TRY(hipStreamSynchronize(s));
      PP_TRY(Timed(ms_acc));
      for (size_t i = 0; i < nb; ++i) {
        PP_REQUIRE_INTERNAL(count[i] >= 0 && count[i] < gcap && set_count[i] <= count[i] + 1, "pp_tracks: the closure of a line outgrew every line");
        ImageLineResult& r = out[(size_t)again[b0 + i]];
        r.list.resize((size_t)count[i]); r.set.resize((size_t)set_count[i]);
        PP_TRY(Download(r.list.data(), a.glist + i * (size_t)gcap, r.list.size(), s)); PP_TRY(Download(r.set.data(), a.gset + i * (size_t)gcap, r.set.size(), s));
        PP_HIP_TRY(hipStreamSynchronize(s));
        r.num_triangulated = num_tri[i]; r.continue_point = cont[i];
      }
    }
    return PP_OK;
  }

  // K11b over the sets of `items` (each with its min_trials set)
  int Triangulate(const std::vector<ImageLineResult*>& items, float* ms_acc) {
    const size_t S = items.size();
    if (S == 0) return PP_OK;
    CallScratch lb(s);
    std::vector<int32_t> start(S + 1, 0), flat;
    std::vector<unsigned long long> mt(S);
    for (size_t i = 0; i < S; ++i) {
      flat.insert(flat.end(), items[i]->set.begin(), items[i]->set.end());
      PP_REQUIRE(flat.size() < 0x7FFFFFFFull, "pp_tracks: too many observations in the create sets");
      start[i + 1] = (int32_t)flat.size();
      mt[i] = items[i]->min_trials;
    }
    const size_t N = flat.size();
    ImageTriArgs a{};
    a.S = (int)S; a.aligned = d_aligned; a.recurse = create ? 1 : 0;
    int32_t* d_start = nullptr;
    unsigned long long* d_mt = nullptr;
    PP_TRY(lb.Put(&d_start, start.data(), S + 1)); PP_TRY(lb.Put(&a.work_line, flat.data(), N)); PP_TRY(lb.Put(&d_mt, mt.data(), S));
    a.set_start = d_start; a.min_trials = d_mt;
    PP_TRY(lb.Alloc(&a.work_pos, N)); PP_TRY(lb.Alloc(&a.flags, N)); PP_TRY(lb.Alloc(&a.round_of, N)); PP_TRY(lb.Alloc(&a.xyz, 3 * N)); PP_TRY(lb.Alloc(&a.num_rounds, S)); PP_TRY(lb.Alloc(&a.trials, S));
    a.m.view_camera = d.pose_camera; a.m.camera_model = d.camera_model; a.m.cam_size = d.cam_size; a.m.P = d.proj; a.m.centers = h->d_centers; a.m.intr = d.intr;
    a.m.min_tri_angle = kDegToRad * o->min_angle;
    const double max_error = create ? kDegToRad * o->create_max_angle_error : o->complete_max_reproj_error;
    a.m.max_residual = max_error * max_error;
    a.m.confidence = 0.9999; a.m.multiplier = 3.0;
    a.m.residual_type = create ? 0 : 1;
    a.m.max_num_trials = std::min<uint64_t>(10000, ComputeNumTrials((uint64_t)(0.02 * 100000), 100000, 0.9999, 3.0, 3));      // RANSAC ctor (optim/ransac.h:149-155)
    PP_HIP_TRY(hipEventRecord(h->ev0, s));
    hipLaunchKernelGGL(k_image_triangulate, dim3(CeilDiv((int64_t)S, 64)), dim3(64), 0, s, d, a);
    PP_HIP_TRY(hipGetLastError());
    PP_HIP_TRY(hipEventRecord(h->ev1, s));
    ++launches;
    std::vector<int32_t> round_of(N), rounds(S);
    std::vector<double> xyz(3 * N);
    std::vector<unsigned long long> trials(S);
    PP_TRY(Download(round_of.data(), a.round_of, N, s)); PP_TRY(Download(xyz.data(), a.xyz, 3 * N, s)); PP_TRY(Download(rounds.data(), a.num_rounds, S, s));
    PP_TRY(Download(trials.data(), a.trials, S, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    PP_TRY(Timed(ms_acc));
    for (size_t i = 0; i < S; ++i) {
      ImageLineResult& r = *items[i];
      const size_t e0 = (size_t)start[i], n = r.set.size();
      PP_REQUIRE_INTERNAL(rounds[i] >= 0 && (size_t)rounds[i] * 3 <= n, "pp_tracks: more points than a create set can give");
      r.round_of.assign(round_of.begin() + e0, round_of.begin() + e0 + n);
      r.xyz.assign(xyz.begin() + 3 * e0, xyz.begin() + 3 * (e0 + (size_t)rounds[i]));
      r.trials = (int64_t)trials[i];
    }
    return PP_OK;
  }
};

int CheckImageCall(pp_tracks_handle h, const pp_tracks_image_options* o, int32_t image, pp_tracks_image_report* report, const int32_t* event_point,
                   const int32_t* event_line, int64_t capacity, const char* where) {
  PP_REQUIRE(h && report && capacity >= 0 && (capacity == 0 || (event_point && event_line)), "%s: bad argument", where);
  PP_REQUIRE(image >= 0 && image < h->C, "%s: image %d of %d", where, image, h->C);
  PP_REQUIRE(o && o->create_max_angle_error >= 0 && o->continue_max_angle_error >= 0 && o->complete_max_reproj_error >= 0 && o->min_angle >= 0 &&
                 o->max_transitivity >= 0 && o->complete_max_transitivity >= 0,
             "%s: bad options", where);
  return PP_OK;
}

std::vector<int32_t> LinesOfImage(const TrackState& st, int32_t image) {
  std::vector<int32_t> lines;
  for (int64_t l = 0; l < st.L; ++l) if (st.line_image[(size_t)l] == image) lines.push_back((int32_t)l);
  return lines;
}

int ReplayError(int error, const char* where) {
  if (error == 1) { SetLastError("%s: a speculative result claims a line that is not free", where); return PP_ERR_INTERNAL; }
  return error ? PP_ERR_HIP : PP_OK;      // (2: a fresh launch failed and has set the message)
}

}  // namespace

extern "C" {

void pp_tracks_image_options_default(pp_tracks_image_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->create_max_angle_error = 2.0; o->continue_max_angle_error = 2.0; o->complete_max_reproj_error = 4.0; o->min_angle = 1.5;
  o->max_transitivity = 1; o->complete_max_transitivity = 5; o->ignore_two_view_tracks = 1;
}

int pp_tracks_triangulate_image(pp_tracks_handle h, const pp_tracks_image_options* o, int32_t image, const uint8_t* line_aligned, pp_tracks_image_report* report,
                                int32_t* event_point, int32_t* event_line, int64_t capacity) try {
  const char* where = "pp_tracks_triangulate_image";
  PP_TRY(CheckImageCall(h, o, image, report, event_point, event_line, capacity, where));
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  TrackState& st = h->st;
  if (!st.image_registered[(size_t)image] || h->image_skip[(size_t)image]) return PP_OK;      // :72-79
  const std::vector<int32_t> lines = LinesOfImage(st, image);
  if (lines.empty()) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  ImageCall call(h, o, line_aligned, true);
  PP_TRY(call.Begin());
  std::vector<ImageLineResult> res;
  auto triangulate = [&](std::vector<ImageLineResult>& rs, float* ms) {
    std::vector<ImageLineResult*> items;
    for (ImageLineResult& r : rs) {
      r.min_trials = CreateMinTrials(r.set.size());
      if (!r.list.empty() && r.set.size() >= 3) items.push_back(&r);
    }
    return call.Triangulate(items, ms);
  };
  PP_TRY(call.Find(lines, o->max_transitivity, res, &call.device_ms));
  PP_TRY(triangulate(res, &call.device_ms));
  report->device_ms = call.device_ms;
  const int32_t spec_launches = call.launches;
  const auto t_replay = Clock::now();
  std::vector<ImageLineResult> one;
  int64_t written = 0;
  const ImageCounters cnt = ReplayTriangulateImage(
      st, lines, [&](size_t i) -> const ImageLineResult& { return res[i]; },
      [&](int32_t line) -> const ImageLineResult* {
        if (call.Sync() || call.Find(std::vector<int32_t>{line}, o->max_transitivity, one, nullptr) || triangulate(one, nullptr)) return nullptr;
        return &one[0];
      },
      [&](int p, int32_t l) { if (written < capacity) { event_point[written] = p; event_line[written] = l; } ++written; });
  PP_TRY(ReplayError(cnt.error, where));
  report->num_changed = cnt.num_tris; report->num_entries = written; report->ransac_trials = cnt.trials;
  report->points_created = cnt.points_created; report->lines_continued = cnt.lines_continued; report->lines_redone = cnt.lines_redone;
  report->fresh_launches = call.launches - spec_launches;
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_triangulate_image")

int pp_tracks_complete_image(pp_tracks_handle h, const pp_tracks_image_options* o, int32_t image, pp_tracks_image_report* report, int32_t* event_point,
                             int32_t* event_line, int64_t capacity) try {
  const char* where = "pp_tracks_complete_image";
  PP_TRY(CheckImageCall(h, o, image, report, event_point, event_line, capacity, where));
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  TrackState& st = h->st;
  if (!st.image_registered[(size_t)image] || h->image_skip[(size_t)image]) return PP_OK;      // :132-139
  const std::vector<int32_t> lines = LinesOfImage(st, image);
  if (lines.empty()) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  const double max2 = o->complete_max_reproj_error * o->complete_max_reproj_error;
  // the lines that have a point: K10a on exactly those points
  std::vector<uint8_t> subset((size_t)st.NumPoints(), 0);
  bool any_point = false;
  std::vector<int32_t> work, work_of(lines.size(), -1);
  for (size_t i = 0; i < lines.size(); ++i) {
    const int p = st.line_point[(size_t)lines[i]];
    if (p >= 0) { subset[(size_t)p] = 1; any_point = true; continue; }
    if (o->ignore_two_view_tracks && IsTwoViewObservation(st, lines[i])) continue;      // :171-174
    work_of[i] = (int32_t)work.size();
    work.push_back(lines[i]);
  }
  CompleteSpec cspec;
  float device_ms = 0.f;
  if (any_point) {
    PP_TRY(SpeculateComplete(h, subset.data(), o->complete_max_transitivity, max2, where, &cspec));
    device_ms += cspec.device_ms;
  }
  ImageCall call(h, o, nullptr, false);
  PP_TRY(call.Begin());
  std::vector<ImageLineResult> res;
  PP_TRY(call.Find(work, o->max_transitivity, res, &call.device_ms));
  {
    std::vector<ImageLineResult*> items;
    uint64_t carried = 0;
    for (ImageLineResult& r : res) {
      if (r.num_triangulated || r.list.empty()) continue;      // :179
      r.min_trials = carried = CompleteMinTrials(r.set.size(), carried);
      if (r.set.size() >= 3) items.push_back(&r);
    }
    PP_TRY(call.Triangulate(items, &call.device_ms));
  }
  report->device_ms = device_ms + call.device_ms;
  const int32_t call_spec_launches = call.launches;
  int32_t fresh_complete_launches = 0;
  const auto t_replay = Clock::now();
  std::vector<ImageLineResult> one;
  CompleteSpec cone;
  std::vector<uint8_t> only;
  int64_t written = 0;
  const ImageCounters cnt = ReplayCompleteImage(
      st, lines, o->ignore_two_view_tracks != 0, o->complete_max_transitivity, [&](size_t i) { return work_of[i] >= 0; },
      [&](size_t i) -> const ImageLineResult& { return res[(size_t)work_of[i]]; },
      [&](int32_t line, uint64_t carried) -> const ImageLineResult* {
        if (call.Sync() || call.Find(std::vector<int32_t>{line}, o->max_transitivity, one, nullptr)) return nullptr;
        ImageLineResult& r = one[0];
        std::vector<ImageLineResult*> items;
        if (!r.num_triangulated && !r.list.empty()) {
          r.min_trials = CompleteMinTrials(r.set.size(), carried);
          if (r.set.size() >= 3) items.push_back(&r);
        }
        if (call.Triangulate(items, nullptr)) return nullptr;
        return &r;
      },
      [&](int p) { return cspec.List(p); },
      [&](int p, std::vector<int32_t>* list) -> int {      // K10a for one point on the current state
        only.assign((size_t)st.NumPoints(), 0);
        only[(size_t)p] = 1;
        cone = CompleteSpec();
        const int rc = SpeculateComplete(h, only.data(), o->complete_max_transitivity, max2, where, &cone);
        if (rc) return rc;
        fresh_complete_launches += 1 + cone.second_launches;
        const SpecList sl = cone.List(p);
        list->assign(sl.line, sl.line + sl.count);
        return PP_OK;
      },
      [&](int p, int32_t l) { if (written < capacity) { event_point[written] = p; event_line[written] = l; } ++written; });
  PP_TRY(ReplayError(cnt.error, where));
  report->num_changed = cnt.num_tris; report->num_entries = written; report->ransac_trials = cnt.trials;
  report->points_created = cnt.points_created; report->lines_continued = 0; report->lines_redone = cnt.lines_redone;
  report->fresh_launches = call.launches - call_spec_launches + fresh_complete_launches;
  report->replay_ms = MsSince(t_replay);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_tracks_complete_image")

}  // extern "C"
