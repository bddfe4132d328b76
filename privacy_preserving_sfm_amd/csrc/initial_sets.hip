// K15 - the image-set search of IncrementalMapper::RegisterInitialLineImages on a pp_tracks_handle: which image quadruples are worth a four-view solve.
//   the 4-view tracks of the check images' lines     reference src/sfm/incremental_mapper.cc:261-363 (assemble_tracks :265-290, the alignment filter :326-332)
//   de-duplication per image set                     :243-250 (std::map<ImageSet, std::set<FeatureIdxs>>), :353-359
//   qualifying, ranking, truncation                  :393-435 (initial_sets_replay.hpp)
// As K10-K14: the device does the data-parallel part on what the handle holds (the CSR correspondence graph and line_image), the host replays the short
// sequential rest.  The handle's state is neither read nor changed: the search knows no points and no registered images.
// K15 k_initial_tracks   <fill = false> counts, <fill = true> writes.  ONE WAVEFRONT PER LINE of a check image that keeps at least three neighbours.  The
//                        neighbours that pass the filter (the same alignment flag as the line, an image of the subset) are staged with their image indices,
//                        64 at a time in corr_line order: in LDS up to kInitList entries, for a longer list in a segment of global memory the host sized by
//                        the line's whole neighbour list (it cannot overflow).  The pairs i < j of that list are dealt round the lanes; a lane walks k > j
//                        and keeps a triple when the four images (the line's and the three neighbours') are pairwise different.  The count form adds up an
//                        int64 per line; the fill form writes the four line numbers ORDERED BY IMAGE INDEX as one 16-byte record at offset[line] + a rank
//                        handed out by an LDS counter (the order inside a line's span is free: the records are sorted next).
//                        The counts are scanned as int64 (LaunchExclusiveScan, scan.hpp), the total last.
//    k_initial_keys      one lane per unique record: the set key (initial_sets_replay.hpp) from line_image and the alignment flag of its first line.
// Between them rocPRIM's device primitives: merge_sort of the records (lexicographic over the four line numbers), unique, radix_sort_pairs by set key
// (stable: inside a set and class the lexicographic order stays - the order in which the reference hands the lines to the solver), run_length_encode.
// No kernel of this file waits for another workgroup.
#include <cstring>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>

#include "initial_sets_replay.hpp"
#include "scan.hpp"
#include "tracks_device.hpp"

namespace ppsfm {

constexpr int kInitList = 64;      // filtered neighbours of a line kept on chip, (line, image) pairs: one chunk of the wavefront, 512 B of LDS

struct InitRecord {
  int32_t l[4];
};
static_assert(sizeof(InitRecord) == 16, "a record is four line numbers");

struct InitRecordLess {
  __host__ __device__ bool operator()(const InitRecord& a, const InitRecord& b) const {
    for (int i = 0; i < 4; ++i)
      if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
  }
};
struct InitRecordEqual {
  __host__ __device__ bool operator()(const InitRecord& a, const InitRecord& b) const {
    return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3];
  }
};

struct InitArgs {
  int N;                              // lines at work
  const int32_t* work_line;           // N, ascending
  const int64_t* glist_off;           // N: -1 = the filtered list stays in LDS, else the line's segment of glist (in pairs)
  int32_t* glist;                     // (line, image) pairs
  const uint8_t* line_aligned;        // L
  const uint8_t* subset;              // C or nullptr
  int64_t* count;                     // count form: N
  const int64_t* offset;              // fill form: N + 1, exclusive scan of count and the total
  InitRecord* rec;                    // fill form: offset[N] records
};

__device__ __forceinline__ void OrderByImage(int& ia, int& la, int& ib, int& lb) {
  if (ib < ia) { const int ti = ia, tl = la; ia = ib; la = lb; ib = ti; lb = tl; }
}

template <bool kFill>
__global__ __launch_bounds__(64) void k_initial_tracks(TrackDev d, InitArgs a) {
  __shared__ int32_t s_list[2 * kInitList];
  __shared__ unsigned long long s_total;      // count form: the line's triples; fill form: the next free rank
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= a.N) return;
  const int ref = a.work_line[w];
  const int ref_img = d.line_image[ref];
  const uint8_t ref_aligned = a.line_aligned[ref];
  const int c0 = d.corr_start[ref], c1 = d.corr_start[ref + 1];
  const int64_t goff = a.glist_off[w];
  int32_t* list = goff < 0 ? s_list : a.glist + 2 * goff;
  const int cap = goff < 0 ? kInitList : c1 - c0;      // (the host chose: at most kInitList neighbours pass, or a segment of c1 - c0 pairs)
  if (lane == 0) s_total = 0;
  int n = 0;
  for (int base = c0; base < c1; base += 64) {
    const int i = base + lane;
    bool keep = false;
    int l = -1, img = -1;
    if (i < c1) {
      l = d.corr_line[i];
      img = d.line_image[l];
      keep = a.line_aligned[l] == ref_aligned && (!a.subset || a.subset[img]);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int pos = n + __popcll(m & ((1ull << lane) - 1));
      if (pos < cap) { list[2 * pos] = l; list[2 * pos + 1] = img; }
    }
    n += __popcll(m);
  }
  if (n > cap) n = cap;
  __syncthreads();      // (one wavefront per workgroup, wave-uniform control flow: the list and s_total become visible to every lane)
  const int64_t span = kFill ? a.offset[w + 1] - a.offset[w] : 0;
  InitRecord* out = kFill ? a.rec + a.offset[w] : nullptr;
  unsigned long long mine = 0;
  // the pairs (i, j), i < j, in row-major order: this lane takes every 64th, starting with its own
  int i = 0;
  int64_t j = 1 + lane;
  while (n >= 3) {
    while (j >= n && i < n - 1) { ++i; j = j - n + i + 1; }
    if (i >= n - 1) break;
    const int li = list[2 * i], ii = list[2 * i + 1], lj = list[2 * (int)j], ij = list[2 * (int)j + 1];
    if (ii != ij && ii != ref_img && ij != ref_img) {
      for (int k = (int)j + 1; k < n; ++k) {
        const int ik = list[2 * k + 1];
        if (ik == ii || ik == ij || ik == ref_img) continue;      // two lines in one image: the reference's std::set on image_id keeps three (:275-283)
        if (!kFill) { ++mine; continue; }
        const unsigned long long pos = atomicAdd(&s_total, 1ull);
        if (pos >= (unsigned long long)span) continue;      // (the count form saw the same list: never taken)
        int i0 = ref_img, l0 = ref, i1 = ii, l1 = li, i2 = ij, l2 = lj, i3 = ik, l3 = list[2 * k];
        OrderByImage(i0, l0, i1, l1); OrderByImage(i2, l2, i3, l3); OrderByImage(i0, l0, i2, l2); OrderByImage(i1, l1, i3, l3); OrderByImage(i1, l1, i2, l2);
        InitRecord r;
        r.l[0] = l0; r.l[1] = l1; r.l[2] = l2; r.l[3] = l3;
        out[pos] = r;
      }
    }
    j += 64;
  }
  if (!kFill) {
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (lane == 0) a.count[w] = (int64_t)s_total;
  }
}

__global__ __launch_bounds__(256) void k_initial_keys(unsigned int n, const InitRecord* __restrict__ rec, const int32_t* __restrict__ line_image,
                                                      const uint8_t* __restrict__ line_aligned, uint64_t* __restrict__ key) {
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const InitRecord r = rec[t];
  key[t] = PackInitSetKey(line_image[r.l[0]], line_image[r.l[1]], line_image[r.l[2]], line_image[r.l[3]], !line_aligned[r.l[0]]);
}

}  // namespace ppsfm

using namespace ppsfm;

namespace {

// one rocPRIM primitive: the size query, the temporary block, the call
template <typename Call>
int WithTemporary(CallScratch& cb, const char* what, Call&& call) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e == hipSuccess) {
    uint8_t* tmp = nullptr;
    PP_TRY(cb.Alloc(&tmp, bytes));
    e = call(tmp, bytes);
  }
  if (e != hipSuccess) { SetLastError("pp_tracks_find_initial_sets: %s failed: %s", what, hipGetErrorString(e)); return PP_ERR_HIP; }
  return PP_OK;
}

}  // namespace

extern "C" {

void pp_init_sets_options_default(pp_init_sets_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->min_num_aligned_tracks = 20; o->min_num_random_tracks = 20; o->max_num_sets = 10; o->max_candidates = (int64_t)1 << 24;
}

int pp_tracks_find_initial_sets(pp_tracks_handle h, const pp_init_sets_options* o, const uint8_t* line_aligned, const uint8_t* image_subset,
                                const int32_t* check_images, int32_t num_check, pp_init_sets_report* report, int32_t* set_images,
                                int32_t* set_num_aligned, int32_t* set_num_random, int64_t* track_start, int32_t* track_lines, int64_t capacity) try {
  const char* where = "pp_tracks_find_initial_sets";
  // what can be decided without the handle comes first
  PP_REQUIRE(h && o && report && line_aligned && check_images && num_check > 0 && capacity >= 0 && (capacity == 0 || track_lines), "%s: bad argument", where);
  PP_REQUIRE(o->min_num_aligned_tracks >= 0 && o->min_num_random_tracks >= 0 && o->max_num_sets >= 0 && o->max_candidates >= 0 &&
                 o->max_candidates <= 0x7FFFFFFF, "%s: bad options", where);
  PP_REQUIRE(o->max_num_sets == 0 || (set_images && set_num_aligned && set_num_random && track_start), "%s: max_num_sets = %d without the set arrays", where,
             o->max_num_sets);
  {
    std::vector<int32_t> sorted(check_images, check_images + num_check);
    std::sort(sorted.begin(), sorted.end());
    PP_REQUIRE(sorted.front() >= 0, "%s: check image %d", where, sorted.front());
    for (int32_t i = 1; i < num_check; ++i) PP_REQUIRE(sorted[(size_t)i] != sorted[(size_t)i - 1], "%s: check image %d is given twice", where, sorted[(size_t)i]);
  }
  const int C = h->C;
  PP_REQUIRE(C <= kInitSetMaxImages, "%s: %d images, the set key holds %d", where, C, kInitSetMaxImages);
  for (int32_t i = 0; i < num_check; ++i) {
    PP_REQUIRE(check_images[i] < C, "%s: check image %d of %d", where, check_images[i], C);
    PP_REQUIRE(!image_subset || image_subset[check_images[i]], "%s: check image %d is outside the subset", where, check_images[i]);
  }
  const auto t_begin = Clock::now();
  std::memset(report, 0, sizeof(*report));
  if (o->max_num_sets > 0) track_start[0] = 0;
  const TrackState& st = h->st;
  // the lines at work: those of the check images that keep at least three neighbours (:337); a filtered list longer than the on-chip list gets a
  // segment of global memory as long as the line's whole list
  std::vector<uint8_t> is_check((size_t)C, 0);
  for (int32_t i = 0; i < num_check; ++i) is_check[(size_t)check_images[i]] = 1;
  std::vector<int32_t> work;
  std::vector<int64_t> goff;
  int64_t gtotal = 0;
  for (int64_t l = 0; l < st.L; ++l) {
    if (!is_check[(size_t)st.line_image[(size_t)l]]) continue;
    const int32_t c0 = st.corr_start[(size_t)l], c1 = st.corr_start[(size_t)l + 1];
    int64_t kept = 0;
    for (int32_t e = c0; e < c1; ++e) {
      const int32_t n = st.corr_line[(size_t)e];
      kept += line_aligned[n] == line_aligned[l] && (!image_subset || image_subset[st.line_image[(size_t)n]]);
    }
    if (kept < 3) continue;
    work.push_back((int32_t)l);
    goff.push_back(kept > kInitList ? gtotal : -1);
    if (kept > kInitList) { gtotal += c1 - c0; ++report->overflow_lines; }
  }
  const int N = (int)work.size();
  report->num_work_lines = N;
  auto finish = [&]() {
    report->total_ms = MsSince(t_begin);
    return PP_OK;
  };
  if (N == 0) return finish();
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  StreamTimer timer(*h);
  CallScratch cb(s);
  const TrackDev d = h->dev;
  InitArgs a{};
  a.N = N;
  int32_t* d_work = nullptr;
  int64_t *d_goff = nullptr, *d_offset = nullptr, *d_scan = nullptr;
  uint8_t *d_aligned = nullptr, *d_subset = nullptr;
  PP_TRY(cb.Put(&d_work, work.data(), (size_t)N)); PP_TRY(cb.Put(&d_goff, goff.data(), (size_t)N));
  PP_TRY(cb.Put(&d_aligned, line_aligned, (size_t)h->L));
  if (image_subset) PP_TRY(cb.Put(&d_subset, image_subset, (size_t)C));
  PP_TRY(cb.Alloc(&a.glist, 2 * (size_t)gtotal)); PP_TRY(cb.Alloc(&a.count, (size_t)N)); PP_TRY(cb.Alloc(&d_offset, (size_t)N + 1));
  PP_TRY(cb.Alloc(&d_scan, ScanScratchCount(N)));
  a.work_line = d_work; a.glist_off = d_goff; a.line_aligned = d_aligned; a.subset = d_subset; a.offset = d_offset;
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_initial_tracks<false>, dim3((unsigned)N), dim3(64), 0, s, d, a);
  const ScanJob<int64_t> offsets{a.count, d_offset, d_offset + N};
  LaunchExclusiveScan(s, N, &offsets, 1, d_scan);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  int64_t total = 0;
  PP_TRY(Download(&total, d_offset + N, 1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  report->device_ms = timer.ms;
  if (total < 0) { SetLastError("%s: the count of candidates is out of range", where); return PP_ERR_INTERNAL; }
  report->num_candidates = total;
  PP_REQUIRE(total <= o->max_candidates, "%s: %lld candidate tracks, max_candidates is %lld", where, (long long)total, (long long)o->max_candidates);
  if (total == 0) return finish();
  const size_t M = (size_t)total;
  InitRecord *d_rec = nullptr, *d_sorted = nullptr;
  uint64_t *d_key = nullptr, *d_key_sorted = nullptr, *d_run_key = nullptr;
  unsigned int *d_run_count = nullptr, *d_num = nullptr;      // d_num: [0] unique records, [1] runs
  PP_TRY(cb.Alloc(&d_rec, M)); PP_TRY(cb.Alloc(&d_sorted, M)); PP_TRY(cb.Alloc(&d_num, 2));
  a.rec = d_rec;
  PP_HIP_TRY(hipMemsetAsync(d_rec, 0, M * sizeof(InitRecord), s));      // (a record the fill form left out would still name lines that exist)
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_initial_tracks<true>, dim3((unsigned)N), dim3(64), 0, s, d, a);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(WithTemporary(cb, "merge_sort", [&](void* tmp, size_t& bytes) { return rocprim::merge_sort(tmp, bytes, d_rec, d_sorted, M, InitRecordLess(), s); }));
  PP_TRY(WithTemporary(cb, "unique", [&](void* tmp, size_t& bytes) { return rocprim::unique(tmp, bytes, d_sorted, d_rec, d_num, M, InitRecordEqual(), s); }));
  PP_TRY(timer.End());
  unsigned int num[2] = {0, 0};
  PP_TRY(Download(num, d_num, 1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  const size_t U = num[0];      // the unique records, in d_rec
  if (U == 0 || U > M) { SetLastError("%s: the count of unique tracks is out of range", where); return PP_ERR_INTERNAL; }
  PP_TRY(cb.Alloc(&d_key, U)); PP_TRY(cb.Alloc(&d_key_sorted, U)); PP_TRY(cb.Alloc(&d_run_key, U)); PP_TRY(cb.Alloc(&d_run_count, U));
  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_initial_keys, dim3(CeilDiv((int64_t)U, 256)), dim3(256), 0, s, (unsigned int)U, (const InitRecord*)d_rec, d.line_image,
                     (const uint8_t*)d_aligned, d_key);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(WithTemporary(cb, "radix_sort_pairs", [&](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, d_key, d_key_sorted, d_rec, d_sorted, U, 0u, (unsigned int)kInitSetKeyBits, s);
  }));
  PP_TRY(WithTemporary(cb, "run_length_encode", [&](void* tmp, size_t& bytes) {
    return rocprim::run_length_encode(tmp, bytes, d_key_sorted, (unsigned int)U, d_run_key, d_run_count, d_num + 1, s);
  }));
  PP_TRY(timer.End());
  PP_TRY(Download(num + 1, d_num + 1, 1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  const size_t R = num[1];
  if (R == 0 || R > U) { SetLastError("%s: the count of image sets is out of range", where); return PP_ERR_INTERNAL; }
  std::vector<uint64_t> run_key(R);
  std::vector<unsigned int> run_count32(R);
  PP_TRY(Download(run_key.data(), d_run_key, R, s)); PP_TRY(Download(run_count32.data(), d_run_count, R, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  report->device_ms = timer.ms;
  const auto t_replay = Clock::now();
  std::vector<int64_t> run_count(run_count32.begin(), run_count32.end()), run_start(R + 1, 0);
  for (size_t i = 0; i < R; ++i) run_start[i + 1] = run_start[i] + run_count[i];
  const InitialSetsResult r = ReplayInitialSets((int64_t)R, run_key.data(), run_count.data(), o->min_num_aligned_tracks, o->min_num_random_tracks, o->max_num_sets);
  report->num_aligned_tracks = r.num_aligned_tracks; report->num_random_tracks = r.num_random_tracks;
  report->num_aligned_sets = r.num_aligned_sets; report->num_random_sets = r.num_random_sets;
  report->num_qualified = r.num_qualified; report->num_returned = (int32_t)r.sets.size();
  // the tracks of the returned sets: aligned, then random, each a run of the sorted records
  int64_t written = 0;
  std::vector<InitRecord> seg;
  for (size_t k = 0; k < r.sets.size(); ++k) {
    const InitialSet& set = r.sets[k];
    std::copy(set.images, set.images + 4, set_images + 4 * k);
    set_num_aligned[k] = (int32_t)set.num_aligned; set_num_random[k] = (int32_t)set.num_random;
    const int64_t runs[2] = {set.aligned_run, set.random_run};
    for (int c = 0; c < 2; ++c) {
      const int64_t begin = run_start[(size_t)runs[c]], len = run_count[(size_t)runs[c]];
      const int64_t take = std::max<int64_t>(0, std::min(len, capacity - written));
      if (take > 0) {
        seg.resize((size_t)take);
        PP_TRY(Download(seg.data(), d_sorted + begin, (size_t)take, s));
        PP_HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(track_lines + 4 * written, seg.data(), (size_t)take * sizeof(InitRecord));
      }
      written += len;
      track_start[2 * k + (size_t)c + 1] = written;
    }
  }
  report->num_track_entries = written;
  report->replay_ms = MsSince(t_replay);
  return finish();
} PP_API_CATCH("pp_tracks_find_initial_sets")

}  // extern "C"
