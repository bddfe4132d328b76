// K18 - the correspondence graph from the match lists: DatabaseCache::Load's use of the matches (reference src/base/database_cache.cc:82-191) and
// CorrespondenceGraph::AddCorrespondences / Finalize (src/base/correspondence_graph.cc:56-163), up to the corr_start / corr_line CSR of pp_tracks_desc.
// The rules that have an order in them, the pair plan and the sequential replay are in corr_graph_replay.hpp; this file is the device half and the C ABI.
// Line x of image k is global line line_start[k] + x.  M matches, L lines, E = 2 * accepted CSR entries; device memory is O(M + L + pairs).
// K18a k_corr_first    one workgroup per (used pair, tile of kCorrTile = 4096 line indices).  Two LDS tables, one per side, hold for every index of the tile the
//                      position of the FIRST valid match of the pair that names it (atomicMin over positions: a minimum does not depend on the order it
//                      was reached in); a second walk over the pair's matches writes dup1 / dup2 = "not the first" for the indices of this tile.  Per pair:
//                      the repeats on either side and the matches with a bad index (integer sums).
// K18b k_corr_accept   one lane per match: its pair (a binary search in match_start), accepted = valid, first on side 1 and first on side 2.
//                      The host then reads the per-pair repeats and overwrites the flags of the pairs CorrNeedsReplay names with CorrReplayPair's.
// K18c k_corr_count    one lane per match: the degree of both lines (atomicAdd of 1: a count) and the accepted matches per pair.
// K18d                 corr_start = the exclusive scan of the degrees, the number of entries last (LaunchExclusiveScan, scan.hpp).
// K18e k_corr_scatter  one lane per accepted match: a slot in each line's range from an atomic cursor; (pair rank, neighbour, owner) go to the slot.
// K18f k_corr_order    one lane per slot: its place is the number of entries of the same line with a smaller pair rank - a line has at most one neighbour
//                      per pair, so the ranks of a list are distinct and the places a permutation.  corr_line is written in pair order whatever slots the
//                      atomics handed out; nothing in the result depends on the schedule.
// K18g k_corr_image    one workgroup per image: lines with a neighbour, and the image's CSR entries.
#include <cstring>

#include "corr_graph_replay.hpp"
#include "device_handle.hpp"
#include "scan.hpp"

namespace ppsfm {

constexpr int kCorrTile = 4096;          // line indices per LDS table of k_corr_first
constexpr int kCorrBlock = 256;

struct CorrPairDev {       // one input pair, as stored
  int32_t swapped;         // the input's columns are (x2, x1)
  int32_t rank;            // among the used pairs that add to the graph; -1: contributes nothing
  int32_t n1, n2;          // line counts of image1 < image2
  int32_t ls1, ls2;        // their first global lines
};

struct CorrWork { int32_t pair, tile; };

__global__ __launch_bounds__(kCorrBlock) void k_corr_first(const CorrWork* __restrict__ work, const CorrPairDev* __restrict__ plan, const int64_t* __restrict__ mstart,
                                                           const int32_t* __restrict__ matches, uint8_t* __restrict__ dup1, uint8_t* __restrict__ dup2,
                                                           int32_t* __restrict__ cls) {
  __shared__ int32_t first1[kCorrTile], first2[kCorrTile];
  __shared__ int32_t red[3];
  const CorrWork w = work[blockIdx.x];
  const CorrPairDev q = plan[w.pair];
  const int64_t m0 = mstart[w.pair];
  const int32_t cnt = (int32_t)(mstart[w.pair + 1] - m0);
  const int32_t t0 = w.tile * kCorrTile;
  const int tid = threadIdx.x;
  for (int k = tid; k < kCorrTile; k += kCorrBlock) { first1[k] = 0x7FFFFFFF; first2[k] = 0x7FFFFFFF; }
  if (tid < 3) red[tid] = 0;
  __syncthreads();
  int bad = 0;
  for (int32_t i = tid; i < cnt; i += kCorrBlock) {
    const int32_t a = matches[2 * (m0 + i)], b = matches[2 * (m0 + i) + 1];
    const int32_t x1 = q.swapped ? b : a, x2 = q.swapped ? a : b;
    if ((uint32_t)x1 < (uint32_t)q.n1 && (uint32_t)x2 < (uint32_t)q.n2) {
      if ((uint32_t)(x1 - t0) < (uint32_t)kCorrTile) atomicMin(&first1[x1 - t0], i);
      if ((uint32_t)(x2 - t0) < (uint32_t)kCorrTile) atomicMin(&first2[x2 - t0], i);
    } else {
      ++bad;
    }
  }
  __syncthreads();
  int r1 = 0, r2 = 0;
  for (int32_t i = tid; i < cnt; i += kCorrBlock) {
    const int32_t a = matches[2 * (m0 + i)], b = matches[2 * (m0 + i) + 1];
    const int32_t x1 = q.swapped ? b : a, x2 = q.swapped ? a : b;
    if ((uint32_t)x1 < (uint32_t)q.n1 && (uint32_t)x2 < (uint32_t)q.n2) {
      if ((uint32_t)(x1 - t0) < (uint32_t)kCorrTile) { const int d = first1[x1 - t0] != i; dup1[m0 + i] = (uint8_t)d; r1 += d; }
      if ((uint32_t)(x2 - t0) < (uint32_t)kCorrTile) { const int d = first2[x2 - t0] != i; dup2[m0 + i] = (uint8_t)d; r2 += d; }
    }
  }
  r1 = WaveSumInt(r1); r2 = WaveSumInt(r2); bad = WaveSumInt(bad);
  if ((tid & 63) == 0) { atomicAdd(&red[0], r1); atomicAdd(&red[1], r2); atomicAdd(&red[2], bad); }
  __syncthreads();
  // every tile of the pair saw every match: the bad indices are counted by tile 0 alone
  if (tid < 3 && red[tid] != 0 && (tid < 2 || w.tile == 0)) atomicAdd(&cls[3 * (int64_t)w.pair + tid], red[tid]);
}

__global__ __launch_bounds__(kCorrBlock) void k_corr_accept(int64_t num_matches, int32_t num_pairs, const CorrPairDev* __restrict__ plan, const int64_t* __restrict__ mstart,
                                                            const int32_t* __restrict__ matches, const uint8_t* __restrict__ dup1, const uint8_t* __restrict__ dup2,
                                                            int32_t* __restrict__ pair_of, uint8_t* __restrict__ accepted) {
  const int64_t m = (int64_t)blockIdx.x * kCorrBlock + threadIdx.x;
  if (m >= num_matches) return;
  int32_t lo = 0, hi = num_pairs;      // the last pair with mstart[p] <= m: its range is not empty, so it is m's
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (mstart[mid] <= m) lo = mid; else hi = mid;
  }
  const CorrPairDev q = plan[lo];
  const int32_t a = matches[2 * m], b = matches[2 * m + 1];
  const int32_t x1 = q.swapped ? b : a, x2 = q.swapped ? a : b;
  const bool valid = (uint32_t)x1 < (uint32_t)q.n1 && (uint32_t)x2 < (uint32_t)q.n2;
  pair_of[m] = lo;
  accepted[m] = q.rank >= 0 && valid && !dup1[m] && !dup2[m];
}

__global__ __launch_bounds__(kCorrBlock) void k_corr_count(int64_t num_matches, const CorrPairDev* __restrict__ plan, const int32_t* __restrict__ matches,
                                                           const int32_t* __restrict__ pair_of, const uint8_t* __restrict__ accepted, int32_t* __restrict__ degree,
                                                           int32_t* __restrict__ pair_accepted) {
  const int64_t m = (int64_t)blockIdx.x * kCorrBlock + threadIdx.x;
  const bool in = m < num_matches;
  const int32_t p = in ? pair_of[m] : -1;
  const bool acc = in && accepted[m];
  if (acc) {
    const CorrPairDev q = plan[p];
    const int32_t a = matches[2 * m], b = matches[2 * m + 1];
    atomicAdd(&degree[q.ls1 + (q.swapped ? b : a)], 1);
    atomicAdd(&degree[q.ls2 + (q.swapped ? a : b)], 1);
  }
  // a wavefront mostly lies inside one pair: one add for it then
  const int32_t p0 = __shfl(p, 0, 64);
  if (__all(!acc || p == p0)) {
    const int n = __popcll(__ballot(acc));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&pair_accepted[p0], n);
  } else if (acc) {
    atomicAdd(&pair_accepted[p], 1);
  }
}

__global__ __launch_bounds__(kCorrBlock) void k_corr_scatter(int64_t num_matches, int64_t num_entries, const CorrPairDev* __restrict__ plan,
                                                             const int32_t* __restrict__ matches, const int32_t* __restrict__ pair_of,
                                                             const uint8_t* __restrict__ accepted, int32_t* __restrict__ cursor, int32_t* __restrict__ slot_rank,
                                                             int32_t* __restrict__ slot_line, int32_t* __restrict__ slot_owner) {
  const int64_t m = (int64_t)blockIdx.x * kCorrBlock + threadIdx.x;
  if (m >= num_matches || !accepted[m]) return;
  const CorrPairDev q = plan[pair_of[m]];
  const int32_t a = matches[2 * m], b = matches[2 * m + 1];
  const int32_t g1 = q.ls1 + (q.swapped ? b : a), g2 = q.ls2 + (q.swapped ? a : b);
  const int32_t s1 = atomicAdd(&cursor[g1], 1), s2 = atomicAdd(&cursor[g2], 1);
  if ((int64_t)s1 < num_entries) { slot_rank[s1] = q.rank; slot_line[s1] = g2; slot_owner[s1] = g1; }
  if ((int64_t)s2 < num_entries) { slot_rank[s2] = q.rank; slot_line[s2] = g1; slot_owner[s2] = g2; }
}

__global__ __launch_bounds__(kCorrBlock) void k_corr_order(int64_t num_entries, const int32_t* __restrict__ corr_start, const int32_t* __restrict__ slot_rank,
                                                           const int32_t* __restrict__ slot_line, const int32_t* __restrict__ slot_owner,
                                                           int32_t* __restrict__ corr_line) {
  const int64_t e = (int64_t)blockIdx.x * kCorrBlock + threadIdx.x;
  if (e >= num_entries) return;
  const int32_t g = slot_owner[e], r = slot_rank[e];
  const int32_t s = corr_start[g], t = corr_start[g + 1];
  int32_t place = 0;
  for (int32_t j = s; j < t; ++j) place += slot_rank[j] < r;
  corr_line[s + place] = slot_line[e];      // (place < t - s: the entry itself is not counted)
}

__global__ __launch_bounds__(kCorrBlock) void k_corr_image(const int32_t* __restrict__ line_start, const int32_t* __restrict__ corr_start,
                                                           int32_t* __restrict__ num_observations, int32_t* __restrict__ num_correspondences) {
  __shared__ int32_t red;
  const int tid = threadIdx.x;
  const int32_t l0 = line_start[blockIdx.x], l1 = line_start[blockIdx.x + 1];
  if (tid == 0) red = 0;
  __syncthreads();
  int n = 0;
  for (int32_t l = l0 + tid; l < l1; l += kCorrBlock) n += corr_start[l + 1] > corr_start[l];
  n = WaveSumInt(n);
  if ((tid & 63) == 0) atomicAdd(&red, n);
  __syncthreads();
  if (tid == 0) { num_observations[blockIdx.x] = red; num_correspondences[blockIdx.x] = corr_start[l1] - corr_start[l0]; }
}

}  // namespace ppsfm

struct pp_corr_graph_impl : ppsfm::DeviceHandle {      // blocks: line_start and the last build's CSR
  int32_t num_images = 0;
  std::vector<int32_t> num_lines, line_start;      // num_images, num_images + 1
  int32_t* d_line_start = nullptr;
  // the last build
  bool built = false;
  int64_t num_entries = 0;
  int32_t* d_corr_start = nullptr;                 // L + 1
  int32_t* d_corr_line = nullptr;                  // num_entries
  std::vector<uint8_t> connected;
  std::vector<int32_t> image_observations, image_correspondences, pair_correspondences;
  int64_t NumLines() const { return line_start[(size_t)num_images]; }
};

using namespace ppsfm;

namespace {

// the CSR of a build in the handle's blocks: given back unless the build completes
struct CorrFresh {
  DeviceBlocks* b;
  int32_t *start = nullptr, *line = nullptr;
  bool keep = false;
  ~CorrFresh() {
    if (keep) return;
    if (start) b->Free(&start);
    if (line) b->Free(&line);
  }
};

}  // namespace

extern "C" {

int pp_corr_graph_destroy(pp_corr_graph_handle h) try {
  delete h;      // (~DeviceHandle)
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_destroy")

int pp_corr_graph_create(int32_t num_images, const int32_t* num_lines, int device, pp_corr_graph_handle* out) try {
  const char* where = "pp_corr_graph_create";
  PP_REQUIRE(out, "%s: null argument", where);
  *out = nullptr;
  PP_REQUIRE(num_images >= 0 && (num_images == 0 || num_lines), "%s: bad argument", where);
  int64_t total = 0;
  for (int32_t k = 0; k < num_images; ++k) {
    PP_REQUIRE(num_lines[k] >= 0, "%s: image %d has a negative line count", where, k);
    total += num_lines[k];
  }
  PP_REQUIRE(total < 0x7FFFFFFFll - kScanTile, "%s: too many lines", where);
  PP_TRY(UseDevice(where, device));
  UnderConstruction<pp_corr_graph_impl, pp_corr_graph_destroy> h{new pp_corr_graph_impl()};
  h->num_images = num_images;
  h->num_lines.assign(num_lines, num_lines + num_images);
  h->line_start.assign((size_t)num_images + 1, 0);
  for (int32_t k = 0; k < num_images; ++k) h->line_start[(size_t)k + 1] = h->line_start[(size_t)k] + num_lines[k];
  PP_TRY(h->Open(device));
  PP_TRY(h->blocks.Put(&h->d_line_start, h->line_start.data(), h->line_start.size(), h->stream, 1));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  *out = h.release();
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_create")

int pp_corr_graph_build(pp_corr_graph_handle h, int32_t min_num_matches, int64_t num_pairs, const int32_t* pairs, const int64_t* match_start,
                        const int32_t* matches, pp_corr_graph_report* report) try {
  const char* where = "pp_corr_graph_build";
  PP_REQUIRE(h && match_start && report, "%s: null argument", where);
  PP_REQUIRE(num_pairs >= 0 && num_pairs < 0x7FFFFFFFll && (num_pairs == 0 || pairs), "%s: bad argument", where);
  const auto t_begin = Clock::now();
  std::vector<CorrPairPlan> plan;
  std::vector<uint8_t> connected;
  int64_t num_ranked = 0;
  const std::string wrong = CorrPlanPairs(h->num_images, min_num_matches, num_pairs, pairs, match_start, &plan, &connected, &num_ranked);
  PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  const int64_t M = match_start[num_pairs], L = h->NumLines();
  PP_REQUIRE(M < 0x7FFFFFFFll - kCorrBlock, "%s: too many matches", where);
  PP_REQUIRE(M == 0 || matches, "%s: null matches", where);

  std::vector<CorrPairDev> dev((size_t)num_pairs);
  std::vector<CorrWork> work;
  int64_t pairs_used = 0;
  for (int64_t p = 0; p < num_pairs; ++p) {
    const CorrPairPlan& q = plan[(size_t)p];
    dev[(size_t)p] = CorrPairDev{q.swapped, q.rank, h->num_lines[(size_t)q.image1], h->num_lines[(size_t)q.image2], h->line_start[(size_t)q.image1],
                                 h->line_start[(size_t)q.image2]};
    pairs_used += q.used;
    if (q.rank < 0) continue;
    const int32_t tiles = CeilDiv(std::max(dev[(size_t)p].n1, dev[(size_t)p].n2), kCorrTile);
    for (int32_t t = 0; t < tiles; ++t) work.push_back(CorrWork{(int32_t)p, t});
  }
  PP_REQUIRE(work.size() < 0x7FFFFFFFull, "%s: too many (pair, tile) work items", where);

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  CorrFresh fresh{&h->blocks};
  CallScratch cb(s);
  CorrPairDev* d_plan = nullptr;
  CorrWork* d_work = nullptr;
  int64_t* d_mstart = nullptr;
  int32_t *d_matches = nullptr, *d_cls = nullptr, *d_pair_of = nullptr, *d_degree = nullptr, *d_pair_acc = nullptr, *d_scan = nullptr, *d_cursor = nullptr;
  int32_t *d_slot_rank = nullptr, *d_slot_line = nullptr, *d_slot_owner = nullptr, *d_img_obs = nullptr, *d_img_corr = nullptr;
  uint8_t *d_dup1 = nullptr, *d_dup2 = nullptr, *d_acc = nullptr;
  PP_TRY(cb.Put(&d_plan, dev.data(), dev.size())); PP_TRY(cb.Put(&d_work, work.data(), work.size()));
  PP_TRY(cb.Put(&d_mstart, match_start, (size_t)num_pairs + 1)); PP_TRY(cb.Put(&d_matches, matches, 2 * (size_t)M));
  PP_TRY(cb.Zeros(&d_cls, 3 * (size_t)num_pairs)); PP_TRY(cb.Zeros(&d_pair_acc, (size_t)num_pairs));
  PP_TRY(cb.Zeros(&d_dup1, (size_t)M)); PP_TRY(cb.Zeros(&d_dup2, (size_t)M)); PP_TRY(cb.Zeros(&d_acc, (size_t)M));
  PP_TRY(cb.Alloc(&d_pair_of, (size_t)M));
  PP_TRY(cb.Zeros(&d_degree, (size_t)L + 1)); PP_TRY(cb.Alloc(&d_scan, ScanScratchCount(L))); PP_TRY(cb.Alloc(&d_cursor, (size_t)L + 1));
  PP_TRY(cb.Alloc(&d_img_obs, (size_t)h->num_images)); PP_TRY(cb.Alloc(&d_img_corr, (size_t)h->num_images));
  PP_TRY(h->blocks.Alloc(&fresh.start, (size_t)L + 1));

  StreamTimer timer(*h);
  double replay_ms = 0.0;
  PP_TRY(timer.Begin());
  if (!work.empty())
    hipLaunchKernelGGL(k_corr_first, dim3((unsigned)work.size()), dim3(kCorrBlock), 0, s, (const CorrWork*)d_work, (const CorrPairDev*)d_plan,
                       (const int64_t*)d_mstart, (const int32_t*)d_matches, d_dup1, d_dup2, d_cls);
  if (M > 0)
    hipLaunchKernelGGL(k_corr_accept, dim3(CeilDiv(M, kCorrBlock)), dim3(kCorrBlock), 0, s, M, (int32_t)num_pairs, (const CorrPairDev*)d_plan,
                       (const int64_t*)d_mstart, (const int32_t*)d_matches, (const uint8_t*)d_dup1, (const uint8_t*)d_dup2, d_pair_of, d_acc);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  std::vector<int32_t> cls(3 * (size_t)num_pairs, 0);
  PP_TRY(Download(cls.data(), d_cls, cls.size(), s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());

  // the pairs the parallel rule is not the greedy one for: the literal loop, its flags over the device's
  int64_t replayed = 0, bad_index = 0, in_graph_pairs = 0;
  {
    const auto t_replay = Clock::now();
    std::vector<std::vector<uint8_t>> flags;
    std::vector<int32_t> stored;
    for (int64_t p = 0; p < num_pairs; ++p) {
      if (plan[(size_t)p].rank < 0) continue;
      in_graph_pairs += match_start[p + 1] - match_start[p];
      bad_index += cls[3 * (size_t)p + 2];
      if (!CorrNeedsReplay(cls[3 * (size_t)p], cls[3 * (size_t)p + 1])) continue;
      const int64_t m0 = match_start[p], cnt = match_start[p + 1] - m0;
      stored.assign(matches + 2 * m0, matches + 2 * (m0 + cnt));
      if (plan[(size_t)p].swapped)
        for (int64_t m = 0; m < cnt; ++m) std::swap(stored[2 * (size_t)m], stored[2 * (size_t)m + 1]);
      flags.emplace_back((size_t)cnt);
      CorrReplayPair(dev[(size_t)p].n1, dev[(size_t)p].n2, stored.data(), cnt, flags.back().data());
      PP_TRY(Upload(d_acc + m0, (const uint8_t*)flags.back().data(), (size_t)cnt, s));
      ++replayed;
    }
    if (replayed) PP_HIP_TRY(hipStreamSynchronize(s));
    replay_ms = MsSince(t_replay);
  }

  PP_TRY(timer.Begin());
  if (M > 0)
    hipLaunchKernelGGL(k_corr_count, dim3(CeilDiv(M, kCorrBlock)), dim3(kCorrBlock), 0, s, M, (const CorrPairDev*)d_plan, (const int32_t*)d_matches,
                       (const int32_t*)d_pair_of, (const uint8_t*)d_acc, d_degree, d_pair_acc);
  const ScanJob<int32_t> degrees{d_degree, fresh.start, fresh.start + L};
  LaunchExclusiveScan(s, L, &degrees, 1, d_scan);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  std::vector<int32_t> pair_acc((size_t)num_pairs, 0);
  PP_TRY(Download(pair_acc.data(), d_pair_acc, pair_acc.size(), s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  int64_t accepted = 0;
  for (int64_t p = 0; p < num_pairs; ++p) accepted += pair_acc[(size_t)p];
  // (2 * accepted <= 2 * M < 2^32: the degrees cannot have wrapped past a positive int32 total unnoticed - the check is on the exact count)
  PP_REQUIRE(2 * accepted <= 0x7FFFFFFFll, "%s: %lld accepted matches, the CSR would need %lld int32 entries", where, (long long)accepted, (long long)(2 * accepted));
  const int64_t E = 2 * accepted;

  PP_TRY(h->blocks.Alloc(&fresh.line, (size_t)E));
  PP_TRY(cb.Alloc(&d_slot_rank, (size_t)E)); PP_TRY(cb.Alloc(&d_slot_line, (size_t)E)); PP_TRY(cb.Alloc(&d_slot_owner, (size_t)E));
  PP_TRY(timer.Begin());
  if (E > 0) {
    PP_HIP_TRY(hipMemcpyAsync(d_cursor, fresh.start, ((size_t)L + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_corr_scatter, dim3(CeilDiv(M, kCorrBlock)), dim3(kCorrBlock), 0, s, M, E, (const CorrPairDev*)d_plan, (const int32_t*)d_matches,
                       (const int32_t*)d_pair_of, (const uint8_t*)d_acc, d_cursor, d_slot_rank, d_slot_line, d_slot_owner);
    hipLaunchKernelGGL(k_corr_order, dim3(CeilDiv(E, kCorrBlock)), dim3(kCorrBlock), 0, s, E, (const int32_t*)fresh.start, (const int32_t*)d_slot_rank,
                       (const int32_t*)d_slot_line, (const int32_t*)d_slot_owner, fresh.line);
  }
  if (h->num_images > 0)
    hipLaunchKernelGGL(k_corr_image, dim3((unsigned)h->num_images), dim3(kCorrBlock), 0, s, (const int32_t*)h->d_line_start, (const int32_t*)fresh.start,
                       d_img_obs, d_img_corr);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  std::vector<int32_t> img_obs((size_t)h->num_images, 0), img_corr((size_t)h->num_images, 0);
  int32_t total_entries = -1;
  PP_TRY(Download(img_obs.data(), d_img_obs, img_obs.size(), s)); PP_TRY(Download(img_corr.data(), d_img_corr, img_corr.size(), s));
  PP_TRY(Download(&total_entries, fresh.start + L, 1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());
  if ((int64_t)total_entries != E) { SetLastError("%s: the degrees sum to %d, the accepted matches to %lld entries", where, total_entries, (long long)E); return PP_ERR_INTERNAL; }

  // the build is complete: it replaces the handle's graph
  if (h->d_corr_start) h->blocks.Free(&h->d_corr_start);
  if (h->d_corr_line) h->blocks.Free(&h->d_corr_line);
  h->d_corr_start = fresh.start; h->d_corr_line = fresh.line; fresh.keep = true;
  h->num_entries = E; h->built = true;
  h->connected.swap(connected); h->image_observations.swap(img_obs); h->image_correspondences.swap(img_corr); h->pair_correspondences.swap(pair_acc);
  std::memset(report, 0, sizeof(*report));
  report->num_pairs_used = pairs_used; report->num_pairs_ignored = num_pairs - pairs_used;
  report->num_matches_in = M; report->num_matches_accepted = accepted; report->num_matches_bad_index = bad_index;
  report->num_matches_duplicate = in_graph_pairs - bad_index - accepted;
  report->num_pairs_replayed = replayed;
  report->device_ms = timer.ms; report->replay_ms = replay_ms; report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_build")

int pp_corr_graph_num_entries(pp_corr_graph_handle h, int64_t* num_lines, int64_t* num_entries) try {
  const char* where = "pp_corr_graph_num_entries";
  PP_REQUIRE(h, "%s: null handle", where);
  PP_REQUIRE(h->built, "%s: no graph has been built", where);
  if (num_lines) *num_lines = h->NumLines();
  if (num_entries) *num_entries = h->num_entries;
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_num_entries")

int pp_corr_graph_get(pp_corr_graph_handle h, int32_t* corr_start, int32_t* corr_line, int64_t capacity, uint8_t* image_connected, int32_t* image_num_observations,
                      int32_t* image_num_correspondences) try {
  const char* where = "pp_corr_graph_get";
  PP_REQUIRE(h, "%s: null handle", where);
  PP_REQUIRE(h->built, "%s: no graph has been built", where);
  PP_REQUIRE(!corr_line || capacity >= h->num_entries, "%s: %lld entries, capacity is %lld", where, (long long)h->num_entries, (long long)capacity);
  if (corr_start || corr_line) {
    PP_HIP_TRY(hipSetDevice(h->device));
    if (corr_start) PP_TRY(Download(corr_start, h->d_corr_start, (size_t)h->NumLines() + 1, h->stream));
    if (corr_line) PP_TRY(Download(corr_line, h->d_corr_line, (size_t)h->num_entries, h->stream));
    PP_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (image_connected) std::copy(h->connected.begin(), h->connected.end(), image_connected);
  if (image_num_observations) std::copy(h->image_observations.begin(), h->image_observations.end(), image_num_observations);
  if (image_num_correspondences) std::copy(h->image_correspondences.begin(), h->image_correspondences.end(), image_num_correspondences);
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_get")

int pp_corr_graph_pair_counts(pp_corr_graph_handle h, int32_t* pair_num_correspondences) try {
  const char* where = "pp_corr_graph_pair_counts";
  PP_REQUIRE(h && pair_num_correspondences, "%s: null argument", where);
  PP_REQUIRE(h->built, "%s: no graph has been built", where);
  std::copy(h->pair_correspondences.begin(), h->pair_correspondences.end(), pair_num_correspondences);
  return PP_OK;
} PP_API_CATCH("pp_corr_graph_pair_counts")

}  // extern "C"
