// K20 - image-pair selection: which image pairs the matcher is given.  The spatial selection of SpatialFeatureMatcher::Run (reference
// src/feature/matching.cc:705-768: an exact k-nearest-neighbour search over all image locations) and one iteration of TransitiveFeatureMatcher::Run
// (:818-869: the two-hop neighbourhood of every image in the match graph, without the pairs already tried).  The rules, the argument checks and a literal
// host version of both are in pair_selection_replay.hpp; this file is the device half and the C ABI.  Both results are a fixed function of the input:
// atomics are used for integer counts, for an order-free OR / AND-NOT on a bitmap and to hand out slots of a list that is sorted before it is written.
// Spatial, m locations, knn = min(max_num_neighbors, m); key(q, j) = float bits of the unfused squared distance << 32 | j (SpatialKey):
// K20a k_spatial_count   one workgroup per query: F = the candidates within max_distance, Z = those of them in front of the query itself; the query
//                        gives min(knn, F) pairs, one fewer when it is among its own first knn (Z < knn).
// K20b                   the exclusive scan of the counts (int64: the total is checked against 2^31 before anything is written).
// K20c k_spatial_fill    one workgroup per query, the candidates in rounds of kSpatialRound = 256 ranks: a radix select over the recomputed keys (8 bits a
//                        pass; the passes over index bits no index has are skipped) finds the round's last key, one more pass collects the keys of the
//                        round into LDS, a bitonic sort orders them, the query is left out.  max_num_neighbors <= 256 is one round - the fast path; a larger
//                        one repeats the round from the last key on, ceil(knn / 256) times 6 to 9 passes over the locations.
// Transitive, N images; adjacency as CSR of the matched pairs, and of the tried ones with the matched among them:
// K20d k_pairs_degree / scan / k_pairs_scatter   the two CSRs; the order inside a list is the atomics' and reaches nothing.
// K20e k_transitive<false>   one workgroup per image a: the images c > a two hops away are marked in an LDS bitmap of kTransChunk = 32768 positions (more
//                        images: one chunk after the other), a wavefront per neighbour b and a lane per neighbour of b, so that a hub's list is read by 64
//                        lanes; the tried neighbours of a are cleared; the set bits are counted.
// K20f                   the exclusive scan of the counts.
// K20g k_transitive<true>    the same walk, the set bits written in ascending order from the image's offset: (a, c) ascending.
#include <cstring>

#include "pair_selection_replay.hpp"
#include "device_handle.hpp"
#include "scan.hpp"

namespace ppsfm {

constexpr int kPairsBlock = 256;
constexpr int kSpatialRound = 256;                 // ranks per round of k_spatial_fill: the keys one LDS sort takes
constexpr int kTransChunk = 32768;                 // image positions per LDS bitmap of k_transitive
constexpr int kTransWords = kTransChunk / 32;
static_assert(kSpatialRound == kPairsBlock && kTransWords == 4 * kPairsBlock, "one key, and four bitmap words, per thread");

// pair_selection_replay.hpp's SpatialKey(SpatialSqDist(q, xyz[j]), j)
__device__ __forceinline__ uint64_t SpatialKeyDevice(const float* __restrict__ xyz, float qx, float qy, float qz, int32_t j) {
  // Plain operators under the pragma: the operations written HERE carry no permission to contract.  (__fmul_rn / __fadd_rn are inline functions of the
  // toolchain's header that are compiled under the unit's default, contraction allowed - called from here they were fused all the same.)
#pragma clang fp contract(off)
  const float d0 = qx - xyz[3 * (int64_t)j], d1 = qy - xyz[3 * (int64_t)j + 1], d2 = qz - xyz[3 * (int64_t)j + 2];
  const float s = ((d0 * d0) + d1 * d1) + d2 * d2;
  return ((uint64_t)__float_as_uint(s) << 32) | (uint32_t)j;
}
__device__ __forceinline__ bool SpatialWithin(uint64_t key, float cut) { return !(__uint_as_float((uint32_t)(key >> 32)) > cut); }

__global__ __launch_bounds__(kPairsBlock) void k_spatial_count(int32_t m, int32_t knn, float cut, const float* __restrict__ xyz, int64_t* __restrict__ count) {
  __shared__ int32_t red[2];
  const int tid = threadIdx.x;
  const int32_t q = blockIdx.x;
  const float qx = xyz[3 * (int64_t)q], qy = xyz[3 * (int64_t)q + 1], qz = xyz[3 * (int64_t)q + 2];
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  const uint64_t self = SpatialKeyDevice(xyz, qx, qy, qz, q);
  int f = 0, z = 0;
  for (int32_t j = tid; j < m; j += kPairsBlock) {
    const uint64_t key = SpatialKeyDevice(xyz, qx, qy, qz, j);
    if (SpatialWithin(key, cut)) { ++f; z += key < self; }
  }
  f = WaveSumInt(f); z = WaveSumInt(z);
  if ((tid & 63) == 0) { atomicAdd(&red[0], f); atomicAdd(&red[1], z); }
  __syncthreads();
  if (tid == 0) count[q] = (int64_t)(red[0] < knn ? red[0] : knn) - (red[1] < knn ? 1 : 0);
}

__global__ __launch_bounds__(kPairsBlock) void k_spatial_fill(int32_t m, int32_t knn, float cut, const float* __restrict__ xyz, const int64_t* __restrict__ offset,
                                                              int32_t* __restrict__ pairs, float* __restrict__ sqdist) {
  __shared__ uint64_t keys[kSpatialRound];
  __shared__ int32_t hist[256];
  __shared__ int32_t wave_total[kPairsBlock / kWave];
  __shared__ int32_t chosen[2];      // the digit the wanted rank falls in, and the rank inside it
  __shared__ int32_t kept;
  const int tid = threadIdx.x;
  const int32_t q = blockIdx.x;
  const float qx = xyz[3 * (int64_t)q], qy = xyz[3 * (int64_t)q + 1], qz = xyz[3 * (int64_t)q + 2];
  int64_t out = offset[q];
  const int64_t end = offset[q + 1];
  if (out == end) return;            // (the whole workgroup)
  uint64_t after = 0;               // the last key of the round before
  bool first = true;
  for (int32_t base = 0; base < knn; base += kSpatialRound) {
    // the key of rank r among the candidates within the distance and behind `after`
    int32_t r = knn - base < kSpatialRound ? knn - base : kSpatialRound;
    uint64_t last = 0;
    bool rest = false;               // fewer than r are left: the round takes them all
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (shift < 32 && ((uint32_t)(m - 1) >> shift) == 0) continue;      // no index has a bit here
      const uint64_t above = shift == 56 ? 0ull : ~0ull << (shift + 8);
      hist[tid] = 0;
      __syncthreads();
      for (int32_t j = tid; j < m; j += kPairsBlock) {
        const uint64_t key = SpatialKeyDevice(xyz, qx, qy, qz, j);
        if (SpatialWithin(key, cut) && (first || key > after) && ((key ^ last) & above) == 0) atomicAdd(&hist[(int)((key >> shift) & 0xFF)], 1);
      }
      __syncthreads();
      const int32_t mine = hist[tid];
      int32_t all;
      const int32_t below = BlockExclusiveScan<kPairsBlock>(mine, wave_total, &all);
      if (shift == 56 && all < r) { rest = true; break; }
      if (below < r && r <= below + mine) { chosen[0] = tid; chosen[1] = r - below; }
      __syncthreads();
      last |= (uint64_t)chosen[0] << shift;
      r = chosen[1];
    }
    if (rest) last = ~0ull;
    if (tid == 0) kept = 0;
    keys[tid] = ~0ull;
    __syncthreads();
    for (int32_t j = tid; j < m; j += kPairsBlock) {
      const uint64_t key = SpatialKeyDevice(xyz, qx, qy, qz, j);
      if (j != q && SpatialWithin(key, cut) && (first || key > after) && key <= last) {
        const int32_t slot = atomicAdd(&kept, 1);
        if (slot < kSpatialRound) keys[slot] = key;
      }
    }
    __syncthreads();
    const int32_t n = kept < kSpatialRound ? kept : kSpatialRound;
    for (int k = 2; k <= kSpatialRound; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        const int other = tid ^ j;
        if (other > tid) {
          const uint64_t x = keys[tid], y = keys[other];
          if ((x > y) == ((tid & k) == 0)) { keys[tid] = y; keys[other] = x; }
        }
        __syncthreads();
      }
    if (tid < n && out + tid < end) {
      const uint64_t key = keys[tid];
      pairs[2 * (out + tid)] = q; pairs[2 * (out + tid) + 1] = (int32_t)(uint32_t)key;
      sqdist[out + tid] = __uint_as_float((uint32_t)(key >> 32));
    }
    out += n; after = last; first = false;
    if (rest) break;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPairsBlock) void k_pairs_degree(int64_t n, const int32_t* __restrict__ pairs, int32_t* __restrict__ degree) {
  const int64_t p = (int64_t)blockIdx.x * kPairsBlock + threadIdx.x;
  if (p >= n) return;
  atomicAdd(&degree[pairs[2 * p]], 1); atomicAdd(&degree[pairs[2 * p + 1]], 1);
}

__global__ __launch_bounds__(kPairsBlock) void k_pairs_scatter(int64_t n, const int32_t* __restrict__ pairs, int32_t* __restrict__ cursor, int32_t* __restrict__ adj) {
  const int64_t p = (int64_t)blockIdx.x * kPairsBlock + threadIdx.x;
  if (p >= n) return;
  const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
  const int32_t sa = atomicAdd(&cursor[a], 1), sb = atomicAdd(&cursor[b], 1);
  if ((int64_t)sa < 2 * n) adj[sa] = b;
  if ((int64_t)sb < 2 * n) adj[sb] = a;
}

template <bool kFill>
__global__ __launch_bounds__(kPairsBlock) void k_transitive(int32_t num_images, const int32_t* __restrict__ mstart, const int32_t* __restrict__ madj,
                                                            const int32_t* __restrict__ tstart, const int32_t* __restrict__ tadj, int64_t* __restrict__ count,
                                                            const int64_t* __restrict__ offset, int32_t* __restrict__ pairs) {
  __shared__ uint32_t bits[kTransWords];
  __shared__ int32_t wave_total[kPairsBlock / kWave];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t a = blockIdx.x;
  const int32_t a0 = mstart[a], a1 = mstart[a + 1];
  if (a0 == a1) {      // (the whole workgroup)
    if (!kFill && tid == 0) count[a] = 0;
    return;
  }
  const int32_t t0 = tstart[a], t1 = tstart[a + 1];
  int64_t out = kFill ? offset[a] : 0, total = 0;
  const int64_t end = kFill ? offset[a + 1] : 0;
  if (kFill && out == end) return;
  for (int64_t c0 = (int64_t)((a + 1) / kTransChunk) * kTransChunk; c0 < num_images; c0 += kTransChunk) {
    for (int k = tid; k < kTransWords; k += kPairsBlock) bits[k] = 0;
    __syncthreads();
    for (int32_t i = a0 + wave; i < a1; i += kPairsBlock / kWave) {
      const int32_t b = madj[i];
      const int32_t b1 = mstart[b + 1];
      for (int32_t k = mstart[b] + lane; k < b1; k += kWave) {
        const int32_t c = madj[k];
        const int64_t rel = c - c0;
        if (c > a && rel >= 0 && rel < kTransChunk) atomicOr(&bits[rel >> 5], 1u << (rel & 31));
      }
    }
    __syncthreads();
    for (int32_t k = t0 + tid; k < t1; k += kPairsBlock) {
      const int64_t rel = tadj[k] - c0;
      if (rel >= 0 && rel < kTransChunk) atomicAnd(&bits[rel >> 5], ~(1u << (rel & 31)));
    }
    __syncthreads();
    uint32_t word[4];
    int32_t n = 0, all;
#pragma unroll
    for (int w = 0; w < 4; ++w) { word[w] = bits[4 * tid + w]; n += __popc(word[w]); }
    const int32_t below = BlockExclusiveScan<kPairsBlock>(n, wave_total, &all);
    if (kFill) {
      int64_t p = out + below;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        for (uint32_t rest = word[w]; rest; rest &= rest - 1, ++p)
          if (p < end) { pairs[2 * p] = a; pairs[2 * p + 1] = (int32_t)(c0 + 32 * (4 * tid + w) + (__ffs(rest) - 1)); }
      out += all;
    } else {
      total += all;
    }
    __syncthreads();
  }
  if (!kFill && tid == 0) count[a] = total;
}

}  // namespace ppsfm

struct pp_pairs_impl : ppsfm::DeviceHandle {      // blocks: the last result
  int64_t num_pairs = 0;
  int32_t* d_pairs = nullptr;      // num_pairs x 2
  float* d_sqdist = nullptr;       // num_pairs; null after a transitive selection
  bool has_sqdist = false;
};

using namespace ppsfm;

namespace {

// a result in the handle's blocks: given back unless the call completes
struct PairsFresh {
  DeviceBlocks* b;
  int32_t* pairs = nullptr;
  float* sqdist = nullptr;
  bool keep = false;
  ~PairsFresh() {
    if (keep) return;
    if (pairs) b->Free(&pairs);
    if (sqdist) b->Free(&sqdist);
  }
};

// the completed call's result replaces the handle's
void PairsAdopt(pp_pairs_impl* h, PairsFresh* fresh, int64_t n, bool has_sqdist) {
  if (h->d_pairs) h->blocks.Free(&h->d_pairs);
  if (h->d_sqdist) h->blocks.Free(&h->d_sqdist);
  h->d_pairs = fresh->pairs; h->d_sqdist = fresh->sqdist; fresh->keep = true;
  h->num_pairs = n; h->has_sqdist = has_sqdist;
}

// stops the clock of one device stage and reads the total behind the scanned counts
int PairsStageTotal(StreamTimer* timer, const int64_t* d_total, int64_t* total) {
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer->End());
  if (d_total) PP_TRY(Download(total, d_total, 1, timer->stream));
  PP_HIP_TRY(hipStreamSynchronize(timer->stream));
  return timer->Add();
}

}  // namespace

extern "C" {

int pp_pairs_destroy(pp_pairs_handle h) try {
  delete h;      // (~DeviceHandle)
  return PP_OK;
} PP_API_CATCH("pp_pairs_destroy")

int pp_pairs_create(int device, pp_pairs_handle* out) try {
  const char* where = "pp_pairs_create";
  PP_REQUIRE(out, "%s: null argument", where);
  *out = nullptr;
  PP_TRY(UseDevice(where, device));
  UnderConstruction<pp_pairs_impl, pp_pairs_destroy> h{new pp_pairs_impl()};
  PP_TRY(h->Open(device));
  *out = h.release();
  return PP_OK;
} PP_API_CATCH("pp_pairs_create")

int pp_pairs_spatial(pp_pairs_handle h, int64_t num_locations, const float* xyz, int32_t max_num_neighbors, double max_distance, pp_pairs_report* report) try {
  const char* where = "pp_pairs_spatial";
  PP_REQUIRE(h && report, "%s: null argument", where);
  const auto t_begin = Clock::now();
  const std::string wrong = PairsCheckSpatial(num_locations, xyz, max_num_neighbors, max_distance);
  PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  const int32_t m = (int32_t)num_locations, knn = (int32_t)std::min<int64_t>(max_num_neighbors, num_locations);
  const float cut = SpatialMaxSqDist(max_distance);

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  PairsFresh fresh{&h->blocks};
  CallScratch cb(s);
  float* d_xyz = nullptr;
  int64_t *d_count = nullptr, *d_offset = nullptr, *d_scan = nullptr;
  int64_t total = 0;
  StreamTimer timer(*h);
  if (m > 0) {
    PP_TRY(cb.Put(&d_xyz, xyz, 3 * (size_t)m));
    PP_TRY(cb.Alloc(&d_count, (size_t)m)); PP_TRY(cb.Alloc(&d_offset, (size_t)m + 1)); PP_TRY(cb.Alloc(&d_scan, ScanScratchCount(m)));
    PP_TRY(timer.Begin());
    hipLaunchKernelGGL(k_spatial_count, dim3((unsigned)m), dim3(kPairsBlock), 0, s, m, knn, cut, (const float*)d_xyz, d_count);
    const ScanJob<int64_t> counts{d_count, d_offset, d_offset + m};
    LaunchExclusiveScan(s, (int64_t)m, &counts, 1, d_scan);
    PP_TRY(PairsStageTotal(&timer, d_offset + m, &total));
    PP_REQUIRE(total >= 0 && total < kPairsMaxResult, "%s: %lld pairs, the result is limited to 2^31 - 1", where, (long long)total);
    PP_TRY(h->blocks.Alloc(&fresh.pairs, 2 * (size_t)total)); PP_TRY(h->blocks.Alloc(&fresh.sqdist, (size_t)total));
    if (total > 0) {
      PP_TRY(timer.Begin());
      hipLaunchKernelGGL(k_spatial_fill, dim3((unsigned)m), dim3(kPairsBlock), 0, s, m, knn, cut, (const float*)d_xyz, (const int64_t*)d_offset, fresh.pairs,
                         fresh.sqdist);
      PP_TRY(PairsStageTotal(&timer, nullptr, nullptr));
    }
  }
  PairsAdopt(h, &fresh, total, true);
  std::memset(report, 0, sizeof(*report));
  report->num_pairs = total; report->num_candidates = (int64_t)m * m;
  report->device_ms = timer.ms; report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_pairs_spatial")

int pp_pairs_transitive(pp_pairs_handle h, int32_t num_images, int64_t num_matched, const int32_t* matched_pairs, int64_t num_tried, const int32_t* tried_pairs,
                        pp_pairs_report* report) try {
  const char* where = "pp_pairs_transitive";
  PP_REQUIRE(h && report, "%s: null argument", where);
  const auto t_begin = Clock::now();
  const std::string wrong = PairsCheckTransitive(num_images, num_matched, matched_pairs, num_tried, tried_pairs);
  PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  const int64_t N = num_images, M = num_matched, T = num_matched + num_tried;

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  PairsFresh fresh{&h->blocks};
  CallScratch cb(s);
  int64_t total = 0;
  StreamTimer timer(*h);
  if (N > 0 && M > 0) {
    // the matched pairs first, the tried ones behind them: the first M make the adjacency, all T the pairs that are done
    std::vector<int32_t> listed(2 * (size_t)T);
    std::copy(matched_pairs, matched_pairs + 2 * M, listed.begin());
    if (num_tried > 0) std::copy(tried_pairs, tried_pairs + 2 * num_tried, listed.begin() + 2 * M);
    int32_t *d_listed = nullptr, *d_degree = nullptr, *d_start = nullptr, *d_cursor = nullptr, *d_madj = nullptr, *d_tadj = nullptr, *d_scan32 = nullptr;
    int64_t *d_count = nullptr, *d_offset = nullptr, *d_scan = nullptr;
    PP_TRY(cb.Put(&d_listed, listed.data(), listed.size()));
    PP_TRY(cb.Zeros(&d_degree, 2 * (size_t)N)); PP_TRY(cb.Alloc(&d_start, 2 * ((size_t)N + 1))); PP_TRY(cb.Alloc(&d_cursor, 2 * ((size_t)N + 1)));
    PP_TRY(cb.Alloc(&d_scan32, 2 * ScanScratchCount(N)));
    PP_TRY(cb.Alloc(&d_madj, 2 * (size_t)M)); PP_TRY(cb.Alloc(&d_tadj, 2 * (size_t)T));
    PP_TRY(cb.Alloc(&d_count, (size_t)N)); PP_TRY(cb.Alloc(&d_offset, (size_t)N + 1)); PP_TRY(cb.Alloc(&d_scan, ScanScratchCount(N)));
    int32_t *d_mstart = d_start, *d_tstart = d_start + N + 1;
    PP_TRY(timer.Begin());
    hipLaunchKernelGGL(k_pairs_degree, dim3(CeilDiv(M, kPairsBlock)), dim3(kPairsBlock), 0, s, M, (const int32_t*)d_listed, d_degree);
    hipLaunchKernelGGL(k_pairs_degree, dim3(CeilDiv(T, kPairsBlock)), dim3(kPairsBlock), 0, s, T, (const int32_t*)d_listed, d_degree + N);
    const ScanJob<int32_t> degrees[2] = {{d_degree, d_mstart, d_mstart + N}, {d_degree + N, d_tstart, d_tstart + N}};
    LaunchExclusiveScan(s, N, degrees, 2, d_scan32);
    PP_HIP_TRY(hipMemcpyAsync(d_cursor, d_start, 2 * ((size_t)N + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_pairs_scatter, dim3(CeilDiv(M, kPairsBlock)), dim3(kPairsBlock), 0, s, M, (const int32_t*)d_listed, d_cursor, d_madj);
    hipLaunchKernelGGL(k_pairs_scatter, dim3(CeilDiv(T, kPairsBlock)), dim3(kPairsBlock), 0, s, T, (const int32_t*)d_listed, d_cursor + N + 1, d_tadj);
    hipLaunchKernelGGL(k_transitive<false>, dim3((unsigned)N), dim3(kPairsBlock), 0, s, num_images, (const int32_t*)d_mstart, (const int32_t*)d_madj,
                       (const int32_t*)d_tstart, (const int32_t*)d_tadj, d_count, (const int64_t*)nullptr, (int32_t*)nullptr);
    const ScanJob<int64_t> counts{d_count, d_offset, d_offset + N};
    LaunchExclusiveScan(s, N, &counts, 1, d_scan);
    PP_TRY(PairsStageTotal(&timer, d_offset + N, &total));
    PP_REQUIRE(total >= 0 && total < kPairsMaxResult, "%s: %lld pairs, the result is limited to 2^31 - 1", where, (long long)total);
    PP_TRY(h->blocks.Alloc(&fresh.pairs, 2 * (size_t)total));
    if (total > 0) {
      PP_TRY(timer.Begin());
      hipLaunchKernelGGL(k_transitive<true>, dim3((unsigned)N), dim3(kPairsBlock), 0, s, num_images, (const int32_t*)d_mstart, (const int32_t*)d_madj,
                         (const int32_t*)d_tstart, (const int32_t*)d_tadj, (int64_t*)nullptr, (const int64_t*)d_offset, fresh.pairs);
      PP_TRY(PairsStageTotal(&timer, nullptr, nullptr));
    }
  }
  PairsAdopt(h, &fresh, total, false);
  std::memset(report, 0, sizeof(*report));
  report->num_pairs = total; report->num_candidates = TransitiveVisited(num_images, num_matched, matched_pairs);
  report->device_ms = timer.ms; report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_pairs_transitive")

int pp_pairs_num(pp_pairs_handle h, int64_t* n) try {
  const char* where = "pp_pairs_num";
  PP_REQUIRE(h && n, "%s: null argument", where);
  *n = h->num_pairs;
  return PP_OK;
} PP_API_CATCH("pp_pairs_num")

int pp_pairs_get(pp_pairs_handle h, int32_t* pairs, float* sqdist, int64_t capacity) try {
  const char* where = "pp_pairs_get";
  PP_REQUIRE(h, "%s: null handle", where);
  PP_REQUIRE(capacity >= h->num_pairs, "%s: %lld pairs, capacity is %lld", where, (long long)h->num_pairs, (long long)capacity);
  PP_REQUIRE(!sqdist || h->has_sqdist || h->num_pairs == 0, "%s: the last selection has no distances", where);
  if (h->num_pairs == 0 || (!pairs && !sqdist)) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  if (pairs) PP_TRY(Download(pairs, h->d_pairs, 2 * (size_t)h->num_pairs, h->stream));
  if (sqdist) PP_TRY(Download(sqdist, h->d_sqdist, (size_t)h->num_pairs, h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
} PP_API_CATCH("pp_pairs_get")

}  // extern "C"
