// K17 - SIFT descriptor matching: MatchSiftFeaturesCPUBruteForce (reference src/feature/sift.cc:54-143, 170-203, 957-970) for a list of image pairs, exact.
// The rule and its integer thresholds are in sift_match_replay.hpp, the handle in sift_match_handle.hpp (sift_extract.hip fills one too); this file is
// the device half and the C ABI.
//   dist(i, j) = d1[i] . d2[j] over 128 uint8.  The gfx950 i8 MFMA is signed, so a handle keeps d' = d - 128 (the same byte with its top bit flipped) and, per
//   row, off = 128 * sum(d') + 2^20 = 128 * sum(d) - 2^20:   dist = d1' . d2' + off1 + off2   (128^3 = 2^21 split over the two sides), exact in int32 - the
//   signed product stays below 2^21.
// K17a k_sift_top2     one workgroup (4 wavefronts) per (pair, direction, tile of 128 query rows).  Each wavefront keeps 32 query rows resident as the B
//                      operand of v_mfma_i32_32x32x32_i8 (4 k-steps x 16 bytes per lane) and the workgroup walks the other image in tiles of 64 rows staged in
//                      LDS (rows padded to 144 bytes; two buffers, the next tile fetched while this one is multiplied), read as the A operand.  A and B fragments are loaded the same way - lane (r, h) takes bytes
//                      32 s + 16 h .. + 15 of row r at k-step s - so the instruction's k order inside a step does not matter: the sum runs over all of k.
//                      The result tile has the QUERY row on the lane (C column = lane & 31) and the scanned rows in the 16 registers
//                      (C row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), ascending in reg: every lane runs the reference's sequential scan over its
//                      share of the columns in ascending order and keeps ONE (best, best_j, second).  The scanned rows' offsets enter as the accumulator's
//                      initial value; a row past the end of the scanned image gets an offset of -2^30, which keeps it below a dist of 0 whatever its bytes
//                      are.  At the end the two lane halves are merged: the larger best wins, at equal best the lower index; the winner's second becomes
//                      max(its second, the loser's best).  The 2 -> 1 direction is the same kernel with the images swapped.  No split over columns.
// K17b k_sift_decide   one lane per (pair, direction, feature): best >= 1, best >= d_min, min(second, 2^18) <= table[min(best, 2^18) - d_min]; writes the
//                      one-way match (or -1) over best_j.
// K17c k_sift_emit     one workgroup per pair: the cross-check, a count, then - after k_sift_offsets, one workgroup, has applied min_num_matches and scanned
//                      the counts of the batch (BlockExclusiveScan, scan.hpp) - the same ordered compaction again (a workgroup scan over i in chunks of 256) writing (i, j) behind the
//                      pair's offset.
// No atomics, no kernel waits for another workgroup: the output does not depend on the schedule.
#include <cstring>

#include "scan.hpp"
#include "sift_match_handle.hpp"

namespace ppsfm {

constexpr int kSiftColTile = 64;        // scanned rows per LDS tile: two MFMA blocks of 32
constexpr int kSiftLdsStride = 144;     // bytes per staged row: 128 + 16, so that the 32 rows of a fragment read spread over the banks
constexpr int32_t kSiftPadOff = -(1 << 30);
constexpr int64_t kSiftDefaultWorkspace = 256ll << 20;

typedef int SiftV4 __attribute__((ext_vector_type(4)));
typedef int SiftV16 __attribute__((ext_vector_type(16)));

struct SiftWork {      // one workgroup of k_sift_top2
  int32_t q_row0, nq;      // the query image: its first row in the handle's descriptor array, its rows
  int32_t s_row0, ns;      // the scanned image
  int32_t i0;              // first query row of the tile
  int32_t out0;            // position of query row 0 in best_j / best / second
};

struct SiftPair {
  int32_t n1, n2;
  int32_t base;            // the 1 -> 2 results start here, the 2 -> 1 results at base + n1
};

// uint8 rows to d - 128 in place, and off[row] = 128 * sum(d) - 2^20
__global__ __launch_bounds__(256) void k_sift_prepare(int64_t rows, uint8_t* desc, int32_t* off) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  uint4* p = reinterpret_cast<uint4*>(desc + (size_t)row * kSiftDim);
  unsigned sum = 0;
#pragma unroll
  for (int c = 0; c < kSiftDim / 16; ++c) {
    uint4 v = p[c];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += (w[k] & 0xFFu) + ((w[k] >> 8) & 0xFFu) + ((w[k] >> 16) & 0xFFu) + (w[k] >> 24);
    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
    p[c] = v;
  }
  off[row] = 128 * (int32_t)sum - (1 << 20);
}

__global__ __launch_bounds__(256) void k_sift_top2(const int8_t* __restrict__ desc, const int32_t* __restrict__ off, const SiftWork* __restrict__ work,
                                                   int32_t* __restrict__ out_j, int32_t* __restrict__ out_best, int32_t* __restrict__ out_second) {
  __shared__ __attribute__((aligned(16))) int8_t tile[2][kSiftColTile * kSiftLdsStride];
  __shared__ __attribute__((aligned(16))) int32_t tile_off[2][kSiftColTile];
  const SiftWork w = work[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
  const int i = w.i0 + 32 * wave + r;
  const bool live = i < w.nq;
  const bool wave_live = w.i0 + 32 * wave < w.nq;      // (wave-uniform)
  SiftV4 q[4] = {};
  int off_i = 0;
  if (live) {
    const SiftV4* p = reinterpret_cast<const SiftV4*>(desc + (size_t)(w.q_row0 + i) * kSiftDim);
#pragma unroll
    for (int s = 0; s < 4; ++s) q[s] = p[2 * s + half];
    off_i = off[w.q_row0 + i];
  }
  // in units of dist - off_i: a dist of 0 is -off_i, where the reference's scan starts
  int best = -off_i, second = -off_i, best_j = -1;
  // The tiles alternate between two LDS buffers: the next tile's rows are fetched into registers before this tile's products, stored into the other
  // buffer after them - every wavefront left that buffer before the barrier that ended the previous tile - and one barrier per tile publishes them.
  SiftV4 fetch[2];
  int fetch_off = kSiftPadOff;
  auto load_tile = [&](int j0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = (tid + 256 * u) >> 3, chunk = (tid + 256 * u) & 7;
      fetch[u] = SiftV4{};
      if (j0 + row < w.ns) fetch[u] = *reinterpret_cast<const SiftV4*>(desc + (size_t)(w.s_row0 + j0 + row) * kSiftDim + 16 * chunk);
    }
    if (tid < kSiftColTile) fetch_off = j0 + tid < w.ns ? off[w.s_row0 + j0 + tid] : kSiftPadOff;
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = (tid + 256 * u) >> 3, chunk = (tid + 256 * u) & 7;
      *reinterpret_cast<SiftV4*>(tile[buf] + row * kSiftLdsStride + 16 * chunk) = fetch[u];
    }
    if (tid < kSiftColTile) tile_off[buf][tid] = fetch_off;
  };
  if (w.ns > 0) { load_tile(0); store_tile(0); }
  __syncthreads();
  for (int j0 = 0, buf = 0; j0 < w.ns; j0 += kSiftColTile, buf ^= 1) {
    const bool more = j0 + kSiftColTile < w.ns;      // (workgroup-uniform)
    if (more) load_tile(j0 + kSiftColTile);
    if (wave_live) {
#pragma unroll
      for (int b = 0; b < kSiftColTile / 32; ++b) {
        SiftV16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const SiftV4 o = *reinterpret_cast<const SiftV4*>(tile_off[buf] + 32 * b + 8 * g + 4 * half);
          acc[4 * g] = o[0]; acc[4 * g + 1] = o[1]; acc[4 * g + 2] = o[2]; acc[4 * g + 3] = o[3];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const SiftV4 a = *reinterpret_cast<const SiftV4*>(tile[buf] + (32 * b + r) * kSiftLdsStride + 32 * s + 16 * half);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, q[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {      // ascending j within the lane: the strict comparison keeps the lowest index of a tie
          const int v = acc[reg];
          const int j = j0 + 32 * b + (reg & 3) + 8 * (reg >> 2) + 4 * half;
          best_j = v > best ? j : best_j;
          second = max(second, min(best, v));
          best = max(best, v);
        }
      }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }
  // the two lane halves hold disjoint column sets of the same query row
  const int o_best = __shfl_xor(best, 32, 64), o_second = __shfl_xor(second, 32, 64), o_j = __shfl_xor(best_j, 32, 64);
  const bool mine = best > o_best || (best == o_best && (unsigned)best_j <= (unsigned)o_j);
  const int m_second = mine ? max(second, o_best) : max(o_second, best);
  const int m_best = mine ? best : o_best, m_j = mine ? best_j : o_j;
  if (live && half == 0) {
    out_j[w.out0 + i] = m_j;
    out_best[w.out0 + i] = m_best + off_i;
    out_second[w.out0 + i] = m_second + off_i;
  }
}

__global__ __launch_bounds__(256) void k_sift_decide(int64_t n, int32_t* __restrict__ match, const int32_t* __restrict__ best, const int32_t* __restrict__ second,
                                                     int32_t d_min, const int32_t* __restrict__ table) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int32_t b = best[e], s = second[e];
  bool pass = match[e] >= 0 && b >= 1 && b >= d_min;
  if (pass) pass = min(s, kSiftClamp) <= table[min(b, kSiftClamp) - d_min];
  if (!pass) match[e] = -1;
}

// kWrite = false: count[pair] = the matches of the pair.  kWrite = true: the pairs (i, j) to out, behind start[pair]; a pair whose count k_sift_offsets
// set to 0 writes nothing.
template <bool kWrite>
__global__ __launch_bounds__(256) void k_sift_emit(const SiftPair* __restrict__ pairs, const int32_t* __restrict__ match, int cross_check, int32_t* __restrict__ count,
                                                   const int32_t* __restrict__ start, int32_t* __restrict__ out, int64_t out_capacity) {
  __shared__ int32_t wave_total[4];
  const SiftPair p = pairs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (kWrite && count[blockIdx.x] == 0) return;
  const int64_t first = kWrite ? start[blockIdx.x] : 0;
  int32_t running = 0;
  for (int c0 = 0; c0 < p.n1; c0 += 256) {
    const int i = c0 + tid;
    int j = -1;
    bool keep = false;
    if (i < p.n1) {
      j = match[p.base + i];
      keep = j >= 0 && j < p.n2 && (!cross_check || match[p.base + p.n1 + j] == i);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { before += k < wave ? wave_total[k] : 0; total += wave_total[k]; }
    if (kWrite && keep) {
      const int64_t pos = first + running + before + __popcll(m & ((1ull << lane) - 1));
      if (pos < out_capacity) { out[2 * pos] = i; out[2 * pos + 1] = j; }
    }
    running += total;
    __syncthreads();
  }
  if (!kWrite && tid == 0) count[blockIdx.x] = running;
}

// one workgroup: count[p] < min_num_matches -> 0 (emptied counts those that had any), start = the exclusive scan of the counts, start[n] the total
__global__ __launch_bounds__(256) void k_sift_offsets(int32_t n, int32_t* __restrict__ count, int32_t min_num_matches, int32_t* __restrict__ start,
                                                      int32_t* __restrict__ emptied) {
  __shared__ int32_t wave_total[4], gone[4];
  const int tid = threadIdx.x;
  const int32_t chunk = (n + 255) / 256;
  const int32_t t0 = min(tid * chunk, n), t1 = min(t0 + chunk, n);
  int32_t local = 0, dropped = 0;
  for (int32_t p = t0; p < t1; ++p) {
    int32_t c = count[p];
    if (c < min_num_matches) { dropped += c > 0; c = 0; count[p] = 0; }
    local += c;
  }
  dropped = WaveSumInt(dropped);
  if ((tid & 63) == 0) gone[tid >> 6] = dropped;      // (read behind the scan's barrier)
  int32_t total;
  int32_t pos = BlockExclusiveScan<256>(local, wave_total, &total);
  for (int32_t p = t0; p < t1; ++p) { start[p] = pos; pos += count[p]; }
  if (tid == 0) { start[n] = total; *emptied = gone[0] + gone[1] + gone[2] + gone[3]; }
}

}  // namespace ppsfm

using namespace ppsfm;

namespace {

int CheckSiftOptions(const pp_sift_match_options* o, const char* where) {
  PP_REQUIRE(o, "%s: null options", where);
  PP_REQUIRE(SiftOptionsValid(o->max_ratio, o->max_distance, o->min_num_matches), "%s: max_ratio and max_distance must be positive, min_num_matches not negative",
             where);
  PP_REQUIRE(o->workspace_bytes >= 0, "%s: workspace_bytes is negative", where);
  return PP_OK;
}

int ThresholdsFor(double max_ratio, double max_distance, const char* where, SiftThresholds* t) {
  const std::string wrong = BuildSiftThresholds(max_ratio, max_distance, t);
  if (wrong.empty()) return PP_OK;
  SetLastError("%s: %s", where, wrong.c_str());
  return wrong.compare(0, 8, "invalid:") == 0 ? PP_ERR_INVALID : PP_ERR_INTERNAL;
}

// the handle's thresholds follow the options: built and uploaded when (max_ratio, max_distance) as floats differ from the last call's
int EnsureThresholds(pp_sift_impl* h, const pp_sift_match_options* o, const char* where) {
  const float ratio = (float)o->max_ratio, distance = (float)o->max_distance;
  if (h->have_thresholds && ratio == h->key_ratio && distance == h->key_distance) return PP_OK;
  h->have_thresholds = false;
  PP_TRY(ThresholdsFor(o->max_ratio, o->max_distance, where, &h->thresholds));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->d_table) h->blocks.Free(&h->d_table);
  PP_TRY(h->blocks.Put(&h->d_table, h->thresholds.s_max.data(), h->thresholds.s_max.size(), h->stream, 1));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  h->key_ratio = ratio; h->key_distance = distance; h->have_thresholds = true;
  return PP_OK;
}

void AppendWork(const pp_sift_impl* h, int32_t query, int32_t scanned, int32_t out0, std::vector<SiftWork>* work) {
  const int32_t nq = h->Rows(query), ns = h->Rows(scanned);
  for (int32_t i0 = 0; i0 < nq; i0 += kSiftRowTile)
    work->push_back(SiftWork{(int32_t)h->desc_start[(size_t)query], nq, (int32_t)h->desc_start[(size_t)scanned], ns, i0, out0});
}

// what a pair can emit at most
int64_t SiftMatchBound(int32_t n1, int32_t n2, bool cross_check) { return cross_check ? std::min(n1, n2) : (n2 > 0 ? n1 : 0); }

}  // namespace

extern "C" {

void pp_sift_match_options_default(pp_sift_match_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_ratio = 0.8; o->max_distance = 0.7; o->cross_check = 1; o->min_num_matches = 15; o->workspace_bytes = 0;
}

int pp_sift_match_thresholds(const pp_sift_match_options* options, int32_t* d_min, int32_t* table, int64_t capacity, int64_t* count) try {
  const char* where = "pp_sift_match_thresholds";
  PP_REQUIRE(options && d_min && count, "%s: null argument", where);
  PP_TRY(CheckSiftOptions(options, where));
  SiftThresholds t;
  PP_TRY(ThresholdsFor(options->max_ratio, options->max_distance, where, &t));
  PP_REQUIRE(!table || capacity >= (int64_t)t.s_max.size(), "%s: %lld entries, capacity is %lld", where, (long long)t.s_max.size(), (long long)capacity);
  *d_min = t.d_min;
  *count = (int64_t)t.s_max.size();
  if (table) std::copy(t.s_max.begin(), t.s_max.end(), table);
  return PP_OK;
} PP_API_CATCH("pp_sift_match_thresholds")

int pp_sift_destroy(pp_sift_handle h) try {
  delete h;      // (~DeviceHandle)
  return PP_OK;
} PP_API_CATCH("pp_sift_destroy")

int pp_sift_create(int32_t num_images, const int64_t* desc_start, const uint8_t* descriptors, int device, pp_sift_handle* out) try {
  const char* where = "pp_sift_create";
  PP_REQUIRE(desc_start && out, "%s: null argument", where);
  *out = nullptr;
  PP_REQUIRE(num_images >= 0, "%s: num_images is negative", where);
  PP_REQUIRE(desc_start[0] == 0, "%s: desc_start[0] != 0", where);
  for (int32_t k = 0; k < num_images; ++k) PP_REQUIRE(desc_start[k] <= desc_start[k + 1], "%s: desc_start decreases at image %d", where, k);
  const int64_t total = desc_start[num_images];
  PP_REQUIRE(SiftRowsFit(total), "%s: too many descriptors", where);
  PP_REQUIRE(total == 0 || descriptors, "%s: null descriptors", where);
  PP_TRY(UseDevice(where, device));
  UnderConstruction<pp_sift_impl, pp_sift_destroy> h{new pp_sift_impl()};
  h->num_images = num_images;
  h->desc_start.assign(desc_start, desc_start + num_images + 1);
  PP_TRY(h->Open(device));
  hipStream_t s = h->stream;
  PP_TRY(AllocSiftStore(h->blocks, total, &h->d_desc, &h->d_off));
  uint8_t* d_raw = reinterpret_cast<uint8_t*>(h->d_desc);      // (k_sift_prepare turns the bytes into d - 128 in place)
  PP_TRY(Upload(d_raw, descriptors, (size_t)total * kSiftDim, s));
  if (total > 0) hipLaunchKernelGGL(k_sift_prepare, dim3(CeilDiv(total, 256)), dim3(256), 0, s, total, d_raw, h->d_off);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { SetLastError("%s: upload failed", where); return PP_ERR_HIP; }
  *out = h.release();
  return PP_OK;
} PP_API_CATCH("pp_sift_create")

int pp_sift_top2(pp_sift_handle h, int32_t image1, int32_t image2, int32_t* best_j, int32_t* best, int32_t* second) try {
  const char* where = "pp_sift_top2";
  PP_REQUIRE(h && best_j && best && second, "%s: null argument", where);
  PP_REQUIRE(image1 >= 0 && image1 < h->num_images && image2 >= 0 && image2 < h->num_images, "%s: image (%d, %d) of %d", where, image1, image2, h->num_images);
  const int32_t n1 = h->Rows(image1);
  if (n1 == 0) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  CallScratch cb(s);
  std::vector<SiftWork> work;
  AppendWork(h, image1, image2, 0, &work);
  SiftWork* d_work = nullptr;
  int32_t *d_j = nullptr, *d_best = nullptr, *d_second = nullptr;
  PP_TRY(cb.Put(&d_work, work.data(), work.size()));
  PP_TRY(cb.Alloc(&d_j, (size_t)n1)); PP_TRY(cb.Alloc(&d_best, (size_t)n1)); PP_TRY(cb.Alloc(&d_second, (size_t)n1));
  hipLaunchKernelGGL(k_sift_top2, dim3((unsigned)work.size()), dim3(256), 0, s, (const int8_t*)h->d_desc, (const int32_t*)h->d_off, (const SiftWork*)d_work, d_j,
                     d_best, d_second);
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(Download(best_j, d_j, (size_t)n1, s)); PP_TRY(Download(best, d_best, (size_t)n1, s)); PP_TRY(Download(second, d_second, (size_t)n1, s));
  PP_HIP_TRY(hipStreamSynchronize(s));
  return PP_OK;
} PP_API_CATCH("pp_sift_top2")

int pp_sift_get_descriptors(pp_sift_handle h, int32_t image, uint8_t* descriptors, int64_t capacity, int64_t* num) try {
  const char* where = "pp_sift_get_descriptors";
  PP_REQUIRE(h && num, "%s: null argument", where);
  PP_REQUIRE(image >= 0 && image < h->num_images, "%s: image %d of %d", where, image, h->num_images);
  const int64_t rows = h->Rows(image);
  *num = rows;
  PP_REQUIRE(capacity >= rows && (descriptors || rows == 0), "%s: capacity %lld for %lld descriptors", where, (long long)capacity, (long long)rows);
  if (rows == 0) return PP_OK;
  PP_HIP_TRY(hipSetDevice(h->device));
  const size_t count = (size_t)rows * kSiftDim;
  PP_TRY(Download(descriptors, reinterpret_cast<const uint8_t*>(h->d_desc) + (size_t)h->desc_start[(size_t)image] * kSiftDim, count, h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < count; ++i) descriptors[i] ^= 0x80;      // the store holds d - 128
  return PP_OK;
} PP_API_CATCH("pp_sift_get_descriptors")

int pp_sift_match_pairs(pp_sift_handle h, const pp_sift_match_options* options, int64_t num_pairs, const int32_t* pairs, pp_sift_match_report* report,
                        int64_t* match_start, int32_t* matches, int64_t capacity) try {
  const char* where = "pp_sift_match_pairs";
  PP_REQUIRE(h && options && report && match_start, "%s: null argument", where);
  PP_REQUIRE(num_pairs >= 0 && (num_pairs == 0 || pairs) && capacity >= 0 && (capacity == 0 || matches), "%s: bad argument", where);
  PP_TRY(CheckSiftOptions(options, where));
  for (int64_t p = 0; p < num_pairs; ++p)
    PP_REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < h->num_images && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < h->num_images, "%s: pair %lld names image (%d, %d) of %d",
               where, (long long)p, pairs[2 * p], pairs[2 * p + 1], h->num_images);
  const auto t_begin = Clock::now();
  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  PP_TRY(EnsureThresholds(h, options, where));
  const bool cross = options->cross_check != 0;
  const int64_t cap_bytes = options->workspace_bytes > 0 ? options->workspace_bytes : kSiftDefaultWorkspace;
  std::vector<int64_t> starts((size_t)num_pairs + 1, 0);
  std::vector<int32_t> all;      // the matches of the batches so far, flat
  StreamTimer timer(*h);
  int32_t batches = 0, emptied_total = 0;
  std::vector<SiftWork> work;
  std::vector<SiftPair> batch;
  std::vector<int32_t> h_start;
  for (int64_t p0 = 0; p0 < num_pairs;) {
    // the batch: pairs p0 .. p1 - 1, at least one, their workspace below the cap
    work.clear(); batch.clear();
    int64_t p1 = p0, bytes = 0, features = 0, bound = 0;
    while (p1 < num_pairs) {
      const int32_t im1 = pairs[2 * p1], im2 = pairs[2 * p1 + 1], n1 = h->Rows(im1), n2 = h->Rows(im2);
      const int64_t pair_bound = SiftMatchBound(n1, n2, cross);
      const int64_t need = 12 * ((int64_t)n1 + n2) + 8 * pair_bound;
      if (p1 > p0 && bytes + need > cap_bytes) break;
      PP_REQUIRE(features + n1 + n2 < 0x7FFFFFFFll && bound + pair_bound < 0x3FFFFFFFll, "%s: pair %lld alone is too large for one batch", where, (long long)p1);
      batch.push_back(SiftPair{n1, n2, (int32_t)features});
      AppendWork(h, im1, im2, (int32_t)features, &work);
      if (cross) AppendWork(h, im2, im1, (int32_t)features + n1, &work);
      bytes += need; features += (int64_t)n1 + n2; bound += pair_bound;
      ++p1;
    }
    const int32_t np = (int32_t)(p1 - p0);
    ++batches;
    CallScratch cb(s);
    SiftWork* d_work = nullptr;
    SiftPair* d_pairs = nullptr;
    int32_t *d_j = nullptr, *d_best = nullptr, *d_second = nullptr, *d_count = nullptr, *d_start = nullptr, *d_emptied = nullptr, *d_out = nullptr;
    PP_TRY(cb.Put(&d_work, work.data(), work.size())); PP_TRY(cb.Put(&d_pairs, batch.data(), batch.size()));
    PP_TRY(cb.Alloc(&d_j, (size_t)features)); PP_TRY(cb.Alloc(&d_best, (size_t)features)); PP_TRY(cb.Alloc(&d_second, (size_t)features));
    PP_TRY(cb.Alloc(&d_count, (size_t)np)); PP_TRY(cb.Alloc(&d_start, (size_t)np + 1)); PP_TRY(cb.Alloc(&d_emptied, 1)); PP_TRY(cb.Alloc(&d_out, 2 * (size_t)bound));
    if (!cross && features > 0) PP_HIP_TRY(hipMemsetAsync(d_j, 0xFF, (size_t)features * sizeof(int32_t), s));      // (the 2 -> 1 halves are not computed)
    PP_TRY(timer.Begin());
    if (!work.empty())
      hipLaunchKernelGGL(k_sift_top2, dim3((unsigned)work.size()), dim3(256), 0, s, (const int8_t*)h->d_desc, (const int32_t*)h->d_off, (const SiftWork*)d_work,
                         d_j, d_best, d_second);
    if (features > 0)
      hipLaunchKernelGGL(k_sift_decide, dim3(CeilDiv(features, 256)), dim3(256), 0, s, features, d_j, (const int32_t*)d_best, (const int32_t*)d_second,
                         h->thresholds.d_min, (const int32_t*)h->d_table);
    hipLaunchKernelGGL(k_sift_emit<false>, dim3((unsigned)np), dim3(256), 0, s, (const SiftPair*)d_pairs, (const int32_t*)d_j, cross ? 1 : 0, d_count,
                       (const int32_t*)d_start, d_out, bound);
    hipLaunchKernelGGL(k_sift_offsets, dim3(1), dim3(256), 0, s, np, d_count, options->min_num_matches, d_start, d_emptied);
    hipLaunchKernelGGL(k_sift_emit<true>, dim3((unsigned)np), dim3(256), 0, s, (const SiftPair*)d_pairs, (const int32_t*)d_j, cross ? 1 : 0, d_count,
                       (const int32_t*)d_start, d_out, bound);
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(timer.End());
    h_start.assign((size_t)np + 1, 0);
    int32_t emptied = 0;
    PP_TRY(Download(h_start.data(), d_start, (size_t)np + 1, s)); PP_TRY(Download(&emptied, d_emptied, 1, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    PP_TRY(timer.Add());
    const int64_t total = h_start[(size_t)np];
    if (total < 0 || total > bound) { SetLastError("%s: the count of matches is out of range", where); return PP_ERR_INTERNAL; }
    const size_t before = all.size() / 2;
    all.resize(all.size() + 2 * (size_t)total);
    PP_TRY(Download(all.data() + 2 * before, d_out, 2 * (size_t)total, s));
    PP_HIP_TRY(hipStreamSynchronize(s));
    for (int32_t k = 0; k <= np; ++k) starts[(size_t)(p0 + k)] = (int64_t)before + h_start[(size_t)k];
    emptied_total += emptied;
    p0 = p1;
  }
  const int64_t need = (int64_t)(all.size() / 2);
  PP_REQUIRE(need <= capacity, "%s: %lld matches, capacity is %lld", where, (long long)need, (long long)capacity);
  std::copy(starts.begin(), starts.end(), match_start);
  std::copy(all.begin(), all.end(), matches);
  std::memset(report, 0, sizeof(*report));
  report->num_matches = need; report->num_pairs_emptied = emptied_total; report->num_batches = batches;
  report->device_ms = timer.ms; report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_sift_match_pairs")

}  // extern "C"
