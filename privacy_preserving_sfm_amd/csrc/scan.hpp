// The one exclusive integer scan of the library: a workgroup primitive and an array scan on top of it.  Integer sums only, so the result does not
// depend on how the work is split.  The kernels are templates: every .hip unit that scans instantiates its own copy (the library is built without
// relocatable device code).
#pragma once
#include "common.hpp"

namespace ppsfm {

// The sum of `mine` over the threads of the workgroup below this one; *block_total = the sum over all of them, on every thread.  kThreads is the
// workgroup's size: a multiple of 64, at most 1024.  T is int32_t or int64_t.  wave_total: kThreads / 64 entries of LDS.  An inclusive shuffle scan
// inside each wavefront, the wavefronts' totals through LDS, ONE barrier.  Every thread of the workgroup must call it; a second call with the same
// wave_total in one kernel needs a __syncthreads() in between (a late reader of the first call's totals against the second call's writer).
template <int kThreads, typename T>
__device__ __forceinline__ T BlockExclusiveScan(T mine, T* wave_total, T* block_total) {
  static_assert(kThreads % kWave == 0 && kThreads >= kWave && kThreads <= 1024, "a workgroup of whole wavefronts");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inclusive = mine;      // over the lanes of the wavefront
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = __shfl_up(inclusive, off, kWave);
    if (lane >= off) inclusive += o;
  }
  if (lane == kWave - 1) wave_total[w] = inclusive;
  __syncthreads();
  T below = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kThreads / kWave; ++k) {
    const T t = wave_total[k];
    if (k < w) below += t;
    all += t;
  }
  *block_total = all;
  return below + inclusive - mine;
}

// out[i] = the sum of in[0 .. i) for i < n; *total = the sum of all n (total may be out + n, or null).  in and out do not overlap.
template <typename T>
struct ScanJob {
  const T* in;
  T* out;
  T* total;
};

constexpr int kScanThreads = 1024;        // the direct kernel's workgroup
constexpr int kScanTile = 1024;           // elements per workgroup of the tiled form: 256 threads x 4 consecutive ones
constexpr int64_t kScanDirect = 4096;     // up to here one workgroup takes the array itself

// One workgroup per job (blockIdx.y), thread t the span [t * chunk, (t + 1) * chunk): any n, 0 included.
template <typename T>
__global__ __launch_bounds__(kScanThreads) void k_scan_direct(int64_t n, ScanJob<T> j0, ScanJob<T> j1) {
  __shared__ T wave_total[kScanThreads / kWave];
  const ScanJob<T> j = blockIdx.y == 0 ? j0 : j1;
  const T* __restrict__ in = j.in;
  T* __restrict__ out = j.out;
  const int tid = threadIdx.x;
  const int64_t chunk = (n + kScanThreads - 1) / kScanThreads;
  const int64_t t0r = (int64_t)tid * chunk;
  const int64_t t0 = t0r < n ? t0r : n, t1 = t0 + chunk < n ? t0 + chunk : n;
  T local = 0;
  for (int64_t i = t0; i < t1; ++i) local += in[i];
  T all;
  T pos = BlockExclusiveScan<kScanThreads>(local, wave_total, &all);
  for (int64_t i = t0; i < t1; ++i) { const T v = in[i]; out[i] = pos; pos += v; }
  if (tid == 0 && j.total) *j.total = all;
}

// The tiled form, workgroup (x, y) = (tile, job).  Of job y's share of the scratch the first `tiles` entries are the tile sums, the next `tiles` their
// exclusive scan (k_scan_direct over the sums, which also writes the job's total).
template <typename T>
__global__ __launch_bounds__(256) void k_scan_tile_sums(int64_t n, int64_t tiles, ScanJob<T> j0, ScanJob<T> j1, T* __restrict__ scratch) {
  __shared__ T wave_total[4];
  const T* __restrict__ in = blockIdx.y == 0 ? j0.in : j1.in;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  T v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + tid + 256 * k;
    if (i < n) v += in[i];
  }
  T all;
  (void)BlockExclusiveScan<256>(v, wave_total, &all);
  if (tid == 0) scratch[(int64_t)blockIdx.y * 2 * tiles + blockIdx.x] = all;
}

template <typename T>
__global__ __launch_bounds__(256) void k_scan_tiles(int64_t n, int64_t tiles, ScanJob<T> j0, ScanJob<T> j1, const T* __restrict__ scratch) {
  __shared__ T wave_total[4];
  const ScanJob<T> j = blockIdx.y == 0 ? j0 : j1;
  const T* __restrict__ in = j.in;
  T* __restrict__ out = j.out;
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + 4 * threadIdx.x;
  T v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] = i0 + k < n ? in[i0 + k] : 0; sum += v[k]; }
  T all;
  T pos = scratch[(int64_t)blockIdx.y * 2 * tiles + tiles + blockIdx.x] + BlockExclusiveScan<256>(sum, wave_total, &all);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = pos;
    pos += v[k];
  }
}

// elements of T the caller provides PER JOB as scratch for a scan of n elements
inline size_t ScanScratchCount(int64_t n) { return n <= kScanDirect ? 0 : 2 * (size_t)((n + kScanTile - 1) / kScanTile); }

// num_jobs (1 or 2) independent scans of the same length n >= 0 on stream s: one launch up to kScanDirect elements, three above (the tile sums, the
// direct kernel over them, every tile from its offset).  scratch: num_jobs * ScanScratchCount(n) elements (not read when that is 0).  For n == 0 only
// the totals are written.  Launch errors are the caller's hipGetLastError().
template <typename T>
inline void LaunchExclusiveScan(hipStream_t s, int64_t n, const ScanJob<T>* jobs, int num_jobs, T* scratch) {
  const ScanJob<T> j0 = jobs[0], j1 = jobs[num_jobs - 1];
  if (n <= kScanDirect) {
    hipLaunchKernelGGL(k_scan_direct<T>, dim3(1, (unsigned)num_jobs), dim3(kScanThreads), 0, s, n, j0, j1);
    return;
  }
  const int64_t tiles = (n + kScanTile - 1) / kScanTile;
  const dim3 grid((unsigned)tiles, (unsigned)num_jobs);
  const ScanJob<T> s0{scratch, scratch + tiles, j0.total}, s1{scratch + (num_jobs - 1) * 2 * tiles, scratch + (num_jobs - 1) * 2 * tiles + tiles, j1.total};
  hipLaunchKernelGGL(k_scan_tile_sums<T>, grid, dim3(256), 0, s, n, tiles, j0, j1, scratch);
  hipLaunchKernelGGL(k_scan_direct<T>, dim3(1, (unsigned)num_jobs), dim3(kScanThreads), 0, s, tiles, s0, s1);
  hipLaunchKernelGGL(k_scan_tiles<T>, grid, dim3(256), 0, s, n, tiles, j0, j1, (const T*)scratch);
}

}  // namespace ppsfm
