// K21 - SIFT keypoints and descriptors of one grey image: ExtractSiftFeaturesCPU (reference src/feature/sift.cc:399-573, over VLFeat's vl_sift_*) on
// the device, the same output bit for bit.  The arithmetic of every pixel and keypoint is sift_core.hpp, the host's share (libm, the level
// containers, the max_num_features cut) sift_extract_replay.hpp; this file is the kernels around the former and the C ABI.  No kernel uses an atomic
// or waits for another workgroup: every list comes out in the reference's order by count, scan (scan.hpp) and scatter.
// K21a k_sift_load / k_sift_upsample / k_sift_downsample   the first level of an octave from the bytes, or from the octave before
// K21b k_sift_convolve   one pass of _vl_sift_smooth: the column convolution with the transposed write.  A workgroup takes a 32 x 32 tile of
//                        outputs: the 32 + 2 W input rows of its 32 columns are staged in LDS (reads along the rows, the ends clamped - padding by
//                        continuity), then one lane per output pixel walks its 2 W + 1 taps down the staged column in the reference's order.  The
//                        lanes of a wavefront take consecutive rows, so the write of out[x * h + y] is contiguous - and that makes the second pass,
//                        which reads the transposed image along ITS rows, contiguous as well.  The LDS pitch of 33 keeps the 32 lanes on 32 banks.
// K21c k_sift_dog, k_sift_gradient   one lane per pixel
// K21d k_sift_detect_count / _scatter   a workgroup per row (level, y): the 26-neighbour test, the row's count; after the scan over the rows the same
//                        test again with a workgroup scan per 256 pixels, so the candidates land in (level, y, x) order
// K21e k_sift_refine     one lane per candidate; the host keeps the survivors in order and evaluates pow for their sigma
// K21f k_sift_orient     one lane per keypoint walking its window in the reference's order (the histogram is a sequential double sum)
// K21g k_sift_describe   one lane per feature: the 4 x 4 x 8 float accumulation in the reference's order straight into the feature's row of the raw
//                        descriptors, then the last normalisation to bytes.  The single call's kernel, and the on-device reference of K23.
// K23  pp_sift_extract_batch: the images of a batch through the octaves in lock-step, the kernels above per image on slices of one workspace, four
//                        waits per octave for all of them; k_sift_describe_wave describes the features of every image of an octave in one launch, a
//                        wavefront per feature with a fixed-order fold (see the kernel).
// K24  pp_sift_extract_to_matcher: the batch with a pp_sift_handle as its way out.  The max_num_features cut is made from the keypoint counts, before
//                        any orientation or descriptor; k_sift_describe_kept describes the kept features of all octaves of a group in one launch
//                        and writes each row, and its offset, where k_sift_top2 (sift_match.hip) reads it.
#include <cstring>

#include "device_handle.hpp"
#include "scan.hpp"
#include "sift_extract_replay.hpp"
#include "sift_match_handle.hpp"

namespace ppsfm {

using namespace sift;

constexpr int kSiftBlock = 256;
constexpr int kSiftTile = 32;                   // outputs per side of a convolution tile
constexpr int kSiftPitch = kSiftTile + 1;
constexpr int kSiftLaneBlock = 64;              // the lane-per-item kernels: few items, many workgroups

__global__ __launch_bounds__(kSiftBlock) void k_sift_load(int64_t n, const uint8_t* __restrict__ grey, float* __restrict__ im) {
  const int64_t i = (int64_t)blockIdx.x * kSiftBlock + threadIdx.x;
  if (i < n) im[i] = PixelFromByte(grey[i]);
}

// copy_and_upsample_rows: dst[X * h + y], X < 2 w
__global__ __launch_bounds__(kSiftBlock) void k_sift_upsample(float* __restrict__ dst, const float* __restrict__ src, int w, int h) {
  const int64_t i = (int64_t)blockIdx.x * kSiftBlock + threadIdx.x;
  if (i >= 2 * (int64_t)w * h) return;
  const int X = (int)(i / h), y = (int)(i % h);
  dst[i] = UpsampleRowValue(src + (int64_t)y * w, w, X);
}

// dst (nw x nh) = every d-th pixel of every d-th row of src (rows of w)
__global__ __launch_bounds__(kSiftBlock) void k_sift_downsample(float* __restrict__ dst, const float* __restrict__ src, int w, int nw, int nh, int d) {
  const int64_t i = (int64_t)blockIdx.x * kSiftBlock + threadIdx.x;
  if (i >= (int64_t)nw * nh) return;
  const int x = (int)(i % nw), y = (int)(i / nw);
  dst[i] = src[(int64_t)(y * d) * w + (int64_t)x * d];
}

__global__ __launch_bounds__(kSiftBlock) void k_sift_convolve(float* __restrict__ dst, const float* __restrict__ src, int w, int h,
                                                              const float* __restrict__ taps, int W) {
  extern __shared__ float lds[];
  float* tile = lds;                                        // (32 + 2 W) rows of 33
  float* tp = lds + (kSiftTile + 2 * W) * kSiftPitch;       // 2 W + 1 taps
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kSiftTile, y0 = blockIdx.y * kSiftTile;
  const int rows = kSiftTile + 2 * W;
  for (int i = tid; i < rows * kSiftTile; i += kSiftBlock) {
    const int r = i >> 5, c = i & 31;
    int p = y0 - W + r;
    p = p < 0 ? 0 : (p > h - 1 ? h - 1 : p);
    const int xx = x0 + c < w ? x0 + c : w - 1;
    tile[r * kSiftPitch + c] = src[(int64_t)p * w + xx];
  }
  for (int i = tid; i < 2 * W + 1; i += kSiftBlock) tp[i] = taps[i];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSiftTile * kSiftTile / kSiftBlock; ++k) {
    const int o = tid + kSiftBlock * k;
    const int ly = o & 31, lx = o >> 5;
    const int x = x0 + lx, y = y0 + ly;
    if (x < w && y < h) dst[(int64_t)x * h + y] = ConvolveTaps(tile + ly * kSiftPitch + lx, kSiftPitch, tp, 2 * W + 1);
  }
}

// dog[j] = octave[j + lev] - octave[j] over the levels laid end to end
__global__ __launch_bounds__(kSiftBlock) void k_sift_dog(float* __restrict__ dog, const float* __restrict__ octave, int64_t lev, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * kSiftBlock + threadIdx.x;
  if (j < n) dog[j] = octave[j + lev] - octave[j];
}

// levels: the Gaussian levels s_min + 1 .. s_max - 2, end to end
__global__ __launch_bounds__(kSiftBlock) void k_sift_gradient(float* __restrict__ grad, const float* __restrict__ levels, int w, int h, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kSiftBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t lev = (int64_t)w * h;
  const int64_t s = i / lev, r = i % lev;
  float mod, ang;
  GradientAt(levels + s * lev, w, h, (int)(r % w), (int)(r / w), &mod, &ang);
  grad[2 * i] = mod;      // (two stores: a level of odd size leaves the next one's pairs off an 8-byte boundary)
  grad[2 * i + 1] = ang;
}

// row = (level - (s_min + 1)) * h + y; dog1 = the DoG level s_min + 1
__global__ __launch_bounds__(kSiftBlock) void k_sift_detect_count(const float* __restrict__ dog1, int w, int h, double threshold, int32_t* __restrict__ row_count) {
  __shared__ int32_t wave_total[kSiftBlock / kWave];
  const int row = blockIdx.x, y = row % h;
  const int64_t lev = (int64_t)w * h;
  int32_t cnt = 0;
  if (y >= 1 && y <= h - 2) {
    const float* base = dog1 + (int64_t)(row / h) * lev + (int64_t)y * w;
    for (int x = 1 + threadIdx.x; x < w - 1; x += kSiftBlock) cnt += IsExtremum(base + x, w, (int)lev, threshold);
  }
  int32_t all;
  (void)BlockExclusiveScan<kSiftBlock>(cnt, wave_total, &all);
  if (threadIdx.x == 0) row_count[row] = all;
}

__global__ __launch_bounds__(kSiftBlock) void k_sift_detect_scatter(const float* __restrict__ dog1, int w, int h, int s_first, double threshold,
                                                                    const int32_t* __restrict__ row_count, const int32_t* __restrict__ row_start,
                                                                    int32_t* __restrict__ cand) {
  __shared__ int32_t wave_total[kSiftBlock / kWave];
  const int row = blockIdx.x, y = row % h;
  if (row_count[row] == 0) return;      // (the whole workgroup)
  const int64_t lev = (int64_t)w * h;
  const float* base = dog1 + (int64_t)(row / h) * lev + (int64_t)y * w;
  int32_t at = row_start[row];
  for (int x0 = 1; x0 < w - 1; x0 += kSiftBlock) {
    const int x = x0 + threadIdx.x;
    const int32_t flag = x < w - 1 && IsExtremum(base + x, w, (int)lev, threshold);
    int32_t all;
    const int32_t pos = BlockExclusiveScan<kSiftBlock>(flag, wave_total, &all);
    if (flag) {
      int32_t* c = cand + 3 * (int64_t)(at + pos);
      c[0] = x; c[1] = y; c[2] = s_first + row / h;
    }
    at += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kSiftLaneBlock) void k_sift_refine(int32_t n, const int32_t* __restrict__ cand, const float* __restrict__ dog, int w, int h, int s_min,
                                                               int s_max, double tp, double te, Refined* __restrict__ out) {
  const int32_t i = blockIdx.x * kSiftLaneBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = RefineCandidate(dog, w, h, s_min, s_max, cand[3 * (int64_t)i], cand[3 * (int64_t)i + 1], cand[3 * (int64_t)i + 2], tp, te);
}

// grad: the octave's gradient levels s_min + 1 .. end to end
__global__ __launch_bounds__(kSiftLaneBlock) void k_sift_orient(int32_t n, const Keypoint* __restrict__ keys, const float* __restrict__ grad, int w, int h, int s_min,
                                                               int s_max, double xper, const double* __restrict__ expn, int32_t* __restrict__ num_angles,
                                                               double* __restrict__ angles) {
  const int32_t i = blockIdx.x * kSiftLaneBlock + threadIdx.x;
  if (i >= n) return;
  const Keypoint k = keys[i];
  double a[kMaxAngles] = {0, 0, 0, 0};
  const int64_t level = (int64_t)(k.is - s_min - 1) * 2 * ((int64_t)w * h);      // (Orientations reads nothing when is is out of range: clamp the pointer)
  const bool in_range = k.is >= s_min + 1 && k.is <= s_max - 2;
  num_angles[i] = Orientations(grad + (in_range ? level : 0), w, h, s_min, s_max, k, xper, expn, a);
#pragma unroll
  for (int j = 0; j < kMaxAngles; ++j) angles[kMaxAngles * (int64_t)i + j] = a[j];
}

struct SiftFeature {
  int32_t key, image;                      // image: its slot in the batch's image table (k_sift_describe_wave); 0 for the single call
  double angle, sin_angle, cos_angle;      // the host's libm
};

__global__ __launch_bounds__(kSiftLaneBlock) void k_sift_describe(int32_t n, const SiftFeature* __restrict__ feats, const Keypoint* __restrict__ keys,
                                                                 const float* __restrict__ grad, int w, int h, int s_min, int s_max, double xper,
                                                                 const double* __restrict__ expn, int normalization, float* __restrict__ raw,
                                                                 uint8_t* __restrict__ bytes, DescriptorWindow* __restrict__ window) {
  const int32_t f = blockIdx.x * kSiftLaneBlock + threadIdx.x;
  if (f >= n) return;
  const SiftFeature q = feats[f];
  const Keypoint k = keys[q.key];
  const bool in_range = k.is >= s_min + 1 && k.is <= s_max - 2;
  const int64_t level = (int64_t)(k.is - s_min - 1) * 2 * ((int64_t)w * h);
  float* row = raw + (int64_t)kDescBins * f;
  window[f] = Descriptor(grad + (in_range ? level : 0), w, h, s_min, s_max, k, xper, q.angle, q.sin_angle, q.cos_angle, expn, row);
  FinishDescriptor(row, normalization, bytes + (int64_t)kDescBins * f);
}

struct SiftOctave {
  int32_t o = 0, w = 0, h = 0;
  bool has_grad = false;
  size_t gauss = 0, dog = 0, grad = 0;      // offsets into the pyramid, in floats
  std::vector<int32_t> cand;                // the unrefined candidates of the last extraction
};

// K23 k_sift_describe_wave - one wavefront (a workgroup of 64) per feature, the features of any number of images in one launch: feats[f].image is the
// slot of the feature's image in `images`, feats[f].key its keypoint in `keys` (all images' keypoints, end to end).  Lane l takes pixel 64 c + l of
// the window's scan for chunk c (the lanes of a window row read adjacent (modulus, angle) pairs) and stages DescriptorSample() of it in LDS; then
// every lane walks the staged pixels in order - all lanes read the same address, a broadcast - and folds them into the two bins it owns, 2 l and
// 2 l + 1: the spatial cell l / 4, the orientations 2 (l % 4) and the next.  So each bin receives its additions in scan order, as in Descriptor().
// The norms: every lane sums the 128 entries from LDS in index order; the divisions, the clamp and the bytes are spread two entries per lane.
struct SiftWaveImage {
  const float* grad;      // the gradient levels s_min + 1 .. of the image's current octave
  int32_t w, h;
  double xper;
};

// The wavefront's work on one feature up to the last norm: *acc0, *acc1 = the lane's two entries 2 l, 2 l + 1 of the float descriptor before the last
// normalisation, *last_norm = FinishNorm() over all 128 (the same on every lane); -> the window.  staged: kWave taps of LDS, hist: kDescBins floats.
__device__ __forceinline__ DescriptorWindow DescribeByWave(const SiftFeature& q, const Keypoint& k, const SiftWaveImage& im, int s_min, int s_max,
                                                          const double* __restrict__ expn, int normalization, DescriptorTap* staged, float* hist,
                                                          float* out0, float* out1, float* last_norm) {
  const int lane = threadIdx.x;
  const DescriptorFrame fr = MakeDescriptorFrame(im.w, im.h, s_min, s_max, k, im.xper);
  const int cx = ((lane >> 2) & 3) - 2, cy = (lane >> 4) - 2, t0 = 2 * (lane & 3);
  float acc0 = 0.f, acc1 = 0.f;
  const int n = DescriptorWindowPixels(fr);      // (0 unless the bounds check passed: nothing is read for a level that does not exist)
  if (n > 0) {
    const int nx = fr.x1 - fr.x0 + 1;
    const float* pt = im.grad + (int64_t)(k.is - s_min - 1) * 2 * ((int64_t)im.w * im.h) + 2 * fr.xi + (int64_t)(2 * im.w) * fr.yi;
    for (int base = 0; base < n; base += kWave) {
      const int p = base + lane;
      if (p < n) {
        const int dxi = fr.x0 + p % nx, dyi = fr.y0 + p / nx;
        const float* gp = pt + 2 * dxi + (int64_t)(2 * im.w) * dyi;
        staged[lane] = DescriptorSample(fr, q.angle, q.sin_angle, q.cos_angle, expn, dxi, dyi, gp[0], gp[1]);
      }
      __syncthreads();
      const int m = n - base < kWave ? n - base : kWave;
      for (int j = 0; j < m; ++j) DescriptorFold(staged[j], cx, cy, t0, &acc0, &acc1);
      __syncthreads();
    }
  }
  hist[2 * lane] = acc0; hist[2 * lane + 1] = acc1;
  __syncthreads();
  float norm = HistogramNorm(hist);
  acc0 = ClampBin(acc0 / norm); acc1 = ClampBin(acc1 / norm);
  __syncthreads();
  hist[2 * lane] = acc0; hist[2 * lane + 1] = acc1;
  __syncthreads();
  norm = HistogramNorm(hist);
  acc0 = acc0 / norm; acc1 = acc1 / norm;
  __syncthreads();
  hist[2 * lane] = acc0; hist[2 * lane + 1] = acc1;
  __syncthreads();
  *last_norm = FinishNorm(hist, normalization);
  *out0 = acc0; *out1 = acc1;
  return fr.win;
}

__global__ __launch_bounds__(kWave) void k_sift_describe_wave(const SiftFeature* __restrict__ feats, const Keypoint* __restrict__ keys,
                                                             const SiftWaveImage* __restrict__ images, int s_min, int s_max,
                                                             const double* __restrict__ expn, int normalization, float* __restrict__ raw,
                                                             uint8_t* __restrict__ bytes, DescriptorWindow* __restrict__ window) {
  __shared__ DescriptorTap staged[kWave];
  __shared__ float hist[kDescBins];
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  const SiftFeature q = feats[f];
  float acc0, acc1, norm;
  const DescriptorWindow win = DescribeByWave(q, keys[q.key], images[q.image], s_min, s_max, expn, normalization, staged, hist, &acc0, &acc1, &norm);
  raw[kDescBins * f + 2 * lane] = acc0; raw[kDescBins * f + 2 * lane + 1] = acc1;
  bytes[kDescBins * f + UbcIndex(2 * lane)] = FinishByte(acc0, norm, normalization);
  bytes[kDescBins * f + UbcIndex(2 * lane + 1)] = FinishByte(acc1, norm, normalization);
  if (lane == 0) window[f] = win;
}

// K24 k_sift_describe_kept - k_sift_describe_wave for the features pp_sift_extract_to_matcher keeps, written as the matcher reads them.  One launch
// covers every octave of a group: `images` has a slot per (octave, image) and feats[f].image names the feature's.  The accumulation and the norms
// are DescribeByWave(), so the bytes are those of the batch call; the tail differs.  No float descriptor leaves the kernel.  The 128 bytes are put
// together in UBC order in LDS with their top bit flipped (d - 128, what k_sift_top2 multiplies) and go to row dst_row[f] of the store as eight
// 16-byte pieces; the row's offset 128 * sum(d) - 2^20 is the integer sum over the wavefront of the two bytes each lane made.
__global__ __launch_bounds__(kWave) void k_sift_describe_kept(const SiftFeature* __restrict__ feats, const Keypoint* __restrict__ keys,
                                                             const SiftWaveImage* __restrict__ images, const int32_t* __restrict__ dst_row, int s_min,
                                                             int s_max, const double* __restrict__ expn, int normalization, int8_t* __restrict__ d_desc,
                                                             int32_t* __restrict__ d_off, DescriptorWindow* __restrict__ window) {
  __shared__ DescriptorTap staged[kWave];
  __shared__ float hist[kDescBins];
  __shared__ __attribute__((aligned(16))) uint8_t row[kDescBins];
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  const SiftFeature q = feats[f];
  float acc0, acc1, norm;
  const DescriptorWindow win = DescribeByWave(q, keys[q.key], images[q.image], s_min, s_max, expn, normalization, staged, hist, &acc0, &acc1, &norm);
  const uint8_t b0 = FinishByte(acc0, norm, normalization), b1 = FinishByte(acc1, norm, normalization);
  row[UbcIndex(2 * lane)] = b0 ^ 0x80; row[UbcIndex(2 * lane + 1)] = b1 ^ 0x80;
  const int sum = WaveSumInt((int)b0 + (int)b1);
  __syncthreads();
  const int64_t r = dst_row[f];
  if (lane < kDescBins / 16) reinterpret_cast<uint4*>(d_desc + kDescBins * r)[lane] = reinterpret_cast<const uint4*>(row)[lane];
  if (lane == 0) { d_off[r] = 128 * sum - (1 << 20); window[f] = win; }
}

// The filters of one option set, one after the other: [0] the first octave's first level (or none), [1] a later octave's (none with the reference's
// geometry), then the levels s_min + 1 .. s_max
struct SiftFilter { size_t offset; int W; };
struct SiftFilters {
  std::vector<float> taps;
  std::vector<SiftFilter> filters;
};

inline int MakeSiftFilters(const char* where, const Geometry& g, SiftFilters* out) {
  auto add_filter = [&](double sigma) {
    if (!(sigma > 0.0)) { out->filters.push_back(SiftFilter{0, 0}); return; }
    const std::vector<float> t = GaussTaps(sigma);
    out->filters.push_back(SiftFilter{out->taps.size(), (int)t.size() / 2});
    out->taps.insert(out->taps.end(), t.begin(), t.end());
  };
  add_filter(FirstLevelSigma(g, true));
  add_filter(FirstLevelSigma(g, false));
  for (int s = g.s_min + 1; s <= g.s_max; ++s) add_filter(LevelSigma(g, s));
  for (const SiftFilter& f : out->filters) PP_REQUIRE(f.W <= kMaxFilterHalfWidth, "%s: a filter of half width %d", where, f.W);
  return PP_OK;
}

// The octaves of one image and their places in its pyramid (offsets in floats from the pyramid's start), the transposed temporary behind them
struct SiftLayout {
  std::vector<SiftOctave> octaves;
  size_t total = 0, temp_offset = 0;      // floats of the pyramid with the temporary; where the temporary starts
  int max_rows = 1;                       // the detection rows (level, y) of the tallest octave
  size_t rows_need = 0;                   // int32s: row counts, row starts, the total (2), the scan's scratch
};

inline SiftLayout LayoutOctaves(const Geometry& g, int width, int height) {
  SiftLayout lay;
  const int L = g.levels(), num_grad = g.S;
  lay.octaves.resize((size_t)g.O);
  for (int q = 0; q < g.O; ++q) {
    SiftOctave& oc = lay.octaves[(size_t)q];
    oc.o = g.o_min + q;
    oc.w = ShiftLeft(width, -oc.o); oc.h = ShiftLeft(height, -oc.o);
    oc.has_grad = oc.w >= 2 && oc.h >= 2;
    const size_t lev = (size_t)oc.w * oc.h;
    oc.gauss = lay.total; lay.total += lev * (size_t)L;
    oc.dog = lay.total; lay.total += lev * (size_t)(L - 1);
    oc.grad = lay.total; lay.total += 2 * lev * (size_t)num_grad;
  }
  lay.temp_offset = lay.total;
  lay.total += (size_t)lay.octaves[0].w * lay.octaves[0].h;
  for (const SiftOctave& oc : lay.octaves) lay.max_rows = std::max(lay.max_rows, g.S * oc.h);
  lay.rows_need = 2 * (size_t)lay.max_rows + 2 + ScanScratchCount(lay.max_rows);
  return lay;
}

inline dim3 SiftGrid(int64_t n, int block) { return dim3((unsigned)std::max<int64_t>(CeilDiv(n, block), 1)); }

// The Gaussian and DoG levels of octave q of one image: its first level from `image` (width x height floats) or from the octave before, the
// smoothing level by level, the differences.  pyramid: where the image's pyramid starts; d_taps: the filters' taps on the device.
inline void LaunchOctavePyramid(hipStream_t s, const Geometry& g, const SiftFilters& filters, const float* d_taps, const SiftLayout& lay, int q, float* pyramid,
                                const float* image, int width, int height) {
  const SiftOctave& oc = lay.octaves[(size_t)q];
  const int w = oc.w, hgt = oc.h, L = g.levels();
  const int64_t lev = (int64_t)w * hgt;
  float* gauss = pyramid + oc.gauss;
  float* dog = pyramid + oc.dog;
  float* temp = pyramid + lay.temp_offset;
  auto smooth = [&](float* out, const float* in, const SiftFilter& f) {
    const size_t lds = ((size_t)(kSiftTile + 2 * f.W) * kSiftPitch + 2 * (size_t)f.W + 1) * sizeof(float);
    hipLaunchKernelGGL(k_sift_convolve, dim3((unsigned)CeilDiv(w, kSiftTile), (unsigned)CeilDiv(hgt, kSiftTile)), dim3(kSiftBlock), lds, s, temp, in, w, hgt,
                       d_taps + f.offset, f.W);
    hipLaunchKernelGGL(k_sift_convolve, dim3((unsigned)CeilDiv(hgt, kSiftTile), (unsigned)CeilDiv(w, kSiftTile)), dim3(kSiftBlock), lds, s, out, (const float*)temp, hgt, w,
                       d_taps + f.offset, f.W);
  };
  // ---- the octave's first level
  if (q == 0) {
    if (g.o_min < 0) {
      hipLaunchKernelGGL(k_sift_upsample, SiftGrid(2 * (int64_t)width * height, kSiftBlock), dim3(kSiftBlock), 0, s, temp, image, width, height);
      hipLaunchKernelGGL(k_sift_upsample, SiftGrid(4 * (int64_t)width * height, kSiftBlock), dim3(kSiftBlock), 0, s, gauss, (const float*)temp, height, 2 * width);
      for (int d = -1; d > g.o_min; --d) {      // (the reference's arguments, as they stand)
        const int dw = width << -d, dh = height << -d;
        hipLaunchKernelGGL(k_sift_upsample, SiftGrid(2 * (int64_t)dw * dh, kSiftBlock), dim3(kSiftBlock), 0, s, temp, (const float*)gauss, dw, dh);
        hipLaunchKernelGGL(k_sift_upsample, SiftGrid(4 * (int64_t)dw * dh, kSiftBlock), dim3(kSiftBlock), 0, s, gauss, (const float*)temp, dw, 2 * dh);
      }
    } else {
      hipLaunchKernelGGL(k_sift_downsample, SiftGrid(lev, kSiftBlock), dim3(kSiftBlock), 0, s, gauss, image, width, w, hgt, 1 << g.o_min);
    }
  } else {
    const SiftOctave& prev = lay.octaves[(size_t)q - 1];
    const int s_best = std::min(g.s_min + g.S, g.s_max);
    const float* from = pyramid + prev.gauss + (size_t)(s_best - g.s_min) * ((size_t)prev.w * prev.h);
    hipLaunchKernelGGL(k_sift_downsample, SiftGrid(lev, kSiftBlock), dim3(kSiftBlock), 0, s, gauss, from, prev.w, w, hgt, 2);
  }
  const SiftFilter& f0 = filters.filters[q == 0 ? 0 : 1];
  if (f0.W > 0) smooth(gauss, gauss, f0);
  for (int lvl = 1; lvl < L; ++lvl) smooth(gauss + (size_t)lvl * lev, gauss + (size_t)(lvl - 1) * lev, filters.filters[(size_t)lvl + 1]);
  hipLaunchKernelGGL(k_sift_dog, SiftGrid(lev * (L - 1), kSiftBlock), dim3(kSiftBlock), 0, s, dog, (const float*)gauss, lev, lev * (L - 1));
}

// every feature of one image of the last batch, before the cut: what pp_sift_extract_batch_features hands out
struct SiftBatchFeatures {
  std::vector<float> raw;
  std::vector<int32_t> octave_level;
  std::vector<double> angles;
};

}  // namespace ppsfm

struct pp_sift_extractor_impl : ppsfm::DeviceHandle {
  // the workspace: grows, never shrinks
  float* pyramid = nullptr;       size_t cap_pyramid = 0;       // every octave's Gaussian, DoG and gradient levels + the transposed temporary
  float* image = nullptr;         uint8_t* grey = nullptr;      size_t cap_image = 0;
  int32_t* rows = nullptr;        size_t cap_rows = 0;          // row counts, row starts, the total, the scan's scratch
  int32_t* cand = nullptr;        ppsfm::sift::Refined* refined = nullptr;      size_t cap_cand = 0;
  ppsfm::sift::Keypoint* keys = nullptr;      int32_t* num_angles = nullptr;      double* angles = nullptr;      size_t cap_keys = 0;
  ppsfm::SiftFeature* feats = nullptr;      float* raw = nullptr;      uint8_t* bytes = nullptr;      ppsfm::sift::DescriptorWindow* window = nullptr;      size_t cap_feats = 0;
  double* expn = nullptr;
  float* taps = nullptr;          size_t cap_taps = 0;
  ppsfm::SiftWaveImage* wave_images = nullptr;      size_t cap_wave_images = 0;      // the image table of k_sift_describe_wave / _kept
  ppsfm::SiftFeature* kept_feats = nullptr;      int32_t* kept_rows = nullptr;      ppsfm::sift::DescriptorWindow* kept_window = nullptr;      size_t cap_kept = 0;      // k_sift_describe_kept
  // the last extraction
  bool extracted = false;
  ppsfm::sift::Geometry geom{};
  std::vector<ppsfm::SiftOctave> octaves;
  std::vector<float> last_raw;
  std::vector<int32_t> last_octave_level;
  std::vector<double> last_angles;
  // or the last batch: one entry per image (then `extracted` is false)
  std::vector<ppsfm::SiftBatchFeatures> batch;
};

using namespace ppsfm;

namespace {

// a buffer of the workspace regrown to at least `count` elements (the old block goes back: the stream has drained whenever this is called with
// work outstanding on it - see the call sites)
template <class T>
int Grow(DeviceBlocks& b, T** p, size_t* cap, size_t count) {
  if (*p && *cap >= count) return PP_OK;
  if (*p) b.Free(p);
  *cap = 0;
  PP_TRY(b.Alloc(p, count));
  *cap = count;
  return PP_OK;
}
template <class T>
int GrowBeside(DeviceBlocks& b, T** p, bool regrow, size_t count) {      // a buffer that shares another one's capacity
  if (*p && !regrow) return PP_OK;
  if (*p) b.Free(p);
  return b.Alloc(p, count);
}

// the counts of one image's extraction (R.cut set); the timing fields are the caller's
void FillReport(const HostResult& R, const Geometry& g, pp_sift_extract_report* report) {
  report->num_octaves = g.O;
  report->num_levels = (int32_t)R.levels.size();
  report->first_level_to_keep = R.cut.first_level_to_keep;
  report->num_features_found = (int64_t)R.angles.size();
  report->num_features = R.cut.num_features;
  report->num_two_orientations = R.two_orientations;
  report->num_windows_cut = R.windows_cut;
  report->num_descriptors_skipped = R.descriptors_skipped;
  for (size_t q = 0; q < R.octaves.size(); ++q) {
    const OctaveCounts& c = R.octaves[q];
    report->octave_width[q] = c.width; report->octave_height[q] = c.height;
    report->octave_candidates[q] = c.num_candidates; report->octave_keypoints[q] = c.num_keypoints;
    report->num_keypoints += c.num_keypoints; report->num_moved += c.moved;
    report->num_rejected_peak += c.reject_peak; report->num_rejected_edge += c.reject_edge;
    report->num_rejected_offset += c.reject_offset; report->num_rejected_bounds += c.reject_bounds;
  }
}

Options FromC(const pp_sift_extract_options& c) {
  Options o;
  o.max_num_features = c.max_num_features; o.first_octave = c.first_octave; o.num_octaves = c.num_octaves; o.octave_resolution = c.octave_resolution;
  o.peak_threshold = c.peak_threshold; o.edge_threshold = c.edge_threshold; o.max_num_orientations = c.max_num_orientations; o.upright = c.upright;
  o.normalization = c.normalization;
  return o;
}

// ---- what pp_sift_extract_batch and pp_sift_extract_to_matcher share: the plan, the event time by phases, a group's way through an octave

enum { kPyramid = 0, kDetect = 1, kGradient = 2, kOrient = 3, kDescribe = 4 };

// the device time of a call: the spans between Begin() and a wait, each counted to the phase that ended in the wait
struct SiftPhases {
  StreamTimer timer;
  hipStream_t s;
  bool split;      // phase_timings: the phases that do not end in a wait get one
  double ms[5] = {0, 0, 0, 0, 0};
  SiftPhases(const DeviceHandle& h, bool phase_timings) : timer(h), s(h.stream), split(phase_timings) {}
  // the span since the last Begin() belongs to `phase`: close it (the wait) and open the next one
  int Close(int phase) {
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(timer.End());
    PP_HIP_TRY(hipStreamSynchronize(s));
    const float before = timer.ms;
    PP_TRY(timer.Add());
    ms[phase] += (double)(timer.ms - before);
    return timer.Begin();
  }
  int Boundary(int phase) { return split ? Close(phase) : PP_OK; }
  int End() {      // the last span, to no phase
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(timer.End());
    PP_HIP_TRY(hipStreamSynchronize(s));
    return timer.Add();
  }
};

// everything the two calls settle before any device work: the options, the filters, every image's layout and the groups
struct SiftBatchPlan {
  Options opt;
  Geometry g;
  SiftFilters filters;
  std::vector<SiftLayout> layouts;
  std::vector<int64_t> bytes_per_image;
  std::vector<int32_t> first;      // PlanSiftBatches: group b is the images first[b] .. first[b + 1] - 1
  int num_groups() const { return (int)first.size() - 1; }
};

// the argument checks of a batch behind the null pointers (in the order pp_sift_extract_batch has always made them), then the plan
int PlanSiftBatch(const char* where, const pp_sift_extract_options* options, int32_t num_images, const pp_sift_batch_image* images, int64_t workspace_bytes,
                  int64_t capacity, SiftBatchPlan* plan) {
  PP_REQUIRE(num_images >= 1, "%s: num_images %d", where, num_images);
  PP_REQUIRE(capacity >= 0, "%s: negative capacity", where);
  PP_REQUIRE(workspace_bytes >= 0, "%s: negative workspace_bytes", where);
  plan->opt = FromC(*options);
  for (int32_t i = 0; i < num_images; ++i) {
    PP_REQUIRE(images[i].grey, "%s: image %d: null argument", where, i);
    const std::string wrong = CheckOptions(plan->opt, images[i].width, images[i].height);
    PP_REQUIRE(wrong.empty(), "%s: image %d: %s", where, i, wrong.c_str());
  }
  plan->g = MakeGeometry(plan->opt);
  PP_TRY(MakeSiftFilters(where, plan->g, &plan->filters));
  const size_t N = (size_t)num_images;
  plan->layouts.resize(N);
  plan->bytes_per_image.resize(N);
  for (size_t i = 0; i < N; ++i) {
    plan->layouts[i] = LayoutOctaves(plan->g, images[i].width, images[i].height);
    const int64_t pixels = (int64_t)images[i].width * images[i].height;
    plan->bytes_per_image[i] = (int64_t)((plan->layouts[i].total + plan->layouts[i].rows_need) * sizeof(float)) + pixels * (int64_t)(sizeof(float) + 1);
  }
  plan->first = PlanSiftBatches(plan->bytes_per_image, workspace_bytes > 0 ? workspace_bytes : (int64_t)8 << 30);
  return PP_OK;
}

// the keypoint buffers regrown to K keypoints (the stream has drained)
int GrowKeys(pp_sift_extractor_impl* h, size_t K) {
  const bool regrow = !h->keys || h->cap_keys < K;
  const size_t want = std::max<size_t>(K, 2 * h->cap_keys);
  if (regrow) { if (h->keys) h->blocks.Free(&h->keys); h->cap_keys = 0; PP_TRY(h->blocks.Alloc(&h->keys, want)); h->cap_keys = want; }
  PP_TRY(GrowBeside(h->blocks, &h->num_angles, regrow, h->cap_keys));
  return GrowBeside(h->blocks, &h->angles, regrow, kMaxAngles * h->cap_keys);
}

// One group of images in the handle's workspace.  Every image has its own slice of the pyramid, of the grey and float images and of the row counts
// (the n candidate totals stand in front of the images' slices).
struct SiftGroup {
  pp_sift_extractor_impl* h;
  const SiftBatchPlan& plan;
  const pp_sift_batch_image* images;
  size_t first, n;
  std::vector<size_t> pyr_off, img_off, rows_off;
  int64_t bytes = 0;
  std::vector<int32_t> totals, cand_off;
  std::vector<Refined> refined;

  SiftGroup(pp_sift_extractor_impl* handle, const SiftBatchPlan& p, const pp_sift_batch_image* ims, int b)
      : h(handle), plan(p), images(ims), first((size_t)p.first[(size_t)b]), n((size_t)p.first[(size_t)b + 1] - first), pyr_off(n), img_off(n), rows_off(n), totals(n),
        cand_off(n) {}
  const SiftOctave& Octave(size_t i, int q) const { return plan.layouts[first + i].octaves[(size_t)q]; }
  float* Pyramid(size_t i) const { return h->pyramid + pyr_off[i]; }

  // the slices, the workspace grown to them (the stream has drained: the call before, or the group before), the images uploaded and converted;
  // table_slots: the image table of the descriptor kernel
  int Begin(SiftPhases* phases, size_t table_slots) {
    hipStream_t s = h->stream;
    size_t pyr_total = 0, img_total = 0, rows_total = n;
    for (size_t i = 0; i < n; ++i) {
      pyr_off[i] = pyr_total; pyr_total += plan.layouts[first + i].total;
      img_off[i] = img_total; img_total += (size_t)images[first + i].width * images[first + i].height;
      rows_off[i] = rows_total; rows_total += plan.layouts[first + i].rows_need;
      bytes += plan.bytes_per_image[first + i];
    }
    PP_TRY(Grow(h->blocks, &h->pyramid, &h->cap_pyramid, pyr_total));
    {
      const bool regrow = !h->image || h->cap_image < img_total;
      PP_TRY(Grow(h->blocks, &h->image, &h->cap_image, img_total));
      PP_TRY(GrowBeside(h->blocks, &h->grey, regrow, h->cap_image));
    }
    PP_TRY(Grow(h->blocks, &h->rows, &h->cap_rows, rows_total));
    PP_TRY(Grow(h->blocks, &h->wave_images, &h->cap_wave_images, table_slots));
    for (size_t i = 0; i < n; ++i) PP_TRY(Upload(h->grey + img_off[i], images[first + i].grey, (size_t)images[first + i].width * images[first + i].height, s));
    PP_TRY(phases->timer.Begin());
    for (size_t i = 0; i < n; ++i) {
      const int64_t pixels = (int64_t)images[first + i].width * images[first + i].height;
      hipLaunchKernelGGL(k_sift_load, SiftGrid(pixels, kSiftBlock), dim3(kSiftBlock), 0, s, pixels, (const uint8_t*)(h->grey + img_off[i]), h->image + img_off[i]);
    }
    return PP_OK;
  }

  // Octave q of every image up to its keypoints, in two waits: pyramid, gradient, candidate counts and their scan image by image, the n totals in one
  // download; then scatter and refinement of every image into one candidate array, the refined candidates in one download.  The keypoints are
  // APPENDED to keys - image i's are the num_keys[i] from key_off[i] on - and the octave's counts to results[first + i].octaves.
  int Keypoints(const char* where, int q, SiftPhases* phases, std::vector<HostResult>* results, std::vector<Keypoint>* keys, int32_t* key_off, int32_t* num_keys) {
    hipStream_t s = h->stream;
    const Geometry& g = plan.g;
    const int o = g.o_min + q, num_grad = g.S;
    const double threshold = 0.8 * plan.opt.peak_threshold;
    for (size_t i = 0; i < n; ++i)
      LaunchOctavePyramid(s, g, plan.filters, (const float*)h->taps, plan.layouts[first + i], q, Pyramid(i), (const float*)(h->image + img_off[i]), images[first + i].width,
                          images[first + i].height);
    PP_TRY(phases->Boundary(kPyramid));
    for (size_t i = 0; i < n; ++i) {
      const SiftOctave& oc = Octave(i, q);
      const int64_t lev = (int64_t)oc.w * oc.h;
      if (oc.has_grad)
        hipLaunchKernelGGL(k_sift_gradient, SiftGrid(lev * num_grad, kSiftBlock), dim3(kSiftBlock), 0, s, Pyramid(i) + oc.grad, (const float*)(Pyramid(i) + oc.gauss + lev), oc.w,
                           oc.h, lev * num_grad);
    }
    PP_TRY(phases->Boundary(kGradient));
    bool any_detect = false;
    for (size_t i = 0; i < n; ++i) {
      const SiftLayout& lay = plan.layouts[first + i];
      const SiftOctave& oc = lay.octaves[(size_t)q];
      if (!(oc.w >= 3 && oc.h >= 3)) continue;
      any_detect = true;
      const int64_t lev = (int64_t)oc.w * oc.h;
      const int rows = g.S * oc.h;
      int32_t* row_count = h->rows + rows_off[i];
      int32_t* row_start = row_count + lay.max_rows;
      int32_t* scan_scratch = row_count + 2 * (size_t)lay.max_rows + 2;
      hipLaunchKernelGGL(k_sift_detect_count, dim3((unsigned)rows), dim3(kSiftBlock), 0, s, (const float*)(Pyramid(i) + oc.dog + lev), oc.w, oc.h, threshold, row_count);
      const ScanJob<int32_t> job{row_count, row_start, h->rows + i};
      LaunchExclusiveScan<int32_t>(s, rows, &job, 1, scan_scratch);
    }
    std::fill(totals.begin(), totals.end(), 0);
    if (any_detect) {
      PP_TRY(Download(totals.data(), (const int32_t*)h->rows, n, s));
      PP_TRY(phases->Close(kDetect));
    }
    size_t num_cand = 0;
    for (size_t i = 0; i < n; ++i) {
      const SiftOctave& oc = Octave(i, q);
      if (!(oc.w >= 3 && oc.h >= 3)) totals[i] = 0;      // (its total was not written)
      cand_off[i] = (int32_t)num_cand;
      num_cand += (size_t)totals[i];
    }
    PP_REQUIRE(num_cand < ((size_t)1 << 31) / 3, "%s: %lld candidates in one octave of a sub-batch", where, (long long)num_cand);
    refined.assign(num_cand, Refined{});
    if (num_cand > 0) {
      {      // (the stream has drained)
        const bool regrow = !h->cand || h->cap_cand < num_cand;
        const size_t want = std::max<size_t>(num_cand, 2 * h->cap_cand);
        if (regrow) { if (h->cand) h->blocks.Free(&h->cand); h->cap_cand = 0; PP_TRY(h->blocks.Alloc(&h->cand, 3 * want)); h->cap_cand = want; }
        PP_TRY(GrowBeside(h->blocks, &h->refined, regrow, h->cap_cand));
      }
      for (size_t i = 0; i < n; ++i) {
        if (totals[i] == 0) continue;
        const SiftLayout& lay = plan.layouts[first + i];
        const SiftOctave& oc = lay.octaves[(size_t)q];
        const int64_t lev = (int64_t)oc.w * oc.h;
        const float* dog = Pyramid(i) + oc.dog;
        const int32_t* row_count = h->rows + rows_off[i];
        int32_t* cand = h->cand + 3 * (size_t)cand_off[i];
        hipLaunchKernelGGL(k_sift_detect_scatter, dim3((unsigned)(g.S * oc.h)), dim3(kSiftBlock), 0, s, dog + lev, oc.w, oc.h, g.s_min + 1, threshold, row_count,
                           row_count + lay.max_rows, cand);
        hipLaunchKernelGGL(k_sift_refine, SiftGrid(totals[i], kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, totals[i], (const int32_t*)cand, dog, oc.w, oc.h, g.s_min,
                           g.s_max, plan.opt.peak_threshold, plan.opt.edge_threshold, h->refined + cand_off[i]);
      }
      PP_TRY(Download(refined.data(), (const Refined*)h->refined, num_cand, s));
      PP_TRY(phases->Close(kDetect));
    }
    for (size_t i = 0; i < n; ++i) {
      const SiftOctave& oc = Octave(i, q);
      OctaveCounts counts{oc.w, oc.h, totals[i], 0, 0, 0, 0, 0, 0};
      key_off[i] = (int32_t)keys->size();
      for (int32_t c = 0; c < totals[i]; ++c) {
        const Refined& r = refined[(size_t)cand_off[i] + (size_t)c];
        counts.moved += r.moves > 0;
        counts.reject_peak += r.reject == 1; counts.reject_edge += r.reject == 2; counts.reject_offset += r.reject == 3; counts.reject_bounds += r.reject == 4;
        if (r.good) keys->push_back(MakeKeypoint(r, o, g));
      }
      num_keys[i] = (int32_t)keys->size() - key_off[i];
      counts.num_keypoints = num_keys[i];
      (*results)[first + i].octaves.push_back(counts);
    }
    return PP_OK;
  }
};

}  // namespace

extern "C" {

void pp_sift_extract_options_default(pp_sift_extract_options* o) {
  if (!o) return;
  const Options d;      // feature/sift.h:46-104
  o->max_num_features = d.max_num_features; o->first_octave = d.first_octave; o->num_octaves = d.num_octaves; o->octave_resolution = d.octave_resolution;
  o->peak_threshold = d.peak_threshold; o->edge_threshold = d.edge_threshold; o->max_num_orientations = d.max_num_orientations; o->upright = d.upright;
  o->normalization = d.normalization; o->phase_timings = 0;
}

int pp_sift_extractor_destroy(pp_sift_extractor_handle h) try {
  delete h;      // (~DeviceHandle)
  return PP_OK;
} PP_API_CATCH("pp_sift_extractor_destroy")

int pp_sift_extractor_create(int device, pp_sift_extractor_handle* out) try {
  const char* where = "pp_sift_extractor_create";
  PP_REQUIRE(out, "%s: null argument", where);
  *out = nullptr;
  PP_TRY(UseDevice(where, device));
  UnderConstruction<pp_sift_extractor_impl, pp_sift_extractor_destroy> h{new pp_sift_extractor_impl()};
  PP_TRY(h->Open(device));
  const std::vector<double> table = ExpnTable();
  PP_TRY(h->blocks.Put(&h->expn, table.data(), table.size(), h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));      // (table is on this frame)
  *out = h.release();
  return PP_OK;
} PP_API_CATCH("pp_sift_extractor_create")

int pp_sift_extract(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t width, int32_t height, const uint8_t* grey,
                    pp_sift_extract_report* report, int64_t capacity, float* keypoints, uint8_t* descriptors, int64_t* num) try {
  const char* where = "pp_sift_extract";
  PP_REQUIRE(options && grey && report && num && keypoints, "%s: null argument", where);
  PP_REQUIRE(capacity >= 0, "%s: negative capacity", where);
  const auto t_begin = Clock::now();
  const Options opt = FromC(*options);
  const std::string wrong = CheckOptions(opt, width, height);
  PP_REQUIRE(wrong.empty(), "%s: %s", where, wrong.c_str());
  PP_REQUIRE(h, "%s: null handle", where);
  const Geometry g = MakeGeometry(opt);
  const int num_grad = g.S;      // gradient levels s_min + 1 .. s_max - 2

  SiftFilters filters;
  PP_TRY(MakeSiftFilters(where, g, &filters));
  const SiftLayout lay = LayoutOctaves(g, width, height);
  std::vector<SiftOctave> octaves = lay.octaves;
  const size_t total = lay.total, rows_need = lay.rows_need;
  const int max_rows = lay.max_rows;
  const std::vector<float>& taps = filters.taps;

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  h->extracted = false;
  h->batch.clear();
  PP_TRY(Grow(h->blocks, &h->pyramid, &h->cap_pyramid, total));
  {
    const bool regrow = !h->image || h->cap_image < (size_t)width * height;
    PP_TRY(Grow(h->blocks, &h->image, &h->cap_image, (size_t)width * height));
    PP_TRY(GrowBeside(h->blocks, &h->grey, regrow, h->cap_image));
  }
  PP_TRY(Grow(h->blocks, &h->rows, &h->cap_rows, rows_need));
  PP_TRY(Grow(h->blocks, &h->taps, &h->cap_taps, taps.size()));
  PP_TRY(Upload(h->taps, taps.data(), taps.size(), s));
  PP_TRY(Upload(h->grey, grey, (size_t)width * height, s));

  StreamTimer timer(*h);
  double phase_ms[5] = {0, 0, 0, 0, 0};
  enum { kPyramid = 0, kDetect = 1, kGradient = 2, kOrient = 3, kDescribe = 4 };
  // the span since the last Begin() belongs to `phase`: close it (the stream is drained) and open the next one
  auto close_span = [&](int phase) -> int {
    PP_HIP_TRY(hipGetLastError());
    PP_TRY(timer.End());
    PP_HIP_TRY(hipStreamSynchronize(s));
    const float before = timer.ms;
    PP_TRY(timer.Add());
    phase_ms[phase] += (double)(timer.ms - before);
    return timer.Begin();
  };
  auto phase_boundary = [&](int phase) -> int { return options->phase_timings ? close_span(phase) : PP_OK; };
  auto grid = SiftGrid;
  HostResult R;      // the containers of the reference, filled octave by octave
  std::vector<Refined> refined;
  std::vector<Keypoint> keys;
  std::vector<int32_t> num_angles, is_of_key, used;
  std::vector<double> angles;
  std::vector<SiftFeature> feats;
  std::vector<DescriptorWindow> window;
  std::memset(report, 0, sizeof(*report));

  PP_TRY(timer.Begin());
  hipLaunchKernelGGL(k_sift_load, grid((int64_t)width * height, kSiftBlock), dim3(kSiftBlock), 0, s, (int64_t)width * height, (const uint8_t*)h->grey, h->image);
  for (int q = 0; q < g.O; ++q) {
    SiftOctave& oc = octaves[(size_t)q];
    const int w = oc.w, hgt = oc.h;
    const int64_t lev = (int64_t)w * hgt;
    float* gauss = h->pyramid + oc.gauss;
    float* dog = h->pyramid + oc.dog;
    float* grad = h->pyramid + oc.grad;
    LaunchOctavePyramid(s, g, filters, (const float*)h->taps, lay, q, h->pyramid, (const float*)h->image, width, height);
    PP_TRY(phase_boundary(kPyramid));
    if (oc.has_grad)
      hipLaunchKernelGGL(k_sift_gradient, grid(lev * num_grad, kSiftBlock), dim3(kSiftBlock), 0, s, grad, (const float*)(gauss + lev), w, hgt, lev * num_grad);
    PP_TRY(phase_boundary(kGradient));
    // ---- detection: count per row, scan, scatter, refine
    const int rows = g.S * hgt;
    int32_t* row_count = h->rows;
    int32_t* row_start = h->rows + max_rows;
    int32_t* d_total = h->rows + 2 * (size_t)max_rows;
    int32_t* scan_scratch = h->rows + 2 * (size_t)max_rows + 2;
    const double threshold = 0.8 * opt.peak_threshold;
    int32_t num_cand = 0;
    if (w >= 3 && hgt >= 3) {
      hipLaunchKernelGGL(k_sift_detect_count, dim3((unsigned)rows), dim3(kSiftBlock), 0, s, (const float*)(dog + lev), w, hgt, threshold, row_count);
      const ScanJob<int32_t> job{row_count, row_start, d_total};
      LaunchExclusiveScan<int32_t>(s, rows, &job, 1, scan_scratch);
      PP_TRY(Download(&num_cand, (const int32_t*)d_total, 1, s));
      PP_TRY(close_span(kDetect));
    }
    oc.cand.assign(3 * (size_t)num_cand, 0);
    refined.assign((size_t)num_cand, Refined{});
    if (num_cand > 0) {
      {      // (the stream has drained)
        const bool regrow = !h->cand || h->cap_cand < (size_t)num_cand;
        const size_t want = std::max<size_t>((size_t)num_cand, 2 * h->cap_cand);
        if (regrow) { if (h->cand) h->blocks.Free(&h->cand); h->cap_cand = 0; PP_TRY(h->blocks.Alloc(&h->cand, 3 * want)); h->cap_cand = want; }
        PP_TRY(GrowBeside(h->blocks, &h->refined, regrow, h->cap_cand));
      }
      hipLaunchKernelGGL(k_sift_detect_scatter, dim3((unsigned)rows), dim3(kSiftBlock), 0, s, (const float*)(dog + lev), w, hgt, g.s_min + 1, threshold,
                         (const int32_t*)row_count, (const int32_t*)row_start, h->cand);
      hipLaunchKernelGGL(k_sift_refine, grid(num_cand, kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, num_cand, (const int32_t*)h->cand, (const float*)dog, w, hgt, g.s_min,
                         g.s_max, opt.peak_threshold, opt.edge_threshold, h->refined);
      PP_TRY(Download(oc.cand.data(), (const int32_t*)h->cand, oc.cand.size(), s));
      PP_TRY(Download(refined.data(), (const Refined*)h->refined, refined.size(), s));
      PP_TRY(close_span(kDetect));
    }
    OctaveCounts counts{w, hgt, num_cand, 0, 0, 0, 0, 0, 0};
    keys.clear();
    for (const Refined& r : refined) {
      counts.moved += r.moves > 0;
      counts.reject_peak += r.reject == 1; counts.reject_edge += r.reject == 2; counts.reject_offset += r.reject == 3; counts.reject_bounds += r.reject == 4;
      if (r.good) keys.push_back(MakeKeypoint(r, oc.o, g));
    }
    counts.num_keypoints = (int32_t)keys.size();
    R.octaves.push_back(counts);
    const size_t K = keys.size();
    if (K == 0) continue;
    // ---- orientations
    const double xper = std::ldexp(1.0, oc.o);
    {
      const bool regrow = !h->keys || h->cap_keys < K;
      const size_t want = std::max<size_t>(K, 2 * h->cap_keys);
      if (regrow) { if (h->keys) h->blocks.Free(&h->keys); h->cap_keys = 0; PP_TRY(h->blocks.Alloc(&h->keys, want)); h->cap_keys = want; }
      PP_TRY(GrowBeside(h->blocks, &h->num_angles, regrow, h->cap_keys));
      PP_TRY(GrowBeside(h->blocks, &h->angles, regrow, kMaxAngles * h->cap_keys));
    }
    if (!opt.upright || descriptors) PP_TRY(Upload(h->keys, keys.data(), K, s));      // (each of the two kernels that read them ends in a drained stream)
    num_angles.assign(K, 1);
    angles.assign(kMaxAngles * K, 0.0);
    if (!opt.upright) {
      hipLaunchKernelGGL(k_sift_orient, grid((int64_t)K, kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, (int32_t)K, (const Keypoint*)h->keys, (const float*)grad, w, hgt, g.s_min,
                         g.s_max, xper, (const double*)h->expn, h->num_angles, h->angles);
      PP_TRY(Download(num_angles.data(), (const int32_t*)h->num_angles, K, s));
      PP_TRY(Download(angles.data(), (const double*)h->angles, kMaxAngles * K, s));
      PP_TRY(close_span(kOrient));
    }
    // ---- the features of the octave, and their descriptors
    is_of_key.resize(K); used.resize(K);
    feats.clear();
    for (size_t i = 0; i < K; ++i) {
      is_of_key[i] = keys[i].is;
      used[i] = std::min(num_angles[i], opt.max_num_orientations);
      R.two_orientations += used[i] >= 2;
      for (int a = 0; a < used[i]; ++a) {
        const double angle = angles[kMaxAngles * i + (size_t)a];
        float row[4];
        FeatureRow(keys[i], angle, row);
        R.keypoints.insert(R.keypoints.end(), row, row + 4);
        R.octave_level.push_back(oc.o); R.octave_level.push_back(keys[i].is);
        R.angles.push_back(angle);
        feats.push_back(SiftFeature{(int32_t)i, 0, angle, std::sin(angle), std::cos(angle)});
      }
    }
    AppendLevels(oc.o, is_of_key.data(), used.data(), (int64_t)K, &R.levels);
    const size_t F = feats.size();
    if (!descriptors || F == 0) {
      R.raw.resize(R.raw.size() + kDescBins * F, 0.f);
      R.descriptors.resize(R.descriptors.size() + kDescBins * F, 0);
      continue;
    }
    {
      const bool regrow = !h->feats || h->cap_feats < F;
      const size_t want = std::max<size_t>(F, 2 * h->cap_feats);
      if (regrow) { if (h->feats) h->blocks.Free(&h->feats); h->cap_feats = 0; PP_TRY(h->blocks.Alloc(&h->feats, want)); h->cap_feats = want; }
      PP_TRY(GrowBeside(h->blocks, &h->raw, regrow, kDescBins * h->cap_feats));
      PP_TRY(GrowBeside(h->blocks, &h->bytes, regrow, kDescBins * h->cap_feats));
      PP_TRY(GrowBeside(h->blocks, &h->window, regrow, h->cap_feats));
    }
    PP_TRY(Upload(h->feats, feats.data(), F, s));
    hipLaunchKernelGGL(k_sift_describe, grid((int64_t)F, kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, (int32_t)F, (const SiftFeature*)h->feats, (const Keypoint*)h->keys,
                       (const float*)grad, w, hgt, g.s_min, g.s_max, xper, (const double*)h->expn, (int)opt.normalization, h->raw, h->bytes, h->window);
    const size_t at = R.raw.size();
    R.raw.resize(at + kDescBins * F);
    R.descriptors.resize(at + kDescBins * F);
    window.resize(F);
    PP_TRY(Download(R.raw.data() + at, (const float*)h->raw, kDescBins * F, s));
    PP_TRY(Download(R.descriptors.data() + at, (const uint8_t*)h->bytes, kDescBins * F, s));
    PP_TRY(Download(window.data(), (const DescriptorWindow*)h->window, F, s));
    PP_TRY(close_span(kDescribe));
    for (const DescriptorWindow& win : window) { R.windows_cut += win.cut; R.descriptors_skipped += !win.computed; }
  }
  PP_HIP_TRY(hipGetLastError());
  PP_TRY(timer.End());
  PP_HIP_TRY(hipStreamSynchronize(s));
  PP_TRY(timer.Add());

  // ---- the host rule
  R.cut = SelectLevels(R.levels, opt.max_num_features);
  FillReport(R, g, report);
  for (int p = 0; p < 5; ++p) report->phase_ms[p] = options->phase_timings ? phase_ms[p] : 0.0;
  report->device_ms = timer.ms;
  h->geom = g;
  h->octaves = std::move(octaves);
  h->last_raw = std::move(R.raw);
  h->last_octave_level = std::move(R.octave_level);
  h->last_angles = std::move(R.angles);
  h->extracted = true;
  *num = R.cut.num_features;
  report->total_ms = MsSince(t_begin);
  PP_REQUIRE(capacity >= R.cut.num_features, "%s: capacity %lld for %lld features", where, (long long)capacity, (long long)R.cut.num_features);
  const size_t first = (size_t)R.cut.first_feature, count = (size_t)R.cut.num_features;
  if (count) std::memcpy(keypoints, R.keypoints.data() + 4 * first, 4 * count * sizeof(float));
  if (count && descriptors) std::memcpy(descriptors, R.descriptors.data() + kDescBins * first, kDescBins * count);
  report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_sift_extract")

int pp_sift_extract_stage(pp_sift_extractor_handle h, int32_t kind, int32_t octave, int32_t level, float* out, int64_t capacity, int32_t* width,
                          int32_t* height) try {
  const char* where = "pp_sift_extract_stage";
  PP_REQUIRE(h && out && width && height, "%s: null argument", where);
  PP_REQUIRE(h->extracted, "%s: no extraction on this handle", where);
  const Geometry& g = h->geom;
  PP_REQUIRE(octave >= g.o_min && octave < g.o_min + g.O, "%s: octave %d", where, octave);
  const SiftOctave& oc = h->octaves[(size_t)(octave - g.o_min)];
  const size_t lev = (size_t)oc.w * oc.h;
  size_t offset = 0, count = lev;
  if (kind == 0) {
    PP_REQUIRE(level >= g.s_min && level <= g.s_max, "%s: Gaussian level %d", where, level);
    offset = oc.gauss + (size_t)(level - g.s_min) * lev;
  } else if (kind == 1) {
    PP_REQUIRE(level >= g.s_min && level <= g.s_max - 1, "%s: DoG level %d", where, level);
    offset = oc.dog + (size_t)(level - g.s_min) * lev;
  } else {
    PP_REQUIRE(kind == 2, "%s: kind %d", where, kind);
    PP_REQUIRE(oc.has_grad && level >= g.s_min + 1 && level <= g.s_max - 2, "%s: gradient level %d", where, level);
    offset = oc.grad + 2 * (size_t)(level - g.s_min - 1) * lev;
    count = 2 * lev;
  }
  *width = oc.w; *height = oc.h;
  PP_REQUIRE(capacity >= (int64_t)count, "%s: capacity %lld for %lld floats", where, (long long)capacity, (long long)count);
  PP_HIP_TRY(hipSetDevice(h->device));
  PP_TRY(Download(out, (const float*)(h->pyramid + offset), count, h->stream));
  PP_HIP_TRY(hipStreamSynchronize(h->stream));
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_stage")

int pp_sift_extract_candidates(pp_sift_extractor_handle h, int32_t octave, int32_t* xys, int64_t capacity, int64_t* num) try {
  const char* where = "pp_sift_extract_candidates";
  PP_REQUIRE(h && num, "%s: null argument", where);
  PP_REQUIRE(h->extracted, "%s: no extraction on this handle", where);
  PP_REQUIRE(octave >= h->geom.o_min && octave < h->geom.o_min + h->geom.O, "%s: octave %d", where, octave);
  const std::vector<int32_t>& c = h->octaves[(size_t)(octave - h->geom.o_min)].cand;
  *num = (int64_t)(c.size() / 3);
  PP_REQUIRE(xys || c.empty(), "%s: null argument", where);
  PP_REQUIRE(capacity >= *num, "%s: capacity %lld for %lld candidates", where, (long long)capacity, (long long)*num);
  if (!c.empty()) std::memcpy(xys, c.data(), c.size() * sizeof(int32_t));
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_candidates")

int pp_sift_extract_features(pp_sift_extractor_handle h, float* raw, int32_t* octave_level, double* angles, int64_t capacity, int64_t* num) try {
  const char* where = "pp_sift_extract_features";
  PP_REQUIRE(h && num, "%s: null argument", where);
  PP_REQUIRE(h->extracted, "%s: no extraction on this handle", where);
  const size_t n = h->last_angles.size();
  *num = (int64_t)n;
  PP_REQUIRE(capacity >= *num, "%s: capacity %lld for %lld features", where, (long long)capacity, (long long)*num);
  if (n && raw) std::memcpy(raw, h->last_raw.data(), kDescBins * n * sizeof(float));
  if (n && octave_level) std::memcpy(octave_level, h->last_octave_level.data(), 2 * n * sizeof(int32_t));
  if (n && angles) std::memcpy(angles, h->last_angles.data(), n * sizeof(double));
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_features")

// K23: the images of a sub-batch go through the octaves in lock-step.  Every image has its own slice of the pyramid, of the grey and float images and
// of the row counts, and the kernels of the single call run on those slices; what the host must know before it can go on - the candidate totals, the
// refined candidates, the orientations, the descriptors - comes back for ALL images of the sub-batch in one download and one wait each.
int pp_sift_extract_batch(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t num_images, const pp_sift_batch_image* images,
                          int64_t workspace_bytes, pp_sift_batch_report* batch_report, pp_sift_extract_report* reports, int64_t capacity, float* keypoints,
                          uint8_t* descriptors, int64_t* offsets) try {
  const char* where = "pp_sift_extract_batch";
  PP_REQUIRE(options && images && batch_report && reports && keypoints && offsets, "%s: null argument", where);
  const auto t_begin = Clock::now();
  SiftBatchPlan plan;
  PP_TRY(PlanSiftBatch(where, options, num_images, images, workspace_bytes, capacity, &plan));
  PP_REQUIRE(h, "%s: null handle", where);
  const Options& opt = plan.opt;
  const Geometry& g = plan.g;
  const std::vector<SiftLayout>& layouts = plan.layouts;
  const size_t N = (size_t)num_images;
  const int num_sub_batches = plan.num_groups();

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  h->extracted = false;
  h->batch.clear();
  PP_TRY(Grow(h->blocks, &h->taps, &h->cap_taps, plan.filters.taps.size()));
  PP_TRY(Upload(h->taps, plan.filters.taps.data(), plan.filters.taps.size(), s));

  SiftPhases phases(*h, options->phase_timings != 0);
  std::vector<HostResult> results(N);      // the containers of the reference, per image, filled octave by octave
  int64_t workspace_used = 0;
  for (int b = 0; b < num_sub_batches; ++b) {
    SiftGroup group(h, plan, images, b);
    const size_t first = group.first, n = group.n;
    PP_TRY(group.Begin(&phases, n));
    workspace_used = std::max(workspace_used, group.bytes);

    std::vector<int32_t> key_off(n), num_keys(n), feat_off(n), num_feats(n);
    std::vector<Keypoint> keys;
    std::vector<int32_t> num_angles, is_of_key, used;
    std::vector<double> angles;
    std::vector<SiftFeature> feats;
    std::vector<SiftWaveImage> table(n);
    std::vector<DescriptorWindow> window;

    for (int q = 0; q < g.O; ++q) {
      const int o = g.o_min + q;
      keys.clear();
      PP_TRY(group.Keypoints(where, q, &phases, &results, &keys, key_off.data(), num_keys.data()));
      const size_t K = keys.size();
      if (K == 0) continue;
      // ---- orientations: the keys of every image uploaded together
      const double xper = std::ldexp(1.0, o);
      PP_TRY(GrowKeys(h, K));
      if (!opt.upright || descriptors) PP_TRY(Upload(h->keys, keys.data(), K, s));
      num_angles.assign(K, 1);
      angles.assign(kMaxAngles * K, 0.0);
      if (!opt.upright) {
        for (size_t i = 0; i < n; ++i) {
          if (num_keys[i] == 0) continue;
          const SiftOctave& oc = layouts[first + i].octaves[(size_t)q];
          hipLaunchKernelGGL(k_sift_orient, SiftGrid(num_keys[i], kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, num_keys[i], (const Keypoint*)(h->keys + key_off[i]),
                             (const float*)(group.Pyramid(i) + oc.grad), oc.w, oc.h, g.s_min, g.s_max, xper, (const double*)h->expn, h->num_angles + key_off[i],
                             h->angles + kMaxAngles * (size_t)key_off[i]);
        }
        PP_TRY(Download(num_angles.data(), (const int32_t*)h->num_angles, K, s));
        PP_TRY(Download(angles.data(), (const double*)h->angles, kMaxAngles * K, s));
        PP_TRY(phases.Close(kOrient));
      }
      // ---- the features of the octave: per image into its containers, all of them into one descriptor launch
      feats.clear();
      for (size_t i = 0; i < n; ++i) {
        HostResult& R = results[first + i];
        const size_t K_i = (size_t)num_keys[i], k0 = (size_t)key_off[i];
        feat_off[i] = (int32_t)feats.size();
        is_of_key.resize(K_i); used.resize(K_i);
        for (size_t j = 0; j < K_i; ++j) {
          const Keypoint& key = keys[k0 + j];
          is_of_key[j] = key.is;
          used[j] = std::min(num_angles[k0 + j], opt.max_num_orientations);
          R.two_orientations += used[j] >= 2;
          for (int a = 0; a < used[j]; ++a) {
            const double angle = angles[kMaxAngles * (k0 + j) + (size_t)a];
            float row[4];
            FeatureRow(key, angle, row);
            R.keypoints.insert(R.keypoints.end(), row, row + 4);
            R.octave_level.push_back(o); R.octave_level.push_back(key.is);
            R.angles.push_back(angle);
            feats.push_back(SiftFeature{(int32_t)(k0 + j), (int32_t)i, angle, std::sin(angle), std::cos(angle)});
          }
        }
        num_feats[i] = (int32_t)feats.size() - feat_off[i];
        AppendLevels(o, is_of_key.data(), used.data(), (int64_t)K_i, &R.levels);
      }
      const size_t F = feats.size();
      if (!descriptors || F == 0) {
        for (size_t i = 0; i < n; ++i) {
          HostResult& R = results[first + i];
          R.raw.resize(R.raw.size() + kDescBins * (size_t)num_feats[i], 0.f);
          R.descriptors.resize(R.descriptors.size() + kDescBins * (size_t)num_feats[i], 0);
        }
        continue;
      }
      {
        const bool regrow = !h->feats || h->cap_feats < F;
        const size_t want = std::max<size_t>(F, 2 * h->cap_feats);
        if (regrow) { if (h->feats) h->blocks.Free(&h->feats); h->cap_feats = 0; PP_TRY(h->blocks.Alloc(&h->feats, want)); h->cap_feats = want; }
        PP_TRY(GrowBeside(h->blocks, &h->raw, regrow, kDescBins * h->cap_feats));
        PP_TRY(GrowBeside(h->blocks, &h->bytes, regrow, kDescBins * h->cap_feats));
        PP_TRY(GrowBeside(h->blocks, &h->window, regrow, h->cap_feats));
      }
      for (size_t i = 0; i < n; ++i) {
        const SiftOctave& oc = layouts[first + i].octaves[(size_t)q];
        table[i] = SiftWaveImage{group.Pyramid(i) + oc.grad, oc.w, oc.h, xper};
      }
      PP_TRY(Upload(h->wave_images, table.data(), n, s));
      PP_TRY(Upload(h->feats, feats.data(), F, s));
      hipLaunchKernelGGL(k_sift_describe_wave, dim3((unsigned)F), dim3(kWave), 0, s, (const SiftFeature*)h->feats, (const Keypoint*)h->keys,
                         (const SiftWaveImage*)h->wave_images, g.s_min, g.s_max, (const double*)h->expn, (int)opt.normalization, h->raw, h->bytes, h->window);
      window.resize(F);
      for (size_t i = 0; i < n; ++i) {      // each image's rows straight into its containers (no second copy on the host), then the one wait
        HostResult& R = results[first + i];
        const size_t f0 = (size_t)feat_off[i], F_i = (size_t)num_feats[i], at = R.raw.size();
        R.raw.resize(at + kDescBins * F_i);
        R.descriptors.resize(at + kDescBins * F_i);
        PP_TRY(Download(R.raw.data() + at, (const float*)(h->raw + kDescBins * f0), kDescBins * F_i, s));
        PP_TRY(Download(R.descriptors.data() + at, (const uint8_t*)(h->bytes + kDescBins * f0), kDescBins * F_i, s));
      }
      PP_TRY(Download(window.data(), (const DescriptorWindow*)h->window, F, s));
      PP_TRY(phases.Close(kDescribe));
      for (size_t i = 0; i < n; ++i) {
        HostResult& R = results[first + i];
        for (size_t f = (size_t)feat_off[i]; f < (size_t)feat_off[i] + (size_t)num_feats[i]; ++f) { R.windows_cut += window[f].cut; R.descriptors_skipped += !window[f].computed; }
      }
    }
    PP_TRY(phases.End());
  }

  // ---- the host rule, per image
  std::memset(batch_report, 0, sizeof(*batch_report));
  offsets[0] = 0;
  for (size_t i = 0; i < N; ++i) {
    HostResult& R = results[i];
    R.cut = SelectLevels(R.levels, opt.max_num_features);
    std::memset(&reports[i], 0, sizeof(reports[i]));
    FillReport(R, g, &reports[i]);
    offsets[i + 1] = offsets[i] + R.cut.num_features;
  }
  batch_report->num_images = num_images;
  batch_report->num_sub_batches = num_sub_batches;
  batch_report->num_features = offsets[N];
  batch_report->workspace_bytes = workspace_used;
  for (int p = 0; p < 5; ++p) batch_report->phase_ms[p] = options->phase_timings ? phases.ms[p] : 0.0;
  batch_report->device_ms = phases.timer.ms;
  h->batch.resize(N);
  for (size_t i = 0; i < N; ++i) {
    h->batch[i].raw = std::move(results[i].raw);
    h->batch[i].octave_level = std::move(results[i].octave_level);
    h->batch[i].angles = std::move(results[i].angles);
  }
  batch_report->total_ms = MsSince(t_begin);
  PP_REQUIRE(capacity >= offsets[N], "%s: capacity %lld for %lld features", where, (long long)capacity, (long long)offsets[N]);
  for (size_t i = 0; i < N; ++i) {
    const HostResult& R = results[i];
    const size_t from = (size_t)R.cut.first_feature, count = (size_t)R.cut.num_features, at = (size_t)offsets[i];
    if (count) std::memcpy(keypoints + 4 * at, R.keypoints.data() + 4 * from, 4 * count * sizeof(float));
    if (count && descriptors) std::memcpy(descriptors + kDescBins * at, R.descriptors.data() + kDescBins * from, kDescBins * count);
  }
  batch_report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_batch")

// K24: pp_sift_extract_batch with the cut BEFORE the orientations and the descriptors, and the matcher as the way out.  Pass 1 takes a group through
// the octaves up to its keypoints (SiftGroup::Keypoints, two waits per octave); the keypoints stay on the host, every octave's gradient levels in the
// workspace.  The cut reads the keypoint counts alone (SelectKeptKeypoints).  Pass 2 runs on what is kept: the kept keypoints of all octaves in one
// upload, k_sift_orient per (octave, image) and one wait, then ONE launch of k_sift_describe_kept over all octaves that writes the matcher's store,
// and one wait: 2 x octaves + 2 waits for a group.  The store belongs to the new pp_sift_handle and is written on the extractor's stream, which has
// drained before the handle is handed out or, on an error, destroyed.
int pp_sift_extract_to_matcher(pp_sift_extractor_handle h, const pp_sift_extract_options* options, int32_t num_images, const pp_sift_batch_image* images,
                               int64_t workspace_bytes, pp_sift_batch_report* batch_report, pp_sift_extract_report* reports, int64_t capacity, float* keypoints,
                               int64_t* offsets, pp_sift_handle* matcher) try {
  const char* where = "pp_sift_extract_to_matcher";
  PP_REQUIRE(matcher, "%s: null argument", where);
  *matcher = nullptr;
  PP_REQUIRE(options && images && batch_report && reports && keypoints && offsets, "%s: null argument", where);
  const auto t_begin = Clock::now();
  SiftBatchPlan plan;
  PP_TRY(PlanSiftBatch(where, options, num_images, images, workspace_bytes, capacity, &plan));
  PP_REQUIRE(h, "%s: null handle", where);
  const Options& opt = plan.opt;
  const Geometry& g = plan.g;
  const size_t N = (size_t)num_images, O = (size_t)g.O;

  PP_HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  h->extracted = false;
  h->batch.clear();
  UnderConstruction<pp_sift_impl, pp_sift_destroy> m{new pp_sift_impl()};
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};      // (destroyed before m: nothing writes the store when it goes back)
  PP_TRY(m->Open(h->device));
  m->num_images = num_images;
  size_t store_rows = 0;      // what the matcher's store holds; the rows of the groups so far are filled
  // the store regrown to `rows`, the `filled` first ones carried over by a copy on the extractor's stream; the old blocks go back behind a wait
  auto grow_store = [&](size_t rows, size_t filled) -> int {
    int8_t* desc = nullptr;
    int32_t* off = nullptr;
    PP_TRY(AllocSiftStore(m->blocks, (int64_t)rows, &desc, &off));
    if (m->d_desc) {
      if (filled) {
        PP_HIP_TRY(hipMemcpyAsync(desc, m->d_desc, filled * kDescBins, hipMemcpyDeviceToDevice, s));
        PP_HIP_TRY(hipMemcpyAsync(off, m->d_off, filled * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
      }
      PP_HIP_TRY(hipStreamSynchronize(s));
      m->blocks.Free(&m->d_desc); m->blocks.Free(&m->d_off);
    }
    m->d_desc = desc; m->d_off = off; store_rows = rows;
    return PP_OK;
  };
  PP_TRY(Grow(h->blocks, &h->taps, &h->cap_taps, plan.filters.taps.size()));
  PP_TRY(Upload(h->taps, plan.filters.taps.data(), plan.filters.taps.size(), s));

  SiftPhases phases(*h, options->phase_timings != 0);
  std::vector<HostResult> results(N);      // levels (keypoint counts), octaves, cut and the kept-only counts; keypoints: the kept rows
  std::vector<int64_t> row0(N + 1, 0);     // image i's first row in the store: the offsets
  int64_t workspace_used = 0;
  for (int b = 0; b < plan.num_groups(); ++b) {
    SiftGroup group(h, plan, images, b);
    const size_t first = group.first, n = group.n;
    PP_TRY(group.Begin(&phases, O * n));
    workspace_used = std::max(workspace_used, group.bytes);
    // ---- pass 1: the keypoints of every octave, block q * n + i = (octave q, image i)
    std::vector<Keypoint> keys, kept;
    std::vector<int32_t> key_off(O * n), num_keys(O * n), kept_off(O * n), kept_num(O * n), is_of_key, none;
    for (size_t q = 0; q < O; ++q) {
      PP_TRY(group.Keypoints(where, (int)q, &phases, &results, &keys, key_off.data() + q * n, num_keys.data() + q * n));
      for (size_t i = 0; i < n; ++i) {
        const size_t K_i = (size_t)num_keys[q * n + i], k0 = (size_t)key_off[q * n + i];
        is_of_key.resize(K_i); none.assign(K_i, 0);
        for (size_t j = 0; j < K_i; ++j) is_of_key[j] = keys[k0 + j].is;
        AppendLevels(g.o_min + (int)q, is_of_key.data(), none.data(), (int64_t)K_i, &results[first + i].levels);
      }
    }
    // ---- the cut
    std::vector<KeptCut> cuts(n);
    for (size_t i = 0; i < n; ++i) cuts[i] = SelectKeptKeypoints(results[first + i].levels, opt.max_num_features, g.o_min, g.O);
    for (size_t q = 0; q < O; ++q)
      for (size_t i = 0; i < n; ++i) {
        const KeptRange& r = cuts[i].octaves[q];
        kept_off[q * n + i] = (int32_t)kept.size(); kept_num[q * n + i] = (int32_t)r.count;
        const auto from = keys.begin() + key_off[q * n + i] + r.first;
        kept.insert(kept.end(), from, from + r.count);
      }
    // ---- pass 2: orientations of the kept keypoints
    const size_t K = kept.size();
    std::vector<int32_t> num_angles(K, 1);
    std::vector<double> angles(kMaxAngles * K, 0.0);
    if (K > 0) {
      PP_TRY(GrowKeys(h, K));      // (nothing outstanding on the stream reads these)
      PP_TRY(Upload(h->keys, kept.data(), K, s));
    }
    if (K > 0 && !opt.upright) {
      for (size_t q = 0; q < O; ++q)
        for (size_t i = 0; i < n; ++i) {
          const int32_t K_b = kept_num[q * n + i], k0 = kept_off[q * n + i];
          if (K_b == 0) continue;
          const SiftOctave& oc = group.Octave(i, (int)q);
          hipLaunchKernelGGL(k_sift_orient, SiftGrid(K_b, kSiftLaneBlock), dim3(kSiftLaneBlock), 0, s, K_b, (const Keypoint*)(h->keys + k0), (const float*)(group.Pyramid(i) + oc.grad),
                             oc.w, oc.h, g.s_min, g.s_max, std::ldexp(1.0, oc.o), (const double*)h->expn, h->num_angles + k0, h->angles + kMaxAngles * (size_t)k0);
        }
      PP_TRY(Download(num_angles.data(), (const int32_t*)h->num_angles, K, s));
      PP_TRY(Download(angles.data(), (const double*)h->angles, kMaxAngles * K, s));
      PP_TRY(phases.Close(kOrient));
    }
    // ---- the features in the reference's order per image, and their rows in the store
    std::vector<SiftFeature> feats;
    std::vector<int64_t> counts(O * n, 0);
    for (size_t q = 0; q < O; ++q)
      for (size_t i = 0; i < n; ++i) {
        HostResult& R = results[first + i];
        for (int32_t j = kept_off[q * n + i]; j < kept_off[q * n + i] + kept_num[q * n + i]; ++j) {
          const Keypoint& key = kept[(size_t)j];
          const int used = std::min(num_angles[(size_t)j], opt.max_num_orientations);
          R.two_orientations += used >= 2;
          for (int a = 0; a < used; ++a) {
            const double angle = angles[kMaxAngles * (size_t)j + (size_t)a];
            float row[4];
            FeatureRow(key, angle, row);
            R.keypoints.insert(R.keypoints.end(), row, row + 4);
            feats.push_back(SiftFeature{j, (int32_t)(q * n + i), angle, std::sin(angle), std::cos(angle)});
          }
          counts[q * n + i] += used;
        }
      }
    for (size_t i = 0; i < n; ++i) row0[first + i + 1] = row0[first + i] + (int64_t)(results[first + i].keypoints.size() / 4);
    PP_REQUIRE(SiftRowsFit(row0[first + n]), "%s: too many descriptors", where);
    const std::vector<int64_t> block_row = KeptBlockRows(counts, O, n, row0.data() + first);
    const size_t F = feats.size();
    std::vector<int32_t> rows;
    rows.reserve(F);
    for (size_t blk = 0; blk < O * n; ++blk)
      for (int64_t c = 0; c < counts[blk]; ++c) rows.push_back((int32_t)(block_row[blk] + c));
    // ---- the descriptors of the group: one launch into the store
    if (F > 0) {
      const size_t filled = (size_t)row0[first], need = (size_t)row0[first + n];
      if (need > store_rows) PP_TRY(grow_store(b + 1 == plan.num_groups() ? need : std::max(need, 2 * store_rows), filled));
      {
        const bool regrow = !h->kept_feats || h->cap_kept < F;
        const size_t want = std::max<size_t>(F, 2 * h->cap_kept);
        if (regrow) { if (h->kept_feats) h->blocks.Free(&h->kept_feats); h->cap_kept = 0; PP_TRY(h->blocks.Alloc(&h->kept_feats, want)); h->cap_kept = want; }
        PP_TRY(GrowBeside(h->blocks, &h->kept_rows, regrow, h->cap_kept));
        PP_TRY(GrowBeside(h->blocks, &h->kept_window, regrow, h->cap_kept));
      }
      std::vector<SiftWaveImage> table(O * n);
      for (size_t q = 0; q < O; ++q)
        for (size_t i = 0; i < n; ++i) {
          const SiftOctave& oc = group.Octave(i, (int)q);
          table[q * n + i] = SiftWaveImage{group.Pyramid(i) + oc.grad, oc.w, oc.h, std::ldexp(1.0, oc.o)};
        }
      PP_TRY(Upload(h->wave_images, table.data(), table.size(), s));
      PP_TRY(Upload(h->kept_feats, feats.data(), F, s));
      PP_TRY(Upload(h->kept_rows, rows.data(), F, s));
      hipLaunchKernelGGL(k_sift_describe_kept, dim3((unsigned)F), dim3(kWave), 0, s, (const SiftFeature*)h->kept_feats, (const Keypoint*)h->keys,
                         (const SiftWaveImage*)h->wave_images, (const int32_t*)h->kept_rows, g.s_min, g.s_max, (const double*)h->expn, (int)opt.normalization, m->d_desc,
                         m->d_off, h->kept_window);
      std::vector<DescriptorWindow> window(F);
      PP_TRY(Download(window.data(), (const DescriptorWindow*)h->kept_window, F, s));
      PP_TRY(phases.Close(kDescribe));
      for (size_t f = 0; f < F; ++f) {
        HostResult& R = results[first + (size_t)feats[f].image % n];
        R.windows_cut += window[f].cut; R.descriptors_skipped += !window[f].computed;
      }
    }
    for (size_t i = 0; i < n; ++i) results[first + i].cut = Cut{cuts[i].first_level_to_keep, 0, row0[first + i + 1] - row0[first + i]};
    PP_TRY(phases.End());
  }
  if (!m->d_desc) PP_TRY(grow_store(0, 0));      // no feature in any image: the blocks of an empty handle
  m->desc_start = row0;

  // ---- the reports: FillReport's counts; the four that follow the features cover the kept ones, nothing else was computed
  std::memset(batch_report, 0, sizeof(*batch_report));
  for (size_t i = 0; i < N; ++i) {
    std::memset(&reports[i], 0, sizeof(reports[i]));
    FillReport(results[i], g, &reports[i]);
    reports[i].num_features_found = reports[i].num_features;
    offsets[i] = row0[i];
  }
  offsets[N] = row0[N];
  batch_report->num_images = num_images;
  batch_report->num_sub_batches = plan.num_groups();
  batch_report->num_features = offsets[N];
  batch_report->workspace_bytes = workspace_used;
  for (int p = 0; p < 5; ++p) batch_report->phase_ms[p] = options->phase_timings ? phases.ms[p] : 0.0;
  batch_report->device_ms = phases.timer.ms;
  batch_report->total_ms = MsSince(t_begin);
  PP_REQUIRE(capacity >= offsets[N], "%s: capacity %lld for %lld features", where, (long long)capacity, (long long)offsets[N]);
  for (size_t i = 0; i < N; ++i)
    if (!results[i].keypoints.empty()) std::memcpy(keypoints + 4 * (size_t)offsets[i], results[i].keypoints.data(), results[i].keypoints.size() * sizeof(float));
  *matcher = m.release();
  batch_report->total_ms = MsSince(t_begin);
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_to_matcher")

int pp_sift_extract_batch_features(pp_sift_extractor_handle h, int32_t image, float* raw, int32_t* octave_level, double* angles, int64_t capacity,
                                   int64_t* num) try {
  const char* where = "pp_sift_extract_batch_features";
  PP_REQUIRE(h && num, "%s: null argument", where);
  PP_REQUIRE(!h->batch.empty(), "%s: no batch on this handle", where);
  PP_REQUIRE(image >= 0 && (size_t)image < h->batch.size(), "%s: image %d of %lld", where, image, (long long)h->batch.size());
  const SiftBatchFeatures& b = h->batch[(size_t)image];
  const size_t n = b.angles.size();
  *num = (int64_t)n;
  PP_REQUIRE(capacity >= *num, "%s: capacity %lld for %lld features", where, (long long)capacity, (long long)*num);
  if (n && raw) std::memcpy(raw, b.raw.data(), kDescBins * n * sizeof(float));
  if (n && octave_level) std::memcpy(octave_level, b.octave_level.data(), 2 * n * sizeof(int32_t));
  if (n && angles) std::memcpy(angles, b.angles.data(), n * sizeof(double));
  return PP_OK;
} PP_API_CATCH("pp_sift_extract_batch_features")

}  // extern "C"
