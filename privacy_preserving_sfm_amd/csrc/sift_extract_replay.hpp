// K21 - the host half of SIFT extraction: what ExtractSiftFeaturesCPU (reference src/feature/sift.cc:399-573) and vl_sift_new / _vl_sift_smooth
// (lib/VLFeat/sift.c) decide or compute OUTSIDE the per-pixel and per-keypoint arithmetic of sift_core.hpp.  Std only.
//   - the option check (SiftExtractionOptions::Check and this project's own refusals) and the scale-space geometry;
//   - everything that needs libm: the Gaussian taps and the exp table (exp), the smoothing sigmas (pow, sqrt), a keypoint's sigma (pow), the
//     descriptor's rotation (sin, cos).  The device never evaluates one of these, so the host's libm is the only one in the result;
//   - the per-level containers, level_num_features (a keypoint without an orientation counts) and the max_num_features cut from the coarsest level
//     down (sift.cc:534-570);
//   - ExtractOnHost: the whole extraction run serially through the functions of sift_core.hpp - the CPU mirror of sift_extract.hip, with the
//     descriptor by either route: Descriptor() as the lane-per-feature kernel calls it, or the wavefront scheme of k_sift_describe_wave replayed
//     with 64 "lanes" in a loop;
//   - PlanSiftBatches: how pp_sift_extract_batch splits its images into sub-batches under a workspace target;
//   - SelectKeptKeypoints, KeptBlockRows: the cut from the keypoint counts alone and the rows of the kept features in the matcher's store
//     (pp_sift_extract_to_matcher).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "sift_core.hpp"

namespace ppsfm {
namespace sift {

struct Options {
  int32_t max_num_features = 8192, first_octave = -1, num_octaves = 4, octave_resolution = 3;
  double peak_threshold = 0.02 / 3.0, edge_threshold = 10.0;
  int32_t max_num_orientations = 2, upright = 0, normalization = 0;      // 0 L1_ROOT, 1 L2
};

constexpr int kMaxFilterHalfWidth = 64;      // the widest filter the pyramid kernel stages (octave_resolution 1 needs 45)
constexpr int kMaxOctaveShift = 8;

inline int ShiftLeft(int v, int n) { return n >= 0 ? v << n : v >> -n; }      // VL_SHIFT_LEFT

// empty: the extraction can run; else why not
inline std::string CheckOptions(const Options& o, int64_t width, int64_t height) {
  if (width <= 0 || height <= 0) return "the image size must be positive";
  if (!(o.max_num_features > 0)) return "max_num_features must be positive";
  if (!(o.octave_resolution > 0)) return "octave_resolution must be positive";
  if (o.octave_resolution > 32) return "octave_resolution above 32";
  if (!(o.peak_threshold > 0.0)) return "peak_threshold must be positive";
  if (!(o.edge_threshold > 0.0)) return "edge_threshold must be positive";
  if (!(o.max_num_orientations > 0)) return "max_num_orientations must be positive";
  if (o.max_num_orientations > kMaxAngles) return "max_num_orientations above 4: an orientation histogram gives at most four";
  if (o.normalization != 0 && o.normalization != 1) return "unknown normalization";
  if (o.num_octaves <= 0 || o.num_octaves > 32) return "num_octaves must be in 1 .. 32";
  if (o.first_octave < -kMaxOctaveShift || o.first_octave > kMaxOctaveShift) return "first_octave outside -8 .. 8";
  if (width >= (1 << 20) || height >= (1 << 20)) return "the first octave overflows int32 indexing";
  const int64_t w0 = o.first_octave < 0 ? width << -o.first_octave : width >> o.first_octave;
  const int64_t h0 = o.first_octave < 0 ? height << -o.first_octave : height >> o.first_octave;
  if (2 * w0 * h0 >= (int64_t)1 << 31 || w0 >= (1 << 21) || h0 >= (1 << 21)) return "the first octave overflows int32 indexing";
  const int last = o.first_octave + o.num_octaves - 1;
  if (last > kMaxOctaveShift + 32 || (last > 0 && ((width >> std::min(last, 30)) < 1 || (height >> std::min(last, 30)) < 1)) || w0 < 1 || h0 < 1)
    return "the last octave would be empty";
  return std::string();
}

struct Geometry {
  int O, S, o_min, s_min, s_max;
  double sigman, sigmak, sigma0, dsigma0;
  int levels() const { return s_max - s_min + 1; }
};

inline Geometry MakeGeometry(const Options& o) {
  Geometry g;
  g.O = o.num_octaves; g.S = o.octave_resolution; g.o_min = o.first_octave; g.s_min = -1; g.s_max = g.S + 1;
  g.sigman = 0.5;
  g.sigmak = std::pow(2.0, 1.0 / g.S);
  g.sigma0 = 1.6 * g.sigmak;
  g.dsigma0 = g.sigma0 * std::sqrt(1.0 - 1.0 / (g.sigmak * g.sigmak));
  return g;
}

// The smoothing of the octave's first level (0: none) and of every further level from the one before
inline double FirstLevelSigma(const Geometry& g, bool first_octave) {
  double sa, sb;
  if (first_octave) {
    sa = g.sigma0 * std::pow(g.sigmak, g.s_min);
    sb = g.sigman * std::pow(2.0, -g.o_min);
  } else {
    const int s_best = std::min(g.s_min + g.S, g.s_max);
    sa = g.sigma0 * powf((float)g.sigmak, (float)g.s_min);
    sb = g.sigma0 * powf((float)g.sigmak, (float)(s_best - g.S));
  }
  return sa > sb ? std::sqrt(sa * sa - sb * sb) : 0.0;
}
inline double LevelSigma(const Geometry& g, int s) { return g.dsigma0 * std::pow(g.sigmak, s); }

// the 2 W + 1 normalised taps of _vl_sift_smooth, W = max(ceil(4 sigma), 1)
inline std::vector<float> GaussTaps(double sigma) {
  const int W = (int)std::max(std::ceil(4.0 * sigma), 1.0);
  std::vector<float> taps(2 * (size_t)W + 1);
  float acc = 0;
  for (int j = 0; j < 2 * W + 1; ++j) {
    const float d = ((float)(j - W)) / ((float)sigma);
    taps[(size_t)j] = (float)std::exp(-0.5 * (double)(d * d));
    acc += taps[(size_t)j];
  }
  for (float& t : taps) t /= acc;
  return taps;
}

inline std::vector<double> ExpnTable() {
  std::vector<double> t(kExpnSize + 1);
  for (int k = 0; k < kExpnSize + 1; ++k) t[(size_t)k] = std::exp(-(double)k * (kExpnMax / kExpnSize));
  return t;
}

inline Keypoint MakeKeypoint(const Refined& r, int o, const Geometry& g) {
  const double xper = std::ldexp(1.0, o);
  Keypoint k;
  k.o = o; k.ix = r.ix; k.iy = r.iy; k.is = r.is;
  k.s = (float)r.sn;
  k.x = (float)(r.xn * xper);
  k.y = (float)(r.yn * xper);
  k.sigma = (float)(g.sigma0 * std::pow(2.0, r.sn / g.S) * xper);
  return k;
}

// FeatureKeypoint(k.x + 0.5f, k.y + 0.5f, k.sigma, angle)
inline void FeatureRow(const Keypoint& k, double angle, float* row) {
  row[0] = k.x + 0.5f; row[1] = k.y + 0.5f; row[2] = k.sigma; row[3] = (float)angle;
}

// One container of the reference per run of equal `is` inside an octave
struct Level {
  int32_t octave, is;
  int64_t num_features;      // the keypoints of the level, with or without an orientation
  int64_t size;              // the features they gave
};

// The features of one octave's keypoints appended to the level list.  is: the level of every keypoint in the octave's order (non-decreasing);
// used: the orientations taken for it.
inline void AppendLevels(int octave, const int32_t* is, const int32_t* used, int64_t n, std::vector<Level>* levels) {
  int prev = -1;
  for (int64_t i = 0; i < n; ++i) {
    if (is[i] != prev) levels->push_back(Level{octave, is[i], 0, 0});
    levels->back().num_features += 1;
    levels->back().size += used[i];
    prev = is[i];
  }
}

struct Cut { int32_t first_level_to_keep; int64_t first_feature, num_features; };

// Levels are dropped from the finest one up until what is left holds no more than max_num_features keypoints - or rather: the level at which the
// running count from the coarsest level down first EXCEEDS max_num_features is the first one kept, and it is kept whole.
inline Cut SelectLevels(const std::vector<Level>& levels, int64_t max_num_features) {
  Cut c{0, 0, 0};
  int64_t num_features = 0;
  for (int i = (int)levels.size() - 1; i >= 0; --i) {
    num_features += levels[(size_t)i].num_features;
    c.num_features += levels[(size_t)i].size;
    if (num_features > max_num_features) { c.first_level_to_keep = i; break; }
  }
  for (int i = 0; i < c.first_level_to_keep; ++i) c.first_feature += levels[(size_t)i].size;
  return c;
}

// K24 - the same cut from the keypoint counts alone.  SelectLevels reads `size` only to count what it keeps; the level it selects depends on
// num_features, and those are known after refinement - before any orientation or descriptor.  The kept keypoints of an octave are a suffix of its
// list (the levels of an octave stand in the order of its keypoints), all of them in the octaves above the cut, none in those below.
struct KeptRange { int64_t first, count; };      // the keypoints [first, first + count) of one octave's list
struct KeptCut {
  int32_t first_level_to_keep;
  int64_t num_keypoints;               // kept, all octaves
  std::vector<KeptRange> octaves;      // by octave index q = octave - o_min
};

inline KeptCut SelectKeptKeypoints(const std::vector<Level>& levels, int64_t max_num_features, int o_min, int num_octaves) {
  KeptCut c{0, 0, std::vector<KeptRange>((size_t)num_octaves, KeptRange{0, 0})};
  int64_t num_features = 0;
  for (int i = (int)levels.size() - 1; i >= 0; --i) {
    num_features += levels[(size_t)i].num_features;
    if (num_features > max_num_features) { c.first_level_to_keep = i; break; }
  }
  for (size_t i = 0; i < levels.size(); ++i) {
    KeptRange& r = c.octaves[(size_t)(levels[i].octave - o_min)];
    if ((int)i < c.first_level_to_keep) { r.first += levels[i].num_features; continue; }
    r.count += levels[i].num_features;
    c.num_keypoints += levels[i].num_features;
  }
  return c;
}

// Where the kept features of a group of n images go in the matcher's store.  The descriptor launch lists them in blocks, octave by octave and image
// by image inside an octave: block q * n + i holds counts[q * n + i] features of image i in the reference's order.  Image i owns the rows from
// row0[i] on and takes its blocks in octave order, so its rows are in the reference's order.  -> the first row of every block.
inline std::vector<int64_t> KeptBlockRows(const std::vector<int64_t>& counts, size_t num_octaves, size_t n, const int64_t* row0) {
  std::vector<int64_t> rows(counts.size());
  for (size_t i = 0; i < n; ++i) {
    int64_t at = row0[i];
    for (size_t q = 0; q < num_octaves; ++q) { rows[q * n + i] = at; at += counts[q * n + i]; }
  }
  return rows;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The serial extraction

struct OctaveCounts { int32_t width, height, num_candidates, num_keypoints, moved, reject_peak, reject_edge, reject_offset, reject_bounds; };

struct HostResult {
  std::vector<float> keypoints;          // N x 4, every feature before the cut
  std::vector<int32_t> octave_level;     // N x 2: (o, is)
  std::vector<double> angles;            // N
  std::vector<float> raw;                // N x 128, VLFeat order, before the last normalisation
  std::vector<uint8_t> descriptors;      // N x 128, UBC order
  std::vector<Level> levels;
  std::vector<OctaveCounts> octaves;
  Cut cut{0, 0, 0};
  int64_t two_orientations = 0, windows_cut = 0, descriptors_skipped = 0;
  std::vector<DescriptorWindow> windows;      // N (with descriptors)
  std::vector<int32_t> window_pixels;         // N: the pixels of each descriptor's window
};

// Consecutive images in input order, taken greedily while the sum of their bytes stays within the target; an image that exceeds the target on its
// own runs alone.  -> the first image of every sub-batch, then the number of images: sub-batch b is [out[b], out[b + 1]).
inline std::vector<int32_t> PlanSiftBatches(const std::vector<int64_t>& bytes_per_image, int64_t target) {
  std::vector<int32_t> first;
  int64_t sum = 0;
  for (size_t i = 0; i < bytes_per_image.size(); ++i) {
    const int64_t b = bytes_per_image[i];
    if (first.empty() || b > target - sum) { first.push_back((int32_t)i); sum = 0; }      // (sum <= target, or the sub-batch is one oversized image)
    sum = b > target ? target : sum + b;
  }
  first.push_back((int32_t)bytes_per_image.size());
  return first;
}

constexpr int kWaveLanes = 64;

// Descriptor() + FinishDescriptor() by the scheme of k_sift_describe_wave, serially: chunks of 64 window pixels in scan order are staged (the array
// in place of LDS), then each of the 64 "lanes" folds the staged pixels, in order, into the two bins it owns; the norms run over the 128 entries.
inline DescriptorWindow DescriptorByWave(const float* grad, int w, int h, int s_min, int s_max, const Keypoint& k, double xper, double angle0, double st0,
                                         double ct0, const double* expn, int normalization, float* descr, uint8_t* bytes) {
  const DescriptorFrame f = MakeDescriptorFrame(w, h, s_min, s_max, k, xper);
  float hist[kDescBins];
  for (int i = 0; i < kDescBins; ++i) hist[i] = 0.f;
  const int n = DescriptorWindowPixels(f), nx = f.x1 - f.x0 + 1;
  DescriptorTap staged[kWaveLanes];
  for (int base = 0; base < n; base += kWaveLanes) {
    const int m = std::min(kWaveLanes, n - base);
    for (int lane = 0; lane < m; ++lane) {
      const int p = base + lane, dxi = f.x0 + p % nx, dyi = f.y0 + p / nx;
      const float* g = grad + 2 * (f.xi + dxi) + (int64_t)(2 * w) * (f.yi + dyi);
      staged[lane] = DescriptorSample(f, angle0, st0, ct0, expn, dxi, dyi, g[0], g[1]);
    }
    for (int lane = 0; lane < kWaveLanes; ++lane)
      for (int j = 0; j < m; ++j) DescriptorFold(staged[j], ((lane >> 2) & 3) - 2, (lane >> 4) - 2, 2 * (lane & 3), &hist[2 * lane], &hist[2 * lane + 1]);
  }
  float norm = HistogramNorm(hist);
  for (int i = 0; i < kDescBins; ++i) hist[i] = ClampBin(hist[i] / norm);
  norm = HistogramNorm(hist);
  for (int i = 0; i < kDescBins; ++i) descr[i] = hist[i] / norm;
  norm = FinishNorm(descr, normalization);
  for (int i = 0; i < kDescBins; ++i) bytes[UbcIndex(i)] = FinishByte(descr[i], norm, normalization);
  return f.win;
}

enum class DescriptorRoute { kLane, kWave };      // Descriptor() as it stands / the wavefront scheme

// name, element size, count, data
using StageSink = std::function<void(const std::string&, size_t, size_t, const void*)>;

// dst (h x w image as w rows of h ... the transposed layout of vl_imconvcol_vf): dst[x * h + y] = the column convolution of src (w x h) at (x, y)
inline void ConvolveColumnsTransposed(float* dst, const float* src, int w, int h, const std::vector<float>& taps) {
  const int n = (int)taps.size(), W = n / 2;
  std::vector<float> col((size_t)h + 2 * (size_t)W);
  for (int x = 0; x < w; ++x) {
    for (int i = 0; i < h + 2 * W; ++i) col[(size_t)i] = src[(int64_t)std::min(std::max(i - W, 0), h - 1) * w + x];
    for (int y = 0; y < h; ++y) dst[(int64_t)x * h + y] = ConvolveTaps(col.data() + y, 1, taps.data(), n);
  }
}
inline void Smooth(float* out, float* temp, const float* in, int w, int h, double sigma) {
  const std::vector<float> taps = GaussTaps(sigma);
  ConvolveColumnsTransposed(temp, in, w, h, taps);
  ConvolveColumnsTransposed(out, temp, h, w, taps);
}
// copy_and_upsample_rows: dst[X * h + y], X < 2 w
inline void UpsampleRowsTransposed(float* dst, const float* src, int w, int h) {
  for (int y = 0; y < h; ++y)
    for (int X = 0; X < 2 * w; ++X) dst[(int64_t)X * h + y] = UpsampleRowValue(src + (int64_t)y * w, w, X);
}

inline HostResult ExtractOnHost(const Options& opt, int width, int height, const uint8_t* grey, bool want_descriptors, const StageSink& sink,
                                DescriptorRoute route = DescriptorRoute::kLane) {
  HostResult R;
  const Geometry g = MakeGeometry(opt);
  const std::vector<double> expn = ExpnTable();
  const int w0 = ShiftLeft(width, -g.o_min), h0 = ShiftLeft(height, -g.o_min);
  const size_t nel = (size_t)w0 * h0;
  const int L = g.levels();
  std::vector<float> octave(nel * (size_t)L), dog(nel * (size_t)(L - 1)), grad(2 * nel * (size_t)std::max(L - 3, 1)), temp(nel), im((size_t)width * height);
  for (size_t i = 0; i < im.size(); ++i) im[i] = PixelFromByte(grey[i]);
  int w = w0, h = h0;
  for (int o = g.o_min; o < g.o_min + g.O; ++o) {
    const bool first = o == g.o_min;
    if (first) {
      if (g.o_min < 0) {
        UpsampleRowsTransposed(temp.data(), im.data(), width, height);
        UpsampleRowsTransposed(octave.data(), temp.data(), height, 2 * width);
        for (int q = -1; q > g.o_min; --q) {
          UpsampleRowsTransposed(temp.data(), octave.data(), width << -q, height << -q);
          UpsampleRowsTransposed(octave.data(), temp.data(), width << -q, 2 * (height << -q));      // (the reference's arguments, as they stand)
        }
      } else {
        const int d = 1 << g.o_min;
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) octave[(size_t)y * w + x] = im[(size_t)(y * d) * width + (size_t)x * d];
      }
    } else {
      const int s_best = std::min(g.s_min + g.S, g.s_max);
      const float* pt = octave.data() + (size_t)(s_best - g.s_min) * ((size_t)w * h);
      const int nw = w >> 1, nh = h >> 1;
      for (int y = 0; y < nh; ++y)
        for (int x = 0; x < nw; ++x) temp[(size_t)y * nw + x] = pt[(size_t)(2 * y) * w + 2 * x];
      w = nw; h = nh;
      std::copy(temp.begin(), temp.begin() + (size_t)w * h, octave.begin());
    }
    const size_t lev = (size_t)w * h;
    const double sd0 = FirstLevelSigma(g, first);
    if (sd0 > 0.0) Smooth(octave.data(), temp.data(), octave.data(), w, h, sd0);
    for (int s = g.s_min + 1; s <= g.s_max; ++s)
      Smooth(octave.data() + (size_t)(s - g.s_min) * lev, temp.data(), octave.data() + (size_t)(s - 1 - g.s_min) * lev, w, h, LevelSigma(g, s));
    for (int s = 0; s < L - 1; ++s)
      for (size_t i = 0; i < lev; ++i) dog[(size_t)s * lev + i] = octave[(size_t)(s + 1) * lev + i] - octave[(size_t)s * lev + i];
    const bool has_grad = w >= 2 && h >= 2;
    if (has_grad)
      for (int s = g.s_min + 1; s <= g.s_max - 2; ++s)
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            float* gp = grad.data() + 2 * ((size_t)(s - g.s_min - 1) * lev + (size_t)y * w + x);
            GradientAt(octave.data() + (size_t)(s - g.s_min) * lev, w, h, x, y, gp, gp + 1);
          }
    const std::string tag = " " + std::to_string(o);
    if (sink) {
      const int32_t dims[2] = {w, h};
      sink("dims" + tag, 4, 2, dims);
      for (int s = 0; s < L; ++s) sink("gauss" + tag + " " + std::to_string(s + g.s_min), 4, lev, octave.data() + (size_t)s * lev);
      for (int s = 0; s < L - 1; ++s) sink("dog" + tag + " " + std::to_string(s + g.s_min), 4, lev, dog.data() + (size_t)s * lev);
      if (has_grad)
        for (int s = g.s_min + 1; s <= g.s_max - 2; ++s) sink("grad" + tag + " " + std::to_string(s), 4, 2 * lev, grad.data() + 2 * (size_t)(s - g.s_min - 1) * lev);
    }
    // detection in scan order, then refinement
    std::vector<int32_t> cand;
    for (int s = g.s_min + 1; s <= g.s_max - 2; ++s)
      for (int y = 1; y < h - 1; ++y)
        for (int x = 1; x < w - 1; ++x)
          if (IsExtremum(dog.data() + (size_t)(s - g.s_min) * lev + (size_t)y * w + x, w, (int)lev, 0.8 * opt.peak_threshold)) {
            cand.push_back(x); cand.push_back(y); cand.push_back(s);
          }
    OctaveCounts oc{w, h, (int32_t)(cand.size() / 3), 0, 0, 0, 0, 0, 0};
    std::vector<Keypoint> keys;
    for (size_t c = 0; c < cand.size(); c += 3) {
      const Refined r = RefineCandidate(dog.data(), w, h, g.s_min, g.s_max, cand[c], cand[c + 1], cand[c + 2], opt.peak_threshold, opt.edge_threshold);
      oc.moved += r.moves > 0;
      oc.reject_peak += r.reject == 1; oc.reject_edge += r.reject == 2; oc.reject_offset += r.reject == 3; oc.reject_bounds += r.reject == 4;
      if (r.good) keys.push_back(MakeKeypoint(r, o, g));
    }
    oc.num_keypoints = (int32_t)keys.size();
    R.octaves.push_back(oc);
    if (sink) sink("cand" + tag, 4, cand.size(), cand.data());
    // orientations and descriptors, keypoint by keypoint
    const double xper = std::ldexp(1.0, o);
    std::vector<int32_t> is(keys.size()), used(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
      const Keypoint& k = keys[i];
      double angles[kMaxAngles] = {0, 0, 0, 0};
      int n = 1;
      const float* level = grad.data() + 2 * (size_t)(k.is - g.s_min - 1) * lev;
      if (!opt.upright) n = Orientations(level, w, h, g.s_min, g.s_max, k, xper, expn.data(), angles);
      is[i] = k.is;
      used[i] = std::min(n, (int)opt.max_num_orientations);
      R.two_orientations += used[i] >= 2;
      for (int a = 0; a < used[i]; ++a) {
        float row[4];
        FeatureRow(k, angles[a], row);
        R.keypoints.insert(R.keypoints.end(), row, row + 4);
        R.octave_level.push_back(o); R.octave_level.push_back(k.is);
        R.angles.push_back(angles[a]);
        if (!want_descriptors) continue;
        float d[kDescBins];
        uint8_t u[kDescBins];
        DescriptorWindow win;
        if (route == DescriptorRoute::kWave) {
          win = DescriptorByWave(level, w, h, g.s_min, g.s_max, k, xper, angles[a], std::sin(angles[a]), std::cos(angles[a]), expn.data(), opt.normalization, d, u);
        } else {
          win = Descriptor(level, w, h, g.s_min, g.s_max, k, xper, angles[a], std::sin(angles[a]), std::cos(angles[a]), expn.data(), d);
          FinishDescriptor(d, opt.normalization, u);
        }
        R.windows_cut += win.cut; R.descriptors_skipped += !win.computed;
        R.windows.push_back(win);
        R.window_pixels.push_back(DescriptorWindowPixels(MakeDescriptorFrame(w, h, g.s_min, g.s_max, k, xper)));
        R.raw.insert(R.raw.end(), d, d + kDescBins);
        R.descriptors.insert(R.descriptors.end(), u, u + kDescBins);
      }
    }
    AppendLevels(o, is.data(), used.data(), (int64_t)keys.size(), &R.levels);
  }
  R.cut = SelectLevels(R.levels, opt.max_num_features);
  return R;
}

}  // namespace sift
}  // namespace ppsfm
