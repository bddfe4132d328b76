// The host half of the line-feature generator (K19, line_features.hip): what LineFeatureWriterThread::Run (reference src/feature/extraction.cc:437-505)
// leaves to chance, pinned, and the checks on its input.
//   The reference seeds its PRNG from the clock, draws Eigen::Vector3d::Random() per random line and inserts RandomInteger(0, N - 1) into a set until
//   size / N >= aligned_line_ratio: its lines differ from run to run.  Here every draw is a function of (seed, image id, feature index, component):
//       mix(z)  = splitmix64's finaliser:  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31   (mod 2^64)
//       image   = mix(mix(seed + 0x9E3779B97F4A7C15) ^ uint32(image id))
//       h(i, c) = mix(image ^ (uint64(uint32(i)) << 2 | c)),   c = 0, 1, 2 the components of the random direction, c = 3 the alignment key
//       draw    = (int64(h >> 10) - 2^53) * 2^-53: a 54-bit integer moved to [-2^53, 2^53) and scaled by a power of two - integer operations and ONE
//                 conversion to double, which is exact; uniform on a grid of spacing 2^-53 in [-1, 1), Eigen's Random() being uniform in [-1, 1]
//       key     = (h(i, 3) & 0xFFFFFFFF00000000) | uint32(i): the hash in the high half, the index in the low half, so the keys of an image never tie
//   No draw depends on another image of the batch or on the position of its own.
//   The aligned set: the reference's loop ends at the smallest n with double(n) / double(N) >= ratio (N = 0: 0 / 0 is NaN, the loop never runs), and
//   its set is a uniform random n-subset; here it is the n features with the smallest key, i.e. key <= the image's n-th smallest key (the threshold
//   the device finds by a radix select).  A ratio outside [0, 1] (NaN included) would never end the reference's loop: refused.
// std only: compiles with plain g++ (tests/line_features_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PP_LF_HD __host__ __device__ inline
#else
#define PP_LF_HD inline
#endif

namespace ppsfm {

PP_LF_HD uint64_t LfMix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
PP_LF_HD uint64_t LfImageState(uint64_t seed, int32_t image_id) { return LfMix(LfMix(seed + 0x9E3779B97F4A7C15ull) ^ (uint64_t)(uint32_t)image_id); }
PP_LF_HD uint64_t LfHash(uint64_t image_state, int32_t index, int component) {
  return LfMix(image_state ^ (((uint64_t)(uint32_t)index << 2) | (uint64_t)component));
}
// component 0, 1, 2 of the random direction of feature `index`: in [-1, 1)
PP_LF_HD double LfDraw(uint64_t image_state, int32_t index, int component) {
  const int64_t k = (int64_t)(LfHash(image_state, index, component) >> 10) - (int64_t)(1ull << 53);
  return (double)k * 0x1p-53;
}
PP_LF_HD uint64_t LfAlignKey(uint64_t image_state, int32_t index) {
  return (LfHash(image_state, index, 3) & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)index;
}

inline bool LfRatioValid(double ratio) { return ratio >= 0.0 && ratio <= 1.0; }      // (false for NaN)

// the size the reference's set reaches (extraction.cc:454-458): the smallest n with double(n) / double(N) >= ratio.  LfRatioValid(ratio) is the caller's.
inline int64_t LfAlignedCount(int64_t N, double ratio) {
  if (N <= 0) return 0;
  const double Nd = (double)N;
  int64_t n = (int64_t)std::floor(ratio * Nd) - 1;      // an estimate; n / N is monotone in n, the two loops below make it exact
  n = std::min(std::max(n, (int64_t)0), N);
  while (n > 0 && (double)(n - 1) / Nd >= ratio) --n;
  while ((double)n / Nd < ratio) ++n;
  return n;
}

// the n-th smallest key of an image with N features (n in 1 .. N), as the device's select finds it
inline uint64_t LfThresholdKey(uint64_t image_state, int64_t N, int64_t n) {
  std::vector<uint64_t> keys((size_t)N);
  for (int64_t i = 0; i < N; ++i) keys[(size_t)i] = LfAlignKey(image_state, (int32_t)i);
  std::nth_element(keys.begin(), keys.begin() + (n - 1), keys.end());
  return keys[(size_t)(n - 1)];
}

// the batch as pp_line_features_desc describes it -> "" or what is wrong (PP_ERR_INVALID).  Pointers are checked by the caller.
inline std::string LfValidate(int32_t num_images, int32_t num_cameras, const int64_t* kp_start, const int32_t* image_camera, const int32_t* camera_model,
                              const int* camera_num_params, const double* intr, int intr_stride, const uint8_t* has_gravity, const double* gravity,
                              double aligned_line_ratio) {
  if (!LfRatioValid(aligned_line_ratio)) return "aligned_line_ratio is outside [0, 1]";
  if (num_images < 0 || num_cameras < 0) return "a negative count";
  if (kp_start[0] != 0) return "kp_start[0] != 0";
  for (int32_t k = 0; k < num_images; ++k) {
    if (kp_start[k + 1] < kp_start[k]) return "kp_start decreases at image " + std::to_string(k);
    if (kp_start[k + 1] - kp_start[k] > 0x7FFFFFFFll) return "image " + std::to_string(k) + " has 2^31 keypoints or more";
  }
  if (kp_start[num_images] >= 0x7FFFFFFFll - 4096) return "too many keypoints";
  for (int32_t c = 0; c < num_cameras; ++c) {
    if (camera_num_params[c] <= 0) return "camera " + std::to_string(c) + " has an unknown model " + std::to_string(camera_model[c]);
    for (int j = 0; j < camera_num_params[c]; ++j)
      if (!std::isfinite(intr[(size_t)c * (size_t)intr_stride + (size_t)j])) return "camera " + std::to_string(c) + " has a non-finite parameter";
  }
  for (int32_t k = 0; k < num_images; ++k) {
    if (image_camera[k] < 0 || image_camera[k] >= num_cameras) return "image " + std::to_string(k) + " names a camera out of range";
    if (has_gravity && has_gravity[k])
      for (int j = 0; j < 3; ++j)
        if (!std::isfinite(gravity[3 * (size_t)k + (size_t)j])) return "image " + std::to_string(k) + " has a non-finite gravity direction";
  }
  return "";
}

}  // namespace ppsfm
