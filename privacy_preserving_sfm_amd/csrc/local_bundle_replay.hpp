// The sequential half of pp_tracks_find_local_bundle (K12, local_bundle.hip): IncrementalMapper::FindLocalBundle
// (reference src/sfm/incremental_mapper.cc:993-1160) after its data-parallel part.  Given the shared-observation count of every image and a provider
// of the 75th-percentile triangulation angle of an image, it does the sort (:1020-1028), num_eff_images (:1033-1035), the early return (:1044-1049),
// the eight selection thresholds as the reference's double expressions (:1058-1071), the break on count < threshold (:1085-1088), the lazy angle
// (:1102-1119; every first use is recorded, which gives angles_used), the selection (:1122-1135) and the fill-up (:1141-1157).
// PINNED where the reference leaves it open:
//   - std::sort over an unordered_map leaves the order of equal counts to the hash table.  Here: descending count, ties by ASCENDING IMAGE INDEX
//     (the point order of K10 was pinned the same way).
//   - a NaN angle (acos of an argument one rounding above 1) sorts ABOVE every number in the percentile; std::nth_element on NaN is undefined in the
//     reference.  A NaN percentile then fails every `>=`, exactly as in the reference.
// std only: compiles with plain g++ (tests/local_bundle_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace ppsfm {

// index of Percentile(elems, 75) (util/math.h:232-246) among N >= 1 elements
inline int64_t LocalBundlePercentileIndex(int64_t N) {
  const int64_t idx = (int64_t)std::round(75.0 / 100 * (double)(N - 1));
  return std::max<int64_t>(0, std::min<int64_t>(N - 1, idx));
}

// the weakest overlap threshold of the eight (:1069-1070): the sequential loop never asks for the angle of an image whose count is below it
inline bool LocalBundleCanBeAsked(int32_t count, int32_t num_points3D) { return !((double)count < 0.1 * (double)num_points3D); }

// order of the percentile: numbers ascending by value, every NaN above them (non-negative doubles order as their bit patterns; a NaN's pattern
// with the sign cleared lies above infinity's)
inline uint64_t LocalBundleAngleKey(double a) {
  if (a != a) return 0x7FF8000000000000ull;
  a = std::fabs(a);
  uint64_t u;
  static_assert(sizeof(u) == sizeof(a), "binary64");
  std::memcpy(&u, &a, sizeof(u));
  return u;
}

struct LocalBundleResult {
  std::vector<int32_t> overlap_image, overlap_count;      // the sorted overlapping list
  std::vector<double> overlap_tri_angle;                  // radians, -1 where the loop never asked
  std::vector<int32_t> bundle;                            // in the reference's order
  int32_t num_eff_images = 0, angles_used = 0, threshold_level = -1, filled = 0;
};

// (:1020-1035) the overlapping images, sorted
inline void LocalBundleSort(const int32_t* count, int32_t num_images, LocalBundleResult* r) {
  std::vector<std::pair<int32_t, int32_t>> ov;      // (image, count)
  for (int32_t c = 0; c < num_images; ++c) if (count[c] > 0) ov.emplace_back(c, count[c]);
  std::sort(ov.begin(), ov.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
    return a.second != b.second ? a.second > b.second : a.first < b.first;
  });
  r->overlap_image.clear(); r->overlap_count.clear();
  for (const auto& e : ov) { r->overlap_image.push_back(e.first); r->overlap_count.push_back(e.second); }
  r->overlap_tri_angle.assign(ov.size(), -1.0);
}

// count: shared observations per image (0: not overlapping; the query image's own entry must be 0).  angle(image) -> the percentile angle in radians.
template <typename AngleFn>
inline LocalBundleResult ReplayFindLocalBundle(const int32_t* count, int32_t num_images, int32_t num_points3D, int32_t local_ba_num_images,
                                               double local_ba_min_tri_angle_deg, AngleFn&& angle) {
  LocalBundleResult r;
  LocalBundleSort(count, num_images, &r);
  const size_t num_overlapping = r.overlap_image.size();
  const size_t num_images_wanted = (size_t)(local_ba_num_images - 1);
  const size_t num_eff_images = std::min(num_images_wanted, num_overlapping);
  r.num_eff_images = (int32_t)num_eff_images;
  if (num_overlapping == num_eff_images) {      // :1044-1049
    r.bundle = r.overlap_image;
    return r;
  }
  const double min_tri_angle_rad = local_ba_min_tri_angle_deg * 0.0174532925199432954743716805978692718781530857086181640625;      // DegToRad
  const double n3 = (double)num_points3D;
  const std::pair<double, double> thresholds[8] = {
      {min_tri_angle_rad / 1.0, 0.6 * n3}, {min_tri_angle_rad / 1.5, 0.6 * n3}, {min_tri_angle_rad / 2.0, 0.5 * n3}, {min_tri_angle_rad / 2.5, 0.4 * n3},
      {min_tri_angle_rad / 3.0, 0.3 * n3}, {min_tri_angle_rad / 4.0, 0.2 * n3}, {min_tri_angle_rad / 5.0, 0.1 * n3}, {min_tri_angle_rad / 6.0, 0.1 * n3}};
  std::vector<char> used(num_overlapping, 0);
  for (int level = 0; level < 8; ++level) {
    r.threshold_level = level;
    for (size_t i = 0; i < num_overlapping; ++i) {
      if ((double)r.overlap_count[i] < thresholds[level].second) break;
      if (used[i]) continue;
      double& tri_angle = r.overlap_tri_angle[i];
      if (tri_angle < 0.0) {      // (an angle is >= 0 or NaN: either way it is asked for once)
        tri_angle = angle(r.overlap_image[i]);
        ++r.angles_used;
      }
      if (tri_angle >= thresholds[level].first) {
        r.bundle.push_back(r.overlap_image[i]);
        used[i] = 1;
        if (r.bundle.size() >= num_eff_images) break;
      }
    }
    if (r.bundle.size() >= num_eff_images) break;
  }
  if (r.bundle.size() < num_eff_images) {      // :1141-1157
    for (size_t i = 0; i < num_overlapping; ++i) {
      if (used[i]) continue;
      r.bundle.push_back(r.overlap_image[i]);
      used[i] = 1;
      ++r.filled;
      if (r.bundle.size() >= num_eff_images) break;
    }
  }
  return r;
}

}  // namespace ppsfm
