// The sequential half of K13 (register_image.hip): IncrementalMapper::FindNextImages (reference src/sfm/incremental_mapper.cc:139-190) after the
// per-image counts, and RegisterNextImage (:570-760) around the device work - its gates in the reference's order, what EstimateAbsolutePoseFromLines
// (src/estimators/pose.cc:52-94) does with the RANSAC report, and the commit rule of :746-757 on a TrackState.
// PINNED where the reference leaves it open: std::sort over the order of an unordered_map leaves the order of equal ranks to the hash table.
// Here: descending rank, ties by ASCENDING IMAGE INDEX (the pin of local_bundle_replay.hpp).
// std only: compiles with plain g++ (tests/register_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "tracks_replay.hpp"

namespace ppsfm {

enum RegisterFailure { kRegOk = 0, kRegFewVisible = 1, kRegFewCorrs = 2, kRegNoInliers = 3, kRegAligned = 4, kRegNaN = 5, kRegFewInliers = 6 };

// RankNextImageMaxVisiblePointsNum / RankNextImageMaxVisiblePointsRatio (:66-73): a float, as the reference's
inline float NextImageRank(int32_t method, int32_t visible, int32_t observed) {
  if (method == 0) return static_cast<float>(visible);
  return static_cast<float>(visible) / static_cast<float>(observed);
}

struct NextImagesResult {
  std::vector<int32_t> ranked;      // first bucket, then second bucket
  int32_t num_first_bucket = 0, num_unregistered = 0;
};

// SortAndAppendNextImages (:50-64)
inline void SortAndAppendNextImages(std::vector<std::pair<int32_t, float>>& ranks, std::vector<int32_t>* out) {
  std::sort(ranks.begin(), ranks.end(), [](const std::pair<int32_t, float>& a, const std::pair<int32_t, float>& b) {
    return a.second > b.second || (a.second == b.second && a.first < b.first);
  });
  for (const auto& r : ranks) out->push_back(r.first);
}

// visible / observed / registered: per image.  num_reg_trials (nullptr = all 0) and filtered (nullptr = none): the caller's num_reg_trials_ /
// filtered_images_.  An image with observed == 0 has visible == 0 and never passes `visible >= abs_pose_min_num_inliers > 0`.
inline NextImagesResult ReplayFindNextImages(int32_t num_images, const int32_t* visible, const int32_t* observed, const uint8_t* registered,
                                             const int32_t* num_reg_trials, const uint8_t* filtered, int32_t abs_pose_min_num_inliers,
                                             int32_t max_reg_trials, int32_t method) {
  NextImagesResult r;
  std::vector<std::pair<int32_t, float>> image_ranks, other_image_ranks;
  for (int32_t c = 0; c < num_images; ++c) {
    if (registered[c]) continue;                                                                             // :159
    ++r.num_unregistered;
    if ((size_t)visible[c] < static_cast<size_t>(abs_pose_min_num_inliers)) continue;                        // :164
    const size_t trials = num_reg_trials ? (size_t)num_reg_trials[c] : 0;
    if (trials >= static_cast<size_t>(max_reg_trials)) continue;                                             // :171
    const float rank = NextImageRank(method, visible[c], observed[c]);
    if (!(filtered && filtered[c]) && trials == 0) image_ranks.emplace_back(c, rank);                        // :178
    else other_image_ranks.emplace_back(c, rank);
  }
  SortAndAppendNextImages(image_ranks, &r.ranked);
  r.num_first_bucket = (int32_t)r.ranked.size();
  SortAndAppendNextImages(other_image_ranks, &r.ranked);
  return r;
}

// :585
inline bool RegisterVisibleGate(int64_t num_visible, int32_t abs_pose_min_num_inliers) {
  return !((size_t)num_visible < static_cast<size_t>(abs_pose_min_num_inliers));
}
// :653-657
inline bool RegisterCorrsGate(int64_t num_corrs, int32_t abs_pose_min_num_inliers) {
  return !((size_t)num_corrs < static_cast<size_t>(abs_pose_min_num_inliers) || (size_t)num_corrs < 6);
}

// RotationMatrixToQuaternion (base/pose.cc:41-51): Eigen::Quaterniond(rot_mat) as (w, x, y, z), no sign normalisation.  R: the left 3x3 of a 3x4 row-major model.
inline void ModelToPose7(const double* model, double* pose7) {
  auto R = [&](int r, int c) { return model[4 * r + c]; };
  double t = (R(0, 0) + R(1, 1)) + R(2, 2);
  double q[4] = {0, 0, 0, 0};
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R(2, 1) - R(1, 2)) * t;
    q[2] = (R(0, 2) - R(2, 0)) * t;
    q[3] = (R(1, 0) - R(0, 1)) * t;
  } else {
    int i = 0;
    if (R(1, 1) > R(0, 0)) i = 1;
    if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    t = std::sqrt(((R(i, i) - R(j, j)) - R(k, k)) + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R(k, j) - R(j, k)) * t;
    q[1 + j] = (R(j, i) + R(i, j)) * t;
    q[1 + k] = (R(k, i) + R(i, k)) * t;
  }
  for (int i = 0; i < 4; ++i) pose7[i] = q[i];
  for (int i = 0; i < 3; ++i) pose7[4 + i] = model[4 * i + 3];
}

struct PoseGateResult { int32_t failure = kRegOk; int32_t num_aligned_inliers = 0; };

// EstimateAbsolutePoseFromLines after the RANSAC (pose.cc:62-93) and the gate of :725.  inlier_mask: n bytes (all 0 when the RANSAC did not
// succeed), aligned: n bytes or nullptr.  pose7 is written once the RANSAC had an inlier.
inline PoseGateResult ReplayPoseGates(uint64_t num_inliers, const double* model, int64_t n, const uint8_t* inlier_mask, const uint8_t* aligned,
                                      int32_t abs_pose_min_num_inliers, double* pose7) {
  PoseGateResult g;
  if (num_inliers == 0) { g.failure = kRegNoInliers; return g; }                                             // pose.cc:65
  int num_aligned_inliers = 0;
  const int num_lines = static_cast<int>(n);
  for (int i = 0; i < num_lines; ++i)
    if (inlier_mask[i] && aligned && aligned[i]) num_aligned_inliers += 1;
  g.num_aligned_inliers = num_aligned_inliers;
  ModelToPose7(model, pose7);
  const size_t inl = (size_t)num_inliers;
  if (num_aligned_inliers > inl * 0.9) { g.failure = kRegAligned; return g; }                                // pose.cc:81 (int > size_t * double)
  for (int i = 0; i < 7; ++i) if (std::isnan(pose7[i])) { g.failure = kRegNaN; return g; }                   // pose.cc:89
  if (inl < static_cast<size_t>(abs_pose_min_num_inliers)) { g.failure = kRegFewInliers; return g; }         // :725
  return g;
}

// what pp_tracks_register_image checks before it touches anything -> 0, or 1 image, 2 a line, 3 a point, 4 the pose
inline int CheckRegisterCommit(const TrackState& st, int32_t num_images, int32_t image, const double* pose7, int64_t n, const int32_t* corr_line,
                               const int32_t* corr_point) {
  if (image < 0 || image >= num_images || st.image_registered[(size_t)image]) return 1;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t l = corr_line[i];
    if (l < 0 || l >= st.L || st.line_image[(size_t)l] != image) return 2;
    if (!st.Exists(corr_point[i])) return 3;
  }
  for (int i = 0; i < 7; ++i) if (!std::isfinite(pose7[i])) return 4;
  return 0;
}

// :743-757 on the state: RegisterImage, then per inlier whose line has no point yet AddObservation; emit(point, line) per observation
template <typename EmitFn>
inline int64_t ReplayRegisterCommit(TrackState& st, int32_t image, int64_t n, const int32_t* corr_line, const int32_t* corr_point,
                                    const uint8_t* inlier_mask, EmitFn&& emit) {
  st.image_registered[(size_t)image] = 1;
  int64_t added = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (inlier_mask && !inlier_mask[i]) continue;
    const int32_t l = corr_line[i], p = corr_point[i];
    if (st.line_point[(size_t)l] != -1) continue;      // !line.HasPoint3D() (:750): an earlier inlier of this line gave it its point
    st.line_point[(size_t)l] = p;
    st.tracks[(size_t)p].push_back(l);
    emit(p, l);
    ++added;
  }
  return added;
}

}  // namespace ppsfm
