// The host half of pp_tracks_bundle_setup (K16, bundle_setup.hip): BundleAdjuster::SetUp (reference src/optim/bundle_adjustment.cc:326-542) around its
// data-parallel part.  Before the device: the validation and the de-duplication of the two point lists (a point listed a second time is skipped, :437-488
// visits variable_points then constant_points).  After it, given the pose list in order of first appearance: everything that is image- or camera-sized -
// pose_const and pose_tvec_mask (:396-421), the camera of each pose and the camera list in order of first appearance over the poses, and
// ParameterizeCameras (:490-528: a camera is constant when no refine flag is set, when the config says so, or when no config image with an observation
// uses it - AddPointToProblem adds the camera of an outside observer to the constant set, :470-476).
// CountBundleSetup is the exact size of the result, for a caller whose capacities are below the bound that always suffices.
// std only: compiles with plain g++ (tests/bundle_setup_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tracks_replay.hpp"

namespace ppsfm {

constexpr uint8_t kBundleImage = 1, kBundleConstPose = 2;      // PP_BUNDLE_IMAGE, PP_BUNDLE_CONST_POSE
constexpr uint8_t kBundleListed = 1, kBundleListedConst = 2;   // BundlePointList::mark

struct BundleConfigView {      // pp_bundle_config
  const uint8_t *image_flags, *tvec_const_mask, *camera_const;
  const uint16_t* camera_subset_mask;
  const int32_t *variable_points, *constant_points;
  int32_t num_variable_points, num_constant_points;
};

// -> "" when the config can be set up on this state, else what is wrong with it
inline std::string ValidateBundleConfig(const TrackState& st, int32_t num_images, const BundleConfigView& c) {
  char buf[160];
  if (!c.image_flags || c.num_variable_points < 0 || c.num_constant_points < 0 || (c.num_variable_points > 0 && !c.variable_points) ||
      (c.num_constant_points > 0 && !c.constant_points))
    return "bad config";
  for (int32_t i = 0; i < num_images; ++i)
    if ((c.image_flags[i] & kBundleImage) && !st.image_registered[(size_t)i]) {
      std::snprintf(buf, sizeof(buf), "image %d of the config is not registered", i);
      return buf;
    }
  const int32_t* lists[2] = {c.variable_points, c.constant_points};
  const int32_t counts[2] = {c.num_variable_points, c.num_constant_points};
  for (int k = 0; k < 2; ++k)
    for (int32_t i = 0; i < counts[k]; ++i) {
      const int32_t p = lists[k][i];
      if (p < 0 || p >= st.NumPoints()) {
        std::snprintf(buf, sizeof(buf), "%s point %d of %d", k ? "constant" : "variable", p, st.NumPoints());
        return buf;
      }
      if (!st.Exists(p)) {
        std::snprintf(buf, sizeof(buf), "%s point %d is deleted or has an empty track", k ? "constant" : "variable", p);
        return buf;
      }
    }
  return "";
}

struct BundlePointList {
  std::vector<int32_t> points;      // the listed points in the order visited, each once: its first occurrence
  std::vector<uint8_t> mark;        // per point of the state: kBundleListed, kBundleListedConst (in constant_points, wherever else it is listed)
};

inline BundlePointList DedupBundlePoints(int32_t num_points, const BundleConfigView& c) {
  BundlePointList r;
  r.mark.assign((size_t)num_points, 0);
  auto visit = [&](int32_t p) {
    if (r.mark[(size_t)p] & kBundleListed) return;
    r.mark[(size_t)p] |= kBundleListed;
    r.points.push_back(p);
  };
  for (int32_t i = 0; i < c.num_variable_points; ++i) visit(c.variable_points[i]);
  for (int32_t i = 0; i < c.num_constant_points; ++i) { r.mark[(size_t)c.constant_points[i]] |= kBundleListedConst; visit(c.constant_points[i]); }
  return r;
}

// the exact number of observations and points of the problem (what the device counts), on the host
inline void CountBundleSetup(const TrackState& st, const uint8_t* image_flags, const std::vector<int32_t>& listed, int64_t* num_obs, int32_t* num_points) {
  std::vector<int32_t> count((size_t)st.NumPoints(), 0);
  int64_t m = 0;
  int32_t n = 0;
  for (int64_t l = 0; l < st.L; ++l) {
    const int32_t p = st.line_point[(size_t)l];
    if (p < 0 || !(image_flags[st.line_image[(size_t)l]] & kBundleImage)) continue;
    ++m;
    n += count[(size_t)p]++ == 0;
  }
  for (const int32_t p : listed) {
    const std::vector<int32_t>& track = st.tracks[(size_t)p];
    if ((size_t)count[(size_t)p] == track.size()) continue;
    int64_t outside = 0;
    for (const int32_t l : track) outside += !(image_flags[st.line_image[(size_t)l]] & kBundleImage);
    m += outside;
    n += count[(size_t)p] == 0 && outside > 0;
  }
  *num_obs = m; *num_points = n;
}

struct BundlePoseResult {
  std::vector<uint8_t> pose_const, pose_tvec_mask;      // per pose
  std::vector<int32_t> pose_camera;                     // per pose: index into camera_index
  std::vector<int32_t> camera_index;                    // the cameras of the problem in order of first appearance over the poses
  std::vector<uint16_t> camera_const_mask;
};

// pose_image: the images of the problem's poses in order of first appearance in the stream; image_camera: the handle's pose_camera
inline BundlePoseResult ReplayBundlePoses(const int32_t* pose_image, int32_t num_poses, const int32_t* image_camera, int32_t num_cameras,
                                          const BundleConfigView& c) {
  BundlePoseResult r;
  std::vector<int32_t> rank((size_t)num_cameras, -1);
  std::vector<uint8_t> in_config((size_t)num_cameras, 0);      // a config image WITH an observation uses the camera
  for (int32_t k = 0; k < num_poses; ++k) {
    const int32_t image = pose_image[k], cam = image_camera[image];
    const uint8_t f = c.image_flags[image];
    const bool constant = !(f & kBundleImage) || (f & kBundleConstPose);
    r.pose_const.push_back(constant ? 1 : 0);
    r.pose_tvec_mask.push_back(!constant && c.tvec_const_mask ? c.tvec_const_mask[image] : 0);
    if (rank[(size_t)cam] < 0) { rank[(size_t)cam] = (int32_t)r.camera_index.size(); r.camera_index.push_back(cam); }
    r.pose_camera.push_back(rank[(size_t)cam]);
    if (f & kBundleImage) in_config[(size_t)cam] = 1;
  }
  for (const int32_t cam : r.camera_index) {
    const bool constant = !c.camera_subset_mask || (c.camera_const && c.camera_const[cam]) || !in_config[(size_t)cam];
    r.camera_const_mask.push_back(constant ? (uint16_t)0xFFFF : c.camera_subset_mask[cam]);
  }
  return r;
}

}  // namespace ppsfm
