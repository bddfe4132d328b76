// Compile-and-link check of the global refinement part of the C++ host mirror (ppsfm/ppsfm.hpp): Normalize, GlobalBundleAdjustmentOptions,
// AdjustGlobalBundle and IterativeGlobalRefinement over FlatReconstruction.  Normalize runs on the host (its output is compared with the Python
// mirror by tests/test_cpp_global_refinement_host.py); the two device functions report a missing GPU as an exception.
#include <cstdio>

#include "../ppsfm/ppsfm.hpp"

int main() {
  ppsfm::FlatReconstruction rec;
  const int C = 5, P = 6;
  for (int c = 0; c < C; ++c) {
    const double a = 0.3 * c, h = std::sqrt(1.0 - 0.04 - 0.01);
    const double pose[7] = {h * std::cos(a), 0.2, h * std::sin(a), 0.1, 0.5 * c - 1.0, 0.25 * c * c, 4.0 - 0.7 * c};
    rec.poses.insert(rec.poses.end(), pose, pose + 7);
    rec.pose_camera.push_back(0);
  }
  for (int p = 0; p < P; ++p) { rec.points.push_back(0.1 * p); rec.points.push_back(-0.2 * p); rec.points.push_back(0.05 * p * p); rec.point_alive.push_back(1); }
  rec.camera_model.push_back(2);
  rec.cam_size = {1280, 960};
  rec.intr.assign(PP_CAM_STRIDE, 0.0);
  rec.intr[0] = 1000; rec.intr[1] = 640; rec.intr[2] = 480; rec.intr[3] = 0.01;
  for (int p = 0; p < P; ++p)
    for (int c = 0; c < 3; ++c) {
      rec.lines.push_back(1.0); rec.lines.push_back(0.0); rec.lines.push_back(0.01 * (p + c));
      rec.obs_pose.push_back(c); rec.obs_point.push_back(p); rec.obs_aligned.push_back(0); rec.obs_id.push_back(3 * p + c);
    }
  ppsfm::Normalize(&rec);
  std::printf("poses");
  for (double v : rec.poses) std::printf(" %.17g", v);
  std::printf("\npoints");
  for (double v : rec.points) std::printf(" %.17g", v);
  const pp_ba_options few = ppsfm::GlobalBundleAdjustmentOptions(9), many = ppsfm::GlobalBundleAdjustmentOptions(10);
  std::printf("\noptions %d %d %g %g %d %d\n", few.max_num_iterations, many.max_num_iterations, few.gradient_tolerance, many.gradient_tolerance,
              few.max_linear_solver_iterations, many.max_linear_solver_iterations);
  try {
    pp_ba_summary s;
    const bool ok = ppsfm::AdjustGlobalBundle(&rec, many, &s);
    std::printf("AdjustGlobalBundle returned %d\n", (int)ok);
  } catch (const ppsfm::Error& e) {
    std::printf("caught: %s\n", e.what());
  }
  try {
    const ppsfm::GlobalRefinementReport rep = ppsfm::IterativeGlobalRefinement(&rec);
    std::printf("IterativeGlobalRefinement ran %d rounds\n", rep.num_rounds);
  } catch (const ppsfm::Error& e) {
    std::printf("caught: %s\n", e.what());
  }
  return 0;
}
