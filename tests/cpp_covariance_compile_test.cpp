// Compile-and-link check of BundleAdjustmentProblem::Covariance (ppsfm/ppsfm.hpp) against libppsfm_hip.so, and its driver on a device:
//   no argument    host only: the entry point refuses a NULL handle and a bad request without touching a device
//   <scene file>   the text scene tests/test_gpu_covariance_mirrors.py writes (counts, then every array of pp_ba_problem_desc and the parameters):
//                  prints the info of the call (I n path device_ms), then every diagonal pose block and the listed point blocks with 17 significant digits
#include <cstdio>
#include <fstream>

#include "../ppsfm/ppsfm.hpp"

template <typename T>
static std::vector<T> ReadArray(std::ifstream& in, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) { double x = 0; in >> x; v[i] = static_cast<T>(x); }
  return v;
}

int main(int argc, char** argv) {
  pp_ba_options bo;
  pp_ba_options_default(&bo);
  if (argc < 2) {
    pp_ba_covariance_info info;
    const int rc = pp_ba_covariance(nullptr, &bo, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &info);
    std::printf("null handle rc=%d (%s)\n", rc, pp_last_error());
    // the member functions instantiate (never called without a device)
    bool (ppsfm::BundleAdjustmentProblem::*all)(const pp_ba_options&, std::vector<double>*, const std::vector<int32_t>&, std::vector<double>*,
                                                     pp_ba_covariance_info*) =
        &ppsfm::BundleAdjustmentProblem::Covariance;
    std::printf("ok sizeof(info)=%d member=%d\n", (int)sizeof(info), all != nullptr);
    return rc == PP_ERR_INVALID ? 0 : 1;
  }
  std::ifstream in(argv[1]);
  if (!in) return 2;
  int C = 0, P = 0, K = 0, loss_type = 0, npts = 0;
  long long M = 0;
  double loss_scale = 1.0;
  in >> C >> P >> K >> M >> loss_type >> loss_scale >> npts;
  const std::vector<double> lines = ReadArray<double>(in, 3 * (size_t)M);
  const std::vector<int32_t> obs_pose = ReadArray<int32_t>(in, (size_t)M), obs_point = ReadArray<int32_t>(in, (size_t)M);
  const std::vector<int32_t> pose_camera = ReadArray<int32_t>(in, (size_t)C), camera_model = ReadArray<int32_t>(in, (size_t)K);
  const std::vector<uint8_t> pose_const = ReadArray<uint8_t>(in, (size_t)C), tvec_mask = ReadArray<uint8_t>(in, (size_t)C), point_const = ReadArray<uint8_t>(in, (size_t)P);
  const std::vector<uint16_t> cam_mask = ReadArray<uint16_t>(in, (size_t)K);
  const std::vector<double> poses = ReadArray<double>(in, 7 * (size_t)C), points = ReadArray<double>(in, 3 * (size_t)P), intr = ReadArray<double>(in, 12 * (size_t)K);
  const std::vector<int32_t> ids = ReadArray<int32_t>(in, (size_t)npts);
  if (!in) return 3;
  pp_ba_problem_desc d = pp_ba_problem_desc();
  d.num_poses = C; d.num_points = P; d.num_cameras = K; d.num_obs = M; d.loss_type = loss_type; d.loss_scale = loss_scale;
  d.lines = lines.data(); d.obs_pose = obs_pose.data(); d.obs_point = obs_point.data(); d.pose_camera = pose_camera.data(); d.camera_model = camera_model.data();
  d.pose_const = pose_const.data(); d.tvec_const_mask = tvec_mask.data(); d.point_const = point_const.data(); d.camera_const_mask = cam_mask.data();
  d.linear_solver = PP_LINEAR_SOLVER_DIRECT;
  try {
    ppsfm::BundleAdjustmentProblem problem(d, 0);
    problem.SetParameters(poses.data(), points.data(), intr.data());
    std::vector<double> pc, xc;
    pp_ba_covariance_info info;
    if (!problem.Covariance(bo, &pc, ids, &xc, &info)) { std::printf("not positive definite\n"); return 4; }
    std::printf("I %d %d %.17g\n", (int)info.n, (int)info.path, info.device_ms);
    for (size_t i = 0; i < pc.size(); ++i) std::printf("P %.17g\n", pc[i]);
    for (size_t i = 0; i < xc.size(); ++i) std::printf("X %.17g\n", xc[i]);
    try {
      problem.Covariance(bo, {{0, C}}, &pc, {}, nullptr);
      return 5;
    } catch (const ppsfm::Error& e) {
      std::printf("caught: %s\n", e.what());
    }
  } catch (const ppsfm::Error& e) {
    std::printf("error: %s\n", e.what());
    return 6;
  }
  return 0;
}
