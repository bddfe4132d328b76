// ppsfm.hpp — header-only C++ host mirror of the reference's extension points on top of the C ABI
// (include/ppsfm_hip.h).  No Eigen / Ceres / glog needed: matrices are plain std::array, errors are
// exceptions carrying pp_last_error().  Where Eigen exists the same layouts map 1:1
// (Matrix3x4d row-major copy, Vector3d data()).
//
//   ppsfm::P6LEstimator          <-> colmap::P6LEstimator   (reference src/estimators/absolute_pose.h:48-80)
//        the colmap Estimator concept used by RANSAC<E> (src/optim/ransac.h:146,191,204-205,223-228):
//        typedefs X_t/Y_t/M_t, kMinNumSamples, Estimate(X, Y), Residuals(X, Y, M, &residuals)
//   ppsfm::AbsolutePoseFromLinesRANSAC <-> RANSAC<P6LEstimator> (src/estimators/pose.cc:48), Estimate(X, Y) -> Report
//   ppsfm::EstimateAbsolutePoseFromLines  <-> src/estimators/pose.h:110-115
//   ppsfm::BundleAdjustmentProblem         <-> the flat form of what BundleAdjuster::SetUp builds
//        (src/optim/bundle_adjustment.cc:326-542); Solve() replaces ceres::Solve (:306)
//   ppsfm::Normalize, AdjustGlobalBundle, IterativeGlobalRefinement over ppsfm::FlatReconstruction <-> Reconstruction::Normalize
//        (src/base/reconstruction.cc:302-397), IncrementalMapper::AdjustGlobalBundle (src/sfm/incremental_mapper.cc:893-939) with the controller's
//        option preset (src/controllers/incremental_mapper.cc:52-70, 221-243), IterativeGlobalRefinement (:102-124)
//   ppsfm::init::initialize_reconstruction <-> src/init/initializer.h:103-108 (four-view initialisation: gravity
//        alignment, FourView2dEstimator LO-MSAC, lifting, PlanarOffsetEstimator LO-MSAC; both runs on the device)
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../include/ppsfm_hip.h"

namespace ppsfm {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void Check(int rc) {
  if (rc != PP_OK) throw Error(rc, pp_last_error());
}

using Vector3d = std::array<double, 3>;
using Vector4d = std::array<double, 4>;
using Matrix3x4d = std::array<double, 12>;  // row-major

// feature/types.h:98-138
struct FeatureLine {
  Vector3d line{{0, 0, 0}};
  bool is_aligned = false;
  uint64_t point3D_id = std::numeric_limits<uint64_t>::max();
  const Vector3d& Line() const { return line; }
  bool IsAligned() const { return is_aligned; }
};
using FeatureLines = std::vector<FeatureLine>;

// optim/ransac.h:47-76
struct RANSACOptions {
  double max_error = 0.0;
  double min_inlier_ratio = 0.1;
  double confidence = 0.99;
  double dyn_num_trials_multiplier = 3.0;
  size_t min_num_trials = 0;
  size_t max_num_trials = std::numeric_limits<size_t>::max();
  void Check() const {
    if (!(max_error > 0) || min_inlier_ratio < 0 || min_inlier_ratio > 1 || confidence < 0 || confidence > 1 ||
        min_num_trials > max_num_trials)
      throw Error(PP_ERR_INVALID, "RANSACOptions::Check failed");
  }
};

namespace detail {
class PoseHandle {
 public:
  PoseHandle(const FeatureLines& X, const std::vector<Vector3d>& Y, int device) {
    if (X.size() != Y.size()) throw Error(PP_ERR_INVALID, "CHECK_EQ(X.size(), Y.size())");
    std::vector<double> l(3 * X.size()), p(3 * X.size());
    std::vector<uint8_t> a(X.size());
    for (size_t i = 0; i < X.size(); ++i) {
      for (int c = 0; c < 3; ++c) { l[3 * i + c] = X[i].line[c]; p[3 * i + c] = Y[i][c]; }
      a[i] = X[i].is_aligned ? 1 : 0;
    }
    Check(pp_pose_create(static_cast<int32_t>(X.size()), l.data(), p.data(), a.data(), device, &h_));
  }
  ~PoseHandle() { pp_pose_destroy(h_); }
  PoseHandle(const PoseHandle&) = delete;
  PoseHandle& operator=(const PoseHandle&) = delete;
  pp_pose_handle get() const { return h_; }

 private:
  pp_pose_handle h_ = nullptr;
};
}  // namespace detail

class P6LEstimator {
 public:
  typedef FeatureLine X_t;
  typedef Vector3d Y_t;
  typedef Matrix3x4d M_t;
  static const int kMinNumSamples = 6;
  int device = 0;

  std::vector<M_t> Estimate(const std::vector<X_t>& lines2D, const std::vector<Y_t>& points3D) const {
    if (lines2D.size() != 6 || points3D.size() != 6) throw Error(PP_ERR_INVALID, "P6LEstimator::Estimate needs 6 pairs");
    detail::PoseHandle h(lines2D, points3D, device);
    const uint32_t sample[6] = {0, 1, 2, 3, 4, 5};
    double models[96];
    int32_t n = 0;
    Check(pp_pose_p6l_batch(h.get(), 1, sample, models, &n));
    std::vector<M_t> out(n);
    for (int k = 0; k < n; ++k)
      for (int e = 0; e < 12; ++e) out[k][e] = models[12 * k + e];
    return out;
  }
  void Residuals(const std::vector<X_t>& lines2D, const std::vector<Y_t>& points3D, const M_t& proj_matrix,
                 std::vector<double>* residuals) const {
    detail::PoseHandle h(lines2D, points3D, device);
    residuals->resize(lines2D.size());
    Check(pp_pose_residuals(h.get(), 1, proj_matrix.data(), residuals->data()));
  }
};

// RANSAC<P6LEstimator, InlierSupportMeasurer, RandomSampler>
class AbsolutePoseFromLinesRANSAC {
 public:
  struct Support {
    size_t num_inliers = 0;
    double residual_sum = std::numeric_limits<double>::max();
  };
  struct Report {
    bool success = false;
    size_t num_trials = 0;
    Support support;
    std::vector<char> inlier_mask;
    Matrix3x4d model{};
  };
  explicit AbsolutePoseFromLinesRANSAC(const RANSACOptions& options, unsigned seed = 0, int device = 0)
      : options_(options), seed_(seed), device_(device) {
    options.Check();
  }
  Report Estimate(const FeatureLines& X, const std::vector<Vector3d>& Y) const {
    detail::PoseHandle h(X, Y, device_);
    pp_ransac_options o;
    pp_ransac_options_default(&o);
    o.max_error = options_.max_error; o.min_inlier_ratio = options_.min_inlier_ratio; o.confidence = options_.confidence;
    o.dyn_num_trials_multiplier = options_.dyn_num_trials_multiplier;
    o.min_num_trials = options_.min_num_trials; o.max_num_trials = options_.max_num_trials; o.seed = seed_;
    pp_ransac_report r;
    std::vector<uint8_t> mask(X.size() ? X.size() : 1);
    Check(pp_pose_ransac(h.get(), &o, &r, mask.data()));
    Report rep;
    rep.success = r.success != 0; rep.num_trials = r.num_trials;
    rep.support.num_inliers = r.num_inliers; rep.support.residual_sum = r.residual_sum;
    for (int e = 0; e < 12; ++e) rep.model[e] = r.model[e];
    if (rep.success) rep.inlier_mask.assign(mask.begin(), mask.begin() + X.size());
    return rep;
  }
  P6LEstimator estimator;

 private:
  RANSACOptions options_;
  unsigned seed_;
  int device_;
};

// base/pose.cc:41-51 (Eigen::Quaterniond(rot_mat) -> (w,x,y,z))
inline Vector4d RotationMatrixToQuaternion(const Matrix3x4d& P) {
  auto R = [&](int r, int c) { return P[4 * r + c]; };
  Vector4d q{{0, 0, 0, 0}};
  double t = R(0, 0) + R(1, 1) + R(2, 2);
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[1] = (R(2, 1) - R(1, 2)) * t; q[2] = (R(0, 2) - R(2, 0)) * t; q[3] = (R(1, 0) - R(0, 1)) * t;
  } else {
    int i = 0;
    if (R(1, 1) > R(0, 0)) i = 1;
    if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
    q[1 + i] = 0.5 * t; t = 0.5 / t;
    q[0] = (R(k, j) - R(j, k)) * t; q[1 + j] = (R(j, i) + R(i, j)) * t; q[1 + k] = (R(k, i) + R(i, k)) * t;
  }
  return q;
}

// estimators/pose.h:110-115, pose.cc:52-94
inline bool EstimateAbsolutePoseFromLines(const RANSACOptions& options, const FeatureLines& lines2D,
                                          const std::vector<Vector3d>& points3D, Vector4d* qvec, Vector3d* tvec,
                                          size_t* num_inliers, std::vector<char>* inlier_mask, unsigned seed = 0, int device = 0) {
  options.Check();
  AbsolutePoseFromLinesRANSAC ransac(options, seed, device);
  const auto report = ransac.Estimate(lines2D, points3D);
  *num_inliers = report.support.num_inliers;
  *inlier_mask = report.inlier_mask;
  if (*num_inliers == 0) return false;
  size_t num_aligned_inliers = 0;
  for (size_t i = 0; i < lines2D.size() && i < inlier_mask->size(); ++i)
    if ((*inlier_mask)[i] && lines2D[i].IsAligned()) ++num_aligned_inliers;
  if (num_aligned_inliers > *num_inliers * 0.9) return false;
  *qvec = RotationMatrixToQuaternion(report.model);
  *tvec = Vector3d{{report.model[3], report.model[7], report.model[11]}};
  for (double v : *qvec) if (std::isnan(v)) return false;
  for (double v : *tvec) if (std::isnan(v)) return false;
  return true;
}

// Flat bundle-adjustment problem (what BundleAdjuster::SetUp produces) + the solve.
class BundleAdjustmentProblem {
 public:
  // (a descriptor that does not say otherwise gets PP_ORDERING_AUTO: the reference's BundleAdjuster::Solve hands the camera ordering to Ceres' SPARSE_SCHUR without
  // being asked, bundle_adjustment.cc:279-282; the handles of a point-sharded group pass PP_ORDERING_NATURAL or a union co-visibility)
  BundleAdjustmentProblem(const pp_ba_problem_desc& desc, int device = 0) : C_(desc.num_poses), P_(desc.num_points), K_(desc.num_cameras) {
    pp_ba_problem_desc d = desc;
    if (d.ordering == PP_ORDERING_DEFAULT) d.ordering = PP_ORDERING_AUTO;
    Check(pp_ba_create(&d, device, &h_));
  }
  ~BundleAdjustmentProblem() { pp_ba_destroy(h_); }
  BundleAdjustmentProblem(const BundleAdjustmentProblem&) = delete;
  BundleAdjustmentProblem& operator=(const BundleAdjustmentProblem&) = delete;
  void SetParameters(const double* poses, const double* points, const double* intr) { Check(pp_ba_set_parameters(h_, poses, points, intr)); }
  void GetParameters(double* poses, double* points, double* intr) { Check(pp_ba_get_parameters(h_, poses, points, intr)); }
  // returns false when the solver reports FAILURE (ceres::Solver::Summary::IsSolutionUsable() == false)
  bool Solve(const pp_ba_options& options, pp_ba_summary* summary) {
    const int rc = pp_ba_solve(h_, &options, summary);
    if (rc == PP_ERR_NUMERIC) return false;
    Check(rc);
    return true;
  }
  // pp_ba_covariance at the current parameters (the counterpart of ceres::Covariance with apply_loss_function = true, no sigma^2 factor): pose_pairs = (i, j)
  // in the descriptor's image order, pose_cov = one row-major 6 x 6 block Cov(delta_i, delta_j) per pair (tangent order: 3 rotation, 3 tvec); point_ids in the
  // descriptor's point order, point_cov = one 3 x 3 block per point.  Either output may be null when its request is empty.  Returns false when the undamped
  // reduced system is not positive definite (a free gauge, a point seen along one direction only); throws for an iterative or group-attached handle and
  // for an index out of range.
  bool Covariance(const pp_ba_options& options, const std::vector<std::pair<int32_t, int32_t>>& pose_pairs, std::vector<double>* pose_cov,
                  const std::vector<int32_t>& point_ids, std::vector<double>* point_cov, pp_ba_covariance_info* info = nullptr) {
    std::vector<int32_t> pi(pose_pairs.size()), pj(pose_pairs.size());
    for (size_t q = 0; q < pose_pairs.size(); ++q) { pi[q] = pose_pairs[q].first; pj[q] = pose_pairs[q].second; }
    if (pose_cov) pose_cov->assign(36 * pose_pairs.size(), 0.0);
    if (point_cov) point_cov->assign(9 * point_ids.size(), 0.0);
    const int rc = pp_ba_covariance(h_, &options, static_cast<int32_t>(pi.size()), pi.data(), pj.data(), pose_cov ? pose_cov->data() : nullptr,
                                    static_cast<int32_t>(point_ids.size()), point_ids.data(), point_cov ? point_cov->data() : nullptr, info);
    if (rc == PP_ERR_NUMERIC) return false;
    Check(rc);
    return true;
  }
  // every diagonal pose block (i, i), in image order
  bool Covariance(const pp_ba_options& options, std::vector<double>* pose_cov, const std::vector<int32_t>& point_ids, std::vector<double>* point_cov,
                  pp_ba_covariance_info* info = nullptr) {
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int32_t i = 0; i < C_; ++i) pairs.emplace_back(i, i);
    return Covariance(options, pairs, pose_cov, point_ids, point_cov, info);
  }
  // pp_ba_covariance_blocks: the covariance block of every listed pair of parameter blocks (PP_COV_POSE 6 rows, PP_COV_INTRINSICS 12, PP_COV_POINT 3; indices
  // in the descriptor's order).  *out is sized here: block q row-major w(a_q) x w(b_q) at CovarianceBlockOffsets(blocks)[q].  Returns and throws as Covariance.
  static std::vector<int64_t> CovarianceBlockOffsets(const std::vector<pp_cov_block>& blocks) {
    const auto width = [](int32_t kind) { return kind == PP_COV_POSE ? 6 : kind == PP_COV_INTRINSICS ? 12 : 3; };
    std::vector<int64_t> offsets(blocks.size() + 1, 0);
    for (size_t q = 0; q < blocks.size(); ++q) offsets[q + 1] = offsets[q] + width(blocks[q].kind_a) * width(blocks[q].kind_b);
    return offsets;
  }
  bool CovarianceBlocks(const pp_ba_options& options, const std::vector<pp_cov_block>& blocks, std::vector<double>* out, pp_ba_covariance_info* info = nullptr) {
    out->assign(static_cast<size_t>(CovarianceBlockOffsets(blocks).back()), 0.0);
    const int rc = pp_ba_covariance_blocks(h_, &options, static_cast<int64_t>(blocks.size()), blocks.data(), out->data(), static_cast<int64_t>(out->size()), info);
    if (rc == PP_ERR_NUMERIC) return false;
    Check(rc);
    return true;
  }
  pp_ba_handle handle() const { return h_; }

 private:
  pp_ba_handle h_ = nullptr;
  int C_, P_, K_;
};


// ---- the mapper's global refinement (controllers/incremental_mapper.cc:52-70, 102-124; sfm/incremental_mapper.cc:893-939) -----------------------------
// A reconstruction in the flat form BundleAdjustmentProblem takes: every registered image (in registration order), every 3D point, and the
// observations grouped per point in track order.  Deleting an observation removes its entry; a deleted point keeps its slot with point_alive = 0.
struct FlatReconstruction {
  std::vector<double> poses;              // C x 7 (qvec w,x,y,z; tvec)
  std::vector<double> points;             // P x 3
  std::vector<uint8_t> point_alive;       // P
  std::vector<double> intr;               // K x PP_CAM_STRIDE-many doubles per camera (12)
  std::vector<int32_t> pose_camera;       // C
  std::vector<int32_t> camera_model;      // K
  std::vector<int32_t> cam_size;          // K x 2 (width, height)
  std::vector<double> lines;              // M x 3
  std::vector<int32_t> obs_pose, obs_point;   // M
  std::vector<uint8_t> obs_aligned;       // M
  std::vector<int64_t> obs_id;            // M: the caller's name of the observation (kept through deletions)
  int NumImages() const { return (int)(poses.size() / 7); }
  int NumPoints() const { return (int)(points.size() / 3); }
  int NumCameras() const { return (int)camera_model.size(); }
  size_t ComputeNumObservations() const { return obs_pose.size(); }
};

// Reconstruction::Normalize (base/reconstruction.cc:302-397): translation, then scale, of every image and point.  Host, O(C log C + P).
inline void Normalize(FlatReconstruction* rec, double extent = 10.0, double p0 = 0.1, double p1 = 0.9, bool use_images = true) {
  if (!(extent > 0) || p0 < 0 || p0 > 1 || p1 < 0 || p1 > 1 || p0 > p1) throw Error(PP_ERR_INVALID, "Normalize: CHECK on extent / p0 / p1");
  const int C = rec->NumImages(), P = rec->NumPoints();
  size_t alive = 0;
  for (int p = 0; p < P; ++p) alive += rec->point_alive[p] ? 1 : 0;
  if ((use_images && C < 2) || (!use_images && alive < 2)) return;
  auto rotate = [](const double* q, const double* v, double* out) {      // Eigen::Quaterniond(q) * v, q as stored
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
  };
  std::vector<double> centers(3 * (size_t)C);
  for (int c = 0; c < C; ++c) {            // ProjectionCenterFromPose (base/pose.cc:94-101): conjugate of the NORMALISED quaternion times -tvec
    const double* q = &rec->poses[7 * c];
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double qc[4] = {q[0] / n, -q[1] / n, -q[2] / n, -q[3] / n};
    const double mt[3] = {-q[4], -q[5], -q[6]};
    rotate(qc, mt, &centers[3 * c]);
  }
  std::vector<float> coords[3];            // cast to float before the sort (:333-352)
  if (use_images) {
    for (int c = 0; c < C; ++c) for (int a = 0; a < 3; ++a) coords[a].push_back(static_cast<float>(centers[3 * c + a]));
  } else {
    for (int p = 0; p < P; ++p) if (rec->point_alive[p]) for (int a = 0; a < 3; ++a) coords[a].push_back(static_cast<float>(rec->points[3 * p + a]));
  }
  for (int a = 0; a < 3; ++a) std::sort(coords[a].begin(), coords[a].end());
  const size_t n = coords[0].size();
  const size_t P0 = static_cast<size_t>((n > 3) ? p0 * (n - 1) : 0);
  const size_t P1 = static_cast<size_t>((n > 3) ? p1 * (n - 1) : n - 1);
  double mean[3] = {0, 0, 0}, ext2 = 0;
  for (int a = 0; a < 3; ++a) {
    for (size_t i = P0; i <= P1; ++i) mean[a] += coords[a][i];
    mean[a] /= (double)(P1 - P0 + 1);
    const double d = (double)coords[a][P1] - (double)coords[a][P0];
    ext2 += d * d;
  }
  const double old_extent = std::sqrt(ext2);
  const double scale = old_extent < std::numeric_limits<double>::epsilon() ? 1.0 : extent / old_extent;
  for (int c = 0; c < C; ++c) {
    double m[3];
    for (int a = 0; a < 3; ++a) m[a] = -((centers[3 * c + a] - mean[a]) * scale);
    rotate(&rec->poses[7 * c], m, &rec->poses[7 * c + 4]);
  }
  for (int p = 0; p < P; ++p)
    if (rec->point_alive[p]) for (int a = 0; a < 3; ++a) rec->points[3 * p + a] = (rec->points[3 * p + a] - mean[a]) * scale;
}

// controllers/incremental_mapper.cc:221-243 and, below ten registered images, :58-66
inline pp_ba_options GlobalBundleAdjustmentOptions(size_t num_reg_images, int ba_global_max_num_iterations = 50) {
  pp_ba_options o;
  pp_ba_options_default(&o);
  o.function_tolerance = 0.0; o.gradient_tolerance = 1.0; o.parameter_tolerance = 0.0;
  o.max_num_iterations = ba_global_max_num_iterations; o.max_linear_solver_iterations = 100;
  const size_t kMinNumRegImagesForFastBA = 10;
  if (num_reg_images < kMinNumRegImagesForFastBA) {
    o.function_tolerance /= 10; o.gradient_tolerance /= 10; o.parameter_tolerance /= 10;
    o.max_num_iterations *= 2; o.max_linear_solver_iterations = 200;
  }
  return o;
}

namespace detail {
// the flat problem over the live points that still have observations (a point index of the problem -> the reconstruction's)
struct RefinementProblem {
  std::vector<int32_t> point_of, obs_point;
  std::vector<double> points;
  std::vector<uint8_t> pose_const, tvec_mask, point_const;
  std::vector<uint16_t> cam_mask;
  pp_ba_problem_desc desc{};
  RefinementProblem(const FlatReconstruction& r, bool gauge) {
    const int C = r.NumImages(), P = r.NumPoints();
    std::vector<int32_t> index(P, -1);
    obs_point.resize(r.obs_point.size());
    for (size_t o = 0; o < r.obs_point.size(); ++o) {
      const int32_t p = r.obs_point[o];
      if (index[p] < 0) { index[p] = (int32_t)point_of.size(); point_of.push_back(p); for (int a = 0; a < 3; ++a) points.push_back(r.points[3 * p + a]); }
      obs_point[o] = index[p];
    }
    pose_const.assign(C, 0); tvec_mask.assign(C, 0); point_const.assign(point_of.size(), 0); cam_mask.assign(r.NumCameras(), 0xFFFF);
    if (gauge) { pose_const[0] = 1; tvec_mask[1] = 1; }      // sfm/incremental_mapper.cc:922-926: the 7 gauge DOFs
    desc.num_poses = C; desc.num_points = (int32_t)point_of.size(); desc.num_cameras = r.NumCameras();
    desc.loss_type = PP_LOSS_TRIVIAL; desc.loss_scale = 1.0; desc.num_obs = (int64_t)r.obs_pose.size();
    desc.lines = r.lines.data(); desc.obs_pose = r.obs_pose.data(); desc.obs_point = obs_point.data();
    desc.pose_camera = r.pose_camera.data(); desc.camera_model = r.camera_model.data();
    desc.pose_const = pose_const.data(); desc.tvec_const_mask = tvec_mask.data(); desc.point_const = point_const.data();
    desc.camera_const_mask = cam_mask.data();
    desc.linear_solver = C <= PP_MAX_NUM_IMAGES_DIRECT_SOLVER ? PP_LINEAR_SOLVER_DIRECT : PP_LINEAR_SOLVER_ITERATIVE_SCHUR;
  }
};
inline void EraseObservations(FlatReconstruction* r, const std::vector<uint8_t>& gone) {
  size_t w = 0;
  for (size_t o = 0; o < gone.size(); ++o) {
    if (gone[o]) continue;
    for (int a = 0; a < 3; ++a) r->lines[3 * w + a] = r->lines[3 * o + a];
    r->obs_pose[w] = r->obs_pose[o]; r->obs_point[w] = r->obs_point[o]; r->obs_aligned[w] = r->obs_aligned[o]; r->obs_id[w] = r->obs_id[o];
    ++w;
  }
  r->lines.resize(3 * w); r->obs_pose.resize(w); r->obs_point.resize(w); r->obs_aligned.resize(w); r->obs_id.resize(w);
}
}  // namespace detail

// Reconstruction::FilterObservationsWithNegativeDepth on the device; returns the number of deleted observations
inline size_t FilterObservationsWithNegativeDepth(FlatReconstruction* rec, int device = 0) {
  if (rec->obs_pose.empty()) return 0;
  detail::RefinementProblem rp(*rec, false);
  BundleAdjustmentProblem problem(rp.desc, device);
  problem.SetParameters(rec->poses.data(), rp.points.data(), rec->intr.data());
  std::vector<uint8_t> neg(rec->obs_pose.size());
  int64_t n = 0;
  Check(pp_ba_filter_negative_depth(problem.handle(), neg.data(), &n));
  detail::EraseObservations(rec, neg);
  return (size_t)n;
}

// Reconstruction::FilterAllPoints3D on the device; returns the reference's count.  deleted_obs_ids / deleted_points (may be null) receive what went.
inline size_t FilterAllPoints3D(FlatReconstruction* rec, double max_reproj_error, double min_tri_angle, int device = 0,
                                std::vector<int64_t>* deleted_obs_ids = nullptr, std::vector<int32_t>* deleted_points = nullptr) {
  if (rec->obs_pose.empty()) return 0;
  detail::RefinementProblem rp(*rec, false);
  BundleAdjustmentProblem problem(rp.desc, device);
  problem.SetParameters(rec->poses.data(), rp.points.data(), rec->intr.data());
  const pp_filter_options fo{max_reproj_error, min_tri_angle};
  pp_filter_report rep;
  std::vector<uint8_t> od(rec->obs_pose.size()), pd(rp.point_of.size());
  std::vector<double> pe(rp.point_of.size());
  Check(pp_ba_filter_points(problem.handle(), &fo, rec->obs_aligned.data(), rec->cam_size.data(), nullptr, od.data(), pd.data(), pe.data(), &rep));
  for (size_t k = 0; k < pd.size(); ++k)
    if (pd[k]) { rec->point_alive[rp.point_of[k]] = 0; if (deleted_points) deleted_points->push_back(rp.point_of[k]); }
  if (deleted_obs_ids) for (size_t o = 0; o < od.size(); ++o) if (od[o]) deleted_obs_ids->push_back(rec->obs_id[o]);
  detail::EraseObservations(rec, od);
  return (size_t)rep.num_filtered;
}

// IncrementalMapper::AdjustGlobalBundle (sfm/incremental_mapper.cc:893-939): negative-depth filter, every image with the first one constant and
// tvec[0] of the second one constant, solve, Normalize.  Returns the solve's success (false: nothing to solve).  fix_existing_images is not mirrored.
inline bool AdjustGlobalBundle(FlatReconstruction* rec, const pp_ba_options& ba_options, pp_ba_summary* summary = nullptr, int device = 0) {
  if (rec->NumImages() < 2) throw Error(PP_ERR_INVALID, "At least two images must be registered for global bundle-adjustment");
  FilterObservationsWithNegativeDepth(rec, device);
  if (rec->obs_pose.empty()) return false;
  detail::RefinementProblem rp(*rec, true);
  BundleAdjustmentProblem problem(rp.desc, device);
  problem.SetParameters(rec->poses.data(), rp.points.data(), rec->intr.data());
  pp_ba_summary local;
  pp_ba_summary* s = summary ? summary : &local;
  const bool usable = problem.Solve(ba_options, s) && s->termination != PP_TERM_USER_FAILURE;
  if (usable) {      // (after FAILURE Ceres restores the parameter blocks it was given: nothing is written back)
    std::vector<double> poses(rec->poses.size()), intr(rec->intr.size());
    problem.GetParameters(poses.data(), rp.points.data(), intr.data());
    for (int c = 1; c < rec->NumImages(); ++c) for (int e = 0; e < 7; ++e) rec->poses[7 * c + e] = poses[7 * c + e];
    for (size_t k = 0; k < rp.point_of.size(); ++k) for (int a = 0; a < 3; ++a) rec->points[3 * rp.point_of[k] + a] = rp.points[3 * k + a];
  }
  Normalize(rec);
  return true;
}

struct GlobalRefinementOptions {      // controllers/incremental_mapper.h:102-108, sfm/incremental_mapper.h:89-92
  int ba_global_max_num_iterations = 50;
  int ba_global_max_refinements = 5;
  double ba_global_max_refinement_change = 0.0005;
  double filter_max_reproj_error = 4.0;
  double filter_min_tri_angle = 1.5;
};
struct GlobalRefinementReport {
  int num_rounds = 0;
  std::vector<pp_ba_summary> summaries;
  std::vector<size_t> num_filtered;
  std::vector<double> changed;
  std::vector<std::vector<int64_t>> obs_deleted;      // per round: obs_id of what the round's filter removed
  std::vector<std::vector<int32_t>> point_deleted;
};

// IterativeGlobalRefinement (controllers/incremental_mapper.cc:102-124).  CompleteAndMergeTracks and FilterImages are the triangulator's and the image
// bookkeeping's work, which this mirror does not restate: they are left out, so `changed` counts filtered observations only.
inline GlobalRefinementReport IterativeGlobalRefinement(FlatReconstruction* rec, const GlobalRefinementOptions& options = GlobalRefinementOptions(), int device = 0) {
  GlobalRefinementReport report;
  for (int i = 0; i < options.ba_global_max_refinements; ++i) {
    const size_t num_observations = rec->ComputeNumObservations();
    pp_ba_summary summary{};
    AdjustGlobalBundle(rec, GlobalBundleAdjustmentOptions((size_t)rec->NumImages(), options.ba_global_max_num_iterations), &summary, device);
    std::vector<int64_t> od;
    std::vector<int32_t> pd;
    const size_t num_filtered = FilterAllPoints3D(rec, options.filter_max_reproj_error, options.filter_min_tri_angle, device, &od, &pd);
    const double changed = num_observations ? static_cast<double>(num_filtered) / num_observations : 0.0;
    ++report.num_rounds;
    report.summaries.push_back(summary); report.num_filtered.push_back(num_filtered); report.changed.push_back(changed);
    report.obs_deleted.push_back(od); report.point_deleted.push_back(pd);
    if (changed < options.ba_global_max_refinement_change) break;
  }
  return report;
}

// ---- four-view initialisation (src/init/initializer.cc:58-216) ------------------------------------------------------
namespace init {

using Pose = Matrix3x4d;
struct InitOptions {              // initializer.h:48-58
  double min_tri_angle = 0.1;     // "Minimum mean triangulation angle (in rad)"
  double min_num_inliers = 6;
  double max_error = 0.005;       // in normalised coordinates
};

namespace detail {
// Eigen::Quaterniond::FromTwoVectors(a, b).toRotationMatrix(), row-major 3x3
inline std::array<double, 9> FromTwoVectors(const Vector3d& a, const Vector3d& b) {
  auto norm = [](const Vector3d& v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  const double na = norm(a), nb = norm(b);
  const Vector3d v0{{a[0] / na, a[1] / na, a[2] / na}}, v1{{b[0] / nb, b[1] / nb, b[2] / nb}};
  const double c = v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2];
  double w, x, y, z;
  if (c < -1.0 + 1e-12) {         // antiparallel: half turn about an axis orthogonal to a
    Vector3d e{{1, 0, 0}};
    if (std::fabs(v0[0]) > 0.9) e = Vector3d{{0, 1, 0}};
    Vector3d ax{{v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0]}};
    const double n = norm(ax);
    w = 0; x = ax[0] / n; y = ax[1] / n; z = ax[2] / n;
  } else {
    const double s = std::sqrt((1.0 + c) * 2.0);
    w = 0.5 * s;
    x = (v0[1] * v1[2] - v0[2] * v1[1]) / s; y = (v0[2] * v1[0] - v0[0] * v1[2]) / s; z = (v0[0] * v1[1] - v0[1] * v1[0]) / s;
  }
  return {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
           2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
}
struct Handles {
  pp_fourview2d_handle fv = nullptr;
  pp_planar_handle pl = nullptr;
  ~Handles() { pp_fourview2d_destroy(fv); pp_planar_destroy(pl); }
};
}  // namespace detail

// lines[i], gravity[i]: the four views.  Returns false exactly where the reference does (too few inliers, mean
// triangulation angle — computed in degrees and compared with min_tri_angle as the reference does, :186-190 —, and the
// planar-offset stage's checks :209-215).
inline bool initialize_reconstruction(const std::vector<FeatureLines>& lines, const std::vector<Vector3d>& gravity, const InitOptions& options,
                                      std::vector<Pose>* output, double* inlier_ratio, int device = 0) {
  *inlier_ratio = 0;
  if (lines.size() != 4 || gravity.size() != 4) throw Error(PP_ERR_INVALID, "initialize_reconstruction: four views expected");
  std::vector<double> x[4], lr[4];
  std::array<double, 36> Rg;
  for (int i = 0; i < 4; ++i) {
    const std::array<double, 9> R = detail::FromTwoVectors(gravity[i], Vector3d{{0.0, 1.0, 0.0}});
    for (int e = 0; e < 9; ++e) Rg[9 * i + e] = R[e];
    for (const FeatureLine& f : lines[i]) {
      const Vector3d& l0 = f.Line();
      if (f.IsAligned()) {       // only the aligned lines are pre-rotated (:76-90)
        const Vector3d l{{R[0] * l0[0] + R[1] * l0[1] + R[2] * l0[2], R[3] * l0[0] + R[4] * l0[1] + R[5] * l0[2], R[6] * l0[0] + R[7] * l0[1] + R[8] * l0[2]}};
        if (std::fabs(l[1]) > 1e-6) throw Error(PP_ERR_INVALID, "initialize_reconstruction: CHECK_NEAR(l(1), 0.0, 1e-6)");
        double a = l[2], b = -l[0];
        if (b < 0) { a = -a; b = -b; }
        const double n = std::sqrt(a * a + b * b);
        x[i].push_back(a / n); x[i].push_back(b / n);
      } else {
        lr[i].insert(lr[i].end(), l0.begin(), l0.end());
      }
    }
  }
  for (int i = 1; i < 4; ++i)
    if (x[i].size() != x[0].size() || lr[i].size() != lr[0].size()) throw Error(PP_ERR_INVALID, "initialize_reconstruction: CHECK_EQ on the track counts");
  const int n2 = (int)(x[0].size() / 2), n3 = (int)(lr[0].size() / 3);
  if (n2 < 5 || n3 < 3) return false;
  std::vector<double> xs, ls;
  for (int i = 0; i < 4; ++i) { xs.insert(xs.end(), x[i].begin(), x[i].end()); ls.insert(ls.end(), lr[i].begin(), lr[i].end()); }

  pp_lomsac_options ro;
  pp_lomsac_options_default(&ro);
  ro.final_least_squares = 1; ro.min_num_iterations = 1000; ro.squared_inlier_threshold = options.max_error;
  detail::Handles hs;
  Check(pp_fourview2d_create(n2, xs.data(), device, &hs.fv));
  pp_lomsac_report rep;
  std::array<double, 24> c2;
  std::vector<double> X2((size_t)2 * n2);
  std::vector<int32_t> inl(n2);
  Check(pp_fourview2d_lomsac(hs.fv, &ro, nullptr, &rep, c2.data(), X2.data(), inl.data()));
  if (rep.best_num_inliers < options.min_num_inliers) return false;

  double angle_sum = 0;             // mean minimum triangulation angle over the first three cameras (:157-190)
  double ctr[3][2];
  for (int c = 0; c < 3; ++c) {
    const double* P = &c2[6 * c];
    ctr[c][0] = -(P[0] * P[2] + P[3] * P[5]); ctr[c][1] = -(P[1] * P[2] + P[4] * P[5]);
  }
  for (int k = 0; k < rep.num_inlier_indices; ++k) {
    const int i = inl[k];
    double best = std::numeric_limits<double>::max();
    for (int c1 = 0; c1 < 3; ++c1)
      for (int c2i = c1 + 1; c2i < 3; ++c2i) {
        const double v1[2] = {ctr[c1][0] - X2[2 * i], ctr[c1][1] - X2[2 * i + 1]}, v2[2] = {ctr[c2i][0] - X2[2 * i], ctr[c2i][1] - X2[2 * i + 1]};
        const double d = (v1[0] * v2[0] + v1[1] * v2[1]) / (std::sqrt(v1[0] * v1[0] + v1[1] * v1[1]) * std::sqrt(v2[0] * v2[0] + v2[1] * v2[1]));
        best = std::min(best, std::acos(std::max(-1.0, std::min(1.0, d))));
      }
    angle_sum += best;
  }
  const double mean_tri_angle = (angle_sum / rep.num_inlier_indices) / M_PI * 180.0;
  if (mean_tri_angle < options.min_tri_angle) return false;

  std::array<double, 48> poses{};   // lift_camera (:45-56)
  for (int c = 0; c < 4; ++c) {
    const double* P = &c2[6 * c];
    double* Q = &poses[12 * c];
    Q[0] = P[0]; Q[2] = P[1]; Q[8] = P[3]; Q[10] = P[4]; Q[5] = 1.0; Q[3] = P[2]; Q[11] = P[5];
  }
  Check(pp_planar_create(n3, poses.data(), ls.data(), Rg.data(), device, &hs.pl));
  pp_lomsac_report rep3;
  std::array<double, 3> ty;
  std::array<double, 48> cams3;
  std::vector<int32_t> inl3(n3);
  Check(pp_planar_lomsac(hs.pl, &ro, &rep3, ty.data(), cams3.data(), inl3.data()));
  if (rep3.best_num_inliers < options.min_tri_angle) return false;     // sic (:209-210)
  output->resize(4);
  for (int c = 0; c < 4; ++c) for (int e = 0; e < 12; ++e) (*output)[c][e] = cams3[12 * c + e];
  *inlier_ratio = rep3.inlier_ratio;
  return rep3.best_num_inliers >= options.min_num_inliers;
}

}  // namespace init

}  // namespace ppsfm
