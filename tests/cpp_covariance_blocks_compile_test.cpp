// Compile-and-link check of BundleAdjustmentProblem::CovarianceBlocks (ppsfm/ppsfm.hpp) against libppsfm_hip.so, host only: the entry point refuses a NULL
// handle without touching a device, an empty request is laid out as no doubles, and the offsets are the prefix sums of w(a) w(b).
#include <cstdio>

#include "../ppsfm/ppsfm.hpp"

int main() {
  pp_ba_options bo;
  pp_ba_options_default(&bo);
  pp_ba_covariance_info info;
  const pp_cov_block one = {PP_COV_POSE, 0, PP_COV_POINT, 0};
  double out[18];
  const int rc = pp_ba_covariance_blocks(nullptr, &bo, 1, &one, out, 18, &info);
  std::printf("null handle rc=%d (%s)\n", rc, pp_last_error());
  // the member function instantiates (never called without a device)
  bool (ppsfm::BundleAdjustmentProblem::*member)(const pp_ba_options&, const std::vector<pp_cov_block>&, std::vector<double>*, pp_ba_covariance_info*) =
      &ppsfm::BundleAdjustmentProblem::CovarianceBlocks;
  const std::vector<pp_cov_block> blocks = {{PP_COV_POSE, 1, PP_COV_POSE, 2},      {PP_COV_INTRINSICS, 0, PP_COV_INTRINSICS, 0}, {PP_COV_POINT, 3, PP_COV_INTRINSICS, 0},
                                            {PP_COV_POSE, 1, PP_COV_INTRINSICS, 0}, {PP_COV_POINT, 3, PP_COV_POINT, 4},           {PP_COV_POINT, 3, PP_COV_POSE, 0}};
  const std::vector<int64_t> offsets = ppsfm::BundleAdjustmentProblem::CovarianceBlockOffsets(blocks);
  std::printf("offsets");
  for (int64_t v : offsets) std::printf(" %lld", (long long)v);
  std::printf("\nok sizeof(block)=%d member=%d empty=%lld\n", (int)sizeof(pp_cov_block), member != nullptr,
              (long long)ppsfm::BundleAdjustmentProblem::CovarianceBlockOffsets({}).back());
  return rc == PP_ERR_INVALID ? 0 : 1;
}
