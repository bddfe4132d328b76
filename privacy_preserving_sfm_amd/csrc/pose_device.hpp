// A pp_pose_handle over correspondences that a kernel writes (abs_pose.hip defines it, register_image.hip fills it).
#pragma once
#include "common.hpp"

namespace ppsfm {

struct PoseStreams { double *l0, *l1, *l2, *x0, *x1, *x2; uint8_t* aligned; };      // n entries each; aligned is nullptr without flags

int PoseCreateUnfilled(int32_t n, bool with_aligned, int device, pp_pose_handle* out, PoseStreams* streams);

}  // namespace ppsfm
