// The pixel-space line error every reprojection gate of the mapper uses - CalculateSquaredLineReprojectionError
// (reference src/base/projection.cc:162-203) - as ONE device function: the observation filter (ba_filter.hip, K7a) and the track
// completion / merging kernels (tracks.hip, K10) call it, so the three decide on the same arithmetic.
#pragma once
#include <cfloat>

#include "camera_models.hpp"
#include "common.hpp"

namespace ppsfm {

__device__ __forceinline__ void QuatToRotNormalized(const double* q_in, double R[9]) {   // QuaternionToRotationMatrix(NormalizeQuaternion(q))
  const double n = sqrt(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
  const double w = q_in[0] / n, x = q_in[1] / n, y = q_in[2] / n, z = q_in[3] / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// (px, py, pz) = [R | t] (X; 1); line (a, b, c) with a^2 + b^2 = 1; DBL_MAX behind the camera or outside the image (size = width, height)
__device__ __forceinline__ double SquaredPixelLineError(double px, double py, double pz, double a, double b, double c, int model, const double* cam,
                                                        const int32_t* size) {
  if (pz < DBL_EPSILON) return DBL_MAX;
  const double inv = 1.0 / pz;
  const double u = inv * px, v = inv * py;
  const double alpha = a * u + b * v + c;
  const double lu = u - a * alpha, lv = v - b * alpha;
  double ix, iy;
  WorldToImage<double, double>(model, cam, u, v, &ix, &iy);
  if (!(ix >= 0 && ix < (double)size[0] && iy >= 0 && iy < (double)size[1])) return DBL_MAX;
  double jx, jy;
  WorldToImage<double, double>(model, cam, lu, lv, &jx, &jy);
  return (ix - jx) * (ix - jx) + (iy - jy) * (iy - jy);
}

// CalculateTriangulationAngle (reference src/base/triangulation.cc:59-82) at the projection centres c1, c2: the point filters of ba_filter.hip (K7b) and
// tracks_filter.hip (K14a) decide on the same arithmetic
__device__ __forceinline__ double TriangulationAngle(const double* c1, const double* c2, double X0, double X1, double X2) {
  const double b2 = (c1[0] - c2[0]) * (c1[0] - c2[0]) + (c1[1] - c2[1]) * (c1[1] - c2[1]) + (c1[2] - c2[2]) * (c1[2] - c2[2]);
  const double r1 = (X0 - c1[0]) * (X0 - c1[0]) + (X1 - c1[1]) * (X1 - c1[1]) + (X2 - c1[2]) * (X2 - c1[2]);
  const double r2 = (X0 - c2[0]) * (X0 - c2[0]) + (X1 - c2[1]) * (X1 - c2[1]) + (X2 - c2[2]) * (X2 - c2[2]);
  const double den = 2.0 * sqrt(r1 * r2);
  if (den == 0.0) return 0.0;
  const double ang = fabs(acos((r1 + r2 - b2) / den));
  return fmin(ang, 3.14159265358979323846 - ang);
}

}  // namespace ppsfm
