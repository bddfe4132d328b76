// Device functions of the robust triangulation of one set of line observations - shared by K8 (triangulation.hip: one lane per track of the
// caller's arrays) and K11b (tracks_image.hip: one lane per create set of a pp_tracks_handle).
//   EstimateTriangulation, TriangulationEstimator::{Estimate, Residuals}      src/estimators/triangulation.cc:55-149
//   TriangulateMultiViewPoint (null vector of the K x 4 system [l_i^T P_i])    src/base/triangulation.cc:41-57
//   LORANSAC<..., InlierSupportMeasurer, CombinationSampler>::Estimate          src/optim/loransac.h:88-235
//   CombinationSampler: the 3-combinations in lexicographic order               src/optim/combination_sampler.cc:41-70
//   residuals: squared pixel line error / squared angular line error            src/base/projection.cc:161-203, 238-262
// The whole RANSAC (it draws no random numbers) runs in one lane: the null vector of a minimal sample is the vector of signed 3x3 minors, the
// local optimisation's is the smallest eigenvector of the 4x4 Gram matrix (cyclic Jacobi in registers).  The observations are reached through
// an accessor `obs` with view(i) -> index of the view and line(i) -> the three line coefficients; the current inlier flags live in `flags`.
#pragma once
#include <cfloat>

#include "camera_models.hpp"
#include "common.hpp"
#include "small_eigen.hpp"

namespace ppsfm {

struct TriModel {      // the views, the cameras and the estimator's options
  const int32_t *view_camera, *camera_model, *cam_size;
  const double *P, *centers, *intr;
  double min_tri_angle, max_residual, confidence, multiplier;
  int residual_type;
  unsigned long long max_num_trials;
};

__device__ __forceinline__ double TriProjZ(const double* P, const double* X) { return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]; }

// CalculateNormalizedLineAngularError of the ray (r0, r1, r2) = P X: false where the reference returns DBL_MAX (behind the camera, outside the image)
__device__ __forceinline__ bool LineAngularError(int model, const double* cam, double w, double h, const double* l, double r0, double r1, double r2, double* ang) {
  if (r2 < 0.0) return false;
  double ix, iy;
  WorldToImage<double, double>(model, cam, r0 / r2, r1 / r2, &ix, &iy);
  if (ix < 0 || ix >= w || iy < 0 || iy >= h) return false;
  const double nl = sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]), nr = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
  *ang = fabs(1.57079632679489661923 - acos(fabs((l[0] * r0 + l[1] * r1 + l[2] * r2) / (nl * nr))));
  return true;
}

__device__ __forceinline__ double TriResidual(const TriModel& a, int v, const double* l, const double* X) {
  const int k = a.view_camera[v];
  const double* P = a.P + 12 * (size_t)v;
  const double* cam = a.intr + (size_t)kCamStride * k;
  const int model = a.camera_model[k];
  const double w = (double)a.cam_size[2 * k], h = (double)a.cam_size[2 * k + 1];
  const double r0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3], r1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7], r2 = TriProjZ(P, X);
  if (a.residual_type == 1) {          // CalculateSquaredLineReprojectionError
    if (r2 < DBL_EPSILON) return DBL_MAX;
    const double inv = 1.0 / r2, u = inv * r0, vv = inv * r1;
    const double alpha = l[0] * u + l[1] * vv + l[2];
    double ix, iy, jx, jy;
    WorldToImage<double, double>(model, cam, u, vv, &ix, &iy);
    if (!(ix >= 0 && ix < w && iy >= 0 && iy < h)) return DBL_MAX;
    WorldToImage<double, double>(model, cam, u - l[0] * alpha, vv - l[1] * alpha, &jx, &jy);
    return (ix - jx) * (ix - jx) + (iy - jy) * (iy - jy);
  }
  // CalculateNormalizedLineAngularError, squared
  double ang;
  if (!LineAngularError(model, cam, w, h, l, r0, r1, r2, &ang)) return DBL_MAX;
  return ang * ang;
}

__device__ __forceinline__ double TriAngle(const double* c1, const double* c2, const double* X) {
  double b2 = 0, r1 = 0, r2 = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { b2 += (c1[i] - c2[i]) * (c1[i] - c2[i]); r1 += (X[i] - c1[i]) * (X[i] - c1[i]); r2 += (X[i] - c2[i]) * (X[i] - c2[i]); }
  const double den = 2.0 * sqrt(r1 * r2);
  if (den == 0.0) return 0.0;
  const double ang = fabs(acos((r1 + r2 - b2) / den));
  return fmin(ang, 3.14159265358979323846 - ang);
}

__device__ __forceinline__ void TriRow(const TriModel& a, int v, const double* l, double row[4]) {
  const double* P = a.P + 12 * (size_t)v;
#pragma unroll
  for (int c = 0; c < 4; ++c) row[c] = l[0] * P[c] + l[1] * P[4 + c] + l[2] * P[8 + c];
}
__device__ __forceinline__ double Det3(const double* a, const double* b, const double* c, int i0, int i1, int i2) {
  return a[i0] * (b[i1] * c[i2] - b[i2] * c[i1]) - a[i1] * (b[i0] * c[i2] - b[i2] * c[i0]) + a[i2] * (b[i0] * c[i1] - b[i1] * c[i0]);
}

// residual pass over the set: support of X; with `flags` the per-observation inlier flags are written
template <typename Obs>
__device__ __forceinline__ void TriSupport(const TriModel& a, const Obs& obs, int n, const double* X, unsigned long long* num_inliers, double* residual_sum, uint8_t* flags) {
  unsigned long long cnt = 0;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r = TriResidual(a, obs.view(i), obs.line(i), X);
    const bool in = r <= a.max_residual;
    if (in) { ++cnt; sum += r; }
    if (flags) flags[i] = in ? 1 : 0;
  }
  *num_inliers = cnt; *residual_sum = sum;
}

__device__ __forceinline__ unsigned long long TriNumTrials(unsigned long long num_inliers, unsigned long long num_samples, double confidence, double multiplier) {
  const double ratio = (double)num_inliers / (double)num_samples;      // RANSAC::ComputeNumTrials (optim/ransac.h:158-176)
  const double nom = 1.0 - confidence;
  if (nom <= 0) return 0xFFFFFFFFFFFFFFFFull;
  const double denom = 1.0 - pow(ratio, 3.0);
  if (denom <= 0) return 1;
  const double v = ceil(log(nom) / log(denom) * multiplier);
  // zero inliers give log(1) = 0 in the denominator, i.e. -inf: the reference's static_cast<size_t> of that is undefined
  // behaviour which on its x86-64 hosts yields 2^63 ("never abort"); a GPU conversion would saturate to 0 and abort at once
  if (!(v >= 0.0 && v < 1.8e19)) return 0x8000000000000000ull;
  return (unsigned long long)v;
}

// The LORANSAC over n >= 3 observations.  -> success; best[3] the winner (written on failure too), *trials_out the trials run, flags[0..n) the
// reported inlier mask (all zero on failure).
template <typename Obs>
__device__ __forceinline__ bool TriRansac(const TriModel& a, const Obs& obs, int n, unsigned long long min_num_trials, uint8_t* flags, double best[3],
                                          unsigned long long* trials_out) {
  unsigned long long best_inl = 0;
  double best_sum = DBL_MAX;
  best[0] = best[1] = best[2] = 0.0;
  const unsigned long long nck = (unsigned long long)n * (n - 1) * (n - 2) / 6;
  const unsigned long long max_trials = a.max_num_trials < nck ? a.max_num_trials : nck;
  unsigned long long dyn = max_trials, trials = 0;
  bool abort = false;
  int c0 = 0, c1 = 1, c2 = 2;
  for (trials = 0; trials < max_trials; ++trials) {
    if (abort) { trials += 1; break; }
    const int s0 = c0, s1 = c1, s2 = c2;
    if (c2 + 1 < n) ++c2;                                              // next 3-combination, lexicographic, wrapping
    else if (c1 + 2 < n) { ++c1; c2 = c1 + 1; }
    else if (c0 + 3 < n) { ++c0; c1 = c0 + 1; c2 = c0 + 2; }
    else { c0 = 0; c1 = 1; c2 = 2; }
    // Estimate on the minimal sample: null vector of the 3 x 4 system = signed 3x3 minors
    const int sv[3] = {obs.view(s0), obs.view(s1), obs.view(s2)};
    double ra[4], rb[4], rc[4];
    TriRow(a, sv[0], obs.line(s0), ra); TriRow(a, sv[1], obs.line(s1), rb); TriRow(a, sv[2], obs.line(s2), rc);
    const double h0 = Det3(ra, rb, rc, 1, 2, 3), h1 = -Det3(ra, rb, rc, 0, 2, 3), h2 = Det3(ra, rb, rc, 0, 1, 3), h3 = -Det3(ra, rb, rc, 0, 1, 2);
    double X[3] = {h0 / h3, h1 / h3, h2 / h3};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && (TriProjZ(a.P + 12 * (size_t)sv[i], X) >= DBL_EPSILON);
    if (!ok) continue;
    ok = TriAngle(a.centers + 3 * (size_t)sv[1], a.centers + 3 * (size_t)sv[0], X) >= a.min_tri_angle ||
         TriAngle(a.centers + 3 * (size_t)sv[2], a.centers + 3 * (size_t)sv[0], X) >= a.min_tri_angle ||
         TriAngle(a.centers + 3 * (size_t)sv[2], a.centers + 3 * (size_t)sv[1], X) >= a.min_tri_angle;
    if (!ok) continue;
    unsigned long long inl; double sum;
    TriSupport(a, obs, n, X, &inl, &sum, flags);
    if (inl > best_inl || (inl == best_inl && sum < best_sum)) {
      best_inl = inl; best_sum = sum; best[0] = X[0]; best[1] = X[1]; best[2] = X[2];
      if (inl > 3) {                                                   // local optimisation on the inliers (loransac.h:157-187)
        double S[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) S[e] = 0.0;
        for (int i = 0; i < n; ++i) {
          if (!flags[i]) continue;
          double row[4];
          TriRow(a, obs.view(i), obs.line(i), row);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) S[4 * r + c] += row[r] * row[c];
        }
        double hv[4];
        SmallestEigenvector<4>(S, hv);
        double L[3] = {hv[0] / hv[3], hv[1] / hv[3], hv[2] / hv[3]};
        bool lok = true;
        for (int i = 0; i < n && lok; ++i) if (flags[i]) lok = TriProjZ(a.P + 12 * (size_t)obs.view(i), L) >= DBL_EPSILON;
        if (lok) {
          lok = false;
          for (int i = 0; i < n && !lok; ++i) {
            if (!flags[i]) continue;
            for (int j = 0; j < i; ++j)
              if (flags[j] && TriAngle(a.centers + 3 * (size_t)obs.view(i), a.centers + 3 * (size_t)obs.view(j), L) >= a.min_tri_angle) { lok = true; break; }
          }
        }
        if (lok) {
          unsigned long long linl; double lsum;
          TriSupport(a, obs, n, L, &linl, &lsum, (uint8_t*)nullptr);
          if (linl > best_inl || (linl == best_inl && lsum < best_sum)) { best_inl = linl; best_sum = lsum; best[0] = L[0]; best[1] = L[1]; best[2] = L[2]; }
        }
      }
      dyn = TriNumTrials(best_inl, (unsigned long long)n, a.confidence, a.multiplier);
    }
    if (trials >= dyn && trials >= min_num_trials) abort = true;
  }
  *trials_out = trials;
  if (best_inl < 3) { for (int i = 0; i < n; ++i) flags[i] = 0; return false; }
  unsigned long long inl; double sum;
  TriSupport(a, obs, n, best, &inl, &sum, flags);                        // the reported inlier mask (loransac.h:213-233)
  return true;
}

}  // namespace ppsfm
