// Device-side camera maps of the reference's 11 camera models
// (reference src/base/camera_models.h: WorldToImage/Distortion per model, ids :189-349), and the other direction,
// ImageToWorld (double only, host and device: IterativeUndistortion :547-588, FOV's Undistortion :1176-1210) at the end.
//
// MI355X design: the maps are written once, templated on the scalar, and instantiated with
//   T = double            residual-only evaluation (cost at a trial point)
//   T = Dual<2>           value + 2x2 derivative w.r.t. the normalised coordinates (u,v): the chain
//                         rule of the line residual only ever needs DW at two points, so the pose /
//                         point Jacobians cost two width-2 duals instead of the reference's
//                         width-(10+N) Ceres jets
//   T = Dual<2+N>         additionally d/d(intrinsics), only when intrinsics are refined
// The model id is per observation (its image's camera).  It is uniform over a wavefront - and the
// switch does not diverge - only where the observations are sorted by image and the cameras of a
// wavefront's images share a model; in point order, or with cameras of several models, the lanes of
// a wavefront take different arms with different Dual widths one after the other: slower, and still
// correct (every lane reads its own model id, intrinsics row and Jacobian columns).
#pragma once
#include <hip/hip_runtime.h>

namespace ppsfm {

template <int N>
struct Dual {
  double a;
  double d[N];
};

#define PP_HD __host__ __device__ __forceinline__

template <int N> PP_HD Dual<N> MakeDual(double s) { Dual<N> r; r.a = s; for (int k = 0; k < N; ++k) r.d[k] = 0.0; return r; }
template <int N> PP_HD Dual<N> MakeVar(double s, int idx) { Dual<N> r = MakeDual<N>(s); r.d[idx] = 1.0; return r; }

template <int N> PP_HD Dual<N> operator+(const Dual<N>& x, const Dual<N>& y) { Dual<N> r; r.a = x.a + y.a; for (int k = 0; k < N; ++k) r.d[k] = x.d[k] + y.d[k]; return r; }
template <int N> PP_HD Dual<N> operator-(const Dual<N>& x, const Dual<N>& y) { Dual<N> r; r.a = x.a - y.a; for (int k = 0; k < N; ++k) r.d[k] = x.d[k] - y.d[k]; return r; }
template <int N> PP_HD Dual<N> operator*(const Dual<N>& x, const Dual<N>& y) { Dual<N> r; r.a = x.a * y.a; for (int k = 0; k < N; ++k) r.d[k] = x.a * y.d[k] + x.d[k] * y.a; return r; }
template <int N> PP_HD Dual<N> operator/(const Dual<N>& x, const Dual<N>& y) {
  Dual<N> r; const double inv = 1.0 / y.a; r.a = x.a * inv;
  for (int k = 0; k < N; ++k) r.d[k] = (x.d[k] - r.a * y.d[k]) * inv;
  return r;
}
template <int N> PP_HD Dual<N> operator+(const Dual<N>& x, double s) { Dual<N> r = x; r.a += s; return r; }
template <int N> PP_HD Dual<N> operator+(double s, const Dual<N>& x) { Dual<N> r = x; r.a += s; return r; }
template <int N> PP_HD Dual<N> operator-(const Dual<N>& x, double s) { Dual<N> r = x; r.a -= s; return r; }
template <int N> PP_HD Dual<N> operator-(double s, const Dual<N>& x) { Dual<N> r; r.a = s - x.a; for (int k = 0; k < N; ++k) r.d[k] = -x.d[k]; return r; }
template <int N> PP_HD Dual<N> operator*(const Dual<N>& x, double s) { Dual<N> r; r.a = x.a * s; for (int k = 0; k < N; ++k) r.d[k] = x.d[k] * s; return r; }
template <int N> PP_HD Dual<N> operator*(double s, const Dual<N>& x) { return x * s; }
template <int N> PP_HD Dual<N> operator/(const Dual<N>& x, double s) { return x * (1.0 / s); }
template <int N> PP_HD Dual<N> operator/(double s, const Dual<N>& y) {
  Dual<N> r; const double inv = 1.0 / y.a; r.a = s * inv;
  for (int k = 0; k < N; ++k) r.d[k] = -r.a * y.d[k] * inv;
  return r;
}

PP_HD double Val(double x) { return x; }
template <int N> PP_HD double Val(const Dual<N>& x) { return x.a; }

PP_HD double Sqrt(double x) { return sqrt(x); }
PP_HD double Atan(double x) { return atan(x); }
PP_HD double Tan(double x) { return tan(x); }
template <int N> PP_HD Dual<N> Sqrt(const Dual<N>& x) { Dual<N> r; r.a = sqrt(x.a); const double g = 0.5 / r.a; for (int k = 0; k < N; ++k) r.d[k] = g * x.d[k]; return r; }
template <int N> PP_HD Dual<N> Atan(const Dual<N>& x) { Dual<N> r; r.a = atan(x.a); const double g = 1.0 / (1.0 + x.a * x.a); for (int k = 0; k < N; ++k) r.d[k] = g * x.d[k]; return r; }
template <int N> PP_HD Dual<N> Tan(const Dual<N>& x) { Dual<N> r; r.a = tan(x.a); const double g = 1.0 + r.a * r.a; for (int k = 0; k < N; ++k) r.d[k] = g * x.d[k]; return r; }

enum CameraModelId {
  kSimplePinhole = 0, kPinhole = 1, kSimpleRadial = 2, kRadial = 3, kOpenCV = 4, kOpenCVFisheye = 5,
  kFullOpenCV = 6, kFOV = 7, kSimpleRadialFisheye = 8, kRadialFisheye = 9, kThinPrismFisheye = 10
};

PP_HD int CameraNumParams(int model) {
  switch (model) {
    case kSimplePinhole: return 3;
    case kPinhole: case kSimpleRadial: case kSimpleRadialFisheye: return 4;
    case kRadial: case kFOV: case kRadialFisheye: return 5;
    case kOpenCV: case kOpenCVFisheye: return 8;
    case kFullOpenCV: case kThinPrismFisheye: return 12;
    default: return -1;
  }
}
PP_HD int CameraNumFocal(int model) {
  return (model == kSimplePinhole || model == kSimpleRadial || model == kRadial || model == kSimpleRadialFisheye ||
          model == kRadialFisheye) ? 1 : 2;
}

constexpr double kDblEps = 2.220446049250313e-16;

// Equidistant fisheye radial term shared by OPENCV_FISHEYE / SIMPLE_RADIAL_FISHEYE / RADIAL_FISHEYE
// (camera_models.h:962-986, :1271-1289, :1347-1367): the distortion (du, dv), the distorted point being (u + du, v + dv).  -> false at the centre
// (r <= DBL_EPSILON), where the distortion is zero and (du, dv) is not written.
template <typename T, typename P, int ORDER>
PP_HD bool FisheyeDistortion(const P* k, const T& u, const T& v, T* du, T* dv) {
  const T r = Sqrt(u * u + v * v);
  if (Val(r) > kDblEps) {
    const T theta = Atan(r);
    const T t2 = theta * theta;
    T series = 1.0 + k[0] * t2;
    if (ORDER >= 2) {
      const T t4 = t2 * t2;
      series = series + k[1] * t4;
      if (ORDER >= 4) series = series + k[2] * (t4 * t2) + k[3] * (t4 * t4);
    }
    const T thetad = theta * series;
    // u * thetad / r - u, added to u by the caller: the reference's two-step form, so values match to rounding
    *du = u * thetad / r - u;
    *dv = v * thetad / r - v;
    return true;
  }
  return false;
}

// CameraModel::Distortion of the reference, MODEL a compile-time id; p is the camera's whole parameter row.  (du, dv) is what the model adds to (u, v) -
// except for FOV, whose Distortion returns the distorted point itself (camera_models.h:1137-1173), and THIN_PRISM_FISHEYE, whose argument is the point
// after the equidistant map (:1413-1429).  The pinhole models have none.  Both directions call it: WorldToImage below, arm by arm, with the operations in
// the order they always had, and IterativeUndistortion through the switch of DistortionOf.  -> false where the distortion is zero and (du, dv) is not
// written: the centre of a fisheye model, a model without distortion.
template <int MODEL, typename T, typename P>
PP_HD bool Distortion(const P* p, const T& u, const T& v, T* du, T* dv) {
  if (MODEL == kSimpleRadial) {
    const T r2 = u * u + v * v;
    const T radial = p[3] * r2;
    *du = u * radial;
    *dv = v * radial;
  } else if (MODEL == kRadial) {
    const T r2 = u * u + v * v;
    const T radial = p[3] * r2 + p[4] * r2 * r2;
    *du = u * radial;
    *dv = v * radial;
  } else if (MODEL == kOpenCV) {
    const T u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
    const T radial = p[4] * r2 + p[5] * r2 * r2;
    *du = u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2);
    *dv = v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2);
  } else if (MODEL == kOpenCVFisheye) {
    return FisheyeDistortion<T, P, 4>(p + 4, u, v, du, dv);
  } else if (MODEL == kFullOpenCV) {
    const T u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
    const T r4 = r2 * r2, r6 = r4 * r2;
    const T radial = (1.0 + p[4] * r2 + p[5] * r4 + p[8] * r6) / (1.0 + p[9] * r2 + p[10] * r4 + p[11] * r6);
    *du = u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2) - u;
    *dv = v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2) - v;
  } else if (MODEL == kFOV) {
    const P omega = p[4];
    const T radius2 = u * u + v * v;
    const P omega2 = omega * omega;
    T factor;
    if (Val(omega2) < 1e-4) {
      factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
    } else if (Val(radius2) < 1e-4) {
      const P th = Tan(omega / 2.0);
      factor = (-2.0 * th * (4.0 * radius2 * th * th - 3.0)) / (3.0 * omega);
    } else {
      const T radius = Sqrt(radius2);
      const T numerator = Atan(radius * 2.0 * Tan(omega / 2.0));
      factor = numerator / (radius * omega);
    }
    *du = u * factor;
    *dv = v * factor;
  } else if (MODEL == kSimpleRadialFisheye) {
    return FisheyeDistortion<T, P, 1>(p + 3, u, v, du, dv);
  } else if (MODEL == kRadialFisheye) {
    return FisheyeDistortion<T, P, 2>(p + 3, u, v, du, dv);
  } else if (MODEL == kThinPrismFisheye) {
    const T u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
    const T r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
    const T radial = p[4] * r2 + p[5] * r4 + p[8] * r6 + p[9] * r8;
    *du = u * radial + 2.0 * p[6] * uv + p[7] * (r2 + 2.0 * u2) + p[10] * r2;
    *dv = v * radial + 2.0 * p[7] * uv + p[6] * (r2 + 2.0 * v2) + p[11] * r2;
  } else {
    return false;
  }
  return true;
}

// the same by a run-time model id
PP_HD void DistortionOf(int model, const double* p, double u, double v, double* du, double* dv) {
  bool set = false;
  switch (model) {
    case kSimpleRadial: set = Distortion<kSimpleRadial>(p, u, v, du, dv); break;
    case kRadial: set = Distortion<kRadial>(p, u, v, du, dv); break;
    case kOpenCV: set = Distortion<kOpenCV>(p, u, v, du, dv); break;
    case kOpenCVFisheye: set = Distortion<kOpenCVFisheye>(p, u, v, du, dv); break;
    case kFullOpenCV: set = Distortion<kFullOpenCV>(p, u, v, du, dv); break;
    case kFOV: set = Distortion<kFOV>(p, u, v, du, dv); break;
    case kSimpleRadialFisheye: set = Distortion<kSimpleRadialFisheye>(p, u, v, du, dv); break;
    case kRadialFisheye: set = Distortion<kRadialFisheye>(p, u, v, du, dv); break;
    case kThinPrismFisheye: set = Distortion<kThinPrismFisheye>(p, u, v, du, dv); break;
    default: break;
  }
  if (!set) { *du = 0.0; *dv = 0.0; }
}

// (u,v) -> pixel (x,y).  P is the intrinsics scalar type (double, or Dual when refining intrinsics).
template <typename T, typename P>
PP_HD void WorldToImage(int model, const P* p, const T& u, const T& v, T* x, T* y) {
  switch (model) {
    case kSimplePinhole:
      *x = p[0] * u + p[1];
      *y = p[0] * v + p[2];
      return;
    case kPinhole:
      *x = p[0] * u + p[2];
      *y = p[1] * v + p[3];
      return;
    case kSimpleRadial: {
      T du, dv;
      Distortion<kSimpleRadial>(p, u, v, &du, &dv);
      *x = p[0] * (u + du) + p[1];
      *y = p[0] * (v + dv) + p[2];
      return;
    }
    case kRadial: {
      T du, dv;
      Distortion<kRadial>(p, u, v, &du, &dv);
      *x = p[0] * (u + du) + p[1];
      *y = p[0] * (v + dv) + p[2];
      return;
    }
    case kOpenCV: {
      T du, dv;
      Distortion<kOpenCV>(p, u, v, &du, &dv);
      *x = p[0] * (u + du) + p[2];
      *y = p[1] * (v + dv) + p[3];
      return;
    }
    case kOpenCVFisheye: {
      T du, dv, xd, yd;
      if (Distortion<kOpenCVFisheye>(p, u, v, &du, &dv)) {
        xd = u + du;
        yd = v + dv;
      } else {
        xd = u;
        yd = v;
      }
      *x = p[0] * xd + p[2];
      *y = p[1] * yd + p[3];
      return;
    }
    case kFullOpenCV: {
      T du, dv;
      Distortion<kFullOpenCV>(p, u, v, &du, &dv);
      *x = p[0] * (u + du) + p[2];
      *y = p[1] * (v + dv) + p[3];
      return;
    }
    case kFOV: {
      T xd, yd;
      Distortion<kFOV>(p, u, v, &xd, &yd);
      *x = p[0] * xd + p[2];
      *y = p[1] * yd + p[3];
      return;
    }
    case kSimpleRadialFisheye: {
      T du, dv, xd, yd;
      if (Distortion<kSimpleRadialFisheye>(p, u, v, &du, &dv)) {
        xd = u + du;
        yd = v + dv;
      } else {
        xd = u;
        yd = v;
      }
      *x = p[0] * xd + p[1];
      *y = p[0] * yd + p[2];
      return;
    }
    case kRadialFisheye: {
      T du, dv, xd, yd;
      if (Distortion<kRadialFisheye>(p, u, v, &du, &dv)) {
        xd = u + du;
        yd = v + dv;
      } else {
        xd = u;
        yd = v;
      }
      *x = p[0] * xd + p[1];
      *y = p[0] * yd + p[2];
      return;
    }
    case kThinPrismFisheye: {
      const T r = Sqrt(u * u + v * v);
      T uu, vv;
      if (Val(r) > kDblEps) {
        const T theta = Atan(r);
        uu = theta * u / r;
        vv = theta * v / r;
      } else {
        uu = u;
        vv = v;
      }
      T du, dv;
      Distortion<kThinPrismFisheye>(p, uu, vv, &du, &dv);
      *x = p[0] * (uu + du) + p[2];
      *y = p[1] * (vv + dv) + p[3];
      return;
    }
    default:
      *x = u * __builtin_nan("");
      *y = *x;
  }
}

constexpr int kUndistortMaxIterations = 100;      // camera_models.h:552

// BaseCameraModel::IterativeUndistortion (camera_models.h:547-588), restated: Newton on x + Distortion(x) - x0 with the Jacobian from central
// differences of step max(DBL_EPSILON, |1e-6 x_i|), at most 100 iterations, over once the squared step is below 1e-10.  The step is
// J^-1 (x + dx - x0) with J^-1 the adjugate over the determinant, as Eigen inverts a 2 x 2.  -> the iterations that ran, 1 .. 100.
PP_HD int IterativeUndistortion(int model, const double* p, double* u, double* v) {
  const double x0 = *u, y0 = *v;
  double x = x0, y = y0;
  int it = 0;
  while (it < kUndistortMaxIterations) {
    ++it;
    const double s0 = fmax(kDblEps, fabs(1e-6 * x));
    const double s1 = fmax(kDblEps, fabs(1e-6 * y));
    double dx, dy, bx0, by0, fx0, fy0, bx1, by1, fx1, fy1;
    DistortionOf(model, p, x, y, &dx, &dy);
    DistortionOf(model, p, x - s0, y, &bx0, &by0);
    DistortionOf(model, p, x + s0, y, &fx0, &fy0);
    DistortionOf(model, p, x, y - s1, &bx1, &by1);
    DistortionOf(model, p, x, y + s1, &fx1, &fy1);
    const double j00 = 1 + (fx0 - bx0) / (2 * s0);
    const double j01 = (fx1 - bx1) / (2 * s1);
    const double j10 = (fy0 - by0) / (2 * s0);
    const double j11 = 1 + (fy1 - by1) / (2 * s1);
    const double inv_det = 1.0 / (j00 * j11 - j01 * j10);
    const double rx = x + dx - x0, ry = y + dy - y0;
    const double step_x = (j11 * inv_det) * rx + (-j01 * inv_det) * ry;
    const double step_y = (-j10 * inv_det) * rx + (j00 * inv_det) * ry;
    x -= step_x;
    y -= step_y;
    if (step_x * step_x + step_y * step_y < 1e-10) break;
  }
  *u = x; *v = y;
  return it;
}

// FOVCameraModel::Undistortion (camera_models.h:1176-1210): closed form, with its two Taylor branches
PP_HD void FovUndistortion(double omega, double u, double v, double* ou, double* ov) {
  const double radius2 = u * u + v * v;
  const double omega2 = omega * omega;
  double factor;
  if (omega2 < 1e-4) {
    factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
  } else if (radius2 < 1e-4) {
    factor = (omega * (omega * omega * radius2 + 3.0)) / (6.0 * tan(omega / 2.0));
  } else {
    const double radius = sqrt(radius2);
    const double numerator = tan(radius * omega);
    factor = numerator / (radius * 2.0 * tan(omega / 2.0));
  }
  *ou = u * factor;
  *ov = v * factor;
}

// pixel (x,y) -> (u,v): every model's ImageToWorld of the reference.  *ran_all (may be null) = 1 when the Newton iteration of a
// distorted model ran all of its 100 iterations, else 0.
PP_HD void ImageToWorld(int model, const double* p, double x, double y, double* u, double* v, int* ran_all = nullptr) {
  int iterations = 0;
  switch (model) {
    case kSimplePinhole:
      *u = (x - p[1]) / p[0];
      *v = (y - p[2]) / p[0];
      break;
    case kPinhole:
      *u = (x - p[2]) / p[0];
      *v = (y - p[3]) / p[1];
      break;
    case kSimpleRadial: case kRadial: case kSimpleRadialFisheye: case kRadialFisheye:
      *u = (x - p[1]) / p[0];
      *v = (y - p[2]) / p[0];
      iterations = IterativeUndistortion(model, p, u, v);
      break;
    case kOpenCV: case kOpenCVFisheye: case kFullOpenCV:
      *u = (x - p[2]) / p[0];
      *v = (y - p[3]) / p[1];
      iterations = IterativeUndistortion(model, p, u, v);
      break;
    case kFOV:
      FovUndistortion(p[4], (x - p[2]) / p[0], (y - p[3]) / p[1], u, v);
      break;
    case kThinPrismFisheye: {      // camera_models.h:1437-1457: Newton in the equidistant plane, then theta -> tan(theta)
      *u = (x - p[2]) / p[0];
      *v = (y - p[3]) / p[1];
      iterations = IterativeUndistortion(model, p, u, v);
      const double theta = sqrt(*u * *u + *v * *v);
      const double theta_cos_theta = theta * cos(theta);
      if (theta_cos_theta > kDblEps) {
        const double scale = sin(theta) / theta_cos_theta;
        *u *= scale;
        *v *= scale;
      }
      break;
    }
    default:
      *u = x * __builtin_nan("");
      *v = *u;
  }
  if (ran_all) *ran_all = iterations >= kUndistortMaxIterations;
}

}  // namespace ppsfm
