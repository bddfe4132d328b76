// K21 - the arithmetic of SIFT extraction, written once: every value the reference's CPU extractor (ExtractSiftFeaturesCPU, feature/sift.cc:399-573,
// over VLFeat's vl_sift_*) computes per pixel or per keypoint, restated in plain IEEE operations.  The kernels of sift_extract.hip call these
// functions, one lane per output; tests/sift_extract_host_driver.cpp calls the same functions serially on the CPU (g++ -ffp-contract=off), which is
// the CPU mirror and the way a difference is located without a device.  Std only.
// The rules that make the two agree bit for bit:
//   - no operation is contracted: every function body starts with PP_SIFT_EXACT (clang: the pragma; g++: the unit's -ffp-contract=off);
//   - the mixed float / double expressions are spelled with the conversions C applies in the reference, one operation per rounding;
//   - no libm call is made here.  exp (the Gaussian taps, the 257-entry table of fast_expn), pow (a keypoint's sigma) and sin / cos (the
//     descriptor's rotation) are host work in sift_extract_replay.hpp: a few per keypoint, and the host's libm is the reference's.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PP_SIFT_HD __host__ __device__ inline
#else
#define PP_SIFT_HD inline
#endif
#if defined(__clang__)
#define PP_SIFT_EXACT _Pragma("clang fp contract(off)")
#else
#define PP_SIFT_EXACT
#endif

namespace ppsfm {
namespace sift {

constexpr double kPi = 3.141592653589793;
constexpr float kEpsF = 1.19209290E-07F;
constexpr double kEpsD = 2.220446049250313e-16;
constexpr int kExpnSize = 256;               // fast_expn: exp(-x) on [0, 25] from a table of 257 entries, linear in between
constexpr double kExpnMax = 25.0;
constexpr int kOriBins = 36;
constexpr int kMaxAngles = 4;
constexpr int kDescBins = 128;               // 4 x 4 cells of 8 orientations
constexpr double kMagnif = 3.0;
constexpr double kWindowSize = 2.0;          // NBP / 2

PP_SIFT_HD float FloatFromBits(uint32_t u) { union { uint32_t i; float f; } v; v.i = u; return v.f; }
PP_SIFT_HD uint32_t BitsOfFloat(float f) { union { uint32_t i; float f; } v; v.f = f; return v.i; }
PP_SIFT_HD float AbsF(float x) { return FloatFromBits(BitsOfFloat(x) & 0x7fffffffu); }
PP_SIFT_HD double AbsD(double x) { return x < 0 ? -x : (x == 0 ? 0.0 : x); }      // (-0.0 -> 0.0 as clearing the sign bit does; every use compares)

// (long) x with floor's rule for negative values
PP_SIFT_HD long FloorF(float x) { const long xi = (long)x; return (x >= 0 || (float)xi == x) ? xi : xi - 1; }
PP_SIFT_HD long FloorD(double x) { const long xi = (long)x; return (x >= 0 || (double)xi == x) ? xi : xi - 1; }

PP_SIFT_HD float Mod2PiF(float x) {
  PP_SIFT_EXACT
  const float two_pi = (float)(2 * kPi);
  while (x > two_pi) x -= two_pi;
  while (x < 0.0F) x += two_pi;
  return x;
}

PP_SIFT_HD float FastAtan2F(float y, float x) {
  PP_SIFT_EXACT
  const float c3 = 0.1821F, c1 = 0.9675F;
  const float abs_y = AbsF(y) + kEpsF;
  float r, angle;
  if (x >= 0) { r = (x - abs_y) / (x + abs_y); angle = (float)(kPi / 4); }
  else { r = (x + abs_y) / (abs_y - x); angle = (float)(3 * kPi / 4); }
  angle += (c3 * r * r - c1) * r;
  return (y < 0) ? -angle : angle;
}

// two Newton steps from the integer guess; 0 below 1e-8
PP_SIFT_HD float FastSqrtF(float x) {
  PP_SIFT_EXACT
  if ((double)x < 1e-8) return 0.f;
  const float xhalf = 0.5f * x;
  float u = FloatFromBits((uint32_t)(0x5f3759df - ((int32_t)BitsOfFloat(x) >> 1)));
  u = u * (1.5f - xhalf * u * u);
  u = u * (1.5f - xhalf * u * u);
  return x * u;
}

PP_SIFT_HD double FastExpn(const double* __restrict__ table, double x) {
  PP_SIFT_EXACT
  if (x > kExpnMax) return 0.0;
  x *= kExpnSize / kExpnMax;
  const int i = (int)FloorD(x);
  const double r = x - i;
  const double a = table[i], b = table[i + 1];
  return a + r * (b - a);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Scale space

PP_SIFT_HD float PixelFromByte(uint8_t v) { return (float)v / 255.0f; }

// element X of a row of w values stretched to 2 w (copy_and_upsample_rows): the value, the mean with the next one, the last one twice
PP_SIFT_HD float UpsampleRowValue(const float* __restrict__ row, int w, int X) {
  PP_SIFT_EXACT
  const int x = X >> 1;
  if (x >= w - 1) return row[w - 1];
  if ((X & 1) == 0) return row[x];
  return (float)(0.5 * (double)(row[x] + row[x + 1]));
}

// One output pixel of the column convolution (vl_imconvcol_vf, padding by continuity): v[i * stride], i = 0 .. ntaps - 1, are the ntaps = 2 W + 1
// input values around it from first to last, the clamping at the image's ends already applied; the taps are taken from the last one down, and the sum
// grows tap by tap from zero.
PP_SIFT_HD float ConvolveTaps(const float* __restrict__ v, int stride, const float* __restrict__ taps, int ntaps) {
  PP_SIFT_EXACT
  float acc = 0.f;
  for (int i = 0; i < ntaps; ++i) acc += v[i * stride] * taps[ntaps - 1 - i];
  return acc;
}

// The 26-neighbour test of vl_sift_detect at pt = dog(x, y, s), 1 <= x <= w - 2, 1 <= y <= h - 2, s with a level on either side.
PP_SIFT_HD bool IsExtremum(const float* __restrict__ pt, int yo, int so, double threshold /* 0.8 * peak_thresh */) {
  const float v = *pt;
  bool above = (double)v >= threshold, below = (double)v <= -threshold;
  if (!above && !below) return false;
  for (int ds = -1; ds <= 1; ++ds)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (ds == 0 && dy == 0 && dx == 0) continue;
        const float n = pt[dx + dy * yo + ds * so];
        above = above && v > n;
        below = below && v < n;
      }
  return above || below;
}

struct Refined {
  int32_t ix, iy, is;      // where the refinement ended
  int32_t good;            // 1: a keypoint
  int32_t moves;           // iterations that ended with a move
  int32_t reject;          // 0 kept; the first test that failed: 1 peak value, 2 edge score, 3 an offset of 1.5 or more, 4 outside the octave
  double xn, yn, sn;       // the refined position in the octave's pixels and levels
};

// The refinement of vl_sift_detect for the candidate (x, y, s): up to five 3 x 3 eliminations, a move of one pixel where the offset exceeds 0.6,
// then the tests.  dog: the octave's levels s_min .. s_max - 1, w x h each.
PP_SIFT_HD Refined RefineCandidate(const float* __restrict__ dog, int w, int h, int s_min, int s_max, int x, int y, int s, double tp, double te) {
  PP_SIFT_EXACT
  const int yo = w;
  const int64_t so = (int64_t)w * h;
  double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0;
  double A[9], b[3] = {0, 0, 0};
  int dx = 0, dy = 0, moves = 0;
  const float* pt = dog;
#define PP_SIFT_AT(ax, ay, as) (pt[(ax) + (ay) * yo + (as) * so])
#define PP_SIFT_A(i, j) (A[(i) + (j) * 3])
  for (int iter = 0; iter < 5; ++iter) {
    x += dx;
    y += dy;
    pt = dog + x + (int64_t)yo * y + so * (s - s_min);
    Dx = 0.5 * (double)(PP_SIFT_AT(+1, 0, 0) - PP_SIFT_AT(-1, 0, 0));
    Dy = 0.5 * (double)(PP_SIFT_AT(0, +1, 0) - PP_SIFT_AT(0, -1, 0));
    Ds = 0.5 * (double)(PP_SIFT_AT(0, 0, +1) - PP_SIFT_AT(0, 0, -1));
    const double c2 = 2.0 * (double)PP_SIFT_AT(0, 0, 0);
    Dxx = (double)(PP_SIFT_AT(+1, 0, 0) + PP_SIFT_AT(-1, 0, 0)) - c2;
    Dyy = (double)(PP_SIFT_AT(0, +1, 0) + PP_SIFT_AT(0, -1, 0)) - c2;
    Dss = (double)(PP_SIFT_AT(0, 0, +1) + PP_SIFT_AT(0, 0, -1)) - c2;
    Dxy = 0.25 * (double)(PP_SIFT_AT(+1, +1, 0) + PP_SIFT_AT(-1, -1, 0) - PP_SIFT_AT(-1, +1, 0) - PP_SIFT_AT(+1, -1, 0));
    const double Dxs = 0.25 * (double)(PP_SIFT_AT(+1, 0, +1) + PP_SIFT_AT(-1, 0, -1) - PP_SIFT_AT(-1, 0, +1) - PP_SIFT_AT(+1, 0, -1));
    const double Dys = 0.25 * (double)(PP_SIFT_AT(0, +1, +1) + PP_SIFT_AT(0, -1, -1) - PP_SIFT_AT(0, -1, +1) - PP_SIFT_AT(0, +1, -1));
    PP_SIFT_A(0, 0) = Dxx; PP_SIFT_A(1, 1) = Dyy; PP_SIFT_A(2, 2) = Dss;
    PP_SIFT_A(0, 1) = PP_SIFT_A(1, 0) = Dxy;
    PP_SIFT_A(0, 2) = PP_SIFT_A(2, 0) = Dxs;
    PP_SIFT_A(1, 2) = PP_SIFT_A(2, 1) = Dys;
    b[0] = -Dx; b[1] = -Dy; b[2] = -Ds;
    bool singular = false;
    for (int j = 0; j < 3 && !singular; ++j) {
      double maxa = 0, maxabsa = 0;
      int maxi = -1;
      for (int i = j; i < 3; ++i) {
        const double a = PP_SIFT_A(i, j), absa = AbsD(a);
        if (absa > maxabsa) { maxa = a; maxabsa = absa; maxi = i; }
      }
      if (maxabsa < (double)1e-10f) { b[0] = 0; b[1] = 0; b[2] = 0; singular = true; break; }
      const int i = maxi;
      for (int jj = j; jj < 3; ++jj) {
        const double tmp = PP_SIFT_A(i, jj); PP_SIFT_A(i, jj) = PP_SIFT_A(j, jj); PP_SIFT_A(j, jj) = tmp;
        PP_SIFT_A(j, jj) /= maxa;
      }
      { const double tmp = b[j]; b[j] = b[i]; b[i] = tmp; }
      b[j] /= maxa;
      for (int ii = j + 1; ii < 3; ++ii) {
        const double f = PP_SIFT_A(ii, j);
        for (int jj = j; jj < 3; ++jj) PP_SIFT_A(ii, jj) -= f * PP_SIFT_A(j, jj);
        b[ii] -= f * b[j];
      }
    }
    // (the reference runs the backward substitution after a singular exit as well, on b = 0 and the half-eliminated A: b stays 0 unless A holds a
    // non-finite value, and then 0 * that is NaN there and here alike)
    for (int i = 2; i > 0; --i) {
      const double f = b[i];
      for (int ii = i - 1; ii >= 0; --ii) b[ii] -= f * PP_SIFT_A(ii, i);
    }
    dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
    dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
    if (dx == 0 && dy == 0) break;
    ++moves;
  }
  Refined r;
  const double val = (double)PP_SIFT_AT(0, 0, 0) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
  const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
  r.xn = x + b[0]; r.yn = y + b[1]; r.sn = s + b[2];
  r.ix = x; r.iy = y; r.is = s; r.moves = moves;
  r.reject = 0;
  if (!(AbsD(val) > tp)) r.reject = 1;
  else if (!(score < (te + 1) * (te + 1) / te && score >= 0)) r.reject = 2;
  else if (!(AbsD(b[0]) < 1.5 && AbsD(b[1]) < 1.5 && AbsD(b[2]) < 1.5)) r.reject = 3;
  else if (!(r.xn >= 0 && r.xn <= w - 1 && r.yn >= 0 && r.yn <= h - 1 && r.sn >= s_min && r.sn <= s_max)) r.reject = 4;
  r.good = r.reject == 0;
  return r;
#undef PP_SIFT_AT
#undef PP_SIFT_A
}

// update_gradient at (x, y) of a w x h level, w, h >= 2: central differences inside, one-sided ones on the border; modulus and angle in [0, 2 pi]
PP_SIFT_HD void GradientAt(const float* __restrict__ src, int w, int h, int x, int y, float* mod, float* ang) {
  PP_SIFT_EXACT
  const float* p = src + (int64_t)y * w + x;
  float gx, gy;
  if (x == 0) gx = p[1] - p[0];
  else if (x == w - 1) gx = p[0] - p[-1];
  else gx = (float)(0.5 * (double)(p[1] - p[-1]));
  if (y == 0) gy = p[w] - p[0];
  else if (y == h - 1) gy = p[0] - p[-w];
  else gy = (float)(0.5 * (double)(p[w] - p[-w]));
  *mod = FastSqrtF(gx * gx + gy * gy);
  *ang = Mod2PiF((float)((double)FastAtan2F(gy, gx) + 2 * kPi));
}

// A keypoint as VlSiftKeypoint holds it (floats), in the coordinates of the whole image
struct Keypoint {
  float x, y, s, sigma;
  int32_t ix, iy, is, o;
};

// vl_sift_calc_keypoint_orientations: grad = the modulus / angle pairs of level k.is of the current octave (w x h), xper = 2^o.  Up to four angles.
PP_SIFT_HD int Orientations(const float* __restrict__ grad, int w, int h, int s_min, int s_max, const Keypoint& k, double xper,
                            const double* __restrict__ expn, double* angles) {
  PP_SIFT_EXACT
  const double winf = 1.5;
  const int xo = 2, yo = 2 * w;
  const double x = (double)k.x / xper, y = (double)k.y / xper, sigma = (double)k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double sigmaw = winf * sigma;
  const double w3 = 3.0 * sigmaw;
  const int W = w3 >= 2.0 ? (int)FloorD(w3) : 1;      // VL_MAX(floor(3 sigmaw), 1)
  if (xi < 0 || xi > w - 1 || yi < 0 || yi > h - 1 || si < s_min + 1 || si > s_max - 2) return 0;
  double hist[kOriBins];
  for (int i = 0; i < kOriBins; ++i) hist[i] = 0.0;
  const float* pt = grad + xo * xi + (int64_t)yo * yi;
  const int ys0 = -W > -yi ? -W : -yi, ys1 = W < h - 1 - yi ? W : h - 1 - yi;
  const int xs0 = -W > -xi ? -W : -xi, xs1 = W < w - 1 - xi ? W : w - 1 - xi;
  for (int ys = ys0; ys <= ys1; ++ys) {
    for (int xs = xs0; xs <= xs1; ++xs) {
      const double dx = (double)(xi + xs) - x, dy = (double)(yi + ys) - y;
      const double r2 = dx * dx + dy * dy;
      if (r2 >= W * W + 0.6) continue;
      const double wgt = FastExpn(expn, r2 / (2 * sigmaw * sigmaw));
      const double mod = pt[xs * xo + ys * yo], ang = pt[xs * xo + ys * yo + 1];
      const double fbin = kOriBins * ang / (2 * kPi);
      const int bin = (int)FloorD(fbin - 0.5);
      const double rbin = fbin - bin - 0.5;
      hist[(bin + kOriBins) % kOriBins] += (1 - rbin) * mod * wgt;
      hist[(bin + 1) % kOriBins] += rbin * mod * wgt;
    }
  }
  for (int iter = 0; iter < 6; ++iter) {
    double prev = hist[kOriBins - 1];
    const double first = hist[0];
    int i;
    for (i = 0; i < kOriBins - 1; ++i) {
      const double newh = (prev + hist[i] + hist[(i + 1) % kOriBins]) / 3.0;
      prev = hist[i];
      hist[i] = newh;
    }
    hist[i] = (prev + hist[i] + first) / 3.0;
  }
  double maxh = 0;
  for (int i = 0; i < kOriBins; ++i) maxh = maxh < hist[i] ? hist[i] : maxh;
  int n = 0;
  for (int i = 0; i < kOriBins && n < kMaxAngles; ++i) {
    const double h0 = hist[i], hm = hist[(i - 1 + kOriBins) % kOriBins], hp = hist[(i + 1 + kOriBins) % kOriBins];
    if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
      const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
      angles[n++] = 2 * kPi * (i + di + 0.5) / kOriBins;
    }
  }
  return n;
}

PP_SIFT_HD float NormalizeHistogram(float* d) {
  PP_SIFT_EXACT
  float norm = 0.0f;
  for (int i = 0; i < kDescBins; ++i) norm += d[i] * d[i];
  norm = FastSqrtF(norm) + kEpsF;
  for (int i = 0; i < kDescBins; ++i) d[i] /= norm;
  return norm;
}

struct DescriptorWindow { int32_t computed, cut; };      // computed: the bounds check passed; cut: the image border cut the window

// vl_sift_calc_keypoint_descriptor for the angle angle0, st0 = sin(angle0) and ct0 = cos(angle0) from the host: the 4 x 4 x 8 histogram in VLFeat's
// bin order, normalised, clamped at 0.2, normalised again.  Where the reference's bounds check returns without writing (it leaves the caller's
// uninitialised buffer as it is) the descriptor here is all zero.
PP_SIFT_HD DescriptorWindow Descriptor(const float* __restrict__ grad, int w, int h, int s_min, int s_max, const Keypoint& k, double xper, double angle0,
                                       double st0, double ct0, const double* __restrict__ expn, float* descr) {
  PP_SIFT_EXACT
  const int xo = 2, yo = 2 * w;
  const double x = (double)k.x / xper, y = (double)k.y / xper, sigma = (double)k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double SBP = kMagnif * sigma + kEpsD;
  const int W = (int)FloorD(1.4142135623730951 * SBP * 5 / 2.0 + 0.5);      // sqrt(2.0) SBP (NBP + 1) / 2 + 0.5
  for (int i = 0; i < kDescBins; ++i) descr[i] = 0.f;
  DescriptorWindow out = {0, 0};
  if (xi < 0 || xi >= w || yi < 0 || yi >= h - 1 || si < s_min + 1 || si > s_max - 2) return out;
  out.computed = 1;
  const float* pt = grad + xi * xo + (int64_t)yi * yo;
  float* dpt = descr + 2 * 32 + 2 * 8;      // the bin of the centre: 32 per y, 8 per x, 1 per orientation
  const int y0 = -W > 1 - yi ? -W : 1 - yi, y1 = W < h - yi - 2 ? W : h - yi - 2;
  const int x0 = -W > 1 - xi ? -W : 1 - xi, x1 = W < w - xi - 2 ? W : w - xi - 2;
  out.cut = y0 != -W || y1 != W || x0 != -W || x1 != W;
  const float wsigma = (float)kWindowSize;
  for (int dyi = y0; dyi <= y1; ++dyi) {
    for (int dxi = x0; dxi <= x1; ++dxi) {
      const float mod = pt[dxi * xo + dyi * yo], angle = pt[dxi * xo + dyi * yo + 1];
      const float theta = Mod2PiF((float)((double)angle - angle0));
      const float dx = (float)((double)(xi + dxi) - x), dy = (float)((double)(yi + dyi) - y);
      const float nx = (float)((ct0 * (double)dx + st0 * (double)dy) / SBP);
      const float ny = (float)((-st0 * (double)dx + ct0 * (double)dy) / SBP);
      const float nt = (float)((double)(8 * theta) / (2 * kPi));
      const float win = (float)FastExpn(expn, (double)(nx * nx + ny * ny) / (2.0 * (double)wsigma * (double)wsigma));
      const int binx = (int)FloorF((float)((double)nx - 0.5)), biny = (int)FloorF((float)((double)ny - 0.5)), bint = (int)FloorF(nt);
      const float rbinx = (float)((double)nx - (binx + 0.5)), rbiny = (float)((double)ny - (biny + 0.5)), rbint = nt - (float)bint;
      for (int dbinx = 0; dbinx < 2; ++dbinx)
        for (int dbiny = 0; dbiny < 2; ++dbiny)
          for (int dbint = 0; dbint < 2; ++dbint) {
            if (binx + dbinx >= -2 && binx + dbinx < 2 && biny + dbiny >= -2 && biny + dbiny < 2) {
              const float weight = win * mod * AbsF((float)(1 - dbinx) - rbinx) * AbsF((float)(1 - dbiny) - rbiny) * AbsF((float)(1 - dbint) - rbint);
              dpt[((bint + dbint) % 8) + (biny + dbiny) * 32 + (binx + dbinx) * 8] += weight;
            }
          }
    }
  }
  NormalizeHistogram(descr);
  for (int i = 0; i < kDescBins; ++i)
    if ((double)descr[i] > 0.2) descr[i] = (float)0.2;
  NormalizeHistogram(descr);
  return out;
}

// 0 for x < 0.5, else round half away from zero; x >= 0 and finite
PP_SIFT_HD float RoundF(float x) {
  PP_SIFT_EXACT
  const float t = (float)(int64_t)x;
  return x - t >= 0.5f ? t + 1.0f : t;
}

// The reference's last steps on one descriptor (VLFeat order in, UBC order out): L1-root (normalization 0) or L2 (1) normalisation,
// round(512 v) cut to 0 .. 255, the bin permutation.  THE PROJECT'S RULE for the norm, where the reference's is Eigen's reduction order: the sum runs
// over the 128 entries from first to last in float32, one addition per entry.  A descriptor whose norm is zero gives 128 zero bytes.
PP_SIFT_HD void FinishDescriptor(const float* __restrict__ raw, int normalization, uint8_t* out) {
  PP_SIFT_EXACT
  float norm = 0.f;
  if (normalization == 0) {
    for (int i = 0; i < kDescBins; ++i) norm += AbsF(raw[i]);
  } else {
    for (int i = 0; i < kDescBins; ++i) norm += raw[i] * raw[i];
    norm = __builtin_sqrtf(norm);      // (correctly rounded on the host and, in the library's build, on the device)
  }
  for (int c = 0; c < 16; ++c)
    for (int k = 0; k < 8; ++k) {
      float v = 0.f;
      if (norm > 0.f) {
        v = raw[8 * c + k] / norm;
        if (normalization == 0) v = __builtin_sqrtf(v);
      }
      const float scaled = RoundF(512.0f * v);
      out[8 * c + ((8 - k) & 7)] = (uint8_t)(scaled > 255.f ? 255.f : scaled);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The descriptor by parts, for a wavefront per feature (k_sift_describe_wave, and ExtractOnHost's wave route through the same functions).
// Descriptor() + FinishDescriptor() above are the definition; these restate their pieces so that 64 lanes can share one feature and still give every
// bit of it.  THE ORDER RULE: a bin receives its additions in the window's scan order (dyi outer, dxi inner) from 0.f.  The eight contributions of one
// pixel go to eight different bins, so the order of the pixels is the whole order: a bin's owner that walks the pixels in scan order and adds what
// they give to ITS bin performs the additions of Descriptor() on that bin, one for one.  The weight is (((win * mod) * ax) * ay) * at in float32, as
// the reference's product associates; the three norms run over the entries 0 .. 127 in index order.

// what Descriptor() settles before its loops: the keypoint in the octave's pixels, the bin size, the window dyi = y0 .. y1, dxi = x0 .. x1 (empty,
// y1 < y0, for a keypoint that fails the bounds check - and possibly for one that passes it)
struct DescriptorFrame {
  double x, y, SBP;
  int32_t xi, yi, y0, y1, x0, x1;
  DescriptorWindow win;
};

PP_SIFT_HD DescriptorFrame MakeDescriptorFrame(int w, int h, int s_min, int s_max, const Keypoint& k, double xper) {
  PP_SIFT_EXACT
  DescriptorFrame f;
  f.x = (double)k.x / xper; f.y = (double)k.y / xper;
  const double sigma = (double)k.sigma / xper;
  f.xi = (int)(f.x + 0.5); f.yi = (int)(f.y + 0.5);
  const int xi = f.xi, yi = f.yi, si = k.is;
  f.SBP = kMagnif * sigma + kEpsD;
  const int W = (int)FloorD(1.4142135623730951 * f.SBP * 5 / 2.0 + 0.5);
  f.y0 = 0; f.y1 = -1; f.x0 = 0; f.x1 = -1;
  f.win.computed = 0; f.win.cut = 0;
  if (xi < 0 || xi >= w || yi < 0 || yi >= h - 1 || si < s_min + 1 || si > s_max - 2) return f;
  f.win.computed = 1;
  f.y0 = -W > 1 - yi ? -W : 1 - yi; f.y1 = W < h - yi - 2 ? W : h - yi - 2;
  f.x0 = -W > 1 - xi ? -W : 1 - xi; f.x1 = W < w - xi - 2 ? W : w - xi - 2;
  f.win.cut = f.y0 != -W || f.y1 != W || f.x0 != -W || f.x1 != W;
  return f;
}

// the pixels of the window; pixel p of the scan is (dxi, dyi) = (x0 + p % nx, y0 + p / nx), nx = x1 - x0 + 1
PP_SIFT_HD int32_t DescriptorWindowPixels(const DescriptorFrame& f) {
  const int nx = f.x1 - f.x0 + 1, ny = f.y1 - f.y0 + 1;
  return nx > 0 && ny > 0 ? nx * ny : 0;
}

// one window pixel before it is spread over its eight bins: 32 bytes, read by every bin owner
struct alignas(16) DescriptorTap {
  float wm;                        // win * mod
  float rbinx, rbiny, rbint;
  int32_t binx, biny, bint, pad_;
};

// the body of Descriptor()'s pixel loop down to the bins, for the pixel (dxi, dyi) of the window with gradient (mod, angle)
PP_SIFT_HD DescriptorTap DescriptorSample(const DescriptorFrame& f, double angle0, double st0, double ct0, const double* __restrict__ expn, int dxi, int dyi,
                                          float mod, float angle) {
  PP_SIFT_EXACT
  const float wsigma = (float)kWindowSize;
  const float theta = Mod2PiF((float)((double)angle - angle0));
  const float dx = (float)((double)(f.xi + dxi) - f.x), dy = (float)((double)(f.yi + dyi) - f.y);
  const float nx = (float)((ct0 * (double)dx + st0 * (double)dy) / f.SBP);
  const float ny = (float)((-st0 * (double)dx + ct0 * (double)dy) / f.SBP);
  const float nt = (float)((double)(8 * theta) / (2 * kPi));
  const float win = (float)FastExpn(expn, (double)(nx * nx + ny * ny) / (2.0 * (double)wsigma * (double)wsigma));
  DescriptorTap t;
  t.binx = (int)FloorF((float)((double)nx - 0.5)); t.biny = (int)FloorF((float)((double)ny - 0.5)); t.bint = (int)FloorF(nt);
  t.rbinx = (float)((double)nx - (t.binx + 0.5)); t.rbiny = (float)((double)ny - (t.biny + 0.5)); t.rbint = nt - (float)t.bint;
  t.wm = win * mod;
  t.pad_ = 0;
  return t;
}

// What the owner of the bins (orientation t0, t0 + 1; t0 even) of the spatial cell (cx, cy), -2 <= cx, cy < 2, adds for one pixel: *acc0 is bin
// t0 + (cy + 2) * 32 + (cx + 2) * 8 of the descriptor, *acc1 the next one.  The pixel reaches the cell with dbinx = cx - binx and dbiny = cy - biny
// where both are 0 or 1 (Descriptor()'s in-range test stands as written); of its two orientations (bint + dbint) % 8 at most one is t0 and at most
// one t0 + 1.
PP_SIFT_HD void DescriptorFold(const DescriptorTap& t, int cx, int cy, int t0, float* acc0, float* acc1) {
  PP_SIFT_EXACT
  const int dbinx = cx - t.binx, dbiny = cy - t.biny;
  if (dbinx < 0 || dbinx > 1 || dbiny < 0 || dbiny > 1) return;
  if (!(t.binx + dbinx >= -2 && t.binx + dbinx < 2 && t.biny + dbiny >= -2 && t.biny + dbiny < 2)) return;
  const float wxy = t.wm * AbsF((float)(1 - dbinx) - t.rbinx) * AbsF((float)(1 - dbiny) - t.rbiny);
  for (int dbint = 0; dbint < 2; ++dbint) {
    const int o = (t.bint + dbint) % 8;
    if (o != t0 && o != t0 + 1) continue;
    const float weight = wxy * AbsF((float)(1 - dbint) - t.rbint);
    if (o == t0) *acc0 += weight; else *acc1 += weight;
  }
}

// NormalizeHistogram()'s norm: the sequential sum of squares over the 128 entries, the fast root, the epsilon
PP_SIFT_HD float HistogramNorm(const float* d) {
  PP_SIFT_EXACT
  float norm = 0.0f;
  for (int i = 0; i < kDescBins; ++i) norm += d[i] * d[i];
  return FastSqrtF(norm) + kEpsF;
}
PP_SIFT_HD float ClampBin(float v) { return (double)v > 0.2 ? (float)0.2 : v; }

// FinishDescriptor() in two parts: its norm over the 128 entries in order, and one entry of its output (raw[i] goes to byte UbcIndex(i))
PP_SIFT_HD float FinishNorm(const float* raw, int normalization) {
  PP_SIFT_EXACT
  float norm = 0.f;
  if (normalization == 0) {
    for (int i = 0; i < kDescBins; ++i) norm += AbsF(raw[i]);
    return norm;
  }
  for (int i = 0; i < kDescBins; ++i) norm += raw[i] * raw[i];
  return __builtin_sqrtf(norm);
}
PP_SIFT_HD uint8_t FinishByte(float raw, float norm, int normalization) {
  PP_SIFT_EXACT
  float v = 0.f;
  if (norm > 0.f) {
    v = raw / norm;
    if (normalization == 0) v = __builtin_sqrtf(v);
  }
  const float scaled = RoundF(512.0f * v);
  return (uint8_t)(scaled > 255.f ? 255.f : scaled);
}
PP_SIFT_HD int UbcIndex(int i) { return (i & ~7) + ((8 - (i & 7)) & 7); }

}  // namespace sift
}  // namespace ppsfm
