// The host half of the SIFT descriptor matcher (K17, sift_match.hip): the rule of MatchSiftFeaturesCPUBruteForce (reference src/feature/sift.cc:54-143,
// 170-203, 957-970) in integers.
//   dist(i, j) = sum_k d1[i][k] * d2[j][k] over 128 uint8 - an int, at most 128 * 255^2 = 8 323 200 < 2^24: its cast to float is exact.
//   One way (:54-106), per row i: best = the largest dist, best_j = the LOWEST j that attains it, second = the second largest WITH multiplicity (a maximum that
//   occurs twice gives second == best); a dist of 0 never counts (best = second = 0 and best_j = -1 at the start, strict comparisons).
//   The two float rules, a(d) = acos(min(kDistNorm * d, 1.0f)), kDistNorm = 1 / 512^2, the options' doubles cast to float at the call:
//     reject if a(best) > max_distance;  then reject if a(best) >= max_ratio * a(second).
// a(d) depends on min(d, 262144) only (kDistNorm * d is exact - a power of two times an integer below 2^24 - and >= 1 from there on).  BuildSiftThresholds
// evaluates it once over 0 .. 262144 with THIS host's acosf and turns the two rules into integers:
//     the distance rule passes  iff  best >= d_min                                           (and best >= 1: there is a match at all)
//     the ratio rule passes     iff  min(second, 262144) <= s_max[min(best, 262144) - d_min]  (-1: no second passes)
// which is what the device compares.  That needs a and max_ratio * a to be non-increasing; both are checked over the whole domain while the table is built and
// the options are refused otherwise.  The rule has this one source on purpose: another acosf (a device's, numpy's) decides boundary cases differently.
// SiftMatchingOptions::max_num_matches is not here: it only truncates the inputs of the reference's SiftGPU path, the brute-force rule never reads it.
// Below that: the plain restatement of the one-way scan, the decision and the cross-check (:108-143) the CPU tests compare with.
// std only: compiles with plain g++ (tests/sift_match_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace ppsfm {

constexpr int32_t kSiftDim = 128;
constexpr int32_t kSiftClamp = 512 * 512;      // from here on kDistNorm * d >= 1 and a(d) = acos(1) = 0

inline float SiftAngle(int32_t dist) {
  const float kDistNorm = 1.0f / (512.0f * 512.0f);
  return std::acos(std::min(kDistNorm * static_cast<float>(dist), 1.0f));
}

// the reference's two rules as it states them (:84-99), for one (best, second) with best >= 1
inline bool SiftAcceptDirect(float max_ratio, float max_distance, int32_t best, int32_t second) {
  const float best_normed = SiftAngle(best);
  if (best_normed > max_distance) return false;
  const float second_normed = SiftAngle(second);
  if (best_normed >= max_ratio * second_normed) return false;
  return true;
}

struct SiftThresholds {
  int32_t d_min = 0;
  std::vector<int32_t> s_max;      // kSiftClamp - d_min + 1 entries
  bool Accept(int32_t best, int32_t second) const {
    if (best < 1 || best < d_min) return false;
    return std::min(second, kSiftClamp) <= s_max[(size_t)(std::min(best, kSiftClamp) - d_min)];
  }
};

// SiftMatchingOptions::Check (feature/sift.h:117-145) for the fields the rule reads
inline bool SiftOptionsValid(double max_ratio, double max_distance, int32_t min_num_matches) {
  return max_ratio > 0.0 && max_distance > 0.0 && min_num_matches >= 0;      // (a NaN fails both comparisons)
}

// -> "" and the thresholds, or what is wrong: "invalid ..." for options Check refuses, "internal ..." when a monotonicity does not hold on this host
inline std::string BuildSiftThresholds(double max_ratio_d, double max_distance_d, SiftThresholds* out) {
  if (!SiftOptionsValid(max_ratio_d, max_distance_d, 0)) return "invalid: max_ratio and max_distance must be positive";
  const float max_ratio = static_cast<float>(max_ratio_d), max_distance = static_cast<float>(max_distance_d);
  std::vector<float> a((size_t)kSiftClamp + 1), r((size_t)kSiftClamp + 1);
  for (int32_t d = 0; d <= kSiftClamp; ++d) {
    a[(size_t)d] = SiftAngle(d);
    r[(size_t)d] = max_ratio * a[(size_t)d];
    if (!(a[(size_t)d] >= 0.0f) || !(r[(size_t)d] >= 0.0f)) return "internal: acosf left [0, pi] or the ratio bound is not a number";
    if (d > 0 && (a[(size_t)d] > a[(size_t)d - 1] || r[(size_t)d] > r[(size_t)d - 1])) return "internal: acosf is not monotonic on this host";
  }
  if (a[(size_t)kSiftClamp] != 0.0f) return "internal: acosf(1) is not 0 on this host";
  int32_t d_min = 0;      // a(kSiftClamp) = 0 <= max_distance: the loop ends
  while (a[(size_t)d_min] > max_distance) ++d_min;
  out->d_min = d_min;
  out->s_max.assign((size_t)(kSiftClamp - d_min) + 1, -1);
  // a(best) falls as best grows, so the seconds that pass - a prefix 0 .. s_max, r being non-increasing - only grow: one sweep
  int32_t s = -1;
  for (int32_t b = d_min; b <= kSiftClamp; ++b) {
    while (s < kSiftClamp && a[(size_t)b] < r[(size_t)s + 1]) ++s;
    out->s_max[(size_t)(b - d_min)] = s;
  }
  return "";
}

// the one-way scan of :64-77 for every row of d1 (n1 x 128) against d2 (n2 x 128), in the reference's order
inline void SiftTop2Host(const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2, int32_t* best_j, int32_t* best, int32_t* second) {
  for (int32_t i = 0; i < n1; ++i) {
    int32_t bj = -1, b = 0, s = 0;
    for (int32_t j = 0; j < n2; ++j) {
      int32_t dist = 0;
      for (int32_t k = 0; k < kSiftDim; ++k) dist += (int32_t)d1[(size_t)i * kSiftDim + k] * (int32_t)d2[(size_t)j * kSiftDim + k];
      if (dist > b) { bj = j; s = b; b = dist; }
      else if (dist > s) s = dist;
    }
    best_j[i] = bj; best[i] = b; second[i] = s;
  }
}

// m[i] = best_j[i] where the row has a match that passes both rules, else -1
inline void SiftDecideHost(const SiftThresholds& t, int32_t n, const int32_t* best_j, const int32_t* best, const int32_t* second, int32_t* m) {
  for (int32_t i = 0; i < n; ++i) m[i] = (best_j[i] >= 0 && t.Accept(best[i], second[i])) ? best_j[i] : -1;
}

// FindBestMatchesBruteForce :118-142: the pairs (i, m12[i]) in ascending i; with cross_check only those with m21[m12[i]] == i
inline std::vector<int32_t> SiftEmitHost(int32_t n1, const int32_t* m12, const int32_t* m21, bool cross_check) {
  std::vector<int32_t> pairs;
  for (int32_t i = 0; i < n1; ++i) {
    const int32_t j = m12[i];
    if (j < 0) continue;
    if (cross_check && m21[j] != i) continue;
    pairs.push_back(i); pairs.push_back(j);
  }
  return pairs;
}

// MatchSiftFeaturesCPUBruteForce on the host: (i, j) pairs, flat
inline std::vector<int32_t> SiftMatchHost(const SiftThresholds& t, bool cross_check, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2) {
  std::vector<int32_t> bj((size_t)std::max(n1, n2)), b(bj.size()), s(bj.size()), m12((size_t)n1), m21((size_t)n2);
  SiftTop2Host(d1, n1, d2, n2, bj.data(), b.data(), s.data());
  SiftDecideHost(t, n1, bj.data(), b.data(), s.data(), m12.data());
  if (cross_check) {
    SiftTop2Host(d2, n2, d1, n1, bj.data(), b.data(), s.data());
    SiftDecideHost(t, n2, bj.data(), b.data(), s.data(), m21.data());
  }
  return SiftEmitHost(n1, m12.data(), m21.data(), cross_check);
}

}  // namespace ppsfm
