// The host half of the image-pair selection (K20, pair_selection.hip): the argument rules, the key the spatial search orders by, and a literal host
// version of both selections - the spatial one of SpatialFeatureMatcher::Run (reference src/feature/matching.cc:705-768) and one iteration of
// TransitiveFeatureMatcher::Run (:818-869).
//   Spatial.  The reference searches a flann::LinearIndex: every location is visited in index order and kept in a list ordered by squared distance, a
//   new point going BEHIND the points of equal distance.  That is the ascending order of (squared distance, location index).  The squared distance is
//   FLANN's L2<float> for three components, ((d0*d0) + d1*d1) + d2*d2 with dk = a[k] - b[k], every operation rounded to float on its own.  The distance is
//   never negative and never NaN (the coordinates are finite), so its float bits order as an unsigned integer and
//   key = bits << 32 | index is the whole order in one uint64.  Of the ordered list the first knn = min(max_num_neighbors, m) are taken, the query itself is
//   dropped where it is among them, and the list is cut at the first distance > float(max_distance * max_distance).
//   Transitive.  Adjacency from the matched pairs; a candidate is {a, c}, a != c, with a common neighbour; it is dropped when {a, c} is a tried pair (the
//   matched pairs count as tried).  The result is oriented a < c and ascending.
// std only: compiles with plain g++ (tests/pair_selection_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace ppsfm {

// a result holds fewer pairs than this, and a call is given fewer locations
constexpr int64_t kPairsMaxResult = 0x7FFFFFFFll;

inline std::string PairsFormat(const char* fmt, long long a = 0, long long b = 0) {
  char buf[160];
  std::snprintf(buf, sizeof(buf), fmt, a, b);
  return buf;
}

// "" or what is wrong with the arguments of pp_pairs_spatial
inline std::string PairsCheckSpatial(int64_t num_locations, const float* xyz, int32_t max_num_neighbors, double max_distance) {
  if (num_locations < 0) return "a negative number of locations";
  if (num_locations >= kPairsMaxResult) return "too many locations";
  if (num_locations > 0 && !xyz) return "null locations";
  if (max_num_neighbors <= 0) return PairsFormat("max_num_neighbors = %lld is not positive", max_num_neighbors);
  if (!(max_distance > 0.0)) return "max_distance is not positive";
  for (int64_t i = 0; i < 3 * num_locations; ++i)
    if (!std::isfinite(xyz[i])) return PairsFormat("location %lld has a coordinate that is not finite", i / 3);
  return "";
}

// "" or what is wrong with the arguments of pp_pairs_transitive
inline std::string PairsCheckTransitive(int32_t num_images, int64_t num_matched, const int32_t* matched, int64_t num_tried, const int32_t* tried) {
  if (num_images < 0) return "a negative number of images";
  if (num_matched < 0 || num_tried < 0) return "a negative number of pairs";
  if (num_matched + num_tried >= kPairsMaxResult / 2) return "too many pairs";
  if ((num_matched > 0 && !matched) || (num_tried > 0 && !tried)) return "null pairs";
  for (int64_t i = 0; i < 2 * num_matched; ++i)
    if (matched[i] < 0 || matched[i] >= num_images) return PairsFormat("matched pair %lld names image position %lld: out of range", i / 2, matched[i]);
  for (int64_t i = 0; i < 2 * num_tried; ++i)
    if (tried[i] < 0 || tried[i] >= num_images) return PairsFormat("tried pair %lld names image position %lld: out of range", i / 2, tried[i]);
  return "";
}

// float(x op y) of two floats through double: the double result is exact (a product of two 24-bit significands) or rounded once to 53 >= 2 * 24 + 2
// bits, so rounding it to float gives the correctly rounded float result - and with a conversion between every two operations no compiler can fuse them.
inline float PairsSub(float x, float y) { return (float)((double)x - (double)y); }
inline float PairsMul(float x, float y) { return (float)((double)x * (double)y); }
inline float PairsAdd(float x, float y) { return (float)((double)x + (double)y); }

// FLANN's L2<float> over three components, unfused
inline float SpatialSqDist(const float* a, const float* b) {
  const float d0 = PairsSub(a[0], b[0]), d1 = PairsSub(a[1], b[1]), d2 = PairsSub(a[2], b[2]);
  return PairsAdd(PairsAdd(PairsMul(d0, d0), PairsMul(d1, d1)), PairsMul(d2, d2));
}

inline uint64_t SpatialKey(float sqdist, uint32_t index) {
  uint32_t bits;
  std::memcpy(&bits, &sqdist, sizeof(bits));
  return ((uint64_t)bits << 32) | index;
}
inline float SpatialKeyDist(uint64_t key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float d;
  std::memcpy(&d, &bits, sizeof(d));
  return d;
}

inline float SpatialMaxSqDist(double max_distance) { return (float)(max_distance * max_distance); }

// The literal rule, query by query: pairs (query, neighbour) as location indices and the squared distances beside them.  Returns m * m, the candidates visited.
inline int64_t SpatialPairsHost(int64_t m, const float* xyz, int32_t max_num_neighbors, double max_distance, std::vector<int32_t>* pairs,
                                std::vector<float>* sqdist) {
  pairs->clear(); sqdist->clear();
  const int64_t knn = std::min<int64_t>(max_num_neighbors, m);
  const float cut = SpatialMaxSqDist(max_distance);
  std::vector<uint64_t> keys((size_t)m);
  for (int64_t q = 0; q < m; ++q) {
    for (int64_t j = 0; j < m; ++j) keys[(size_t)j] = SpatialKey(SpatialSqDist(xyz + 3 * q, xyz + 3 * j), (uint32_t)j);
    std::sort(keys.begin(), keys.end());
    for (int64_t k = 0; k < knn; ++k) {
      const int64_t j = (int64_t)(keys[(size_t)k] & 0xFFFFFFFFull);
      const float d = SpatialKeyDist(keys[(size_t)k]);
      if (j == q) continue;
      if (d > cut) break;
      pairs->push_back((int32_t)q); pairs->push_back((int32_t)j);
      sqdist->push_back(d);
    }
  }
  return m * m;
}

// the (a, b, c) walks one iteration makes: the sum over the images b of degree(b)^2, the degrees from the matched pairs as listed
inline int64_t TransitiveVisited(int32_t num_images, int64_t num_matched, const int32_t* matched) {
  std::vector<int64_t> degree((size_t)std::max(num_images, 0), 0);
  for (int64_t i = 0; i < 2 * num_matched; ++i) ++degree[(size_t)matched[i]];
  int64_t visited = 0;
  for (int64_t d : degree) visited += d * d;
  return visited;
}

// The literal rule: pairs (a, c), a < c, ascending.  Returns the candidates visited.
inline int64_t TransitivePairsHost(int32_t num_images, int64_t num_matched, const int32_t* matched, int64_t num_tried, const int32_t* tried,
                                   std::vector<int32_t>* pairs) {
  pairs->clear();
  std::vector<std::vector<int32_t>> adjacency((size_t)std::max(num_images, 0));
  std::set<std::pair<int32_t, int32_t>> done, found;
  for (int64_t p = 0; p < num_matched; ++p) {
    const int32_t a = matched[2 * p], b = matched[2 * p + 1];
    adjacency[(size_t)a].push_back(b); adjacency[(size_t)b].push_back(a);
    done.insert({std::min(a, b), std::max(a, b)});
  }
  for (int64_t p = 0; p < num_tried; ++p) done.insert({std::min(tried[2 * p], tried[2 * p + 1]), std::max(tried[2 * p], tried[2 * p + 1])});
  int64_t visited = 0;
  for (int32_t a = 0; a < num_images; ++a)
    for (int32_t b : adjacency[(size_t)a])
      for (int32_t c : adjacency[(size_t)b]) {
        ++visited;
        if (a == c) continue;
        const std::pair<int32_t, int32_t> key{std::min(a, c), std::max(a, c)};
        if (!done.count(key)) found.insert(key);
      }
  for (const auto& key : found) { pairs->push_back(key.first); pairs->push_back(key.second); }
  return visited;
}

}  // namespace ppsfm
