// The host half of the correspondence-graph builder (K18, corr_graph.hip): the rules of DatabaseCache::Load (reference src/base/database_cache.cc:82-191)
// and CorrespondenceGraph::AddCorrespondences (src/base/correspondence_graph.cc:56-163) that have an order in them.
//   A pair is stored under its smaller image first (the columns swapped when it was given the other way) and the pairs are applied in ascending
//   (image1, image2).  Within a pair AddCorrespondences walks the matches in their order: a match whose line index does not exist is skipped, and so is
//   one whose line ALREADY corresponds to the other image.  Pair ids are unique, so "already" can only come from an earlier match of the same pair: the
//   rule is a greedy, sequential one over the valid matches of one pair - accept (x1, x2) iff neither x1 nor x2 was accepted before.
//   When the valid matches repeat indices on AT MOST ONE side the greedy rule is "accepted iff first occurrence of its index on the repeating side":
//   the other side never rejects.  With first occurrences taken on both sides that is "first on side 1 and first on side 2", which is what the device
//   computes; every output of the matcher is of this kind (ascending, distinct first indices).  With repeats on BOTH sides a rejected match can shadow a later one -
//   (a, x) (a, y) (b, y): the third is accepted because the second was rejected, though y occurred before - and the pair goes through CorrReplayPair
//   below, the literal loop.
// std only: compiles with plain g++ (tests/corr_graph_replay_host_driver.cpp runs it under the sanitizers without a device).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

namespace ppsfm {

// what the device reports per used pair, and what CorrClassifyPair restates on the host
struct CorrPairClass {
  int64_t valid = 0;        // matches with both indices in range
  int64_t repeats1 = 0;     // valid matches whose first index occurred in an earlier valid match of the pair
  int64_t repeats2 = 0;     // the same on the second index
};

// the pair needs the sequential loop iff its valid matches repeat on both sides
inline bool CorrNeedsReplay(int64_t repeats1, int64_t repeats2) { return repeats1 > 0 && repeats2 > 0; }

// matches: count x 2 (x1, x2) as stored, i.e. already under the smaller image first; n1, n2 the line counts of the two images
inline CorrPairClass CorrClassifyPair(int32_t n1, int32_t n2, const int32_t* matches, int64_t count) {
  CorrPairClass c;
  std::vector<uint8_t> seen1((size_t)std::max(n1, 0), 0), seen2((size_t)std::max(n2, 0), 0);
  for (int64_t m = 0; m < count; ++m) {
    const int32_t x1 = matches[2 * m], x2 = matches[2 * m + 1];
    if (x1 < 0 || x1 >= n1 || x2 < 0 || x2 >= n2) continue;
    ++c.valid;
    c.repeats1 += seen1[(size_t)x1]; c.repeats2 += seen2[(size_t)x2];
    seen1[(size_t)x1] = 1; seen2[(size_t)x2] = 1;
  }
  return c;
}

// AddCorrespondences for one pair (correspondence_graph.cc:95-160): accepted[m] = 1 for the matches that enter the graph -> their number
inline int64_t CorrReplayPair(int32_t n1, int32_t n2, const int32_t* matches, int64_t count, uint8_t* accepted) {
  std::vector<uint8_t> used1((size_t)std::max(n1, 0), 0), used2((size_t)std::max(n2, 0), 0);
  int64_t num = 0;
  for (int64_t m = 0; m < count; ++m) {
    const int32_t x1 = matches[2 * m], x2 = matches[2 * m + 1];
    accepted[m] = 0;
    if (x1 < 0 || x1 >= n1 || x2 < 0 || x2 >= n2) continue;      // "has no valid line index"
    if (used1[(size_t)x1] || used2[(size_t)x2]) continue;         // "duplicate correspondence"
    used1[(size_t)x1] = 1; used2[(size_t)x2] = 1;
    accepted[m] = 1;
    ++num;
  }
  return num;
}

// the parallel rule the device applies, on the host: first valid occurrence on both sides.  Equals CorrReplayPair unless CorrNeedsReplay.
inline int64_t CorrFirstOccurrencePair(int32_t n1, int32_t n2, const int32_t* matches, int64_t count, uint8_t* accepted) {
  std::vector<uint8_t> seen1((size_t)std::max(n1, 0), 0), seen2((size_t)std::max(n2, 0), 0);
  int64_t num = 0;
  for (int64_t m = 0; m < count; ++m) {
    const int32_t x1 = matches[2 * m], x2 = matches[2 * m + 1];
    accepted[m] = 0;
    if (x1 < 0 || x1 >= n1 || x2 < 0 || x2 >= n2) continue;
    accepted[m] = !seen1[(size_t)x1] && !seen2[(size_t)x2];
    seen1[(size_t)x1] = 1; seen2[(size_t)x2] = 1;
    num += accepted[m];
  }
  return num;
}

struct CorrPairPlan {            // one input pair as the database would hold it
  int32_t image1 = 0, image2 = 0;      // image1 <= image2
  int32_t swapped = 0;           // the input named the larger image first: its columns are (x2, x1)
  int32_t used = 0;              // more than min_num_matches matches
  int32_t rank = -1;             // position among the used pairs with image1 != image2, in ascending (image1, image2); -1 otherwise
};

// The pair list of one build: validated, oriented, ranked.  -> "" or what is wrong (PP_ERR_INVALID).  connected[k] = image k belongs to a used pair.
inline std::string CorrPlanPairs(int32_t num_images, int32_t min_num_matches, int64_t num_pairs, const int32_t* pairs, const int64_t* match_start,
                                 std::vector<CorrPairPlan>* plan, std::vector<uint8_t>* connected, int64_t* num_ranked) {
  if (min_num_matches < 0) return "min_num_matches is negative";
  if (num_pairs < 0) return "num_pairs is negative";
  if (match_start[0] != 0) return "match_start[0] != 0";
  for (int64_t p = 0; p < num_pairs; ++p)
    if (match_start[p + 1] < match_start[p]) return "match_start decreases at pair " + std::to_string(p);
  plan->assign((size_t)num_pairs, CorrPairPlan());
  for (int64_t p = 0; p < num_pairs; ++p) {
    const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= num_images || b < 0 || b >= num_images) return "pair " + std::to_string(p) + " names an image out of range";
    CorrPairPlan& q = (*plan)[(size_t)p];
    q.image1 = std::min(a, b); q.image2 = std::max(a, b); q.swapped = a > b;
    q.used = match_start[p + 1] - match_start[p] > (int64_t)min_num_matches;
  }
  std::vector<int64_t> order((size_t)num_pairs);
  std::iota(order.begin(), order.end(), (int64_t)0);
  auto key = [&](int64_t p) { return ((int64_t)(*plan)[(size_t)p].image1 << 32) | (int64_t)(*plan)[(size_t)p].image2; };
  std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
  for (int64_t k = 1; k < num_pairs; ++k)
    if (key(order[(size_t)k]) == key(order[(size_t)k - 1])) return "pair " + std::to_string(order[(size_t)k]) + " is listed twice";
  connected->assign((size_t)num_images, 0);
  int64_t rank = 0;
  for (int64_t k = 0; k < num_pairs; ++k) {
    CorrPairPlan& q = (*plan)[(size_t)order[(size_t)k]];
    if (!q.used) continue;
    (*connected)[(size_t)q.image1] = 1; (*connected)[(size_t)q.image2] = 1;
    if (q.image1 != q.image2) q.rank = (int32_t)rank++;      // "Cannot use self-matches": connected, nothing added
  }
  *num_ranked = rank;
  return "";
}

}  // namespace ppsfm
