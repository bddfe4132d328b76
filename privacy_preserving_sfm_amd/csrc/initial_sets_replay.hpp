// Host replay of the end of the image-set search of IncrementalMapper::RegisterInitialLineImages - std only, no HIP:
//   the qualifying rule                         reference src/sfm/incremental_mapper.cc:393-409
//   the ranking                                                                        :416-423
//   the truncation to max_num_init_tries sets                                          :434-435
// The device enumerates, sorts and de-duplicates the 4-view tracks and run-length encodes them by (image set, class) (initial_sets.hip: K15a / K15b, then
// the sorts); what is left is a pass over those runs, replayed here.  initial_sets.hip drives it.
// THE SET KEY packs the four image indices of a set, most significant first, and the class (0 = gravity-aligned, 1 = random) in the lowest bit: ascending key
// order is ascending image set, lexicographic over the image indices, and inside a set the aligned tracks first - the order of the reference's std::map, and of
// the line lists it hands to the solver (:459-481).  15 bits per image: C <= kInitSetMaxImages.
// PINNED where the reference is unspecified (std::sort is not stable, :418): sets of equal aligned count are ordered by ascending image set.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ppsfm {

constexpr int kInitSetImageBits = 15;
constexpr int kInitSetMaxImages = 1 << kInitSetImageBits;
constexpr int kInitSetKeyBits = 4 * kInitSetImageBits + 1;

#if defined(__HIPCC__)
#define PP_INIT_SETS_HD __host__ __device__
#else
#define PP_INIT_SETS_HD
#endif

PP_INIT_SETS_HD inline uint64_t PackInitSetKey(int i0, int i1, int i2, int i3, bool random) {
  uint64_t key = (uint64_t)i0;
  key = (key << kInitSetImageBits) | (uint64_t)i1;
  key = (key << kInitSetImageBits) | (uint64_t)i2;
  key = (key << kInitSetImageBits) | (uint64_t)i3;
  return (key << 1) | (random ? 1u : 0u);
}

inline void UnpackInitSetKey(uint64_t key, int32_t images[4], bool* random) {
  *random = (key & 1) != 0;
  key >>= 1;
  for (int i = 3; i >= 0; --i) { images[i] = (int32_t)(key & (kInitSetMaxImages - 1)); key >>= kInitSetImageBits; }
}

struct InitialSet {
  int32_t images[4];
  int64_t num_aligned = 0, num_random = 0;
  int64_t aligned_run = -1, random_run = -1;      // indices into the runs the replay was given
};

struct InitialSetsResult {
  std::vector<InitialSet> sets;      // the returned sets, best first
  int64_t num_aligned_tracks = 0, num_random_tracks = 0;
  int32_t num_aligned_sets = 0, num_random_sets = 0, num_qualified = 0;
};

// run_key ascending and distinct, run_count > 0: what the run-length encoding of the sorted set keys gives
inline InitialSetsResult ReplayInitialSets(int64_t num_runs, const uint64_t* run_key, const int64_t* run_count, int64_t min_num_aligned_tracks,
                                           int64_t min_num_random_tracks, int64_t max_num_sets) {
  InitialSetsResult r;
  std::vector<InitialSet> qualified;
  for (int64_t i = 0; i < num_runs; ++i) {
    const bool random = (run_key[i] & 1) != 0;
    (random ? r.num_random_tracks : r.num_aligned_tracks) += run_count[i];
    ++(random ? r.num_random_sets : r.num_aligned_sets);
    if (random) continue;
    // the aligned run of a set; its random run, if there is one, is the next run
    const bool has_random = i + 1 < num_runs && run_key[i + 1] == (run_key[i] | 1);
    const int64_t num_random = has_random ? run_count[i + 1] : 0;
    if (run_count[i] < min_num_aligned_tracks || !has_random || num_random < min_num_random_tracks) continue;      // (:399-402)
    InitialSet s;
    bool unused = false;
    UnpackInitSetKey(run_key[i], s.images, &unused);
    s.num_aligned = run_count[i]; s.num_random = num_random; s.aligned_run = i; s.random_run = i + 1;
    qualified.push_back(s);
  }
  r.num_qualified = (int32_t)qualified.size();
  // (:418-423 with unaligned_weight = 0) `qualified` is in ascending image set: a stable sort by descending aligned count is the pinned order
  std::stable_sort(qualified.begin(), qualified.end(), [](const InitialSet& a, const InitialSet& b) { return a.num_aligned > b.num_aligned; });
  if ((int64_t)qualified.size() > max_num_sets) qualified.resize((size_t)std::max<int64_t>(max_num_sets, 0));
  r.sets = std::move(qualified);
  return r;
}

}  // namespace ppsfm
