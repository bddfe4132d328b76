// Host driver of csrc/initial_sets_replay.hpp (std only).  Built with -fsanitize=address,undefined by tests/test_initial_sets_replay_host.py.
//   replay min_aligned min_random max_sets R, then R runs "i0 i1 i2 i3 random count" in ascending key order      -> ReplayInitialSets
//       prints "totals aligned_tracks random_tracks aligned_sets random_sets qualified" and one "set i0 i1 i2 i3 aligned random aligned_run random_run" per
//       returned set; "unpacked ..." echoes every key through UnpackInitSetKey
// --time: the comparison partner of pp_tracks_find_initial_sets where no device result can be compared with the reference's own program - a std::map of
// std::sets restatement of the search, written from its semantics (built -O2 without sanitizers for the measurement in DESIGN.md):
//   graph C L E | line_image L | aligned L | corr_start L + 1 | corr_line E | subset n idx... (n = -1: all) | check n idx... | options min_a min_r max_sets
//       prints "time_ms t", "totals candidates aligned_tracks random_tracks aligned_sets random_sets qualified" and the "set" lines (runs as -1)
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <set>
#include <string>

#include "../privacy_preserving_sfm_amd/csrc/initial_sets_replay.hpp"

using namespace ppsfm;

static void PrintSet(const InitialSet& s) {
  std::printf("set %d %d %d %d %lld %lld %lld %lld\n", s.images[0], s.images[1], s.images[2], s.images[3], (long long)s.num_aligned, (long long)s.num_random,
              (long long)s.aligned_run, (long long)s.random_run);
}

static int Replay() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd != "replay") { std::fprintf(stderr, "ERROR: unknown command %s\n", cmd.c_str()); return 2; }
    long long min_a, min_r, max_sets, R;
    std::cin >> min_a >> min_r >> max_sets >> R;
    std::vector<uint64_t> key((size_t)R);
    std::vector<int64_t> count((size_t)R);
    for (long long i = 0; i < R; ++i) {
      int im[4], random;
      long long n;
      std::cin >> im[0] >> im[1] >> im[2] >> im[3] >> random >> n;
      key[(size_t)i] = PackInitSetKey(im[0], im[1], im[2], im[3], random != 0);
      count[(size_t)i] = n;
      if (i > 0 && key[(size_t)i] <= key[(size_t)i - 1]) { std::fprintf(stderr, "ERROR: the runs are not in ascending key order\n"); return 2; }
      int32_t back[4];
      bool rnd = false;
      UnpackInitSetKey(key[(size_t)i], back, &rnd);
      std::printf("unpacked %d %d %d %d %d\n", back[0], back[1], back[2], back[3], rnd ? 1 : 0);
    }
    const InitialSetsResult r = ReplayInitialSets(R, key.data(), count.data(), min_a, min_r, max_sets);
    std::printf("totals %lld %lld %d %d %d\n", (long long)r.num_aligned_tracks, (long long)r.num_random_tracks, r.num_aligned_sets, r.num_random_sets, r.num_qualified);
    for (const InitialSet& s : r.sets) PrintSet(s);
  }
  return 0;
}

static int Time() {
  using ImageSet = std::array<int32_t, 4>;
  using Track = std::array<int32_t, 4>;
  std::string word;
  long long C = 0, L = 0, E = 0, n = 0, min_a = 20, min_r = 20, max_sets = 10;
  std::vector<int32_t> line_image, corr_start, corr_line, check;
  std::vector<uint8_t> aligned, subset;
  while (std::cin >> word) {
    if (word == "graph") { std::cin >> C >> L >> E; subset.assign((size_t)C, 1); }
    else if (word == "line_image") { line_image.resize((size_t)L); for (auto& v : line_image) std::cin >> v; }
    else if (word == "aligned") { aligned.resize((size_t)L); for (auto& v : aligned) { int x; std::cin >> x; v = (uint8_t)x; } }
    else if (word == "corr_start") { corr_start.resize((size_t)L + 1); for (auto& v : corr_start) std::cin >> v; }
    else if (word == "corr_line") { corr_line.resize((size_t)E); for (auto& v : corr_line) std::cin >> v; }
    else if (word == "subset") {
      std::cin >> n;
      if (n >= 0) subset.assign((size_t)C, 0);
      for (long long i = 0; i < n; ++i) { int c; std::cin >> c; subset[(size_t)c] = 1; }
    } else if (word == "check") { std::cin >> n; check.resize((size_t)n); for (auto& v : check) std::cin >> v; }
    else if (word == "options") std::cin >> min_a >> min_r >> max_sets;
    else { std::fprintf(stderr, "ERROR: unknown word %s\n", word.c_str()); return 2; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::map<ImageSet, std::set<Track>> tracks[2];      // [0] aligned, [1] random
  std::vector<uint8_t> is_check((size_t)C, 0);
  for (const int32_t c : check) is_check[(size_t)c] = 1;
  long long candidates = 0;
  std::vector<int32_t> kept;
  for (int32_t r = 0; r < (int32_t)L; ++r) {
    if (!is_check[(size_t)line_image[(size_t)r]]) continue;
    kept.clear();
    for (int32_t e = corr_start[(size_t)r]; e < corr_start[(size_t)r + 1]; ++e) {
      const int32_t m = corr_line[(size_t)e];
      if (aligned[(size_t)m] == aligned[(size_t)r] && subset[(size_t)line_image[(size_t)m]]) kept.push_back(m);
    }
    const size_t k = kept.size();
    if (k < 3) continue;
    for (size_t a = 0; a < k; ++a)
      for (size_t b = a + 1; b < k; ++b)
        for (size_t c = b + 1; c < k; ++c) {
          std::map<int32_t, int32_t> by_image;      // image -> line, the first line of an image stays
          by_image.emplace(line_image[(size_t)r], r);
          by_image.emplace(line_image[(size_t)kept[a]], kept[a]);
          by_image.emplace(line_image[(size_t)kept[b]], kept[b]);
          by_image.emplace(line_image[(size_t)kept[c]], kept[c]);
          if (by_image.size() != 4) continue;
          ++candidates;
          ImageSet set;
          Track track;
          int at = 0;
          for (const auto& il : by_image) { set[(size_t)at] = il.first; track[(size_t)at] = il.second; ++at; }
          tracks[aligned[(size_t)r] ? 0 : 1][set].insert(track);
        }
  }
  std::vector<InitialSet> qualified;
  long long totals[2] = {0, 0};
  for (int c = 0; c < 2; ++c) for (const auto& st : tracks[c]) totals[c] += (long long)st.second.size();
  for (const auto& st : tracks[0]) {
    const auto other = tracks[1].find(st.first);
    if ((long long)st.second.size() < min_a || other == tracks[1].end() || (long long)other->second.size() < min_r) continue;
    InitialSet s;
    std::copy(st.first.begin(), st.first.end(), s.images);
    s.num_aligned = (int64_t)st.second.size(); s.num_random = (int64_t)other->second.size();
    qualified.push_back(s);
  }
  const size_t num_qualified = qualified.size();
  std::stable_sort(qualified.begin(), qualified.end(), [](const InitialSet& a, const InitialSet& b) { return a.num_aligned > b.num_aligned; });
  if ((long long)qualified.size() > max_sets) qualified.resize((size_t)max_sets);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("time_ms %.3f\n", ms);
  std::printf("totals %lld %lld %lld %zu %zu %zu\n", candidates, totals[0], totals[1], tracks[0].size(), tracks[1].size(), num_qualified);
  for (const InitialSet& s : qualified) PrintSet(s);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return Time();
  return Replay();
}
