// Stand-alone driver of the host half of K24 (SelectKeptKeypoints and KeptBlockRows in csrc/sift_extract_replay.hpp) for
// tests/test_sift_extract_kept_host.py: no device, built with g++ -fsanitize=address,undefined -ffp-contract=off.  One command per line on stdin,
// the options as tests/sift_extract_host_driver.cpp reads them:
//   kept image_file width height <options>
//        ExtractOnHost on the image, then the cut twice: SelectLevels on the reference's containers, SelectKeptKeypoints on the same list with every
//        `size` set to zero (all it may read is the keypoint counts).
//        -> same|differs first_level L first_feature A num_features B levels N keypoints K kept_keypoints P ranges ok|bad membership ok|bad
//           grouping ok|bad found F two_orientations T windows_cut W skipped S octaves first:count ...
//        same: both select level L.  ranges ok: every octave's range ends at the octave's last keypoint, lies wholly above or below the cut unless
//        the cut falls inside the octave, and the counts sum to P.  membership ok: a feature is in the kept suffix [A, A + B) exactly when its
//        (octave, level) container is kept.  F, T, W, S: ExtractOnHost's full result restricted to the kept suffix - what pp_sift_extract_to_matcher
//        reports.  grouping ok: the rule that finds T (consecutive features of one keypoint share their first three floats and their container)
//        gives the full result's count when applied to all features.
//   rows num_octaves n row0[0] .. row0[n - 1] counts[0] .. counts[num_octaves * n - 1]   -> the first row of every block (KeptBlockRows)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/sift_extract_replay.hpp"

using namespace ppsfm::sift;

static double ReadDouble(std::istream& in) {
  std::string s;
  in >> s;
  return std::strtod(s.c_str(), nullptr);
}

static Options ReadOptions(std::istream& in) {
  Options o;
  in >> o.max_num_features >> o.first_octave >> o.num_octaves >> o.octave_resolution;
  o.peak_threshold = ReadDouble(in);
  o.edge_threshold = ReadDouble(in);
  in >> o.max_num_orientations >> o.upright >> o.normalization;
  return o;
}

// keypoints with more than one feature among the features [from, to)
static int64_t TwoOrientations(const HostResult& R, size_t from, size_t to) {
  int64_t n = 0;
  size_t run = 0;
  for (size_t f = from; f < to; ++f) {
    const bool same = f > from && std::memcmp(&R.keypoints[4 * f], &R.keypoints[4 * (f - 1)], 3 * sizeof(float)) == 0 &&
                      R.octave_level[2 * f] == R.octave_level[2 * (f - 1)] && R.octave_level[2 * f + 1] == R.octave_level[2 * (f - 1) + 1];
    run = same ? run + 1 : 1;
    n += run == 2;
  }
  return n;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "kept") {
      std::string image_file;
      int w = 0, h = 0;
      in >> image_file >> w >> h;
      const Options o = ReadOptions(in);
      const std::string why = CheckOptions(o, w, h);
      if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
      std::vector<uint8_t> grey((size_t)w * h);
      std::ifstream f(image_file, std::ios::binary);
      f.read(reinterpret_cast<char*>(grey.data()), (std::streamsize)grey.size());
      if (!f) { std::printf("refused cannot read %s\n", image_file.c_str()); continue; }
      const HostResult R = ExtractOnHost(o, w, h, grey.data(), true, StageSink());
      std::vector<Level> counts_only = R.levels;
      for (Level& l : counts_only) l.size = 0;
      const KeptCut c = SelectKeptKeypoints(counts_only, o.max_num_features, o.first_octave, o.num_octaves);
      const size_t first = (size_t)R.cut.first_feature, end = first + (size_t)R.cut.num_features, F = R.angles.size();
      int64_t keypoints = 0, in_ranges = 0;
      bool ranges = c.octaves.size() == R.octaves.size();
      for (size_t q = 0; q < c.octaves.size() && ranges; ++q) {
        const KeptRange& r = c.octaves[q];
        keypoints += R.octaves[q].num_keypoints;
        in_ranges += r.count;
        ranges = r.first >= 0 && r.count >= 0 && r.first + r.count == R.octaves[q].num_keypoints;
      }
      bool started = false;      // once an octave keeps anything, every later one is kept whole
      for (size_t q = 0; q < c.octaves.size() && ranges; ++q) {
        ranges = !started || c.octaves[q].first == 0;
        started = started || c.octaves[q].count > 0;
      }
      ranges = ranges && in_ranges == c.num_keypoints;
      bool membership = end == F;
      for (size_t i = 0, at = 0; i < R.levels.size(); ++i) {
        for (int64_t k = 0; k < R.levels[i].size && membership; ++k, ++at)
          membership = at < F && R.octave_level[2 * at] == R.levels[i].octave && R.octave_level[2 * at + 1] == R.levels[i].is &&
                       ((int)i >= c.first_level_to_keep) == (at >= first);
      }
      int64_t cut = 0, skipped = 0;
      for (size_t k = first; k < end && k < R.windows.size(); ++k) { cut += R.windows[k].cut; skipped += !R.windows[k].computed; }
      std::printf("%s first_level %d first_feature %lld num_features %lld levels %zu keypoints %lld kept_keypoints %lld ranges %s membership %s grouping %s",
                  c.first_level_to_keep == R.cut.first_level_to_keep ? "same" : "differs", c.first_level_to_keep, (long long)R.cut.first_feature,
                  (long long)R.cut.num_features, R.levels.size(), (long long)keypoints, (long long)c.num_keypoints, ranges ? "ok" : "bad", membership ? "ok" : "bad",
                  TwoOrientations(R, 0, F) == R.two_orientations ? "ok" : "bad");
      std::printf(" found %lld two_orientations %lld windows_cut %lld skipped %lld octaves", (long long)R.cut.num_features, (long long)TwoOrientations(R, first, end),
                  (long long)cut, (long long)skipped);
      for (const KeptRange& r : c.octaves) std::printf(" %lld:%lld", (long long)r.first, (long long)r.count);
      std::printf("\n");
    } else if (cmd == "rows") {
      size_t num_octaves = 0, n = 0;
      in >> num_octaves >> n;
      std::vector<int64_t> row0(n), counts(num_octaves * n);
      for (int64_t& v : row0) in >> v;
      for (int64_t& v : counts) in >> v;
      if (!in) { std::printf("refused short command\n"); continue; }
      const std::vector<int64_t> rows = KeptBlockRows(counts, num_octaves, n, row0.data());
      for (size_t i = 0; i < rows.size(); ++i) std::printf(i ? " %lld" : "%lld", (long long)rows[i]);
      std::printf("\n");
    } else if (!cmd.empty()) {
      std::printf("refused unknown command %s\n", cmd.c_str());
    }
    std::fflush(stdout);
  }
  return 0;
}
