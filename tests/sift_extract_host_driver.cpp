// Stand-alone driver of csrc/sift_core.hpp and csrc/sift_extract_replay.hpp (K21) for tests/test_sift_extract_host.py: no device, built with
// g++ -fsanitize=address,undefined -ffp-contract=off.  The whole extraction runs serially through the functions the kernels call.
// One command per line on stdin; the options are
//   max_num_features first_octave num_octaves octave_resolution peak_threshold edge_threshold max_num_orientations upright normalization
// with the two thresholds as %la or decimal:
//   check width height <options>                                  -> ok,  or  refused <why>
//   extract image_file width height dump_file want_descriptors <options>
//                                                                 -> ok,  or  refused <why>; the stages and results go to dump_file as records of
//                                                                    (uint32 name length, name, uint32 element size, uint64 count, the elements)
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
  return std::strtod(s.c_str(), nullptr);      // (reads nan, inf and hex floats)
}

static Options ReadOptions(std::istream& in) {
  Options o;
  in >> o.max_num_features >> o.first_octave >> o.num_octaves >> o.octave_resolution;
  o.peak_threshold = ReadDouble(in);
  o.edge_threshold = ReadDouble(in);
  in >> o.max_num_orientations >> o.upright >> o.normalization;
  return o;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "check") {
      long long w = 0, h = 0;
      in >> w >> h;
      const std::string why = CheckOptions(ReadOptions(in), w, h);
      std::printf("%s\n", why.empty() ? "ok" : ("refused " + why).c_str());
    } else if (cmd == "extract") {
      std::string image_file, dump_file;
      int w = 0, h = 0, want = 1;
      in >> image_file >> w >> h >> dump_file >> want;
      const Options o = ReadOptions(in);
      const std::string why = CheckOptions(o, w, h);
      if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
      std::vector<uint8_t> grey((size_t)w * h);
      std::ifstream f(image_file, std::ios::binary);
      f.read(reinterpret_cast<char*>(grey.data()), (std::streamsize)grey.size());
      if (!f) { std::printf("refused cannot read %s\n", image_file.c_str()); continue; }
      std::ofstream out(dump_file, std::ios::binary);
      const StageSink sink = [&out](const std::string& name, size_t elem, size_t count, const void* data) {
        const uint32_t n = (uint32_t)name.size(), e = (uint32_t)elem;
        const uint64_t c = count;
        out.write(reinterpret_cast<const char*>(&n), 4);
        out.write(name.data(), n);
        out.write(reinterpret_cast<const char*>(&e), 4);
        out.write(reinterpret_cast<const char*>(&c), 8);
        if (count) out.write(static_cast<const char*>(data), (std::streamsize)(elem * count));
      };
      const HostResult R = ExtractOnHost(o, w, h, grey.data(), want != 0, sink);
      sink("keypoints", 4, R.keypoints.size(), R.keypoints.data());
      sink("octave_level", 4, R.octave_level.size(), R.octave_level.data());
      sink("angles", 8, R.angles.size(), R.angles.data());
      sink("raw", 4, R.raw.size(), R.raw.data());
      sink("descriptors", 1, R.descriptors.size(), R.descriptors.data());
      std::vector<int64_t> lv;
      for (const Level& l : R.levels) { lv.push_back(l.octave); lv.push_back(l.is); lv.push_back(l.num_features); lv.push_back(l.size); }
      sink("levels", 8, lv.size(), lv.data());
      std::vector<int32_t> oc;
      for (const OctaveCounts& c : R.octaves)
        for (int32_t v : {c.width, c.height, c.num_candidates, c.num_keypoints, c.moved, c.reject_peak, c.reject_edge, c.reject_offset, c.reject_bounds})
          oc.push_back(v);
      sink("octaves", 4, oc.size(), oc.data());
      const int64_t cut[6] = {R.cut.first_level_to_keep, R.cut.first_feature, R.cut.num_features, R.two_orientations, R.windows_cut, R.descriptors_skipped};
      sink("cut", 8, 6, cut);
      out.close();
      std::printf("%s\n", out ? "ok" : "refused cannot write the dump");
    } else if (!cmd.empty()) {
      std::printf("refused unknown command %s\n", cmd.c_str());
    }
    std::fflush(stdout);
  }
  return 0;
}
