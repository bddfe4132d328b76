// Stand-alone driver of csrc/line_features_replay.hpp (K19) for tests/test_line_features_replay_host.py: no device, built with g++ -fsanitize=address,undefined.
// One command per line on stdin:
//   draws seed image first count        -> draws d0 d1 d2 ... (count x 3 doubles as the hex of their bits)
//   keys seed image first count         -> keys k ... (hex)
//   count N ratio                       -> count n,  or  refused <why>          (ratio as %la or decimal)
//   threshold seed image N n            -> threshold key (hex)
//   validate ratio num_cameras num_images | model nparams p0 .. (per camera) | start... (num_images + 1) | camera has_gravity gx gy gz (per image)
//                                       -> ok,  or  refused <why>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/line_features_replay.hpp"

static double ReadDouble(std::istream& in) {
  std::string s;
  in >> s;
  return std::strtod(s.c_str(), nullptr);      // (reads nan, inf and hex floats)
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "draws" || cmd == "keys") {
      uint64_t seed = 0;
      long long image = 0, first = 0, count = 0;
      in >> seed >> image >> first >> count;
      const uint64_t state = ppsfm::LfImageState(seed, (int32_t)image);
      std::printf("%s", cmd.c_str());
      for (long long i = first; i < first + count; ++i) {
        if (cmd == "keys") { std::printf(" %016" PRIx64, ppsfm::LfAlignKey(state, (int32_t)i)); continue; }
        for (int c = 0; c < 3; ++c) {
          const double d = ppsfm::LfDraw(state, (int32_t)i, c);
          uint64_t bits;
          std::memcpy(&bits, &d, sizeof(bits));
          std::printf(" %016" PRIx64, bits);
        }
      }
      std::printf("\n");
    } else if (cmd == "count") {
      long long N = 0;
      in >> N;
      const double ratio = ReadDouble(in);
      if (!ppsfm::LfRatioValid(ratio)) { std::printf("refused aligned_line_ratio is outside [0, 1]\n"); continue; }
      std::printf("count %lld\n", (long long)ppsfm::LfAlignedCount(N, ratio));
    } else if (cmd == "threshold") {
      uint64_t seed = 0;
      long long image = 0, N = 0, n = 0;
      in >> seed >> image >> N >> n;
      std::printf("threshold %016" PRIx64 "\n", ppsfm::LfThresholdKey(ppsfm::LfImageState(seed, (int32_t)image), N, n));
    } else if (cmd == "validate") {
      const double ratio = ReadDouble(in);
      int num_cameras = 0, num_images = 0;
      in >> num_cameras >> num_images;
      std::string bar;
      in >> bar;
      std::vector<int32_t> model((size_t)num_cameras);
      std::vector<int> nparams((size_t)num_cameras);
      std::vector<double> intr(12 * (size_t)num_cameras, 0.0);
      for (int c = 0; c < num_cameras; ++c) {
        in >> model[(size_t)c] >> nparams[(size_t)c];
        for (int j = 0; j < nparams[(size_t)c] && j < 12; ++j) intr[12 * (size_t)c + (size_t)j] = ReadDouble(in);
      }
      in >> bar;
      std::vector<int64_t> start((size_t)num_images + 1);
      for (auto& v : start) { long long t = 0; in >> t; v = t; }
      in >> bar;
      std::vector<int32_t> camera((size_t)num_images);
      std::vector<uint8_t> has_gravity((size_t)num_images);
      std::vector<double> gravity(3 * (size_t)num_images);
      for (int k = 0; k < num_images; ++k) {
        int hg = 0;
        in >> camera[(size_t)k] >> hg;
        has_gravity[(size_t)k] = (uint8_t)hg;
        for (int j = 0; j < 3; ++j) gravity[3 * (size_t)k + (size_t)j] = ReadDouble(in);
      }
      const std::string wrong = ppsfm::LfValidate(num_images, num_cameras, start.data(), camera.data(), model.data(), nparams.data(), intr.data(), 12,
                                                  has_gravity.data(), gravity.data(), ratio);
      if (wrong.empty()) std::printf("ok\n"); else std::printf("refused %s\n", wrong.c_str());
    } else if (!cmd.empty()) {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
