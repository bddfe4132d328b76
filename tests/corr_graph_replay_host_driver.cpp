// Stand-alone driver of csrc/corr_graph_replay.hpp (K18) for tests/test_corr_graph_replay_host.py: no device, built with g++ -fsanitize=address,undefined.
// One command per line on stdin:
//   pair n1 n2 count x1 x2 ...                      -> pair valid repeats1 repeats2 needs_replay | accepted flags... | first flags...
//   plan num_images min_num_matches num_pairs (a b count)...   -> plan num_ranked | connected... | image1 image2 swapped used rank per pair,  or  refused <why>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/corr_graph_replay.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "pair") {
      int32_t n1 = 0, n2 = 0;
      long long count = 0;
      in >> n1 >> n2 >> count;
      std::vector<int32_t> m(2 * (size_t)count);
      for (auto& v : m) in >> v;
      const ppsfm::CorrPairClass c = ppsfm::CorrClassifyPair(n1, n2, m.data(), count);
      std::vector<uint8_t> seq((size_t)count), first((size_t)count);
      const long long ns = ppsfm::CorrReplayPair(n1, n2, m.data(), count, seq.data());
      const long long nf = ppsfm::CorrFirstOccurrencePair(n1, n2, m.data(), count, first.data());
      std::printf("pair %lld %lld %lld %d | %lld", (long long)c.valid, (long long)c.repeats1, (long long)c.repeats2,
                  (int)ppsfm::CorrNeedsReplay(c.repeats1, c.repeats2), ns);
      for (uint8_t f : seq) std::printf(" %d", (int)f);
      std::printf(" | %lld", nf);
      for (uint8_t f : first) std::printf(" %d", (int)f);
      std::printf("\n");
    } else if (cmd == "plan") {
      int32_t num_images = 0, min_num_matches = 0;
      long long num_pairs = 0;
      in >> num_images >> min_num_matches >> num_pairs;
      std::vector<int32_t> pairs(2 * (size_t)(num_pairs > 0 ? num_pairs : 0));
      std::vector<int64_t> start(1, 0);
      for (long long p = 0; p < num_pairs; ++p) {
        long long count = 0;
        in >> pairs[2 * (size_t)p] >> pairs[2 * (size_t)p + 1] >> count;
        start.push_back(start.back() + count);
      }
      std::vector<ppsfm::CorrPairPlan> plan;
      std::vector<uint8_t> connected;
      int64_t ranked = 0;
      const std::string wrong = ppsfm::CorrPlanPairs(num_images, min_num_matches, num_pairs, pairs.data(), start.data(), &plan, &connected, &ranked);
      if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); continue; }
      std::printf("plan %lld |", (long long)ranked);
      for (uint8_t c : connected) std::printf(" %d", (int)c);
      std::printf(" |");
      for (const auto& q : plan) std::printf(" %d %d %d %d %d", q.image1, q.image2, q.swapped, q.used, q.rank);
      std::printf("\n");
    } else if (!cmd.empty()) {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
