// Stand-alone driver of csrc/pair_selection_replay.hpp (K20) for tests/test_pair_selection_replay_host.py: no device, built with
// g++ -fsanitize=address,undefined.  Floats travel as their uint32 bit patterns.  One command per line on stdin:
//   spatial m max_num_neighbors max_distance null_xyz bits...   -> spatial n visited | (query neighbour distbits)...   or  refused <why>
//   keys n (distbits index)...                                  -> keys <the positions 0 .. n-1 in ascending key order>
//   transitive N M null_matched (a b)... T null_tried (a b)...  -> transitive n visited | (a c)...                     or  refused <why>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/pair_selection_replay.hpp"

namespace {
float FromBits(uint32_t bits) { float f; std::memcpy(&f, &bits, sizeof(f)); return f; }
uint32_t ToBits(float f) { uint32_t bits; std::memcpy(&bits, &f, sizeof(bits)); return bits; }
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "spatial") {
      long long m = 0;
      int32_t knn = 0, null_xyz = 0;
      double max_distance = 0;
      std::string dist;
      in >> m >> knn >> dist >> null_xyz;
      max_distance = std::strtod(dist.c_str(), nullptr);      // ("nan" and "inf" too)
      std::vector<float> xyz(3 * (size_t)(m > 0 ? m : 0));
      for (auto& v : xyz) { uint32_t bits = 0; in >> bits; v = FromBits(bits); }
      const std::string wrong = ppsfm::PairsCheckSpatial(m, null_xyz ? nullptr : xyz.data(), knn, max_distance);
      if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); continue; }
      std::vector<int32_t> pairs;
      std::vector<float> sqdist;
      const long long visited = ppsfm::SpatialPairsHost(m, xyz.data(), knn, max_distance, &pairs, &sqdist);
      std::printf("spatial %zu %lld |", sqdist.size(), visited);
      for (size_t k = 0; k < sqdist.size(); ++k) std::printf(" %d %d %u", pairs[2 * k], pairs[2 * k + 1], ToBits(sqdist[k]));
      std::printf("\n");
    } else if (cmd == "keys") {
      long long n = 0;
      in >> n;
      std::vector<std::pair<uint64_t, int>> keys((size_t)n);
      for (long long k = 0; k < n; ++k) {
        uint32_t bits = 0, index = 0;
        in >> bits >> index;
        keys[(size_t)k] = {ppsfm::SpatialKey(FromBits(bits), index), (int)k};
        if (ToBits(ppsfm::SpatialKeyDist(keys[(size_t)k].first)) != bits) { std::fprintf(stderr, "the key does not return its distance\n"); return 3; }
      }
      std::sort(keys.begin(), keys.end());
      std::printf("keys");
      for (const auto& k : keys) std::printf(" %d", k.second);
      std::printf("\n");
    } else if (cmd == "transitive") {
      int32_t N = 0, null_matched = 0, null_tried = 0;
      long long M = 0, T = 0;
      in >> N >> M >> null_matched;
      std::vector<int32_t> matched(2 * (size_t)(M > 0 ? M : 0));
      for (auto& v : matched) in >> v;
      in >> T >> null_tried;
      std::vector<int32_t> tried(2 * (size_t)(T > 0 ? T : 0));
      for (auto& v : tried) in >> v;
      const std::string wrong = ppsfm::PairsCheckTransitive(N, M, null_matched ? nullptr : matched.data(), T, null_tried ? nullptr : tried.data());
      if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); continue; }
      std::vector<int32_t> pairs;
      const long long visited = ppsfm::TransitivePairsHost(N, M, matched.data(), T, tried.data(), &pairs);
      if (visited != ppsfm::TransitiveVisited(N, M, matched.data())) { std::fprintf(stderr, "the walk and the degree sum disagree\n"); return 3; }
      std::printf("transitive %zu %lld |", pairs.size() / 2, visited);
      for (int32_t v : pairs) std::printf(" %d", v);
      std::printf("\n");
    } else if (!cmd.empty()) {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
