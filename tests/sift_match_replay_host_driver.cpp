// Stand-alone driver of csrc/sift_match_replay.hpp (the host half of K17), compiled with g++ -fsanitize=address,undefined by
// tests/test_sift_match_replay_host.py.  Commands on stdin, one per line:
//   thresholds <max_ratio> <max_distance>        builds the integer thresholds and compares them with the float rules evaluated directly: every best of the
//                                                table (and the 64 below d_min) against every second within 64 of its boundary, and 200 000 random pairs
//                                                -> "thresholds <d_min> <count> <checked> <mismatches>"   or   "refused <why>"
//   dump <max_ratio> <max_distance> <path>       the table as raw int32 to <path> -> "dump <d_min> <count>"
//   match <n1> <n2> <cross_check> <max_ratio> <max_distance>   followed by n1 + n2 lines of 256 hex digits (one descriptor each)
//                                                -> "top2 <n1> then best_j best second per row", "matches <n> i j i j ..."
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/sift_match_replay.hpp"

using namespace ppsfm;

namespace {

// the two rules of sift.cc:84-99 on angles computed once per integer by the header's SiftAngle
struct DirectRule {
  float max_ratio, max_distance;
  std::vector<float> a;
  DirectRule(double ratio, double distance) : max_ratio((float)ratio), max_distance((float)distance), a((size_t)kSiftClamp + 1) {
    for (int32_t d = 0; d <= kSiftClamp; ++d) a[(size_t)d] = SiftAngle(d);
  }
  bool Accept(int32_t best, int32_t second) const {
    const float best_normed = a[(size_t)std::min(best, kSiftClamp)];
    if (best_normed > max_distance) return false;
    const float second_normed = a[(size_t)std::min(second, kSiftClamp)];
    if (best_normed >= max_ratio * second_normed) return false;
    return true;
  }
};

void Thresholds(double ratio, double distance) {
  SiftThresholds t;
  const std::string wrong = BuildSiftThresholds(ratio, distance, &t);
  if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); return; }
  const DirectRule rule(ratio, distance);
  long long checked = 0, bad = 0;
  for (int32_t b = std::max(1, t.d_min - 64); b <= kSiftClamp; ++b) {
    if (b < t.d_min) {
      for (int32_t s = 0; s <= std::min(b, 64); ++s) { ++checked; bad += t.Accept(b, s) != rule.Accept(b, s); }
      continue;
    }
    const int32_t edge = t.s_max[(size_t)(b - t.d_min)];
    for (int32_t s = std::max(0, edge - 64); s <= std::min(kSiftClamp, edge + 64); ++s) { ++checked; bad += t.Accept(b, s) != rule.Accept(b, s); }
  }
  std::mt19937_64 rng(12345);
  const int32_t kMaxDist = 128 * 255 * 255;
  for (int k = 0; k < 200000; ++k) {
    const int32_t top = (k & 1) ? kMaxDist : kSiftClamp + 1000;
    const int32_t b = 1 + (int32_t)(rng() % (uint64_t)top);
    const int32_t s = (int32_t)(rng() % (uint64_t)(b + 1));
    ++checked;
    bad += t.Accept(b, s) != SiftAcceptDirect((float)ratio, (float)distance, b, s);      // (acosf called afresh)
  }
  std::printf("thresholds %d %zu %lld %lld\n", t.d_min, t.s_max.size(), checked, bad);
}

bool ReadRows(int32_t n, std::vector<uint8_t>* d) {
  d->assign((size_t)n * kSiftDim, 0);
  std::string line;
  for (int32_t i = 0; i < n; ++i) {
    if (!std::getline(std::cin, line) || line.size() != 2 * (size_t)kSiftDim) return false;
    for (int32_t k = 0; k < kSiftDim; ++k) (*d)[(size_t)i * kSiftDim + k] = (uint8_t)std::strtoul(line.substr(2 * (size_t)k, 2).c_str(), nullptr, 16);
  }
  return true;
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd.empty()) continue;
    if (cmd == "thresholds") {
      double ratio = 0, distance = 0;
      in >> ratio >> distance;
      Thresholds(ratio, distance);
    } else if (cmd == "dump") {
      double ratio = 0, distance = 0;
      std::string path;
      in >> ratio >> distance >> path;
      SiftThresholds t;
      const std::string wrong = BuildSiftThresholds(ratio, distance, &t);
      if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); continue; }
      std::FILE* f = std::fopen(path.c_str(), "wb");
      if (!f || std::fwrite(t.s_max.data(), sizeof(int32_t), t.s_max.size(), f) != t.s_max.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
      std::fclose(f);
      std::printf("dump %d %zu\n", t.d_min, t.s_max.size());
    } else if (cmd == "match") {
      int32_t n1 = 0, n2 = 0, cross = 0;
      double ratio = 0, distance = 0;
      in >> n1 >> n2 >> cross >> ratio >> distance;
      std::vector<uint8_t> d1, d2;
      if (n1 < 0 || n2 < 0 || !ReadRows(n1, &d1) || !ReadRows(n2, &d2)) { std::fprintf(stderr, "bad descriptor rows\n"); return 2; }
      SiftThresholds t;
      const std::string wrong = BuildSiftThresholds(ratio, distance, &t);
      if (!wrong.empty()) { std::printf("refused %s\n", wrong.c_str()); continue; }
      std::vector<int32_t> bj((size_t)n1), b((size_t)n1), s((size_t)n1);
      SiftTop2Host(d1.data(), n1, d2.data(), n2, bj.data(), b.data(), s.data());
      std::printf("top2 %d", n1);
      for (int32_t i = 0; i < n1; ++i) std::printf(" %d %d %d", bj[(size_t)i], b[(size_t)i], s[(size_t)i]);
      std::printf("\n");
      const std::vector<int32_t> m = SiftMatchHost(t, cross != 0, d1.data(), n1, d2.data(), n2);
      std::printf("matches %zu", m.size() / 2);
      for (const int32_t v : m) std::printf(" %d", v);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
