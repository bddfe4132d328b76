// Stand-alone driver of csrc/local_bundle_replay.hpp (std only, no device, no library): tests/test_local_bundle_replay_host.py compiles it with
// g++ -fsanitize=address,undefined and feeds it, on stdin, the shared-observation counts and the per-point triangulation angles of every image;
// it prints the replay's decisions.  The percentile of an image is taken lazily, when the replay asks for it, with std::nth_element over the
// header's keys (LocalBundleAngleKey: NaN above every number) at the header's index (LocalBundlePercentileIndex).
//   images C
//   count <image> <n>
//   angles <image> a0 a1 ... ;        (C99 hex floats or decimals, "nan" allowed)
//   find <num_points3D> <local_ba_num_images> <local_ba_min_tri_angle>
// ->  asked <image>                   in the order of the requests
//     overlap <image> <count> <tri_angle %.17g>
//     bundle <image> ...
//     result level <l> filled <f> used <u> eff <e>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../privacy_preserving_sfm_amd/csrc/local_bundle_replay.hpp"

int main() {
  std::vector<int32_t> count;
  std::vector<std::vector<double>> angles;
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "images") {
      int c;
      std::cin >> c;
      count.assign((size_t)c, 0);
      angles.assign((size_t)c, {});
    } else if (cmd == "count") {
      int c, n;
      std::cin >> c >> n;
      count.at((size_t)c) = n;
    } else if (cmd == "angles") {
      int c;
      std::cin >> c;
      std::string tok;
      while (std::cin >> tok && tok != ";") angles.at((size_t)c).push_back(std::strtod(tok.c_str(), nullptr));
    } else if (cmd == "find") {
      int n3, num_images;
      double min_angle;
      std::cin >> n3 >> num_images >> min_angle;
      const ppsfm::LocalBundleResult r = ppsfm::ReplayFindLocalBundle(count.data(), (int32_t)count.size(), n3, num_images, min_angle, [&](int32_t c) {
        std::printf("asked %d\n", c);
        std::vector<double>& a = angles.at((size_t)c);
        if (a.empty()) { std::printf("missing %d\n", c); return -1.0; }
        const int64_t k = ppsfm::LocalBundlePercentileIndex((int64_t)a.size());
        std::nth_element(a.begin(), a.begin() + k, a.end(), [](double x, double y) { return ppsfm::LocalBundleAngleKey(x) < ppsfm::LocalBundleAngleKey(y); });
        return a[(size_t)k];
      });
      for (size_t i = 0; i < r.overlap_image.size(); ++i) std::printf("overlap %d %d %.17g\n", r.overlap_image[i], r.overlap_count[i], r.overlap_tri_angle[i]);
      std::printf("bundle");
      for (const int32_t b : r.bundle) std::printf(" %d", b);
      std::printf("\nresult level %d filled %d used %d eff %d\n", r.threshold_level, r.filled, r.angles_used, r.num_eff_images);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
