// Stand-alone driver of csrc/bundle_setup_replay.hpp (std only, no device, no library): tests/test_bundle_setup_replay_host.py compiles it with
// g++ -fsanitize=address,undefined and feeds it, on stdin, a config and either the pose list of a problem or a tracks state; it prints the header's answers.
//   config C K                          then five lines: C image flags; C tvec masks or "none"; K camera_const or "none"; K subset masks or "none";
//                                       C handle cameras of the images
//   points nv v... nc c...              the two point lists of the config
//   poses n i...                        -> pose_const / pose_tvec / pose_camera / cameras / camera_mask, one line each
//   dedup P                             -> list ... / mark ...
//   state C P L                         then: L line_image; L line_point; C image_registered; P deleted; P lines "n l..." (the tracks)
//   validate                            -> valid | invalid <text>
//   count                               -> count <num_obs> <num_points>      (the lists de-duplicated first)
#include <cstdio>
#include <iostream>
#include <string>

#include "../privacy_preserving_sfm_amd/csrc/bundle_setup_replay.hpp"

namespace {

template <typename T>
bool ReadOptional(size_t n, std::vector<T>* out) {      // n numbers, or the word "none"
  std::string tok;
  out->clear();
  for (size_t i = 0; i < n; ++i) {
    std::cin >> tok;
    if (tok == "none") return false;
    out->push_back((T)std::stol(tok));
  }
  return true;
}

template <typename T>
void Print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T x : v) std::printf(" %ld", (long)x);
  std::printf("\n");
}

}  // namespace

int main() {
  int C = 0, K = 0;
  std::vector<uint8_t> flags, tvec, camconst;
  std::vector<uint16_t> subset;
  std::vector<int32_t> image_camera, variable, constant;
  bool has_tvec = false, has_camconst = false, has_subset = false;
  ppsfm::TrackState st;
  auto view = [&]() {
    return ppsfm::BundleConfigView{flags.data(), has_tvec ? tvec.data() : nullptr, has_camconst ? camconst.data() : nullptr, has_subset ? subset.data() : nullptr,
                                   variable.data(), constant.data(), (int32_t)variable.size(), (int32_t)constant.size()};
  };
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "config") {
      std::cin >> C >> K;
      ReadOptional((size_t)C, &flags);
      has_tvec = ReadOptional((size_t)C, &tvec);
      has_camconst = ReadOptional((size_t)K, &camconst);
      has_subset = ReadOptional((size_t)K, &subset);
      ReadOptional((size_t)C, &image_camera);
    } else if (cmd == "points") {
      size_t n;
      std::cin >> n;
      ReadOptional(n, &variable);
      std::cin >> n;
      ReadOptional(n, &constant);
    } else if (cmd == "poses") {
      size_t n;
      std::cin >> n;
      std::vector<int32_t> poses;
      ReadOptional(n, &poses);
      const ppsfm::BundlePoseResult r = ppsfm::ReplayBundlePoses(poses.data(), (int32_t)poses.size(), image_camera.data(), K, view());
      Print("pose_const", r.pose_const); Print("pose_tvec", r.pose_tvec_mask); Print("pose_camera", r.pose_camera);
      Print("cameras", r.camera_index); Print("camera_mask", r.camera_const_mask);
    } else if (cmd == "dedup") {
      int P;
      std::cin >> P;
      const ppsfm::BundlePointList r = ppsfm::DedupBundlePoints(P, view());
      Print("list", r.points); Print("mark", r.mark);
    } else if (cmd == "state") {
      int sc, P;
      long L;
      std::cin >> sc >> P >> L;
      st = ppsfm::TrackState();
      st.L = L;
      ReadOptional((size_t)L, &st.line_image); ReadOptional((size_t)L, &st.line_point); ReadOptional((size_t)sc, &st.image_registered);
      ReadOptional((size_t)P, &st.deleted);
      st.tracks.assign((size_t)P, {});
      for (int p = 0; p < P; ++p) {
        size_t n;
        std::cin >> n;
        ReadOptional(n, &st.tracks[(size_t)p]);
      }
      st.points.assign(3 * (size_t)P, 0.0);
    } else if (cmd == "validate") {
      const std::string wrong = ppsfm::ValidateBundleConfig(st, C, view());
      if (wrong.empty()) std::printf("valid\n"); else std::printf("invalid %s\n", wrong.c_str());
    } else if (cmd == "count") {
      const ppsfm::BundlePointList list = ppsfm::DedupBundlePoints(st.NumPoints(), view());
      int64_t m = 0;
      int32_t n = 0;
      ppsfm::CountBundleSetup(st, flags.data(), list.points, &m, &n);
      std::printf("count %lld %d\n", (long long)m, n);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
