// Drives csrc/tracks_replay.hpp - the host replay of track completion and merging - WITHOUT a device: the header is std only, so this file compiles with
// plain g++ (tests/test_tracks_replay_host.py builds it with -fsanitize=address,undefined).  The speculative lists and the per-pair flags the device would
// deliver come from the script on standard input; the decisions come back on standard output.
//   line <image> <point | -1>            the next line (numbered 0, 1, ...)           images <n>  /  unreg <image>
//   corr <a> <b>                         b joins a's correspondence list (directed)   point <x> <y> <z>   the next point
//   track <p> <l ...> ;                  spec <p> <l ...> ;                            ok <a> <q> <1 | 0 | negative error>
//   complete <max_transitivity> <subset p ...> ;     merge <subset p ...> ;    (an empty subset = all points)         state
#include <cstdio>
#include <iostream>
#include <map>
#include <string>
#include <utility>

#include "../privacy_preserving_sfm_amd/csrc/tracks_replay.hpp"

using namespace ppsfm;

static std::vector<int32_t> ReadList() {
  std::vector<int32_t> v;
  std::string tok;
  while (std::cin >> tok && tok != ";") v.push_back(std::stoi(tok));
  return v;
}

int main() {
  TrackState st;
  std::vector<std::vector<int32_t>> nbr;
  std::map<int, std::vector<int32_t>> spec;
  std::map<std::pair<int, int>, int> ok;
  bool frozen = false;
  auto freeze = [&] {      // CSR of the correspondences, once
    if (frozen) return;
    frozen = true;
    st.L = (int64_t)st.line_image.size();
    nbr.resize((size_t)st.L);
    st.corr_start.assign(1, 0);
    for (const auto& v : nbr) { st.corr_line.insert(st.corr_line.end(), v.begin(), v.end()); st.corr_start.push_back((int32_t)st.corr_line.size()); }
    st.deleted.resize(st.tracks.size());
    for (size_t p = 0; p < st.tracks.size(); ++p) st.deleted[p] = st.tracks[p].empty();
  };
  auto subset_of = [&](const std::vector<int32_t>& ids, std::vector<uint8_t>* sub) -> const uint8_t* {
    if (ids.empty()) return nullptr;
    sub->assign((size_t)st.NumPoints(), 0);
    for (int32_t p : ids) (*sub)[(size_t)p] = 1;
    return sub->data();
  };
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "images") { int n; std::cin >> n; st.image_registered.assign((size_t)n, 1); }
    else if (cmd == "unreg") { int i; std::cin >> i; st.image_registered.at((size_t)i) = 0; }
    else if (cmd == "line") { int c, p; std::cin >> c >> p; st.line_image.push_back(c); st.line_point.push_back(p); }
    else if (cmd == "corr") { int a, b; std::cin >> a >> b; if (nbr.size() <= (size_t)a) nbr.resize((size_t)a + 1); nbr[(size_t)a].push_back(b); }
    else if (cmd == "point") { double x, y, z; std::cin >> x >> y >> z; st.points.insert(st.points.end(), {x, y, z}); st.tracks.emplace_back(); }
    else if (cmd == "track") { int p; std::cin >> p; st.tracks.at((size_t)p) = ReadList(); }
    else if (cmd == "spec") { int p; std::cin >> p; spec[p] = ReadList(); }
    else if (cmd == "ok") { int a, q, v; std::cin >> a >> q >> v; ok[{a, q}] = v; }
    else if (cmd == "complete") {
      freeze();
      int T; std::cin >> T;
      std::vector<uint8_t> sub;
      const uint8_t* s = subset_of(ReadList(), &sub);
      const CompleteCounters c = ReplayComplete(
          st, s, T, [&](int p) { const auto& v = spec[p]; return SpecList{v.data(), (int64_t)v.size()}; },
          [&](int p, int32_t l) { std::printf("pair %d %d\n", p, (int)l); });
      std::printf("completed %lld conflicts %d\n", (long long)c.num_completed, (int)c.conflict_replays);
    } else if (cmd == "merge") {
      freeze();
      std::vector<uint8_t> sub;
      const uint8_t* s = subset_of(ReadList(), &sub);
      auto eval = [&](int a, int q) -> int {
        std::printf("eval %d %d\n", a, q);
        const auto it = ok.find({a, q});
        if (it == ok.end()) { std::printf("missing %d %d\n", a, q); return 0; }
        return it->second;
      };
      auto emit = [&](int a, int q, int m) { std::printf("merge %d %d %d\n", a, q, m); };
      MergeReplay<decltype(eval), decltype(emit)> replay{st, eval, emit, {}, {}, 0};
      replay.Run(s);
      std::printf("merged %lld merges %lld error %d\n", (long long)replay.cnt.num_merged, (long long)replay.cnt.num_merges, replay.error);
    } else if (cmd == "state") {
      freeze();
      std::printf("lp");
      for (int32_t p : st.line_point) std::printf(" %d", (int)p);
      std::printf("\n");
      for (int p = 0; p < st.NumPoints(); ++p) {
        std::printf("track %d exists %d xyz %.17g %.17g %.17g :", p, st.Exists(p) ? 1 : 0, st.points[3 * (size_t)p], st.points[3 * (size_t)p + 1], st.points[3 * (size_t)p + 2]);
        for (int32_t l : st.tracks[(size_t)p]) std::printf(" %d", (int)l);
        std::printf("\n");
      }
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
